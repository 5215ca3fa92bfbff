// mixed_capi.hpp -- launchers of the mixed-radix fused kernels (mixed_kernels.hpp), compiled in their
// own translation unit (mixed_capi.hip) and called by the solver's orchestration in admm_capi.hip
// (its MixedOps backend of fused_forward / fused_backward, and setup).
// Every launcher returns hipSuccess or the launch error.
#pragma once
#include <hip/hip_runtime.h>

#include "admm_backward.hpp"
#include "admm_kernels.hpp"

namespace admm_mixed {

using admm::cf;

// plans exist for the row length N = W/2 / the column length H
bool row_ok(int N);
bool col_ok(int H);
int col_cols(int H);  // the fewest columns per column-pass block (N must be a multiple)
int pass_b_cols(int H, int N);  // the columns per block pass_b launches (0: N fits no plan)
int row_lanes(int N);  // lanes of a row group (up to 256: several waves)
int pass_a_blocks_per_cu(int N);  // resident 256-thread blocks of the row pass per CU (occupancy query)

hipError_t r2c(int N, const float* img, cf* spec, const cf* twW, long long rows, hipStream_t s);
hipError_t c2r(int N, const cf* spec, float* img, const cf* twW, long long rows, hipStream_t s);
// hist: the training forward (a_k into the history; admm_kernels.hpp k_pass_a HIST)
hipError_t pass_a(int N, const admm::PassAArgs& a, bool iso, bool first, bool hist, hipStream_t s);
hipError_t iso_norm(int N, const admm::IsoArgs& a, bool first, bool hist, hipStream_t s);
// the training backward's reverse row pass and iso Q pass (admm_backward.hpp, mixed transforms)
hipError_t bwd_pass_a(int N, const admm::BwdArgs& a, bool iso, bool lastk, bool firstk, hipStream_t s);
hipError_t bwd_iso_q(int N, const admm::BwdIsoArgs& a, bool lastk, hipStream_t s);
// the column pass of P planes from `in` into `out`: the same buffer (in place), or -- the training forward with
// a PSF gradient, whose r_k stay in the history -- another one
// bank: a PSF bank's table index (fcM then holds bank->T tables), null for one PSF
hipError_t pass_b(int H, const cf* in, cf* out, const float* fcM, const cf* twH, int N, long long P, hipStream_t s,
                  const admm::BankIdx* bank = nullptr);
// PSF gradient: part[g][kx][ky] = scale * sum over plane group g (ppg planes) of conj(colFFT U_p) colFFT V_p,
// kx in [0, N] (k_xspec's layout: k_xspec_reduce and k_psf_grad follow)
// xb: a PSF bank's gradient -- `tables` x xb->cpt plane groups, each a chunk of one table's planes (admm::XBank)
hipError_t xspec(int H, const cf* U, const cf* V, cf* part, const cf* twH, int N, long long P, int ppg, float scale,
                 hipStream_t s, const admm::XBank* xb = nullptr, int tables = 0);
// fcM: [H][N + 1] then the column-block-packed copy [N / C][H][C] (C = pass_b_cols): H (2N + 1) floats
// (tables > 0: a PSF bank's tables, one after another in fcT and in fcM, in one launch)
hipError_t fc_mixed(const float* fcT, float* fcM, int H, int N, hipStream_t s, int tables = 0);
// b = H_t(xin) on the mixed transforms: the column pass with the complex PSF multiplier mM ([H][N + 1],
// mt_mixed of the generic path's mT [N + 1][H], halved for the packed row transforms)
hipError_t pass_b_cm(int H, cf* spec, const cf* mM, const cf* twH, int N, long long P, hipStream_t s,
                     const admm::BankIdx* bank = nullptr);
hipError_t mt_mixed(const cf* mT, cf* mM, int H, int N, hipStream_t s, int tables = 0);

}  // namespace admm_mixed
