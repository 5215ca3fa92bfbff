// admm_capi.hip -- host side of the MI355X ADMM-TV library: the C ABI declared in
// include/admm_tv.h.  Orchestrates setup kernels and the per-iteration passes on
// the caller's stream; no host synchronisation, no allocation (workspace is the
// caller's), so the whole call is graph-capturable.
//
// Replaces the reference's Python loop  fft_admm_tv  (deconv.py:35-117): ~30 ATen
// launches per iteration there, 2 fused kernels per iteration here (3 for iso).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "gcol_mm.hpp"
#include "knobs.hpp"
#include "mixed_capi.hpp"
#include "odd_capi.hpp"
#include "state_kernels.hpp"
#include "admm_tv.h"

using namespace admm;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

// ------------------------------------------------------------------ profiling
struct ProfRec {
    int kind, dev;
    hipEvent_t a, b;
};
// process-wide totals (bench.py reads them); every access holds g_prof.mu, so solves on
// several threads / streams may record concurrently
struct Prof {
    std::mutex mu;
    bool on = false;
    std::vector<ProfRec> recs;
    std::vector<std::pair<int, hipEvent_t>> pool;  // (device, event): an event records on its device's streams
    double ms[4] = {0, 0, 0, 0};
    int64_t n[4] = {0, 0, 0, 0};
} g_prof;

hipEvent_t prof_event() {  // caller holds g_prof.mu; an event of the current device
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    for (size_t i = 0; i < g_prof.pool.size(); ++i)
        if (g_prof.pool[i].first == dev) {
            hipEvent_t e = g_prof.pool[i].second;
            g_prof.pool[i] = g_prof.pool.back();
            g_prof.pool.pop_back();
            return e;
        }
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

struct ProfScope {
    int kind, dev = 0;
    hipStream_t s;
    hipEvent_t a = nullptr, b = nullptr;
    ProfScope(int k, hipStream_t st) : kind(k), s(st) {
        std::lock_guard<std::mutex> lk(g_prof.mu);
        if (g_prof.on && hipGetDevice(&dev) == hipSuccess) {
            a = prof_event();
            b = prof_event();
            if (a && b) (void)hipEventRecord(a, s);
        }
    }
    ~ProfScope() {
        if (a && b) {
            (void)hipEventRecord(b, s);
            std::lock_guard<std::mutex> lk(g_prof.mu);
            g_prof.recs.push_back({kind, dev, a, b});
        }
    }
};

// cross-rank reduction hook (iso): carried per call in the descriptor (admm_tv_desc.allreduce)
void allreduce(const admm_tv_desc& d, float* buf, size_t count, hipStream_t s) {
    if (d.allreduce) d.allreduce(buf, count, s, d.allreduce_ctx);
}
// an empty shard of an iso solve over ranks: only its part of the reductions remains
bool participate_only(const admm_tv_desc& d) { return d.iso && d.allreduce && d.B * d.C == 0; }

// ------------------------------------------------------------------ geometry
bool pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }

// fused power-of-two kernels
bool supported_hw(int64_t H, int64_t W) {
    return pow2(H) && pow2(W) && H >= 16 && H <= 4096 && W >= 16 && W <= 2048;
}
// any other size runs on the generic kernels (generic_kernels.hpp): a line of each dimension in
// their LDS image (two line buffers + twiddles and Bluestein tables, the latter read from global
// memory for lines beyond ~6,800 points) up to 10,240 points (5,120 in fp64); longer lines keep
// their two buffers in a global scratch slot per block (GPlan::glb), up to kGenericMax
constexpr int64_t kGenericMax = 65536;
bool gen_fits(int n, bool f64 = false);  // below, with the plans
bool generic_hw(int64_t H, int64_t W) {
    return !supported_hw(H, W) && H >= 1 && W >= 1 && H <= kGenericMax && W <= kGenericMax && gen_fits((int)H) &&
           gen_fits((int)W);
}
// smooth sizes on the fused two-pass iteration with mixed-radix register transforms (mixed_kernels.hpp,
// DESIGN.md §7c): W even with a row plan for W / 2, a column plan for H, not both powers of two (those
// are supported_hw).  Training too (Layout::mixed_train), with or without a PSF gradient, except grouped modules.
// ADMM_MIXED=0 (A/B knob) keeps them on the generic kernels.
bool mixed_hw(int64_t H, int64_t W) {
    if (supported_hw(H, W) || H < 16 || W < 16 || (W & 1) || H > 4096 || W > 4096) return false;
    if (!admm_mixed::row_ok((int)(W / 2)) || !admm_mixed::col_ok((int)H)) return false;
    return (W / 2) % admm_mixed::col_cols((int)H) == 0 && env_int("ADMM_MIXED", 1) != 0;
}
// odd row lengths with a fused row pass instance (odd_kernels.hpp; BSD's W = 481 = 13 * 37): the
// aniso inference solve runs the two-launch iteration -- the generic column pass, then ONE row pass
// (inverse rows, step, forward rows) -- instead of the generic three.  iso and training keep the generic
// kernels.  ADMM_ODD=0 (A/B knob) keeps every solve on them.
bool odd_hw(int64_t H, int64_t W) {
    return generic_hw(H, W) && !mixed_hw(H, W) && admm_odd::row_ok((int)W) && env_int("ADMM_ODD", 1) != 0;
}
// ... and the transposed orientation (H an odd-path row length, W not: BSD portrait frames, 481 x 321): the
// solve commutes with transposing the image and the PSF (Dx and Dy trade places; the x-update's
// |Dx^|^2 + |Dy^|^2, the shrinkage and the centred H_t are symmetric in them), so the aniso inference solve
// transposes xin and the PSF, runs the odd-length iteration on the W x H problem and transposes the result
// back (two transposes per solve, not per iteration; Layout::tr)
bool odd_t_hw(int64_t H, int64_t W) {
    return generic_hw(H, W) && !mixed_hw(H, W) && !odd_hw(H, W) && odd_hw(W, H);
}
// fp64 solves (ADMM_TV_FLAG_F64) run on the generic kernels' double instantiation at every size
bool is_f64(const admm_tv_desc& d) { return (d.flags & ADMM_TV_FLAG_F64) != 0; }
bool f64_hw(int64_t H, int64_t W) {
    return H >= 1 && W >= 1 && H <= kGenericMax && W <= kGenericMax && gen_fits((int)H, true) && gen_fits((int)W, true);
}

GPlan make_plan(int n, bool f64 = false);  // generic-size transform plan (below)
size_t glb_scratch(int H, int W, long long P, bool f64);  // long lines' scratch bytes (below)
// matrix-core column pass (gcol_mm.hpp): H = S R, odd R in [17, 127] carrying H's largest prime
// factor (>= 17), S in {1, ..., 8} with a kernel instance; ok = false: the LDS column pass
struct MMPlan {
    bool ok;
    int R, S, h, KS, MT, NL, RP;
    size_t lds;
    int nth;  // threads per block (the row inverse; the column pass picks its own)
};
MMPlan mm_plan(int H, int W);
MMPlan mm_plan_row(int W);  // the row inverse (k_grow_inv_mm): W = S R, S in {1..5, 8, 13}

// modules solved together (admm_tv_desc.groups)
int ngroups_of(const admm_tv_desc& d) { return d.groups > 1 ? d.groups : 1; }

// a PSF bank (ADMM_TV_FLAG_PSF_PER_IMAGE / _PER_CHANNEL): kern holds (Bk, Ck, k, k) PSFs and the solve T = Bk Ck
// copies of every PSF table; plane p = b C + c takes table (Bk > 1 ? b : 0) Ck + (Ck > 1 ? c : 0)
bool is_bank(const admm_tv_desc& d) { return (d.flags & (ADMM_TV_FLAG_PSF_PER_IMAGE | ADMM_TV_FLAG_PSF_PER_CHANNEL)) != 0; }
BankIdx bank_of(const admm_tv_desc& d) {
    const int Bk = (d.flags & ADMM_TV_FLAG_PSF_PER_IMAGE) ? (int)d.B : 1;
    const int Ck = (d.flags & ADMM_TV_FLAG_PSF_PER_CHANNEL) ? (int)d.C : 1;
    return BankIdx{(int)d.C, Bk > 1 ? Ck : 0, Ck > 1 ? 1 : 0, Bk * Ck};
}
// planes in a row that share a table (the column pass's planes per block divide it)
int bank_run(const admm_tv_desc& d) { return (d.flags & ADMM_TV_FLAG_PSF_PER_CHANNEL) ? 1 : (int)d.C; }
constexpr long long kBankMax = 65535;  // the setup kernels take the table from a grid dimension
// the bank's PSF gradient: table t's planes (XBank) in chunks of ppg -- a per-image bank's C consecutive planes, a
// per-channel bank's B planes at stride C, a per-plane bank's one
XBank xbank_of(const admm_tv_desc& d, int ppg) {
    const bool pi = (d.flags & ADMM_TV_FLAG_PSF_PER_IMAGE) != 0, pc = (d.flags & ADMM_TV_FLAG_PSF_PER_CHANNEL) != 0;
    const int n = pi && pc ? 1 : pi ? (int)d.C : (int)d.B;
    ppg = std::max(ppg, 1);
    return XBank{pi && !pc ? (int)d.C : 1, pi ? 1 : (int)d.C, n, (n + ppg - 1) / ppg};
}

constexpr size_t kAlign = 256;
size_t up(size_t v) { return (v + kAlign - 1) / kAlign * kAlign; }

struct Layout {
    size_t spec[2], u[4], b, fcT, mT, twW, twH, twHd, G, part, nsq, sigma, total;
    size_t mM;  // mixed path with a PSF: the multiplier for b = H_t(xin) on the mixed transforms (mt_mixed)
    // generic path: the matrix-core plans, decided once per call (their environment knobs are read
    // here only, so the regions sized below and the kernels launched later always agree)
    MMPlan mm, mmr;
    // mixed-radix fused iteration (mixed_hw; fused_forward on MixedOps): the Wiener factor for its column pass.
    // mixed_train: training forward / backward on it too, one module (mixed_train_hw); with a PSF gradient the
    // history keeps r_k's packed row spectra, as on the power-of-two path
    bool mixed, mixed_train;
    size_t fcM;
    // fused odd-length row pass (odd_hw, aniso inference): the second half-spectrum buffer of its ping-pong
    bool odd;
    size_t spec2;
    // transposed odd-length solve (odd_t_hw, aniso inference): xin and the result transposed, the PSF
    // transposed, then the W x H problem's own workspace at tws
    bool tr;
    size_t xT, oT, kT, tws;
    size_t rimg;  // generic path: spec[0] = half spectra [P][H][W/2+1], spec[1] = x image, rimg = r image
    size_t gscr;  // generic path, lines beyond the LDS image: the transform blocks' scratch slots
    int ngroups, ppg;
    bool gen;
    // generic fp32 inference with both matrix-core plans: the half-spectrum row pitch (complex values)
    // padded to a multiple of 16 (128 B), so the column pass's 16-column row segments are whole cache
    // lines (A/B knob ADMM_GEN_PITCH=0: Wh)
    int ldw;
};

// The kernels a call runs on, decided here and nowhere else: admm_tv_path reports it, run_forward, run_backward
// and run_forward_state switch on it, make_hist and make_bwd_layout size their regions by it.
//   Pow2      the fused two-pass iteration, power-of-two sizes (Pow2Ops)
//   Mixed     the same on the mixed-radix register transforms, smooth sizes (MixedOps)
//   Generic   the generic kernels' three-launch iteration (run_forward_gen / run_backward_gen)
//   OddRows   the generic column pass and the fused odd-length row pass (aniso inference)
//   OddRowsT  OddRows on the transposed problem
// mode: 0 inference, 1 training (forward with a history, backward), 2 stateful inference (fp32: state_check),
//       3 inference with bounds on x (fp32: box_check)
enum class Backend { Pow2, Mixed, Generic, OddRows, OddRowsT };
Backend backend_of(const admm_tv_desc& d, const Layout& Lo, int mode) {
    if (mode < 2 && is_f64(d)) return Backend::Generic;  // the generic kernels' double instantiation
    if (mode < 2 && Lo.tr) return mode == 0 ? Backend::OddRowsT : Backend::Generic;
    if (!Lo.gen) return Backend::Pow2;
    // (the projection and its dual exist in the power-of-two row pass and the generic step only)
    if (mode == 3) return Backend::Generic;
    if (Lo.mixed && (mode != 1 || Lo.mixed_train)) return Backend::Mixed;
    // (the odd-length row pass keeps no history and carries no state)
    if (mode == 0 && Lo.odd) return Backend::OddRows;
    return Backend::Generic;
}

// (transposes a single PSF's shape: never reached with a PSF bank, make_layout leaves Layout::tr unset for one)
admm_tv_desc transposed(const admm_tv_desc& d) {
    admm_tv_desc t = d;
    t.H = d.W;
    t.W = d.H;
    t.kh = d.kw;
    t.kw = d.kh;
    return t;
}

// a training step of this descriptor runs on the mixed-radix fused kernels: fp32, one module, a smooth size
// (Layout::mixed_train)
bool mixed_train_hw(const admm_tv_desc& d) {
    return !is_f64(d) && ngroups_of(d) == 1 && generic_hw(d.H, d.W) && mixed_hw(d.H, d.W);
}

Layout make_layout(const admm_tv_desc& d) {
    Layout L{};
    const bool f64 = is_f64(d);
    const size_t rs = f64 ? sizeof(double) : sizeof(float), csz = 2 * rs;  // real / complex element
    const size_t G = ngroups_of(d);
    const size_t P = (size_t)d.B * d.C * G, H = d.H, W = d.W, N = W / 2;  // all modules' planes
    const size_t img = P * H * W * rs;
    const size_t img_m = (size_t)d.B * d.C * H * W * rs;         // one module's planes
    const int k = d.kh;
    // a PSF bank: T copies of the PSF tables (G, fcT and its copy, mT; fcM, mM); one module, fp32 (bank_check)
    const bool bank = is_bank(d);
    const size_t T = bank ? (size_t)bank_of(d).T : 1;
    size_t o = 0;
    auto take = [&](size_t bytes) {
        size_t at = o;
        o += up(bytes);
        return at;
    };
    L.gen = f64 || generic_hw(d.H, d.W);
    if (L.gen && !f64) {
        // (a bank keeps the LDS column pass: the matrix-core one reads one transposed factor table)
        if (!bank) L.mm = mm_plan((int)H, (int)W);
        L.mmr = mm_plan_row((int)W);
    }
    L.mixed = L.gen && !f64 && mixed_hw(d.H, d.W) && (G == 1 || !(d.flags & ADMM_TV_FLAG_PSF_GRAD));
    L.mixed_train = mixed_train_hw(d);
    L.odd = L.gen && !f64 && G == 1 && !d.iso && !bank && odd_hw(d.H, d.W);  // (the row pass's wrapper knows one PSF)
    L.ldw = (int)(N + 1);
    if (L.gen && !f64 && L.mm.ok && L.mmr.ok && env_int("ADMM_GEN_PITCH", 1)) L.ldw = (int)((N + 1 + 15) / 16 * 16);
    L.spec[0] = take(L.gen ? P * H * (size_t)L.ldw * csz : img);
    L.spec[1] = take(img);
    // generic path: the r image (unfused step)
    L.rimg = L.gen ? take(img) : 0;
    for (int i = 0; i < 4; ++i) L.u[i] = take(img);
    // b = H_t(xin), shared by the modules; on the fused path also without a PSF (b = xin re-laid
    // out for the inference pass, lane-paired rows)
    L.b = (k > 0 || !L.gen) ? take(img_m) : 0;
    // one Wiener factor per module (its rho); on the fused path followed by their packed copies for
    // the column pass (k_fc_pack)
    // (generic path: a [H][Wh] copy for the matrix-core column pass, k_fc_transpose)
    L.fcT = take(G * T * (N + 1) * H * rs * ((!L.gen || L.mm.ok) ? 2 : 1));
    L.mT = take(T * (N + 1) * H * csz);
    // twiddles; on the generic path followed by the plan's Bluestein tables (make_plan)
    L.twW = take((W + (L.gen ? make_plan((int)W, f64).ntab : 0)) * csz);
    L.twH = take((H + (L.gen ? make_plan((int)H, f64).ntab : 0)) * csz);
    L.twHd = take(H * sizeof(double2));
    L.G = take(T * (size_t)(k > 0 ? k : 1) * (N + 1) * sizeof(double2));
    L.gscr = L.gen ? take(glb_scratch((int)H, (int)W, (long long)P, f64)) : 0;
    L.fcM = L.mixed ? take(G * T * (2 * N + 1) * H * sizeof(float)) : 0;  // per module: [H][N + 1] + packed copy, k_fc_mixed
    L.mM = (L.mixed && k > 0) ? take(T * (N + 1) * H * 2 * sizeof(float)) : 0;
    L.spec2 = L.odd ? take(P * H * (size_t)L.ldw * csz) : 0;
    L.sigma = (k > 0 && (d.flags & ADMM_TV_FLAG_PSF_GRAD)) ? take(T * (N + 1) * H * sizeof(double2)) : 0;  // per table
    if (d.iso) {
        // plane groups for the iso norm pass: enough (group,row) items to fill the chip
        // planes per group: at most 64 (each group writes and the reduce reads one 2HW partial;
        // C3 iso norm pass: 16 -> 0.49 ms, 32 -> 0.46, 64 -> 0.45; 8 -> 499 it/s, 16 -> 497-507,
        // 64 -> 509),
        // fewer when (group, row) items would not give ~3 waves per SIMD (C5: 48 planes of 512^2
        // -> 4, iso norm -30 %)
        const int lanes = (int)std::min<size_t>(64, N / (N >= 1024 ? 16 : N >= 64 ? 8 : N >= 16 ? 4 : 2));
        const long long want = 3LL * 1024 * 64 / std::max(lanes, 1);
        int ppg = (int)std::max<long long>(1, std::min<long long>(64, (long long)(P * H) / want));
        if (const int e = env_int("ADMM_ISO_PPG", 0); e > 0) ppg = e;  // A/B knob; <= 0: the rule
        if ((size_t)P <= (size_t)ppg) ppg = (int)std::max<long long>(1, P);
        if (G > 1) {  // a plane group must not straddle two modules: a divisor of B*C
            const int pm = (int)(d.B * d.C);
            ppg = std::min(ppg, pm);
            while (pm % ppg) --ppg;
        }
        L.ppg = ppg;
        L.ngroups = (int)((P + ppg - 1) / ppg);
        L.part = take((size_t)L.ngroups * 2 * H * W * rs);
        L.nsq = take(G * 2 * H * W * rs);  // per module
    }
    L.total = o;
    if (!f64 && G == 1 && !d.iso && !bank && odd_t_hw(d.H, d.W)) {
        // the transposed inference solve: [xin^T][result^T][PSF^T][the W x H problem's workspace], laid over
        // the regions above (a call uses one or the other: training and the helpers keep this layout)
        size_t t = 0;
        auto takeT = [&](size_t bytes) {
            size_t at = t;
            t += up(bytes);
            return at;
        };
        L.tr = true;
        L.xT = takeT(img);
        L.oT = takeT(img);
        L.kT = takeT((size_t)std::max(1, d.kh * d.kw) * sizeof(float));
        L.tws = takeT(make_layout(transposed(d)).total);
        L.total = std::max(L.total, t);
    }
    return L;
}


template <class T> T* at(void* ws, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(ws) + off); }

#define HIPCHK(expr)                                                                    \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess) return fail(ADMM_TV_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

template <class K> int set_lds(K kern, size_t bytes) {
    if (bytes > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return fail(ADMM_TV_EHIP, std::string("hipFuncSetAttribute: ") + hipGetErrorString(e));
    }
    return 0;
}

int launch_check(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ADMM_TV_EHIP, std::string(what) + ": " + hipGetErrorString(e));
    return 0;
}

// a launcher's hipError_t (mixed_capi.hpp) as the library's error code, with the kernel's name
int hip_code(hipError_t e, const char* what) {
    return e == hipSuccess ? 0 : fail(ADMM_TV_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

// the caller's workspace: given, large enough for the call's layout, 256-byte aligned
int check_workspace(const void* ws, size_t have, size_t need) {
    if (!ws || have < need || (reinterpret_cast<uintptr_t>(ws) % kAlign) != 0)
        return fail(ADMM_TV_EWORKSPACE, "workspace too small or not 256-byte aligned");
    return 0;
}

// lambda / rho gradients of one module from the reverse row pass's per-strip fp64 partials
// ([K][nstrips][2], the module's strips at [soff, soff + spm)) and, iso, the tau^ partials: per-iteration
// sums (K blocks, in place), then the sum over the iterations.  Fixed order: deterministic.
template <class T>
int bwd_scalars(double* part, int K, long long nstrips, long long spm, long long soff, const double* tpart, int ntp,
                int G, int g, const T* lam, const T* rho, T* glam, T* grho, hipStream_t s) {
    if (K < 1) return fail(ADMM_TV_EINVAL, "bwd_scalars: no iterations");
    hipLaunchKernelGGL(k_bwd_iter_sums, dim3((unsigned)K), dim3(256), 0, s, part, nstrips, spm, soff, tpart, ntp, G, g);
    if (int e = launch_check("k_bwd_iter_sums")) return e;
    hipLaunchKernelGGL(k_bwd_scalars<T>, dim3(1), dim3(256), 0, s, (const double*)part, K, nstrips, 1LL, soff,
                       (const double*)nullptr, ntp, G, g, lam, rho, glam, grho);
    return launch_check("k_bwd_scalars");
}

// ------------------------------------------------------------------ row-side ops (templated on N = W/2)
template <int N> struct RowOps {
    using G = RowKernelGeom<N>;
    static unsigned blocks(long long items) { return (unsigned)((items + G::SG - 1) / G::SG); }

    // pl: the lane-paired row layout (admm_kernels.hpp ld_row) for the image side
    static int r2c(const float* img, cf* spec, const cf* twW, long long rows, hipStream_t s, bool pl = false) {
        if (pl)
            hipLaunchKernelGGL((k_row_r2c<N, true>), dim3(blocks(rows)), dim3(G::NT), G::lds_bytes(), s, img, spec, twW, rows);
        else
            hipLaunchKernelGGL((k_row_r2c<N, false>), dim3(blocks(rows)), dim3(G::NT), G::lds_bytes(), s, img, spec, twW, rows);
        return launch_check("k_row_r2c");
    }
    static int c2r(const cf* spec, float* img, const cf* twW, long long rows, hipStream_t s, bool pl = false) {
        if (pl)
            hipLaunchKernelGGL((k_row_c2r<N, true>), dim3(blocks(rows)), dim3(G::NT), G::lds_bytes(), s, spec, img, twW, rows);
        else
            hipLaunchKernelGGL((k_row_c2r<N, false>), dim3(blocks(rows)), dim3(G::NT), G::lds_bytes(), s, spec, img, twW, rows);
        return launch_check("k_row_c2r");
    }
    static int pair(const float* img, float* out, long long rows, hipStream_t s) {
        hipLaunchKernelGGL(k_row_pair<N>, dim3(blocks(rows)), dim3(G::NT), 0, s, img, out, rows);
        return launch_check("k_row_pair");
    }
    template <bool ISO, bool FIRST, bool HIST, bool PL> static void pa(const PassAArgs& a, unsigned nb, hipStream_t s) {
        hipLaunchKernelGGL((k_pass_a<N, ISO, FIRST, HIST, PL>), dim3(nb), dim3(G::NT), G::lds_bytes(), s, a);
    }
    // the solve with bounds on x (k_pass_a BOX): the plain walk, at every row width the kernel is built for
    template <bool ISO, bool FIRST, bool PL> static void pa_box(const PassAArgs& a, unsigned nb, hipStream_t s) {
        hipLaunchKernelGGL((k_pass_a<N, ISO, FIRST, false, PL, false, false, true>), dim3(nb), dim3(G::NT), G::lds_bytes(), s, a);
    }
    // the cooperative variant (admm_kernels.hpp k_pass_a COOP): aniso inference at 1,024-pixel rows
    // (sub-groups of one wave; the iso variant of it spills at 3 waves per SIMD and is not built)
    static constexpr bool kCoop = N == 512;
    // pf: its pipelined form (k_pass_a PF: every row stream loaded a row ahead, 2 waves per SIMD)
    template <bool FIRST, bool PL> static void pa_coop(const PassAArgs& a, unsigned nb, hipStream_t s, bool pf) {
        if constexpr (kCoop) {
            if (pf)
                hipLaunchKernelGGL((k_pass_a<N, false, FIRST, false, PL, true, true>), dim3(nb), dim3(G::NT), passa_coop_lds<N>(), s, a);
            else
                hipLaunchKernelGGL((k_pass_a<N, false, FIRST, false, PL, true>), dim3(nb), dim3(G::NT), passa_coop_lds<N>(), s, a);
        }
    }
    // coop: launch the cooperative variant where it can run -- whole blocks of SG strips inside one
    // plane (its exchange barriers need every wave of a block), strips of two rows or more
    static int pass_a(const PassAArgs& a, bool iso, bool first, bool hist, hipStream_t s, bool pl = false,
                      bool coop = false, bool pf = false) {
        const unsigned nb = blocks(a.nstrips);
        const int sel = (iso ? 4 : 0) | (first ? 2 : 0) | (hist ? 1 : 0);
        if (a.v) {  // bounds on x: the plain kernel's BOX instantiation, also where inference runs the cooperative one
            if (hist) return fail(ADMM_TV_EINVAL, "k_pass_a: bounds on x in a training pass");
            switch ((iso ? 4 : 0) | (first ? 2 : 0) | (pl ? 1 : 0)) {
                case 0: pa_box<false, false, false>(a, nb, s); break;
                case 1: pa_box<false, false, true>(a, nb, s); break;
                case 2: pa_box<false, true, false>(a, nb, s); break;
                case 3: pa_box<false, true, true>(a, nb, s); break;
                case 4: pa_box<true, false, false>(a, nb, s); break;
                case 5: pa_box<true, false, true>(a, nb, s); break;
                case 6: pa_box<true, true, false>(a, nb, s); break;
                default: pa_box<true, true, true>(a, nb, s); break;
            }
            return launch_check("k_pass_a<box>");
        }
        if (kCoop && coop && !iso && !hist && !a.rev && a.R >= 2 && a.nstrips % G::SG == 0 &&
            (a.H / a.R) % G::SG == 0) {
            static_assert(!kCoop || passa_coop_lds<N>() <= 53 * 1024, "three blocks of the row pass per CU");
            // (the pipelined kernel addresses a plane through 32-bit buffer offsets)
            pf = pf && (long long)a.H * N * (long long)sizeof(cf) < (1LL << 31);
            if (first) pl ? pa_coop<true, true>(a, nb, s, pf) : pa_coop<true, false>(a, nb, s, pf);
            else pl ? pa_coop<false, true>(a, nb, s, pf) : pa_coop<false, false>(a, nb, s, pf);
            return launch_check("k_pass_a");
        }
        if (pl && !hist) {  // inference: lane-paired images
            switch (sel) {
                case 0: pa<false, false, false, true>(a, nb, s); break;
                case 2: pa<false, true, false, true>(a, nb, s); break;
                case 4: pa<true, false, false, true>(a, nb, s); break;
                default: pa<true, true, false, true>(a, nb, s); break;
            }
            return launch_check("k_pass_a");
        }
        switch (sel) {
            case 0: pa<false, false, false, false>(a, nb, s); break;
            case 1: pa<false, false, true, false>(a, nb, s); break;
            case 2: pa<false, true, false, false>(a, nb, s); break;
            case 3: pa<false, true, true, false>(a, nb, s); break;
            case 4: pa<true, false, false, false>(a, nb, s); break;
            case 5: pa<true, false, true, false>(a, nb, s); break;
            case 6: pa<true, true, false, false>(a, nb, s); break;
            default: pa<true, true, true, false>(a, nb, s); break;
        }
        return launch_check("k_pass_a");
    }
    static int iso_norm(const IsoArgs& a, bool first, bool hist, hipStream_t s, bool pl = false) {
        const unsigned nb = blocks(a.nitems);
        if (first && pl)
            hipLaunchKernelGGL((k_iso_norm<N, true, false, true>), dim3(nb), dim3(G::NT), G::lds_bytes(), s, a);
        else if (first)
            hipLaunchKernelGGL((k_iso_norm<N, true, false, false>), dim3(nb), dim3(G::NT), G::lds_bytes(), s, a);
        else if (hist)
            hipLaunchKernelGGL((k_iso_norm<N, false, true, false>), dim3(nb), dim3(G::NT), G::lds_bytes(), s, a);
        else if (pl)
            hipLaunchKernelGGL((k_iso_norm<N, false, false, true>), dim3(nb), dim3(G::NT), G::lds_bytes(), s, a);
        else
            hipLaunchKernelGGL((k_iso_norm<N, false, false, false>), dim3(nb), dim3(G::NT), G::lds_bytes(), s, a);
        return launch_check("k_iso_norm");
    }
    template <bool ISO, bool LASTK, bool FIRSTK> static void bpa(const BwdArgs& a, unsigned nb, hipStream_t s) {
        using BG = BwdGeom<N>;
        hipLaunchKernelGGL((k_bwd_pass_a<N, ISO, LASTK, FIRSTK>), dim3(nb), dim3(BG::NT), BG::lds_bytes(), s, a);
    }
    static int bwd_pass_a(const BwdArgs& a, bool iso, bool lastk, bool firstk, hipStream_t s) {
        const unsigned nb = (unsigned)((a.nstrips + BwdGeom<N>::SG - 1) / BwdGeom<N>::SG);  // its own strips per block
        const int sel = (iso ? 4 : 0) | (lastk ? 2 : 0) | (firstk ? 1 : 0);
        switch (sel) {
            case 0: bpa<false, false, false>(a, nb, s); break;
            case 1: bpa<false, false, true>(a, nb, s); break;
            case 2: bpa<false, true, false>(a, nb, s); break;
            case 3: bpa<false, true, true>(a, nb, s); break;
            case 4: bpa<true, false, false>(a, nb, s); break;
            case 5: bpa<true, false, true>(a, nb, s); break;
            case 6: bpa<true, true, false>(a, nb, s); break;
            default: bpa<true, true, true>(a, nb, s); break;
        }
        return launch_check("k_bwd_pass_a");
    }
    static int bwd_iso_q(const BwdIsoArgs& a, bool lastk, hipStream_t s) {
        const unsigned nb = blocks(a.nitems);
        if (lastk)
            hipLaunchKernelGGL((k_bwd_iso_q<N, true>), dim3(nb), dim3(G::NT), G::lds_bytes(), s, a);
        else
            hipLaunchKernelGGL((k_bwd_iso_q<N, false>), dim3(nb), dim3(G::NT), G::lds_bytes(), s, a);
        return launch_check("k_bwd_iso_q");
    }
};

template <class F> int with_row(int N, F&& f) {
    switch (N) {
        case 8: return f(RowOps<8>{});
        case 16: return f(RowOps<16>{});
        case 32: return f(RowOps<32>{});
        case 64: return f(RowOps<64>{});
        case 128: return f(RowOps<128>{});
        case 256: return f(RowOps<256>{});
        case 512: return f(RowOps<512>{});
        case 1024: return f(RowOps<1024>{});
        default: return fail(ADMM_TV_EUNSUPPORTED, "unsupported W");
    }
}

// ------------------------------------------------------------------ column-side ops (templated on H, C)
// f(integral_constant H) for the power-of-two column lengths
template <class F> int with_col(int H, F&& f) {
    switch (H) {
        case 16: return f(std::integral_constant<int, 16>{});
        case 32: return f(std::integral_constant<int, 32>{});
        case 64: return f(std::integral_constant<int, 64>{});
        case 128: return f(std::integral_constant<int, 128>{});
        case 256: return f(std::integral_constant<int, 256>{});
        case 512: return f(std::integral_constant<int, 512>{});
        case 1024: return f(std::integral_constant<int, 1024>{});
        case 2048: return f(std::integral_constant<int, 2048>{});
        case 4096: return f(std::integral_constant<int, 4096>{});
        default: return fail(ADMM_TV_EUNSUPPORTED, "unsupported H");
    }
}

// column-pass tile order (k_pass_b pb_tile): planes per group, 1 = plane-major.  Two planes at
// H >= 1024 (C3 pass B 0.376 -> 0.362 ms, C3 iso 0.381 -> 0.369; 4 and 8 planes slower: DRAM
// locality), plane-major below (C2: neutral).  A/B knob ADMM_PASSB_GROUP.
// values per lane of the column transforms (RowCfg<H>::E)
int col_e(int H) { return H >= 1024 ? 16 : H >= 64 ? 8 : 4; }

int passb_order(int H) { return std::max(1, std::min(64, env_int("ADMM_PASSB_GROUP", H >= 1024 ? 2 : 1))); }

// planes per pass B block (k_pass_b gp): the block keeps its multipliers in registers across them
// and reads the Wiener-factor table once per gp planes.  A divisor of the planes per module (a group
// never straddles two Wiener factors).  Measured at C3 (profiles/r03_ab_passb_gp.txt): gp = 4 takes
// pass B 0.346 -> 0.336 ms but the following pass A +1.5 % (whole iteration +-0), gp = 8 slower;
// default 1.  ADMM_PASSB_GP (A/B knob) overrides it.
int passb_gp(int H, int P, int ppm) {
    (void)H;
    int g = env_int("ADMM_PASSB_GP", 1);
    g = std::max(1, std::min(g, 64));
    while (g > 1 && (ppm % g)) --g;
    (void)P;
    return g;
}

// bank: a PSF bank's table index (k_pass_b<H, C, MODE, BankIdx>; ppm is then the run of planes that share a table, which gp
// divides: 1 for per-channel and per-plane banks, C for per-image ones), null for the shared PSF
template <int H, int C> int pass_b_hc(const cf* spec, cf* out, const float* fcT, const cf* mT, const cf* twH, int N,
                                      int P, int mode, int ppm, hipStream_t s, const BankIdx* bank) {
    using G = ColGeom<H, C>;
    const int colblocks = N / C;
    const int gp = passb_gp(H, P, ppm);
    const dim3 grid((unsigned)((long long)((P + gp - 1) / gp) * colblocks));
    const int order = gp > 1 ? 1 : passb_order(H);
    const int fpack = mode == 0 && env_int("ADMM_PASSB_FPACK", 1) ? 1 : 0;  // A/B knob
    // block remap / plane order (k_pass_b pmode): contiguous XCD ranges (2), plane groups walked
    // forward; the reverse walk (3) takes pass B alone 0.3465 -> 0.3420 ms at C3 but the iteration is
    // faster with the forward one (4 interleaved rounds: C3 706-722 -> 710-728 it/s, C2 5,572 ->
    // 5,624, C3 iso +0.5 %; profiles/r03_sweep_knobs_c3.txt); pair-interleaved remap (4, 5) +9 %
    // (profiles/r03_ab_passb_order.txt)
    const int pmode = env_int("ADMM_PASSB_PMODE", 2);
    if (bank) {  // the Wiener factor (mode 0), H_t (mode 1) and its adjoint (mode 2)
        if (mode == 0) {
            if (int e = set_lds(k_pass_b<H, C, 0, BankIdx>, G::lds_bytes())) return e;
            hipLaunchKernelGGL((k_pass_b<H, C, 0, BankIdx>), grid, dim3(G::NT), G::lds_bytes(), s, spec, out, fcT, mT, twH, N,
                               colblocks, ppm, order, fpack, gp, P, pmode, *bank);
        } else if (mode == 1) {
            if (int e = set_lds(k_pass_b<H, C, 1, BankIdx>, G::lds_bytes())) return e;
            hipLaunchKernelGGL((k_pass_b<H, C, 1, BankIdx>), grid, dim3(G::NT), G::lds_bytes(), s, spec, out, fcT, mT, twH, N,
                               colblocks, ppm, order, fpack, gp, P, pmode, *bank);
        } else {  // the training backward's x^_in = H_t^T b^: each plane's conjugate multiplier
            if (int e = set_lds(k_pass_b<H, C, 2, BankIdx>, G::lds_bytes())) return e;
            hipLaunchKernelGGL((k_pass_b<H, C, 2, BankIdx>), grid, dim3(G::NT), G::lds_bytes(), s, spec, out, fcT, mT, twH, N,
                               colblocks, ppm, order, fpack, gp, P, pmode, *bank);
        }
        return launch_check("k_pass_b<bank>");
    }
    if (mode == 0) {
        if (int e = set_lds(k_pass_b<H, C, 0>, G::lds_bytes())) return e;
        hipLaunchKernelGGL((k_pass_b<H, C, 0>), grid, dim3(G::NT), G::lds_bytes(), s, spec, out, fcT, mT, twH, N, colblocks, ppm,
                           order, fpack, gp, P, pmode);
    } else if (mode == 1) {
        if (int e = set_lds(k_pass_b<H, C, 1>, G::lds_bytes())) return e;
        hipLaunchKernelGGL((k_pass_b<H, C, 1>), grid, dim3(G::NT), G::lds_bytes(), s, spec, out, fcT, mT, twH, N, colblocks, ppm,
                           order, fpack, gp, P, pmode);
    } else {
        if (int e = set_lds(k_pass_b<H, C, 2>, G::lds_bytes())) return e;
        hipLaunchKernelGGL((k_pass_b<H, C, 2>), grid, dim3(G::NT), G::lds_bytes(), s, spec, out, fcT, mT, twH, N, colblocks, ppm,
                           order, fpack, gp, P, pmode);
    }
    return launch_check("k_pass_b");
}

template <int H> int pass_b_h(const cf* spec, cf* out, const float* fcT, const cf* mT, const cf* twH, int N, int P,
                              int mode, int ppm, hipStream_t s, const BankIdx* bank) {
    constexpr int L = ColGeom<H, 1>::L;
    if constexpr (L <= 64) {
        // column pairs with 16-byte accesses (k_pass_b2): measured faster up to H = 512 (C2: pass B
        // -7.5 %, same bits); at H = 1024 the doubled register set costs occupancy (+30 %)
        if (mode == 0 && N >= 16 && env_int("ADMM_PASSB_PAIR", H <= 512 ? 1 : 0)) {
            using G = ColGeom<H, 8>;
            const int colblocks = N / 16;
            if (bank) {
                if (int e = set_lds(k_pass_b2<H, 8, BankIdx>, G::lds_bytes())) return e;
                hipLaunchKernelGGL((k_pass_b2<H, 8, BankIdx>), dim3((unsigned)((long long)P * colblocks)), dim3(G::NT),
                                   G::lds_bytes(), s, spec, out, fcT, twH, N, colblocks, ppm, passb_order(H),
                                   env_int("ADMM_PASSB_FPACK", 1) ? 1 : 0, *bank);
                return launch_check("k_pass_b2<bank>");
            }
            if (int e = set_lds(k_pass_b2<H, 8>, G::lds_bytes())) return e;
            hipLaunchKernelGGL((k_pass_b2<H, 8>), dim3((unsigned)((long long)P * colblocks)), dim3(G::NT), G::lds_bytes(),
                               s, spec, out, fcT, twH, N, colblocks, ppm, passb_order(H), env_int("ADMM_PASSB_FPACK", 1) ? 1 : 0);
            return launch_check("k_pass_b2");
        }
        int C = env_int("ADMM_PASSB_C", 8);
        if (C > N) C = N;
        if (C >= 16) return pass_b_hc<H, 16>(spec, out, fcT, mT, twH, N, P, mode, ppm, s, bank);
        return pass_b_hc<H, 8>(spec, out, fcT, mT, twH, N, P, mode, ppm, s, bank);
    } else if constexpr (L == 128) {
        return pass_b_hc<H, 8>(spec, out, fcT, mT, twH, N, P, mode, ppm, s, bank);
    } else {
        return pass_b_hc<H, 4>(spec, out, fcT, mT, twH, N, P, mode, ppm, s, bank);
    }
}

// column pass; out == spec (in place) or a separate buffer
// ppm: planes per module (module m = plane / ppm uses Wiener factor m); ppm = P for one module
int pass_b_oop(int H, const cf* spec, cf* out, const float* fcT, const cf* mT, const cf* twH, int N, int P, int mode,
               hipStream_t s, int ppm = 0, const BankIdx* bank = nullptr) {
    if (ppm <= 0) ppm = P;
    return with_col(H, [&](auto h) { return pass_b_h<decltype(h)::value>(spec, out, fcT, mT, twH, N, P, mode, ppm, s, bank); });
}

int pass_b(int H, cf* spec, const float* fcT, const cf* mT, const cf* twH, int N, int P, int mode, hipStream_t s,
           int ppm = 0, const BankIdx* bank = nullptr) {
    return pass_b_oop(H, spec, spec, fcT, mT, twH, N, P, mode, s, ppm, bank);
}

// cross-spectrum partials sum_{p in group} conj(colFFT U_p) colFFT V_p  -> part[g][N+1][H]
// xb: a PSF bank's gradient -- T x xb->cpt plane groups, each a chunk of one table's planes (XBank)
template <int H, int C> int xspec_hc(const cf* U, const cf* V, cf* part, const cf* twH, int N, int P, int ppg,
                                     hipStream_t s, const XBank* xb, int T) {
    using G = ColGeom<H, C>;
    const int colblocks = N / C;
    if (xb) {
        const int groups = T * xb->cpt;
        if (int e = set_lds(k_xspec<H, C, true, XBank>, G::lds_bytes())) return e;
        if (int e = set_lds(k_xspec<H, C, false, XBank>, G::lds_bytes())) return e;
        hipLaunchKernelGGL((k_xspec<H, C, true, XBank>), dim3(groups), dim3(G::NT), G::lds_bytes(), s, U, V, part, twH, N,
                           colblocks, P, ppg, *xb);
        if (colblocks > 1)
            hipLaunchKernelGGL((k_xspec<H, C, false, XBank>), dim3(groups * (colblocks - 1)), dim3(G::NT), G::lds_bytes(), s,
                               U, V, part, twH, N, colblocks, P, ppg, *xb);
        return launch_check("k_xspec<bank>");
    }
    const int groups = (P + ppg - 1) / ppg;
    if (int e = set_lds(k_xspec<H, C, true>, G::lds_bytes())) return e;
    if (int e = set_lds(k_xspec<H, C, false>, G::lds_bytes())) return e;
    hipLaunchKernelGGL((k_xspec<H, C, true>), dim3(groups), dim3(G::NT), G::lds_bytes(), s, U, V, part, twH, N,
                       colblocks, P, ppg);
    if (colblocks > 1)
        hipLaunchKernelGGL((k_xspec<H, C, false>), dim3(groups * (colblocks - 1)), dim3(G::NT), G::lds_bytes(), s, U,
                           V, part, twH, N, colblocks, P, ppg);
    return launch_check("k_xspec");
}
template <int H> int xspec_h(const cf* U, const cf* V, cf* part, const cf* twH, int N, int P, int ppg, hipStream_t s,
                             const XBank* xb, int T) {
    constexpr int L = ColGeom<H, 1>::L;
    if constexpr (L <= 64) return xspec_hc<H, 8>(U, V, part, twH, N, P, ppg, s, xb, T);
    else if constexpr (L == 128) return xspec_hc<H, 8>(U, V, part, twH, N, P, ppg, s, xb, T);
    else return xspec_hc<H, 4>(U, V, part, twH, N, P, ppg, s, xb, T);
}
int xspec(int H, const cf* U, const cf* V, cf* part, const cf* twH, int N, int P, int ppg, hipStream_t s,
          const XBank* xb = nullptr, int T = 0) {
    return with_col(H, [&](auto h) { return xspec_h<decltype(h)::value>(U, V, part, twH, N, P, ppg, s, xb, T); });
}

// grouped modules train only on the fused power-of-two path (a smooth size solves them one after
// another for inference only; training there takes one call per module)
int grouped_train_check(const admm_tv_desc& d) {
    if (d.groups > 1 && !supported_hw(d.H, d.W))
        return fail(ADMM_TV_EUNSUPPORTED, "grouped training needs power-of-two H, W: one call per module");
    return 0;
}

int validate(const admm_tv_desc* d) {
    if (!d) return fail(ADMM_TV_EINVAL, "null descriptor");
    const bool empty_ok = d->iso && d->allreduce && d->B >= 0 && d->C >= 0;  // see participate_only
    if ((empty_ok ? (d->B < 0 || d->C < 0) : (d->B <= 0 || d->C <= 0)) || d->H <= 0 || d->W <= 0 || d->maxit < 0 ||
        d->kh < 0 || d->kw < 0 || d->groups < 0)
        return fail(ADMM_TV_EINVAL, "invalid sizes or maxit");
    if (d->kh != d->kw) return fail(ADMM_TV_ENONSQUARE, "non-square PSF (the reference's H_t swaps H/W pads)");
    if (is_f64(*d) ? !f64_hw(d->H, d->W) : (!supported_hw(d->H, d->W) && !generic_hw(d->H, d->W)))
        return fail(ADMM_TV_EUNSUPPORTED, "unsupported H, W (admm_tv_supported / admm_tv_supported_f64: up to 65,536)");
    if (is_f64(*d) && d->groups > 1) return fail(ADMM_TV_EUNSUPPORTED, "groups > 1: fp32 only");
    if (d->kh > d->H || d->kw > d->W) return fail(ADMM_TV_EKERNEL, "PSF larger than the image");
    if (d->groups > 1 && ((!supported_hw(d->H, d->W) && !mixed_hw(d->H, d->W)) || (d->flags & ADMM_TV_FLAG_PSF_GRAD)))
        return fail(ADMM_TV_EUNSUPPORTED, "groups > 1 needs power-of-two or smooth H, W and no PSF gradient");
    return 0;
}

// what a PSF bank refuses (after validate, before any other check, in every entry point, size query and
// admm_tv_path alike).  train: a training entry point; f64: an *_f64 entry point
int bank_check(const admm_tv_desc& d, bool train = false, bool f64 = false) {
    // training with a bank is opted into (ADMM_TV_FLAG_PSF_BANK_TRAIN): without the bit a bank answers as it did
    // before the bit existed, so a caller can probe an older library of the same ABI version with bank | bit
    const bool bt = (d.flags & ADMM_TV_FLAG_PSF_BANK_TRAIN) != 0;
    if (!is_bank(d)) {
        if (bt) return fail(ADMM_TV_EINVAL, "ADMM_TV_FLAG_PSF_BANK_TRAIN without a PSF bank (ADMM_TV_FLAG_PSF_PER_IMAGE / _PER_CHANNEL)");
        return 0;
    }
    if (f64 || is_f64(d)) return fail(ADMM_TV_EUNSUPPORTED, "PSF bank: fp32 only (ADMM_TV_FLAG_F64 / an _f64 entry point)");
    if (train && !bt)
        return fail(ADMM_TV_EUNSUPPORTED, "PSF bank: inference only without ADMM_TV_FLAG_PSF_BANK_TRAIN (training with a bank is opt-in)");
    if ((d.flags & ADMM_TV_FLAG_PSF_GRAD) && !bt)
        return fail(ADMM_TV_EUNSUPPORTED, "PSF bank: no PSF gradient (ADMM_TV_FLAG_PSF_GRAD) without ADMM_TV_FLAG_PSF_BANK_TRAIN");
    if (d.kh == 0) return fail(ADMM_TV_EINVAL, "PSF bank without a PSF (kh == 0)");
    if (d.groups > 1) return fail(ADMM_TV_EUNSUPPORTED, "PSF bank: groups > 1 (one solve per module)");
    if (d.allreduce) return fail(ADMM_TV_EUNSUPPORTED, "PSF bank: no cross-rank all-reduce hook");
    const long long T = ((d.flags & ADMM_TV_FLAG_PSF_PER_IMAGE) ? d.B : 1) * ((d.flags & ADMM_TV_FLAG_PSF_PER_CHANNEL) ? d.C : 1);
    if (T > kBankMax || d.B > 0x7fffffffLL || d.C > 0x7fffffffLL)
        return fail(ADMM_TV_EUNSUPPORTED, "PSF bank: more than 65,535 PSFs");
    return 0;
}

// the multiplier tables carry the transforms' normalisation: the packed power-of-two row
// transforms produce 2 rfft, the generic ones rfft
double spectra_scale(int H, int W) {
    return (supported_hw(H, W) ? 0.5 : 1.0) / ((double)H * (double)W);
}

// k_spectra_bank with every table's sigma kept (training with a bank and a PSF gradient: T sigma tables, table after
// table).  Defined here, in the one unit that launches it, so that the shared header's kernels compile as before.
static __global__ void k_spectra_bank_sigma(const double2* __restrict__ G, const double2* __restrict__ twHd,
                                            const float* __restrict__ rho_p, float* __restrict__ fcT,
                                            cf* __restrict__ mT, int k, int H, int N, int W,
                                            double2* __restrict__ sigma_out, double scale) {
    const size_t n = (size_t)(N + 1) * H;
    spectra_body<float>(G + (size_t)blockIdx.y * k * (N + 1), twHd, rho_p, fcT + blockIdx.y * n, mT + blockIdx.y * n, k, H,
                        N, W, sigma_out + blockIdx.y * n, scale);
}

// The PSF tables of a bank (setup's PSF part, after its twiddle tables): every kernel takes its table from the
// grid's second dimension, so a bank of B C PSFs is set up by the launches one PSF takes.  rho is the bank's.
// bank_spectra: the Wiener factors into fcT (T tables) and the H_t multipliers (with their smooth-size copy).
int bank_spectra(const admm_tv_desc& d, const Layout& Lo, void* ws, const float* rho, float* fcT, hipStream_t s) {
    const int H = (int)d.H, W = (int)d.W, N = W / 2, nt = 256, n = (N + 1) * H;
    const unsigned T = (unsigned)bank_of(d).T;
    if (Lo.sigma) {  // training with a PSF gradient: every table's sigma is kept
        hipLaunchKernelGGL(k_spectra_bank_sigma, dim3((n + nt - 1) / nt, T), dim3(nt), 0, s, at<double2>(ws, Lo.G),
                           at<double2>(ws, Lo.twHd), rho, fcT, at<cf>(ws, Lo.mT), d.kh, H, N, W, at<double2>(ws, Lo.sigma),
                           spectra_scale(H, W));
        if (int e = launch_check("k_spectra_bank_sigma")) return e;
    } else {
        hipLaunchKernelGGL(k_spectra_bank, dim3((n + nt - 1) / nt, T), dim3(nt), 0, s, at<double2>(ws, Lo.G),
                           at<double2>(ws, Lo.twHd), rho, fcT, at<cf>(ws, Lo.mT), d.kh, H, N, W, spectra_scale(H, W));
        if (int e = launch_check("k_spectra_bank")) return e;
    }
    if (Lo.mixed) return hip_code(admm_mixed::mt_mixed(at<cf>(ws, Lo.mT), at<cf>(ws, Lo.mM), H, N, s, (int)T), "k_mt_mixed_bank");
    return 0;
}
int setup_bank(const admm_tv_desc& d, const Layout& Lo, void* ws, const float* kern, const float* rho, hipStream_t s) {
    const int H = (int)d.H, W = (int)d.W, N = W / 2, k = d.kh, nt = 256, n = (N + 1) * H;
    const unsigned T = (unsigned)bank_of(d).T;
    hipLaunchKernelGGL(k_psf_rows_bank, dim3((k * (N + 1) + nt - 1) / nt, T), dim3(nt), 0, s, kern, at<double2>(ws, Lo.G), k,
                       N, W);
    if (int e = launch_check("k_psf_rows_bank")) return e;
    if (!rho) return 0;
    float* fc = at<float>(ws, Lo.fcT);
    if (int e = bank_spectra(d, Lo, ws, rho, fc, s)) return e;
    if (!Lo.gen) {  // the packed copies follow the T tables
        hipLaunchKernelGGL(k_fc_pack_bank, dim3((n + nt - 1) / nt, T), dim3(nt), 0, s, fc, fc + (size_t)T * n, H, N, col_e(H));
        if (int e = launch_check("k_fc_pack_bank")) return e;
    }
    if (Lo.mixed) return hip_code(admm_mixed::fc_mixed(fc, at<float>(ws, Lo.fcM), H, N, s, (int)T), "k_fc_mixed_bank");
    return 0;
}

// setup: twiddle tables, PSF spectrum, Wiener factor (if rho given), centred-PSF multiplier
// box: the Wiener factor of the solve with bounds on x (k_spectra: + rho in the denominator)
template <class T>
int setup(const admm_tv_desc& d, const Layout& Lo, void* ws, const T* kern, const T* rho, hipStream_t s, bool box = false) {
    using C = cx_t<T>;
    ProfScope ps(3, s);
    const int H = (int)d.H, W = (int)d.W, N = W / 2, k = d.kh;
    const int nt = 256;
    hipLaunchKernelGGL(k_tables<C>, dim3((std::max(H, W) + nt - 1) / nt), dim3(nt), 0, s, at<C>(ws, Lo.twW),
                       at<C>(ws, Lo.twH), at<double2>(ws, Lo.twHd), H, W);
    if (int e = launch_check("k_tables")) return e;
    if (Lo.gen && !std::is_same<T, double>::value) {  // Bluestein tables of the row and column plans
        for (int dim = 0; dim < 2; ++dim) {
            const GPlan pl = make_plan(dim == 0 ? W : H);
            if (pl.ntab == 0) continue;
            hipLaunchKernelGGL(k_blue_tables, dim3((3 * 1024 * 64 + nt - 1) / nt), dim3(nt), 0, s,  // a wave per entry
                               at<cf>(ws, dim == 0 ? Lo.twW : Lo.twH), pl);
            if (int e = launch_check("k_blue_tables")) return e;
        }
    }
    if constexpr (std::is_same<T, float>::value) {
        if (is_bank(d)) return setup_bank(d, Lo, ws, kern, rho, s);
    }
    if (k > 0) {
        const int n = k * (N + 1);
        hipLaunchKernelGGL(k_psf_rows<T>, dim3((n + nt - 1) / nt), dim3(nt), 0, s, kern, at<double2>(ws, Lo.G), k, N, W);
        if (int e = launch_check("k_psf_rows")) return e;
    }
    const int n = (N + 1) * H;
    if (rho) {
        for (int g = 0; g < ngroups_of(d); ++g) {  // one Wiener factor per module
            hipLaunchKernelGGL(k_spectra<T>, dim3((n + nt - 1) / nt), dim3(nt), 0, s, at<double2>(ws, Lo.G),
                               at<double2>(ws, Lo.twHd), rho + g, at<T>(ws, Lo.fcT) + (size_t)g * n, at<C>(ws, Lo.mT),
                               k, H, N, W, Lo.sigma ? at<double2>(ws, Lo.sigma) : nullptr,
                               (std::is_same<T, double>::value ? 1.0 / ((double)H * W) : spectra_scale(H, W)), box ? 1 : 0);
            if (int e = launch_check("k_spectra")) return e;
            if constexpr (std::is_same<T, float>::value) if (!Lo.gen) {
                float* fc = at<float>(ws, Lo.fcT) + (size_t)g * n;
                hipLaunchKernelGGL(k_fc_pack, dim3((n + nt - 1) / nt), dim3(nt), 0, s, fc,
                                   fc + (size_t)ngroups_of(d) * n, H, N, col_e(H));
                if (int e = launch_check("k_fc_pack")) return e;
            }
            if constexpr (std::is_same<T, float>::value) if (Lo.mixed) {
                if (int e = hip_code(admm_mixed::fc_mixed(at<float>(ws, Lo.fcT) + (size_t)g * n,
                                                          at<float>(ws, Lo.fcM) + (size_t)g * (2 * N + 1) * H, H, N, s),
                                     "k_fc_mixed"))
                    return e;
            }
            if constexpr (std::is_same<T, float>::value) if (Lo.gen && Lo.mm.ok && ngroups_of(d) == 1) {
                float* fc = at<float>(ws, Lo.fcT);  // the generic path has one module (grouped: the mixed path)
                hipLaunchKernelGGL(k_fc_transpose, dim3(std::min(4096, (n + nt - 1) / nt)), dim3(nt), 0, s, fc, fc + n, H,
                                   N + 1);
                if (int e = launch_check("k_fc_transpose")) return e;
            }
        }
        if constexpr (std::is_same<T, float>::value) if (Lo.mixed && k > 0) {
            if (int e = hip_code(admm_mixed::mt_mixed(at<cf>(ws, Lo.mT), at<cf>(ws, Lo.mM), H, N, s), "k_mt_mixed")) return e;
        }
    }
    return 0;
}

int pow2_floor(int v);

// coop: the solve's row pass may run the cooperative kernel (aniso inference, its knob on, no ADMM_PASSA_REV)
int strip_rows(int H, int N, long long rows, bool aniso_fwd = false, bool coop = false) {
    int R = env_int("ADMM_PASSA_R", 0);
    // A/B knob: a strip must tile H exactly (pass A maps strip -> (plane, first row) by H / R),
    // so an override is rounded down to a power of two in [2, H]; <= 0 selects the rule below
    if (R > 0) R = pow2_floor(std::max(2, std::min(R, H)));
    if (R <= 0) {
        // rows per strip (measured on MI355X, tools/sweep.py: R = 8 beats 16 at W = 1024 with
        // the 3-waves/SIMD row pass); halve while there are fewer than ~3 waves per SIMD of
        // strips.  The aniso forward at W = 512 (with the XCD strip remap) takes R = 16 down to
        // ~1.5 waves per SIMD of strips: C2 pass A 0.126 -> 0.120 ms; the iso row pass there
        // keeps the rule (C5 module: R = 4 best).
        const int L = std::min(64, N / (N >= 1024 ? 16 : N >= 64 ? 8 : N >= 16 ? 4 : 2));
        long long want = 3LL * 1024 * 64 / L;
        R = 8;
        if (aniso_fwd && N == 256) {
            R = 16;
            want /= 2;
        }
        // The cooperative row pass at W = 1024 (halo rows shared inside a block, every stream loaded a row
        // ahead, 2 waves per SIMD): R = 4, interleaved on one MI355X (profiles/r08_ab_env_c3_passa_pipeline.txt)
        // C3 745.6-749.4 it/s against 729.7-730.7 with R = 8 and 733.6-736.5 with R = 2.  Only where that
        // kernel launches (RowOps::pass_a: whole blocks of four strips inside a plane; rows is a multiple
        // of H): the plain kernel keeps R = 8, which measured best for it.
        if (coop && aniso_fwd && N == 512 && (H / 4) % 4 == 0) R = 4;
        while (R > 2 && rows / R < want) R /= 2;
    }
    if (R > H) R = H;
    return R;
}

// The device a call runs on is the device of its stream (the legacy default stream: the current
// device).  Every entry point switches to it for the duration of the call and switches back, so
// an input on cuda:1 solved while the current device is 0 launches, records and waits on device 1.
struct DeviceGuard {
    int prev = -1, dev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(hipStream_t s) {
        err = hipGetDevice(&prev);
        if (err != hipSuccess) return;
        dev = prev;
        if (s) {
            hipDevice_t d = 0;
            err = hipStreamGetDevice(s, &d);
            if (err != hipSuccess) return;
            dev = (int)d;
        }
        if (dev != prev) err = hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0 && dev != prev) (void)hipSetDevice(prev);
    }
    // the entry points' check: 0, or the error of finding / selecting the stream's device
    int check() const {
        return err == hipSuccess ? 0 : fail(ADMM_TV_EHIP, std::string("device of the stream: ") + hipGetErrorString(err));
    }
};

// Auxiliary streams of the two-stream solves, one per (device, caller stream): two solves on
// independent caller streams keep independent auxiliary streams (no false dependency between
// them), and every thread that uses the same caller stream shares its auxiliary stream (no
// per-thread leak).  Bounded: beyond kAuxPerDev caller streams per device the entries are reused
// round-robin (a reused entry only adds ordering, never a hazard).  The streams live until the
// process ends (destroying them from a static destructor could race the HIP runtime's teardown).
constexpr int kMaxAux = 3;  // auxiliary streams per caller stream (solves on up to 4 streams)
struct AuxEntry {
    hipStream_t caller = nullptr, aux[kMaxAux] = {};
};
constexpr int kAuxDev = 64, kAuxPerDev = 32;
struct AuxPool {
    std::mutex mu;
    AuxEntry e[kAuxDev][kAuxPerDev];
    int used[kAuxDev] = {}, next[kAuxDev] = {};
} g_aux;

// the k-th auxiliary stream (k < kMaxAux) paired with caller stream s on device dev (the current
// device, see DeviceGuard), created on first use
hipStream_t aux_stream(hipStream_t s, int dev, int k = 0) {
    if (dev < 0 || dev >= kAuxDev || k < 0 || k >= kMaxAux) return nullptr;
    std::lock_guard<std::mutex> lk(g_aux.mu);
    AuxEntry* row = g_aux.e[dev];
    AuxEntry* slot = nullptr;
    for (int i = 0; i < g_aux.used[dev] && !slot; ++i)
        if (row[i].caller == s) slot = &row[i];
    if (!slot) {
        if (g_aux.used[dev] < kAuxPerDev) {
            slot = &row[g_aux.used[dev]++];
        } else {
            slot = &row[g_aux.next[dev]];
            g_aux.next[dev] = (g_aux.next[dev] + 1) % kAuxPerDev;
        }
        slot->caller = s;
    }
    if (!slot->aux[k] && hipStreamCreateWithFlags(&slot->aux[k], hipStreamNonBlocking) != hipSuccess) {
        slot->aux[k] = nullptr;
        return nullptr;
    }
    return slot->aux[k];
}

// fork / join of a solve on several streams: the auxiliary streams start after the work already
// queued on s, and s waits for everything queued on them -- also when a part fails after the fork
// (every join is issued)
struct ForkJoin {
    hipStream_t s;
    std::vector<hipStream_t> aux;
    hipEvent_t fork = nullptr;
    std::vector<hipEvent_t> joins;
    hipError_t err = hipSuccess;
    ForkJoin(hipStream_t a, std::vector<hipStream_t> b) : s(a), aux(std::move(b)), joins(aux.size(), nullptr) {
        if ((err = hipEventCreateWithFlags(&fork, hipEventDisableTiming)) != hipSuccess) return;
        for (auto& j : joins)
            if ((err = hipEventCreateWithFlags(&j, hipEventDisableTiming)) != hipSuccess) return;
        if ((err = hipEventRecord(fork, s)) != hipSuccess) return;
        for (hipStream_t x : aux)
            if ((err = hipStreamWaitEvent(x, fork, 0)) != hipSuccess) return;
    }
    hipError_t finish() {
        hipError_t first = hipSuccess;
        for (size_t i = 0; i < aux.size(); ++i) {
            hipError_t e = hipEventRecord(joins[i], aux[i]);
            if (e == hipSuccess) e = hipStreamWaitEvent(s, joins[i], 0);
            if (first == hipSuccess) first = e;
        }
        return first;
    }
    ~ForkJoin() {
        if (fork) (void)hipEventDestroy(fork);
        for (hipEvent_t j : joins)
            if (j) (void)hipEventDestroy(j);
    }
};

// split of P planes into up to ns parts for the generic row kernels, which transform real rows in
// pairs (rows 2c, 2c + 1 of a launch's range): every part but the last must hold an even number of
// rows, or the pairs of the parts after it would shift and the results would differ in the last
// bits from a one-stream solve.  Returns the parts' first planes (one entry: no split).
std::vector<long long> gen_parts(long long P, int H, int ns) {
    long long c = (P + ns - 1) / std::max(ns, 1);
    if (H & 1) c += c & 1;  // an even plane count per part when H is odd
    std::vector<long long> starts;
    for (long long p = 0; p < P; p += std::max(c, 1LL)) starts.push_back(p);
    return starts;
}


// b = H_t(xin) into `bb` through the FFT passes (scratch: spec)
int psf_transpose_into(const admm_tv_desc& d, const Layout& Lo, void* ws, const float* xin, float* bb, cf* spec,
                       int mode, hipStream_t s, bool pl = false) {
    const long long rows = d.B * d.C * d.H;
    const int H = (int)d.H, N = (int)d.W / 2;
    cf* twW = at<cf>(ws, Lo.twW);
    int e = with_row(N, [&](auto ops) { return decltype(ops)::r2c(xin, spec, twW, rows, s); });
    if (e) return e;
    const BankIdx bk = bank_of(d);  // a PSF bank: each plane's own multiplier
    if ((e = pass_b(H, spec, at<float>(ws, Lo.fcT), at<cf>(ws, Lo.mT), at<cf>(ws, Lo.twH), N, (int)(d.B * d.C), mode, s,
                    is_bank(d) ? bank_run(d) : 0, is_bank(d) ? &bk : nullptr)))
        return e;
    return with_row(N, [&](auto ops) { return decltype(ops)::c2r(spec, bb, twW, rows, s, pl); });
}


// ------------------------------------------------------------------ generic sizes (generic_kernels.hpp)
GPlan make_plan_radices(int n);

// Bluestein stages (generic_kernels.hpp gstage_blue): a prime radix R >= ADMM_BLUE_MIN (default
// below) with 2R - 1 <= 1024 runs as a chirp-z transform on the register-resident power-of-two FFT;
// larger primes keep the O(R)-per-output stage.  ADMM_BLUE_MIN <= 0 disables it (A/B).
int blue_min() { return env_int("ADMM_BLUE_MIN", 41); }

constexpr size_t kMaxLds = 160 * 1024;
// LDS bytes of a generic transform kernel: twiddles + tables, two line buffers, Bluestein exchange
// (csz: bytes of a complex element, 16 for the fp64 kernels)
size_t glds(int n, int lines, const GPlan& p, size_t csz = sizeof(cf)) {
    if (p.glb) return 0;  // the line buffers live in global scratch
    return csz * ((p.twg ? 0 : (size_t)n + p.ntab) + 2 * (size_t)n * lines + p.xslots);
}

// long-line blocks (GPlan::glb): scratch slots (resident blocks walking their items grid-stride) and
// the bytes of the scratch region a solve needs for its longer dimension
constexpr long long kGlbSlots = 1024;
constexpr size_t kGlbBudget = 512ull << 20;
long long glb_slots(int n, size_t csz) {
    return std::max<long long>(64, std::min<long long>(kGlbSlots, (long long)(kGlbBudget / (2 * (size_t)n * csz))));
}

// fp64 plan: any prime > 5 first (its stage at NS = 1 needs no twiddle pass), then radices 4, 2, 3, 5
// (the radices the double kernels have butterflies for; no Bluestein stages); twiddles from global
// memory when a line's LDS image would not fit
GPlan make_plan_f64(int n) {
    GPlan p{};
    p.n = n;
    int m = n, r = n;
    auto take_all = [&](int q) {
        while (m % q == 0 && m > 1) {
            p.rad[p.nst++] = q;
            m /= q;
        }
    };
    for (int q : {2, 3, 5})
        while (r % q == 0) r /= q;
    for (int f = 7; f * f <= r; f += 2)
        if (r % f == 0) {
            take_all(f);
            while (r % f == 0) r /= f;
        }
    if (r > 1) take_all(r);
    take_all(4);
    take_all(2);
    take_all(3);
    take_all(5);
    p.twg = glds(n, 1, p, sizeof(double2)) > kMaxLds ? 1 : 0;
    p.glb = (p.twg && glds(n, 1, p, sizeof(double2)) > kMaxLds) ? 1 : 0;
    return p;
}

GPlan make_plan(int n, bool f64) {
    if (f64) return make_plan_f64(n);
    GPlan p = make_plan_radices(n);
    const int bmin = blue_min();
    int M = 0;  // one Bluestein size for the plan: M = 2^k >= 2R - 1 for its largest such prime
    for (int s = 0; s < p.nst; ++s) {
        const int R = p.rad[s];
        if (bmin <= 0 || R <= 7 || (R & (R - 1)) == 0 || R < bmin || 2 * R - 1 > 1024) continue;  // primes only
        int m = 32;
        while (m < 2 * R - 1) m *= 2;
        M = std::max(M, m);
    }
    int off = n;
    for (int s = 0; s < p.nst; ++s) {
        const int R = p.rad[s];
        const bool blue = M > 0 && R > 7 && (R & (R - 1)) != 0 && R >= bmin && 2 * R - 1 <= 1024;
        p.bst[s] = blue ? M : 0;
        p.boff[s] = blue ? off : 0;
        if (blue) off += R + 2 * M;
    }
    p.bm = M;
    p.ntab = off - n;
    p.xslots = M > 0 ? (GNT / (M / blue_e(M))) * (M + M / 8) : 0;
    // one line must fit the LDS: else no Bluestein, else twiddles from global memory, else the
    // line buffers too (a global scratch slot per block)
    if (glds(n, 1, p) <= kMaxLds) return p;
    GPlan q = make_plan_radices(n);
    q.twg = glds(n, 1, q) > kMaxLds ? 1 : 0;
    if (q.twg && glds(n, 1, q) > kMaxLds) q.glb = 1;
    return q;
}

bool gen_fits(int n, bool f64) {
    return n >= 1 && n <= kGenericMax && glds(n, 1, make_plan(n, f64), f64 ? sizeof(double2) : sizeof(cf)) <= kMaxLds;
}
// (as many slots as a launch of that dimension uses: min(slots, its items) -- gen_grid)
size_t glb_scratch(int H, int W, long long P, bool f64) {
    const size_t csz = f64 ? sizeof(double2) : sizeof(cf);
    size_t b = 0;
    if (make_plan(W, f64).glb)  // row transforms: two real rows per item
        b = std::max(b, (size_t)std::min(glb_slots(W, csz), (P * H + 1) / 2) * 2 * (size_t)W * csz);
    if (make_plan(H, f64).glb)  // column pass: one column per item
        b = std::max(b, (size_t)std::min(glb_slots(H, csz), P * (W / 2 + 1)) * 2 * (size_t)H * csz);
    return b;
}

// threads per block of the generic transform kernels (A/B knob; 64, 128 or 256)
int gen_threads(const char* knob) {
    const int v = env_int(knob, GNT);
    return v <= 64 ? 64 : v <= 128 ? 128 : v <= 256 || GNT <= 256 ? 256 : GNT;
}

// long lines without Bluestein stages run their transform blocks with 512 threads (a 1,920-point
// row's stages have 480-960 butterflies; 256 threads leave them latency-bound: HD 1080x1920
// 716 -> 850 it/s; BSD-like lines with Bluestein stages are faster at 256).  ADMM_GEN_WIDE_MIN:
// the line length from which it applies (0: never).
constexpr int kGenWide = 512;
bool gen_wide(int n, const GPlan& p) {
    const int mn = env_int("ADMM_GEN_WIDE_MIN", 1024);
    return p.bm == 0 && mn > 0 && n >= mn;
}

// f(integral_constant BM, bool_constant TWG, bool_constant GLB)
template <class F> int with_plan(const GPlan& p, F&& f) {
    if (p.glb) return f(std::integral_constant<int, 0>{}, std::true_type{}, std::true_type{});
    if (p.twg) return f(std::integral_constant<int, 0>{}, std::true_type{}, std::false_type{});
    return with_bm(p.bm, [&](auto bm) { return f(bm, std::false_type{}, std::false_type{}); });
}

// the kernel instantiation for a plan's Bluestein size
template <class F> int with_bm(int bm, F&& f) {
    // f(integral_constant BM, bool_constant TWG): global-memory twiddles only on plans without Bluestein
    switch (bm) {
        case 0: return f(std::integral_constant<int, 0>{});
        case 32: return f(std::integral_constant<int, 32>{});
        case 64: return f(std::integral_constant<int, 64>{});
        case 128: return f(std::integral_constant<int, 128>{});
        case 256: return f(std::integral_constant<int, 256>{});
        case 512: return f(std::integral_constant<int, 512>{});
        case 1024: return f(std::integral_constant<int, 1024>{});
        default: return fail(ADMM_TV_EUNSUPPORTED, "generic plan: Bluestein size");
    }
}

GPlan make_plan_radices(int n) {
    GPlan p{};
    p.n = n;
    int m = n;
    auto take_all = [&](int r) {
        while (m % r == 0 && m > 1) {
            p.rad[p.nst++] = r;
            m /= r;
        }
    };
    if (env_int("ADMM_GPLAN_PRIME_FIRST", 1)) {
        // any other prime first: at NS = 1 its stage needs no twiddle pass (BSD size: column pass
        // 122 -> 112 ms per 250 launches, 1,410 -> 1,491 it/s)
        // (the primes >= 11 of n by trial division of n stripped of 2, 3, 5, 7: O(sqrt n))
        int r = n;
        // (11 and 13 run as compile-time butterflies like 3, 5, 7: after the powers of two)
        for (int q : {2, 3, 5, 7, 11, 13})
            while (r % q == 0) r /= q;
        for (int f = 11; f * f <= r; f += 2)
            if (r % f == 0) {
                take_all(f);
                while (r % f == 0) r /= f;
            }
        if (r > 1) take_all(r);
        // powers of two as radix-16 / 8 stages (one LDS round trip per 16 / 8 instead of two /
        // three radix-4 / 2 ones); ADMM_GPLAN_R16=0 for the radix-4/2 plan (A/B)
        if (env_int("ADMM_GPLAN_R16", 1)) {
            take_all(16);
            take_all(8);
        }
        take_all(4);
        take_all(2);
        take_all(3);
        take_all(5);
        take_all(7);
        take_all(11);
        take_all(13);
        return p;
    }
    take_all(4);
    take_all(2);
    take_all(3);
    take_all(5);
    take_all(7);
    take_all(11);
    take_all(13);
    for (int f = 17; f * f <= m; f += 2) take_all(f);  // any other prime: O(R) per output
    if (m > 1) take_all(m);
    return p;
}

// complex rows (= 2 real rows each) per block of the row transforms / columns per block of
// the column pass
// (powers of two, so the per-item line index is a shift)
int pow2_floor(int v) { int p = 1; while (2 * p <= v) p *= 2; return p; }
// LDS image <= ~32 KB (4+ resident blocks per CU: the prime-radix stages are latency-bound
// chains and need the waves), except where one line alone is bigger
// (A/B knobs ADMM_GROW_LINES / ADMM_GCOL_COLS: rounded down to a power of two in [1, 32])
// With Bluestein stages the column pass takes at least as many columns as make one item per
// sub-group (16x3x509^2: 2 -> 4 columns, 1,125 -> 1,368 it/s; BSD keeps 4).  Either count is
// halved until the block's LDS fits.
int fit_lines(int n, int lines, const GPlan& p, size_t csz = sizeof(cf)) {
    while (lines > 1 && glds(n, lines, p, csz) > kMaxLds) lines /= 2;
    return lines;
}
int grow_lines(int W, const GPlan& p, size_t csz = sizeof(cf)) {
    if (p.glb) return 1;  // one line per scratch slot
    if (csz != sizeof(cf)) return fit_lines(W, pow2_floor(std::max(1, std::min(32, (2048 / W - 1) / 2))), p, csz);
    const int dflt = pow2_floor(std::max(1, std::min(32, (4096 / W - 1) / 2)));
    return fit_lines(W, pow2_floor(std::max(1, std::min(32, env_int("ADMM_GROW_LINES", dflt)))), p);
}
int gcol_cols(int H, const GPlan& p, size_t csz = sizeof(cf)) {
    if (p.glb) return 1;
    if (csz != sizeof(cf)) return fit_lines(H, pow2_floor(std::max(1, std::min(16, (3072 / H - 1) / 2))), p, csz);
    // column blocks: ~48 KB LDS images without Bluestein stages (VGA 480: 2 -> 4 columns +7 %,
    // 500: +4 %, HD 1080: 1 -> 2 columns +6 %; tools/bench_generic_sizes.py), ~32 KB with them
    int dflt = pow2_floor(std::max(1, std::min(16, ((p.bm > 0 ? 4096 : 6144) / H - 1) / 2)));
    if (p.bm > 0) {
        int nb = H;  // butterflies per line of the Bluestein stages (fewest)
        for (int s = 0; s < p.nst; ++s)
            if (p.bst[s] > 0) nb = std::min(nb, H / p.rad[s]);
        const int nsg = GNT / (p.bm / blue_e(p.bm));
        while (dflt * nb < nsg && dflt < 16) dflt *= 2;
    }
    return fit_lines(H, pow2_floor(std::max(1, std::min(32, env_int("ADMM_GCOL_COLS", dflt)))), p);
}

// matrix-core column pass plan (gcol_mm.hpp).  A/B knobs: ADMM_GCOL_MM=0 keeps the LDS column pass,
// ADMM_GCOL_MM_NL the columns per block (8 or 16)
MMPlan mm_plan(int H, int W) {
    MMPlan m{};
    if (!env_int("ADMM_GCOL_MM", 1) || H < 17) return m;
    int r = H, big = 1;  // largest prime factor of H
    for (int f = 2; f * f <= r; ++f)
        while (r % f == 0) {
            big = std::max(big, f);
            r /= f;
        }
    big = std::max(big, r);
    if (big < 17 || big > 127) return m;
    for (int S = 1; S <= 8; ++S) {
        if (S == 7 || H % S) continue;  // instances: S = 1..6, 8
        const int R = H / S;
        if (R > 127 || !(R & 1) || R % big) continue;
        m.R = R;
        m.S = S;
        break;
    }
    if (!m.R) return m;
    m.h = (m.R - 1) / 2;
    m.KS = (m.h + 1 + 3) / 4;
    m.MT = (m.h + 1 + 15) / 16;
    const int G = m.MT == 3 ? 1 : 4 / m.MT;
    int NL = env_int("ADMM_GCOL_MM_NL", 16) >= 16 ? 16 : 8;
    // n-tiles of 16 real columns: ceil(NL S / 8) of them (the last one padded), at most 8 per wave (the
    // accumulator arrays)
    while (NL > 1 && ((NL * m.S + 7) / 8 + G - 1) / G > 8) NL /= 2;
    if (((NL * m.S + 7) / 8 + G - 1) / G > 8) return m;
    m.NL = NL;
    m.RP = std::max(4 * NL * m.S, 32 * ((NL * m.S + 7) / 8));
    while (m.RP % 64 != 32) m.RP += 16;
    m.lds = (size_t)4 * m.KS * m.RP * sizeof(float) + (size_t)H * sizeof(cf);  // image + twiddles
    m.ok = m.lds <= kMaxLds;
    (void)W;
    return m;
}

// row inverse on the matrix cores: lines (row pairs) per block NL, one (line, k1) item per thread,
// at most 8 n-tiles per wave.  A/B knob: ADMM_GROW_MM=0 keeps the LDS row inverse.
MMPlan mm_plan_row(int W) {
    MMPlan m{};
    if (!env_int("ADMM_GROW_MM", 1) || W < 17) return m;
    int r = W, big = 1;
    for (int f = 2; f * f <= r; ++f)
        while (r % f == 0) {
            big = std::max(big, f);
            r /= f;
        }
    big = std::max(big, r);
    if (big < 17 || big > 127) return m;
    for (int S : {1, 2, 3, 4, 5, 8, 13}) {
        if (W % S) continue;
        const int R = W / S;
        if (R > 127 || !(R & 1) || R % big) continue;
        m.R = R;
        m.S = S;
        break;
    }
    if (!m.R) return m;
    m.h = (m.R - 1) / 2;
    m.KS = (m.h + 1 + 3) / 4;
    m.MT = (m.h + 1 + 15) / 16;
    const int G = m.MT == 3 ? 1 : 4 / m.MT;
    // 256-thread blocks; A/B knob ADMM_GROW_MM_NT=512: 2 G waves per row tile, at most 4 n-tiles per wave
    // (BSD two streams 4,281-4,310 -> 4,130 it/s, profiles/r03_grow_inv_mm_nt.txt)
    m.nth = env_int("ADMM_GROW_MM_NT", 256) == 512 ? 512 : 256;
    const int Gt = m.nth == 512 ? 2 * G : G, maxt = m.nth == 512 ? 4 : 8;
    int NL = 16;
    while (NL > 1 && (NL * (m.h + 1) > m.nth || ((NL * m.S + 7) / 8 + Gt - 1) / Gt > maxt)) NL /= 2;
    if (NL * (m.h + 1) > m.nth || ((NL * m.S + 7) / 8 + Gt - 1) / Gt > maxt) return m;  // one (line, k1) item per thread
    m.NL = NL;
    m.RP = std::max(4 * NL * m.S, 32 * ((NL * m.S + 7) / 8));
    while (m.RP % 64 != 32) m.RP += 16;
    const size_t stage = (size_t)2 * NL * (W / 2 + 1) * 2;  // floats
    m.lds = std::max(stage, (size_t)4 * m.KS * m.RP) * sizeof(float) + (size_t)W * sizeof(cf);
    m.ok = m.lds <= kMaxLds;
    return m;
}


// the launchers below are templated on the real type T of the solve: float, or double for fp64
// inputs (ADMM_TV_FLAG_F64: the generic kernels' double instantiation, plans without Bluestein
// stages, 256-thread blocks)
template <class T> constexpr bool kF64 = std::is_same<T, double>::value;
template <class T> constexpr size_t kCsz = sizeof(cx_t<T>);

// f(integral_constant BM, bool_constant TWG) for a plan: the fp64 kernels exist for BM = 0 only
template <class T, class F> int with_plan_t(const GPlan& p, F&& f) {
    if constexpr (kF64<T>) {
        if (p.bm != 0) return fail(ADMM_TV_EUNSUPPORTED, "fp64 plan with a Bluestein stage");
        if (p.glb) return f(std::integral_constant<int, 0>{}, std::true_type{}, std::true_type{});
        if (p.twg) return f(std::integral_constant<int, 0>{}, std::true_type{}, std::false_type{});
        return f(std::integral_constant<int, 0>{}, std::false_type{}, std::false_type{});
    } else {
        return with_plan(p, f);
    }
}
// grid of a transform launch: one block per item, or (long lines) the scratch slots walking them
inline dim3 gen_grid(long long items, const GPlan& p, size_t csz) {
    return dim3((unsigned)(p.glb ? std::min(items, glb_slots(p.n, csz)) : items));
}

#define GLB_CHECK(pl, gscr)                                                                          \
    if ((pl).glb && !(gscr)) return fail(ADMM_TV_EINVAL, "long lines: no scratch region");
template <class T>
int grow_fwd(const T* img, cx_t<T>* spec, const cx_t<T>* tw, int W, long long rows, hipStream_t s,
             cx_t<T>* gscr = nullptr, int ldw = 0) {
    const GPlan pl = make_plan(W, kF64<T>);
    GLB_CHECK(pl, gscr)
    GRowArgsT<T> a{img, spec, nullptr, tw, pl, rows, grow_lines(W, pl, kCsz<T>), gscr, ldw};
    const size_t lds = glds(W, a.lines, a.plan, kCsz<T>);
    return with_plan_t<T>(a.plan, [&](auto bm, auto twg, auto glb) {
        constexpr int BM = decltype(bm)::value;
        constexpr bool TWG = decltype(twg)::value, GLB = decltype(glb)::value;
        const dim3 grid = gen_grid((rows + 2 * a.lines - 1) / (2 * a.lines), pl, kCsz<T>);
        if constexpr (BM == 0 && !kF64<T> && !GLB) {
            if (gen_wide(W, pl)) {
                if (int e = set_lds(k_grow_fwd<BM, TWG, kGenWide>, lds)) return e;
                hipLaunchKernelGGL((k_grow_fwd<BM, TWG, kGenWide>), grid, dim3(kGenWide), lds, s, a);
                return launch_check("k_grow_fwd");
            }
        }
        if (int e = set_lds(k_grow_fwd<BM, TWG, GNT, T, GLB>, lds)) return e;
        hipLaunchKernelGGL((k_grow_fwd<BM, TWG, GNT, T, GLB>), grid,
                           dim3(kF64<T> || GLB ? GNT : gen_threads("ADMM_GROW_NT")), lds, s, a);
        return launch_check("k_grow_fwd");
    });
}
// the step fused into the row transform of r (k_grow_fwd_step; inference iterations)
// (BOX: with bounds on x, fp32 -- g.v and g.bounds set)
template <bool ISO, bool FIRST, class T, bool BOX = false>
int grow_fwd_step_t(const GStepArgsT<T>& g, cx_t<T>* spec, const cx_t<T>* tw, int W, long long rows, hipStream_t s,
                    cx_t<T>* gscr, int ldw) {
    const GPlan pl = make_plan(W, kF64<T>);
    GLB_CHECK(pl, gscr)
    GRowArgsT<T> a{nullptr, spec, nullptr, tw, pl, rows, grow_lines(W, pl, kCsz<T>), gscr, ldw};
    const size_t lds = glds(W, a.lines, a.plan, kCsz<T>);
    return with_plan_t<T>(a.plan, [&](auto bm, auto twg, auto glb) {
        constexpr int BM = decltype(bm)::value;
        constexpr bool TWG = decltype(twg)::value, GLB = decltype(glb)::value;
        const dim3 grid = gen_grid((rows + 2 * a.lines - 1) / (2 * a.lines), pl, kCsz<T>);
        if constexpr (BM == 0 && !kF64<T> && !GLB) {
            if (gen_wide(W, pl)) {
                if (int e = set_lds(k_grow_fwd_step<BM, TWG, ISO, FIRST, kGenWide, float, false, BOX>, lds)) return e;
                hipLaunchKernelGGL((k_grow_fwd_step<BM, TWG, ISO, FIRST, kGenWide, float, false, BOX>), grid, dim3(kGenWide), lds, s, a, g);
                return launch_check("k_grow_fwd_step");
            }
        }
        if (int e = set_lds(k_grow_fwd_step<BM, TWG, ISO, FIRST, GNT, T, GLB, BOX>, lds)) return e;
        hipLaunchKernelGGL((k_grow_fwd_step<BM, TWG, ISO, FIRST, GNT, T, GLB, BOX>), grid,
                           dim3(kF64<T> || GLB ? GNT : gen_threads("ADMM_GROW_NT")), lds, s, a, g);
        return launch_check("k_grow_fwd_step");
    });
}
template <class T>
int grow_fwd_step(const GStepArgsT<T>& g, cx_t<T>* spec, const cx_t<T>* tw, int W, long long rows, bool iso,
                  bool first, hipStream_t s, cx_t<T>* gscr = nullptr, int ldw = 0) {
    if constexpr (!kF64<T>) {
        if (g.v) {
            if (iso) return first ? grow_fwd_step_t<true, true, T, true>(g, spec, tw, W, rows, s, gscr, ldw)
                                  : grow_fwd_step_t<true, false, T, true>(g, spec, tw, W, rows, s, gscr, ldw);
            return first ? grow_fwd_step_t<false, true, T, true>(g, spec, tw, W, rows, s, gscr, ldw)
                         : grow_fwd_step_t<false, false, T, true>(g, spec, tw, W, rows, s, gscr, ldw);
        }
    }
    if (iso) return first ? grow_fwd_step_t<true, true>(g, spec, tw, W, rows, s, gscr, ldw)
                          : grow_fwd_step_t<true, false>(g, spec, tw, W, rows, s, gscr, ldw);
    return first ? grow_fwd_step_t<false, true>(g, spec, tw, W, rows, s, gscr, ldw)
                 : grow_fwd_step_t<false, false>(g, spec, tw, W, rows, s, gscr, ldw);
}
template <int S> int grow_inv_mm_launch(const GRowInvMMArgs& a, size_t lds, int nth, hipStream_t s) {
    const dim3 grid((unsigned)((a.rows + 2 * a.NL - 1) / (2 * a.NL)));
    if (nth == 512) {
        if (int e = set_lds(k_grow_inv_mm<S, 512>, lds)) return e;
        hipLaunchKernelGGL((k_grow_inv_mm<S, 512>), grid, dim3(512), lds, s, a);
        return launch_check("k_grow_inv_mm");
    }
    if (int e = set_lds(k_grow_inv_mm<S>, lds)) return e;
    hipLaunchKernelGGL(k_grow_inv_mm<S>, grid, dim3(256), lds, s, a);
    return launch_check("k_grow_inv_mm");
}
// mmr: the layout's row-inverse plan (Layout::mmr)
template <class T>
int grow_inv(const cx_t<T>* spec, T* img, const cx_t<T>* tw, int W, long long rows, hipStream_t s,
             cx_t<T>* gscr, const MMPlan& mmr, int ldw = 0) {
    if constexpr (!kF64<T>) {
        const MMPlan m = mmr;
        if (m.ok && rows > 0) {
            const int Wh = W / 2 + 1;
            GRowInvMMArgs a{spec, img, tw, rows, W, m.R, m.h, m.KS, m.MT, m.NL, m.RP, Wh, 2 * m.NL * Wh * 2,
                            ldw ? ldw : Wh};
            switch (m.S) {
                case 1: return grow_inv_mm_launch<1>(a, m.lds, m.nth, s);
                case 2: return grow_inv_mm_launch<2>(a, m.lds, m.nth, s);
                case 3: return grow_inv_mm_launch<3>(a, m.lds, m.nth, s);
                case 4: return grow_inv_mm_launch<4>(a, m.lds, m.nth, s);
                case 5: return grow_inv_mm_launch<5>(a, m.lds, m.nth, s);
                case 8: return grow_inv_mm_launch<8>(a, m.lds, m.nth, s);
                default: return grow_inv_mm_launch<13>(a, m.lds, m.nth, s);
            }
        }
    }
    const GPlan pl = make_plan(W, kF64<T>);
    GLB_CHECK(pl, gscr)
    GRowArgsT<T> a{nullptr, const_cast<cx_t<T>*>(spec), img, tw, pl, rows, grow_lines(W, pl, kCsz<T>), gscr, ldw};
    const size_t lds = glds(W, a.lines, a.plan, kCsz<T>);
    return with_plan_t<T>(a.plan, [&](auto bm, auto twg, auto glb) {
        constexpr int BM = decltype(bm)::value;
        constexpr bool TWG = decltype(twg)::value, GLB = decltype(glb)::value;
        const dim3 grid = gen_grid((rows + 2 * a.lines - 1) / (2 * a.lines), pl, kCsz<T>);
        if constexpr (BM == 0 && !kF64<T> && !GLB) {
            if (gen_wide(W, pl)) {
                if (int e = set_lds(k_grow_inv<BM, TWG, kGenWide>, lds)) return e;
                hipLaunchKernelGGL((k_grow_inv<BM, TWG, kGenWide>), grid, dim3(kGenWide), lds, s, a);
                return launch_check("k_grow_inv");
            }
        }
        if (int e = set_lds(k_grow_inv<BM, TWG, GNT, T, GLB>, lds)) return e;
        hipLaunchKernelGGL((k_grow_inv<BM, TWG, GNT, T, GLB>), grid,
                           dim3(kF64<T> || GLB ? GNT : gen_threads("ADMM_GROW_NT")), lds, s, a);
        return launch_check("k_grow_inv");
    });
}

template <int MODE, int BM, bool TWG, bool GLB, class T>
int gcol_launch(const GColArgsT<T>& a, size_t lds, dim3 grid, hipStream_t s) {
    if constexpr (BM == 0 && !kF64<T> && !GLB) {
        if (gen_wide(a.plan.n, a.plan)) {
            if (int e = set_lds(k_gcol<MODE, BM, TWG, kGenWide>, lds)) return e;
            hipLaunchKernelGGL((k_gcol<MODE, BM, TWG, kGenWide>), grid, dim3(kGenWide), lds, s, a);
            return launch_check("k_gcol");
        }
    }
    if (int e = set_lds(k_gcol<MODE, BM, TWG, GNT, T, GLB>, lds)) return e;
    hipLaunchKernelGGL((k_gcol<MODE, BM, TWG, GNT, T, GLB>), grid,
                       dim3(kF64<T> || GLB ? GNT : gen_threads("ADMM_GCOL_NT")), lds, s, a);
    return launch_check("k_gcol");
}
template <int S> int gcol_mm_launch(const GColMMArgs& a, size_t lds, hipStream_t s) {
    const dim3 grid((unsigned)(a.P * a.colblocks));
    // 512-thread blocks for S <= 4 (NL = 16: at most 8 n-tiles, 2+ waves per row tile -> at most 4 per
    // wave; BSD 4,191-4,230 -> 4,343-4,354 it/s, profiles/r03_gcol_mm_nt.txt); A/B knob ADMM_GCOL_MM_NT
    if constexpr (S <= 4) {
        if (a.NL == 16 && env_int("ADMM_GCOL_MM_NT", 512) == 512) {
            if (int e = set_lds(k_gcol_mm<S, 512>, lds)) return e;
            hipLaunchKernelGGL((k_gcol_mm<S, 512>), grid, dim3(512), lds, s, a);
            return launch_check("k_gcol_mm");
        }
    }
    if (int e = set_lds(k_gcol_mm<S>, lds)) return e;
    hipLaunchKernelGGL(k_gcol_mm<S>, grid, dim3(256), lds, s, a);
    return launch_check("k_gcol_mm");
}
// phase skips of the matrix-core column pass for timing experiments (results invalid): only in a
// library built with -DADMM_MM_DBG_BUILD=1 (tools/build_variant.sh), never from the environment of a
// product build
#ifndef ADMM_MM_DBG_BUILD
#define ADMM_MM_DBG_BUILD 0
#endif
inline int mm_dbg() { return ADMM_MM_DBG_BUILD ? env_int("ADMM_MM_DBG", 0) : 0; }

// mm: the layout's column-pass plan (Layout::mm; its factor copy was sized and written for it)
// the column pass of a PSF bank's planes [p0, p0 + P) (k_gcol_bank: modes 0 and 1, the LDS column pass)
template <int MODE, int BM, bool TWG, bool GLB>
int gcol_bank_launch(const GColBankArgs& a, size_t lds, dim3 grid, hipStream_t s) {
    if constexpr (BM == 0 && !GLB) {
        if (gen_wide(a.plan.n, a.plan)) {
            if (int e = set_lds(k_gcol_bank<MODE, BM, TWG, kGenWide>, lds)) return e;
            hipLaunchKernelGGL((k_gcol_bank<MODE, BM, TWG, kGenWide>), grid, dim3(kGenWide), lds, s, a);
            return launch_check("k_gcol_bank");
        }
    }
    if (int e = set_lds(k_gcol_bank<MODE, BM, TWG, GNT, GLB>, lds)) return e;
    hipLaunchKernelGGL((k_gcol_bank<MODE, BM, TWG, GNT, GLB>), grid, dim3(GLB ? GNT : gen_threads("ADMM_GCOL_NT")), lds, s, a);
    return launch_check("k_gcol_bank");
}

// bank, p0: a PSF bank's table index and the solve's plane that the launch's plane 0 is (fp32; modes 0, 1 and the
// training backward's 2, with or without a dump)
template <class T>
int gcol(cx_t<T>* spec, cx_t<T>* dump, const T* fcT, const cx_t<T>* mT, const cx_t<T>* tw, int H, int W, long long P,
         int mode, hipStream_t s, cx_t<T>* gscr, const MMPlan& mm, int ldw = 0, const BankIdx* bank = nullptr,
         long long p0 = 0) {
    if constexpr (!kF64<T>) {
        if (bank && mode != 3) {  // (mode 3 multiplies by nothing: the plain kernel below)
            if (mm.ok) return fail(ADMM_TV_EUNSUPPORTED, "PSF bank: the LDS column pass only");
            const GPlan pl = make_plan(H, false);
            GLB_CHECK(pl, gscr)
            const int Wh = W / 2 + 1, cols = gcol_cols(H, pl);
            if (ldw && ldw != Wh) return fail(ADMM_TV_EINVAL, "padded spectrum pitch without the matrix-core column pass");
            const int colblocks = (Wh + cols - 1) / cols;
            const GColBankArgs a{{spec, dump, fcT, mT, tw, pl, Wh, cols, colblocks, P, gscr}, *bank, p0};
            const size_t lds = glds(H, cols, pl);
            const dim3 grid = gen_grid(P * colblocks, pl, sizeof(cf));
            return with_plan(pl, [&](auto bm, auto twg, auto glb) {
                constexpr int BM = decltype(bm)::value;
                constexpr bool TWG = decltype(twg)::value, GLB = decltype(glb)::value;
                return mode == 0   ? gcol_bank_launch<0, BM, TWG, GLB>(a, lds, grid, s)
                       : mode == 1 ? gcol_bank_launch<1, BM, TWG, GLB>(a, lds, grid, s)
                                   : gcol_bank_launch<2, BM, TWG, GLB>(a, lds, grid, s);
            });
        }
    }
    if constexpr (!kF64<T>) {
        const MMPlan m = mm;
        if (mode == 0 && m.ok) {  // the factor's [H][Wh] copy follows fcT (setup, k_fc_transpose)
            const int Wh = W / 2 + 1;
            GColMMArgs a{spec, dump, fcT + (size_t)Wh * H, tw, H, m.R, m.h, m.KS, m.MT, m.NL, __builtin_ctz(m.NL), m.RP,
                         Wh, (Wh + m.NL - 1) / m.NL, P, mm_dbg(), ldw ? ldw : Wh};
            switch (m.S) {
                case 1: return gcol_mm_launch<1>(a, m.lds, s);
                case 2: return gcol_mm_launch<2>(a, m.lds, s);
                case 3: return gcol_mm_launch<3>(a, m.lds, s);
                case 4: return gcol_mm_launch<4>(a, m.lds, s);
                case 5: return gcol_mm_launch<5>(a, m.lds, s);
                case 6: return gcol_mm_launch<6>(a, m.lds, s);
                default: return gcol_mm_launch<8>(a, m.lds, s);
            }
        }
    }
    const GPlan pl = make_plan(H, kF64<T>);
    GLB_CHECK(pl, gscr)
    const int Wh = W / 2 + 1, cols = gcol_cols(H, pl, kCsz<T>);
    if (ldw && ldw != Wh) return fail(ADMM_TV_EINVAL, "padded spectrum pitch without the matrix-core column pass");
    const int colblocks = (Wh + cols - 1) / cols;
    GColArgsT<T> a{spec, dump, fcT, mT, tw, pl, Wh, cols, colblocks, P, gscr};
    const size_t lds = glds(H, cols, a.plan, kCsz<T>);
    const dim3 grid = gen_grid(P * colblocks, pl, kCsz<T>);
    return with_plan_t<T>(a.plan, [&](auto bm, auto twg, auto glb) {
        constexpr int BM = decltype(bm)::value;
        constexpr bool TWG = decltype(twg)::value, GLB = decltype(glb)::value;
        switch (mode) {
            case 0: return gcol_launch<0, BM, TWG, GLB>(a, lds, grid, s);
            case 1: return gcol_launch<1, BM, TWG, GLB>(a, lds, grid, s);
            case 2: return gcol_launch<2, BM, TWG, GLB>(a, lds, grid, s);
            default: return gcol_launch<3, BM, TWG, GLB>(a, lds, grid, s);
        }
    });
}
// img_out = real part of the 2-D transform chain  rowFFT -> column pass (mode) -> rowIFFT  of img_in
template <class T>
int gapply(const T* img_in, T* img_out, cx_t<T>* spec, const Layout& Lo, void* ws, const admm_tv_desc& d, int mode,
           hipStream_t s) {
    using C = cx_t<T>;
    const long long P = d.B * d.C, rows = P * d.H;
    const int H = (int)d.H, W = (int)d.W;
    C* twW = at<C>(ws, Lo.twW);
    C* gs = at<C>(ws, Lo.gscr);
    if (int e = grow_fwd(img_in, spec, twW, W, rows, s, gs)) return e;
    const BankIdx bk = bank_of(d);  // a PSF bank: each plane's own multiplier
    if (int e = gcol<T>(spec, nullptr, at<T>(ws, Lo.fcT), at<C>(ws, Lo.mT), at<C>(ws, Lo.twH), H, W, P, mode, s, gs,
                        Lo.mm, 0, is_bank(d) ? &bk : nullptr))
        return e;
    return grow_inv<T>(spec, img_out, twW, W, rows, s, gs, Lo.mmr);
}

template <class T> int gstep(const GStepArgsT<T>& a, bool iso, bool first, bool hist, hipStream_t s) {
    // one block row per image row (P H <= 2^31 - 1 rows), column chunks of 256 pixels
    const long long rows = a.npx / a.W;
    if (rows <= 0) return 0;
    if (rows > 0x7fffffffLL) return fail(ADMM_TV_EUNSUPPORTED, "too many image rows for the generic step kernel");
    const dim3 grid((unsigned)rows, (unsigned)((a.W + 255) / 256)), blk(256);
    const int sel = (iso ? 4 : 0) | (first ? 2 : 0) | (hist ? 1 : 0);
    if constexpr (!kF64<T>) {
        if (a.v) {  // bounds on x (inference: the step outside the row transform, ADMM_GSTEP_FUSE=0)
            if (hist) return fail(ADMM_TV_EINVAL, "k_gstep: bounds on x in a training step");
            switch (sel) {
                case 0: hipLaunchKernelGGL((k_gstep<false, false, false, T, true>), grid, blk, 0, s, a); break;
                case 2: hipLaunchKernelGGL((k_gstep<false, true, false, T, true>), grid, blk, 0, s, a); break;
                case 4: hipLaunchKernelGGL((k_gstep<true, false, false, T, true>), grid, blk, 0, s, a); break;
                default: hipLaunchKernelGGL((k_gstep<true, true, false, T, true>), grid, blk, 0, s, a); break;
            }
            return launch_check("k_gstep<box>");
        }
    }
    switch (sel) {
        case 0: hipLaunchKernelGGL((k_gstep<false, false, false, T>), grid, blk, 0, s, a); break;
        case 1: hipLaunchKernelGGL((k_gstep<false, false, true, T>), grid, blk, 0, s, a); break;
        case 2: hipLaunchKernelGGL((k_gstep<false, true, false, T>), grid, blk, 0, s, a); break;
        case 3: hipLaunchKernelGGL((k_gstep<false, true, true, T>), grid, blk, 0, s, a); break;
        case 4: hipLaunchKernelGGL((k_gstep<true, false, false, T>), grid, blk, 0, s, a); break;
        case 5: hipLaunchKernelGGL((k_gstep<true, false, true, T>), grid, blk, 0, s, a); break;
        case 6: hipLaunchKernelGGL((k_gstep<true, true, false, T>), grid, blk, 0, s, a); break;
        default: hipLaunchKernelGGL((k_gstep<true, true, true, T>), grid, blk, 0, s, a); break;
    }
    return launch_check("k_gstep");
}

template <class T> int gbwd(const GBwdArgsT<T>& a, bool iso, bool lastk, bool firstk, hipStream_t s) {
    const dim3 grid((unsigned)((a.npx + 255) / 256)), blk(256);
    const int sel = (iso ? 4 : 0) | (lastk ? 2 : 0) | (firstk ? 1 : 0);
    switch (sel) {
        case 0: hipLaunchKernelGGL((k_gbwd<false, false, false, T>), grid, blk, 0, s, a); break;
        case 1: hipLaunchKernelGGL((k_gbwd<false, false, true, T>), grid, blk, 0, s, a); break;
        case 2: hipLaunchKernelGGL((k_gbwd<false, true, false, T>), grid, blk, 0, s, a); break;
        case 3: hipLaunchKernelGGL((k_gbwd<false, true, true, T>), grid, blk, 0, s, a); break;
        case 4: hipLaunchKernelGGL((k_gbwd<true, false, false, T>), grid, blk, 0, s, a); break;
        case 5: hipLaunchKernelGGL((k_gbwd<true, false, true, T>), grid, blk, 0, s, a); break;
        case 6: hipLaunchKernelGGL((k_gbwd<true, true, false, T>), grid, blk, 0, s, a); break;
        default: hipLaunchKernelGGL((k_gbwd<true, true, true, T>), grid, blk, 0, s, a); break;
    }
    return launch_check("k_gbwd");
}

// history (training) storage: a_k for k = 1..K (x and y images), iso norms N_k
struct Hist {
    size_t a_slot;     // bytes of one image
    size_t t_slot;     // bytes of one kept spectrum (fused paths: packed row spectra; generic: 2-D half spectra)
    size_t n_slot;     // bytes of one norm pair [2][H][W]
    size_t n_off;      // offset of the norm history
    size_t t_off;      // offset of the r_k spectra (PSF gradient only)
    bool keep_t;
    size_t total;
};
Hist make_hist(const admm_tv_desc& d, const Layout& Lo) {
    Hist h{};
    const size_t rs = is_f64(d) ? sizeof(double) : sizeof(float);
    const size_t G = ngroups_of(d);
    const size_t img = G * d.B * d.C * d.H * d.W * rs;
    h.a_slot = up(img);
    h.n_slot = d.iso ? up(G * 2 * (size_t)d.H * d.W * rs) : 0;
    h.n_off = (size_t)d.maxit * 2 * h.a_slot;
    h.t_off = h.n_off + (size_t)d.maxit * h.n_slot;
    h.keep_t = d.kh > 0 && (d.flags & ADMM_TV_FLAG_PSF_GRAD);
    const bool generic_t = backend_of(d, Lo, 1) == Backend::Generic;
    h.t_slot = generic_t ? up((size_t)d.B * d.C * d.H * (d.W / 2 + 1) * 2 * rs) : h.a_slot;
    h.total = h.t_off + (h.keep_t ? (size_t)d.maxit * h.t_slot : 0);
    return h;
}
// a call's history buffer as typed slots (k >= 1; a backward only reads them)
template <class T> struct HistView {
    Hist h;
    char* base;
    HistView(const admm_tv_desc& d, const Layout& Lo, const void* hist) : h(make_hist(d, Lo)), base(static_cast<char*>(const_cast<void*>(hist))) {}
    T* a(int k, int comp) const {  // a_k image, comp 0 = x, 1 = y
        return reinterpret_cast<T*>(base + (size_t)(2 * (k - 1) + comp) * h.a_slot);
    }
    T* n(int k) const { return reinterpret_cast<T*>(base + h.n_off + (size_t)(k - 1) * h.n_slot); }  // N_k
    // r_k's kept spectrum (PSF gradient: h.keep_t)
    cx_t<T>* r(int k) const { return reinterpret_cast<cx_t<T>*>(base + h.t_off + (size_t)(k - 1) * h.t_slot); }
};


// ------------------------------------------------------------------ solver state in and out (state_kernels.hpp)
// A stateful solve (admm_tv_forward_state): where the iterations start (in: null = the reference's zeros) and
// whether the state after the last one is wanted (out).  One module, no cross-rank hook.
struct StateIO {
    const admm_tv_state* in;
    const admm_tv_state* out;
};

// pixels per thread of the state kernels: 4 (16-byte accesses) where the row length and every pointer allow
int state_vec(int W, std::initializer_list<const void*> ptrs) {
    uintptr_t bits = 0;
    for (const void* p : ptrs) bits |= reinterpret_cast<uintptr_t>(p);
    if (W % 4 == 0 && bits % 16 == 0) return 4;
    if (W % 2 == 0 && bits % 8 == 0) return 2;
    return 1;
}
// block shape: 2^lgtx pixel groups of 256 >> lgtx rows; grid (row blocks, column chunks)
struct StateGrid {
    int lgtx;
    dim3 grid;
    unsigned rowblocks;
};
StateGrid state_grid(long long rows, int W, int V) {
    const int wv = W / V;
    int lg = 0;
    while (lg < 8 && (1 << lg) < wv) ++lg;
    const int ry = 256 >> lg;
    const unsigned rb = (unsigned)((rows + ry - 1) / ry);
    return {lg, dim3(rb, (unsigned)((wv + (1 << lg) - 1) >> lg)), rb};
}
int state_rows_check(const admm_tv_desc& d) {
    if (d.B * d.C * d.H > 0x7fffffffLL)
        return fail(ADMM_TV_EUNSUPPORTED, "admm_tv_forward_state: more than 2^31 - 1 image rows (B C H)");
    return 0;
}

// v = b + rho D^T (z0 - u0) into `v` (pixel order) and u0 into uxo / uyo in the path's layout (L lanes
// lane-paired, 0: pixel order)
int state_import(const admm_tv_desc& d, const admm_tv_state& st, const float* b, float* v, float* uxo, float* uyo,
                 const float* lam, const float* rho, int L, hipStream_t s) {
    ProfScope ps(3, s);
    if (int e = state_rows_check(d)) return e;
    const long long rows = d.B * d.C * d.H;
    const int W = (int)d.W;
    const int V = state_vec(W, {st.zx, st.zy, st.ux, st.uy, b, v, uxo, uyo});
    const StateGrid g = state_grid(rows, W, V);
    const StateImportArgs a{st.zx, st.zy, st.ux, st.uy, b, v, uxo, uyo, lam, rho, (int)d.H, W, L, g.lgtx, (unsigned)rows};
    if (V == 4) hipLaunchKernelGGL(k_state_import<4>, g.grid, dim3(256), 0, s, a);
    else if (V == 2) hipLaunchKernelGGL(k_state_import<2>, g.grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_state_import<1>, g.grid, dim3(256), 0, s, a);
    return launch_check("k_state_import");
}

// z_K, u_K into `st` from x_K (pixel order) and u_{K-1} (uxp / uyp in the path's layout; null: zero); iso: the
// norm over every plane through the layout's part / nsq regions first
int state_export(const admm_tv_desc& d, const Layout& Lo, void* ws, const float* x, const float* uxp, const float* uyp,
                 const admm_tv_state& st, const float* lam, const float* rho, int L, hipStream_t s) {
    if (int e = state_rows_check(d)) return e;
    const long long P = d.B * d.C, rows = P * d.H;
    const int H = (int)d.H, W = (int)d.W;
    float* nsq = d.iso ? at<float>(ws, Lo.nsq) : nullptr;
    float* part = d.iso ? at<float>(ws, Lo.part) : nullptr;
    const int V = state_vec(W, {st.zx, st.zy, st.ux, st.uy, x, uxp, uyp});
    const StateGrid g = state_grid(rows, W, V);
    StateExportArgs a{x, uxp, uyp, st.zx, st.zy, st.ux, st.uy, nsq, part, lam, rho, H, W, L, g.lgtx, (unsigned)rows, Lo.ppg, P};
    if (d.iso) {
        ProfScope ps(2, s);
        const StateGrid gi = state_grid(H, W, V);
        const dim3 grid(gi.rowblocks * (unsigned)Lo.ngroups, gi.grid.y);
        if (V == 4) hipLaunchKernelGGL(k_state_iso_part<4>, grid, dim3(256), 0, s, a, gi.rowblocks);
        else if (V == 2) hipLaunchKernelGGL(k_state_iso_part<2>, grid, dim3(256), 0, s, a, gi.rowblocks);
        else hipLaunchKernelGGL(k_state_iso_part<1>, grid, dim3(256), 0, s, a, gi.rowblocks);
        if (int e = launch_check("k_state_iso_part")) return e;
        const long long n = 2LL * H * W;
        hipLaunchKernelGGL(k_state_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, nsq, Lo.ngroups, n);
        if (int e = launch_check("k_state_reduce")) return e;
    }
    ProfScope ps(3, s);
    if (d.iso) {
        if (V == 4) hipLaunchKernelGGL((k_state_export<4, true>), g.grid, dim3(256), 0, s, a);
        else if (V == 2) hipLaunchKernelGGL((k_state_export<2, true>), g.grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((k_state_export<1, true>), g.grid, dim3(256), 0, s, a);
    } else {
        if (V == 4) hipLaunchKernelGGL((k_state_export<4, false>), g.grid, dim3(256), 0, s, a);
        else if (V == 2) hipLaunchKernelGGL((k_state_export<2, false>), g.grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((k_state_export<1, false>), g.grid, dim3(256), 0, s, a);
    }
    return launch_check("k_state_export");
}


// A solve with bounds on x (admm_tv_forward_box): {lo, hi} on the device and the image of the scaled dual v
// (the workspace's last region).  One module, fp32 inference, no state.
struct BoxIO {
    const float* bounds;
    float* v;
};

// generic-size forward (same contract as run_forward; generic_kernels.hpp)
// odd_rows (Backend::OddRows: fp32 aniso inference, no state): the two-launch iteration on the odd-length row pass
template <class T>
int run_forward_gen(const admm_tv_desc& d, const Layout& Lo, bool odd_rows, const T* xin, const T* lam, const T* rho,
                    T* out, void* ws, void* hist, hipStream_t s, const StateIO* sio = nullptr, const BoxIO* box = nullptr) {
    using C = cx_t<T>;
    const long long P = d.B * d.C;
    const int H = (int)d.H, W = (int)d.W;
    C* twW = at<C>(ws, Lo.twW);
    C* twH = at<C>(ws, Lo.twH);
    T* fcT = at<T>(ws, Lo.fcT);
    C* mT = at<C>(ws, Lo.mT);
    C* spec = at<C>(ws, Lo.spec[0]);
    C* gs = at<C>(ws, Lo.gscr);  // long lines: the transform blocks' scratch slots
    T* ximg = at<T>(ws, Lo.spec[1]);
    T* rimg = at<T>(ws, Lo.rimg);
    T* u[4] = {at<T>(ws, Lo.u[0]), at<T>(ws, Lo.u[1]), at<T>(ws, Lo.u[2]), at<T>(ws, Lo.u[3])};
    const bool train = hist != nullptr;
    const HistView<T> hv(d, Lo, hist);
    const bool keep_t = train && hv.h.keep_t;  // PSF gradient: keep every r_k's 2-D spectrum
    const T* bimg = xin;
    if (d.kh > 0) {  // b = H_t(xin) once
        ProfScope ps(3, s);
        T* bb = at<T>(ws, Lo.b);
        if (int e = gapply(xin, bb, spec, Lo, ws, d, 1, s)) return e;
        bimg = bb;
    }
    // a stateful solve (fp32 inference; fused_forward): r_1 from v = b + rho D^T (z0 - u0) in `out`, u0 the
    // first iteration's u input
    const bool sin = sio && sio->in, sout = sio && sio->out;
    const BankIdx bank = bank_of(d);
    const BankIdx* const bankp = is_bank(d) ? &bank : nullptr;
    const T* r1img = bimg;
    if constexpr (!kF64<T>) {
        if (sin) {
            if (int e = state_import(d, *sio->in, bimg, out, u[0], u[1], lam, rho, 0, s)) return e;
            r1img = out;
        }
    }
    // the iteration loop over planes [p0, p0 + np) on stream st (every plane, or -- aniso inference,
    // whose planes are independent -- one half per stream, ADMM_GEN_STREAMS)
    auto solve_planes = [&](long long p0, long long np, hipStream_t st) -> int {
    // the inference iteration's spectrum pitch (Layout::ldw); training keeps Wh (its history layout)
    const int ld = train ? W / 2 + 1 : Lo.ldw;
    const size_t so = (size_t)p0 * H * ld, io = (size_t)p0 * H * W;  // cf / float offsets
    C* cspec = spec + so;
    T* cx = ximg + io;
    T* crimg = rimg + io;
    T* cout = out + io;
    const T* cb = bimg + io;
    const long long crows = np * H;
    {
        ProfScope ps(3, st);
        if (int e = grow_fwd(r1img + io, cspec, twW, W, crows, st, gs, ld)) return e;  // r_1 = b (or from the state)
    }
    if constexpr (!kF64<T>) {
        if (odd_rows) {
            // the two-launch iteration (odd_kernels.hpp): the column pass in place on spec[cur], then pass A
            // (inverse rows, step, forward rows) from spec[cur] into spec[1 - cur]; u ping-pong as below
            C* sp[2] = {cspec, at<C>(ws, Lo.spec2) + so};
            const int rs = admm_odd::strip_rows(W);
            const int ns = (H + rs - 1) / rs;
            int cur = 0, ui = 0;
            for (int it = 1; it <= d.maxit; ++it) {
                {
                    ProfScope ps(1, st);
                    if (int e = gcol<T>(sp[cur], nullptr, fcT, mT, twH, H, W, np, 0, st, gs, Lo.mm, ld)) return e;
                }
                if (it == d.maxit) {
                    ProfScope ps(3, st);
                    return grow_inv<T>(sp[cur], cout, twW, W, crows, st, gs, Lo.mmr, ld);
                }
                ProfScope ps(0, st);
                OddPassAArgs oa{sp[cur], sp[1 - cur], cb, u[2 * ui] + io, u[2 * ui + 1] + io, u[2 * (1 - ui)] + io,
                                u[2 * (1 - ui) + 1] + io, lam, rho, H, ld, ns, np * ns};
                const hipError_t he = admm_odd::pass_a(W, oa, it == 1, st);
                if (he != hipSuccess) return fail(ADMM_TV_EHIP, std::string("k_pass_a_odd: ") + hipGetErrorString(he));
                cur = 1 - cur;
                ui = 1 - ui;
            }
            return 0;
        }
    }
    int uin = 0;
    for (int it = 1; it <= d.maxit; ++it) {
        const bool last = it == d.maxit;
        {
            ProfScope ps(1, st);
            // (a PSF bank: the table index comes from the solve's plane p0 + p, not the part's)
            if (int e = gcol<T>(cspec, keep_t ? hv.r(it) : nullptr, fcT, mT, twH, H, W, np, 0, st, gs, Lo.mm, ld, bankp, p0))
                return e;
            if (int e = grow_inv<T>(cspec, last ? cout : cx, twW, W, crows, st, gs, Lo.mmr, ld)) return e;
        }
        if (last && !train) break;
        const T* xk = last ? cout : cx;
        const bool first = it == 1 && !sin;
        const T *uxi, *uyi, *nprev = nullptr;
        T *uxo, *uyo;
        if (train) {
            uxi = first ? nullptr : hv.a(it - 1, 0);
            uyi = first ? nullptr : hv.a(it - 1, 1);
            uxo = hv.a(it, 0);
            uyo = hv.a(it, 1);
            if (d.iso && !first) nprev = hv.n(it - 1);
        } else {
            uxi = u[2 * uin] + io;
            uyi = u[2 * uin + 1] + io;
            uxo = u[2 * (1 - uin)] + io;
            uyo = u[2 * (1 - uin) + 1] + io;
        }
        const T* nsq = nullptr;
        if (d.iso) {
            ProfScope ps(2, st);
            T* nout = train ? hv.n(it) : at<T>(ws, Lo.nsq);
            const long long hw = (long long)H * W;
            const dim3 grid((unsigned)((hw + 255) / 256)), blk(256);
            if (first)
                hipLaunchKernelGGL((k_giso_norm<true, false, T>), grid, blk, 0, st, xk, uxi, uyi, nprev, lam, rho, nout, H, W, np);
            else if (train)
                hipLaunchKernelGGL((k_giso_norm<false, true, T>), grid, blk, 0, st, xk, uxi, uyi, nprev, lam, rho, nout, H, W, np);
            else
                hipLaunchKernelGGL((k_giso_norm<false, false, T>), grid, blk, 0, st, xk, uxi, uyi, nprev, lam, rho, nout, H, W, np);
            if (int e = launch_check("k_giso_norm")) return e;
            allreduce(d, reinterpret_cast<float*>(nout), 2ull * H * W, st);
            nsq = nout;
        }
        {
            ProfScope ps(0, st);
            GStepArgsT<T> ga{xk, cb, uxi, uyi, uxo, uyo, last ? nullptr : crimg, nsq, nprev, lam, rho, H, W, np * H * W};
            if constexpr (!kF64<T>) {
                if (box) {  // bounds on x: this part's planes of v (each pixel reads and writes its own)
                    ga.v = box->v + io;
                    ga.bounds = box->bounds;
                }
            }
            // inference: the step runs inside the row transform of r (ADMM_GSTEP_FUSE=0: separate)
            if (!train && !last && env_int("ADMM_GSTEP_FUSE", 1)) {
                if (int e = grow_fwd_step(ga, cspec, twW, W, crows, d.iso != 0, first, st, gs, ld)) return e;
            } else {
                if (int e = gstep(ga, d.iso != 0, first, train, st)) return e;
                if (!last)
                    if (int e = grow_fwd(crimg, cspec, twW, W, crows, st, gs, ld)) return e;
            }
        }
        uin = 1 - uin;
    }
    return 0;
    };
    // plane parts on several streams (the caller's and auxiliary ones, aux_stream): one part's
    // compute-bound column pass overlaps another part's row / step passes (ADMM_GEN_STREAMS parts,
    // default 2: BSD 2,790 -> 3,150 it/s, every generic size measured gains).
    // Not under stream capture: a captured solve stays on the caller's stream.
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIPCHK(hipStreamIsCapturing(s, &cap));
    const int ns = std::max(1, std::min(kMaxAux + 1, env_setting("ADMM_GEN_STREAMS", 2)));
    const std::vector<long long> parts = gen_parts(P, H, ns);
    // (long lines: the parts would share the transform blocks' scratch slots -- one stream)
    const bool glb = make_plan(H, kF64<T>).glb || make_plan(W, kF64<T>).glb;
    if (!d.iso && !train && parts.size() > 1 && !glb && cap == hipStreamCaptureStatusNone) {
        int dev = 0;
        HIPCHK(hipGetDevice(&dev));
        std::vector<hipStream_t> aux;
        for (size_t i = 1; i < parts.size(); ++i) {
            hipStream_t x = aux_stream(s, dev, (int)i - 1);
            if (!x) return fail(ADMM_TV_EHIP, "auxiliary stream");
            aux.push_back(x);
        }
        ForkJoin fj(s, aux);
        if (fj.err != hipSuccess) return fail(ADMM_TV_EHIP, std::string("fork: ") + hipGetErrorString(fj.err));
        int e = 0;
        for (size_t i = 0; i < parts.size() && !e; ++i) {
            const long long p1 = i + 1 < parts.size() ? parts[i + 1] : P;
            e = solve_planes(parts[i], p1 - parts[i], i == 0 ? s : aux[i - 1]);
        }
        const hipError_t je = fj.finish();
        if (e) return e;
        if (je != hipSuccess) return fail(ADMM_TV_EHIP, std::string("join: ") + hipGetErrorString(je));
    } else {
        if (int e = solve_planes(0, P, s)) return e;
    }
    if constexpr (!kF64<T>) {
        if (sout) {  // after K - 1 steps u_{K-1} is in u[2 ((K-1) & 1)] (the imported u0, or none, when K = 1)
            const int ui = (d.maxit - 1) & 1;
            const bool none = d.maxit == 1 && !sin;
            return state_export(d, Lo, ws, out, none ? nullptr : u[2 * ui], none ? nullptr : u[2 * ui + 1], *sio->out, lam,
                                rho, 0, s);
        }
    }
    return 0;
}

// rows per strip of the mixed row pass: the R dividing H that minimises (rounds of blocks over the chip)
// x (R + 1) -- a strip of R rows inverts R + 1 row spectra (one halo row), and the blocks run in rounds
// of (CUs x resident blocks per CU), so a short last round costs a whole one.  HD (1080 rows, 2 blocks of
// 2 strips per CU): R = 15 -> 1,981 it/s against 1,910-1,927 with R = 8, and the model orders R = 8, 10,
// 12, 15, 20, 24 as measured (profiles/r04_ab_hd_r.txt).  A/B knob ADMM_MIXED_R.
// The block slots (CUs x resident pass A blocks) are queried once per (device, N) and cached.
long long mixed_slots(int N) {
    static std::mutex mu;
    static std::vector<std::pair<std::pair<int, int>, long long>> cache;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 512;
    std::lock_guard<std::mutex> lk(mu);
    for (const auto& c : cache)
        if (c.first.first == dev && c.first.second == N) return c.second;
    long long slots = 0;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess)
        slots = (long long)cus * std::max(1, admm_mixed::pass_a_blocks_per_cu(N));
    if (slots <= 0) return 512;  // not cached: a failed query is retried
    cache.push_back({{dev, N}, slots});
    return slots;
}
// slots <= 0: this device's (mixed_slots); the training backward's layout passes a fixed count (its
// workspace size must not depend on the device)
int strip_rows_mixed(int H, long long rows, int N, long long slots = 0) {
    if (const int e = env_int("ADMM_MIXED_R", 0); e > 0 && H % e == 0) return e;
    const int sg = 256 / std::max(1, admm_mixed::row_lanes(N));  // strips per block
    if (slots <= 0) slots = mixed_slots(N);
    int best = 1;
    double best_t = 1e300;
    for (int R = 1; R <= 32 && R <= H; ++R) {
        if (H % R) continue;
        const long long strips = rows / R;
        const long long blocks = (strips + sg - 1) / sg;
        const double t = (double)((blocks + slots - 1) / slots) * (R + 1);
        if (t < best_t - 1e-9 || (t < best_t + 1e-9 && R > best)) {
            best_t = t;
            best = R;
        }
    }
    return best;
}

// ------------------------------------------------------------------ the fused two-pass solvers
// Power-of-two sizes and smooth sizes (mixed_hw) run one iteration sequence, fused_forward and
// fused_backward below, each on the backend that launches its kernels: Pow2Ops (RowOps<N>, pass_b) or
// MixedOps (admm_mixed::*, inside the generic layout's regions).  Whatever differs between the two paths
// is a backend method or constant (DESIGN.md §7e lists them); every operation returns the library's
// error code.
struct FusedOps {  // what both backends launch with: the call's descriptor, layout, workspace and tables
    const admm_tv_desc& d;
    const Layout& Lo;
    void* const ws;
    const int H, N;
    cf *const twW, *const twH;
    FusedOps(const admm_tv_desc& d_, const Layout& L, void* w)
        : d(d_), Lo(L), ws(w), H((int)d_.H), N((int)d_.W / 2), twW(at<cf>(w, L.twW)), twH(at<cf>(w, L.twH)) {}
};

struct Pow2Ops : FusedOps {
    static constexpr bool kPsfGrad = true;  // trains with a PSF gradient: r_k's row spectra in the history
    float* const fcT;
    cf* const mT;
    const bool coop;  // A/B knob of the cooperative row pass (RowOps::pass_a): 0 = the plain kernel
    const int rev;
    const bool pf;  // A/B knob of the cooperative row pass's pipelined loads: 0 = the kernel without them
    Pow2Ops(const admm_tv_desc& d_, const Layout& L, void* w)
        : FusedOps(d_, L, w), fcT(at<float>(w, L.fcT)), mT(at<cf>(w, L.mT)),
          coop(env_int("ADMM_PASSA_COOP", 1) != 0), rev(env_int("ADMM_PASSA_REV", 0)),
          pf(env_int("ADMM_PASSA_PF", 1) != 0) {}
    // every module's planes go through each launch (module = plane / planes per module)
    int modules_per_pass(int G) const { return G; }
    // The inference path keeps its internal images (u, b, iso norm maps) in the lane-paired row
    // layout (16-byte accesses, admm_kernels.hpp ld_row); the training history stays in pixel order.
    // ADMM_PL=0 for the pixel-order layout (A/B).
    // Default on for iso (C3 iso 507-514 -> 533-544 it/s) and rows up to 512 (C2 +1 %), off for aniso
    // rows of 1,024+ where the pixel-order streams measured faster (C3 pass A 1.0355 -> 1.0295 ms, 4
    // interleaved rounds, profiles/r03_sweep_knobs_c3.txt).
    bool lane_paired(bool train) const { return !train && env_int("ADMM_PL", (d.iso || d.W < 1024) ? 1 : 0) != 0; }
    // lanes per row of the lane-paired layout (the state kernels address u and b through it)
    int row_lanes() const {
        int L = 0;
        with_row(N, [&](auto ops) { return L = decltype(ops)::G::L; });
        return L;
    }
    // (plain: the row pass runs the plain kernel whatever the knobs say -- a solve with bounds on x)
    int strip(long long rows, bool aniso_fwd, bool plain = false) const {
        return strip_rows(H, N, rows, aniso_fwd, coop && !rev && !plain);
    }
    int r2c(const float* img, cf* spec, long long rows, hipStream_t s, bool pl = false) const {
        return with_row(N, [&](auto ops) { return decltype(ops)::r2c(img, spec, twW, rows, s, pl); });
    }
    int c2r(const cf* spec, float* img, long long rows, hipStream_t s) const {
        return with_row(N, [&](auto ops) { return decltype(ops)::c2r(spec, img, twW, rows, s); });
    }
    // column pass of np planes, ppm per module, from `in` into `out` (the same buffer, or -- PSF-gradient
    // training -- r_k's kept spectra); the modules' Wiener factors follow one another from fcT (g0 == 0)
    // (a PSF bank, one module: each plane's table instead, the kernels' BankIdx instances)
    int col(const cf* in, cf* out, long long np, long long ppm, int /*g0*/, hipStream_t s) const {
        if (is_bank(d)) {
            const BankIdx bk = bank_of(d);
            return pass_b_oop(H, in, out, fcT, mT, twH, N, (int)np, 0, s, bank_run(d), &bk);
        }
        return pass_b_oop(H, in, out, fcT, mT, twH, N, (int)np, 0, s, (int)ppm);
    }
    // cross-spectrum partials for the PSF gradient (weighted: the A terms, which k_xspec_reduce weights by
    // fcT^2 -- fcT is stored / (2HW) here, so no factor is due)
    // (xb: a PSF bank's gradient, the plane groups per table)
    int xspec(const cf* U, const cf* V, cf* part, long long P, int ppg, bool /*weighted*/, hipStream_t s,
              const XBank* xb = nullptr) const {
        return ::xspec(H, U, V, part, twH, N, (int)P, ppg, s, xb, xb ? bank_of(d).T : 0);  // the free launcher above
    }
    int iso_norm(const IsoArgs& a, bool first, bool hist, hipStream_t s, bool pl) const {
        return with_row(N, [&](auto ops) { return decltype(ops)::iso_norm(a, first, hist, s, pl); });
    }
    int pass_a(const PassAArgs& a, bool iso, bool first, bool hist, hipStream_t s, bool pl) const {
        return with_row(N, [&](auto ops) { return decltype(ops)::pass_a(a, iso, first, hist, s, pl, coop, pf); });
    }
    int bwd_iso_q(const BwdIsoArgs& a, bool lastk, hipStream_t s) const {
        return with_row(N, [&](auto ops) { return decltype(ops)::bwd_iso_q(a, lastk, s); });
    }
    int bwd_pass_a(const BwdArgs& a, bool iso, bool lastk, bool firstk, hipStream_t s) const {
        return with_row(N, [&](auto ops) { return decltype(ops)::bwd_pass_a(a, iso, lastk, firstk, s); });
    }
    // b = H_t(xin) through the FFT passes; without a PSF (pl only) b = xin, re-laid out
    int make_b(const float* xin, float* bb, cf* spec, bool pl, hipStream_t s) const {
        if (d.kh > 0) return psf_transpose_into(d, Lo, ws, xin, bb, spec, 1, s, pl);
        return with_row(N, [&](auto ops) { return decltype(ops)::pair(xin, bb, d.B * d.C * H, s); });
    }
    // x^_in = H_t^T b^ : the conjugate multiplier (pass B mode 2)
    int apply_ht_t(const float* bbar, float* gxin, cf* spec, hipStream_t s) const {
        return psf_transpose_into(d, Lo, ws, bbar, gxin, spec, 2, s);
    }
};

struct MixedOps : FusedOps {
    static constexpr bool kPsfGrad = true;  // trains with a PSF gradient: r_k's row spectra in the history
    const float* const fcM;
    static constexpr int rev = 0;  // no ADMM_PASSA_REV here
    MixedOps(const admm_tv_desc& d_, const Layout& L, void* w) : FusedOps(d_, L, w), fcM(at<float>(w, L.fcM)) {}
    // grouped modules (desc.groups, inference only): one module after another through the iterations, each
    // with its own Wiener factor, lambda, rho and (iso) norm, sharing b, the tables and the regions
    int modules_per_pass(int) const { return 1; }
    bool lane_paired(bool) const { return false; }  // pixel order throughout
    int row_lanes() const { return 0; }
    int strip(long long rows, bool, bool = false) const { return strip_rows_mixed(H, rows, N); }
    int r2c(const float* img, cf* spec, long long rows, hipStream_t s, bool = false) const {
        return hip_code(admm_mixed::r2c(N, img, spec, twW, rows, s), "k_row_r2c_m");
    }
    int c2r(const cf* spec, float* img, long long rows, hipStream_t s) const {
        return hip_code(admm_mixed::c2r(N, spec, img, twW, rows, s), "k_row_c2r_m");
    }
    // one module's planes with module g0's factor, from `in` into `out` (the same buffer, or -- PSF-gradient
    // training -- r_k's kept spectra)
    // (a PSF bank, one module: one launch over all planes, each with its table)
    int col(const cf* in, cf* out, long long np, long long, int g0, hipStream_t s) const {
        if (is_bank(d)) {
            const BankIdx bk = bank_of(d);
            return hip_code(admm_mixed::pass_b(H, in, out, fcM, twH, N, np, s, &bk), "k_pass_b_m<bank>");
        }
        return hip_code(admm_mixed::pass_b(H, in, out, fcM + (size_t)g0 * (2 * N + 1) * H, twH, N, np, s), "k_pass_b_m");
    }
    // Cross spectra of two sets of packed row spectra.  They carry the packed transforms' factor 2 each, as on
    // the power-of-two path, so conj(U) V is 4 times the plain product.  For Z that is k_psf_grad's zscale
    // 0.25, on both paths.  For A, k_xspec_reduce weights by fcT^2, and fcT at a smooth size holds the generic
    // scale fc / (HW), not the power-of-two path's fc / (2HW) (spectra_scale; k_fc_mixed halves it into fcM,
    // which is laid out [ky][kx] and so cannot be fed to the reduce): the missing (1/2)^2 goes on the
    // partials instead, the kernel's scale 0.25 (a power of two: exact), so that A = fc^2 Re(conj(X^) R) /
    // (HW)^2 and A_true = (HW)^2 A holds as k_psf_grad expects.
    int xspec(const cf* U, const cf* V, cf* part, long long P, int ppg, bool weighted, hipStream_t s,
              const XBank* xb = nullptr) const {
        return hip_code(admm_mixed::xspec(H, U, V, part, twH, N, P, ppg, weighted ? 0.25f : 1.f, s, xb,
                                          xb ? bank_of(d).T : 0),
                        "k_xspec_m");
    }
    int iso_norm(const IsoArgs& a, bool first, bool hist, hipStream_t s, bool) const {
        return hip_code(admm_mixed::iso_norm(N, a, first, hist, s), "k_iso_norm_m");
    }
    int pass_a(const PassAArgs& a, bool iso, bool first, bool hist, hipStream_t s, bool) const {
        return hip_code(admm_mixed::pass_a(N, a, iso, first, hist, s), "k_pass_a_m");
    }
    int bwd_iso_q(const BwdIsoArgs& a, bool lastk, hipStream_t s) const {
        return hip_code(admm_mixed::bwd_iso_q(N, a, lastk, s), "k_bwd_iso_q_m");
    }
    int bwd_pass_a(const BwdArgs& a, bool iso, bool lastk, bool firstk, hipStream_t s) const {
        return hip_code(admm_mixed::bwd_pass_a(N, a, iso, lastk, firstk, s), "k_bwd_pass_a_m");
    }
    // b = H_t(xin) into the generic b region on the mixed transforms: row r2c, the column pass with the PSF
    // multiplier, row c2r (HD: three fast launches in place of the generic transforms' ~1 ms); A/B knob
    // ADMM_MIXED_BGEN=1: the generic transforms (half spectra as scratch)
    int make_b(const float* xin, float* bb, cf* spec, bool, hipStream_t s) const {
        const long long P = d.B * d.C;
        if (env_int("ADMM_MIXED_BGEN", 0)) return gapply<float>(xin, bb, spec, Lo, ws, d, 1, s);
        if (int e = r2c(xin, spec, P * H, s)) return e;
        const BankIdx bk = bank_of(d);
        if (int e = hip_code(admm_mixed::pass_b_cm(H, spec, at<cf>(ws, Lo.mM), twH, N, P, s, is_bank(d) ? &bk : nullptr),
                             "k_pass_b_m<cm>"))
            return e;
        return c2r(spec, bb, P * H, s);
    }
    // x^_in = H_t^T b^ (the conjugate multiplier, generic transforms)
    int apply_ht_t(const float* bbar, float* gxin, cf* spec, hipStream_t s) const {
        return gapply<float>(bbar, gxin, spec, Lo, ws, d, 2, s);
    }
};

// The forward solve on a fused backend: b = H_t(xin) once (the reference recomputes it every iteration,
// deconv.py:104), then the modules' iterations, modules_per_pass of them at a time.  Per pass over modules
// [g0, g0 + ng): r_1 = rowFFT(b) for each, then per iteration the column pass (column FFT, Wiener factor,
// column IFFT), [iso: the norm pass, its reduce per module and the cross-rank hook], the row pass; the last
// iteration ends in the output transform.  spec[0] / spec[1] hold the packed row spectra ping-pong, u[0..3]
// the u images.
// hist == nullptr: inference (u ping-pong).  Otherwise training: a_k -> hist slot k-1 (x image at 2(k-1),
// y image at 2(k-1)+1), N_k -> norm slot k-1, and the last iteration's row pass also runs (a_K is needed
// by the backward); with a PSF gradient (Hist::keep_t) every r_k's row spectra are kept too, so r_1 goes
// to the history, the column pass reads r_k from there and the row pass writes r_{k+1} there.
// sio (inference, one module): a stateful solve.  With sio->in, r_1 is the row transform of v = b + rho D^T (z0 -
// u0), which the import kernel leaves in `out`, u0 is the first iteration's u input and that iteration runs
// the steady kernels; with sio->out the row pass of iteration K - 1 keeps its u stores and the export kernel
// follows the output transform.  sio == nullptr launches exactly what it always did.
// (measured and removed: plane chunks kept resident in the Infinity Cache through all iterations, and
// two plane halves on two streams -- DESIGN.md §9; both no faster at C3)
template <class B>
int fused_forward(const B& be, const float* xin, const float* lam, const float* rho, float* out, void* hist,
                  hipStream_t s, const StateIO* sio = nullptr, const BoxIO* box = nullptr) {
    const admm_tv_desc& d = be.d;
    const Layout& Lo = be.Lo;
    void* ws = be.ws;
    const int H = be.H, N = be.N, W = (int)d.W, G = ngroups_of(d);
    const long long Pm = d.B * d.C;  // planes of one module
    cf* spec[2] = {at<cf>(ws, Lo.spec[0]), at<cf>(ws, Lo.spec[1])};
    float* u[4] = {at<float>(ws, Lo.u[0]), at<float>(ws, Lo.u[1]), at<float>(ws, Lo.u[2]), at<float>(ws, Lo.u[3])};
    const bool train = hist != nullptr;
    const HistView<float> hv(d, Lo, hist);
    const bool keep_t = B::kPsfGrad && train && hv.h.keep_t;
    const bool pl = be.lane_paired(train);
    const float* bimg = xin;
    if (d.kh > 0 || pl) {
        ProfScope ps(3, s);
        float* bb = at<float>(ws, Lo.b);
        if (int e = be.make_b(xin, bb, spec[0], pl, s)) return e;
        bimg = bb;
    }
    const int ng = be.modules_per_pass(G);
    const long long np = ng * Pm, rows = np * H;  // planes and rows of a pass
    const int gpm = Lo.ngroups / G;               // iso plane groups per module (a group never straddles two)
    const int R = be.strip(rows, !d.iso && !train, box != nullptr);
    const bool sin = sio && sio->in, sout = sio && sio->out;
    const int sl = pl ? be.row_lanes() : 0;  // the state kernels' view of the u / b layout
    for (int g0 = 0; g0 < G; g0 += ng) {
        const float* lamg = lam + g0;
        const float* rhog = rho + g0;
        float* outg = out + (size_t)g0 * Pm * H * W;
        for (int g = 0; g < ng; ++g) {  // r_1 = b for every module of the pass (the one before overwrote it)
            ProfScope ps(3, s);
            cf* t0 = (keep_t ? hv.r(1) : spec[0]) + (size_t)g * Pm * H * N;
            if (sin) {  // r_1 from the state: v in `out` (free until the output transform), u0 into u[0], u[1]
                if (int e = state_import(d, *sio->in, bimg, outg, u[0], u[1], lamg, rhog, sl, s)) return e;
                if (int e = be.r2c(outg, t0, Pm * H, s, false)) return e;
                continue;
            }
            if (int e = be.r2c(bimg, t0, Pm * H, s, pl)) return e;
        }
        int cur = 0, uin = 0;  // spec[cur] holds the current r spectra; u[2*uin], u[2*uin+1] = u_x, u_y in
        for (int it = 1; it <= d.maxit; ++it) {
            {
                ProfScope ps(1, s);
                if (int e = be.col(keep_t ? hv.r(it) : spec[cur], spec[cur], np, Pm, g0, s)) return e;
            }
            if (it == d.maxit) {
                ProfScope ps(3, s);
                if (int e = be.c2r(spec[cur], outg, rows, s)) return e;
                if (sout) {  // u[2 uin], u[2 uin + 1]: u_{K-1} -- iteration K - 1's, the imported u0, or none
                    const bool none = d.maxit == 1 && !sin;
                    if (int e = state_export(d, Lo, ws, outg, none ? nullptr : u[2 * uin], none ? nullptr : u[2 * uin + 1],
                                             *sio->out, lamg, rhog, sl, s))
                        return e;
                }
                if (!train) break;
            }
            const bool first = (it == 1) && !sin;
            const float *uxi, *uyi, *nprev = nullptr;
            float *uxo, *uyo;
            if (train) {  // a_{k-1} in, a_k out (u is rebuilt from a in the kernels)
                uxi = first ? nullptr : hv.a(it - 1, 0);
                uyi = first ? nullptr : hv.a(it - 1, 1);
                uxo = hv.a(it, 0);
                uyo = hv.a(it, 1);
                if (d.iso && !first) nprev = hv.n(it - 1);
            } else {
                uxi = u[2 * uin];
                uyi = u[2 * uin + 1];
                uxo = u[2 * (1 - uin)];
                uyo = u[2 * (1 - uin) + 1];
                // the last row pass of the solve: only its r spectra are used (the last column pass and
                // the output transform follow), so it writes no u (k_pass_a: a null output)
                // (kept when the state is wanted: the export forms a_K from this u)
                if (it == d.maxit - 1 && !sout) uxo = uyo = nullptr;
            }
            const float* nsq = nullptr;
            if (d.iso) {
                ProfScope ps(2, s);
                float* nout = train ? hv.n(it) : at<float>(ws, Lo.nsq);
                IsoArgs ia{spec[cur], uxi, uyi, nprev, lamg, rhog, at<float>(ws, Lo.part), be.twW, (int)np, H, Lo.ppg,
                           (long long)ng * gpm * H, Pm};
                if (int e = be.iso_norm(ia, first, train, s, pl)) return e;
                const long long n4 = 2LL * H * W / 4;
                for (int g = 0; g < ng; ++g) {  // each module's norm over its own planes
                    hipLaunchKernelGGL(k_iso_reduce, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s,
                                       at<float4>(ws, Lo.part) + (size_t)g * gpm * n4,  // n4 float4 = 2HW floats
                                       reinterpret_cast<float4*>(nout) + (size_t)g * n4, gpm, n4);
                    if (int e = launch_check("k_iso_reduce")) return e;
                }
                // sharded batch: the per-pixel sums must cover every rank's planes
                allreduce(d, nout, (size_t)ng * 2 * H * W, s);
                nsq = nout;
            }
            {
                ProfScope ps(0, s);
                cf* tout = (keep_t && it < d.maxit) ? hv.r(it + 1) : spec[1 - cur];
                PassAArgs pa{spec[cur], tout, bimg, uxi, uyi, uxo, uyo, nsq, nprev, lamg, rhog, be.twW, H, R, rows / R, Pm,
                             be.rev};
                if (box) {  // bounds on x (Pow2Ops: the row pass's BOX instantiation)
                    pa.v = box->v;
                    pa.bounds = box->bounds;
                }
                if (int e = be.pass_a(pa, d.iso != 0, first, train, s, pl)) return e;
            }
            cur = 1 - cur;
            uin = 1 - uin;
        }
    }
    return 0;
}

// The forward solver.  hist == nullptr: inference; otherwise training mode, the iterates kept in the
// history (fused_forward, run_forward_gen).
int run_forward(const admm_tv_desc& d, const float* xin, const float* kern, const float* lam, const float* rho,
                float* out, void* ws, size_t ws_bytes, void* hist, hipStream_t s) {
    const Layout Lo = make_layout(d);
    if (int e = check_workspace(ws, ws_bytes, Lo.total)) return e;
    const Backend be = backend_of(d, Lo, hist ? 1 : 0);
    if (be == Backend::OddRowsT && d.maxit > 0) {  // the transposed odd-length solve (odd_t_hw)
        const long long P = d.B * d.C;
        const int H = (int)d.H, W = (int)d.W;
        float* xT = at<float>(ws, Lo.xT);
        float* oT = at<float>(ws, Lo.oT);
        float* kT = d.kh > 0 ? at<float>(ws, Lo.kT) : nullptr;
        {
            ProfScope ps(3, s);
            hipError_t e = admm_odd::transpose(xin, xT, H, W, P, s);
            if (e == hipSuccess && kT) e = admm_odd::transpose(kern, kT, d.kh, d.kw, 1, s);
            if (e != hipSuccess) return fail(ADMM_TV_EHIP, std::string("k_transpose: ") + hipGetErrorString(e));
        }
        const admm_tv_desc dT = transposed(d);
        if (int e = run_forward(dT, xT, kT, lam, rho, oT, at<char>(ws, Lo.tws), ws_bytes - Lo.tws, nullptr, s)) return e;
        ProfScope ps(3, s);
        const hipError_t e = admm_odd::transpose(oT, out, W, H, P, s);
        return e == hipSuccess ? 0 : fail(ADMM_TV_EHIP, std::string("k_transpose: ") + hipGetErrorString(e));
    }
    const int G = ngroups_of(d);
    const long long Pm = d.B * d.C, P = G * Pm;  // planes of one module, of all modules
    const int H = (int)d.H, W = (int)d.W;
    const size_t img_bytes = (size_t)P * H * W * sizeof(float);
    if (d.maxit == 0) {
        if (img_bytes) HIPCHK(hipMemsetAsync(out, 0, img_bytes, s));  // the reference returns x = zeros (deconv.py:61,117)
        return 0;
    }
    if (participate_only(d)) {  // the same reductions as the solve's iso loop, contributing zeros
        // (grouped modules at a smooth size: one module's iterations after another, 2HW per reduction)
        const bool by_module = Lo.gen && G > 1;
        const size_t n = (Lo.gen ? 1 : (size_t)G) * 2 * H * W;
        for (int g = 0; g < (by_module ? G : 1); ++g)
            for (int it = 1; it <= d.maxit; ++it) {
                if (it == d.maxit && !hist) break;
                HIPCHK(hipMemsetAsync(at<float>(ws, Lo.nsq), 0, n * sizeof(float), s));
                allreduce(d, at<float>(ws, Lo.nsq), n, s);
            }
        return 0;
    }
    if (int e = setup(d, Lo, ws, kern, rho, s)) return e;
    switch (be) {
        case Backend::Pow2: return fused_forward(Pow2Ops(d, Lo, ws), xin, lam, rho, out, hist, s);
        case Backend::Mixed: return fused_forward(MixedOps(d, Lo, ws), xin, lam, rho, out, hist, s);
        case Backend::Generic: return run_forward_gen(d, Lo, false, xin, lam, rho, out, ws, hist, s);
        case Backend::OddRows: return run_forward_gen(d, Lo, true, xin, lam, rho, out, ws, hist, s);
        case Backend::OddRowsT: break;  // (returned above)
    }
    return fail(ADMM_TV_EINVAL, "run_forward: no backend");
}

// what a stateful solve refuses (admm_tv_forward_state, admm_tv_state_workspace_size, admm_tv_path(desc, 2))
int state_check(const admm_tv_desc& d) {
    if (d.flags & (ADMM_TV_FLAG_F64 | ADMM_TV_FLAG_PSF_GRAD | ADMM_TV_FLAG_PSF_BANK_TRAIN))
        return fail(ADMM_TV_EINVAL, "admm_tv_forward_state: fp32 inference only (ADMM_TV_FLAG_F64 / ADMM_TV_FLAG_PSF_GRAD / "
                                    "ADMM_TV_FLAG_PSF_BANK_TRAIN set)");
    if (d.groups > 1) return fail(ADMM_TV_EUNSUPPORTED, "admm_tv_forward_state: groups > 1 (one stateful solve per module)");
    if (d.allreduce) return fail(ADMM_TV_EUNSUPPORTED, "admm_tv_forward_state: no cross-rank all-reduce hook");
    // the state kernels run one block row per image row (as the generic step kernel does): B C H < 2^31.  Checked
    // here, so that the size and path queries answer as the call does.
    return state_rows_check(d);
}

// The stateful forward solver (admm_tv_forward_state's contract, its descriptor already validated): the
// iterations of run_forward's inference solve, started from st.in and followed by the export of st.out.
int run_forward_state(const admm_tv_desc& d, const float* xin, const float* kern, const float* lam, const float* rho,
                      const StateIO& st, float* out, void* ws, size_t ws_bytes, hipStream_t s) {
    const Layout Lo = make_layout(d);
    if (int e = check_workspace(ws, ws_bytes, Lo.total)) return e;
    const size_t img_bytes = (size_t)d.B * d.C * d.H * d.W * sizeof(float);
    if (d.maxit == 0) {  // x = zeros (deconv.py:61,117); the state passes through
        if (img_bytes) HIPCHK(hipMemsetAsync(out, 0, img_bytes, s));
        if (st.out && img_bytes) {
            float* const dst[4] = {st.out->zx, st.out->zy, st.out->ux, st.out->uy};
            const float* const src[4] = {st.in ? st.in->zx : nullptr, st.in ? st.in->zy : nullptr,
                                         st.in ? st.in->ux : nullptr, st.in ? st.in->uy : nullptr};
            for (int i = 0; i < 4; ++i) {
                if (!st.in) HIPCHK(hipMemsetAsync(dst[i], 0, img_bytes, s));
                else if (dst[i] != src[i]) HIPCHK(hipMemcpyAsync(dst[i], src[i], img_bytes, hipMemcpyDeviceToDevice, s));
            }
        }
        return 0;
    }
    if (int e = setup(d, Lo, ws, kern, rho, s)) return e;
    switch (backend_of(d, Lo, 2)) {
        case Backend::Pow2: return fused_forward(Pow2Ops(d, Lo, ws), xin, lam, rho, out, nullptr, s, &st);
        case Backend::Mixed: return fused_forward(MixedOps(d, Lo, ws), xin, lam, rho, out, nullptr, s, &st);
        case Backend::Generic: return run_forward_gen<float>(d, Lo, false, xin, lam, rho, out, ws, nullptr, s, &st);
        case Backend::OddRows:
        case Backend::OddRowsT: break;  // (the odd-length row pass carries no state: never answered for mode 2)
    }
    return fail(ADMM_TV_EINVAL, "run_forward_state: no backend");
}

// what a solve with bounds on x refuses (admm_tv_forward_box, admm_tv_box_workspace_size, admm_tv_path(desc, 3))
int box_check(const admm_tv_desc& d) {
    if (d.flags & (ADMM_TV_FLAG_F64 | ADMM_TV_FLAG_PSF_GRAD | ADMM_TV_FLAG_PSF_BANK_TRAIN))
        return fail(ADMM_TV_EINVAL, "admm_tv_forward_box: fp32 inference only (ADMM_TV_FLAG_F64 / ADMM_TV_FLAG_PSF_GRAD / "
                                    "ADMM_TV_FLAG_PSF_BANK_TRAIN set)");
    if (is_bank(d)) return fail(ADMM_TV_EUNSUPPORTED, "admm_tv_forward_box: no PSF bank (ADMM_TV_FLAG_PSF_PER_IMAGE / _PER_CHANNEL)");
    if (d.groups > 1) return fail(ADMM_TV_EUNSUPPORTED, "admm_tv_forward_box: groups > 1 (one solve with bounds per module)");
    if (d.allreduce) return fail(ADMM_TV_EUNSUPPORTED, "admm_tv_forward_box: no cross-rank all-reduce hook");
    // the generic step kernel runs one block row per image row: B C H < 2^31 at the sizes it serves
    if (!supported_hw(d.H, d.W) && d.B * d.C * d.H > 0x7fffffffLL)
        return fail(ADMM_TV_EUNSUPPORTED, "admm_tv_forward_box: more than 2^31 - 1 image rows (B C H) on the generic kernels");
    return 0;
}

// the workspace of a solve with bounds on x: the forward's regions, then the image of v
size_t box_v_offset(const Layout& Lo) { return up(Lo.total); }
size_t box_total(const admm_tv_desc& d, const Layout& Lo) {
    return box_v_offset(Lo) + up((size_t)d.B * d.C * d.H * d.W * sizeof(float));
}

// The solver with bounds on x (admm_tv_forward_box's contract, its descriptor already validated): run_forward's
// inference iterations with the Wiener factor of the split w = x and the projection in the row pass / the step.
int run_forward_box(const admm_tv_desc& d, const float* xin, const float* kern, const float* lam, const float* rho,
                    const float* bounds, float* out, void* ws, size_t ws_bytes, hipStream_t s) {
    const Layout Lo = make_layout(d);
    if (int e = check_workspace(ws, ws_bytes, box_total(d, Lo))) return e;
    if (d.maxit == 0) {  // x = zeros (deconv.py:61,117)
        HIPCHK(hipMemsetAsync(out, 0, (size_t)d.B * d.C * d.H * d.W * sizeof(float), s));
        return 0;
    }
    if (int e = setup(d, Lo, ws, kern, rho, s, true)) return e;
    const BoxIO box{bounds, at<float>(ws, box_v_offset(Lo))};  // (v_0 = 0: the first row pass reads no v)
    switch (backend_of(d, Lo, 3)) {
        case Backend::Pow2: return fused_forward(Pow2Ops(d, Lo, ws), xin, lam, rho, out, nullptr, s, nullptr, &box);
        case Backend::Generic: return run_forward_gen<float>(d, Lo, false, xin, lam, rho, out, ws, nullptr, s, nullptr, &box);
        case Backend::Mixed:
        case Backend::OddRows:
        case Backend::OddRowsT: break;  // (never answered for mode 3)
    }
    return fail(ADMM_TV_EINVAL, "run_forward_box: no backend");
}

// backward workspace = forward layout + a^ ping-pong (4 images) + b^ + per-iteration partials
struct BwdLayout {
    Layout f;
    size_t abar[4], bbar, part, tpart, q, xpart, aacc, zacc, total;
    // a PSF bank's gradient: the taps' phase tables Eh [k][H], Ew [k][W/2 + 1] and stage-1 sums [T][k][W/2 + 1]
    size_t tapE, tapS;
    long long nstrips;
    int R, ntp, xgroups, xppg;
};
BwdLayout make_bwd_layout(const admm_tv_desc& d) {
    BwdLayout B{};
    B.f = make_layout(d);
    const size_t rs = is_f64(d) ? sizeof(double) : sizeof(float);
    const size_t G = ngroups_of(d);
    const size_t img = G * d.B * d.C * d.H * d.W * rs;  // all modules' planes
    size_t o = B.f.total;
    auto take = [&](size_t bytes) {
        size_t at_ = o;
        o += up(bytes);
        return at_;
    };
    for (int i = 0; i < 4; ++i) B.abar[i] = take(img);
    B.bbar = take(img);  // per module; summed into gxin at the end
    const long long rows = (long long)G * d.B * d.C * d.H;
    const Backend be = backend_of(d, B.f, 1);
    if (be == Backend::Mixed) {  // mixed-radix reverse row pass: strips of R rows (a device-independent rule)
        B.R = strip_rows_mixed((int)d.H, rows, (int)d.W / 2, 512);
        B.nstrips = rows / B.R;
    } else if (be == Backend::Generic) {  // generic backward: one partial pair per 256-pixel block
        B.R = 0;
        B.nstrips = (rows * d.W + 255) / 256;
    } else {
        B.R = strip_rows((int)d.H, (int)d.W / 2, rows);
        B.nstrips = rows / B.R;
    }
    // the lambda / rho gradient partials are fp64 in every solve (admm_backward.hpp)
    B.part = take((size_t)std::max(d.maxit, 1) * B.nstrips * 2 * sizeof(double));
    // tau^ partials per iteration and module: one per block of the fused paths' Q reduce (k_iso_reduce_tau,
    // 1,024 values per block); the generic path's k_iso_tau_partial runs that many blocks too
    B.ntp = (int)std::max<long long>(1, ((long long)d.H * d.W / 2 + 255) / 256);
    B.tpart = take((size_t)std::max(d.maxit, 1) * G * B.ntp * sizeof(double));  // [K][G][ntp]
    B.q = take(G * 2 * (size_t)d.H * d.W * rs);
    if (d.kh > 0 && (d.flags & ADMM_TV_FLAG_PSF_GRAD)) {
        const size_t nf = ((size_t)d.W / 2 + 1) * d.H;
        B.xppg = 8;
        B.xgroups = (int)((d.B * d.C + B.xppg - 1) / B.xppg);
        // fused paths: per-plane-group cross-spectrum partials; generic: one 2-D spectrum set
        const bool generic_x = be == Backend::Generic;
        // a PSF bank: plane groups of one table each (T x cpt of them), A_t real fp64 and Z_t complex fp64 per table
        // -- 24 bytes per half-spectrum point and table -- and the separable taps' phase tables and k rows of
        // W/2 + 1 complex fp64 sums per table
        const bool bank = is_bank(d);
        const size_t T = bank ? (size_t)bank_of(d).T : 1, k = (size_t)d.kh, N1 = (size_t)d.W / 2 + 1;
        if (bank) B.xgroups = (int)T * xbank_of(d, B.xppg).cpt;
        B.xpart = take((generic_x ? (size_t)d.B * d.C : (size_t)B.xgroups) * nf * 2 * rs);
        B.aacc = take(bank ? T * nf * sizeof(double) : nf * sizeof(double2));
        B.zacc = take(T * nf * sizeof(double2));
        if (bank) {
            B.tapE = take(k * ((size_t)d.H + N1) * sizeof(double2));
            B.tapS = take(T * k * N1 * sizeof(double2));
        }
    }
    B.total = o;
    return B;
}


// A PSF bank's taps from its per-table accumulators (A_t at BL.aacc, Z_t at BL.zacc, sigma_t at Layout::sigma):
// the phase tables once, then the two separable stages (admm_backward.hpp).  gkern: T kh kw floats, bank order.
int bank_taps(const admm_tv_desc& d, const BwdLayout& BL, void* ws, float* gkern, double zscale, hipStream_t s) {
    const int H = (int)d.H, W = (int)d.W, N1 = W / 2 + 1, k = d.kh;
    const unsigned T = (unsigned)bank_of(d).T;
    double2* Eh = at<double2>(ws, BL.tapE);
    double2* Ew = Eh + (size_t)k * H;
    const long long ne = (long long)k * (H + N1);
    hipLaunchKernelGGL(k_tap_tables, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, s, Eh, Ew, k, H, W);
    if (int e = launch_check("k_tap_tables")) return e;
    hipLaunchKernelGGL(k_psf_taps_col, dim3((unsigned)N1, T), dim3(256), 0, s, at<double>(ws, BL.aacc),
                       at<double2>(ws, BL.zacc), at<double2>(ws, BL.f.sigma), Eh, Ew, at<double2>(ws, BL.tapS), k, H, W, zscale);
    if (int e = launch_check("k_psf_taps_col")) return e;
    hipLaunchKernelGGL(k_psf_taps_row, dim3((unsigned)(k * k), T), dim3(256), 0, s, at<double2>(ws, BL.tapS), Ew, k, W, gkern);
    return launch_check("k_psf_taps_row");
}

// generic-size backward (same contract as admm_tv_backward, PSF gradient excluded)
template <class T>
int run_backward_gen(const admm_tv_desc& d, const BwdLayout& BL, const T* xin, const T* lam, const T* rho,
                     const T* gout, const void* hist, T* gxin, T* glam, T* grho, T* gkern, void* ws, hipStream_t s) {
    using C = cx_t<T>;
    const Layout& Lo = BL.f;
    const long long P = d.B * d.C;
    const int H = (int)d.H, W = (int)d.W, K = d.maxit;
    const long long npx = P * H * W;
    const long long HW = (long long)H * W;
    const HistView<T> hv(d, Lo, hist);
    const bool psf_grad = gkern != nullptr;
    const int Wh = W / 2 + 1;
    const long long nf = (long long)Wh * H;
    C* xspec = psf_grad ? at<C>(ws, BL.xpart) : nullptr;  // 2-D spectra of x^_k (then of b^)
    const bool bank = is_bank(d);  // fp32 (bank_check): each plane's table, the PSF gradient per table
    const BankIdx bk = bank_of(d);
    const BankIdx* const bankp = bank ? &bk : nullptr;
    if (psf_grad && bank) {
        HIPCHK(hipMemsetAsync(at<double>(ws, BL.aacc), 0, (size_t)bk.T * nf * sizeof(double), s));
    } else if (psf_grad) {
        HIPCHK(hipMemsetAsync(at<double2>(ws, BL.aacc), 0, nf * sizeof(double2), s));
        HIPCHK(hipMemsetAsync(at<double2>(ws, BL.zacc), 0, nf * sizeof(double2), s));
    }
    C* twW = at<C>(ws, Lo.twW);
    C* twH = at<C>(ws, Lo.twH);
    C* gs = at<C>(ws, Lo.gscr);  // long lines: the transform blocks' scratch slots
    T* fcT = at<T>(ws, Lo.fcT);
    const long long rows = P * H;
    const dim3 fgrid((unsigned)((nf + 255) / 256)), fblk(256);
    C* spec = at<C>(ws, Lo.spec[0]);
    T* rb = at<T>(ws, Lo.spec[1]);   // r^_k
    T* xbuf[2] = {at<T>(ws, Lo.rimg), at<T>(ws, Lo.u[0])};  // x^ ping-pong
    T* ab[4] = {at<T>(ws, BL.abar[0]), at<T>(ws, BL.abar[1]), at<T>(ws, BL.abar[2]),
                    at<T>(ws, BL.abar[3])};
    T* bbar = (d.kh == 0 && gxin) ? gxin : at<T>(ws, BL.bbar);
    double* part = at<double>(ws, BL.part);
    double* tpart = at<double>(ws, BL.tpart);
    T* q = at<T>(ws, BL.q);
    if (d.iso) HIPCHK(hipMemsetAsync(tpart, 0, (size_t)K * BL.ntp * sizeof(double), s));
    const T* xbk = gout;
    int ain = 0, xo = 0;
    for (int k = K; k >= 1; --k) {
        const bool lastk = (k == K), firstk = (k == 1);
        {
            ProfScope ps(1, s);
            // r^_k = M x^_k; with the PSF gradient the column pass also dumps X^_k's spectrum and
            // A += fc^2 Re(sum_p conj(X^_k) R_k)
            if (int e = grow_fwd(xbk, spec, twW, W, rows, s, gs)) return e;
            if (int e = gcol<T>(spec, xspec, fcT, at<C>(ws, Lo.mT), twH, H, W, P, 0, s, gs, Lo.mm, 0, bankp)) return e;
            if (int e = grow_inv<T>(spec, rb, twW, W, rows, s, gs, Lo.mmr)) return e;
            if constexpr (!kF64<T>) {
                if (psf_grad && bank) {  // A_t += fc_t^2 Re(sum over table t's planes of conj(X^_k) R_k)
                    hipLaunchKernelGGL(k_gxspec_acc_bank, dim3(fgrid.x, (unsigned)bk.T), fblk, 0, s, xspec, hv.r(k),
                                       xbank_of(d, BL.xppg), H, Wh, fcT, at<double>(ws, BL.aacc), (double2*)nullptr);
                    if (int e = launch_check("k_gxspec_acc_bank")) return e;
                }
            }
            if (psf_grad && !bank) {
                hipLaunchKernelGGL(k_gxspec_acc<T>, fgrid, fblk, 0, s, xspec, hv.r(k), P, H, Wh, fcT, at<double2>(ws, BL.aacc));
                if (int e = launch_check("k_gxspec_acc")) return e;
            }
        }
        if (d.iso && !firstk) {
            ProfScope ps(2, s);
            const dim3 grid((unsigned)((HW + 255) / 256)), blk(256);
            if (lastk)
                hipLaunchKernelGGL((k_giso_q<true, T>), grid, blk, 0, s, rb, ab[2 * ain], ab[2 * ain + 1], hv.a(k - 1, 0),
                                   hv.a(k - 1, 1), rho, q, H, W, P);
            else
                hipLaunchKernelGGL((k_giso_q<false, T>), grid, blk, 0, s, rb, ab[2 * ain], ab[2 * ain + 1], hv.a(k - 1, 0),
                                   hv.a(k - 1, 1), rho, q, H, W, P);
            if (int e = launch_check("k_giso_q")) return e;
            hipLaunchKernelGGL(k_iso_tau_partial<T>, dim3(BL.ntp), dim3(256), 0, s, q, hv.n(k - 1), lam, rho,
                               tpart + (size_t)(K - k) * BL.ntp, 2LL * HW);
            if (int e = launch_check("k_iso_tau_partial")) return e;
            allreduce(d, reinterpret_cast<float*>(q), 2ull * H * W, s);
        }
        {
            ProfScope ps(0, s);
            GBwdArgsT<T> ba{rb, xbuf[xo], bbar,
                        ab[2 * ain], ab[2 * ain + 1], ab[2 * (1 - ain)], ab[2 * (1 - ain) + 1],
                        hv.a(k, 0), hv.a(k, 1),
                        firstk ? nullptr : hv.a(k - 1, 0), firstk ? nullptr : hv.a(k - 1, 1),
                        (d.iso && !firstk) ? hv.n(k - 1) : nullptr, q, lam, rho,
                        part + (size_t)(K - k) * BL.nstrips * 2, H, W, npx};
            if (int e = gbwd(ba, d.iso != 0, lastk, firstk, s)) return e;
        }
        xbk = xbuf[xo];
        xo = 1 - xo;
        ain = 1 - ain;
    }
    if (glam && grho) {
        if (int e = bwd_scalars<T>(part, K, BL.nstrips, BL.nstrips, 0LL, d.iso ? tpart : nullptr, BL.ntp, 1, 0, lam, rho,
                                   glam, grho, s))
            return e;
    } else if (glam || grho) {
        return fail(ADMM_TV_EINVAL, "glam and grho must be given together");
    }
    if (psf_grad) {  // Z = sum_p conj(Bbar_p) Xin_p, then the k x k taps
        if (int e = grow_fwd(bbar, spec, twW, W, rows, s, gs)) return e;
        if (int e = gcol<T>(spec, xspec, nullptr, nullptr, twH, H, W, P, 3, s, gs, Lo.mm)) return e;
        if (int e = grow_fwd(xin, spec, twW, W, rows, s, gs)) return e;
        if (int e = gcol<T>(spec, spec, nullptr, nullptr, twH, H, W, P, 3, s, gs, Lo.mm)) return e;
        if constexpr (!kF64<T>) {
            if (bank) {
                hipLaunchKernelGGL(k_gxspec_acc_bank, dim3(fgrid.x, (unsigned)bk.T), fblk, 0, s, xspec, spec,
                                   xbank_of(d, BL.xppg), H, Wh, (const float*)nullptr, (double*)nullptr,
                                   at<double2>(ws, BL.zacc));
                if (int e = launch_check("k_gxspec_acc_bank")) return e;
                if (int e = bank_taps(d, BL, ws, gkern, 1.0, s)) return e;
            }
        }
        if (!bank) {
            hipLaunchKernelGGL(k_gxspec_acc<T>, fgrid, fblk, 0, s, xspec, spec, P, H, Wh, nullptr, at<double2>(ws, BL.zacc));
            if (int e = launch_check("k_gxspec_acc")) return e;
            hipLaunchKernelGGL(k_psf_grad<T>, dim3(d.kh * d.kw), dim3(256), 0, s, at<double2>(ws, BL.aacc),
                               at<double2>(ws, BL.zacc), at<double2>(ws, Lo.sigma), d.kh, H, W, gkern, 1.0);
            if (int e = launch_check("k_psf_grad")) return e;
        }
    }
    if (gxin && d.kh > 0)  // x^_in = H_t^T b^
        if (int e = gapply<T>(bbar, gxin, spec, Lo, ws, d, 2, s)) return e;
    return 0;
}

// The training backward on a fused backend: the forward's reverse sequence.  x^_K = gout; per iteration,
// K down to 1: r^_k = M x^_k by the inference column pass, [iso: Q_{k-1} per module, its tau^ partial and
// the cross-rank hook], the reverse row pass; then the scalar gradients per module, [PSF gradient: the k x k
// taps,] [grouped modules: their b^ summed,] and x^_in = H_t^T b^ when there is a PSF.  All modules' planes
// go through every launch (a backend that trains grouped modules runs them together).
template <class B>
int fused_backward(const B& be, const BwdLayout& BL, const float* xin, const float* lam, const float* rho,
                   const float* gout, const void* hist, float* gxin, float* glam, float* grho, float* gkern,
                   hipStream_t s) {
    const admm_tv_desc& d = be.d;
    const Layout& Lo = be.Lo;
    void* ws = be.ws;
    const int H = be.H, N = be.N, W = (int)d.W, K = d.maxit, G = ngroups_of(d);
    const long long Pm = d.B * d.C, P = G * Pm;  // planes of one module, of all modules
    const HistView<float> hv(d, Lo, hist);
    const bool psf_grad = B::kPsfGrad && gkern != nullptr;
    const long long nf = (long long)(N + 1) * H;
    // a PSF bank (one module): the cross spectra in plane groups of one table each, reduced per table
    // (BL.xppg is set with the PSF gradient only: no chunks to count without it)
    const bool bank = is_bank(d);
    const XBank xb = (bank && psf_grad) ? xbank_of(d, BL.xppg) : XBank{1, 1, 1, 1};
    const XBank* const xbp = bank ? &xb : nullptr;
    const unsigned nT = bank ? (unsigned)bank_of(d).T : 1;
    if (psf_grad && bank) {
        HIPCHK(hipMemsetAsync(at<double>(ws, BL.aacc), 0, (size_t)nT * nf * sizeof(double), s));
    } else if (psf_grad) {
        HIPCHK(hipMemsetAsync(at<double2>(ws, BL.aacc), 0, nf * sizeof(double2), s));
        HIPCHK(hipMemsetAsync(at<double2>(ws, BL.zacc), 0, nf * sizeof(double2), s));
    }
    cf* spec[2] = {at<cf>(ws, Lo.spec[0]), at<cf>(ws, Lo.spec[1])};
    float* ab[4] = {at<float>(ws, BL.abar[0]), at<float>(ws, BL.abar[1]), at<float>(ws, BL.abar[2]),
                    at<float>(ws, BL.abar[3])};
    // b^ accumulates straight into gxin when there is no PSF and one module (x^_in = b^)
    float* bbar = (d.kh == 0 && gxin && G == 1) ? gxin : at<float>(ws, BL.bbar);
    double* part = at<double>(ws, BL.part);
    double* tpart = at<double>(ws, BL.tpart);
    float* q = at<float>(ws, BL.q);
    const long long rows = P * H;
    if (d.iso) HIPCHK(hipMemsetAsync(tpart, 0, (size_t)K * G * BL.ntp * sizeof(double), s));
    if (int e = be.r2c(gout, spec[0], rows, s)) return e;
    int cur = 0, ain = 0;
    for (int k = K; k >= 1; --k) {
        if (psf_grad && bank) {  // A_t += fc_t^2 Re(sum over table t's planes), as below
            if (int e = be.xspec(spec[cur], hv.r(k), at<cf>(ws, BL.xpart), P, BL.xppg, true, s, xbp)) return e;
            hipLaunchKernelGGL(k_xspec_reduce_bank, dim3((unsigned)((nf + 255) / 256), nT), dim3(256), 0, s,
                               at<cf>(ws, BL.xpart), xb.cpt, nf, at<float>(ws, Lo.fcT), at<double>(ws, BL.aacc),
                               (double2*)nullptr);
            if (int e = launch_check("k_xspec_reduce_bank")) return e;
        } else if (psf_grad) {  // A += fc^2 Re(sum_p conj(X^_k) R_k), before the column pass rewrites X^_k
            if (int e = be.xspec(spec[cur], hv.r(k), at<cf>(ws, BL.xpart), P, BL.xppg, true, s)) return e;
            hipLaunchKernelGGL(k_xspec_reduce, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, s,
                               at<cf>(ws, BL.xpart), BL.xgroups, nf, at<float>(ws, Lo.fcT), at<double2>(ws, BL.aacc));
            if (int e = launch_check("k_xspec_reduce")) return e;
        }
        {
            ProfScope ps(1, s);
            if (int e = be.col(spec[cur], spec[cur], P, Pm, 0, s)) return e;
        }
        const bool lastk = (k == K), firstk = (k == 1);
        if (d.iso && !firstk) {
            ProfScope ps(2, s);
            BwdIsoArgs qa{spec[cur], ab[2 * ain], ab[2 * ain + 1], hv.a(k - 1, 0), hv.a(k - 1, 1), rho,
                          at<float>(ws, Lo.part), be.twW, (int)P, H, Lo.ppg, (long long)Lo.ngroups * H, Pm};
            if (int e = be.bwd_iso_q(qa, lastk, s)) return e;
            const long long n4 = 2LL * H * W / 4;
            const int gpm = Lo.ngroups / G;
            for (int g = 0; g < G; ++g) {  // per module: Q over its planes, then its tau^ partial
                float* qg = q + (size_t)g * 2 * H * W;
                // Q and the tau^ partials from this rank's Q (the norm N is already global): summing the
                // ranks' lambda/rho gradients then counts every plane once
                hipLaunchKernelGGL(k_iso_reduce_tau, dim3((unsigned)BL.ntp), dim3(256), 0, s,
                                   at<float4>(ws, Lo.part) + (size_t)g * gpm * n4, reinterpret_cast<float4*>(qg), gpm, n4,
                                   reinterpret_cast<const float4*>(hv.n(k - 1) + (size_t)g * 2 * H * W), lam + g, rho + g,
                                   tpart + ((size_t)(K - k) * G + g) * BL.ntp);
                if (int e = launch_check("k_iso_reduce_tau")) return e;
            }
            allreduce(d, q, (size_t)G * 2 * H * W, s);  // Q over every rank's planes
        }
        {
            ProfScope ps(0, s);
            BwdArgs ba{spec[cur], spec[1 - cur], bbar,
                       ab[2 * ain], ab[2 * ain + 1], ab[2 * (1 - ain)], ab[2 * (1 - ain) + 1],
                       hv.a(k, 0), hv.a(k, 1),
                       firstk ? nullptr : hv.a(k - 1, 0), firstk ? nullptr : hv.a(k - 1, 1),
                       (d.iso && !firstk) ? hv.n(k - 1) : nullptr, q, lam, rho,
                       part + (size_t)(K - k) * BL.nstrips * 2, be.twW, H, BL.R, BL.nstrips, Pm};
            if (int e = be.bwd_pass_a(ba, d.iso != 0, lastk, firstk, s)) return e;
        }
        cur = 1 - cur;
        ain = 1 - ain;
    }
    if (glam && grho) {
        const long long spm = BL.nstrips / G;  // strips of one module (module-major planes)
        for (int g = 0; g < G; ++g) {
            if (int e = bwd_scalars<float>(part, K, BL.nstrips, spm, (long long)g * spm, d.iso ? tpart : nullptr, BL.ntp, G,
                                           g, lam + g, rho + g, glam + g, grho + g, s))
                return e;
        }
    } else if (glam || grho) {
        return fail(ADMM_TV_EINVAL, "glam and grho must be given together");
    }
    if (psf_grad) {  // Z = sum_p conj(Bbar_p) Xin_p, then the k x k taps
        if (int e = be.r2c(bbar, spec[0], rows, s)) return e;
        if (int e = be.r2c(xin, spec[1], rows, s)) return e;
        if (bank) {  // Z_t per table, then the separable taps
            if (int e = be.xspec(spec[0], spec[1], at<cf>(ws, BL.xpart), P, BL.xppg, false, s, xbp)) return e;
            hipLaunchKernelGGL(k_xspec_reduce_bank, dim3((unsigned)((nf + 255) / 256), nT), dim3(256), 0, s,
                               at<cf>(ws, BL.xpart), xb.cpt, nf, (const float*)nullptr, (double*)nullptr,
                               at<double2>(ws, BL.zacc));
            if (int e = launch_check("k_xspec_reduce_bank")) return e;
            if (int e = bank_taps(d, BL, ws, gkern, 0.25, s)) return e;
        } else {
            if (int e = be.xspec(spec[0], spec[1], at<cf>(ws, BL.xpart), P, BL.xppg, false, s)) return e;
            hipLaunchKernelGGL(k_xspec_reduce, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, s, at<cf>(ws, BL.xpart),
                               BL.xgroups, nf, nullptr, at<double2>(ws, BL.zacc));
            if (int e = launch_check("k_xspec_reduce")) return e;
            hipLaunchKernelGGL(k_psf_grad<float>, dim3(d.kh * d.kw), dim3(256), 0, s, at<double2>(ws, BL.aacc),
                               at<double2>(ws, BL.zacc), at<double2>(ws, Lo.sigma), d.kh, H, W, gkern, 0.25);
            if (int e = launch_check("k_psf_grad")) return e;
        }
    }
    if (gxin && G > 1) {  // the modules share xin: x^_in collects every module's b^
        const long long n4 = Pm * H * W / 4;
        float* sum = d.kh > 0 ? bbar : gxin;  // with a PSF, sum in place (module 0's slot) first
        hipLaunchKernelGGL(k_sum_modules, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s,
                           reinterpret_cast<const float4*>(bbar), reinterpret_cast<float4*>(sum), G, n4);
        if (int e = launch_check("k_sum_modules")) return e;
    }
    if (gxin && d.kh > 0)
        if (int e = be.apply_ht_t(bbar, gxin, spec[0], s)) return e;
    return 0;
}

// The backward solver (admm_tv_backward's contract, its descriptor already validated).
int run_backward(const admm_tv_desc& d, const float* xin, const float* kern, const float* lam, const float* rho,
                 const float* gout, const void* hist, size_t hist_bytes, float* gxin, float* glam, float* grho,
                 float* gkern, void* ws, size_t ws_bytes, hipStream_t s) {
    if ((!gout && !participate_only(d)) || !lam || !rho || (d.kh > 0 && !kern))
        return fail(ADMM_TV_EINVAL, "null pointer argument");
    const BwdLayout BL = make_bwd_layout(d);
    const Layout& Lo = BL.f;
    if (int e = check_workspace(ws, ws_bytes, BL.total)) return e;
    const int G = ngroups_of(d);
    const int H = (int)d.H, W = (int)d.W, K = d.maxit;
    const size_t img_bytes = (size_t)d.B * d.C * H * W * sizeof(float);  // gxin: one module's planes
    if (gkern && (d.kh == 0 || !(d.flags & ADMM_TV_FLAG_PSF_GRAD) || (!xin && !participate_only(d))))
        return fail(ADMM_TV_EINVAL, "gkern needs a PSF, ADMM_TV_FLAG_PSF_GRAD (forward and backward) and xin");
    if (K == 0) {  // output is identically zero
        if (gxin) HIPCHK(hipMemsetAsync(gxin, 0, img_bytes, s));
        if (glam) HIPCHK(hipMemsetAsync(glam, 0, sizeof(float) * G, s));
        if (grho) HIPCHK(hipMemsetAsync(grho, 0, sizeof(float) * G, s));
        if (gkern) HIPCHK(hipMemsetAsync(gkern, 0, sizeof(float) * (is_bank(d) ? bank_of(d).T : 1) * d.kh * d.kw, s));
        return 0;
    }
    if (participate_only(d)) {  // the same reductions as the iso backward, contributing zeros
        const size_t n = (size_t)G * 2 * H * W;
        for (int k = K; k >= 2; --k) {
            HIPCHK(hipMemsetAsync(at<float>(ws, BL.q), 0, n * sizeof(float), s));
            allreduce(d, at<float>(ws, BL.q), Lo.gen ? 2ull * H * W : n, s);
        }
        if (glam) HIPCHK(hipMemsetAsync(glam, 0, sizeof(float) * G, s));
        if (grho) HIPCHK(hipMemsetAsync(grho, 0, sizeof(float) * G, s));
        if (gkern) HIPCHK(hipMemsetAsync(gkern, 0, sizeof(float) * d.kh * d.kw, s));
        return 0;
    }
    if (!hist || hist_bytes < make_hist(d, Lo).total) return fail(ADMM_TV_EWORKSPACE, "history buffer too small");
    if (int e = setup(d, Lo, ws, kern, rho, s)) return e;
    switch (backend_of(d, Lo, 1)) {
        case Backend::Pow2: return fused_backward(Pow2Ops(d, Lo, ws), BL, xin, lam, rho, gout, hist, gxin, glam, grho, gkern, s);
        case Backend::Mixed: return fused_backward(MixedOps(d, Lo, ws), BL, xin, lam, rho, gout, hist, gxin, glam, grho, gkern, s);
        case Backend::Generic: return run_backward_gen(d, BL, xin, lam, rho, gout, hist, gxin, glam, grho, gkern, ws, s);
        case Backend::OddRows:
        case Backend::OddRowsT: break;  // (training never runs the odd-length row pass: never answered for mode 1)
    }
    return fail(ADMM_TV_EINVAL, "run_backward: no backend");
}

// ------------------------------------------------------------------ fp64 solves (ADMM_TV_FLAG_F64)
// The forward of an fp64 solve: run_forward's contract on the generic kernels' double instantiation.
int run_forward_f64(const admm_tv_desc& d, const double* xin, const double* kern, const double* lam,
                    const double* rho, double* out, void* ws, size_t ws_bytes, void* hist, hipStream_t s) {
    const Layout Lo = make_layout(d);
    if (int e = check_workspace(ws, ws_bytes, Lo.total)) return e;
    const int H = (int)d.H, W = (int)d.W;
    const size_t img_bytes = (size_t)d.B * d.C * H * W * sizeof(double);
    if (d.maxit == 0) {
        if (img_bytes) HIPCHK(hipMemsetAsync(out, 0, img_bytes, s));  // the reference returns x = zeros
        return 0;
    }
    if (participate_only(d)) {  // the same reductions as the iso loop, contributing zeros
        for (int it = 1; it <= d.maxit; ++it) {
            if (it == d.maxit && !hist) break;
            HIPCHK(hipMemsetAsync(at<double>(ws, Lo.nsq), 0, 2ull * H * W * sizeof(double), s));
            allreduce(d, at<float>(ws, Lo.nsq), 2ull * H * W, s);
        }
        return 0;
    }
    if (int e = setup<double>(d, Lo, ws, kern, rho, s)) return e;
    return run_forward_gen<double>(d, Lo, false, xin, lam, rho, out, ws, hist, s);
}

int run_backward_f64(const admm_tv_desc& d, const double* xin, const double* kern, const double* lam,
                     const double* rho, const double* gout, const void* hist, size_t hist_bytes, double* gxin,
                     double* glam, double* grho, double* gkern, void* ws, size_t ws_bytes, hipStream_t s) {
    const BwdLayout BL = make_bwd_layout(d);
    if (int e = check_workspace(ws, ws_bytes, BL.total)) return e;
    const int H = (int)d.H, W = (int)d.W, K = d.maxit;
    const size_t img_bytes = (size_t)d.B * d.C * H * W * sizeof(double);
    if (gkern && (d.kh == 0 || !(d.flags & ADMM_TV_FLAG_PSF_GRAD) || (!xin && !participate_only(d))))
        return fail(ADMM_TV_EINVAL, "gkern needs a PSF, ADMM_TV_FLAG_PSF_GRAD (forward and backward) and xin");
    if ((glam == nullptr) != (grho == nullptr)) return fail(ADMM_TV_EINVAL, "glam and grho must be given together");
    if (K == 0 || participate_only(d)) {
        if (participate_only(d) && K > 0)
            for (int k = K; k >= 2; --k) {
                HIPCHK(hipMemsetAsync(at<double>(ws, BL.q), 0, 2ull * H * W * sizeof(double), s));
                allreduce(d, at<float>(ws, BL.q), 2ull * H * W, s);
            }
        if (gxin && img_bytes) HIPCHK(hipMemsetAsync(gxin, 0, img_bytes, s));
        if (glam) HIPCHK(hipMemsetAsync(glam, 0, sizeof(double), s));
        if (grho) HIPCHK(hipMemsetAsync(grho, 0, sizeof(double), s));
        if (gkern) HIPCHK(hipMemsetAsync(gkern, 0, sizeof(double) * d.kh * d.kw, s));
        return 0;
    }
    if (!hist || hist_bytes < make_hist(d, BL.f).total) return fail(ADMM_TV_EWORKSPACE, "history buffer too small");
    if (int e = setup<double>(d, BL.f, ws, kern, rho, s)) return e;
    return run_backward_gen<double>(d, BL, xin, lam, rho, gout, hist, gxin, glam, grho, gkern, ws, s);
}

}  // namespace

// ============================================================================ C ABI
extern "C" {

int admm_tv_abi_version(void) { return ADMM_TV_ABI_VERSION; }

int admm_tv_supported(int64_t H, int64_t W) {
    return supported_hw(H, W) ? 1 : mixed_hw(H, W) ? 3 : (odd_hw(H, W) || odd_t_hw(H, W)) ? 4 : generic_hw(H, W) ? 2 : 0;
}

int admm_tv_supported_f64(int64_t H, int64_t W) { return f64_hw(H, W) ? 1 : 0; }

int admm_tv_path(const admm_tv_desc* d, int train) {
    if (int e = validate(d)) return e;
    if (train == 3) {  // admm_tv_forward_box (its refusals come ahead of a bank's own)
        if (int e = box_check(*d)) return e;
    }
    if (int e = bank_check(*d, train == 1)) return e;
    if (train == 2) {  // admm_tv_forward_state
        if (int e = state_check(*d)) return e;
    } else if (train && train != 3) {
        if (int e = grouped_train_check(*d)) return e;
    }
    switch (backend_of(*d, make_layout(*d), train == 2 || train == 3 ? train : train ? 1 : 0)) {
        case Backend::Pow2: return ADMM_TV_PATH_FUSED;
        case Backend::Mixed: return ADMM_TV_PATH_MIXED;
        case Backend::Generic: return ADMM_TV_PATH_GENERIC;
        case Backend::OddRows:
        case Backend::OddRowsT: return ADMM_TV_PATH_ODD;
    }
    return ADMM_TV_PATH_GENERIC;
}

const char* admm_tv_last_error(void) { return g_err.c_str(); }

int admm_tv_workspace_size(const admm_tv_desc* d, size_t* bytes) {
    if (int e = validate(d)) return e;
    if (int e = bank_check(*d)) return e;
    if (!bytes) return fail(ADMM_TV_EINVAL, "null bytes");
    *bytes = make_layout(*d).total;
    return 0;
}

int admm_tv_forward(const admm_tv_desc* dp, const float* xin, const float* kern, const float* lam, const float* rho,
                    float* out, void* ws, size_t ws_bytes, void* stream) {
    if (int e = validate(dp)) return e;
    if (int e = bank_check(*dp)) return e;
    if (is_f64(*dp)) return fail(ADMM_TV_EINVAL, "ADMM_TV_FLAG_F64: use admm_tv_forward_f64");
    if (((!xin || !out) && !participate_only(*dp)) || !lam || !rho || (dp->kh > 0 && !kern))
        return fail(ADMM_TV_EINVAL, "null pointer argument");
    DeviceGuard dg(reinterpret_cast<hipStream_t>(stream));
    if (int e = dg.check()) return e;
    return run_forward(*dp, xin, kern, lam, rho, out, ws, ws_bytes, nullptr, reinterpret_cast<hipStream_t>(stream));
}

int admm_tv_state_workspace_size(const admm_tv_desc* d, size_t* bytes) {
    if (int e = validate(d)) return e;
    if (int e = bank_check(*d)) return e;
    if (int e = state_check(*d)) return e;
    if (!bytes) return fail(ADMM_TV_EINVAL, "null bytes");
    *bytes = make_layout(*d).total;  // the forward's regions serve: v lives in `out`, the iso norm in part / nsq
    return 0;
}

int admm_tv_forward_state(const admm_tv_desc* dp, const float* xin, const float* kern, const float* lam,
                          const float* rho, const admm_tv_state* state_in, const admm_tv_state* state_out, float* out,
                          void* ws, size_t ws_bytes, void* stream) {
    if (int e = validate(dp)) return e;
    if (int e = bank_check(*dp)) return e;
    if (int e = state_check(*dp)) return e;
    if (!xin || !out || !lam || !rho || (dp->kh > 0 && !kern)) return fail(ADMM_TV_EINVAL, "null pointer argument");
    for (const admm_tv_state* st : {state_in, state_out})
        if (st && (!st->zx || !st->zy || !st->ux || !st->uy))
            return fail(ADMM_TV_EINVAL, "admm_tv_state with a null member (pass a NULL struct for no state)");
    DeviceGuard dg(reinterpret_cast<hipStream_t>(stream));
    if (int e = dg.check()) return e;
    return run_forward_state(*dp, xin, kern, lam, rho, StateIO{state_in, state_out}, out, ws, ws_bytes,
                             reinterpret_cast<hipStream_t>(stream));
}

int admm_tv_box_workspace_size(const admm_tv_desc* d, size_t* bytes) {
    if (int e = validate(d)) return e;
    if (int e = box_check(*d)) return e;
    if (!bytes) return fail(ADMM_TV_EINVAL, "null bytes");
    *bytes = box_total(*d, make_layout(*d));  // the forward's regions, then v
    return 0;
}

int admm_tv_forward_box(const admm_tv_desc* dp, const float* xin, const float* kern, const float* lam, const float* rho,
                        const float* bounds, float* out, void* ws, size_t ws_bytes, void* stream) {
    if (int e = validate(dp)) return e;
    if (int e = box_check(*dp)) return e;
    if (!bounds) return fail(ADMM_TV_EINVAL, "admm_tv_forward_box: null bounds_dev (a device float[2] = {lo, hi})");
    if (!xin || !out || !lam || !rho || (dp->kh > 0 && !kern)) return fail(ADMM_TV_EINVAL, "null pointer argument");
    DeviceGuard dg(reinterpret_cast<hipStream_t>(stream));
    if (int e = dg.check()) return e;
    return run_forward_box(*dp, xin, kern, lam, rho, bounds, out, ws, ws_bytes, reinterpret_cast<hipStream_t>(stream));
}

int admm_tv_history_size(const admm_tv_desc* d, size_t* bytes) {
    if (int e = validate(d)) return e;
    if (int e = bank_check(*d, true)) return e;
    if (int e = grouped_train_check(*d)) return e;
    if (!bytes) return fail(ADMM_TV_EINVAL, "null bytes");
    *bytes = make_hist(*d, make_layout(*d)).total;
    return 0;
}

int admm_tv_forward_train(const admm_tv_desc* dp, const float* xin, const float* kern, const float* lam,
                          const float* rho, float* out, void* hist, size_t hist_bytes, void* ws, size_t ws_bytes,
                          void* stream) {
    if (int e = validate(dp)) return e;
    if (int e = bank_check(*dp, true)) return e;
    if (int e = grouped_train_check(*dp)) return e;
    if (is_f64(*dp)) return fail(ADMM_TV_EINVAL, "ADMM_TV_FLAG_F64: use admm_tv_forward_train_f64");
    if (((!xin || !out) && !participate_only(*dp)) || !lam || !rho || (dp->kh > 0 && !kern))
        return fail(ADMM_TV_EINVAL, "null pointer argument");
    if (dp->maxit > 0 && (!hist || hist_bytes < make_hist(*dp, make_layout(*dp)).total))
        return fail(ADMM_TV_EWORKSPACE, "history buffer too small");
    DeviceGuard dg(reinterpret_cast<hipStream_t>(stream));
    if (int e = dg.check()) return e;
    return run_forward(*dp, xin, kern, lam, rho, out, ws, ws_bytes, dp->maxit > 0 ? hist : nullptr,
                       reinterpret_cast<hipStream_t>(stream));
}

int admm_tv_backward_workspace_size(const admm_tv_desc* d, size_t* bytes) {
    if (int e = validate(d)) return e;
    if (int e = bank_check(*d, true)) return e;
    if (int e = grouped_train_check(*d)) return e;
    if (!bytes) return fail(ADMM_TV_EINVAL, "null bytes");
    *bytes = make_bwd_layout(*d).total;
    return 0;
}

int admm_tv_backward(const admm_tv_desc* dp, const float* xin, const float* kern, const float* lam,
                     const float* rho, const float* gout, const void* hist, size_t hist_bytes, float* gxin,
                     float* glam, float* grho, float* gkern, void* ws, size_t ws_bytes, void* stream) {
    if (int e = validate(dp)) return e;
    if (int e = bank_check(*dp, true)) return e;
    if (int e = grouped_train_check(*dp)) return e;
    if (is_f64(*dp)) return fail(ADMM_TV_EINVAL, "ADMM_TV_FLAG_F64: use admm_tv_backward_f64");
    DeviceGuard dg(reinterpret_cast<hipStream_t>(stream));
    if (int e = dg.check()) return e;
    return run_backward(*dp, xin, kern, lam, rho, gout, hist, hist_bytes, gxin, glam, grho, gkern, ws, ws_bytes,
                        reinterpret_cast<hipStream_t>(stream));
}

int admm_tv_psf_transpose(const admm_tv_desc* dp, const float* xin, const float* kern, float* out, void* ws,
                          size_t ws_bytes, void* stream) {
    if (int e = validate(dp)) return e;
    if (int e = bank_check(*dp)) return e;
    if (is_f64(*dp)) return fail(ADMM_TV_EINVAL, "ADMM_TV_FLAG_F64: fp32 entry point");
    const admm_tv_desc d = *dp;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    DeviceGuard dg(reinterpret_cast<hipStream_t>(stream));
    if (int e = dg.check()) return e;
    const Layout Lo = make_layout(d);
    if (!ws || ws_bytes < Lo.total) return fail(ADMM_TV_EWORKSPACE, "workspace too small");
    const long long P = d.B * d.C;
    const int H = (int)d.H, W = (int)d.W, N = W / 2;
    if (d.kh == 0) {
        HIPCHK(hipMemcpyAsync(out, xin, (size_t)P * H * W * sizeof(float), hipMemcpyDeviceToDevice, s));
        return 0;
    }
    if (int e = setup<float>(d, Lo, ws, kern, nullptr, s)) return e;
    const int n = (N + 1) * H;
    // k_spectra needs a rho pointer: point it at a zeroed float inside the workspace (fcT region)
    HIPCHK(hipMemsetAsync(at<float>(ws, Lo.fcT), 0, sizeof(float), s));
    if (is_bank(d)) {
        // a bank: every table's multiplier (the unused factors, T (N + 1) H floats, fit the spec[1] image:
        // T <= B C, N + 1 <= W); a smooth size runs the mixed transforms, whose multiplier index the solve uses
        if (int e = bank_spectra(d, Lo, ws, at<float>(ws, Lo.fcT), at<float>(ws, Lo.spec[1]), s)) return e;
        if (Lo.mixed) return MixedOps(d, Lo, ws).make_b(xin, out, at<cf>(ws, Lo.spec[0]), false, s);
        if (Lo.gen) return gapply(xin, out, at<cf>(ws, Lo.spec[0]), Lo, ws, d, 1, s);
        return psf_transpose_into(d, Lo, ws, xin, out, at<cf>(ws, Lo.spec[0]), 1, s);
    }
    hipLaunchKernelGGL(k_spectra<float>, dim3((n + 255) / 256), dim3(256), 0, s, at<double2>(ws, Lo.G),
                       at<double2>(ws, Lo.twHd), at<float>(ws, Lo.fcT), at<float>(ws, Lo.spec[1]),
                       at<cf>(ws, Lo.mT), d.kh, H, N, W, nullptr, spectra_scale(H, W), 0);
    if (int e = launch_check("k_spectra")) return e;
    if (Lo.gen) return gapply(xin, out, at<cf>(ws, Lo.spec[0]), Lo, ws, d, 1, s);
    return psf_transpose_into(d, Lo, ws, xin, out, at<cf>(ws, Lo.spec[0]), 1, s);
}

int admm_tv_forward_f64(const admm_tv_desc* dp, const double* xin, const double* kern, const double* lam,
                        const double* rho, double* out, void* ws, size_t ws_bytes, void* stream) {
    if (int e = validate(dp)) return e;
    if (int e = bank_check(*dp, false, true)) return e;
    if (!is_f64(*dp)) return fail(ADMM_TV_EINVAL, "admm_tv_forward_f64 needs ADMM_TV_FLAG_F64");
    if (((!xin || !out) && !participate_only(*dp)) || !lam || !rho || (dp->kh > 0 && !kern))
        return fail(ADMM_TV_EINVAL, "null pointer argument");
    DeviceGuard dg(reinterpret_cast<hipStream_t>(stream));
    if (int e = dg.check()) return e;
    return run_forward_f64(*dp, xin, kern, lam, rho, out, ws, ws_bytes, nullptr, reinterpret_cast<hipStream_t>(stream));
}

int admm_tv_forward_train_f64(const admm_tv_desc* dp, const double* xin, const double* kern, const double* lam,
                              const double* rho, double* out, void* hist, size_t hist_bytes, void* ws, size_t ws_bytes,
                              void* stream) {
    if (int e = validate(dp)) return e;
    if (int e = bank_check(*dp, false, true)) return e;
    if (!is_f64(*dp)) return fail(ADMM_TV_EINVAL, "admm_tv_forward_train_f64 needs ADMM_TV_FLAG_F64");
    if (((!xin || !out) && !participate_only(*dp)) || !lam || !rho || (dp->kh > 0 && !kern))
        return fail(ADMM_TV_EINVAL, "null pointer argument");
    if (dp->maxit > 0 && (!hist || hist_bytes < make_hist(*dp, make_layout(*dp)).total))
        return fail(ADMM_TV_EWORKSPACE, "history buffer too small");
    DeviceGuard dg(reinterpret_cast<hipStream_t>(stream));
    if (int e = dg.check()) return e;
    return run_forward_f64(*dp, xin, kern, lam, rho, out, ws, ws_bytes, dp->maxit > 0 ? hist : nullptr,
                           reinterpret_cast<hipStream_t>(stream));
}

int admm_tv_backward_f64(const admm_tv_desc* dp, const double* xin, const double* kern, const double* lam,
                         const double* rho, const double* gout, const void* hist, size_t hist_bytes, double* gxin,
                         double* glam, double* grho, double* gkern, void* ws, size_t ws_bytes, void* stream) {
    if (int e = validate(dp)) return e;
    if (int e = bank_check(*dp, false, true)) return e;
    if (!is_f64(*dp)) return fail(ADMM_TV_EINVAL, "admm_tv_backward_f64 needs ADMM_TV_FLAG_F64");
    if ((!gout && !participate_only(*dp)) || !lam || !rho || (dp->kh > 0 && !kern))
        return fail(ADMM_TV_EINVAL, "null pointer argument");
    DeviceGuard dg(reinterpret_cast<hipStream_t>(stream));
    if (int e = dg.check()) return e;
    return run_backward_f64(*dp, xin, kern, lam, rho, gout, hist, hist_bytes, gxin, glam, grho, gkern, ws, ws_bytes,
                            reinterpret_cast<hipStream_t>(stream));
}

int admm_tv_profile_enable(int enable) {
    std::lock_guard<std::mutex> lk(g_prof.mu);
    g_prof.on = enable != 0;
    return 0;
}

int admm_tv_profile_reset(void) {
    std::lock_guard<std::mutex> lk(g_prof.mu);
    for (auto& r : g_prof.recs) {
        (void)hipEventSynchronize(r.b);
        g_prof.pool.push_back({r.dev, r.a});
        g_prof.pool.push_back({r.dev, r.b});
    }
    g_prof.recs.clear();
    for (int i = 0; i < 4; ++i) {
        g_prof.ms[i] = 0;
        g_prof.n[i] = 0;
    }
    return 0;
}

int admm_tv_profile_read(double* ms4, int64_t* count4) {
    std::lock_guard<std::mutex> lk(g_prof.mu);
    for (auto& r : g_prof.recs) {
        if (hipEventSynchronize(r.b) != hipSuccess) return fail(ADMM_TV_EHIP, "hipEventSynchronize");
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            g_prof.ms[r.kind] += ms;
            g_prof.n[r.kind] += 1;
        }
        g_prof.pool.push_back({r.dev, r.a});
        g_prof.pool.push_back({r.dev, r.b});
    }
    g_prof.recs.clear();
    for (int i = 0; i < 4; ++i) {
        if (ms4) ms4[i] = g_prof.ms[i];
        if (count4) count4[i] = g_prof.n[i];
    }
    return 0;
}

}  // extern "C"
