// state_kernels.hpp -- the solver state (the reference's z_x, z_y, u_x, u_y; deconv.py:63-67,111-115) entering
// and leaving a solve in image space (admm_tv_forward_state, include/admm_tv.h).  The iterations in between
// run on the inference kernels of the solve's path, which carry u in the path's own layout and r as packed
// row spectra; the two streaming kernels here translate at the call's two ends:
//
//   k_state_import   v = b + rho D^T (z0 - u0)  (the argument of the reference's rfftn, deconv.py:104) in pixel
//                    order, whose row transform is r_1; and u0 copied into the loop's u input buffers in the
//                    layout the path's row pass reads (pixel order, or lane-paired: admm_kernels.hpp ld_row)
//   k_state_export   after the output transform: a = D x_K + u_{K-1}, z_K = shrink(a, tau), u_K = a - z_K,
//                    from x_K in pixel order and the u that iteration K - 1 wrote (the imported u0, or none,
//                    when K = 1).  iso: the per-pixel norm over every (b, c) plane first -- k_state_iso_part
//                    (partial sums per plane group) and k_state_reduce -- then the same kernel applies it.
//
// One thread per V consecutive pixels of a row (V = 4: 16-byte accesses, where W and every pointer allow;
// 2 or 1 otherwise); a block covers TX pixel groups of 256 / TX rows; rows and pixels are indexed in 64
// bits.  Neighbours wrap circularly (a one-row or one-column image onto itself), as in k_gstep /
// k_giso_norm (generic_kernels.hpp), and the arithmetic is theirs expression for expression.
#pragma once
#include "admm_kernels.hpp"

namespace admm {

struct StateImportArgs {
    const float *zx, *zy, *ux, *uy;  // state_in, pixel order            [P][H][W]
    const float* b;                  // H_t(xin), the path's layout
    float* v;                        // b + rho D^T (z0 - u0), pixel order
    float *uxo, *uyo;                // the loop's u input, the path's layout
    const float *lam, *rho;
    int H, W;
    int L;                           // lanes per row of the lane-paired layout; 0: pixel order
    int lgtx;                        // log2 of the pixel groups per block row
    unsigned rows;                   // P H
};

struct StateExportArgs {
    const float* x;                  // x_K, pixel order
    const float *uxp, *uyp;          // u_{K-1}, the path's layout (null: zero)
    float *zx, *zy, *ux, *uy;        // state_out, pixel order
    const float* nsq;                // iso: N_K = sum over planes of a^2   [2][H][W], pixel order
    float* part;                     // iso partials                        [groups][2][H][W]
    const float *lam, *rho;
    int H, W, L, lgtx;
    unsigned rows;
    int ppg;                         // iso: planes per partial group
    long long P;
};

// V consecutive floats
template <int V> struct fvec { float v[V]; };
template <int V> __device__ __forceinline__ fvec<V> ldv(const float* __restrict__ p) {
    fvec<V> r;
    if constexpr (V == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        r.v[0] = q.x, r.v[1] = q.y, r.v[2] = q.z, r.v[3] = q.w;
    } else if constexpr (V == 2) {
        const float2 q = *reinterpret_cast<const float2*>(p);
        r.v[0] = q.x, r.v[1] = q.y;
    } else {
        r.v[0] = *p;
    }
    return r;
}
template <int V> __device__ __forceinline__ void stv(float* __restrict__ p, const fvec<V>& r) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    else if constexpr (V == 2) *reinterpret_cast<float2*>(p) = make_float2(r.v[0], r.v[1]);
    else *p = r.v[0];
}

// float offset, inside a row, of pixel pair q in the lane-paired layout of L lanes: lane t = q % L holds the
// pairs t + L jj; the pairs jj = 2j', 2j' + 1 share the 16-byte slot t + L j' (ld_row / st_row)
__device__ __forceinline__ int pl_off(int q, int L) {
    const int t = q % L, jj = q / L;
    return 2 * (2 * (t + L * (jj >> 1)) + (jj & 1));
}
// V pixels from pixel j0 of a row in the path's layout (row: the row's first float)
template <int V> __device__ __forceinline__ fvec<V> ld_path(const float* __restrict__ row, int j0, int L) {
    if (L == 0) return ldv<V>(row + j0);
    fvec<V> r;
    if constexpr (V >= 2) {  // (a lane-paired row has an even number of pixels)
#pragma unroll
        for (int e = 0; e < V; e += 2) {
            const fvec<2> q = ldv<2>(row + pl_off((j0 + e) >> 1, L));
            r.v[e] = q.v[0], r.v[e + 1] = q.v[1];
        }
    } else {  // one pixel (a caller's pointer is only 4-byte aligned): its half of the pair's slot
        r.v[0] = row[pl_off(j0 >> 1, L) + (j0 & 1)];
    }
    return r;
}
template <int V> __device__ __forceinline__ void st_path(float* __restrict__ row, int j0, int L, const fvec<V>& r) {
    if (L == 0) {
        stv<V>(row + j0, r);
        return;
    }
    if constexpr (V >= 2) {
#pragma unroll
        for (int e = 0; e < V; e += 2) {
            fvec<2> q;
            q.v[0] = r.v[e], q.v[1] = r.v[e + 1];
            stv<2>(row + pl_off((j0 + e) >> 1, L), q);
        }
    } else {
        row[pl_off(j0 >> 1, L) + (j0 & 1)] = r.v[0];
    }
}

// the thread's (row, first pixel); false: outside the image
template <int V> __device__ __forceinline__ bool state_item(int lgtx, unsigned rows, int W, unsigned bx, unsigned& row, int& j0) {
    const unsigned tx = threadIdx.x & ((1u << lgtx) - 1u), ty = threadIdx.x >> lgtx;
    const unsigned long long r = (unsigned long long)bx * (256u >> lgtx) + ty;
    j0 = (int)((blockIdx.y << lgtx) + tx) * V;
    row = (unsigned)r;
    return r < rows && j0 < W;
}

template <int V> __global__ void __launch_bounds__(256) k_state_import(StateImportArgs a) {
    unsigned row;
    int j0;
    if (!state_item<V>(a.lgtx, a.rows, a.W, blockIdx.x, row, j0)) return;
    const int H = a.H, W = a.W;
    const int i = (int)(row % (unsigned)H);
    const size_t rb = (size_t)row * W;                                      // this row
    const size_t rd = (size_t)(row - (unsigned)i + (unsigned)(i == H - 1 ? 0 : i + 1)) * W;  // the row below
    const int jn = j0 + V >= W ? 0 : j0 + V;                                // the pixel right of the group
    const float rho = a.rho[0];
    const fvec<V> zx = ldv<V>(a.zx + rb + j0), ux = ldv<V>(a.ux + rb + j0);
    const fvec<V> zy = ldv<V>(a.zy + rb + j0), uy = ldv<V>(a.uy + rb + j0);
    const fvec<V> zyd = ldv<V>(a.zy + rd + j0), uyd = ldv<V>(a.uy + rd + j0);
    const float wxn = a.zx[rb + jn] - a.ux[rb + jn];
    const fvec<V> b = ld_path<V>(a.b + rb, j0, a.L);
    float wx[V + 1];
#pragma unroll
    for (int e = 0; e < V; ++e) wx[e] = zx.v[e] - ux.v[e];
    wx[V] = wxn;
    fvec<V> v;
#pragma unroll
    for (int e = 0; e < V; ++e) {
        const float wy = zy.v[e] - uy.v[e], wyd = zyd.v[e] - uyd.v[e];
        v.v[e] = fmat(rho, (wx[e] - wx[e + 1]) + (wy - wyd), b.v[e]);
    }
    stv<V>(a.v + rb + j0, v);
    st_path<V>(a.uxo + rb, j0, a.L, ux);
    st_path<V>(a.uyo + rb, j0, a.L, uy);
}

// a_x, a_y of the thread's pixels: D x_K + u_{K-1}
template <int V>
__device__ __forceinline__ void state_a(const StateExportArgs& a, unsigned row, int i, int j0, fvec<V>& ax, fvec<V>& ay) {
    const int H = a.H, W = a.W;
    const size_t rb = (size_t)row * W;
    const size_t ru = (size_t)(row - (unsigned)i + (unsigned)(i == 0 ? H - 1 : i - 1)) * W;  // the row above
    const fvec<V> x = ldv<V>(a.x + rb + j0), xu = ldv<V>(a.x + ru + j0);
    const float xl = a.x[rb + (j0 == 0 ? W - 1 : j0 - 1)];
    fvec<V> ux, uy;
    if (a.uxp) {
        ux = ld_path<V>(a.uxp + rb, j0, a.L);
        uy = ld_path<V>(a.uyp + rb, j0, a.L);
    } else {
#pragma unroll
        for (int e = 0; e < V; ++e) ux.v[e] = uy.v[e] = 0.f;
    }
#pragma unroll
    for (int e = 0; e < V; ++e) {
        ax.v[e] = (x.v[e] - (e == 0 ? xl : x.v[e > 0 ? e - 1 : 0])) + ux.v[e];
        ay.v[e] = (x.v[e] - xu.v[e]) + uy.v[e];
    }
}

template <int V, bool ISO> __global__ void __launch_bounds__(256) k_state_export(StateExportArgs a) {
    unsigned row;
    int j0;
    if (!state_item<V>(a.lgtx, a.rows, a.W, blockIdx.x, row, j0)) return;
    const int i = (int)(row % (unsigned)a.H);
    const size_t rb = (size_t)row * a.W;
    const float tau = a.lam[0] / a.rho[0];
    fvec<V> ax, ay, nx, ny, zx, zy, ux, uy;
    state_a<V>(a, row, i, j0, ax, ay);
    if constexpr (ISO) {
        const size_t hw = (size_t)i * a.W + j0;
        nx = ldv<V>(a.nsq + hw);
        ny = ldv<V>(a.nsq + (size_t)a.H * a.W + hw);
    }
#pragma unroll
    for (int e = 0; e < V; ++e) {
        zx.v[e] = shrink_z<ISO>(ax.v[e], tau, ISO ? nx.v[e] : 0.f);
        zy.v[e] = shrink_z<ISO>(ay.v[e], tau, ISO ? ny.v[e] : 0.f);
        ux.v[e] = ax.v[e] - zx.v[e];
        uy.v[e] = ay.v[e] - zy.v[e];
    }
    stv<V>(a.zx + rb + j0, zx);
    stv<V>(a.zy + rb + j0, zy);
    stv<V>(a.ux + rb + j0, ux);
    stv<V>(a.uy + rb + j0, uy);
}

// iso: part[g][0 | 1][H][W] = sum over the planes of group g of a_x^2 | a_y^2; grid.x = groups x row blocks
template <int V> __global__ void __launch_bounds__(256) k_state_iso_part(StateExportArgs a, unsigned rowblocks) {
    const unsigned g = blockIdx.x / rowblocks;
    unsigned i;
    int j0;
    if (!state_item<V>(a.lgtx, (unsigned)a.H, a.W, blockIdx.x % rowblocks, i, j0)) return;
    const long long p0 = (long long)g * a.ppg, p1 = min(a.P, p0 + a.ppg);
    fvec<V> sx, sy;
#pragma unroll
    for (int e = 0; e < V; ++e) sx.v[e] = sy.v[e] = 0.f;
    for (long long p = p0; p < p1; ++p) {
        fvec<V> ax, ay;
        state_a<V>(a, (unsigned)(p * a.H) + i, (int)i, j0, ax, ay);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            sx.v[e] = fmat(ax.v[e], ax.v[e], sx.v[e]);
            sy.v[e] = fmat(ay.v[e], ay.v[e], sy.v[e]);
        }
    }
    const size_t HW = (size_t)a.H * a.W, hw = (size_t)i * a.W + j0;
    stv<V>(a.part + (size_t)g * 2 * HW + hw, sx);
    stv<V>(a.part + (size_t)g * 2 * HW + HW + hw, sy);
}

// nsq[k] = sum over the groups of part[g][k], k < n (= 2 H W), in the groups' order: deterministic
static __global__ void __launch_bounds__(256) k_state_reduce(const float* __restrict__ part, float* __restrict__ nsq,
                                                             int groups, long long n) {
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    float s = 0.f;
    for (int g = 0; g < groups; ++g) s += part[(size_t)g * n + k];
    nsq[k] = s;
}

}  // namespace admm
