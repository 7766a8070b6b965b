// occ_spatial.hip -- the two kernels of the spatial residual check and their launcher (occ_spatial.hpp; DESIGN.md section
// 19).  A translation unit of its own, linked into libocc_gibbs.so: it shares occ_state.hpp and occ_rng.hpp with the
// engine's unit and none of its kernels.
#include "occ_spatial.hpp"

namespace occ {

__device__ __forceinline__ unsigned long long sp_fx(double x) { return (unsigned long long)__double2ll_rn(x * 0x1.0p32); }

// The row of SpArgs::rec that the sequence of parity e adds to, or null; *it: the iteration.  Uniform over the chain.
// The kernels of sequence e read ChainScalars::ctl[e]; its z update, the kernel in front of these two, read mid[e] -- the same
// iteration number `it`, with the carry decision -- and left ctl[e ^ 1]: it + 1 if it completed iteration `it`, and `it`
// itself (with its koff) if the chain idled -- past it_stop, err set, or a solve carried to the next replay (koff > 0).  So
// ctl[e ^ 1].it == ctl[e].it + 1 says "completed"; err (which the z update itself may have raised) is asked again; and
// it_base, burnin, keep give the window exactly as record_draws reads it: 0 <= it - it_base - burnin < keep.
__device__ __forceinline__ long long *sp_row(const SpArgs &a, const ChainScalars &sc, int chain, int e, uint32_t *it)
{
    const uint32_t t = sc.ctl[e].it, after = sc.ctl[e ^ 1].it;
    const uint32_t rel = t - sc.it_base;
    *it = t;
    if (a.on[chain] == 0u || a.rec == nullptr || after != t + 1u || sc.err != 0 || rel < sc.burnin || rel - sc.burnin >= sc.keep) return nullptr;
    return a.rec + ((size_t)chain * sc.keep + (rel - sc.burnin)) * (size_t)SP_NCOL;
}

__global__ void __launch_bounds__(256) k_sp_resid(const SpArgs a, const ChainScalars *__restrict__ scs, int e)
{
    const int chain = blockIdx.y;
    const ChainScalars &sc = scs[chain];
    uint32_t it;
    if (sp_row(a, sc, chain, e, &it) == nullptr) return;
    const int n = a.n, i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n) return;
    const double psi = expit(xdot(a.Xt, n, i, sc.beta, a.p) + a.eta[(size_t)chain * n + i]);
    const double u = block_uniform(sc.key, (uint32_t)i, 0, it, STREAM_SPATIAL);
    const double zi = a.z[(size_t)chain * n + i] ? 1.0 : 0.0, zr = (u < psi) ? 1.0 : 0.0;
    a.res[(size_t)chain * n + i] = make_double2(zi - psi, zr - psi);
}

// The reduction has the shape of ppc_count: a wave's sums by DPP, the workgroup's in LDS, then one 64-bit integer add to
// device memory per column.  The guard is uniform over the chain, so a workgroup leaves as a whole or not at all: no thread
// leaves between it and the barriers (one past n carries zeros).
__global__ void __launch_bounds__(256) k_sp_moran(const SpArgs a, const ChainScalars *__restrict__ scs, int e)
{
    __shared__ unsigned long long s_sum[SP_NCOL];
    const int chain = blockIdx.y;
    uint32_t it;
    long long *row = sp_row(a, scs[chain], chain, e, &it);
    if (row == nullptr) return;
    if (threadIdx.x < SP_NCOL) s_sum[threadIdx.x] = 0ull;
    __syncthreads();
    const int n = a.n, i = (int)(blockIdx.x * 256u + threadIdx.x);
    unsigned long long term[SP_NCOL] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    if (i < n) {
        const double2 *__restrict__ res = a.res + (size_t)chain * n;
        const double2 ri = res[i];
        double d = 0.0, s = 0.0, sr = 0.0;
        for (int k = a.ptr[i], k1 = a.ptr[i + 1]; k < k1; ++k) {
            const double w = a.val[k];
            const double2 rj = res[a.col[k]];
            d += w;
            s = fma(w, rj.x, s);
            sr = fma(w, rj.y, sr);
        }
        term[SP_A] = sp_fx(ri.x * s), term[SP_B] = sp_fx(d * ri.x), term[SP_C] = sp_fx(ri.x), term[SP_D] = sp_fx(ri.x * ri.x);
        term[4 + SP_A] = sp_fx(ri.y * sr), term[4 + SP_B] = sp_fx(d * ri.y), term[4 + SP_C] = sp_fx(ri.y), term[4 + SP_D] = sp_fx(ri.y * ri.y);
    }
    unsigned long long w[SP_NCOL];
#pragma unroll
    for (int k = 0; k < SP_NCOL; ++k) w[k] = wave_sum_u64(term[k]);
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (int k = 0; k < SP_NCOL; ++k)
            if (w[k] != 0ull) atomicAdd(&s_sum[k], w[k]);
    }
    __syncthreads();
    if (threadIdx.x < SP_NCOL) {
        const unsigned long long v = s_sum[threadIdx.x];
        if (v != 0ull) atomicAdd((unsigned long long *)row + threadIdx.x, v);
    }
}

void sp_launch(const SpArgs &a, const ChainScalars *scs, int C, int e, hipStream_t st)
{
    const dim3 grid((unsigned)((a.n + 255) / 256), (unsigned)C);
    hipLaunchKernelGGL(k_sp_resid, grid, dim3(256), 0, st, a, scs, e);
    hipLaunchKernelGGL(k_sp_moran, grid, dim3(256), 0, st, a, scs, e);
}

}  // namespace occ
