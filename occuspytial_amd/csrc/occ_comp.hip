// occ_comp.hip -- the kernels of the per-component sum-to-zero pass (occ_comp.hpp).  A translation unit
// of its own inside libocc_gibbs.so, like occ_spatial.hip: it includes nothing of occ_kernels.hpp.
#include "occ_comp.hpp"

namespace occ {

namespace {

// The kernels of sequence e read mid[e], which the solve's last kernel (k_iter, k_tiles, k_beta_partial) published: ctl[e] with
// the carry decision.  Idle: past it_stop, err set, or the solve goes on in the next replay -- the question k_z_ob asks.
__device__ __forceinline__ bool comp_idle(const ChainScalars &sc, int e)
{
    const Ctl ctl = sc.mid[e];
    return ctl.koff || ctl.it >= sc.it_stop || sc.err != 0;
}

}  // namespace

// grid (ceil(nchunk / 256), chains)
__global__ void __launch_bounds__(256) k_comp_part(const CompArgs a, const ChainScalars *__restrict__ scs, int chain_base, int e)
{
    const int chain = chain_base + (int)blockIdx.y, j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (comp_idle(scs[chain], e) || j >= a.nchunk) return;
    const int b = a.chunk_start[j], end = a.chunk_start[j + 1];
    const double2 *xv = a.Xv + (size_t)chain * a.n;
    double sx = 0.0, sz = 0.0;
#pragma unroll 8
    for (int t = b; t < end; ++t) {
        const double2 v = xv[a.list[t]];
        sx += v.x;
        sz += v.y;
    }
    double *out = a.part + 2 * ((size_t)chain * a.nchunk + j);
    out[0] = sx;
    out[1] = sz;
}

// grid (ceil(k / 256) + ceil(nheavy / 4), chains): blocks of one thread per component, then blocks of one wave per heavy one
__global__ void __launch_bounds__(256) k_comp_coef(const CompArgs a, const ChainScalars *__restrict__ scs, int chain_base, int e)
{
    const int chain = chain_base + (int)blockIdx.y;
    if (comp_idle(scs[chain], e)) return;
    const double *part = a.part + 2 * (size_t)chain * a.nchunk;
    double *coef = a.coef + (size_t)chain * a.k;
    const int nb_light = (a.k + 255) / 256;
    if ((int)blockIdx.x < nb_light) {
        const int comp = (int)(blockIdx.x * 256 + threadIdx.x);
        if (comp >= a.k) return;
        const int c0 = a.comp_chunk[comp], c1 = a.comp_chunk[comp + 1];
        if (c1 - c0 > COMP_LIGHT) return;                        // a wave's, below
        if (a.chunk_start[c1] - a.chunk_start[c0] == 1) return;  // one site: eta is 0.0, no coefficient
        double sx = 0.0, sz = 0.0;
#pragma unroll 8
        for (int j = c0; j < c1; ++j) {
            sx += part[2 * j];
            sz += part[2 * j + 1];
        }
        coef[comp] = -sx / sz;
        return;
    }
    const int lane = threadIdx.x & 63, h = ((int)blockIdx.x - nb_light) * 4 + (int)(threadIdx.x >> 6);
    if (h >= a.nheavy) return;  // (uniform over the wave)
    const int comp = a.heavy[h], c0 = a.comp_chunk[comp], c1 = a.comp_chunk[comp + 1];
    double sx = 0.0, sz = 0.0;
    for (int j0 = c0; j0 < c1; j0 += 64) {  // (uniform trip count: a lane past the end adds nothing)
        const int j = j0 + lane;
        if (j < c1) {
            sx += part[2 * j];
            sz += part[2 * j + 1];
        }
    }
    sx = wave_sum(sx);
    sz = wave_sum(sz);
    if (lane == 0) coef[comp] = -sx / sz;
}

// grid (ceil(n / 256), chains)
__global__ void __launch_bounds__(256) k_comp_eta(const CompArgs a, const ChainScalars *__restrict__ scs, int chain_base, int e)
{
    const int chain = chain_base + (int)blockIdx.y, i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (comp_idle(scs[chain], e) || i >= a.n) return;
    const size_t ci = (size_t)chain * a.n + i;
    const uint32_t lab = a.site_lab[i];
    const double2 xz = a.Xv[ci];
    // (eta_project of occ_kernels.hpp: one fma)
    a.eta[ci] = (lab & COMP_SINGLE) ? 0.0 : fma(a.coef[(size_t)chain * a.k + lab], xz.y, xz.x);
}

void comp_launch(const CompArgs &a, const ChainScalars *scs, CompStage stage, int chain_base, int chains, int e, hipStream_t st)
{
    const unsigned C = (unsigned)chains;
    switch (stage) {
        case COMP_PART: hipLaunchKernelGGL(k_comp_part, dim3((unsigned)((a.nchunk + 255) / 256), C), dim3(256), 0, st, a, scs, chain_base, e); break;
        case COMP_COEF:
            hipLaunchKernelGGL(k_comp_coef, dim3((unsigned)((a.k + 255) / 256 + (a.nheavy + 3) / 4), C), dim3(256), 0, st, a, scs, chain_base, e);
            break;
        case COMP_ETA: hipLaunchKernelGGL(k_comp_eta, dim3((unsigned)((a.n + 255) / 256), C), dim3(256), 0, st, a, scs, chain_base, e); break;
    }
}

}  // namespace occ
