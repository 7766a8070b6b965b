// occ_state.hpp -- what more than one translation unit of the engine reads: the limits, the chains' scalars (ChainScalars, Ctl)
// and a few device functions -- expit, the covariate dot product, the wave sums of a double and of a 64-bit integer.  occ_kernels.hpp includes
// it; occ_spatial.hip is a unit of its own and includes nothing else of the kernels (occ_kernels.hpp defines kernels, which
// must exist once per library).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "occ_plan.hpp"

namespace occ {

constexpr int NACC_MAX = MAXC * (MAXC + 1) / 2 + MAXC;  // 44
constexpr int MAXG = 32;                            // OCC_MAX_COVARIATES: the generic path (P = 0 instantiations, run-time p and q)
constexpr int NACC_G = MAXG * (MAXG + 1) / 2 + MAXG;    // 560
constexpr int NSLOT = 4;
constexpr int MAX_WAVES = 4;  // threads per block <= 256

struct Ctl {
    uint32_t it;    // Gibbs iteration number (Philox counter word 2)
    uint32_t koff;  // Krylov launches already spent on the current eta solve by earlier graph replays:
                    // 0 normally; > 0 when a replay ran out of captured launches and the NEXT replay
                    // continues the same solve (no host involvement, same arithmetic)
};

// Control words are handed over between kernels, never updated in place: the kernels of launch
// sequence ("slot") number s read ctl[s & 1]; k_z_ob, the last kernel of the slot, writes ctl[(s+1) & 1];
// k_beta_partial publishes the carry decision of the slot in mid[s & 1].  No kernel reads a word that
// another block of the same kernel writes.
struct ChainScalars {
    double alpha[MAXG], beta[MAXG];
    double tau;
    double tau_gamma[2];       // the standard gamma variate of tau's draw of iteration t in [t & 1] (logit.py:209): it depends on
                               // nothing but (key, t), so k_noise draws it one iteration ahead, off the critical path
    double beta_eps[2][MAXG];  // likewise the p standard normals of beta's draw of iteration t in [t & 1] (distributions.pyx:95-96):
                               // block_normal(key, k, 0, t, STREAM_BETA), drawn by k_noise beside tau_gamma, read by every beta
                               // draw of a running chain (k_z_ob, k_z_ob_stats, k_beta_draw); the INJ kernels keep their own
    uint64_t key;
    Ctl ctl[2], mid[2];
    uint32_t it_stop, it_base, burnin, keep;
    uint32_t bar_base;         // arrivals counted so far by the chain's barrier counter (occ_iter.hpp), never reset
    int32_t err;               // OCC_E_* raised on device
    int32_t minres_itn_last;
    uint32_t site_on;          // OUT_SITE: per-site posterior sums (Ctx::site_acc) are kept for this chain; OUT_LL: the log-likelihood
                               // sums (Ctx::ll_acc); OUT_REGION: the occupied sites per region and draw (Ctx::occ_rec); OUT_PPC: the
                               // posterior predictive check (Ctx::ppc_rec) -- occ_plan.hpp; sits where the layout had padding
    unsigned long long krylov_total, krylov_sq_total, solves, carries;
};

static_assert(sizeof(ChainScalars) == 640 + 2 * MAXG * 8, "ChainScalars: the layout every kernel was compiled against");

__device__ __forceinline__ double expit(double x)
{
    if (x < 0.0) { const double e = exp(x); return e / (1.0 + e); }
    return 1.0 / (1.0 + exp(-x));
}
// expit(a) and 1 - expit(a), both from e = exp(-|a|).  The first performs the operations of expit() (exp(a) for a < 0,
// exp(-a) otherwise), so it has its bits.  The second is formed without cancellation: for a < 0, psi <= 1/2 and 1 - psi is
// exact to an ulp; for a >= 0 it is e psi = e / (1 + e), where 1 - psi would lose digits in proportion to 1 / (1 - psi)
// and be 0 from a = 36.74 on.  z_den: the likelihood D = (1 - psi) + num, num = psi P, of a site without a detection, which
// every z update divides by and the held-out score takes the logarithm of.  D <= 1; with P = 1 the rounded e psi + psi can
// be 1 + 2^-52 (1 - psi, subtracted, gave exactly 1), so it is held to 1: log D <= 0 as before.
__device__ __forceinline__ double expit_e(double a, double e) { return a < 0.0 ? e / (1.0 + e) : 1.0 / (1.0 + e); }
__device__ __forceinline__ double expit_c(double a, double e, double psi) { return a < 0.0 ? 1.0 - psi : e * psi; }
__device__ __forceinline__ double z_den(double a, double e, double psi, double num) { return fmin(expit_c(a, e, psi) + num, 1.0); }

// x_i . coef over the structure-of-arrays design (explicit contractions: every caller evaluates the same operations)
__device__ __forceinline__ double xdot(const double *Xt, int n, int i, const double *coef, int p)
{
    double acc = 0.0;
    for (int a = 0; a < p; ++a) acc = fma(Xt[(size_t)a * n + i], coef[a], acc);
    return acc;
}

// The wave-level sum of a double (the reductions of occ_kernels.hpp say why DPP and why this order); occ_comp.hip adds a
// component's chunk sums with it.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_shifted(double v)
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, ROW_MASK, 0xf, false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ double wave_sum(double v)
{
    v += dpp_shifted<0xB1, 0xf>(v);   // quad_perm [1,0,3,2]
    v += dpp_shifted<0x4E, 0xf>(v);   // quad_perm [2,3,0,1]
    v += dpp_shifted<0x141, 0xf>(v);  // row_half_mirror
    v += dpp_shifted<0x140, 0xf>(v);  // row_mirror: every lane of a 16-lane row holds the row sum
    v += dpp_shifted<0x142, 0xa>(v);  // row_bcast:15 into rows 1 and 3
    v += dpp_shifted<0x143, 0xc>(v);  // row_bcast:31 into rows 2 and 3: lane 63 holds the wave sum
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)b, 63), hi = __builtin_amdgcn_readlane((int)(b >> 32), 63);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);  // uniform
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned long long dpp_shifted_u64(unsigned long long b)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)b, CTRL, ROW_MASK, 0xf, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), CTRL, ROW_MASK, 0xf, false);
    return ((unsigned long long)hi << 32) | lo;
}
// wave_sum's levels on 64-bit integers; the total is uniform (lane 63's)
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v)
{
    v += dpp_shifted_u64<0xB1, 0xf>(v);
    v += dpp_shifted_u64<0x4E, 0xf>(v);
    v += dpp_shifted_u64<0x141, 0xf>(v);
    v += dpp_shifted_u64<0x140, 0xf>(v);
    v += dpp_shifted_u64<0x142, 0xa>(v);
    v += dpp_shifted_u64<0x143, 0xc>(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, 63);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), 63);
    return ((unsigned long long)hi << 32) | lo;
}

}  // namespace occ
