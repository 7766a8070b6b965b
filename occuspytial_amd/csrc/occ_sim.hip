// occ_sim.hip -- libocc_sim.so, the C ABI of include/occ_sim.h: realisations of the intrinsic CAR field x ~ N(0, Q^+)
// (occuspytial_amd/simulate.py drives it).
//
//   u = B'eps   k_sim_draw: gather form of the edge-form prior term (stream ETA_EDGE, it = draw number) -- both endpoints of
//               an edge regenerate its normal, no atomic
//   x = Q^+ u   Jacobi-preconditioned conjugate gradients from x = 0 on the b columns at once, z = r / d never stored:
//                 k_sim_start, k_sim_scal_start      x = 0, r = u, p = r / d;  r'z, ||u||^2;  done_c = (u_c = 0)
//               one step, five launches:
//                 k_sim_spmv<0>                      Qp, the tiles' partial sums of p'Qp
//                 k_sim_scal_alpha                   alpha_c = r'z / p'Qp  (0 for a column that is done)
//                 k_sim_update                       x += alpha p, r -= alpha Qp;  the tiles' partial sums of r'z and r'r
//                 k_sim_scal_beta                    done_c where ||r_c|| <= tol ||u_c||;  beta_c = r'z / (old r'z)
//                 k_sim_dir                          p = r / d + beta p
//               k_sim_spmv<1>, k_sim_scal_res        the true residual || u - Q x || / || u || from scratch
//               k_sim_comp_chunk, _mean, _apply      x minus its component's mean, twice (the second pass takes off the
//                                                    rounding of the first): the minimum-norm solution
// Blocks are n x ld row-major, ld a multiple of 16: 16 consecutive doubles of a row are one 128-byte line, which is what a
// quarter-wave loads.  A workgroup of the n-sized kernels owns one TILE of 256 sites and 16 columns: thread t has column
// t % 16 and the sites (t / 16) + 16 r, r = 0 .. 15, adds its own terms in that order, and the 16 threads of a column are
// added in thread order through LDS; the scalar kernels add the tiles in tile order.  So every sum has one fixed order that
// depends neither on b nor on a grid nor on timing: a column is a CG of its own, and its bits are (Q, key, draw, tol)'s.
// No kernel waits on the device, none uses an atomic.  alpha, beta, r'z, ||r||^2 and done stay on the device; the host
// reads only the done flags, every check_every iterations.  The handle's device, stream, allocations, deadline wait and
// create / destroy are occ_handle.hpp's.
#include "../../include/occ_sim.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "occ_handle.hpp"
#include "occ_rng.hpp"
#include "occ_sim_plan.hpp"

namespace occ_sim_impl {

constexpr int TS = occ::SIM_TILE;

// the site r of thread-row sq in tile `tile` (consecutive sq: consecutive sites, so consecutive SELL slots)
__device__ __forceinline__ int tile_site(int tile, int sq, int r) { return tile * TS + sq + 16 * r; }

// the 16 threads of column cl, added in thread order; the result is thread-row 0's
__device__ __forceinline__ double tile_sum(double v, double (*s)[16], int sq, int cl)
{
    s[sq][cl] = v;
    __syncthreads();
    double t = 0.0;
    if (sq == 0) {
#pragma unroll
        for (int g = 0; g < 16; ++g) t += s[g][cl];
    }
    __syncthreads();
    return t;
}

// the tiles' partial sums of column c, added in tile order from 0.0 (32 loads in flight at a time: the additions are a chain,
// the loads need not be)
__device__ __forceinline__ double tiles_in_order(const double *__restrict__ part, int ntile, int ld, int c)
{
    double acc = 0.0;
    int t = 0;
    for (; t + 32 <= ntile; t += 32) {
        double v[32];
#pragma unroll
        for (int k = 0; k < 32; ++k) v[k] = part[(size_t)(t + k) * ld + c];
#pragma unroll
        for (int k = 0; k < 32; ++k) acc += v[k];
    }
    for (; t < ntile; ++t) acc += part[(size_t)t * ld + c];
    return acc;
}

// U[i][c] = sum over the row's off-diagonals, in column order from 0.0, of sgn_root * N(key; min(i,j), max(i,j), first + c)
__global__ void __launch_bounds__(256) k_sim_draw(double *__restrict__ U, const int *__restrict__ sell_ptr, const int *__restrict__ sell_col,
                                                  const double *__restrict__ sgn_root, int ell_w, uint64_t key, uint32_t first, int n, int ld, int b)
{
    const int cl = (int)threadIdx.x & 15, sq = (int)threadIdx.x >> 4, c = (int)blockIdx.y * 16 + cl;
    for (int r = 0; r < 16; ++r) {
        const int i = tile_site((int)blockIdx.x, sq, r);
        if (i >= n) break;
        const int sl = i >> 6, lane = i & 63;
        const int base = ell_w ? sl * ell_w * 64 : sell_ptr[sl];
        const int width = ell_w ? ell_w : (sell_ptr[sl + 1] - base) / 64;
        double acc = 0.0;
        if (c < b) {
            for (int k = 0; k < width; ++k) {
                const int slot = base + k * 64 + lane;
                const double sw = sgn_root[slot];
                if (sw == 0.0) continue;  // (padding, or a stored zero)
                const int j = sell_col[slot];
                const double e = occ::block_normal(key, (uint32_t)min(i, j), (uint32_t)max(i, j), first + (uint32_t)c, occ::STREAM_ETA_EDGE);
                acc = __dadd_rn(acc, __dmul_rn(sw, e));
            }
        }
        U[(size_t)i * ld + c] = acc;  // (columns b .. bc - 1: zeros)
    }
}

// x = 0, r = u, p = r / d;  part_rz, part_rr: the tile's sums of r'z and r'r
__global__ void __launch_bounds__(256) k_sim_start(const double *__restrict__ U, const double *__restrict__ dinv, double *__restrict__ X, double *__restrict__ R,
                                                   double *__restrict__ P, double *__restrict__ part_rz, double *__restrict__ part_rr, int n, int ld)
{
    __shared__ double s[16][16];
    const int cl = (int)threadIdx.x & 15, sq = (int)threadIdx.x >> 4, c = (int)blockIdx.y * 16 + cl;
    double prz = 0.0, prr = 0.0;
    for (int r = 0; r < 16; ++r) {
        const int i = tile_site((int)blockIdx.x, sq, r);
        if (i >= n) break;
        const size_t at = (size_t)i * ld + c;
        const double u = U[at], z = dinv[i] * u;
        X[at] = 0.0;
        R[at] = u;
        P[at] = z;
        prz = fma(u, z, prz);
        prr = fma(u, u, prr);
    }
    const double a = tile_sum(prz, s, sq, cl), e = tile_sum(prr, s, sq, cl);
    if (sq == 0) {
        part_rz[(size_t)blockIdx.x * ld + c] = a;
        part_rr[(size_t)blockIdx.x * ld + c] = e;
    }
}

__global__ void __launch_bounds__(64) k_sim_scal_start(const double *__restrict__ part_rz, const double *__restrict__ part_rr, double *__restrict__ rz,
                                                       double *__restrict__ rr, double *__restrict__ rr0, double *__restrict__ alpha,
                                                       double *__restrict__ beta, int *__restrict__ done, int *__restrict__ iters, int ntile, int ld, int bc)
{
    const int c = (int)threadIdx.x;
    if (c >= bc) return;
    const double a = tiles_in_order(part_rz, ntile, ld, c), e = tiles_in_order(part_rr, ntile, ld, c);
    rz[c] = a;
    rr[c] = e;
    rr0[c] = e;
    alpha[c] = 0.0;
    beta[c] = 0.0;
    done[c] = e > 0.0 ? 0 : 1;  // (u_c = 0: done at once, x_c = 0)
    iters[c] = 0;
}

// MODE 0: out = Q src, part = the tile's sum of src . out (a column that is done is left alone);
// MODE 1: nothing is stored, part = the tile's sum of (U - Q src)^2
template <int MODE>
__global__ void __launch_bounds__(256) k_sim_spmv(const double *__restrict__ src, double *__restrict__ out, const double *__restrict__ U,
                                                  const double *__restrict__ diag, const int *__restrict__ sell_ptr, const int *__restrict__ sell_col,
                                                  const double *__restrict__ sell_val, int ell_w, const int *__restrict__ done, double *__restrict__ part,
                                                  int n, int ld)
{
    __shared__ double s[16][16];
    const int cl = (int)threadIdx.x & 15, sq = (int)threadIdx.x >> 4, c = (int)blockIdx.y * 16 + cl;
    const bool live = MODE == 1 || done[c] == 0;
    double ps = 0.0;
    for (int r = 0; r < 16; ++r) {
        const int i = tile_site((int)blockIdx.x, sq, r);
        if (i >= n || !live) break;
        const int sl = i >> 6, lane = i & 63;
        const int base = ell_w ? sl * ell_w * 64 : sell_ptr[sl];
        const int width = ell_w ? ell_w : (sell_ptr[sl + 1] - base) / 64;
        const size_t at = (size_t)i * ld + c;
        const double v = src[at];
        double acc = diag[i] * v;
        for (int k = 0; k < width; ++k) {
            const int slot = base + k * 64 + lane;
            acc = fma(sell_val[slot], src[(size_t)sell_col[slot] * ld + c], acc);
        }
        if (MODE == 0) {
            out[at] = acc;
            ps = fma(v, acc, ps);
        } else {
            const double d = U[at] - acc;
            ps = fma(d, d, ps);
        }
    }
    const double t = tile_sum(ps, s, sq, cl);
    if (sq == 0) part[(size_t)blockIdx.x * ld + c] = t;
}

__global__ void __launch_bounds__(64) k_sim_scal_alpha(const double *__restrict__ part, const double *__restrict__ rz, const int *__restrict__ done,
                                                       double *__restrict__ alpha, int ntile, int ld, int bc)
{
    const int c = (int)threadIdx.x;
    if (c >= bc) return;
    const double pap = tiles_in_order(part, ntile, ld, c);
    alpha[c] = (done[c] == 0 && pap > 0.0) ? rz[c] / pap : 0.0;
}

// x += alpha p, r -= alpha Qp;  part_rz, part_rr: the tile's sums of r'z (z = r / d) and r'r
__global__ void __launch_bounds__(256) k_sim_update(double *__restrict__ X, double *__restrict__ R, const double *__restrict__ P, const double *__restrict__ AP,
                                                    const double *__restrict__ dinv, const double *__restrict__ alpha, const int *__restrict__ done,
                                                    double *__restrict__ part_rz, double *__restrict__ part_rr, int n, int ld)
{
    __shared__ double s[16][16];
    const int cl = (int)threadIdx.x & 15, sq = (int)threadIdx.x >> 4, c = (int)blockIdx.y * 16 + cl;
    const bool live = done[c] == 0;
    const double a = alpha[c];
    double prz = 0.0, prr = 0.0;
    for (int r = 0; r < 16; ++r) {
        const int i = tile_site((int)blockIdx.x, sq, r);
        if (i >= n || !live) break;
        const size_t at = (size_t)i * ld + c;
        X[at] = fma(a, P[at], X[at]);
        const double rn = fma(-a, AP[at], R[at]);
        R[at] = rn;
        prz = fma(rn, dinv[i] * rn, prz);
        prr = fma(rn, rn, prr);
    }
    const double t1 = tile_sum(prz, s, sq, cl), t2 = tile_sum(prr, s, sq, cl);
    if (sq == 0) {
        part_rz[(size_t)blockIdx.x * ld + c] = t1;
        part_rr[(size_t)blockIdx.x * ld + c] = t2;
    }
}

// iteration `it` of column c ends: done where ||r|| <= tol ||u|| (tol2 = tol^2), else beta = new r'z / old r'z
__global__ void __launch_bounds__(64) k_sim_scal_beta(const double *__restrict__ part_rz, const double *__restrict__ part_rr, double *__restrict__ rz,
                                                      double *__restrict__ rr, const double *__restrict__ rr0, double *__restrict__ alpha,
                                                      double *__restrict__ beta, int *__restrict__ done, int *__restrict__ iters, double tol2, int it,
                                                      int ntile, int ld, int bc)
{
    const int c = (int)threadIdx.x;
    if (c >= bc || done[c] != 0) return;  // (alpha = beta = 0 since the iteration in which it was done)
    const double a = tiles_in_order(part_rz, ntile, ld, c), e = tiles_in_order(part_rr, ntile, ld, c);
    rr[c] = e;
    if (e <= tol2 * rr0[c]) {
        done[c] = 1;
        iters[c] = it;
        alpha[c] = 0.0;
        beta[c] = 0.0;
    } else {
        beta[c] = a / rz[c];
        rz[c] = a;
        iters[c] = it;
    }
}

// p = r / d + beta p
__global__ void __launch_bounds__(256) k_sim_dir(double *__restrict__ P, const double *__restrict__ R, const double *__restrict__ dinv,
                                                 const double *__restrict__ beta, const int *__restrict__ done, int n, int ld)
{
    const int cl = (int)threadIdx.x & 15, sq = (int)threadIdx.x >> 4, c = (int)blockIdx.y * 16 + cl;
    if (done[c] != 0) return;
    const double bt = beta[c];
    for (int r = 0; r < 16; ++r) {
        const int i = tile_site((int)blockIdx.x, sq, r);
        if (i >= n) break;
        const size_t at = (size_t)i * ld + c;
        P[at] = fma(bt, P[at], dinv[i] * R[at]);
    }
}

__global__ void __launch_bounds__(64) k_sim_scal_res(const double *__restrict__ part, const double *__restrict__ rr0, double *__restrict__ res, int ntile,
                                                     int ld, int bc)
{
    const int c = (int)threadIdx.x;
    if (c >= bc) return;
    const double e = tiles_in_order(part, ntile, ld, c);
    res[c] = rr0[c] > 0.0 ? sqrt(e / rr0[c]) : 0.0;
}

// ---- centring on every component (occ_comp_plan.hpp's tables; a fixed order of addition: a chunk's sites from 0.0 left to
// right, then a component's chunks from 0.0 left to right) -------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_sim_comp_chunk(const double *__restrict__ X, const int *__restrict__ list, const int *__restrict__ chunk_start,
                                                        double *__restrict__ chunk_sum, int nchunk, int ld)
{
    const int cl = (int)threadIdx.x & 15, c = (int)blockIdx.y * 16 + cl;
    const int j = (int)blockIdx.x * 16 + ((int)threadIdx.x >> 4);
    if (j >= nchunk) return;
    double sum = 0.0;
    for (int t = chunk_start[j]; t < chunk_start[j + 1]; ++t) sum += X[(size_t)list[t] * ld + c];
    chunk_sum[(size_t)j * ld + c] = sum;
}

__global__ void __launch_bounds__(256) k_sim_comp_mean(const double *__restrict__ chunk_sum, const int *__restrict__ comp_chunk, const int *__restrict__ comp_size,
                                                       double *__restrict__ mean, int k, int ld)
{
    const int cl = (int)threadIdx.x & 15, c = (int)blockIdx.y * 16 + cl;
    const int m = (int)blockIdx.x * 16 + ((int)threadIdx.x >> 4);
    if (m >= k) return;
    double sum = 0.0;
    for (int j = comp_chunk[m]; j < comp_chunk[m + 1]; ++j) sum += chunk_sum[(size_t)j * ld + c];
    mean[(size_t)m * ld + c] = sum / (double)comp_size[m];
}

// (a site alone in its component: exactly 0.0)
__global__ void __launch_bounds__(256) k_sim_comp_apply(double *__restrict__ X, const uint32_t *__restrict__ site_lab, const double *__restrict__ mean, int n,
                                                        int ld)
{
    const int cl = (int)threadIdx.x & 15, sq = (int)threadIdx.x >> 4, c = (int)blockIdx.y * 16 + cl;
    for (int r = 0; r < 16; ++r) {
        const int i = tile_site((int)blockIdx.x, sq, r);
        if (i >= n) break;
        const uint32_t lab = site_lab[i];
        const size_t at = (size_t)i * ld + c;
        X[at] = (lab & occ::COMP_SINGLE) ? 0.0 : X[at] - mean[(size_t)(lab & ~occ::COMP_SINGLE) * ld + c];
    }
}

}  // namespace occ_sim_impl

using namespace occ_sim_impl;

struct occ_sim : occ::HandleBase {
    int n = 0, ld = 0, b = 0, b_max = 0, ell_w = 0, nslice = 0, ntile = 0, k = 0, nchunk = 0;
    bool have_u = false;
    int *sell_ptr = nullptr, *sell_col = nullptr, *list = nullptr, *chunk_start = nullptr, *comp_chunk = nullptr, *comp_size = nullptr;
    uint32_t *site_lab = nullptr;
    double *sell_val = nullptr, *sgn_root = nullptr, *diag = nullptr, *dinv = nullptr;
    double *X = nullptr, *U = nullptr, *R = nullptr, *P = nullptr, *AP = nullptr;
    double *part_a = nullptr, *part_b = nullptr, *chunk_sum = nullptr, *mean = nullptr;
    double *rz = nullptr, *rr = nullptr, *rr0 = nullptr, *alpha = nullptr, *beta = nullptr, *res = nullptr;
    int *done = nullptr, *iters = nullptr;
    int *host_flags = nullptr;   // pinned: done[ld], then iters[ld]
    double *host_res = nullptr;  // pinned: res[ld]
};
OCC_HANDLE_CODES(OCC_SIM_OK, OCC_SIM_E_BADARG, OCC_SIM_E_HIP);

static thread_local std::string g_create_err;

extern "C" {

int32_t occ_sim_version(void) { return OCC_SIM_VERSION; }

const char *occ_sim_last_error(const occ_sim *h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int occ_sim_destroy(occ_sim *h) { return occ::handle_destroy(h, "occ_sim_destroy"); }

static int create_impl(occ_sim *h, int64_t n64, const int32_t *indptr, const int32_t *indices, const double *qdata, const int32_t *labels, int32_t b_max,
                       int32_t device)
{
    std::string why;
    if (!occ::sim_check_sizes(n64, b_max, &why)) H_ARG(false, why);
    H_ARG(indptr && indices && qdata && labels, "null input");
    const int n = (int)n64;
    std::vector<int32_t> ip(indptr, indptr + n + 1);
    if (!occ::layout_q_indptr(n, ip, &why)) H_ARG(false, why);
    std::vector<int32_t> ix(indices, indices + ip[n]);
    std::vector<double> qd(qdata, qdata + ip[n]);
    std::vector<int32_t> lab(labels, labels + n);
    occ::SimPlan S;
    if (!occ::sim_plan_build(n64, ip, ix, qd, lab, b_max, &S, &why)) H_ARG(false, why);
    if (!occ::sim_plan_ok(lab, S, &why)) H_ARG(false, std::string("internal: the plan is wanting: ") + why);
    h->n = n;
    h->b_max = b_max;
    h->ld = S.ld;
    h->ell_w = S.ell_w;
    h->nslice = S.nslice;
    h->ntile = S.ntile;
    h->k = S.comp.k;
    h->nchunk = S.comp.nchunk();

    int rc;
    if ((rc = h->open(device)) != OCC_SIM_OK) return rc;
    if ((rc = h->upload(&h->sell_ptr, S.sell_ptr)) != OCC_SIM_OK) return rc;
    if ((rc = h->upload(&h->sell_col, S.sell_col)) != OCC_SIM_OK) return rc;
    if ((rc = h->upload(&h->sell_val, S.sell_val)) != OCC_SIM_OK) return rc;
    if ((rc = h->upload(&h->sgn_root, S.sgn_root)) != OCC_SIM_OK) return rc;
    if ((rc = h->upload(&h->diag, S.diag)) != OCC_SIM_OK) return rc;
    if ((rc = h->upload(&h->dinv, S.diag_inv)) != OCC_SIM_OK) return rc;
    if ((rc = h->upload(&h->list, S.comp.list)) != OCC_SIM_OK) return rc;
    if ((rc = h->upload(&h->chunk_start, S.comp.chunk_start)) != OCC_SIM_OK) return rc;
    if ((rc = h->upload(&h->comp_chunk, S.comp.comp_chunk)) != OCC_SIM_OK) return rc;
    if ((rc = h->upload(&h->comp_size, S.comp_size)) != OCC_SIM_OK) return rc;
    if ((rc = h->upload(&h->site_lab, S.comp.site_lab)) != OCC_SIM_OK) return rc;
    const size_t ld = (size_t)h->ld;
    for (double **bp : {&h->X, &h->U, &h->R, &h->P, &h->AP})
        if ((rc = h->alloc(bp, (size_t)n * ld, true)) != OCC_SIM_OK) return rc;
    if ((rc = h->alloc(&h->part_a, (size_t)h->ntile * ld, false)) != OCC_SIM_OK) return rc;
    if ((rc = h->alloc(&h->part_b, (size_t)h->ntile * ld, false)) != OCC_SIM_OK) return rc;
    if ((rc = h->alloc(&h->chunk_sum, (size_t)std::max(h->nchunk, 1) * ld, false)) != OCC_SIM_OK) return rc;
    if ((rc = h->alloc(&h->mean, (size_t)std::max(h->k, 1) * ld, false)) != OCC_SIM_OK) return rc;
    for (double **sp : {&h->rz, &h->rr, &h->rr0, &h->alpha, &h->beta, &h->res})
        if ((rc = h->alloc(sp, ld, true)) != OCC_SIM_OK) return rc;
    if ((rc = h->alloc(&h->done, ld, true)) != OCC_SIM_OK) return rc;
    if ((rc = h->alloc(&h->iters, ld, true)) != OCC_SIM_OK) return rc;
    if ((rc = h->alloc_pinned(&h->host_flags, 2 * ld)) != OCC_SIM_OK) return rc;
    if ((rc = h->alloc_pinned(&h->host_res, ld)) != OCC_SIM_OK) return rc;
    H_WAIT("occ_sim_create");
    return OCC_SIM_OK;
}

int occ_sim_create(int64_t n, const int32_t *q_indptr, const int32_t *q_indices, const double *q_data, const int32_t *labels, int32_t b_max,
                   int32_t device, occ_sim **out)
{
    return occ::handle_create(out, g_create_err, "occ_sim_destroy",
                              [&](occ_sim *h) { return create_impl(h, n, q_indptr, q_indices, q_data, labels, b_max, device); });
}

int occ_sim_info(const occ_sim *h, double *info6)
{
    if (!h || !info6) return OCC_SIM_E_BADARG;
    info6[0] = h->ell_w;
    info6[1] = h->ld;
    info6[2] = h->ntile;
    info6[3] = h->k;
    info6[4] = h->b;
    info6[5] = h->nchunk;
    return OCC_SIM_OK;
}

int occ_sim_draw(occ_sim *h, uint64_t key, int64_t first, int32_t b)
{
    if (!h) return OCC_SIM_E_BADARG;
    std::string why;
    if (!occ::sim_check_draw(first, b, h->b_max, &why)) H_ARG(false, why);
    H_TRY(hipSetDevice(h->device));
    const int bc = occ::sim_bc(b);
    h->have_u = false;
    hipLaunchKernelGGL(k_sim_draw, dim3(h->ntile, bc / 16), dim3(256), 0, h->st, h->U, (const int *)h->sell_ptr, (const int *)h->sell_col,
                       (const double *)h->sgn_root, h->ell_w, key, (uint32_t)first, h->n, h->ld, (int)b);
    H_TRY(hipGetLastError());
    H_WAIT("occ_sim_draw");
    h->b = b;
    h->have_u = true;
    return OCC_SIM_OK;
}

// x minus its component's mean (launches only)
static void launch_centre(occ_sim *h, int bc)
{
    const dim3 cols(1, bc / 16);
    hipLaunchKernelGGL(k_sim_comp_chunk, dim3((h->nchunk + 15) / 16, cols.y), dim3(256), 0, h->st, (const double *)h->X, (const int *)h->list,
                       (const int *)h->chunk_start, h->chunk_sum, h->nchunk, h->ld);
    hipLaunchKernelGGL(k_sim_comp_mean, dim3((h->k + 15) / 16, cols.y), dim3(256), 0, h->st, (const double *)h->chunk_sum, (const int *)h->comp_chunk,
                       (const int *)h->comp_size, h->mean, h->k, h->ld);
    hipLaunchKernelGGL(k_sim_comp_apply, dim3(h->ntile, cols.y), dim3(256), 0, h->st, h->X, (const uint32_t *)h->site_lab, (const double *)h->mean, h->n,
                       h->ld);
}

int occ_sim_solve(occ_sim *h, double tol, int64_t max_iter, int32_t check_every, double *info)
{
    if (!h) return OCC_SIM_E_BADARG;
    std::string why;
    if (!occ::sim_check_solve(tol, max_iter, check_every, &why)) H_ARG(false, why);
    H_ARG(h->have_u && h->b >= 1, "no right-hand side has been drawn");
    H_TRY(hipSetDevice(h->device));
    const int b = h->b, bc = occ::sim_bc(b), ld = h->ld, n = h->n, nt = h->ntile;
    const dim3 grid(nt, bc / 16), blk(256);
    const double tol2 = tol * tol;
    hipLaunchKernelGGL(k_sim_start, grid, blk, 0, h->st, (const double *)h->U, (const double *)h->dinv, h->X, h->R, h->P, h->part_a, h->part_b, n, ld);
    hipLaunchKernelGGL(k_sim_scal_start, dim3(1), dim3(64), 0, h->st, (const double *)h->part_a, (const double *)h->part_b, h->rz, h->rr, h->rr0, h->alpha,
                       h->beta, h->done, h->iters, nt, ld, bc);
    H_TRY(hipGetLastError());
    bool all_done = false;
    for (int64_t it = 0; it < max_iter && !all_done;) {
        const int64_t stop = std::min<int64_t>(max_iter, it + check_every);
        for (; it < stop; ++it) {
            hipLaunchKernelGGL(k_sim_spmv<0>, grid, blk, 0, h->st, (const double *)h->P, h->AP, (const double *)h->U, (const double *)h->diag,
                               (const int *)h->sell_ptr, (const int *)h->sell_col, (const double *)h->sell_val, h->ell_w, (const int *)h->done, h->part_a,
                               n, ld);
            hipLaunchKernelGGL(k_sim_scal_alpha, dim3(1), dim3(64), 0, h->st, (const double *)h->part_a, (const double *)h->rz, (const int *)h->done,
                               h->alpha, nt, ld, bc);
            hipLaunchKernelGGL(k_sim_update, grid, blk, 0, h->st, h->X, h->R, (const double *)h->P, (const double *)h->AP, (const double *)h->dinv,
                               (const double *)h->alpha, (const int *)h->done, h->part_a, h->part_b, n, ld);
            hipLaunchKernelGGL(k_sim_scal_beta, dim3(1), dim3(64), 0, h->st, (const double *)h->part_a, (const double *)h->part_b, h->rz, h->rr,
                               (const double *)h->rr0, h->alpha, h->beta, h->done, h->iters, tol2, (int)(it + 1), nt, ld, bc);
            hipLaunchKernelGGL(k_sim_dir, grid, blk, 0, h->st, h->P, (const double *)h->R, (const double *)h->dinv, (const double *)h->beta,
                               (const int *)h->done, n, ld);
        }
        H_TRY(hipGetLastError());
        H_TRY(hipMemcpyAsync(h->host_flags, h->done, (size_t)bc * sizeof(int), hipMemcpyDeviceToHost, h->st));
        H_WAIT("occ_sim_solve");
        all_done = true;
        for (int c = 0; c < bc; ++c) all_done = all_done && h->host_flags[c] != 0;
    }
    // the true residual, from scratch
    hipLaunchKernelGGL(k_sim_spmv<1>, grid, blk, 0, h->st, (const double *)h->X, (double *)nullptr, (const double *)h->U, (const double *)h->diag,
                       (const int *)h->sell_ptr, (const int *)h->sell_col, (const double *)h->sell_val, h->ell_w, (const int *)h->done, h->part_a, n, ld);
    hipLaunchKernelGGL(k_sim_scal_res, dim3(1), dim3(64), 0, h->st, (const double *)h->part_a, (const double *)h->rr0, h->res, nt, ld, bc);
    H_TRY(hipGetLastError());
    H_TRY(hipMemcpyAsync(h->host_flags, h->done, (size_t)bc * sizeof(int), hipMemcpyDeviceToHost, h->st));
    H_TRY(hipMemcpyAsync(h->host_flags + ld, h->iters, (size_t)bc * sizeof(int), hipMemcpyDeviceToHost, h->st));
    H_TRY(hipMemcpyAsync(h->host_res, h->res, (size_t)bc * sizeof(double), hipMemcpyDeviceToHost, h->st));
    H_WAIT("occ_sim_solve");
    if (info)
        for (int c = 0; c < b; ++c) {
            info[c] = (double)h->host_flags[ld + c];
            info[b + c] = h->host_res[c];
        }
    for (int c = 0; c < b; ++c)
        if (h->host_flags[c] == 0) {
            char msg[160];
            std::snprintf(msg, sizeof(msg), "column %d is not done after %lld iterations: relative residual %.3e", c, (long long)max_iter, h->host_res[c]);
            h->err = msg;
            return OCC_SIM_E_BADARG;
        }
    launch_centre(h, bc);
    launch_centre(h, bc);
    H_TRY(hipGetLastError());
    H_WAIT("occ_sim_solve");
    return OCC_SIM_OK;
}

int occ_sim_get(occ_sim *h, int32_t which, double *out, int32_t b)
{
    if (!h) return OCC_SIM_E_BADARG;
    H_ARG((which == 0 || which == 1) && out, "which must be 0 (x) or 1 (u)");
    H_ARG(b >= 1 && b <= h->b_max, "b must lie in [1, b_max]");
    H_TRY(hipSetDevice(h->device));
    H_TRY(hipMemcpy2DAsync(out, (size_t)b * sizeof(double), which == 0 ? h->X : h->U, (size_t)h->ld * sizeof(double), (size_t)b * sizeof(double),
                            (size_t)h->n, hipMemcpyDeviceToHost, h->st));
    H_WAIT("occ_sim_get");
    return OCC_SIM_OK;
}

}  // extern "C"
