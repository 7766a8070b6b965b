// occ_basis.hip -- libocc_basis.so, the C ABI of include/occ_basis.h: the device primitives of the filtered block subspace
// iteration that builds the reduced-rank Moran basis (occuspytial_amd/basis.py drives them).
//
//   Omega = s P A P,   P = I - X (X'X)^-1 X',   A = -offdiag(Q) in SELL-64 / ELL (occ_layout.hpp),   s = n / sum(A)
//
// Omega . V for a block of b columns is five launches and no n x n array:
//   k_basis_xt, k_basis_xt_solve     D1 = (X'X)^-1 X'V                               (p x b; partial sums per tile of 256 sites,
//                                                                                     added in tile order)
//   k_basis_spmm                     T  = A V - (A X) D1  =  A (P V)                 (A X is n x p, formed once on the host)
//   k_basis_xt, k_basis_xt_solve     D2 = (X'X)^-1 X'T
//   k_basis_combine                  out = alpha (T - X D2) + beta Y1 + gamma Y0     (alpha = s: Omega V; the other two terms
//                                                                                     are the Chebyshev recurrence's)
// Blocks are n x ld row-major, ld a multiple of 16: 16 consecutive doubles of a row are one 128-byte line, which is what a
// quarter-wave loads in every kernel here.  k_basis_gram and k_basis_rotate run on v_mfma_f64_16x16x4_f64 with the operand
// layout occ_rsr.hpp states (wave64: lane l carries A[l % 16][l / 16] and B[l / 16][l % 16], receives D[4 v + l / 16][l % 16]).
// No kernel waits on the device, none uses an atomic: every sum has one fixed order, so a repeated call returns the same
// bits.  The handle's device, stream, allocations, deadline wait and create / destroy are occ_handle.hpp's.
#include "../../include/occ_basis.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "occ_handle.hpp"
#include "occ_layout.hpp"

namespace occ_basis_impl {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int TS = 256;        // sites per tile of the column reductions (X'V, residual norms)
constexpr int MAXP = OCC_BASIS_MAX_P;
constexpr int FASTP = 8;       // columns of X the MP = 8 instantiations of the projection kernels hold; more (to MAXP): MP = MAXP
constexpr int GRAM_WAVES = 16; // waves per workgroup of k_basis_gram
constexpr int ROT_NJ = 4;      // 16-column tiles of the result one wave of k_basis_rotate holds

// part[(tile * MP + a) * ld + c] = sum over the tile's sites i of X[i][a] src[i][c], sites in order.  MP: the columns of X the
// kernel's register sums hold (FASTP, or MAXP for p > FASTP); the loops over them are unrolled, no array is indexed at run time.
template <int MP>
__global__ void __launch_bounds__(256) k_basis_xt(const double *__restrict__ src, const double *__restrict__ X, double *__restrict__ part, int n, int p,
                                                  int ld, int bc)
{
    const int c = (int)blockIdx.y * 256 + (int)threadIdx.x;
    if (c >= bc) return;
    const int i0 = (int)blockIdx.x * TS, i1 = min(n, i0 + TS);
    double acc[MP];
#pragma unroll
    for (int a = 0; a < MP; ++a) acc[a] = 0.0;
    for (int i = i0; i < i1; ++i) {
        const double v = src[(size_t)i * ld + c];
#pragma unroll
        for (int a = 0; a < MP; ++a)
            if (a < p) acc[a] = fma(X[(size_t)i * p + a], v, acc[a]);
    }
#pragma unroll
    for (int a = 0; a < MP; ++a)
        if (a < p) part[((size_t)blockIdx.x * MP + a) * ld + c] = acc[a];
}

// D[a][c] = sum_a' Xi[a][a'] C[a'][c],  C[a'][c] = the tiles' partial sums in tile order
template <int MP>
__global__ void __launch_bounds__(256) k_basis_xt_solve(const double *__restrict__ part, const double *__restrict__ Xi, double *__restrict__ D, int ntile,
                                                        int p, int ld, int bc)
{
    const int c = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (c >= bc) return;
    double C[MP];
#pragma unroll
    for (int a = 0; a < MP; ++a) C[a] = 0.0;
    for (int t = 0; t < ntile; ++t) {
#pragma unroll
        for (int a = 0; a < MP; ++a)
            if (a < p) C[a] += part[((size_t)t * MP + a) * ld + c];
    }
#pragma unroll
    for (int a = 0; a < MP; ++a) {
        if (a >= p) continue;
        double d = 0.0;
#pragma unroll
        for (int a2 = 0; a2 < MP; ++a2)
            if (a2 < p) d = fma(Xi[a * p + a2], C[a2], d);
        D[(size_t)a * ld + c] = d;
    }
}

// dst = A src - AX D: one workgroup per SELL slice of 64 sites and 64 columns; a quarter-wave owns a site and 16 columns
__global__ void __launch_bounds__(256) k_basis_spmm(const double *__restrict__ src, double *__restrict__ dst, const int *__restrict__ sell_ptr,
                                                    const int *__restrict__ sell_col, const double *__restrict__ sell_val, int ell_w,
                                                    const double *__restrict__ AX, const double *__restrict__ D, int n, int p, int ld, int bc)
{
    const int sl = (int)blockIdx.x, cl = (int)threadIdx.x & 15, sq = (int)threadIdx.x >> 4;
    const int c0 = (int)blockIdx.y * 64 + cl;
    const int base = ell_w ? sl * ell_w * 64 : sell_ptr[sl];
    const int width = ell_w ? ell_w : (sell_ptr[sl + 1] - base) / 64;
    for (int r = 0; r < 4; ++r) {
        const int ls = sq + 16 * r, i = sl * 64 + ls;
        if (i >= n) continue;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k < width; ++k) {
            const int slot = base + k * 64 + ls;
            const int j = sell_col[slot];
            const double a = sell_val[slot];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = c0 + 16 * g;
                if (c < bc) acc[g] = fma(a, src[(size_t)j * ld + c], acc[g]);
            }
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c = c0 + 16 * g;
            if (c >= bc) continue;
            double v = acc[g];
            for (int a = 0; a < p; ++a) v = fma(-AX[(size_t)i * p + a], D[(size_t)a * ld + c], v);
            dst[(size_t)i * ld + c] = v;
        }
    }
}

// out = alpha (in - X D) + beta y1 + gamma y0  (y1 / y0 are read only where beta / gamma is not zero; in may be out)
template <int MP>
__global__ void __launch_bounds__(256) k_basis_combine(const double *in, double *out, const double *__restrict__ X, const double *__restrict__ D,
                                                       const double *__restrict__ y1, const double *__restrict__ y0, double alpha, double beta,
                                                       double gamma, int n, int p, int ld, int bc)
{
    const int c = (int)blockIdx.y * 64 + ((int)threadIdx.x & 63);
    if (c >= bc) return;
    double d[MP];
#pragma unroll
    for (int a = 0; a < MP; ++a) d[a] = a < p ? D[(size_t)a * ld + c] : 0.0;
    const int i0 = (int)blockIdx.x * 64 + ((int)threadIdx.x >> 6);
    for (int r = 0; r < 16; ++r) {
        const int i = i0 + 4 * r;
        if (i >= n) break;
        const size_t at = (size_t)i * ld + c;
        double v = in[at];
#pragma unroll
        for (int a = 0; a < MP; ++a)
            if (a < p) v = fma(-X[(size_t)i * p + a], d[a], v);
        v *= alpha;
        if (beta != 0.0) v = fma(beta, y1[at], v);
        if (gamma != 0.0) v = fma(gamma, y0[at], v);
        out[at] = v;
    }
}

// G[ta-th 16 rows][tc-th 16 columns] = U[:, ta]' W[:, tc] for the tiles ta <= tc of the upper triangle, one workgroup each.
// A wave takes every GRAM_WAVES-th block of 32 sites (eight MFMAs, the next block's loads issued first); the waves' partial
// tiles are added in wave order through LDS.
__device__ __forceinline__ void gram_load(const double *__restrict__ U, const double *__restrict__ W, int n, int ld, int i0, int lk, int ca, int cc,
                                          double (&av)[8], double (&bv)[8])
{
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int i = i0 + 4 * t + lk;
        const bool vi = i < n;
        const size_t row = (size_t)(vi ? i : 0) * ld;
        const double x = U[row + ca], y = W[row + cc];
        av[t] = vi ? x : 0.0;
        bv[t] = vi ? y : 0.0;
    }
}

__global__ void __launch_bounds__(64 * GRAM_WAVES) k_basis_gram(const double *__restrict__ U, const double *__restrict__ W, double *__restrict__ G, int n,
                                                                int ld, int T)
{
    __shared__ double s_part[GRAM_WAVES - 1][64][4];
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63, lc = lane & 15, lk = lane >> 4;
    int ta = 0, rem = (int)blockIdx.x;  // upper triangle of tiles, row by row
    while (ta < T - 1 && rem >= T - ta) { rem -= T - ta; ++ta; }
    const int tc = min(ta + rem, T - 1);
    const int ca = ta * 16 + lc, cc = tc * 16 + lc;
    v4d acc = {0.0, 0.0, 0.0, 0.0};
    double av[8], bv[8], an[8], bn[8];
    int i0 = wave * 32;
    if (i0 < n) gram_load(U, W, n, ld, i0, lk, ca, cc, av, bv);
    for (; i0 < n; i0 += 32 * GRAM_WAVES) {
        const int i1 = i0 + 32 * GRAM_WAVES;
        if (i1 < n) gram_load(U, W, n, ld, i1, lk, ca, cc, an, bn);
#pragma unroll
        for (int t = 0; t < 8; ++t) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[t], bv[t], acc, 0, 0, 0);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            av[t] = an[t];
            bv[t] = bn[t];
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int v = 0; v < 4; ++v) s_part[wave - 1][lane][v] = acc[v];
    }
    __syncthreads();
    if (wave == 0) {
        for (int w = 0; w < GRAM_WAVES - 1; ++w) {
#pragma unroll
            for (int v = 0; v < 4; ++v) acc[v] += s_part[w][lane][v];
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) G[(size_t)(ta * 16 + 4 * v + lk) * ld + cc] = acc[v];
    }
}

// out = V Y: a wave owns 16 sites and ROT_NJ tiles of 16 result columns.  Per 16 columns of V a lane loads four consecutive
// doubles of its site's row (lane group lk: columns kb + 4 lk .. + 3) and feeds them to four MFMAs; MFMA t contracts over
// the columns kb + 4 lk + t, lk = 0 .. 3, and reads the matching rows of Y.  Y: kend x ldy, zero-padded.
__global__ void __launch_bounds__(256) k_basis_rotate(const double *__restrict__ V, const double *__restrict__ Y, double *__restrict__ out, int n, int ld,
                                                      int kend, int ldy, int Tout)
{
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63, lc = lane & 15, lk = lane >> 4;
    const int st = (int)blockIdx.x * 4 + wave;
    if (st * 16 >= n) return;
    const int i = st * 16 + lc;
    const bool vi = i < n;
    const double *row = V + (size_t)(vi ? i : 0) * ld;
    const int jt0 = (int)blockIdx.y * ROT_NJ;
    v4d acc[ROT_NJ];
#pragma unroll
    for (int j = 0; j < ROT_NJ; ++j) acc[j] = v4d{0.0, 0.0, 0.0, 0.0};
    for (int kb = 0; kb < kend; kb += 16) {
        double a[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const double x = row[kb + 4 * lk + t];
            a[t] = vi ? x : 0.0;
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const double *yrow = Y + (size_t)(kb + 4 * lk + t) * ldy + lc;
#pragma unroll
            for (int j = 0; j < ROT_NJ; ++j) {
                const int jt = min(jt0 + j, Tout - 1);  // (a tile past the end repeats the last one and is not stored)
                acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t], yrow[jt * 16], acc[j], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < ROT_NJ; ++j) {
        if (jt0 + j >= Tout) continue;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int io = st * 16 + 4 * v + lk;
            if (io < n) out[(size_t)io * ld + (jt0 + j) * 16 + lc] = acc[j][v];
        }
    }
}

// part[tile * ld + c] = sum over the tile's sites of (W[i][c] - lam[c] V[i][c])^2
__global__ void __launch_bounds__(256) k_basis_res(const double *__restrict__ W, const double *__restrict__ V, const double *__restrict__ lam,
                                                   double *__restrict__ part, int n, int ld, int bc)
{
    const int c = (int)blockIdx.y * 256 + (int)threadIdx.x;
    if (c >= bc) return;
    const int i0 = (int)blockIdx.x * TS, i1 = min(n, i0 + TS);
    const double l = lam[c];
    double acc = 0.0;
    for (int i = i0; i < i1; ++i) {
        const size_t at = (size_t)i * ld + c;
        const double d = fma(-l, V[at], W[at]);
        acc = fma(d, d, acc);
    }
    part[(size_t)blockIdx.x * ld + c] = acc;
}

__global__ void __launch_bounds__(256) k_basis_res_sum(const double *__restrict__ part, double *__restrict__ out, int ntile, int ld, int bc)
{
    const int c = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (c >= bc) return;
    double acc = 0.0;
    for (int t = 0; t < ntile; ++t) acc += part[(size_t)t * ld + c];
    out[c] = sqrt(acc);
}

}  // namespace occ_basis_impl

using namespace occ_basis_impl;

struct occ_basis : occ::HandleBase {
    int n = 0, p = 0, ld = 0, b = 0, b_max = 0, ell_w = 0, wmax = 0, nslice = 0, ntile = 0;
    double s = 0.0, rho = 0.0;
    int *sell_ptr = nullptr, *sell_col = nullptr;
    double *sell_val = nullptr, *X = nullptr, *AX = nullptr, *Xi = nullptr;
    double *blk[3] = {nullptr, nullptr, nullptr};
    int slot[3] = {0, 1, 2};  // logical -> physical block
    double *part = nullptr, *D = nullptr, *Y = nullptr, *G = nullptr, *lam = nullptr, *res = nullptr;
    bool w_valid = false;  // logical block 1 holds Omega . (logical block 0)
    std::vector<double> stage;
};
OCC_HANDLE_CODES(OCC_BASIS_OK, OCC_BASIS_E_BADARG, OCC_BASIS_E_HIP);

static thread_local std::string g_create_err;

static int bc_of(int b) { return (b + 15) / 16 * 16; }
static double *blk(occ_basis *h, int logical) { return h->blk[h->slot[logical]]; }

// D = (X'X)^-1 X' src
static int launch_xt(occ_basis *h, const double *src)
{
    const int bc = bc_of(h->b);
    const bool fast = h->p <= FASTP;  // (the two instantiations lay `part` out by their own MP: written and read by the same one)
    hipLaunchKernelGGL(fast ? k_basis_xt<FASTP> : k_basis_xt<MAXP>, dim3(h->ntile, (bc + 255) / 256), dim3(256), 0, h->st, src, h->X, h->part, h->n, h->p, h->ld, bc);
    hipLaunchKernelGGL(fast ? k_basis_xt_solve<FASTP> : k_basis_xt_solve<MAXP>, dim3((bc + 255) / 256), dim3(256), 0, h->st, h->part, h->Xi, h->D, h->ntile, h->p, h->ld, bc);
    return OCC_BASIS_OK;
}

// out = alpha s P A P src + beta y1 + gamma y0 (out != src; launches only)
static int launch_apply(occ_basis *h, const double *src, double *out, double alpha, double beta, const double *y1, double gamma, const double *y0)
{
    const int bc = bc_of(h->b);
    launch_xt(h, src);
    hipLaunchKernelGGL(k_basis_spmm, dim3(h->nslice, (bc + 63) / 64), dim3(256), 0, h->st, src, out, h->sell_ptr, h->sell_col, h->sell_val, h->ell_w,
                       h->AX, h->D, h->n, h->p, h->ld, bc);
    launch_xt(h, out);
    hipLaunchKernelGGL(h->p <= FASTP ? k_basis_combine<FASTP> : k_basis_combine<MAXP>, dim3(h->nslice, (bc + 63) / 64), dim3(256), 0, h->st, (const double *)out, out, h->X, h->D, y1, y0,
                       alpha * h->s, beta, gamma, h->n, h->p, h->ld, bc);
    H_TRY(hipGetLastError());
    return OCC_BASIS_OK;
}

static int ensure_w(occ_basis *h)
{
    if (h->w_valid) return OCC_BASIS_OK;
    const int rc = launch_apply(h, blk(h, 0), blk(h, 1), 1.0, 0.0, nullptr, 0.0, nullptr);
    if (rc == OCC_BASIS_OK) h->w_valid = true;
    return rc;
}

extern "C" {

int32_t occ_basis_version(void) { return OCC_BASIS_VERSION; }

const char *occ_basis_last_error(const occ_basis *h) { return h ? h->err.c_str() : g_create_err.c_str(); }

int occ_basis_destroy(occ_basis *h) { return occ::handle_destroy(h, "occ_basis_destroy"); }

static int create_impl(occ_basis *h, int64_t n64, const int32_t *indptr, const int32_t *indices, const double *qdata, const double *X, int32_t p,
                       const double *XtX_inv, int32_t b_max, int32_t device)
{
    H_ARG(n64 >= 1 && n64 < (int64_t)1 << 30, "n must lie in [1, 2^30)");
    H_ARG(p >= 1 && p <= MAXP, "p must lie in [1, 32]");
    H_ARG(b_max >= 1 && b_max <= 16384, "b_max must lie in [1, 16384]");
    H_ARG(indptr && indices && qdata && X && XtX_inv, "null input");
    const int n = (int)n64;
    std::vector<int32_t> ip(indptr, indptr + n + 1);
    std::string why;
    if (!occ::layout_q_indptr(n, ip, &why)) H_ARG(false, why);
    for (int i = 0; i < n; ++i) H_ARG(ip[i + 1] >= ip[i], "malformed Q indptr");
    std::vector<int32_t> ix(indices, indices + ip[n]);
    std::vector<double> qd(qdata, qdata + ip[n]);
    occ::HostLayout L;
    // (has_prior_factor: weights of either sign, no singularity test -- the basis needs neither)
    if (!occ::layout_q(n, ip, ix, qd, true, L, &why)) H_ARG(false, why);
    double total = 0.0, rowmax = 0.0;
    std::vector<double> AX((size_t)n * p, 0.0);
    for (int i = 0; i < n; ++i) {
        double rowabs = 0.0;
        for (int k = ip[i]; k < ip[i + 1]; ++k) {
            const int j = ix[k];
            if (j == i) continue;
            const double a = -qd[k];
            total += a;
            rowabs += std::fabs(a);
            for (int c = 0; c < p; ++c) AX[(size_t)i * p + c] += a * X[(size_t)j * p + c];
        }
        rowmax = std::max(rowmax, rowabs);
    }
    H_ARG(total > 0.0 && std::isfinite(total), "the off-diagonals of -Q must have a positive sum");
    for (double &v : L.sell_val) v = -v;  // A = -offdiag(Q)
    h->n = n;
    h->p = p;
    h->b_max = b_max;
    h->ld = bc_of(b_max);
    h->b = 0;
    h->ell_w = L.ell_w;
    h->wmax = L.wmax();
    h->nslice = (n + 63) / 64;
    h->ntile = (n + TS - 1) / TS;
    h->s = (double)n / total;
    h->rho = h->s * rowmax;

    int rc;
    if ((rc = h->open(device)) != OCC_BASIS_OK) return rc;
    if ((rc = h->upload(&h->sell_ptr, L.sell_ptr)) != OCC_BASIS_OK) return rc;
    if ((rc = h->upload(&h->sell_col, L.sell_col)) != OCC_BASIS_OK) return rc;
    if ((rc = h->upload(&h->sell_val, L.sell_val)) != OCC_BASIS_OK) return rc;
    if ((rc = h->upload(&h->X, std::vector<double>(X, X + (size_t)n * p))) != OCC_BASIS_OK) return rc;
    if ((rc = h->upload(&h->AX, AX)) != OCC_BASIS_OK) return rc;
    if ((rc = h->upload(&h->Xi, std::vector<double>(XtX_inv, XtX_inv + (size_t)p * p))) != OCC_BASIS_OK) return rc;
    const size_t ld = (size_t)h->ld;
    for (int k = 0; k < 3; ++k)
        if ((rc = h->alloc(&h->blk[k], (size_t)n * ld, true)) != OCC_BASIS_OK) return rc;
    const size_t mp = p <= FASTP ? FASTP : MAXP;  // (the rows the instantiation in use lays `part` and D out by: launch_xt)
    if ((rc = h->alloc(&h->part, (size_t)h->ntile * mp * ld, false)) != OCC_BASIS_OK) return rc;
    if ((rc = h->alloc(&h->D, mp * ld, false)) != OCC_BASIS_OK) return rc;
    if ((rc = h->alloc(&h->Y, ld * ld, false)) != OCC_BASIS_OK) return rc;
    if ((rc = h->alloc(&h->G, ld * ld, false)) != OCC_BASIS_OK) return rc;
    if ((rc = h->alloc(&h->lam, ld, false)) != OCC_BASIS_OK) return rc;
    if ((rc = h->alloc(&h->res, ld, false)) != OCC_BASIS_OK) return rc;
    H_WAIT("occ_basis_create");
    return OCC_BASIS_OK;
}

int occ_basis_create(int64_t n, const int32_t *q_indptr, const int32_t *q_indices, const double *q_data, const double *X, int32_t p,
                     const double *XtX_inv, int32_t b_max, int32_t device, occ_basis **out)
{
    return occ::handle_create(out, g_create_err, "occ_basis_destroy",
                              [&](occ_basis *h) { return create_impl(h, n, q_indptr, q_indices, q_data, X, p, XtX_inv, b_max, device); });
}

int occ_basis_info(const occ_basis *h, double *info6)
{
    if (!h || !info6) return OCC_BASIS_E_BADARG;
    info6[0] = h->s;
    info6[1] = h->rho;
    info6[2] = h->ell_w;
    info6[3] = h->ld;
    info6[4] = h->b;
    info6[5] = h->wmax;
    return OCC_BASIS_OK;
}

int occ_basis_set_block(occ_basis *h, int32_t which, const double *V, int32_t b)
{
    if (!h) return OCC_BASIS_E_BADARG;
    H_ARG(which >= 0 && which < 3 && V, "block index must be 0, 1 or 2");
    H_ARG(b >= 1 && b <= h->b_max, "b must lie in [1, b_max]");
    H_TRY(hipSetDevice(h->device));
    double *dst = blk(h, which);
    H_TRY(hipMemsetAsync(dst, 0, (size_t)h->n * h->ld * sizeof(double), h->st));
    H_TRY(hipMemcpy2DAsync(dst, (size_t)h->ld * sizeof(double), V, (size_t)b * sizeof(double), (size_t)b * sizeof(double), (size_t)h->n,
                            hipMemcpyHostToDevice, h->st));
    H_WAIT("occ_basis_set_block");
    h->b = b;
    h->w_valid = false;
    return OCC_BASIS_OK;
}

int occ_basis_get_block(occ_basis *h, int32_t which, double *V, int32_t b)
{
    if (!h) return OCC_BASIS_E_BADARG;
    H_ARG(which >= 0 && which < 3 && V, "block index must be 0, 1 or 2");
    H_ARG(b >= 1 && b <= h->b_max, "b must lie in [1, b_max]");
    H_TRY(hipSetDevice(h->device));
    H_TRY(hipMemcpy2DAsync(V, (size_t)b * sizeof(double), blk(h, which), (size_t)h->ld * sizeof(double), (size_t)b * sizeof(double), (size_t)h->n,
                            hipMemcpyDeviceToHost, h->st));
    H_WAIT("occ_basis_get_block");
    return OCC_BASIS_OK;
}

int occ_basis_apply(occ_basis *h, int32_t src, int32_t dst)
{
    if (!h) return OCC_BASIS_E_BADARG;
    H_ARG(src >= 0 && src < 3 && dst >= 0 && dst < 3 && src != dst, "src and dst must be two different blocks of 0, 1, 2");
    H_ARG(h->b >= 1, "no block has been set");
    H_TRY(hipSetDevice(h->device));
    const int rc = launch_apply(h, blk(h, src), blk(h, dst), 1.0, 0.0, nullptr, 0.0, nullptr);
    if (rc != OCC_BASIS_OK) return rc;
    if (dst == 0) h->w_valid = false;
    else if (dst == 1) h->w_valid = (src == 0);
    H_WAIT("occ_basis_apply");
    return OCC_BASIS_OK;
}

int occ_basis_project(occ_basis *h)
{
    if (!h) return OCC_BASIS_E_BADARG;
    H_ARG(h->b >= 1, "no block has been set");
    H_TRY(hipSetDevice(h->device));
    const int bc = bc_of(h->b);
    double *v = blk(h, 0);
    launch_xt(h, v);
    hipLaunchKernelGGL(h->p <= FASTP ? k_basis_combine<FASTP> : k_basis_combine<MAXP>, dim3(h->nslice, (bc + 63) / 64), dim3(256), 0, h->st, (const double *)v, v, h->X, h->D, (const double *)nullptr,
                       (const double *)nullptr, 1.0, 0.0, 0.0, h->n, h->p, h->ld, bc);
    H_TRY(hipGetLastError());
    h->w_valid = false;
    H_WAIT("occ_basis_project");
    return OCC_BASIS_OK;
}

int occ_basis_filter(occ_basis *h, int32_t degree, double lo, double hi, double top)
{
    if (!h) return OCC_BASIS_E_BADARG;
    H_ARG(h->b >= 1, "no block has been set");
    H_ARG(degree >= 1 && degree <= 4096, "degree must lie in [1, 4096]");
    H_ARG(lo < hi && hi < top && std::isfinite(lo) && std::isfinite(top), "the damped interval needs lo < hi < top");
    H_TRY(hipSetDevice(h->device));
    const double c = 0.5 * (lo + hi), e = 0.5 * (hi - lo);
    // sigma_k = T_{k-1}(x0) / T_k(x0), x0 = (top - c) / e > 1: in (0, 1], so every coefficient below is bounded
    const double sigma1 = e / (top - c);
    double sigma = sigma1;
    // Y1 = sigma1 (Omega - c) V / e
    int rc = launch_apply(h, blk(h, 0), blk(h, 1), sigma1 / e, -sigma1 * c / e, blk(h, 0), 0.0, nullptr);
    if (rc != OCC_BASIS_OK) return rc;
    h->w_valid = false;
    int y0 = h->slot[0], y1 = h->slot[1], y2 = h->slot[2];
    for (int k = 2; k <= degree; ++k) {
        const double sn = 1.0 / (2.0 / sigma1 - sigma);
        // Y2 = 2 sn (Omega - c) Y1 / e - sigma sn Y0
        rc = launch_apply(h, h->blk[y1], h->blk[y2], 2.0 * sn / e, -2.0 * sn * c / e, h->blk[y1], -sigma * sn, h->blk[y0]);
        if (rc != OCC_BASIS_OK) return rc;
        const int t = y0;
        y0 = y1;
        y1 = y2;
        y2 = t;
        sigma = sn;
    }
    h->slot[0] = y1;  // the result becomes V
    h->slot[1] = y0;
    h->slot[2] = y2;
    H_WAIT("occ_basis_filter");
    return OCC_BASIS_OK;
}

int occ_basis_gram(occ_basis *h, int32_t which, double *out)
{
    if (!h) return OCC_BASIS_E_BADARG;
    H_ARG((which == 0 || which == 1) && out, "which must be 0 (V'V) or 1 (V' Omega V)");
    H_ARG(h->b >= 1, "no block has been set");
    H_TRY(hipSetDevice(h->device));
    const int b = h->b, bc = bc_of(b), T = bc / 16, ld = h->ld;
    if (which == 1) {
        const int rc = ensure_w(h);
        if (rc != OCC_BASIS_OK) return rc;
    }
    hipLaunchKernelGGL(k_basis_gram, dim3(T * (T + 1) / 2), dim3(64 * GRAM_WAVES), 0, h->st, (const double *)blk(h, 0), (const double *)blk(h, which), h->G,
                       h->n, ld, T);
    H_TRY(hipGetLastError());
    h->stage.resize((size_t)bc * bc);
    H_TRY(hipMemcpy2DAsync(h->stage.data(), (size_t)bc * sizeof(double), h->G, (size_t)ld * sizeof(double), (size_t)bc * sizeof(double), (size_t)bc,
                            hipMemcpyDeviceToHost, h->st));
    H_WAIT("occ_basis_gram");
    for (int i = 0; i < b; ++i)
        for (int j = i; j < b; ++j) out[(size_t)i * b + j] = out[(size_t)j * b + i] = h->stage[(size_t)i * bc + j];
    return OCC_BASIS_OK;
}

int occ_basis_rotate(occ_basis *h, const double *Y, int32_t b_out)
{
    if (!h) return OCC_BASIS_E_BADARG;
    H_ARG(h->b >= 1, "no block has been set");
    H_ARG(Y && b_out >= 1 && b_out <= h->b_max, "b_out must lie in [1, b_max]");
    H_TRY(hipSetDevice(h->device));
    const int b = h->b, kend = bc_of(b), ldy = bc_of(b_out), Tout = ldy / 16;
    h->stage.assign((size_t)kend * ldy, 0.0);
    for (int k = 0; k < b; ++k) std::memcpy(&h->stage[(size_t)k * ldy], Y + (size_t)k * b_out, (size_t)b_out * sizeof(double));
    H_TRY(hipMemcpyAsync(h->Y, h->stage.data(), h->stage.size() * sizeof(double), hipMemcpyHostToDevice, h->st));
    double *dst = blk(h, 2);
    H_TRY(hipMemsetAsync(dst, 0, (size_t)h->n * h->ld * sizeof(double), h->st));
    const int nst = (h->n + 15) / 16;
    hipLaunchKernelGGL(k_basis_rotate, dim3((nst + 3) / 4, (Tout + ROT_NJ - 1) / ROT_NJ), dim3(256), 0, h->st, (const double *)blk(h, 0), (const double *)h->Y,
                       dst, h->n, h->ld, kend, ldy, Tout);
    H_TRY(hipGetLastError());
    H_WAIT("occ_basis_rotate");
    std::swap(h->slot[0], h->slot[2]);
    h->b = b_out;
    h->w_valid = false;
    return OCC_BASIS_OK;
}

int occ_basis_residual(occ_basis *h, const double *lam, double *out)
{
    if (!h) return OCC_BASIS_E_BADARG;
    H_ARG(h->b >= 1, "no block has been set");
    H_ARG(lam && out, "null input");
    H_TRY(hipSetDevice(h->device));
    const int b = h->b, bc = bc_of(b);
    h->stage.assign((size_t)bc, 0.0);
    std::memcpy(h->stage.data(), lam, (size_t)b * sizeof(double));
    H_TRY(hipMemcpyAsync(h->lam, h->stage.data(), (size_t)bc * sizeof(double), hipMemcpyHostToDevice, h->st));
    const int rc = ensure_w(h);
    if (rc != OCC_BASIS_OK) return rc;
    hipLaunchKernelGGL(k_basis_res, dim3(h->ntile, (bc + 255) / 256), dim3(256), 0, h->st, (const double *)blk(h, 1), (const double *)blk(h, 0),
                       (const double *)h->lam, h->part, h->n, h->ld, bc);
    hipLaunchKernelGGL(k_basis_res_sum, dim3((bc + 255) / 256), dim3(256), 0, h->st, (const double *)h->part, h->res, h->ntile, h->ld, bc);
    H_TRY(hipGetLastError());
    H_TRY(hipMemcpyAsync(out, h->res, (size_t)b * sizeof(double), hipMemcpyDeviceToHost, h->st));
    H_WAIT("occ_basis_residual");
    return OCC_BASIS_OK;
}

}  // extern "C"
