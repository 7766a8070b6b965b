/*
 * occ_basis.h -- C ABI of libocc_basis.so: the primitives of a filtered block subspace iteration for the leading
 * eigenvectors of the Moran operator  Omega = s P A P,  P = I - X (X'X)^-1 X',  A = -offdiag(Q),  s = n / sum(A),
 * on an MI355X (gfx950).  Omega is never formed: A is sparse (SELL-64 / ELL), P a rank-p correction.
 *
 * The driver is Python (occuspytial_amd/basis.py: moran_basis); the b x b Cholesky and eigen-decompositions of an outer
 * round are the host's.  A library of its own: nothing here is part of include/occ_gibbs.h, and a handle takes no
 * stream of the engine's pool (one plain, unmasked stream per handle).
 *
 * A handle owns three n x ld blocks of doubles, row-major, ld = b_max rounded up to 16, named by LOGICAL index:
 *   0  V, the current block of b columns        1  W = Omega V (valid after gram(1) / residual)        2  work space
 * filter and rotate leave their result in block 0 by renaming blocks, not by copying.  Columns b .. bc-1 hold zeros, bc = b
 * rounded up to 16; nothing reads a column from bc on (after a rotate to fewer columns they may hold a wider block's data).
 *
 * Conventions: every function returns OCC_BASIS_OK or a negative code, occ_basis_last_error() gives the text; all real
 * data is IEEE float64, C-contiguous; index arrays are int32; a handle is driven by one host thread at a time.
 * No result depends on the order in which workgroups run: partial sums are kept per tile of sites and added in tile
 * order, so a repeated call returns the same bits.
 */
#ifndef OCC_BASIS_H
#define OCC_BASIS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OCC_BASIS_VERSION 1
#define OCC_BASIS_MAX_P 32 /* columns of X (up to 8: the projection kernels with 8 register sums; more: with 32) */

enum {
    OCC_BASIS_OK = 0,
    OCC_BASIS_E_BADARG = -1, /* -> ValueError */
    OCC_BASIS_E_HIP = -2     /* -> EngineUnavailable (HIP runtime failure / no device / a wait that ran out) */
};

typedef struct occ_basis occ_basis;

int32_t occ_basis_version(void);
const char *occ_basis_last_error(const occ_basis *h); /* h may be NULL: the last failed occ_basis_create of this thread */

/* Q: n x n CSR, sorted unique columns (its diagonal is ignored, its off-diagonals negated: weights allowed, any sign);
 * X: n x p row-major, 1 <= p <= OCC_BASIS_MAX_P;  XtX_inv: p x p, the inverse of X'X formed by the caller;
 * 1 <= b_max.  Computes s = n / sum(A) and rho = s max_i sum_j |a_ij| >= ||Omega|| (Gershgorin; ||P|| = 1). */
int occ_basis_create(int64_t n, const int32_t *q_indptr, const int32_t *q_indices, const double *q_data, const double *X, int32_t p,
                     const double *XtX_inv, int32_t b_max, int32_t device, occ_basis **out);
int occ_basis_destroy(occ_basis *h);
/* info[0] = s, info[1] = rho, info[2] = ELL width (0: true SELL-64), info[3] = ld, info[4] = b, info[5] = widest slice */
int occ_basis_info(const occ_basis *h, double *info6);

/* host (n x b, row-major) <-> logical block `which`; set_block makes b the handle's current number of columns */
int occ_basis_set_block(occ_basis *h, int32_t which, const double *V, int32_t b);
int occ_basis_get_block(occ_basis *h, int32_t which, double *V, int32_t b);

/* block dst = Omega . block src   (src != dst) */
int occ_basis_apply(occ_basis *h, int32_t src, int32_t dst);
/* V <- P V */
int occ_basis_project(occ_basis *h);
/* V <- T_d((Omega - c) / e) V / T_d((top - c) / e),  c = (lo + hi) / 2, e = (hi - lo) / 2, lo < hi < top, degree >= 1:
 * the Chebyshev polynomial that stays within +-1 / T_d(..) on [lo, hi] and is 1 at top, by the three-term recurrence in
 * the scaled form whose coefficients stay bounded (sigma_k = T_{k-1} / T_k at top lies in (0, 1]). */
int occ_basis_filter(occ_basis *h, int32_t degree, double lo, double hi, double top);
/* out (b x b, row-major) = V'V (which = 0) or V'(Omega V) (which = 1), on v_mfma_f64_16x16x4_f64; the upper triangle is
 * computed and mirrored, so out is exactly symmetric */
int occ_basis_gram(occ_basis *h, int32_t which, double *out);
/* V <- V Y,  Y: b x b_out row-major, 1 <= b_out <= b_max; b_out becomes the current number of columns */
int occ_basis_rotate(occ_basis *h, const double *Y, int32_t b_out);
/* out[j] = || Omega v_j - lam[j] v_j ||_2,  j < b */
int occ_basis_residual(occ_basis *h, const double *lam, double *out);

#ifdef __cplusplus
}
#endif
#endif
