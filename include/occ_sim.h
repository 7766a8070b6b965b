/*
 * occ_sim.h -- C ABI of libocc_sim.so: realisations of the intrinsic CAR field  x ~ N(0, Q^+)  on an MI355X (gfx950), for
 * any ICAR precision Q = D - W (zero row sums, non-positive off-diagonals) with any number of connected components.
 *
 *   u = B'eps  (edge form, B'B = Q; stream ETA_EDGE with it = draw number)  has law N(0, Q);
 *   x = Q^+ u  has law N(0, Q^+ Q Q^+) = N(0, Q^+):  one sparse solve per draw, O(nnz) memory, no n x n array.
 *
 * The solve is Jacobi-preconditioned conjugate gradients from x = 0 on all columns of a batch at once, every column a CG
 * of its own, then centring on every component (the minimum-norm solution).  Q is sparse (SELL-64 / ELL).  The driver is
 * Python (occuspytial_amd/simulate.py).  A library of its own: nothing here is part of include/occ_gibbs.h, and a handle
 * takes no stream of the engine's pool (one plain, non-blocking stream per handle).
 *
 * A handle owns five n x ld blocks of doubles, row-major, ld = b_max rounded up to 16:  x, u, r, p, Qp.
 *
 * Conventions: every function returns OCC_SIM_OK or a negative code, occ_sim_last_error() gives the text; all real data is
 * IEEE float64, C-contiguous; index arrays are int32; a handle is driven by one host thread at a time.
 * No kernel waits on the device, none uses an atomic: every sum has one fixed order (per tile of 256 sites, the tiles in
 * tile order), so a repeated call returns the same bits, and the bits of a draw depend on (Q, key, draw number, tol) alone --
 * not on b, on the columns that share its batch or on check_every.
 */
#ifndef OCC_SIM_H
#define OCC_SIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OCC_SIM_VERSION 1
#define OCC_SIM_MAX_B 64 /* columns of one batch */

enum {
    OCC_SIM_OK = 0,
    OCC_SIM_E_BADARG = -1, /* -> ValueError (also: a column that is not done after max_iter iterations) */
    OCC_SIM_E_HIP = -2     /* -> EngineUnavailable (HIP runtime failure / no device / a wait that ran out) */
};

typedef struct occ_sim occ_sim;

int32_t occ_sim_version(void);
const char *occ_sim_last_error(const occ_sim *h); /* h may be NULL: the last failed occ_sim_create of this thread */

/* Q: n x n CSR, sorted unique columns, zero row sums, non-positive off-diagonals;  labels[n]: the component of every site
 * (whole numbers in [0, n), equal for neighbours);  1 <= b_max <= OCC_SIM_MAX_B. */
int occ_sim_create(int64_t n, const int32_t *q_indptr, const int32_t *q_indices, const double *q_data, const int32_t *labels,
                   int32_t b_max, int32_t device, occ_sim **out);
int occ_sim_destroy(occ_sim *h);
/* info[0] = ELL width (0: true SELL-64), info[1] = ld, info[2] = tiles of 256 sites, info[3] = components, info[4] = b,
 * info[5] = chunks of the component tables */
int occ_sim_info(const occ_sim *h, double *info6);

/* Right-hand sides: column c < b is  u_i = sum_j +-sqrt(w_ij) block_normal(key, min(i,j), max(i,j), first + c, ETA_EDGE),  the
 * row's off-diagonals in column order from 0.0, + for i < j.  1 <= b <= b_max, first + b <= 2^32.  b becomes the handle's
 * current number of columns. */
int occ_sim_draw(occ_sim *h, uint64_t key, int64_t first, int32_t b);
/* x_c = Q^+ u_c for the b columns drawn last.  Column c is done in the iteration in which ||r_c|| <= tol ||u_c|| first holds
 * (0 < tol < 1); the host looks at the done flags every check_every iterations (>= 1; 16 is a good value).
 * info (2 b doubles, may be NULL): info[c] = iterations of column c, info[b + c] = || u_c - Q x_c || / || u_c || formed from
 * scratch after the loop (0 for u_c = 0).  A column that is not done after max_iter iterations: OCC_SIM_E_BADARG, the text
 * names the column and its residual; info is filled all the same, x is then not centred and must not be used. */
int occ_sim_solve(occ_sim *h, double tol, int64_t max_iter, int32_t check_every, double *info);
/* out (n x b, row-major) = x (which = 0) or u (which = 1) */
int occ_sim_get(occ_sim *h, int32_t which, double *out, int32_t b);

#ifdef __cplusplus
}
#endif
#endif
