// occ_spatial.hpp -- the spatial residual check (state names moran_stats, moran_draws; logit models): Moran's I of the
// occupancy residuals z - psi of a kept draw and of one replicate of them, as eight integer sums per chain and draw.
// DESIGN.md section 19 is the specification.
//
// Two kernels (occ_spatial.hip, a translation unit of its own inside libocc_gibbs.so: the unit of occ_gibbs.hip keeps the
// kernel symbols it had), launched directly behind the z update on its stream while a chain of the handle has the switch
// on.  They cannot be part of the z update: a site's term needs its neighbours' NEW z, and the z update has no barrier across the
// workgroups of a chain.  Stream order is the synchronisation: nothing writes z, eta or beta between the z update and the
// first kernel of the next sequence.
//
//   k_sp_resid   per site i:  psi_i = expit(x_i beta + eta_i) (the operations of the z update's site_psi),  r_i = z_i - psi_i,
//                u_i = block_uniform(key, i, 0, it, STREAM_SPATIAL),  z*_i = [u_i < psi_i],  r*_i = z*_i - psi_i;
//                stores (r_i, r*_i) as one double2.
//   k_sp_moran   per site i, over the off-diagonals of its row of Q in column order, w_ij = -Q_ij:
//                d_i = sum_j w_ij,  s_i = sum_j w_ij r_j,  s*_i = sum_j w_ij r*_j, and adds
//                fx(r_i s_i), fx(d_i r_i), fx(r_i), fx(r_i^2), fx(r*_i s*_i), fx(d_i r*_i), fx(r*_i), fx(r*_i^2)
//                to the draw's row [A, B, C, D, A*, B*, C*, D*];  fx(x) = llrint(x 2^32), added in two's complement.
// Integer sums: the order of addition cannot change a bit, so the rows are the same on every path and placement.
// The host admits a graph only if every off-diagonal of Q is <= 0, 0 < S0 = sum_i d_i < 2^30 and n < 2^30: |r| < 1, so
// |A| < S0, |B| < S0, |C| < n and D < n, and every column stays below 2^62 quanta.
#pragma once
#include "occ_rng.hpp"
#include "occ_state.hpp"

namespace occ {

enum : int { SP_A = 0, SP_B = 1, SP_C = 2, SP_D = 3, SP_NCOL = 8 };  // the replicate's four follow in the same order

// By-value argument block of the two kernels.  Everything but `rec` is fixed from the handle's first switch-on; `rec` moves
// only when the record of a call grows, between calls (the host then drops the captured graphs).
struct SpArgs {
    int n, p;
    const double *Xt;      // Ctx::Xt
    const double *eta;     // Ctx::eta  [C][n] (reduced rank: K theta as stored)
    const uint8_t *z;      // Ctx::z    [C][n]
    const int *ptr, *col;  // off-diagonal CSR of Q: ptr[n + 1], columns in column order
    const double *val;     // -Q_ij
    double2 *res;          // [C][n] (r, r*) of the iteration in hand
    long long *rec;        // [C][keep][SP_NCOL] of the running occ_run, zeroed by the host when the call's window opens
    const uint32_t *on;    // [C] the chains' switches (a word of the handle, not a bit of ChainScalars::site_on)
};

// Both kernels behind the z update of sequence parity e on `st`, a (ceil(n / 256), C) grid of 256 threads each (occ_spatial.hip).
// A launch the runtime rejects shows in hipGetLastError(), which the caller asks.
void sp_launch(const SpArgs &a, const ChainScalars *scs, int C, int e, hipStream_t st);

}  // namespace occ
