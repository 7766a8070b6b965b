// occ_comp.hpp -- SUM-TO-ZERO PER CONNECTED COMPONENT, the device's part: the correction pass that follows the solve part of a
// launch sequence while the handle has more than one component (state name component_id; tables: occ_comp_plan.hpp).
// DESIGN.md section 24 is the specification.
//
// Lambda = tau Q + diag(omega) is block diagonal over the components of Q's graph, so the joint solve's x = Lambda^-1 y and
// z = Lambda^-1 1 restricted to a component ARE that block's solves, and the conditional under one constraint per component
// is eta_i = x_i + a_c z_i with a_c = -(sum of x over c) / (sum of z over c).  The solve -- whatever its form -- has left
// the unprojected (x, z) in Xv, the globally projected eta and beta's partial sums formed from it.  Between it and the z
// update, on the main stream (stream order is the synchronisation), three kernels of occ_comp.hip -- a translation unit of
// its own inside libocc_gibbs.so: the unit of occ_gibbs.hip keeps the kernel symbols it had --
//   k_comp_part   one thread per chunk: (sum x, sum z) of its sites, serially                       -> CompArgs::part
//   k_comp_coef   one thread per component of at most COMP_LIGHT chunks, one wave per larger one    -> CompArgs::coef
//   k_comp_eta    one thread per site: eta_i = fma(a_c, z_i, x_i) -- 0.0 at a component of one site, where the fma would
//                 leave its rounding residue
// and then k_beta_sums (occ_kernels.hpp, what occ_cond_beta launches) forms beta's partial sums again from that eta.
// No floating-point atomics: the order of every sum is the tables' (occ_comp_plan.hpp), the same for every form of the solve.
// A chain that idles in this sequence -- past it_stop, err set, or a solve carried to the next replay (mid[e].koff > 0) --
// is left alone by the three, as the projection leaves it alone (k_beta_sums then re-forms sums nobody reads).
#pragma once
#include "occ_comp_plan.hpp"
#include "occ_state.hpp"

namespace occ {

// By-value argument block of the kernels (device addresses): setting the labels drops the captured graphs on the host.
// k <= 1: the pass is not launched (no labels set, or one component: the global constraint).
struct CompArgs {
    int n, k, nchunk, nheavy;
    const int32_t *list, *chunk_start, *comp_chunk, *heavy;
    const uint32_t *site_lab;
    const double2 *Xv;  // Ctx::Xv   [C][n]  the solve's unprojected (x, z)
    double *eta;        // Ctx::eta  [C][n]
    double *part;       // [C][nchunk][2]  a chunk's (sum x, sum z)
    double *coef;       // [C][k]          a_c of component c (singletons: not written, not read)
};

enum CompStage : int { COMP_PART = 0, COMP_COEF, COMP_ETA };

// One of the three kernels for the chains chain_base .. chain_base + chains - 1 of sequence parity e on `st` (occ_comp.hip).
// A launch the runtime rejects shows in hipGetLastError(), which the caller asks.
void comp_launch(const CompArgs &a, const ChainScalars *scs, CompStage stage, int chain_base, int chains, int e, hipStream_t st);

}  // namespace occ
