/*
 * occ_gibbs.h -- C ABI of the MI355X (gfx950) Gibbs engine for the ICAR spatial occupancy model.
 *
 * The reference (zoj613/OccuSpytial v0.2.0) has no FFI boundary of its own for this path: the hot
 * loop is the Python method LogitICARGibbs.step() (occuspytial/gibbs/logit.py:254-266) calling
 * numpy/scipy, two Cython helpers and the third-party `polyagamma` C sampler.  This header is the
 * boundary a binding of that path would use: one opaque handle per (device, batch of chains), plain
 * pointers and sizes, int status codes that map onto the reference's exception types/messages.
 * The Python classes occuspytial_amd.gibbs.LogitICARGibbs / LogitRSRGibbs bind it with ctypes
 * (INTEGRATION.md shows the stub a maintainer of the reference would add).
 *
 * Conventions
 *  - every function returns OCC_OK (0) or a negative OCC_E* code; occ_last_error() gives the text;
 *  - input pointers may be host or device memory (copied with hipMemcpyDefault); the library never
 *    frees or keeps caller memory; outputs are host buffers owned by the caller;
 *  - all real data is IEEE float64, C-contiguous; index arrays are int32;
 *  - a handle is driven by one host thread at a time; handles on DIFFERENT devices are independent, and ctypes
 *    releases the GIL so host threads can drive several GPUs (occ_create_group;
 *    occuspytial_amd.gibbs.LogitICARGibbs(..., devices=[...]) does exactly that); handles on the SAME device share
 *    that device's pooled streams and their calls run one after the other (a per-device lock inside the library);
 *  - there is NO CPU fallback: creation fails with OCC_E_HIP when no gfx950 device is usable.
 */
#ifndef OCC_GIBBS_H
#define OCC_GIBBS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OCC_ABI_VERSION 7
#define OCC_MAX_COVARIATES 32 /* p and q limit.  Up to 8 of each: kernels with the p x p / q x q accumulators in registers and the
                                fused iteration kernel; 9 to 32: generic kernels (run-time p and q, terms reduced one at a time,
                                Cholesky factor in LDS) on the launch-per-step path */

enum {
    OCC_OK = 0,
    OCC_E_BADARG = -1,   /* -> ValueError */
    OCC_E_HIP = -2,      /* -> RuntimeError (HIP runtime failure / no device) */
    OCC_E_MINRES = -3,   /* -> RuntimeError('MINRES solver did not converge!')        logit.py:91-92 */
    OCC_E_CHOLESKY = -4, /* -> RuntimeError('Cholesky factorization/solver failed!')  distributions.pyx:21,107-108 */
    OCC_E_STATE = -5     /* unknown state name / wrong length */
};

/* The fixed inputs of LogitICARGibbs(Q, W, X, y, hparams) (logit.py:172-174, base.py:84-88,107-162)
 * flattened by the host: W/y dictionaries become one (R x q) matrix / R vector in surveyed-site
 * order with site_ptr offsets (replaces the Data container, data.pyx:61-140); Q is CSR with sorted
 * columns (the reference keeps CSC of the same symmetric matrix, base.py:122). */
typedef struct occ_problem {
    int64_t n;               /* sites                                   base.py:123 */
    int64_t n_surveyed;      /* S = len(W)                              data.pyx:142-144 */
    int64_t n_rows;          /* R = total visits over surveyed sites */
    int32_t p;               /* occupancy covariates  (X.shape[1]) */
    int32_t q;               /* detection covariates  (W[i].shape[1]) */
    const int32_t *q_indptr; /* n+1 */
    const int32_t *q_indices;
    const double *q_data;    /* ICAR precision: zero row sums, non-positive off-diagonals */
    const double *X;         /* n x p, row-major */
    const int32_t *site_id;  /* S: site number of each surveyed site (Data.surveyed order) */
    const int32_t *site_ptr; /* S+1: row offsets into W / y */
    const double *W;         /* R x q, row-major */
    const double *y;         /* R: 0/1 detections */
    const double *a_mu, *a_prec; /* q, q x q    base.py:49-61,177-186 */
    const double *b_mu, *b_prec; /* p, p x p */
    double tau_rate, tau_shape;
    /* Reduced-rank model (LogitRSRGibbs, logit.py:269-485), optional: rsr_dim = m > 0 selects it.  The spatial
     * effects are eta = K theta with K the n x m Moran-operator basis the host computed (logit.py:413-446);
     * rsr_Q = K'QK (m x m), rsr_E its eigenfactor, E E' = K'QK (logit.py:321-323); all row-major; m <= 4096 (up to 128 the
     * system is solved in LDS and registers, beyond that panel by panel in device memory). */
    int32_t rsr_dim;
    const double *rsr_K, *rsr_Q, *rsr_E;
    /* Prior draw of the eta conditional, optional.  NULL (default): the engine draws the N(0, Q) prior term in EDGE form,
     * u = B'eps with Q = B'B the weighted incidence factorisation -- O(nnz) work, no set-up -- which needs Q to be an ICAR
     * precision D - W with W >= 0.  Non-NULL: the reference's own form (logit.py:64-67, 77): u = F eps with F an
     * n x prior_factor_cols matrix, row-major, F F' = Q (the reference's eigenfactor E = U[:, 1:] sqrt(s[1:]) from the
     * dense eigh of Q; any factor gives the same law) and eps standard normals of Philox stream 10 -- O(n^2) memory and
     * bytes per iteration, but ANY symmetric positive semi-definite singular Q is accepted (positive off-diagonals too). */
    const double *prior_factor;
    int64_t prior_factor_cols;
    /* ABI 7: the link function.  0: logit (everything above).  1: probit with reduced-rank spatial effects (ProbitRSRGibbs,
     * reference gibbs/probit.py): rsr_dim = m (1 to 4096) and rsr_K (n x m) as for the logit model, p and q at most 8, and the
     * generalized eigenvectors of (K'QK, K'K) that make the eta update factor-free: pb_G (m x m, row-major) with
     * K'QK pb_G = K'K pb_G diag(pb_lam) and pb_G' K'K pb_G = I, pb_lam (m, >= 0), pb_Phi = K pb_G (n x m, row-major).
     * State names of a probit handle: alpha beta tau iter z k exists omega_b omega_a, eta (= K theta), eps (n), theta (m, = G c;
     * setting it sets c and eta), c (m, the engine's coordinates: theta = pb_G c), link (read-only, 1).  Its Philox streams
     * (sub-stream index in brackets; block 0 for uniforms and normals): omega_b uniform 1 [site], eps normal 11 [site],
     * xi normal 12 [column], tau gamma 2 [0, cursor], beta normals 5 [component], omega_a uniform 6 [visit row],
     * alpha normals 7 [component], z uniform 8 [site].  occ_profile counts its kernels under the existing kinds by role:
     * omega_b (k_pb_site), eta_init (k_pb_proj), minres (k_pb_coef: tau and c), beta_partial (k_pb_eta), omega_a
     * (k_pb_omega_a), alpha_draw (k_pb_alpha: beta and alpha), z_ob (k_pb_z + k_pb_tail); the chains' counters are restored
 * afterwards, their vectors are not.  The occ_cond_* entry points, occ_create_group and
     * occ_create_distributed reject it (OCC_E_BADARG). */
    int32_t link;
    const double *pb_Phi, *pb_G, *pb_lam;
} occ_problem;

typedef struct occ_sampler occ_sampler;

/* Build device-resident state for `n_chains` independent chains of one problem on HIP device
 * `device`.  keys[c] seeds chain c's counter-based (Philox4x32-10) variate streams; the host derives
 * it from the chain's numpy SeedSequence (base.py:88, 293-306).  Replaces GibbsBase.__init__ /
 * _configure (base.py:84-164) and _EtaICARPosterior.__init__ (logit.py:64-71; no dense eigenfactor). */
int occ_create(const occ_problem *problem, int32_t n_chains, const uint64_t *keys, int32_t device,
               occ_sampler **out);
int occ_destroy(occ_sampler *s);
/* Replace the chains' Philox keys (a new sample() call on an existing sampler draws new keys from
 * its generator, exactly as the reference's rng stream simply continues, base.py:88). */
int occ_set_keys(occ_sampler *s, const uint64_t *keys);

/* Starting values of one chain: base.py:188-197 (`start` dict) / 199-212 (default start, drawn by
 * the host with numpy exactly as the reference does).  Resets the chain's iteration counter and the
 * MINRES warm start (logit.py:71).  Reduced-rank model: `eta` points at the m coefficients theta (logit.py:457-460). */
int occ_set_start(occ_sampler *s, int32_t chain, const double *alpha, const double *beta, double tau,
                  const double *eta);

/* One Gibbs iteration of every chain, launched kernel by kernel on one stream in the reference's order:
 * LogitICARGibbs.step() (logit.py:254-266). */
int occ_step(occ_sampler *s);

/* n_iter iterations of every chain; alpha/beta/tau of iterations >= burnin are recorded:
 * GibbsBase._run's loop (base.py:236-239) for all chains at once (gibbs/parallel.py:38-41).
 * out_alpha: [n_chains][n_iter-burnin][q], out_beta: [..][p], out_tau: [n_chains][n_iter-burnin].
 * The iteration is replayed from captured hipGraphs on two streams (omega_a/alpha overlap the eta solve,
 * see DESIGN.md). */
int occ_run(occ_sampler *s, int64_t n_iter, int64_t burnin, double *out_alpha, double *out_beta,
            double *out_tau);

/* State of one chain by name (reference attribute names, base.py:65-82 / logit.py):
 *   alpha(q) beta(p) tau(1) eta(n) z(n) k(n) omega_b(n) omega_a(R) exists(S) xz(2n) rhs(n)
 *   minres_itn(1) iter(1); reduced-rank model: theta(m), and eta is K theta (the reference's `spatial`);
 *   rsr_gram(m*m), for tests: K' diag(omega_b) K of the last theta update up to 128 columns, beyond that the rows of
 *   the factor U (Lam = U'U) right of each 32-row panel's diagonal block (the rest is working storage)
 * occ_get_state copies into out (capacity cap doubles) and stores the length in *len.
 * occ_set_state accepts alpha beta tau eta z omega_a xz iter theta (theta also sets eta = K theta); omega_b of
 * the coming iteration is then redrawn from the new state.  A probit handle's names: occ_problem::link.
 * A read of a name the model does not have: OCC_E_STATE, "unknown state name".  A write of a name that is unknown, read-only
 * or not the model's, and of alpha, beta, tau or iter with another length: "unknown state name or wrong length"; of any other
 * name with another length: "wrong length".  With out = NULL occ_get_state stores the length alone; for these names it is a
 * function of the problem's sizes and nothing is copied off the device.
 * The engine reads all of this -- length, who reads, who writes, where the value lives, whether a write redraws -- off one
 * table, STATE of occuspytial_amd/csrc/occ_names.hpp, which also routes every other family of names below to its own code.
 *
 * Per-site posterior summaries (logit models; ICAR and reduced rank), accumulated on the device by the z update of every
 * KEPT iteration of a chain whose switch is on: an iteration `it` of a call counts when it - (first iteration of the
 * call) >= the call's burnin (occ_step: every step) and it completes.  Five float64 sums per site and one count per chain:
 *   site_psi(n)   sum of psi_i = expit(x_i beta + eta_i), every site            -> / count: posterior mean occupancy probability
 *   site_occ(n)   sum of P(z_i = 1 | alpha, beta, eta, y) of the z update (logit.py:234-252), exactly 1 per iteration at a
 *                 site with a detection                                          -> P(z_i = 1 | data), Rao-Blackwellised
 *   site_z(n)     sum of the new z_i                                             -> raw frequency of occupancy
 *   site_eta(n)   sum of eta_i (reduced rank: (K theta)_i)   site_eta2(n)  sum of eta_i^2   -> mean and sd of the spatial effect
 *   site_count(1) iterations accumulated                     site_stats(1) the chain's switch, 0 / 1
 * occ_set_state "site_stats" 1: allocates at first use (40 n bytes per chain of the handle), ZEROES the chain's sums and
 * count, switches on; 0: switches off, the sums stay readable.  occ_set_state also accepts site_count and the five sums
 * (checkpoint restore), only while the chain's switch is on.  occ_get_state of any of the seven names before the handle's
 * first switch-on: OCC_E_STATE.  The names do not touch the chain's state (nothing is redrawn); occ_set_start and
 * occ_set_keys touch neither switch nor sums; a call that is re-run after a device-side wait gave up (occ_stats::
 * fused_fallbacks) counts no iteration twice; occ_profile and the occ_cond_* entry points never accumulate.  alpha, beta,
 * tau, eta, z are bit-identical with the switch on or off.  A probit handle (link = 1) answers every one of these names
 * with OCC_E_STATE, "site summaries are not available for the probit model".
 *
 * Per-site log-likelihood sums of streaming WAIC (logit models; ICAR and reduced rank), accumulated by the z update over the
 * SAME iterations as the sums above, at the SURVEYED sites only (an unsurveyed site's sums stay exactly 0).  The likelihood
 * is the site's marginal one, z integrated out.  With lsig(a) = min(a, 0) - log1p(exp(-|a|)) and r the site's visit rows:
 *   no detection at the site:  L = D = (1 - psi) + psi prod_r expit(-w_r alpha), the very D the z update divides by; l = log D
 *                              (1 - psi is not subtracted where psi > 1/2: for x_i beta + eta_i = a >= 0 it is exp(-a) psi, so D
 *                              keeps its digits where psi rounds to 1)
 *   a detection at the site:   l = lsig(x_i beta + eta_i) + sum_r lsig(+- w_r alpha), + where y_r = 1, rows in row order; L = exp(l)
 * Three float64 sums per site and one count per chain:
 *   ll_lik(n)    sum of L      -> log(ll_lik / count): the site's log pointwise predictive density
 *   ll_log(n)    sum of l      ll_log2(n)  sum of l^2      -> the variance of l: the site's effective number of parameters
 *   ll_count(1)  iterations accumulated                    ll_stats(1) the chain's switch, 0 / 1
 * The semantics are those of the site_* names, word for word: occ_set_state "ll_stats" 1 allocates at first use (24 n bytes
 * per chain of the handle), ZEROES the chain's three sums and count and switches on; 0 switches off, the sums stay readable;
 * ll_count and the three sums are writable only while on; occ_get_state of any of the five names before the handle's first
 * switch-on: OCC_E_STATE; nothing is redrawn, a re-run call counts nothing twice, occ_profile and occ_cond_* never accumulate;
 * alpha, beta, tau, eta, z are bit-identical with the switch on or off; a probit handle answers every one of the names with
 * OCC_E_STATE.  ll_stats and site_stats are independent of each other: either, both or neither may be on for a chain, and
 * the site_* sums are the same bits with ll_stats on or off.
 *
 * Occupied sites per region and draw (every model: logit ICAR, logit reduced rank, probit): N_g(t) = sum over the sites i of
 * region g of z_i(t), counted on the device by the z update and recorded per KEPT draw of occ_run, like alpha, beta and tau:
 * row t = it - (first iteration of the call) - burnin, 0 <= t < keep.  Sites with a detection count (their z is 1 in every
 * iteration); sites of no region (-1) do not.  Counts are unsigned 32-bit integers added with integer atomics: the same
 * values whatever the path, the placement or the order of addition.
 *   region_id(n)          the HANDLE's map, set and read through any valid chain index: whole numbers in [-1, 256), -1 = no
 *                         region; G = max + 1 >= 1.  Another value: OCC_E_BADARG.  Settable only while no chain of the handle
 *                         has region_stats on (else OCC_E_STATE); allocates at first use.
 *   region_stats(1)       the chain's switch, 0 / 1 (another value: OCC_E_BADARG).
 *   region_draws(keep G)  read-only: the chain's counts of the last completed occ_run, row-major [t][g], as doubles; length 0
 *                         if the chain's switch was off during that call (or no call has completed since).
 * Every one of the three names answers OCC_E_STATE before the handle's first region_id.  Nothing is redrawn; occ_set_start
 * and occ_set_keys touch neither map nor switch; a call that is re-run after a device-side wait gave up counts nothing
 * twice; occ_step, occ_profile and the occ_cond_* entry points never count.  alpha, beta, tau, eta, z and the site_* and
 * ll_* sums are bit-identical with the switch on or off.
 *
 * Sum-to-zero per connected component (ICAR model): on a graph of k > 1 connected components the null space of Q has dimension
 * k, and the ICAR model centres eta on every component, not once over all sites.
 *   component_id(n)       the HANDLE's components, set and read through any valid chain index: whole numbers in [0, n), equal
 *                         numbers = one component.  Validated as a whole: another value is OCC_E_BADARG and nothing changes.
 *                         Settable only before the handle's first iteration (OCC_E_STATE afterwards); reading it before it was
 *                         set: OCC_E_STATE.  A probit or reduced-rank handle answers OCC_E_STATE: its eta = K theta carries no
 *                         constraint.
 * With more than one component a correction pass follows every solve (occ_run, occ_step, occ_cond_eta, and the real iterations
 * occ_profile runs on a fused handle -- whose kernel-by-kernel replays afterwards leave every chain mid-solve, as under the
 * global constraint: eta after occ_profile is no draw of either model, re-start the chains): from the solve's
 * x = Lambda^-1 y and z = Lambda^-1 1, eta_i = x_i + a_c z_i with a_c = -(sum of x over i's component) / (sum of z over it),
 * exactly 0.0 at a component of one site, and beta's partial sums are formed again from that eta.  The sums are added in an
 * order fixed by the labels alone: the same bits on every path and after a resume.  With one component nothing changes: no
 * launch, no allocation, the same bits as without the name.  occ_cond_beta is unchanged; tau_shape is the caller's
 * (0.5 + 0.5 (n - k) for this model).
 *
 * Posterior predictive check of the detection histories (logit models; ICAR and reduced rank), conditional on z: per KEPT draw
 * of occ_run -- row t as above -- of a chain whose switch is on, the z update replicates the detections of every surveyed
 * site i, visit rows r0 <= r < r1, from alpha of the iteration and the NEW z_i:
 *   d_r = expit(w_r alpha), from the dot product and the exponential the update forms anyway;
 *   u_r = the uniform of Philox stream 13 (STREAM_PPC) at sub-stream index r, the FLAT visit row, block 0, first 64-bit word:
 *         what occ_draw(kind 3, key, iteration, 13, R) returns, so a caller can re-draw it;
 *   y_i = sum_r y_r,   E_i = z_i sum_r d_r (rows in row order),   y*_i = z_i sum_r [u_r < d_r];
 *   Freeman-Tukey terms a_i = (sqrt y_i - sqrt E_i)^2 and b_i = (sqrt y*_i - sqrt E_i)^2 (both 0 where z_i = 0: such a site
 *   has had no detection).
 * A row holds four unsigned 64-bit integers: sum_i fx(a_i) (T_obs), sum_i fx(b_i) (T_rep), sum_i y*_i (replicated detections;
 * observed counterpart: sum y) and #{i: y*_i > 0} (replicated sites with a detection; observed: the sites with one), with
 * fx(x) = x 2^32 rounded to nearest.  Fixed point makes every column an integer sum, added with integer atomics: the same
 * values whatever the path, the placement or the order of addition (a term is at most the site's visits and R < 2^31, so a
 * column stays below 2^63; a quantum is 2^-32 = 2.3e-10 per site against terms of order 0.1 to 1).
 *   ppc_stats(1)        the chain's switch, 0 / 1 (another value: OCC_E_BADARG); allocates at first use.
 *   ppc_draws(keep 4)   read-only: the chain's rows of the last completed occ_run, row-major [t][column], as doubles, columns 0
 *                       and 1 multiplied by 2^-32 (exact below 2^53 quanta, otherwise rounded to nearest); length 0 if the
 *                       chain's switch was off during that call (or no call has completed since).
 * Both names answer OCC_E_STATE before the handle's first switch-on, and a probit handle answers them with OCC_E_STATE,
 * "posterior predictive checks are not available for the probit model".  Nothing is redrawn; occ_set_start and occ_set_keys
 * do not touch the switch; a call that is re-run after a device-side wait gave up counts nothing twice; occ_step, occ_profile
 * and the occ_cond_* entry points never count.  alpha, beta, tau, eta, z, the site_* and ll_* sums and region_draws are
 * bit-identical with the switch on or off, and the four switches are independent of each other.
 *
 * Spatial residual check (logit models; ICAR and reduced rank): did the spatial term absorb the spatial structure?  Per KEPT
 * draw of occ_run -- row t as above -- of a chain whose switch is on, with beta, eta (reduced rank: K theta) and the NEW z of
 * the iteration, two kernels launched directly behind the z update form, with weights w_ij = -Q_ij (i != j):
 *   psi_i = expit(x_i beta + eta_i), as site_psi forms it;   r_i = z_i - psi_i;
 *   u_i = the uniform of Philox stream 14 (STREAM_SPATIAL) at sub-stream index i, the site, block 0, first 64-bit word: what
 *         occ_draw(kind 3, key, iteration, 14, n) returns, so a caller can re-draw it;
 *   z*_i = [u_i < psi_i];   r*_i = z*_i - psi_i;   d_i = sum_j w_ij (column order);   S0 = sum_i d_i;
 *   A = sum_i r_i sum_j w_ij r_j,   B = sum_i d_i r_i,   C = sum_i r_i,   D = sum_i r_i^2,   and A*, B*, C*, D* of r*.
 * A row holds eight SIGNED 64-bit integers [A, B, C, D, A*, B*, C*, D*], each the sum over the sites of fx(term) =
 * llrint(term 2^32), added with integer atomics in two's complement: the same values whatever the path, the placement or the
 * order of addition.  Moran's I, centred at rbar = C / n:  I = (n / S0) (A - 2 rbar B + rbar^2 S0) / (D - n rbar^2).
 * Checked at the handle's first switch-on, OCC_E_BADARG otherwise: every off-diagonal of Q <= 0 (a Q that came with a
 * prior_factor may hold positive ones: refused here), 0 < S0 < 2^30 and n < 2^30, so that every column stays below 2^62.
 *   moran_stats(1)
 *       a word of the handle per chain that says whether the chain's kept draws are recorded: 1 or 0, any other value is
 *       OCC_E_BADARG.  It is not one of the z update's outputs above.  The first 1 allocates (the weights, 16 n bytes per chain).
 *   moran_draws(keep 8)
 *       read-only: the chain's rows of the last completed occ_run, row-major [t][column], as doubles multiplied by 2^-32 (exact
 *       below 2^53 quanta, otherwise rounded to nearest); length 0 if the chain's switch was off during that call.
 * Both names answer OCC_E_STATE before the handle's first switch-on (switching a chain off before that is accepted), and a
 * probit handle answers them with OCC_E_STATE, "the spatial residual check is not available for the probit model".  Nothing
 * is redrawn; occ_set_start and occ_set_keys do not touch it; a call that is re-run after a device-side wait gave up counts
 * nothing twice; occ_step, occ_profile and the occ_cond_* entry points never count.  alpha, beta, tau, eta, z, the site_* and
 * ll_* sums, region_draws and ppc_draws are bit-identical with it on or off, and it is independent of the four outputs.
 *
 * Per-site intervals (logit models; ICAR and reduced rank): how sure is the model about psi at a site?  psi lives in (0, 1), so
 * a histogram per site with B equal bins answers every quantile of psi_i to within 1 / B, with an exact bracket, and the
 * chains' histograms merge exactly by addition; the draws are not needed.  Per iteration past the call's burn-in -- the rule of
 * the per-site sums above: `keep` does not matter, so occ_step counts as well -- of a chain whose switch is on, with beta and
 * eta (reduced rank: K theta) of the iteration, one kernel launched directly behind the z update forms
 *   psi_i = expit(x_i beta + eta_i), as the z update forms it;   b = min(B - 1, (int)(psi_i B));
 * and adds 1 to the chain's 32-bit count of (bin b, site i), and 1 to the chain's count of accumulated iterations.  Integer
 * counts: the same values whatever the path, the placement or the block size.  4 B bytes per site and chain.
 *   hist_stats(1)
 *       a word of the handle per chain: 0 is off, B with 4 <= B <= 1024 is on with B bins, any other value is OCC_E_BADARG.  It
 *       is not one of the z update's outputs above.  The first switch-on allocates; switching on ZEROES the chain's histograms
 *       and count; 0 keeps everything readable.  B belongs to the handle: a chain that asks for another B while any chain is on
 *       gets OCC_E_BADARG (the message names the handle's B); with every chain off a new B frees and reallocates, and every
 *       chain's histograms start from zero.
 *   hist_count(1)
 *       the chain's count of accumulated iterations.
 *   hist_counts(B n)
 *       the chain's histograms, bin-major [bin][site], as doubles (32-bit counts: exact).
 * hist_count and hist_counts are writable while the chain's switch is on (checkpoint restore): whole numbers in [0, 2^32),
 * OCC_E_BADARG otherwise.  The handle keeps, per chain, an upper bound on every count -- the iterations past burn-in of every
 * call since the last zeroing, raised to what a write holds -- and occ_run / occ_step refuse with OCC_E_BADARG a call that
 * could take a count past 2^32 - 1.  All three names answer OCC_E_STATE before the handle's first switch-on (switching a chain
 * off before that is accepted), and a probit handle answers them with OCC_E_STATE, "per-site intervals are not available for
 * the probit model".  Nothing is redrawn; occ_set_start and occ_set_keys do not touch them; a call that is re-run after a
 * device-side wait gave up counts nothing twice; occ_profile and the occ_cond_* entry points never count.  alpha, beta, tau,
 * eta, z, every sum and every record above are bit-identical with the switch on or off.
 *
 * Per-site convergence diagnostics (logit models; ICAR and reduced rank): have the chains converged at a site?  R-hat needs
 * each chain's mean and variance, ESS and the Monte-Carlo standard error need the variance of batch means: a handful of
 * running sums per site; the draws are not needed.  Per iteration past the call's burn-in -- the rule of the per-site
 * intervals above, so occ_step counts as well -- of a chain whose switch is on, one kernel launched directly behind the z
 * update does, per site i and for v = psi_i = expit(x_i beta + eta_i) and for v = eta_i (reduced rank: K theta), with
 * m = cnt the site's own count and L the batch length:
 *   if (m == 0) ref = v;   d = v - ref;   s1 += d;   s2 += d d;   run += d;   if ((m + 1) % L == 0) { bsq += run run; run = 0; }
 * then cnt = m + 1, and it adds 1 to the chain's count of accumulated iterations.  A column belongs to one thread and
 * additions run in iteration order: the same values whatever the path, the placement, the block size or the split into
 * calls (an unfinished batch stays in `run` across calls).  88 bytes per site and chain.
 *   conv_stats(1)
 *       a word of the handle per chain: 0 is off, L with 1 <= L <= 2^30 is on with batch length L, any other value is
 *       OCC_E_BADARG.  It is not one of the z update's outputs above.  The first switch-on allocates; switching on ZEROES the
 *       chain's sums and count; 0 keeps everything readable.  L belongs to the handle: a chain that asks for another L while
 *       any chain is on gets OCC_E_BADARG (the message names the handle's L); with every chain off a new L is accepted.
 *   conv_count(1)
 *       the chain's count of accumulated iterations.
 *   conv_sums(11 n)
 *       the chain's sums, slot-major [slot][site]: cnt, then ref, s1, s2, run, bsq of psi, then the same five of eta.
 * conv_count and conv_sums are writable while the chain's switch is on (checkpoint restore): the count and every cnt are
 * whole numbers >= 0 and every cnt of a written conv_sums is the same, OCC_E_BADARG otherwise.  All three names answer
 * OCC_E_STATE before the handle's first switch-on (switching a chain off before that is accepted), and a probit handle answers
 * them with OCC_E_STATE, "per-site convergence diagnostics are not available for the probit model".  Nothing is redrawn;
 * occ_set_start and occ_set_keys do not touch them; a call that is re-run after a device-side wait gave up counts nothing
 * twice; occ_profile and the occ_cond_* entry points never count.  alpha, beta, tau, eta, z, every sum and every record above
 * are bit-identical with the switch on or off.
 *
 * Held-out predictive scoring (logit models; ICAR and reduced rank): how well does the fit predict detection histories it has
 * not seen, at sites it does not survey?  The held-out sites are simply absent from the handle's problem (W, y); their
 * withheld visits are given separately.  The log predictive density of a held-out site needs the mean over the kept draws of
 * the site's marginal likelihood of its withheld history: a handful of running sums; the draws are not needed.  A held-out
 * entry h is a site i with visit rows r = ptr[h] .. ptr[h + 1] - 1, covariates w_r (q columns) and detections y_r.  Per
 * iteration past the call's burn-in -- the rule of the per-site intervals above, so occ_step counts as well -- of a chain
 * whose switch is on, one kernel launched directly behind the z update does, per entry, with a = x_i beta + eta_i (reduced
 * rank: eta = K theta), psi = expit(a), lsig(t) = min(t, 0) - log1p(exp(-|t|)) and P = prod_r expit(-w_r alpha):
 *   no detection in the withheld history:   D = (1 - psi) + psi P,   L = D,   l = log D   (1 - psi as the z update forms it:
 *                                           exp(-a) psi for a >= 0, no subtraction where psi > 1/2)
 *   a detection:                            l = lsig(a) + sum_r lsig(+- w_r alpha)  (+ where y_r = 1, rows in row order),   L = exp(l)
 *   pd = psi (1 - P)                        the predictive probability of at least one detection in these visits
 *   cnt += 1;   sum L += L;   sum l += l;   sum l^2 += l l;   sum pd += pd
 * -- the formulas of the log-likelihood sums above, taken over the withheld rows -- and it adds 1 to the chain's count of
 * accumulated iterations.  A column belongs to one thread and additions run in iteration order: the same values whatever
 * the path, the placement, the block size or the split into calls.  40 bytes per entry and chain.
 *   holdout_data(2 + 2 H + 1 + R + R q)
 *       the handle's withheld data, set and read through any valid chain index: one packed array
 *       [H, R, site[H], ptr[H + 1], y[R], W[R q] row-major].  Validated as a whole, OCC_E_BADARG otherwise and nothing
 *       changes: whole numbers only; 1 <= H; the sites lie in [0, n), are distinct and are NOT surveyed in this handle's
 *       problem; ptr rises from 0 to R with at least one row per entry; y is 0 or 1; W is finite; the length is exactly
 *       2 + 2 H + 1 + R + R q.  Settable only while no chain has holdout_stats on (OCC_E_STATE otherwise).  The first one
 *       allocates; setting it again replaces the data and ZEROES every chain's sums and count.
 *   holdout_stats(1)
 *       a word of the handle per chain, 0 or 1 (any other value is OCC_E_BADARG).  It is not one of the z update's outputs
 *       above.  Switching on ZEROES the chain's sums and count; 0 keeps everything readable.
 *   holdout_count(1)
 *       the chain's count of accumulated iterations.
 *   holdout_sums(5 H)
 *       the chain's sums, slot-major [slot][entry]: cnt, sum L, sum l, sum l^2, sum pd.
 * holdout_count and holdout_sums are writable while the chain's switch is on (checkpoint restore): the count and every cnt
 * are whole numbers >= 0 and every cnt of a written holdout_sums is the same, OCC_E_BADARG otherwise.  All four names answer
 * OCC_E_STATE before the handle's first holdout_data, and a probit handle answers them with OCC_E_STATE, "held-out scoring is
 * not available for the probit model".  Nothing is redrawn; occ_set_start and occ_set_keys do not touch them; a call that is
 * re-run after a device-side wait gave up counts nothing twice; occ_profile and the occ_cond_* entry points never count.
 * alpha, beta, tau, eta, z, every sum and every record above are bit-identical with the switch on or off. */
int occ_get_state(occ_sampler *s, int32_t chain, const char *name, double *out, int64_t cap, int64_t *len);
int occ_set_state(occ_sampler *s, int32_t chain, const char *name, const double *in, int64_t len);

typedef struct occ_stats {
    int64_t iterations;      /* Gibbs iterations completed (chain 0) */
    int64_t graph_launches;  /* hipGraph replays */
    int64_t eager_iterations;
    int64_t stalls;          /* eta solves carried into a second graph replay (more Krylov steps than captured) */
    int32_t krylov_cap;      /* Krylov steps captured per eta solve */
    int32_t krylov_last;     /* MINRES iterations of the last eta solve (chain 0) */
    double krylov_mean;      /* mean MINRES iterations per solve since creation (all chains) */
    int64_t krylov_total;    /* MINRES iterations since creation (all chains) */
    int64_t solves;          /* eta solves since creation (all chains) */
    double last_run_ms;      /* device time of the last occ_run (HIP events on the engine's stream) */
    int32_t n_blocks_sites, n_blocks_rows, threads_per_block, n_chains;
    int32_t persistent_solve; /* 1, 2: fused iteration kernel with the persistent eta solve (k_iter + k_z_ob per iteration;
                                 2: one XCD per chain, its workgroups exchange through that XCD's L2), 0: one launch per
                                 MINRES step, omega_a/alpha/noise on a side stream */
    int32_t solve_workgroups; /* workgroups per chain of the persistent solve */
    int32_t main_stream_cus;  /* > 0: CUs reserved for the main stream (k_iter, k_z_ob); the side stream has the others */
    int32_t fused_fallbacks;  /* calls that were re-run without device-side waits after one of them gave up -- a barrier of the
                                 fused kernel (its workgroups were not resident together) or a hand-over between the two
                                 streams (they were not running beside each other); the engine then runs one launch per
                                 MINRES step (ICAR) / on one stream (reduced-rank model) until a later call finds the device
                                 as creation found it (repromotions) */
    double profile_minres_iterations; /* mean MINRES iterations per solve over the k_iter launches of the last occ_profile */
    int64_t iter_kernel_launches;     /* k_iter launches of the last occ_run ... */
    double iter_kernel_mean_us;       /* ... and their mean duration, first workgroup in to last chain out, by the
                                         device's constant-rate wall clock read inside the kernel */
    /* ABI 5: streams are pooled per (process, device, CU partition) -- a CU-masked stream holds one of the device's 24
     * hardware queues for itself, and a process that oversubscribes them gets its queues time-sliced */
    int32_t repromotions;         /* returns to the fused kernel / device-side hand-overs after a run-time fallback */
    int32_t stream_probes;        /* "do my two streams run beside each other?" asked so far (creation + whenever the
                                     process's set of streams changed before a call) */
    int32_t handover_mode;        /* 2: device-side counters, 1: events (or one stream), between the two streams */
    int32_t stream_pairs_masked;  /* live CU-masked stream pairs of this process on the handle's device ... */
    int32_t stream_pairs_plain;   /* ... and unmasked ones (each pair is shared by all engines that want its partition) */
    int32_t demoted;              /* 1: running without device-side waits after a fallback (see fused_fallbacks) */
    double profile_iter_dispatch_us; /* mean DISPATCH duration of k_iter over the launches of the last occ_profile: start / stop
                                        events of hipExtLaunchKernel, i.e. the begin / end timestamps of the dispatch's
                                        completion signal -- what rocprofv3 --kernel-trace reports for a kernel (launch ramp
                                        and end-of-kernel release included, which the in-kernel clock cannot see) */
    /* ABI 6 */
    int32_t stream_pairs_idle;    /* pairs no engine holds, kept for the next taker of their CU partition (not live) */
    int32_t stream_pairs_evicted; /* idle CU-masked pairs this process destroyed to make room under the cap of four, all devices */
} occ_stats;
int occ_get_stats(occ_sampler *s, occ_stats *out);

/* Per-kernel launch time in the mode occ_run uses: for each kernel kind, `reps` back-to-back launches
 * of that ONE kernel are captured into a hipGraph and bracketed by two HIP events on the engine's
 * stream; total_us[kind] / counts[kind] = kernel duration + one dependent-launch boundary.  k_minres is
 * timed inside a replayed graph of a real solve prefix (k_eta_init + launches 1..8), see occ_gibbs.hip.
 * kinds: 0 omega_b, 1 noise, 2 eta_init, 3 minres, 4 beta_partial, 5 omega_a, 6 alpha_draw,
 * 7 z_ob (beta draw + z update + next iteration's omega_b), 8 iter (the fused iteration kernel k_iter, timed IN SITU
 * first: `reps` real iterations continue the chains, nothing recorded, two HIP events around every k_iter launch
 * on the main stream while the side stream runs omega_a / alpha / noise as in occ_run; counts[8] = launches,
 * total_us[8] = sum of their durations; zero when the engine does not use the fused iteration).
 * The chains are left mid-solve in an unspecified state: call occ_set_start before sampling again. */
#define OCC_N_KERNEL_KINDS 9
int occ_profile(occ_sampler *s, int32_t reps, int64_t counts[OCC_N_KERNEL_KINDS],
                double total_us[OCC_N_KERNEL_KINDS]);

/* ---- chains sharded over GPUs (reference gibbs/parallel.py:4-42 runs one process per chain) -----------
 * Chains are independent: the only communication is ONE broadcast of the fixed problem arrays at set-up, device to
 * device over RCCL (xGMI), called directly -- librccl is opened with dlopen when one of these entry points is first
 * used -- and never a host round trip on the receiving side.  There is no per-iteration collective.
 *
 * In-process (what LogitICARGibbs(..., devices=[...]).sample(chains=N) does; chain c lives on devices[c % G]):
 *   occ_create_group lays the problem out once, uploads it to devices[0], creates one sampler per device and broadcasts
 *   the fixed arrays from devices[0] (ncclCommInitAll + grouped ncclBroadcast; hipMemcpyPeer if librccl is unusable or
 *   OCC_GROUP_TRANSPORT=peer).  keys: the chains' keys, device after device.  Each handle is then driven by its own
 *   host thread (the C ABI holds no global state; ctypes releases the GIL).
 * One process per GPU (bench.py --gpus N under torch.distributed.run, or any launcher that sets RANK / WORLD_SIZE):
 *   occ_comm_unique_id on rank 0 -> the 128 bytes reach the other ranks by any side channel -> occ_comm_create on every
 *   rank (ncclCommInitRank) -> occ_create_distributed: the root lays the problem out and uploads it, the other ranks
 *   (problem = NULL) size their arrays from a small header and receive them by ncclBroadcast.  occ_comm_barrier /
 *   occ_comm_allreduce_max / occ_comm_broadcast_host are the host-side collectives a benchmark needs (staged through
 *   a device buffer).  occ_group_transport says how a handle got its arrays. */
typedef struct occ_comm occ_comm;
int occ_create_group(const occ_problem *problem, int32_t n_devices, const int32_t *devices, const int32_t *chains_per_device,
                     const uint64_t *keys, occ_sampler **out /* n_devices handles */);
int occ_comm_unique_id(uint8_t id[128]);
int occ_comm_create(int32_t world, int32_t rank, const uint8_t id[128], int32_t device, occ_comm **out);
int occ_comm_destroy(occ_comm *comm);
int occ_comm_barrier(occ_comm *comm);
int occ_comm_allreduce_max(occ_comm *comm, double *inout, int32_t n);
int occ_comm_broadcast_host(occ_comm *comm, void *buf, int64_t bytes, int32_t root);
const char *occ_comm_last_error(const occ_comm *comm); /* NULL: error of the last failed occ_comm_create / _unique_id */
int occ_create_distributed(const occ_problem *problem /* root only */, occ_comm *comm, int32_t root, int32_t n_chains,
                           const uint64_t *keys, occ_sampler **out);
const char *occ_group_transport(const occ_sampler *s);
int occ_synchronize(occ_sampler *s); /* the handle's streams have drained (deadline poll), then hipDeviceSynchronize on its device */

/* ---- per-conditional entry points with INJECTED variates ---------------------------------------------------
 * One conditional update of ONE chain of the ICAR model, run on the device by the kernels of the launch-per-step path
 * (grid over that chain only), with the random variates the reference would have drawn supplied by the caller instead
 * of the chain's Philox streams.  Inputs that are not arguments are the chain's current state (occ_set_start /
 * occ_set_state: alpha, beta, tau, eta, z, xz).  They exist so that a test can feed the inputs and the recorded
 * variates of the REFERENCE's own run (tests/golden/\*.npz) and compare with the reference's recorded outputs in one
 * hop (tests/test_gpu_golden.py); the Polya-Gamma variates (omega_b, omega_a) are inputs, since their draw counts are
 * data dependent.  The chain's iteration number does not advance; results are also left in the chain's state, so the
 * calls chain like the reference's _update_* methods.  Call occ_set_start before sampling with the handle again.
 *
 * occ_cond_tau    logit.py:206-209   tau = gamma_variate / (eta'Q eta / 2 + tau_rate), gamma_variate ~ standard
 *                                    gamma(tau_shape) (numpy: rng.gamma(shape, 1 / rate) = standard_gamma(shape) / rate)
 * occ_cond_eta    logit.py:211-217, 73-99   omega_b[n]; eps_site[n] = the first n standard normals; prior_term[n] = the
 *                                    N(0, Q) vector E eps_2 of logit.py:77 BEFORE the sqrt(tau) factor (the engine draws
 *                                    it in edge form, a test passes the reference's).  Uses the chain's beta, z, tau
 *                                    and warm start xz.  Outputs (each may be NULL): the right-hand side y[n],
 *                                    [x z][2n], eta[n], the MINRES iteration count.
 * occ_cond_beta   logit.py:226-232, distributions.pyx:42-110   omega_b[n], eps[p] standard normals; the chain's eta, z
 * occ_cond_alpha  logit.py:180-190, 219-224   omega_a[R] in flat visit-row order (rows of sites that do not exist --
 *                                    no detection and z = 0 -- are ignored), eps[q]; the chain's z
 * occ_cond_z      logit.py:234-252   u[n]: the uniform of site i (sites with a detection ignore theirs); the chain's
 *                                    alpha, beta, eta.  z_out[n] in {0, 1}. */
int occ_cond_tau(occ_sampler *s, int32_t chain, double gamma_variate, double *tau_out);
int occ_cond_eta(occ_sampler *s, int32_t chain, const double *omega_b, const double *eps_site, const double *prior_term,
                 double *rhs_out, double *xz_out, double *eta_out, int32_t *itn_out);
int occ_cond_beta(occ_sampler *s, int32_t chain, const double *omega_b, const double *eps, double *beta_out);
int occ_cond_alpha(occ_sampler *s, int32_t chain, const double *omega_a, const double *eps, double *alpha_out);
int occ_cond_z(occ_sampler *s, int32_t chain, const double *u, double *z_out);

/* Variates of the engine's own generators, drawn ON THE DEVICE by the device functions the kernels use, for the
 * known-answer and distributional tests of the samplers that stand where the reference calls the third-party
 * polyagamma package (logit.py:191-193, 202-204) and numpy's Generator.gamma (logit.py:209): out[i] comes from the
 * sub-stream (key, index i, iteration, stream) exactly as a kernel of the iteration would draw it.
 * kind 0: PG(1, param[i]);  1: standard gamma of shape param[i];  2: standard normal;  3: uniform on (0, 1)
 * (param is ignored for kinds 2 and 3).  Host pointers (or device pointers of `device`); n < 2^31.
 * kind 5: N(param[i], 1) truncated to (0, inf), kind 6: to (-inf, 0) -- the probit model's truncated normal at the uniform of
 * kind 3 from the same sub-stream (one uniform per draw, the inverse CDF).
 * kind 4 is a device self-test, not a variate: n (a multiple of 64) values in param, out[i] = the wave sum of one of four
 * quantities derived from them, NaN where the three forms of the engine's wave sum (plain, four at once, transposed)
 * disagree in a bit (tests/test_gpu_rng.py).
 * The streams (sub-stream index in brackets): 1 omega_b [site], 2 tau's gamma, 3 and 4 the site and edge normals of eta's
 * prior term, 5 beta's normals [coefficient], 6 omega_a [visit row], 7 alpha's normals [coefficient], 8 the uniform of the z
 * update [site], 10 the normals of the reference-form prior draw [column of the factor], 11 and 12 the probit model's eps
 * [site] and coefficient normals [basis column], 13 (STREAM_PPC) the uniform of a replicated detection of the posterior
 * predictive check [flat visit row], 14 (STREAM_SPATIAL) the uniform of a replicated occupancy of the spatial residual check
 * [site].
 * Errors are reported through occ_last_error(NULL). */
int occ_draw(int32_t device, int32_t kind, uint64_t key, uint32_t iteration, uint32_t stream, int64_t n, const double *param,
             double *out);

const char *occ_last_error(const occ_sampler *s); /* NULL handle: error of the last failed occ_create */
int32_t occ_abi_version(void);
int32_t occ_device_count(void);

#ifdef __cplusplus
}
#endif
#endif
