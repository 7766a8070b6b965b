// occ_plan.hpp -- the engine's LAUNCH PLAN (fused solve's form, workgroup geometry, CU partition and the XCDs' shares of it),
// plain C++17: a function of the problem's shape, the device's CU count, the plan knobs and whether the CU-masked stream pair
// was granted.  plan_wanted: before the streams are asked for; plan_granted: the rest, with the LADDER of forms the residency
// probes walk (k_tiles -> one XCD per chain -> any placement -> one launch per MINRES step); plan_settle: the form chosen.
// Below the plan: the ORDER of a launch sequence and the scheduling MODE (seq_launches, seq_mode, seq_parts), which the
// engine walks.  tests/test_plan_cpu.py and tests/test_order_cpu.py pin both on the CPU.
#pragma once
#include "../../include/occ_gibbs.h"  // (OCC_N_KERNEL_KINDS)

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

namespace occ {

constexpr int MAXC = 8;                 // covariates of the register-resident fast path (templates on P, Q)
constexpr int NPRE = 8;                 // neighbour slots k_iter fetches before the scalars are known (queen lattice: all)
constexpr int nacc(int d) { return d * (d + 1) / 2 + d; }
constexpr int ITER_WG = 256;            // threads per workgroup of k_iter, any placement
constexpr int ITER_WG_XL = 512;         // ... one XCD per chain: two waves per SIMD IN one workgroup (see k_iter)
constexpr int ITER_SITES_SW = 448;      // ... of which the first wave owns no sites (the scalar wave): seven site waves
constexpr int XL_MAX_WG = 64;           // workgroups per chain of an XCD-local launch (one flag per lane of the polling wave)
constexpr int XL_SLOTS = 8;             // chains of an XCD-local launch = XCDs the grid's x dimension walks over
constexpr int TILE = 256;               // sites per tile of k_tiles
// Workgroups per CU by tiles per workgroup: registers (512 per lane and SIMD: 128 / 168 / 256 per wave at 4 / 3 / 2 workgroups
// of four waves) and LDS (16 KB per tile of the CU's 160 KB).  Tiles per CU: 4, 6, 9, 8.  (constexpr: device code too)
constexpr int tiles_wg_per_cu(int T) { return T == 1 ? 4 : (T == 4 ? 2 : 3); }
constexpr int RSR_MAX_DIM = 128;        // m x m doubles of LDS for the Cholesky factor: 128 KB of the CU's 160 KB
constexpr int TILES_GB_DEFAULT = 1;     // tiles of a k_tiles workgroup whose gathers are in flight together (T = 4, diagonal form)

// The fused solve's forms (= occ_stats::persistent_solve)
enum Form : int { FORM_STEPS = 0 /* one launch per MINRES step */, FORM_ANY = 1, FORM_XCD = 2, FORM_TILES = 3 };

struct PlanShape {  // wmax: the widest SELL-64 slice (off-diagonals of its longest row); dia: Q has the diagonal form
    int n = 0, rows = 0, chains = 1, p = 1, q = 1, rsr_dim = 0, wmax = 0;
    bool dia = false;
};

constexpr int KNOB_UNSET = INT_MIN;  // an integer knob that is not set
struct PlanOptions {  // every knob that shapes the plan; booleans: the variable is set
    bool no_persistent = false, no_tiles = false, no_xcd_local = false, no_scalar_wave = false, no_xcd_shares = false;
    bool no_beta_split = false, no_side_stream = false, stream_events = false, event_sync = false;
    bool skip_residency_probe = false, no_dia = false, no_gram32 = false, gram32_one_chain = false, break_handover = false;
    int force_tiles = KNOB_UNSET, tiles_main_cus = KNOB_UNSET, cold_cus = KNOB_UNSET, cu_split = KNOB_UNSET, main_share = KNOB_UNSET;
    int surplus_last = 0, zob_skip = 0, tiles_gb = TILES_GB_DEFAULT;
};

struct PlanForm {  // nbg: k_iter's workgroups per chain; wide: one XCD per chain with 512-thread workgroups, 1 = a scalar wave
    int form = FORM_STEPS, nbg = 0, wide = 0;  // beside seven site waves, 2 = eight site waves
};

struct Plan {
    PlanShape shape; PlanOptions opt; int ncu = 0;  // the device's CUs
    int tpb = 256, tpb_plain = 256, nbg = 0;  // threads per block (of the device-filling kernels / with no fused form); k_iter's
                                              // workgroups per chain, any placement
    int iter_window = 8;     // neighbour window of k_iter: 8 (two workgroups per CU) or 16 (rows of 9-16 off-diagonals, one per CU)
    bool generic = false;    // more than 8 occupancy or detection covariates: the P = 0 / Q = 0 kernels, launch-per-step path
    bool dia = false, side_enabled = true, event_nodes = true;
    // k_tiles (occ_tiles.hpp): tiles_layout: the problem has its shape (256-thread blocks, the MINRES sums added in groups of
    // T blocks: the launch-per-step kernels follow the same order, KryArgs::group_T); tiles: k_tiles is a candidate
    bool tiles_layout = false, tiles = false;
    int tiles_T = 1, tiles_G = 0, tiles_B = 0, tiles_gb = 1;
    // one XCD per chain (k_iter<8, 1, *>): workgroups per chain and CU, main-stream CUs wanted (0: none), per XCD (0: evenly)
    bool xl = false;
    int xl_wide = 0, xl_nbg = 0, xl_per_cu = 1, xl_main = 0, xl_per_xcd[XL_SLOTS] = {};
    bool any = false, any_fits = false, persistent = false;  // any placement: a candidate / fits; some fused form is
    // the CU partition: wanted (nmain CUs of the main stream, per_xcd on each XCD, the masks), then held (main_cus > 0)
    bool partition = false;
    int nmain = 0, main_cus = 0, main_hot_cus = 0, per_xcd[XL_SLOTS] = {};  // (main_hot_cus: on a chain's XCD)
    std::vector<uint32_t> m_main, m_side;
    int share_on = 0, share_cum[2][XL_SLOTS + 1] = {};
    int nb_n = 0, nb_r = 0, surplus_last = 0, tile_first[3][XL_SLOTS + 1] = {}, tile_most[3] = {};  // -> Ctx
    bool beta_split = false;  // beta drawn by k_beta_draw (one wave per chain) in front of k_z_ob
    int zob_flags = 0;        // OCC_DEBUG_ZOB_SKIP: 8 = no z update, 16 = no omega_b draw
    bool gram32 = false, gram32_pair = false;  // large bases: k_rsr_gram32, two chains per workgroup
    std::vector<PlanForm> ladder;  // the forms the residency probes try, in order; FORM_STEPS at its foot
    int form = FORM_STEPS;    // what creation settled on (plan_settle): the engine comes back to it after a run-time fallback
    bool flag_sync = false;   // ... with device-side hand-overs
};

// Stage 1.  false: an invalid knob, the reason in *err.
inline bool plan_wanted(const PlanShape &sh, int ncu, const PlanOptions &o, Plan *out, std::string *err)
{
    Plan P;
    P.shape = sh; P.opt = o; P.ncu = ncu;
    const int n = sh.n, C = sh.chains, wmax = sh.wmax;
    P.side_enabled = !o.no_side_stream;
    P.event_nodes = P.side_enabled && !o.stream_events;  // diagnostic: fork/join by stream calls
    P.dia = sh.dia && !o.no_dia; P.zob_flags = (o.zob_skip & 3) << 3;
    P.gram32 = sh.rsr_dim > RSR_MAX_DIM && !o.no_gram32; P.gram32_pair = C > 1 && !o.gram32_one_chain;
    // ---- launch geometry: one site (or visit row) per thread; enough blocks to spread over the CUs
    int tpb = 256;
    while (tpb > 64 && ((long long)n * C + tpb - 1) / tpb < 512) tpb >>= 1;
    // CUs of the main stream with k_tiles: half the device (whole shader engines per XCD), OCC_TILES_MAIN_CUS overrides
    int main_t = (ncu / 64) * 32;
    if (o.tiles_main_cus != KNOB_UNSET) main_t = std::max(32, std::min((o.tiles_main_cus / 32) * 32, ncu - 32));
    // Fused iteration kernel (occ_iter.hpp): every workgroup of every chain must be resident at once (at most two
    // per CU) and a matrix row must fit the register-resident neighbour window.  Its partial sums are per
    // 64-site slice, so the other kernels use 64-thread blocks too.
    const int nbg = P.nbg = (n + ITER_WG - 1) / ITER_WG;
    // (k_iter's 240 VGPRs allow two of its workgroups per CU: 8 chains at 100x100 run 210 us per iteration that way
    // against 251 us with one launch per MINRES step)
    P.iter_window = wmax <= 8 ? 8 : 16;
    const int wg_per_cu = P.iter_window == 8 ? 2 : 1;  // 255 and ~400 VGPRs
    P.generic = sh.p > MAXC || sh.q > MAXC;
    const bool fused_shape = sh.rsr_dim == 0 && wmax <= 16 && !P.generic;
    const bool fused_ok = !o.no_persistent && fused_shape;
    bool persistent = fused_ok && (long long)nbg * C <= (long long)wg_per_cu * ncu;
    // k_tiles for what k_iter cannot hold: T tiles of 256 sites per workgroup, four workgroups per CU on HALF the device (the
    // side stream's Polya-Gamma draws need the other half: 1.25 M per iteration at 500x500), at most 512 workgroups per
    // chain (a band's records: one per lane).  The LAYOUT (256-thread blocks, sums grouped by T) follows from the shape
    // alone: OCC_NO_PERSISTENT=1 and a run-time fallback sum in the same order, same bits.
    {
        const int ntile = (n + TILE - 1) / TILE;
        int T = 0;
        for (int t : {1, 2, 4, 3}) {  // the fewest tiles per workgroup whose workgroups are all resident (4 before 3: it keeps its registers)
            const int g = (ntile + t - 1) / t;
            if (T == 0 && (long long)C * g <= (long long)tiles_wg_per_cu(t) * main_t && g <= 512) T = t;
        }
        if (o.force_tiles >= 1 && o.force_tiles <= 4) T = o.force_tiles;  // tests: that many tiles per workgroup whatever the size
        // (beyond 64 workgroups of 512 sites per chain k_iter only has its any-placement form, every exchange a round trip to
        // the memory side: 250x250 x 1 chain 186 us per iteration against 123 with tiles, x 2 chains 322 / 161, 350x350
        // 299 / 152; at 150x150 x 2 chains k_iter still wins, 117 / 136)
        const bool big = n > XL_MAX_WG * ITER_WG_XL && ((long long)nbg * C > 2LL * ncu || (long long)n * C >= 50000);
        P.tiles_layout = fused_shape && wmax <= 8 && T > 0 && !o.no_tiles && (big || o.force_tiles != KNOB_UNSET);
        if (P.tiles_layout) {  // (k_iter's forms are out: decided below)
            P.tiles_T = T; P.tiles_G = (ntile + T - 1) / T; P.tiles_B = (P.tiles_G + XL_SLOTS - 1) / XL_SLOTS;
            persistent = false;
        }
    }
    // one XCD per chain (k_iter<8, 1, *>); candidates -- the probe decides.  Per XCD the main stream has 20 CUs (24 for larger
    // lattices, 28 when few chains leave the side stream little to do), a multiple of four: an XCD deals a chain's workgroups
    // round-robin over its four shader engines (26 workgroups on 26 CUs per XCD dead-locked, on 28 they run).
    //   A  256-thread workgroups, one per CU            nbg <= 20
    //   B  512-thread workgroups (scalar wave + 448 sites), one per CU: ceil(n / 448) <= 28 CUs of the chain's XCD
    //   C  256-thread workgroups, two per CU            nbg <= 64 (partition of at most 24 CUs per XCD, else none)
    // Form B with fewer than eight chains: only the XCDs that host a chain need that many CUs -- the others give the
    // main stream fewer, so that the side stream keeps its share of the device (4 chains at 100x100: 24 CUs on four
    // XCDs, 16 on the other four: 160 + 96 as before).
    {
        const int nbg512 = (n + ITER_SITES_SW - 1) / ITER_SITES_SW;  // (one wave of the 512 threads owns no sites)
        const int nbg512p = (n + ITER_WG_XL - 1) / ITER_WG_XL;       // (eight site waves)
        const int base = (ncu * 5 / 64) * 8;                          // 160 of 256
        // (more than eight chains: launches of eight, one behind the other -- 16 chains at 100x100: 2 x 60 us, launch per
        // step 374; rows of 9-16 off-diagonals take the one-XCD form too, 256 threads, one workgroup per CU: round 3)
        const bool xl_any = fused_ok && C <= 8 * XL_SLOTS && !o.no_xcd_local;
        const bool xl_ok = xl_any && P.iter_window == 8;
        auto part = [&](int per_xcd) { return std::max(32 * ((per_xcd + 3) / 4), base); };
        const int need = 4 * ((nbg512 + 3) / 4), hot = std::min(C, XL_SLOTS), per_xcd = ncu / XL_SLOTS;
        int wide_main = 0, wide_xcd[XL_SLOTS] = {};
        if (need <= per_xcd - 4) {  // the hot XCDs leave the side stream one CU per shader engine at least
            int rest = need;
            if (hot < XL_SLOTS) {
                rest = 4 * (int)std::lround((double)(base - hot * need) / (4.0 * (XL_SLOTS - hot)));
                rest = std::max(8, std::min(rest, need));
                while (hot * need + (XL_SLOTS - hot) * rest > ncu - 96 && rest > 8) rest -= 4;  // the side stream keeps 96 CUs
                if (o.cold_cus != KNOB_UNSET) rest = std::max(4, std::min(o.cold_cus / 4 * 4, need));  // developer knob
            }
            for (int x = 0; x < XL_SLOTS; ++x) { wide_xcd[x] = x < hot ? need : rest; wide_main += wide_xcd[x]; }
        }
        if (xl_any && nbg <= base / XL_SLOTS) {
            P.xl = true; P.xl_wide = 0; P.xl_nbg = nbg; P.xl_per_cu = 1; P.xl_main = base;
        } else if (xl_ok && nbg512 <= 64 && wide_main > 0 && wide_main <= ncu - 96 && hot <= 5 && !o.no_scalar_wave) {
            // (the scalar wave's seventh of the sites costs CUs: taken while the side stream keeps its 96 and most of them on
            // XCDs without a chain -- 100x100: 4 chains 70.0 us per iteration against 80.0 with eight site waves, 5 chains
            // 80.3 / 81.8, 6 chains 99.3 / 82.3; 8 chains on 192 + 64 CUs 121.7 / 92.5, side-stream bound)
            P.xl = true; P.xl_wide = 1; P.xl_nbg = nbg512; P.xl_per_cu = 1; P.xl_main = wide_main;
            for (int x = 0; x < XL_SLOTS; ++x) P.xl_per_xcd[x] = wide_xcd[x];
        } else if (xl_ok && nbg512p <= 64 && (part(nbg512p) <= ncu - 64 || (part(nbg512p) <= ncu - 32 && C <= 2))) {
            P.xl = true; P.xl_wide = 2; P.xl_nbg = nbg512p; P.xl_per_cu = 1; P.xl_main = part(nbg512p);
        } else if (xl_ok && nbg <= 64 && nbg <= 2 * (ncu / XL_SLOTS)) {
            P.xl = true; P.xl_wide = 0; P.xl_nbg = nbg; P.xl_per_cu = 2;
            P.xl_main = part((nbg + 1) / 2) <= ncu - 64 ? part((nbg + 1) / 2) : 0;  // 0: no CU partition
        }
    }
    P.any = persistent;  // what holds without the XCD-local form
    persistent = persistent || P.xl;
    if (P.tiles_layout) {
        P.xl = P.any = false;
        persistent = P.tiles = fused_ok;
        tpb = TILE;
        P.tiles_gb = P.dia && P.tiles_T == 4 && (o.tiles_gb == 2 || o.tiles_gb == 4) ? o.tiles_gb : 1;
    }
    P.tpb_plain = tpb, P.tpb = persistent && !P.tiles ? 64 : tpb, P.persistent = persistent;
    // ---- the CU partition: the main stream (the eta solve) and the side stream (omega_a / alpha / noise) on DISJOINT CUs with
    // the fused kernel -- latency-bound k_iter waves lose more to Polya-Gamma waves on their SIMDs than the side work gains
    // (100x100, 4 chains: 143 -> 127 us per iteration).  A mask of N bits enables N CUs spread evenly over the 8 XCDs
    // (tools/xcc_probe3.hip); k_iter's grid is dealt round-robin over them: a multiple of 8 keeps one workgroup per CU.
    // at least 5/8 of the device for the main stream: k_z_ob's Polya-Gamma draws run there too
    int nmain = std::max(((nbg * C + 7) / 8) * 8, (ncu * 5 / 64) * 8);
    // more workgroups than the partition can give one CU each: the 8-wide window runs two per CU
    if (nmain > ncu - 32 && P.iter_window == 8) nmain = std::max((((nbg * C + 1) / 2 + 7) / 8) * 8, (ncu * 5 / 64) * 8);
    // one XCD per chain: a chain's nbg workgroups share the nmain / 8 CUs of one XCD whatever the number of chains
    if (P.xl) nmain = P.xl_main;  // 0: none
    if (sh.rsr_dim > 0) nmain = ((ncu * 3 / 4) / 8) * 8;  // reduced-rank model: k_rsr_gram's tiles and the theta solve
    // ... with a large basis (the m x m system in device memory: k_rsr_gram32, k_rsrb_*) the main sequence is milliseconds of
    // device-filling kernels and the side sequence 30 us: no partition, one stream (round 3 kept 64 CUs for a side stream
    // whose k_omega_a spent 4.3 ms of a 4.4 ms iteration waiting at its gate)
    if (sh.rsr_dim > RSR_MAX_DIM) nmain = 0;
    if (P.tiles) nmain = main_t;  // k_tiles: eight tiles per CU
    if (o.cu_split != KNOB_UNSET) {              // developer knob: CUs of the main stream; 0: no masks
        nmain = o.cu_split;
        // a partition is cut in whole shader engines per XCD (see above): multiples of 32 CUs, both streams non-empty
        if (nmain != 0 && (nmain < 32 || nmain % 32 != 0 || nmain > ncu - 32)) {
            *err = "OCC_CU_SPLIT must be 0 (no partition) or a multiple of 32 that leaves the side stream at least 32 CUs";
            return false;
        }
    }
    P.nmain = nmain;
    P.partition = (persistent || sh.rsr_dim > 0) && P.side_enabled && nmain >= 8 && nmain <= ncu - 32;
    if (P.partition) {
        // bit i of a mask is CU i / 8 of XCD i % 8: the main stream takes the first per_xcd[x] CUs of XCD x
        P.m_main.assign((ncu + 31) / 32, 0u); P.m_side.assign((ncu + 31) / 32, 0u);
        int *per = P.per_xcd;
        for (int x = 0; x < XL_SLOTS; ++x) per[x] = (P.xl && P.xl_per_xcd[0] > 0 && o.cu_split == KNOB_UNSET) ? P.xl_per_xcd[x] : nmain / XL_SLOTS;
        for (int i = 0; i < ncu; ++i) (i / XL_SLOTS < per[i % XL_SLOTS] ? P.m_main : P.m_side)[i / 32] |= 1u << (i % 32);
        P.main_hot_cus = per[0];
        // the XCDs' shares of each stream's CUs (tile_of_block_shared) when they differ; tile tables: plan_granted
        for (int x = 0; x < XL_SLOTS; ++x) {
            P.share_cum[0][x + 1] = P.share_cum[0][x] + per[x];
            P.share_cum[1][x + 1] = P.share_cum[1][x] + (ncu / XL_SLOTS - per[x]);
            if (per[x] != per[0]) P.share_on = 1;
        }
        if (o.no_xcd_shares) P.share_on = 0;
    }
    *out = P;
    return true;
}

// Stage 2: the masked pair was (not) granted.  Arithmetic first (workgroups against the CUs the main stream owns); the
// RESIDENCY PROBES -- k_iter itself, one barrier per chain -- walk the ladder and have the last word.
inline void plan_granted(Plan &P, bool granted)
{
    const PlanOptions &o = P.opt;
    const int n = P.shape.n, C = P.shape.chains;
    granted = granted && P.partition;
    P.main_cus = granted ? P.nmain : 0;
    P.share_on = granted ? P.share_on : 0;
    const int cus = P.main_cus > 0 ? P.main_cus : P.ncu;
    P.any_fits = P.any && (long long)P.nbg * C <= (long long)(P.iter_window == 8 ? 2 : 1) * cus;
    const bool trust = o.skip_residency_probe;  // tests of the run-time fallback
    const int hot_cus = P.main_cus > 0 ? P.main_hot_cus : P.ncu / XL_SLOTS;  // CUs of a chain's XCD
    if (!trust && P.xl && P.xl_nbg > P.xl_per_cu * hot_cus) P.xl = false;
    if (P.tiles && !trust && (long long)P.tiles_G * C > (long long)tiles_wg_per_cu(P.tiles_T) * cus) P.tiles = false;
    P.persistent = P.xl || P.any_fits || P.tiles;
    if (!P.persistent) P.tpb = P.tpb_plain;
    if (!P.persistent && P.shape.rsr_dim == 0) P.main_cus = P.share_on = 0;  // the partition is for the fused kernel's sake
    const int tpb = P.tpb, nb_n = P.nb_n = (n + tpb - 1) / tpb;
    P.beta_split = tpb != 64 && nb_n >= 128 && !o.no_beta_split;
    P.nb_r = std::max(1, (P.shape.rows + tpb - 1) / tpb);
    if (P.share_on) {  // tiles of the device-filling kernels per XCD, in proportion to the CUs of their stream
        const int per_chain[3] = {tpb == 64 ? 2 * ((n + 255) / 256) : 2 * P.nb_n, P.nb_r, (n + 255) / 256}, which[3] = {0, 1, 1};
        P.surplus_last = o.surplus_last;
        if (o.main_share != KNOB_UNSET) {  // developer knob: weight of an XCD without a chain in k_z_ob's shares
            const int w = o.main_share, hot = std::min(C, XL_SLOTS);
            for (int x = hot; x < XL_SLOTS; ++x) P.share_cum[0][x + 1] = P.share_cum[0][x] + w;
        }
        for (int k = 0; k < 3; ++k) {
            const long long T = (long long)per_chain[k] * C, W = P.share_cum[which[k]][8];
            for (int x = 0; x <= XL_SLOTS; ++x) P.tile_first[k][x] = (int)(T * P.share_cum[which[k]][x] / W);
            for (int x = 0; x < XL_SLOTS; ++x) P.tile_most[k] = std::max(P.tile_most[k], P.tile_first[k][x + 1] - P.tile_first[k][x]);
        }
    }
    // k_tiles (which excludes the other two) or one XCD per chain, then any placement, else one launch per MINRES step
    if (P.tiles) P.ladder.push_back({FORM_TILES, P.nbg, 0});
    if (P.xl) P.ladder.push_back({FORM_XCD, P.xl_nbg, P.xl_wide});
    if (P.any_fits) P.ladder.push_back({FORM_ANY, P.nbg, 0});
    P.ladder.push_back({FORM_STEPS, P.nbg, 0});
}

// The probes chose `form`: launch per step after a fused form was wanted gives the partition up (ICAR model).
inline void plan_settle(Plan &P, int form)
{
    P.form = form;
    if (form == FORM_STEPS && P.persistent) P.main_cus = P.share_on = 0;
    P.flag_sync = P.main_cus > 0 && !P.opt.event_sync;
}

// ---- the ORDER of a launch sequence and the engine's scheduling MODE ---------------------------------------------------
// A launch sequence is one Gibbs iteration of every chain (or a carried solve).  It has three PARTS, and every scheduling
// mode is a way of laying them on the two streams (tests/test_order_cpu.py pins all of it):
//   SIDE   k_omega_a (with alpha's draw), k_noise of the NEXT iteration: inputs are last iteration's alpha and z
//   SOLVE  the eta conditional: k_iter, or k_eta_init / k_minres ... / k_beta_partial, or the reduced-rank three
//   TAIL   k_z_ob (beta, z, omega_b): after both
// The kernel kinds: occ_profile's indices first (include/occ_gibbs.h), then the ones it does not report.
enum Kind { K_OMEGA_B = 0, K_NOISE, K_ETA_INIT, K_MINRES, K_BETA_PARTIAL, K_OMEGA_A, K_ALPHA_DRAW, K_Z_OB, K_ITER, K_GATE /* internal: not a profiled kind */,
            K_RSR_GRAM, K_RSR_SOLVE, K_RSR_ETA_BETA /* reduced-rank model */,
            K_COMP_PART, K_COMP_COEF, K_COMP_ETA, K_COMP_BETA /* sum-to-zero per component: occ_comp.hpp */ };
static_assert(K_ITER + 1 == OCC_N_KERNEL_KINDS, "kernel kinds out of sync with the header");

// launch sequences (iterations) per captured graph on the paths that need no host decision between iterations:
// even, so that the sequence parity is the same at every replay; a graph boundary costs several microseconds
constexpr int GRAPH_SEQ = 2;
// ... and per LONG graph, captured beside the short one when a call has that many iterations to run.  The boundary between two
// replays costs the device about 9 us on each stream (profiles/call_cost_timeline.txt: nothing runs between the last kernel
// of one replay and the first of the next, although the host enqueued both long before): 4.5 us per iteration with the
// short graph alone.  A batch is cut into long replays while that many sequences are left, then short ones: no surplus
// sequence beyond the short graph's.
constexpr int GRAPH_SEQ_LONG = 8;
constexpr int graph_len(long long left, bool have_long) { return have_long && left >= GRAPH_SEQ_LONG ? GRAPH_SEQ_LONG : GRAPH_SEQ; }

enum SeqMode : int {
    SEQ_COUNTERS = 0,        // hand-overs by device counters: two graphs of GRAPH_SEQ sequences, main and side
    SEQ_RSR_ONE_STREAM = 1,  // reduced-rank model without them: one graph of GRAPH_SEQ sequences
    SEQ_EVENT_NODES = 2,     // per-parity graphs that carry their own event waits and records
    SEQ_STREAM_EVENTS = 3,   // per-parity graphs, fork / join by stream calls, k_z_ob behind them (diagnostic)
    SEQ_ONE_STREAM = 4       // the same graphs one behind the other on the main stream (diagnostic)
};
constexpr SeqMode seq_mode(bool flag_sync, bool rsr, bool event_nodes, bool side_enabled)
{
    return flag_sync ? SEQ_COUNTERS : rsr ? SEQ_RSR_ONE_STREAM : event_nodes ? SEQ_EVENT_NODES : side_enabled ? SEQ_STREAM_EVENTS : SEQ_ONE_STREAM;
}
constexpr int sequences_per_enqueue(SeqMode m) { return m <= SEQ_RSR_ONE_STREAM ? GRAPH_SEQ : 1; }
constexpr int seq_parity(int p, int t) { return p ^ (t & 1); }  // of sequence t of a graph captured at parity p

// The shape of the solve.  CAPTURED / EAGER: one launch per MINRES step, a fixed number of them in a graph / the host
// watching the chains' `done` flags between launches.
enum SeqSolve : int { SOLVE_RSR = 0, SOLVE_FUSED, SOLVE_CAPTURED, SOLVE_EAGER };
// The counters' graphs hold GRAPH_SEQ whole sequences: a solve the host has to size or watch cannot stand in them.
constexpr bool seq_mode_runs(SeqMode m, SeqSolve sv) { return m == SEQ_COUNTERS ? sv <= SOLVE_FUSED : m != SEQ_RSR_ONE_STREAM || sv == SOLVE_RSR; }
// The side stream's gate (it waits for the previous k_z_ob's counter): none without counters; else the head of k_omega_a,
// or a kernel of its own (OCC_GATE_KERNEL, diagnostic: as until round 3)
enum SeqGate : int { GATE_NONE = 0, GATE_IN_OMEGA_A, GATE_KERNEL };
constexpr SeqGate seq_gate(SeqMode m, bool as_kernel) { return m != SEQ_COUNTERS ? GATE_NONE : as_kernel ? GATE_KERNEL : GATE_IN_OMEGA_A; }

enum SeqPart : int { PART_SIDE = 0, PART_SOLVE, PART_TAIL, PART_WAIT /* event wait node */, PART_RECORD /* event record node */ };
struct SeqLaunch { int kind, e, extra; };
// SOLVE_EAGER: the host-watched stretch of k_minres launches stands where this `extra` of a K_MINRES is; the last launch's
// number is K_BETA_PARTIAL's extra
constexpr int EXTRA_HOST_WATCHED = -1, EXTRA_K_LAST = -2;

// The launches of one part with sequence parity e, in order, handed to emit(SeqLaunch).  cap: the captured Krylov cap
// (iteration j of a solve is tested by launch j + 3: cap + 3 launches).  comp: the handle has more than one connected
// component to centre (ICAR model, state name component_id) -- the correction pass stands behind the solve's last launch,
// whatever the solve's shape, and so in front of the z update.  A solve that is carried to the next sequence is a decision of
// the device (Ctl::koff): the four launches stand in every sequence and leave a carrying chain alone, as k_z_ob does.
template <class Emit>
void seq_launches(SeqPart part, SeqSolve sv, int e, int cap, SeqGate gate, Emit &&emit, bool comp = false)
{
    auto correction = [&]() {
        if (comp)
            for (int k : {K_COMP_PART, K_COMP_COEF, K_COMP_ETA, K_COMP_BETA}) emit(SeqLaunch{k, e, 0});
    };
    switch (part) {
        case PART_SIDE:
            if (gate == GATE_KERNEL) emit(SeqLaunch{K_GATE, 0, 0});
            emit(SeqLaunch{K_OMEGA_A, e, gate == GATE_IN_OMEGA_A ? 1 : 0});
            emit(SeqLaunch{K_NOISE, e, 1});  // ahead = 1: the coming iteration's
            break;
        case PART_SOLVE:
            if (sv == SOLVE_RSR)  // the theta conditional stands where the ICAR solve is
                for (int k : {K_RSR_GRAM, K_RSR_SOLVE, K_RSR_ETA_BETA}) emit(SeqLaunch{k, e, 0});
            if (sv == SOLVE_FUSED) {
                emit(SeqLaunch{K_ITER, e, 0});
                correction();
            }
            if (sv <= SOLVE_FUSED) break;
            emit(SeqLaunch{K_ETA_INIT, e, 0});  // one launch per MINRES step
            if (sv == SOLVE_EAGER) emit(SeqLaunch{K_MINRES, e, EXTRA_HOST_WATCHED});
            else for (int k = 1; k <= cap + 3; ++k) emit(SeqLaunch{K_MINRES, e, k});
            emit(SeqLaunch{K_BETA_PARTIAL, e, sv == SOLVE_EAGER ? EXTRA_K_LAST : cap + 3});
            correction();
            break;
        case PART_TAIL: emit(SeqLaunch{K_Z_OB, e, 0}); break;
        default: break;  // (the event nodes are the engine's: no launch)
    }
}

// What a mode lays where, per sequence: the main-stream graph, the side graph, and what is enqueued eagerly behind the
// graphs.  The graphs of the first two modes hold GRAPH_SEQ sequences of alternating parity, the others one per parity.
enum SeqWhere : int { ON_MAIN = 0, ON_SIDE, BEHIND };
struct SeqParts { int n; SeqPart part[4]; };
constexpr SeqParts seq_parts(SeqMode m, SeqWhere w)
{
    switch (m) {
        case SEQ_COUNTERS: return w == ON_MAIN ? SeqParts{2, {PART_SOLVE, PART_TAIL}} : w == ON_SIDE ? SeqParts{1, {PART_SIDE}} : SeqParts{0, {}};
        case SEQ_RSR_ONE_STREAM: return w == ON_MAIN ? SeqParts{3, {PART_SIDE, PART_SOLVE, PART_TAIL}} : SeqParts{0, {}};
        case SEQ_EVENT_NODES:  // main: ... -> wait(side chain of this iteration) -> k_z_ob -> record; side: wait(previous k_z_ob) -> ... -> record
            return w == ON_MAIN ? SeqParts{4, {PART_SOLVE, PART_WAIT, PART_TAIL, PART_RECORD}} : w == ON_SIDE ? SeqParts{3, {PART_WAIT, PART_SIDE, PART_RECORD}} : SeqParts{0, {}};
        default: return w == ON_MAIN ? SeqParts{1, {PART_SOLVE}} : w == ON_SIDE ? SeqParts{1, {PART_SIDE}} : SeqParts{1, {PART_TAIL}};
    }
}
// Which stream's graph an enqueue launches FIRST.  With the counters: the main stream's.  On an idle device (the head of a
// call) k_iter is then resident and through the part of its head that needs no noise while the host launches the side
// graph; the noise itself was left by the previous call, but it is ANNOUNCED by the gate at the head of this sequence's
// k_omega_a (SYNC_NOISE), so k_iter's bounded wait ends when that kernel starts -- the wait it has in every sequence, for
// microseconds of host time here.  The side stream is released by the main stream's kernels, never the other way round.
// Measured: the 20-iteration call 7 to 15 us shorter than with the side graph first, two sessions of six alternating runs
// whose ranges overlap (profiles/call_cost_ab.txt): a small gain.  The event modes launch the side graph first, as they did.
constexpr bool seq_main_first(SeqMode m) { return m == SEQ_COUNTERS; }
// An eager sequence in every mode: everything on the main stream, the reference's order of conditionals (logit.py:254-266)
// with omega_a / alpha moved up front -- stream order is the synchronisation
constexpr SeqParts seq_eager() { return SeqParts{3, {PART_SIDE, PART_SOLVE, PART_TAIL}}; }

// ---- the z update's optional OUTPUTS ---------------------------------------------------------------------------------
// Each is switched per chain by a state name and is a bit of ChainScalars::site_on.  Its LEVEL is the STATS value of the
// kernel family that serves it where k_z_ob stands (0: k_z_ob itself); a family also serves every output below its own.
// probit: the probit model has the output too.  tests/test_outputs_cpu.py pins the table and output_level.
constexpr uint32_t OUT_SITE = 1u, OUT_LL = 2u, OUT_REGION = 4u, OUT_PPC = 8u;
struct Output { uint32_t bit; int level; const char *sw; bool probit; };
constexpr int N_OUTPUTS = 4;
constexpr Output OUTPUTS[N_OUTPUTS] = {{OUT_SITE, 1, "site_stats", false},      // per-site posterior sums: k_z_ob_stats
                                       {OUT_LL, 2, "ll_stats", false},          // log-likelihood sums of streaming WAIC: k_z_ob_ll
                                       {OUT_REGION, 3, "region_stats", true},   // occupied sites per region and draw: k_z_ob_occ
                                       {OUT_PPC, 4, "ppc_stats", false}};       // posterior predictive check: k_z_ob_ppc
constexpr const Output &output_of(uint32_t bit) { return OUTPUTS[bit == OUT_SITE ? 0 : bit == OUT_LL ? 1 : bit == OUT_REGION ? 2 : 3]; }
static_assert(output_of(OUT_SITE).bit == OUT_SITE && output_of(OUT_LL).bit == OUT_LL && output_of(OUT_REGION).bit == OUT_REGION && output_of(OUT_PPC).bit == OUT_PPC, "output_of");
// The level that must run while the OR of every chain's site_on is `on`: the highest whose bit is set (unknown bits: none)
constexpr int output_level(uint32_t on)
{
    int level = 0;
    for (int k = 0; k < N_OUTPUTS; ++k)
        if ((on & OUTPUTS[k].bit) && OUTPUTS[k].level > level) level = OUTPUTS[k].level;
    return level;
}

}  // namespace occ
