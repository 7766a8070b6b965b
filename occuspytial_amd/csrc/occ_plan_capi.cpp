// occ_plan_capi.cpp -- the planner, the launch order and the z update's outputs (occ_plan.hpp), the accumulators behind the z
// update (occ_accum.hpp), the draws of a call (occ_draws.hpp), the state names (occ_names.hpp), a call's host decisions
// (occ_call.hpp) and the problem layout (occ_layout.hpp) behind C entry points for tests/test_plan_cpu.py,
// tests/test_order_cpu.py, tests/test_outputs_cpu.py, tests/test_accum_cpu.py, tests/test_draws_cpu.py, tests/test_names_cpu.py,
// tests/test_call_cpu.py and tests/test_layout_cpu.py (ctypes).  Test infrastructure: `make plan` builds it with g++ into build/; it is never linked
// into libocc_gibbs.so.
#include <cstdio>
#include <cstring>

#include "occ_accum.hpp"
#include "occ_call.hpp"
#include "occ_draws.hpp"
#include "occ_layout.hpp"
#include "occ_names.hpp"

using namespace occ;

extern "C" {

struct OccPlanOut {  // (mirrored by tests/test_plan_cpu.py)
    int32_t form, main_cus, tpb, nb_n, nb_r, beta_split, share_on, surplus_last, iter_window, generic, nbg;
    int32_t tiles_T, tiles_G, xl_wide, xl_nbg, xl_per_cu, main_hot_cus, nmain, partition, flag_sync;
    int32_t per_xcd[XL_SLOTS], tile_first[3][XL_SLOTS + 1], tile_most[3];
    int32_t n_ladder, ladder_form[4], ladder_nbg[4];
};

// shape = {n, rows, chains, p, q, rsr_dim, wmax, dia}.  The plan with the masked pair `granted` or not, settled on the
// ladder's first form (every form resident).  0, or -1 with the planner's error in err.
int occ_plan_eval(const int32_t shape[8], int32_t ncu, const PlanOptions *opt, int32_t granted, OccPlanOut *out, char *err, int32_t errlen)
{
    PlanShape sh;
    sh.n = shape[0]; sh.rows = shape[1]; sh.chains = shape[2]; sh.p = shape[3]; sh.q = shape[4];
    sh.rsr_dim = shape[5]; sh.wmax = shape[6]; sh.dia = shape[7] != 0;
    Plan P;
    std::string why;
    if (!plan_wanted(sh, ncu, *opt, &P, &why)) {
        std::snprintf(err, (size_t)errlen, "%s", why.c_str());
        return -1;
    }
    plan_granted(P, granted != 0);
    plan_settle(P, P.ladder.front().form);
    *out = OccPlanOut{};
    out->form = P.form; out->main_cus = P.main_cus; out->tpb = P.tpb; out->nb_n = P.nb_n; out->nb_r = P.nb_r;
    out->beta_split = P.beta_split; out->share_on = P.share_on; out->surplus_last = P.surplus_last;
    out->iter_window = P.iter_window; out->generic = P.generic; out->nbg = P.nbg;
    out->tiles_T = P.tiles_T; out->tiles_G = P.tiles_G; out->xl_wide = P.xl_wide; out->xl_nbg = P.xl_nbg;
    out->xl_per_cu = P.xl_per_cu; out->main_hot_cus = P.main_hot_cus; out->nmain = P.nmain; out->partition = P.partition;
    out->flag_sync = P.flag_sync;
    for (int x = 0; x < XL_SLOTS; ++x) out->per_xcd[x] = P.per_xcd[x];
    for (int k = 0; k < 3; ++k) {
        for (int x = 0; x <= XL_SLOTS; ++x) out->tile_first[k][x] = P.tile_first[k][x];
        out->tile_most[k] = P.tile_most[k];
    }
    out->n_ladder = (int32_t)P.ladder.size();
    for (size_t i = 0; i < P.ladder.size() && i < 4; ++i) { out->ladder_form[i] = P.ladder[i].form; out->ladder_nbg[i] = P.ladder[i].nbg; }
    return 0;
}

// The scheduling mode of the four flags; -1 where that mode cannot run a solve of shape `solve`.
int32_t occ_order_mode(int32_t flag_sync, int32_t rsr, int32_t event_nodes, int32_t side_enabled, int32_t solve)
{
    const SeqMode m = seq_mode(flag_sync != 0, rsr != 0, event_nodes != 0, side_enabled != 0);
    return seq_mode_runs(m, (SeqSolve)solve) ? (int32_t)m : -1;
}
int32_t occ_order_sequences_per_enqueue(int32_t mode) { return sequences_per_enqueue((SeqMode)mode); }
// The long graph's length; the length of the next replay with `left` sequences to go; whether a mode launches its main graph first
int32_t occ_order_graph_seq_long(void) { return GRAPH_SEQ_LONG; }
int32_t occ_order_graph_len(int64_t left, int32_t have_long) { return graph_len(left, have_long != 0); }
int32_t occ_order_main_first(int32_t mode) { return seq_main_first((SeqMode)mode); }

// What one enqueue of a mode puts `where` (a SeqWhere; 3: an eager sequence instead) from sequence parity p, as
// {kind, e, extra} triples; an event wait / record node is {-1 / -2, e, 0}.  The number of triples, -1 beyond `max`.
// occ_order_launches_comp: the same with `comp` != 0 -- a handle with more than one connected component to centre
// (tests/test_components_cpu.py).
int32_t occ_order_launches_comp(int32_t mode, int32_t where, int32_t solve, int32_t p, int32_t cap, int32_t gate_kernel, int32_t comp, int32_t *out, int32_t max);
int32_t occ_order_launches(int32_t mode, int32_t where, int32_t solve, int32_t p, int32_t cap, int32_t gate_kernel, int32_t *out, int32_t max)
{
    return occ_order_launches_comp(mode, where, solve, p, cap, gate_kernel, 0, out, max);
}
int32_t occ_order_launches_comp(int32_t mode, int32_t where, int32_t solve, int32_t p, int32_t cap, int32_t gate_kernel, int32_t comp, int32_t *out, int32_t max)
{
    const SeqMode m = (SeqMode)mode;
    const SeqParts parts = where == 3 ? seq_eager() : seq_parts(m, (SeqWhere)where);
    int32_t n = 0;
    for (int t = 0; t < (where == 3 ? 1 : sequences_per_enqueue(m)); ++t)
        for (int i = 0; i < parts.n; ++i) {
            auto emit = [&](const SeqLaunch &l) {
                if (n < max) { out[3 * n] = l.kind; out[3 * n + 1] = l.e; out[3 * n + 2] = l.extra; }
                ++n;
            };
            if (parts.part[i] == PART_WAIT || parts.part[i] == PART_RECORD) emit(SeqLaunch{parts.part[i] == PART_WAIT ? -1 : -2, seq_parity(p, t), 0});
            else seq_launches(parts.part[i], (SeqSolve)solve, seq_parity(p, t), cap, where == 3 ? GATE_NONE : seq_gate(m, gate_kernel != 0), emit, comp != 0);
        }
    return n <= max ? n : -1;
}

// The z update's outputs (OUTPUTS): how many; row k's bit with its level, switch name and whether the probit model has it;
// the level that runs while the OR of the chains' site_on is `on`.
int32_t occ_output_count(void) { return N_OUTPUTS; }
uint32_t occ_output_row(int32_t k, int32_t *level, const char **sw, int32_t *probit)
{
    *level = OUTPUTS[k].level; *sw = OUTPUTS[k].sw; *probit = OUTPUTS[k].probit;
    return OUTPUTS[k].bit;
}
int32_t occ_output_level(uint32_t on) { return output_level(on); }

// The accumulators behind the z update (occ_accum.hpp: ACCUM): how many; row k's words -- what messages call it, its four
// state names by field (null: none), its four refusals -- and numbers {elem, slots, cnt_slot}, {on_min, on_max}; then its
// functions as they are.
int32_t occ_accum_count(void) { return N_ACCUM; }
void occ_accum_row(int32_t k, const char **what, const char *name[4], const char *refusal[4], int32_t num[3], double range[2])
{
    const Accum &a = ACCUM[k];
    *what = a.what;
    for (int f = 0; f < 4; ++f) name[f] = a.name[f];
    refusal[0] = a.not_ready; refusal[1] = a.bad_switch; refusal[2] = a.bad_count; refusal[3] = a.bad_data;
    num[0] = a.elem; num[1] = a.slots; num[2] = a.cnt_slot;
    range[0] = a.on_min; range[1] = a.on_max;
}
int64_t occ_accum_words(int32_t k, int64_t C, int64_t unit) { return (int64_t)accum_words(ACCUM[k], (size_t)C, (size_t)unit); }
int64_t occ_accum_offset(int64_t C, int64_t unit, int64_t slot, int64_t chain) { return (int64_t)accum_offset((size_t)C, (size_t)unit, (size_t)slot, (size_t)chain); }
int32_t occ_accum_lookup(const char *name, int32_t *field) { return accum_lookup(name, field); }
int32_t occ_accum_switch_ok(int32_t k, double v) { return accum_switch_ok(ACCUM[k], v); }
const char *occ_accum_write_refusal(int32_t k, int32_t field, const double *in, int64_t len, int64_t unit)
{
    return accum_write_refusal(ACCUM[k], field, in, (size_t)len, (size_t)unit);
}

// The draws of a call (occ_draws.hpp: DRAWS): how many; row k's three state names by field (null: none), its five refusals
// and numbers {elem, is_signed, width, scaled, bit, probit}; then its functions as they are (a raw element as its 64 bits).
int32_t occ_draws_count(void) { return N_DRAWS; }
void occ_draws_row(int32_t k, const char *name[3], const char *refusal[5], int32_t num[6])
{
    const Draws &d = DRAWS[k];
    for (int f = 0; f < 3; ++f) name[f] = d.name[f];
    refusal[0] = d.not_ready; refusal[1] = d.no_probit; refusal[2] = d.bad_switch; refusal[3] = d.read_only; refusal[4] = d.input_locked;
    num[0] = d.elem; num[1] = d.is_signed; num[2] = d.width; num[3] = d.scaled; num[4] = (int32_t)d.bit; num[5] = d.probit;
}
int32_t occ_draws_lookup(const char *name, int32_t *field) { return draws_lookup(name, field); }
double occ_draws_value(int32_t k, uint64_t raw, int64_t col) { return draws_value(DRAWS[k], &raw, (size_t)col); }
int64_t occ_draws_length(int32_t field, int64_t n, int64_t keep, int64_t width) { return (int64_t)draws_length(field, (size_t)n, (size_t)keep, (size_t)width); }

// The state names (occ_names.hpp).  The plain state of a chain (STATE): how many; row k's name and numbers {unit, read, write,
// at, prologue, ckpt}; its length for dims = {n, S, R, p, q, m}; what a read or a write of `len` elements earns (row -1: a
// name that is none).  The kinds of per-site sums (SUMS): how many; row k's words -- what, switch, count, the sums (null: none)
// -- and numbers {bit, nacc}.  The router: out = {family, kind, field}.
static StateDims state_dims(const int64_t d[6]) { return {(size_t)d[0], (size_t)d[1], (size_t)d[2], (size_t)d[3], (size_t)d[4], (size_t)d[5]}; }
int32_t occ_state_count(void) { return N_STATE; }
const char *occ_state_row(int32_t k, int32_t num[6])
{
    const StateName &st = STATE[k];
    num[0] = st.unit; num[1] = (int32_t)st.read; num[2] = (int32_t)st.write; num[3] = st.at; num[4] = st.prologue; num[5] = (int32_t)st.ckpt;
    return st.name;
}
int32_t occ_state_lookup(const char *name) { return state_lookup(name); }
int64_t occ_state_length(int32_t row, const int64_t dims[6]) { return (int64_t)state_length(row, state_dims(dims)); }
const char *occ_state_refusal(int32_t row, uint32_t model, int32_t write, int64_t len, const int64_t dims[6])
{
    return state_refusal(row, model, write != 0, len, state_dims(dims));
}
int32_t occ_sums_count(void) { return N_SUMS; }
void occ_sums_row(int32_t k, const char *word[3], const char *sum[5], int32_t num[2])
{
    const SumsKind &s = SUMS[k];
    word[0] = s.what; word[1] = s.sw; word[2] = s.cnt;
    for (int q = 0; q < 5; ++q) sum[q] = q < s.nacc ? s.sum[q] : nullptr;
    num[0] = (int32_t)s.bit; num[1] = s.nacc;
}
void occ_name_route(const char *name, int32_t out[3])
{
    const NameRoute r = name_route(name);
    out[0] = r.family; out[1] = r.kind; out[2] = r.field;
}

// What a call decides on the host (occ_call.hpp), as it is.  occ_call_head: the steps as {kind, n, from_calib, long_pair} rows,
// -> how many.  occ_call_progress: at = [C]{it, koff, it_base}, seen = [C]{it, koff} (updated) -> the stuck chain or -1.
// occ_call_backoff: one operation (0 arm, 1 fail, 2 pass, 3 due) on state = {wait, step} -> due()'s answer, else 0.
int32_t occ_call_head(int32_t eager_only, int32_t solve, int64_t seq_per_enqueue, int32_t have_graph, int32_t aligned, int64_t n_iter, int32_t need_prologue, int64_t out[3][4])
{
    const CallHead h = call_head(eager_only != 0, (SeqSolve)solve, seq_per_enqueue, have_graph != 0, aligned != 0, n_iter, need_prologue != 0);
    for (int i = 0; i < h.n; ++i) { out[i][0] = h.step[i].kind; out[i][1] = h.step[i].n; out[i][2] = h.step[i].from_calib; out[i][3] = h.step[i].long_pair; }
    return h.n;
}
int64_t occ_call_batch(int64_t left, int64_t graph_launches, int64_t seq_per_enqueue) { return call_batch(left, graph_launches, seq_per_enqueue); }
int32_t occ_call_cap_from_calibration(int32_t calib_max, const char *force) { return cap_from_calibration(calib_max, force); }
int32_t occ_call_cap_resize(int32_t cap, uint64_t d_tot, uint64_t d_sq, uint64_t d_solves) { return cap_resize(cap, d_tot, d_sq, d_solves); }
int32_t occ_call_progress(int32_t C, const uint32_t *at, uint32_t *seen, int64_t n_iter, int64_t *done_min)
{
    std::vector<SeenAt> sn((size_t)C);
    for (int ch = 0; ch < C; ++ch) sn[(size_t)ch] = {seen[2 * ch], seen[2 * ch + 1]};
    const CallProgress r = call_progress(C, [&](int ch) { return ChainAt{at[3 * ch], at[3 * ch + 1], at[3 * ch + 2]}; }, sn.data(), n_iter);
    for (int ch = 0; ch < C; ++ch) { seen[2 * ch] = sn[(size_t)ch].first; seen[2 * ch + 1] = sn[(size_t)ch].second; }
    *done_min = r.done_min;
    return r.stuck;
}
int32_t occ_call_backoff(int32_t state[2], int32_t op)
{
    Backoff b;
    b.wait = state[0]; b.step = state[1];
    const bool due = op == 3 && b.due();
    if (op == 0) b.arm();
    if (op == 1) b.fail();
    if (op == 2) b.pass();
    state[0] = b.wait; state[1] = b.step;
    return due;
}

// The layout of a logit problem, by build_layout's steps in its order (occ_gibbs.hip), plus the probit model's row_t.
// A handle for occ_layout_array / occ_layout_peer, or null with the refusal in err.
struct OccLayout {
    HostLayout L;
    std::vector<int> row_t;
};
OccLayout *occ_layout_build(int32_t n, int32_t S, int32_t R, int32_t p, int32_t q, const int32_t *indptr, const int32_t *indices, const double *data,
                            int32_t has_prior_factor, const double *X, const int32_t *site_id, const int32_t *site_ptr, const double *W,
                            const double *y, const double *a_mu, const double *a_prec, const double *b_mu, const double *b_prec, char *err, int32_t errlen)
{
    OccLayout *h = new OccLayout();
    HostLayout &L = h->L;
    L.n = n; L.S = S; L.R = R; L.p = p; L.q = q;
    std::string why;
    auto build = [&]() {
        const std::vector<int32_t> ip(indptr, indptr + n + 1);
        if (!layout_q_indptr(n, ip, &why)) return false;
        const size_t nnz = (size_t)ip[n];
        L.site_id.assign(site_id, site_id + S);
        L.site_ptr.assign(site_ptr, site_ptr + S + 1);
        if (!layout_site_span(S, R, L.site_ptr, &why)) return false;
        if (!layout_q(n, ip, std::vector<int32_t>(indices, indices + nnz), std::vector<double>(data, data + nnz), has_prior_factor != 0, L, &why)) return false;
        layout_transpose(n, p, std::vector<double>(X, X + (size_t)n * p), L.Xt);
        layout_transpose(R, q, std::vector<double>(W, W + (size_t)R * q), L.Wt);
        if (!layout_sites(n, S, R, L.site_id, L.site_ptr, std::vector<double>(y, y + R), L.site_sidx, h->row_t, L.yrow, L.obs_site, &why)) return false;
        layout_row_site(L);
        layout_hyp(p, q, std::vector<double>(a_mu, a_mu + q), std::vector<double>(a_prec, a_prec + q * q), std::vector<double>(b_mu, b_mu + p),
                   std::vector<double>(b_prec, b_prec + p * p), L.hyp);
        return true;
    };
    if (build()) return h;
    std::snprintf(err, (size_t)errlen, "%s", why.c_str());
    delete h;
    return nullptr;
}

// What a peer sizes from the root's header and sell_ptr (occ_create_distributed), before any array arrives
OccLayout *occ_layout_peer(const OccLayout *root)
{
    OccLayout *h = new OccLayout();
    h->L.sell_ptr = root->L.sell_ptr;
    size_peer_layout(h->L, layout_header(root->L));
    return h;
}

void occ_layout_free(OccLayout *h) { delete h; }

// One array of the layout, by its name in HostLayout, as doubles (ell_w, wmax: one element).  Its length (the first `cap`
// elements are written), -1 for an unknown name.
int64_t occ_layout_array(const OccLayout *h, const char *name, double *out, int64_t cap)
{
    const HostLayout &L = h->L;
    auto give = [&](const auto &v) {
        for (size_t i = 0; i < v.size() && (int64_t)i < cap; ++i) out[i] = (double)v[i];
        return (int64_t)v.size();
    };
#define OCC_LAYOUT_ARRAY(NAME) if (!std::strcmp(name, #NAME)) return give(L.NAME);
    OCC_LAYOUT_ARRAY(sell_ptr) OCC_LAYOUT_ARRAY(sell_col) OCC_LAYOUT_ARRAY(sell_val) OCC_LAYOUT_ARRAY(qdiag) OCC_LAYOUT_ARRAY(dia_off)
    OCC_LAYOUT_ARRAY(dia_val) OCC_LAYOUT_ARRAY(dia_mask) OCC_LAYOUT_ARRAY(Xt) OCC_LAYOUT_ARRAY(Wt) OCC_LAYOUT_ARRAY(yrow) OCC_LAYOUT_ARRAY(row_site)
    OCC_LAYOUT_ARRAY(site_sidx) OCC_LAYOUT_ARRAY(site_id) OCC_LAYOUT_ARRAY(site_ptr) OCC_LAYOUT_ARRAY(obs_site) OCC_LAYOUT_ARRAY(hyp)
#undef OCC_LAYOUT_ARRAY
    if (!std::strcmp(name, "row_t")) return give(h->row_t);
    if (!std::strcmp(name, "ell_w")) return give(std::vector<int>{L.ell_w});
    if (!std::strcmp(name, "wmax")) return give(std::vector<int>{L.wmax()});
    return -1;
}

}  // extern "C"
