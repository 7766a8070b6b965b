// occ_names.hpp -- the state names of occ_get_state / occ_set_state, described once.  Five families answer a name:
// component_id, the draws of a call (occ_draws.hpp), the accumulators behind the z update (occ_accum.hpp), the per-site
// running sums (SUMS, below) and the plain state of a chain (STATE, below); name_route asks them in that order, for both
// entry points.  A plain name's row says its length, which models read and write it, where its value lives, whether a write
// makes the next call redraw omega_b, and which models' checkpoints hold it; state_refusal words what a mistake earns.  The
// host (occ_gibbs.hip: get / set_plain_state) refuses off the table and switches on `at`; the addresses per model and the
// few computed values are its own.  Plain C++17, no HIP: tests/test_names_cpu.py drives it through occ_plan_capi.cpp.
// To add a state name: DESIGN.md 7.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "occ_accum.hpp"
#include "occ_draws.hpp"

namespace occ {

// ---- the kinds of per-site running sums: their names (occ_gibbs.hip keeps the Ctx members per kind, SUMS_CTX) ------------
// SUMS_SITE: the posterior summaries (state names site_*); SUMS_LL: the log-likelihood sums of streaming WAIC (ll_*).  A kind
// is switched per chain (its bit of ChainScalars::site_on) and is kept in arrays of its own: [nacc C n] sums, [C] counts.
enum : int { SUMS_SITE = 0, SUMS_LL = 1, N_SUMS = 2 };
enum : int { SITE_NONE = -1, SITE_COUNT = -2, SITE_SWITCH = -3 };  // the fields of a kind's names; 0..: the sum's place in the kind's array
struct SumsKind {
    uint32_t bit;  // of ChainScalars::site_on (OUTPUTS)
    int nacc;
    const char *what, *sw, *cnt, *sum[5];  // in messages; state names: switch, count, the sums in their *_NACC order
};
constexpr SumsKind SUMS[N_SUMS] = {
    {OUT_SITE, 5, "site summaries", output_of(OUT_SITE).sw, "site_count", {"site_psi", "site_occ", "site_z", "site_eta", "site_eta2"}},
    {OUT_LL, 3, "log-likelihood sums", output_of(OUT_LL).sw, "ll_count", {"ll_lik", "ll_log", "ll_log2"}}};

// The kind and (*field) the field of a state name; -1 and SITE_NONE for a name that is none of theirs.
inline int sums_lookup(const char *name, int *field)
{
    for (int k = 0; k < N_SUMS; ++k) {
        *field = !std::strcmp(name, SUMS[k].sw) ? SITE_SWITCH : !std::strcmp(name, SUMS[k].cnt) ? SITE_COUNT : SITE_NONE;
        for (int q = 0; q < SUMS[k].nacc; ++q)
            if (!std::strcmp(name, SUMS[k].sum[q])) *field = q;
        if (*field != SITE_NONE) return k;
    }
    return -1;
}

// ---- the plain state of a chain -----------------------------------------------------------------------------------------
enum : unsigned { MODEL_ICAR = 1u, MODEL_RSR = 2u, MODEL_PROBIT = 4u, MODEL_LOGIT = MODEL_ICAR | MODEL_RSR, MODEL_ALL = 7u };
enum : int { UNIT_ONE, UNIT_N, UNIT_S, UNIT_R, UNIT_P, UNIT_Q, UNIT_M, UNIT_TWO_N, UNIT_M_SQ };
// where the value lives: a per-chain device array of doubles, a field of the chain's scalars, a view of the occupancy
// bytes, a value the host computes, a word of the handle
enum : int { AT_ARRAY, AT_SCALARS, AT_Z, AT_COMPUTED, AT_HANDLE };
struct StateDims { size_t n, S, R, p, q, m; };  // m: the reduced-rank dimension, 0 without a basis

struct StateName {
    const char *name;
    int unit;
    unsigned read, write;  // the models that answer a read, that accept a write
    int at;
    bool prologue;         // a successful write on a logit handle sets need_prologue: omega_b of the coming iteration is redrawn
    unsigned ckpt;         // the models whose checkpoint holds it (Engine.checkpoint, in table order)
};
enum : int {
    ST_ALPHA, ST_BETA, ST_TAU, ST_ETA, ST_THETA, ST_Z, ST_XZ, ST_C, ST_EPS, ST_ITER, ST_K, ST_EXISTS, ST_OMEGA_A, ST_OMEGA_B,
    ST_RHS, ST_MINRES_ITN, ST_RSR_GRAM, ST_LINK, ST_DEBUG_CLOSE_WINDOW, ST_DEBUG_MAXITER, N_STATE
};
constexpr StateName STATE[N_STATE] = {
    {"alpha", UNIT_Q, MODEL_ALL, MODEL_ALL, AT_SCALARS, true, MODEL_ALL},
    {"beta", UNIT_P, MODEL_ALL, MODEL_ALL, AT_SCALARS, true, MODEL_ALL},
    {"tau", UNIT_ONE, MODEL_ALL, MODEL_ALL, AT_SCALARS, true, MODEL_ALL},
    {"eta", UNIT_N, MODEL_ALL, MODEL_ALL, AT_ARRAY, true, MODEL_ICAR | MODEL_PROBIT},
    // reduced rank: the coefficients, a write also sets eta = K theta; probit: G c formed on the host, a write sets c, eta, eps
    {"theta", UNIT_M, MODEL_RSR | MODEL_PROBIT, MODEL_RSR | MODEL_PROBIT, AT_COMPUTED, true, MODEL_RSR | MODEL_PROBIT},
    {"z", UNIT_N, MODEL_ALL, MODEL_ALL, AT_Z, true, MODEL_ALL},  // a write takes non-zero as occupied
    {"xz", UNIT_TWO_N, MODEL_LOGIT, MODEL_LOGIT, AT_COMPUTED, true, MODEL_ICAR},  // the MINRES warm start, de-interleaved: x, then z
    {"c", UNIT_M, MODEL_PROBIT, MODEL_PROBIT, AT_ARRAY, false, MODEL_PROBIT},
    {"eps", UNIT_N, MODEL_PROBIT, MODEL_PROBIT, AT_ARRAY, false, MODEL_PROBIT},
    {"iter", UNIT_ONE, MODEL_ALL, MODEL_ALL, AT_SCALARS, true, 0u},  // iterations completed; logit: a write resets the control words
    {"k", UNIT_N, MODEL_ALL, 0u, AT_Z, false, 0u},                    // z - 1/2
    {"exists", UNIT_S, MODEL_ALL, 0u, AT_Z, false, 0u},               // per surveyed site: detected there, or z = 1
    {"omega_a", UNIT_R, MODEL_ALL, MODEL_ALL, AT_ARRAY, true, 0u},
    {"omega_b", UNIT_N, MODEL_ALL, 0u, AT_ARRAY, false, 0u},          // of the last completed iteration (logit: one of two buffers)
    {"rhs", UNIT_N, MODEL_LOGIT, 0u, AT_ARRAY, false, 0u},
    {"minres_itn", UNIT_ONE, MODEL_LOGIT, 0u, AT_SCALARS, false, 0u},
    {"rsr_gram", UNIT_M_SQ, MODEL_RSR, 0u, AT_ARRAY, false, 0u},      // tests only
    {"link", UNIT_ONE, MODEL_PROBIT, 0u, AT_COMPUTED, false, 0u},     // always 1.0: "this handle runs the probit model"
    // tests: the next call's window is opened with zero iterations; the iteration limit of every chain's solve (0: the default)
    {"debug_close_window", UNIT_ONE, 0u, MODEL_LOGIT, AT_HANDLE, false, 0u},
    {"debug_maxiter", UNIT_ONE, 0u, MODEL_LOGIT, AT_HANDLE, true, 0u}};

// The row of a plain state name; -1 for a name that is none.
inline int state_lookup(const char *name)
{
    for (int k = 0; k < N_STATE; ++k)
        if (!std::strcmp(name, STATE[k].name)) return k;
    return -1;
}

// The elements a row holds -- what a write must bring, what a read returns.
constexpr size_t state_length(int row, const StateDims &d)
{
    switch (STATE[row].unit) {
    case UNIT_N: return d.n;
    case UNIT_S: return d.S;
    case UNIT_R: return d.R;
    case UNIT_P: return d.p;
    case UNIT_Q: return d.q;
    case UNIT_M: return d.m;
    case UNIT_TWO_N: return 2 * d.n;
    case UNIT_M_SQ: return d.m * d.m;
    default: return 1;
    }
}

// What keeps `model` (one MODEL_ bit) from reading row `row` (-1: no row), or from writing `len` elements to it: the
// message, or null.  A name the model does not read: "unknown state name".  A name it does not write -- unknown, read-only,
// theta without a basis -- and a wrong length of a name that lives in the chain's scalars: "... or wrong length"; a wrong
// length of any other name: "wrong length".
inline const char *state_refusal(int row, unsigned model, bool write, int64_t len, const StateDims &d)
{
    if (!write) return row >= 0 && (STATE[row].read & model) ? nullptr : "unknown state name";
    if (row < 0 || !(STATE[row].write & model)) return "unknown state name or wrong length";
    if (len == (int64_t)state_length(row, d)) return nullptr;
    return STATE[row].at == AT_SCALARS ? "unknown state name or wrong length" : "wrong length";
}

// ---- one router for every name ------------------------------------------------------------------------------------------
// The family that answers a name, with the kind and the field its own lookup gives (plain state: the row and 0); the families
// in the order occ_get_state and occ_set_state ask them.  A name that is none: FAM_NONE with kind -1, which state_refusal
// words as it words a plain name the model lacks.
enum : int { FAM_NONE = -1, FAM_COMPONENT = 0, FAM_DRAWS = 1, FAM_ACCUM = 2, FAM_SUMS = 3, FAM_STATE = 4 };
struct NameRoute { int family, kind, field; };
inline NameRoute name_route(const char *name)
{
    int field = 0;
    int kind = std::strcmp(name, "component_id") ? -1 : 0;
    if (kind >= 0) return {FAM_COMPONENT, kind, 0};
    if ((kind = draws_lookup(name, &field)) >= 0) return {FAM_DRAWS, kind, field};
    if ((kind = accum_lookup(name, &field)) >= 0) return {FAM_ACCUM, kind, field};
    if ((kind = sums_lookup(name, &field)) >= 0) return {FAM_SUMS, kind, field};
    if ((kind = state_lookup(name)) >= 0) return {FAM_STATE, kind, 0};
    return {FAM_NONE, -1, 0};
}

}  // namespace occ
