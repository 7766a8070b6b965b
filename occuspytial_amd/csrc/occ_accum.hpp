// occ_accum.hpp -- the accumulators behind the z update, described once: the per-site intervals (occ_hist.hpp), the per-site
// convergence diagnostics (occ_conv.hpp) and the held-out predictive scoring (occ_holdout.hpp).  Each keeps running sums on
// the device -- `slots` arrays of [C][unit] elements, unit being the per-chain, per-slot length (B n, n or H), and [C] counts
// of accumulated iterations -- updated by one kernel launched directly behind the z update while a chain's switch, a word of
// the handle, is on.  Whatever the host does for them -- names, refusals, addresses, what a write may hold -- is read off this
// table (occ_gibbs.hip: ACCUM loops and get / set_accum_state); the kernels and their argument blocks are the kinds' own.
// Plain C++17, no HIP: tests/test_accum_cpu.py drives it through occ_plan_capi.cpp.  To add an accumulator: a row here, a
// kernel unit with its *Args block, its run-time struct in occ_sampler and its case in accum_switch_on.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstring>

namespace occ {

enum : int { ACC_HIST = 0, ACC_CONV = 1, ACC_HOLD = 2, N_ACCUM = 3 };
enum : int { ACC_NONE = -1, ACC_SWITCH = 0, ACC_COUNT = 1, ACC_DATA = 2, ACC_INPUT = 3 };  // the fields of a kind's state names

struct Accum {
    const char *what, *verb;      // in messages: "<what> <verb> not available for the probit model"
    const char *name[4];          // state names by field; input: what the handle must be given before the first switch-on (or none)
    int elem, slots;              // bytes per element (4: uint32 counts, 8: float64 sums, the count alike); arrays of [C][unit]
    bool cnt_slot;                // slot 0 of the data is the columns' own count: whole, and one number at every column
    double on_min, on_max;        // the switch is 0 (off) or a whole number in [on_min, on_max]
    const char *not_ready, *bad_switch, *bad_count, *bad_data;  // refusals, word for word
};
constexpr Accum ACCUM[N_ACCUM] = {
    // histograms of psi, chain-major [C][B][n]: one slot of unit B n; the switch is the number of bins B
    {"per-site intervals", "are", {"hist_stats", "hist_count", "hist_counts", nullptr}, 4, 1, false, 4.0, 1024.0,
     "per-site intervals have not been switched on for this handle (set hist_stats first)", "hist_stats is 0 or a number of bins from 4 to 1024",
     "hist_count and hist_counts are whole numbers in [0, 2^32)", "hist_count and hist_counts are whole numbers in [0, 2^32)"},
    // batch-means sums, slot-major [11][C n]: unit n; the switch is the batch length L
    {"per-site convergence diagnostics", "are", {"conv_stats", "conv_count", "conv_sums", nullptr}, 8, 11, true, 1.0, 0x1.0p30,
     "per-site convergence diagnostics have not been switched on for this handle (set conv_stats first)", "conv_stats is 0 or a batch length from 1 to 2^30",
     "conv_count is a whole number >= 0", "the cnt slot of conv_sums holds one whole number >= 0 at every site"},
    // sums over the withheld entries, slot-major [5][C H]: unit H, which holdout_data sets; the switch is 0 or 1
    {"held-out scoring", "is", {"holdout_stats", "holdout_count", "holdout_sums", "holdout_data"}, 8, 5, true, 1.0, 1.0,
     "no held-out data have been set for this handle (set holdout_data first)", "holdout_stats is 0 or 1",
     "holdout_count is a whole number >= 0", "the cnt slot of holdout_sums holds one whole number >= 0 at every entry"}};

// Elements of a kind's data for C chains, and where the part of (slot, chain) starts.  With one slot this is the chain-major
// address of the histograms.
constexpr size_t accum_words(const Accum &a, size_t C, size_t unit) { return (size_t)a.slots * C * unit; }
constexpr size_t accum_offset(size_t C, size_t unit, size_t slot, size_t chain) { return slot * C * unit + chain * unit; }

// The kind and (*field) the field of a state name; -1 for a name that is none of theirs.
inline int accum_lookup(const char *name, int *field)
{
    for (int k = 0; k < N_ACCUM; ++k)
        for (int f = 0; f < 4; ++f)
            if (ACCUM[k].name[f] && !std::strcmp(name, ACCUM[k].name[f])) {
                *field = f;
                return k;
            }
    *field = ACC_NONE;
    return -1;
}

inline bool accum_switch_ok(const Accum &a, double v) { return v == 0.0 || (v >= a.on_min && v <= a.on_max && v == std::floor(v)); }

// What keeps `in` (len elements, already of the right length) from being written as a chain's count or data: the message,
// or null.  Whole numbers the element holds exactly: below 2^32 in 4 bytes, below 2^53 in a float64.  Of float64 data only
// the cnt slot -- the first `unit` elements -- is bound: the columns of a chain have counted the same iterations.
inline const char *accum_write_refusal(const Accum &a, int field, const double *in, size_t len, size_t unit)
{
    const double limit = a.elem == 4 ? 0x1.0p32 : 0x1.0p53;
    const auto whole = [limit](double x) { return x >= 0.0 && x < limit && x == std::floor(x); };
    if (field == ACC_COUNT) return whole(in[0]) ? nullptr : a.bad_count;
    for (size_t i = 0; i < (a.cnt_slot ? unit : len); ++i)
        if (!whole(in[i]) || (a.cnt_slot && in[i] != in[0])) return a.bad_data;
    return nullptr;
}

}  // namespace occ
