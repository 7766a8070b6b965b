// occ_call.hpp -- what a call of occ_run / occ_step DECIDES on the host, plain C++17: the steps in front of the first batch
// (call_head), the size of a batch (call_batch), the captured Krylov cap (cap_from_calibration, cap_resize), the progress of a
// batch (call_progress) and the back-off of the questions the engine asks the device again (Backoff).  run_impl, try_repromote
// and refresh_paths (occ_gibbs.hip) walk them; tests/test_call_cpu.py pins them on the CPU.
#pragma once
#include "occ_plan.hpp"

#include <cstdlib>
#include <utility>

namespace occ {

// ---- the HEAD of a call: what runs in front of the first batch, in order.  n: the eager sequences a step runs, each of which
// moves every chain by one iteration and counts towards the call's.
enum HeadKind : int {
    HEAD_EAGER = 0,  // n eager sequences: the whole call (OCC_EAGER_ONLY: counter collection cannot follow graph launches); ONE
                     // that realigns (the captured pair of iterations starts with one sequence parity: an odd number of stepped
                     // iterations since the capture); the one step of a one-iteration call
    HEAD_PROLOGUE,   // omega_b and the noise of the coming iteration, stand-alone
    HEAD_CALIBRATE,  // no graph yet: n eager sequences measure the Krylov launches a solve needs (calib_max, reset before the
                     // last: the count of the last, warm-started solve sizes the captured graph)
    HEAD_BUILD       // capture -- from_calib: with cap_from_calibration, else cap 0 (the solve is one launch: nothing to
                     // calibrate); long_pair: the long pair with the short one (no later call captures anything)
};
struct HeadStep { int kind; int64_t n; bool from_calib, long_pair; };
struct CallHead { int n; HeadStep step[3]; };
// have_graph: a captured graph exists; aligned: the engine's sequence parity is the one the captured pair starts with
inline CallHead call_head(bool eager_only, SeqSolve solve, int64_t seq_per_enqueue, bool have_graph, bool aligned, int64_t n_iter, bool need_prologue)
{
    CallHead h{0, {}};
    auto add = [&](bool when, int kind, int64_t n = 0, bool from_calib = false, bool long_pair = false) {
        if (when) h.step[h.n++] = HeadStep{kind, n, from_calib, long_pair};
    };
    const bool realign = have_graph && !aligned;
    const int64_t n_calib = n_iter < 3 ? n_iter : 3;
    if (eager_only) {
        add(true, HEAD_EAGER, n_iter);
    } else if (solve == SOLVE_FUSED && seq_per_enqueue == 1) {
        add(!have_graph, HEAD_BUILD);
        add(need_prologue, HEAD_PROLOGUE);
    } else if (seq_per_enqueue > 1) {
        add(need_prologue, HEAD_PROLOGUE);
        add(realign, HEAD_EAGER, 1);
        add(!have_graph && n_iter > 1, HEAD_BUILD, 0, false, true);
        add(n_iter == 1 && !realign, HEAD_EAGER, 1);
    } else if (!have_graph) {  // (the first eager sequence launches a pending prologue itself)
        add(true, HEAD_CALIBRATE, n_calib);
        add(n_calib < n_iter, HEAD_BUILD, 0, true);
    } else {
        add(need_prologue, HEAD_PROLOGUE);
    }
    return h;
}

// ---- a BATCH: the sequences enqueued between two reads of the chains' scalars; whole enqueues (a surplus sequence idles: it_stop)
constexpr int64_t call_batch(int64_t left, int64_t graph_launches, int64_t seq_per_enqueue)
{
    const int64_t most = graph_launches < 128 ? 32 : 256, batch = left < most ? left : most;
    return (batch + seq_per_enqueue - 1) / seq_per_enqueue * seq_per_enqueue;
}

// ---- the captured Krylov CAP.  From the calibration; force: OCC_FORCE_KRYLOV_CAP (tests), or null.
inline int cap_from_calibration(int calib_max, const char *force) { return force ? std::max(1, std::atoi(force)) : std::max(4, calib_max + 2); }
// Re-sized from the solves since the last decision (the counters' differences): mean + 2.5 sd, at least 4.  0: too few solves to
// decide, the counters run on; else the cap to go on with -- `cap` itself inside the hysteresis: grow at once, shrink only when
// two launches too many are captured.
inline int cap_resize(int cap, unsigned long long d_tot, unsigned long long d_sq, unsigned long long d_solves)
{
    if (d_solves < 32) return 0;
    const double mean = (double)d_tot / d_solves;
    const double var = std::max(0.0, (double)d_sq / d_solves - mean * mean);
    const int want = std::max(4, (int)std::ceil(mean + 2.5 * std::sqrt(var)));
    return want > cap || want < cap - 1 ? want : cap;
}

// ---- the PROGRESS of a batch.  ChainAt: (iteration, launches spent on a carried solve) of a chain as the batch left it, and the
// iteration its window started at; SeenAt: the first two after the previous batch ({0xffffffff, 0xffffffff}: there was none).
// -> done_min: the iterations every chain has done; stuck: the first unfinished chain the batch left exactly where it was, or
// -1.  seen is brought up to date for the chains in front of `stuck`.  at(ch) -> ChainAt.
struct ChainAt { uint32_t it, koff, it_base; };
using SeenAt = std::pair<uint32_t, uint32_t>;
struct CallProgress { int64_t done_min; int stuck; };
template <class At>
CallProgress call_progress(int C, At &&at, SeenAt *seen, int64_t n_iter)
{
    CallProgress r{n_iter, -1};
    for (int ch = 0; ch < C; ++ch) {
        const ChainAt a = at(ch);
        const int64_t done = (int64_t)a.it - (int64_t)a.it_base;
        r.done_min = std::min(r.done_min, done);
        if (r.stuck >= 0) continue;
        if (done < n_iter && seen[ch] == SeenAt{a.it, a.koff}) r.stuck = ch;
        else seen[ch] = {a.it, a.koff};
    }
    return r;
}

// ---- BACK-OFF of a question the device answered with "no".  wait: calls until it is asked again; step: what the next arming
// waits.  arm() with the step as it is (the "no" came from elsewhere: creation's probe, a fallback); fail() after an attempt of
// one's own: twice the step, at most 64, then armed; pass(): the next "no" starts from 1 again; due() counts one call.
struct Backoff {
    int wait = 0, step = 1;
    void arm() { wait = step; }
    void fail() { step = std::min(64, step * 2), arm(); }
    void pass() { step = 1; }
    bool due() { return --wait <= 0; }
};

}  // namespace occ
