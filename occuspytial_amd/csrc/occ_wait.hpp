// occ_wait.hpp -- the host's deadline poll, stated once: plain C++17, no HIP include (csrc/occ_wait_check.cpp runs it under
// the sanitizers for tests/test_wait_cpu.py).  The engine's poll_stream (occ_gibbs.hip) and the side libraries' wait
// (occ_handle.hpp) are calls of poll_until with hipStreamQuery as the question.
#pragma once

#include <chrono>
#include <cstdlib>
#include <thread>

namespace occ {

// seconds a host wait may last: OCC_HOST_WAIT_S, default 20; non-positive or unparsable gives 20
inline double host_wait_limit_s()
{
    const char *e = std::getenv("OCC_HOST_WAIT_S");
    const double v = e ? std::atof(e) : 20.0;
    return v > 0.0 ? v : 20.0;
}

enum class WaitEnd { done, failed, late };
struct WaitResult {
    WaitEnd end;
    int code;  // done: 0; failed: what `query` answered, unchanged; late: `not_ready`
};

// Asks `query` until it answers 0 (done) or anything but `not_ready` (failed with that code), or until `limit_s` seconds have
// passed (late).  The clock is read every 64th poll; past 2 ms the thread yields between polls (a long wait: the host thread
// need not own a core).
template <class Query>
WaitResult poll_until(Query &&query, int not_ready, double limit_s)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned polls = 1;; ++polls) {
        const int q = query();
        if (q == 0) return {WaitEnd::done, 0};
        if (q != not_ready) return {WaitEnd::failed, q};
        if ((polls & 63u) == 0u) {
            const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (sec > limit_s) return {WaitEnd::late, not_ready};
            if (sec > 0.002) std::this_thread::yield();
        }
    }
}

}  // namespace occ
