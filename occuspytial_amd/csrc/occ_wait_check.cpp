// occ_wait_check.cpp -- the host's deadline poll (occ_wait.hpp) as a stand-alone program for tests/test_wait_cpu.py:
// `make wait_check` builds it with g++ under AddressSanitizer and UBSan.  Test infrastructure; never linked into a library.
// stdin, one request per line: `limit` -> "limit <host_wait_limit_s()>" (OCC_HOST_WAIT_S comes from the environment);
// `poll LIMIT_S NOT_READY FAIL_AT CODE` -> "done|failed|late <code> <polls> <elapsed seconds>" of a scripted query: poll number
// FAIL_AT (from 1; 0: none) answers CODE, the polls up to NOT_READY (-1: all of them) answer 600, the next one 0
#include <chrono>
#include <cstdio>
#include <cstring>

#include "occ_wait.hpp"

int main()
{
    char word[16];
    while (std::scanf("%15s", word) == 1) {
        if (std::strcmp(word, "limit") == 0) {
            std::printf("limit %.17g\n", occ::host_wait_limit_s());
            continue;
        }
        double limit = 0.0;
        long not_ready = 0, fail_at = 0, polls = 0;
        int code = 0;
        if (std::strcmp(word, "poll") != 0 || std::scanf("%lf %ld %ld %d", &limit, &not_ready, &fail_at, &code) != 4) return 2;
        const auto t0 = std::chrono::steady_clock::now();
        const occ::WaitResult r = occ::poll_until(
            [&] {
                ++polls;
                if (polls == fail_at) return code;
                return not_ready < 0 || polls <= not_ready ? 600 : 0;
            },
            600, limit);
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        const char *end = r.end == occ::WaitEnd::done ? "done" : r.end == occ::WaitEnd::failed ? "failed" : "late";
        std::printf("%s %d %ld %.6f\n", end, r.code, polls, sec);
    }
    return 0;
}
