// occ_sim_check.cpp -- the host's part of the field simulator (occ_sim_plan.hpp) as a stand-alone program for
// tests/test_sim_plan_cpu.py: `make sim_check` builds it with g++ under AddressSanitizer and UBSan.  Test infrastructure;
// never linked into libocc_sim.so.
// stdin, one request after the other until the end:
//   plan n nnz b_max, then n + 1 indptr, nnz indices, nnz values, n labels
//        -> "refused: <why>", or "ok ld ntile nslice ell_w k nchunk", one line "row i d dinv : j val sgn_root ; ..." per site with
//           every slot of its slice's width, and the lines "list ...", "chunk_start ...", "comp_chunk ...", "comp_size ..."
//   size n b            -> "size ld-for-b bc ntile nslice"
//   create n b_max      -> "ok" or "refused: <why>"          (sim_check_sizes)
//   draw first b b_max  -> the same                          (sim_check_draw)
//   solve tol max_iter check_every -> the same               (sim_check_solve)
// exit status 1 and the reason on stderr if sim_plan_ok finds a plan wanting, 2 for a request it cannot read.
#include <cstdio>
#include <cstring>

#include "occ_sim_plan.hpp"

static void answer(bool ok, const std::string &why)
{
    if (ok) std::printf("ok\n");
    else std::printf("refused: %s\n", why.c_str());
}

template <class T>
static void line(const char *name, const std::vector<T> &v)
{
    std::printf("%s", name);
    for (const T &x : v) std::printf(" %lld", (long long)x);
    std::printf("\n");
}

int main()
{
    char what[32];
    while (std::scanf("%31s", what) == 1) {
        std::string why;
        if (!std::strcmp(what, "size")) {
            int n = 0, b = 0;
            if (std::scanf("%d %d", &n, &b) != 2) return 2;
            std::printf("size %d %d %d %d\n", occ::sim_bc(b), occ::sim_bc(b), occ::sim_ntile(n), occ::sim_nslice(n));
        } else if (!std::strcmp(what, "create")) {
            long long n = 0;
            int b_max = 0;
            if (std::scanf("%lld %d", &n, &b_max) != 2) return 2;
            answer(occ::sim_check_sizes(n, b_max, &why), why);
        } else if (!std::strcmp(what, "draw")) {
            long long first = 0;
            int b = 0, b_max = 0;
            if (std::scanf("%lld %d %d", &first, &b, &b_max) != 3) return 2;
            answer(occ::sim_check_draw(first, b, b_max, &why), why);
        } else if (!std::strcmp(what, "solve")) {
            double tol = 0.0;
            long long max_iter = 0;
            int every = 0;
            if (std::scanf("%lf %lld %d", &tol, &max_iter, &every) != 3) return 2;
            answer(occ::sim_check_solve(tol, max_iter, every, &why), why);
        } else if (!std::strcmp(what, "plan")) {
            int n = 0, nnz = 0, b_max = 0;
            if (std::scanf("%d %d %d", &n, &nnz, &b_max) != 3 || n < 0 || nnz < 0) return 2;
            std::vector<int32_t> ip((size_t)n + 1), ix((size_t)nnz), lab((size_t)n);
            std::vector<double> qd((size_t)nnz);
            for (auto &v : ip)
                if (std::scanf("%d", &v) != 1) return 2;
            for (auto &v : ix)
                if (std::scanf("%d", &v) != 1) return 2;
            for (auto &v : qd)
                if (std::scanf("%lf", &v) != 1) return 2;
            for (auto &v : lab)
                if (std::scanf("%d", &v) != 1) return 2;
            occ::SimPlan P;
            if (n < 1 || ip[(size_t)n] != nnz) {
                std::printf("refused: malformed Q indptr\n");
                continue;
            }
            if (!occ::sim_plan_build(n, ip, ix, qd, lab, b_max, &P, &why)) {
                std::printf("refused: %s\n", why.c_str());
                continue;
            }
            if (!occ::sim_plan_ok(lab, P, &why)) {
                std::fprintf(stderr, "plan wanting: %s\n", why.c_str());
                return 1;
            }
            std::printf("ok %d %d %d %d %d %d\n", P.ld, P.ntile, P.nslice, P.ell_w, P.comp.k, P.comp.nchunk());
            for (int i = 0; i < n; ++i) {
                const int sl = i / 64, lane = i % 64, base = P.sell_ptr[(size_t)sl], width = (P.sell_ptr[(size_t)sl + 1] - base) / 64;
                std::printf("row %d %.17g %.17g :", i, P.diag[(size_t)i], P.diag_inv[(size_t)i]);
                for (int k = 0; k < width; ++k) {
                    const size_t slot = (size_t)base + (size_t)k * 64 + (size_t)lane;
                    std::printf(" %d %.17g %.17g ;", P.sell_col[slot], P.sell_val[slot], P.sgn_root[slot]);
                }
                std::printf("\n");
            }
            line("list", P.comp.list);
            line("chunk_start", P.comp.chunk_start);
            line("comp_chunk", P.comp.comp_chunk);
            line("comp_size", P.comp_size);
        } else {
            return 2;
        }
    }
    return 0;
}
