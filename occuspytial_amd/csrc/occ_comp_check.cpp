// occ_comp_check.cpp -- the host's tables of the per-component sum-to-zero pass (occ_comp_plan.hpp) as a stand-alone program
// for tests/test_components_cpu.py: `make comp_check` builds it with g++ under AddressSanitizer and UBSan.  Test
// infrastructure; never linked into libocc_gibbs.so.
// stdin: n, then n labels.  stdout: "ok k nchunk nheavy longest_chunk", or the refusal of comp_tables_build; exit status 1 and
// the reason on stderr if comp_tables_ok finds the tables wanting.
#include <cstdio>

#include "occ_comp_plan.hpp"

int main()
{
    int n = 0;
    if (std::scanf("%d", &n) != 1 || n < 0) return 2;
    std::vector<int32_t> label((size_t)n);
    for (int i = 0; i < n; ++i)
        if (std::scanf("%d", &label[(size_t)i]) != 1) return 2;
    occ::CompTables T;
    std::string why;
    if (!occ::comp_tables_build(label, &T, &why)) {
        std::printf("refused: %s\n", why.c_str());
        return 0;
    }
    if (!occ::comp_tables_ok(label, T, &why)) {
        std::fprintf(stderr, "tables wanting: %s\n", why.c_str());
        return 1;
    }
    int longest = 0;
    for (int j = 0; j < T.nchunk(); ++j) longest = std::max(longest, T.chunk_start[(size_t)j + 1] - T.chunk_start[(size_t)j]);
    std::printf("ok %d %d %d %d\n", T.k, T.nchunk(), (int)T.heavy.size(), longest);
    return 0;
}
