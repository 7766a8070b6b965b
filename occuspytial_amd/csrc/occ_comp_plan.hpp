// occ_comp_plan.hpp -- SUM-TO-ZERO PER CONNECTED COMPONENT, the host's part, plain C++17: from the component label of every
// site the tables the correction pass reads (occ_comp.hpp, occ_comp.hip).
//   list         the sites sorted by component, ascending inside one
//   chunk_start  the list cut into CHUNKS of at most COMP_CHUNK sites that never straddle a component: chunk j is
//                list[chunk_start[j] .. chunk_start[j + 1])
//   comp_chunk   component c owns the chunks comp_chunk[c] .. comp_chunk[c + 1]
//   heavy        the components of more than COMP_LIGHT chunks, ascending: their second level is a wave's, not a thread's
//   site_lab     per site its component, bit 31 set where the component is that site alone
// The ORDER of a component's sums (sum of x, sum of z of Xv) follows from the tables alone -- not from a solve's form, a grid
// or timing:  level 1: a chunk's sites from 0.0, left to right;  level 2, at most COMP_LIGHT chunks: the chunks' sums from
// 0.0, left to right;  more: lane l of one wave adds the chunks l, l + 64, ... from 0.0, then one wave_sum.
// comp_tables_ok restates what the kernels rely on; tests build it into a stand-alone program.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace occ {

constexpr int COMP_CHUNK = 32;  // sites per chunk: one thread's serial sum (level 1)
constexpr int COMP_LIGHT = 64;  // chunks a single thread adds at level 2 (2048 sites); beyond: one wave
constexpr uint32_t COMP_SINGLE = 1u << 31;

struct CompTables {
    int n = 0, k = 0;  // k: components (labels in use)
    std::vector<int32_t> list, chunk_start, comp_chunk, heavy;
    std::vector<uint32_t> site_lab;
    int nchunk() const { return (int)chunk_start.size() - 1; }
};

// label[i]: any whole number in [0, n); equal labels = one component.  Components are numbered by ascending label.
// false: a label out of range (nothing is built).
inline bool comp_tables_build(const std::vector<int32_t> &label, CompTables *out, std::string *why)
{
    const int n = (int)label.size();
    CompTables T;
    T.n = n;
    std::vector<int32_t> count((size_t)n + 1, 0);
    for (int i = 0; i < n; ++i) {
        if (label[i] < 0 || label[i] >= n) {
            if (why) *why = "component_id holds whole numbers from 0 to n - 1";
            return false;
        }
        count[(size_t)label[i]] += 1;
    }
    std::vector<int32_t> dense((size_t)n, -1), first;  // label -> component; component -> its first place in the list
    for (int l = 0, at = 0; l < n; ++l)
        if (count[(size_t)l] > 0) {
            dense[(size_t)l] = T.k++;
            first.push_back(at);
            at += count[(size_t)l];
        }
    first.push_back(n);
    T.list.assign((size_t)n, 0);
    T.site_lab.assign((size_t)n, 0u);
    std::vector<int32_t> fill(first.begin(), first.end() - 1);
    for (int i = 0; i < n; ++i) {  // (ascending i: ascending inside a component)
        const int c = dense[(size_t)label[i]];
        T.list[(size_t)fill[(size_t)c]++] = i;
        T.site_lab[(size_t)i] = (uint32_t)c | (count[(size_t)label[i]] == 1 ? COMP_SINGLE : 0u);
    }
    T.comp_chunk.assign(1, 0);
    for (int c = 0; c < T.k; ++c) {
        for (int at = first[(size_t)c]; at < first[(size_t)c + 1]; at += COMP_CHUNK) T.chunk_start.push_back(at);
        T.comp_chunk.push_back((int32_t)T.chunk_start.size());
        if (T.comp_chunk[(size_t)c + 1] - T.comp_chunk[(size_t)c] > COMP_LIGHT) T.heavy.push_back(c);
    }
    T.chunk_start.push_back(n);
    *out = std::move(T);
    return true;
}

// What the kernels rely on: the list is a permutation sorted by component; the chunks tile it exactly, none is empty, longer
// than COMP_CHUNK or straddles a component; comp_chunk tiles the chunks; heavy and the single marks are what the sizes say.
inline bool comp_tables_ok(const std::vector<int32_t> &label, const CompTables &T, std::string *why)
{
    auto fail = [&](const char *m) { if (why) *why = m; return false; };
    const int n = T.n, nc = T.nchunk();
    if ((int)label.size() != n || (int)T.list.size() != n || (int)T.site_lab.size() != n) return fail("sizes");
    if ((int)T.comp_chunk.size() != T.k + 1 || T.comp_chunk.front() != 0 || T.comp_chunk.back() != nc) return fail("comp_chunk ends");
    if (T.chunk_start.front() != 0 || T.chunk_start.back() != n) return fail("chunk_start ends");
    std::vector<uint8_t> seen((size_t)n, 0);
    for (int t = 0; t < n; ++t) {
        const int i = T.list[(size_t)t];
        if (i < 0 || i >= n || seen[(size_t)i]) return fail("list is no permutation");
        seen[(size_t)i] = 1;
    }
    size_t h = 0;
    for (int c = 0; c < T.k; ++c) {
        const int c0 = T.comp_chunk[(size_t)c], c1 = T.comp_chunk[(size_t)c + 1];
        if (c1 <= c0) return fail("an empty component");
        const int size = T.chunk_start[(size_t)c1] - T.chunk_start[(size_t)c0];
        const int32_t lab0 = label[(size_t)T.list[(size_t)T.chunk_start[(size_t)c0]]];
        for (int j = c0; j < c1; ++j) {
            const int b = T.chunk_start[(size_t)j], e = T.chunk_start[(size_t)j + 1];
            if (e <= b || e - b > COMP_CHUNK) return fail("a chunk's length");
            for (int t = b; t < e; ++t) {
                const int i = T.list[(size_t)t];
                if (label[(size_t)i] != lab0) return fail("a chunk straddles a component");
                if (t > b && T.list[(size_t)t - 1] >= i) return fail("a chunk is not ascending");
                if (T.site_lab[(size_t)i] != ((uint32_t)c | (size == 1 ? COMP_SINGLE : 0u))) return fail("site_lab");
            }
        }
        if (c > 0 && label[(size_t)T.list[(size_t)T.chunk_start[(size_t)c0] - 1]] >= lab0) return fail("components out of order");
        if (c1 - c0 > COMP_LIGHT && (h >= T.heavy.size() || T.heavy[h++] != c)) return fail("heavy");
    }
    if (h != T.heavy.size()) return fail("heavy has extra entries");
    return true;
}

}  // namespace occ
