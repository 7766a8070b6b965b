// occ_sim_plan.hpp -- THE FIELD SIMULATOR, the host's part, plain C++17: everything libocc_sim.so (occ_sim.hip, the C ABI of
// include/occ_sim.h) derives before a HIP call is needed.
//   sizes       ld = b_max rounded up to 16 (the leading dimension of the n x ld working blocks), bc = b rounded up to 16 (the
//               columns a launch touches), tiles of SIM_TILE = 256 sites (the unit of every partial sum), slices of 64
//   layout      diagonal d_i, 1 / d_i (0 where d_i = 0: a site without neighbours), the off-diagonals in SELL-64 / uniform ELL
//               exactly as occ_layout.hpp lays them out for the other two libraries
//   sgn_root    per slot (i, j) of that layout  ([i < j] - [i > j]) sqrt(w_ij),  w_ij = -q_ij;  0 in a padding slot
//   components  occ_comp_plan.hpp's chunk tables of the labels, and per component its number of sites
//   refusals    word for word: the C ABI returns them, the tests match them
// tests/test_sim_plan_cpu.py drives this header through the stand-alone program occ_sim_check.cpp under the sanitizers.
#pragma once
#include "occ_comp_plan.hpp"
#include "occ_layout.hpp"

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

namespace occ {

constexpr int SIM_TILE = 256;   // sites per tile: a workgroup's partial sum of p'Qp, r'z, r'r; the tiles are added in tile order
constexpr int SIM_MAX_B = 64;   // columns of one batch

inline int sim_bc(int b) { return (b + 15) / 16 * 16; }
inline int sim_ntile(int n) { return (n + SIM_TILE - 1) / SIM_TILE; }
inline int sim_nslice(int n) { return (n + 63) / 64; }

struct SimPlan {
    int n = 0, b_max = 0, ld = 0, ntile = 0, nslice = 0, ell_w = 0;
    std::vector<int> sell_ptr, sell_col;
    std::vector<double> sell_val, sgn_root, diag, diag_inv;
    CompTables comp;
    std::vector<int32_t> comp_size;  // sites of every component
};

inline bool sim_fail(std::string *why, const char *msg)
{
    if (why) *why = msg;
    return false;
}

inline bool sim_check_sizes(int64_t n, int32_t b_max, std::string *why)
{
    if (!(n >= 1 && n < (int64_t)1 << 30)) return sim_fail(why, "n must lie in [1, 2^30)");
    if (!(b_max >= 1 && b_max <= SIM_MAX_B)) return sim_fail(why, "b_max must lie in [1, 64]");
    return true;
}

// draw numbers are the 32-bit `it` word of the Philox counter: first .. first + b - 1 must all be below 2^32
inline bool sim_check_draw(int64_t first, int32_t b, int32_t b_max, std::string *why)
{
    if (!(b >= 1 && b <= b_max)) return sim_fail(why, "b must lie in [1, b_max]");
    if (first < 0) return sim_fail(why, "first must not be negative");
    if (first + (int64_t)b > (int64_t)1 << 32) return sim_fail(why, "first + b must not exceed 2^32");
    return true;
}

inline bool sim_check_solve(double tol, int64_t max_iter, int32_t check_every, std::string *why)
{
    if (!(tol > 0.0 && tol < 1.0)) return sim_fail(why, "tol must lie in (0, 1)");
    if (!(max_iter >= 1 && max_iter < (int64_t)1 << 31)) return sim_fail(why, "max_iter must lie in [1, 2^31)");
    if (!(check_every >= 1)) return sim_fail(why, "check_every must be at least 1");
    return true;
}

// Q: CSR with sorted unique columns, an ICAR precision (zero row sums, non-positive off-diagonals: layout_q's checks for the
// edge form); label: the component of every site -- two neighbours carry the same label.
inline bool sim_plan_build(int64_t n64, const std::vector<int32_t> &indptr, const std::vector<int32_t> &indices, const std::vector<double> &qdata,
                           const std::vector<int32_t> &label, int32_t b_max, SimPlan *out, std::string *why)
{
    if (!sim_check_sizes(n64, b_max, why)) return false;
    const int n = (int)n64;
    if ((int64_t)indptr.size() != n64 + 1 || (int64_t)label.size() != n64) return sim_fail(why, "indptr has n + 1 entries and labels n");
    if (!layout_q_indptr(n, indptr, why)) return false;
    for (int i = 0; i < n; ++i)
        if (indptr[(size_t)i + 1] < indptr[(size_t)i]) return sim_fail(why, "malformed Q indptr");
    if ((int64_t)indices.size() < indptr[(size_t)n] || (int64_t)qdata.size() < indptr[(size_t)n]) return sim_fail(why, "malformed Q indptr");
    HostLayout L;
    if (!layout_q(n, indptr, indices, qdata, false, L, why)) return false;
    SimPlan P;
    P.n = n;
    P.b_max = b_max;
    P.ld = sim_bc(b_max);
    P.ntile = sim_ntile(n);
    P.nslice = sim_nslice(n);
    P.ell_w = L.ell_w;
    if (!comp_tables_build(label, &P.comp, why)) return false;
    for (int i = 0; i < n; ++i)
        for (int k = indptr[(size_t)i]; k < indptr[(size_t)i + 1]; ++k)
            if (indices[(size_t)k] != i && qdata[(size_t)k] != 0.0 && label[(size_t)indices[(size_t)k]] != label[(size_t)i])
                return sim_fail(why, "labels must give two neighbouring sites the same component");
    P.comp_size.assign((size_t)P.comp.k, 0);
    for (int c = 0; c < P.comp.k; ++c)
        P.comp_size[(size_t)c] = P.comp.chunk_start[(size_t)P.comp.comp_chunk[(size_t)c + 1]] - P.comp.chunk_start[(size_t)P.comp.comp_chunk[(size_t)c]];
    P.diag = L.qdiag;
    P.diag_inv.assign((size_t)n, 0.0);
    for (int i = 0; i < n; ++i)
        if (P.diag[(size_t)i] > 0.0) P.diag_inv[(size_t)i] = 1.0 / P.diag[(size_t)i];
    P.sgn_root.assign(L.sell_val.size(), 0.0);
    for (int sl = 0; sl < P.nslice; ++sl) {
        const int base = L.sell_ptr[(size_t)sl], width = (L.sell_ptr[(size_t)sl + 1] - base) / 64;
        for (int lane = 0; lane < 64; ++lane) {
            const int i = sl * 64 + lane;
            if (i >= n) continue;
            for (int kk = 0; kk < width; ++kk) {
                const size_t slot = (size_t)base + (size_t)kk * 64 + (size_t)lane;
                const int j = L.sell_col[slot];
                const double w = -L.sell_val[slot];
                if (j == i || !(w > 0.0)) continue;  // (padding, or a stored zero)
                P.sgn_root[slot] = i < j ? std::sqrt(w) : -std::sqrt(w);
            }
        }
    }
    P.sell_ptr = std::move(L.sell_ptr);
    P.sell_col = std::move(L.sell_col);
    P.sell_val = std::move(L.sell_val);
    *out = std::move(P);
    return true;
}

// What the kernels rely on: every column in range, the slices inside the slot arrays, every site in exactly one chunk table
// entry (comp_tables_ok), the sizes adding up to n.
inline bool sim_plan_ok(const std::vector<int32_t> &label, const SimPlan &P, std::string *why)
{
    const int n = P.n;
    if (P.ld < P.b_max || P.ld % 16 != 0 || P.ld - P.b_max >= 16) return sim_fail(why, "ld");
    if (P.ntile != sim_ntile(n) || P.nslice != sim_nslice(n)) return sim_fail(why, "tile counts");
    if ((int)P.sell_ptr.size() != P.nslice + 1 || P.sell_ptr[0] != 0) return sim_fail(why, "sell_ptr");
    const size_t slots = P.sell_col.size();
    if (P.sell_val.size() != slots || P.sgn_root.size() != slots) return sim_fail(why, "slot arrays");
    for (int sl = 0; sl < P.nslice; ++sl) {
        const int w = P.sell_ptr[(size_t)sl + 1] - P.sell_ptr[(size_t)sl];
        if (w < 0 || w % 64 != 0 || (size_t)P.sell_ptr[(size_t)sl + 1] > slots) return sim_fail(why, "a slice's extent");
        if (P.ell_w && w != P.ell_w * 64) return sim_fail(why, "a slice's width under ELL");
    }
    for (size_t s = 0; s < slots; ++s)
        if (P.sell_col[s] < 0 || P.sell_col[s] >= n) return sim_fail(why, "a column out of range");
    if ((int)P.diag.size() != n || (int)P.diag_inv.size() != n) return sim_fail(why, "diagonal");
    if (!comp_tables_ok(label, P.comp, why)) return false;
    long long total = 0;
    for (int32_t s : P.comp_size) total += s;
    if ((int)P.comp_size.size() != P.comp.k || total != n) return sim_fail(why, "component sizes");
    return true;
}

}  // namespace occ
