// occ_layout.hpp -- the PROBLEM LAYOUT, plain C++17: everything the host derives from the caller's problem before a HIP call
// is needed.  Checked inputs in the layouts the kernels read: SELL-64 / diagonal form of Q, structure-of-arrays designs,
// the index sets of base.py:112-152, the prior products; and what a peer of a multi-GPU group sizes from the root's header.
// Every function takes host vectors and returns false with the reason in *why (the engine: OCC_E_BADARG).
// tests/test_layout_cpu.py pins every array on the CPU.
#pragma once
#include "occ_plan.hpp"  // (NPRE)

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

namespace occ {

// A group of samplers -- one per device, or one per process -- is built from ONE layout: the root uploads it, the others
// receive the device arrays by RCCL broadcast (occ_create_group, occ_create_distributed).
struct HostLayout {
    int n = 0, S = 0, R = 0, p = 0, q = 0, ell_w = 0, rsr_dim = 0;
    double tau_rate = 0.0, tau_shape = 0.0;
    std::vector<int> sell_ptr, sell_col, dia_off, row_site, site_sidx;
    std::vector<double> sell_val, qdiag, dia_val, Xt, Wt, hyp, Kh, Qh, Eh;
    std::vector<double> prior_F;  // reference-form prior draw: n x prior_m, row-major (empty: edge form)
    int prior_m = 0;
    std::vector<uint8_t> dia_mask, yrow, obs_site;
    std::vector<int32_t> site_id, site_ptr;
    int wmax() const  // the widest SELL-64 slice (off-diagonals of its longest row)
    {
        int w = 0;
        for (size_t sl = 0; sl + 1 < sell_ptr.size(); ++sl) w = std::max(w, (sell_ptr[sl + 1] - sell_ptr[sl]) / 64);
        return w;
    }
};

inline bool layout_fail(std::string *why, const char *msg)
{
    if (why) *why = msg;
    return false;
}

// (before the columns and values are fetched: indptr[n] is their number)
inline bool layout_q_indptr(int n, const std::vector<int32_t> &indptr, std::string *why)
{
    if (indptr[0] != 0 || indptr[n] < n) return layout_fail(why, "malformed Q indptr");
    return true;
}

// Q: CSR -> diagonal + SELL-64 off-diagonals (coalesced per-wave slices), and the diagonal form when it has one.
// Also checks what the edge form of the prior term needs: zero row sums, non-positive
// off-diagonals (Q = D - W), the singular ICAR precision of gibbs/base.py:166-170.
inline bool layout_q(int n, const std::vector<int32_t> &indptr, const std::vector<int32_t> &indices, const std::vector<double> &qdata,
                     bool has_prior_factor, HostLayout &L, std::string *why)
{
    const int nslice = (n + 63) / 64;
    L.sell_ptr.assign((size_t)nslice + 1, 0);
    L.qdiag.assign((size_t)n, 0.0);
    double scale = 0.0;
    for (int i = 0; i < n; ++i) {
        double rowsum = 0.0, rowabs = 0.0;
        int last = -1;
        for (int k = indptr[i]; k < indptr[i + 1]; ++k) {
            const int j = indices[k];
            if (j < 0 || j >= n || j <= last) return layout_fail(why, "Q columns must be sorted, unique and in range");
            last = j;
            rowsum += qdata[k];
            rowabs += std::fabs(qdata[k]);
            if (j == i) L.qdiag[i] = qdata[k];
            else if (qdata[k] > 0.0 && !has_prior_factor)
                return layout_fail(why, "Q must have non-positive off-diagonal entries (or come with a prior factor: occ_problem::prior_factor)");
        }
        scale = std::max(scale, rowabs);
        // (with a prior factor the caller has established the singularity: F F' = Q of rank < n)
        if (!has_prior_factor && std::fabs(rowsum) > 1e-10 * std::max(rowabs, 1e-300))
            return layout_fail(why, "Spatial precision matrix Q must be singular.");
    }
    if (!(scale > 0.0)) return layout_fail(why, "Spatial precision matrix Q must be singular.");
    for (int sl = 0; sl < nslice; ++sl) {
        int width = 0;
        for (int i = sl * 64; i < std::min(n, sl * 64 + 64); ++i) {
            int cnt = 0;
            for (int k = indptr[i]; k < indptr[i + 1]; ++k) cnt += (indices[k] != i);
            width = std::max(width, cnt);
        }
        L.sell_ptr[sl + 1] = L.sell_ptr[sl] + width * 64;
    }
    // uniform width (ELL) when the padding it adds is small: the slice base becomes arithmetic
    {
        const int wmax = L.wmax();
        const long long ell_slots = (long long)wmax * 64 * nslice;
        L.ell_w = (wmax > 0 && ell_slots <= (long long)(1.25 * L.sell_ptr[nslice]) + 64) ? wmax : 0;
        if (L.ell_w)
            for (int sl = 0; sl <= nslice; ++sl) L.sell_ptr[sl] = sl * wmax * 64;
    }
    // 64 spare slots: k_iter reads slot `base + lane` of a slice even when the slice has no off-diagonals
    L.sell_col.assign((size_t)L.sell_ptr[nslice] + 64, 0);
    L.sell_val.assign((size_t)L.sell_ptr[nslice] + 64, 0.0);
    for (int sl = 0; sl < nslice; ++sl) {
        const int base = L.sell_ptr[sl], width = (L.sell_ptr[sl + 1] - base) / 64;
        for (int lane = 0; lane < 64; ++lane) {
            const int i = sl * 64 + lane;
            int kk = 0;
            if (i < n)
                for (int k = indptr[i]; k < indptr[i + 1]; ++k)
                    if (indices[k] != i) {
                        L.sell_col[(size_t)base + kk * 64 + lane] = indices[k];
                        L.sell_val[(size_t)base + kk * 64 + lane] = qdata[k];
                        ++kk;
                    }
            for (; kk < width; ++kk) L.sell_col[(size_t)base + kk * 64 + lane] = std::min(i, n - 1);  // padding: value 0
        }
    }

    // ---- diagonal form, when the off-diagonals lie on at most NPRE diagonals with one value each (lattices) -----
    {
        std::vector<long long> offs;
        bool ok = true;
        for (int i = 0; i < n && ok; ++i)
            for (int k = indptr[i]; k < indptr[i + 1] && ok; ++k) {
                if (indices[k] == i) continue;
                const long long d = (long long)indices[k] - i;
                size_t t = 0;
                while (t < offs.size() && offs[t] != d) ++t;
                if (t == offs.size()) {
                    if (offs.size() == (size_t)NPRE) { ok = false; break; }
                    offs.push_back(d);
                    L.dia_val.push_back(qdata[k]);
                } else if (L.dia_val[t] != qdata[k]) ok = false;
            }
        if (ok && !offs.empty()) {
            std::vector<size_t> order(offs.size());
            for (size_t t = 0; t < order.size(); ++t) order[t] = t;
            std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return offs[a] < offs[b]; });  // CSR column order
            std::vector<double> v2;
            for (size_t t : order) { L.dia_off.push_back((int)offs[t]); v2.push_back(L.dia_val[t]); }
            L.dia_val = v2;
            L.dia_mask.assign((size_t)n, 0);
            for (int i = 0; i < n; ++i)
                for (int k = indptr[i]; k < indptr[i + 1]; ++k) {
                    if (indices[k] == i) continue;
                    const int d = indices[k] - i;
                    for (size_t t = 0; t < L.dia_off.size(); ++t)
                        if (L.dia_off[t] == d) L.dia_mask[i] |= (uint8_t)(1u << t);
                }
        } else {
            L.dia_val.clear();
        }
    }
    return true;
}

// (the logit model takes no surveyed site at all; the probit model has refused that before it comes here)
inline bool layout_site_span(int S, int R, const std::vector<int32_t> &site_ptr, std::string *why)
{
    if (S > 0 && (site_ptr[0] != 0 || site_ptr[S] != R)) return layout_fail(why, "site_ptr does not span the rows");
    return true;
}

// Ragged visits; the index sets of base.py:112-152: the surveyed index of every site (-1: none) and of every row, the
// rows and the surveyed sites with a detection
inline bool layout_sites(int n, int S, int R, const std::vector<int32_t> &site_id, const std::vector<int32_t> &site_ptr, const std::vector<double> &y,
                         std::vector<int> &site_sidx, std::vector<int> &row_t, std::vector<uint8_t> &yrow, std::vector<uint8_t> &obs_site,
                         std::string *why)
{
    yrow.assign((size_t)R, 0);
    row_t.assign((size_t)R, 0);
    site_sidx.assign((size_t)n, -1);
    obs_site.assign((size_t)S, 0);
    for (int t = 0; t < S; ++t) {
        const int site = site_id[t];
        if (site < 0 || site >= n || site_sidx[site] != -1) return layout_fail(why, "site_id entries must be unique and in [0, n)");
        if (site_ptr[t + 1] < site_ptr[t]) return layout_fail(why, "site_ptr must be non-decreasing");
        site_sidx[site] = t;
        for (int r = site_ptr[t]; r < site_ptr[t + 1]; ++r) {
            row_t[r] = t;
            yrow[r] = (y[r] != 0.0) ? 1 : 0;
            obs_site[t] |= yrow[r];
        }
    }
    return true;
}

// the logit kernels' row -> site, bit 31: that site has a detection
inline void layout_row_site(HostLayout &L)
{
    L.row_site.assign((size_t)L.R, 0);
    for (int t = 0; t < L.S; ++t)
        for (int r = L.site_ptr[t]; r < L.site_ptr[t + 1]; ++r) L.row_site[r] = L.site_id[t] | (L.obs_site[t] ? (int)0x80000000 : 0);
}

// a design matrix (rows x cols, row-major) as structure-of-arrays
inline void layout_transpose(int rows, int cols, const std::vector<double> &M, std::vector<double> &Mt)
{
    Mt.assign((size_t)rows * cols, 0.0);
    for (int i = 0; i < rows; ++i)
        for (int a = 0; a < cols; ++a) Mt[(size_t)a * rows + i] = M[(size_t)i * cols + a];
}

// out += prec . mu (d x d row-major; base.py:161-162)
inline void layout_prec_mu(int d, const std::vector<double> &prec, const std::vector<double> &mu, double *out)
{
    for (int a = 0; a < d; ++a)
        for (int b = 0; b < d; ++b) out[a] += prec[(size_t)a * d + b] * mu[b];
}

// the logit kernels' prior block: a_prec, a_prec . a_mu, b_prec, b_prec . b_mu
inline void layout_hyp(int p, int q, const std::vector<double> &a_mu, const std::vector<double> &a_prec, const std::vector<double> &b_mu,
                       const std::vector<double> &b_prec, std::vector<double> &hyp)
{
    hyp.assign((size_t)q * q + q + (size_t)p * p + p, 0.0);
    double *ap = hyp.data(), *apm = ap + q * q, *bp = apm + q, *bpm = bp + p * p;
    std::copy(a_prec.begin(), a_prec.end(), ap);
    std::copy(b_prec.begin(), b_prec.end(), bp);
    layout_prec_mu(q, a_prec, a_mu, apm);
    layout_prec_mu(p, b_prec, b_mu, bpm);
}

// What a peer needs to size its arrays before the broadcast (sell_ptr follows it)
struct LayoutHeader {
    int32_t ok, n, S, R, p, q, ell_w, ndia, nsell_ptr, pad_;
    double tau_rate, tau_shape;
    int32_t dia_off[NPRE];
    double dia_val[NPRE];
};

inline LayoutHeader layout_header(const HostLayout &L)
{
    LayoutHeader h{};
    h.ok = 1;
    h.n = L.n; h.S = L.S; h.R = L.R; h.p = L.p; h.q = L.q; h.ell_w = L.ell_w;
    h.ndia = (int32_t)L.dia_off.size(); h.nsell_ptr = (int32_t)L.sell_ptr.size();
    h.tau_rate = L.tau_rate; h.tau_shape = L.tau_shape;
    for (int d = 0; d < h.ndia; ++d) { h.dia_off[d] = L.dia_off[d]; h.dia_val[d] = L.dia_val[d]; }
    return h;
}

// (L.sell_ptr has arrived)
inline void size_peer_layout(HostLayout &L, const LayoutHeader &h)
{
    L.n = h.n; L.S = h.S; L.R = h.R; L.p = h.p; L.q = h.q; L.ell_w = h.ell_w; L.rsr_dim = 0;
    L.tau_rate = h.tau_rate; L.tau_shape = h.tau_shape;
    L.dia_off.assign(h.dia_off, h.dia_off + h.ndia);
    L.dia_val.assign(h.dia_val, h.dia_val + h.ndia);
    const size_t slots = (size_t)L.sell_ptr.back() + 64;
    L.sell_col.assign(slots, 0);
    L.sell_val.assign(slots, 0.0);
    L.qdiag.assign((size_t)h.n, 0.0);
    if (h.ndia > 0) L.dia_mask.assign((size_t)h.n, 0);
    L.Xt.assign((size_t)h.n * h.p, 0.0);
    L.Wt.assign((size_t)h.R * h.q, 0.0);
    L.yrow.assign((size_t)h.R, 0);
    L.row_site.assign((size_t)h.R, 0);
    L.site_sidx.assign((size_t)h.n, -1);
    L.hyp.assign((size_t)h.q * h.q + h.q + (size_t)h.p * h.p + h.p, 0.0);
    L.site_id.assign((size_t)h.S, 0);
    for (int t = 0; t < h.S; ++t) L.site_id[t] = t;  // placeholders (unique, in range) until the real arrays arrive
    L.site_ptr.assign((size_t)h.S + 1, 0);
    L.obs_site.assign((size_t)h.S, 0);
}

}  // namespace occ
