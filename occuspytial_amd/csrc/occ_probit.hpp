// occ_probit.hpp -- kernels of the probit reduced-rank model (ProbitRSRGibbs; reference occuspytial/gibbs/probit.py).
//
// One iteration of every chain, in the reference's order (omega_b, tau, eps, theta, beta, omega_a, alpha, z), as eight
// launches on one stream:
//   k_pb_site   per (chain, site): omega_b (truncated normal), eps, s = omega_b - X beta - eps
//   k_pb_proj   per (64-site tile, 256 columns): partial sums of u = Phi' s for every chain, Phi's rows read once
//   k_pb_coef   per chain: tau from the old coefficients, then c = D u + D^1/2 xi, D = diag(1 / (1 + tau lam))
//   k_pb_eta    per 16-site tile: eta = Phi c (one wave per site row) and the tile's partial sums of X'(omega_b - eta - eps)
//   k_pb_omega_a per (chain, visit row): omega_a (truncated normal) on the rows of the sites that exist
//   k_pb_alpha  per chain: beta from the FIXED factor of X'X + b_prec, then alpha's sums and alpha's draw
//   k_pb_z      per (chain, site): z with Phi(.) in place of the logistic function
//   k_pb_tail   per chain: the record of the iteration (occ_run) and the iteration counter
// The eta precision is A = K'K + tau K'QK.  With the generalized eigenvectors G of (K'QK, K'K) (G'K'K G = I, K'QK G =
// K'K G diag(lam)) and Phi = K G, A^-1 = G D G', so theta = G c needs no factorisation per iteration (DESIGN.md
// "ProbitRSRGibbs").  Every reduction runs in a fixed order that does not depend on the number of chains: a chain's values
// are the same bits batched or alone, run after run.
#pragma once
#include "occ_kernels.hpp"

namespace occ {

// Philox streams of the probit conditionals (occ_rng.hpp, the header's list): omega_b STREAM_OMEGA_B (index site), eps
// STREAM_PB_EPS (site), xi STREAM_PB_XI (column), tau STREAM_TAU (cursor at index 0), beta STREAM_BETA (component), omega_a
// STREAM_OMEGA_A (visit row), alpha STREAM_ALPHA (component), z STREAM_Z (site).  Uniforms and normals take block 0 of
// their sub-stream.

constexpr int PB_WG = 256;
constexpr int PB_TS = 64;          // sites per tile of k_pb_proj
constexpr int PB_TS_ETA = 16;      // ... and of k_pb_eta (four per wave)
constexpr int PB_MAX_DIM = 4096;   // basis columns
constexpr double kInvSqrt2Pi = 0.39894228040143267794;
constexpr double kSqrt2OverPi = 0.79788456080286535588;

struct PbChain {
    uint64_t key;
    uint32_t it;         // iterations completed
    uint32_t rec_first;  // occ_run: iteration number of the first recorded row ...
    uint32_t rec_keep;   // ... and the rows recorded
    int32_t err;         // -4: alpha's precision was not positive definite
    double tau;
    double alpha[MAXC], beta[MAXC];
};

struct PbArgs {
    int n, m, ldm, p, q, R, S, C, ntile, ntile_eta;
    double tau_rate, tau_shape;
    const double *Phi;     // n x ldm, row-major: K G
    const double *lam;     // m
    const double *Xt;      // p x n
    const double *Wt;      // q x R
    const double *bU;      // p x p: upper Cholesky factor of X'X + b_prec (creation; never overwritten)
    const double *b_pbm;   // b_prec b_mu
    const double *a_prec, *a_pbm;
    const uint8_t *yrow;   // R
    const uint8_t *obs_site;  // S
    const int *site_id, *site_ptr, *sidx /* n: surveyed index or -1 */, *row_t /* R: surveyed index of the row */;
    PbChain *ch;           // C
    double **rec;          // -> [C][rec_keep][q + p + 1] of the running occ_run, or null
    double *omega_b, *eps, *eta, *s;  // C x n
    uint8_t *z;            // C x n
    double *omega_a;       // C x R
    double *c;             // C x m
    double *upart;         // ntile x C x m
    double *bpart;         // ntile_eta x C x p
};

// ---- the truncated normal ----------------------------------------------------------------------------------------
// Phi^-1(p), p in (0, 1): AS 241 (Wichura 1988, PPND16), then one Newton step on the tail that holds p.
__device__ inline double pb_ndtri(double p)
{
    const double q = p - 0.5;
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        const double num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r +
                                 4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
                              1.3314166789178437745e+2) * r + 3.3871328727963666080e0);
        const double den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r +
                                 2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
                              4.2313330701600911252e+1) * r + 1.0);
        return q * num / den;
    }
    const double pt = q < 0.0 ? p : 1.0 - p;
    double r = sqrt(-log(pt)), x;
    if (r <= 5.0) {
        r -= 1.6;
        x = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
                 1.27045825245236838258e0) * r + 3.64784832476320460504e0) * r + 5.76949722146069140550e0) * r +
              4.63033784615654529590e0) * r + 1.42343711074968357734e0) /
            (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
                 1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e0) * r +
              2.05319162663775882187e0) * r + 1.0);
    } else {
        r -= 5.0;
        x = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r +
                 2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580e0) * r +
              5.46378491116411436990e0) * r + 6.65790464350110377720e0) /
            (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r +
                 7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
              5.99832206555887937690e-1) * r + 1.0);
    }
    if (q < 0.0) x = -x;
    const bool lo = q < 0.0;
    const double cdf = 0.5 * erfc((lo ? -x : x) * kSqrtHalf);
    const double pdf = exp(-0.5 * x * x) * kInvSqrt2Pi;
    const double step = (lo ? cdf - pt : pt - cdf) / pdf;
    return isfinite(step) ? x - step : x;
}

// the normal hazard phi(y) / Q(y)
__device__ __forceinline__ double pb_hazard(double y) { return kSqrt2OverPi / erfcx(y * kSqrtHalf); }

// Gauss-Legendre, 16 points on [0, 1] (nodes 1/2 -+ x_k / 2, weights w_k / 2 of the rule on [-1, 1]); tests/
// test_probit_reference_cpu.py checks the table against numpy's leggauss(16)
__constant__ double kPbGlT[16] = {
    0.5 - 0.5 * 0.9894009349916499325961542, 0.5 - 0.5 * 0.9445750230732325760779884, 0.5 - 0.5 * 0.8656312023878317438804679,
    0.5 - 0.5 * 0.7554044083550030338951012, 0.5 - 0.5 * 0.6178762444026437484466718, 0.5 - 0.5 * 0.4580167776572273863424194,
    0.5 - 0.5 * 0.2816035507792589132304605, 0.5 - 0.5 * 0.0950125098376374401853193, 0.5 + 0.5 * 0.0950125098376374401853193,
    0.5 + 0.5 * 0.2816035507792589132304605, 0.5 + 0.5 * 0.4580167776572273863424194, 0.5 + 0.5 * 0.6178762444026437484466718,
    0.5 + 0.5 * 0.7554044083550030338951012, 0.5 + 0.5 * 0.8656312023878317438804679, 0.5 + 0.5 * 0.9445750230732325760779884,
    0.5 + 0.5 * 0.9894009349916499325961542};
__constant__ double kPbGlW[16] = {
    0.5 * 0.0271524594117540948517806, 0.5 * 0.0622535239386478928628438, 0.5 * 0.0951585116824927848099251,
    0.5 * 0.1246289712555338720524763, 0.5 * 0.1495959888165767320815017, 0.5 * 0.1691565193950025381893121,
    0.5 * 0.1826034150449235888667637, 0.5 * 0.1894506104550684962853967, 0.5 * 0.1894506104550684962853967,
    0.5 * 0.1826034150449235888667637, 0.5 * 0.1691565193950025381893121, 0.5 * 0.1495959888165767320815017,
    0.5 * 0.1246289712555338720524763, 0.5 * 0.0951585116824927848099251, 0.5 * 0.0622535239386478928628438,
    0.5 * 0.0271524594117540948517806};

// Newton's method on h(x) = int_a^{a+x} H = E (h by the Gauss-Legendre rule on [a, a + x]; h' = H(a + x)).  (The rule's loop
// is not unrolled: sixteen erfcx in flight at once spilled to scratch.)
__device__ inline double pb_newton(double a, double E, double x)
{
    for (int k = 0; k < 40; ++k) {
        double s = 0.0;
#pragma unroll 1
        for (int g = 0; g < 16; ++g) s = fma(kPbGlW[g], pb_hazard(fma(x, kPbGlT[g], a)), s);
        const double dx = (x * s - E) / pb_hazard(a + x);
        x -= dx;
        if (!(fabs(dx) > 1e-14 * fabs(x))) break;  // (convergence is quadratic: the next step would be below rounding)
    }
    return x;
}

// x >= 0 with Q(a + x) = Q(a) v, given v, w = 1 - v and E = -log v (tests/_probit_reference.py states the method)
__device__ inline double pb_excess(double a, double v, double w, double E)
{
    if (a > 0.0) return pb_newton(a, E, 2.0 * E / (a + sqrt(fma(a, a, 2.0 * E))));
    const double Qa = 0.5 * erfc(a * kSqrtHalf), Pa = 0.5 * erfc(-a * kSqrtHalf);
    const double q = Qa * v;
    const double N = q <= 0.5 ? -pb_ndtri(q) : pb_ndtri(fmin(fma(Qa, w, Pa), 0.5));
    double x = N - a;
    if (x < fmax(-a, 1.0) * (1.0 / 32.0)) x = pb_newton(a, E, fmax(x, 0.0));
    return x;
}

// N(loc, 1) truncated to (0, inf) / (-inf, 0) at the uniform U (the reference's inverse CDF, evaluated stably)
__device__ inline double tn_pos(double loc, double U) { return pb_excess(-loc, 1.0 - U, U, -log1p(-U)); }
__device__ inline double tn_neg(double loc, double U) { return -pb_excess(loc, U, 1.0 - U, -log(U)); }

// x = M^-1 r + U^-1 eps with M = U'U and U fixed (row-major upper, d x d): precision_mvnorm_dev without the factorisation
__device__ inline void pb_fixed_draw(int d, const double *U, const double *r, uint64_t key, uint32_t it, uint32_t stream, double *o,
                                     double *out)
{
    for (int i = 0; i < d; ++i) o[i] = 0.0;
    for (int k = 0; k < d; ++k) {
        const double e = block_normal(key, (uint32_t)k, 0, it, stream);
        for (int i = k; i < d; ++i) o[i] += U[k * d + i] * e;
    }
    for (int i = 0; i < d; ++i) o[i] += r[i];
    for (int i = 0; i < d; ++i) {
        double v = o[i];
        for (int k = 0; k < i; ++k) v -= U[k * d + i] * o[k];
        o[i] = v / U[i * d + i];
    }
    for (int i = d - 1; i >= 0; --i) {
        double v = o[i];
        for (int k = i + 1; k < d; ++k) v -= U[i * d + k] * o[k];
        o[i] = v / U[i * d + i];
    }
    for (int i = 0; i < d; ++i) out[i] = o[i];
}

// ---- kernels ------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PB_WG) k_pb_site(const PbArgs A)
{
    const long long g = (long long)blockIdx.x * PB_WG + threadIdx.x;
    if (g >= (long long)A.C * A.n) return;
    const int chain = (int)(g / A.n), i = (int)(g - (long long)chain * A.n);
    const PbChain &ch = A.ch[chain];
    const uint64_t key = ch.key;
    const uint32_t it = ch.it;
    const size_t ci = (size_t)chain * A.n + i;
    const double xb = xdot(A.Xt, A.n, i, ch.beta, A.p);
    const double eta = A.eta[ci];
    const double loc = (xb + eta) + A.eps[ci];
    const double U = block_uniform(key, (uint32_t)i, 0, it, STREAM_OMEGA_B);
    const double ob = A.z[ci] ? tn_pos(loc, U) : tn_neg(loc, U);
    const double e1 = fma(kSqrtHalf, block_normal(key, (uint32_t)i, 0, it, STREAM_PB_EPS), 0.5 * ((ob - xb) - eta));
    A.omega_b[ci] = ob;
    A.eps[ci] = e1;
    A.s[ci] = (ob - xb) - e1;
}

__global__ void __launch_bounds__(PB_WG) k_pb_proj(const PbArgs A)
{
    __shared__ double s_s[4][PB_TS];
    const int t = blockIdx.x, j = blockIdx.y * PB_WG + threadIdx.x;
    const int i0 = t * PB_TS, cnt = min(PB_TS, A.n - i0);
    for (int c0 = 0; c0 < A.C; c0 += 4) {
        const int nc = min(4, A.C - c0);
        __syncthreads();
        {
            const int k = threadIdx.x / PB_TS, ii = threadIdx.x % PB_TS;
            s_s[k][ii] = (k < nc && ii < cnt) ? A.s[(size_t)(c0 + k) * A.n + i0 + ii] : 0.0;
        }
        __syncthreads();
        if (j < A.m) {
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            for (int ii = 0; ii < cnt; ++ii) {
                const double ph = A.Phi[(size_t)(i0 + ii) * A.ldm + j];
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] = fma(ph, s_s[k][ii], acc[k]);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < nc) A.upart[((size_t)t * A.C + c0 + k) * A.m + j] = acc[k];
        }
    }
}

__global__ void __launch_bounds__(PB_WG) k_pb_coef(const PbArgs A)
{
    __shared__ double s_red[PB_WG];
    __shared__ double s_tau;
    const int chain = blockIdx.x, tid = threadIdx.x;
    PbChain &ch = A.ch[chain];
    const uint64_t key = ch.key;
    const uint32_t it = ch.it;
    double *cc = A.c + (size_t)chain * A.m;
    double part = 0.0;  // theta' Qr theta = sum lam c^2 of the current coefficients
    for (int j = tid; j < A.m; j += PB_WG) {
        const double v = cc[j];
        part = fma(A.lam[j] * v, v, part);
    }
    s_red[tid] = part;
    for (int w = PB_WG / 2; w > 0; w >>= 1) {
        __syncthreads();
        if (tid < w) s_red[tid] += s_red[tid + w];
    }
    __syncthreads();
    if (tid == 0) {
        const double rate = fma(0.5, s_red[0], A.tau_rate);
        Cursor g(key, 0u, it, STREAM_TAU);
        const double tau = std_gamma(g, A.tau_shape) / rate;
        s_tau = tau;
        ch.tau = tau;
    }
    __syncthreads();
    const double tau = s_tau;
    for (int j = tid; j < A.m; j += PB_WG) {
        double u = 0.0;
        for (int t = 0; t < A.ntile; ++t) u += A.upart[((size_t)t * A.C + chain) * A.m + j];
        const double D = 1.0 / fma(tau, A.lam[j], 1.0);
        cc[j] = fma(sqrt(D), block_normal(key, (uint32_t)j, 0, it, STREAM_PB_XI), D * u);
    }
}

__global__ void __launch_bounds__(PB_WG) k_pb_eta(const PbArgs A)
{
    __shared__ double s_b[4][4][MAXC];
    const int t = blockIdx.x, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i0 = t * PB_TS_ETA + wv * (PB_TS_ETA / 4), i1 = min(i0 + PB_TS_ETA / 4, A.n);
    for (int c0 = 0; c0 < A.C; c0 += 4) {
        const int nc = min(4, A.C - c0);
        double bacc[4][MAXC];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int a = 0; a < MAXC; ++a) bacc[k][a] = 0.0;
        for (int i = i0; i < i1; ++i) {
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            const double *row = A.Phi + (size_t)i * A.ldm;
            for (int j = lane; j < A.m; j += 64) {
                const double ph = row[j];
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < nc) acc[k] = fma(ph, A.c[(size_t)(c0 + k) * A.m + j], acc[k]);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double e = wave_sum(acc[k]);
                if (k < nc) {
                    const size_t ci = (size_t)(c0 + k) * A.n + i;
                    if (lane == 0) A.eta[ci] = e;
                    const double r = (A.omega_b[ci] - e) - A.eps[ci];
#pragma unroll
                    for (int a = 0; a < MAXC; ++a)
                        if (a < A.p) bacc[k][a] = fma(A.Xt[(size_t)a * A.n + i], r, bacc[k][a]);
                }
            }
        }
        __syncthreads();
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int a = 0; a < MAXC; ++a) s_b[wv][k][a] = bacc[k][a];
        }
        __syncthreads();
        if (threadIdx.x < 4 * MAXC) {
            const int k = threadIdx.x / MAXC, a = threadIdx.x % MAXC;
            if (k < nc && a < A.p)
                A.bpart[((size_t)t * A.C + c0 + k) * A.p + a] = ((s_b[0][k][a] + s_b[1][k][a]) + s_b[2][k][a]) + s_b[3][k][a];
        }
    }
}

// omega_a over the rows of the sites that exist (a detection, or z = 1 from the previous iteration); 0 on the others
__global__ void __launch_bounds__(PB_WG) k_pb_omega_a(const PbArgs A)
{
    const long long g = (long long)blockIdx.x * PB_WG + threadIdx.x;
    if (g >= (long long)A.C * A.R) return;
    const int chain = (int)(g / A.R), r = (int)(g - (long long)chain * A.R);
    const int t = A.row_t[r];
    double om = 0.0;
    if (A.obs_site[t] || A.z[(size_t)chain * A.n + A.site_id[t]]) {
        const PbChain &ch = A.ch[chain];
        double loc = 0.0;
        for (int a = 0; a < A.q; ++a) loc = fma(A.Wt[(size_t)a * A.R + r], ch.alpha[a], loc);
        const double U = block_uniform(ch.key, (uint32_t)r, 0, ch.it, STREAM_OMEGA_A);
        om = A.yrow[r] ? tn_pos(loc, U) : tn_neg(loc, U);
    }
    A.omega_a[(size_t)chain * A.R + r] = om;
}

template <int Q>
__global__ void __launch_bounds__(PB_WG) k_pb_alpha(const PbArgs A)
{
    constexpr int NA = nacc(Q);
    __shared__ double s_w[4][NA];
    __shared__ double s_acc[NA];
    __shared__ double s_U[MAXC * MAXC], s_work[2 * MAXC], s_out[MAXC], s_r[MAXC];
    const int chain = blockIdx.x, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    PbChain &ch = A.ch[chain];
    const uint64_t key = ch.key;
    const uint32_t it = ch.it;
    // beta: the tiles' partial sums in tile order, then the draw from the fixed factor
    if (tid < A.p) {
        double v = 0.0;
        for (int t = 0; t < A.ntile_eta; ++t) v += A.bpart[((size_t)t * A.C + chain) * A.p + tid];
        s_r[tid] = v + A.b_pbm[tid];
    }
    __syncthreads();
    if (tid == 0) {
        pb_fixed_draw(A.p, A.bU, s_r, key, it, STREAM_BETA, s_work, s_out);
        for (int a = 0; a < A.p; ++a) ch.beta[a] = s_out[a];
    }
    // alpha's sums over the rows of the existing sites: W_e'W_e (upper) and W_e' omega_a
    double acc[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) acc[k] = 0.0;
    for (int r = tid; r < A.R; r += PB_WG) {
        const int t = A.row_t[r];
        if (!(A.obs_site[t] || A.z[(size_t)chain * A.n + A.site_id[t]])) continue;
        const double om = A.omega_a[(size_t)chain * A.R + r];
        double w[Q];
#pragma unroll
        for (int a = 0; a < Q; ++a) w[a] = A.Wt[(size_t)a * A.R + r];
        int k = 0;
#pragma unroll
        for (int a = 0; a < Q; ++a)
#pragma unroll
            for (int b = a; b < Q; ++b) { acc[k] = fma(w[a], w[b], acc[k]); ++k; }
#pragma unroll
        for (int a = 0; a < Q; ++a) acc[NA - Q + a] = fma(w[a], om, acc[NA - Q + a]);
    }
#pragma unroll
    for (int k = 0; k < NA; ++k) {
        const double v = wave_sum(acc[k]);
        if (lane == 0) s_w[wv][k] = v;
    }
    __syncthreads();
    if (tid == 0) {
        for (int k = 0; k < NA; ++k) s_acc[k] = ((s_w[0][k] + s_w[1][k]) + s_w[2][k]) + s_w[3][k];
        const bool ok = precision_mvnorm_dev(Q, s_acc, A.a_prec, A.a_pbm, key, it, STREAM_ALPHA, s_U, s_work, s_out, nullptr);
        if (!ok) ch.err = -4;  // OCC_E_CHOLESKY
        for (int a = 0; a < Q; ++a) ch.alpha[a] = s_out[a];
    }
}

// the z update of one site of one chain -> its z
__device__ __forceinline__ int pb_z_site(const PbArgs &A, int chain, int i)
{
    const int t = A.sidx[i];
    if (t >= 0 && A.obs_site[t]) return 1;  // a detection: z stays 1
    const PbChain &ch = A.ch[chain];
    const size_t ci = (size_t)chain * A.n + i;
    const double loc = (xdot(A.Xt, A.n, i, ch.beta, A.p) + A.eta[ci]) + A.eps[ci];
    const double pz = 0.5 * erfc(-loc * kSqrtHalf), qz = 0.5 * erfc(loc * kSqrtHalf);
    double pr = pz;
    if (t >= 0) {
        double prod = 1.0;
        for (int r = A.site_ptr[t]; r < A.site_ptr[t + 1]; ++r) {
            double wa = 0.0;
            for (int a = 0; a < A.q; ++a) wa = fma(A.Wt[(size_t)a * A.R + r], ch.alpha[a], wa);
            prod *= 0.5 * erfc(wa * kSqrtHalf);
        }
        const double num = pz * prod;
        pr = num / (qz + num);
    }
    const double u = block_uniform(ch.key, (uint32_t)i, 0, ch.it, STREAM_Z);
    A.z[ci] = u < pr ? 1 : 0;
    return u < pr ? 1 : 0;
}

__global__ void __launch_bounds__(PB_WG) k_pb_z(const PbArgs A)
{
    const long long g = (long long)blockIdx.x * PB_WG + threadIdx.x;
    if (g >= (long long)A.C * A.n) return;
    const int chain = (int)(g / A.n), i = (int)(g - (long long)chain * A.n);
    (void)pb_z_site(A, chain, i);
}

// k_pb_z with the occupied sites per region and draw: launched in its place while a chain of the handle has its switch on.
// One chain per workgroup (blockIdx.y), so that a workgroup's sites share the row they add to (region_count); the update of
// a site is k_pb_z's own function: the same z.  `on` [C]: the chains' switches; *rec: [C][rec_keep][G] counts of the running
// occ_run, or null; the rows are those k_pb_tail records.
struct PbRegions {
    const int16_t *region_id;  // [n], -1: no region
    const uint32_t *on;
    uint32_t **rec;
    int G;
};
__global__ void __launch_bounds__(PB_WG) k_pb_z_occ(const PbArgs A, const PbRegions Rg)
{
    const int chain = blockIdx.y, i = blockIdx.x * PB_WG + threadIdx.x;
    const PbChain &ch = A.ch[chain];
    const uint32_t it = ch.it;
    uint32_t *rec = *Rg.rec;
    uint32_t *row = nullptr;  // (uniform over the workgroup)
    if (rec && Rg.on[chain] && it >= ch.rec_first && it - ch.rec_first < ch.rec_keep)
        row = rec + ((size_t)chain * ch.rec_keep + (it - ch.rec_first)) * (size_t)Rg.G;
    const int g = (row != nullptr && i < A.n) ? (int)Rg.region_id[i] : -1;
    int zi = 0;
    if (i < A.n) zi = pb_z_site(A, chain, i);
    if (row != nullptr) region_count(row, Rg.G, g, zi);
}

__global__ void __launch_bounds__(64) k_pb_tail(const PbArgs A)
{
    const int c = blockIdx.x * 64 + threadIdx.x;  // (launched with ceil(C / 64) blocks)
    if (c >= A.C) return;
    PbChain &ch = A.ch[c];
    const uint32_t it = ch.it;
    double *rec = *A.rec;
    if (rec && it >= ch.rec_first && it - ch.rec_first < ch.rec_keep) {
        const int w = A.q + A.p + 1;
        double *row = rec + ((size_t)c * ch.rec_keep + (it - ch.rec_first)) * w;
        for (int a = 0; a < A.q; ++a) row[a] = ch.alpha[a];
        for (int a = 0; a < A.p; ++a) row[A.q + a] = ch.beta[a];
        row[A.q + A.p] = ch.tau;
    }
    ch.it = it + 1;
}

// occ_draw kinds 5 and 6
__global__ void __launch_bounds__(256) k_pb_draw(int negative, uint64_t key, uint32_t it, uint32_t stream, long long n,
                                                 const double *__restrict__ loc, double *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double U = block_uniform(key, (uint32_t)i, 0, it, stream);
    out[i] = negative ? tn_neg(loc[i], U) : tn_pos(loc[i], U);
}

}  // namespace occ
