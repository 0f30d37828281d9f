// sampler_math.h — the arithmetic of the sampled chains, written ONCE for the device (k_sample_next, kernels/sample.h) and the host
// mirror (llm_sample_chain / llm_sample_exact, host/llm_infer.cpp).  The chain's contract is equality with the stepped loop, ids byte
// for byte, so nothing here calls a library transcendental: only IEEE f32 / f64 multiply, add, subtract, divide, rintf, conversions and
// integer construction / dissection of a float's bits, which round identically on both sides when neither contracts a multiply and an
// add (-ffp-contract=off, as the whole library is built).  Plain C++ where __HIPCC__ is absent.
//
// ---- THE SPECIFICATION (tests/sampler_chain_ref.py restates it in numpy from this text) ----
// One step takes a row x[V] (no NaN), the window (the last <= 64 tokens, repeats allowed), {k, top_p, temperature, penalty}, the extras
// freq, presence, tail_free_z, typical_p, min_p, n_bias <= 64 pairs (id, b), mirostat in {0, 2}, tau, eta, and the per-session state
// rng (xorshift64*) and mu (f32).  Neutral extras — freq 0, presence 0, z 1, typical 1, min_p 0, no bias, mirostat 0 — give the
// default chain of the four parameters, bit for bit.
//  A. Adjusted values.  M = the window's distinct ids united with the bias ids, each once (|M| <= 128).  For t in M, in f32, every
//     operation rounded (sampler_adjust; the reference's order: flat bias, repetition, frequency / presence):
//       v = x[t];  biased: v = v + b;  in the window, c >= 1 occurrences: v = sampler_penalise(v, penalty), then, unless
//       freq == 0 && presence == 0, v = v - ((float)c * freq + presence).  (A token that is only biased has no occurrence: neither
//       penalty touches it, as in the reference, whose penalties walk the last tokens.)  b = -inf is legal: the usual ban.
//  B. Candidates (mirostat == 0).  The raw top-k (value descending, lower id first among equals) united with M, M's members with
//     their adjusted values; sorted by (value descending, id ascending); the k best kept.  The raw (k + 1)-th logit does not move up.
//  C. Survivor filters, on B's ordered list, in the reference's order.  q_i = sampler_exp(v_i - v_0) and p_i = sampler_exp((v_i -
//     v_0) / temperature), f32, computed once against B's first value.  Every sum is f64 over the current survivors in list order;
//     every filter keeps >= 1 entry; survivors stay in list order.
//     1. tail-free (skipped when z >= 1 or n < 3; sampler_tail_free): d1_i = (double)q_i - (double)q_{i+1}, d2_i = |d1_i - d1_{i+1}|,
//        i = 0 .. n - 3, D = sum d2; skipped when D == 0; i = the first index whose running sum of d2 exceeds (double)z * D: the first
//        max(i, 1) entries are kept, all of them if there is no such index.
//     2. locally typical (skipped when typical_p >= 1): s_i = v_0 - v_i (f32); Q = sum q_i; mean = (sum of (double)q_i * (double)s_i
//        over the entries with q_i > 0) / Q; t_i = |(double)s_i - mean|, +inf where q_i == 0; entries are visited by (t ascending,
//        index ascending), q accumulated, until the sum exceeds (double)typical_p * Q; the visited entries are kept (all, if it never
//        does).  The keys are unique, so any sorting algorithm gives the same order.  No logarithm: |-ln p_i - H| is |s_i - E s|.
//     3. top-p (skipped when top_p >= 1): Q = sum q over the survivors, the shortest prefix m >= 1 of them whose running sum reaches
//        (double)top_p * Q.
//     4. min-p (skipped when min_p <= 0): the entries with q_i >= min_p * q_first (an f32 product), first = the first survivor.
//  D. Draw.  S = sum of p over the survivors; x = xorshift64*(rng); u = (double)((x * 0x2545F4914F6CDD1D) >> 11) / 2^53 * S; the
//     first survivor whose running sum of p exceeds u, else the last.
//  E. Mirostat 2 (mirostat == 2) replaces B - D (the reference's chain with Mirostat has no truncating sampler).  Over ALL V entries
//     a_i = the adjusted value for i in M, else x_i; amax = max a_i; e_i = sampler_exp((a_i - amax) / temperature).  Ids are taken in
//     blocks of 32 consecutive ids: S_b = the f64 sum of block b's e in id order from 0, S = the sum of the S_b in block order from 0.
//     Retained: R = {i : (double)e_i >= S * (double)sampler_exp(-mu * ln2)} (ln2 = 0.693147182f, the product f32; the condition
//     "surprise <= mu" without a logarithm) and, in every case, the lowest id with a_i == amax; when mu < 0, R is that id alone.
//     S_R,b and S_R: the same sums over the retained entries.  x = xorshift64*(rng), u = (double)(bits) / 2^53 * S_R.  Blocks are
//     walked in order, run += S_R,b, to the first block with run > u; inside it the retained ids in id order, acc from 0, acc += e_i,
//     the first with u - (run before the block) < acc, else the block's last retained id.  No such block: the last retained id.
//     s_obs = -sampler_log2((double)e_sel / S_R); mu <- mu - eta * (s_obs - tau), three f32 operations.  Callers start mu at 2 tau.
//     sampler_log2: f64 in; exponent and mantissa from the bits, mantissa m in [sqrt(1/2), sqrt(2)); ln m = 2 s (1 + s^2/3 + ... +
//     s^14/15), s = (m - 1) / (m + 1), by Horner in f64; result (E + ln m * log2 e) rounded to f32; -1022 below the normal range.
//  Declined (-1, nothing executed, rng and mu unmoved): k outside 1 .. V (the device entries: > 256), temperature, top_p or penalty
//  <= 0, a window token outside the vocabulary, NaN in any parameter, z <= 0, typical_p <= 0, min_p outside [0, 1], n_bias outside
//  0 .. 64, a bias id outside the vocabulary or listed twice, a bias that is NaN or +inf, mirostat not 0 or 2, mirostat == 2 with
//  top_p < 1, z < 1, typical_p < 1 or min_p > 0 (k is not read then), tau <= 0, eta < 0, a NaN mu; the device entries only:
//  mirostat == 2 with V > 32768.  Not representable: Mirostat 1, top-a, sequence repetition, another window.
// Rows are assumed free of NaN (and of +inf beside a -inf bias); -inf gets probability 0 (a row of nothing but -inf gives candidate 0).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SAMPLER_FN __host__ __device__ inline
#else
#define SAMPLER_FN inline
#endif

constexpr int SAMPLER_K_MAX = 256;   // k_sample_next's LDS budget
constexpr int SAMPLER_WINDOW = 64;   // tokens of history the repetition penalty looks at
constexpr int SAMPLER_BIAS_MAX = 64; // entries of the flat token bias
constexpr int SAMPLER_M_MAX = SAMPLER_WINDOW + SAMPLER_BIAS_MAX;  // ids whose value a step adjusts
constexpr int SAMPLER_BLOCK = 32;    // Mirostat 2 sums ids in blocks of this many (k_sample_next: one thread's registers)

// e^x for x <= 0, Cephes' expf scheme in separate f32 operations: exactly 0 below -80 (and for NaN), exactly 1 at 0; relative error
// against f64 exp 7.9e-8 (1.33 * 2^-24) at most on [-80, 0], monotone there (tests/test_sampler_ref.py measures both).
SAMPLER_FN float sampler_exp(float x) {
    if (!(x >= -80.0f)) return 0.0f;
    const float n = rintf(x * 1.44269504f);
    float r = x - n * 0.693359375f;
    r = r - n * -2.12194440e-4f;
    const float r2 = r * r;
    float p = 1.9875691500e-4f;
    p = p * r + 1.3981999507e-3f;
    p = p * r + 8.3334519073e-3f;
    p = p * r + 4.1665795894e-2f;
    p = p * r + 1.6666665459e-1f;
    p = p * r + 5.0000001201e-1f;
    const float y = (p * r2 + r) + 1.0f;
    const uint32_t bits = (uint32_t)((int)n + 127) << 23;  // 2^n, n >= -115
    return y * __builtin_bit_cast(float, bits);
}
// the repetition penalty on one logit of the window
SAMPLER_FN float sampler_penalise(float v, float penalty) { return v > 0.0f ? v / penalty : v * penalty; }
SAMPLER_FN float sampler_q(float v, float v0) { return sampler_exp(v - v0); }
SAMPLER_FN float sampler_p(float v, float v0, float temperature) { return sampler_exp((v - v0) / temperature); }
// top-p over q[0 .. n), then the draw over p: returns the candidate's index and steps *rng once (xorshift64*)
SAMPLER_FN int sampler_pick(const float *q, const float *p, int n, float top_p, uint64_t *rng) {
    int m = n;
    if (top_p < 1.0f) {
        double Q = 0.0;
        for (int i = 0; i < n; i++) Q += (double)q[i];
        const double need = (double)top_p * Q;
        double acc = 0.0;
        for (int i = 0; i < n; i++) {
            acc += (double)q[i];
            if (acc >= need) {
                m = i + 1;
                break;
            }
        }
    }
    double S = 0.0;
    for (int i = 0; i < m; i++) S += (double)p[i];
    uint64_t x = *rng;
    x ^= x >> 12;
    x ^= x << 25;
    x ^= x >> 27;
    *rng = x;
    const double u = (double)((x * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0 * S;
    double acc = 0.0;
    for (int i = 0; i < m; i++) {
        acc += (double)p[i];
        if (u < acc) return i;
    }
    return m - 1;
}

// ---- the extended chain (specification A, C - E) ----
// A: the adjusted value of a token of M; c = its occurrences in the window (0: only biased)
SAMPLER_FN float sampler_adjust(float x, bool biased, float b, int c, float penalty, float freq, float presence) {
    float v = x;
    if (biased) v = v + b;
    if (c > 0) {
        v = sampler_penalise(v, penalty);
        if (!(freq == 0.0f && presence == 0.0f)) v = v - ((float)c * freq + presence);
    }
    return v;
}
SAMPLER_FN double sampler_abs(double d) { return d < 0.0 ? -d : d; }
SAMPLER_FN uint64_t sampler_rng_step(uint64_t x) {
    x ^= x >> 12;
    x ^= x << 25;
    x ^= x >> 27;
    return x;
}
SAMPLER_FN double sampler_rng_unit(uint64_t x) { return (double)((x * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0; }
// C.1: how many of q[0 .. n) tail-free keeps (a prefix)
SAMPLER_FN int sampler_tail_free(const float *q, int n, float z) {
    if (z >= 1.0f || n < 3) return n;
    double D = 0.0;
    for (int i = 0; i + 2 < n; i++) D += sampler_abs(((double)q[i] - (double)q[i + 1]) - ((double)q[i + 1] - (double)q[i + 2]));
    if (!(D > 0.0)) return n;
    const double need = (double)z * D;
    double run = 0.0;
    for (int i = 0; i + 2 < n; i++) {
        run += sampler_abs(((double)q[i] - (double)q[i + 1]) - ((double)q[i + 1] - (double)q[i + 2]));
        if (run > need) return i < 1 ? 1 : i;
    }
    return n;
}
// C.2: Q and the mean of s over v / q[0 .. n); then the key of one entry
SAMPLER_FN double sampler_typical_mean(const float *v, const float *q, int n, double *Q_out) {
    double Q = 0.0, A = 0.0;
    for (int i = 0; i < n; i++) Q += (double)q[i];
    for (int i = 0; i < n; i++)
        if (q[i] > 0.0f) A += (double)q[i] * (double)(v[0] - v[i]);
    *Q_out = Q;
    return A / Q;
}
SAMPLER_FN double sampler_typical_key(float v0, float vi, float qi, double mean) {
    if (!(qi > 0.0f)) return (double)INFINITY;
    return sampler_abs((double)(v0 - vi) - mean);
}
// C.2's visit, C.3, C.4 and D over the n entries tail-free left: ord (null: locally typical is skipped) lists them by (key ascending,
// index ascending), Q is sampler_typical_mean's; idx[n] is scratch (the survivors' indices).  Returns the drawn entry's index and
// steps *rng once.  With ord == null and min_p <= 0 this is sampler_pick, operation for operation.
SAMPLER_FN int sampler_pick_chain(const float *q, const float *p, int n, const int *ord, double Q, float typical_p, float top_p,
                                  float min_p, int *idx, uint64_t *rng) {
    int m = n;
    if (ord) {
        for (int i = 0; i < n; i++) idx[i] = 0;
        const double need = (double)typical_p * Q;
        double acc = 0.0;
        for (int j = 0; j < n; j++) {
            idx[ord[j]] = 1;
            acc += (double)q[ord[j]];
            if (acc > need) break;
        }
        m = 0;
        for (int i = 0; i < n; i++)
            if (idx[i]) idx[m++] = i;
    } else {
        for (int i = 0; i < n; i++) idx[i] = i;
    }
    if (top_p < 1.0f) {
        double Qs = 0.0;
        for (int j = 0; j < m; j++) Qs += (double)q[idx[j]];
        const double need = (double)top_p * Qs;
        double acc = 0.0;
        for (int j = 0; j < m; j++) {
            acc += (double)q[idx[j]];
            if (acc >= need) {
                m = j + 1;
                break;
            }
        }
    }
    if (min_p > 0.0f) {
        const float least = min_p * q[idx[0]];
        int kept = 0;
        for (int j = 0; j < m; j++)
            if (q[idx[j]] >= least) idx[kept++] = idx[j];
        m = kept;
    }
    double S = 0.0;
    for (int j = 0; j < m; j++) S += (double)p[idx[j]];
    const uint64_t x = sampler_rng_step(*rng);
    *rng = x;
    const double u = sampler_rng_unit(x) * S;
    double acc = 0.0;
    for (int j = 0; j < m; j++) {
        acc += (double)p[idx[j]];
        if (u < acc) return idx[j];
    }
    return idx[m - 1];
}
// E: log2 of a positive f64, rounded to f32.  Against f64 log2 over the ratios Mirostat 2 forms (e an f32 in (1e-35, 1], S in
// [1, 32768], powers of two): relative error 5.952e-8 (1.0 * 2^-24, the final rounding) at most, the exponent exactly at powers of
// two (tests/test_sampler_chain_ref.py measures both).
SAMPLER_FN float sampler_log2(double r) {
    if (!(r >= 2.2250738585072014e-308) || !(r <= 1.7976931348623157e308)) return -1022.0f;
    const uint64_t b = __builtin_bit_cast(uint64_t, r);
    int E = (int)(b >> 52) - 1023;
    double m = __builtin_bit_cast(double, (b & 0xFFFFFFFFFFFFFull) | 0x3FF0000000000000ull);
    if (m >= 1.4142135623730951) {
        m = m * 0.5;
        E += 1;
    }
    const double s = (m - 1.0) / (m + 1.0), s2 = s * s;
    double t = 1.0 / 15.0;
    t = t * s2 + 1.0 / 13.0;
    t = t * s2 + 1.0 / 11.0;
    t = t * s2 + 1.0 / 9.0;
    t = t * s2 + 1.0 / 7.0;
    t = t * s2 + 1.0 / 5.0;
    t = t * s2 + 1.0 / 3.0;
    t = t * s2 + 1.0;
    const double ln = (2.0 * s) * t;
    return (float)((double)E + ln * 1.4426950408889634);
}
// E: e_i of one entry; the retain threshold (compare (double)e_i >= it; mu >= 0); mu's update
SAMPLER_FN float sampler_mirostat_e(float a, float amax, float temperature) { return sampler_exp((a - amax) / temperature); }
SAMPLER_FN double sampler_mirostat_least(double S, float mu) { return S * (double)sampler_exp(-mu * 0.693147182f); }
SAMPLER_FN float sampler_mirostat_mu(float mu, float e_sel, double S_R, float tau, float eta) {
    const float s_obs = -sampler_log2((double)e_sel / S_R);
    return mu - eta * (s_obs - tau);
}

// What a chain's parameters must satisfy before anything runs (the specification's "declined"), for any struct laid out as
// ggml_hip_sampler_chain; k_max: 256 for the device entries, V for the host's.  mu is checked by the caller, where it has one.
template <class Chain>
inline bool sampler_chain_ok(const Chain &c, int64_t V, int64_t k_max) {
    const auto nan = [](float f) { return f != f; };
    if (c.mirostat != 0 && c.mirostat != 2) return false;
    if (!(c.base.temperature > 0.0f) || !(c.base.top_p > 0.0f) || !(c.base.penalty > 0.0f)) return false;
    if (c.mirostat == 0 && (c.base.k < 1 || c.base.k > k_max || c.base.k > V)) return false;
    if (nan(c.freq) || nan(c.presence) || !(c.tail_free_z > 0.0f) || !(c.typical_p > 0.0f) || !(c.min_p >= 0.0f && c.min_p <= 1.0f)) return false;
    if (!(c.tau > 0.0f) || !(c.eta >= 0.0f)) return false;
    if (c.n_bias < 0 || c.n_bias > SAMPLER_BIAS_MAX) return false;
    for (int i = 0; i < c.n_bias; i++) {
        if (c.bias_id[i] < 0 || c.bias_id[i] >= V || nan(c.bias[i]) || c.bias[i] == INFINITY) return false;
        for (int j = 0; j < i; j++)
            if (c.bias_id[j] == c.bias_id[i]) return false;
    }
    if (c.mirostat == 2 && (c.base.top_p < 1.0f || c.tail_free_z < 1.0f || c.typical_p < 1.0f || c.min_p > 0.0f)) return false;
    return true;
}
// the default chain's four parameters with neutral extras
template <class Chain, class Base>
inline Chain sampler_chain_neutral(const Base &b) {
    Chain c = {};
    c.base = b;
    c.tail_free_z = 1.0f;
    c.typical_p = 1.0f;
    c.tau = 5.0f;
    c.eta = 0.1f;
    return c;
}
// whether a chain is the default chain: k_sample_next's default instantiation serves it
template <class Chain>
inline bool sampler_chain_is_default(const Chain &c) {
    return c.mirostat == 0 && c.n_bias == 0 && c.freq == 0.0f && c.presence == 0.0f && c.tail_free_z >= 1.0f && c.typical_p >= 1.0f &&
           c.min_p <= 0.0f;
}
