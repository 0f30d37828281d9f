// sampler_math.h — the arithmetic of the sampled chains (top-k / repetition penalty / top-p / temperature / draw), written
// ONCE for the device (k_sample_next, kernels/sample.h) and the host mirror (llm_sample_exact, host/llm_infer.cpp). The chain's
// contract is equality with the stepped loop, ids byte for byte, so nothing here calls a library transcendental: only IEEE f32 / f64
// multiply, add, subtract, divide, rintf and integer construction of a power of two, which round identically on both sides when
// neither contracts a multiply and an add (-ffp-contract=off, as the whole library is built).  Plain C++ where __HIPCC__ is absent.
//
// One sampling step, from a row of logits, a window of token ids (each once) and {k, top_p, temperature, penalty}:
//   1. candidates: the k largest raw logits (value descending, lower id first among equals) and the window's tokens, each id once;
//      a window token's value v becomes sampler_penalise(v); sorted by (value descending, id ascending), the k best kept
//      (the raw (k + 1)-th logit does not move up when the penalty pushes a window token out of the k best);
//   2. q_i = sampler_exp(v_i - v_0), p_i = sampler_exp((v_i - v_0) / temperature), all f32;
//   3. sampler_pick: top-p on q (f64 sums in candidate order, the shortest prefix m >= 1 reaching top_p * Q; skipped when
//      top_p >= 1), then one xorshift64* draw over the f64 sums of p_0 .. p_{m-1}.
// Rows are assumed free of NaN; -inf gets probability 0 (a row of nothing but -inf gives candidate 0).
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
