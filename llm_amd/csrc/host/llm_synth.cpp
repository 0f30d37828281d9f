// llm_synth.cpp — generators of benchmark and test data: synthetic GGML blocks and quantized gaussian rows at full model size.
// Exported with the host mirror's entry points (llm_host.h); no part of inference.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "llm_host.h"

static uint64_t splitmix64(uint64_t &x) {  // the counter-based generator of both: one step
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// work(b0, b1) over [0, n) cut into equal ranges, one thread each: as many as the host has, `cap` at the most
template <class F>
static void on_threads(int64_t n, unsigned cap, F work) {
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt == 0 ? 1 : (nt > cap ? cap : nt);
    std::vector<std::thread> th;
    const int64_t per = (n + nt - 1) / nt;
    for (unsigned t = 0; t < nt; t++) {
        const int64_t b0 = (int64_t)t * per, b1 = std::min<int64_t>(n, b0 + per);
        if (b0 < b1) th.emplace_back(work, b0, b1);
    }
    for (auto &t : th) t.join();
}

extern "C" {

// Synthetic GGML blocks for full-size benchmarks (no checkpoints are obtainable offline): uniform random
// quants, f16 scale d = d_scale*(0.5+u), and for the *_1 types a min that centres the block.  Fills
// `nblocks` blocks of `type` at dst; deterministic in (seed, block index); multi-threaded.
void llm_synth_blocks(int type, void *dst, int64_t nblocks, uint64_t seed, float d_scale) {
    const size_t bs = ggml_type_size((ggml_type)type);
    const bool has_m = type == GGML_TYPE_Q4_1 || type == GGML_TYPE_Q5_1;
    const float lv = type == GGML_TYPE_Q4_1 ? 7.5f : 15.5f;
    on_threads(nblocks, 32, [&](int64_t b0, int64_t b1) {
        uint8_t *p = (uint8_t *)dst + (size_t)b0 * bs;
        for (int64_t b = b0; b < b1; b++, p += bs) {
            uint64_t x = seed * 0x9E3779B97F4A7C15ull + (uint64_t)b * 0xD1B54A32D192ED03ull;
            auto next = [&x]() { return splitmix64(x); };
            for (size_t o = 0; o < bs; o += 8) {
                const uint64_t r = next();
                memcpy(p + o, &r, bs - o < 8 ? bs - o : 8);
            }
            const float u = (float)(next() >> 40) * (1.0f / 16777216.0f);
            const float d = d_scale * (0.5f + u);
            const ggml_fp16_t dh = ggml_fp32_to_fp16(d);
            if (type == GGML_TYPE_Q6_K) {  // block_q6_K: ql[128] qh[64] scales[16] d — int8 scales x 6-bit quants, |sc*q| ~ 1e3
                const ggml_fp16_t d6 = ggml_fp32_to_fp16(d * (1.0f / 1024.0f));
                memcpy(p + 208, &d6, 2);
                continue;
            }
            if (type == GGML_TYPE_Q5_K) {  // block_q5_K: d dmin scales[12] qh[32] qs[128] — x = d*sc*q - dmin*m, q five-bit, sc, m six-bit
                const ggml_fp16_t d5 = ggml_fp32_to_fp16(d * (1.0f / 64.0f)), m5 = ggml_fp32_to_fp16(d * (15.5f / 64.0f));
                memcpy(p, &d5, 2);
                memcpy(p + 2, &m5, 2);
                continue;
            }
            if (type == GGML_TYPE_Q3_K) {  // block_q3_K: hmask[32] qs[64] scales[12] d — x = d*(sc-32)*(q-4), sc six-bit, q three-bit
                const ggml_fp16_t d3 = ggml_fp32_to_fp16(d * (1.0f / 16.0f));
                memcpy(p + 108, &d3, 2);
                continue;
            }
            if (type == GGML_TYPE_Q2_K) {  // block_q2_K: scales[16] qs[64] d dmin — x = d*sc*q - dmin*m, sc, m four-bit, q two-bit
                const ggml_fp16_t d2 = ggml_fp32_to_fp16(d * (1.0f / 4.0f)), m2 = ggml_fp32_to_fp16(d * (1.5f / 4.0f));
                memcpy(p + 80, &d2, 2);
                memcpy(p + 82, &m2, 2);
                continue;
            }
            if (type == GGML_TYPE_Q4_K) {  // block_q4_K: d dmin scales[12] qs[128] — x = d*sc*q - dmin*m, sc, m six-bit
                const ggml_fp16_t d4 = ggml_fp32_to_fp16(d * (1.0f / 32.0f)), m4 = ggml_fp32_to_fp16(d * (7.5f / 32.0f));
                memcpy(p, &d4, 2);
                memcpy(p + 2, &m4, 2);
                continue;
            }
            memcpy(p, &dh, 2);
            if (has_m) {
                const ggml_fp16_t mh = ggml_fp32_to_fp16(-lv * ggml_fp16_to_fp32(dh));
                memcpy(p + 2, &mh, 2);
            }
        }
    });
}

// BASELINE.md section 4's synthetic weights at full size: rows of N(0, std^2) f32 quantized by ggml_quantize_q* (the
// product's host quantizer = what the reference's quantize tool calls), written as raw GGML blocks.  The gaussians come
// from a counter-based generator (splitmix64 + Box-Muller, deterministic in (seed, row)) instead of numpy's stream:
// 6.6e9 numpy draws take minutes of single-thread time before a bench could start.  Rows are cut over the host's
// threads.  `type` = a block type of 32 weights; ne0 = row length (multiple of 32); ne1 = rows.
void llm_synth_gaussian(int type, void *dst, int64_t ne0, int64_t ne1, uint64_t seed, float std) {
    const size_t row_bytes = (size_t)(ne0 / 32) * ggml_type_size((ggml_type)type);
    on_threads(ne1, 64, [&](int64_t r0, int64_t r1) {
        std::vector<float> row((size_t)ne0);
        int64_t hist[16] = {0};
        for (int64_t r = r0; r < r1; r++) {
            uint64_t x = seed * 0x9E3779B97F4A7C15ull + (uint64_t)r * 0xD1B54A32D192ED03ull;
            auto next = [&x]() { return splitmix64(x); };
            for (int64_t i = 0; i < ne0; i += 2) {
                const uint64_t u = next();
                const float u1 = ((float)(u >> 40) + 1.0f) * (1.0f / 16777216.0f);  // (0, 1]
                const float u2 = (float)((u >> 16) & 0xFFFFFF) * (1.0f / 16777216.0f);
                const float m = std * sqrtf(-2.0f * logf(u1));
                row[i] = m * cosf(6.2831853071795865f * u2);
                if (i + 1 < ne0) row[i + 1] = m * sinf(6.2831853071795865f * u2);
            }
            ggml_quantize_chunk((ggml_type)type, row.data(), (uint8_t *)dst + (size_t)r * row_bytes, 0, (int)ne0, hist);
        }
    });
}

}  // extern "C"
