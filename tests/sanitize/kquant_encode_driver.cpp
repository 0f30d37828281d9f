// kquant_encode_driver.cpp — sanitizer job for the host K-quant encoders (llm_amd/csrc/ggml_core.cpp: ggml_quantize_q2_K ..
// q6_K, ggml_quantize_chunk), built by tests/test_sanitize_kquant.py with -fsanitize=address,undefined.  Every type at
// (ne0, ne1) = (256, 1), (768, 3), (11008, 2) and at 4096 super-blocks (the threaded path); source and destination live in
// heap buffers of the exact size, so a read or write one byte past a block is a report.  The inputs carry an all-zero
// super-block, an all-zero sub-block, a super-block of non-negative values and a row of values too small for an f16 scale.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>

#include "ggml_hip.h"

typedef size_t (*quantize_fn)(const float *, void *, int, int, int64_t *);

static uint32_t g_state = 12345u;
static float next_gauss() {  // sum of four uniforms, centred: enough of a bell for a memory test
    float s = 0.0f;
    for (int i = 0; i < 4; i++) {
        g_state = g_state * 1664525u + 1013904223u;
        s += (float)(g_state >> 8) / 16777216.0f;
    }
    return 0.02f * (s - 2.0f);
}

static int run(const char *name, ggml_type type, quantize_fn fn, int ne0, int ne1) {
    const int n = ne0 * ne1;
    const size_t bytes = (size_t)(n / 256) * ggml_type_size(type);
    std::unique_ptr<float[]> x(new float[(size_t)n]);
    for (int i = 0; i < n; i++) x[(size_t)i] = next_gauss();
    const int nsb = n / 256;
    if (nsb > 1) memset(x.get(), 0, 256 * sizeof(float));                                 // an all-zero super-block
    if (nsb > 2) memset(x.get() + 256 + 32, 0, 32 * sizeof(float));                       // an all-zero sub-block
    if (nsb > 3) for (int i = 0; i < 256; i++) x[(size_t)(512 + i)] = fabsf(x[(size_t)(512 + i)]);  // max_min == 0
    if (nsb > 4) for (int i = 0; i < 256; i++) x[(size_t)(768 + i)] = (i & 1) ? 1e-9f : -1e-9f;     // f16(d) == 0
    std::unique_ptr<uint8_t[]> whole(new uint8_t[bytes]), halves(new uint8_t[bytes]);
    int64_t hist[16];
    for (int i = 0; i < 16; i++) hist[i] = 7 * i - 3;
    if (fn(x.get(), whole.get(), n, ne0, hist) != bytes) {
        fprintf(stderr, "%s [%d, %d]: wrong return value\n", name, ne0, ne1);
        return 1;
    }
    const int start = (nsb / 2) * 256;
    size_t got = 0;
    if (start > 0) got += ggml_quantize_chunk(type, x.get(), halves.get(), 0, start, hist);
    got += ggml_quantize_chunk(type, x.get(), halves.get(), start, n - start, nullptr);
    if (got != bytes || memcmp(whole.get(), halves.get(), bytes) != 0) {
        fprintf(stderr, "%s [%d, %d]: ggml_quantize_chunk in two halves differs from the whole\n", name, ne0, ne1);
        return 1;
    }
    for (int i = 0; i < 16; i++)
        if (hist[i] != 7 * i - 3) {
            fprintf(stderr, "%s [%d, %d]: hist was written\n", name, ne0, ne1);
            return 1;
        }
    return 0;
}

int main() {
    const struct { const char *name; ggml_type type; quantize_fn fn; } types[] = {
        {"q2_K", GGML_TYPE_Q2_K, ggml_quantize_q2_K}, {"q3_K", GGML_TYPE_Q3_K, ggml_quantize_q3_K},
        {"q4_K", GGML_TYPE_Q4_K, ggml_quantize_q4_K}, {"q5_K", GGML_TYPE_Q5_K, ggml_quantize_q5_K},
        {"q6_K", GGML_TYPE_Q6_K, ggml_quantize_q6_K}};
    const int shapes[][2] = {{256, 1}, {768, 3}, {11008, 2}, {4096, 256}};
    int bad = 0;
    for (const auto &t : types)
        for (const auto &s : shapes) bad += run(t.name, t.type, t.fn, s[0], s[1]);
    if (bad) return 1;
    printf("kquant encode driver OK\n");
    return 0;
}
