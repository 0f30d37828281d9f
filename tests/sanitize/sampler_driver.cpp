// sampler_driver.cpp — the workload of the sanitizer job for the sampled batched chain's host side (tests/test_sanitize_sampler.py):
// llm_host.cpp and ggml_core.cpp under ASan + UBSan, linked against tests/sanitize/stub_backend.cpp, which has neither a batched step
// nor a sampled chain.  What runs here: llm_sample_exact on edge rows (one entry, k = V, all equal, all -inf, zeros of both signs,
// a window longer than 64 tokens, bad arguments), and llm_infer_tokens_sampled_batch_via / llm_infer_next_tokens_sampled_batch_via
// with NULL entries and with a chain entry that declines: the argument checks (-1, no session and no generator moved), the staging
// of B graphs and windows for the entry, and the fall-back loop's indexing of out_ids [n][B] — one session with a prompt of 70
// tokens, so that its window is cut to 64.  Row 0 of every call is checked against llm_sample_exact on the session's own logits.
// usage: sampler_driver <model.ggjt>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ggml_hip.h"
#include "host/llm_host.h"

#define CHECK(c)                                                                      \
    do {                                                                              \
        if (!(c)) {                                                                   \
            fprintf(stderr, "sampler driver: CHECK failed at line %d: %s\n", __LINE__, #c); \
            exit(2);                                                                  \
        }                                                                             \
    } while (0)

static const llm_sampler_params DEFAULT = {40, 0.95f, 0.8f, 1.30f};

static int g_chain_calls = 0;
static std::vector<int32_t> g_windows, g_window_n;
static int declining_chain(struct ggml_cgraph *const *graphs, int n_graphs, int n_steps, const ggml_hip_sampler *params,
                           const int32_t *windows, const int32_t *window_n, uint64_t *rng, int32_t *out_ids) {
    CHECK(graphs && params && windows && window_n && rng && out_ids && n_steps >= 1);
    for (int i = 0; i < n_graphs; i++) CHECK(graphs[i] && graphs[i]->n_nodes > 0);
    g_windows.assign(windows, windows + (size_t)n_graphs * 64);  // (reads all of [B][64])
    g_window_n.assign(window_n, window_n + n_graphs);
    for (int i = 0; i < (n_steps - 1) * n_graphs; i++) out_ids[i] = -9;  // (writes all of [n_steps - 1][B]; discarded by the caller)
    for (int i = 0; i < n_graphs; i++) rng[i] ^= 0x5555;                 // (a declining entry's scribbles must not reach the caller)
    g_chain_calls++;
    return -1;  // nothing executed
}

static std::vector<int32_t> prompt_of(int c, int V) {
    std::vector<int32_t> toks((size_t)(c == 1 ? 70 : 2 + 3 * c));  // ragged; session 1 comes with more than a window of history
    for (size_t i = 0; i < toks.size(); i++) toks[i] = (int32_t)((i * 37 + 5 * (size_t)c + 1) % (size_t)V);
    return toks;
}
static std::vector<llm_session *> make_sessions(llm_model *m, int B, int V) {
    std::vector<llm_session *> ss;
    for (int c = 0; c < B; c++) {
        llm_session_config cfg = {GGML_TYPE_F16, GGML_TYPE_F16, 8, 4};
        llm_session *s = llm_start_session(m, &cfg);
        CHECK(s);
        const std::vector<int32_t> toks = prompt_of(c, V);
        llm_feed_prompt(m, s, toks.data(), (int)toks.size());
        ss.push_back(s);
    }
    return ss;
}

static void sample_exact_edges() {
    uint64_t rng = 42;
    const float one[1] = {-3.5f};
    const llm_sampler_params k1 = {1, 0.95f, 0.8f, 1.30f};
    const int32_t w0[3] = {0, 0, 0};
    CHECK(llm_sample_exact(one, 1, nullptr, 0, &k1, &rng) == 0 && rng != 42);
    CHECK(llm_sample_exact(one, 1, w0, 3, &k1, &rng) == 0);
    std::vector<float> row(40);
    for (int i = 0; i < 40; i++) row[(size_t)i] = 0.25f * (float)((i * 7) % 11) - 1.0f;
    std::vector<int32_t> window(80);
    for (int i = 0; i < 80; i++) window[(size_t)i] = (i * 13) % 40;
    const llm_sampler_params kv = {40, 0.95f, 0.8f, 1.30f};  // k = V, a window longer than 64 tokens
    for (int i = 0; i < 50; i++) {
        const int32_t id = llm_sample_exact(row.data(), 40, window.data(), 80, &kv, &rng);
        CHECK(id >= 0 && id < 40);
    }
    std::vector<float> flat(33, -0.5f), ninf(33, -INFINITY), zeros(33);
    for (int i = 0; i < 33; i++) zeros[(size_t)i] = (i & 1) ? -0.0f : 0.0f;
    const llm_sampler_params k8 = {8, 1e-6f, 0.1f, 1.30f}, k8p1 = {8, 1.0f, 1.0f, 1.30f};
    const int32_t w5[5] = {0, 13, 26, 32, 13};
    for (const std::vector<float> *r : {&flat, &ninf, &zeros})
        for (const llm_sampler_params *p : {&k8, &k8p1}) {
            const int32_t id = llm_sample_exact(r->data(), 33, w5, 5, p, &rng);
            CHECK(id >= 0 && id < 33);
        }
    CHECK(llm_sample_exact(ninf.data(), 33, nullptr, 0, &k8, &rng) == 0);  // nothing but -inf: candidate 0
    // bad arguments: -1, the generator as it was
    const uint64_t before = rng;
    const llm_sampler_params bad_k0 = {0, 0.95f, 0.8f, 1.3f}, bad_kv = {41, 0.95f, 0.8f, 1.3f}, bad_t = {8, 0.95f, 0.0f, 1.3f},
                             bad_p = {8, 0.0f, 0.8f, 1.3f}, bad_pen = {8, 0.95f, 0.8f, 0.0f};
    for (const llm_sampler_params *p : {&bad_k0, &bad_kv, &bad_t, &bad_p, &bad_pen}) CHECK(llm_sample_exact(row.data(), 40, window.data(), 80, p, &rng) == -1);
    const int32_t outside[2] = {3, 40};
    CHECK(llm_sample_exact(row.data(), 40, outside, 2, &kv, &rng) == -1);
    CHECK(llm_sample_exact(nullptr, 40, window.data(), 80, &kv, &rng) == -1);
    CHECK(llm_sample_exact(row.data(), 0, window.data(), 80, &kv, &rng) == -1);
    CHECK(llm_sample_exact(row.data(), 40, nullptr, 3, &kv, &rng) == -1);
    CHECK(llm_sample_exact(row.data(), 40, window.data(), 80, nullptr, &rng) == -1);
    CHECK(llm_sample_exact(row.data(), 40, window.data(), 80, &kv, nullptr) == -1);
    CHECK(rng == before);
}

int main(int argc, char **argv) {
    CHECK(argc == 2);
    sample_exact_edges();
    const int C = 128;
    llm_model_params mp = {C, 1, -1, 0, 1.0f, 10000, 0, -1, 0};
    llm_model *m = llm_llama_load(argv[1], &mp);
    CHECK(m);
    const int V = llm_model_n_vocab(m);
    for (int B : {1, 2, 5}) {
        for (int n : {1, 6}) {
            for (llm_batch_sample_entry chain : {(llm_batch_sample_entry) nullptr, (llm_batch_sample_entry)declining_chain}) {
                std::vector<llm_session *> ss = make_sessions(m, B, V);
                std::vector<int32_t> want((size_t)B), ids((size_t)n * B + 1, -7);
                std::vector<uint64_t> rngs((size_t)B + 1), first((size_t)B);
                for (int c = 0; c < B; c++) {
                    rngs[(size_t)c] = first[(size_t)c] = 0x9E3779B97F4A7C15ull * (uint64_t)(c + 1);
                    const std::vector<int32_t> hist = prompt_of(c, V);
                    want[(size_t)c] = llm_sample_exact(llm_session_last_logits(ss[(size_t)c]), V, hist.data(), (int)hist.size(), &DEFAULT, &first[(size_t)c]);
                    CHECK(want[(size_t)c] >= 0);
                }
                rngs[(size_t)B] = 99;
                const int calls0 = g_chain_calls;
                CHECK(llm_infer_tokens_sampled_batch_via(nullptr, chain, m, ss.data(), B, n, &DEFAULT, rngs.data(), ids.data()) == 0);
                CHECK(g_chain_calls - calls0 == (chain && B >= 2 ? 1 : 0));
                if (chain && B >= 2)
                    for (int c = 0; c < B; c++) {  // the window handed to the entry: the history's last 63 tokens and row 0's id
                        const std::vector<int32_t> hist = prompt_of(c, V);
                        const int keep = (int)hist.size() < 63 ? (int)hist.size() : 63;
                        CHECK(g_window_n[(size_t)c] == keep + 1);
                        CHECK(g_windows[(size_t)c * 64 + (size_t)keep] == want[(size_t)c]);
                        for (int j = 0; j < keep; j++) CHECK(g_windows[(size_t)c * 64 + (size_t)j] == hist[hist.size() - (size_t)keep + (size_t)j]);
                    }
                CHECK(ids[(size_t)n * B] == -7 && rngs[(size_t)B] == 99);  // nothing behind [n][B] / [B]
                for (int c = 0; c < B; c++) {
                    CHECK(ids[(size_t)c] == want[(size_t)c]);
                    if (n == 1) CHECK(rngs[(size_t)c] == first[(size_t)c]);
                    CHECK(llm_session_n_past(ss[(size_t)c]) == (int)prompt_of(c, V).size() + n);
                    for (int k = 0; k < n; k++) CHECK(ids[(size_t)k * B + c] >= 0 && ids[(size_t)k * B + c] < V);
                }
                for (llm_session *s : ss) llm_session_free(s);
            }
        }
    }
    // ---- -1: nothing evaluated, no session and no generator moved
    {
        std::vector<llm_session *> ss = make_sessions(m, 3, V);
        std::vector<int32_t> ids(8 * 64, -7);
        std::vector<uint64_t> rngs = {11, 22, 33};
        const int calls0 = g_chain_calls;
        llm_session *twice[3] = {ss[0], ss[1], ss[0]}, *hole[2] = {ss[0], nullptr};
        const llm_sampler_params k0 = {0, 0.95f, 0.8f, 1.3f}, kbig = {V + 1, 0.95f, 0.8f, 1.3f}, t0 = {40, 0.95f, 0.0f, 1.3f},
                                 p0 = {40, 0.0f, 0.8f, 1.3f}, pen0 = {40, 0.95f, 0.8f, -1.0f};
        for (llm_batch_sample_entry chain : {(llm_batch_sample_entry) nullptr, (llm_batch_sample_entry)declining_chain}) {
            for (const llm_sampler_params *p : {&k0, &kbig, &t0, &p0, &pen0, (const llm_sampler_params *)nullptr}) {
                CHECK(llm_infer_tokens_sampled_batch_via(nullptr, chain, m, ss.data(), 3, 2, p, rngs.data(), ids.data()) == -1);
                CHECK(llm_infer_next_tokens_sampled_batch_via(nullptr, m, ss.data(), 3, p, rngs.data(), ids.data()) == -1);
            }
            CHECK(llm_infer_tokens_sampled_batch_via(nullptr, chain, nullptr, ss.data(), 3, 2, &DEFAULT, rngs.data(), ids.data()) == -1);
            CHECK(llm_infer_tokens_sampled_batch_via(nullptr, chain, m, nullptr, 3, 2, &DEFAULT, rngs.data(), ids.data()) == -1);
            CHECK(llm_infer_tokens_sampled_batch_via(nullptr, chain, m, ss.data(), 3, 2, &DEFAULT, nullptr, ids.data()) == -1);
            CHECK(llm_infer_tokens_sampled_batch_via(nullptr, chain, m, ss.data(), 3, 2, &DEFAULT, rngs.data(), nullptr) == -1);
            CHECK(llm_infer_tokens_sampled_batch_via(nullptr, chain, m, ss.data(), 0, 2, &DEFAULT, rngs.data(), ids.data()) == -1);
            CHECK(llm_infer_tokens_sampled_batch_via(nullptr, chain, m, ss.data(), 3, 0, &DEFAULT, rngs.data(), ids.data()) == -1);
            CHECK(llm_infer_tokens_sampled_batch_via(nullptr, chain, m, ss.data(), 3, -4, &DEFAULT, rngs.data(), ids.data()) == -1);
            CHECK(llm_infer_tokens_sampled_batch_via(nullptr, chain, m, twice, 3, 2, &DEFAULT, rngs.data(), ids.data()) == -1);
            CHECK(llm_infer_tokens_sampled_batch_via(nullptr, chain, m, hole, 2, 2, &DEFAULT, rngs.data(), ids.data()) == -1);
            // session 1 stands at 70: 58 tokens fit the context of 128, 59 do not
            CHECK(llm_infer_tokens_sampled_batch_via(nullptr, chain, m, ss.data(), 3, C - 70 + 1, &DEFAULT, rngs.data(), ids.data()) == -1);
        }
        CHECK(g_chain_calls == calls0);
        for (int32_t v : ids) CHECK(v == -7);
        CHECK(rngs[0] == 11 && rngs[1] == 22 && rngs[2] == 33);
        for (int c = 0; c < 3; c++) CHECK(llm_session_n_past(ss[(size_t)c]) == (int)prompt_of(c, V).size());
        // ... and to the context's last position
        CHECK(llm_infer_tokens_sampled_batch_via(nullptr, declining_chain, m, ss.data(), 3, C - 70, &DEFAULT, rngs.data(), ids.data()) == 0);
        CHECK(llm_session_n_past(ss[1]) == C && rngs[0] != 11);
        CHECK(llm_infer_tokens_sampled_batch_via(nullptr, declining_chain, m, ss.data(), 3, 1, &DEFAULT, rngs.data(), ids.data()) == -1);
        for (llm_session *s : ss) llm_session_free(s);
    }
    llm_model_free(m);
    printf("sampler driver OK\n");
    return 0;
}
