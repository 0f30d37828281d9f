// sampler_driver.cpp — the workload of the sanitizer job for the sampled batched chain's host side (tests/test_sanitize_sampler.py):
// the host mirror and ggml_core.cpp under ASan + UBSan, linked against tests/sanitize/stub_backend.cpp, which has neither a batched
// step nor a sampled chain.  What runs here: llm_sample_exact on edge rows (one entry, k = V, all equal, all -inf, zeros of both signs,
// a window longer than 64 tokens, bad arguments), and llm_infer_tokens_sampled_batch_via / llm_infer_next_tokens_sampled_batch_via
// with NULL entries and with a chain entry that declines: the argument checks (-1, no session and no generator moved), the staging
// of B graphs and windows for the entry, and the fall-back loop's indexing of out_ids [n][B] — one session with a prompt of 70
// tokens, so that its window is cut to 64.  Row 0 of every call is checked against llm_sample_exact on the session's own logits.
// Last, the commit after a chain entry that accepts without computing anything: ids, positions, histories, generator states.
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

// a chain entry that accepts: it computes nothing and answers 0 with rows 1 .. n - 1 filled with ids that name their place and
// every generator moved on by a known amount, so that the host's commit can be checked on the CPU.  At n = 1 it writes no id.
static int g_V = 0;
static int32_t chain_id(int step, int column) { return (int32_t)((step * 31 + column * 7 + 3) % g_V); }
static uint64_t chain_rng_step(int column) { return 0x100u + (uint64_t)column; }
static int accepting_chain(struct ggml_cgraph *const *graphs, int n_graphs, int n_steps, const ggml_hip_sampler *params,
                           const int32_t *windows, const int32_t *window_n, uint64_t *rng, int32_t *out_ids) {
    CHECK(graphs && params && windows && window_n && rng && out_ids && n_steps >= 1);
    for (int i = 0; i < n_graphs; i++) CHECK(graphs[i] && graphs[i]->n_nodes > 0);
    g_windows.assign(windows, windows + (size_t)n_graphs * 64);
    g_window_n.assign(window_n, window_n + n_graphs);
    for (int k = 1; k < n_steps; k++)
        for (int c = 0; c < n_graphs; c++) out_ids[(size_t)(k - 1) * n_graphs + c] = chain_id(k, c);
    for (int c = 0; c < n_graphs; c++) rng[c] += chain_rng_step(c);
    g_chain_calls++;
    return 0;
}

// the last n tokens of the session's history are column c of ids [n][B] (the snapshot holds the history in front of V logits and the
// K/V bytes; size0 = the snapshot's size before the n tokens)
static void check_history_tail(llm_session *s, size_t size0, const int32_t *ids, int B, int c, int n, int V) {
    const size_t sn = llm_session_snapshot(s, nullptr, 0);
    CHECK(sn == size0 + 4 * (size_t)n);
    std::vector<unsigned char> snap(sn);
    CHECK(llm_session_snapshot(s, snap.data(), sn) == sn);
    const size_t at = sn - llm_session_kv(s, 0, 0, nullptr, 0) - llm_session_kv(s, 1, 0, nullptr, 0) - 4 * (size_t)V - 4 * (size_t)n;
    for (int k = 0; k < n; k++) {
        int32_t t;
        memcpy(&t, snap.data() + at + 4 * (size_t)k, 4);
        CHECK(t == ids[(size_t)k * B + c] && t >= 0 && t < V);
    }
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

// the windows handed to the chain entry last: each session's last 63 tokens of history and row 0's id
static void check_windows(int B, int V, const std::vector<int32_t> &want) {
    for (int c = 0; c < B; c++) {
        const std::vector<int32_t> hist = prompt_of(c, V);
        const int keep = (int)hist.size() < 63 ? (int)hist.size() : 63;
        CHECK(g_window_n[(size_t)c] == keep + 1);
        CHECK(g_windows[(size_t)c * 64 + (size_t)keep] == want[(size_t)c]);
        for (int j = 0; j < keep; j++) CHECK(g_windows[(size_t)c * 64 + (size_t)j] == hist[hist.size() - (size_t)keep + (size_t)j]);
    }
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
                if (chain && B >= 2) check_windows(B, V, want);
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
    // ---- a chain entry that accepts: 1, out_ids = row 0 as the stepped form draws it and then the entry's rows, every session moved
    // by n with its column at the end of its history (session 1's was longer than the window before), every generator where the
    // entry left it.  out_ids and rngs hold exactly [n][B] and [B]: at n = 1 nothing behind row 0 exists.
    g_V = V;
    for (int B : {2, 3}) {
        for (int n : {1, 2, 5}) {
            std::vector<llm_session *> ss = make_sessions(m, B, V);
            std::vector<int32_t> want((size_t)B), ids((size_t)n * B, -7);
            std::vector<uint64_t> rngs((size_t)B), first((size_t)B);
            std::vector<size_t> size0((size_t)B);
            for (int c = 0; c < B; c++) {
                rngs[(size_t)c] = first[(size_t)c] = 0x9E3779B97F4A7C15ull * (uint64_t)(c + 1);
                const std::vector<int32_t> hist = prompt_of(c, V);
                want[(size_t)c] = llm_sample_exact(llm_session_last_logits(ss[(size_t)c]), V, hist.data(), (int)hist.size(), &DEFAULT, &first[(size_t)c]);
                CHECK(want[(size_t)c] >= 0);
                size0[(size_t)c] = llm_session_snapshot(ss[(size_t)c], nullptr, 0);
            }
            const int calls0 = g_chain_calls;
            CHECK(llm_infer_tokens_sampled_batch_via(nullptr, accepting_chain, m, ss.data(), B, n, &DEFAULT, rngs.data(), ids.data()) == 1);
            CHECK(g_chain_calls - calls0 == 1);
            check_windows(B, V, want);
            for (int c = 0; c < B; c++) {
                CHECK(ids[(size_t)c] == want[(size_t)c]);
                for (int k = 1; k < n; k++) CHECK(ids[(size_t)k * B + c] == chain_id(k, c));
                CHECK(rngs[(size_t)c] == first[(size_t)c] + chain_rng_step(c));
                CHECK(llm_session_n_past(ss[(size_t)c]) == (int)prompt_of(c, V).size() + n);
                check_history_tail(ss[(size_t)c], size0[(size_t)c], ids.data(), B, c, n, V);
            }
            for (llm_session *s : ss) llm_session_free(s);
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
