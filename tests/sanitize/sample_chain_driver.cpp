// sample_chain_driver.cpp — the workload of the sanitizer job for the host side of ONE session's sampled chain
// (tests/test_sanitize_sample_chain.py): the host mirror and ggml_core.cpp under ASan + UBSan, linked against
// tests/sanitize/stub_backend.cpp, which has no ggml_hip_decode_sampled_chain — the entry is a parameter of
// llm_infer_tokens_sampled_via.  What runs here: llm_infer_next_token_sampled and llm_infer_tokens_sampled_via with a NULL entry, an
// entry that declines (and scribbles over what it was given) and an entry that accepts and fills ids, generator state and logits
// without computing anything; sessions whose history is longer and shorter than the 64-token window; n = 1, 2 and 5 with `out` of
// the exact size; bad arguments (-1, nothing moved, the entry not called).
// usage: sample_chain_driver <model.ggjt>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ggml_hip.h"
#include "host/llm_host.h"

#define CHECK(c)                                                                           \
    do {                                                                                   \
        if (!(c)) {                                                                        \
            fprintf(stderr, "sample chain driver: CHECK failed at line %d: %s\n", __LINE__, #c); \
            exit(2);                                                                       \
        }                                                                                  \
    } while (0)

static const llm_sampler_params DEFAULT = {40, 0.95f, 0.8f, 1.30f};
static const uint64_t SEED = 0x9E3779B97F4A7C15ull;

static int g_V = 0, g_calls = 0, g_last_n = 0;
static std::vector<int32_t> g_window;
static void note_call(struct ggml_cgraph *last, int n, const ggml_hip_sampler *params, const int32_t *window, int window_n, uint64_t *rng,
                      int32_t *out_tokens, float *last_logits) {
    CHECK(last && last->n_nodes > 0 && n >= 1 && params && rng && out_tokens && last_logits && window_n >= 0 && window_n <= 64);
    CHECK(window || window_n == 0);
    g_window.assign(window, window + window_n);  // (reads all of it)
    for (int32_t t : g_window) CHECK(t >= 0 && t < g_V);
    g_last_n = n;
    g_calls++;
}
static int declining_chain(struct ggml_cgraph *last, int n, const ggml_hip_sampler *params, const int32_t *window, int window_n,
                           uint64_t *rng, int32_t *out_tokens, float *last_logits) {
    note_call(last, n, params, window, window_n, rng, out_tokens, last_logits);
    for (int i = 0; i < n; i++) out_tokens[i] = -9;  // (writes all of [n]; a declining entry's scribbles must not reach the caller)
    *rng ^= 0x5555;
    return -1;  // nothing executed (the logits stay as they are: the stepped token draws from them)
}
// accepts: ids that name their place, the generator moved on by a known amount, logits that say which call wrote them
static int32_t chain_id(int i) { return (int32_t)((i * 31 + 3) % g_V); }
static int accepting_chain(struct ggml_cgraph *last, int n, const ggml_hip_sampler *params, const int32_t *window, int window_n,
                           uint64_t *rng, int32_t *out_tokens, float *last_logits) {
    note_call(last, n, params, window, window_n, rng, out_tokens, last_logits);
    for (int i = 0; i < n; i++) out_tokens[i] = chain_id(i);
    *rng += 0x100;
    for (int i = 0; i < g_V; i++) last_logits[i] = 0.5f * (float)n + (float)i;  // (writes all of [V])
    return 0;
}

static std::vector<int32_t> prompt_of(int len) {
    std::vector<int32_t> toks((size_t)len);
    for (size_t i = 0; i < toks.size(); i++) toks[i] = (int32_t)((i * 37 + 1) % (size_t)g_V);
    return toks;
}
static llm_session *make_session(llm_model *m, int len) {
    llm_session_config cfg = {GGML_TYPE_F16, GGML_TYPE_F16, 8, 4};
    llm_session *s = llm_start_session(m, &cfg);
    CHECK(s);
    const std::vector<int32_t> toks = prompt_of(len);
    llm_feed_prompt(m, s, toks.data(), (int)toks.size());
    return s;
}
static std::vector<unsigned char> snapshot(llm_session *s) {
    std::vector<unsigned char> snap(llm_session_snapshot(s, nullptr, 0));
    CHECK(llm_session_snapshot(s, snap.data(), snap.size()) == snap.size());
    return snap;
}
// the last n tokens of the session's history (the snapshot holds the history in front of V logits and the K/V bytes)
static std::vector<int32_t> history_tail(llm_session *s, int n) {
    const std::vector<unsigned char> snap = snapshot(s);
    const size_t at = snap.size() - llm_session_kv(s, 0, 0, nullptr, 0) - llm_session_kv(s, 1, 0, nullptr, 0) - 4 * (size_t)g_V - 4 * (size_t)n;
    std::vector<int32_t> t((size_t)n);
    memcpy(t.data(), snap.data() + at, 4 * (size_t)n);
    return t;
}

int main(int argc, char **argv) {
    CHECK(argc == 2);
    const int C = 128;
    llm_model_params mp = {C, 1, -1, 0, 1.0f, 10000, 0, -1, 0};
    llm_model *m = llm_llama_load(argv[1], &mp);
    CHECK(m);
    const int V = g_V = llm_model_n_vocab(m);
    // ---- a NULL entry and one that declines: the stepped loop
    for (int len : {70, 5}) {  // a history longer than the window, and a shorter one
        for (int n : {1, 2, 5}) {
            for (llm_sample_chain_entry entry : {(llm_sample_chain_entry) nullptr, (llm_sample_chain_entry)declining_chain}) {
                // (the stand-in computes nothing: logits behind an evaluation are nobody's, so only the first token has a yardstick —
                // llm_sample_exact on the session's own logits and history)
                llm_session *s = make_session(m, len);
                const std::vector<int32_t> hist = prompt_of(len);
                std::vector<int32_t> out((size_t)n, -7);
                uint64_t rng = SEED, first = SEED;
                const int32_t want = llm_sample_exact(llm_session_last_logits(s), V, hist.data(), (int)hist.size(), &DEFAULT, &first);
                CHECK(want >= 0);
                const int calls0 = g_calls;
                CHECK(llm_infer_tokens_sampled_via(entry, m, s, n, &DEFAULT, &rng, out.data()) == 0);
                CHECK(g_calls - calls0 == (entry ? (n > 1 ? 2 : 1) : 0));  // behind the prompt, then behind the stepped token
                if (entry && n > 1) {  // the second call's window: the last 64 of the history with the stepped token at its end
                    CHECK(g_last_n == n - 1 && (int)g_window.size() == (len + 1 < 64 ? len + 1 : 64) && g_window.back() == out[0]);
                }
                CHECK(out[0] == want && rng != SEED && (n > 1 || rng == first));
                for (int32_t t : out) CHECK(t >= 0 && t < V);
                CHECK(llm_session_n_past(s) == len + n && history_tail(s, n) == out);
                llm_session_free(s);
            }
        }
    }
    // ---- an entry that accepts: its ids, its generator state, its logits; the history and n_past moved by n
    for (int len : {70, 5}) {
        for (int n : {1, 2, 5}) {
            llm_session *s = make_session(m, len);
            const std::vector<int32_t> hist = prompt_of(len);
            std::vector<int32_t> out((size_t)n, -7);
            uint64_t rng = SEED;
            const int calls0 = g_calls;
            CHECK(llm_infer_tokens_sampled_via(accepting_chain, m, s, n, &DEFAULT, &rng, out.data()) == n);
            CHECK(g_calls - calls0 == 1 && g_last_n == n);
            const int w = len < 64 ? len : 64;
            CHECK((int)g_window.size() == w);
            for (int j = 0; j < w; j++) CHECK(g_window[(size_t)j] == hist[hist.size() - (size_t)w + (size_t)j]);
            for (int i = 0; i < n; i++) CHECK(out[(size_t)i] == chain_id(i));
            CHECK(rng == SEED + 0x100);
            CHECK(llm_session_n_past(s) == len + n && history_tail(s, n) == out);
            const float *l = llm_session_last_logits(s);
            CHECK(l[0] == 0.5f * (float)n && l[V - 1] == 0.5f * (float)n + (float)(V - 1));
            // behind a chain the session goes on: a stepped token, then a chain the entry takes in its first attempt again
            CHECK(llm_infer_next_token_sampled(m, s, &DEFAULT, &rng) >= 0);
            std::vector<int32_t> two(2, -7);
            CHECK(llm_infer_tokens_sampled_via(accepting_chain, m, s, 2, &DEFAULT, &rng, two.data()) == 2 && g_calls - calls0 == 2);
            CHECK(llm_session_n_past(s) == len + n + 3);
            llm_session_free(s);
        }
    }
    // ---- -1: nothing moved, the entry not called
    {
        llm_session *s = make_session(m, 70);
        const std::vector<unsigned char> snap0 = snapshot(s);
        std::vector<int32_t> out(64, -7);
        uint64_t rng = 11;
        const int calls0 = g_calls;
        const llm_sampler_params k0 = {0, 0.95f, 0.8f, 1.3f}, kbig = {V + 1, 0.95f, 0.8f, 1.3f}, t0 = {40, 0.95f, 0.0f, 1.3f},
                                 p0 = {40, 0.0f, 0.8f, 1.3f}, pen0 = {40, 0.95f, 0.8f, -1.0f};
        for (llm_sample_chain_entry entry : {(llm_sample_chain_entry) nullptr, (llm_sample_chain_entry)declining_chain, (llm_sample_chain_entry)accepting_chain}) {
            for (const llm_sampler_params *p : {&k0, &kbig, &t0, &p0, &pen0, (const llm_sampler_params *)nullptr}) {
                CHECK(llm_infer_tokens_sampled_via(entry, m, s, 2, p, &rng, out.data()) == -1);
                CHECK(llm_infer_next_token_sampled(m, s, p, &rng) == -1);
            }
            CHECK(llm_infer_tokens_sampled_via(entry, nullptr, s, 2, &DEFAULT, &rng, out.data()) == -1);
            CHECK(llm_infer_tokens_sampled_via(entry, m, nullptr, 2, &DEFAULT, &rng, out.data()) == -1);
            CHECK(llm_infer_tokens_sampled_via(entry, m, s, 2, &DEFAULT, nullptr, out.data()) == -1);
            CHECK(llm_infer_tokens_sampled_via(entry, m, s, 2, &DEFAULT, &rng, nullptr) == -1);
            CHECK(llm_infer_tokens_sampled_via(entry, m, s, 0, &DEFAULT, &rng, out.data()) == -1);
            CHECK(llm_infer_tokens_sampled_via(entry, m, s, -4, &DEFAULT, &rng, out.data()) == -1);
            // the session stands at 70: the stepped loop takes 57 tokens in a context of 128 and refuses the 58th
            CHECK(llm_infer_tokens_sampled_via(entry, m, s, C - 70, &DEFAULT, &rng, out.data()) == -1);
        }
        CHECK(llm_infer_next_token_sampled(nullptr, s, &DEFAULT, &rng) == -1);
        CHECK(llm_infer_next_token_sampled(m, nullptr, &DEFAULT, &rng) == -1);
        CHECK(llm_infer_next_token_sampled(m, s, &DEFAULT, nullptr) == -1);
        CHECK(g_calls == calls0 && rng == 11 && llm_session_n_past(s) == 70 && snapshot(s) == snap0);
        for (int32_t v : out) CHECK(v == -7);
        // ... and as far as the stepped loop goes
        out.assign((size_t)(C - 70 - 1), -7);
        CHECK(llm_infer_tokens_sampled_via(declining_chain, m, s, C - 70 - 1, &DEFAULT, &rng, out.data()) == 0);
        CHECK(llm_session_n_past(s) == C - 1 && rng != 11);
        CHECK(llm_infer_tokens_sampled_via(declining_chain, m, s, 1, &DEFAULT, &rng, out.data()) == -1);
        llm_session_free(s);
    }
    llm_model_free(m);
    printf("sample chain driver OK\n");
    return 0;
}
