// batch_chain_driver.cpp — the workload of the sanitizer job for llm_infer_tokens_greedy_batch_via (tests/test_sanitize_batch_chain.py):
// the host mirror and ggml_core.cpp under ASan + UBSan, linked against tests/sanitize/stub_backend.cpp, which has neither a batched
// step nor a chain.  What runs here is therefore the host's own part: the argument checks (-1, no session moved), the staging of B
// graphs for an entry that answers -1, and the fall-back loop with its indexing of out_ids [n][B] — with a NULL chain entry and with
// one that declines — and the commit after an entry that accepts without computing anything.  (The stand-in's logits depend on how many graphs it has seen, so two sets of sessions never agree: the checks are
// each call's own — row 0, the sessions' positions, their token histories.)
// usage: batch_chain_driver <model.ggjt>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ggml_hip.h"
#include "host/llm_host.h"

#define CHECK(c)                                                                          \
    do {                                                                                  \
        if (!(c)) {                                                                       \
            fprintf(stderr, "batch chain driver: CHECK failed at line %d: %s\n", __LINE__, #c); \
            exit(2);                                                                      \
        }                                                                                 \
    } while (0)

static int g_chain_calls = 0, g_chain_B = 0, g_chain_n = 0;
static int declining_chain(struct ggml_cgraph *const *graphs, int n_graphs, int n_steps, int32_t *out_ids) {
    CHECK(graphs && out_ids);
    for (int i = 0; i < n_graphs; i++) CHECK(graphs[i] && graphs[i]->n_nodes > 0);
    g_chain_calls++;
    g_chain_B = n_graphs;
    g_chain_n = n_steps;
    return -1;  // nothing executed
}

// a chain entry that accepts: it computes nothing and answers 0 with rows 1 .. n - 1 filled with ids that name their place, so that
// the host's commit (ids out, positions, token histories) can be checked on the CPU.  At n = 1 it writes nothing.
static int g_V = 0;
static int32_t chain_id(int step, int column) { return (int32_t)((step * 31 + column * 7 + 3) % g_V); }
static int accepting_chain(struct ggml_cgraph *const *graphs, int n_graphs, int n_steps, int32_t *out_ids) {
    CHECK(graphs && out_ids && n_steps >= 1);
    for (int i = 0; i < n_graphs; i++) CHECK(graphs[i] && graphs[i]->n_nodes > 0);
    for (int k = 1; k < n_steps; k++)
        for (int c = 0; c < n_graphs; c++) out_ids[(size_t)(k - 1) * n_graphs + c] = chain_id(k, c);
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

static std::vector<llm_session *> make_sessions(llm_model *m, int B, int V) {
    std::vector<llm_session *> ss;
    for (int c = 0; c < B; c++) {
        llm_session_config cfg = {GGML_TYPE_F16, GGML_TYPE_F16, 8, 4};
        llm_session *s = llm_start_session(m, &cfg);
        CHECK(s);
        std::vector<int32_t> toks((size_t)(2 + 3 * c));  // ragged prompts
        for (size_t i = 0; i < toks.size(); i++) toks[i] = (int32_t)((i * 37 + 5 * (size_t)c + 1) % (size_t)V);
        llm_feed_prompt(m, s, toks.data(), (int)toks.size());
        ss.push_back(s);
    }
    return ss;
}

int main(int argc, char **argv) {
    CHECK(argc == 2);
    const int C = 64;
    llm_model_params mp = {C, 1, -1, 0, 1.0f, 10000, 0, -1, 0};
    llm_model *m = llm_llama_load(argv[1], &mp), *other = llm_llama_load(argv[1], &mp);
    CHECK(m && other);
    const int V = llm_model_n_vocab(m);
    for (int B : {1, 2, 5, 8}) {
        for (int n : {1, 6}) {
            // the chained call's fall-back: without a chain entry, and with one that declines
            for (llm_batch_chain_entry chain : {(llm_batch_chain_entry) nullptr, (llm_batch_chain_entry)declining_chain}) {
                std::vector<llm_session *> ss = make_sessions(m, B, V);
                std::vector<int32_t> want((size_t)B), ids((size_t)n * B + 1, -7);
                std::vector<size_t> size0((size_t)B);
                for (int c = 0; c < B; c++) {
                    want[(size_t)c] = llm_argmax_first(llm_session_last_logits(ss[(size_t)c]), V, 0);
                    size0[(size_t)c] = llm_session_snapshot(ss[(size_t)c], nullptr, 0);
                }
                const int calls0 = g_chain_calls;
                CHECK(llm_infer_tokens_greedy_batch_via(nullptr, chain, m, ss.data(), B, n, ids.data()) == 0);
                CHECK(g_chain_calls - calls0 == (chain && B >= 2 ? 1 : 0));  // (one session: nothing to batch, the entry is not asked)
                if (chain && B >= 2) CHECK(g_chain_B == B && g_chain_n == n);
                CHECK(ids[(size_t)n * B] == -7);  // nothing behind [n][B]
                for (int c = 0; c < B; c++) {
                    llm_session *s = ss[(size_t)c];
                    CHECK(ids[(size_t)c] == want[(size_t)c]);  // row 0: the first maximum of the logits the session came with
                    CHECK(llm_session_n_past(s) == 2 + 3 * c + n);
                    check_history_tail(s, size0[(size_t)c], ids.data(), B, c, n, V);  // the history grew by this session's column of ids
                }
                for (llm_session *s : ss) llm_session_free(s);
            }
        }
    }
    // ---- a chain entry that accepts: 1, out_ids = row 0 as the stepped form draws it and then the entry's rows, every session
    // moved by n with its column at the end of its history.  out_ids holds exactly [n][B]: at n = 1 nothing behind row 0 exists.
    g_V = V;
    for (int B : {2, 3}) {
        for (int n : {1, 2, 5}) {
            std::vector<llm_session *> ss = make_sessions(m, B, V);
            std::vector<int32_t> want((size_t)B), ids((size_t)n * B, -7);
            std::vector<size_t> size0((size_t)B);
            for (int c = 0; c < B; c++) {
                want[(size_t)c] = llm_argmax_first(llm_session_last_logits(ss[(size_t)c]), V, 0);
                size0[(size_t)c] = llm_session_snapshot(ss[(size_t)c], nullptr, 0);
            }
            const int calls0 = g_chain_calls;
            CHECK(llm_infer_tokens_greedy_batch_via(nullptr, accepting_chain, m, ss.data(), B, n, ids.data()) == 1);
            CHECK(g_chain_calls - calls0 == 1);
            for (int c = 0; c < B; c++) {
                CHECK(ids[(size_t)c] == want[(size_t)c]);
                for (int k = 1; k < n; k++) CHECK(ids[(size_t)k * B + c] == chain_id(k, c));
                CHECK(llm_session_n_past(ss[(size_t)c]) == 2 + 3 * c + n);
                check_history_tail(ss[(size_t)c], size0[(size_t)c], ids.data(), B, c, n, V);
            }
            for (llm_session *s : ss) llm_session_free(s);
        }
    }
    // ---- -1: nothing evaluated, no session moved
    {
        std::vector<llm_session *> ss = make_sessions(m, 3, V);
        llm_session_config cfg = {GGML_TYPE_F16, GGML_TYPE_F16, 8, 4};
        llm_session *x = llm_start_session(other, &cfg);
        CHECK(x);
        const int32_t t3[3] = {1, 2, 3};
        llm_feed_prompt(other, x, t3, 3);
        std::vector<int32_t> ids(8 * 64, -7);
        const int calls0 = g_chain_calls;
        llm_session *twice[3] = {ss[0], ss[1], ss[0]}, *foreign[2] = {ss[0], x}, *hole[2] = {ss[0], nullptr};
        for (llm_batch_chain_entry chain : {(llm_batch_chain_entry) nullptr, (llm_batch_chain_entry)declining_chain}) {
            CHECK(llm_infer_tokens_greedy_batch_via(nullptr, chain, nullptr, ss.data(), 3, 2, ids.data()) == -1);
            CHECK(llm_infer_tokens_greedy_batch_via(nullptr, chain, m, nullptr, 3, 2, ids.data()) == -1);
            CHECK(llm_infer_tokens_greedy_batch_via(nullptr, chain, m, ss.data(), 3, 2, nullptr) == -1);
            CHECK(llm_infer_tokens_greedy_batch_via(nullptr, chain, m, ss.data(), 0, 2, ids.data()) == -1);
            CHECK(llm_infer_tokens_greedy_batch_via(nullptr, chain, m, ss.data(), 3, 0, ids.data()) == -1);
            CHECK(llm_infer_tokens_greedy_batch_via(nullptr, chain, m, ss.data(), 3, -4, ids.data()) == -1);
            CHECK(llm_infer_tokens_greedy_batch_via(nullptr, chain, m, twice, 3, 2, ids.data()) == -1);
            CHECK(llm_infer_tokens_greedy_batch_via(nullptr, chain, m, foreign, 2, 2, ids.data()) == -1);
            CHECK(llm_infer_tokens_greedy_batch_via(nullptr, chain, m, hole, 2, 2, ids.data()) == -1);
            // session 2 stands at 8: 56 tokens fit the context of 64, 57 do not
            CHECK(llm_infer_tokens_greedy_batch_via(nullptr, chain, m, ss.data(), 3, C - 8 + 1, ids.data()) == -1);
        }
        CHECK(g_chain_calls == calls0);
        for (int32_t v : ids) CHECK(v == -7);
        for (int c = 0; c < 3; c++) CHECK(llm_session_n_past(ss[(size_t)c]) == 2 + 3 * c);
        CHECK(llm_session_n_past(x) == 3);
        // ... and to the context's last position: the sessions end at 58, 61 and 64
        CHECK(llm_infer_tokens_greedy_batch_via(nullptr, declining_chain, m, ss.data(), 3, C - 8, ids.data()) == 0);
        CHECK(llm_session_n_past(ss[2]) == C && llm_session_n_past(ss[0]) == C - 6);
        CHECK(llm_infer_tokens_greedy_batch_via(nullptr, declining_chain, m, ss.data(), 3, 1, ids.data()) == -1);
        CHECK(llm_session_n_past(ss[2]) == C && llm_session_n_past(ss[0]) == C - 6);
        for (llm_session *s : ss) llm_session_free(s);
        llm_session_free(x);
    }
    llm_model_free(other);
    llm_model_free(m);
    printf("batch chain driver OK\n");
    return 0;
}
