// pool_driver.cpp — the workload of the sanitizer job for llm_infer_until_pool_via (tests/test_sanitize_pool.py): the host mirror and
// ggml_core.cpp under ASan + UBSan, linked against tests/sanitize/stub_backend.cpp, which has no pool entry.  What runs here is the
// host's own part: the argument checks (-1, nothing moved, generator states untouched), the staging of the pool's graphs, the stepped
// loop under the admission rule — without an entry and with one that declines — and the commit behind an entry that accepts without
// computing anything: one that runs every request to its end, and one that stops short of n_steps, so that the mirror calls again for
// what is unfinished or unstarted and a lone remainder goes through llm_infer_until_via.  The accepting entries place their requests
// with llm_pool_schedule and fill the ids with values that name their step and column.  Checked per session: the count, the reason,
// the position, and the token history against its row of the ids.
// usage: pool_driver <model.ggjt>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "ggml_hip.h"
#include "host/llm_host.h"

#define CHECK(c)                                                                   \
    do {                                                                           \
        if (!(c)) {                                                                \
            fprintf(stderr, "pool driver: CHECK failed at line %d: %s\n", __LINE__, #c); \
            exit(2);                                                               \
        }                                                                          \
    } while (0)

static int g_V = 0, g_calls = 0, g_short = 0;  // g_short > 0: the entry runs at most that many steps of the n_steps it is asked for
static int32_t pool_id(int step, int column) { return (int32_t)((step * 31 + column * 7 + 3) % (g_V - 1)); }  // (never V - 1: a stop id below)

static int declining_pool(struct ggml_cgraph *const *graphs, int n_pool, int n_cols, int n_steps, const ggml_hip_sampler_chain *const *,
                          const ggml_hip_chain_end *ends, const int32_t *, const int32_t *, uint64_t *, float *, int32_t *, int32_t *, int32_t *,
                          int32_t *, int32_t *, int32_t *) {
    CHECK(graphs && ends && n_cols >= 2 && n_cols <= 8 && n_pool >= n_cols && n_pool <= 64 && n_steps >= 1);
    for (int i = 0; i < n_pool; i++) CHECK(graphs[i] && graphs[i]->n_nodes > 0 && ends[i].budget >= 1 && ends[i].budget <= n_steps);
    g_calls++;
    return -1;  // nothing executed
}
static int accepting_pool(struct ggml_cgraph *const *graphs, int n_pool, int n_cols, int n_steps, const ggml_hip_sampler_chain *const *chains,
                          const ggml_hip_chain_end *ends, const int32_t *windows, const int32_t *window_n, uint64_t *rng, float *, int32_t *out_ids,
                          int32_t *col, int32_t *first_step, int32_t *n_evaluated, int32_t *ended_by, int32_t *steps_run) {
    CHECK(graphs && chains && ends && col && first_step && n_evaluated && ended_by && steps_run && (n_steps == 1 || out_ids));
    CHECK(n_cols >= 2 && n_cols <= 8 && n_pool >= n_cols && n_pool <= 64 && n_steps >= 1);
    std::vector<int32_t> evals((size_t)n_pool);
    for (int i = 0; i < n_pool; i++) {
        CHECK(graphs[i] && graphs[i]->n_nodes > 0 && ends[i].budget >= 1 && ends[i].budget <= n_steps);
        if (chains[i]) CHECK(windows && window_n && rng && window_n[i] >= 1 && window_n[i] <= 64);
        evals[(size_t)i] = ends[i].budget;
    }
    CHECK(llm_pool_schedule(evals.data(), n_pool, n_cols, col, first_step) <= n_steps);
    const int run = g_short > 0 ? std::min(n_steps, g_short) : n_steps;
    for (int k = 0; k < (n_steps - 1) * n_cols; k++) out_ids[k] = -1;
    *steps_run = 0;
    for (int i = 0; i < n_pool; i++) {
        if (first_step[i] >= run) {  // it never left the queue
            col[i] = -1;
            first_step[i] = n_evaluated[i] = ended_by[i] = 0;
            continue;
        }
        const int e = std::min((int)evals[(size_t)i], run - first_step[i]);
        n_evaluated[i] = e;
        ended_by[i] = e == evals[(size_t)i] ? GGML_HIP_CHAIN_END_BUDGET : 0;
        for (int k = 1; k < e; k++) out_ids[(size_t)(first_step[i] + k - 1) * n_cols + col[i]] = pool_id(first_step[i] + k, col[i]);
        *steps_run = std::max(*steps_run, first_step[i] + e);
    }
    g_calls++;
    return 0;
}

// the last n tokens of the session's history are ids[0 .. n) (the snapshot holds the history in front of V logits and the K/V bytes)
static void check_history_tail(llm_session *s, size_t size0, const int32_t *ids, int n, int V) {
    const size_t sn = llm_session_snapshot(s, nullptr, 0);
    CHECK(sn == size0 + 4 * (size_t)n);
    std::vector<unsigned char> snap(sn);
    CHECK(llm_session_snapshot(s, snap.data(), sn) == sn);
    const size_t at = sn - llm_session_kv(s, 0, 0, nullptr, 0) - llm_session_kv(s, 1, 0, nullptr, 0) - 4 * (size_t)V - 4 * (size_t)n;
    for (int k = 0; k < n; k++) {
        int32_t t;
        memcpy(&t, snap.data() + at + 4 * (size_t)k, 4);
        CHECK(t == ids[k] && t >= 0 && t < V);
    }
}

static const int N = 7, CTX = 64;
static int prompt_len(int i) { return i == 4 ? CTX - 3 : 2 + 3 * i; }  // session 4 has room for two draws only
static std::vector<llm_session *> make_sessions(llm_model *m, int V) {
    std::vector<llm_session *> ss;
    for (int i = 0; i < N; i++) {
        llm_session_config cfg = {GGML_TYPE_F16, GGML_TYPE_F16, 8, 4};
        llm_session *s = llm_start_session(m, &cfg);
        CHECK(s);
        std::vector<int32_t> toks((size_t)prompt_len(i));
        for (size_t k = 0; k < toks.size(); k++) toks[k] = (int32_t)((k * 37 + 5 * (size_t)i + 1) % (size_t)(V - 1));
        // (a chunk per call: the stand-in completes an enqueued chunk by reading its graph again at the next begin, which a long
        // prompt's recreated arena does not survive)
        for (size_t at = 0; at < toks.size(); at += 8) llm_feed_prompt(m, s, toks.data() + at, (int)std::min((size_t)8, toks.size() - at));
        ss.push_back(s);
    }
    return ss;
}

int main(int argc, char **argv) {
    CHECK(argc == 2);
    llm_model_params mp = {CTX, 1, -1, 0, 1.0f, 10000, 0, -1, 0};
    llm_model *m = llm_llama_load(argv[1], &mp);
    CHECK(m);
    const int V = g_V = llm_model_n_vocab(m);
    llm_sampler_chain dflt;
    memset(&dflt, 0, sizeof(dflt));
    dflt.base = {40, 0.95f, 0.8f, 1.3f};  // the default chain: neutral extras
    dflt.tail_free_z = dflt.typical_p = 1.0f;
    dflt.tau = 5.0f;
    dflt.eta = 0.1f;
    // (the sampled request is session 0 with two tokens: it starts in column 0 and ends inside every entry's first call, so it never
    // draws from the logits of a graph an accepting entry left uncomputed)
    const int max_tokens[N] = {2, 3, 1, 5, 8, 6, 4};
    struct Leg {
        llm_pool_requests_entry entry;
        int shortest, max_cols, want_rc;
    };
    const Leg legs[] = {{nullptr, 0, 3, 0},        {declining_pool, 0, 3, 0}, {accepting_pool, 0, 3, 1}, {accepting_pool, 2, 3, 1},
                        {accepting_pool, 3, 8, 1}, {accepting_pool, 0, 1, 0}, {nullptr, 0, 8, 0}};
    for (const Leg &leg : legs) {
        std::vector<llm_session *> ss = make_sessions(m, V);
        std::vector<llm_until_request> reqs((size_t)N);
        std::vector<uint64_t> rngs((size_t)N, 0x9E3779B97F4A7C15ull);
        std::vector<size_t> size0((size_t)N);
        for (int i = 0; i < N; i++) {
            memset(&reqs[(size_t)i], 0, sizeof(llm_until_request));
            reqs[(size_t)i].chain = i == 0 ? &dflt : nullptr;  // one sampled request: its generator state is committed with its draws
            reqs[(size_t)i].max_tokens = max_tokens[i];
            if (i == 3) {  // its first token is its stop id: born ended
                reqs[(size_t)i].n_stop = 2;
                reqs[(size_t)i].stop_id[0] = V - 1;
                reqs[(size_t)i].stop_id[1] = llm_argmax_first(llm_session_last_logits(ss[(size_t)i]), V, 0);
            }
            size0[(size_t)i] = llm_session_snapshot(ss[(size_t)i], nullptr, 0);
        }
        const int n = 8;
        std::vector<int32_t> ids((size_t)N * n + 1, -7), n_out((size_t)N, -7), why((size_t)N, -7);
        g_short = leg.shortest;
        const int calls0 = g_calls;
        CHECK(llm_infer_until_pool_via(nullptr, nullptr, leg.entry, m, ss.data(), N, reqs.data(), rngs.data(), nullptr, leg.max_cols, ids.data(),
                                       n_out.data(), why.data()) == leg.want_rc);
        if (leg.entry == declining_pool) CHECK(g_calls - calls0 == 1);
        if (leg.entry == accepting_pool && leg.max_cols > 1) CHECK(g_calls - calls0 >= (leg.shortest ? 2 : 1));
        if (leg.max_cols == 1) CHECK(g_calls == calls0);  // one column: every session through the one-session form
        CHECK(ids[(size_t)N * n] == -7);
        for (int i = 0; i < N; i++) {
            const int want_n = i == 3 ? 1 : (i == 4 ? 2 : max_tokens[i]);
            const int want_why = i == 3 ? LLM_ENDED_BY_STOP : (i == 4 ? LLM_ENDED_BY_CONTEXT : LLM_ENDED_BY_BUDGET);
            CHECK(n_out[(size_t)i] == want_n && why[(size_t)i] == want_why);
            CHECK(llm_session_n_past(ss[(size_t)i]) == prompt_len(i) + want_n);
            check_history_tail(ss[(size_t)i], size0[(size_t)i], ids.data() + (size_t)i * n, want_n, V);
            for (int k = want_n; k < n; k++) CHECK(ids[(size_t)i * n + k] == -1);
            CHECK((rngs[(size_t)i] == 0x9E3779B97F4A7C15ull) == (i != 0));  // only the sampled request's state moved
        }
        for (llm_session *s : ss) llm_session_free(s);
    }
    g_short = 0;
    // ---- -1: nothing evaluated, no session moved, no state moved
    {
        std::vector<llm_session *> ss = make_sessions(m, V);
        std::vector<llm_until_request> reqs((size_t)N);
        for (int i = 0; i < N; i++) {
            memset(&reqs[(size_t)i], 0, sizeof(llm_until_request));
            reqs[(size_t)i].chain = &dflt;
            reqs[(size_t)i].max_tokens = 4;
        }
        std::vector<uint64_t> rngs((size_t)N, 77);
        std::vector<int32_t> ids((size_t)N * 8, -7), n_out((size_t)N, -7), why((size_t)N, -7);
        llm_session *twice[3] = {ss[0], ss[1], ss[0]};
        const int calls0 = g_calls;
        for (llm_pool_requests_entry entry : {(llm_pool_requests_entry) nullptr, (llm_pool_requests_entry)accepting_pool}) {
            const auto call = [&](llm_model *mm, llm_session *const *s, int cnt, const llm_until_request *q, uint64_t *r, int cols, int32_t *o) {
                return llm_infer_until_pool_via(nullptr, nullptr, entry, mm, s, cnt, q, r, nullptr, cols, o, n_out.data(), why.data());
            };
            CHECK(call(nullptr, ss.data(), N, reqs.data(), rngs.data(), 3, ids.data()) == -1);
            CHECK(call(m, nullptr, N, reqs.data(), rngs.data(), 3, ids.data()) == -1);
            CHECK(call(m, ss.data(), 0, reqs.data(), rngs.data(), 3, ids.data()) == -1);
            CHECK(call(m, ss.data(), N, nullptr, rngs.data(), 3, ids.data()) == -1);
            CHECK(call(m, ss.data(), N, reqs.data(), nullptr, 3, ids.data()) == -1);  // sampled requests need generator states
            CHECK(call(m, ss.data(), N, reqs.data(), rngs.data(), 0, ids.data()) == -1);
            CHECK(call(m, ss.data(), N, reqs.data(), rngs.data(), 9, ids.data()) == -1);
            CHECK(call(m, ss.data(), N, reqs.data(), rngs.data(), 3, nullptr) == -1);
            CHECK(call(m, twice, 3, reqs.data(), rngs.data(), 3, ids.data()) == -1);
            std::vector<llm_until_request> bad = reqs;
            bad[6].max_tokens = 0;
            CHECK(call(m, ss.data(), N, bad.data(), rngs.data(), 3, ids.data()) == -1);
            bad = reqs;
            bad[6].n_stop = 1;
            bad[6].stop_id[0] = V;
            CHECK(call(m, ss.data(), N, bad.data(), rngs.data(), 3, ids.data()) == -1);
        }
        CHECK(g_calls == calls0);
        for (int32_t v : ids) CHECK(v == -7);
        for (uint64_t r : rngs) CHECK(r == 77);
        for (int i = 0; i < N; i++) CHECK(llm_session_n_past(ss[(size_t)i]) == prompt_len(i));
        for (llm_session *s : ss) llm_session_free(s);
    }
    // ---- the rule alone, at the edges of its arguments
    {
        const int32_t evals[4] = {3, 1, 2, 2};
        int32_t col[4], first[4];
        CHECK(llm_pool_schedule(evals, 4, 2, col, first) == 5 && col[2] == 1 && first[2] == 1 && col[3] == 0 && first[3] == 3);
        CHECK(llm_pool_schedule(evals, 4, 4, nullptr, nullptr) == 3 && llm_pool_schedule(evals, 4, 5, nullptr, nullptr) == -1);
        CHECK(llm_pool_schedule(nullptr, 4, 2, nullptr, nullptr) == -1 && llm_pool_schedule(evals, 4, 0, nullptr, nullptr) == -1);
    }
    llm_model_free(m);
    printf("pool driver OK\n");
    return 0;
}
