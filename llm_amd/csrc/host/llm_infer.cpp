// llm_infer.cpp — the host mirror's token steps (inference_session.rs:381-424 infer_next_token with the sampler spelled out): the
// greedy argmax and step, the top-k measurement step, the greedy device chain, the batched steps and chains of several sessions
// with the backend's entries as parameters (llm_batch.cpp binds the real ones), and llm_sample_exact.
#if defined(__x86_64__)
#include <immintrin.h>
#endif
#include "llm_session.hpp"
#include "kernels/sampler_math.h"
#include "kernels/pool_rule.h"

using namespace llm_host;

// Greedy sampling on the host: the index the loop `best = 0; if (l[i] > l[best]) best = i` returns (first maximum; NaNs never win;
// a NaN in front keeps index 0).  The AVX2 version finds the maximum with the same `>` rule lane by lane, then the first
// position that holds it: 7 -> ~1.5 us for 32000 logits, on the critical path of every decoded token.
static size_t argmax_first_scalar(const float *l, size_t n) {
    size_t best = 0;
    for (size_t i = 1; i < n; i++)
        if (l[i] > l[best]) best = i;
    return best;
}
#if defined(__x86_64__)
__attribute__((target("avx2"))) static size_t argmax_first_avx2(const float *l, size_t n) {
    if (n < 16) return argmax_first_scalar(l, n);
    __m256 mx = _mm256_set1_ps(l[0]);
    size_t i = 0;
    for (; i + 8 <= n; i += 8) {
        const __m256 v = _mm256_loadu_ps(l + i);
        mx = _mm256_blendv_ps(mx, v, _mm256_cmp_ps(v, mx, _CMP_GT_OQ));
    }
    float lanes[8];
    _mm256_storeu_ps(lanes, mx);
    float m = l[0];
    for (int k = 0; k < 8; k++) m = lanes[k] > m ? lanes[k] : m;
    for (; i < n; i++) m = l[i] > m ? l[i] : m;
    if (!(m == m)) return 0;  // l[0] is NaN: nothing compares greater
    const __m256 mv = _mm256_set1_ps(m);
    for (i = 0; i + 8 <= n; i += 8) {
        const int mask = _mm256_movemask_ps(_mm256_cmp_ps(_mm256_loadu_ps(l + i), mv, _CMP_EQ_OQ));
        if (mask) return i + (size_t)__builtin_ctz((unsigned)mask);
    }
    for (; i < n; i++)
        if (l[i] == m) return i;
    return 0;
}
#endif
static size_t argmax_first(const float *l, size_t n) {
#if defined(__x86_64__)
    static const bool have_avx2 = __builtin_cpu_supports("avx2");
    if (have_avx2) return argmax_first_avx2(l, n);
#endif
    return argmax_first_scalar(l, n);
}
static int32_t argmax_of(const llm_session *s) { return (int32_t)argmax_first(s->s->last_logits.data(), s->s->last_logits.size()); }

// inference_session.rs:388-390: a session without room for n more tokens ends the process as the reference's error would
static void require_room(const llm_model *m, const llm_session *s, size_t n, const char *who) {
    if (s->s->n_past + n < m->llama->params.context_size) return;
    fprintf(stderr, "%s: InferenceError::ContextFull\n", who);
    abort();
}

// what a batched step asks of its sessions, whatever their tokens: B different whole-model sessions of m on the calling thread's
// slot, each with room for n more tokens
static bool batch_sessions_ok(const llm_model *m, llm_session *const *sessions, int B, size_t n) {
    if (!m || !sessions || B < 1) return false;
    if (!m->stages.empty() || !m->llama->is_first() || !m->llama->is_last()) return false;
    for (int i = 0; i < B; i++) {
        const llm_session *s = sessions[i];
        if (!s || !s->s || s->model != m || !s->stage_sessions.empty() || s->device != ggml_hip_get_main_device()) return false;
        for (int j = 0; j < i; j++)
            if (sessions[j] == s) return false;
        if (s->s->n_past + n > m->llama->params.context_size) return false;
    }
    return true;
}

// ---- the three pieces every batched step and chain is made of
namespace {
// Stage: the single-token graph of each of B sessions for its id, built exactly as llm_evaluate builds it and not computed — the
// caller hands `graphs` to a backend entry; finish(i) is what evaluate does for session i once an entry has computed them
struct Staged {
    llm_model *m;
    llm_session *const *sessions;
    std::vector<ggml_cgraph *> graphs;
    std::vector<llm::GraphOutputs> outs;
    Staged(llm_model *m, llm_session *const *sessions, const int32_t *ids, int B) : m(m), sessions(sessions), graphs((size_t)B), outs((size_t)B) {
        for (int i = 0; i < B; i++) graphs[(size_t)i] = m->llama->stage_single(*sessions[i]->s, (llm::TokenId)ids[i], outs[(size_t)i]);
    }
    void finish(int i) { m->llama->finish_single(*sessions[i]->s, graphs[(size_t)i], outs[(size_t)i]); }
};
// Commit a chain: an entry ran the staged graphs of row 0 of ids [n][B] and n - 1 more steps on the ids of rows 1 .. n - 1, which it
// sampled itself.  Every session ends as after n steps: the graph's bookkeeping and last_logits (its nodes hold the LAST step's
// results), its column at the end of its history, n_past moved by n.
void commit_chain(Staged &st, int B, int n, const int32_t *ids) {
    std::vector<llm::TokenId> col((size_t)n);
    for (int i = 0; i < B; i++) {
        llm::InferenceSession &s = *st.sessions[i]->s;
        st.finish(i);
        for (int k = 0; k < n; k++) col[(size_t)k] = (llm::TokenId)ids[(size_t)k * B + i];
        s.tokens.push_back(col[0]);
        if (n > 1) s.advance_device_chain(col.data() + 1, (size_t)(n - 1));
    }
}
// Commit a step: the ids a batched step evaluated go to the end of the sessions' histories and out to the caller
void commit_step(llm_session *const *sessions, int B, const int32_t *next, int32_t *out_ids) {
    for (int i = 0; i < B; i++) {
        sessions[i]->s->tokens.push_back((llm::TokenId)next[i]);
        out_ids[i] = next[i];
    }
}
}  // namespace

// ---- the sampled batched chain's host side.  The sampler is kernels/sampler_math.h — the header k_sample_next compiles — so
// the ids drawn here and on the device are the same ids.
static llm_sampler_chain neutral_chain(const llm_sampler_params *p) {
    static const llm_sampler_params none = {0, 0.0f, 0.0f, 0.0f};  // (declined by every check)
    return sampler_chain_neutral<llm_sampler_chain>(p ? *p : none);
}
static bool chain_ok(const llm_sampler_chain *c, size_t V, const float *mus, int B) {
    if (!c || !sampler_chain_ok(*c, (int64_t)V, (int64_t)V)) return false;
    if (c->mirostat == 2) {
        if (!mus) return false;
        for (int i = 0; i < B; i++)
            if (mus[i] != mus[i]) return false;
    }
    return true;
}
// the draw for each of B sessions: from its last_logits and the last 64 tokens of its history, with its own generator (and Mirostat
// state; mus may be null without Mirostat).  All B ids are drawn before anything is staged, so a draw that fails (false) leaves every
// session and — the caller hands in copies — every state unmoved
static bool sample_sessions(llm_session *const *sessions, int B, const llm_sampler_chain *chain, uint64_t *rngs, float *mus, int32_t *ids) {
    for (int i = 0; i < B; i++) {
        const llm::InferenceSession &s = *sessions[i]->s;
        const std::vector<llm::TokenId> &h = s.tokens;  // (TokenId is int32_t)
        const size_t w = std::min(h.size(), (size_t)SAMPLER_WINDOW);
        ids[i] = llm_sample_chain(s.last_logits.data(), (int)s.last_logits.size(), h.data() + (h.size() - w), (int)w, chain, &rngs[i],
                                  mus ? &mus[i] : nullptr);
        if (ids[i] < 0) return false;
    }
    return true;
}
// copies of B Mirostat states to work on (empty: the caller has none)
static std::vector<float> mu_copy(const float *mus, int B) { return mus ? std::vector<float>(mus, mus + B) : std::vector<float>(); }
static float *mu_ptr(std::vector<float> &v) { return v.empty() ? nullptr : v.data(); }

// n sampled tokens of one session with the sampler on the device: `entry` (graph, n, window, window_n, rng, mu, ids, logits) is
// ggml_hip_decode_sampled_chain_ex, or its four-parameter sibling behind a neutral chain; null: always the stepped loop.
// llm_infer_tokens_greedy_device's two attempts: the chain continues a single-token fused-plan run, so after a prompt chunk (or on a
// fresh session) one stepped token arms it; an entry that still declines leaves the rest to the stepped loop.  The session, *rng and
// *mu end exactly as after n calls of llm_infer_next_token_sampled_chain.  Returns the number of tokens the DEVICE drew (n, n - 1 or
// 0); -1 with nothing moved on bad arguments or without room for n tokens.
template <class Entry>
static int tokens_sampled(const Entry *entry, llm_model *m, llm_session *s, int n, const llm_sampler_chain *chain, uint64_t *rng, float *mu,
                          int32_t *out) {
    if (!m || !s || !s->s || !rng || !out || n < 1) return -1;
    if (s->s->n_past + (size_t)n >= m->llama->params.context_size) return -1;
    if (!chain_ok(chain, s->s->last_logits.size(), mu, 1)) return -1;
    int done = 0;
    for (int attempt = 0; attempt < 2 && done < n; attempt++) {
        if (entry && m->stages.empty() && s->s->last_graph) {
            const std::vector<llm::TokenId> &h = s->s->tokens;
            const size_t w = std::min(h.size(), (size_t)SAMPLER_WINDOW);
            uint64_t r = *rng;
            float u = mu ? *mu : 0.0f;
            // (a buffer of the chain's own: a declining entry's scribbles stay away from out)
            std::vector<int32_t> ids((size_t)(n - done));
            if ((*entry)(s->s->last_graph, n - done, h.data() + (h.size() - w), (int)w, &r, mu ? &u : nullptr, ids.data(),
                         s->s->last_logits.data()) == 0) {
                std::copy(ids.begin(), ids.end(), out + done);
                s->s->advance_device_chain((const llm::TokenId *)ids.data(), ids.size());
                *rng = r;
                if (mu) *mu = u;
                return n - done;
            }
        }
        const int32_t id = llm_infer_next_token_sampled_chain(m, s, chain, rng, mu);
        if (id < 0) return -1;  // (only the first: the parameters held for it, and hold for every later one)
        out[done++] = id;
    }
    for (; done < n; done++) out[done] = llm_infer_next_token_sampled_chain(m, s, chain, rng, mu);
    return 0;
}
// n sampled tokens for each of B sessions (`entry` (graphs, B, n, windows, window_n, rngs, mus, ids): ggml_hip_decode_batch_sampled_ex or
// its sibling behind a neutral chain): the host draws row 0 of out_ids [n][B], the device rows 1 .. n - 1 — each column's window moves
// on over the ids the device draws, and the states come back advanced by n draws in all.  Every session and state ends as after n
// calls of the stepped form, which is what runs when there is no entry or it declines.  Returns 1 / 0 / -1 as the greedy form.
template <class Entry>
static int tokens_sampled_batch(llm_batch_entry step, const Entry *entry, llm_model *m, llm_session *const *sessions, int B, int n,
                                const llm_sampler_chain *chain, uint64_t *rngs, float *mus, int32_t *out_ids) {
    if (!out_ids || !rngs || n < 1 || !batch_sessions_ok(m, sessions, B, (size_t)n)) return -1;
    if (!chain_ok(chain, m->llama->hyperparameters.n_vocab, mus, B)) return -1;
    if (entry && B >= 2) {
        std::vector<uint64_t> r(rngs, rngs + B);
        std::vector<float> u = mu_copy(mus, B);
        std::vector<int32_t> first((size_t)B), windows((size_t)B * SAMPLER_WINDOW, 0), window_n((size_t)B);
        if (!sample_sessions(sessions, B, chain, r.data(), mu_ptr(u), first.data())) return -1;
        Staged st(m, sessions, first.data(), B);
        for (int i = 0; i < B; i++) {
            // the window the device starts from: the session's history with this token at its end
            const std::vector<llm::TokenId> &h = sessions[i]->s->tokens;
            const size_t keep = std::min(h.size(), (size_t)SAMPLER_WINDOW - 1);
            int32_t *w = windows.data() + (size_t)i * SAMPLER_WINDOW;
            for (size_t j = 0; j < keep; j++) w[j] = (int32_t)h[h.size() - keep + j];
            w[keep] = first[(size_t)i];
            window_n[(size_t)i] = (int32_t)keep + 1;
        }
        // (a buffer of the chain's own, never empty: a declining entry's scribbles, and at n = 1 its address, stay away from out_ids)
        std::vector<int32_t> rest((size_t)(n - 1) * (size_t)B + 1);
        if ((*entry)(st.graphs.data(), B, n, windows.data(), window_n.data(), r.data(), mu_ptr(u), rest.data()) == 0) {
            std::copy(first.begin(), first.end(), out_ids);
            std::copy(rest.begin(), rest.end() - 1, out_ids + B);
            commit_chain(st, B, n, out_ids);
            std::copy(r.begin(), r.end(), rngs);
            std::copy(u.begin(), u.end(), mus);
            return 1;
        }
    }
    for (int k = 0; k < n; k++)
        if (llm_infer_next_tokens_sampled_chain_batch_via(step, m, sessions, B, chain, rngs, mus, out_ids + (size_t)k * B) < 0) return -1;
    return 0;
}

// ---- generation that stops (llm_infer_until, llm_infer_until_batch): the end rule of InferenceSession::infer, once, for the stepped
// loops, for what the device chains are asked to do and for the test hook.  A session at n_past may draw while n_past + 1 is below
// the context size (inference_session.rs:388); the budget is max_tokens or that room, whichever is less, and a run that uses up a
// budget the room cut short ended on the context.
struct UntilRule {
    const llm_until_request *q;
    int budget;
    bool cut;
    UntilRule(const llm_until_request *q, size_t n_past, size_t context) : q(q) {
        const size_t room = n_past + 1 < context ? context - 1 - n_past : 0;
        budget = (int)std::min((size_t)q->max_tokens, room);
        cut = budget < q->max_tokens;
    }
    bool is_stop(int32_t id) const {
        for (int j = 0; j < q->n_stop; j++)
            if (q->stop_id[j] == id) return true;
        return false;
    }
    int out_of_budget() const { return cut ? LLM_ENDED_BY_CONTEXT : LLM_ENDED_BY_BUDGET; }
    // 0: go on; otherwise why the run ends behind its drawn-th draw, which was `id` (the stop id wins: it is what the reference reports)
    int after(int drawn, int32_t id) const { return is_stop(id) ? LLM_ENDED_BY_STOP : (drawn >= budget ? out_of_budget() : 0); }
};
static bool until_request_ok(const llm_until_request *q, size_t V, const uint64_t *rng, const float *mu) {
    if (!q || q->max_tokens < 1 || q->n_stop < 0 || q->n_stop > 8) return false;
    for (int j = 0; j < q->n_stop; j++)
        if (q->stop_id[j] < 0 || (size_t)q->stop_id[j] >= V) return false;
    return !q->chain || (rng && chain_ok(q->chain, V, mu, 1));
}
static ggml_hip_chain_end until_end(const llm_until_request *q, int budget) {
    ggml_hip_chain_end e;
    memset(&e, 0, sizeof(e));
    e.budget = budget;
    e.n_stop = q->n_stop;
    for (int j = 0; j < q->n_stop; j++) e.stop_id[j] = q->stop_id[j];
    return e;
}
// one draw of a request from a logits row and a window (oldest first, the last 64 count): its sampler, or the first maximum
static int32_t until_draw(const llm_until_request *q, const float *logits, size_t V, const int32_t *hist, size_t n_hist, uint64_t *rng, float *mu) {
    if (!q->chain) return (int32_t)argmax_first(logits, V);
    const size_t w = std::min(n_hist, (size_t)SAMPLER_WINDOW);
    return llm_sample_chain(logits, (int)V, hist + (n_hist - w), (int)w, q->chain, rng, mu);
}
// ... of a session, appended and evaluated (a greedy request steps as llm_infer_next_token_greedy does, a sampling one as
// llm_infer_next_token_sampled_chain); -1 with nothing moved if the sampler declines
static int32_t until_step(llm_model *m, llm_session *s, const llm_until_request *q, uint64_t *rng, float *mu) {
    if (!q->chain) return llm_infer_next_token_greedy(m, s);
    return llm_infer_next_token_sampled_chain(m, s, q->chain, rng, mu);
}

extern "C" {

// test hook: which = 0 the dispatching version, 1 the scalar loop
int llm_argmax_first(const float *l, int n, int which) { return (int)(which ? argmax_first_scalar(l, (size_t)n) : argmax_first(l, (size_t)n)); }

int32_t llm_infer_next_token_greedy(llm_model *m, llm_session *s) {
    // inference_session.rs:381-424 with the sampler chain replaced by argmax over last_logits
    require_room(m, s, 1, "llm_infer_next_token");
    const double t0 = llm::InferenceSession::now_ns();
    const llm::TokenId next = (llm::TokenId)argmax_of(s);
    s->s->tokens.push_back(next);
    llm::OutputRequest req;
    const double t1 = llm::InferenceSession::now_ns();
    req.greedy_next = true;  // the call after this one evaluates the first maximum of this one's logits: the backend may run it ahead
    model_evaluate(m, s, std::vector<llm::TokenId>{next}, req);
    llm::InferenceSession::host_ns_add(5, t1 - t0);                                // argmax
    llm::InferenceSession::host_ns_add(6, llm::InferenceSession::now_ns() - t1);  // evaluate, all of it
    return next;
}
// The reference's token step with the SHAPE of its default sampler (crates/llm-base/src/samplers.rs:97-188: repetition penalty
// 1.30 over the last 64 tokens, top-k 40, [tail-free, typical, top-p: act on the <= 40 survivors], temperature 0.80) instead of
// greedy argmax: what a caller that samples gets from the unchanged sequence sample -> evaluate (inference_session.rs:381-424).
//   device_topk = 0: as the reference does it — all n_vocab logits are read back by the evaluation (model/common.rs:6-19), the
//                    candidates are found on the host (std::partial_sort);
//   device_topk = 1: the evaluation leaves the logits in HBM (OutputRequest::logits_on_device) and the k best + the raw logits of
//                    the penalty window come from llm_session_topk: k + 64 pairs instead of 128 KB per token.
// Same candidates, same arithmetic, same generator: both settings draw the same tokens (tests/test_device_tools_gpu.py).
// `rng`: the caller's xorshift64* state.  Not llm-samplers' chain itself — a measurement of what the read-back costs a sampler.
int32_t llm_infer_next_token_topk(llm_model *m, llm_session *s, int k, float temperature, uint64_t *rng, int device_topk) {
    require_room(m, s, 1, "llm_infer_next_token_topk");
    const size_t V = s->s->last_logits.size();
    if (k < 1 || (size_t)k > V || !rng) return -1;
    const std::vector<llm::TokenId> &hist = s->s->tokens;
    std::vector<int32_t> window;  // the last 64 tokens, each once
    for (size_t i = hist.size() > 64 ? hist.size() - 64 : 0; i < hist.size(); i++)
        if (std::find(window.begin(), window.end(), (int32_t)hist[i]) == window.end()) window.push_back((int32_t)hist[i]);
    std::vector<float> vals(k + window.size());
    std::vector<int32_t> ids(k + window.size());
    if (device_topk) {
        if (llm_session_topk(s, k, window.empty() ? nullptr : window.data(), (int)window.size(), vals.data(), ids.data()) != 0) return -1;
    } else {
        const std::vector<float> &l = s->s->last_logits;
        std::vector<int32_t> order(V);
        for (size_t i = 0; i < V; i++) order[i] = (int32_t)i;
        std::partial_sort(order.begin(), order.begin() + k, order.end(),
                          [&](int32_t a, int32_t b) { return l[a] > l[b] || (l[a] == l[b] && a < b); });
        for (int i = 0; i < k; i++) { ids[i] = order[i]; vals[i] = l[order[i]]; }
        for (size_t i = 0; i < window.size(); i++) { ids[k + i] = window[i]; vals[k + i] = l[window[i]]; }
    }
    // candidates = top-k and the window's tokens (each once), penalised, the k best of them kept
    struct Cand { float v; int32_t id; };
    std::vector<Cand> c;
    for (size_t i = 0; i < ids.size(); i++) {
        bool dup = false;
        for (auto &x : c) dup = dup || x.id == ids[i];
        if (dup) continue;
        float v = vals[i];
        if (std::find(window.begin(), window.end(), ids[i]) != window.end()) v = v > 0.0f ? v / 1.30f : v * 1.30f;
        c.push_back({v, ids[i]});
    }
    std::sort(c.begin(), c.end(), [](const Cand &a, const Cand &b) { return a.v > b.v || (a.v == b.v && a.id < b.id); });
    if (c.size() > (size_t)k) c.resize(k);
    double sum = 0.0;
    std::vector<double> pr(c.size());
    for (size_t i = 0; i < c.size(); i++) sum += (pr[i] = std::exp((double)(c[i].v - c[0].v) / (double)temperature));
    uint64_t x = *rng;  // xorshift64*
    x ^= x >> 12; x ^= x << 25; x ^= x >> 27;
    *rng = x;
    const double u = (double)((x * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0 * sum;
    double acc = 0.0;
    llm::TokenId next = (llm::TokenId)c.back().id;
    for (size_t i = 0; i < c.size(); i++) {
        acc += pr[i];
        if (u < acc) { next = (llm::TokenId)c[i].id; break; }
    }
    s->s->tokens.push_back(next);
    llm::OutputRequest req;
    req.logits_on_device = device_topk != 0;
    model_evaluate(m, s, std::vector<llm::TokenId>{next}, req);
    return next;
}
// n greedy tokens with the sampler on the device (ggml_hip_decode_greedy_chain): the same ids and the
// same final logits as n calls of llm_infer_next_token_greedy, without a logits read-back and host sync per token.
// Falls back to that loop when the backend cannot chain (last evaluation not a single-token fused-plan run, layer
// split stage, ...).  Returns the number of tokens written to out (n).
int llm_infer_tokens_greedy_device(llm_model *m, llm_session *s, int n, int32_t *out) {
    if (n < 1) return 0;
    require_room(m, s, (size_t)n, "llm_infer_tokens_greedy_device");
    int done = 0;
    // the chain continues a single-token fused-plan run; after a prompt chunk (or a fresh session) one normal step arms it
    for (int attempt = 0; attempt < 2 && done < n; attempt++) {
        if (m->stages.empty() && s->s->last_graph &&
            ggml_hip_decode_greedy_chain(s->s->last_graph, n - done, out + done, s->s->last_logits.data()) == 0) {
            s->s->advance_device_chain((const llm::TokenId *)(out + done), (size_t)(n - done));
            return n;
        }
        out[done++] = llm_infer_next_token_greedy(m, s);
    }
    for (; done < n; done++) out[done] = llm_infer_next_token_greedy(m, s);
    return n;
}
// The token step of a caller that samples, in the exact arithmetic of kernels/sampler_math.h: llm_sample_chain on last_logits and the
// last 64 tokens of the history, the id appended and evaluated.  greedy_next stays false: the backend never runs ahead of a sampling
// caller.  -1 with nothing moved on llm_sample_chain's bad arguments.
int32_t llm_infer_next_token_sampled_chain(llm_model *m, llm_session *s, const llm_sampler_chain *chain, uint64_t *rng, float *mu) {
    if (!m || !s || !s->s || !rng) return -1;
    require_room(m, s, 1, "llm_infer_next_token_sampled");
    uint64_t r = *rng;
    float u = mu ? *mu : 0.0f;
    llm_session *one[1] = {s};
    int32_t next = -1;
    if (!sample_sessions(one, 1, chain, &r, mu ? &u : nullptr, &next)) return -1;
    *rng = r;
    if (mu) *mu = u;
    s->s->tokens.push_back((llm::TokenId)next);
    llm::OutputRequest req;
    model_evaluate(m, s, std::vector<llm::TokenId>{(llm::TokenId)next}, req);
    return next;
}
int32_t llm_infer_next_token_sampled(llm_model *m, llm_session *s, const llm_sampler_params *params, uint64_t *rng) {
    const llm_sampler_chain c = neutral_chain(params);
    return llm_infer_next_token_sampled_chain(m, s, &c, rng, nullptr);
}
// n such tokens with the sampler on the device (tokens_sampled above): `entry` = ggml_hip_decode_sampled_chain_ex, or — the
// four-parameter form — ggml_hip_decode_sampled_chain behind a neutral chain; a parameter for the reason the batched entries are.
int llm_infer_tokens_sampled_chain_via(llm_sample_chain_ex_entry entry, llm_model *m, llm_session *s, int n, const llm_sampler_chain *chain,
                                       uint64_t *rng, float *mu, int32_t *out) {
    const auto call = [&](ggml_cgraph *g, int k, const int32_t *w, int wn, uint64_t *r, float *u, int32_t *ids, float *logits) {
        return entry(g, k, chain, w, wn, r, u, ids, logits);
    };
    return tokens_sampled(entry ? &call : nullptr, m, s, n, chain, rng, mu, out);
}
int llm_infer_tokens_sampled_via(llm_sample_chain_entry entry, llm_model *m, llm_session *s, int n, const llm_sampler_params *params,
                                 uint64_t *rng, int32_t *out) {
    const llm_sampler_chain c = neutral_chain(params);
    const auto call = [&](ggml_cgraph *g, int k, const int32_t *w, int wn, uint64_t *r, float *, int32_t *ids, float *logits) {
        return entry(g, k, params, w, wn, r, ids, logits);
    };
    return tokens_sampled(entry ? &call : nullptr, m, s, n, &c, rng, nullptr, out);
}
// One decode step of B sessions of one model (batched multi-session decode): every session's single-token graph is built exactly as
// llm_evaluate builds it and the B graphs go to the backend together (`entry` = ggml_hip_decode_batch: one pass over the weights for
// all of them).  If the backend declines (-1: nothing was executed) the sessions are evaluated one after the other — the same
// results, B passes.  The entry is a parameter because this file also links against backends that have none (the sanitizer jobs'
// host stand-in); host/llm_batch.cpp binds the real one.  Returns 1 = ran batched, 0 = ran one by one, -1 = bad arguments, nothing
// evaluated: a session listed twice, of another model or on another device slot than the calling thread's, a split model, a
// token outside the vocabulary, a session whose context is full.  Like llm_evaluate it leaves the token history to the caller.
int llm_evaluate_batch_via(llm_batch_entry entry, llm_model *m, llm_session *const *sessions, const int32_t *tokens, int B, float *logits) {
    if (!tokens || !batch_sessions_ok(m, sessions, B, 1)) return -1;
    const size_t V = m->llama->hyperparameters.n_vocab;
    for (int i = 0; i < B; i++)
        if (tokens[i] < 0 || (size_t)tokens[i] >= V) return -1;
    int batched = 0;
    if (entry && B >= 2) {
        Staged st(m, sessions, tokens, B);
        if (entry(st.graphs.data(), B) == 0) {
            for (int i = 0; i < B; i++) st.finish(i);
            batched = 1;
        }
    }
    if (!batched)
        for (int i = 0; i < B; i++) {
            llm::OutputRequest req;
            model_evaluate(m, sessions[i], std::vector<llm::TokenId>{(llm::TokenId)tokens[i]}, req);
        }
    if (logits)
        for (int i = 0; i < B; i++) memcpy(logits + (size_t)i * V, sessions[i]->s->last_logits.data(), V * sizeof(float));
    return batched;
}
// llm_infer_next_token_greedy for B sessions in one step: the first maximum of every session's last_logits, then the step above
int llm_infer_next_tokens_greedy_batch_via(llm_batch_entry entry, llm_model *m, llm_session *const *sessions, int B, int32_t *out_ids) {
    if (!m || !sessions || !out_ids || B < 1) return -1;
    std::vector<int32_t> next((size_t)B);
    for (int i = 0; i < B; i++) {
        if (!sessions[i] || !sessions[i]->s) return -1;
        next[(size_t)i] = argmax_of(sessions[i]);
    }
    const int r = llm_evaluate_batch_via(entry, m, sessions, next.data(), B, nullptr);
    if (r >= 0) commit_step(sessions, B, next.data(), out_ids);
    return r;
}
// n greedy tokens for each of B sessions with the sampler on the device (`chain` = ggml_hip_decode_batch_greedy): row 0 of out_ids
// [n][B] is the first maximum of every session's last_logits, as above; the sessions' graphs for those tokens go to the backend once,
// which evaluates them and n - 1 more steps on the tokens it samples itself (rows 1 .. n - 1, written straight into out_ids).  Every
// session ends as after n calls of llm_infer_next_tokens_greedy_batch_via — n_past, token history, last_logits, K/V — and that loop is
// what runs, through `step`, when there is no chain entry or it declines.  Returns 1 = ran chained, 0 = ran as that loop, -1 = nothing
// evaluated, no session moved: the bad arguments of llm_evaluate_batch_via, n < 1, a session without room for n tokens.
int llm_infer_tokens_greedy_batch_via(llm_batch_entry step, llm_batch_chain_entry chain, llm_model *m, llm_session *const *sessions, int B,
                                      int n, int32_t *out_ids) {
    if (!out_ids || n < 1 || !batch_sessions_ok(m, sessions, B, (size_t)n)) return -1;
    if (chain && B >= 2) {
        for (int i = 0; i < B; i++) out_ids[i] = argmax_of(sessions[i]);
        Staged st(m, sessions, out_ids, B);
        if (chain(st.graphs.data(), B, n, out_ids + B) == 0) {
            commit_chain(st, B, n, out_ids);
            return 1;
        }
    }
    for (int k = 0; k < n; k++)
        if (llm_infer_next_tokens_greedy_batch_via(step, m, sessions, B, out_ids + (size_t)k * B) < 0) return -1;
    return 0;
}
// One draw by the written specification (kernels/sampler_math.h, A - E), for any V.  -1 on what it declines; *rng and *mu unmoved then.
int32_t llm_sample_chain(const float *logits, int V, const int32_t *window, int n_window, const llm_sampler_chain *chain, uint64_t *rng,
                         float *mu) {
    if (!logits || V < 1 || n_window < 0 || (n_window > 0 && !window) || !rng || !chain_ok(chain, (size_t)V, mu, 1)) return -1;
    if (n_window > SAMPLER_WINDOW) {
        window += n_window - SAMPLER_WINDOW;
        n_window = SAMPLER_WINDOW;
    }
    const llm_sampler_params *params = &chain->base;
    struct Cand { float v; int32_t id; };
    // A: M with its adjusted values — the window's distinct ids, then the bias ids that are not in it
    std::vector<Cand> c;
    c.reserve((size_t)SAMPLER_K_MAX + SAMPLER_M_MAX);
    for (int i = 0; i < n_window; i++) {
        const int32_t id = window[i];
        if (id < 0 || id >= V) return -1;
        bool dup = false;
        for (const Cand &x : c) dup = dup || x.id == id;
        if (dup) continue;
        int count = 0, at = -1;
        for (int j = 0; j < n_window; j++) count += window[j] == id;
        for (int j = 0; j < chain->n_bias; j++)
            if (chain->bias_id[j] == id) at = j;
        c.push_back({sampler_adjust(logits[id], at >= 0, at >= 0 ? chain->bias[at] : 0.0f, count, params->penalty, chain->freq, chain->presence), id});
    }
    for (int j = 0; j < chain->n_bias; j++) {
        bool in_window = false;
        for (const Cand &x : c) in_window = in_window || x.id == chain->bias_id[j];
        if (!in_window) c.push_back({sampler_adjust(logits[chain->bias_id[j]], true, chain->bias[j], 0, params->penalty, chain->freq, chain->presence), chain->bias_id[j]});
    }
    const size_t n_m = c.size();
    if (chain->mirostat == 2) {  // E
        std::vector<float> e(logits, logits + V);
        for (size_t j = 0; j < n_m; j++) e[(size_t)c[j].id] = c[j].v;
        float amax = e[0];
        int first = 0;
        for (int i = 1; i < V; i++)
            if (e[(size_t)i] > amax) {
                amax = e[(size_t)i];
                first = i;
            }
        for (int i = 0; i < V; i++) e[(size_t)i] = sampler_mirostat_e(e[(size_t)i], amax, params->temperature);
        const int nb = (V + SAMPLER_BLOCK - 1) / SAMPLER_BLOCK;
        std::vector<double> sums((size_t)nb);
        std::vector<char> keep((size_t)V, 1);
        const auto total = [&] {  // the block sums over the kept entries, then their sum
            double S = 0.0;
            for (int b = 0; b < nb; b++) {
                double sb = 0.0;
                for (int i = b * SAMPLER_BLOCK; i < std::min(V, (b + 1) * SAMPLER_BLOCK); i++)
                    if (keep[(size_t)i]) sb += (double)e[(size_t)i];
                sums[(size_t)b] = sb;
            }
            for (int b = 0; b < nb; b++) S += sums[(size_t)b];
            return S;
        };
        const double S = total();
        if (*mu < 0.0f) {
            std::fill(keep.begin(), keep.end(), 0);
        } else {
            const double least = sampler_mirostat_least(S, *mu);
            for (int i = 0; i < V; i++) keep[(size_t)i] = (double)e[(size_t)i] >= least;
        }
        keep[(size_t)first] = 1;
        const double S_R = total();
        const uint64_t x = sampler_rng_step(*rng);
        const double u = sampler_rng_unit(x) * S_R;
        int sel = -1;
        double run = 0.0;
        for (int b = 0; b < nb && sel < 0; b++) {
            const double before = run;
            run += sums[(size_t)b];
            if (!(run > u)) continue;
            double acc = 0.0;
            for (int i = b * SAMPLER_BLOCK; i < std::min(V, (b + 1) * SAMPLER_BLOCK); i++) {
                if (!keep[(size_t)i]) continue;
                sel = i;  // (the block's last retained id, unless the walk stops before it)
                acc += (double)e[(size_t)i];
                if (u - before < acc) break;
            }
        }
        for (int i = V - 1; i >= 0 && sel < 0; i--)
            if (keep[(size_t)i]) sel = i;
        *rng = x;
        *mu = sampler_mirostat_mu(*mu, e[(size_t)sel], S_R, chain->tau, chain->eta);
        return sel;
    }
    // B: the raw top-k beside M, the k best kept
    const int k = params->k;
    std::vector<int32_t> order((size_t)V);
    for (int i = 0; i < V; i++) order[(size_t)i] = i;
    std::partial_sort(order.begin(), order.begin() + k, order.end(),
                      [&](int32_t a, int32_t b) { return logits[a] > logits[b] || (logits[a] == logits[b] && a < b); });
    for (int i = 0; i < k; i++) {
        bool in_m = false;
        for (size_t j = 0; j < n_m; j++) in_m = in_m || c[j].id == order[(size_t)i];
        if (!in_m) c.push_back({logits[order[(size_t)i]], order[(size_t)i]});
    }
    std::sort(c.begin(), c.end(), [](const Cand &a, const Cand &b) { return a.v > b.v || (a.v == b.v && a.id < b.id); });
    c.resize((size_t)k);  // (the raw top-k alone are k candidates)
    std::vector<float> v((size_t)k), q((size_t)k), p((size_t)k);
    for (int i = 0; i < k; i++) {
        v[(size_t)i] = c[(size_t)i].v;
        q[(size_t)i] = sampler_q(c[(size_t)i].v, c[0].v);
        p[(size_t)i] = sampler_p(c[(size_t)i].v, c[0].v, params->temperature);
    }
    // C, D
    const int n = sampler_tail_free(q.data(), k, chain->tail_free_z);
    std::vector<int> ord, idx((size_t)n);
    double Q = 0.0;
    if (chain->typical_p < 1.0f) {
        const double mean = sampler_typical_mean(v.data(), q.data(), n, &Q);
        std::vector<double> t((size_t)n);
        ord.resize((size_t)n);
        for (int i = 0; i < n; i++) {
            t[(size_t)i] = sampler_typical_key(v[0], v[(size_t)i], q[(size_t)i], mean);
            ord[(size_t)i] = i;
        }
        std::sort(ord.begin(), ord.end(), [&](int a, int b) { return t[(size_t)a] < t[(size_t)b] || (t[(size_t)a] == t[(size_t)b] && a < b); });
    }
    return c[(size_t)sampler_pick_chain(q.data(), p.data(), n, ord.empty() ? nullptr : ord.data(), Q, chain->typical_p, params->top_p,
                                        chain->min_p, idx.data(), rng)].id;
}
int32_t llm_sample_exact(const float *logits, int V, const int32_t *window, int n_window, const llm_sampler_params *params, uint64_t *rng) {
    const llm_sampler_chain c = neutral_chain(params);
    return llm_sample_chain(logits, V, window, n_window, &c, rng, nullptr);
}
void llm_sampler_log2(const double *r, int n, float *out) {
    for (int i = 0; i < n; i++) out[i] = sampler_log2(r[i]);
}
// llm_infer_next_tokens_greedy_batch_via with that sampler: every session draws from its own generator (rngs[i]; Mirostat state
// mus[i]), the id is appended to its history and evaluated in one batched step.  -1: nothing evaluated, no session and no state moved.
int llm_infer_next_tokens_sampled_chain_batch_via(llm_batch_entry entry, llm_model *m, llm_session *const *sessions, int B,
                                                  const llm_sampler_chain *chain, uint64_t *rngs, float *mus, int32_t *out_ids) {
    if (!out_ids || !rngs || !batch_sessions_ok(m, sessions, B, 1) || !chain_ok(chain, m->llama->hyperparameters.n_vocab, mus, B)) return -1;
    std::vector<int32_t> next((size_t)B);
    std::vector<uint64_t> r(rngs, rngs + B);
    std::vector<float> u = mu_copy(mus, B);
    if (!sample_sessions(sessions, B, chain, r.data(), mu_ptr(u), next.data())) return -1;
    const int rc = llm_evaluate_batch_via(entry, m, sessions, next.data(), B, nullptr);
    if (rc < 0) return -1;
    commit_step(sessions, B, next.data(), out_ids);
    std::copy(r.begin(), r.end(), rngs);
    std::copy(u.begin(), u.end(), mus);
    return rc;
}
int llm_infer_next_tokens_sampled_batch_via(llm_batch_entry entry, llm_model *m, llm_session *const *sessions, int B,
                                            const llm_sampler_params *params, uint64_t *rngs, int32_t *out_ids) {
    const llm_sampler_chain c = neutral_chain(params);
    return llm_infer_next_tokens_sampled_chain_batch_via(entry, m, sessions, B, &c, rngs, nullptr, out_ids);
}
// llm_infer_tokens_greedy_batch_via with that sampler (tokens_sampled_batch above): `chain_entry` = ggml_hip_decode_batch_sampled_ex, or
// — the four-parameter form — ggml_hip_decode_batch_sampled behind a neutral chain.
int llm_infer_tokens_sampled_chain_batch_via(llm_batch_entry step, llm_batch_sample_ex_entry chain_entry, llm_model *m,
                                             llm_session *const *sessions, int B, int n, const llm_sampler_chain *chain, uint64_t *rngs,
                                             float *mus, int32_t *out_ids) {
    const auto call = [&](ggml_cgraph *const *graphs, int nb, int k, const int32_t *w, const int32_t *wn, uint64_t *r, float *u, int32_t *ids) {
        return chain_entry(graphs, nb, k, chain, w, wn, r, u, ids);
    };
    return tokens_sampled_batch(step, chain_entry ? &call : nullptr, m, sessions, B, n, chain, rngs, mus, out_ids);
}
int llm_infer_tokens_sampled_batch_via(llm_batch_entry step, llm_batch_sample_entry chain, llm_model *m, llm_session *const *sessions, int B,
                                       int n, const llm_sampler_params *params, uint64_t *rngs, int32_t *out_ids) {
    const llm_sampler_chain c = neutral_chain(params);
    const auto call = [&](ggml_cgraph *const *graphs, int nb, int k, const int32_t *w, const int32_t *wn, uint64_t *r, float *, int32_t *ids) {
        return chain(graphs, nb, k, params, w, wn, r, ids);
    };
    return tokens_sampled_batch(step, chain ? &call : nullptr, m, sessions, B, n, &c, rngs, nullptr, out_ids);
}

// ---- generation that stops ----
// One session (`entry` = ggml_hip_decode_chain_requests, or NULL: always the stepped loop).  tokens_sampled's two attempts: the chain
// continues a single-token fused-plan run, so behind a prompt chunk one stepped token arms it.  The entry is asked for what is left of
// the budget and ends by itself; whatever it declines is left to the stepped loop under the same rule.
int llm_infer_until_via(llm_chain_requests_entry entry, llm_model *m, llm_session *s, const llm_until_request *req, uint64_t *rng, float *mu,
                        int32_t *out, int32_t *n_out, int32_t *ended_by) {
    if (!m || !s || !s->s || !out || !n_out || !ended_by) return -1;
    if (!until_request_ok(req, s->s->last_logits.size(), rng, mu)) return -1;
    const UntilRule rule(req, s->s->n_past, m->llama->params.context_size);
    int done = 0, why = rule.budget == 0 ? LLM_ENDED_BY_CONTEXT : 0, ran = 0;
    for (int attempt = 0; attempt < 2 && !why; attempt++) {
        if (entry && m->stages.empty() && s->s->last_graph) {
            const std::vector<llm::TokenId> &h = s->s->tokens;
            const size_t w = std::min(h.size(), (size_t)SAMPLER_WINDOW);
            const int left = rule.budget - done;
            const ggml_hip_chain_end end = until_end(req, left);
            uint64_t r = rng ? *rng : 0;
            float u = mu ? *mu : 0.0f;
            int32_t drawn = 0, dev_why = 0;
            std::vector<int32_t> ids((size_t)left);  // (a buffer of the chain's own: a declining entry's scribbles stay away from out)
            if (entry(s->s->last_graph, left, req->chain, &end, h.data() + (h.size() - w), (int)w, rng ? &r : nullptr, mu ? &u : nullptr, ids.data(),
                      &drawn, &dev_why, s->s->last_logits.data()) == 0) {
                std::copy(ids.begin(), ids.begin() + drawn, out + done);
                s->s->advance_device_chain((const llm::TokenId *)ids.data(), (size_t)drawn);
                if (rng) *rng = r;
                if (mu) *mu = u;
                done += drawn;
                why = dev_why == GGML_HIP_CHAIN_END_STOP ? LLM_ENDED_BY_STOP : rule.out_of_budget();
                ran = 1;
                break;
            }
        }
        const int32_t id = until_step(m, s, req, rng, mu);
        if (id < 0) return -1;  // (only the first: the parameters held for it, and hold for every later one)
        out[done++] = id;
        why = rule.after(done, id);
    }
    while (!why) {
        const int32_t id = until_step(m, s, req, rng, mu);
        out[done++] = id;
        why = rule.after(done, id);
    }
    for (int i = done; i < req->max_tokens; i++) out[i] = -1;
    *n_out = done;
    *ended_by = why;
    return ran;
}
// B sessions (`entry` = ggml_hip_decode_batch_requests; `step` = ggml_hip_decode_batch for the stepped form; either may be NULL).
// The host draws row 0 for every session — a session whose first token is a stop id enters the chain with a budget of one evaluation —
// and the chain runs for the largest budget.  Without an entry, or when it declines, or when a session has no room at all: steps over
// the sessions that are still going, each drawn from its own request.
int llm_infer_until_batch_via(llm_batch_entry step, llm_batch_requests_entry entry, llm_model *m, llm_session *const *sessions, int B,
                              const llm_until_request *reqs, uint64_t *rngs, float *mus, int32_t *out_ids, int32_t *n_out, int32_t *ended_by) {
    if (!reqs || !out_ids || !n_out || !ended_by || !batch_sessions_ok(m, sessions, B, 0)) return -1;
    const size_t V = m->llama->hyperparameters.n_vocab;
    int n = 0;
    bool room_for_all = true;
    std::vector<UntilRule> rules;
    for (int i = 0; i < B; i++) {
        if (!until_request_ok(&reqs[i], V, rngs ? &rngs[i] : nullptr, mus ? &mus[i] : nullptr)) return -1;
        rules.emplace_back(&reqs[i], sessions[i]->s->n_past, m->llama->params.context_size);
        n = std::max(n, (int)reqs[i].max_tokens);
        room_for_all = room_for_all && rules.back().budget > 0;
    }
    std::vector<int> done((size_t)B, 0), why((size_t)B, 0);
    std::fill(out_ids, out_ids + (size_t)n * B, -1);
    const auto history = [&](int i) -> const std::vector<llm::TokenId> & { return sessions[i]->s->tokens; };
    if (entry && B >= 2 && room_for_all) {
        std::vector<uint64_t> r((size_t)B, 0);
        std::vector<float> u((size_t)B, 0.0f);
        if (rngs) std::copy(rngs, rngs + B, r.begin());
        if (mus) std::copy(mus, mus + B, u.begin());
        std::vector<int32_t> first((size_t)B), windows((size_t)B * SAMPLER_WINDOW, 0), window_n((size_t)B);
        std::vector<const ggml_hip_sampler_chain *> chains((size_t)B);
        std::vector<ggml_hip_chain_end> ends((size_t)B);
        int n_steps = 1;
        bool drew = true;
        for (int i = 0; i < B && drew; i++) {
            const llm::InferenceSession &s = *sessions[i]->s;
            first[(size_t)i] = until_draw(&reqs[i], s.last_logits.data(), V, history(i).data(), history(i).size(), &r[(size_t)i], mus ? &u[(size_t)i] : nullptr);
            drew = first[(size_t)i] >= 0;
            chains[(size_t)i] = reqs[i].chain;
            ends[(size_t)i] = until_end(&reqs[i], rules[(size_t)i].is_stop(first[(size_t)i]) ? 1 : rules[(size_t)i].budget);
            n_steps = std::max(n_steps, (int)ends[(size_t)i].budget);
        }
        if (!drew) return -1;
        Staged st(m, sessions, first.data(), B);
        for (int i = 0; i < B; i++) {  // the window the device starts from: the session's history with this token at its end
            const std::vector<llm::TokenId> &h = history(i);
            const size_t keep = std::min(h.size(), (size_t)SAMPLER_WINDOW - 1);
            int32_t *w = windows.data() + (size_t)i * SAMPLER_WINDOW;
            for (size_t j = 0; j < keep; j++) w[j] = (int32_t)h[h.size() - keep + j];
            w[keep] = first[(size_t)i];
            window_n[(size_t)i] = (int32_t)keep + 1;
        }
        std::vector<int32_t> rest((size_t)(n_steps - 1) * (size_t)B + 1), evaluated((size_t)B), dev_why((size_t)B);
        if (entry(st.graphs.data(), B, n_steps, chains.data(), ends.data(), windows.data(), window_n.data(), r.data(), mus ? u.data() : nullptr,
                  rest.data(), evaluated.data(), dev_why.data()) == 0) {
            std::vector<llm::TokenId> col;
            for (int i = 0; i < B; i++) {
                llm::InferenceSession &s = *sessions[i]->s;
                const int e = evaluated[(size_t)i];
                st.finish(i);
                s.tokens.push_back((llm::TokenId)first[(size_t)i]);
                out_ids[i] = first[(size_t)i];
                col.clear();
                for (int k = 1; k < e; k++) col.push_back((llm::TokenId)(out_ids[(size_t)k * B + i] = rest[(size_t)(k - 1) * B + i]));
                if (!col.empty()) s.advance_device_chain(col.data(), col.size());
                n_out[i] = e;
                ended_by[i] = (dev_why[(size_t)i] == GGML_HIP_CHAIN_END_STOP || rules[(size_t)i].is_stop(first[(size_t)i])) ? LLM_ENDED_BY_STOP
                                                                                                                         : rules[(size_t)i].out_of_budget();
            }
            if (rngs) std::copy(r.begin(), r.end(), rngs);
            if (mus) std::copy(u.begin(), u.end(), mus);
            return 1;
        }
    }
    for (int i = 0; i < B; i++) why[(size_t)i] = rules[(size_t)i].budget == 0 ? LLM_ENDED_BY_CONTEXT : 0;
    for (;;) {
        std::vector<llm_session *> going;
        std::vector<int> who;
        std::vector<int32_t> next;
        for (int i = 0; i < B; i++)
            if (!why[(size_t)i]) {
                const llm::InferenceSession &s = *sessions[i]->s;
                uint64_t r = rngs ? rngs[i] : 0;
                float u = mus ? mus[i] : 0.0f;
                const int32_t id = until_draw(&reqs[i], s.last_logits.data(), V, history(i).data(), history(i).size(), &r, mus ? &u : nullptr);
                if (id < 0) return -1;  // (only in the first round, before anything moved: the parameters hold for every later draw)
                if (rngs) rngs[i] = r;
                if (mus) mus[i] = u;
                going.push_back(sessions[i]);
                who.push_back(i);
                next.push_back(id);
            }
        if (going.empty()) break;
        if (llm_evaluate_batch_via(step, m, going.data(), next.data(), (int)going.size(), nullptr) < 0) return -1;
        for (size_t j = 0; j < going.size(); j++) {
            const int i = who[j];
            going[j]->s->tokens.push_back((llm::TokenId)next[j]);
            out_ids[(size_t)done[(size_t)i] * B + i] = next[j];
            done[(size_t)i]++;
            why[(size_t)i] = rules[(size_t)i].after(done[(size_t)i], next[j]);
        }
    }
    for (int i = 0; i < B; i++) {
        n_out[i] = done[(size_t)i];
        ended_by[i] = why[(size_t)i];
    }
    return 0;
}
// the end rule alone, on recorded rows (test hook): the same UntilRule, the same draw, no session
int llm_until_rule(const float *rows, int n_rows, int V, const llm_until_request *req, const int32_t *window, int n_window, int n_past0,
                   int context_size, uint64_t *rng, float *mu, int32_t *out, int32_t *n_out, int32_t *ended_by) {
    if (!rows || n_rows < 0 || V < 1 || !out || !n_out || !ended_by || n_window < 0 || (n_window > 0 && !window) || n_past0 < 0 || context_size < 1)
        return -1;
    if (!until_request_ok(req, (size_t)V, rng, mu)) return -1;
    const UntilRule rule(req, (size_t)n_past0, (size_t)context_size);
    std::vector<int32_t> hist(window, window + n_window);
    int done = 0, why = rule.budget == 0 ? LLM_ENDED_BY_CONTEXT : 0;
    while (!why && done < n_rows) {
        const int32_t id = until_draw(req, rows + (size_t)done * V, (size_t)V, hist.data(), hist.size(), rng, mu);
        if (id < 0) return -1;
        hist.push_back(id);
        out[done++] = id;
        why = rule.after(done, id);
    }
    *n_out = done;
    *ended_by = why;
    return 0;
}

// ---- the request pool: N sessions' requests over at most max_cols columns (kernels/pool_rule.h) ----
int llm_pool_schedule(const int32_t *evals, int n, int n_cols, int32_t *col_out, int32_t *first_step_out) {
    if (!evals || n_cols < 1 || n_cols > POOL_COLS_MAX || n < n_cols) return -1;
    for (int i = 0; i < n; i++)
        if (evals[i] < 1) return -1;
    return pool_schedule(evals, n, n_cols, col_out, first_step_out);
}
static int g_pool_step_cap = 4096;  // (BATCH_CHAIN_MAX_STEPS)
int llm_pool_step_cap(int cap) {
    const int was = g_pool_step_cap;
    if (cap >= 1 && cap <= 4096) g_pool_step_cap = cap;
    return was;
}
// `entry` = ggml_hip_decode_pool_requests, `single` = ggml_hip_decode_chain_requests (a lone remainder: llm_infer_until_via), `step` =
// ggml_hip_decode_batch for the stepped form; any may be NULL.  The host draws every request's first token; the entry gets the first
// 64 unfinished requests and is called again for whatever it left unfinished or unstarted (more than 64, the step cap); a request
// whose budget the cap cut comes back "ended by its budget" with budget left, and simply goes on in the next call.  When the entry
// declines, everything left runs as steps under the same admission rule.
int llm_infer_until_pool_via(llm_batch_entry step, llm_chain_requests_entry single, llm_pool_requests_entry entry, llm_model *m,
                             llm_session *const *sessions, int N, const llm_until_request *reqs, uint64_t *rngs, float *mus, int max_cols,
                             int32_t *out_ids, int32_t *n_out, int32_t *ended_by) {
    if (!reqs || !out_ids || !n_out || !ended_by || max_cols < 1 || max_cols > POOL_COLS_MAX || !batch_sessions_ok(m, sessions, N, 0)) return -1;
    const size_t V = m->llama->hyperparameters.n_vocab;
    int n = 0;
    std::vector<UntilRule> rules;
    for (int i = 0; i < N; i++) {
        if (!until_request_ok(&reqs[i], V, rngs ? &rngs[i] : nullptr, mus ? &mus[i] : nullptr)) return -1;
        rules.emplace_back(&reqs[i], sessions[i]->s->n_past, m->llama->params.context_size);
        n = std::max(n, (int)reqs[i].max_tokens);
    }
    std::vector<int> done((size_t)N, 0), why((size_t)N, 0);
    std::fill(out_ids, out_ids + (size_t)n * N, -1);
    for (int i = 0; i < N; i++) why[(size_t)i] = rules[(size_t)i].budget == 0 ? LLM_ENDED_BY_CONTEXT : 0;  // (it never enters the pool)
    const auto history = [&](int i) -> const std::vector<llm::TokenId> & { return sessions[i]->s->tokens; };
    const auto draw = [&](int i, uint64_t *r, float *u) {
        const llm::InferenceSession &s = *sessions[i]->s;
        return until_draw(&reqs[i], s.last_logits.data(), V, history(i).data(), history(i).size(), r, u);
    };
    const auto finish = [&](int ran) {
        for (int i = 0; i < N; i++) {
            n_out[i] = done[(size_t)i];
            ended_by[i] = why[(size_t)i];
        }
        return ran;
    };
    int ran = 0;
    bool moved = false;  // (a draw can fail only before anything moved: the parameters then hold for every later draw)
    for (;;) {
        std::vector<int> todo;
        for (int i = 0; i < N; i++)
            if (!why[(size_t)i]) todo.push_back(i);
        if (todo.empty()) return finish(ran);
        if (todo.size() == 1 || max_cols == 1) {  // a lone remainder (or one column): the one-session form, one after the other
            for (const int i : todo) {
                llm_until_request q = reqs[i];
                q.max_tokens = rules[(size_t)i].budget - done[(size_t)i];
                std::vector<int32_t> ids((size_t)q.max_tokens);
                int32_t cnt = 0, w = 0;
                const int rc = llm_infer_until_via(single, m, sessions[i], &q, rngs ? &rngs[i] : nullptr, mus ? &mus[i] : nullptr, ids.data(), &cnt, &w);
                if (rc < 0) return -1;
                moved = true;
                std::copy(ids.begin(), ids.begin() + cnt, out_ids + (size_t)i * n + done[(size_t)i]);
                done[(size_t)i] += cnt;
                why[(size_t)i] = w == LLM_ENDED_BY_STOP ? w : rules[(size_t)i].out_of_budget();
                ran = ran || rc;
            }
            return finish(ran);
        }
        if (!entry) break;
        const int P = (int)std::min(todo.size(), (size_t)POOL_REQUESTS_MAX), B = std::min(max_cols, P);
        std::vector<uint64_t> r((size_t)P, 0);
        std::vector<float> u((size_t)P, 0.0f);
        std::vector<int32_t> first((size_t)P), windows((size_t)P * SAMPLER_WINDOW, 0), window_n((size_t)P), budgets((size_t)P);
        std::vector<const ggml_hip_sampler_chain *> chains((size_t)P);
        std::vector<ggml_hip_chain_end> ends((size_t)P);
        std::vector<llm_session *> who((size_t)P);
        for (int j = 0; j < P; j++) {
            const int i = todo[(size_t)j];
            if (rngs) r[(size_t)j] = rngs[i];
            if (mus) u[(size_t)j] = mus[i];
            first[(size_t)j] = draw(i, &r[(size_t)j], mus ? &u[(size_t)j] : nullptr);
            if (first[(size_t)j] < 0) {
                if (!moved) return -1;
                abort();  // (cannot happen: see `moved`)
            }
            who[(size_t)j] = sessions[i];
            chains[(size_t)j] = reqs[i].chain;
            budgets[(size_t)j] = rules[(size_t)i].is_stop(first[(size_t)j]) ? 1 : rules[(size_t)i].budget - done[(size_t)i];
        }
        const int n_steps = std::min(pool_schedule(budgets.data(), P, B, nullptr, nullptr), g_pool_step_cap);
        for (int j = 0; j < P; j++) {
            const int i = todo[(size_t)j];
            ends[(size_t)j] = until_end(&reqs[i], std::min((int)budgets[(size_t)j], n_steps));
            const std::vector<llm::TokenId> &h = history(i);  // the window the device starts from: the history with this token at its end
            const size_t keep = std::min(h.size(), (size_t)SAMPLER_WINDOW - 1);
            int32_t *w = windows.data() + (size_t)j * SAMPLER_WINDOW;
            for (size_t k = 0; k < keep; k++) w[k] = (int32_t)h[h.size() - keep + k];
            w[keep] = first[(size_t)j];
            window_n[(size_t)j] = (int32_t)keep + 1;
        }
        Staged st(m, who.data(), first.data(), P);
        std::vector<int32_t> rest((size_t)(n_steps - 1) * (size_t)B + 1), col((size_t)P), first_step((size_t)P), evaluated((size_t)P), dev_why((size_t)P);
        int32_t steps_run = 0;
        if (entry(st.graphs.data(), P, B, n_steps, chains.data(), ends.data(), windows.data(), window_n.data(), r.data(), mus ? u.data() : nullptr,
                  rest.data(), col.data(), first_step.data(), evaluated.data(), dev_why.data(), &steps_run) != 0)
            break;
        ran = 1;
        moved = true;
        std::vector<llm::TokenId> ids;
        for (int j = 0; j < P; j++) {
            const int i = todo[(size_t)j], c = col[(size_t)j], e = evaluated[(size_t)j], f = first_step[(size_t)j];
            if (c < 0 || e < 1) continue;  // it never left the queue: untouched, its draw forgotten
            llm::InferenceSession &s = *sessions[i]->s;
            st.finish(j);
            s.tokens.push_back((llm::TokenId)first[(size_t)j]);
            int32_t *o = out_ids + (size_t)i * n + done[(size_t)i];
            o[0] = first[(size_t)j];
            ids.clear();
            for (int k = 1; k < e; k++) ids.push_back((llm::TokenId)(o[k] = rest[(size_t)(f + k - 1) * B + c]));
            if (!ids.empty()) s.advance_device_chain(ids.data(), ids.size());
            done[(size_t)i] += e;
            if (rngs) rngs[i] = r[(size_t)j];
            if (mus) mus[i] = u[(size_t)j];
            const UntilRule &rule = rules[(size_t)i];
            if (dev_why[(size_t)j] == GGML_HIP_CHAIN_END_STOP || rule.is_stop(first[(size_t)j])) why[(size_t)i] = LLM_ENDED_BY_STOP;
            else if (done[(size_t)i] >= rule.budget) why[(size_t)i] = rule.out_of_budget();
        }
    }
    // The stepped form under the same admission rule: columns, a tail that draws, an admission, a step of the columns that have a
    // token to evaluate.  (A session's results do not depend on its column or its step; the rule decides who waits.)
    std::vector<int> todo;
    for (int i = 0; i < N; i++)
        if (!why[(size_t)i]) todo.push_back(i);
    const int P = (int)todo.size(), B = std::min(max_cols, P);
    int owner[POOL_COLS_MAX], live[POOL_COLS_MAX], was_live[POOL_COLS_MAX], take[POOL_COLS_MAX], cursor = B;
    int32_t next[POOL_COLS_MAX];
    bool has[POOL_COLS_MAX];
    // a draw for the request in column c: the token waits for the next step; the request stays live while more draws will follow
    const auto draw_col = [&](int c) -> bool {
        const int i = owner[c];
        uint64_t r = rngs ? rngs[i] : 0;
        float u = mus ? mus[i] : 0.0f;
        const int32_t id = draw(i, &r, mus ? &u : nullptr);
        if (id < 0) return false;
        if (rngs) rngs[i] = r;
        if (mus) mus[i] = u;
        next[c] = id;
        has[c] = true;
        why[(size_t)i] = rules[(size_t)i].after(done[(size_t)i] + 1, id);
        live[c] = !why[(size_t)i];
        return true;
    };
    for (int c = 0; c < B; c++) {
        owner[c] = todo[(size_t)c];
        has[c] = false;
    }
    {  // every first draw before anything moves, on copies
        std::vector<uint64_t> r0;
        std::vector<float> u0;
        if (rngs) r0.assign(rngs, rngs + N);
        if (mus) u0.assign(mus, mus + N);
        bool ok = true;
        for (int c = 0; c < B && ok; c++) ok = draw_col(c);
        if (!ok) {
            if (rngs) std::copy(r0.begin(), r0.end(), rngs);
            if (mus) std::copy(u0.begin(), u0.end(), mus);
            if (!moved) return -1;
            abort();
        }
    }
    for (int c = 0; c < B; c++) was_live[c] = live[c];
    for (;;) {
        std::vector<llm_session *> going;
        std::vector<int32_t> ids;
        std::vector<int> cols;
        for (int c = 0; c < B; c++)
            if (has[c]) {
                going.push_back(sessions[owner[c]]);
                ids.push_back(next[c]);
                cols.push_back(c);
            }
        if (going.empty()) break;
        if (llm_evaluate_batch_via(step, m, going.data(), ids.data(), (int)going.size(), nullptr) < 0) return -1;
        for (size_t j = 0; j < going.size(); j++) {  // the step's commit
            const int c = cols[j], i = owner[c];
            going[j]->s->tokens.push_back((llm::TokenId)ids[j]);
            out_ids[(size_t)i * n + done[(size_t)i]] = ids[j];
            done[(size_t)i]++;
            has[c] = false;
        }
        for (int c = 0; c < B; c++)  // the tail
            if (live[c] && !draw_col(c)) abort();
        cursor = pool_assign(live, was_live, B, cursor, P, take);  // the admission
        for (int c = 0; c < B; c++) {
            if (take[c] >= 0) {
                owner[c] = todo[(size_t)take[c]];
                if (!draw_col(c)) abort();
            }
            was_live[c] = live[c];
        }
    }
    return finish(ran);
}

}  // extern "C"
