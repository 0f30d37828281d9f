// llm_pack.cpp — feeding the prompts of several sessions as packed prompt batches: llm_pack_schedule (the rule for rounds, no device),
// llm_feed_prompt_batch_via and llm_prompt_pack_via (one evaluation, for tests and tools), with the backend's entry
// (ggml_hip_prompt_pack) as a parameter as every batched call of the mirror has it; host/llm_batch.cpp binds the library's own.
#include <algorithm>
#include <vector>

#include "llm_session.hpp"

using namespace llm_host;

namespace {
const int PACK_ROWS_DEFAULT = 512, PACK_ROWS_MAX = 4096, PACK_SESSIONS_MAX = 64;  // (the entry's: PROMPT_PLAN_MAX rows, 64 graphs)

// The ONE rule for rounds: in every round the sessions are visited in index order and a session with tokens left takes
// min(left, room) rows, room being what is left of max_rows; rounds repeat until nothing is left.  take: [rounds][B], row-major.
int schedule(const int32_t *counts, int B, int max_rows, std::vector<int32_t> *take) {
    std::vector<int32_t> left(counts, counts + B);
    int rounds = 0;
    for (;;) {
        int room = max_rows;
        std::vector<int32_t> row((size_t)B, 0);
        for (int i = 0; i < B && room > 0; i++) {
            row[(size_t)i] = std::min(left[(size_t)i], room);
            left[(size_t)i] -= row[(size_t)i];
            room -= row[(size_t)i];
        }
        if (room == max_rows) return rounds;  // nothing was left
        if (take) take->insert(take->end(), row.begin(), row.end());
        rounds++;
    }
}
// One evaluation of the entry: session who[k] appends the n[k] tokens at tk[k].  The graphs are built as llm_evaluate builds them for a
// default OutputRequest and not computed; if the entry runs them (true) every session gets compute()'s bookkeeping, its tokens, and —
// last[k] — last_logits from its last row; all_logits (nullable): every row's logits, [sum n][V] in order; embeddings (nullable):
// [who.size()][E], each session's last row.  false: the entry declined, nothing was executed and no session moved.
bool pack_once(llm_pack_entry entry, llm_model *m, llm_session *const *sessions, const std::vector<int> &who, const std::vector<const int32_t *> &tk,
               const std::vector<int32_t> &n, const std::vector<char> &last, float *all_logits, float *embeddings) {
    const size_t V = m->llama->hyperparameters.n_vocab, E = m->llama->hyperparameters.n_embd;
    std::vector<ggml_cgraph *> graphs(who.size());
    std::vector<llm::GraphOutputs> outs(who.size());
    for (size_t k = 0; k < who.size(); k++)
        graphs[k] = m->llama->stage_rows(*sessions[who[k]]->s, (const llm::TokenId *)tk[k], (size_t)n[k], outs[k]);
    if (entry(graphs.data(), (int)graphs.size()) != 0) return false;
    size_t row0 = 0;
    for (size_t k = 0; k < who.size(); k++) {
        llm::InferenceSession &ss = *sessions[who[k]]->s;
        m->llama->finish_rows(ss, graphs[k], (size_t)n[k], outs[k], last[k] != 0);
        ss.tokens.insert(ss.tokens.end(), tk[k], tk[k] + n[k]);
        if (all_logits) outs[k].result.read_data(0, all_logits + row0 * V, (size_t)n[k] * V * sizeof(float));
        if (embeddings)
            ggml_hip_tensor_get(outs[k].embedding_result.ptr(), embeddings + k * E, (size_t)(n[k] - 1) * E * sizeof(float), E * sizeof(float));
        row0 += (size_t)n[k];
    }
    return true;
}
// what both calls ask of their sessions: B different whole-model sessions of m on the calling thread's slot, counts >= 1, room for
// them as llm_feed_prompt asks it, tokens inside the vocabulary; first[i]: where session i's tokens begin
bool pack_args_ok(const llm_model *m, llm_session *const *sessions, int B, const int32_t *tokens, const int32_t *counts, std::vector<size_t> &first) {
    if (!m || !sessions || !tokens || !counts || B < 1) return false;
    if (!m->stages.empty() || !m->llama->is_first() || !m->llama->is_last()) return false;
    const size_t V = m->llama->hyperparameters.n_vocab;
    first.assign((size_t)B, 0);
    size_t total = 0;
    for (int i = 0; i < B; i++) {
        const llm_session *s = sessions[i];
        if (!s || !s->s || s->model != m || !s->stage_sessions.empty() || s->device != ggml_hip_get_main_device() || counts[i] < 1) return false;
        for (int j = 0; j < i; j++)
            if (sessions[j] == s) return false;
        if (s->s->n_past + (size_t)counts[i] >= m->llama->params.context_size) return false;  // llm_feed_prompt's ContextFull
        first[(size_t)i] = total;
        total += (size_t)counts[i];
    }
    for (size_t t = 0; t < total; t++)
        if (tokens[t] < 0 || (size_t)tokens[t] >= V) return false;
    return true;
}
}  // namespace

extern "C" {
int llm_pack_schedule(const int32_t *counts, int B, int max_rows, int32_t *take_out) {
    if (!counts || B < 1 || max_rows < 0 || max_rows > PACK_ROWS_MAX) return -1;
    for (int i = 0; i < B; i++)
        if (counts[i] < 1) return -1;
    std::vector<int32_t> take;
    const int rounds = schedule(counts, B, max_rows ? max_rows : PACK_ROWS_DEFAULT, take_out ? &take : nullptr);
    if (take_out) std::copy(take.begin(), take.end(), take_out);
    return rounds;
}

// test hook: the session's graph for these n tokens at its n_past, built and not computed; the session does not move
struct ggml_cgraph *llm_session_stage_rows(llm_model *m, llm_session *s, const int32_t *tokens, int n) {
    if (!m || !s || !s->s || !tokens || n < 1 || !m->stages.empty()) return nullptr;
    llm::GraphOutputs out;
    return m->llama->stage_rows(*s->s, (const llm::TokenId *)tokens, (size_t)n, out);
}

// ONE evaluation of the entry over all B sessions' tokens, no rounds and no fallback (tests, tools): 0 = it ran, -1 = bad arguments, more
// than 64 sessions, or the entry declined — nothing moved.
int llm_prompt_pack_via(llm_pack_entry entry, llm_model *m, llm_session *const *sessions, int B, const int32_t *tokens, const int32_t *counts,
                        float *all_logits, float *embeddings) {
    std::vector<size_t> first;
    if (!entry || B > PACK_SESSIONS_MAX || !pack_args_ok(m, sessions, B, tokens, counts, first)) return -1;
    std::vector<int> who((size_t)B);
    std::vector<const int32_t *> tk((size_t)B);
    std::vector<int32_t> n(counts, counts + B);
    for (int i = 0; i < B; i++) {
        who[(size_t)i] = i;
        tk[(size_t)i] = tokens + first[(size_t)i];
    }
    return pack_once(entry, m, sessions, who, tk, n, std::vector<char>((size_t)B, 1), all_logits, embeddings) ? 0 : -1;
}

// Every round goes to `entry` as its sessions' graphs — one graph per session with rows in the round; a round of more than 64
// sessions goes in pieces of 64 in index order.  The session's own n_batch is not consulted: the round is the unit.  Once the entry
// declines (or there is none), that round's sessions and all later rounds are fed one by one through llm_feed_prompt, which chunks by
// n_batch as ever.
int llm_feed_prompt_batch_via(llm_pack_entry entry, llm_model *m, llm_session *const *sessions, int B, const int32_t *tokens,
                              const int32_t *counts, int max_rows) {
    std::vector<size_t> first;  // session i's tokens begin at tokens[first[i]]
    if (max_rows < 0 || max_rows > PACK_ROWS_MAX || !pack_args_ok(m, sessions, B, tokens, counts, first)) return -1;
    std::vector<int32_t> take;
    const int rounds = schedule(counts, B, max_rows ? max_rows : PACK_ROWS_DEFAULT, &take);
    std::vector<size_t> done((size_t)B, 0);
    for (int r = 0; r < rounds; r++) {
        const int32_t *row = take.data() + (size_t)r * B;
        for (int i0 = 0; i0 < B;) {  // pieces of at most 64 sessions with rows in this round
            std::vector<int> who;
            int i = i0;
            for (; i < B && (int)who.size() < PACK_SESSIONS_MAX; i++)
                if (row[i] > 0) who.push_back(i);
            i0 = i;
            if (who.empty()) continue;
            if (entry) {
                std::vector<const int32_t *> tk(who.size());
                std::vector<int32_t> n(who.size());
                std::vector<char> last(who.size());
                for (size_t k = 0; k < who.size(); k++) {
                    const int s = who[k];
                    tk[k] = tokens + first[(size_t)s] + done[(size_t)s];
                    n[k] = row[s];
                    last[k] = done[(size_t)s] + (size_t)row[s] == (size_t)counts[s];  // (as feed_prompt: only the last chunk's logits can be observed)
                }
                if (pack_once(entry, m, sessions, who, tk, n, last, nullptr, nullptr)) {
                    for (int s : who) done[(size_t)s] += (size_t)row[s];
                    continue;
                }
            }
            // declined (nothing was executed): this round's sessions and every later round's one by one — each session's remaining
            // tokens as ONE llm_feed_prompt call, so a call that never packs leaves exactly what llm_feed_prompt alone leaves
            for (int s = 0; s < B; s++)
                if (done[(size_t)s] < (size_t)counts[s])
                    llm_feed_prompt(m, sessions[s], tokens + first[(size_t)s] + done[(size_t)s], counts[s] - (int)done[(size_t)s]);
            return 0;
        }
    }
    return 1;
}
}
