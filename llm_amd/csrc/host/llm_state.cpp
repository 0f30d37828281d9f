// llm_state.cpp — what a caller reads from and writes to a session of the host mirror besides evaluating it: timers and accessors,
// rewind, the layer-split hand-off buffers, K/V in and out, snapshots (inference_session.rs:590-646), reads of graph nodes (test
// hooks), the device top-k, the entry points InferenceSession::perplexity (llm_perplexity.cpp) is written over, device scopes.
#include "llm_session.hpp"

using namespace llm_host;

// InferenceSession::get_snapshot / from_snapshot (inference_session.rs:590-646): npast, config, tokens, last_logits,
// memory_k, memory_v.  The reference serialises the struct with serde/bincode; without a Rust toolchain the byte
// format here is our own (little-endian header + the four payloads), the CONTENT is the reference's.  The K/V memory
// lives on the device, so both directions go through the backend (ggml_hip_tensor_get / _set).
namespace {
struct SnapHeader {
    char magic[8];  // "LLMSNAP1"
    uint64_t npast, n_tokens, n_logits, k_bytes, v_bytes;
    int32_t memory_k_type, memory_v_type, n_batch, n_threads;
};
}  // namespace

extern "C" {

// Accumulated host nanoseconds per phase (see InferenceSession::host_ns; [5] greedy argmax, [6] evaluate as a whole);
// reset != 0 clears the accumulators after the read.
void llm_host_timing(double *out8, int reset) {
    for (int i = 0; i < 8; i++) out8[i] = (double)llm::InferenceSession::host_ns[i].load(std::memory_order_relaxed);
    if (reset) for (int i = 0; i < 8; i++) llm::InferenceSession::host_ns[i].store(0, std::memory_order_relaxed);
}
int llm_session_rewind(llm_session *s, int num) {
    if ((size_t)num >= s->s->n_past) return -1;  // RewindError::NotEnoughTokens
    if ((size_t)num <= s->s->tokens.size()) s->s->tokens.resize(s->s->tokens.size() - (size_t)num);
    s->s->n_past -= (size_t)num;
    for (size_t i = 0; i + 1 < s->stage_sessions.size(); i++) s->stage_sessions[i]->n_past -= (size_t)num;
    return 0;
}
const float *llm_session_last_logits(const llm_session *s) { return s->s->last_logits.data(); }
int llm_session_n_past(const llm_session *s) { return (int)s->s->n_past; }
int llm_model_n_vocab(const llm_model *m) { return (int)m->llama->hyperparameters.n_vocab; }
int llm_model_context_size(const llm_model *m) { return (int)m->llama->params.context_size; }
int llm_session_n_batch(const llm_session *s) { return (int)s->s->config.n_batch; }
void llm_session_last_graph_stats(const llm_session *s, int *n_nodes, int *n_leafs) {
    if (n_nodes) *n_nodes = s->s->last_n_nodes;
    if (n_leafs) *n_leafs = s->s->last_n_leafs;
}

// Device addresses of the layer-split hand-off buffers of a session (NULL when the stage has none): the residual
// [n_embd * n_tokens] f32 is received into *in_dev before llm_evaluate and is in *out_dev after it.
void llm_session_stage_buffers(llm_session *s, void **in_dev, void **out_dev, size_t *nbytes) {
    HomeDevice hd;
    if (s->stage_sessions.empty()) hd.go(s->device);
    if (in_dev) *in_dev = s->s->stage_in.is_null() ? nullptr : ggml_hip_tensor_device_ptr(s->s->stage_in.ptr());
    if (out_dev) *out_dev = s->s->stage_out.is_null() ? nullptr : ggml_hip_tensor_device_ptr(s->s->stage_out.ptr());
    if (nbytes) *nbytes = !s->s->stage_in.is_null() ? s->s->stage_in.nbytes() : !s->s->stage_out.is_null() ? s->s->stage_out.nbytes() : 0;
}

// Session K/V memory as raw bytes (which: 0 = memory_k, 1 = memory_v) — the payload of the reference's
// InferenceSnapshot (inference_session.rs:599-646), which reads `memory_k.data()` on the host; here the
// authoritative copy lives on the device, so the snapshot goes through the backend.  set=0 reads, set=1 writes.
size_t llm_session_kv(llm_session *s, int which, int set, void *buf, size_t nbytes) {
    if (!s->stage_sessions.empty()) {  // the stages' caches in layer order = the whole model's layout (layer-major)
        size_t total = 0, off = 0;
        for (auto *ss : s->stage_sessions) total += (which == 0 ? ss->memory_k : ss->memory_v).nbytes();
        if (!buf) return total;
        const int home = ggml_hip_get_main_device();
        for (size_t i = 0; i < s->stage_sessions.size() && off < nbytes; i++) {
            ggml::Tensor &t = which == 0 ? s->stage_sessions[i]->memory_k : s->stage_sessions[i]->memory_v;
            const size_t n = std::min(t.nbytes(), nbytes - off);
            ggml_hip_bind_thread_device(s->devices[i]);
            if (set)
                ggml_hip_tensor_set(t.ptr(), (char *)buf + off, 0, n);
            else
                ggml_hip_tensor_get(t.ptr(), (char *)buf + off, 0, n);
            off += n;
        }
        ggml_hip_bind_thread_device(home);
        return off;
    }
    ggml::Tensor &t = which == 0 ? s->s->memory_k : s->s->memory_v;
    const size_t n = t.nbytes();
    if (!buf) return n;
    if (nbytes > n) nbytes = n;
    HomeDevice hd;
    hd.go(s->device);
    if (set)
        ggml_hip_tensor_set(t.ptr(), buf, 0, nbytes);
    else
        ggml_hip_tensor_get(t.ptr(), buf, 0, nbytes);
    return nbytes;
}

size_t llm_session_snapshot(llm_session *s, void *buf, size_t cap) {
    llm::InferenceSession &ss = *s->s;
    SnapHeader h;
    memcpy(h.magic, "LLMSNAP1", 8);
    h.npast = ss.n_past;
    h.n_tokens = ss.tokens.size();
    h.n_logits = ss.last_logits.size();
    // a session split over device slots holds one K/V cache per stage: concatenated in layer order they ARE the unsplit
    // layout (llm_session_kv), so a snapshot does not depend on how the model was split when it was taken
    h.k_bytes = llm_session_kv(s, 0, 0, nullptr, 0);
    h.v_bytes = llm_session_kv(s, 1, 0, nullptr, 0);
    h.memory_k_type = (int32_t)ss.config.memory_k_type;
    h.memory_v_type = (int32_t)ss.config.memory_v_type;
    h.n_batch = (int32_t)ss.config.n_batch;
    h.n_threads = (int32_t)ss.config.n_threads;
    const size_t need = sizeof(h) + h.n_tokens * 4 + h.n_logits * 4 + h.k_bytes + h.v_bytes;
    if (!buf || cap < need) return need;
    char *p = (char *)buf;
    memcpy(p, &h, sizeof(h));
    p += sizeof(h);
    memcpy(p, ss.tokens.data(), h.n_tokens * 4);
    p += h.n_tokens * 4;
    memcpy(p, ss.last_logits.data(), h.n_logits * 4);
    p += h.n_logits * 4;
    llm_session_kv(s, 0, 0, p, h.k_bytes);
    p += h.k_bytes;
    llm_session_kv(s, 1, 0, p, h.v_bytes);
    return need;
}
// NULL = SnapshotError (bad header, or MemorySizeMismatch: the model's session has other K/V sizes than the snapshot)
llm_session *llm_session_from_snapshot(llm_model *m, const void *buf, size_t n) {
    SnapHeader h;
    if (!buf || n < sizeof(h)) return nullptr;
    memcpy(&h, buf, sizeof(h));
    if (memcmp(h.magic, "LLMSNAP1", 8) != 0) return nullptr;
    if (n != sizeof(h) + h.n_tokens * 4 + h.n_logits * 4 + h.k_bytes + h.v_bytes) return nullptr;
    llm_session_config cfg{h.memory_k_type, h.memory_v_type, h.n_batch, h.n_threads};
    llm_session *s = llm_start_session(m, &cfg);
    llm::InferenceSession &ss = *s->s;
    if (llm_session_kv(s, 0, 0, nullptr, 0) != h.k_bytes || llm_session_kv(s, 1, 0, nullptr, 0) != h.v_bytes ||
        ss.last_logits.size() != h.n_logits) {
        llm_session_free(s);
        return nullptr;  // SnapshotError::MemorySizeMismatch
    }
    const char *p = (const char *)buf + sizeof(h);
    ss.tokens.assign((const llm::TokenId *)p, (const llm::TokenId *)p + h.n_tokens);
    p += h.n_tokens * 4;
    memcpy(ss.last_logits.data(), p, h.n_logits * 4);
    p += h.n_logits * 4;
    llm_session_kv(s, 0, 1, (void *)p, h.k_bytes);
    p += h.k_bytes;
    llm_session_kv(s, 1, 1, (void *)p, h.v_bytes);
    ss.n_past = h.npast;
    for (auto *st : s->stage_sessions) st->n_past = h.npast;  // every stage of a split session is at the same position
    return s;
}

// test hook: device contents of a node of the last evaluated graph, by index (>= 0) or by the k-th node
// carrying `name` (index < 0).  Returns the number of bytes the node holds, 0 if not found.
size_t llm_session_read_node(const llm_session *s, int index, const char *name, int occurrence, void *dst,
                             size_t max_bytes) {
    ggml_cgraph *g = s->s->last_graph;
    if (!g) return 0;
    ggml_tensor *t = nullptr;
    if (index >= 0) {
        if (index < g->n_nodes) t = g->nodes[index];
    } else {
        int seen = 0;
        for (int i = 0; i < g->n_nodes && !t; i++)
            if (strcmp(g->nodes[i]->name, name) == 0 && seen++ == occurrence) t = g->nodes[i];
    }
    if (!t || !ggml_is_contiguous(t)) return 0;
    const size_t n = ggml_nbytes(t);
    HomeDevice hd;
    hd.go(s->stage_sessions.empty() ? s->device : s->devices.back());
    if (dst && n <= max_bytes) ggml_hip_tensor_get(t, dst, 0, n);
    return n;
}

// test hook: the HOST bytes of node `n_nodes - 1 - from_end` of the last evaluated graph (what an unchanged caller that reads
// tensor->data sees; from_end = 1 is the embedding_result node of the LLaMA graph, models/llama/src/lib.rs:343-347)
size_t llm_session_read_node_host(const llm_session *s, int from_end, void *dst, size_t max_bytes) {
    ggml_cgraph *g = s->s->last_graph;
    if (!g || from_end < 0 || from_end >= g->n_nodes) return 0;
    ggml_tensor *t = g->nodes[g->n_nodes - 1 - from_end];
    const size_t n = ggml_nbytes(t);
    if (dst && n <= max_bytes && t->data) memcpy(dst, t->data, n);
    return n;
}

// The k best logits of the last evaluated token without reading n_vocab floats back (ggml_hip_topk on the logits node of
// the last graph = its last node, last row): what the sampler chain's top-k stage needs (samplers.rs:289-306).
// `extra_ids`: tokens whose raw logits the caller wants too (repetition-penalty window, bias list).  0 on success.
int llm_session_topk(const llm_session *s, int k, const int32_t *extra_ids, int n_extra, float *out_vals, int32_t *out_ids) {
    int slot = 0;
    const ggml_tensor *t = llm_session_logits_node(s, &slot);
    if (!t) return -1;
    HomeDevice hd;
    hd.go(slot);
    return ggml_hip_topk(t, t->ne[1] - 1, k, extra_ids, n_extra, out_vals, out_ids);
}

// ---- what InferenceSession::perplexity (host/llm_perplexity.cpp) is written over ----
// Model::evaluate with the two extensions of OutputRequest spelled out.  flags & 1: logits_on_device (the [n_vocab, n] logits
// stay in HBM, last_logits is not refreshed); flags & 2: intermediate_chunk (nobody looks at this evaluation's logits before the
// next one: it is only enqueued where feed_prompt would do so: unsplit model, more than one token).  all_logits: nullable.
void llm_evaluate_flags(llm_model *m, llm_session *s, const int32_t *tokens, int n, int flags, float *all_logits) {
    std::vector<llm::TokenId> toks(tokens, tokens + n);
    std::vector<float> logits;
    llm::OutputRequest req;
    if (all_logits) req.all_logits = &logits;
    req.logits_on_device = (flags & 1) != 0;
    const bool more = (flags & 2) != 0 && !all_logits && may_pipeline_chunk(m, (size_t)n);
    req.intermediate_chunk = more;
    s->s->pipeline_chunk = more;
    model_evaluate(m, s, toks, req);
    s->s->pipeline_chunk = false;
    if (all_logits) memcpy(all_logits, logits.data(), logits.size() * sizeof(float));
}
// The logits node of the last evaluated graph (its last node: [n_vocab, n] f32) and the device slot that owns it (the last
// stage's for a layer-split model); NULL if there is no evaluated graph.
const struct ggml_tensor *llm_session_logits_node(const llm_session *s, int *device_slot) {
    ggml_cgraph *g = s->s->last_graph;
    if (!g || g->n_nodes < 1) return nullptr;
    const ggml_tensor *t = g->nodes[g->n_nodes - 1];
    if (t->type != GGML_TYPE_F32 || (size_t)t->ne[0] != s->s->last_logits.size()) return nullptr;
    if (device_slot) *device_slot = s->stage_sessions.empty() ? s->device : s->devices.back();
    return t;
}
// common::read_last_token (model/common.rs:6-19) for an evaluation that left its logits on the device: the last row of the
// logits node -> last_logits (n_vocab floats).  0, or -1 if there is no evaluated graph.
int llm_session_fetch_last_logits(llm_session *s) {
    int slot = 0;
    const ggml_tensor *t = llm_session_logits_node(s, &slot);
    if (!t) return -1;
    HomeDevice hd;
    hd.go(slot);
    const size_t row = (size_t)t->ne[0] * sizeof(float);
    ggml_hip_tensor_get(t, s->s->last_logits.data(), row * (size_t)(t->ne[1] - 1), row);
    return 0;
}
// HomeDevice for callers that do not see the mirror's types: the thread goes to device slot `slot` until the scope is closed,
// which leaves the caller's main device as it was found.  Scopes nest; close them in reverse order.
llm_device_scope *llm_device_scope_open(int slot) {
    HomeDevice *hd = new HomeDevice();
    hd->go(slot);
    return reinterpret_cast<llm_device_scope *>(hd);
}
void llm_device_scope_close(llm_device_scope *scope) { delete reinterpret_cast<HomeDevice *>(scope); }

}  // extern "C"
