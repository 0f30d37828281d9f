// llm_host.cpp — the core of the host mirror (its types: llm_session.hpp): Model::evaluate for whole and layer-split models, making
// and freeing models and sessions, llm_evaluate and llm_feed_prompt.  The loaders are llm_file.cpp, the token steps llm_infer.cpp,
// accessors, K/V, snapshots and test hooks llm_state.cpp.
#include "llm_session.hpp"

using namespace llm_host;

// (weak: this file also links against backends that have no such entry — the hint is then simply not given)
extern "C" void ggml_hip_expect_greedy_next(void) __attribute__((weak));

// May an evaluation of `len` tokens whose logits nobody looks at be only enqueued (InferenceSession::pipeline_chunk)?  Unsplit
// models, more than one token, LLM_HOST_PIPELINE_CHUNKS != 0: the one rule of llm_feed_prompt and llm_evaluate_flags.
bool llm_host::may_pipeline_chunk(const llm_model *m, size_t len) {
    static const bool pipeline_on = !(getenv("LLM_HOST_PIPELINE_CHUNKS") && atoi(getenv("LLM_HOST_PIPELINE_CHUNKS")) == 0);
    return pipeline_on && m->stages.empty() && len > 1;
}
// Model::evaluate for both kinds of model
void llm_host::model_evaluate(llm_model *m, llm_session *s, const std::vector<llm::TokenId> &toks, llm::OutputRequest &req) {
    HomeDevice hd;
    if (m->stages.empty()) {
        hd.go(s->device);  // the session's slot: the model's, or a sibling slot of the same GPU (llm_start_session_on)
        if (req.greedy_next && toks.size() == 1 && ggml_hip_expect_greedy_next) ggml_hip_expect_greedy_next();
        if (!m->llama->is_first() || !m->llama->is_last())  // one stage of a per-process split (llm_amd/pipeline.py)
            s->s->ensure_stage_rows(m->llama->hyperparameters.n_embd, toks.size());
        m->llama->evaluate(*s->s, toks, req);
        return;
    }
    const size_t G = m->stages.size();
    const size_t hop_bytes = (size_t)m->llama->hyperparameters.n_embd * toks.size() * sizeof(float);
    for (size_t i = 0; i < G; i++) {  // a call with more tokens than n_batch: the hand-off buffers grow to it first
        hd.go(m->devices[i]);
        s->stage_sessions[i]->ensure_stage_rows(m->llama->hyperparameters.n_embd, toks.size());
    }
    for (size_t i = 0; i < G; i++) {
        ggml_hip_bind_thread_device(m->devices[i]);
        llm::InferenceSession &ss = *s->stage_sessions[i];
        if (i > 0) {  // the residual [n_embd, N] f32 of the previous stage -> this stage's hand-off buffer, device to device
            void *dst = ggml_hip_tensor_device_ptr(ss.stage_in.ptr());
            ggml_hip_bind_thread_device(m->devices[i - 1]);
            const void *src = ggml_hip_tensor_device_ptr(s->stage_sessions[i - 1]->stage_out.ptr());
            ggml_hip_copy_between_devices(m->devices[i], dst, m->devices[i - 1], src, hop_bytes);
            ggml_hip_bind_thread_device(m->devices[i]);
        }
        llm::OutputRequest none;
        m->stages[i]->evaluate(ss, toks, i + 1 == G ? req : none);
    }
}

namespace {
std::atomic<int> g_split_sessions{0};  // live sessions of layer-split models (see llm_start_session)
// contiguous layer ranges for G stages in proportion to `split` (ggml's convention: device i takes split[i] / sum; all
// zero or NULL = equal shares); every stage gets at least one layer
std::vector<size_t> split_layers(size_t n_layer, int G, const float *split) {
    std::vector<double> w(G, 1.0);
    double sum = 0;
    bool any = false;
    for (int i = 0; i < G; i++) any = any || (split && split[i] > 0.0f);
    for (int i = 0; i < G; i++) {
        if (any) w[i] = std::max(0.0f, split[i]);
        sum += w[i];
    }
    std::vector<size_t> bounds(G + 1, 0);
    double acc = 0;
    for (int i = 0; i < G; i++) {
        acc += w[i];
        size_t b = (size_t)std::llround(acc / sum * (double)n_layer);
        b = std::max(b, bounds[i] + 1);                       // at least one layer per stage
        b = std::min(b, n_layer - (size_t)(G - 1 - i));       // ... and one left for each later stage
        bounds[i + 1] = b;
    }
    bounds[G] = n_layer;
    return bounds;
}
// InferenceSessionConfig of the C struct (NULL: the defaults)
llm::InferenceSessionConfig session_config(const llm_session_config *cfg) {
    llm::InferenceSessionConfig c;
    if (cfg) {
        c.memory_k_type = (ggml_type)cfg->memory_k_type;
        c.memory_v_type = (ggml_type)cfg->memory_v_type;
        c.n_batch = cfg->n_batch > 0 ? (size_t)cfg->n_batch : 8;
        c.n_threads = cfg->n_threads > 0 ? (size_t)cfg->n_threads : 8;
    }
    return c;
}
}  // namespace

// ---------------------------------------------------------------------------------------------------
// C entry points
// ---------------------------------------------------------------------------------------------------
extern "C" {

llm_model *llm_llama_new(const llm_llama_hparams *hp, const llm_model_params *mp, const llm_tensor_desc *tensors,
                         int n_tensors) {
    llm::Hyperparameters h;
    h.n_vocab = hp->n_vocab;
    h.n_embd = hp->n_embd;
    h.n_mult = hp->n_mult;
    h.n_head = hp->n_head;
    h.n_head_kv = hp->n_head_kv > 0 ? hp->n_head_kv : hp->n_head;
    h.n_layer = hp->n_layer;
    h.n_rot = hp->n_rot;
    h.file_type = hp->file_type;
    if (mp->n_gqa > 0 && h.n_layer >= 80) {  // models/llama/src/lib.rs:106-117: "temporary fix for 70B models"
        if (h.n_head % (size_t)mp->n_gqa != 0) ggml::panic("assuming 70B Llama2 model based on GQA == 8");  // the reference's assert_eq!
        h.n_head_kv = h.n_head / (size_t)mp->n_gqa;
    }
    llm::ModelParameters p;
    p.context_size = mp->context_size > 0 ? mp->context_size : 2048;
    p.use_gpu = mp->use_gpu != 0;
    p.gpu_layers = mp->gpu_layers;
    p.has_rope_overrides = mp->has_rope_overrides != 0;
    p.rope_overrides.frequency_scale = mp->rope_frequency_scale;
    p.rope_overrides.frequency_base = (size_t)mp->rope_frequency_base;
    p.layer_begin = mp->layer_begin > 0 ? (size_t)mp->layer_begin : 0;
    p.layer_end = mp->layer_end > 0 ? (size_t)mp->layer_end : (size_t)-1;
    if (!p.use_gpu) {
        fprintf(stderr, "llm_llama_new: use_gpu=0 requested, but libggml_hip has no CPU compute path\n");
        abort();
    }
    // Layer split inside this process: more than one device slot with a positive share in ggml_hip_set_layer_split (the
    // explicit-length sibling of the reference's split hook, crates/ggml/sys/src/cuda.rs:11, which itself carries ONE float:
    // accelerator/mod.rs:74-75), or GGML_HIP_LAYER_SPLIT=G for equal shares.
    // A caller that passes its own layer range (one process per GPU, llm_amd/pipeline.py) is left alone.
    std::vector<int> slots;     // the device slots that take part, in order
    std::vector<float> shares;  // their fractions (all zero = equal)
    {
        float split[16] = {0};
        const int nslot = std::min(ggml_hip_get_layer_split(split, 16), ggml_hip_device_count());
        for (int i = 0; i < nslot; i++)
            if (split[i] > 0.0f) {
                slots.push_back(i);
                shares.push_back(split[i]);
            }
        if (slots.size() < 2) {
            slots.clear();
            shares.clear();
            if (const char *v = getenv("GGML_HIP_LAYER_SPLIT"))
                for (int i = 0; i < std::min(atoi(v), ggml_hip_device_count()); i++) {
                    slots.push_back(i);
                    shares.push_back(0.0f);
                }
        }
    }
    const bool whole = p.layer_begin == 0 && p.layer_end >= (size_t)h.n_layer;  // the caller did not ask for a stage
    while (slots.size() > (size_t)h.n_layer) {
        slots.pop_back();
        shares.pop_back();
    }
    llm_model *m = new llm_model();
    if (slots.size() > 1 && whole) {
        const int G = (int)slots.size();
        const std::vector<size_t> bounds = split_layers(h.n_layer, G, shares.data());
        const int home = ggml_hip_get_main_device();
        for (int i = 0; i < G; i++) {
            llm::ModelParameters ps = p;
            ps.layer_begin = bounds[i];
            ps.layer_end = bounds[i + 1];
            ps.main_device = slots[i];
            ggml_hip_bind_thread_device(slots[i]);
            m->stages.push_back(new llm::Llama(h, ps, llm::TensorLoader(tensors, n_tensors)));
            m->devices.push_back(slots[i]);
        }
        ggml_hip_bind_thread_device(home);
        m->llama = m->stages.back();
        return m;
    }
    llm::TensorLoader tl(tensors, n_tensors);
    llm::ModelParameters pu = p;
    // a whole model made while a slot other than 0 is this thread's: its sessions stay on that slot (the reference's
    // InferenceSession::new always initialises device 0 — it knows one device)
    if (pu.main_device < 0 && m->device != 0) pu.main_device = m->device;
    m->llama = new llm::Llama(h, pu, std::move(tl));
    return m;
}
// The layer ranges an in-process split over G device slots gets for the fractions `split` (ggml_cuda_set_tensor_split's
// convention: slot i takes split[i] / sum; NULL or all zero = equal shares): bounds_out[0..G], stage i = layers
// [bounds_out[i], bounds_out[i+1]).  Pure host arithmetic (no device needed): what llm_llama_new applies.
void llm_split_layers(int n_layer, int G, const float *split, int *bounds_out) {
    const int Gu = std::max(1, std::min(G, n_layer));  // more slots than layers: the surplus slots get empty ranges at the end
    const std::vector<size_t> b = split_layers((size_t)std::max(1, n_layer), Gu, split);
    for (int i = 0; i <= G; i++) bounds_out[i] = i <= Gu ? (int)b[(size_t)i] : n_layer;
}
// the layer range and device slot of every stage of a model (1 entry for an unsplit one); returns the stage count
int llm_model_stages(const llm_model *m, int *layer_begin, int *layer_end, int *device, int cap) {
    if (m->stages.empty()) {
        if (cap > 0) {
            if (layer_begin) layer_begin[0] = (int)m->llama->params.layer_begin;
            if (layer_end) layer_end[0] = (int)std::min(m->llama->params.layer_end, m->llama->hyperparameters.n_layer);
            if (device) device[0] = m->device;
        }
        return 1;
    }
    for (size_t i = 0; i < m->stages.size() && (int)i < cap; i++) {
        if (layer_begin) layer_begin[i] = (int)m->stages[i]->params.layer_begin;
        if (layer_end) layer_end[i] = (int)m->stages[i]->params.layer_end;
        if (device) device[i] = m->devices[i];
    }
    return (int)m->stages.size();
}
void llm_model_free(llm_model *m) {
    if (!m) return;
    if (!m->stages.empty()) {
        const int home = ggml_hip_get_main_device();
        for (size_t i = 0; i < m->stages.size(); i++) {
            ggml_hip_bind_thread_device(m->devices[i]);
            delete m->stages[i];
        }
        ggml_hip_bind_thread_device(home);
        m->llama = nullptr;
    }
    if (m->llama) {
        HomeDevice hd;
        hd.go(m->device);
        delete m->llama;
    }
    if (m->file) llm_ggml_file_close(m->file);
    delete m;
}

llm_session *llm_start_session(llm_model *m, const llm_session_config *cfg) {
    const llm::InferenceSessionConfig c = session_config(cfg);
    llm_session *s = new llm_session();
    s->model = m;
    if (!m->stages.empty()) {
        const int home = ggml_hip_get_main_device();
        for (size_t i = 0; i < m->stages.size(); i++) {
            ggml_hip_bind_thread_device(m->devices[i]);
            s->stage_sessions.push_back(m->stages[i]->start_session(c));
        }
        ggml_hip_bind_thread_device(home);
        // the stages of ONE split session run one after the other: on a GPU that hosts several of them (virtual slots) they are one
        // sharer of its compute units, not G (the option set below); with a second split session alive they are not
        const bool only_split_session = g_split_sessions.fetch_add(1) == 0;
        ggml_hip_set_option("serial_stage_slots", only_split_session ? (int)m->stages.size() : 0);
        // ... and stages that share a physical GPU share its queue too: the residual then crosses a stage boundary inside one stream
        // instead of through an event of another queue (ggml_hip_share_stream; it declines slots of different GPUs)
        if (only_split_session)
            for (size_t i = 1; i < m->devices.size(); i++)
                for (size_t j = 0; j < i; j++)
                    if (ggml_hip_share_stream(m->devices[i], m->devices[j])) break;
        s->shares_streams = only_split_session;
        s->s = s->stage_sessions.back();
        s->devices = m->devices;
        return s;
    }
    HomeDevice hd;
    hd.go(m->device);
    s->device = m->device;
    struct AfterNew {  // GGML_HIP_SESSION_SLOTS: the backend may have assigned this thread a sibling slot while the K/V memory was created
        llm_session *s;
        ~AfterNew() {
            if (s->s && ggml_hip_thread_session_slot() >= 0) s->device = ggml_hip_thread_session_slot();
        }
    } after_new{s};
    s->s = m->llama->start_session(c);
    return s;
}
// Several sessions of ONE model on one GPU (crates/llm-base/src/inference_session.rs:43-48: a session is Send;
// model/mod.rs:275-276: "spawn several sessions for one model"): every session gets its own device SLOT on the model's GPU — its
// own stream, arena shadows, K/V memory, plan cache and workspace — and reads the model's weights where the model's slot put them
// (slots of one physical device may read each other's weights, backend_state.inc extra_of).  Sessions on different slots run
// concurrently (per-slot locks; the host arenas are an event log, no cross-slot locking per token), so two decode streams fill
// each other's kernel-boundary and latency gaps.  `slot` must drive the same physical device as the model's slot
// (GGML_HIP_VIRTUAL_DEVICES=n provides n slots on a 1-GPU box; slot = -1: the model's own).  Unsplit models only.
llm_session *llm_start_session_on(llm_model *m, const llm_session_config *cfg, int slot) {
    if (slot < 0 || !m->stages.empty() || slot == m->device) return llm_start_session(m, cfg);
    // a sibling slot reads the model's ONE copy of the weights: it must drive the GPU that holds them (checked here, before any
    // K/V memory is allocated on the wrong one; the backend would only notice at the first evaluation)
    if (ggml_hip_slot_physical_device(slot) < 0 || ggml_hip_slot_physical_device(slot) != ggml_hip_slot_physical_device(m->device)) {
        fprintf(stderr, "llm_start_session_on: slot %d does not drive the GPU of the model's slot %d\n", slot, m->device);
        return nullptr;
    }
    llm_session *s = new llm_session();
    s->model = m;
    HomeDevice hd;
    hd.go(slot);
    s->device = slot;
    s->s = m->llama->start_session(session_config(cfg), slot);
    return s;
}
// test / restore hook: the session continues at position n_past (what InferenceSession::from_snapshot does with the snapshot's
// npast, inference_session.rs:640) — the caller has put the K/V of the positions before it in place (llm_session_kv)
void llm_session_seek(llm_session *s, int n_past) {
    s->s->n_past = (size_t)n_past;
    for (auto *st : s->stage_sessions) st->n_past = (size_t)n_past;
    s->s->drop_prebuilt();
}
// 0 = the reference's own call sequence inside InferenceSession::compute (build the graph, then ggml_graph_compute, synchronously:
// inference_session.rs:220-295); 1 (default; env LLM_HOST_SPECULATE) = the patched sequence that builds the NEXT token's graph
// between ggml_hip_graph_compute_begin / _end while the device runs
void llm_session_set_speculate(llm_session *s, int on) {
    s->s->speculate = on != 0;
    for (auto *st : s->stage_sessions) st->speculate = on != 0;
    s->s->drop_prebuilt();
}
void llm_session_free(llm_session *s) {
    if (!s) return;
    if (!s->stage_sessions.empty()) {
        const int home = ggml_hip_get_main_device();
        for (size_t i = 0; i < s->stage_sessions.size(); i++) {
            ggml_hip_bind_thread_device(s->devices[i]);
            delete s->stage_sessions[i];
        }
        ggml_hip_bind_thread_device(home);
        s->s = nullptr;
        if (s->shares_streams)
            for (size_t i = 1; i < s->devices.size(); i++) ggml_hip_share_stream(s->devices[i], -1);
        g_split_sessions.fetch_sub(1);
        ggml_hip_set_option("serial_stage_slots", 0);
    }
    if (s->s) {
        HomeDevice hd;
        hd.go(s->device);
        delete s->s;
    }
    delete s;
}
void llm_evaluate(llm_model *m, llm_session *s, const int32_t *tokens, int n, float *all_logits, float *embeddings) {
    std::vector<llm::TokenId> toks(tokens, tokens + n);
    std::vector<float> logits, emb;
    llm::OutputRequest req;
    if (all_logits) req.all_logits = &logits;
    if (embeddings) req.embeddings = &emb;
    model_evaluate(m, s, toks, req);
    if (all_logits) memcpy(all_logits, logits.data(), logits.size() * sizeof(float));
    if (embeddings) memcpy(embeddings, emb.data(), emb.size() * sizeof(float));
}
void llm_feed_prompt(llm_model *m, llm_session *s, const int32_t *tokens, int n) {
    // inference_session.rs:311-316: ContextFull check, then chunks(n_batch)
    if (s->s->n_past + (size_t)n >= m->llama->params.context_size) {
        fprintf(stderr, "llm_feed_prompt: InferenceError::ContextFull\n");
        abort();
    }
    const size_t nb = s->s->config.n_batch;
    for (size_t i = 0; i < (size_t)n; i += nb) {
        const size_t len = std::min(nb, (size_t)n - i);
        std::vector<llm::TokenId> batch(tokens + i, tokens + i + len);
        // every chunk but the last is only enqueued (unsplit models): the host builds and matches the next chunk's graph while the
        // device runs this one, instead of waiting for it and for a row of logits nobody can see
        llm::OutputRequest req;
        const bool more = i + len < (size_t)n && may_pipeline_chunk(m, len);
        req.intermediate_chunk = more;
        s->s->pipeline_chunk = more;
        model_evaluate(m, s, batch, req);
        s->s->pipeline_chunk = false;
        for (auto tk : batch) s->s->tokens.push_back(tk);
    }
}

}  // extern "C"
