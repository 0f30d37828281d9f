// llm_session.hpp — the types of the host mirror, shared by its translation units (internal: nothing here is exported; the C
// entry points are llm_host.h's).  C++ mirror of the host code on the hot path of rustformers/llm:
//   crates/llm-base/src/inference_session.rs  InferenceSession {new, compute, feed_prompt,
//                                              infer_next_token, rewind}            (:114-424)
//   crates/llm-base/src/model/{mod,common}.rs  ModelParameters, OutputRequest, read_last_token …
//   crates/models/llama/src/lib.rs             Llama {new, start_session, evaluate}  (:43-368)
// The reference is Rust and no Rust toolchain exists in this image; this file keeps its structure,
// names and call order so that the graph handed to ggml_graph_compute is node-for-node the graph the
// Rust code builds (tests/test_llama_gpu.py counts the nodes).  All compute goes through the C ABI
// of include/ggml_hip.h.
//   llm_host.cpp   Model::evaluate for whole and layer-split models, models and sessions, llm_evaluate, llm_feed_prompt
//   llm_file.cpp   the GGML / GGMF / GGJT container reader, llm_llama_load, the LoRA loader
//   llm_infer.cpp  the token steps: greedy, top-k, the device chains, the batched steps and chains, llm_sample_exact
//   llm_state.cpp  accessors, K/V in and out, snapshots, node reads, what llm_perplexity.cpp needs, device scopes
#pragma once
#include "llm_host.h"

#include <algorithm>
#include <atomic>
#include <chrono>

#include <cmath>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "ggml_wrap.hpp"

namespace llm {

using ggml::Backend;
using ggml::Buffer;
using ggml::ComputationGraph;
using ggml::Context;
using ggml::GraphExecutionPlan;
using ggml::Tensor;

using TokenId = int32_t;

// crates/llm-base/src/model/mod.rs:196-251
struct ModelParameters {
    size_t context_size = 2048;
    bool use_gpu = false;
    long gpu_layers = -1;  // None
    bool has_rope_overrides = false;
    ggml::RoPEOverrides rope_overrides;
    long n_gqa = -1;
    // layer-split extension: this process owns layers [layer_begin, layer_end)
    size_t layer_begin = 0, layer_end = (size_t)-1;
    int main_device = -1;  // >= 0: a stage of an in-process layer split, bound to this device slot

    bool should_offload(size_t layer) const {
        if (!use_gpu) return false;
        return gpu_layers < 0 ? true : (long)layer < gpu_layers;
    }
    Backend backend(size_t layer) const { return should_offload(layer) ? Backend::Gpu : Backend::Cpu; }
};

// crates/llm-base/src/inference_session.rs:799-841
struct InferenceSessionConfig {
    ggml::Type memory_k_type = GGML_TYPE_F16;
    ggml::Type memory_v_type = GGML_TYPE_F16;
    size_t n_batch = 8;
    size_t n_threads = 8;
};

// crates/llm-base/src/model/mod.rs:257-266
struct OutputRequest {
    std::vector<float> *all_logits = nullptr;
    std::vector<float> *embeddings = nullptr;
    // extension (no reference counterpart): the caller samples from a device-side top-k (llm_session_topk) — the logits node stays
    // in HBM like every other node and last_logits is NOT refreshed: 40 pairs cross the bus instead of n_vocab floats
    bool logits_on_device = false;
    // extension: a chunk of feed_prompt that is not its last one — nobody can observe its last-token logits (the next chunk
    // overwrites last_logits before feed_prompt returns), so they are not fetched and the evaluation need not be waited for
    bool intermediate_chunk = false;
    // extension: the caller is greedy by construction — its next evaluation will be of the first maximum of this one's logits
    // (llm_infer_next_token_greedy): handed to the backend as ggml_hip_expect_greedy_next before the graph is computed
    bool greedy_next = false;
};

struct GraphOutputs {  // inference_session.rs:31-37
    Tensor result;
    Tensor embedding_result;
};

constexpr size_t SCRATCH_SIZE = 512ull * 1024 * 1024;  // inference_session.rs:19

struct BuildContext {  // inference_session.rs:96-109
    Context *ctx0;
    const Tensor *embd;
    const Tensor *memory_k;
    const Tensor *memory_v;
    const std::shared_ptr<Buffer> *scratch;
    const Buffer *get_scratch(size_t idx) const { return scratch[idx].get(); }
};

class InferenceSession {
   public:
    // inference_session.rs:114-217
    InferenceSession(const InferenceSessionConfig &config, const ModelParameters &params, size_t n_layer,
                     size_t n_embd, size_t n_vocab)
        : config(config), n_embd_(n_embd) {
        const size_t context_size = params.context_size;
        const size_t context_byte_size = [&] {
            double size = 0;
            size += (double)context_size * (double)n_layer * (double)n_embd * (double)ggml_type_sizef(config.memory_k_type);
            size += (double)context_size * (double)n_layer * (double)n_embd * (double)ggml_type_sizef(config.memory_v_type);
            return (size_t)size + (5 + 10 * n_layer) * 256;  // object overhead
        }();
        if (params.use_gpu) {
            // inference_session.rs: ggml::accelerator::initialize(0).  A stage of an in-process layer split lives on its
            // own device slot, which llm_start_session made current: it must stay current (and the caller's split stay set)
            if (params.main_device < 0) ggml::accelerator::initialize(0);
            ggml::accelerator::set_scratch_size(config.n_batch * 1024 * 1024);
        }
        session_ctx_ = std::make_shared<Context>(Context::new_with_allocate(context_byte_size));
        memory_size_ = context_byte_size;
        // Initialize key + value memory tensors (kv_memory, inference_session.rs:996-1021)
        const size_t n_mem = n_layer * context_size;
        const size_t n_elements = n_embd * n_mem;
        memory_k = session_ctx_->new_tensor_1d(config.memory_k_type, n_elements).set_name("memory_k");
        memory_v = session_ctx_->new_tensor_1d(config.memory_v_type, n_elements).set_name("memory_v");
        if (params.use_gpu) {
            memory_k.offload_no_scratch();
            memory_v.offload_no_scratch();
        }
        scratch_[0] = std::make_shared<Buffer>(SCRATCH_SIZE);
        scratch_[1] = std::make_shared<Buffer>(SCRATCH_SIZE);
        const size_t buf_size_mb = n_layer >= 80 ? 1536 : n_layer >= 60 ? 1280 : 1024;
        const size_t buf_size = buf_size_mb * 1024 * 1024 + ggml_graph_overhead();
        ctx0_[0] = Context::new_with_buffer(std::make_shared<Buffer>(buf_size));
        ctx0_[1] = Context::new_with_buffer(std::make_shared<Buffer>(buf_size));
        if (const char *v = getenv("LLM_HOST_SPECULATE")) speculate = atoi(v) != 0;
        last_logits.assign(n_vocab, 0.0f);
    }
    ~InferenceSession() {
        // inference_session.rs:659-665: free accelerator scratch; K/V are freed by the session ctx destructor
        ggml::accelerator::free_scratch();
    }

    using Builder = std::function<std::pair<ComputationGraph, GraphOutputs>(BuildContext &)>;
    // host time per phase of compute(), ns, accumulated (llm_host_timing): [0] adopt/build, [1] token write + plan,
    // [2] begin (match + enqueue), [3] speculative build of the next graph, [4] end (wait + result copy)
    // (process-wide and updated by every session thread: relaxed atomics — a statistic, but not a data race;
    //  static inline: one set of timers however many translation units include this header)
    static inline std::atomic<int64_t> host_ns[8] = {};
    static inline void host_ns_add(int k, double ns) { host_ns[k].fetch_add((int64_t)ns, std::memory_order_relaxed); }
    static inline double now_ns() {
        return (double)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
    }

    // inference_session.rs:220-295.  `next_builder` (optional) is a host-side latency optimisation that does not
    // change what is computed: while the device runs a single-token graph, the graph of the NEXT single-token call
    // (same session, n_past + 1) is built into the other of two ctx0 arenas; the following compute() adopts it if
    // the session is where the speculation assumed (otherwise it is discarded and the graph is built as usual).
    // The reference rebuilds the graph inside every evaluate; this hides that cost behind the device.
    GraphOutputs compute(const std::vector<TokenId> &input_tokens, const Builder &builder,
                         const std::function<Builder(size_t /*session_len*/)> &next_builder = nullptr,
                         const void *model_key = nullptr, size_t context_size = 0) {
        const bool single = input_tokens.size() == 1;
        double t0 = now_ns(), t1;
        auto lap = [&](int k) { t1 = now_ns(); host_ns_add(k, t1 - t0); t0 = t1; };
        Built built;
        if (single && pre_.valid && pre_.n_past == n_past && pre_.model_key == model_key) {
            cur_ = pre_.slot;  // adopt the speculatively built graph
            built = std::move(pre_.b);
        } else {
            cur_ ^= 1;
            built = build_into(cur_, input_tokens.size(), builder);
        }
        pre_.valid = false;
        lap(0);
        Context &ctx0 = ctx0_[cur_];
        built.embd.write_data(input_tokens.data(), input_tokens.size() * sizeof(TokenId));  // Write input tokens
        {
            GraphExecutionPlan plan(built.gf, config.n_threads);
            lap(1);
            // (pipeline_chunk: a chunk of feed_prompt behind which another one follows at once — begin without end: the next
            //  evaluation's begin, or any other entry point of the backend, completes it; the stream keeps the order)
            const bool pipe = !single && pipeline_chunk && speculate && !defer_end;
            const bool running = (single && speculate) || pipe ? plan.execute_begin(ctx0) : (plan.execute(ctx0), false);
            lap(2);
            if (running && next_builder && n_past + 2 <= context_size) {
                pre_.b = build_into(cur_ ^ 1, 1, next_builder(n_past + 1));
                pre_.slot = cur_ ^ 1;
                pre_.n_past = n_past + 1;
                pre_.model_key = model_key;
                pre_.valid = true;
                GraphExecutionPlan::prepare(pre_.b.gf);
            }
            lap(3);
            // a middle stage of an in-process layer split has nothing for the host to read: its wait is left to the slot's next
            // begin (finish_pending), so the host goes straight on to enqueue the next stage while this one runs
            if (single && speculate && !defer_end) GraphExecutionPlan::execute_end();
            lap(4);
        }
        last_n_nodes = built.gf.raw()->n_nodes;
        last_n_leafs = built.gf.raw()->n_leafs;
        last_graph = built.gf.raw();  // lives in its ctx0 arena until that arena is recreated
        if (mem_per_token == 0) mem_per_token = ctx0.used_mem() / n_embd_;
        n_past += input_tokens.size();
        return GraphOutputs{built.out.result.share(), built.out.embedding_result.share()};
    }

    // n tokens were decoded on the device behind this session's back (ggml_hip_decode_greedy_chain): the K/V memory
    // holds them; bring the bookkeeping of inference_session.rs (n_past, tokens) in line.
    void advance_device_chain(const TokenId *toks, size_t n) {
        tokens.insert(tokens.end(), toks, toks + n);
        n_past += n;
        pre_.valid = false;  // the speculatively built graph assumed n_past + 1
        last_graph = nullptr;
    }

    // Batched decode (llm_evaluate_batch): the session's single-token graph for `tok` at n_past, built as compute() builds it and
    // its token written, but not computed — the caller hands the graphs of several sessions to the backend together.  No
    // speculative build of the next graph.  The graph lives in its ctx0 arena until that arena is recreated.
    ggml_cgraph *stage_single(TokenId tok, const Builder &builder, GraphOutputs &out) {
        pre_.valid = false;
        cur_ ^= 1;
        Built built = build_into(cur_, 1, builder);
        built.embd.write_data(&tok, sizeof(TokenId));
        out = GraphOutputs{built.out.result.share(), built.out.embedding_result.share()};
        return built.gf.raw();
    }
    // ... and compute()'s bookkeeping once that graph has run
    void commit_single(ggml_cgraph *gr) {
        last_n_nodes = gr->n_nodes;
        last_n_leafs = gr->n_leafs;
        last_graph = gr;
        if (mem_per_token == 0) mem_per_token = ctx0_[cur_].used_mem() / n_embd_;
        n_past += 1;
    }

    // The packed prompt batch (llm_feed_prompt_batch): the session's graph for `n` tokens at n_past, built as compute() builds it and its
    // tokens written, but not computed; commit_rows is compute()'s bookkeeping once a backend entry has run it.
    ggml_cgraph *stage_rows(const TokenId *toks, size_t n, const Builder &builder, GraphOutputs &out) {
        pre_.valid = false;
        cur_ ^= 1;
        Built built = build_into(cur_, n, builder);
        built.embd.write_data(toks, n * sizeof(TokenId));
        out = GraphOutputs{built.out.result.share(), built.out.embedding_result.share()};
        return built.gf.raw();
    }
    void commit_rows(ggml_cgraph *gr, size_t n) {
        last_n_nodes = gr->n_nodes;
        last_n_leafs = gr->n_leafs;
        last_graph = gr;
        if (mem_per_token == 0) mem_per_token = ctx0_[cur_].used_mem() / n_embd_;
        n_past += n;
    }

    void drop_prebuilt() {  // a speculatively built next-token graph no longer describes the session's next call
        pre_.valid = false;
        last_graph = nullptr;
    }

    // hand-off buffers of a layer-split stage: n_embd * rows floats each, rows = n_batch to begin with.  Model::evaluate may
    // be called with more tokens than n_batch (an unsplit model takes any count): the buffers then grow to that count
    // (ensure_stage_rows, called by the graph builder before it makes its views).
    void make_stage_buffers(size_t n_embd, bool in, bool out, size_t rows = 0) {
        if (rows == 0) rows = config.n_batch;
        stage_in = Tensor();
        stage_out = Tensor();
        stage_ctx_.reset();  // drops the old buffers' device copies (Context drop frees offloaded tensors)
        stage_ctx_ = std::make_shared<Context>(Context::new_with_allocate(2 * (n_embd * rows * 4 + 1024)));
        if (in) {
            stage_in = stage_ctx_->new_tensor_1d(GGML_TYPE_F32, n_embd * rows).set_name("stage_in");
            stage_in.offload_no_scratch();
        }
        if (out) {
            stage_out = stage_ctx_->new_tensor_1d(GGML_TYPE_F32, n_embd * rows).set_name("stage_out");
            stage_out.offload_no_scratch();
        }
        stage_rows_ = rows;
        stage_has_in_ = in;
        stage_has_out_ = out;
    }
    void ensure_stage_rows(size_t n_embd, size_t rows) {
        if (rows <= stage_rows_) return;
        pre_.valid = false;  // a speculatively built graph holds views of the old buffers
        make_stage_buffers(n_embd, stage_has_in_, stage_has_out_, rows);
    }
    size_t stage_rows() const { return stage_rows_; }

    InferenceSessionConfig config;
    Tensor memory_k, memory_v;
    Tensor stage_in, stage_out;  // layer-split hand-off buffers (null for a whole-model session)
    size_t n_past = 0;
    size_t mem_per_token = 0;
    std::vector<TokenId> tokens;
    std::vector<float> last_logits;
    int last_n_nodes = 0, last_n_leafs = 0;
    ggml_cgraph *last_graph = nullptr;

   private:
    std::shared_ptr<Context> session_ctx_;
    std::shared_ptr<Context> stage_ctx_;
    size_t stage_rows_ = 0;
    bool stage_has_in_ = false, stage_has_out_ = false;
    size_t memory_size_ = 0;
    struct Built {
        ComputationGraph gf{nullptr};
        GraphOutputs out;
        Tensor embd;
    };
    Built build_into(int slot, size_t n_tokens, const Builder &builder) {
        Context &ctx0 = ctx0_[slot];
        ctx0.recreate();
        Built b;
        b.embd = ctx0.new_tensor_1d(GGML_TYPE_I32, n_tokens).set_name("embd");
        BuildContext bc{&ctx0, &b.embd, &memory_k, &memory_v, scratch_};
        auto built = builder(bc);
        b.gf = built.first;
        b.out = built.second;
        b.gf.build_forward_expand(b.out.result);  // Compute the graph
        return b;
    }
    struct Prebuilt {
        bool valid = false;
        size_t n_past = 0;
        const void *model_key = nullptr;
        int slot = 0;
        Built b;
    } pre_;
    Context ctx0_[2];
    int cur_ = 0;
    size_t n_embd_;
    std::shared_ptr<Buffer> scratch_[2];

   public:
    bool speculate = true;  // build the next single-token graph while the device runs (LLM_HOST_SPECULATE=0 disables)
    bool defer_end = false;  // set for the stages of an in-process split that produce no logits (Llama::start_session)
    bool pipeline_chunk = false;  // set by feed_prompt around every chunk but its last (see compute)
};

// crates/llm-base/src/model/common.rs:6-59
namespace common {
inline void read_last_token(InferenceSession &session, const Tensor &input_layer, size_t n_vocab, size_t n) {
    if (session.last_logits.size() != n_vocab) ggml::panic("last_logits size mismatch");
    input_layer.read_data(n_vocab * (n - 1) * sizeof(float), session.last_logits.data(), n_vocab * sizeof(float));
}
inline void extract_logits(OutputRequest &req, const Tensor &input_layer, size_t n_vocab, size_t n) {
    if (!req.all_logits) return;
    req.all_logits->assign(n_vocab * n, 0.0f);
    if (input_layer.nelements() != n_vocab * n) ggml::panic("extract_logits: element count mismatch");
    input_layer.read_data(0, req.all_logits->data(), n_vocab * n * sizeof(float));
}
inline void extract_embeddings(OutputRequest &req, const Tensor &embeddings_tensor, size_t n_embd, size_t n) {
    if (!req.embeddings) return;
    req.embeddings->assign(n_embd, 0.0f);
    std::vector<float> all(n_embd * n);
    if (embeddings_tensor.nelements() != n_embd * n) ggml::panic("extract_embeddings: element count mismatch");
    // The reference reads the host pointer (common.rs:52-56); the node is device-resident when offloaded, so
    // the mirror asks the backend for the device copy instead of reading stale host memory.
    ggml_hip_tensor_get(embeddings_tensor.ptr(), all.data(), 0, all.size() * sizeof(float));
    std::copy(all.begin() + n_embd * (n - 1), all.end(), req.embeddings->begin());
}
}  // namespace common

struct Hyperparameters {  // models/llama/src/lib.rs:399-416
    size_t n_vocab = 0, n_embd = 0, n_mult = 0, n_head = 0, n_head_kv = 0, n_layer = 0, n_rot = 0;
    int32_t file_type = 0;
};

struct Layer {  // models/llama/src/lib.rs:474-488
    Tensor attention_norm, wq, wk, wv, wo, ffn_norm, w1, w2, w3;
};

// TensorLoader (crates/llm-base/src/loader.rs:651-678): creates the named tensor in the model context and
// points its data at the caller's bytes (the mmap flavour: loader.rs:733-737).
class TensorLoader {
   public:
    TensorLoader(const llm_tensor_desc *t, int n) : descs_(t, t + n) {
        ctx_ = std::make_shared<Context>(
            Context::new_with_mmap((size_t)n * (sizeof(ggml_tensor) + sizeof(ggml_object) + 64) + 1024));
    }
    Tensor load(const std::string &name) {
        for (auto &d : descs_) {
            if (name != d.name) continue;
            Tensor t = d.n_dims == 1 ? ctx_->new_tensor_1d((ggml_type)d.type, (size_t)d.ne[0])
                                     : ctx_->new_tensor_2d((ggml_type)d.type, (size_t)d.ne[0], (size_t)d.ne[1]);
            t.set_data(d.data);
            t.set_name(name.c_str());
            return t;
        }
        fprintf(stderr, "llm: unknown tensor '%s'\n", name.c_str());  // LoadError::UnknownTensor
        abort();
    }
    std::shared_ptr<Context> finish() { return ctx_; }

   private:
    std::vector<llm_tensor_desc> descs_;
    std::shared_ptr<Context> ctx_;
};

class Llama {
   public:
    // models/llama/src/lib.rs:43-130
    Llama(Hyperparameters hp, ModelParameters params_, TensorLoader tl) : hyperparameters(hp), params(params_) {
        // layer split: this process owns [layer_begin, layer_end); the first stage also owns the
        // embedding table, the last one the final norm and the lm_head.  Default = the whole model = the reference.
        if (params.layer_end > hp.n_layer) params.layer_end = hp.n_layer;
        if (params.layer_begin >= params.layer_end) ggml::panic("empty layer range");
        if (is_first()) wte = tl.load("tok_embeddings.weight");
        const Backend backend = params.backend(0);
        if (is_last()) {
            norm = tl.load("norm.weight").transfer_to(backend);
            output = tl.load("output.weight").transfer_to(backend);
        }
        for (size_t i = params.layer_begin; i < params.layer_end; i++) {
            const Backend b = params.backend(i);
            auto name = [&](const char *s) { return "layers." + std::to_string(i) + "." + s; };
            Layer l;
            l.attention_norm = tl.load(name("attention_norm.weight")).transfer_to(b);
            l.wq = tl.load(name("attention.wq.weight")).transfer_to(b);
            l.wk = tl.load(name("attention.wk.weight")).transfer_to(b);
            l.wv = tl.load(name("attention.wv.weight")).transfer_to(b);
            l.wo = tl.load(name("attention.wo.weight")).transfer_to(b);
            l.ffn_norm = tl.load(name("ffn_norm.weight")).transfer_to(b);
            l.w1 = tl.load(name("feed_forward.w1.weight")).transfer_to(b);
            l.w2 = tl.load(name("feed_forward.w2.weight")).transfer_to(b);
            l.w3 = tl.load(name("feed_forward.w3.weight")).transfer_to(b);
            layers.push_back(l);
        }
        context = tl.finish();
    }

    bool is_first() const { return params.layer_begin == 0; }
    bool is_last() const { return params.layer_end == hyperparameters.n_layer; }
    size_t n_local_layers() const { return params.layer_end - params.layer_begin; }

    // on_slot >= 0: the session lives on that device slot (which the caller made current) instead of the model's — a sibling
    // slot of the same GPU: its own stream, shadows and plan workspace, the model's weights (llm_start_session_on)
    InferenceSession *start_session(const InferenceSessionConfig &config, int on_slot = -1) const {  // :133-141
        ModelParameters sp = params;
        if (on_slot >= 0) sp.main_device = on_slot;  // (keeps InferenceSession::new from re-initialising device 0, as for split stages)
        InferenceSession *s = new InferenceSession(config, sp, n_local_layers(), hyperparameters.n_embd,
                                                   hyperparameters.n_vocab);
        // stage hand-off buffers: persistent device tensors (like memory_k/v) that RCCL sends from / receives into
        if (!is_first() || !is_last()) s->make_stage_buffers(hyperparameters.n_embd, !is_first(), !is_last());
        s->defer_end = params.main_device >= 0 && !is_last();
        return s;
    }

    // The graph builder of Llama::evaluate (models/llama/src/lib.rs:166-362) for `input_len` tokens at position
    // `session_len`, as a value so that the session can also build the graph of the next call ahead of time.
    // logits_on_device: the logits node stays in HBM (like every other node) instead of being mirrored to the host after the
    // compute — taken for a multi-token evaluation that did not ask for all logits (feed_prompt: OutputRequest::default()):
    // read_last_token then fetches the one row it wants (65 MB of read-back per 512-token batch otherwise)
    InferenceSession::Builder make_builder(InferenceSession *session_ptr, size_t input_len, size_t session_len,
                                           bool logits_on_device = false) {
        return [this, session_ptr, input_len, session_len, logits_on_device](BuildContext &builder) {
            InferenceSession &session = *session_ptr;
            const size_t ctx_size = params.context_size;
            const size_t n_embd = hyperparameters.n_embd, n_head = hyperparameters.n_head,
                         n_head_kv = hyperparameters.n_head_kv, n_layer = hyperparameters.n_layer,
                         n_rot = hyperparameters.n_rot;
            const size_t n_embd_gqa = n_embd / (n_head / n_head_kv);

            Context &ctx0 = *builder.ctx0;
            const Tensor &embd = *builder.embd;
            (void)n_layer;
            // a stage of a layer split exchanges the residual through hand-off buffers of n_embd * rows floats (rows = n_batch
            // at first); ggml_view_1d has no bounds check (upstream neither), so the buffers must hold this call's rows
            if ((!is_first() || !is_last()) && input_len > session.stage_rows())
                ggml::panic("evaluate: the stage hand-off buffers hold fewer rows than this call (ensure_stage_rows not called)");
            Tensor input_layer = is_first()
                                     ? ctx0.op_get_rows(wte, embd)  // :170
                                     : ctx0.op_reshape_2d(ctx0.op_view_1d(session.stage_in, n_embd * input_len, 0), n_embd,
                                                          input_len);  // residual received from the previous stage
            ComputationGraph gf = ctx0.create_compute_graph();  // :172
            for (size_t il = 0; il < n_local_layers(); il++) {
                ctx0.set_offloading(params.should_offload(il));  // :175
                Tensor input_self_attention = input_layer.share();
                Tensor current;
                ctx0.use_scratch(builder.get_scratch(0));  // :180
                current = ctx0.op_rms_norm(input_layer);  // :183
                current = ctx0.op_mul(current, layers[il].attention_norm);  // :186
                const ggml::RoPEOverrides *overrides = params.has_rope_overrides ? &params.rope_overrides : nullptr;
                Tensor q_current =  // :191-204
                    ctx0.op_rope_inplace(ctx0.op_reshape_3d(ctx0.op_mul_mat(layers[il].wq, current), n_embd / n_head,
                                                            n_head, input_len),
                                         session_len, n_rot, 0, overrides)
                        .set_name("Qcur");
                Tensor k_current =  // :205-218
                    ctx0.op_rope_inplace(ctx0.op_reshape_3d(ctx0.op_mul_mat(layers[il].wk, current), n_embd / n_head,
                                                            n_head_kv, input_len),
                                         session_len, n_rot, 0, overrides)
                        .set_name("Kcur");
                Tensor v_current = ctx0.op_transpose(  // :222-226
                    ctx0.op_reshape_2d(ctx0.op_mul_mat(layers[il].wv, current), n_embd_gqa, input_len));
                const size_t kes = builder.memory_k->element_size(), ves = builder.memory_v->element_size();
                Tensor k = ctx0.op_view_1d(*builder.memory_k, input_len * n_embd_gqa,  // :228-232
                                           (kes * n_embd_gqa) * (il * ctx_size + session_len));
                Tensor v = ctx0.op_view_2d(*builder.memory_v, input_len, n_embd_gqa, ctx_size * ves,  // :234-240
                                           (il * ctx_size) * ves * n_embd_gqa + session_len * ves);
                gf.build_forward_expand(ctx0.op_cpy(k_current, k));  // :243
                gf.build_forward_expand(ctx0.op_cpy(v_current, v));  // :244
                Tensor q = ctx0.op_permute(q_current, 0, 2, 1, 3).set_name("Q");  // :246
                Tensor kk = ctx0.op_permute(  // :248-262
                                    ctx0.op_reshape_3d(ctx0.op_view_1d(*builder.memory_k,
                                                                       (session_len + input_len) * n_embd_gqa,
                                                                       il * ctx_size * kes * n_embd_gqa),
                                                       n_embd / n_head, n_head_kv, session_len + input_len),
                                    0, 2, 1, 3)
                                .set_name("K");
                Tensor k_q = ctx0.op_mul_mat(kk, q).set_name("KQ");  // :265
                Tensor kq_scale =  // :268-270
                    ctx0.new_f32(1.0f / std::sqrt((float)n_embd / (float)n_head)).set_name("1/sqrt(n_embd/n_head)");
                Tensor k_q_scaled = ctx0.op_scale_inplace(k_q, kq_scale).set_name("KQ_scaled");  // :271
                Tensor k_q_masked = ctx0.op_diag_mask_inf_inplace(k_q_scaled, session_len).set_name("KQ_masked");  // :274
                Tensor k_q_soft_max = ctx0.op_soft_max_inplace(k_q_masked).set_name("KQ_soft_max");  // :279
                Tensor vv = ctx0.op_view_3d(*builder.memory_v, session_len + input_len, n_embd / n_head, n_head_kv,  // :284-294
                                            ctx_size * ves, ctx_size * ves * n_embd / n_head,
                                            il * ctx_size * ves * n_embd_gqa)
                                .set_name("V");
                Tensor k_q_v = ctx0.op_mul_mat(vv, k_q_soft_max).set_name("KQV");  // :296
                Tensor k_q_v_merged = ctx0.op_permute(k_q_v, 0, 2, 1, 3).set_name("KQV_merged");  // :299
                current = ctx0.op_cpy(k_q_v_merged, ctx0.new_tensor_2d(GGML_TYPE_F32, n_embd, input_len))  // :302-307
                              .set_name("KQV_merged_contiguous");
                current = ctx0.op_mul_mat(layers[il].wo, current);  // :310
                ctx0.use_scratch(builder.get_scratch(1));  // :312
                Tensor input_feed_forward = ctx0.op_add(current, input_self_attention);  // :314
                current = ctx0.op_rms_norm(input_feed_forward);  // :318
                current = ctx0.op_mul(current, layers[il].ffn_norm);  // :321
                Tensor tmp = ctx0.op_mul_mat(layers[il].w3, current);  // :323
                current = ctx0.op_mul_mat(layers[il].w1, current);  // :325
                current = ctx0.op_silu(current);  // :328
                current = ctx0.op_mul(current, tmp);  // :330
                current = ctx0.op_mul_mat(layers[il].w2, current);  // :332
                current = ctx0.op_add(current, input_feed_forward);  // :334
                input_layer = current;  // :337
            }
            if (!is_last()) {  // hand the residual to the next stage through the persistent buffer
                ctx0.use_scratch(nullptr);
                Tensor out = ctx0.op_cpy(input_layer, ctx0.op_view_1d(session.stage_out, n_embd * input_len, 0));
                return std::make_pair(gf, GraphOutputs{out, out});
            }
            ctx0.use_scratch(builder.get_scratch(0));  // :340
            input_layer = ctx0.op_rms_norm(input_layer);  // :343
            input_layer = ctx0.op_mul(input_layer, norm);  // :346
            Tensor embedding_result = input_layer.share();
            ctx0.set_offloading(logits_on_device && params.use_gpu);  // :350 (false in the reference: the logits live on the host)
            input_layer = ctx0.op_mul_mat(output, input_layer);  // :352 lm_head
            ctx0.use_scratch(nullptr);  // :354
            return std::make_pair(gf, GraphOutputs{input_layer, embedding_result});
        };
    }

    // models/llama/src/lib.rs:144-368 — line numbers of the Rust builder are cited per step
    void evaluate(InferenceSession &session, const std::vector<TokenId> &input_tokens, OutputRequest &output_request) {
        const size_t input_len = input_tokens.size();
        const size_t session_len = session.n_past;
        const size_t ctx_size = params.context_size;
        const size_t n_vocab = hyperparameters.n_vocab, n_embd = hyperparameters.n_embd;

        InferenceSession *sp = &session;
        GraphOutputs outputs = session.compute(
            input_tokens, make_builder(sp, input_len, session_len, (input_len > 1 && !output_request.all_logits) || output_request.logits_on_device),
            [this, sp](size_t next_len) { return make_builder(sp, 1, next_len); }, this, ctx_size);
        if (!is_last()) return;
        // finish evaluation (:364-367)
        if (output_request.intermediate_chunk) return;  // (feed_prompt: only the last chunk's logits can be observed)
        if (!output_request.logits_on_device) common::read_last_token(session, outputs.result, n_vocab, input_len);
        common::extract_logits(output_request, outputs.result, n_vocab, input_len);
        common::extract_embeddings(output_request, outputs.embedding_result, n_embd, input_len);
    }

    // evaluate() of one token in two halves around a computation the caller arranges (llm_evaluate_batch): the graph exactly as
    // evaluate builds it, then what evaluate does once it has been computed
    ggml_cgraph *stage_single(InferenceSession &session, TokenId tok, GraphOutputs &out) {
        return session.stage_single(tok, make_builder(&session, 1, session.n_past), out);
    }
    void finish_single(InferenceSession &session, ggml_cgraph *gr, const GraphOutputs &out) {
        session.commit_single(gr);
        common::read_last_token(session, out.result, hyperparameters.n_vocab, 1);
    }

    // ... and evaluate() of n tokens the same way (llm_feed_prompt_batch): the graph evaluate builds for a default OutputRequest — the
    // logits of more than one token stay on the device — then n_past, and last_logits from the last row
    ggml_cgraph *stage_rows(InferenceSession &session, const TokenId *toks, size_t n, GraphOutputs &out) {
        return session.stage_rows(toks, n, make_builder(&session, n, session.n_past, n > 1), out);
    }
    void finish_rows(InferenceSession &session, ggml_cgraph *gr, size_t n, const GraphOutputs &out, bool last_piece) {
        session.commit_rows(gr, n);
        if (last_piece) common::read_last_token(session, out.result, hyperparameters.n_vocab, n);  // (as feed_prompt: only the last chunk's logits can be observed)
    }

    Hyperparameters hyperparameters;
    ModelParameters params;
    Tensor wte, norm, output;
    std::vector<Layer> layers;
    std::shared_ptr<Context> context;  // must be kept alive for the model
};

}  // namespace llm

// A model is one Llama — or, for the ggml-style layer split of ONE session over several GPUs of this process (SURVEY.md
// section 8e; ModelParameters / ggml_cuda_set_tensor_split, crates/ggml/src/accelerator/mod.rs:68-77), one Llama per device
// slot, each owning a contiguous layer range [layer_begin, layer_end) and its K/V on its own device.  `llama` / `s` are
// the LAST stage's (final norm, lm_head, logits, token history), so everything that reads hyperparameters or logits is
// unchanged; evaluation walks the stages in order and hands the residual on with ggml_hip_copy_between_devices.
struct llm_model {
    llm::Llama *llama;
    llm_ggml_file *file = nullptr;  // mmap'd container the weights point into (llm_llama_load)
    std::vector<llm::Llama *> stages;  // empty: unsplit
    std::vector<int> devices;          // device slot of each stage
    int device = ggml_hip_get_main_device();  // unsplit: the slot that was current when the model was made (its weights live there)
};
struct llm_session {
    llm::InferenceSession *s;
    std::vector<llm::InferenceSession *> stage_sessions;  // parallel to llm_model::stages
    bool shares_streams = false;  // its stages of one GPU enqueue on one stream (ggml_hip_share_stream), undone when the session goes
    std::vector<int> devices;
    int device = 0;  // unsplit: the model's slot (K/V, shadows and plans of the session live there)
    const llm_model *model = nullptr;  // the model it was started from
};

// what the mirror's translation units share beyond the types
namespace llm_host {
// Every entry point leaves the caller's main device as it found it: an unsplit model runs on the slot it was loaded on
// (llm_model::device), a split one walks its stages' slots.
struct HomeDevice {
    int pinned = ggml_hip_thread_pinned_device();  // -1: the thread follows the process default, and must again afterwards
    int home = ggml_hip_get_main_device();
    void go(int d) const {
        if (ggml_hip_get_main_device() != d) ggml_hip_bind_thread_device(d);  // this thread only: the process default stays
    }
    ~HomeDevice() {
        if (pinned < 0)
            ggml_hip_unbind_thread_device();  // (a later ggml_hip_set_main_device from another thread reaches this one again)
        else
            go(home);
    }
};
// both in llm_host.cpp
bool may_pipeline_chunk(const llm_model *m, size_t len);
void model_evaluate(llm_model *m, llm_session *s, const std::vector<llm::TokenId> &toks, llm::OutputRequest &req);
}  // namespace llm_host
