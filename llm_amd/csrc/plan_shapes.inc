// plan_*.inc — the fused LLaMA plans.  The graph that crates/models/llama/src/lib.rs:166-362 builds (37 nodes per layer +
// get_rows + final norm/mul/lm_head, rebuilt by the caller for EVERY evaluation: crates/llm-base/src/inference_session.rs:230)
// is recognised as a whole and executed as one of five launch sequences over the same cached DecodePlan:
//   single-token decode, block formats (plan_launch_all): 3 launches per layer with wq|wk|wv + attention + wo fused, 5 without;
//   K-quants (plan_launch_k): single-token decode, 4-6 launches per layer on the big workgroups; chunks of up to 31 tokens and —
//   option plan_batch_k — batched steps, 10-13 launches per layer on the helper-launch form;
//   single-token decode, chunks of up to 31 tokens and batched steps, F16 weights (plan_launch_f16): 5 launches per layer;
//   a chunk of 2..31 tokens, block formats (plan_launch_multi): 8 launches per layer and pass of 8 columns;
//   a prompt batch (plan_launch_prompt): 13 launches per layer around the matrix-core GEMMs, launched eagerly;
//   one token each of 2..8 sessions of one model (plan_launch_batch; ggml_hip_decode_batch hands over their graphs together): the
//   chunk's launches with a per-column position and cache.
// One more family has a plan over the same DecodePlan and run path: MPT's single-token graph (LlamaMatch::mpt, match_mpt_decode, plan_launch_mpt:
// five launches per layer; option plan_mpt) — decode and the greedy chain alone, everything else of it runs on the generic executor.
// A block-format model whose output matrix alone is a K-quant (LlamaMatch::out_k: llama.cpp's "mostly Q4_0 ... Q8_0" files) takes the block
// formats' sequences with the K plan's tail as its lm_head (plan_decode.inc plan_lm_head_k).
// The first three and the last are captured once in a hipGraph per attention variant and replayed for the following tokens with only
// {n_past, token} changing in a device-side parameter block.  One file per concern, included in this order from
// backend_executor.inc inside hip_backend.hip's anonymous namespace; the only forward declarations are DecodePlan and PrepMatch in
// front of Backend (backend_state.inc), whose fields name the slot's plans by their type:
//   plan_shapes.inc  LlamaMatch, DecodePlan (the layers' matrices as LayerMats<format>, the captured graphs as one VariantGraphs
//                    per attention variant), live_plan (what a remembered plan pointer still names) and every "which kernel, which
//                    grid for which shape" decision (plain host functions the matcher, the launchers, the run loop and the test
//                    hooks of the debug_*.inc files all call)
//   plan_match.inc   the structural graph matcher
//   plan_build.inc   weights, signature and activation pool of a plan (plan_pool_layout: every buffer declared once)
//   plan_decode.inc  the single-token launchers: plan_launch_all, plan_launch_k, plan_launch_f16, and what the last two share
//                    around their mat-vecs (plan_open_rows, plan_attn_f32, plan_hand_on)
//   plan_prompt.inc  plan_launch_multi, plan_launch_batch, prompt_attention, plan_launch_prompt
//   plan_run.inc     capture and replay, an evaluation as its steps (try_decode_plan), speculation, the fused-timeout re-run, the
//                    greedy chain, the batched step
//   plan_pool.inc    the request pool (ggml_hip_decode_pool_requests)
//   plan_pack.inc    the packed prompt batch (ggml_hip_prompt_pack): plan_launch_prompt over the rows of several sessions
//
// The matcher is structural (it follows src[] pointers from the logits back to get_rows and checks every view's
// shape/stride/offset against the KV-cache layout), so any graph that is not exactly the reference's LLaMA
// graph falls through to the generic per-node executor — same results, more launches.

// an F16 weight as the F16 plan reads it: the device pointer of the tensor's first row, the row stride in elements, the rows
struct F16W {
    const __half *p;
    int64_t ld, M;
};
// the seven matrices of a layer in whatever form W a matcher or a plan holds them; at(0 .. LAYER_MATS - 1) is "for each matrix"
static const int LAYER_MATS = 7;
template <class W>
struct LayerMats {
    W wq{}, wk{}, wv{}, wo{}, w1{}, w2{}, w3{};
    const W &at(int i) const {
        const W *const all[LAYER_MATS] = {&wq, &wk, &wv, &wo, &w1, &w2, &w3};
        return *all[i];
    }
    W &at(int i) { return const_cast<W &>(static_cast<const LayerMats *>(this)->at(i)); }
};
struct LayerW : LayerMats<const ggml_tensor *> {
    const ggml_tensor *attn_norm = nullptr, *ffn_norm = nullptr;
    const ggml_tensor *cur = nullptr;  // the normed activation feeding wq/wk/wv (identity key for the KV stores)
    bool k_store = false, v_store = false;
};
static const int PROMPT_PLAN_MAX = 4096;  // tokens per evaluation the prompt plan accepts
#define MULTI_MAX_N 31  /* tokens of the multi-token plan: passes of 8 columns below the prompt plan's threshold */
struct LlamaMatch {
    int L = 0;
    int64_t E = 0, H = 0, Hkv = 0, D = 0, F = 0, V = 0, C = 0, Egqa = 0;
    int n_past = 0, n_dims = 0;
    int N = 1;  // tokens in this evaluation: 1 = decode, 2..31 below mmq_min = a prompt chunk (multi-token plan), >= mmq_min = prompt plan
    bool prompt = false;  // the prompt plan takes it
    bool kquant = false;  // every matrix is a K-quant (any mix of Q2_K … Q6_K): the K plan (plan_launch_k): decode, chunks of up to 31 tokens below k_prompt_min, batched steps (option plan_batch_k)
    bool f16w = false;    // every matrix is F16 (file type 1): the F16 plan (plan_launch_f16), decode, chunks and batched steps
    bool out_k = false;   // a block-format model (wtype = the layers' type, kquant = false) whose output matrix alone is a K-quant, as llama.cpp's quantizer writes
                          // every block-format file: every plan of the block formats, the lm_head as the K plan's launches (plan_lm_head_k; option plan_out_k)
    // an MPT graph (plan_match.inc match_mpt_decode; option plan_mpt): the MPT plan (plan_launch_mpt), single-token decode alone.  Its four
    // matrices per layer sit in the LLaMA names — wq = Wqkv (3 E rows), wo = out_proj, w1 = up_proj, w2 = down_proj; wk, wv and w3 name
    // wq and w1 again so that "for each matrix" needs no second form — F = 4 E, Hkv = H, eps is ggml_norm's, and K AND V are token-major
    bool mpt = false;
    float alibi_bias_max = 0;
    float eps = 0, freq_base = 0, freq_scale = 0, kq_scale = 0;
    ggml_type wtype = GGML_TYPE_F32;
    const ggml_tensor *wte = nullptr, *norm = nullptr, *output = nullptr, *embd = nullptr, *memory_k = nullptr,
                      *memory_v = nullptr;
    ggml_tensor *logits = nullptr, *embedding = nullptr;
    const ggml_tensor *stage_in = nullptr, *stage_out = nullptr;  // layer-split hand-off buffers (persistent f32 leaves)
    std::vector<LayerW> layers;
};
// Attention variants of the single-token plan (one hipGraph each, chosen per token by the context length: attn_variant):
//   AV_SHORT  the attention of a head is ONE workgroup: inside the wq|wk|wv launch (k_qkv_attn) where the shape allows, else k_attn_decode
//   AV_SPLIT  plain wq|wk|wv launch, then the position-split attention over all CUs (k_attn_split_one / the three launches)
//   AV_FUSED2 / 3 / 4  k_qkv_attn with 2 / 3 / 4 attention workgroups per head (512 positions each: up to 1024 / 1536 / 2048)
enum { AV_SHORT = 0, AV_SPLIT = 1, AV_FUSED2 = 2, AV_FUSED3 = 3, AV_FUSED4 = 4, AV_COUNT = 5 };
enum { TAIL_FIRST = 0, TAIL_AHEAD = 1 };  // flavours of a greedy token's graph (VariantGraphs::tail_exec)
static inline int av_heads_split(int av) { return av >= AV_FUSED2 ? av : 1; }
// the captured graphs of ONE attention variant of a plan (they freeze which kernels run: options and the device's slot count at capture time)
struct VariantGraphs {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr, exec2 = nullptr;  // exec2: a second instance of the same graph — a chain alternates so that a launch never waits for its own previous run
    // a greedy token's graph: the same launches aimed at result set q (DecodePlan::res_logits), then k_token_tail into slot q; tokens alternate
    // between the two, so a launch never waits for its own previous run and never writes what the host or a device-side reader still reads.
    // Two flavours each, [flavour][q] (tail_prepares: the block-format plan on the big workgroups under option tail_prepare; every other
    // plan has flavour TAIL_FIRST alone, with its k_kv_row_save in front):
    //   TAIL_FIRST  behind a host upload of the parameters: get_rows and the RoPE table, the layers, the tail — which prepares the next token
    //   TAIL_AHEAD  directly behind another tail graph of the same plan, and only there: the layers on what that graph's tail prepared
    //               (row, table, epoch, saved cache rows), the tail; its first kernel is the layer-0 launch
    hipGraph_t tail_graph[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    hipGraphExec_t tail_exec[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    void drop() {
        for (hipGraphExec_t e : {exec, exec2, tail_exec[0][0], tail_exec[0][1], tail_exec[1][0], tail_exec[1][1]})
            if (e) (void)hipGraphExecDestroy(e);
        for (hipGraph_t gr : {graph, tail_graph[0][0], tail_graph[0][1], tail_graph[1][0], tail_graph[1][1]})
            if (gr) (void)hipGraphDestroy(gr);
        *this = VariantGraphs{};
    }
};
// ---------------------------------------------------------------------------------------------------
// the cached plan
// ---------------------------------------------------------------------------------------------------
struct DecodePlan {
    std::vector<uint64_t> sig;
    LlamaMatch m;  // tensors of the graph the plan was built from (weights are persistent; IO nodes by address)
    // the layers' matrices in the one form the plan's kind reads, the other two vectors empty: block formats as SoA weights (the
    // K-quant prompt plan fills these too, from the f16 copies: k_prompt_weights), K-quants as planar K weights (each carries its own
    // type), F16 as the tensors' own rows (no re-layout, no copy)
    using LW = LayerMats<QWeight>;
    using KLW = LayerMats<KWeight>;
    using FLW = LayerMats<F16W>;
    std::vector<LW> lw;
    std::vector<KLW> klw;
    std::vector<FLW> flw;
    struct LayerNorms {
        const float *attn_norm, *ffn_norm;
    };
    std::vector<LayerNorms> ln;  // every kind of plan
    F16W f_wte{}, f_output{};
    KWeight k_wte{}, k_output{};
    // K plan activations: f32 rows of wk / wv / the merged heads / w3, and ONE Q8_K row (max(E, F) wide) every mat-vec reads
    float *k_kf = nullptr, *k_vf = nullptr, *k_att = nullptr, *k_g3 = nullptr;
    int8_t *k_q8 = nullptr;
    float *k_d8 = nullptr;
    int16_t *k_bs = nullptr;
    QWeight wte, output;
    const float *norm = nullptr;
    __half *mem_k = nullptr, *mem_v = nullptr;
    __half *mem_k_at(int il) const { return mem_k + (size_t)il * m.C * m.Egqa; }  // layer il's part of the caches
    __half *mem_v_at(int il) const { return mem_v + (size_t)il * m.C * m.Egqa; }
    int64_t kv_off(int il) const { return (int64_t)il * m.C * m.Egqa; }  // the same offset, for caches named by a table:
    // a batched step's plan (plan_launch_batch; m is its first graph's match with N = the columns): the per-column table on the device,
    // uploaded with prm for every step.  Its logits_out / emb_out are rows of the pool (one per column), not a graph's nodes; mem_k / mem_v are unused.
    bool batch = false;
    BatchCols *bcols = nullptr;
    // the sampled chains (ggml_hip_decode_batch_sampled; ggml_hip_decode_sampled_chain on a single-token whole-model plan, column 0):
    // the columns' history rings and the sampler's parameters (k_sample_next)
    SampleCols *scols = nullptr;
    // persistent activations
    char *pool = nullptr;
    DecParams *prm = nullptr;
    float *rope = nullptr;      // this token's RoPE (cos, sin) table, D/2 pairs (k_rope_table)
    float *alibi = nullptr;     // MPT plan: the 256 ALiBi slopes (alibi_slopes' values, uploaded when the plan is built)
    unsigned *epoch = nullptr;  // k_qkv_attn (kernels/decode_fused.h): the token's granule tag, bumped by k_rope_table
    const void *hot = nullptr;  // 256 zero bytes that every dummy ring step of k_mmvq_big reads (BigArgs::hot)
    unsigned *ferr = nullptr;   // ... raised when an attention workgroup gave up waiting for its rows
    unsigned long long *gran = nullptr;  // ... granules: (E + 2 Egqa) / 2 per layer
    unsigned long long *gran_at(int il) const { return gran + (size_t)il * (size_t)((m.E + 2 * m.Egqa) / 2); }
    unsigned long long *ogran = nullptr;      // ... E / 32 x OGRAN granules per layer: the attention output on its way to wo (WO form)
    unsigned long long *dead_gran = nullptr;  // one layer's worth of granules nobody writes (test hook: a hand-off that never arrives)
    uint64_t dev_gen = 0;                // g_dev_gen of the device when the graphs below were captured (see device_sharers)
    uint64_t wgen = 0;                   // g_dev_wgen of the device when the plan was built: a weight record freed since (by ANY slot of the device) makes the plan stale
    float *xa = nullptr, *xb = nullptr, *q = nullptr, *gate = nullptr, *logits = nullptr;
    int8_t *e_lo = nullptr, *e_hi = nullptr, *f_lo = nullptr, *f_hi = nullptr;
    float *e_d = nullptr, *f_d = nullptr;
    int *e_s = nullptr, *f_s = nullptr;
    float *e_dT = nullptr, *f_dT = nullptr;  // multi-token plan: the same scales / sums as [block][8] tables (k_mmq_cols)
    int *e_sT = nullptr, *f_sT = nullptr;
    // prompt plan (N > 8): f32 GEMM outputs, the f16 GEMM operand, scores, token ids
    float *p_te = nullptr, *p_qf = nullptr, *p_kf = nullptr, *p_vf = nullptr, *p_mg = nullptr, *p_g1 = nullptr, *p_g3 = nullptr, *p_sc = nullptr;
    _Float16 *p_x16 = nullptr, *p_p16 = nullptr;  // GEMM operand; softmax probabilities as f16 rows of (C + 8) & ~7
    int *p_tok = nullptr;
    float *stage_in = nullptr, *stage_out = nullptr;  // layer split: residual received / handed on
    // Result set 0: the device images of the graph's own embedding_result / logits nodes.  Result set 1 (single-token plans): the same
    // two buffers again in the plan's pool.  Greedy tokens alternate between the sets (VariantGraphs::tail_exec): the token the device
    // runs AHEAD of its caller writes the set the last evaluated token does not sit in, so that set stays what every device-side
    // reader must see (ggml_hip_topk, ggml_hip_tensor_get, llm_session_read_node, the greedy chain, perplexity: result_dev_ptr /
    // plan_cur_logits).  A hit only flips cur_set; nothing is copied.  Everything that is not a greedy token writes set 0.
    float *emb_out = nullptr;
    char *logits_out = nullptr;
    char *logits_alt = nullptr;
    float *emb_alt = nullptr;
    int cur_set = 0;  // the set of the last evaluated token (meaningful while the slot's res_plan is this plan; set 0 otherwise)
    char *res_logits(int q) const { return q ? logits_alt : logits_out; }
    float *res_emb(int q) const { return emb_out ? (q ? emb_alt : emb_out) : nullptr; }
    // the two result slots of the greedy tokens, pinned host memory k_token_tail stores into: logits | embedding row | id
    char *slot[2] = {nullptr, nullptr};
    hipEvent_t slot_ev[2] = {nullptr, nullptr};  // recorded directly behind the launch of the graph that fills the slot
    size_t slot_emb_off = 0, slot_id_off = 0;
    __half *kv_save[2] = {nullptr, nullptr};  // per parity: the cache rows of the position that graph writes, as they were before (k_kv_row_save)
    float *xnext = nullptr;  // the NEXT token's embedding row, dequantized by k_token_tail (TailPrep): layer 0's input in a TAIL_AHEAD graph.  Not xa:
                             // that is the residual stream and the last layer's output, which readers of the finished token may still look at
    bool prm_ahead = false;  // a token tail has moved the device's DecParams past m's token: whoever replays the plan next uploads them first
    int *chain_out = nullptr;   // ggml_hip_decode_greedy_chain / ggml_hip_decode_batch_greedy: sampled ids (device)
    int *chain_ring = nullptr;  // ... of one K-token graph launch (option chain_k), copied into chain_out behind it
    int chain_cap = 0;
    char *chain_req = nullptr;  // the chains that stop: the call's request table (a SampleReqs, kernels/sample.h), made at the first such call
    char *pool_tab = nullptr;   // the request pools (plan_pool.inc): the call's PoolTable (kernels/pool_admit.h) and the retire slots
    float *pool_rows = nullptr;  // ... logits [n_pool][V], then embedding rows [n_pool][E]; both made at the first such call
    size_t pool_rows_cap = 0;
    VariantGraphs graphs[AV_COUNT];  // per attention variant; a batched step's plan has the one of AV_SHORT
    bool any_captured() const {
        for (const VariantGraphs &v : graphs)
            if (v.exec) return true;
        return false;
    }
    float *att_sc = nullptr, *att_pmax = nullptr, *att_part = nullptr;  // scratch of the split attention
    unsigned long long *att_mxg = nullptr, *att_sumg = nullptr, *att_partg = nullptr;  // ... as one launch (k_attn_split_one): range maxima / sums / partial-output granules, [L] sets of them (att_*_at)
    unsigned long long *att_mxg_at(int il) const { return att_mxg + (size_t)il * m.H * att_S; }
    unsigned long long *att_sumg_at(int il) const { return att_sumg + (size_t)il * m.H * att_S * 2; }
    unsigned long long *att_partg_at(int il) const { return att_partg + (size_t)il * m.H * att_S * m.D; }
    unsigned *att_cnt = nullptr;                                         // ... and the per-head arrival counters
    int att_S = 1;                       // workgroups per head of the split attention
    hipGraph_t graph_chain = nullptr;      // option chain_k: k_argmax_next + one token, K times over, as ONE graph
    hipGraphExec_t exec_chain = nullptr;
    int chain_k = 0;                       // tokens captured in graph_chain
    uint64_t replays = 0;
    uint64_t w16_gen = 0;  // g.w16_gen the QWeight::w16 pointers above were read at (0 = never)
};

std::vector<DecodePlan *> g_plans_[GGML_HIP_MAX_BACKENDS];  // per slot: a plan holds device addresses
#define g_plans (g_plans_[g.slot])
// the plan of this slot that `p` names, or null: a pointer remembered across evaluations (Backend::chain_plan, res_plan, ferr_plan,
// spec.plan, PrepMatch::p) may have outlived its plan (drop_all_plans) and is only compared here, never dereferenced
static DecodePlan *live_plan(const DecodePlan *p) {
    for (auto *q : g_plans)
        if (q == p) return q;
    return nullptr;
}

void drop_plan_graphs(DecodePlan *p) {
    for (VariantGraphs &v : p->graphs) v.drop();
    if (p->exec_chain) (void)hipGraphExecDestroy(p->exec_chain);
    if (p->graph_chain) (void)hipGraphDestroy(p->graph_chain);
    p->exec_chain = nullptr;
    p->graph_chain = nullptr;
    p->chain_k = 0;
}
void destroy_plan(DecodePlan *p) {
    drop_plan_graphs(p);
    if (p->chain_ring) (void)hipFree(p->chain_ring);
    if (p->chain_out) (void)hipFree(p->chain_out);
    if (p->chain_req) (void)hipFree(p->chain_req);
    if (p->pool_tab) (void)hipFree(p->pool_tab);
    if (p->pool_rows) (void)hipFree(p->pool_rows);
    if (p->pool) (void)hipFree(p->pool);
    for (int q = 0; q < 2; q++) {
        if (p->slot[q]) (void)hipHostFree(p->slot[q]);
        if (p->slot_ev[q]) (void)hipEventDestroy(p->slot_ev[q]);
    }
    if (g.res_plan == p) g.res_plan = nullptr;
    delete p;
}
// The device address a reader of node `t` reads: the tensor's own image, unless it lies in result set 0 of the plan whose last
// evaluated token sits in set 1 — then the same offset of set 1 (DecodePlan::cur_set).
char *result_dev_ptr(const ggml_tensor *t) {
    char *d = dev_ptr(t);
    const DecodePlan *p = g.res_plan;
    if (!p || p->cur_set != 1 || !p->logits_alt) return d;
    const size_t lb = (size_t)p->m.V * 4, eb = (size_t)p->m.E * 4;
    if (p->logits_out && d >= p->logits_out && d < p->logits_out + lb) return p->logits_alt + (d - p->logits_out);
    if (p->emb_out && d >= (char *)p->emb_out && d < (char *)p->emb_out + eb) return (char *)p->emb_alt + (d - (char *)p->emb_out);
    return d;
}
// Another graph overtakes the plan whose last evaluated token sits in result set 1 (anything but a hit on that plan): its values go
// into set 0, the graph nodes' own images, behind whatever ran ahead into set 0 — readers of that session's nodes keep seeing its
// last evaluated token however many other sessions, chunks or generic graphs run on the slot afterwards.  Never on the hit path.
static void res_settle() {
    DecodePlan *p = live_plan(g.res_plan);
    g.res_plan = nullptr;
    if (!p || p->cur_set != 1 || !p->logits_alt || !p->logits_out) return;
    HIP_CHECK(hipMemcpyAsync(p->logits_out, p->logits_alt, (size_t)p->m.V * 4, hipMemcpyDeviceToDevice, g.stream));
    if (p->emb_out) HIP_CHECK(hipMemcpyAsync(p->emb_out, p->emb_alt, (size_t)p->m.E * 4, hipMemcpyDeviceToDevice, g.stream));
    p->cur_set = 0;
}
static inline char *plan_cur_logits(const DecodePlan *p) { return p->res_logits(g.res_plan == p ? p->cur_set : 0); }
// A token the device ran ahead of its caller is in flight or finished unused: nothing of it may be taken for a result any more (its
// plan's buffers are about to be reused, dropped, or replayed for a measurement).  The stream is drained so that it is over.
// the K/V rows the pending ahead run wrote (a position its session has not reached) as they were before it, behind it on the stream
static inline int kv_row_grid(const DecodePlan *p) { return (int)std::min<int64_t>(256, ((int64_t)p->m.L * p->m.Egqa + 255) / 256); }
static void spec_take_back() {
    DecodePlan *p = live_plan(g.spec.plan);
    if (!p || !p->kv_save[g.spec.parity] || !p->mem_k) return;
    hipLaunchKernelGGL(k_kv_row_restore, dim3(kv_row_grid(p)), dim3(256), 0, g.stream, g.spec.n_past, p->mem_k, p->mem_v,
                       (const __half *)p->kv_save[g.spec.parity], (int)p->m.L, (int)p->m.C, (int)p->m.Egqa);
    HIP_CHECK(hipGetLastError());
}
void spec_cancel() {
    if (!g.spec.pending) return;
    g.spec.pending = false;
    spec_take_back();
    if (g.stream) HIP_CHECK(hipStreamSynchronize(g.stream));
}
// an access to device memory from outside (ggml_hip_tensor_get / _set, ggml_hip_memcpy): if it touches the caches the pending ahead
// run reads and writes, that run is taken back first (a read then sees what a session that never ran ahead holds; after a write
// the next evaluation runs on the new contents)
void spec_guard_read(const char *d, size_t n) {
    if (!g.spec.pending) return;
    const DecodePlan *p = live_plan(g.spec.plan);
    if (!p || !p->mem_k) return;
    const size_t kvb = (size_t)p->m.L * p->m.C * p->m.Egqa * 2;
    const char *k = (const char *)p->mem_k, *v = (const char *)p->mem_v;
    if ((d < k + kvb && k < d + n) || (d < v + kvb && v < d + n)) spec_cancel();
}
void finish_pending();
void drop_all_plans() {
    finish_pending(); // (a token whose results still sit in a plan's slot is delivered before the slot goes)
    spec_cancel();
    if (g_plans.empty()) return;
    if (g.stream) HIP_CHECK(hipStreamSynchronize(g.stream));
    for (auto *p : g_plans) destroy_plan(p);
    g_plans.clear();
    g.ferr_plan = nullptr;
}
static inline size_t attn_decode_lds(int64_t C, int64_t D) { return (size_t)(C + D) * 4 + (size_t)C * 2; }
static const size_t ATTN_DECODE_LDS_MAX = 150 * 1024;  // of the CU's 160 KiB (the kernel's static arrays take a little)
// Waves per workgroup of a k_mmvq_big launch: the count in [8, 16] with the best
//   (units / (rounds * G * W))  x  (1 - 0.015 * (16 - W))
// i.e. how evenly `units` are dealt over G workgroups of W waves, discounted by what fewer waves cost in loads in
// flight (measured: 8 waves stream w1|w3 12 % slower than 16).  7B: wq|wk|wv 12 waves (6144 row pairs: 2 per wave
// instead of 2|1: 11.1 -> 9.5 us per launch), w1|w3 15; 13B: wo and w2 10 (5120 rows: 2 per wave instead of 2|1).
static int big_waves(int64_t units, int G, int min_waves) {
    static const int forced = getenv("GGML_HIP_BIG_WAVES") ? atoi(getenv("GGML_HIP_BIG_WAVES")) : 0;
    if (forced >= 8 && forced <= BIG_W) return std::max(forced, min_waves);
    auto score = [&](int W) {
        const int64_t per_round = (int64_t)G * W, rounds = (units + per_round - 1) / per_round;
        return (double)units / (double)(rounds * per_round) * (1.0 - 0.015 * (BIG_W - W));
    };
    int best = BIG_W;
    for (int W = BIG_W - 1; W >= std::max(8, min_waves); W--)
        if (score(W) > score(best) + 1e-9) best = W;
    return best;
}
// what the staging of a k_mmvq_big launch needs: Q8 source one thread per block; f32 source 24 elements per thread; the norm 8
// stager waves (+ the 2 RoPE-table waves of wq|wk|wv).  Above BIG_W the launch cannot stage the row (ggml_hip_debug_mat_vec_big).
static int big_min_waves(int xsrc, int epi, int64_t nb) {
    int min_waves = 8;
    if (xsrc == XSRC_Q8) min_waves = (int)((nb + 63) / 64);
    if (xsrc == XSRC_F32) min_waves = (int)((nb * 32 + 24 * 64 - 1) / (24 * 64));
    if (xsrc == XSRC_NORM) min_waves = epi == EPI_QKV ? 10 : 8;
    return std::max(min_waves, 8);
}
// workgroups of a mat-vec launch over `cus` CUs: one resident wave of workgroups, BIG_W units each before a second round starts
static inline int big_groups(int64_t units, int cus) { return (int)std::min<int64_t>(cus, std::max<int64_t>(1, (units + BIG_W - 1) / BIG_W)); }
static inline int64_t big_rounds(int64_t units, int G, int W) { return (units + (int64_t)G * W - 1) / ((int64_t)G * W); }
// the dealing of one k_mmvq_big launch: G workgroups of which W waves take units, and its LDS; !ok: more than 64 units per wave
// (one epilogue lane per unit of a wave)
struct BigShape {
    bool ok;
    int G, W;
    size_t lds;
};
static BigShape big_shape(int xsrc, int epi, int64_t nb, int64_t units) {
    BigShape s;
    s.G = big_groups(units, g.num_cus);
    s.W = big_waves(units, s.G, big_min_waves(xsrc, epi, nb));
    s.ok = big_rounds(units, s.G, s.W) <= 64;
    s.lds = (size_t)((nb + 63) / 64 * 64) * 40;
    return s;
}
// wq|wk|wv + attention in one launch (kernels/decode_fused.h): n_head attention workgroups + the mat-vec on the remaining
// G - n_head.  Taken when the mat-vec deals as evenly over G - n_head workgroups as over G (7B on 256 CUs: 6144 row pairs
// = 2 per wave of 224 x 14 as of 256 x 12) — otherwise the two-launch pair is the faster one.
struct FusedShape {
    bool ok = false;
    int G = 0, W = 0, S = 1;
    bool wo = false;   // the WO form: wo + residual as the mat-vec workgroups' second phase (kernels/decode_fused.h wo_tail)
    bool affine = false;  // head h's rows of wq|wk|wv are dealt to the mat-vec workgroups of the XCD its attention workgroup runs on (BigArgs::aff_hpl)
};
static FusedShape fused_qkv_shape(const LlamaMatch &m, int S = 1) {
    FusedShape s;
    if (!g.opt_fuse_attn || !g.opt_big || m.kquant || m.f16w || m.mpt || m.N != 1 || m.D > 128 || m.D % 32 != 0) return s;
    const int H = (int)m.H * S;  // attention workgroups
    const int64_t units = (m.E + 2 * m.Egqa) / 2;
    if (H + 1 > g.num_cus) return s;
    // several slots (sessions) on this GPU: their launches run side by side, and attention workgroups hold a CU until their
    // producers have run — all of them together must leave most of the chip to producers, or nobody may wait at all.  Measured
    // (bench.py --mode sessions, LLaMA-7B Q4_0, aggregate tokens/s fused / two-launch): 2 sessions 1030 / 1006, 3 sessions
    // 1139 / 1190 — a quarter of the CUs is the limit (7B: two sessions keep the fused launch, three take the pair).
    if (device_sharers() > 1 && (int64_t)device_sharers() * H > g.num_cus / 4) return s;
    s.S = S;
    // workgroups of the plain launch (launch_big) and of the mat-vec part here: one resident wave of workgroups either way
    const int G0 = big_groups(units, g.num_cus), Gp = big_groups(units, g.num_cus - H);
    const int Wp = big_waves(units, Gp, big_min_waves(XSRC_NORM, EPI_QKV, m.E / 32));
    if (big_rounds(units, Gp, Wp) > 64) return s;
    // one attention workgroup per head: measured to pay wherever the mat-vec keeps most of the chip (tests/tools/ctx_sweep.py at 200 /
    // 400 positions, ms per token two-launch -> fused: 7B Q4_0 224 of 256 workgroups 1.37 -> 1.27; 13B Q5_1, 216: 2.81 -> 2.60 and
    // 2.97 -> 2.69 (the WO form rides along); 65B Q8_0, 192: 12.67 -> 12.40).  Below ~70 % of the plain launch's workgroups nothing
    // was measured: refused.
    if (S == 1 && g.opt_fuse_attn < 2 && (Gp * 10 < G0 * 7 || Gp < 2 * H)) return s;  // 2 = wherever it is legal (tests)
    if (S > 1) {
        // several workgroups per head take CUs from the mat-vec for the whole launch.  Measured against the best other path
        // (tests/tools/ctx_sweep.py, ms per token, S = 2 / 3 / 4 at 700-900 / 1100 / 1800 positions; + = the fused heads win):
        //   7B  Q4_0 28 MB of wq|wk|wv, 192 / 160 / 128 workgroups left: + + + (641 against 610 tok/s at 1800)
        //   7B  Q5_1 38 MB: + + + (1.68 / 1.77 / 1.84 against 1.76 / 1.91 / 1.95);  7B Q8_0 53 MB: + + + (1.86 / 1.96 / 2.01 against 1.96 / 2.05 / 2.10)
        //   13B Q4_0 44 MB, 176 / 136 / 96 left: + + = (2.37 / 2.46 / 2.63 against 2.44 / 2.54 / 2.64);  13B Q8_0 84 MB: + + - (3.09 / 3.21 / 3.45 against 3.17 / 3.26 / 3.36)
        //   13B Q5_1 59 MB: - - - (3.05 / 3.06 / 3.29 against 2.97 / 3.02 / 3.09);  65B Q8_0 214 MB, 128 left: - (13.32 against 12.79)
        // No single quantity explains all of it; the rule is a fit: the mat-vec keeps 45 % of the plain launch's workgroups, and the stream — counted
        // 1.7-fold for the types whose 5-bit unpack makes a workgroup compute-bound — is at most 90 MB.
        const double qkv_bytes = (double)(m.E + 2 * m.Egqa) * (double)(m.E / 32) * (double)blk_bytes(qt_of(m.wtype));
        const bool q5 = qt_of(m.wtype) == QT_Q5_0 || qt_of(m.wtype) == QT_Q5_1;
        if (Gp < g.num_cus / 4) return s;
        if (g.opt_fuse_attn < 2 && (Gp * 100 < G0 * 45 || qkv_bytes * (q5 ? 1.7 : 1.0) > 90e6)) return s;
    }
    s.ok = true;
    s.G = H + Gp;
    s.W = Wp;
    // wo under the attention's tail: both directions of the launch wait for each other, so the whole launch must be resident —
    // this slot alone on the GPU — and a workgroup's rows of wo, the gathered activation and the granule sweep must fit
    if (g.opt_fuse_wo && device_sharers() == 1) {
        const int64_t nbE = m.E / 32, rows = (m.E + Gp - 1) / Gp;
        if (rows <= 16 * WO_RW && (nbE + 63) / 64 <= 4 && nbE * OGRAN <= 1024 * WO_NG_MAX) s.wo = true;
    }
    // XCD-affine dealing: head h's attention workgroup(s) at blockIdx = h mod n_head, the mat-vec workgroups behind them in multiples of 8, MHA
    // (a K / V head feeds ONE attention workgroup), this slot alone on the GPU (nobody else's workgroups in the dispatcher's round robin)
    if (g.opt_affine && g.xcd_labels == 1 && device_sharers() == 1 && m.H % 8 == 0 && Gp % 8 == 0 && m.Egqa == m.E &&
        (m.D == 32 || m.D == 64 || m.D == 128) && m.E == m.H * m.D)
        s.affine = true;
    return s;
}
// option "attn_split": 0 off, 1 = from ATTN_SPLIT_MIN positions on, n > 1 = from n positions on
// fused: the short-context attention is k_qkv_attn (stays ahead of the split path for longer than k_attn_decode does)
static inline int64_t attn_split_min(bool fused = true) { return g.opt_attn_split > 1 ? g.opt_attn_split : fused ? ATTN_SPLIT_MIN_FUSED : ATTN_SPLIT_MIN; }
static inline int64_t attn_split_min_of(const LlamaMatch &m) { return attn_split_min(fused_qkv_shape(m).ok); }
// workgroups per head of the split attention (DecodePlan::att_S) ...
static inline int plan_att_S(int64_t H) { return (int)std::max<int64_t>(1, std::min<int64_t>(16, g.num_cus / std::max<int64_t>(1, H))); }
// ... and whether a single-token evaluation of H heads goes over to it from attn_split_min positions on
static inline bool attn_split_from_min(int64_t H) { return g.opt_attn_split && g.opt_big && plan_att_S(H) >= 2; }
// the split attention as one launch: every workgroup must be resident (they wait for each other); scores + probabilities of a
// range stay in LDS
static inline size_t attn_split_chunk_max(int64_t C, int S) { return ((((size_t)C + S - 1) / S) + 63) & ~(size_t)63; }  // positions of a workgroup
static bool attn_one_ok(const LlamaMatch &m, int att_S) {
    const size_t chunk_max = attn_split_chunk_max(m.C, att_S);
    // (every workgroup of this launch waits for peers: it must have the GPU to itself — one slot per device)
    return g.opt_attn_one && device_sharers() == 1 && m.N == 1 && att_S <= 16 && (int64_t)m.H * att_S <= g.num_cus && chunk_max * 6 <= 60 * 1024 && m.D % 32 == 0 && m.D <= 128;
}
// The attention variant of a single-token evaluation whose token sits at position T - 1 (see the enum above).  Option
// fuse_heads (default 1): contexts beyond k_qkv_attn's 512-position register window get 2 / 4 attention workgroups per head inside
// the wq|wk|wv launch instead of the separate split attention, where the chip has room for them.
static int attn_variant(const LlamaMatch &m, const DecodePlan *p, int64_t T) {
    if (m.N != 1 || m.mpt) return AV_SHORT;  // (the MPT plan has the one attention: k_attn_decode_alibi over the whole context)
    const bool split_ok = (!(m.kquant || m.f16w) || attn_one_ok(m, p->att_S)) && attn_split_from_min(m.H);
    if (g.opt_fuse_heads && g.opt_attn_split == 1 && split_ok && T > FUSE_HEADS_MIN && fused_qkv_shape(m).ok) {
        const int S = (int)((T + 511) / 512);  // workgroups per head: 512 positions each
        if (S <= 4 && p->att_S >= S && fused_qkv_shape(m, S).ok) return S;  // = AV_FUSED2 / 3 / 4
    }
    return split_ok && T >= attn_split_min_of(m) ? AV_SPLIT : AV_SHORT;
}
// positions k_attn_decode's LDS arrays must hold for an evaluation of N tokens at context C: longer rows of a single token
// run on the split attention
static inline int64_t attn_decode_rows(int64_t C, int N, int64_t H) {
    return N == 1 && attn_split_from_min(H) ? std::min<int64_t>(C, (attn_split_min() + 7) & ~(int64_t)7) : C;
}
// wq|wk|wv + attention of a K-quant token in one launch (k_qkv_attn_k): legal like fused_qkv_shape's S = 1 form
static bool kfused_ok(const DecodePlan *p, int av) {
    const LlamaMatch &m = p->m;
    if (!g.opt_fuse_attn || av != AV_SHORT || m.N != 1 || m.D > 128 || m.D % 32 != 0 || !p->gran) return false;
    const int H = (int)m.H;
    if (H * 4 > g.num_cus) return false;                                                       // the mat-vec keeps >= 3/4 of the chip
    if (device_sharers() > 1 && (int64_t)device_sharers() * H > g.num_cus / 4) return false;  // see fused_qkv_shape
    const int64_t units = (m.E + 2 * m.Egqa) / 2, waves = (int64_t)(g.num_cus - H) * 16;
    return (units + waves - 1) / waves <= 31;  // two parked values per unit lane
}
// a K matrix of M rows of nsb super-blocks that k_mmvq_kbig takes; norm_width: the row its norm staging would hold (0: none)
static bool kbig_weight_ok(int kt, int64_t nsb, int64_t M, int64_t norm_width) {
    return kt >= 0 && kt <= KT_Q5_K && nsb <= 64 && norm_width <= 8192 &&  // all five K types; staging limits of k_mmvq_kbig (KBIG_SBW, KBIG_SQ)
           (M + (int64_t)g.num_cus * 16 - 1) / ((int64_t)g.num_cus * 16) <= 21;  // (three matrices per launch: 63 rows per wave)
}
// the lm_head of an out_k model as ONE k_mmvq_kbig launch that stages the final norm itself: a single token whose output matrix that
// kernel takes; every other evaluation runs it as k_k_norm_quant + k_mmvq_k (plan_lm_head_k)
static bool out_k_big(const LlamaMatch &m) {
    return m.out_k && g.opt_kbig && m.N == 1 && kbig_weight_ok(kt_of(m.output->type), m.E / 256, m.V, m.E);
}
static bool kbig_ok(const DecodePlan *p) {  // K matrices whose rows of a wave fit its 64 epilogue lanes and whose activation row fits the staging
    if (!g.opt_kbig || p->m.N != 1) return false;
    auto ok = [&](const KWeight &w) { return kbig_weight_ok(w.kt, w.nsb, w.M, p->m.E); };
    for (auto &l : p->klw)
        for (int i = 0; i < LAYER_MATS; i++)
            if (!ok(l.at(i))) return false;
    return !p->m.output || ok(p->k_output);
}
// ---- k_mmvq_f16 (kernels/decode_f16.h) ----
// columns of one pass over a matrix of width K when `left` columns remain: 8 / 4 / 2 / 1, whichever the LDS holds (launch_mmvq_kn's rule)
static inline int f16_pass_cols(int64_t K, int left) {
    int ncols = 8;
    while (ncols > 1 && (ncols > left || (size_t)ncols * (size_t)K * 2 > 150 * 1024)) ncols >>= 1;
    return ncols;
}
// a launch over `units` (rows; pairs of rows for the gate and wq|wk|wv) of width K: 16-byte chunks, one column in LDS, one epilogue lane per unit of a wave
static inline bool f16_launch_shape_ok(int64_t K, int64_t units) {
    return K >= 8 && K % 8 == 0 && (size_t)K * 2 <= 150 * 1024 && units >= 1 && units <= (int64_t)64 * 16 * g.num_cus;
}
static inline bool f16_weight_ok(const F16W &w) { return w.p && ((uintptr_t)w.p & 15) == 0 && w.ld % 8 == 0 && w.M >= 1; }
// the launches of the F16 plan for this shape
static bool f16_plan_shape_ok(const LlamaMatch &m) {
    return f16_launch_shape_ok(m.E, (m.E + 2 * m.Egqa) / 2) && f16_launch_shape_ok(m.E, m.F) && f16_launch_shape_ok(m.F, m.E) &&
           (!m.output || f16_launch_shape_ok(m.E, m.V)) && m.E % 2 == 0 && m.Egqa % 2 == 0 && m.D % 2 == 0;
}
// what the launches of the multi-token plan on k_mmvq_big8 need of N = 2..8 columns (kernels/decode_big8.h): 8 Q8 columns of the widest row in LDS
static bool multi_shape_ok(const LlamaMatch &m, int N) {
    const int64_t nbp = (std::max(m.E, m.F) / 32 + 63) / 64 * 64;
    return 8 * nbp * 40 <= 150 * 1024 && (int64_t)N * std::max(m.E, m.F) / 32 <= 4 * BIG_T;
}
// ---- the same launches on the integer matrix cores (kernels/mmq_cols.h) ----
struct ColsShape {
    int G, kc;
    size_t lds;
};
// grid and LDS of k_mmq_cols for `ngroups` 16-row groups (pairs for the gate) of nb blocks; G = 0: does not fit
static ColsShape cols_shape(int ngroups, int nsub, int nb) {
    ColsShape s{0, 0, 0};
    if (nb % 4 != 0 || nb < 32 || ngroups < 1) return s;
    const int max_groups = COLS_MAX_UNITS / nsub;  // per workgroup
    s.G = std::max(std::min(g.num_cus, ngroups), (ngroups + max_groups - 1) / max_groups);
    const int per = (ngroups + s.G - 1) / s.G;
    s.kc = 1;
    s.lds = (size_t)320 * nb + (size_t)per * nsub * COLS_W * 512;
    if (s.lds > 150 * 1024) s.G = 0, s.kc = 0;
    return s;
}
// whether a launch of the multi-token plan can run on k_mmq_cols (else k_mmvq_big8)
static bool cols_ok(int M_total, int nsub, int64_t nb, std::initializer_list<int64_t> Ms) {
    if (!g.opt_mmq_cols) return false;
    for (int64_t M : Ms)
        if (M % 16 != 0) return false;
    return cols_shape(M_total / 16 / nsub, nsub, (int)nb).kc > 0;
}
// the mat-vecs of a chunk (wq|wk|wv, wo, w1|w3, w2, lm_head) that run on k_mmq_cols; a chunk of more than 8 tokens needs all of them
struct MultiCols {
    bool qkv, wo, gate, w2, out;
};
static MultiCols multi_cols(const LlamaMatch &m) {
    const int64_t nbE = m.E / 32, nbF = m.F / 32;
    if (m.N < 2) return MultiCols{false, false, false, false, false};
    return MultiCols{cols_ok((int)(m.E + 2 * m.Egqa), 1, nbE, {m.E, m.Egqa}), cols_ok((int)m.E, 1, nbE, {m.E}),
                     cols_ok((int)(2 * m.F), 2, nbE, {m.F}), cols_ok((int)m.E, 1, nbF, {m.E}),
                     m.output != nullptr && cols_ok((int)m.V, 1, nbE, {m.V})};
}
// ---- the prompt plan's fused attention (kernels/prompt_attn.h): LDS bytes of a score row of T keys ----
static inline int prompt_attn_row_bytes(int64_t T) { return (int)(((T + 63) & ~(int64_t)63) * 4 + 16); }
// queries per workgroup the fused kernel takes rows of T keys with: 32, 16 (long rows), or 0 = the scores do not fit LDS
static inline int prompt_attn_queries(int64_t D, int64_t T) {
    if (!(D == 128 || D == 64 || D == 32)) return 0;
    if ((size_t)PATTN_Q * prompt_attn_row_bytes(T) <= 150 * 1024) return PATTN_Q;  // (row_bytes >= 272 >= the staged Q row)
    if ((size_t)16 * prompt_attn_row_bytes(T) <= 150 * 1024) return 16;
    return 0;
}
static inline bool prompt_attn_fits(int64_t D, int64_t T) { return prompt_attn_queries(D, T) != 0; }
// ---- a packed prompt batch (plan_pack.inc, kernels/prompt_pack.h): what plan_launch_prompt's three placing launches read instead of
// "rows n_past .. of one cache" — the tables of the call, on the device ----
struct PackLaunch {
    const int *pos;            // [R] the position of row r
    const int *row_seg;        // [R] its segment
    const PackSeg *segs;       // [L][n_segs]: layer il's table at segs + il * n_segs
    const PackTile *vtiles;    // [n_vtiles] 64-token V tiles
    const int *atiles;         // [n_atiles][2] attention tiles in dealing order
    int n_segs, n_vtiles, n_atiles;
    int64_t T_max;             // the longest n_past + N of the pack: the score rows' LDS
};
// ---- GGML_OP_FLASH_ATTN (kernels/flash_attn.h): queries per workgroup of the MFMA kernel k_flash_attn_tile — 32, 16 (long rows) —
// or 0: one row per workgroup (k_flash_attn_row).  The tile kernel takes f16 K/V of head size 32 / 64 / 128, at least two query
// rows, rows of at most FLASH_ATTN_MAX_KEYS_TILE keys (its score rows have k_p_attn's size) and reads K rows and V rows 16 bytes
// at a time: `aligned16` says that their first elements and every stride are multiples of 16.
static inline int flash_attn_tile_queries(bool kv_f16, int64_t D, int64_t N, int64_t M, bool aligned16) {
    if (!kv_f16 || N < 2 || !aligned16 || M > FLASH_ATTN_MAX_KEYS_TILE) return 0;
    return prompt_attn_queries(D, M);
}
