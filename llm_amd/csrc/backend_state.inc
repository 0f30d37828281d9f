// backend_state.inc — part of libggml_hip.so's backend translation unit (included by hip_backend.hip, inside its anonymous
// namespace where noted): fatal messages, the per-device-slot Backend state, initialisation, address translation (arena shadows), the graph workspace, pinned staging for host <-> device copies, per-class kernel timing.  Inside the anonymous namespace.

[[noreturn]] void die(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    fatal_note("%s", buf);
    abort();
}

int g_cur_slot();
struct Arena {
    uintptr_t base = 0;
    size_t size = 0;
    char *dev = nullptr;  // lazily allocated shadow
    bool live = true;
    bool is_scratch = false;  // registered through ggml_set_scratch (caller-owned Buffer, never unregistered)
};

// Record behind ggml_tensor.extra (and behind auto-uploaded persistent leaves).
struct DevTensor {
    uint32_t magic = 0x48495054;  // 'HIPT'
    int slot = (int)(g_cur_slot());  // the device slot that owns the copy
    uintptr_t host = 0;           // host data range this record mirrors
    size_t nbytes = 0;
    char *dev = nullptr;          // base of the device allocation
    size_t dev_bytes = 0;
    bool soa = false;             // quantized SoA layout (see QWeight)
    bool auto_uploaded = false;
    int refs = 1;                 // explicit records: tensors sharing this device copy
    bool zero_filled = false;     // created by assign_buffers_no_scratch (mutable state: never shared)
    uintptr_t owner_hdr = 0;      // auto-uploaded only: address of the ggml_tensor header that named this data
    QWeight qw{};
    char *w16 = nullptr;          // resident f16 copy of a quantized weight for the prompt GEMM (ensure_w16); qw.w16 names it
    size_t w16_size = 0;
    bool ksoa = false;            // K-quant planar layout (see KWeight, kernels/kquant.h)
    KWeight kw{};
    ggml_type type = GGML_TYPE_F32;
    int64_t ne[4] = {0, 0, 0, 0};
};

struct Timing {
    bool on = false;
    struct Rec {
        hipEvent_t a, b;
    };
    std::vector<Rec> recs[GGML_HIP_KCLASS_COUNT];
    std::vector<Rec> pool;
    double bytes[GGML_HIP_KCLASS_COUNT] = {0, 0, 0, 0};
    int64_t launches[GGML_HIP_KCLASS_COUNT] = {0, 0, 0, 0};
};

// One instance per device a process drives ("slot").  The reference's hooks address devices by index
// (ggml_cuda_set_main_device, crates/ggml/sys/src/cuda.rs:62; the split fractions of ggml_cuda_set_tensor_split, :11): here
// set_main_device makes a slot CURRENT and every entry point acts on the current slot — its stream, arena shadows, weight
// records, plan cache, options.  A session that spans several GPUs (the ggml-style layer split, host/llm_host.cpp) keeps the
// layers of a stage on one slot and switches slots between stages; the residual crosses with ggml_hip_copy_between_devices.
// GGML_HIP_VIRTUAL_DEVICES=n maps n slots onto the visible devices round-robin (several slots on ONE GPU: how the split is
// tested on a 1-GPU box).  One thread drives a SLOT at a time (Backend::mu); slots run concurrently.
#define GGML_HIP_MAX_BACKENDS 16
struct DecodePlan;  // plan_shapes.inc
struct PrepMatch;   // plan_run.inc
struct Backend {
    int slot = 0;
    bool inited = false;
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;  // != nullptr while `stream` is another slot's (ggml_hip_share_stream): this slot's own, to come back to
    std::recursive_mutex mu;       // serialises the entry points that act on this slot (SlotLock)
    hipEvent_t xfer_ev = nullptr;  // ggml_hip_copy_between_devices: "what this slot's stream has enqueued so far"
    int opt_fuse_heads = 1, opt_attn_one = 1, opt_attn_split = 1;  // options: what each means is said once, at its row of g_options below
    std::map<uintptr_t, Arena> arenas;          // by base
    std::map<uintptr_t, DevTensor *> tensors;   // explicit records (transform_tensor / assign_buffers_no_scratch)
    std::map<uintptr_t, DevTensor *> auto_tensors;  // persistent leaves uploaded on first use (never offloaded by
                                                    // the caller); evicted when their host range is recycled
    // per-graph workspace (activation re-quantization, temp SoA): bump allocator over chunks; chunks
    // added mid-graph stay alive until the next graph starts, where they are merged into one.
    struct WsChunk {
        char *p;
        size_t size;
    };
    std::vector<WsChunk> ws_chunks;
    size_t ws_off = 0;  // offset in the last chunk
    Timing timing;
    int opt_fuse = 1, opt_plan = 1, opt_plan_k = 1, opt_plan_multi = 1, opt_plan_prompt = 1, opt_graph = 1, opt_big = 1, opt_kbig = 1;
    int opt_chain_k = 0, opt_prepare = 1, opt_plan_batch = 1, opt_plan_f16 = 1, opt_plan_batch_chain = 1, opt_plan_batch_sample = 1, opt_plan_sample_chain = 1, opt_plan_batch_k = 0, opt_plan_out_k = 1, opt_plan_mpt = 0;
    int opt_fuse_attn = 1, opt_fuse_wo = 1, opt_warm_mb = 24, opt_affine = 1;
    int opt_act_quant = 0, opt_mmq_i8 = 0;
    int opt_mmq_min = 32, opt_k_prompt_min = 12, opt_mmq_fuse = 3, opt_mmq_cols = 1, opt_mmq_t256 = 1, opt_attn_fused = 1;
    int opt_mmq_w16 = 1, opt_w16_headroom_gb = 16;
    int opt_probe = 0;
    std::atomic<size_t> w16_bytes{0};  // HBM held by the resident f16 weight copies (a sibling slot of the device adds to it when IT builds a copy of this slot's record)
    uint64_t w16_gen = 1;    // bumped when copies are released: cached prompt plans re-resolve their pointers
    int num_cus = 256;
    long long *timeline = nullptr;  // device buffer of in-kernel timestamps (the timeline option)
    size_t timeline_bytes = 0;
    int timeline_wgs = 4;  // sampled workgroups per launch
    // counters: what each counts is said once, at its row of g_counters below
    uint64_t stat_plan_tokens = 0, stat_generic_graphs = 0, stat_split_tokens = 0, stat_prompt_plan_tokens = 0, stat_fused_tokens = 0, stat_kplan_tokens = 0, stat_fused_heads_tokens = 0, stat_fused_wo_tokens = 0, stat_fused_affine_tokens = 0, stat_prepared_tokens = 0;
    uint64_t stat_alibi_fused = 0;
    uint64_t stat_batch_tokens = 0, stat_batch_steps = 0, stat_batch_chain_steps = 0, stat_batch_chain_tokens = 0;
    uint64_t stat_batch_sample_steps = 0, stat_batch_sample_tokens = 0, stat_batch_k_steps = 0, stat_out_k_tokens = 0, stat_mpt_plan_tokens = 0;
    uint64_t stat_sample_chain_steps = 0, stat_sample_chain_tokens = 0;
    // the chains that stop (plan_run.inc chain_req_run): steps per group behind which the host looks at the columns' live flags, the
    // pinned words the flags are copied into (two sets: the host reads one while the next group's copy is in flight) and their events
    int opt_chain_group = 8;
    int *chain_live_pin = nullptr;
    hipEvent_t chain_live_ev[2] = {nullptr, nullptr};
    uint64_t stat_chain_stopped_columns = 0, stat_chain_frozen_steps = 0, stat_chain_steps_cut = 0;
    // the request pools (plan_pool.inc): the pinned words the pool's head is copied into behind a group of steps (two sets, as the
    // live flags above) and their events
    int opt_plan_batch_pool = 1;
    PoolHead *pool_pin = nullptr;
    hipEvent_t pool_ev[2] = {nullptr, nullptr};
    uint64_t stat_pool_calls = 0, stat_pool_admitted = 0, stat_pool_steps = 0;
    // the packed prompt batch (plan_pack.inc)
    int opt_plan_prompt_pack = 1;
    uint64_t stat_prompt_pack_calls = 0, stat_prompt_pack_segments = 0, stat_prompt_pack_tokens = 0;
    uint64_t stat_flash_attn_nodes = 0;
    // prompt-GEMM launches by kernel (ggml_hip_get_stat("mmq_launches_<name>")): bench.py labels its MFMA roofline with the
    // kernels that actually ran
    enum { MMQ_K_PLAIN, MMQ_K_DMA_P8, MMQ_K_W16_P8, MMQ_K_W16_256, MMQ_K_I8, MMQ_K_COUNT };
    uint64_t stat_mmq[MMQ_K_COUNT] = {0, 0, 0, 0, 0};
    DecodePlan *chain_plan = nullptr;      // the plan a greedy chain may continue (set by its last single-token run)
    ggml_cgraph *chain_graph = nullptr;    // ... and the cgraph that run executed
    bool pending_wait = false;  // a decode plan was launched by graph_compute_begin and not yet waited for
    bool pending_light = false;  // ... and it was a multi-token plan run: no in-launch waits (no error word to look at); if it also queued no read-back, the next begin() need not wait for it
    // One token ahead of a greedy caller (plan_run.inc): a single-token plan run whose caller is known to take the first maximum next —
    // ggml_hip_expect_greedy_next said so for this evaluation, or option speculate_next says so for every one — runs as a graph that
    // ends in k_token_tail: the device samples the greedy token itself, writes the next replay's parameters and stores the token's
    // results into a pinned slot; the NEXT token's graph is launched right behind it.  If the caller's next ggml_graph_compute asks
    // for exactly that (same plan, position + 1, the same token) its results are already on their way: a hit enqueues one graph
    // launch and one event record, and nothing but kernels sits between two token graphs.  Anything else simply runs behind the
    // ahead run (which wrote only plan-private buffers and the K/V row of a position the session has not reached).
    int opt_speculate_next = 0, opt_token_tail = 1, opt_tail_prepare = 1;
    bool greedy_hint = false;  // ggml_hip_expect_greedy_next: consumed by the next graph of this slot
    struct Spec {
        bool pending = false;
        DecodePlan *plan = nullptr;
        int n_past = 0, av = 0;
        int parity = 0;                 // the result set / slot the ahead run fills
        bool prepared = false;          // it ran as a TAIL_AHEAD graph: no prologue launch (stat tail_prepared_tokens on a hit)
        int32_t fed_id = 0;             // the token the device fed it: the id that came with the previous token's slot ...
        bool fed_id_valid = false;      // ... once that slot has been delivered (token_finish): the hit check needs no synchronisation
        int cooldown = 0;               // evaluations to sit out after a miss
    } spec;
    struct TailWait {                   // the token whose results the host takes from a slot: set by begin, consumed by token_finish
        DecodePlan *plan = nullptr;
        int q = 0;
        void *logits_dst = nullptr, *emb_dst = nullptr;
        bool staged = false;            // its parameters went up through the small staging: free again once its event is done
    } tail;
    DecodePlan *res_plan = nullptr;     // the most recently evaluated plan while its last token sits in result set 1 (DecodePlan::cur_set); null: set 0 everywhere (res_settle)
    uint64_t stat_tail_tokens = 0, stat_result_copies = 0, stat_tail_hits = 0, stat_tail_misses = 0;
    uint64_t stat_spec_hits = 0, stat_spec_misses = 0, stat_tail_prepared_tokens = 0;
    // in-launch hand-offs that gave up (kernels/common.h GRAN_SPIN_MAX): the plan's error word travels back with every token's
    // results (plan_run.inc token_finish)
    unsigned *ferr_pin = nullptr;    // the slot's error word: pinned HOST memory the kernels write straight into (zero-copy; written
                                     // only when a wait gives up, read by the host behind every token's result wait: no copy per token)
    DecodePlan *ferr_plan = nullptr; // the plan whose token is in flight
    int opt_fused_fallback = 1, opt_fused_rearm_tokens = 256;
    uint64_t fused_rearm_at = 0;     // stat_plan_tokens at which the saved options come back (0 = nothing to restore)
    uint64_t fused_rearm_stretch = 0;
    int fused_saved_fuse_attn = 0, fused_saved_attn_one = 0;
    uint64_t stat_fused_rearms = 0;
    uint64_t stat_cols_warm_launches = 0;
    int opt_test_fused_timeout = 0;
    uint64_t stat_fused_timeouts = 0;  // tokens the host saw the error word for (re-run or fatal)
    uint64_t ns_match = 0, ns_launch = 0, ns_wait = 0, ns_compute = 0, ns_mirror = 0, stat_mirror_bytes = 0;
    size_t dead_shadow_bytes = 0;
    uint64_t arena_seen = 0;  // the last event of the process-wide arena log this slot has applied (sync_arenas)
    PrepMatch *prep = nullptr;  // (plan_run.inc) the match of a graph handed over by ggml_hip_graph_prepare, waiting for its begin()
    int opt_gen = 0;       // bumped by every ggml_hip_set_option: a remembered match does not outlive an option change
    int xcd_labels = -1;  // 1: workgroups with equal blockIdx mod 8 of a one-workgroup-per-CU launch share an XCD, eight labels on eight XCDs (xcd_labels_ok); -1 = not looked yet
    void *hot_line = nullptr;  // 256 zero bytes on the device: what the dummy ring steps of the K plan's mat-vecs read (kernels/kquant_big.h KBigArgs::hot)
    int session_records = 0;  // zero-filled (mutable session state) records alive on this slot, see g_dev_slots
};
// The runtime options: one row per key of ggml_hip_set_option / ggml_hip_get_option.  The row is the only place that says what a
// key means, which field holds it and how it is applied; the environment variable of a key is GGML_HIP_<KEY IN CAPITALS>.  A new
// option is one row here (and one case in ggml_hip_internal_set_option_here if storing the value is not all it does).
enum : unsigned {
    OPT_ENV = 1,     // has an environment variable, stored into the field when a slot is initialised (the option log is replayed after it)
    OPT_DROPS = 2,   // cached plans froze the value: a change drops them
    OPT_DEVICE = 4,  // acts on an initialised device: only logged while no slot exists
    OPT_ACTION = 8,  // does something now and holds no state: never logged, reads back as -1
};
enum OptEffect { FX_NONE, FX_ACT_QUANT, FX_TIMELINE, FX_MMQ_W16, FX_W16_RELEASE, FX_FUSE_ATTN, FX_SPECULATE_NEXT, FX_FUSED_REARM_TOKENS, FX_TEST_FUSED_TIMEOUT, FX_SERIAL_STAGE_SLOTS };
struct OptRow {
    const char *key;
    int Backend::*field;  // nullptr: the state lives elsewhere (see the row's effect)
    unsigned flags;
    OptEffect fx = FX_NONE;  // what setting it does besides the store (ggml_hip_internal_set_option_here)
    int lo = 0, hi = -1;     // lo <= hi: the value is clamped to [lo, hi]
};
static const OptRow g_options[] = {
    // ---- plans
    {"fuse", &Backend::opt_fuse, OPT_ENV},  // peephole fusion in the node-by-node executor
    {"plan", &Backend::opt_plan, OPT_ENV},  // recognise the LLaMA decode graph and run the fused plan
    // ... and the K plan for a model whose matrices are K-quants (plan_decode.inc plan_launch_k); 2 = one launch per matrix
    {"plan_k", &Backend::opt_plan_k, OPT_ENV | OPT_DROPS},
    // ... and the F16 plan for a model whose matrices are F16 (plan_decode.inc plan_launch_f16); 0 = such a model runs node by node
    {"plan_f16", &Backend::opt_plan_f16, OPT_ENV | OPT_DROPS},
    // ... and the block formats' plans for a block-format model whose output matrix alone is a K-quant (what llama.cpp's quantizer writes:
    // LlamaMatch::out_k, the lm_head as the K plan's launches); 0 = such a model runs node by node
    {"plan_out_k", &Backend::opt_plan_out_k, OPT_ENV | OPT_DROPS},
    // ... and the MPT plan for the single-token graph of an MPT model with block-format weights (plan_match.inc match_mpt_decode,
    // plan_decode.inc plan_launch_mpt: five launches per layer).  The default is 0 ONLY because tests/test_alibi_families_gpu.py, written
    // before it, pins "single-token MPT steps run on the executor" (generic_graphs + 3, plan_tokens unchanged, alibi_fused per chunk and
    // layer): at 0 nothing behaves differently from before the option existed — the plan_batch_k precedent.  Making it 1 is a change to
    // those pins and to this initialiser, nothing else.
    {"plan_mpt", &Backend::opt_plan_mpt, OPT_ENV | OPT_DROPS},
    {"plan_multi", &Backend::opt_plan_multi, OPT_ENV | OPT_DROPS},    // fused plan for prompt chunks of 2..8 tokens (kernels/decode_big8.h)
    {"plan_prompt", &Backend::opt_plan_prompt, OPT_ENV | OPT_DROPS},  // fused plan for prompt batches of >= mmq_min tokens (kernels/prompt.h)
    // ggml_hip_decode_batch: one decode step of 2..8 sessions of one model as one pass over the weights (0: it answers -1, the caller steps them one by one)
    {"plan_batch", &Backend::opt_plan_batch, OPT_ENV | OPT_DROPS},
    // ... and of a K-quant model, on the K plan's chunk form (plan_launch_k; needs plan_k and plan_batch on).  The default is 0 ONLY
    // because three GPU tests written before it pin "a Q4_K model at default options is declined and runs one by one" (the q4_k cases
    // of tests/test_batch_decode_gpu.py, test_batch_chain_gpu.py and test_batch_sample_gpu.py): at 0 nothing behaves differently from
    // before the option existed.  Making it 1 is a change to those three cases and to this initialiser, nothing else.
    {"plan_batch_k", &Backend::opt_plan_batch_k, OPT_ENV | OPT_DROPS},
    // ggml_hip_decode_batch_greedy: n greedy steps of those sessions with the argmax on the device, the step's graph replayed (0: it
    // answers -1, the caller takes n single steps).  It shapes no plan: the chain replays the graph of ggml_hip_decode_batch.
    {"plan_batch_chain", &Backend::opt_plan_batch_chain, OPT_ENV},
    // ggml_hip_decode_batch_sampled: the same chain with the top-k / top-p / temperature sampler on the device (0: it answers -1, the
    // caller samples on the host and takes single steps).  It shapes no plan either.
    {"plan_batch_sample", &Backend::opt_plan_batch_sample, OPT_ENV},
    // ggml_hip_decode_pool_requests: ended columns take waiting requests on the device (0: the entry declines, callers step)
    {"plan_batch_pool", &Backend::opt_plan_batch_pool, OPT_ENV},
    // ggml_hip_prompt_pack: the prompt rows of up to 64 sessions as one pass of the prompt plan (0: the entry declines, callers feed one by one)
    {"plan_prompt_pack", &Backend::opt_plan_prompt_pack, OPT_ENV},
    // ggml_hip_decode_sampled_chain: n tokens of ONE session with that sampler on the device between two replays of its single-token
    // plan (0: it answers -1, the caller samples on the host and evaluates token by token).  It shapes no plan.
    {"plan_sample_chain", &Backend::opt_plan_sample_chain, OPT_ENV},
    {"graph", &Backend::opt_graph, OPT_ENV},                          // replay the plan from a captured hipGraph
    {"big", &Backend::opt_big, OPT_ENV | OPT_DROPS},                  // decode mat-vec as one wave of 1024-thread workgroups (kernels/decode_big.h)
    // K plan: its decode mat-vecs as one wave of 1024-thread workgroups that stage the activation themselves (kernels/kquant_big.h)
    {"kbig", &Backend::opt_kbig, OPT_ENV | OPT_DROPS},
    {"chain_k", &Backend::opt_chain_k, OPT_ENV, FX_NONE, 0, 64},  // greedy chain: tokens per hipGraph launch (0 / 1 = one token per launch)
    // the chains that stop (ggml_hip_decode_chain_requests / ggml_hip_decode_batch_requests): steps enqueued between two looks at the
    // columns' live flags; a call whose columns cannot end early never looks.  8: the smallest group whose median lay inside the
    // no-stop run's own spread (DESIGN section 3 item 5; 8 .. 64 all did, one session and B = 8)
    {"chain_group", &Backend::opt_chain_group, OPT_ENV, FX_NONE, 1, 4096},
    // ggml_hip_graph_prepare remembers its match (0: it answers 0 and every begin() matches its graph itself)
    {"prepare", &Backend::opt_prepare, OPT_ENV},
    // 1 = run the greedy next token ahead behind every single-token plan run, whoever the caller is (Backend::spec, plan_run.inc)
    {"speculate_next", &Backend::opt_speculate_next, OPT_ENV, FX_SPECULATE_NEXT},
    // 0 = no token runs ahead of its caller, whatever ggml_hip_expect_greedy_next or speculate_next say: every single-token plan run
    // takes the plain graph and the staged result copies
    {"token_tail", &Backend::opt_token_tail, OPT_ENV, FX_SPECULATE_NEXT},
    // a greedy token's k_token_tail also prepares the next token (embedding row, RoPE table and epoch, saved cache rows: TailPrep), so
    // that the graph launched directly behind it opens with its layer-0 launch; the block-format plan on the big workgroups only.
    // 0 = every greedy token's graph opens with k_kv_row_save, get_rows and k_rope_table.  (The captured graphs froze it.)
    {"tail_prepare", &Backend::opt_tail_prepare, OPT_ENV | OPT_DROPS},
    // ---- the fused decode launch
    // decode: wq|wk|wv and the attention as ONE launch (kernels/decode_fused.h) where the mat-vec deals as evenly over the remaining
    // workgroups; 2 = wherever legal (tests); 0 = the two-launch pair.  An explicit choice outlives a pending re-arm.
    {"fuse_attn", &Backend::opt_fuse_attn, OPT_ENV | OPT_DROPS, FX_FUSE_ATTN},
    // ... and wo + residual as the second phase of that launch's mat-vec workgroups (the WO form), where this slot has the GPU to itself
    {"fuse_wo", &Backend::opt_fuse_wo, OPT_ENV | OPT_DROPS},
    // WO form: MB of the first rows of w1|w3 that the mat-vec workgroups pull into L2 while the attention runs (kernels/decode_fused.h
    // NextWarm); 0 = off.  LLaMA-7B Q4_0, all mat-vec launches of a token, one box: 0 MB 1.183 ms, 16 MB 1.145, 24 MB 1.123-1.125,
    // 28 MB 1.124, 32 MB 1.126, 40 MB 1.147, 50 MB 1.200 (8 x 4 MB of L2: ~3 MB per XCD is what stays)
    {"warm_mb", &Backend::opt_warm_mb, OPT_ENV | OPT_DROPS},
    // XCD-affine dealing of wq|wk|wv's rows in the fused launch: head h's rows come from the XCD its attention workgroup runs on,
    // through that L2 (BigArgs::aff_hpl)
    {"affine", &Backend::opt_affine, OPT_ENV | OPT_DROPS},
    // contexts beyond k_qkv_attn's register window: 2 / 4 attention workgroups per head inside the wq|wk|wv launch
    {"fuse_heads", &Backend::opt_fuse_heads, OPT_ENV | OPT_DROPS},
    {"attn_split", &Backend::opt_attn_split, OPT_ENV | OPT_DROPS},  // long contexts: attention split over positions too (kernels/decode_attn_split.h)
    {"attn_one", &Backend::opt_attn_one, OPT_ENV | OPT_DROPS},      // ... its three phases as ONE launch (k_attn_split_one) where every workgroup is resident
    // a token whose in-launch hand-off gave up: 1 = re-run it on the kernels that do not wait inside a launch and keep them; 0 = abort
    {"fused_fallback", &Backend::opt_fused_fallback, OPT_ENV},
    // ... and take the fused forms back once the slot has decoded this many tokens cleanly on the two-launch forms (whoever held the
    // compute units may be gone); every further give-up doubles the stretch (one hiccup used to cost the slot 9 % for the rest of
    // its life).  0 = never.  Setting it starts the stretch over.
    {"fused_rearm_tokens", &Backend::opt_fused_rearm_tokens, OPT_ENV, FX_FUSED_REARM_TOKENS},
    // ---- arithmetic
    // activation re-quantizer: 0 = ggml's AVX2 branch (id = 127/amax, round half to even: what the reference's build runs,
    // crates/ggml/sys/build.rs:46-62), 1 = its scalar branch (kernels/common.h); any other value counts as 1, and the environment
    // variable also takes the word "scalar".  Lives in the device's constant memory (apply_act_quant).
    {"act_quant", &Backend::opt_act_quant, OPT_ENV | OPT_DEVICE, FX_ACT_QUANT},
    // 1 = prompt GEMM on the integer matrix cores (kernels/mmq_i8.h): ggml's exact block dots (error 2e-5 * scale instead of 1.1e-3),
    // but the per-block scaling of every product is VALU-bound: 309 vs 464 TFLOP/s-equivalent on 7B Q4_0, so the f16 kernels stay
    // the default
    {"mmq_i8", &Backend::opt_mmq_i8, OPT_ENV},
    // ---- prompt GEMMs
    {"mmq_min", &Backend::opt_mmq_min, OPT_ENV},  // token count from which mul_mat runs on the MFMA GEMM (0 = never)
    // tokens from which a K-quant model's batch takes the prompt plan (f16 copies) instead of the K plan's multi-token form
    {"k_prompt_min", &Backend::opt_k_prompt_min, OPT_ENV},
    {"mmq_fuse", &Backend::opt_mmq_fuse, OPT_ENV},  // prompt plan: wq|wk|wv (bit 0) and w1|w3 (bit 1) as one GEMM launch each
    // prompt chunks of 2..8 tokens: mat-muls on the integer matrix cores (kernels/mmq_cols.h) instead of k_mmvq_big8
    {"mmq_cols", &Backend::opt_mmq_cols, OPT_ENV | OPT_DROPS},
    // prompt GEMM on 256 x 256 tiles (kernels/mmq_w16_256.h) where the launch fills the chip with them; 2 = wherever legal (tests)
    {"mmq_t256", &Backend::opt_mmq_t256, OPT_ENV | OPT_DROPS},
    // prompt plan: K.Q, softmax and V.P as one launch with the scores in LDS (kernels/prompt_attn.h)
    {"attn_fused", &Backend::opt_attn_fused, OPT_ENV},
    // prompt GEMM on resident f16 copies of the quantized weights when HBM has room (kernels/mmq_w16.h); the copies are a cache of
    // this option: 0 releases them
    {"mmq_w16", &Backend::opt_mmq_w16, OPT_ENV | OPT_DROPS | OPT_DEVICE, FX_MMQ_W16},
    // HBM that must stay free after a copy is made (KV caches, workspaces, other models)
    {"w16_headroom_gb", &Backend::opt_w16_headroom_gb, OPT_ENV},
    // drop the resident f16 weight copies now (they come back with the next prompt batch)
    {"w16_release", nullptr, OPT_DEVICE | OPT_ACTION, FX_W16_RELEASE},
    // ---- sessions / split
    // how many of a device's session slots are stages of ONE split session (g_dev_serial_stages, device_sharers): per device, not per slot
    {"serial_stage_slots", nullptr, 0, FX_SERIAL_STAGE_SLOTS},
    // ---- measurement and tests
    // in-kernel timestamps of the decode mat-vec launches (Backend::timeline): 1 = 4 sampled workgroups per launch, n > 1 = n of
    // them, 0 = off; reads back as the number of sampled workgroups.  Every call drops the plans and clears the buffer.
    {"timeline", nullptr, OPT_DEVICE, FX_TIMELINE},
    {"probe", &Backend::opt_probe, OPT_DROPS},  // measurement only: k_mmvq_big returns early (BigArgs::probe), tests/tools/launch_probe.py
    // test hook: layer 0's attention workgroups of k_qkv_attn poll granules nobody writes; turning it off forgets the hook's own
    // give-ups (they do not count against the rest of the process)
    {"test_fused_timeout", &Backend::opt_test_fused_timeout, OPT_DROPS, FX_TEST_FUSED_TIMEOUT},
};
// the row of `key`; an unknown key is fatal (`who`: the entry point that was asked)
const OptRow &opt_row(const char *key, const char *who) {
    for (const OptRow &o : g_options)
        if (!strcmp(o.key, key)) return o;
    die("%s: unknown key '%s'", who, key);
}
// the value a row stores for `v`
inline int opt_value(const OptRow &o, int v) {
    if (o.fx == FX_ACT_QUANT) return v ? 1 : 0;
    return o.lo <= o.hi ? std::min(o.hi, std::max(o.lo, v)) : v;
}
// what the environment says for a row (GGML_HIP_<KEY IN CAPITALS>), stored into *out; false: the row has no variable or it is not set
inline bool opt_env_value(const OptRow &o, int *out) {
    if (!(o.flags & OPT_ENV)) return false;
    std::string name = "GGML_HIP_";
    for (const char *c = o.key; *c; c++) name += (char)toupper((unsigned char)*c);
    const char *v = getenv(name.c_str());
    if (!v) return false;
    *out = o.fx == FX_ACT_QUANT ? (!strcmp(v, "scalar") || atoi(v) == 1) : opt_value(o, atoi(v));
    return true;
}
// The plain counters of ggml_hip_get_stat (the computed ones are in that function): the row says what the counter counts.
struct StatRow {
    const char *key;
    uint64_t Backend::*field;
};
static const StatRow g_counters[] = {
    {"plan_tokens", &Backend::stat_plan_tokens},                  // tokens executed by the fused decode plan
    {"fused_attn_tokens", &Backend::stat_fused_tokens},           // decode tokens whose attention rode in the wq|wk|wv launch
    {"fused_heads_tokens", &Backend::stat_fused_heads_tokens},    // ... whose k_qkv_attn had 2 / 4 attention workgroups per head
    {"fused_wo_tokens", &Backend::stat_fused_wo_tokens},          // ... whose wo + residual rode in that launch too (the WO form)
    {"fused_affine_tokens", &Backend::stat_fused_affine_tokens},  // ... whose wq|wk|wv rows were dealt XCD-affine and handed over through the XCD's L2
    {"attn_split_tokens", &Backend::stat_split_tokens},           // tokens whose attention ran split over positions
    {"kplan_tokens", &Backend::stat_kplan_tokens},                // decode tokens of K-quant models that ran as the K plan
    {"mpt_plan_tokens", &Backend::stat_mpt_plan_tokens},          // decode tokens of MPT models that ran as the MPT plan (option plan_mpt), evaluations and greedy chains; counted in plan_tokens too, never in generic_graphs
    {"out_k_tokens", &Backend::stat_out_k_tokens},                // tokens whose lm_head ran as the K launch inside a block-format plan (LlamaMatch::out_k); counted in plan_tokens / prompt_plan_tokens too
    {"prepared_tokens", &Backend::stat_prepared_tokens},          // decode tokens whose graph had been matched ahead of time (ggml_hip_graph_prepare)
    {"prompt_plan_tokens", &Backend::stat_prompt_plan_tokens},    // tokens executed by the fused prompt plan
    {"batch_decode_tokens", &Backend::stat_batch_tokens},         // decode tokens that ran as columns of a batched step (ggml_hip_decode_batch); counted in plan_tokens too
    {"batch_decode_steps", &Backend::stat_batch_steps},           // ... and the steps
    {"batch_k_steps", &Backend::stat_batch_k_steps},              // ... those of them that ran on a K plan (a K-quant model under option plan_batch_k); their tokens count in kplan_tokens too
    {"batch_chain_steps", &Backend::stat_batch_chain_steps},      // ... those of them that ran on device-sampled tokens (ggml_hip_decode_batch_greedy: all but a call's first)
    {"batch_chain_tokens", &Backend::stat_batch_chain_tokens},    // ... and their tokens
    {"batch_sample_steps", &Backend::stat_batch_sample_steps},    // batched steps that ran on tokens the device SAMPLED (ggml_hip_decode_batch_sampled: all but a call's first; not in batch_chain_*)
    {"batch_sample_tokens", &Backend::stat_batch_sample_tokens},  // ... and their tokens
    {"sample_chain_steps", &Backend::stat_sample_chain_steps},    // replays of a single-token plan on a token the device SAMPLED (ggml_hip_decode_sampled_chain: every token of a call); counted in plan_tokens too
    {"chain_stopped_columns", &Backend::stat_chain_stopped_columns},  // columns of the chains that stop that ended on one of their stop ids
    {"chain_frozen_steps", &Backend::stat_chain_frozen_steps},        // column-steps such a chain replayed for a column that had ended (the same token at the same position again)
    {"chain_steps_cut", &Backend::stat_chain_steps_cut},              // steps of such calls that were never launched: every column had ended
    {"pool_calls", &Backend::stat_pool_calls},                        // calls of ggml_hip_decode_pool_requests that ran
    {"pool_admitted", &Backend::stat_pool_admitted},                  // requests k_pool_admit moved from the queue into a column
    {"pool_steps", &Backend::stat_pool_steps},                        // their steps_run: steps up to the last evaluation any request took (what was launched counts in batch_decode_steps)
    {"prompt_pack_calls", &Backend::stat_prompt_pack_calls},          // calls of ggml_hip_prompt_pack that ran
    {"prompt_pack_segments", &Backend::stat_prompt_pack_segments},    // their graphs (one segment each)
    {"prompt_pack_tokens", &Backend::stat_prompt_pack_tokens},        // their rows (counted in prompt_plan_tokens too)
    {"sample_chain_tokens", &Backend::stat_sample_chain_tokens},  // ... and their tokens (one session a step: the same number, kept beside batch_sample_*)
    {"cols_warm_launches", &Backend::stat_cols_warm_launches},    // chunk-plan norm launches that carried warming workgroups (ColsWarm), counted when enqueued or captured
    {"fused_rearms", &Backend::stat_fused_rearms},                // times the fused forms came back after a clean stretch behind a give-up
    {"spec_hits", &Backend::stat_spec_hits},                      // evaluations that found their results already running (option speculate_next)
    {"spec_misses", &Backend::stat_spec_misses},                  // ... ahead runs nobody asked for
    {"tail_tokens", &Backend::stat_tail_tokens},                  // evaluations whose results came through k_token_tail's slot
    {"tail_hits", &Backend::stat_tail_hits},                      // ahead runs the caller's next evaluation asked for, however they were armed ...
    {"tail_misses", &Backend::stat_tail_misses},                  // ... and those it did not (a greedy-by-hint caller that keeps missing shows here)
    {"tail_prepared_tokens", &Backend::stat_tail_prepared_tokens},  // evaluations whose graph ran with no prologue launch (a hit on a TAIL_AHEAD graph: option tail_prepare)
    {"result_copies", &Backend::stat_result_copies},             // stream copies enqueued for parameters or results of single-token plan runs
    {"generic_graphs", &Backend::stat_generic_graphs},            // graphs run node by node
    {"alibi_fused", &Backend::stat_alibi_fused},                  // scale -> alibi -> diag_mask_inf -> soft_max chains (BLOOM, MPT) run as one launch (k_alibi_soft_max)
    {"flash_attn_nodes", &Backend::stat_flash_attn_nodes},        // GGML_OP_FLASH_ATTN nodes computed (one launch each: kernels/flash_attn.h)
    {"ns_match", &Backend::ns_match},      // host-side time split of plan tokens: ns spent recognising decode graphs
    {"ns_launch", &Backend::ns_launch},    // ... enqueueing (param upload, graph launch, read-back queue)
    {"ns_wait", &Backend::ns_wait},        // ... waiting for the device + copying results out
    {"ns_compute", &Backend::ns_compute},  // total inside ggml_graph_compute
    {"ns_mirror", &Backend::ns_mirror},    // generic graphs: host ns in download_outputs (the wait for the graph included)
    {"mirror_bytes", &Backend::stat_mirror_bytes},  // ... bytes of CPU-backend nodes copied back
};
// Locking.  Every device slot has its own recursive mutex (Backend::mu): an entry point locks the slot it acts on (SlotLock),
// so sessions on DIFFERENT slots (GPUs) of one process run concurrently — enqueue, device wait and read-back included —
// while calls on one slot are serialised (one stream, one workspace, one plan cache per slot).  g_mu guards the few
// process-wide settings (option log, split fractions) and is a LEAF lock: never held while a slot lock is taken.
// Two slots are only ever locked together by ggml_hip_copy_between_devices, in slot order.
std::recursive_mutex g_mu;
std::map<std::string, int> g_opt_log;  // every option set through ggml_hip_set_option: replayed by a slot initialised later
float g_tensor_split[GGML_HIP_MAX_BACKENDS] = {1.0f};  // [0] = the one float of ggml_hip_set_tensor_split; the rest stay 0
float g_layer_split[GGML_HIP_MAX_BACKENDS] = {0.0f};   // ggml_hip_set_layer_split
int g_layer_split_n = 0;
Backend g_backends[GGML_HIP_MAX_BACKENDS];
// The current slot is per THREAD (as the current device of the HIP runtime is).  ggml_hip_set_main_device — the
// reference's process-wide hook (crates/ggml/sys/src/cuda.rs:62) — sets the process default and pins the calling thread;
// a thread that never chose a slot follows the default at every entry point; ggml_hip_bind_thread_device pins the calling
// thread only (the session mirror binds a model's slot around each call with it, host/llm_host.cpp).
std::atomic<int> g_default_slot{0};
// Slots that drive one physical device share its compute units.  The fused decode launches (k_qkv_attn, k_attn_split_one)
// contain workgroups that WAIT for other workgroups of the same launch, which is only safe while every workgroup of the launch
// can be resident: with several slots on a device their attention workgroups together must leave the producers room, and the
// all-workgroups-wait form is refused outright (plan_shapes.inc fused_qkv_shape / attn_one_ok).  A slot counts while it holds
// mutable session state (zero-filled records: the K/V memory of a live session; Backend::session_records) — a slot that only
// keeps a model's weights launches nothing.  g_dev_gen moves whenever the count of a device changes, so that plans captured
// under another count re-capture.
std::atomic<int> g_dev_slots[64];   // slots of a device that hold session state right now (K/V memory, hand-off buffers)
std::atomic<uint64_t> g_dev_gen[64];
// bumped whenever a WEIGHT record of the device is freed: the decode plans of every slot of that device hold device addresses (and
// resident-copy pointers) of weight records, also of records a sibling slot owns (llm_start_session_on); a plan built under another
// value is discarded at its next lookup, under its own slot's lock (plan_run.inc try_decode_plan)
std::atomic<uint64_t> g_dev_wgen[64];
thread_local Backend *g_cur = &g_backends[0];
thread_local bool tl_pinned = false;
#define g (*g_cur)
int g_cur_slot() { return (int)(g_cur - g_backends); }
// Stage slots of ONE layer-split session that sit on one GPU (virtual slots: how the split is exercised on a 1-GPU box) never run
// at the same time — stage i + 1 waits for stage i's residual — so together they are ONE sharer of the device: the caller that
// builds the split says how many of the device's session slots are such stages (the serial_stage_slots option: the
// host mirror while exactly one split session is alive, 0 otherwise).  Round 5 counted them one by one and the stages lost the WO
// form of the fused launch (device_sharers() == 1): most of the 86 us per hop of profiles/r05_split2.json.
std::atomic<int> g_dev_serial_stages[64];
inline int device_sharers() {
    const int n = g_dev_slots[g.device & 63].load(std::memory_order_relaxed), ser = g_dev_serial_stages[g.device & 63].load(std::memory_order_relaxed);
    return std::max(1, n - (ser > 1 ? std::min(ser, n) - 1 : 0));
}
// other initialised slots that drive THIS slot's physical device, whether or not they hold session state right now: they may read
// this slot's weight records (a model on one slot, its sessions on siblings: llm_start_session_on) and cache pointers into them
inline int device_siblings() {
    int n = 0;
    for (int i = 0; i < GGML_HIP_MAX_BACKENDS; i++)
        if (&g_backends[i] != g_cur && g_backends[i].inited && g_backends[i].device == g.device) n++;
    return n;
}
void bind_device();
void sync_arenas();
std::atomic<int> g_calls_inside{0}, g_calls_inside_peak{0};  // threads inside entry points right now / the most ever (statistic)
thread_local int tl_lock_depth = 0;
struct SlotLock {  // first statement of an entry point: resolves this thread's slot and locks it
    Backend *b;
    void enter() {
        b->mu.lock();
        if (tl_lock_depth++ == 0) {
            const int n = g_calls_inside.fetch_add(1, std::memory_order_relaxed) + 1;
            int peak = g_calls_inside_peak.load(std::memory_order_relaxed);
            while (n > peak && !g_calls_inside_peak.compare_exchange_weak(peak, n, std::memory_order_relaxed)) {}
        }
    }
    SlotLock() {
        if (!tl_pinned) g_cur = &g_backends[g_default_slot.load(std::memory_order_relaxed)];
        b = g_cur;
        enter();
        if (b->inited) bind_device();
        sync_arenas();
    }
    explicit SlotLock(Backend *slot) : b(slot) { enter(); }  // a named slot (for_each_slot, frees on the owner slot)
    ~SlotLock() {
        if (--tl_lock_depth == 0) g_calls_inside.fetch_sub(1, std::memory_order_relaxed);
        b->mu.unlock();
    }
    SlotLock(const SlotLock &) = delete;
    SlotLock &operator=(const SlotLock &) = delete;
};
// a flag per slot for things done once per DEVICE (hipFuncSetAttribute acts on the current device's copy of a kernel)
struct DevOnce {
    bool done[GGML_HIP_MAX_BACKENDS] = {};
    bool first() {
        bool &d = done[g.slot];
        if (d) return false;
        d = true;
        return true;
    }
};
// Above the 64 KiB default a kernel must ask for its dynamic LDS, once per device.  Every launch that may need more goes through
// here first: `launch_lds` is what this launch takes, `max_bytes` the most its site ever asks for.  A launch below the default leaves
// the flag alone, so a later large one still opts in.
template <auto Kern>
void lds_opt_in(size_t launch_lds, size_t max_bytes) {
    static DevOnce opted;
    if (launch_lds > 64 * 1024 && opted.first())
        HIP_CHECK(hipFuncSetAttribute((const void *)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)max_bytes));
}

int kt_of(ggml_type t) {
    switch (t) {
        case GGML_TYPE_Q2_K: return KT_Q2_K;
        case GGML_TYPE_Q3_K: return KT_Q3_K;
        case GGML_TYPE_Q4_K: return KT_Q4_K;
        case GGML_TYPE_Q5_K: return KT_Q5_K;
        case GGML_TYPE_Q6_K: return KT_Q6_K;
        default: return -1;
    }
}
int qt_of(ggml_type t) {
    switch (t) {
        case GGML_TYPE_Q4_0: return QT_Q4_0;
        case GGML_TYPE_Q4_1: return QT_Q4_1;
        case GGML_TYPE_Q5_0: return QT_Q5_0;
        case GGML_TYPE_Q5_1: return QT_Q5_1;
        case GGML_TYPE_Q8_0: return QT_Q8_0;
        default: return -1;
    }
}
// The one place a run-time type becomes a template argument: f(std::integral_constant<int, QT_…>{}), and likewise for the K
// types and for a bool.  `bad`: what to die with for a type outside the five (the node-by-node executor's launches); without it
// such a type runs as Q8_0 / Q5_K, as the plans have always taken theirs (the matcher has checked it).
#define CT(x) (decltype(x)::value) /* the compile-time value of the argument a with_* helper hands to f */
template <class F>
void with_qt(int qt, F &&f, const char *bad = nullptr) {
    if (bad && (qt < QT_Q4_0 || qt > QT_Q8_0)) die("%s", bad);
    switch (qt) {
        case QT_Q4_0: f(std::integral_constant<int, QT_Q4_0>{}); break;
        case QT_Q4_1: f(std::integral_constant<int, QT_Q4_1>{}); break;
        case QT_Q5_0: f(std::integral_constant<int, QT_Q5_0>{}); break;
        case QT_Q5_1: f(std::integral_constant<int, QT_Q5_1>{}); break;
        default: f(std::integral_constant<int, QT_Q8_0>{}); break;
    }
}
template <class F>
void with_kt(int kt, F &&f) {
    switch (kt) {
        case KT_Q4_K: f(std::integral_constant<int, KT_Q4_K>{}); break;
        case KT_Q6_K: f(std::integral_constant<int, KT_Q6_K>{}); break;
        case KT_Q2_K: f(std::integral_constant<int, KT_Q2_K>{}); break;
        case KT_Q3_K: f(std::integral_constant<int, KT_Q3_K>{}); break;
        default: f(std::integral_constant<int, KT_Q5_K>{}); break;
    }
}
template <class F>
void with_bool(bool b, F &&f) {
    if (b)
        f(std::true_type{});
    else
        f(std::false_type{});
}
// the weight types whose activation rows get their block scale rounded to f16 first: the bool argument of the quantizing kernels
static inline bool qt_f16d(int qt) { return qt == QT_Q4_0 || qt == QT_Q5_0 || qt == QT_Q8_0; }

thread_local int tl_device = -1;  // the device this thread last made current
void bind_device() {
    if (tl_device != g.device) {
        HIP_CHECK(hipSetDevice(g.device));
        tl_device = g.device;
    }
}
// slots this process may address: GGML_HIP_VIRTUAL_DEVICES if set, else the visible devices
int slot_count() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    if (const char *v = getenv("GGML_HIP_VIRTUAL_DEVICES")) n = std::max(n, atoi(v));
    if (const char *v = getenv("GGML_HIP_SESSION_SLOTS")) n = std::max(n, atoi(v));  // (see auto_session_slot)
    return std::min(n, GGML_HIP_MAX_BACKENDS);
}
// Sessions of ONE model on several threads, for callers that change nothing (crates/llm-base/src/inference_session.rs:43-48: "spawn
// several InferenceSessions" — each on its own thread — and model/mod.rs:270-276: the model is Send + Sync).  Such a caller only
// ever says ggml_cuda_set_main_device(0) (accelerator::initialize, once per InferenceSession::new), so all its sessions would share
// slot 0: one stream, one lock, one after the other.  With GGML_HIP_SESSION_SLOTS=n (opt-in) the FIRST K/V memory a thread creates
// (ggml_hip_assign_buffers_no_scratch: InferenceSession::new) assigns the thread a slot among the n sibling slots of that GPU — the
// one with the fewest session threads so far, the asked-for slot on a tie — and pins it there: its K/V, arena shadows, plans and
// stream live on that slot, the weights are read from the slot that holds them (extra_of), and later set_main_device calls of the
// thread for the same GPU keep the assignment.  A session stays with the thread that created it (its records live on that
// thread's slot); llm_start_session_on remains the explicit form.
thread_local int tl_auto_slot = -1;  // the slot this thread's sessions were assigned (-1: none yet)
int g_session_threads[GGML_HIP_MAX_BACKENDS] = {};  // threads assigned per slot (guarded by g_mu)
inline int session_slots_env() {
    static const int n = getenv("GGML_HIP_SESSION_SLOTS") ? atoi(getenv("GGML_HIP_SESSION_SLOTS")) : 0;
    return n;
}
// The one statement of which GPU a slot drives: slot s drives physical device (base + s) mod n.  base: GGML_HIP_DEVICE (one
// process per GPU launchers set it to the local rank when they did not restrict visibility); several slots on one device when
// GGML_HIP_VIRTUAL_DEVICES asks for more slots than there are devices.  -1: no device.
inline int slot_physical_device(int slot) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return -1;
    int base = 0;
    if (const char *lr = getenv("GGML_HIP_DEVICE")) base = atoi(lr);
    return (base + slot) % n;
}
struct AutoSlotRelease {  // a thread that ends gives its place back
    ~AutoSlotRelease() {
        if (tl_auto_slot >= 0) {
            std::lock_guard<std::recursive_mutex> lk(g_mu);
            if (g_session_threads[tl_auto_slot] > 0) g_session_threads[tl_auto_slot]--;
        }
    }
};
thread_local AutoSlotRelease tl_auto_release;
// runs f with every slot current in turn (host-side bookkeeping that all slots share: arenas, options)
template <typename F>
void for_each_slot(F f) {  // one slot locked at a time; the caller holds no slot lock (g_mu is a leaf, see above)
    Backend *keep = g_cur;
    for (int i = 0; i < GGML_HIP_MAX_BACKENDS; i++) {
        SlotLock lk(&g_backends[i]);
        g_cur = &g_backends[i];
        g.slot = i;
        if (g.inited) bind_device();
        f();
    }
    g_cur = keep;
    if (g.inited) bind_device();
}
// the quantizer branch lives in the device's constant memory (kernels/common.h c_act_quant_scalar): one copy per device
void apply_act_quant() {
    if (!g.inited) return;
    bind_device();
    HIP_CHECK(hipStreamSynchronize(g.stream));
    const int v = g.opt_act_quant;
    HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(c_act_quant_scalar), &v, sizeof(v)));
    if (mpt_plan_set_act_quant(v)) die("option act_quant: the MPT plan's code object did not take it");  // (its own copy of the constant: mpt_plan.hip)
}
void ensure_init() {
    if (g.inited) {
        bind_device();
        return;
    }
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        die("no HIP device available (hipGetDeviceCount -> %d, n=%d). This library has no CPU compute path.", (int)e, n);
    g.slot = (int)(g_cur - g_backends);
    g.device = slot_physical_device(g.slot);
    if (g.device >= 64) die("device index %d: the per-device tables of this library hold 64 GPUs", g.device);
    HIP_CHECK(hipSetDevice(g.device));
    tl_device = g.device;
    HIP_CHECK(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking));
    for (const OptRow &o : g_options) {  // the environment: stored straight into the field; the option log below wins over it
        int v = 0;
        if (opt_env_value(o, &v)) g.*o.field = v;
    }
    {
        hipDeviceProp_t prop;
        HIP_CHECK(hipGetDeviceProperties(&prop, g.device));
        g.num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        if (const char *v = getenv("GGML_HIP_BIG_WGS")) g.num_cus = std::max(1, atoi(v));
    }
    g.inited = true;
    apply_act_quant();  // several slots may share a device: the last writer wins, and all slots hold the same option
    std::map<std::string, int> log;
    {
        std::lock_guard<std::recursive_mutex> lk(g_mu);  // leaf lock: copied, then applied without it
        log = g_opt_log;
    }
    for (auto &kv : log) ggml_hip_internal_set_option_here(kv.first.c_str(), kv.second);
}

// ---------------------------------------------------------------------------------------------------
// host arenas: a process-wide event log, applied by every slot at its own pace
// ---------------------------------------------------------------------------------------------------
// Host arenas (ggml context buffers, scratch buffers) are known to every slot — a context made while one device is current may
// be used while another is — but each slot owns its device shadows.  ggml_init / ggml_free / ggml_set_scratch only APPEND an
// event here (a leaf mutex, no slot lock): the session mirror recreates its graph arena for every token, and taking every
// slot's lock for that made a session wait for whatever another session's slot was doing (a whole token's device wait).  A slot
// replays the events it has not seen yet at its next entry point, under its own lock, in order — so its view of the arenas is
// exactly what eager registration gave it, later.  The log keeps the last ARENA_LOG_KEEP events; a slot further behind than that
// (or not initialised when they happened) rebuilds its view from the live set.
struct ArenaEvent {
    uint64_t seq;
    bool reg;
    uintptr_t base;
    size_t size;
    int is_scratch;
};
std::mutex g_arena_mu;
std::deque<ArenaEvent> g_arena_log;
std::map<uintptr_t, std::pair<size_t, int>> g_arena_live;  // base -> (size, is_scratch) of every registered arena
std::atomic<uint64_t> g_arena_seq{0};
static const size_t ARENA_LOG_KEEP = 4096;
void arena_event(bool reg, void *host_base, size_t size, int is_scratch) {
    if (reg && size == 0) return;
    std::lock_guard<std::mutex> lk(g_arena_mu);
    const uintptr_t b = (uintptr_t)host_base;
    if (reg) {
        auto same = g_arena_live.find(b);
        if (same != g_arena_live.end() && same->second.first == size && same->second.second == is_scratch)
            return;  // already registered as it is (ggml_set_scratch names the same buffer for every layer of every graph)
        for (auto it = g_arena_live.begin(); it != g_arena_live.end();)  // what the new range overlaps is gone (recycled host memory)
            if (it->first < b + size && b < it->first + it->second.first && it->first != b) it = g_arena_live.erase(it);
            else ++it;
        g_arena_live[b] = {size, is_scratch};
    } else {
        g_arena_live.erase(b);
    }
    const uint64_t seq = g_arena_seq.load(std::memory_order_relaxed) + 1;
    g_arena_log.push_back({seq, reg, b, size, is_scratch});
    if (g_arena_log.size() > ARENA_LOG_KEEP) g_arena_log.pop_front();
    g_arena_seq.store(seq, std::memory_order_release);
}
void register_arena_here(void *host_base, size_t size, int is_scratch);
void unregister_arena_here(void *host_base);
void evict_all_auto_tensors();
// called with the current slot locked (SlotLock): applies the arena events this slot has not seen
void sync_arenas() {
    const uint64_t target = g_arena_seq.load(std::memory_order_acquire);
    if (g.arena_seen == target) return;
    std::vector<ArenaEvent> todo;
    std::map<uintptr_t, std::pair<size_t, int>> live;
    bool full = false;
    uint64_t upto;
    {
        std::lock_guard<std::mutex> lk(g_arena_mu);
        upto = g_arena_seq.load(std::memory_order_relaxed);
        if (g_arena_log.empty() || g.arena_seen + 1 < g_arena_log.front().seq) {
            full = true;
            live = g_arena_live;
        } else {
            for (auto &e : g_arena_log)
                if (e.seq > g.arena_seen) todo.push_back(e);
        }
    }
    if (full) {
        std::vector<uintptr_t> gone;
        for (auto &kv : g.arenas) {
            auto it = live.find(kv.first);
            if (kv.second.live && (it == live.end() || it->second.first != kv.second.size)) gone.push_back(kv.first);
        }
        for (uintptr_t b : gone) unregister_arena_here((void *)b);
        if (g.arena_seen != 0) evict_all_auto_tensors();  // re-registrations this slot slept through may have recycled their bytes
        for (auto &kv : live) register_arena_here((void *)kv.first, kv.second.first, kv.second.second);
    } else {
        for (auto &e : todo) {
            if (e.reg)
                register_arena_here((void *)e.base, e.size, e.is_scratch);
            else
                unregister_arena_here((void *)e.base);
        }
    }
    g.arena_seen = upto;
}

// ---------------------------------------------------------------------------------------------------
// address translation
// ---------------------------------------------------------------------------------------------------
Arena *find_arena(uintptr_t p) {
    auto it = g.arenas.upper_bound(p);
    if (it == g.arenas.begin()) return nullptr;
    --it;
    Arena &a = it->second;
    if (p >= a.base && p < a.base + a.size && a.live) return &a;
    return nullptr;
}
DevTensor *find_in(std::map<uintptr_t, DevTensor *> &m, uintptr_t p) {
    auto it = m.upper_bound(p);
    if (it == m.begin()) return nullptr;
    --it;
    DevTensor *t = it->second;
    if (p >= t->host && p < t->host + std::max<size_t>(t->nbytes, 1)) return t;
    return nullptr;
}
// explicit records never overlap each other (enforced at registration), so the nearest base below p decides;
// auto records are consulted second and are evicted whenever anything else claims their host range.
DevTensor *find_tensor(uintptr_t p) {
    if (DevTensor *t = find_in(g.tensors, p)) return t;
    return find_in(g.auto_tensors, p);
}
void destroy_record(DevTensor *e);
size_t release_w16_copies();
// Every device allocation of the library goes through here.  The resident f16 weight copies of the prompt GEMM
// (ensure_w16) are a CACHE: when HBM runs out (a second model, a long-context KV cache, score workspaces) they are
// released, the plans that name them dropped, and the allocation retried before giving up.
void dev_malloc(void **p, size_t bytes, const char *what) {
    if (hipMalloc(p, bytes) == hipSuccess) return;
    (void)hipGetLastError();
    const size_t freed = release_w16_copies();
    if (freed && hipMalloc(p, bytes) == hipSuccess) {
        fprintf(stderr, "libggml_hip: released %.2f GB of resident f16 weight copies to allocate %.2f GB for %s\n", freed / 1e9,
                bytes / 1e9, what);
        return;
    }
    (void)hipGetLastError();
    size_t free_b = 0, total_b = 0;
    (void)hipMemGetInfo(&free_b, &total_b);
    die("out of device memory: %s needs %zu bytes, %zu of %zu free", what, bytes, free_b, total_b);
}
// drops every record of `m` whose host range intersects [b, b+size)
void evict_overlapping(std::map<uintptr_t, DevTensor *> &m, uintptr_t b, size_t size) {
    for (auto it = m.begin(); it != m.end();) {
        DevTensor *e = it->second;
        if (e->host < b + size && b < e->host + std::max<size_t>(e->nbytes, 1)) {
            it = m.erase(it);
            destroy_record(e);
        } else {
            ++it;
        }
    }
}
void ensure_init();
DevTensor *extra_of(const ggml_tensor *t) {
    DevTensor *e = (DevTensor *)t->extra;
    if (e && e->magic != 0x48495054) die("tensor '%s': extra does not belong to this backend", t->name);
    if (e && e->slot != g_cur_slot()) {
        // Slots that drive the SAME physical device may read each other's persistent tensors: several sessions of one model, each
        // on its own slot (stream, shadows, plan workspace), stream the one copy of the weights.  Mutable session state (K/V
        // memory, hand-off buffers: zero_filled records) stays private to the slot that made it.
        ensure_init();
        const Backend &o = g_backends[e->slot];
        if (!o.inited || o.device != g.device || e->zero_filled)
            die("tensor '%s' lives on device slot %d but slot %d is current (ggml_hip_set_main_device)", t->name, e->slot, g_cur_slot());
    }
    return e;
}
char *arena_dev(Arena *a) {
    if (!a->dev) {
        ensure_init();
        dev_malloc((void **)&a->dev, a->size, "an arena shadow");
    }
    return a->dev;
}

// Host tensors staged raw into the workspace for the current graph only (the src0 leaves of a quantized / f16 ADD, the
// LoRA patch: backend_executor.inc stage_add_targets).  Emptied with the workspace (ws_reset).
struct Staged {
    uintptr_t host;
    size_t nbytes;
    char *dev;
};
std::vector<Staged> g_staged_[GGML_HIP_MAX_BACKENDS];
#define g_staged (g_staged_[g.slot])

// device address of the raw bytes of `t` (strided views included). Aborts for SoA weights.
char *dev_ptr(const ggml_tensor *t) {
    if (DevTensor *e = extra_of(t)) {
        if (e->soa) die("tensor '%s' is a re-laid-out quantized weight; only mul_mat/get_rows may read it", t->name);
        return e->dev + ((uintptr_t)t->data - e->host);
    }
    const uintptr_t p = (uintptr_t)t->data;
    if (p == 0) die("tensor '%s' has no data", t->name);
    for (const Staged &st : g_staged)
        if (p >= st.host && p < st.host + st.nbytes) return st.dev + (p - st.host);
    if (DevTensor *e = find_tensor(p)) {
        if (e->soa) die("tensor '%s' aliases a re-laid-out quantized weight", t->name);
        return e->dev + (p - e->host);
    }
    if (Arena *a = find_arena(p)) return arena_dev(a) + (p - a->base);
    die("tensor '%s' (op %s): data pointer %p is in no registered arena and has no device copy", t->name,
        ggml_op_name(t->op), t->data);
}

TView view_of(const ggml_tensor *t) {
    TView v;
    v.p = dev_ptr(t);
    for (int i = 0; i < 4; i++) {
        v.ne[i] = t->ne[i];
        v.nb[i] = (int64_t)t->nb[i];
    }
    return v;
}

// ---------------------------------------------------------------------------------------------------
// workspace
// ---------------------------------------------------------------------------------------------------
struct QActBuf {
    const void *src_data = nullptr;  // host address identity of the source tensor data
    size_t src_bytes = 0;
    bool f16_d = false;
    int64_t nb = 0, ncols = 0;
    QAct act{};
    bool valid = false;
} g_qact_[GGML_HIP_MAX_BACKENDS];
#define g_qact (g_qact_[g.slot])
struct XF16Buf {  // the prefill GEMM's activation operand (kernels/mmq.h), cached like g_qact
    const void *src_data = nullptr;
    size_t src_bytes = 0;
    bool f16_d = false;
    int64_t nb = 0, ncols = 0;
    const _Float16 *x = nullptr;
    bool valid = false;
} g_xf16_[GGML_HIP_MAX_BACKENDS];
#define g_xf16 (g_xf16_[g.slot])

char *ws_alloc(size_t bytes) {
    bytes = (bytes + 255) & ~(size_t)255;
    if (g.ws_chunks.empty() || g.ws_off + bytes > g.ws_chunks.back().size) {
        size_t total = 0;
        for (auto &c : g.ws_chunks) total += c.size;
        const size_t want = std::max<size_t>(std::max<size_t>(bytes, total), (size_t)256 << 20);
        Backend::WsChunk c{nullptr, want};
        dev_malloc((void **)&c.p, want, "the graph workspace");
        g.ws_chunks.push_back(c);
        g.ws_off = 0;
    }
    char *p = g.ws_chunks.back().p + g.ws_off;
    g.ws_off += bytes;
    return p;
}
// called at the start of every graph: rewind, and merge chunks that were added during the last graph
void ws_reset() {
    g.ws_off = 0;
    g_staged.clear();
    if (g.ws_chunks.size() <= 1) return;
    HIP_CHECK(hipStreamSynchronize(g.stream));
    size_t total = 0;
    for (auto &c : g.ws_chunks) {
        total += c.size;
        HIP_CHECK(hipFree(c.p));
    }
    g.ws_chunks.clear();
    Backend::WsChunk c{nullptr, total};
    dev_malloc((void **)&c.p, total, "the graph workspace");
    g.ws_chunks.push_back(c);
}

// ---------------------------------------------------------------------------------------------------
// host <-> device transfers through library-owned pinned staging.  Caller memory (ggml arenas, mmap'd
// weight files, numpy buffers) is pageable and may be unmapped/recycled at any time; copying through
// our own hipHostMalloc'd buffers keeps the runtime from pinning (and caching pins of) memory it does
// not own, and makes the small per-evaluation uploads truly asynchronous.
// ---------------------------------------------------------------------------------------------------
struct Staging {
    static constexpr size_t BIG = (size_t)32 << 20;   // bulk chunk (weights upload, large read-backs)
    static constexpr size_t SMALL = (size_t)8 << 20;  // per-graph bump region (token ids, constants, logits)
    char *big[2] = {nullptr, nullptr};
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool busy[2] = {false, false};
    int next = 0;
    char *small = nullptr;
    size_t small_off = 0;
    struct Pending {
        void *host_dst;
        const char *stage;
        size_t n;
    };
    std::vector<Pending> pending;  // D2H copies whose staging → user memcpy happens after the stream sync
} stg_[GGML_HIP_MAX_BACKENDS];
#define stg (stg_[g.slot])

void staging_init() {
    if (stg.small) return;
    for (int i = 0; i < 2; i++) {
        HIP_CHECK(hipHostMalloc((void **)&stg.big[i], Staging::BIG, hipHostMallocDefault));
        HIP_CHECK(hipEventCreateWithFlags(&stg.ev[i], hipEventDisableTiming));
    }
    HIP_CHECK(hipHostMalloc((void **)&stg.small, Staging::SMALL, hipHostMallocDefault));
}

// bulk upload; returns when the data has left `src` (the device copy is ordered on g.stream)
void h2d_bulk(char *dst, const void *src, size_t n) {
    staging_init();
    size_t off = 0;
    while (off < n) {
        const int b = stg.next;
        stg.next ^= 1;
        if (stg.busy[b]) {
            HIP_CHECK(hipEventSynchronize(stg.ev[b]));
            stg.busy[b] = false;
        }
        const size_t len = std::min(Staging::BIG, n - off);
        memcpy(stg.big[b], (const char *)src + off, len);
        HIP_CHECK(hipMemcpyAsync(dst + off, stg.big[b], len, hipMemcpyHostToDevice, g.stream));
        HIP_CHECK(hipEventRecord(stg.ev[b], g.stream));
        stg.busy[b] = true;
        off += len;
    }
}
// small asynchronous upload for the current graph (staging lives until the graph's final sync)
void h2d_small(char *dst, const void *src, size_t n) {
    staging_init();
    const size_t need = (n + 63) & ~(size_t)63;
    if (stg.small_off + need > Staging::SMALL) {
        h2d_bulk(dst, src, n);
        return;
    }
    char *s = stg.small + stg.small_off;
    stg.small_off += need;
    memcpy(s, src, n);
    HIP_CHECK(hipMemcpyAsync(dst, s, n, hipMemcpyHostToDevice, g.stream));
}
// read-back: queued on the stream now, delivered to user memory by d2h_finish() (which synchronises)
void d2h_queue(void *host_dst, const char *src, size_t n) {
    staging_init();
    const size_t need = (n + 63) & ~(size_t)63;
    if (stg.small_off + need > Staging::SMALL) {
        // large (the [V, N] logits of a prompt batch: 65 MB at N = 512): 8 MiB pieces, the DMA of piece i+1 into one
        // pinned buffer overlaps the copy of piece i out of the other; that copy is split over 4 threads (one
        // thread moves ~8 GB/s into pageable memory, which made the read-back ~20 % of a 512-token batch)
        const size_t PIECE = (size_t)8 << 20;
        for (int i = 0; i < 2; i++)
            if (stg.busy[i]) {
                HIP_CHECK(hipEventSynchronize(stg.ev[i]));
                stg.busy[i] = false;
            }
        auto par_copy = [](char *dst, const char *src_, size_t len) {
            const int nt = len >= ((size_t)2 << 20) ? 4 : 1;
            if (nt == 1) {
                memcpy(dst, src_, len);
                return;
            }
            std::thread th[3];
            const size_t part = (len / nt + 63) & ~(size_t)63;
            for (int t = 1; t < nt; t++) {
                const size_t o = (size_t)t * part;
                if (o < len) th[t - 1] = std::thread([=] { memcpy(dst + o, src_ + o, std::min(part, len - o)); });
            }
            memcpy(dst, src_, std::min(part, len));
            for (int t = 1; t < nt; t++)
                if (th[t - 1].joinable()) th[t - 1].join();
        };
        size_t off = 0;
        int cur = 0;
        size_t len = std::min(PIECE, n);
        HIP_CHECK(hipMemcpyAsync(stg.big[cur], src, len, hipMemcpyDeviceToHost, g.stream));
        HIP_CHECK(hipEventRecord(stg.ev[cur], g.stream));
        while (off < n) {
            const size_t noff = off + len, nlen = noff < n ? std::min(PIECE, n - noff) : 0;
            if (nlen) {
                HIP_CHECK(hipMemcpyAsync(stg.big[cur ^ 1], src + noff, nlen, hipMemcpyDeviceToHost, g.stream));
                HIP_CHECK(hipEventRecord(stg.ev[cur ^ 1], g.stream));
            }
            HIP_CHECK(hipEventSynchronize(stg.ev[cur]));
            par_copy((char *)host_dst + off, stg.big[cur], len);
            off = noff;
            len = nlen;
            cur ^= 1;
        }
        return;
    }
    char *s = stg.small + stg.small_off;
    stg.small_off += need;
    HIP_CHECK(hipMemcpyAsync(s, src, n, hipMemcpyDeviceToHost, g.stream));
    stg.pending.push_back({host_dst, s, n});
}
void d2h_finish() {
    HIP_CHECK(hipStreamSynchronize(g.stream));
    for (auto &p : stg.pending) memcpy(p.host_dst, p.stage, p.n);
    stg.pending.clear();
    stg.small_off = 0;
    stg.busy[0] = stg.busy[1] = false;
}

// ---------------------------------------------------------------------------------------------------
// timing (HIP events on the backend stream, per kernel class)
// ---------------------------------------------------------------------------------------------------
struct Timed {
    int k;
    Timing::Rec rec{};
    bool on;
    Timed(int kclass, double algo_bytes) : k(kclass), on(g.timing.on) {
        if (!on) return;
        if (!g.timing.pool.empty()) {
            rec = g.timing.pool.back();
            g.timing.pool.pop_back();
        } else {
            HIP_CHECK(hipEventCreate(&rec.a));
            HIP_CHECK(hipEventCreate(&rec.b));
        }
        HIP_CHECK(hipEventRecord(rec.a, g.stream));
        g.timing.bytes[k] += algo_bytes;
        g.timing.launches[k]++;
    }
    ~Timed() {
        if (!on) return;
        HIP_CHECK(hipEventRecord(rec.b, g.stream));
        g.timing.recs[k].push_back(rec);
    }
};

inline dim3 grid1(int64_t n, int bs = 256) { return dim3((unsigned)((n + bs - 1) / bs)); }
