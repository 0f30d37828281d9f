// llama_plan.inc — recognises the single-token LLaMA decode graph that crates/models/llama/src/lib.rs:166-362
// builds (37 nodes per layer + get_rows + final norm/mul/lm_head, rebuilt by the caller for EVERY token:
// crates/llm-base/src/inference_session.rs:230) and executes it as ~8 fused launches per layer (kernels/decode.h),
// captured once in a hipGraph and replayed for the following tokens with only {n_past, token} changing in a
// device-side parameter block.  Included inside hip_backend.hip's anonymous namespace.
//
// The matcher is structural (it follows src[] pointers from the logits back to get_rows and checks every view's
// shape/stride/offset against the KV-cache layout), so any graph that is not exactly the reference's LLaMA
// graph falls through to the generic per-node executor — same results, more launches.

struct LayerW {
    const ggml_tensor *attn_norm = nullptr, *wq = nullptr, *wk = nullptr, *wv = nullptr, *wo = nullptr,
                      *ffn_norm = nullptr, *w1 = nullptr, *w2 = nullptr, *w3 = nullptr;
    const ggml_tensor *cur = nullptr;  // the normed activation feeding wq/wk/wv (identity key for the KV stores)
    bool k_store = false, v_store = false;
};

static inline size_t attn_decode_lds(int64_t C, int64_t D) { return (size_t)(C + D) * 4 + (size_t)C * 2; }
static const size_t ATTN_DECODE_LDS_MAX = 150 * 1024;  // of the CU's 160 KiB (the kernel's static arrays take a little)
static void attn_decode_opt_in() {  // above the 64 KiB default a kernel must ask for its dynamic LDS once
    static DevOnce done;
    if (!done.first()) return;
    HIP_CHECK(hipFuncSetAttribute((const void *)k_attn_decode<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ATTN_DECODE_LDS_MAX));
    HIP_CHECK(hipFuncSetAttribute((const void *)k_attn_decode<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ATTN_DECODE_LDS_MAX));
}

// positions k_attn_decode's LDS arrays must hold for an evaluation of N tokens at context C
static inline int64_t attn_split_min(bool fused = true);
static inline int64_t attn_decode_rows(int64_t C, int N, int64_t H) {
    const bool split_from_min = N == 1 && g.opt_attn_split && g.opt_big && g.num_cus / std::max<int64_t>(1, H) >= 2;  // = long_ctx of try_decode_plan
    return split_from_min ? std::min<int64_t>(C, (attn_split_min() + 7) & ~(int64_t)7) : C;
}

static const int PROMPT_PLAN_MAX = 4096;  // tokens per evaluation the prompt plan accepts
struct LlamaMatch;
static bool attn_one_ok(const LlamaMatch &m, int att_S);

#define MULTI_MAX_N 31  /* tokens of the multi-token plan: passes of 8 columns below the prompt plan's threshold */
static bool cols_ok(int M_total, int nsub, int64_t nb, std::initializer_list<int64_t> Ms);

struct LlamaMatch {
    int L = 0;
    int64_t E = 0, H = 0, Hkv = 0, D = 0, F = 0, V = 0, C = 0, Egqa = 0;
    int n_past = 0, n_dims = 0;
    int N = 1;  // tokens in this evaluation: 1 = decode, 2..31 below mmq_min = a prompt chunk (multi-token plan), >= mmq_min = prompt plan
    bool prompt = false;  // the prompt plan takes it
    bool kquant = false;  // every matrix is a K-quant (any mix of Q2_K … Q6_K): the K plan (plan_launch_k), single-token decode only
    float eps = 0, freq_base = 0, freq_scale = 0, kq_scale = 0;
    ggml_type wtype = GGML_TYPE_F32;
    const ggml_tensor *wte = nullptr, *norm = nullptr, *output = nullptr, *embd = nullptr, *memory_k = nullptr,
                      *memory_v = nullptr;
    ggml_tensor *logits = nullptr, *embedding = nullptr;
    const ggml_tensor *stage_in = nullptr, *stage_out = nullptr;  // layer-split hand-off buffers (persistent f32 leaves)
    std::vector<LayerW> layers;
};

// Node bookkeeping of the matcher: node pointer -> index through a side table (open addressing, pointer hash, rebuilt per
// graph: ~1200 insertions into a 4096-entry table, about a microsecond).  Nothing is written into the caller's tensors.
struct Claims {
    ggml_cgraph *gr = nullptr;
    std::vector<char> claimed;
    int n = 0;
    std::vector<const ggml_tensor *> keys;
    std::vector<int> vals;
    size_t mask = 0;
    static size_t hash(const void *p) {
        uint64_t x = (uint64_t)(uintptr_t)p;
        x ^= x >> 17;
        x *= 0x9E3779B97F4A7C15ull;
        return (size_t)(x >> 24);
    }
    void index(ggml_cgraph *g_) {
        gr = g_;
        claimed.assign(g_->n_nodes, 0);
        size_t cap = 64;
        while (cap < 2 * (size_t)g_->n_nodes) cap <<= 1;
        keys.assign(cap, nullptr);
        vals.assign(cap, -1);
        mask = cap - 1;
        for (int i = 0; i < g_->n_nodes; i++) {
            size_t s = hash(g_->nodes[i]) & mask;
            while (keys[s] && keys[s] != g_->nodes[i]) s = (s + 1) & mask;
            keys[s] = g_->nodes[i];
            vals[s] = i;
        }
    }
    int find(const ggml_tensor *t) const {
        for (size_t s = hash(t) & mask; keys[s]; s = (s + 1) & mask)
            if (keys[s] == t) return vals[s];
        return -1;  // a leaf
    }
    bool take(const ggml_tensor *t) {
        const int i = find(t);
        if (i < 0) return true;  // a leaf
        if (!claimed[i]) {
            claimed[i] = 1;
            n++;
        }
        return true;
    }
};

static inline bool is_op(const ggml_tensor *t, ggml_op op) { return t && t->op == op; }
static inline bool is_leaf(const ggml_tensor *t) { return t && t->op == GGML_OP_NONE; }
static inline size_t view_offset(const ggml_tensor *v, const ggml_tensor *root) {
    return (size_t)((const char *)v->data - (const char *)root->data);
}
static inline bool perm_0213(const ggml_tensor *t) {
    return t->op_params[0] == 0 && t->op_params[1] == 2 && t->op_params[2] == 1 && t->op_params[3] == 3;
}

// set while try_decode_plan re-matches a K-quant batch whose f16 copies have no room: the K plan's multi-token form instead
static thread_local bool tl_k_prompt_off = false;
#define MATCH(cond)       \
    do {                  \
        if (!(cond)) return false; \
    } while (0)

// rope(reshape_3d(mul_mat(w, cur), D, heads, 1), n_past, n_dims, mode 0)
static bool match_roped_proj(const ggml_tensor *rope, Claims &c, const ggml_tensor *&w, const ggml_tensor *&cur,
                             LlamaMatch &m, int64_t heads) {
    MATCH(is_op(rope, GGML_OP_ROPE) && rope->op_params[2] == 0);
    const ggml_tensor *rs = rope->src[0];
    MATCH(is_op(rs, GGML_OP_RESHAPE) && rope->data == rs->data);
    const ggml_tensor *mm = rs->src[0];
    MATCH(is_op(mm, GGML_OP_MUL_MAT) && rs->data == mm->data);
    MATCH(rs->ne[0] == m.D && rs->ne[1] == heads && rs->ne[2] == m.N);
    float fb, fs;
    memcpy(&fb, rope->op_params + 4, 4);
    memcpy(&fs, rope->op_params + 5, 4);
    if (m.n_dims == 0) {
        m.n_past = rope->op_params[0];
        m.n_dims = rope->op_params[1];
        m.freq_base = fb;
        m.freq_scale = fs;
    }
    MATCH(rope->op_params[0] == m.n_past && rope->op_params[1] == m.n_dims && fb == m.freq_base && fs == m.freq_scale);
    w = mm->src[0];
    cur = mm->src[1];
    c.take(rope);
    c.take(rs);
    c.take(mm);
    return true;
}

// mul(rms_norm(x), weight)
static bool match_norm(const ggml_tensor *mul, Claims &c, const ggml_tensor *&x, const ggml_tensor *&weight,
                       LlamaMatch &m) {
    MATCH(is_op(mul, GGML_OP_MUL));
    const ggml_tensor *rms = mul->src[0];
    MATCH(is_op(rms, GGML_OP_RMS_NORM));
    weight = mul->src[1];
    MATCH(is_leaf(weight) && weight->type == GGML_TYPE_F32 && ggml_nelements(weight) == m.E);
    float eps;
    memcpy(&eps, rms->op_params, 4);
    if (m.eps == 0) m.eps = eps;
    MATCH(eps == m.eps);
    x = rms->src[0];
    c.take(mul);
    c.take(rms);
    return true;
}

static bool match_llama_decode(ggml_cgraph *gr, LlamaMatch &m) {
    const int n = gr->n_nodes;
    MATCH(n >= 40);
    Claims c;
    c.index(gr);

    // tail: final norm + lm_head (whole model / last stage of a layer split), or the hand-off copy of the
    // residual into the next stage's buffer (models/llama mirror, llm_host.cpp: `stage_out`)
    ggml_tensor *last = gr->nodes[n - 1];
    const ggml_tensor *x = nullptr;
    if (is_op(last, GGML_OP_MUL_MAT)) {
        MATCH(last->type == GGML_TYPE_F32 && last->ne[1] >= 1 && last->ne[1] <= PROMPT_PLAN_MAX && last->ne[2] == 1);
        m.N = (int)last->ne[1];
        m.output = last->src[0];
        MATCH(is_leaf(m.output) && (qt_of(m.output->type) >= 0 || kt_of(m.output->type) >= 0));
        m.wtype = m.output->type;
        m.kquant = kt_of(m.output->type) >= 0;
        m.E = m.output->ne[0];
        m.V = m.output->ne[1];
        m.logits = last;
        c.take(last);
        ggml_tensor *fin = last->src[1];
        MATCH(fin->ne[0] == m.E && fin->ne[1] == m.N);
        MATCH(match_norm(fin, c, x, m.norm, m));
        m.embedding = fin;
    } else {
        MATCH(is_op(last, GGML_OP_CPY) && last->type == GGML_TYPE_F32);
        const ggml_tensor *dst = last->src[1];
        MATCH(is_op(dst, GGML_OP_VIEW) && is_leaf(dst->src[0]) && dst->src[0]->type == GGML_TYPE_F32 &&
              view_offset(dst, dst->src[0]) == 0);
        m.stage_out = dst->src[0];
        x = last->src[0];
        m.E = x->ne[0];
        MATCH(x->ne[1] >= 1 && x->ne[1] <= PROMPT_PLAN_MAX && ggml_nelements(dst) == m.E * x->ne[1]);
        m.N = (int)x->ne[1];
        c.take(last);
        c.take(dst);
    }
    // number of layers = length of the residual chain add(add(...)) below the tail
    {
        int cnt = 0;
        const ggml_tensor *y = x;
        while (is_op(y, GGML_OP_ADD) && is_op(y->src[1], GGML_OP_ADD) && cnt < 4096) {
            y = y->src[1]->src[1];
            cnt++;
        }
        MATCH(cnt >= 1);
        m.L = cnt;
    }

    m.layers.resize(m.L);
    for (int il = m.L - 1; il >= 0; il--) {
        LayerW &lw = m.layers[il];
        // out = add(mul_mat(w2, gate), inpFF)
        const ggml_tensor *out = x;
        MATCH(is_op(out, GGML_OP_ADD));
        const ggml_tensor *m2 = out->src[0], *inpFF = out->src[1];
        MATCH(is_op(m2, GGML_OP_MUL_MAT));
        lw.w2 = m2->src[0];
        if (!m.output && m.wtype == GGML_TYPE_F32) {
            MATCH(qt_of(lw.w2->type) >= 0 || kt_of(lw.w2->type) >= 0);
            m.wtype = lw.w2->type;
            m.kquant = kt_of(lw.w2->type) >= 0;
        }
        const ggml_tensor *gate = m2->src[1];
        MATCH(is_op(gate, GGML_OP_MUL));
        const ggml_tensor *silu = gate->src[0], *t3 = gate->src[1];
        MATCH(is_op(silu, GGML_OP_UNARY) && silu->op_params[0] == GGML_UNARY_OP_SILU && is_op(t3, GGML_OP_MUL_MAT));
        const ggml_tensor *t1 = silu->src[0];
        MATCH(is_op(t1, GGML_OP_MUL_MAT));
        lw.w1 = t1->src[0];
        lw.w3 = t3->src[0];
        const ggml_tensor *cur2 = t1->src[1];
        MATCH(t3->src[1] == cur2);
        if (m.F == 0) m.F = lw.w1->ne[1];
        MATCH(lw.w1->ne[0] == m.E && lw.w1->ne[1] == m.F && lw.w3->ne[0] == m.E && lw.w3->ne[1] == m.F &&
              lw.w2->ne[0] == m.F && lw.w2->ne[1] == m.E);
        c.take(out); c.take(m2); c.take(gate); c.take(silu); c.take(t3); c.take(t1);
        const ggml_tensor *nx = nullptr;
        MATCH(match_norm(cur2, c, nx, lw.ffn_norm, m) && nx == inpFF);
        // inpFF = add(mul_mat(wo, merged), inpSA)
        MATCH(is_op(inpFF, GGML_OP_ADD));
        const ggml_tensor *mo = inpFF->src[0], *inpSA = inpFF->src[1];
        MATCH(is_op(mo, GGML_OP_MUL_MAT));
        lw.wo = mo->src[0];
        MATCH(lw.wo->ne[0] == m.E && lw.wo->ne[1] == m.E);
        const ggml_tensor *merged = mo->src[1];
        MATCH(is_op(merged, GGML_OP_CPY) && merged->type == GGML_TYPE_F32 && merged->ne[0] == m.E && merged->ne[1] == m.N &&
              ggml_is_contiguous(merged) && is_leaf(merged->src[1]));
        const ggml_tensor *perm = merged->src[0];
        MATCH(is_op(perm, GGML_OP_PERMUTE) && perm_0213(perm));
        const ggml_tensor *kqv = perm->src[0];
        MATCH(is_op(kqv, GGML_OP_MUL_MAT));
        c.take(inpFF); c.take(mo); c.take(merged); c.take(perm); c.take(kqv);
        // V view and probabilities
        const ggml_tensor *vv = kqv->src[0], *probs = kqv->src[1];
        MATCH(is_op(vv, GGML_OP_VIEW) && is_leaf(vv->src[0]) && vv->type == GGML_TYPE_F16);
        if (!m.memory_v) m.memory_v = vv->src[0];
        MATCH(vv->src[0] == m.memory_v);
        MATCH(is_op(probs, GGML_OP_SOFT_MAX));
        const ggml_tensor *mask = probs->src[0];
        MATCH(is_op(mask, GGML_OP_DIAG_MASK_INF));
        const ggml_tensor *sc = mask->src[0];
        MATCH(is_op(sc, GGML_OP_SCALE));
        const ggml_tensor *kq = sc->src[0], *kqs = sc->src[1];
        MATCH(is_op(kq, GGML_OP_MUL_MAT) && is_leaf(kqs) && kqs->type == GGML_TYPE_F32 && kqs->data);
        MATCH(probs->data == kq->data && mask->data == kq->data && sc->data == kq->data);  // in-place chain
        const float kqsv = *(const float *)kqs->data;
        if (m.kq_scale == 0) m.kq_scale = kqsv;
        MATCH(kqsv == m.kq_scale);
        c.take(vv); c.take(probs); c.take(mask); c.take(sc); c.take(kq);
        // K = permute(reshape_3d(view_1d(memory_k)))  Q = permute(rope(reshape(mul_mat(wq, cur))))
        const ggml_tensor *kp = kq->src[0], *qp = kq->src[1];
        MATCH(is_op(kp, GGML_OP_PERMUTE) && perm_0213(kp) && is_op(qp, GGML_OP_PERMUTE) && perm_0213(qp));
        const ggml_tensor *kr = kp->src[0];
        MATCH(is_op(kr, GGML_OP_RESHAPE));
        const ggml_tensor *kv1 = kr->src[0];
        MATCH(is_op(kv1, GGML_OP_VIEW) && is_leaf(kv1->src[0]) && kv1->type == GGML_TYPE_F16);
        if (!m.memory_k) m.memory_k = kv1->src[0];
        MATCH(kv1->src[0] == m.memory_k);
        if (m.D == 0) {
            m.D = kr->ne[0];
            m.Hkv = kr->ne[1];
            MATCH(m.D > 0 && m.E % m.D == 0);
            m.H = m.E / m.D;
            MATCH(m.Hkv > 0 && m.H % m.Hkv == 0);
            m.Egqa = m.D * m.Hkv;
        }
        c.take(kp); c.take(qp); c.take(kr); c.take(kv1);
        const ggml_tensor *cur = nullptr;
        MATCH(match_roped_proj(qp->src[0], c, lw.wq, cur, m, m.H));
        lw.cur = cur;
        MATCH(mask->op_params[0] == m.n_past);
        MATCH(lw.wq->ne[0] == m.E && lw.wq->ne[1] == m.E);
        const int P = m.n_past, T = P + m.N;
        // geometry of the cache views (llama lib.rs:248-262, 284-294)
        MATCH(kr->ne[0] == m.D && kr->ne[1] == m.Hkv && kr->ne[2] == T && kv1->ne[0] == (int64_t)T * m.Egqa);
        MATCH(vv->ne[0] == T && vv->ne[1] == m.D && vv->ne[2] == m.Hkv && vv->nb[0] == 2);
        if (m.C == 0) m.C = (int64_t)vv->nb[1] / 2;
        MATCH((int64_t)vv->nb[1] == m.C * 2 && (int64_t)vv->nb[2] == m.C * 2 * m.D && T <= m.C);
        MATCH(view_offset(kv1, m.memory_k) == (size_t)il * m.C * m.Egqa * 2);
        MATCH(view_offset(vv, m.memory_v) == (size_t)il * m.C * m.Egqa * 2);
        const ggml_tensor *nx1 = nullptr;
        MATCH(match_norm(cur, c, nx1, lw.attn_norm, m) && nx1 == inpSA);
        x = inpSA;
    }
    // the residual stream starts at get_rows(wte, embd) — or, for a later stage of a layer split, at the residual
    // received into the stage's hand-off buffer: reshape_2d(view_1d(stage_in))
    if (is_op(x, GGML_OP_GET_ROWS)) {
        m.wte = x->src[0];
        m.embd = x->src[1];
        MATCH(is_leaf(m.wte) && (m.kquant ? kt_of(m.wte->type) >= 0 : m.wte->type == m.wtype) && m.wte->ne[0] == m.E && is_leaf(m.embd) &&
              m.embd->type == GGML_TYPE_I32 && m.embd->ne[0] == m.N && m.embd->data);
        c.take(x);
    } else {
        MATCH(is_op(x, GGML_OP_RESHAPE) && x->type == GGML_TYPE_F32 && x->ne[0] == m.E && x->ne[1] == m.N);
        const ggml_tensor *v = x->src[0];
        MATCH(is_op(v, GGML_OP_VIEW) && is_leaf(v->src[0]) && v->src[0]->type == GGML_TYPE_F32 &&
              view_offset(v, v->src[0]) == 0 && v->ne[0] == m.E * m.N);
        m.stage_in = v->src[0];
        c.take(x);
        c.take(v);
    }
    // KV stores: the graph roots cpy(rope(..wk..), view_1d(memory_k)) and cpy(transpose(reshape(..wv..)), view_2d(memory_v))
    for (int i = 0; i < n; i++) {
        const ggml_tensor *t = gr->nodes[i];
        if (c.claimed[i] || t->op != GGML_OP_CPY) continue;
        const ggml_tensor *dst = t->src[1], *src = t->src[0];
        MATCH(is_op(dst, GGML_OP_VIEW) && dst->type == GGML_TYPE_F16);
        if (dst->src[0] == m.memory_k) {
            const ggml_tensor *w = nullptr, *cur = nullptr;
            MATCH(match_roped_proj(src, c, w, cur, m, m.Hkv));
            int il = -1;
            for (int j = 0; j < m.L; j++)
                if (m.layers[j].cur == cur) il = j;
            MATCH(il >= 0 && !m.layers[il].k_store && w->ne[0] == m.E && w->ne[1] == m.Egqa);
            MATCH(dst->ne[0] == m.N * m.Egqa && ggml_nelements(dst) == m.N * m.Egqa);
            MATCH(view_offset(dst, m.memory_k) == ((size_t)il * m.C + m.n_past) * m.Egqa * 2);
            m.layers[il].wk = w;
            m.layers[il].k_store = true;
        } else if (dst->src[0] == m.memory_v) {
            MATCH(is_op(src, GGML_OP_TRANSPOSE));
            const ggml_tensor *rs = src->src[0];
            MATCH(is_op(rs, GGML_OP_RESHAPE));
            const ggml_tensor *mm = rs->src[0];
            MATCH(is_op(mm, GGML_OP_MUL_MAT));
            int il = -1;
            for (int j = 0; j < m.L; j++)
                if (m.layers[j].cur == mm->src[1]) il = j;
            MATCH(il >= 0 && !m.layers[il].v_store && mm->src[0]->ne[0] == m.E && mm->src[0]->ne[1] == m.Egqa);
            MATCH(dst->ne[0] == m.N && dst->ne[1] == m.Egqa && (int64_t)dst->nb[1] == m.C * 2);
            MATCH(view_offset(dst, m.memory_v) == (size_t)il * m.C * m.Egqa * 2 + (size_t)m.n_past * 2);
            m.layers[il].wv = mm->src[0];
            m.layers[il].v_store = true;
            c.take(src); c.take(rs); c.take(mm);
        } else {
            return false;
        }
        c.take(t);
        c.take(dst);
    }
    for (auto &lw : m.layers) MATCH(lw.k_store && lw.v_store);
    MATCH(c.n == n);  // every node of the graph is accounted for (n = 37 L + 3..5 depending on head / tail)
    // the fused kernels' own preconditions
    MATCH(m.D <= 128 && m.D % 32 == 0 && m.E % 32 == 0 && m.F % 32 == 0 && m.Egqa % 8 == 0 && m.C % 8 == 0);
    MATCH(m.memory_k->type == GGML_TYPE_F16 && m.memory_v->type == GGML_TYPE_F16);
    // k_attn_decode keeps the scores (f32), D outputs and the probabilities (f16) of the longest row the launch can meet in
    // LDS (a captured launch cannot grow): the context for a prompt chunk, the split threshold for single-token decode
    // (longer rows run on kernels/decode_attn_split.h), nothing for the prompt plan (it does not launch k_attn_decode).
    // What does not fit the CU's LDS runs on the generic executor.
    // (a K-quant model takes the prompt plan from 12 tokens on — option k_prompt_min: its multi-token mat-vecs are VALU-bound — chunks of 12 / 16 / 24 tokens
    // of LLaMA-7B Q4_K 1.70k / 1.83k / 1.85k tok/s on the K plan against 1.98k / 2.67k / 3.84k on the f16 copies; the block formats'
    // k_mmq_cols is ahead of the GEMM up to 31 tokens: 3.69k against 2.68k at 16)
    const bool k_early = m.kquant && g.opt_mmq_w16 && g.opt_plan_prompt && !g.opt_mmq_i8;  // (the early switch only where that plan can run)
    m.prompt = m.N > 8 && g.opt_mmq_min > 0 && m.N >= (k_early ? std::min(g.opt_mmq_min, std::max(9, g.opt_k_prompt_min)) : g.opt_mmq_min);
    if (m.kquant && tl_k_prompt_off && m.N <= MULTI_MAX_N) m.prompt = false;
    if (!m.prompt) MATCH(attn_decode_lds(attn_decode_rows(m.C, m.N, m.H), m.D) <= ATTN_DECODE_LDS_MAX);
    if (m.prompt) {  // prompt plan (plan_launch_prompt): the default f16 GEMM path only, score buffer bounded
        MATCH(g.opt_plan_prompt && !g.opt_mmq_i8);
        MATCH(m.n_past + m.N <= m.C && m.D % 8 == 0 && m.D <= 128);
        MATCH((double)m.H * m.N * (m.n_past + m.N) * 4.0 <= 8e9);  // the scores of one layer
    } else if (m.kquant) {  // the K plan's own conditions follow below
    } else if (m.N > 8) {  // multi-token plan in passes of 8 columns: k_mmq_cols only (kernels/mmq_cols.h)
        MATCH(g.opt_plan_multi && g.opt_big && m.N <= MULTI_MAX_N && m.n_past + m.N <= m.C && qt_of(m.wtype) >= 0);
        const int64_t nbE = m.E / 32, nbF = m.F / 32;
        MATCH(m.E % 32 == 0 && m.F % 32 == 0);
        MATCH(cols_ok((int)(m.E + 2 * m.Egqa), 1, nbE, {m.E, m.Egqa}) && cols_ok((int)m.E, 1, nbE, {m.E}) &&
              cols_ok((int)(2 * m.F), 2, nbE, {m.F}) && cols_ok((int)m.E, 1, nbF, {m.E}));
        if (m.output) MATCH(cols_ok((int)m.V, 1, nbE, {m.V}));
    } else if (m.N > 1) {  // multi-token plan (kernels/decode_big8.h): 8 Q8 columns of the widest row must fit LDS
        const int64_t nbp = (std::max(m.E, m.F) / 32 + 63) / 64 * 64;
        MATCH(g.opt_plan_multi && g.opt_big && 8 * nbp * 40 <= 150 * 1024 && (int64_t)m.N * std::max(m.E, m.F) / 32 <= 4 * BIG_T);
        MATCH(m.n_past + m.N <= m.C);
    }
    for (auto &lw : m.layers)
        for (const ggml_tensor *w : {lw.wq, lw.wk, lw.wv, lw.wo, lw.w1, lw.w2, lw.w3})
            MATCH(is_leaf(w) && (m.kquant ? kt_of(w->type) >= 0 : w->type == m.wtype));
    if (m.kquant && m.prompt) {  // prompt plan on the resident f16 copies of the K weights (mul_mat_k_gemm's operands: k_prompt_weights below)
        MATCH(g.opt_plan_k && g.opt_mmq_w16 && m.E % 256 == 0 && m.F % 256 == 0);
    } else if (m.kquant) {  // K plan: decode and chunks of up to 31 tokens (every helper kernel has the row as a grid dimension, the mat-vecs take
                     // the columns in passes of 8 / 4 / 2 / 1; DecParams carries 32 token ids), super-blocks of 256, k_attn_decode over the whole context
        MATCH(g.opt_plan_k && m.N >= 1 && m.N <= MULTI_MAX_N && m.n_past + m.N <= m.C && m.E % 256 == 0 && m.F % 256 == 0 && m.D == m.n_dims);
        MATCH((size_t)m.E + (size_t)(m.E / 256) * 68 <= 150 * 1024 && (size_t)m.F + (size_t)(m.F / 256) * 68 <= 150 * 1024);
        MATCH(attn_decode_lds(m.C, m.D) <= ATTN_DECODE_LDS_MAX);
    }
    return true;
}
#undef MATCH

// ---------------------------------------------------------------------------------------------------
// the cached plan
// ---------------------------------------------------------------------------------------------------
struct DecodePlan {
    std::vector<uint64_t> sig;
    LlamaMatch m;  // tensors of the graph the plan was built from (weights are persistent; IO nodes by address)
    struct LW {
        QWeight wq, wk, wv, wo, w1, w2, w3;
        const float *attn_norm, *ffn_norm;
    };
    std::vector<LW> lw;
    struct KLW {  // K plan: the same seven matrices as planar K weights (each carries its own type)
        KWeight wq, wk, wv, wo, w1, w2, w3;
    };
    std::vector<KLW> klw;
    KWeight k_wte{}, k_output{};
    // K plan activations: f32 rows of wk / wv / the merged heads / w3, and ONE Q8_K row (max(E, F) wide) every mat-vec reads
    float *k_kf = nullptr, *k_vf = nullptr, *k_att = nullptr, *k_g3 = nullptr;
    int8_t *k_q8 = nullptr;
    float *k_d8 = nullptr;
    int16_t *k_bs = nullptr;
    QWeight wte, output;
    const float *norm = nullptr;
    __half *mem_k = nullptr, *mem_v = nullptr;
    // persistent activations
    char *pool = nullptr;
    DecParams *prm = nullptr;
    float *rope = nullptr;      // this token's RoPE (cos, sin) table, D/2 pairs (k_rope_table)
    unsigned *epoch = nullptr;  // k_qkv_attn (kernels/decode_fused.h): the token's granule tag, bumped by k_rope_table
    const void *hot = nullptr;  // 256 zero bytes that every dummy ring step of k_mmvq_big reads (BigArgs::hot)
    unsigned *ferr = nullptr;   // ... raised when an attention workgroup gave up waiting for its rows
    unsigned long long *gran = nullptr;  // ... granules: (E + 2 Egqa) / 2 per layer
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
    float *emb_out = nullptr;   // device mirror of the embedding_result node
    char *logits_out = nullptr; // device mirror of the logits node
    // the backend's own speculative next-token run (option speculate_next) writes its logits / embedding row HERE, never into the
    // mirrors above: those are caller-visible (ggml_hip_topk, ggml_hip_tensor_get, llm_session_read_node read them on the device)
    // and must keep the LAST EVALUATED token's values while the speculation is in flight or unused.  On a hit the results go to
    // the host from here and are copied into the mirrors on the stream.
    char *logits_alt = nullptr;
    float *emb_alt = nullptr;
    bool spec_out = false;  // set while the speculative graph is captured: plan_launch_* aim the final norm / lm_head at the alternates
    hipGraph_t graph_s[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};       // ... that graph, per attention variant
    hipGraphExec_t exec_s[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    int *chain_out = nullptr;   // ggml_hip_decode_greedy_chain: sampled ids (device)
    int *chain_ring = nullptr;  // ... of one K-token graph launch (option chain_k), copied into chain_out behind it
    int chain_cap = 0;
    // one captured graph per ATTENTION VARIANT of the plan (enum below); exec2: a second instance of the same graph — a chain
    // alternates so that a launch never waits for its own previous run
    hipGraph_t graph_v[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    hipGraphExec_t exec_v[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}, exec2_v[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
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

// the captured graphs of a plan (they freeze which kernels run: options and the device's slot count at capture time)
void drop_plan_graphs(DecodePlan *p) {
    for (int v = 0; v < 5; v++) {
        if (p->exec_v[v]) (void)hipGraphExecDestroy(p->exec_v[v]);
        if (p->exec2_v[v]) (void)hipGraphExecDestroy(p->exec2_v[v]);
        if (p->graph_v[v]) (void)hipGraphDestroy(p->graph_v[v]);
        p->exec_v[v] = p->exec2_v[v] = nullptr;
        p->graph_v[v] = nullptr;
        if (p->exec_s[v]) (void)hipGraphExecDestroy(p->exec_s[v]);
        if (p->graph_s[v]) (void)hipGraphDestroy(p->graph_s[v]);
        p->exec_s[v] = nullptr;
        p->graph_s[v] = nullptr;
    }
    if (p->exec_chain) (void)hipGraphExecDestroy(p->exec_chain);
    if (p->graph_chain) (void)hipGraphDestroy(p->graph_chain);
    p->exec_chain = nullptr;
    p->graph_chain = nullptr;
    p->chain_k = 0;
}
void destroy_plan(DecodePlan *p) {
    drop_plan_graphs(p);
    if (p->chain_ring) (void)hipFree(p->chain_ring);
    if (p->pool) (void)hipFree(p->pool);
    delete p;
}
// A speculative next-token run is in flight or finished unused: nothing of it may be taken for a result any more (its plan's
// buffers are about to be reused, dropped, or replayed for a measurement).  The stream is drained so that it is over.
void spec_cancel() {
    if (!g.spec.pending) return;
    g.spec.pending = false;
    if (g.stream) HIP_CHECK(hipStreamSynchronize(g.stream));
}
void drop_all_plans() {
    spec_cancel();
    if (g_plans.empty()) return;
    if (g.stream) HIP_CHECK(hipStreamSynchronize(g.stream));
    for (auto *p : g_plans) destroy_plan(p);
    g_plans.clear();
    g.ferr_plan = nullptr;
}

static KWeight plan_kw(const ggml_tensor *t) {
    DevTensor *e = extra_of(t);
    if (!e) e = find_tensor((uintptr_t)t->data);
    if (!e || !e->ksoa || (uintptr_t)t->data != e->host) die("decode plan: K-quant weight '%s' has no resident planar copy", t->name);
    return e->kw;
}
static QWeight plan_qw(const ggml_tensor *t) {
    DevTensor *e = extra_of(t);
    if (!e) e = find_tensor((uintptr_t)t->data);
    if (!e || !e->soa || (uintptr_t)t->data != e->host) die("decode plan: weight '%s' has no resident SoA copy", t->name);
    return e->qw;
}
static uint64_t rec_id(const ggml_tensor *t) {
    DevTensor *e = extra_of(t);
    if (!e) e = find_tensor((uintptr_t)t->data);
    return e ? (uint64_t)(uintptr_t)e->dev : 0;
}

static bool plan_weights_resident(const LlamaMatch &m) {
    auto ok_q = [](const ggml_tensor *t) {
        DevTensor *e = extra_of(t);
        if (!e) e = find_tensor((uintptr_t)t->data);
        return e && (e->soa || e->ksoa) && (uintptr_t)t->data == e->host;
    };
    auto ok_raw = [](const ggml_tensor *t) {
        DevTensor *e = extra_of(t);
        if (!e) e = find_tensor((uintptr_t)t->data);
        return e && !e->soa;
    };
    if (!ok_raw(m.memory_k) || !ok_raw(m.memory_v)) return false;
    if (m.wte && !ok_q(m.wte)) return false;
    if (m.output && (!ok_q(m.output) || !ok_raw(m.norm))) return false;
    if (m.stage_in && !ok_raw(m.stage_in)) return false;
    if (m.stage_out && !ok_raw(m.stage_out)) return false;
    for (auto &l : m.layers) {
        for (const ggml_tensor *w : {l.wq, l.wk, l.wv, l.wo, l.w1, l.w2, l.w3})
            if (!ok_q(w)) return false;
        if (!ok_raw(l.attn_norm) || !ok_raw(l.ffn_norm)) return false;
    }
    return true;
}

static std::vector<uint64_t> plan_signature(const LlamaMatch &m) {
    std::vector<uint64_t> s;
    auto f2u = [](float f) { uint32_t u; memcpy(&u, &f, 4); return (uint64_t)u; };
    s.push_back((uint64_t)m.N);
    for (uint64_t v : {(uint64_t)m.L, (uint64_t)m.E, (uint64_t)m.H, (uint64_t)m.Hkv, (uint64_t)m.D, (uint64_t)m.F,
                       (uint64_t)m.V, (uint64_t)m.C, (uint64_t)m.n_dims, (uint64_t)m.wtype, f2u(m.eps),
                       f2u(m.freq_base), f2u(m.freq_scale), f2u(m.kq_scale)})
        s.push_back(v);
    for (const ggml_tensor *t : {m.wte, m.norm, m.output, m.memory_k, m.memory_v, m.stage_in, m.stage_out})
        s.push_back(t ? rec_id(t) : 0);
    for (auto &l : m.layers)
        for (const ggml_tensor *t : {l.attn_norm, l.wq, l.wk, l.wv, l.wo, l.ffn_norm, l.w1, l.w2, l.w3})
            s.push_back(rec_id(t));
    s.push_back(m.logits ? (uint64_t)(uintptr_t)dev_ptr(m.logits) : 0);
    s.push_back(m.embedding ? (uint64_t)(uintptr_t)dev_ptr(m.embedding) : 0);
    return s;
}

static DevTensor *plan_rec(const ggml_tensor *t) {
    DevTensor *e = extra_of(t);
    if (!e) e = find_tensor((uintptr_t)t->data);
    return e;
}
// Prompt plan of a K-quant model: its GEMMs have no operand but the resident f16 copy of each weight (mul_mat_k_gemm,
// backend_ops.inc) — every matrix must have one before anything is launched; they are made here, all or none, by the first batch
// the prompt plan sees (mmq_min = 32 tokens and more; the executor alone waits for W16_MIN_TOKENS, but without a copy its K path
// streams every matrix through the mat-vec kernel: 1.7k tok/s at n_batch = 48).  false = no room: the node-by-node executor runs.
static bool k_prompt_weights(const LlamaMatch &m, DecodePlan *p);
// Does blockIdx mod 8 name the XCD of a one-workgroup-per-CU launch on this device?  (The dispatcher deals workgroups round robin over
// the XCDs; HW_REG_XCC_ID says where each one landed.)  Looked at once per slot, outside any capture (build_plan).
static void xcd_labels_probe() {
    if (g.xcd_labels >= 0) return;
    g.xcd_labels = 0;
    if (g.num_cus % 8 != 0 || g.num_cus < 16) return;
    unsigned *d = nullptr;
    dev_malloc((void **)&d, (size_t)g.num_cus * 4, "XCD probe");
    std::vector<unsigned> id((size_t)g.num_cus);
    bool ok = true;
    for (int rep = 0; rep < 2 && ok; rep++) {
        hipLaunchKernelGGL(k_xcc_ids, dim3((unsigned)g.num_cus), dim3(1024), 0, g.stream, d);
        HIP_CHECK(hipMemcpyAsync(id.data(), d, id.size() * 4, hipMemcpyDeviceToHost, g.stream));
        HIP_CHECK(hipStreamSynchronize(g.stream));
        unsigned seen = 0;
        for (int b = 0; b < 8; b++) seen |= 1u << id[(size_t)b];
        ok = __builtin_popcount(seen) == 8;
        for (int b = 8; b < g.num_cus && ok; b++) ok = id[(size_t)b] == id[(size_t)(b & 7)];
    }
    HIP_CHECK(hipFree(d));
    g.xcd_labels = ok ? 1 : 0;
}
static DecodePlan *build_plan(const LlamaMatch &m, std::vector<uint64_t> sig) {
    if (m.prompt && !m.kquant) {  // prompt plan: resident f16 copies of the GEMM weights, all or none (a model either fits twice or not)
        std::vector<const ggml_tensor *> ws;
        for (auto &l : m.layers)
            for (const ggml_tensor *w : {l.wq, l.wk, l.wv, l.wo, l.w1, l.w2, l.w3}) ws.push_back(w);
        if (m.output) ws.push_back(m.output);
        size_t need = 0;
        for (auto *w : ws) {
            DevTensor *e = plan_rec(w);
            if (e && !e->w16) need += (size_t)e->qw.M * e->qw.nb * 64;
        }
        size_t free_b = 0, total_b = 0;
        const bool room = hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b >= need + w16_headroom();
        if (room)
            for (auto *w : ws) ensure_w16(plan_rec(w));
    }
    xcd_labels_probe();
    if (!g.hot_line) {  // (here, not at the first launch: launches may be inside a stream capture)
        dev_malloc(&g.hot_line, 256, "the dummy ring steps' line");
        HIP_CHECK(hipMemsetAsync(g.hot_line, 0, 256, g.stream));
    }
    DecodePlan *p = new DecodePlan();
    p->sig = std::move(sig);
    p->m = m;
    if (m.wte) (m.kquant ? (void)(p->k_wte = plan_kw(m.wte)) : (void)(p->wte = plan_qw(m.wte)));
    if (m.output) {
        if (m.kquant) p->k_output = plan_kw(m.output);
        else p->output = plan_qw(m.output);
        p->norm = (const float *)dev_ptr(m.norm);
    }
    if (m.stage_in) p->stage_in = (float *)dev_ptr(m.stage_in);
    if (m.stage_out) p->stage_out = (float *)dev_ptr(m.stage_out);
    p->mem_k = (__half *)dev_ptr(m.memory_k);
    p->mem_v = (__half *)dev_ptr(m.memory_v);
    for (auto &l : m.layers) {
        DecodePlan::LW w;
        memset(&w, 0, sizeof(w));
        if (m.kquant) {
            DecodePlan::KLW kw;
            kw.wq = plan_kw(l.wq); kw.wk = plan_kw(l.wk); kw.wv = plan_kw(l.wv); kw.wo = plan_kw(l.wo);
            kw.w1 = plan_kw(l.w1); kw.w2 = plan_kw(l.w2); kw.w3 = plan_kw(l.w3);
            p->klw.push_back(kw);
        } else {
            w.wq = plan_qw(l.wq); w.wk = plan_qw(l.wk); w.wv = plan_qw(l.wv); w.wo = plan_qw(l.wo);
            w.w1 = plan_qw(l.w1); w.w2 = plan_qw(l.w2); w.w3 = plan_qw(l.w3);
        }
        w.attn_norm = (const float *)dev_ptr(l.attn_norm);
        w.ffn_norm = (const float *)dev_ptr(l.ffn_norm);
        p->lw.push_back(w);
    }
    if (m.embedding) p->emb_out = (float *)dev_ptr(m.embedding);
    if (m.logits) p->logits_out = dev_ptr(m.logits);
    // one pool for all persistent activations
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; };
    const size_t R = (size_t)m.N;  // activation rows: 1 for decode, 2..8 for a prompt chunk, more for the prompt plan
    const int att_S = (int)std::max<int64_t>(1, std::min<int64_t>(16, g.num_cus / std::max<int64_t>(1, m.H)));
    const size_t o_asc = take((size_t)m.H * m.C * 4), o_apm = take((size_t)m.H * att_S * 4), o_apt = take((size_t)m.H * att_S * m.D * 4);
    // hand-off granules of the in-launch attention exchanges: one set per LAYER (the tag is the token's epoch alone)
    const size_t Lg = m.N == 1 ? (size_t)m.L : 1;
    const size_t o_amxg = take(Lg * m.H * att_S * 8), o_asmg = take(Lg * m.H * att_S * 16), o_aptg = take(m.N == 1 ? Lg * m.H * att_S * m.D * 8 : 0),
                 o_acnt = take((size_t)m.H * 4);
    const size_t o_hot = take(256);
    const size_t o_lalt = take(m.N == 1 && m.logits ? (size_t)m.V * 4 : 0), o_ealt = take(m.N == 1 && m.logits ? (size_t)m.E * 4 : 0);
    const size_t o_epoch = take(256), o_gran = take(m.N == 1 ? (size_t)m.L * (size_t)((m.E + 2 * m.Egqa) / 2) * 8 : 0);
    const size_t o_dead = take(m.N == 1 ? (size_t)((m.E + 2 * m.Egqa) / 2) * 8 : 0);  // never written (tag 0): option test_fused_timeout
    const size_t o_ogran = take(m.N == 1 ? (size_t)m.L * (size_t)(m.E / 32) * OGRAN * 8 : 0);  // the heads' outputs as granules (WO form)
    const size_t o_prm = take(sizeof(DecParams)), o_rope = take(std::max<size_t>(8, R) * 128 * 4), o_xa = take(R * m.E * 4), o_xb = take(R * m.E * 4),
                 o_q = take(R * m.E * 4), o_gate = take(R * m.F * 4), o_elo = take(R * m.E / 2), o_ehi = take(R * m.E / 2),
                 o_ed = take(R * m.E / 32 * 4), o_es = take(R * m.E / 32 * 4), o_flo = take(R * m.F / 2),
                 o_fhi = take(R * m.F / 2), o_fd = take(R * m.F / 32 * 4), o_fs = take(R * m.F / 32 * 4);
    const bool multi = m.N >= 2 && !m.prompt;
    const size_t passes = (R + 7) / 8;  // one [block][8] table per pass of 8 rows
    const size_t o_edT = take(multi ? passes * m.E / 32 * 32 : 0), o_esT = take(multi ? passes * m.E / 32 * 32 : 0),
                 o_fdT = take(multi ? passes * m.F / 32 * 32 : 0), o_fsT = take(multi ? passes * m.F / 32 * 32 : 0);
    const size_t kW = (size_t)std::max(m.E, m.F);
    const size_t o_kkf = take(m.kquant ? R * m.Egqa * 4 : 0), o_kvf = take(m.kquant ? R * m.Egqa * 4 : 0),
                 o_katt = take(m.kquant ? R * m.E * 4 : 0), o_kg3 = take(m.kquant ? R * m.F * 4 : 0),
                 o_kq8 = take(m.kquant ? R * kW : 0), o_kd8 = take(m.kquant ? R * kW / 256 * 4 : 0), o_kbs = take(m.kquant ? R * kW / 256 * 32 : 0);
    const bool prompt = m.prompt;  // the prompt plan's buffers live only during one evaluation: shared workspace (plan_launch_prompt)
    size_t o_tok = 0, o_rope_n = 0;
    if (prompt) {
        o_tok = take(R * 4);
        o_rope_n = take(R * 128 * 4);
    }
    dev_malloc((void **)&p->pool, off, "a decode plan's activation pool");
    HIP_CHECK(hipMemsetAsync(p->pool, 0, off, g.stream));
    p->prm = (DecParams *)(p->pool + o_prm);
    p->epoch = (unsigned *)(p->pool + o_epoch);
    p->hot = p->pool + o_hot;
    if (m.N == 1 && m.logits) { p->logits_alt = p->pool + o_lalt; p->emb_alt = (float *)(p->pool + o_ealt); }
    if (!g.ferr_pin) {
        HIP_CHECK(hipHostMalloc((void **)&g.ferr_pin, 64, hipHostMallocDefault));
        *g.ferr_pin = 0;
    }
    p->ferr = g.ferr_pin;  // device-visible address of the slot's pinned word
    if (m.N == 1) p->gran = (unsigned long long *)(p->pool + o_gran);
    if (m.N == 1) p->dead_gran = (unsigned long long *)(p->pool + o_dead);
    if (m.N == 1) p->ogran = (unsigned long long *)(p->pool + o_ogran);
    p->rope = (float *)(p->pool + (prompt ? o_rope_n : o_rope));
    if (prompt) p->p_tok = (int *)(p->pool + o_tok);
    p->att_sc = (float *)(p->pool + o_asc);
    p->att_pmax = (float *)(p->pool + o_apm);
    p->att_part = (float *)(p->pool + o_apt);
    p->att_S = att_S;
    p->att_mxg = (unsigned long long *)(p->pool + o_amxg);
    p->att_sumg = (unsigned long long *)(p->pool + o_asmg);
    if (m.N == 1) p->att_partg = (unsigned long long *)(p->pool + o_aptg);
    p->att_cnt = (unsigned *)(p->pool + o_acnt);
    p->xa = (float *)(p->pool + o_xa);
    p->xb = (float *)(p->pool + o_xb);
    p->q = (float *)(p->pool + o_q);
    p->gate = (float *)(p->pool + o_gate);
    p->e_lo = (int8_t *)(p->pool + o_elo); p->e_hi = (int8_t *)(p->pool + o_ehi);
    p->e_d = (float *)(p->pool + o_ed);    p->e_s = (int *)(p->pool + o_es);
    p->f_lo = (int8_t *)(p->pool + o_flo); p->f_hi = (int8_t *)(p->pool + o_fhi);
    p->f_d = (float *)(p->pool + o_fd);    p->f_s = (int *)(p->pool + o_fs);
    if (m.kquant) {
        p->k_kf = (float *)(p->pool + o_kkf); p->k_vf = (float *)(p->pool + o_kvf);
        p->k_att = (float *)(p->pool + o_katt); p->k_g3 = (float *)(p->pool + o_kg3);
        p->k_q8 = (int8_t *)(p->pool + o_kq8); p->k_d8 = (float *)(p->pool + o_kd8); p->k_bs = (int16_t *)(p->pool + o_kbs);
    }
    if (multi) {
        p->e_dT = (float *)(p->pool + o_edT); p->e_sT = (int *)(p->pool + o_esT);
        p->f_dT = (float *)(p->pool + o_fdT); p->f_sT = (int *)(p->pool + o_fsT);
    }
    return p;
}

template <int QT, int EPI, int XSRC>
static void launch_dec(const DecMmvqArgs &a, int nwg) {
    hipLaunchKernelGGL((k_mmvq_dec<QT, EPI, XSRC>), dim3(nwg), dim3(256), (size_t)a.nb * 40, g.stream, a);
}
template <int EPI, int XSRC>
static void launch_dec_t(int qt, const DecMmvqArgs &a, int nwg) {
    switch (qt) {
        case QT_Q4_0: launch_dec<QT_Q4_0, EPI, XSRC>(a, nwg); break;
        case QT_Q4_1: launch_dec<QT_Q4_1, EPI, XSRC>(a, nwg); break;
        case QT_Q5_0: launch_dec<QT_Q5_0, EPI, XSRC>(a, nwg); break;
        case QT_Q5_1: launch_dec<QT_Q5_1, EPI, XSRC>(a, nwg); break;
        default: launch_dec<QT_Q8_0, EPI, XSRC>(a, nwg); break;
    }
    HIP_CHECK(hipGetLastError());
}

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
template <int QT, int EPI, int XSRC>
static void launch_big(const BigArgs &a) {

    constexpr int RU = EPI == EPI_QKV ? 2 : 1;
    const int64_t Mtot = a.d.w[0].M + (EPI == EPI_QKV ? a.d.w[1].M + a.d.w[2].M : 0);
    const int64_t units = Mtot / RU;
    const int min_waves = big_min_waves(XSRC, EPI, a.d.nb);
    const int G = (int)std::min<int64_t>(g.num_cus, std::max<int64_t>(1, (units + BIG_W - 1) / BIG_W));
    const int W = big_waves(units, G, min_waves);
    if ((units + (int64_t)G * W - 1) / ((int64_t)G * W) > 64) {  // one epilogue lane per unit of a wave
        fprintf(stderr, "ggml-hip: k_mmvq_big: %lld units over %d x %d waves exceed 64 per wave\n", (long long)units, G, W);
        abort();
    }
    const size_t lds = (size_t)((a.d.nb + 63) / 64 * 64) * 40;
    // the norm is staged by all 16 waves (BigX<XSRC_NORM>): such a launch always has 1024 threads, W of its waves take units
    BigArgs b = a;
    int threads = W * 64;
    if (XSRC == XSRC_NORM) {
        threads = BigX<XSRC_NORM>::NT;
        b.wdeal = W;
    }
    if (a.probe || a.ts)  // measurement build (tests/tools/launch_probe.py, timeline.py)
        hipLaunchKernelGGL((k_mmvq_big<QT, EPI, XSRC, true>), dim3(G), dim3(threads), lds, g.stream, b);
    else
        hipLaunchKernelGGL((k_mmvq_big<QT, EPI, XSRC, false>), dim3(G), dim3(threads), lds, g.stream, b);
}
template <int EPI, int XSRC>
static void launch_big_t(int qt, const BigArgs &a) {
    switch (qt) {
        case QT_Q4_0: launch_big<QT_Q4_0, EPI, XSRC>(a); break;
        case QT_Q4_1: launch_big<QT_Q4_1, EPI, XSRC>(a); break;
        case QT_Q5_0: launch_big<QT_Q5_0, EPI, XSRC>(a); break;
        case QT_Q5_1: launch_big<QT_Q5_1, EPI, XSRC>(a); break;
        default: launch_big<QT_Q8_0, EPI, XSRC>(a); break;
    }
    HIP_CHECK(hipGetLastError());
}

// wq|wk|wv + attention in one launch (kernels/decode_fused.h): n_head attention workgroups + the mat-vec on the remaining
// G - n_head.  Taken when the mat-vec deals as evenly over G - n_head workgroups as over G (7B on 256 CUs: 6144 row pairs
// = 2 per wave of 224 x 14 as of 256 x 12) — otherwise the two-launch pair is the faster one.
// Attention variants of the single-token plan (one hipGraph each, chosen per token by the context length: attn_variant):
//   AV_SHORT  the attention of a head is ONE workgroup: inside the wq|wk|wv launch (k_qkv_attn) where the shape allows, else k_attn_decode
//   AV_SPLIT  plain wq|wk|wv launch, then the position-split attention over all CUs (k_attn_split_one / the three launches)
//   AV_FUSED2 / 3 / 4  k_qkv_attn with 2 / 3 / 4 attention workgroups per head (512 positions each: up to 1024 / 1536 / 2048)
enum { AV_SHORT = 0, AV_SPLIT = 1, AV_FUSED2 = 2, AV_FUSED3 = 3, AV_FUSED4 = 4, AV_COUNT = 5 };
static inline int av_heads_split(int av) { return av >= AV_FUSED2 ? av : 1; }
struct FusedShape {
    bool ok = false;
    int G = 0, W = 0, S = 1;
    bool wo = false;   // the WO form: wo + residual as the mat-vec workgroups' second phase (kernels/decode_fused.h wo_tail)
    bool affine = false;  // head h's rows of wq|wk|wv are dealt to the mat-vec workgroups of the XCD its attention workgroup runs on (BigArgs::aff_hpl)
};
static FusedShape fused_qkv_shape(const LlamaMatch &m, int S = 1) {
    FusedShape s;
    if (!g.opt_fuse_attn || !g.opt_big || m.kquant || m.N != 1 || m.D > 128 || m.D % 32 != 0) return s;
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
    const int G0 = (int)std::min<int64_t>(g.num_cus, std::max<int64_t>(1, (units + BIG_W - 1) / BIG_W));
    const int Gp = (int)std::min<int64_t>(g.num_cus - H, std::max<int64_t>(1, (units + BIG_W - 1) / BIG_W));
    const int W0 = big_waves(units, G0, 10), Wp = big_waves(units, Gp, 10);
    const int64_t r0 = (units + (int64_t)G0 * W0 - 1) / ((int64_t)G0 * W0), rp = (units + (int64_t)Gp * Wp - 1) / ((int64_t)Gp * Wp);
    if (rp > 64) return s;
    (void)r0;
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
template <int QT>
static void launch_qkv_attn(const BigArgs &ba, const FusedAttnArgs &fa, const FusedShape &sh, size_t lds) {
    if (lds > 64 * 1024) {  // a context whose score rows exceed the 64 KiB default: the kernel asks for its dynamic LDS once per device
        static DevOnce done;
        if (done.first()) {
            HIP_CHECK(hipFuncSetAttribute((const void *)k_qkv_attn<QT, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ATTN_DECODE_LDS_MAX));
            HIP_CHECK(hipFuncSetAttribute((const void *)k_qkv_attn<QT, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ATTN_DECODE_LDS_MAX));
        }
    }
    if (ba.probe || ba.ts)
        hipLaunchKernelGGL((k_qkv_attn<QT, true>), dim3(sh.G), dim3(1024), lds, g.stream, ba, fa);
    else
        hipLaunchKernelGGL((k_qkv_attn<QT, false>), dim3(sh.G), dim3(1024), lds, g.stream, ba, fa);
}
template <int QT>
static void launch_qkv_attn_wo(const BigArgs &ba, const FusedAttnArgs &fa, const WoTailArgs &wt, const FusedShape &sh, size_t lds) {
    const bool two = (wt.w.nb + 63) / 64 <= 2;  // blocks of a row per lane: 2 steps up to 4096-wide rows, else up to 4
    if (lds > 64 * 1024) {
        static DevOnce done;
        if (done.first()) {
            HIP_CHECK(hipFuncSetAttribute((const void *)k_qkv_attn_wo<QT, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ATTN_DECODE_LDS_MAX));
            HIP_CHECK(hipFuncSetAttribute((const void *)k_qkv_attn_wo<QT, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ATTN_DECODE_LDS_MAX));
        }
    }
    if (two)
        hipLaunchKernelGGL((k_qkv_attn_wo<QT, 2>), dim3(sh.G), dim3(1024), lds, g.stream, ba, fa, wt);
    else
        hipLaunchKernelGGL((k_qkv_attn_wo<QT, 4>), dim3(sh.G), dim3(1024), lds, g.stream, ba, fa, wt);
}
static void launch_qkv_attn_wo_t(int qt, const BigArgs &ba, const FusedAttnArgs &fa, const WoTailArgs &wt, const FusedShape &sh, size_t lds) {
    switch (qt) {
        case QT_Q4_0: launch_qkv_attn_wo<QT_Q4_0>(ba, fa, wt, sh, lds); break;
        case QT_Q4_1: launch_qkv_attn_wo<QT_Q4_1>(ba, fa, wt, sh, lds); break;
        case QT_Q5_0: launch_qkv_attn_wo<QT_Q5_0>(ba, fa, wt, sh, lds); break;
        case QT_Q5_1: launch_qkv_attn_wo<QT_Q5_1>(ba, fa, wt, sh, lds); break;
        default: launch_qkv_attn_wo<QT_Q8_0>(ba, fa, wt, sh, lds); break;
    }
    HIP_CHECK(hipGetLastError());
}
static void launch_qkv_attn_t(int qt, const BigArgs &ba, const FusedAttnArgs &fa, const FusedShape &sh, size_t lds) {
    switch (qt) {
        case QT_Q4_0: launch_qkv_attn<QT_Q4_0>(ba, fa, sh, lds); break;
        case QT_Q4_1: launch_qkv_attn<QT_Q4_1>(ba, fa, sh, lds); break;
        case QT_Q5_0: launch_qkv_attn<QT_Q5_0>(ba, fa, sh, lds); break;
        case QT_Q5_1: launch_qkv_attn<QT_Q5_1>(ba, fa, sh, lds); break;
        default: launch_qkv_attn<QT_Q8_0>(ba, fa, sh, lds); break;
    }
    HIP_CHECK(hipGetLastError());
}

// per-class launch/byte accounting of one token (filled by plan_launch_all when given)
struct PlanStats {
    double bytes[GGML_HIP_KCLASS_COUNT] = {0, 0, 0, 0};
    int64_t launches[GGML_HIP_KCLASS_COUNT] = {0, 0, 0, 0};
};

// enqueues the whole token on g.stream (eagerly, or into a stream capture).  `mask` selects kernel classes
// (bit k = GGML_HIP_KCLASS k): the roofline leg replays one class alone to time it without event overhead.
// g.opt_big : 1 (default) = k_mmvq_big, norm / re-quantization fused into its staging (3 launches per layer with the fused
//             wq|wk|wv + attention + wo launch, 5 without it);
//             0 = k_mmvq_dec behind separate k_rmsnorm_quant / k_quant_row launches (8 per layer; kept for the tests).
static void plan_launch_all(DecodePlan *p, unsigned mask = ~0u, PlanStats *st = nullptr, unsigned kind_mask = ~0u,
                            int av = AV_SHORT) {
    const bool long_ctx = av == AV_SPLIT;
    auto want = [&](int k, double bytes) {
        if (!(mask & (1u << k))) return false;
        if (st) {
            st->bytes[k] += bytes;
            st->launches[k]++;
        }
        return true;
    };
    const LlamaMatch &m = p->m;
    int ts_idx = 0;  // timeline: one timeline_wgs x 8 x int64 record per big launch, in launch order
    auto next_ts = [&]() -> long long * {
        if (!g.timeline) return nullptr;
        if ((size_t)(ts_idx + 1) * g.timeline_wgs * 8 * 8 > g.timeline_bytes) return nullptr;
        return g.timeline + (size_t)(ts_idx++) * g.timeline_wgs * 8;
    };
    const int qt = qt_of(m.wtype);
    const bool f16d = qt == QT_Q4_0 || qt == QT_Q5_0 || qt == QT_Q8_0;
    const bool big = g.opt_big != 0;            // one-wave-of-big-workgroups mat-vec (kernels/decode_big.h)
    const bool fuse_x = big;  // norm / re-quantization fused into the mat-vec's staging
    const int64_t E = m.E, F = m.F, nbE = E / 32, nbF = F / 32;
    const QAct actE{(const i32x4 *)p->e_lo, (const i32x4 *)p->e_hi, p->e_d, p->e_s};
    const QAct actF{(const i32x4 *)p->f_lo, (const i32x4 *)p->f_hi, p->f_d, p->f_s};
    const float theta_scale = powf(m.freq_base, -2.0f / m.n_dims);
    const double bb = (double)blk_bytes(qt);
    // rms_norm + weight + Q8 of the E-wide residual row (separate launch)
    auto rmsq = [&](const float *x, const float *w, float *y) {
        const double bytes = (double)E * 9.25;
        if (!want(GGML_HIP_KCLASS_OTHER, bytes)) return;
        Timed tm(GGML_HIP_KCLASS_OTHER, bytes);
        if (f16d)
            hipLaunchKernelGGL(k_rmsnorm_quant<true>, dim3(1), dim3(1024), (size_t)E * 4, g.stream, x, w, m.eps, (int)E, y,
                               p->e_lo, p->e_hi, p->e_d, p->e_s);
        else
            hipLaunchKernelGGL(k_rmsnorm_quant<false>, dim3(1), dim3(1024), (size_t)E * 4, g.stream, x, w, m.eps, (int)E, y,
                               p->e_lo, p->e_hi, p->e_d, p->e_s);
        HIP_CHECK(hipGetLastError());
    };
    // kind: 0 wq|wk|wv, 1 wo, 2 w1|w3, 3 w2, 4 lm_head (GGML_HIP_KKIND_*; the roofline leg times one kind alone)
    auto mmvq = [&](int kind, auto launch, double bytes) {
        if (!(kind_mask & (1u << kind))) return;
        if (!want(GGML_HIP_KCLASS_MMVQ, bytes)) return;
        Timed tm(GGML_HIP_KCLASS_MMVQ, bytes);
        launch();
    };
    // A stage of a layer split: its first layer reads the residual straight from the hand-off buffer (xin below) and its last layer's
    // w2 launch writes straight into the outgoing one — no copy node at either end of the stage (each was a copy-engine start + a
    // boundary on the token's path: ~5 us per stage boundary and side)
    if (!m.wte) {
    } else if (want(GGML_HIP_KCLASS_OTHER, (double)E * 4.6)) {  // token embedding: get_rows(wte, embd)
        Timed tm(GGML_HIP_KCLASS_OTHER, (double)E * 4.6);
        hipLaunchKernelGGL(k_get_rows_q, dim3((unsigned)((nbE + 255) / 256), 1), dim3(256), 0, g.stream, p->wte,
                           (const int *)&p->prm->token, p->xa, E);
        HIP_CHECK(hipGetLastError());
    }
    // wq|wk|wv + attention as one launch (kernels/decode_fused.h) below the split-attention threshold
    const FusedShape fsh = long_ctx ? FusedShape{} : fused_qkv_shape(m, av_heads_split(av));
    // this position's RoPE table, shared by all layers; it also opens the token's granule epoch, so a replay of the mat-vec
    // class alone (roofline leg) takes it along when the fused launch is part of that class — the hand-off wait is then
    // inside the measured time, not skipped on stale-but-equal tags
    const bool rope_for_fused = fsh.ok && (mask & (1u << GGML_HIP_KCLASS_MMVQ)) && (kind_mask & 1u) && !(mask & (1u << GGML_HIP_KCLASS_OTHER));
    if (big && (want(GGML_HIP_KCLASS_OTHER, (double)m.D * 4.0) || rope_for_fused)) {
        hipLaunchKernelGGL(k_rope_table, dim3(1), dim3(128), 0, g.stream, (const DecParams *)p->prm, theta_scale,
                           m.freq_scale, (int)(m.D >> 1), p->rope, p->epoch);
        HIP_CHECK(hipGetLastError());
    }
    // experiment hook (GGML_HIP_BENCH_SAME_LAYER=1, roofline replays only): every iteration uses layer 0's weights, so
    // a 50 MB matrix is re-read from the 256 MB Infinity Cache instead of HBM — measures what a MALL hit is worth
    static const bool same_layer = getenv("GGML_HIP_BENCH_SAME_LAYER") && atoi(getenv("GGML_HIP_BENCH_SAME_LAYER"));
    // the WO form needs the wo launch's kind in the replay too (a roofline replay of kind 0 alone would wait for nothing: fine —
    // and one of kind 1 alone has no wo launch to time: the kind reports 0 launches)
    const bool fuse_wo = fsh.ok && fsh.wo && p->ogran != nullptr;
    const double wo_bytes = (double)E * nbE * bb + nbE * 40.0 + E * 8.0;
    for (int il = 0; il < m.L; il++) {
        const DecodePlan::LW &w = p->lw[(same_layer && kind_mask != ~0u) ? 0 : il];
        __half *mk = p->mem_k + (size_t)il * m.C * m.Egqa, *mv = p->mem_v + (size_t)il * m.C * m.Egqa;
        // ---- attention norm + wq|wk|wv + rope + KV store ----
        float *const xin = (il == 0 && !m.wte) ? p->stage_in : p->xa;                    // the layer's input row (residual stream)
        float *const xout = (il == m.L - 1 && !m.output) ? p->stage_out : p->xa;        // ... and where its w2 + residual goes
        if (!fuse_x) rmsq(xin, w.attn_norm, nullptr);
        {
            DecMmvqArgs a;
            memset(&a, 0, sizeof(a));
            a.w[0] = w.wq; a.w[1] = w.wk; a.w[2] = w.wv;
            a.wg_begin[0] = 0;
            a.wg_begin[1] = (int)((E + 7) / 8);
            a.wg_begin[2] = a.wg_begin[1] + (int)((m.Egqa + 7) / 8);
            const int nwg = a.wg_begin[2] + (int)((m.Egqa + 7) / 8);
            a.x = actE; a.xf = xin; a.xw = w.attn_norm; a.eps = m.eps;
            a.nb = nbE; a.dst = p->q; a.prm = p->prm; a.mem_k = mk; a.mem_v = mv;
            a.Egqa = m.Egqa; a.C = m.C; a.D = (int)m.D; a.theta_scale = theta_scale; a.freq_scale = m.freq_scale;
            const double qkv_bytes = (double)(E + 2 * m.Egqa) * nbE * bb + nbE * 40.0 + (E + 2 * m.Egqa) * 4.0;
            if (fsh.ok) {  // the attention workgroups ride in the same launch; no k_attn_decode below
                const double att_bytes = (double)(m.n_past + 1) * m.Egqa * 4.0 + m.E * 9.0;
                mmvq(0, [&] {
                    unsigned long long *gr_l = p->gran + (size_t)il * (size_t)((E + 2 * m.Egqa) / 2);
                    BigArgs ba{a, nullptr, next_ts(), g.timeline_wgs, p->rope, g.opt_probe, gr_l, p->epoch, fsh.W, p->hot};
                    FusedAttnArgs fa;
                    memset(&fa, 0, sizeof(fa));
                    if (fsh.affine) {
                        ba.aff_hpl = (int)(m.H / 8);
                        ba.aff_shift = m.D == 128 ? 6 : m.D == 64 ? 5 : 4;
                        fa.local_rows = 1;
                    }
                    fa.mem_k = mk; fa.mem_v = mv; fa.prm = p->prm; fa.epoch = p->epoch; fa.gran = gr_l;
                    fa.k_pair0 = (int)(E / 2); fa.v_pair0 = (int)((E + m.Egqa) / 2);
                    fa.scale = m.kq_scale; fa.D = (int)m.D; fa.n_rep = (int)(m.H / m.Hkv); fa.n_head = (int)m.H;
                    fa.Egqa = m.Egqa; fa.C = m.C; fa.Clds = attn_decode_rows(m.C, 1, m.H);
                    fa.lo = p->e_lo; fa.hi = p->e_hi; fa.dq = p->e_d; fa.sumq = p->e_s;
                    fa.ts = next_ts(); fa.ts_heads = g.timeline_wgs; fa.err = p->ferr;
                    fa.S = fsh.S; fa.layer = il; fa.mx_g = p->att_mxg_at(il); fa.sum_g = p->att_sumg_at(il); fa.part_g = p->att_partg_at(il); fa.cnt = p->att_cnt;
                    if (g.opt_test_fused_timeout && il == 0) fa.gran = p->dead_gran;  // test hook: layer 0's attention never gets its rows
                    const size_t lds = std::max(attn_decode_lds(fa.Clds, m.D), (size_t)((nbE + 63) / 64 * 64) * 40);
                    if (fuse_wo) {  // wo + residual ride along too: no wo launch below
                        fa.ogran = p->ogran + (size_t)il * (size_t)(nbE * OGRAN);
                        WoTailArgs wt;
                        memset(&wt, 0, sizeof(wt));
                        wt.w = w.wo; wt.res = xin; wt.dst = p->xb;
                        wt.ts = next_ts(); wt.ts_wgs = g.timeline_wgs;  // (the slot the wo launch would have taken)
                        if (g.opt_warm_mb > 0 && big && (kind_mask & 5u) == 5u && g.num_cus % 8 == 0 && F >= (int64_t)g.num_cus * BIG_W) {  // (w1|w3 on num_cus workgroups: rows = x mod 8 on XCD x)  // the first rows of w1|w3 into L2 while the attention runs (NextWarm); not in a replay that has no w1|w3 launch to profit
                            NextWarm &nw = wt.warm;
                            auto add_matrix = [&](const QWeight *q, int64_t nbq, int64_t rows_q) {
                                auto add = [&](const void *b, size_t rb) {
                                    if (b && nw.n < WARM_MAX) { nw.base[nw.n] = (const uint8_t *)b; nw.row_bytes[nw.n] = (uint32_t)rb; nw.rows_of[nw.n++] = (int)rows_q; }
                                };
                                add(q->qs, (size_t)nbq * 16);  // arrays a type does not have alias the next one (qw_at): by type
                                if (qt == QT_Q8_0) add(q->qs2, (size_t)nbq * 16);
                                if (qt == QT_Q5_0 || qt == QT_Q5_1) add(q->qh, (size_t)nbq * 4);
                                add(q->d, (size_t)nbq * 2);
                                if (qt == QT_Q4_1 || qt == QT_Q5_1) add(q->m, (size_t)nbq * 2);
                            };
                            int64_t wrows = (int64_t)((double)g.opt_warm_mb * 1e6 / (2.0 * (double)nbE * bb)) & ~(int64_t)7;
                            wrows = std::min<int64_t>(wrows, F);
                            add_matrix(&w.w1, nbE, wrows);
                            add_matrix(&w.w3, nbE, wrows);
                            nw.rows = (int)wrows;
                            nw.bcast = (const uint8_t *)w.ffn_norm; nw.bcast_bytes = (int)(E * 4);
                            wt.warm_wave = 15;
                        }
                        launch_qkv_attn_wo_t(qt, ba, fa, wt, fsh, lds);
                    } else
                    launch_qkv_attn_t(qt, ba, fa, fsh, lds);
                }, qkv_bytes + att_bytes + (fuse_wo ? wo_bytes : 0.0));
            } else
            mmvq(0, [&] {
                if (big)
                    launch_big_t<EPI_QKV, XSRC_NORM>(qt, BigArgs{a, nullptr, next_ts(), g.timeline_wgs, p->rope, g.opt_probe, nullptr, nullptr, 0, p->hot});
                else
                    fuse_x ? launch_dec_t<EPI_QKV, XSRC_NORM>(qt, a, nwg) : launch_dec_t<EPI_QKV, XSRC_Q8>(qt, a, nwg);
            }, qkv_bytes);
        }
        // ---- attention over the cache; output re-quantized for wo ----
        if (!fsh.ok) {
            const double bytes = (double)(m.n_past + 1) * m.Egqa * 4.0 + m.E * 9.0;
            if (want(GGML_HIP_KCLASS_ATTN, bytes)) {
                Timed tm(GGML_HIP_KCLASS_ATTN, bytes);
                long long *ts_attn = next_ts();
                if (long_ctx) {  // three launches, every CU pulls a piece of the cache (kernels/decode_attn_split.h)
                    AttnSplitArgs sa;
                    memset(&sa, 0, sizeof(sa));
                    sa.q = p->q; sa.mem_k = mk; sa.mem_v = mv; sa.prm = p->prm; sa.scale = m.kq_scale; sa.D = (int)m.D;
                    sa.n_rep = (int)(m.H / m.Hkv); sa.n_head = (int)m.H; sa.S = p->att_S; sa.Egqa = m.Egqa; sa.C = m.C;
                    sa.sc = p->att_sc; sa.pmax = p->att_pmax; sa.part = p->att_part;
                    sa.lo = p->e_lo; sa.hi = p->e_hi; sa.dq = p->e_d; sa.sumq = p->e_s;
                    const size_t chunk_max = ((((size_t)m.C + sa.S - 1) / sa.S) + 63) & ~(size_t)63;
                    if (attn_one_ok(m, p->att_S)) {  // the three phases as ONE launch (k_attn_split_one)
                        AttnSplitOneArgs oa;
                        memset(&oa, 0, sizeof(oa));
                        oa.a = sa;
                        oa.mx_g = p->att_mxg_at(il); oa.sum_g = p->att_sumg_at(il); oa.part_g = p->att_partg_at(il); oa.cnt = p->att_cnt; oa.epoch = p->epoch; oa.layer = il;
                        oa.err = p->ferr;
                        if (f16d)
                            hipLaunchKernelGGL(k_attn_split_one<true>, dim3((unsigned)m.H, (unsigned)sa.S), dim3(1024), chunk_max * 6, g.stream, oa);
                        else
                            hipLaunchKernelGGL(k_attn_split_one<false>, dim3((unsigned)m.H, (unsigned)sa.S), dim3(1024), chunk_max * 6, g.stream, oa);
                    } else {
                    hipLaunchKernelGGL(k_attn_split_scores, dim3((unsigned)m.H, (unsigned)sa.S), dim3(1024), 0, g.stream, sa);
                    hipLaunchKernelGGL(k_attn_split_vp, dim3((unsigned)m.H, (unsigned)sa.S), dim3(1024), chunk_max * 2, g.stream, sa);
                    if (f16d)
                        hipLaunchKernelGGL(k_attn_split_out<true>, dim3((unsigned)m.H), dim3(256), 0, g.stream, sa);
                    else
                        hipLaunchKernelGGL(k_attn_split_out<false>, dim3((unsigned)m.H), dim3(256), 0, g.stream, sa);
                    }
                } else if (attn_decode_opt_in(), f16d)
                    hipLaunchKernelGGL(k_attn_decode<true>, dim3((unsigned)m.H), dim3(1024), attn_decode_lds(attn_decode_rows(m.C, 1, m.H), m.D),
                                       g.stream, p->q, mk, mv, p->prm, m.kq_scale, (int)m.D, (int)(m.H / m.Hkv), m.Egqa,
                                       m.C, (float *)nullptr, p->e_lo, p->e_hi, p->e_d, p->e_s, ts_attn, (int)m.H, attn_decode_rows(m.C, 1, m.H));
                else
                    hipLaunchKernelGGL(k_attn_decode<false>, dim3((unsigned)m.H), dim3(1024), attn_decode_lds(attn_decode_rows(m.C, 1, m.H), m.D),
                                       g.stream, p->q, mk, mv, p->prm, m.kq_scale, (int)m.D, (int)(m.H / m.Hkv), m.Egqa,
                                       m.C, (float *)nullptr, p->e_lo, p->e_hi, p->e_d, p->e_s, ts_attn, (int)m.H, attn_decode_rows(m.C, 1, m.H));
                HIP_CHECK(hipGetLastError());
            }
        }
        // ---- wo + residual ----
        if (!fuse_wo) {
            DecMmvqArgs a;
            memset(&a, 0, sizeof(a));
            a.w[0] = w.wo; a.x = actE; a.nb = nbE; a.dst = p->xb; a.res = xin;
            mmvq(1, [&] {
                if (big)
                    launch_big_t<EPI_ADD, XSRC_Q8>(qt, BigArgs{a, nullptr, next_ts(), g.timeline_wgs, nullptr, g.opt_probe, nullptr, nullptr, 0, p->hot});
                else
                    launch_dec_t<EPI_ADD, XSRC_Q8>(qt, a, (int)((E + 7) / 8));
            }, (double)E * nbE * bb + nbE * 40.0 + E * 8.0);
        }
        // ---- ffn norm + silu(w1 x) * (w3 x) ----
        if (!fuse_x) rmsq(p->xb, w.ffn_norm, nullptr);
        {
            DecMmvqArgs a;
            memset(&a, 0, sizeof(a));
            a.w[0] = w.w1; a.w[1] = w.w3; a.x = actE; a.xf = p->xb; a.xw = w.ffn_norm; a.eps = m.eps; a.nb = nbE;
            a.dst = p->gate;
            mmvq(2, [&] {
                if (big)
                    launch_big_t<EPI_GATE, XSRC_NORM>(qt, BigArgs{a, nullptr, next_ts(), g.timeline_wgs, nullptr, g.opt_probe, nullptr, nullptr, 0, p->hot});
                else
                    fuse_x ? launch_dec_t<EPI_GATE, XSRC_NORM>(qt, a, (int)((F + 7) / 8))
                           : launch_dec_t<EPI_GATE, XSRC_Q8>(qt, a, (int)((F + 7) / 8));
            },
                 2.0 * F * nbE * bb + nbE * 40.0 + F * 4.0);
        }
        // ---- re-quantize the gate, w2 + residual → next layer's input ----
        if (!fuse_x && want(GGML_HIP_KCLASS_OTHER, (double)F * 5.25)) {
            Timed tm(GGML_HIP_KCLASS_OTHER, (double)F * 5.25);
            if (f16d)
                hipLaunchKernelGGL(k_quant_row<true>, grid1(nbF * 32), dim3(256), 0, g.stream, (const float *)p->gate,
                                   (int)nbF, p->f_lo, p->f_hi, p->f_d, p->f_s);
            else
                hipLaunchKernelGGL(k_quant_row<false>, grid1(nbF * 32), dim3(256), 0, g.stream, (const float *)p->gate,
                                   (int)nbF, p->f_lo, p->f_hi, p->f_d, p->f_s);
            HIP_CHECK(hipGetLastError());
        }
        {
            DecMmvqArgs a;
            memset(&a, 0, sizeof(a));
            a.w[0] = w.w2; a.x = actF; a.xf = p->gate; a.nb = nbF; a.dst = xout; a.res = p->xb;
            mmvq(3, [&] {
                if (big)
                    launch_big_t<EPI_ADD, XSRC_F32>(qt, BigArgs{a, nullptr, next_ts(), g.timeline_wgs, nullptr, g.opt_probe, nullptr, nullptr, 0, p->hot});
                else
                    fuse_x ? launch_dec_t<EPI_ADD, XSRC_F32>(qt, a, (int)((E + 7) / 8))
                           : launch_dec_t<EPI_ADD, XSRC_Q8>(qt, a, (int)((E + 7) / 8));
            },
                 (double)E * nbF * bb + nbF * 40.0 + E * 8.0);
        }
    }
    if (!m.output) return;  // not the last stage: the last layer's w2 launch has written the residual into the outgoing hand-off buffer
    float *const emb_dst = p->spec_out && p->emb_out ? p->emb_alt : p->emb_out;  // (see DecodePlan::logits_alt)
    char *const logits_dst = p->spec_out ? p->logits_alt : p->logits_out;
    if (!big) rmsq(p->xa, p->norm, emb_dst);  // final norm: f32 copy for OutputRequest.embeddings + Q8 for lm_head
    {
        DecMmvqArgs a;
        memset(&a, 0, sizeof(a));
        a.w[0] = p->output; a.x = actE; a.nb = nbE; a.dst = (float *)logits_dst;
        a.xf = p->xa; a.xw = p->norm; a.eps = m.eps;
        mmvq(4, [&] {
            if (big)
                launch_big_t<EPI_STORE, XSRC_NORM>(qt, BigArgs{a, emb_dst, next_ts(), g.timeline_wgs, nullptr, g.opt_probe, nullptr, nullptr, 0, p->hot});
            else
                launch_dec_t<EPI_STORE, XSRC_Q8>(qt, a, (int)((m.V + 7) / 8));
        },
             (double)m.V * nbE * bb + nbE * 40.0 + m.V * 4.0);
    }
}

// ---------------------------------------------------------------------------------------------------
// The K plan: single-token decode of a LLaMA whose matrices are K-quants (any mix of Q2_K … Q6_K per tensor, as the
// *_K_S / *_K_M file types of crates/llm-base/src/loader.rs:80-93 mix them).  10-13 launches per layer (kernels/kquant_plan.h):
//   norm+Q8_K | wq|wk|wv | rope + K/V store | attention | Q8_K | wo+residual | norm+Q8_K | w1|w3 | silu·mul+Q8_K | w2+residual
// (matrices that share an activation row go out as ONE launch per run of equal types: 10 launches per layer for a uniform
// model, up to 13 for a mixed one)
// the mat-vecs are the node-by-node executor's k_mmvq_k / k_mmvq_k2 (same row sums), the attention is k_attn_decode over the
// whole context.  Same `mask` / `kind_mask` protocol as plan_launch_all for the roofline leg (kinds: 0 wq+wk+wv, 1 wo,
// 2 w1+w3, 3 w2, 4 lm_head).
// ---------------------------------------------------------------------------------------------------
// launches over up to three matrices of ONE type that share the activation rows (rows of all of them dealt together); N columns
// in chunks of 8 / 4 / 2 / 1 as the node-by-node executor takes them (mul_mat_k): dsts[i] is [N][M_i], res like dsts[0]
static void launch_mmvq_kn(int nseg, const KWeight *const *ws, float *const *dsts, const KAct &x, int N, const float *res) {
    const KWeight &w = *ws[0];
    const int64_t K = w.nsb * 256, nsb = w.nsb;
    int64_t Mt = 0;
    for (int i = 0; i < nseg; i++) Mt += ws[i]->M;
    const size_t col_lds = (size_t)K + (size_t)nsb * (4 + 64);
    for (int c0 = 0; c0 < N;) {
        int ncols = 8;
        while (ncols > 1 && (ncols > N - c0 || (size_t)ncols * col_lds > 150 * 1024)) ncols >>= 1;
        const size_t lds = (size_t)ncols * col_lds;
        const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, (150 * 1024) / std::max<size_t>(lds, 1)));
        const int nwg = (int)std::min<int64_t>((Mt + 3) / 4, (int64_t)g.num_cus * per_cu);
        MmvqKArgs a;
        memset(&a, 0, sizeof(a));
        a.w = w;
        a.x.q8 = x.q8 + (int64_t)c0 * K;
        a.x.d8 = x.d8 + (int64_t)c0 * nsb;
        a.x.bs = x.bs + (int64_t)c0 * nsb * 16;
        a.dst = dsts[0] + (int64_t)c0 * ws[0]->M;
        a.ldd = ws[0]->M;
        a.res = res ? res + (int64_t)c0 * ws[0]->M : nullptr;
        a.nseg = nseg;
        if (nseg > 1) { a.wb = *ws[1]; a.dst_b = dsts[1] + (int64_t)c0 * ws[1]->M; a.ldd_b = ws[1]->M; }
        if (nseg > 2) { a.wc = *ws[2]; a.dst_c = dsts[2] + (int64_t)c0 * ws[2]->M; a.ldd_c = ws[2]->M; }
        switch (w.kt) {
            case KT_Q4_K: launch_mmvq_k_c<KT_Q4_K>(a, ncols, nwg, lds); break;
            case KT_Q6_K: launch_mmvq_k_c<KT_Q6_K>(a, ncols, nwg, lds); break;
            case KT_Q2_K: launch_mmvq_k_c<KT_Q2_K>(a, ncols, nwg, lds); break;
            case KT_Q3_K: launch_mmvq_k_c<KT_Q3_K>(a, ncols, nwg, lds); break;
            default: launch_mmvq_k_c<KT_Q5_K>(a, ncols, nwg, lds); break;
        }
        HIP_CHECK(hipGetLastError());
        c0 += ncols;
    }
}
// the decode mat-vec of Q4_K / Q6_K matrices as one wave of 1024-thread workgroups that stage the activation themselves
// (kernels/kquant_big.h): xsrc says what the row is made from (KX_NORM: rms_norm(xf) * xw; KX_F32: xf; KX_SILU_MUL: silu(xf) * xw)
struct KBigSrc {
    int xsrc;
    const float *xf, *xw;
    float eps;
    float *y_out;
};
template <int KT>
static void launch_qkv_attn_k(const KBigArgs &ka, const FusedAttnArgs &fa, size_t lds);
template <int KT>
static void launch_kbig_x(const KBigArgs &a, int xsrc, size_t lds, int epi) {
    const dim3 grid((unsigned)g.num_cus), block(KBIG_T);
    if (epi == KE_GATE) {  // silu(w1 x) * (w3 x): always behind the ffn norm
        hipLaunchKernelGGL((k_mmvq_kbig<KT, KX_NORM, KE_GATE>), grid, block, lds, g.stream, a);
        return;
    }
    if (epi == KE_QKV) {  // RoPE + K/V store in the epilogue: always behind the attention norm
        hipLaunchKernelGGL((k_mmvq_kbig<KT, KX_NORM, KE_QKV>), grid, block, lds, g.stream, a);
        return;
    }
    switch (xsrc) {
        case KX_NORM: hipLaunchKernelGGL((k_mmvq_kbig<KT, KX_NORM>), grid, block, lds, g.stream, a); break;
        case KX_F32: hipLaunchKernelGGL((k_mmvq_kbig<KT, KX_F32>), grid, block, lds, g.stream, a); break;
        default: hipLaunchKernelGGL((k_mmvq_kbig<KT, KX_SILU_MUL>), grid, block, lds, g.stream, a); break;
    }
}
static void launch_kbig(int nseg, const KWeight *const *ws, float *const *dsts, const KBigSrc &src, const float *res, int epi = KE_ROW,
                        const KBigArgs *qkv = nullptr, const FusedAttnArgs *fused = nullptr) {
    const KWeight &w = *ws[0];
    const int64_t K = w.nsb * 256, nsb = w.nsb;
    KBigArgs ka;
    memset(&ka, 0, sizeof(ka));
    MmvqKArgs &a = ka.m;
    a.w = w;
    a.dst = dsts[0];
    a.ldd = ws[0]->M;
    a.res = res;
    a.nseg = nseg;
    if (nseg > 1) { a.wb = *ws[1]; a.dst_b = dsts[1]; a.ldd_b = ws[1]->M; }
    if (nseg > 2) { a.wc = *ws[2]; a.dst_c = dsts[2]; a.ldd_c = ws[2]->M; }
    ka.xf = src.xf; ka.xw = src.xw; ka.eps = src.eps; ka.y_out = src.y_out;
    if (qkv) {
        for (int i = 0; i < 3; i++) ka.seg_kind[i] = qkv->seg_kind[i];
        ka.rope = qkv->rope; ka.prm = qkv->prm; ka.mem_k = qkv->mem_k; ka.mem_v = qkv->mem_v; ka.Egqa = qkv->Egqa; ka.C = qkv->C; ka.D = qkv->D;
        ka.gran = qkv->gran; ka.epoch = qkv->epoch;
    }
    ka.hot = g.hot_line;
    {   // waves that take units: the count in [8, 16] that deals the launch's units most evenly (as launch_big does)
        int64_t Mt = 0;
        for (int i = 0; i < nseg; i++) Mt += ws[i]->M;
        const int64_t units = epi == KE_GATE ? ws[0]->M : epi == KE_QKV ? Mt / 2 : Mt;
        // (measured, LLaMA-7B Q4_K: dealing wq|wk|wv's 6144 row pairs over 12 waves — two each — is no faster than over all 16:
        //  the K dots are VALU-bound, every wave that sits out costs issue slots; GGML_HIP_KBIG_WAVES=0 selects the even dealing)
        static const int kw = getenv("GGML_HIP_KBIG_WAVES") ? atoi(getenv("GGML_HIP_KBIG_WAVES")) : 16;
        ka.wdeal = kw == 0 ? big_waves(units, g.num_cus, 8) : std::min(16, std::max(8, kw));
    }
    const size_t lds = (size_t)K + (size_t)((nsb + 3) & ~(int64_t)3) * 4 + (size_t)nsb * 64;
    if (fused) {  // the attention workgroups ride in this launch
        ka.wdeal = 0;
        const size_t lds2 = std::max(lds, attn_decode_lds(fused->Clds, fused->D));
        switch (w.kt) {
            case KT_Q4_K: launch_qkv_attn_k<KT_Q4_K>(ka, *fused, lds2); break;
            case KT_Q6_K: launch_qkv_attn_k<KT_Q6_K>(ka, *fused, lds2); break;
            case KT_Q2_K: launch_qkv_attn_k<KT_Q2_K>(ka, *fused, lds2); break;
            case KT_Q3_K: launch_qkv_attn_k<KT_Q3_K>(ka, *fused, lds2); break;
            default: launch_qkv_attn_k<KT_Q5_K>(ka, *fused, lds2); break;
        }
        HIP_CHECK(hipGetLastError());
        return;
    }
    switch (w.kt) {
        case KT_Q4_K: launch_kbig_x<KT_Q4_K>(ka, src.xsrc, lds, epi); break;
        case KT_Q6_K: launch_kbig_x<KT_Q6_K>(ka, src.xsrc, lds, epi); break;
        case KT_Q2_K: launch_kbig_x<KT_Q2_K>(ka, src.xsrc, lds, epi); break;
        case KT_Q3_K: launch_kbig_x<KT_Q3_K>(ka, src.xsrc, lds, epi); break;
        default: launch_kbig_x<KT_Q5_K>(ka, src.xsrc, lds, epi); break;
    }
    HIP_CHECK(hipGetLastError());
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
template <int KT>
static void launch_qkv_attn_k(const KBigArgs &ka, const FusedAttnArgs &fa, size_t lds) {
    if (lds > 64 * 1024) {
        static DevOnce done;
        if (done.first()) HIP_CHECK(hipFuncSetAttribute((const void *)k_qkv_attn_k<KT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)ATTN_DECODE_LDS_MAX));
    }
    hipLaunchKernelGGL((k_qkv_attn_k<KT>), dim3((unsigned)g.num_cus), dim3(KBIG_T), lds, g.stream, ka, fa);
}
static bool kbig_ok(const DecodePlan *p) {  // K matrices whose rows of a wave fit its 64 epilogue lanes and whose activation row fits the staging
    if (!g.opt_kbig || p->m.N != 1) return false;
    auto ok = [&](const KWeight &w) {
        return w.kt >= 0 && w.kt <= KT_Q5_K && w.nsb <= 64 && p->m.E <= 8192 &&  // all five K types; staging limits of k_mmvq_kbig (KBIG_SBW, KBIG_SQ)
               (w.M + (int64_t)g.num_cus * 16 - 1) / ((int64_t)g.num_cus * 16) <= 21;  // (three matrices per launch: 63 rows per wave)
    };
    for (auto &l : p->klw)
        for (const KWeight *w : {&l.wq, &l.wk, &l.wv, &l.wo, &l.w1, &l.w2, &l.w3})
            if (!ok(*w)) return false;
    return !p->m.output || ok(p->k_output);
}
static void plan_launch_k(DecodePlan *p, unsigned mask = ~0u, PlanStats *st = nullptr, unsigned kind_mask = ~0u, int av = AV_SHORT) {
    const bool long_ctx = av == AV_SPLIT;
    const bool kbig = kbig_ok(p);
    auto want = [&](int k, double bytes) {
        if (!(mask & (1u << k))) return false;
        if (st) {
            st->bytes[k] += bytes;
            st->launches[k]++;
        }
        return true;
    };
    const LlamaMatch &m = p->m;
    const int64_t E = m.E, F = m.F, nsbE = E / 256, nsbF = F / 256;
    const int N = m.N;  // 1 = decode; 2..8 = a prompt chunk (rows of every activation buffer, columns of every mat-vec)
    const KAct act{p->k_q8, p->k_d8, p->k_bs};
    const float theta_scale = powf(m.freq_base, -2.0f / m.n_dims);
    // matrices of one kind that share the activation row: one launch per run of equal types (a *_K_M file mixes Q4_K and Q6_K)
    // src: what the big-workgroup form stages the activation from (kbig); the helper-launch form reads the Q8_K row `act`
    auto mmvq = [&](int kind, std::initializer_list<const KWeight *> wl, std::initializer_list<float *> dl, const float *res,
                    const KBigSrc &src) {
        if (!(kind_mask & (1u << kind))) return;
        const KWeight *const *ws = wl.begin();
        float *const *ds = dl.begin();
        const int n = (int)wl.size();
        for (int i = 0; i < n;) {
            int j = i + 1;
            while (g.opt_plan_k != 2 && j < n && ws[j]->kt == ws[i]->kt) j++;  // plan_k = 2: one launch per matrix (tests)
            double bytes = (double)N * ws[i]->nsb * 292.0;
            for (int k = i; k < j; k++) bytes += (double)ws[k]->M * ws[k]->nsb * k_block_bytes(ws[k]->kt) + (double)N * ws[k]->M * (res ? 8.0 : 4.0);
            if (want(GGML_HIP_KCLASS_MMVQ, bytes)) {
                Timed tm(GGML_HIP_KCLASS_MMVQ, bytes);
                if (kbig)
                    launch_kbig(j - i, ws + i, ds + i, src, res);
                else
                    launch_mmvq_kn(j - i, ws + i, ds + i, act, N, res);
            }
            i = j;
        }
    };
    auto other = [&](double bytes, auto launch) {
        if (!want(GGML_HIP_KCLASS_OTHER, bytes)) return;
        Timed tm(GGML_HIP_KCLASS_OTHER, bytes);
        launch();
        HIP_CHECK(hipGetLastError());
    };
    auto norm_quant = [&](const float *x, const float *w, float *y) {
        if (kbig) return;  // staged by the mat-vec that follows
        other((double)N * E * 9.3, [&] {
            hipLaunchKernelGGL(k_k_norm_quant, dim3((unsigned)nsbE, (unsigned)N), dim3(256), 0, g.stream, x, w, m.eps, (int)E, y, p->k_q8, p->k_d8, p->k_bs);
        });
    };
    if (!m.wte) {
        if (want(GGML_HIP_KCLASS_OTHER, (double)N * E * 8.0))
            HIP_CHECK(hipMemcpyAsync(p->xa, p->stage_in, (size_t)N * E * 4, hipMemcpyDeviceToDevice, g.stream));
    } else {  // DecParams::tokens[0] == token: the ids of the chunk
        other((double)N * E * 4.6, [&] { dequant_k_rows(p->k_wte, (const int *)p->prm->tokens, N, p->xa, E); });
    }
    other((double)N * m.D * 4.0, [&] {  // one (cos, sin) table per token of the chunk, 128 floats apart
        hipLaunchKernelGGL(k_rope_table, dim3((unsigned)N), dim3(128), 0, g.stream, (const DecParams *)p->prm, theta_scale, m.freq_scale,
                           (int)(m.D >> 1), p->rope, p->epoch);  // block 0 also opens the token's epoch (the tag of k_attn_split_one's granules)
    });
    attn_decode_opt_in();
    bool kfused = false;
    for (int il = 0; il < m.L; il++) {
        const DecodePlan::KLW &w = p->klw[il];
        const DecodePlan::LW &nw = p->lw[il];
        __half *mk = p->mem_k + (size_t)il * m.C * m.Egqa, *mv = p->mem_v + (size_t)il * m.C * m.Egqa;
        norm_quant(p->xa, nw.attn_norm, nullptr);
        // big-workgroup form: RoPE and the K/V store ride in the epilogue of the wq / wk / wv launches (a unit = two adjacent rows of a
        // matrix, k_k_rope_store's expressions); one launch per run of equal types, as below
        const bool kqkv = kbig && g.opt_plan_k != 2 && m.D % 2 == 0 && E % 2 == 0 && m.Egqa % 2 == 0;
        // ... and, while one attention workgroup per head suffices and the three matrices are of one type, the attention itself
        // (k_qkv_attn_k): no k_attn_decode launch below
        kfused = kqkv && w.wq.kt == w.wk.kt && w.wk.kt == w.wv.kt && kfused_ok(p, av) && (mask & (1u << GGML_HIP_KCLASS_MMVQ)) && (kind_mask & 1u);
        if (kqkv) {
            const KWeight *ws3[3] = {&w.wq, &w.wk, &w.wv};
            float *ds3[3] = {p->q, p->k_kf, p->k_vf};
            for (int i = 0; i < 3;) {
                int j = i + 1;
                while (j < 3 && ws3[j]->kt == ws3[i]->kt) j++;
                double bytes = (double)ws3[i]->nsb * 292.0;
                for (int k = i; k < j; k++) bytes += (double)ws3[k]->M * ws3[k]->nsb * k_block_bytes(ws3[k]->kt) + (double)ws3[k]->M * 4.0;
                if ((kind_mask & 1u) && want(GGML_HIP_KCLASS_MMVQ, bytes)) {
                    Timed tm(GGML_HIP_KCLASS_MMVQ, bytes);
                    KBigArgs qa;
                    memset(&qa, 0, sizeof(qa));
                    for (int k = i; k < j; k++) qa.seg_kind[k - i] = k;
                    qa.rope = p->rope; qa.prm = p->prm; qa.mem_k = mk; qa.mem_v = mv; qa.Egqa = m.Egqa; qa.C = m.C; qa.D = (int)m.D;
                    if (kfused) {
                        unsigned long long *gr_l = p->gran + (size_t)il * (size_t)((E + 2 * m.Egqa) / 2);
                        qa.gran = gr_l; qa.epoch = p->epoch;
                        FusedAttnArgs fa;
                        memset(&fa, 0, sizeof(fa));
                        fa.mem_k = mk; fa.mem_v = mv; fa.prm = p->prm; fa.epoch = p->epoch; fa.gran = gr_l;
                        fa.k_pair0 = (int)(E / 2); fa.v_pair0 = (int)((E + m.Egqa) / 2);
                        fa.scale = m.kq_scale; fa.D = (int)m.D; fa.n_rep = (int)(m.H / m.Hkv); fa.n_head = (int)m.H;
                        fa.Egqa = m.Egqa; fa.C = m.C; fa.Clds = m.C;
                        fa.err = p->ferr; fa.S = 1; fa.layer = il; fa.out_f32 = p->k_att;
                        launch_kbig(j - i, ws3 + i, ds3 + i, KBigSrc{KX_NORM, p->xa, nw.attn_norm, m.eps, nullptr}, nullptr, KE_QKV, &qa, &fa);
                    } else
                    launch_kbig(j - i, ws3 + i, ds3 + i, KBigSrc{KX_NORM, p->xa, nw.attn_norm, m.eps, nullptr}, nullptr, KE_QKV, &qa);
                }
                i = j;
            }
        } else
        mmvq(0, {&w.wq, &w.wk, &w.wv}, {p->q, p->k_kf, p->k_vf}, nullptr, KBigSrc{KX_NORM, p->xa, nw.attn_norm, m.eps, nullptr});
        if (!kqkv) other((double)N * (E + 2 * m.Egqa) * 6.0, [&] {
            KRopeStoreArgs ra;
            ra.q = p->q; ra.k = p->k_kf; ra.v = p->k_vf; ra.rope = p->rope; ra.prm = p->prm; ra.mem_k = mk; ra.mem_v = mv;
            ra.E = E; ra.Egqa = m.Egqa; ra.C = m.C; ra.D = (int)m.D;
            hipLaunchKernelGGL(k_k_rope_store, dim3(grid1(E / 2 + m.Egqa / 2 + m.Egqa).x, (unsigned)N), dim3(256), 0, g.stream, ra);
        });
        if (!kfused) {
            const double bytes = (double)N * ((double)(m.n_past + N) * m.Egqa * 4.0 + m.E * 9.0);
            if (want(GGML_HIP_KCLASS_ATTN, bytes)) {
                Timed tm(GGML_HIP_KCLASS_ATTN, bytes);
                // the Q8_0 copy of the heads' outputs goes to the (unused) E-wide Q8_0 row of the plan; wo reads the f32 row
                if (long_ctx) {  // >= 512 positions: every CU pulls a piece of the cache (k_attn_split_one, kernels/decode_attn_split.h)
                    AttnSplitOneArgs oa;
                    memset(&oa, 0, sizeof(oa));
                    AttnSplitArgs &sa = oa.a;
                    sa.q = p->q; sa.mem_k = mk; sa.mem_v = mv; sa.prm = p->prm; sa.scale = m.kq_scale; sa.D = (int)m.D;
                    sa.n_rep = (int)(m.H / m.Hkv); sa.n_head = (int)m.H; sa.S = p->att_S; sa.Egqa = m.Egqa; sa.C = m.C;
                    sa.lo = p->e_lo; sa.hi = p->e_hi; sa.dq = p->e_d; sa.sumq = p->e_s;
                    oa.mx_g = p->att_mxg_at(il); oa.sum_g = p->att_sumg_at(il); oa.part_g = p->att_partg_at(il); oa.cnt = p->att_cnt; oa.epoch = p->epoch; oa.layer = il;
                    oa.err = p->ferr; oa.out_f32 = p->k_att;
                    const size_t chunk_max = ((((size_t)m.C + sa.S - 1) / sa.S) + 63) & ~(size_t)63;
                    hipLaunchKernelGGL(k_attn_split_one<true>, dim3((unsigned)m.H, (unsigned)sa.S), dim3(1024), chunk_max * 6, g.stream, oa);
                } else
                hipLaunchKernelGGL(k_attn_decode<true>, dim3((unsigned)m.H, (unsigned)N), dim3(1024), attn_decode_lds(m.C, m.D), g.stream, (const float *)p->q,
                                   (const __half *)mk, (const __half *)mv, (const DecParams *)p->prm, m.kq_scale, (int)m.D, (int)(m.H / m.Hkv),
                                   m.Egqa, m.C, p->k_att, p->e_lo, p->e_hi, p->e_d, p->e_s, (long long *)nullptr, (int)m.H, m.C);
                HIP_CHECK(hipGetLastError());
            }
        }
        if (!kbig) other((double)N * E * 5.3, [&] { hipLaunchKernelGGL(k_k_quant, dim3((unsigned)nsbE, (unsigned)N), dim3(256), 0, g.stream, (const float *)p->k_att, p->k_q8, p->k_d8, p->k_bs); });
        mmvq(1, {&w.wo}, {p->xb}, p->xa, KBigSrc{KX_F32, p->k_att, nullptr, 0.0f, nullptr});
        norm_quant(p->xb, nw.ffn_norm, nullptr);
        // w1 and w3 of one type: one launch whose epilogue is silu(w1 x) * (w3 x) (the product lands in p->gate, w2 stages it as a
        // plain f32 row); a mixed pair keeps two row launches and the SiLU·mul in w2's staging
        const bool kgate = kbig && w.w1.kt == w.w3.kt && w.w1.M == w.w3.M && g.opt_plan_k != 2;
        if (kgate) {
            const KWeight *ws2[2] = {&w.w1, &w.w3};
            float *ds2[2] = {p->gate, p->k_g3};
            const double bytes = (double)w.w1.nsb * 292.0 + 2.0 * (double)w.w1.M * w.w1.nsb * k_block_bytes(w.w1.kt) + (double)w.w1.M * 4.0;
            if ((kind_mask & (1u << 2)) && want(GGML_HIP_KCLASS_MMVQ, bytes)) {
                Timed tm(GGML_HIP_KCLASS_MMVQ, bytes);
                launch_kbig(2, ws2, ds2, KBigSrc{KX_NORM, p->xb, nw.ffn_norm, m.eps, nullptr}, nullptr, KE_GATE);
            }
        } else {
            mmvq(2, {&w.w1, &w.w3}, {p->gate, p->k_g3}, nullptr, KBigSrc{KX_NORM, p->xb, nw.ffn_norm, m.eps, nullptr});
        }
        if (!kbig) other((double)N * F * 9.3, [&] {
            hipLaunchKernelGGL(k_k_silu_mul_quant, dim3((unsigned)nsbF, (unsigned)N), dim3(256), 0, g.stream, (const float *)p->gate, (const float *)p->k_g3,
                               p->k_q8, p->k_d8, p->k_bs);
        });
        mmvq(3, {&w.w2}, {p->xa}, p->xb, kgate ? KBigSrc{KX_F32, p->gate, nullptr, 0.0f, nullptr} : KBigSrc{KX_SILU_MUL, p->gate, p->k_g3, 0.0f, nullptr});
    }
    if (!m.output) {
        if (want(GGML_HIP_KCLASS_OTHER, (double)N * E * 8.0))
            HIP_CHECK(hipMemcpyAsync(p->stage_out, p->xa, (size_t)N * E * 4, hipMemcpyDeviceToDevice, g.stream));
        return;
    }
    float *const emb_dst = p->spec_out && p->emb_out ? p->emb_alt : p->emb_out;  // (see DecodePlan::logits_alt)
    char *const logits_dst = p->spec_out ? p->logits_alt : p->logits_out;
    norm_quant(p->xa, p->norm, emb_dst);  // all N rows: f32 copy (embedding_result node) + Q8_K
    mmvq(4, {&p->k_output}, {(float *)logits_dst}, nullptr, KBigSrc{KX_NORM, p->xa, p->norm, m.eps, emb_dst});
}
// the decode launches of a plan, whichever kind it is
static void plan_launch_decode(DecodePlan *p, unsigned mask = ~0u, PlanStats *st = nullptr, unsigned kind_mask = ~0u, int av = AV_SHORT) {
    if (p->m.kquant)
        plan_launch_k(p, mask, st, kind_mask, av);
    else
        plan_launch_all(p, mask, st, kind_mask, av);
}

template <int QT, int EPI>
static void launch_big8(const Big8Args &a) {
    constexpr int RU = EPI == EPI_QKV ? 2 : 1;
    const int64_t Mtot = a.d.w[0].M + (EPI == EPI_QKV ? a.d.w[1].M + a.d.w[2].M : 0);
    const int64_t units = Mtot / RU;
    const int nwg = (int)std::min<int64_t>(g.num_cus, std::max<int64_t>(1, (units + BIG_W - 1) / BIG_W));
    // waves per workgroup as for k_mmvq_big; the staging needs ncols*nb <= 4 blocks per thread and 512 RoPE threads
    const int W = big_waves(units, nwg, std::max<int>(8, (int)((a.ncols * a.d.nb + 4 * 64 - 1) / (4 * 64))));
    const size_t lds = (size_t)8 * ((a.d.nb + 63) / 64 * 64) * 40;
    static DevOnce attr_set;
    if (attr_set.first()) {  // up to 150 KB of dynamic LDS
        HIP_CHECK(hipFuncSetAttribute((const void *)k_mmvq_big8<QT, EPI>, hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024));
    }
    hipLaunchKernelGGL((k_mmvq_big8<QT, EPI>), dim3(nwg), dim3(W * 64), lds, g.stream, a);
}
template <int EPI>
static void launch_big8_t(int qt, const Big8Args &a) {
    switch (qt) {
        case QT_Q4_0: launch_big8<QT_Q4_0, EPI>(a); break;
        case QT_Q4_1: launch_big8<QT_Q4_1, EPI>(a); break;
        case QT_Q5_0: launch_big8<QT_Q5_0, EPI>(a); break;
        case QT_Q5_1: launch_big8<QT_Q5_1, EPI>(a); break;
        default: launch_big8<QT_Q8_0, EPI>(a); break;
    }
    HIP_CHECK(hipGetLastError());
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
template <int QT, int EPI>
static void launch_cols(const ColsArgs &a0, int M_total) {
    ColsArgs a = a0;
    a.ngroups = M_total / 16 / (EPI == EPI_GATE ? 2 : 1);
    const ColsShape sh = cols_shape(a.ngroups, EPI == EPI_GATE ? 2 : 1, (int)a.d.nb);
    a.gq = a.ngroups / sh.G;
    a.gr = a.ngroups % sh.G;
    static DevOnce attr_set;
    if (attr_set.first()) {
        HIP_CHECK(hipFuncSetAttribute((const void *)k_mmq_cols<QT, EPI>, hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024));
    }
    if (a.ts) {  // measurement build (tests/tools/cols_timeline.py)
        static DevOnce attr_set_i;
        if (attr_set_i.first())
            HIP_CHECK(hipFuncSetAttribute((const void *)k_mmq_cols<QT, EPI, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024));
        hipLaunchKernelGGL((k_mmq_cols<QT, EPI, true>), dim3(sh.G), dim3(COLS_T), sh.lds, g.stream, a);
    } else
        hipLaunchKernelGGL((k_mmq_cols<QT, EPI>), dim3(sh.G), dim3(COLS_T), sh.lds, g.stream, a);
}
template <int EPI>
static void launch_cols_t(int qt, const ColsArgs &a, int M_total) {
    switch (qt) {
        case QT_Q4_0: launch_cols<QT_Q4_0, EPI>(a, M_total); break;
        case QT_Q4_1: launch_cols<QT_Q4_1, EPI>(a, M_total); break;
        case QT_Q5_0: launch_cols<QT_Q5_0, EPI>(a, M_total); break;
        case QT_Q5_1: launch_cols<QT_Q5_1, EPI>(a, M_total); break;
        default: launch_cols<QT_Q8_0, EPI>(a, M_total); break;
    }
    HIP_CHECK(hipGetLastError());
}
// whether a launch of the multi-token plan can run on k_mmq_cols (else k_mmvq_big8)
static bool cols_ok(int M_total, int nsub, int64_t nb, std::initializer_list<int64_t> Ms) {
    if (!g.opt_mmq_cols) return false;
    for (int64_t M : Ms)
        if (M % 16 != 0) return false;
    return cols_shape(M_total / 16 / nsub, nsub, (int)nb).kc > 0;
}

// The multi-token plan: a prompt chunk of 2..8 tokens (InferenceSession::feed_prompt at the default n_batch = 8) as
// 8 launches per layer — k_rmsnorm_quant (N rows), k_mmvq_big8<QKV>, k_attn_decode (grid heads x N: query n attends
// to positions <= n_past + n), k_mmvq_big8<ADD> (wo), k_rmsnorm_quant, k_mmvq_big8<GATE>, k_quant_row, k_mmvq_big8<ADD>
// (w2) — every weight matrix streamed once per chunk instead of once per token-column pass of the generic executor.
static void plan_launch_multi(DecodePlan *p) {
    const LlamaMatch &m = p->m;
    int ts_idx = 0;  // timeline: one timeline_wgs x 8 x int64 record per k_mmq_cols launch, in launch order
    auto next_ts = [&]() -> long long * {
        if (!g.timeline) return nullptr;
        if ((size_t)(ts_idx + 1) * g.timeline_wgs * 8 * 8 > g.timeline_bytes) return nullptr;
        return g.timeline + (size_t)(ts_idx++) * g.timeline_wgs * 8;
    };
    const int N = m.N, qt = qt_of(m.wtype);
    const bool f16d = qt == QT_Q4_0 || qt == QT_Q5_0 || qt == QT_Q8_0;
    const int64_t E = m.E, F = m.F, nbE = E / 32, nbF = F / 32;
    const QAct actE{(const i32x4 *)p->e_lo, (const i32x4 *)p->e_hi, p->e_d, p->e_s};
    const QAct actF{(const i32x4 *)p->f_lo, (const i32x4 *)p->f_hi, p->f_d, p->f_s};
    const float theta_scale = powf(m.freq_base, -2.0f / m.n_dims);
    // the rows the NEXT launch (k_mmq_cols over `ws`, nsub = 2: w1 and w3 as pairs of groups) will read first, for the idle workgroups of
    // the norm launch to pull into the right L2s (ColsWarm, kernels/decode.h): as many leading groups per workgroup as warm_mb buys
    auto cols_warm_of = [&](std::initializer_list<const QWeight *> ws, int nsub, int64_t nb) {
        ColsWarm cw;
        memset(&cw, 0, sizeof(cw));
        if (g.opt_warm_mb <= 0 || g.xcd_labels != 1 || N < 2 || N > 8 || N + 8 > g.num_cus) return cw;
        int64_t Mt = 0;
        for (const QWeight *q : ws) Mt += q->M;
        const int ngroups = (int)(Mt / 16 / nsub);
        const ColsShape sh = cols_shape(ngroups, nsub, (int)nb);
        if (sh.G != g.num_cus) return cw;  // (one workgroup per CU: the placement the labels were probed for)
        double row_bytes = 0;
        int64_t row0 = 0;
        for (const QWeight *q : ws) {
            auto add = [&](const void *b, size_t rb) {
                if (!b || cw.n >= CW_MAX) return;
                cw.base[cw.n] = (const uint8_t *)b; cw.row_bytes[cw.n] = (uint32_t)rb; cw.row0[cw.n] = (int)row0; cw.rows[cw.n] = (int)q->M;
                cw.n++;
                row_bytes += (double)rb;
            };
            add(q->qs, (size_t)nb * 16);
            if (qt == QT_Q8_0) add(q->qs2, (size_t)nb * 16);
            if (qt == QT_Q5_0 || qt == QT_Q5_1) add(q->qh, (size_t)nb * 4);
            add(q->d, (size_t)nb * 2);
            if (qt == QT_Q4_1 || qt == QT_Q5_1) add(q->m, (size_t)nb * 2);
            if (nsub == 1) row0 += q->M;  // wq | wk | wv are one row space; w1 and w3 share theirs
        }
        if (nsub == 1) row_bytes /= (double)ws.size();  // bytes per row of the launch's row space (gate: both matrices' rows per group)
        cw.G = sh.G; cw.gq = ngroups / sh.G; cw.gr = ngroups % sh.G;
        // budget: 14 MB per launch at most (sweep r6_colswarm2.sh: 12-16 MB = one leading group of wq|wk|wv and lm_head per workgroup
        // 3.48k -> 3.51k tok/s at n_batch 8; 20 MB = two groups + one of w1|w3 3.50k; 8 MB = nothing fits)
        const double budget_mb = std::min(14.0, (double)g.opt_warm_mb);
        cw.wg = (int)std::min<double>((double)cw.gq + 1.0, floor(budget_mb * 1e6 / ((double)sh.G * 16.0 * row_bytes)));
        if (cw.wg < 1) cw.n = 0;
        return cw;
    };
    auto rmsq = [&](const float *x, const float *w, float *y, const ColsWarm &cw) {
        Timed tm(GGML_HIP_KCLASS_OTHER, (double)N * E * 9.25);
        if (cw.n > 0) {  // N norm workgroups + one warming workgroup on every other CU
            g.stat_cols_warm_launches++;
            if (f16d)
                hipLaunchKernelGGL(k_rmsnorm_quant_warm<true>, dim3((unsigned)g.num_cus), dim3(1024), (size_t)E * 4, g.stream, x, w, m.eps, (int)E, y,
                                   p->e_lo, p->e_hi, p->e_d, p->e_s, p->e_dT, p->e_sT, N, cw);
            else
                hipLaunchKernelGGL(k_rmsnorm_quant_warm<false>, dim3((unsigned)g.num_cus), dim3(1024), (size_t)E * 4, g.stream, x, w, m.eps, (int)E, y,
                                   p->e_lo, p->e_hi, p->e_d, p->e_s, p->e_dT, p->e_sT, N, cw);
        } else if (f16d)
            hipLaunchKernelGGL(k_rmsnorm_quant<true>, dim3(N), dim3(1024), (size_t)E * 4, g.stream, x, w, m.eps, (int)E, y,
                               p->e_lo, p->e_hi, p->e_d, p->e_s, p->e_dT, p->e_sT);
        else
            hipLaunchKernelGGL(k_rmsnorm_quant<false>, dim3(N), dim3(1024), (size_t)E * 4, g.stream, x, w, m.eps, (int)E, y,
                               p->e_lo, p->e_hi, p->e_d, p->e_s, p->e_dT, p->e_sT);
        HIP_CHECK(hipGetLastError());
    };
    ColsWarm cw_none;
    memset(&cw_none, 0, sizeof(cw_none));
    auto big8 = [&](auto launch, double bytes) {
        Timed tm(GGML_HIP_KCLASS_MMVQ, bytes);
        launch();
    };
    const double bb = (double)blk_bytes(qt);
    // k_mmq_cols in passes of 8 columns (one pass for the default n_batch = 8; chunks of 9..31 tokens stream the weights once
    // per pass): pass i takes rows 8i.. of the activations, of dst / res, of the RoPE table, and table i of the scales
    auto cols_passes = [&](auto launch_one, const ColsArgs &base, const float *dT, const int *sT, int64_t nb, double bytes) {
        for (int c0 = 0; c0 < N; c0 += 8) {
            ColsArgs c = base;
            c.ncols = std::min(8, N - c0);
            c.col0 = c0;
            c.d.x.lo = base.d.x.lo + (int64_t)c0 * nb;
            c.d.x.hi = base.d.x.hi + (int64_t)c0 * nb;
            c.d.x.d = base.d.x.d + (int64_t)c0 * nb;
            c.d.x.sum = base.d.x.sum + (int64_t)c0 * nb;
            c.d.dst = base.d.dst + (int64_t)c0 * base.ldd;
            if (base.d.res) c.d.res = base.d.res + (int64_t)c0 * base.ldr;
            if (base.rope) c.rope = base.rope + (int64_t)c0 * 128;
            c.dxT = dT + (int64_t)(c0 / 8) * nb * 8;
            c.sxT = sT + (int64_t)(c0 / 8) * nb * 8;
            c.ts = next_ts();
            c.ts_wgs = g.timeline_wgs;
            c.hot = g.hot_line;
            big8([&] { launch_one(c); }, bytes);
        }
    };
    if (!m.wte) {
        HIP_CHECK(hipMemcpyAsync(p->xa, p->stage_in, (size_t)N * E * 4, hipMemcpyDeviceToDevice, g.stream));
    } else {
        Timed tm(GGML_HIP_KCLASS_OTHER, (double)N * E * 4.6);
        hipLaunchKernelGGL(k_get_rows_q, dim3((unsigned)((nbE + 255) / 256), (unsigned)N), dim3(256), 0, g.stream, p->wte,
                           (const int *)p->prm->tokens, p->xa, E);
        HIP_CHECK(hipGetLastError());
    }
    // RoPE tables of the chunk's N positions, shared by all layers
    hipLaunchKernelGGL(k_rope_table, dim3((unsigned)N), dim3(128), 0, g.stream, (const DecParams *)p->prm, theta_scale,
                       m.freq_scale, (int)(m.D >> 1), p->rope);
    HIP_CHECK(hipGetLastError());
    for (int il = 0; il < m.L; il++) {
        const DecodePlan::LW &w = p->lw[il];
        __half *mk = p->mem_k + (size_t)il * m.C * m.Egqa, *mv = p->mem_v + (size_t)il * m.C * m.Egqa;
        rmsq(p->xa, w.attn_norm, nullptr,
             cols_ok((int)(E + 2 * m.Egqa), 1, nbE, {E, m.Egqa}) && N >= 2 ? cols_warm_of({&w.wq, &w.wk, &w.wv}, 1, nbE) : cw_none);
        {
            Big8Args a;
            memset(&a, 0, sizeof(a));
            a.d.w[0] = w.wq; a.d.w[1] = w.wk; a.d.w[2] = w.wv;
            a.d.x = actE; a.d.nb = nbE; a.d.dst = p->q; a.d.prm = p->prm; a.d.mem_k = mk; a.d.mem_v = mv;
            a.d.Egqa = m.Egqa; a.d.C = m.C; a.d.D = (int)m.D; a.d.theta_scale = theta_scale; a.d.freq_scale = m.freq_scale;
            a.ncols = N; a.ldd = E; a.ldr = E; a.rope = p->rope;
            if (cols_ok((int)(E + 2 * m.Egqa), 1, nbE, {E, m.Egqa}) && N >= 2) {
                ColsArgs c;
                memset(&c, 0, sizeof(c));
                c.d = a.d; c.ldd = a.ldd; c.ldr = a.ldr; c.rope = a.rope;
                cols_passes([&](const ColsArgs &cc) { launch_cols_t<EPI_QKV>(qt, cc, (int)(E + 2 * m.Egqa)); }, c, p->e_dT, p->e_sT, nbE,
                            (double)(E + 2 * m.Egqa) * nbE * bb);
            } else
                big8([&] { launch_big8_t<EPI_QKV>(qt, a); }, (double)(E + 2 * m.Egqa) * nbE * bb);
        }
        {
            Timed tm(GGML_HIP_KCLASS_ATTN, (double)N * (m.n_past + N) * m.Egqa * 4.0);
            attn_decode_opt_in();
            if (f16d)
                hipLaunchKernelGGL(k_attn_decode<true>, dim3((unsigned)m.H, (unsigned)N), dim3(1024), (size_t)(m.C + m.D) * 4 + (size_t)m.C * 2,
                                   g.stream, p->q, mk, mv, p->prm, m.kq_scale, (int)m.D, (int)(m.H / m.Hkv), m.Egqa, m.C,
                                   (float *)nullptr, p->e_lo, p->e_hi, p->e_d, p->e_s, (long long *)nullptr, (int)m.H, m.C, p->e_dT, p->e_sT);
            else
                hipLaunchKernelGGL(k_attn_decode<false>, dim3((unsigned)m.H, (unsigned)N), dim3(1024), (size_t)(m.C + m.D) * 4 + (size_t)m.C * 2,
                                   g.stream, p->q, mk, mv, p->prm, m.kq_scale, (int)m.D, (int)(m.H / m.Hkv), m.Egqa, m.C,
                                   (float *)nullptr, p->e_lo, p->e_hi, p->e_d, p->e_s, (long long *)nullptr, (int)m.H, m.C, p->e_dT, p->e_sT);
            HIP_CHECK(hipGetLastError());
        }
        {
            Big8Args a;
            memset(&a, 0, sizeof(a));
            a.d.w[0] = w.wo; a.d.x = actE; a.d.nb = nbE; a.d.dst = p->xb; a.d.res = p->xa;
            a.ncols = N; a.ldd = E; a.ldr = E;
            if (cols_ok((int)E, 1, nbE, {E}) && N >= 2) {
                ColsArgs c;
                memset(&c, 0, sizeof(c));
                c.d = a.d; c.ldd = a.ldd; c.ldr = a.ldr;
                cols_passes([&](const ColsArgs &cc) { launch_cols_t<EPI_ADD>(qt, cc, (int)E); }, c, p->e_dT, p->e_sT, nbE, (double)E * nbE * bb);
            } else
                big8([&] { launch_big8_t<EPI_ADD>(qt, a); }, (double)E * nbE * bb);
        }
        rmsq(p->xb, w.ffn_norm, nullptr, cols_ok((int)(2 * F), 2, nbE, {F}) && N >= 2 ? cols_warm_of({&w.w1, &w.w3}, 2, nbE) : cw_none);
        {
            Big8Args a;
            memset(&a, 0, sizeof(a));
            a.d.w[0] = w.w1; a.d.w[1] = w.w3; a.d.x = actE; a.d.nb = nbE; a.d.dst = p->gate;
            a.ncols = N; a.ldd = F; a.ldr = F;
            if (cols_ok((int)(2 * F), 2, nbE, {F}) && N >= 2) {
                ColsArgs c;
                memset(&c, 0, sizeof(c));
                c.d = a.d; c.ldd = a.ldd; c.ldr = a.ldr;
                cols_passes([&](const ColsArgs &cc) { launch_cols_t<EPI_GATE>(qt, cc, (int)(2 * F)); }, c, p->e_dT, p->e_sT, nbE, 2.0 * F * nbE * bb);
            } else
                big8([&] { launch_big8_t<EPI_GATE>(qt, a); }, 2.0 * F * nbE * bb);
        }
        {
            Timed tm(GGML_HIP_KCLASS_OTHER, (double)N * F * 5.25);
            const dim3 grid((unsigned)((nbF * 32 + 255) / 256), (unsigned)N);
            if (f16d)
                hipLaunchKernelGGL(k_quant_row<true>, grid, dim3(256), 0, g.stream, (const float *)p->gate, (int)nbF, p->f_lo,
                                   p->f_hi, p->f_d, p->f_s, p->f_dT, p->f_sT);
            else
                hipLaunchKernelGGL(k_quant_row<false>, grid, dim3(256), 0, g.stream, (const float *)p->gate, (int)nbF, p->f_lo,
                                   p->f_hi, p->f_d, p->f_s, p->f_dT, p->f_sT);
            HIP_CHECK(hipGetLastError());
        }
        {
            Big8Args a;
            memset(&a, 0, sizeof(a));
            a.d.w[0] = w.w2; a.d.x = actF; a.d.nb = nbF; a.d.dst = p->xa; a.d.res = p->xb;
            a.ncols = N; a.ldd = E; a.ldr = E;
            if (cols_ok((int)E, 1, nbF, {E}) && N >= 2) {
                ColsArgs c;
                memset(&c, 0, sizeof(c));
                c.d = a.d; c.ldd = a.ldd; c.ldr = a.ldr;
                cols_passes([&](const ColsArgs &cc) { launch_cols_t<EPI_ADD>(qt, cc, (int)E); }, c, p->f_dT, p->f_sT, nbF, (double)E * nbF * bb);
            } else
                big8([&] { launch_big8_t<EPI_ADD>(qt, a); }, (double)E * nbF * bb);
        }
    }
    if (!m.output) {
        HIP_CHECK(hipMemcpyAsync(p->stage_out, p->xa, (size_t)N * E * 4, hipMemcpyDeviceToDevice, g.stream));
        return;
    }
    rmsq(p->xa, p->norm, p->emb_out,  // final norm of all N rows: f32 copy (embedding_result node) + Q8
         cols_ok((int)m.V, 1, nbE, {m.V}) && N >= 2 ? cols_warm_of({&p->output}, 1, nbE) : cw_none);
    {
        Big8Args a;
        memset(&a, 0, sizeof(a));
        a.d.w[0] = p->output; a.d.x = actE; a.d.nb = nbE; a.d.dst = (float *)p->logits_out;
        a.ncols = N; a.ldd = m.V; a.ldr = m.V;
        if (cols_ok((int)m.V, 1, nbE, {m.V}) && N >= 2) {
            ColsArgs c;
            memset(&c, 0, sizeof(c));
            c.d = a.d; c.ldd = a.ldd; c.ldr = a.ldr;
            cols_passes([&](const ColsArgs &cc) { launch_cols_t<EPI_STORE>(qt, cc, (int)m.V); }, c, p->e_dT, p->e_sT, nbE, (double)m.V * nbE * bb);
        } else
            big8([&] { launch_big8_t<EPI_STORE>(qt, a); }, (double)m.V * nbE * bb);
    }
}

// ---------------------------------------------------------------------------------------------------
// The prompt plan: a batch of N >= mmq_min tokens (crates/llm-base/src/inference_session.rs:315-316 feeds n_batch tokens
// per evaluate) through the same graph.  The quantized mat-muls run on the matrix cores (mmq_f16_launch, as in the
// node-by-node executor), K.Q and V.P on k_gemm_f16 — V.P writes the merged-heads layout directly — and everything
// between two GEMMs is one launch (kernels/prompt.h): 13 launches per layer instead of 24, the same bits.
// Launched eagerly (a few hundred launches of tens of microseconds each: no hipGraph needed).
// ---------------------------------------------------------------------------------------------------
// Attention of a prompt batch (lib.rs:246-307): q [N][E] f32 (RoPE applied), mk / mv this layer's cache, out [N][E] f32 in
// the merged-heads layout.  fused: one launch with the scores in LDS (kernels/prompt_attn.h); else K.Q -> k_p_soft_max ->
// V.P with the scores (sc: [H][N][T] f32) and probabilities (p16: [H][N][Tp] f16, Tp = T rounded up to 8) in HBM.
static inline int prompt_attn_row_bytes(int64_t T) { return (int)(((T + 63) & ~(int64_t)63) * 4 + 16); }
// queries per workgroup the fused kernel takes rows of T keys with: 32, 16 (long rows), or 0 = the scores do not fit LDS
static inline int prompt_attn_queries(int64_t D, int64_t T) {
    if (!(D == 128 || D == 64 || D == 32)) return 0;
    if ((size_t)PATTN_Q * prompt_attn_row_bytes(T) <= 150 * 1024) return PATTN_Q;  // (row_bytes >= 272 >= the staged Q row)
    if ((size_t)16 * prompt_attn_row_bytes(T) <= 150 * 1024) return 16;
    return 0;
}
static inline bool prompt_attn_fits(int64_t D, int64_t T) { return prompt_attn_queries(D, T) != 0; }
static void prompt_attention(bool fused, const float *q, const __half *mk, const __half *mv, float *out, float *sc, _Float16 *p16,
                             int N, int64_t E, int64_t Egqa, int64_t H, int64_t Hkv, int64_t D, int n_past, int64_t C, float scale,
                             _Float16 *x16_out = nullptr /* fused only: write wo's re-quantized f16 operand instead of `out` */,
                             bool f16d = false, const float *rope = nullptr /* fused only: q is un-rotated (+ q_part) */, int64_t q_part = 0) {
    const int64_t T = (int64_t)n_past + N, Tp = (T + 7) & ~(int64_t)7;
    if (fused) {
        PAttnArgs pa;
        pa.q = q; pa.mem_k = mk; pa.mem_v = mv; pa.out = out;
        pa.N = N; pa.E = (int)E; pa.Egqa = (int)Egqa; pa.H = (int)H; pa.r = (int)(H / Hkv); pa.n_past = n_past;
        pa.C = C; pa.scale = scale; pa.row_bytes = prompt_attn_row_bytes(T);
        pa.x16 = x16_out; pa.f16d = f16d ? 1 : 0;
        pa.rope = rope; pa.q_part = q_part;
        static DevOnce pattn_attr;
        if (pattn_attr.first()) {
            HIP_CHECK(hipFuncSetAttribute((const void *)k_p_attn<128>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
            HIP_CHECK(hipFuncSetAttribute((const void *)k_p_attn<64>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
            HIP_CHECK(hipFuncSetAttribute((const void *)k_p_attn<32>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
        }
        const int QR = prompt_attn_queries(D, T);
        const dim3 grid((unsigned)(((N + QR - 1) / QR) * H));
        const size_t lds = (size_t)QR * std::max<size_t>(pa.row_bytes, 2 * D + 16);  // score rows (the staged Q tile borrows them)
        {   // two workgroups per CU (LDS permitting) and more workgroups than CUs: the first num_cus workgroups take the longest tiles,
            // the rest come shortest first so that a CU's two workgroups add up to the same work everywhere (kernels/prompt_attn.h);
            // worth 0.4 % of a 512-token batch (r06_sweeps.txt 15: a tile's duration is its own dependent chain, not its neighbour's)
            const int ntile = (N + QR - 1) / QR;
            const bool two_per_cu = 2 * (lds + 1024) <= 160 * 1024 && (int64_t)ntile * H > g.num_cus;
            pa.r1 = two_per_cu ? std::max(1, std::min(ntile, (int)(g.num_cus / H))) : ntile;
        }
        Timed tm(GGML_HIP_KCLASS_ATTN, (double)T * Egqa * 4.0 + (double)N * E * 8.0);
        pa.ts = nullptr;
        static DevOnce pattn_attr16;
        if (QR == 16 && pattn_attr16.first()) {
            HIP_CHECK(hipFuncSetAttribute((const void *)k_p_attn<128, false, 16>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
            HIP_CHECK(hipFuncSetAttribute((const void *)k_p_attn<64, false, 16>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
            HIP_CHECK(hipFuncSetAttribute((const void *)k_p_attn<32, false, 16>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
        }
        if (QR == 16) {
            if (D == 128) hipLaunchKernelGGL((k_p_attn<128, false, 16>), grid, dim3(256), lds, g.stream, pa);
            else if (D == 64) hipLaunchKernelGGL((k_p_attn<64, false, 16>), grid, dim3(256), lds, g.stream, pa);
            else hipLaunchKernelGGL((k_p_attn<32, false, 16>), grid, dim3(256), lds, g.stream, pa);
        } else if (g.timeline && D == 128 && (size_t)grid.x * 64 <= g.timeline_bytes) {  // measurement build (tests/tools/pattn_timeline.py)
            static DevOnce pattn_attr_i;
            if (pattn_attr_i.first())
                HIP_CHECK(hipFuncSetAttribute((const void *)k_p_attn<128, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
            pa.ts = g.timeline;
            hipLaunchKernelGGL((k_p_attn<128, true>), grid, dim3(256), lds, g.stream, pa);
        } else if (D == 128) hipLaunchKernelGGL(k_p_attn<128>, grid, dim3(256), lds, g.stream, pa);
        else if (D == 64) hipLaunchKernelGGL(k_p_attn<64>, grid, dim3(256), lds, g.stream, pa);
        else hipLaunchKernelGGL(k_p_attn<32>, grid, dim3(256), lds, g.stream, pa);
        HIP_CHECK(hipGetLastError());
        return;
    }
    {  // scores = K . Q  (lib.rs:248-266): [T, N, H]
        GemmF16Args ga;
        ga.a = (const char *)mk; ga.a_nb1 = Egqa * 2; ga.a_nb2 = D * 2; ga.a_nb3 = 0;
        ga.b = (const char *)q; ga.b_nb1 = E * 4; ga.b_nb2 = D * 4; ga.b_nb3 = 0;
        ga.d = (char *)sc; ga.d_nb1 = T * 4; ga.d_nb2 = (int64_t)N * T * 4; ga.d_nb3 = 0;
        ga.M = T; ga.N = N; ga.K = D; ga.ne12 = H; ga.r2 = H / Hkv; ga.r3 = 1;
        ga.causal = 1; ga.causal_past = n_past;
        ga.tiles_n = (N + 127) / 128;
        const int tiles_m = (int)((T + 127) / 128);
        Timed tm(GGML_HIP_KCLASS_ATTN, (double)T * Egqa * 2.0 + (double)N * E * 4.0 + (double)H * N * T * 4.0);
        hipLaunchKernelGGL(k_gemm_f16, dim3((unsigned)(tiles_m * ga.tiles_n), (unsigned)H), dim3(256), MMQ_LDS, g.stream, ga);
        HIP_CHECK(hipGetLastError());
    }
    {
        const int64_t rows = (int64_t)H * N;
        Timed tm(GGML_HIP_KCLASS_OTHER, (double)rows * T * 8.0);
        hipLaunchKernelGGL(k_p_soft_max, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, g.stream, sc, rows, (int)T, N, scale, n_past, p16, Tp);
        HIP_CHECK(hipGetLastError());
    }
    {  // V . P (lib.rs:284-300), written in the merged-heads layout [E, N] (the permute + cpy of lib.rs:302-307)
        GemmF16Args ga;
        ga.a = (const char *)mv; ga.a_nb1 = C * 2; ga.a_nb2 = C * D * 2; ga.a_nb3 = 0;
        ga.b = (const char *)p16; ga.b_nb1 = Tp * 2; ga.b_nb2 = (int64_t)N * Tp * 2; ga.b_nb3 = 0;  // f16 rows
        ga.d = (char *)out; ga.d_nb1 = E * 4; ga.d_nb2 = D * 4; ga.d_nb3 = 0;
        ga.M = D; ga.N = N; ga.K = T; ga.ne12 = H; ga.r2 = H / Hkv; ga.r3 = 1;
        ga.causal = 2; ga.causal_past = n_past;
        ga.tiles_n = (N + 127) / 128;
        const int tiles_m = (int)((D + 127) / 128);
        Timed tm(GGML_HIP_KCLASS_ATTN, (double)T * Egqa * 2.0 + (double)H * N * T * 2.0 + (double)N * E * 4.0);
        hipLaunchKernelGGL(k_gemm_f16_b16, dim3((unsigned)(tiles_m * ga.tiles_n), (unsigned)H), dim3(256), MMQ_LDS, g.stream, ga);
        HIP_CHECK(hipGetLastError());
    }
}

static bool k_prompt_weights(const LlamaMatch &m, DecodePlan *p) {
    std::vector<const ggml_tensor *> ws;
    for (auto &l : m.layers)
        for (const ggml_tensor *w : {l.wq, l.wk, l.wv, l.wo, l.w1, l.w2, l.w3}) ws.push_back(w);
    if (m.output) ws.push_back(m.output);
    size_t need = 0;
    for (auto *w : ws) {
        DevTensor *e = plan_rec(w);
        if (!e || !e->ksoa || (uintptr_t)w->data != e->host) return false;
        if (!e->w16) need += (size_t)e->kw.M * (size_t)e->kw.nsb * 512;
    }
    if (need) {  // all or none: a model either fits twice or it does not
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < need + ((size_t)1 << 30) + w16_headroom()) return false;
        for (auto *w : ws)
            if (!ensure_w16_k(plan_rec(w))) return false;
    }
    if (!p) return true;
    auto qw_of = [&](const ggml_tensor *t) {
        DevTensor *e = plan_rec(t);
        QWeight w;
        memset(&w, 0, sizeof(w));
        w.M = e->kw.M;
        w.nb = e->kw.nsb * 8;
        w.qt = QT_Q8_0;  // never read: every kernel that takes a resident copy reads only w16 (as in mul_mat_k_gemm)
        w.w16 = e->w16;
        return w;
    };
    for (int il = 0; il < m.L; il++) {
        DecodePlan::LW &w = p->lw[il];
        const auto &l = m.layers[il];
        w.wq = qw_of(l.wq); w.wk = qw_of(l.wk); w.wv = qw_of(l.wv); w.wo = qw_of(l.wo);
        w.w1 = qw_of(l.w1); w.w2 = qw_of(l.w2); w.w3 = qw_of(l.w3);
    }
    if (m.output) p->output = qw_of(m.output);
    p->w16_gen = g.w16_gen;
    return true;
}
static void plan_launch_prompt(DecodePlan *p) {
    const LlamaMatch &m = p->m;
    const bool kq = m.kquant;  // K-quant model: the GEMMs' token operand is the Q8_K round trip, the weights their f16 copies (k_prompt_weights)
    const int N = m.N, qt = kq ? QT_Q8_0 : qt_of(m.wtype);
    const bool f16d = !kq && (qt == QT_Q4_0 || qt == QT_Q5_0 || qt == QT_Q8_0);
    const int64_t E = m.E, F = m.F, nbE = E / 32, nbF = F / 32, T = (int64_t)m.n_past + N;
    const int64_t Tp = (T + 7) & ~(int64_t)7;  // row length of the f16 probabilities (16-byte aligned rows)
    const float theta_scale = powf(m.freq_base, -2.0f / m.n_dims);
    const bool fused_attn = g.opt_attn_fused && prompt_attn_fits(m.D, T);
    {   // Transient buffers from the executor's grow-only workspace (rewound at the start of every graph), shared by all
        // prompt plans: sized by this evaluation's T, not by the context (scores of a 512-token batch at 16k context
        // would otherwise pin 1.5 GB per cached plan).  GEMM outputs have room for the two partials of a K split.
        const size_t R = (size_t)N;
        p->p_te = (float *)ws_alloc(2 * R * E * 4);
        p->p_mg = (float *)ws_alloc(R * E * 4);
        p->p_qf = (float *)ws_alloc(2 * R * (E + 2 * m.Egqa) * 4);  // q | k | v
        p->p_kf = p->p_qf + R * E;
        p->p_vf = p->p_kf + R * m.Egqa;
        p->p_g1 = (float *)ws_alloc(2 * R * 2 * F * 4);  // w1 x | w3 x
        p->p_g3 = p->p_g1 + R * F;
        if (!fused_attn) {  // the three-launch attention keeps the scores of all heads in HBM
            p->p_sc = (float *)ws_alloc((size_t)m.H * R * T * 4);
            p->p_p16 = (_Float16 *)ws_alloc((size_t)m.H * R * Tp * 2);
        }
        p->p_x16 = (_Float16 *)ws_alloc(R * std::max(E, F) * 2);
    }
    // the f16 copies are a cache (dev_malloc may have released them, also just above); a K-quant model has no other operand
    if (kq && p->w16_gen != g.w16_gen && !k_prompt_weights(m, p))
        die("prompt plan: no room for the f16 copies of the K-quant weights any more (set GGML_HIP_PLAN_K=0 to run the node-by-node executor)");
    if (!kq && p->w16_gen != g.w16_gen) {
        auto w16_of = [](const ggml_tensor *t) { DevTensor *e = plan_rec(t); return e ? e->qw.w16 : nullptr; };
        for (int il = 0; il < m.L; il++) {
            DecodePlan::LW &w = p->lw[il];
            const auto &l = m.layers[il];
            w.wq.w16 = w16_of(l.wq); w.wk.w16 = w16_of(l.wk); w.wv.w16 = w16_of(l.wv); w.wo.w16 = w16_of(l.wo);
            w.w1.w16 = w16_of(l.w1); w.w2.w16 = w16_of(l.w2); w.w3.w16 = w16_of(l.w3);
        }
        if (m.output) p->output.w16 = w16_of(m.output);
        p->w16_gen = g.w16_gen;
    }
    // [x + r ->] rms_norm * w -> Q8 -> f16 operand of the next GEMM
    auto norm_quant = [&](const float *x, const float *x2, const float *r, float *xsum, const float *w, float *y_f32) {
        Timed tm(GGML_HIP_KCLASS_OTHER, (double)N * E * (r ? 18.0 : 6.0));
        if (E > 8192) die("prompt plan: rows of %lld elements (k_p_norm_quant holds a row of up to 8192 in registers)", (long long)E);
        if (kq) {
            if (r)
                hipLaunchKernelGGL((k_p_norm_quant<false, true, true>), dim3(N), dim3(256), (size_t)E * 4, g.stream, x, x2, r, xsum, w, m.eps, (int)E, y_f32, p->p_x16);
            else
                hipLaunchKernelGGL((k_p_norm_quant<false, false, true>), dim3(N), dim3(256), (size_t)E * 4, g.stream, x, x2, r, xsum, w, m.eps, (int)E, y_f32, p->p_x16);
        } else if (r) {
            if (f16d)
                hipLaunchKernelGGL((k_p_norm_quant<true, true>), dim3(N), dim3(256), (size_t)E * 4, g.stream, x, x2, r, xsum, w, m.eps, (int)E, y_f32, p->p_x16);
            else
                hipLaunchKernelGGL((k_p_norm_quant<false, true>), dim3(N), dim3(256), (size_t)E * 4, g.stream, x, x2, r, xsum, w, m.eps, (int)E, y_f32, p->p_x16);
        } else {
            if (f16d)
                hipLaunchKernelGGL((k_p_norm_quant<true, false>), dim3(N), dim3(256), (size_t)E * 4, g.stream, x, x2, r, xsum, w, m.eps, (int)E, y_f32, p->p_x16);
            else
                hipLaunchKernelGGL((k_p_norm_quant<false, false>), dim3(N), dim3(256), (size_t)E * 4, g.stream, x, x2, r, xsum, w, m.eps, (int)E, y_f32, p->p_x16);
        }
        HIP_CHECK(hipGetLastError());
    };
    // A GEMM whose tile count leaves CUs idle splits K in two (mmq_auto_splits, as in the node-by-node executor).  There
    // the halves meet through f32 atomics in a zeroed dst; here each half stores its partial tile (`stride` floats
    // apart) and the kernel that consumes the result adds the two — the same two addends, no memset, no atomics
    // (an E x E GEMM at 512 tokens: 41 -> ~31 us).  Returns the number of splits used.
    const int tiles_n = (N + MMQ_TN - 1) / MMQ_TN;
    const int64_t te_stride = (int64_t)N * E, qkv_stride = (int64_t)N * (E + 2 * m.Egqa), g13_stride = (int64_t)N * 2 * F;
    int sp_qkv = 1, sp_13 = 1, sp_w2 = 1;
    auto gemm = [&](const QWeight &w, float *dst, int64_t nb, int64_t stride) {
        const MmqSegHost seg{w, dst, w.M};
        const int sp = mmq_auto_splits((int)((w.M + MMQ_TM - 1) / MMQ_TM) * tiles_n, nb, true);
        mmq_f16_launch_multi(qt, 1, &seg, p->p_x16, N, nb, true, sp, false, stride);
        return sp;
    };
    // matrices that share the activations go out as ONE launch when each of them would take the same K split on its own
    // (same arithmetic as separate launches, bit for bit); their outputs are one contiguous buffer starting at dsts[0]
    auto gemm_multi = [&](int nseg, const QWeight *const *ws, float *const *dsts, int64_t nb, int64_t stride) {
        MmqSegHost segs[3];
        int splits = 0;
        bool same = (g.opt_mmq_fuse & (nseg == 3 ? 1 : 2)) != 0;  // option mmq_fuse: bit 0 = wq|wk|wv, bit 1 = w1|w3
        for (int i = 0; i < nseg; i++) {
            segs[i] = MmqSegHost{*ws[i], dsts[i], ws[i]->M};
            const int sp = mmq_auto_splits((int)((ws[i]->M + MMQ_TM - 1) / MMQ_TM) * tiles_n, nb, true);
            if (i == 0) splits = sp;
            same = same && sp == splits;
        }
        if (!same) {  // separate launches, each with its own split; the consumer adds partials for all matrices or for
                      // none, so an unsplit matrix next to a split one gets a zero second partial
            int any = 1;
            for (int i = 0; i < nseg; i++) any = std::max(any, gemm(*ws[i], dsts[i], nb, stride));
            if (any > 1)
                for (int i = 0; i < nseg; i++)
                    if (mmq_auto_splits((int)((ws[i]->M + MMQ_TM - 1) / MMQ_TM) * tiles_n, nb, true) == 1)
                        HIP_CHECK(hipMemsetAsync(dsts[i] + stride, 0, (size_t)ws[i]->M * N * 4, g.stream));
            return any;
        }
        mmq_f16_launch_multi(qt, nseg, segs, p->p_x16, N, nb, true, splits, false, stride);
        return splits;
    };
    static DevOnce attr_set;
    if (attr_set.first()) {
        HIP_CHECK(hipFuncSetAttribute((const void *)k_gemm_f16, hipFuncAttributeMaxDynamicSharedMemorySize, MMQ_LDS));
        HIP_CHECK(hipFuncSetAttribute((const void *)k_gemm_f16_b16, hipFuncAttributeMaxDynamicSharedMemorySize, MMQ_LDS));
    }
    if (!m.wte) {
        HIP_CHECK(hipMemcpyAsync(p->xa, p->stage_in, (size_t)N * E * 4, hipMemcpyDeviceToDevice, g.stream));
    } else if (kq) {
        Timed tm(GGML_HIP_KCLASS_OTHER, (double)N * E * 4.6);
        dequant_k_rows(p->k_wte, (const int *)p->p_tok, N, p->xa, E);
    } else {
        Timed tm(GGML_HIP_KCLASS_OTHER, (double)N * E * 4.6);
        hipLaunchKernelGGL(k_get_rows_q, dim3((unsigned)((nbE + 255) / 256), (unsigned)N), dim3(256), 0, g.stream, p->wte,
                           (const int *)p->p_tok, p->xa, E);
        HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_rope_table, dim3((unsigned)N), dim3(128), 0, g.stream, (const DecParams *)p->prm, theta_scale,
                       m.freq_scale, (int)(m.D >> 1), p->rope);
    HIP_CHECK(hipGetLastError());
    for (int il = 0; il < m.L; il++) {
        const DecodePlan::LW &w = p->lw[il];
        __half *mk = p->mem_k + (size_t)il * m.C * m.Egqa, *mv = p->mem_v + (size_t)il * m.C * m.Egqa;
        // inpSA (xa) = the previous layer's inpFF + its w2 output; cur = rms_norm(inpSA) * attn_norm
        if (il == 0)
            norm_quant(p->xa, nullptr, nullptr, nullptr, w.attn_norm, nullptr);
        else
            norm_quant(p->p_te, sp_w2 > 1 ? p->p_te + te_stride : nullptr, p->xb, p->xa, w.attn_norm, nullptr);
        {
            const QWeight *ws[3] = {&w.wq, &w.wk, &w.wv};
            float *ds[3] = {p->p_qf, p->p_kf, p->p_vf};
            sp_qkv = gemm_multi(3, ws, ds, nbE, qkv_stride);
        }
        {
            PQkvPost a;
            a.q = p->p_qf; a.kf = p->p_kf; a.vf = p->p_vf; a.tab = p->rope; a.mem_k = mk; a.mem_v = mv;
            a.N = N; a.E = (int)E; a.Egqa = (int)m.Egqa; a.D = (int)m.D; a.n_past = m.n_past; a.C = m.C;
            a.skip_q = fused_attn ? 1 : 0;  // the fused attention kernel rotates Q while loading it
            a.nb_rope = (int)(((int64_t)N * (((fused_attn ? 0 : E) + m.Egqa) / 4) + 255) / 256);
            a.part = sp_qkv > 1 ? qkv_stride : 0;
            a.vt_n = (N + 63) / 64;
            a.vt_m = (int)((m.Egqa + 63) / 64);
            Timed tm(GGML_HIP_KCLASS_OTHER, (double)N * (E * 8.0 + m.Egqa * 12.0));
            hipLaunchKernelGGL(k_p_qkv_post, dim3((unsigned)(a.nb_rope + a.vt_n * a.vt_m)), dim3(256), 0, g.stream, a);
            HIP_CHECK(hipGetLastError());
        }
        // the fused attention kernel hands wo its GEMM operand directly (k_p_quant4's arithmetic in its epilogue)
        // (K-quant model: a Q8_K super-block spans two heads, so the attention writes f32 and k_p_quant4 makes the operand)
        prompt_attention(fused_attn, p->p_qf, mk, mv, p->p_mg, p->p_sc, p->p_p16, N, E, m.Egqa, m.H, m.Hkv, m.D, m.n_past, m.C, m.kq_scale,
                         fused_attn && !kq ? p->p_x16 : nullptr, f16d, fused_attn ? p->rope : nullptr, fused_attn && sp_qkv > 1 ? qkv_stride : 0);
        if (!fused_attn || kq) {
            Timed tm(GGML_HIP_KCLASS_OTHER, (double)N * E * 6.0);
            const int64_t n4 = (int64_t)N * E / 4;
            if (kq)
                hipLaunchKernelGGL((k_p_quant4<false, true>), dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, g.stream, (const f32x4 *)p->p_mg, n4, p->p_x16);
            else if (f16d)
                hipLaunchKernelGGL(k_p_quant4<true>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, g.stream, (const f32x4 *)p->p_mg, n4, p->p_x16);
            else
                hipLaunchKernelGGL(k_p_quant4<false>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, g.stream, (const f32x4 *)p->p_mg, n4, p->p_x16);
            HIP_CHECK(hipGetLastError());
        }
        const int sp_wo = gemm(w.wo, p->p_te, nbE, te_stride);
        norm_quant(p->p_te, sp_wo > 1 ? p->p_te + te_stride : nullptr, p->xa, p->xb, w.ffn_norm, nullptr);  // inpFF (xb) = wo output + inpSA
        {
            const QWeight *ws[2] = {&w.w1, &w.w3};
            float *ds[2] = {p->p_g1, p->p_g3};
            sp_13 = gemm_multi(2, ws, ds, nbE, g13_stride);
        }
        {
            const int64_t n4 = (int64_t)N * F / 4;
            Timed tm(GGML_HIP_KCLASS_OTHER, (double)n4 * 40.0);
            if (kq)
                hipLaunchKernelGGL((k_p_silu_mul_quant<false, true>), dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, g.stream, (const f32x4 *)p->p_g1, (const f32x4 *)p->p_g3, n4, sp_13 > 1 ? g13_stride / 4 : 0, p->p_x16);
            else if (f16d)
                hipLaunchKernelGGL(k_p_silu_mul_quant<true>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, g.stream, (const f32x4 *)p->p_g1, (const f32x4 *)p->p_g3, n4, sp_13 > 1 ? g13_stride / 4 : 0, p->p_x16);
            else
                hipLaunchKernelGGL(k_p_silu_mul_quant<false>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, g.stream, (const f32x4 *)p->p_g1, (const f32x4 *)p->p_g3, n4, sp_13 > 1 ? g13_stride / 4 : 0, p->p_x16);
            HIP_CHECK(hipGetLastError());
        }
        sp_w2 = gemm(w.w2, p->p_te, nbF, te_stride);
    }
    if (!m.output) {  // a stage of a layer split hands the residual on: out = w2 output + inpFF
        const int64_t n4 = (int64_t)N * E / 4;
        Timed tm(GGML_HIP_KCLASS_OTHER, (double)N * E * 12.0);
        if (sp_w2 > 1) {
            hipLaunchKernelGGL(k_bin4<BIN_ADD>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, g.stream, (const f32x4 *)p->p_te,
                               (const f32x4 *)(p->p_te + te_stride), (f32x4 *)p->p_te, n4);
            HIP_CHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_bin4<BIN_ADD>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, g.stream, (const f32x4 *)p->p_te,
                           (const f32x4 *)p->xb, (f32x4 *)p->stage_out, n4);
        HIP_CHECK(hipGetLastError());
        return;
    }
    norm_quant(p->p_te, sp_w2 > 1 ? p->p_te + te_stride : nullptr, p->xb, p->xa, p->norm, p->emb_out);
    mmq_f16_launch(qt, p->output, p->p_x16, (float *)p->logits_out, m.V, N, nbE, true);
}

// option "attn_split": 0 off, 1 = from ATTN_SPLIT_MIN positions on, n > 1 = from n positions on (forward-declared above)
// fused: the short-context attention is k_qkv_attn (stays ahead of the split path for longer than k_attn_decode does)
static inline int64_t attn_split_min(bool fused) { return g.opt_attn_split > 1 ? g.opt_attn_split : fused ? ATTN_SPLIT_MIN_FUSED : ATTN_SPLIT_MIN; }
static inline int64_t attn_split_min_of(const LlamaMatch &m) { return attn_split_min(fused_qkv_shape(m).ok); }
static bool attn_one_ok(const LlamaMatch &m, int att_S);
// The attention variant of a single-token evaluation whose token sits at position T - 1 (see the enum above).  Option
// fuse_heads (default 1): contexts beyond k_qkv_attn's 512-position register window get 2 / 4 attention workgroups per head inside
// the wq|wk|wv launch instead of the separate split attention, where the chip has room for them.
static int attn_variant(const LlamaMatch &m, const DecodePlan *p, int64_t T) {
    if (m.N != 1) return AV_SHORT;
    const bool split_ok = (!m.kquant || attn_one_ok(m, p->att_S)) && g.opt_attn_split && g.opt_big && p->att_S >= 2;
    if (g.opt_fuse_heads && g.opt_attn_split == 1 && split_ok && T > FUSE_HEADS_MIN && fused_qkv_shape(m).ok) {
        const int S = (int)((T + 511) / 512);  // workgroups per head: 512 positions each
        if (S <= 4 && p->att_S >= S && fused_qkv_shape(m, S).ok) return S;  // = AV_FUSED2 / 3 / 4
    }
    return split_ok && T >= attn_split_min_of(m) ? AV_SPLIT : AV_SHORT;
}
// the split attention as one launch: every workgroup must be resident (they wait for each other); scores + probabilities of a
// range stay in LDS
static bool attn_one_ok(const LlamaMatch &m, int att_S) {
    const size_t chunk_max = ((((size_t)m.C + att_S - 1) / att_S) + 63) & ~(size_t)63;
    // (every workgroup of this launch waits for peers: it must have the GPU to itself — one slot per device)
    return g.opt_attn_one && device_sharers() == 1 && m.N == 1 && att_S <= 16 && (int64_t)m.H * att_S <= g.num_cus && chunk_max * 6 <= 60 * 1024 && m.D % 32 == 0 && m.D <= 128;
}
// returns true if the graph was executed by the fused decode plan
static inline uint64_t now_ns() {
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
               std::chrono::steady_clock::now().time_since_epoch()).count();
}
// ---- the end of a single-token plan run: wait, deliver the results, and look at the plan's error word ----
// k_qkv_attn / k_attn_split_one contain workgroups that wait for rows or partial results of OTHER workgroups of the same launch.
// That is only live while the whole launch is resident (one 1024-thread workgroup per CU).  Several slots of one process on a GPU
// are accounted for (fused_qkv_shape, attn_one_ok); another PROCESS on the GPU, or a CU mask, is invisible from here: the waits are
// bounded (GRAN_SPIN_MAX), the error word comes back with the token's results, and a token whose hand-off gave up is re-run on
// the kernels that do not wait inside a launch (k_mmvq_big + k_attn_decode / the three split launches — bit-identical results),
// which the slot then keeps; option fused_fallback = 0, a stage of a layer split (its garbage residual has already travelled
// on) and a device-sampled chain abort with the message instead.  SURVEY 8b: no error returns; never silent garbage.
static void plan_launch_decode(DecodePlan *p, unsigned mask, PlanStats *st, unsigned kind_mask, int av);
static int attn_variant(const LlamaMatch &m, const DecodePlan *p, int64_t T);
static void token_results_queue(DecodePlan *p) {
    if (p->m.N != 1 || p->m.prompt || !p->ferr) return;
    g.ferr_plan = p;  // the word itself needs no copy: the kernels write it into pinned host memory, visible once the token's
                      // result copies (queued behind its kernels) are done
}
static void token_finish(bool can_rerun = true) {
    d2h_finish();
    DecodePlan *p = (DecodePlan *)g.ferr_plan;
    g.ferr_plan = nullptr;
    if (!p || !g.ferr_pin || !*(volatile unsigned *)g.ferr_pin) return;
    *(volatile unsigned *)g.ferr_pin = 0;
    g.stat_fused_timeouts++;
    spec_cancel();
    static const char *what =
        "an attention workgroup of k_qkv_attn / k_attn_split_one gave up waiting for rows of its own launch (these launches "
        "need all their workgroups resident at once: is another process, or a CU mask, holding compute units of this GPU?)";
    bool live = false;
    for (auto *q : g_plans) live = live || q == p;
    if (!live) die("%s", what);
    const bool whole = p->m.wte && p->m.output;  // a stage's garbage residual has already been handed on
    if (!g.opt_fused_fallback || !can_rerun || !whole || p->m.N != 1)
        die("%s; set GGML_HIP_FUSE_ATTN=0 GGML_HIP_ATTN_ONE=0 to run the two-launch forms", what);
    static bool warned = false;
    if (!warned) fprintf(stderr, "libggml_hip: %s — re-running the token on the two-launch forms and keeping them on this device slot\n", what);
    warned = true;
    if (g.opt_fuse_attn || g.opt_attn_one) {  // what comes back after a clean stretch (try_decode_plan)
        g.fused_saved_fuse_attn = g.opt_fuse_attn;
        g.fused_saved_attn_one = g.opt_attn_one;
    }
    g.fused_rearm_stretch = g.fused_rearm_stretch ? g.fused_rearm_stretch * 2 : (uint64_t)std::max(0, g.opt_fused_rearm_tokens);
    g.fused_rearm_at = g.opt_fused_rearm_tokens > 0 ? g.stat_plan_tokens + g.fused_rearm_stretch : 0;
    g.opt_fuse_attn = 0;
    g.opt_attn_one = 0;
    if (!g.opt_test_fused_timeout) g.opt_affine = 0;  // (stays off when the fused forms come back: a placement the dealing cannot rely on is the likeliest cause)
    g.opt_test_fused_timeout = 0;
    for (auto *q : g_plans) drop_plan_graphs(q);
    const LlamaMatch &m = p->m;
    {   // this token and position again: a speculative run queued behind the token has moved the device's parameters on
        DecParams hp;
        memset(&hp, 0, sizeof(hp));
        hp.n_past = m.n_past;
        hp.token = m.embd ? ((const int32_t *)m.embd->data)[0] : 0;
        hp.tokens[0] = hp.token;
        h2d_small((char *)p->prm, &hp, sizeof(hp));
    }
    plan_launch_decode(p, ~0u, nullptr, ~0u, attn_variant(m, p, m.n_past + 1));
    if (m.logits && m.logits->backend == GGML_BACKEND_CPU) d2h_queue(m.logits->data, p->logits_out, (size_t)m.V * m.N * 4);
    if (m.embedding && m.embedding->data && p->emb_out) d2h_queue(m.embedding->data, (const char *)p->emb_out, (size_t)m.E * 4);
    d2h_finish();
    if (*(volatile unsigned *)g.ferr_pin) die("%s — and again on the re-run", what);
}

// ggml_hip_graph_prepare: the match of the NEXT token's graph, made while the device runs the current one.  Only the plain case is
// remembered — a single-token decode graph whose weights are resident and whose plan exists; everything else takes the usual way
// at its begin().  Nothing of the plan is touched here: the token in flight may still need DecodePlan::m for a re-run.
struct PrepMatch {
    ggml_cgraph *gr = nullptr;
    LlamaMatch m;
    DecodePlan *p = nullptr;
    uint64_t arena_seq = 0, wgen = 0;
    int opt_gen = 0;
};
static std::vector<uint64_t> plan_signature(const LlamaMatch &m);
static bool prepare_decode_plan(ggml_cgraph *gr) {
    if (!g.prep) g.prep = new PrepMatch();
    PrepMatch *pm = (PrepMatch *)g.prep;
    pm->gr = nullptr;
    if (!g.opt_plan || !g.opt_prepare || !gr) return false;
    LlamaMatch m;
    if (!match_llama_decode(gr, m) || m.prompt || m.N != 1 || !plan_weights_resident(m)) return false;
    const std::vector<uint64_t> sig = plan_signature(m);
    const uint64_t wgen = g_dev_wgen[g.device & 63].load(std::memory_order_acquire);
    DecodePlan *p = nullptr;
    for (auto *q : g_plans)
        if (q->sig == sig && q->wgen == wgen) p = q;
    if (!p) return false;  // the first token of a shape builds its plan the usual way
    pm->m = m;
    pm->p = p;
    pm->arena_seq = g_arena_seq.load(std::memory_order_acquire);
    pm->wgen = wgen;
    pm->opt_gen = g.opt_gen;
    pm->gr = gr;
    return true;
}

static bool try_decode_plan(ggml_cgraph *gr, bool defer_wait = false) {
    g.chain_plan = nullptr;  // any new graph ends the chainable state; a single-token plan run re-arms it below
    if (!g.opt_plan) return false;
    if (g.fused_rearm_at && g.stat_plan_tokens >= g.fused_rearm_at) {  // a clean stretch behind a hand-off that gave up: the fused forms again
        g.fused_rearm_at = 0;
        g.opt_fuse_attn = g.fused_saved_fuse_attn;
        g.opt_attn_one = g.fused_saved_attn_one;
        g.stat_fused_rearms++;
        spec_cancel();
        if (g.stream) HIP_CHECK(hipStreamSynchronize(g.stream));
        for (auto *q : g_plans) drop_plan_graphs(q);
    }
    const uint64_t t0 = now_ns();
    LlamaMatch m;
    DecodePlan *p = nullptr;
    if (PrepMatch *pm = (PrepMatch *)g.prep) {  // matched ahead of time (ggml_hip_graph_prepare) and nothing has happened since that could change the answer?
        if (pm->gr == gr && pm->arena_seq == g_arena_seq.load(std::memory_order_acquire) && pm->opt_gen == g.opt_gen &&
            pm->wgen == g_dev_wgen[g.device & 63].load(std::memory_order_acquire))
            for (auto *q : g_plans)
                if (q == pm->p) p = q;
        if (p) {
            m = pm->m;
            p->m = m;
            g.stat_prepared_tokens++;
        }
        pm->gr = nullptr;
    }
    if (!p) {
        if (!match_llama_decode(gr, m)) return false;
        if (!plan_weights_resident(m)) {
            // first evaluation of a model: tok_embeddings is a leaf the caller never offloads (models/llama lib.rs:52);
            // upload the graph's leaves the way the generic executor would, then look again
            upload_inputs(gr);
            if (!plan_weights_resident(m)) return false;
        }
        if (m.prompt && m.kquant && !k_prompt_weights(m, nullptr)) {  // (before anything is built or launched) no room for the copies:
            if (m.N > MULTI_MAX_N) return false;                       // the node-by-node executor, or for up to 31 tokens the K plan's chunks
            LlamaMatch m2;
            tl_k_prompt_off = true;
            const bool ok = match_llama_decode(gr, m2);
            tl_k_prompt_off = false;
            if (!ok) return false;
            m = m2;
        }
        std::vector<uint64_t> sig = plan_signature(m);
        const uint64_t wgen = g_dev_wgen[g.device & 63].load(std::memory_order_acquire);
        {   // plans built before some weight record of this device was freed (perhaps by a sibling slot): gone before anything matches them
            bool stale = false;
            for (auto *q : g_plans) stale = stale || q->wgen != wgen;
            if (stale) drop_all_plans();
        }
        for (auto *q : g_plans)
            if (q->sig == sig) p = q;
        if (!p) {
            if (g_plans.size() >= 32) drop_all_plans();
            p = build_plan(m, sig);
            p->wgen = wgen;
            g_plans.push_back(p);
        } else {
            p->m = m;  // same devices buffers, fresh tensor pointers of this evaluation (n_past, embd)
        }
    }
    const uint64_t t1 = now_ns();
    // ---- speculative next token: is this evaluation the one the device is already running? ----
    bool spec_hit = false;
    if (g.spec.pending) {
        g.spec.pending = false;
        const bool same = g.spec.plan == (void *)p && m.N == 1 && !m.prompt && m.embd && m.n_past == g.spec.n_past &&
                          attn_variant(m, p, m.n_past + 1) == g.spec.av && g.opt_graph && !g.timing.on;
        if (same) {
            HIP_CHECK(hipEventSynchronize(g.spec.tok_ev));  // long done: recorded right behind the argmax kernel of the previous token
            spec_hit = *g.spec.tok_pin == ((const int32_t *)m.embd->data)[0];
        }
        if (spec_hit) {
            g.stat_spec_hits++;
        } else {
            g.stat_spec_misses++;
            g.spec.cooldown = 8;  // a sampler that does not take the first maximum: stop guessing for a while
        }
    }
    DecParams hp;
    hp.n_past = m.n_past;
    hp.token = m.embd ? ((const int32_t *)m.embd->data)[0] : 0;
    hp.store_at = hp.pad1 = 0;
    for (int i = 0; i < 32; i++) {
        hp.tokens[i] = (m.embd && i < m.N && !m.prompt) ? ((const int32_t *)m.embd->data)[i] : 0;
        if (m.wte && (hp.tokens[i] < 0 || hp.tokens[i] >= m.wte->ne[1])) die("token id %d out of range", hp.tokens[i]);
    }
    if (!spec_hit) h2d_small((char *)p->prm, &hp, sizeof(hp));  // (a hit: the device wrote exactly these itself)
    if (m.prompt) {  // prompt plan: all token ids, launched eagerly
        if (m.wte) {
            const int32_t *ids = (const int32_t *)m.embd->data;
            for (int i = 0; i < m.N; i++)
                if (ids[i] < 0 || ids[i] >= m.wte->ne[1]) die("token id %d out of range", ids[i]);
            h2d_small((char *)p->p_tok, ids, (size_t)m.N * 4);
        }
        plan_launch_prompt(p);
        if (m.logits && m.logits->backend == GGML_BACKEND_CPU)
            d2h_queue(m.logits->data, p->logits_out, (size_t)m.V * m.N * 4);
        const uint64_t t2p = now_ns();
        g.ns_match += t1 - t0;
        g.ns_launch += t2p - t1;
        g.stat_prompt_plan_tokens += (uint64_t)m.N;
        if (defer_wait) {  // ggml_hip_graph_compute_begin (a batch of feed_prompt behind which another follows)
            g.pending_wait = true;
            g.pending_light = true;
            return true;
        }
        d2h_finish();
        g.ns_wait += now_ns() - t2p;
        return true;
    }
    const bool use_graph = g.opt_graph && !g.timing.on;
    {   // graphs captured while this device had another number of slots on it froze another choice of kernels
        const uint64_t dgen = g_dev_gen[g.device & 63].load(std::memory_order_relaxed);
        if (p->dev_gen != dgen) {
            if (p->dev_gen) {
                HIP_CHECK(hipStreamSynchronize(g.stream));
                drop_plan_graphs(p);
            }
            p->dev_gen = dgen;
        }
    }
    // the attention variant for this context length (a graph each of the same plan)
    const int av = attn_variant(m, p, m.n_past + 1);
    const bool long_ctx = av == AV_SPLIT;
    if (spec_hit) {
        // already enqueued behind the previous token (same plan, position, token and attention variant): only the results are missing
    } else if (use_graph) {
        hipGraph_t &gr_v = p->graph_v[av];
        hipGraphExec_t &ex_v = p->exec_v[av];
        if (!ex_v) {
            HIP_CHECK(hipStreamBeginCapture(g.stream, hipStreamCaptureModeThreadLocal));
            if (m.N > 1 && !m.kquant)
                plan_launch_multi(p);
            else
                plan_launch_decode(p, ~0u, nullptr, ~0u, av);
            HIP_CHECK(hipStreamEndCapture(g.stream, &gr_v));
            HIP_CHECK(hipGraphInstantiate(&ex_v, gr_v, nullptr, nullptr, 0));
        }
        HIP_CHECK(hipGraphLaunch(ex_v, g.stream));
        p->replays++;
    } else if (m.N > 1 && !m.kquant) {
        plan_launch_multi(p);
    } else {
        plan_launch_decode(p, ~0u, nullptr, ~0u, av);
    }
    if (spec_hit) {  // the speculative run's results sit in the plan's alternates: into the caller-visible mirrors first (stream order)
        HIP_CHECK(hipMemcpyAsync(p->logits_out, p->logits_alt, (size_t)m.V * 4, hipMemcpyDeviceToDevice, g.stream));
        if (p->emb_out) HIP_CHECK(hipMemcpyAsync(p->emb_out, p->emb_alt, (size_t)m.E * 4, hipMemcpyDeviceToDevice, g.stream));
    }
    // results the host reads: the logits (CPU-backend node, model/common.rs:6-38)
    if (m.logits && m.logits->backend == GGML_BACKEND_CPU)
        d2h_queue(m.logits->data, p->logits_out, (size_t)m.V * m.N * 4);
    // the embedding_result node is offloaded in the reference's graph, yet common::extract_embeddings reads its HOST pointer
    // (crates/llm-base/src/model/common.rs:41-59): a decode token's / prompt chunk's rows (16 KB per token) are mirrored to the node's
    // host data with the logits, so that an unchanged caller reads what the device computed.  (Bigger evaluations keep the node on
    // the device only: 8 MB per 512-token batch nobody may want — read it with ggml_hip_tensor_get, INTEGRATION.md.)
    if (m.embedding && m.embedding->data && p->emb_out && (size_t)m.N * (size_t)m.E * 4 <= ((size_t)128 << 10))
        d2h_queue(m.embedding->data, (const char *)p->emb_out, (size_t)m.N * (size_t)m.E * 4);
    token_results_queue(p);
    // ---- ... and the next one on spec: greedy token on the device, then the plan again, behind this token's result copies ----
    if (g.spec.cooldown > 0) g.spec.cooldown--;
    if (g.opt_speculate_next && g.spec.cooldown == 0 && use_graph && m.N == 1 && m.logits && m.wte && m.output &&
        m.n_past + 2 < m.C && p->exec_v[av]) {
        const int av2 = attn_variant(m, p, m.n_past + 2);
        {
            if (!g.results_ev) HIP_CHECK(hipEventCreateWithFlags(&g.results_ev, hipEventDisableTiming));
            if (!g.spec.tok_ev) {
                HIP_CHECK(hipEventCreateWithFlags(&g.spec.tok_ev, hipEventDisableTiming));
                HIP_CHECK(hipHostMalloc((void **)&g.spec.tok_pin, 64, hipHostMallocDefault));
                HIP_CHECK(hipMalloc((void **)&g.spec.tok_dev, 64));
            }
            HIP_CHECK(hipEventRecord(g.results_ev, g.stream));  // the host waits for THIS (d2h_finish), not for the stream's end
            g.results_ev_armed = true;
            g.results_ev_copies = stg.pending.size();
            hipLaunchKernelGGL(k_argmax_next, dim3(1), dim3(1024), 0, g.stream, (const float *)p->logits_out, (int)m.V, p->prm, g.spec.tok_dev);
            HIP_CHECK(hipMemcpyAsync(g.spec.tok_pin, g.spec.tok_dev, 4, hipMemcpyDeviceToHost, g.stream));
            HIP_CHECK(hipEventRecord(g.spec.tok_ev, g.stream));
            hipGraphExec_t &e2 = p->exec_s[av2];
            if (!e2) {  // the plan once more, captured with its final norm / lm_head aimed at the alternates (DecodePlan::logits_alt)
                p->spec_out = true;
                HIP_CHECK(hipStreamBeginCapture(g.stream, hipStreamCaptureModeThreadLocal));
                plan_launch_decode(p, ~0u, nullptr, ~0u, av2);
                HIP_CHECK(hipStreamEndCapture(g.stream, &p->graph_s[av2]));
                p->spec_out = false;
                HIP_CHECK(hipGraphInstantiate(&e2, p->graph_s[av2], nullptr, nullptr, 0));
            }
            HIP_CHECK(hipGraphLaunch(e2, g.stream));
            g.spec.pending = true;
            g.spec.plan = p;
            g.spec.n_past = m.n_past + 1;
            g.spec.av = av2;
        }
    }
    const uint64_t t2 = now_ns();
    g.ns_match += t1 - t0;
    g.ns_launch += t2 - t1;
    g.stat_plan_tokens += (uint64_t)m.N;
    if (long_ctx) g.stat_split_tokens++;
    if (m.N == 1 && !long_ctx) {
        const FusedShape fs = fused_qkv_shape(m, av_heads_split(av));
        if (fs.ok) g.stat_fused_tokens++;
        if (fs.ok && fs.wo) g.stat_fused_wo_tokens++;
        if (fs.ok && fs.affine) g.stat_fused_affine_tokens++;
    }
    if (av >= AV_FUSED2) g.stat_fused_heads_tokens++;
    if (m.kquant) g.stat_kplan_tokens += (uint64_t)m.N;
    g.chain_plan = (m.N == 1 && m.logits && m.wte) ? (void *)p : nullptr;  // whole model, one token: chainable
    g.chain_graph = gr;
    if (defer_wait) {  // ggml_hip_graph_compute_begin: the caller overlaps host work, then ..._end() waits
        g.pending_wait = true;
        g.pending_light = m.N > 1;  // (the waiting launches — fused attention, the one-launch split attention — are single-token forms)
        return true;
    }
    token_finish();
    g.ns_wait += now_ns() - t2;
    return true;
}

// SURVEY section 8f N3: n greedy tokens back to back without a host round trip per token.  `last` must be the cgraph
// of the caller's most recent ggml_graph_compute (a single-token LLaMA evaluation that ran as the fused plan, whole
// model on this device); the plan's decode parameters still hold that token and position on the device, and its
// logits are in HBM.  Per token: k_argmax_next (argmax -> parameters of the next replay) + one replay of the plan.
// Returns 0 and fills out_tokens[n] (and last_logits[V] with the logits after the n-th token, if not NULL); -1 if
// the precondition does not hold (the caller then decodes token by token).
static int decode_greedy_chain(ggml_cgraph *last, int n, int32_t *out_tokens, float *last_logits) {
    finish_pending();
    if (g.spec.pending) {  // the device has already gone one token further on its own: the caller decodes token by token (and hits)
        spec_cancel();
        return -1;
    }
    DecodePlan *p = (DecodePlan *)g.chain_plan;
    if (!p || g.chain_graph != last || n < 1) return -1;
    bool live = false;
    for (auto *q : g_plans) live = live || q == p;
    const LlamaMatch &m = p->m;
    if (!live || m.N != 1 || !m.logits || !m.wte || m.n_past + 1 + n > m.C) return -1;
    if (p->chain_cap < n) {
        if (p->chain_out) (void)hipFree(p->chain_out);
        p->chain_cap = std::max(n, 256);
        HIP_CHECK(hipMalloc((void **)&p->chain_out, (size_t)p->chain_cap * 4));
    }
    if (!p->chain_ring) HIP_CHECK(hipMalloc((void **)&p->chain_ring, 64 * 4));
    const bool use_graph = g.opt_graph && !g.timing.on && (p->exec_v[0] || p->exec_v[1] || p->exec_v[2] || p->exec_v[3] || p->exec_v[4]);
    int i0 = 0;
    // option chain_k = K (> 1): K tokens per graph launch — every kernel of the plan reads its token and position from the
    // DecParams that k_argmax_next advances on the device, so the launches of consecutive tokens are the same launches.  Only
    // while the whole group stays on the short-context attention variant; the graph's sampled ids land in chain_out[i0 ..].
    if (use_graph && g.opt_chain_k > 1) {
        const int K = g.opt_chain_k;
        const auto long_at = [&](int i) { return attn_variant(m, p, m.n_past + 1 + i + 1) != AV_SHORT; };
        while (i0 + K <= n && !long_at(i0 + K - 1)) {
            if (!p->exec_chain || p->chain_k != K) {  // (the graph writes its ids to a fixed ring: reusable at any offset)
                if (p->exec_chain) (void)hipGraphExecDestroy(p->exec_chain);
                if (p->graph_chain) (void)hipGraphDestroy(p->graph_chain);
                HIP_CHECK(hipStreamBeginCapture(g.stream, hipStreamCaptureModeThreadLocal));
                for (int k = 0; k < K; k++) {
                    hipLaunchKernelGGL(k_argmax_next, dim3(1), dim3(1024), 0, g.stream, (const float *)p->logits_out, (int)m.V, p->prm,
                                       p->chain_ring + k);
                    plan_launch_decode(p, ~0u, nullptr, ~0u, AV_SHORT);
                }
                HIP_CHECK(hipStreamEndCapture(g.stream, &p->graph_chain));
                HIP_CHECK(hipGraphInstantiate(&p->exec_chain, p->graph_chain, nullptr, nullptr, 0));
                p->chain_k = K;
            }
            HIP_CHECK(hipGraphLaunch(p->exec_chain, g.stream));
            if (fused_qkv_shape(m).ok) g.stat_fused_tokens += (uint64_t)K;
            HIP_CHECK(hipMemcpyAsync(p->chain_out + i0, p->chain_ring, (size_t)K * 4, hipMemcpyDeviceToDevice, g.stream));
            i0 += K;
        }
    }
    for (int i = i0; i < n; i++) {
        hipLaunchKernelGGL(k_argmax_next, dim3(1), dim3(1024), 0, g.stream, (const float *)p->logits_out, (int)m.V, p->prm,
                           p->chain_out + i);
        // the token of step i sits at position n_past + 1 + i; same rule as try_decode_plan for the attention variant
        const int av = attn_variant(m, p, m.n_past + 1 + i + 1);
        if (av != AV_SPLIT && fused_qkv_shape(m, av_heads_split(av)).ok) g.stat_fused_tokens++;
        if (av >= AV_FUSED2) g.stat_fused_heads_tokens++;
        if (use_graph) {
            hipGraph_t &gr_v = p->graph_v[av];
            hipGraphExec_t &e1 = p->exec_v[av], &e2 = p->exec2_v[av];
            if (!e1) {  // the chain crossed into a variant no evaluation has captured yet
                HIP_CHECK(hipStreamBeginCapture(g.stream, hipStreamCaptureModeThreadLocal));
                plan_launch_decode(p, ~0u, nullptr, ~0u, av);
                HIP_CHECK(hipStreamEndCapture(g.stream, &gr_v));
                HIP_CHECK(hipGraphInstantiate(&e1, gr_v, nullptr, nullptr, 0));
            }
            if (!e2) HIP_CHECK(hipGraphInstantiate(&e2, gr_v, nullptr, nullptr, 0));
            HIP_CHECK(hipGraphLaunch((i & 1) ? e2 : e1, g.stream));
        } else {
            plan_launch_decode(p, ~0u, nullptr, ~0u, av);
        }
    }
    HIP_CHECK(hipGetLastError());
    d2h_queue(out_tokens, (const char *)p->chain_out, (size_t)n * 4);
    if (last_logits) d2h_queue(last_logits, p->logits_out, (size_t)m.V * 4);
    token_results_queue(p);
    token_finish(false);  // a hand-off that gave up inside the chain has already fed the sampler garbage: abort
    p->m.n_past += n;
    p->replays += use_graph ? (uint64_t)n : 0;
    g.stat_plan_tokens += (uint64_t)n;
    g.chain_plan = nullptr;  // the caller's next evaluation re-arms it
    return 0;
}
