// plan_match.inc — the structural matcher of the LLaMA graph (see plan_shapes.inc for the plan files): fills a LlamaMatch or says no.
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
// set while prompt_pack (plan_pack.inc) matches its graphs: each is a segment of a prompt-plan evaluation whatever its own token count
static thread_local bool tl_match_pack = false;
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
        MATCH(is_leaf(m.output) && (qt_of(m.output->type) >= 0 || kt_of(m.output->type) >= 0 || m.output->type == GGML_TYPE_F16));
        m.wtype = m.output->type;
        m.kquant = kt_of(m.output->type) >= 0;
        m.f16w = m.output->type == GGML_TYPE_F16;
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
            MATCH(qt_of(lw.w2->type) >= 0 || kt_of(lw.w2->type) >= 0 || lw.w2->type == GGML_TYPE_F16);
            m.wtype = lw.w2->type;
            m.kquant = kt_of(lw.w2->type) >= 0;
            m.f16w = lw.w2->type == GGML_TYPE_F16;
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
    // The output matrix disagrees with the layers: the model is what its layers are.  Block-format layers under a K output — what
    // llama.cpp's quantizer writes for every block-format file type whose output has dimensions in multiples of 256 — are a block-format
    // model whose lm_head alone runs as the K plan's launches (out_k; option plan_out_k, 0 = the node-by-node executor as before the
    // option existed).  Every other disagreement fails the per-matrix type check below.
    if (m.output && m.kquant && qt_of(m.layers[0].wq->type) >= 0) {
        MATCH(g.opt_plan_out_k);
        m.wtype = m.layers[0].wq->type;
        m.kquant = false;
        m.out_k = true;
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
    // F16 weights (option plan_f16; 0 = the node-by-node executor, as before the F16 plan existed): decode, chunks of up to 31 tokens and
    // batched steps on k_mmvq_f16; a batch of mmq_min tokens and more stays on the executor, which runs it on k_gemm_f16
    if (m.f16w) {
        MATCH(g.opt_plan_f16 && m.N >= 1 && m.N <= MULTI_MAX_N && (g.opt_mmq_min <= 0 || m.N < g.opt_mmq_min) && m.n_past + m.N <= m.C);
        MATCH(m.D == m.n_dims && f16_plan_shape_ok(m) && attn_decode_lds(m.C, m.D) <= ATTN_DECODE_LDS_MAX);
        for (auto &lw : m.layers)
            for (int i = 0; i < LAYER_MATS; i++) {
                const ggml_tensor *w = lw.at(i);
                MATCH(is_leaf(w) && w->type == GGML_TYPE_F16 && w->ne[2] == 1 && w->ne[3] == 1 && ggml_is_contiguous(w));
            }
        for (const ggml_tensor *w : {m.wte, m.output})
            MATCH(!w || (w->type == GGML_TYPE_F16 && w->ne[2] == 1 && w->ne[3] == 1 && ggml_is_contiguous(w)));
        m.prompt = false;
        return true;
    }
    const bool k_early = m.kquant && g.opt_mmq_w16 && g.opt_plan_prompt && !g.opt_mmq_i8;  // (the early switch only where that plan can run)
    m.prompt = m.N > 8 && g.opt_mmq_min > 0 && m.N >= (k_early ? std::min(g.opt_mmq_min, std::max(9, g.opt_k_prompt_min)) : g.opt_mmq_min);
    if (m.kquant && tl_k_prompt_off && m.N <= MULTI_MAX_N) m.prompt = false;
    if (tl_match_pack) m.prompt = true;  // (one token or many: the pack's rows run on the prompt plan, so its conditions are the ones that count)
    if (!m.prompt) MATCH(attn_decode_lds(attn_decode_rows(m.C, m.N, m.H), m.D) <= ATTN_DECODE_LDS_MAX);
    if (m.prompt) {  // prompt plan (plan_launch_prompt): the default f16 GEMM path only, score buffer bounded
        MATCH(g.opt_plan_prompt && !g.opt_mmq_i8);
        MATCH(m.n_past + m.N <= m.C && m.D % 8 == 0 && m.D <= 128);
        MATCH((double)m.H * m.N * (m.n_past + m.N) * 4.0 <= 8e9);  // the scores of one layer
    } else if (m.kquant) {  // the K plan's own conditions follow below
    } else if (m.N > 8) {  // multi-token plan in passes of 8 columns: k_mmq_cols only (kernels/mmq_cols.h)
        MATCH(g.opt_plan_multi && g.opt_big && m.N <= MULTI_MAX_N && m.n_past + m.N <= m.C && qt_of(m.wtype) >= 0);
        MATCH(m.E % 32 == 0 && m.F % 32 == 0);
        const MultiCols mc = multi_cols(m);
        MATCH(mc.qkv && mc.wo && mc.gate && mc.w2 && (mc.out || !m.output || m.out_k));  // (out_k: the lm_head does not run on k_mmq_cols)
    } else if (m.N > 1) {  // multi-token plan (kernels/decode_big8.h): 8 Q8 columns of the widest row must fit LDS
        MATCH(g.opt_plan_multi && g.opt_big && multi_shape_ok(m, m.N));
        MATCH(m.n_past + m.N <= m.C);
    }
    for (auto &lw : m.layers)
        for (int i = 0; i < LAYER_MATS; i++) {
            const ggml_tensor *w = lw.at(i);
            MATCH(is_leaf(w) && (m.kquant ? kt_of(w->type) >= 0 : w->type == m.wtype));
        }
    if (m.out_k) {  // the lm_head's own conditions: super-blocks of 256; a prompt batch multiplies by the resident f16 copy of the output (no other
                    // operand); decode, chunks and batched steps (whose columns are matched here one by one, at N = 1) need a column of the
                    // helper launches in LDS — the weaker condition for every E k_mmvq_kbig takes (out_k_big: E <= 8192), so it is asked always
        MATCH(m.E % 256 == 0 && (!m.prompt || g.opt_mmq_w16));
        MATCH(m.prompt || (size_t)m.E + (size_t)(m.E / 256) * 68 <= 150 * 1024);
    }
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

// ---------------------------------------------------------------------------------------------------
// MPT (crates/models/mpt/src/lib.rs:93-259 as llm_amd/mpt.py builds it with every node offloaded): the single-token graph, for the MPT
// plan (plan_decode.inc plan_launch_mpt; option plan_mpt).  Per layer, from the residual x:
//   cur = mul(norm(x), norm_1) -> qkv = mul_mat(Wqkv, cur) -> views at 0, E, 2E -> cpy(K view, memory_k row) | cpy(V view, memory_v row)
//   q = permute(cpy(Q view, [D, H, 1])) ; k = permute(reshape_3d(view_1d(memory_k)))            -> kq = mul_mat(k, q)
//   soft_max(diag_mask_inf(alibi(scale(kq))))  ; vt = cpy(permute(reshape_3d(view_1d(memory_v)), 1, 2, 0, 3), [T, D, H] f16)
//   cpy(permute(mul_mat(vt, p)), [E, 1]) -> x = add(x, mul_mat(out_proj, .))
//   x = add(x, mul_mat(down_proj, gelu(mul_mat(up_proj, mul(norm(x), norm_2)))))
// then mul(norm(x), norm_f) and mul_mat(wte, .) with the leaf get_rows read: 35 nodes per layer + 4. The vt copy is matched and never
// executed: its destination has the one reader, which the plan's attention replaces.  No node but the logits may be mirrored to the
// host (the reference's own form never offloads, every node is mirrored: the executor's).
// ---------------------------------------------------------------------------------------------------
static bool match_mpt_norm(const ggml_tensor *mul, Claims &c, const ggml_tensor *&x, const ggml_tensor *&gain, const LlamaMatch &m) {
    MATCH(is_op(mul, GGML_OP_MUL) && mul->type == GGML_TYPE_F32 && !mirrored_to_host(mul));
    const ggml_tensor *nr = mul->src[0];
    MATCH(is_op(nr, GGML_OP_NORM) && !mirrored_to_host(nr) && nr->ne[0] == m.E && nr->ne[1] == 1 && ggml_nelements(nr) == m.E);
    gain = mul->src[1];
    MATCH(is_leaf(gain) && gain->type == GGML_TYPE_F32 && ggml_nelements(gain) == m.E && gain->ne[0] == m.E);
    x = nr->src[0];
    MATCH(x && x->type == GGML_TYPE_F32 && ggml_is_contiguous(x));
    c.take(mul);
    c.take(nr);
    return true;
}
static bool match_mpt_decode(ggml_cgraph *gr, LlamaMatch &m) {
    const int n = gr->n_nodes;
    MATCH(g.opt_plan_mpt && g.opt_big && n >= 39);
    Claims c;
    c.index(gr);
    auto dev_op = [&](const ggml_tensor *t, ggml_op op) { return is_op(t, op) && !mirrored_to_host(t); };
    m.mpt = true;
    m.N = 1;
    m.eps = 1e-5f;  // ggml_norm's (op_norm)
    ggml_tensor *last = gr->nodes[n - 1];
    MATCH(is_op(last, GGML_OP_MUL_MAT) && last->type == GGML_TYPE_F32 && last->ne[1] == 1 && last->ne[2] == 1 && last->ne[3] == 1);
    MATCH(last->backend == GGML_BACKEND_CPU && last->data && ggml_is_contiguous(last));  // the results go to the node's host data
    m.output = last->src[0];
    MATCH(is_leaf(m.output) && qt_of(m.output->type) >= 0);
    m.wtype = m.output->type;
    m.E = m.output->ne[0];
    m.V = m.output->ne[1];
    m.logits = last;
    c.take(last);
    ggml_tensor *fin = last->src[1];
    const ggml_tensor *x = nullptr;
    MATCH(match_mpt_norm(fin, c, x, m.norm, m));
    m.embedding = fin;
    {   // number of layers = length of the residual chain add(add(x, ..), ..) below the tail
        int cnt = 0;
        const ggml_tensor *y = x;
        while (is_op(y, GGML_OP_ADD) && is_op(y->src[0], GGML_OP_ADD) && cnt < 4096) {
            y = y->src[0]->src[0];
            cnt++;
        }
        MATCH(cnt >= 1);
        m.L = cnt;
    }
    m.F = 4 * m.E;
    m.layers.resize(m.L);
    for (int il = m.L - 1; il >= 0; il--) {
        LayerW &lw = m.layers[il];
        // x = add(inpFF, mul_mat(down_proj, gelu(mul_mat(up_proj, mul(norm(inpFF), norm_2)))))
        MATCH(dev_op(x, GGML_OP_ADD) && ggml_nelements(x) == m.E);
        const ggml_tensor *inpFF = x->src[0], *dn = x->src[1];
        MATCH(dev_op(dn, GGML_OP_MUL_MAT));
        lw.w2 = dn->src[0];
        const ggml_tensor *ge = dn->src[1];
        MATCH(dev_op(ge, GGML_OP_UNARY) && ge->op_params[0] == GGML_UNARY_OP_GELU);
        const ggml_tensor *up = ge->src[0];
        MATCH(dev_op(up, GGML_OP_MUL_MAT));
        lw.w1 = lw.w3 = up->src[0];
        MATCH(is_leaf(lw.w1) && is_leaf(lw.w2) && lw.w1->ne[0] == m.E && lw.w1->ne[1] == m.F && lw.w2->ne[0] == m.F && lw.w2->ne[1] == m.E);
        c.take(x); c.take(dn); c.take(ge); c.take(up);
        const ggml_tensor *nx = nullptr;
        MATCH(match_mpt_norm(up->src[1], c, nx, lw.ffn_norm, m) && nx == inpFF);
        // inpFF = add(inpSA, mul_mat(out_proj, merged))
        MATCH(dev_op(inpFF, GGML_OP_ADD));
        const ggml_tensor *inpSA = inpFF->src[0], *mo = inpFF->src[1];
        MATCH(dev_op(mo, GGML_OP_MUL_MAT));
        lw.wo = mo->src[0];
        MATCH(is_leaf(lw.wo) && lw.wo->ne[0] == m.E && lw.wo->ne[1] == m.E);
        const ggml_tensor *merged = mo->src[1];
        MATCH(is_op(merged, GGML_OP_CPY) && merged->type == GGML_TYPE_F32 && merged->ne[0] == m.E && merged->ne[1] == 1 && ggml_nelements(merged) == m.E &&
              ggml_is_contiguous(merged) && is_leaf(merged->src[1]));
        const ggml_tensor *perm = merged->src[0];
        MATCH(is_op(perm, GGML_OP_PERMUTE) && perm_0213(perm));
        const ggml_tensor *kqv = perm->src[0];
        MATCH(dev_op(kqv, GGML_OP_MUL_MAT));
        c.take(inpFF); c.take(mo); c.take(merged); c.take(perm); c.take(kqv);
        // V re-laid per token (never executed) and the probabilities
        const ggml_tensor *vt = kqv->src[0], *probs = kqv->src[1];
        MATCH(is_op(vt, GGML_OP_CPY) && vt->type == GGML_TYPE_F16 && is_leaf(vt->src[1]) && ggml_is_contiguous(vt));
        const ggml_tensor *vp = vt->src[0];
        MATCH(is_op(vp, GGML_OP_PERMUTE) && vp->op_params[0] == 1 && vp->op_params[1] == 2 && vp->op_params[2] == 0 && vp->op_params[3] == 3);
        const ggml_tensor *vr = vp->src[0];
        MATCH(is_op(vr, GGML_OP_RESHAPE));
        const ggml_tensor *vv1 = vr->src[0];
        MATCH(is_op(vv1, GGML_OP_VIEW) && is_leaf(vv1->src[0]) && vv1->type == GGML_TYPE_F16);
        if (!m.memory_v) m.memory_v = vv1->src[0];
        MATCH(vv1->src[0] == m.memory_v);
        MATCH(dev_op(probs, GGML_OP_SOFT_MAX));
        const ggml_tensor *mask = probs->src[0];
        MATCH(dev_op(mask, GGML_OP_DIAG_MASK_INF));
        const ggml_tensor *al = mask->src[0];
        MATCH(dev_op(al, GGML_OP_ALIBI));
        const ggml_tensor *sc = al->src[0];
        MATCH(dev_op(sc, GGML_OP_SCALE));
        const ggml_tensor *kq = sc->src[0], *kqs = sc->src[1];
        MATCH(dev_op(kq, GGML_OP_MUL_MAT) && is_leaf(kqs) && kqs->type == GGML_TYPE_F32 && kqs->data && ggml_nelements(kqs) == 1);
        const float kqsv = *(const float *)kqs->data;
        float bias_max;
        memcpy(&bias_max, al->op_params + 2, 4);
        if (il == m.L - 1) {
            m.kq_scale = kqsv;
            m.n_past = al->op_params[0];
            m.H = al->op_params[1];
            m.alibi_bias_max = bias_max;
            MATCH(m.H >= 1 && m.H <= 256 && m.E % m.H == 0 && m.n_past >= 0);
            m.Hkv = m.H;
            m.D = m.E / m.H;
            m.Egqa = m.E;
        }
        MATCH(kqsv == m.kq_scale && al->op_params[0] == m.n_past && al->op_params[1] == m.H && bias_max == m.alibi_bias_max &&
              mask->op_params[0] == m.n_past);
        c.take(vt); c.take(vp); c.take(vr); c.take(vv1); c.take(probs); c.take(mask); c.take(al); c.take(sc); c.take(kq);
        const int P = m.n_past, T = P + 1;
        MATCH(kq->ne[0] == T && kq->ne[1] == 1 && kq->ne[2] == m.H && kq->ne[3] == 1);
        // K = permute(reshape_3d(view_1d(memory_k)))   Q = permute(cpy(view of qkv at 0, [D, H, 1]))
        const ggml_tensor *kp = kq->src[0], *qp = kq->src[1];
        MATCH(is_op(kp, GGML_OP_PERMUTE) && perm_0213(kp) && is_op(qp, GGML_OP_PERMUTE) && perm_0213(qp));
        const ggml_tensor *kr = kp->src[0];
        MATCH(is_op(kr, GGML_OP_RESHAPE));
        const ggml_tensor *kv1 = kr->src[0];
        MATCH(is_op(kv1, GGML_OP_VIEW) && is_leaf(kv1->src[0]) && kv1->type == GGML_TYPE_F16);
        if (!m.memory_k) m.memory_k = kv1->src[0];
        MATCH(kv1->src[0] == m.memory_k && m.memory_k != m.memory_v);
        if (m.C == 0) {  // the context: what the caches hold per layer
            MATCH(m.L > 0 && ggml_nelements(m.memory_k) % ((int64_t)m.L * m.E) == 0 && ggml_nelements(m.memory_k) == ggml_nelements(m.memory_v));
            m.C = ggml_nelements(m.memory_k) / ((int64_t)m.L * m.E);
        }
        MATCH(T <= m.C);
        for (const ggml_tensor *r3 : {kr, vr}) MATCH(r3->ne[0] == m.D && r3->ne[1] == m.H && r3->ne[2] == T && r3->ne[3] == 1);
        for (const ggml_tensor *v1 : {kv1, vv1}) MATCH(v1->ne[0] == (int64_t)T * m.E && ggml_nelements(v1) == (int64_t)T * m.E && v1->nb[0] == 2);
        MATCH(view_offset(kv1, m.memory_k) == (size_t)il * m.C * m.E * 2 && view_offset(vv1, m.memory_v) == (size_t)il * m.C * m.E * 2);
        MATCH(vt->ne[0] == T && vt->ne[1] == m.D && vt->ne[2] == m.H);
        const ggml_tensor *qcp = qp->src[0];
        MATCH(is_op(qcp, GGML_OP_CPY) && qcp->type == GGML_TYPE_F32 && is_leaf(qcp->src[1]) && ggml_is_contiguous(qcp) && qcp->ne[0] == m.D &&
              qcp->ne[1] == m.H && ggml_nelements(qcp) == m.E);
        const ggml_tensor *qv = qcp->src[0];
        MATCH(is_op(qv, GGML_OP_VIEW) && qv->type == GGML_TYPE_F32 && ggml_nelements(qv) == m.E && qv->ne[0] == m.E && qv->nb[0] == 4);
        const ggml_tensor *qkv = qv->src[0];
        MATCH(dev_op(qkv, GGML_OP_MUL_MAT) && qkv->ne[0] == 3 * m.E && ggml_nelements(qkv) == 3 * m.E && view_offset(qv, qkv) == 0);
        lw.wq = lw.wk = lw.wv = qkv->src[0];
        MATCH(is_leaf(lw.wq) && lw.wq->ne[0] == m.E && lw.wq->ne[1] == 3 * m.E);
        c.take(kp); c.take(qp); c.take(kr); c.take(kv1); c.take(qcp); c.take(qv); c.take(qkv);
        const ggml_tensor *nx1 = nullptr;
        MATCH(match_mpt_norm(qkv->src[1], c, nx1, lw.attn_norm, m) && nx1 == inpSA);
        lw.cur = qkv;
        x = inpSA;
    }
    MATCH(dev_op(x, GGML_OP_GET_ROWS));
    m.wte = x->src[0];
    m.embd = x->src[1];
    MATCH(m.wte == m.output && is_leaf(m.embd) && m.embd->type == GGML_TYPE_I32 && m.embd->ne[0] == 1 && ggml_nelements(m.embd) == 1 && m.embd->data);
    c.take(x);
    // the K/V stores: cpy(view of qkv at E | 2E, view_1d(memory_k | memory_v) at position n_past of the layer)
    for (int i = 0; i < n; i++) {
        const ggml_tensor *t = gr->nodes[i];
        if (c.claimed[i] || t->op != GGML_OP_CPY) continue;
        const ggml_tensor *dst = t->src[1], *src = t->src[0];
        MATCH(is_op(dst, GGML_OP_VIEW) && dst->type == GGML_TYPE_F16 && is_op(src, GGML_OP_VIEW) && src->type == GGML_TYPE_F32);
        const bool isk = dst->src[0] == m.memory_k;
        MATCH(isk || dst->src[0] == m.memory_v);
        int il = -1;
        for (int j = 0; j < m.L; j++)
            if (m.layers[j].cur == src->src[0]) il = j;
        MATCH(il >= 0 && !(isk ? m.layers[il].k_store : m.layers[il].v_store));
        MATCH(ggml_nelements(src) == m.E && src->ne[0] == m.E && src->nb[0] == 4 && view_offset(src, src->src[0]) == (size_t)(isk ? 1 : 2) * m.E * 4);
        MATCH(dst->ne[0] == m.E && ggml_nelements(dst) == m.E && dst->nb[0] == 2);
        MATCH(view_offset(dst, dst->src[0]) == ((size_t)il * m.C + m.n_past) * m.E * 2);
        (isk ? m.layers[il].k_store : m.layers[il].v_store) = true;
        c.take(t); c.take(dst); c.take(src);
    }
    for (auto &lw : m.layers) MATCH(lw.k_store && lw.v_store);
    MATCH(c.n == n);  // every node of the graph is accounted for
    // the plan's kernels' own preconditions
    MATCH(m.D % 32 == 0 && m.D <= 128 && m.E % 32 == 0 && m.E <= 8192);
    MATCH(m.memory_k->type == GGML_TYPE_F16 && m.memory_v->type == GGML_TYPE_F16);
    MATCH(attn_decode_lds((m.C + 7) & ~(int64_t)7, m.D) <= ATTN_DECODE_LDS_MAX);  // (k_attn_decode_alibi's arrays hold the context rounded up to 8)
    for (auto &lw : m.layers)
        for (int i = 0; i < LAYER_MATS; i++) MATCH(lw.at(i)->type == m.wtype && lw.at(i)->ne[2] == 1 && lw.at(i)->ne[3] == 1);
    MATCH(big_shape(XSRC_LNORM, EPI_QKV_TM, m.E / 32, 3 * m.E).ok && big_shape(XSRC_LNORM, EPI_GELU, m.E / 32, m.F).ok &&
          big_shape(XSRC_LNORM, EPI_STORE, m.E / 32, m.V).ok && big_shape(XSRC_F32, EPI_ADD, m.E / 32, m.E).ok &&
          big_shape(XSRC_F32, EPI_ADD, m.F / 32, m.E).ok && m.F <= 24 * BIG_T);
    return true;
}
#undef MATCH
