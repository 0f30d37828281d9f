// plan_build.inc — from a LlamaMatch to a DecodePlan: resident weights, the signature plans are cached by, the activation pool.
// the device record of a graph leaf: offloaded by the caller, or uploaded by the executor
static DevTensor *plan_rec(const ggml_tensor *t) {
    DevTensor *e = extra_of(t);
    if (!e) e = find_tensor((uintptr_t)t->data);
    return e;
}
static KWeight plan_kw(const ggml_tensor *t) {
    DevTensor *e = plan_rec(t);
    if (!e || !e->ksoa || (uintptr_t)t->data != e->host) die("decode plan: K-quant weight '%s' has no resident planar copy", t->name);
    return e->kw;
}
static QWeight plan_qw(const ggml_tensor *t) {
    DevTensor *e = plan_rec(t);
    if (!e || !e->soa || (uintptr_t)t->data != e->host) die("decode plan: weight '%s' has no resident SoA copy", t->name);
    return e->qw;
}
// an F16 matrix: the record's bytes are the tensor's rows — pointer, row stride and row count are all the plan keeps
static F16W plan_f16w(const ggml_tensor *t) {
    DevTensor *e = plan_rec(t);
    if (!e || e->soa || e->ksoa) die("decode plan: F16 weight '%s' has no resident copy", t->name);
    return F16W{(const __half *)(e->dev + ((uintptr_t)t->data - e->host)), (int64_t)t->nb[1] / 2, t->ne[1]};
}
static uint64_t rec_id(const ggml_tensor *t) {
    DevTensor *e = plan_rec(t);
    return e ? (uint64_t)(uintptr_t)e->dev : 0;
}

static bool plan_weights_resident(const LlamaMatch &m) {
    auto ok_q = [](const ggml_tensor *t) {
        DevTensor *e = plan_rec(t);
        if (t->type == GGML_TYPE_F16) return e && !e->soa && !e->ksoa && f16_weight_ok(plan_f16w(t));  // the raw rows
        return e && (e->soa || e->ksoa) && (uintptr_t)t->data == e->host;
    };
    auto ok_raw = [](const ggml_tensor *t) {
        DevTensor *e = plan_rec(t);
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

// session = false: what a batched step's graphs must share and its plan is cached by — the model and the shape, not the caches and result nodes
static std::vector<uint64_t> plan_signature(const LlamaMatch &m, bool session = true) {
    std::vector<uint64_t> s;
    auto f2u = [](float f) { uint32_t u; memcpy(&u, &f, 4); return (uint64_t)u; };
    s.push_back((uint64_t)m.N);
    for (uint64_t v : {(uint64_t)m.L, (uint64_t)m.E, (uint64_t)m.H, (uint64_t)m.Hkv, (uint64_t)m.D, (uint64_t)m.F,
                       (uint64_t)m.V, (uint64_t)m.C, (uint64_t)m.n_dims, (uint64_t)m.wtype, f2u(m.eps),
                       f2u(m.freq_base), f2u(m.freq_scale), f2u(m.kq_scale)})
        s.push_back(v);
    for (const ggml_tensor *t : {m.wte, m.norm, m.output, m.stage_in, m.stage_out}) s.push_back(t ? rec_id(t) : 0);
    if (session)
        for (const ggml_tensor *t : {m.memory_k, m.memory_v}) s.push_back(rec_id(t));
    for (auto &l : m.layers)
        for (const ggml_tensor *t : {l.attn_norm, l.wq, l.wk, l.wv, l.wo, l.ffn_norm, l.w1, l.w2, l.w3})
            s.push_back(rec_id(t));
    if (m.f16w) {  // an F16 weight record is pointer, stride and rows: a view of another part of a record is another weight
        auto rec = [&](const ggml_tensor *t) {
            if (!t) return;
            s.push_back((uint64_t)(uintptr_t)t->data);
            s.push_back((uint64_t)t->nb[1]);
            s.push_back((uint64_t)t->ne[1]);
        };
        rec(m.wte);
        rec(m.output);
        for (auto &l : m.layers)
            for (const ggml_tensor *t : {l.wq, l.wk, l.wv, l.wo, l.w1, l.w2, l.w3}) rec(t);
    }
    if (!session) return s;
    s.push_back(m.logits ? (uint64_t)(uintptr_t)dev_ptr(m.logits) : 0);
    s.push_back(m.embedding ? (uint64_t)(uintptr_t)dev_ptr(m.embedding) : 0);
    return s;
}
// Prompt plan of a K-quant model: its GEMMs have no operand but the resident f16 copy of each weight (mul_mat_k_gemm,
// backend_ops.inc) — every matrix must have one before anything is launched; they are made here, all or none, by the first batch
// the prompt plan sees (mmq_min = 32 tokens and more; the executor alone waits for W16_MIN_TOKENS, but without a copy its K path
// streams every matrix through the mat-vec kernel: 1.7k tok/s at n_batch = 48).  false = no room: the node-by-node executor runs.
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
// batch: the plan of a batched step (m: its first graph's match with N = the columns)
static DecodePlan *build_plan(const LlamaMatch &m, std::vector<uint64_t> sig, bool batch = false) {
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
    if (m.wte) (m.f16w ? (void)(p->f_wte = plan_f16w(m.wte)) : m.kquant ? (void)(p->k_wte = plan_kw(m.wte)) : (void)(p->wte = plan_qw(m.wte)));
    if (m.output) {
        if (m.f16w) p->f_output = plan_f16w(m.output);
        else if (m.kquant) p->k_output = plan_kw(m.output);
        else p->output = plan_qw(m.output);
        p->norm = (const float *)dev_ptr(m.norm);
    }
    if (m.stage_in) p->stage_in = (float *)dev_ptr(m.stage_in);
    if (m.stage_out) p->stage_out = (float *)dev_ptr(m.stage_out);
    p->batch = batch;
    if (!batch) {
        p->mem_k = (__half *)dev_ptr(m.memory_k);
        p->mem_v = (__half *)dev_ptr(m.memory_v);
    }
    for (auto &l : m.layers) {
        DecodePlan::LW w;
        memset(&w, 0, sizeof(w));
        if (m.f16w) {
            DecodePlan::FLW fw;
            fw.wq = plan_f16w(l.wq); fw.wk = plan_f16w(l.wk); fw.wv = plan_f16w(l.wv); fw.wo = plan_f16w(l.wo);
            fw.w1 = plan_f16w(l.w1); fw.w2 = plan_f16w(l.w2); fw.w3 = plan_f16w(l.w3);
            p->flw.push_back(fw);
        } else if (m.kquant) {
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
    if (m.embedding && !batch) p->emb_out = (float *)dev_ptr(m.embedding);
    if (m.logits && !batch) p->logits_out = dev_ptr(m.logits);
    // one pool for all persistent activations
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = (off + bytes + 255) & ~(size_t)255; return o; };
    const size_t R = (size_t)m.N;  // activation rows: 1 for decode, 2..8 for a prompt chunk, more for the prompt plan
    const int att_S = plan_att_S(m.H);
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
    const size_t o_bcols = take(batch ? sizeof(BatchCols) : 0), o_blogits = take(batch ? R * m.V * 4 : 0), o_bemb = take(batch ? R * m.E * 4 : 0);
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
                 o_katt = take(m.kquant || m.f16w ? R * m.E * 4 : 0), o_kg3 = take(m.kquant ? R * m.F * 4 : 0),
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
    if (batch) {
        p->bcols = (BatchCols *)(p->pool + o_bcols);
        p->logits_out = p->pool + o_blogits;
        p->emb_out = (float *)(p->pool + o_bemb);
    }
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
    if (m.f16w) p->k_att = (float *)(p->pool + o_katt);  // the F16 plan's attention output: the f32 row wo stages
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
