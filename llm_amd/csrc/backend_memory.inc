// backend_memory.inc — part of libggml_hip.so's backend translation unit (included by hip_backend.hip, inside its anonymous
// namespace where noted): persistent device tensors — SoA / planar re-layout of quantized weights at upload, records behind ggml_tensor.extra, release.  Inside the anonymous namespace.
// ---------------------------------------------------------------------------------------------------
// persistent device tensors
// ---------------------------------------------------------------------------------------------------
// The f16 scale planes (Q d / m, Q6_K d) are read as the aligned-pair 32-bit word that holds a scale (kernels/decode_big.h
// `issue`, kernels/kquant_big.h `load`): when a row has an odd number of blocks, the word of its last block reaches 2 bytes past
// the row — for the matrix's last row, past the plane.  Such a plane must end at least 2 bytes before the 256-byte boundary it is
// rounded up to.  The rounding alone leaves no slack when the plane is a multiple of 256 bytes long (odd block count and
// M % 128 == 0, e.g. 4096 rows of Q6_K at 11008 columns = 43 super-blocks, whose d plane is the last of the layout: the word
// read past it lay outside the layout), so those planes get 256 bytes more.  Even block counts never read past a row:
// their layout is unchanged.
size_t scale_plane_end(size_t o, size_t bytes, bool odd_rows) {
    const size_t end = (o + bytes + (odd_rows ? 2 : 0) + 255) & ~(size_t)255;
    if (odd_rows && end < o + bytes + 2) die("weight layout: a scale plane without 2 bytes of slack");
    return end;
}
size_t qw_layout(int qt, int64_t M, int64_t nb, size_t off[5]) {
    // returns total bytes; off = {qs, qs2, qh, d, m}
    const int64_t nblocks = M * nb;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    size_t o = 0;
    off[0] = o;
    o = al(o + (size_t)nblocks * 16);
    off[1] = o;
    if (qt == QT_Q8_0) o = al(o + (size_t)nblocks * 16);
    off[2] = o;
    if (qt == QT_Q5_0 || qt == QT_Q5_1) o = al(o + (size_t)nblocks * 4);
    off[3] = o;
    o = scale_plane_end(o, (size_t)nblocks * 2, nb & 1);
    off[4] = o;
    if (qt == QT_Q4_1 || qt == QT_Q5_1) o = scale_plane_end(o, (size_t)nblocks * 2, nb & 1);
    return o;
}

QWeight qw_at(char *base, int qt, int64_t M, int64_t nb) {
    size_t off[5];
    qw_layout(qt, M, nb, off);
    QWeight w;
    w.qs = (const uint8_t *)(base + off[0]);
    w.qs2 = (const uint8_t *)(base + off[1]);
    w.qh = (const uint32_t *)(base + off[2]);
    w.d = (const __half *)(base + off[3]);
    w.m = (const __half *)(base + off[4]);
    w.M = M;
    w.nb = nb;
    w.qt = qt;
    w.w16 = nullptr;
    return w;
}

void relayout_launch(const char *raw_dev, int qt, int64_t M, int64_t nb, char *soa_base) {
    QWeight w = qw_at(soa_base, qt, M, nb);
    const int64_t nblocks = M * nb;
    hipLaunchKernelGGL(k_relayout_q, grid1(nblocks), dim3(256), 0, g.stream, (const uint8_t *)raw_dev, qt, nblocks,
                       (uint8_t *)w.qs, (uint8_t *)w.qs2, (uint32_t *)w.qh, (__half *)w.d, (__half *)w.m);
    HIP_CHECK(hipGetLastError());
}

bool wants_soa(const ggml_tensor *t) {
    return qt_of(t->type) >= 0 && t->ne[2] == 1 && t->ne[3] == 1 && t->ne[0] % 32 == 0 && ggml_is_contiguous(t);
}

// K-quants (kernels/kquant.h, kquant2.h): planes {qs, aux (Q6_K high bits / Q3_K hmask / Q5_K qh), sc, d}; bytes per super-block
struct KPlanes { int qs, aux, sc, d; };
KPlanes k_planes(int kt) {
    switch (kt) {
        case KT_Q4_K: return {128, 0, 16, 4};
        case KT_Q6_K: return {128, 64, 16, 2};
        case KT_Q2_K: return {64, 0, 16, 4};
        case KT_Q3_K: return {64, 32, 16, 4};
        default: return {128, 32, 16, 4};  // KT_Q5_K
    }
}
double k_block_bytes(int kt) { return kt == KT_Q4_K ? 144.0 : kt == KT_Q6_K ? 210.0 : kt == KT_Q2_K ? 84.0 : kt == KT_Q3_K ? 110.0 : 176.0; }
size_t kw_layout(int kt, int64_t M, int64_t nsb, size_t off[4]) {
    const int64_t nsbt = M * nsb;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const KPlanes pl = k_planes(kt);
    size_t o = 0;
    off[0] = o;
    o = al(o + (size_t)nsbt * pl.qs);
    off[1] = o;
    if (pl.aux) o = al(o + (size_t)nsbt * pl.aux);
    off[2] = o;
    o = al(o + (size_t)nsbt * pl.sc);
    off[3] = o;
    o = scale_plane_end(o, (size_t)nsbt * pl.d, pl.d == 2 && (nsb & 1));  // (Q6_K: 2-byte scales read in pairs)
    return o;
}
// rows row0 .. of a planar K weight (every plane is row-major)
KWeight kw_rows(KWeight w, int64_t row0, int64_t rows) {
    const KPlanes pl = k_planes(w.kt);
    const int64_t s = row0 * w.nsb;
    w.qs += s * pl.qs;
    w.aux += s * pl.aux / 4;
    w.sc += s * pl.sc;
    w.d += s * pl.d / 2;
    w.M = rows;
    return w;
}
KWeight kw_at(char *base, int kt, int64_t M, int64_t nsb) {
    size_t off[4];
    kw_layout(kt, M, nsb, off);
    KWeight w;
    w.qs = (const uint8_t *)(base + off[0]);
    w.aux = (const uint32_t *)(base + off[1]);
    w.sc = (const uint8_t *)(base + off[2]);
    w.d = (const __half *)(base + off[3]);
    w.M = M;
    w.nsb = nsb;
    w.kt = kt;
    return w;
}
void relayout_k_launch(const char *raw_dev, int kt, int64_t M, int64_t nsb, char *base) {
    const KWeight w = kw_at(base, kt, M, nsb);
    if (kt == KT_Q4_K || kt == KT_Q6_K)
        hipLaunchKernelGGL(k_relayout_k, grid1(M * nsb * 8), dim3(256), 0, g.stream, (const uint8_t *)raw_dev, kt, M * nsb,
                           (uint8_t *)w.qs, (uint32_t *)w.aux, (uint8_t *)w.sc, (__half *)w.d);
    else
        hipLaunchKernelGGL(k_relayout_k2, grid1(M * nsb), dim3(256), 0, g.stream, (const uint8_t *)raw_dev, kt, M * nsb,
                           (uint8_t *)w.qs, (uint32_t *)w.aux, (uint8_t *)w.sc, (__half *)w.d);
    HIP_CHECK(hipGetLastError());
}
bool wants_ksoa(const ggml_tensor *t) {
    return kt_of(t->type) >= 0 && t->ne[2] == 1 && t->ne[3] == 1 && t->ne[0] % 256 == 0 && ggml_is_contiguous(t);
}

static const size_t SESSION_GUARD_BYTES = 4096;  // behind every zero-filled (session state) record, see below
// Uploads `nbytes` from host `data` as the device copy of `t`. Returns the record (registered in g.tensors).
DevTensor *upload_tensor(const void *data, const ggml_tensor *t, bool zero_fill, bool is_auto = false) {
    ensure_init();
    const size_t nbytes = ggml_nbytes(t);
    if (!is_auto && !zero_fill) {
        // The same host bytes offloaded again (two models over one mmap / one weight buffer): share the
        // device copy instead of evicting it from under the first owner.
        auto it = g.tensors.find((uintptr_t)data);
        if (it != g.tensors.end()) {
            DevTensor *o = it->second;
            if (o->nbytes == nbytes && o->type == t->type && o->ne[0] == t->ne[0] && o->ne[1] == t->ne[1] &&
                o->ne[2] == t->ne[2] && o->ne[3] == t->ne[3] && !o->zero_filled) {
                o->refs++;
                return o;
            }
        }
    }
    DevTensor *e = new DevTensor();
    e->zero_filled = zero_fill;
    if (zero_fill && g.session_records++ == 0) {  // this slot now drives a session on its device
        g_dev_slots[g.device & 63].fetch_add(1);
        g_dev_gen[g.device & 63].fetch_add(1);
    }
    e->host = (uintptr_t)data;
    e->nbytes = nbytes;
    e->type = t->type;
    for (int i = 0; i < 4; i++) e->ne[i] = t->ne[i];
    if (!zero_fill && wants_soa(t)) {
        const int qt = qt_of(t->type);
        const int64_t M = t->ne[1], nb = t->ne[0] / 32;
        size_t off[5];
        const size_t total = qw_layout(qt, M, nb, off);
        dev_malloc((void **)&e->dev, total, "a weight tensor");
        e->dev_bytes = total;
        char *tmp = nullptr;
        dev_malloc((void **)&tmp, nbytes, "an upload staging buffer");
        h2d_bulk(tmp, data, nbytes);
        relayout_launch(tmp, qt, M, nb, e->dev);
        HIP_CHECK(hipStreamSynchronize(g.stream));
        HIP_CHECK(hipFree(tmp));
        e->soa = true;
        e->qw = qw_at(e->dev, qt, M, nb);
    } else if (!zero_fill && wants_ksoa(t)) {
        const int kt = kt_of(t->type);
        const int64_t M = t->ne[1], nsb = t->ne[0] / 256;
        size_t off[4];
        const size_t total = kw_layout(kt, M, nsb, off);
        dev_malloc((void **)&e->dev, total, "a weight tensor");
        e->dev_bytes = total;
        char *tmp = nullptr;
        dev_malloc((void **)&tmp, nbytes, "an upload staging buffer");
        h2d_bulk(tmp, data, nbytes);
        relayout_k_launch(tmp, kt, M, nsb, e->dev);
        HIP_CHECK(hipStreamSynchronize(g.stream));
        HIP_CHECK(hipFree(tmp));
        e->ksoa = true;
        e->kw = kw_at(e->dev, kt, M, nsb);
    } else {
        // Session state (K/V memory, hand-off buffers) ends in a zeroed guard of its own.  A caller whose graph runs a little past
        // the context — the reference's perplexity loop never lowers n_past between chunks (INTEGRATION.md section 4), a test that feeds
        // 72 tokens into a context of 64 — gets views that end beyond the tensor (ggml does not check them); without the guard those
        // rows are whatever the allocator put next: another session's cache, which such a caller then reads and WRITES.  With several
        // sessions alive (and more of them per process since the batched step) what it computes must not depend on its neighbours.
        const size_t guard = zero_fill ? SESSION_GUARD_BYTES : 0;
        dev_malloc((void **)&e->dev, std::max<size_t>(nbytes, 16) + guard, "a persistent tensor");
        e->dev_bytes = nbytes;
        if (zero_fill)
            HIP_CHECK(hipMemsetAsync(e->dev, 0, std::max<size_t>(nbytes, 16) + guard, g.stream));
        else
            h2d_bulk(e->dev, data, nbytes);
        HIP_CHECK(hipStreamSynchronize(g.stream));
    }
    e->auto_uploaded = is_auto;
    // whoever held this host range before is gone (the memory was recycled)
    evict_overlapping(g.auto_tensors, e->host, std::max<size_t>(nbytes, 1));
    if (is_auto) {
        g.auto_tensors[e->host] = e;
    } else {
        evict_overlapping(g.tensors, e->host, std::max<size_t>(nbytes, 1));
        g.tensors[e->host] = e;
    }
    return e;
}

void drop_all_plans();
void destroy_record(DevTensor *e) {
    drop_all_plans();  // cached decode plans hold device addresses of weight / KV records
    if (g.stream) HIP_CHECK(hipStreamSynchronize(g.stream));
    if (e->dev) HIP_CHECK(hipFree(e->dev));
    if (e->w16) {
        HIP_CHECK(hipFree(e->w16));
        g.w16_bytes -= e->w16_size;
    }
    if (!e->zero_filled) g_dev_wgen[g.device & 63].fetch_add(1);  // sibling slots' plans may hold this record's addresses
    if (e->zero_filled && --g.session_records == 0) {
        g_dev_slots[g.device & 63].fetch_sub(1);
        g_dev_gen[g.device & 63].fetch_add(1);
    }
    e->magic = 0;
    delete e;
}
// Frees on the slot that OWNS the record, whichever slot is current (a context freed while another device is the main
// one): the owner's maps lose the record, the owner's plans (which hold its device addresses) are dropped, the owner's
// w16 accounting is adjusted — on the current slot all three would go to the wrong device and leave a dangling record.
void free_dev_tensor(DevTensor *e) {
    if (--e->refs > 0) return;
    Backend *keep = g_cur;
    if (e->slot >= 0 && e->slot < GGML_HIP_MAX_BACKENDS && &g_backends[e->slot] != g_cur) {
        g_cur = &g_backends[e->slot];
        if (g.inited) bind_device();
    }
    auto &m = e->auto_uploaded ? g.auto_tensors : g.tensors;
    auto it = m.find(e->host);
    if (it != m.end() && it->second == e) m.erase(it);
    destroy_record(e);
    if (g_cur != keep) {
        g_cur = keep;
        if (g.inited) bind_device();
    }
}

// the SoA view of a quantized mul_mat / get_rows operand; re-lays-out on the fly for raw arena tensors
QWeight qweight_of(const ggml_tensor *t) {
    DevTensor *e = extra_of(t);
    if (!e) e = find_tensor((uintptr_t)t->data);
    if (e && e->soa) {
        if ((uintptr_t)t->data != e->host || t->ne[0] != e->ne[0] || t->ne[1] != e->ne[1])
            die("tensor '%s': views of re-laid-out quantized weights are not supported", t->name);
        return e->qw;
    }
    if (!wants_soa(t)) die("tensor '%s': quantized operand must be a contiguous 2-D matrix with ne0 %% 32 == 0", t->name);
    // raw GGML blocks in an arena (e.g. a weight created in the compute context): convert into workspace
    const int qt = qt_of(t->type);
    const int64_t M = t->ne[1], nb = t->ne[0] / 32;
    size_t off[5];
    const size_t total = qw_layout(qt, M, nb, off);
    char *raw = dev_ptr(t);
    char *soa = ws_alloc(total);
    relayout_launch(raw, qt, M, nb, soa);
    return qw_at(soa, qt, M, nb);
}

KWeight kweight_of(const ggml_tensor *t) {
    DevTensor *e = extra_of(t);
    if (!e) e = find_tensor((uintptr_t)t->data);
    if (e && e->ksoa) {
        if ((uintptr_t)t->data != e->host || t->ne[0] != e->ne[0] || t->ne[1] != e->ne[1])
            die("tensor '%s': views of re-laid-out quantized weights are not supported", t->name);
        return e->kw;
    }
    if (!wants_ksoa(t)) die("tensor '%s': K-quant operand must be a contiguous 2-D matrix with ne0 %% 256 == 0", t->name);
    const int kt = kt_of(t->type);
    const int64_t M = t->ne[1], nsb = t->ne[0] / 256;
    size_t off[4];
    const size_t total = kw_layout(kt, M, nsb, off);
    char *soa = ws_alloc(total);
    relayout_k_launch(dev_ptr(t), kt, M, nsb, soa);
    return kw_at(soa, kt, M, nsb);
}
