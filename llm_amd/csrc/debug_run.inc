// debug_run.inc — part of libggml_hip.so's backend translation unit (included by hip_backend.hip, inside its anonymous
// namespace where noted): the scaffold of a test hook's run (DebugRun) and the fixtures several ggml_hip_debug_* hooks share.  At file scope.
namespace {
constexpr size_t DEBUG_GUARD = 256;
// One run of a test hook.  Constructed once the hook has vetted what it can vet without a device: takes the slot, brings the device
// up and idle.  Owns every device buffer and pinned host slot the run makes and frees them on every path out of the hook.  A new
// test hook is a DebugRun plus its launch.
struct DebugRun {
    SlotLock lk;
    std::vector<char *> owned, pinned;
    DebugRun() {
        ensure_init();
        finish_pending();
    }
    ~DebugRun() {
        for (char *b : owned) HIP_CHECK(hipFree(b));
        for (char *p : pinned) HIP_CHECK(hipHostFree(p));
    }
    // n bytes on the device without a guard (inputs, scratch, the oldest hooks' outputs): `init`'s bytes, or as they come
    char *raw(size_t n, const void *init = nullptr) {
        char *d;
        dev_malloc((void **)&d, n, "a debug buffer");
        owned.push_back(d);
        if (init) h2d_bulk(d, init, n);
        return d;
    }
    // n bytes + the guard on the device: `init`'s n bytes (nullptr: 0xFF) followed by 0xFF
    char *buf(size_t n, const void *init = nullptr) {
        char *d = raw(n + DEBUG_GUARD, nullptr);
        if (init) {
            h2d_bulk(d, init, n);
            HIP_CHECK(hipMemsetAsync(d + n, 0xFF, DEBUG_GUARD, g.stream));
        } else {
            HIP_CHECK(hipMemsetAsync(d, 0xFF, n + DEBUG_GUARD, g.stream));
        }
        return d;
    }
    template <class T>
    T *put(const T &v) {  // a struct's round trip: buf() of its bytes, back(&v, d) after the launch
        return (T *)buf(sizeof(T), &v);
    }
    char *host_slot(size_t n) {  // n pinned host bytes of 0xFF, as a token's result slot
        char *s = nullptr;
        HIP_CHECK(hipHostMalloc((void **)&s, n, hipHostMallocDefault));
        pinned.push_back(s);
        memset(s, 0xff, n);
        return s;
    }
    void back(void *host, const void *dev, size_t n) { d2h_queue(host, (const char *)dev, n); }
    template <class T>
    void back(T *host, const T *dev) {
        back(host, dev, sizeof(T));
    }
    int finish() {  // the launches took, the queued read-backs are in the caller's memory: the hook's 0
        HIP_CHECK(hipGetLastError());
        d2h_finish();
        return 0;
    }
};
void debug_hot_line() {
    if (!g.hot_line) {  // as plan building makes it
        dev_malloc(&g.hot_line, 256, "the dummy ring steps' line");
        HIP_CHECK(hipMemsetAsync(g.hot_line, 0, 256, g.stream));
    }
}

// ---- the QKV fixture of the mat-vec hooks (debug_matvec.inc): ncols tokens at positions n_past .., as a plan stages them ----
// The token's DecParams (n_past; store_at 0 = n_past), the RoPE table of its ncols columns made by k_rope_table as the plans make it
// (128 floats a column; a head of more than 128 elements runs on into the next 128, so one column more is allocated), and the
// caller's K / V caches of width Egqa with guards.
struct DebugQkv {
    DecParams *prm = nullptr;
    float *rope = nullptr, theta_scale = 0.0f;
    char *dk = nullptr, *dv = nullptr;
    size_t nkv = 0;
    uint16_t *mem_k = nullptr, *mem_v = nullptr;  // the caller's, in-out
};
// head size D, matrices of M0 (wq), M1 (wk), M2 (wv) rows, columns n_past .. n_past + ncols - 1 inside a cache of C positions
bool debug_qkv_ok(const uint16_t *mem_k, const uint16_t *mem_v, int D, int64_t M0, int64_t M1, int64_t M2, int n_past, int ncols, int64_t C) {
    return mem_k && mem_v && D >= 2 && D % 2 == 0 && D <= 256 && M0 % D == 0 && M1 % D == 0 && M1 == M2 && n_past >= 0 &&
           (int64_t)n_past + ncols <= C;
}
DebugQkv debug_qkv(DebugRun &run, int n_past, int ncols, int D, float freq_base, float freq_scale, int64_t C, int64_t Egqa, uint16_t *mem_k,
                   uint16_t *mem_v) {
    DebugQkv q;
    DecParams hp;
    memset(&hp, 0, sizeof(hp));
    hp.n_past = n_past;
    q.prm = run.put(hp);
    q.rope = (float *)run.buf((size_t)(ncols + 1) * 128 * 4);
    q.theta_scale = powf(freq_base, -2.0f / (float)D);  // n_dims = the head size, as in LlamaMatch
    hipLaunchKernelGGL(k_rope_table, dim3((unsigned)ncols), dim3(128), 0, g.stream, (const DecParams *)q.prm, q.theta_scale, freq_scale, D >> 1,
                       q.rope, (unsigned *)nullptr);
    HIP_CHECK(hipGetLastError());
    q.nkv = (size_t)C * Egqa * 2;
    q.dk = run.buf(q.nkv, mem_k);
    q.dv = run.buf(q.nkv, mem_v);
    q.mem_k = mem_k;
    q.mem_v = mem_v;
    return q;
}
// what a mat-vec hook hands back, guards included: out (n_out bytes), the normed row(s) y_out (n_y bytes) where dy was made, the caches
// of a QKV launch
int debug_matvec_finish(DebugRun &run, float *out, const char *dout, size_t n_out, float *y_out, const char *dy, size_t n_y, const DebugQkv &q) {
    run.back(out, dout, n_out + DEBUG_GUARD);
    if (dy) run.back(y_out, dy, n_y + DEBUG_GUARD);
    if (q.dk) {
        run.back(q.mem_k, q.dk, q.nkv + DEBUG_GUARD);
        run.back(q.mem_v, q.dv, q.nkv + DEBUG_GUARD);
    }
    return run.finish();
}

// ---- the state of the next-token hooks (debug_token.inc): what sits between two steps of a chain, staged from and unpacked into the
// caller's arrays.  tokens_in[32] as DecParams::tokens (token = tokens_in[0]) at n_past, pos_in[8] as a step's BatchCols::pos (null: no
// BatchCols, one session), the rings and counts of T entries (hist null: none), ids of n_draws launches on B rows. ----
struct DebugToken {
    const bool cols;  // with a BatchCols
    const int T;      // entries of the rings, counts and generator states: 8 with a BatchCols, 1 without
    DecParams hp;
    BatchCols hb;
    SampleCols hs;
    const float *dl = nullptr;
    DecParams *dp = nullptr;
    BatchCols *db = nullptr;
    SampleCols *ds = nullptr;
    int *dids = nullptr;
    size_t n_ids = 0;
    DebugToken(int n_past, const int32_t *pos_in, const int32_t *tokens_in, const int32_t *hist, const int32_t *hist_n)
        : cols(pos_in != nullptr), T(cols ? BATCH_COLS_MAX : 1) {
        memset(&hp, 0, sizeof(hp));
        memset(&hb, 0, sizeof(hb));
        memset(&hs, 0, sizeof(hs));
        for (int i = 0; i < 32; i++) hp.tokens[i] = tokens_in[i];
        hp.n_past = n_past;
        hp.token = tokens_in[0];
        for (int i = 0; cols && i < BATCH_COLS_MAX; i++) hb.pos[i] = pos_in[i];
        if (hist) {
            memcpy(hs.hist, hist, (size_t)T * SAMPLER_WINDOW * 4);
            memcpy(hs.hist_n, hist_n, (size_t)T * 4);
        }
    }
    // generator states and mu of the T entries into / out of a table's SampleState (entries from B on make the round trip untouched)
    void state_in(SampleState &st, const uint64_t *rng, const float *mu) const {
        for (int i = 0; i < T; i++) {
            st.rng[i] = rng[i];
            if (mu) st.mu[i] = mu[i];
        }
    }
    void state_out(const SampleState &st, uint64_t *rng, float *mu) const {
        for (int i = 0; i < T; i++) {
            rng[i] = st.rng[i];
            if (mu) mu[i] = st.mu[i];
        }
    }
    void upload(DebugRun &run, const float *logits, int B, int V, int n_draws) {
        dl = (const float *)run.buf((size_t)B * V * 4, logits);
        dp = run.put(hp);
        db = cols ? run.put(hb) : nullptr;
        ds = run.put(hs);
        n_ids = (size_t)n_draws * B * 4;
        dids = (int *)run.buf(n_ids);
    }
    // reads everything back (with what the hook queued itself) and unpacks it: prm_out[34] = n_past, token, tokens[0..32)
    void finish(DebugRun &run, int32_t *ids_out, int32_t *prm_out, int32_t *pos_out, int32_t *hist, int32_t *hist_n) {
        run.back(ids_out, dids, n_ids);
        run.back(&hp, dp);
        if (db) run.back(&hb, db);
        if (hist) run.back(&hs, ds);
        run.finish();
        prm_out[0] = hp.n_past;
        prm_out[1] = hp.token;
        for (int i = 0; i < 32; i++) prm_out[2 + i] = hp.tokens[i];
        for (int i = 0; cols && i < BATCH_COLS_MAX; i++) pos_out[i] = hb.pos[i];
        if (hist) {
            memcpy(hist, hs.hist, (size_t)T * SAMPLER_WINDOW * 4);
            memcpy(hist_n, hs.hist_n, (size_t)T * 4);
        }
    }
};
}  // namespace
