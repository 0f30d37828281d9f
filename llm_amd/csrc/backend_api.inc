// backend_api.inc — part of libggml_hip.so's backend translation unit (included by hip_backend.hip, inside its anonymous
// namespace where noted): the decode and prompt entry points serving code calls — chains, batched steps, request chains, the request pool, the packed prompt batch.  At file scope.
namespace {
// n graphs of a batched entry, lo <= n <= hi, none of them null, for n_steps steps (before any device is touched)
bool graphs_ok(struct ggml_cgraph *const *graphs, int n, int lo, int hi, int n_steps = 1) {
    if (!graphs || n < lo || n > hi || n_steps < 1 || n_steps > BATCH_CHAIN_MAX_STEPS) return false;
    for (int i = 0; i < n; i++)
        if (!graphs[i]) return false;
    return true;
}
// a request's end: a budget of 1 .. n_steps tokens, 0 .. CHAIN_STOP_MAX stop ids
bool chain_end_ok(const ggml_hip_chain_end &e, int n_steps) {
    return e.budget >= 1 && e.budget <= n_steps && e.n_stop >= 0 && e.n_stop <= CHAIN_STOP_MAX;
}
// a request per graph: its end, and what its sampler needs where it has one
bool requests_ok(int n, int n_steps, const ggml_hip_sampler_chain *const *chains, const ggml_hip_chain_end *ends, const int32_t *windows,
                 const int32_t *window_n, const uint64_t *rng) {
    if (!chains || !ends) return false;
    for (int i = 0; i < n; i++)
        if ((chains[i] && (!windows || !window_n || !rng)) || !chain_end_ok(ends[i], n_steps)) return false;
    return true;
}
// the entries whose whole run counts as compute time (statistic ns_compute); the chains of one session count theirs further in
template <class F>
int timed_compute(F &&run) {
    const uint64_t t0 = now_ns();
    const int r = run();
    g.ns_compute += now_ns() - t0;
    return r;
}
// The generator states and Mirostat mu of n requests on copies: a run works on them, and commit() hands those of the requests that
// sample back to the caller — after a run that succeeded; nothing of the caller's moves otherwise.
struct StateCopies {
    std::vector<uint64_t> r;
    std::vector<float> u;
    StateCopies(int n, const uint64_t *rng, const float *mu) : r((size_t)n, 0), u((size_t)n, 0.0f) {
        for (int i = 0; i < n; i++) {
            if (rng) r[(size_t)i] = rng[i];
            if (mu) u[(size_t)i] = mu[i];
        }
    }
    void commit(const ggml_hip_sampler_chain *const *chains, uint64_t *rng, float *mu) const {
        for (size_t i = 0; i < r.size(); i++) {
            if (rng && chains[i]) rng[i] = r[i];
            if (mu && chains[i]) mu[i] = u[i];
        }
    }
};
}  // namespace
extern "C" {
int ggml_hip_decode_greedy_chain(struct ggml_cgraph *last, int n, int32_t *out_tokens, float *last_logits) {
    SlotLock lk;
    return decode_greedy_chain(last, n, out_tokens, last_logits);
}

int ggml_hip_decode_batch(struct ggml_cgraph *const *graphs, int n_graphs) {
    if (!graphs_ok(graphs, n_graphs, 2, BATCH_COLS_MAX)) return -1;
    SlotLock lk;
    return timed_compute([&] { return decode_batch(graphs, n_graphs); });
}

int ggml_hip_decode_batch_greedy(struct ggml_cgraph *const *graphs, int n_graphs, int n_steps, int32_t *out_ids) {
    if (!graphs_ok(graphs, n_graphs, 2, BATCH_COLS_MAX, n_steps) || (n_steps > 1 && !out_ids)) return -1;
    SlotLock lk;
    return timed_compute([&] { return decode_batch_steps(graphs, n_graphs, n_steps, out_ids, true); });
}

int ggml_hip_decode_batch_sampled_ex(struct ggml_cgraph *const *graphs, int n_graphs, int n_steps, const ggml_hip_sampler_chain *chain,
                                     const int32_t *windows, const int32_t *window_n, uint64_t *rng, float *mu, int32_t *out_ids) {
    if (!graphs_ok(graphs, n_graphs, 2, BATCH_COLS_MAX, n_steps)) return -1;
    if (!chain || !windows || !window_n || !rng || (n_steps > 1 && !out_ids)) return -1;
    SlotLock lk;
    return timed_compute([&] {
        const BatchSample smp = {chain, windows, window_n, rng, mu};
        return decode_batch_steps(graphs, n_graphs, n_steps, out_ids, true, &smp);
    });
}
int ggml_hip_decode_batch_sampled(struct ggml_cgraph *const *graphs, int n_graphs, int n_steps, const ggml_hip_sampler *params,
                                  const int32_t *windows, const int32_t *window_n, uint64_t *rng, int32_t *out_ids) {
    if (!params) return -1;
    const ggml_hip_sampler_chain chain = sample_neutral(params);
    return ggml_hip_decode_batch_sampled_ex(graphs, n_graphs, n_steps, &chain, windows, window_n, rng, nullptr, out_ids);
}

int ggml_hip_decode_sampled_chain_ex(struct ggml_cgraph *last, int n, const ggml_hip_sampler_chain *chain, const int32_t *window, int window_n,
                                     uint64_t *rng, float *mu, int32_t *out_tokens, float *last_logits) {
    if (!last || n < 1 || !chain || !rng || !out_tokens || window_n < 0 || window_n > SAMPLER_WINDOW || (window_n > 0 && !window))
        return -1;  // (before any device is touched)
    SlotLock lk;
    const BatchSample smp = {chain, window, &window_n, rng, mu};
    return decode_chain(last, n, out_tokens, last_logits, &smp);
}
int ggml_hip_decode_sampled_chain(struct ggml_cgraph *last, int n, const ggml_hip_sampler *params, const int32_t *window, int window_n,
                                  uint64_t *rng, int32_t *out_tokens, float *last_logits) {
    if (!params) return -1;
    const ggml_hip_sampler_chain chain = sample_neutral(params);
    return ggml_hip_decode_sampled_chain_ex(last, n, &chain, window, window_n, rng, nullptr, out_tokens, last_logits);
}

// ---- the chains that stop: a request per column (plan_run.inc ChainRequests) ----
int ggml_hip_decode_chain_requests(struct ggml_cgraph *last, int n, const ggml_hip_sampler_chain *chain, const ggml_hip_chain_end *end,
                                   const int32_t *window, int window_n, uint64_t *rng, float *mu, int32_t *out_tokens, int32_t *n_drawn,
                                   int32_t *ended_by, float *last_logits) {
    if (!last || n < 1 || n > BATCH_CHAIN_MAX_STEPS || !end || !out_tokens || !n_drawn || !ended_by) return -1;  // (before any device is touched)
    if (window_n < 0 || window_n > SAMPLER_WINDOW || (window_n > 0 && !window) || (chain && !rng)) return -1;
    if (!chain_end_ok(*end, n)) return -1;
    SlotLock lk;
    const int32_t none[1] = {0};
    uint64_t r = rng ? *rng : 0;  // (copies: nothing moves unless the chain ran)
    float u = mu ? *mu : 0.0f;
    int32_t count = 0, why = 0;
    ChainRequests req = {&chain, end, window ? window : none, &window_n, &r, mu ? &u : nullptr, &count, &why, 0, {0, 0, 0, 0}};
    std::vector<int32_t> ids((size_t)end->budget);
    if (decode_chain(last, end->budget, ids.data(), last_logits, nullptr, &req) != 0) return -1;
    for (int i = 0; i < n; i++) out_tokens[i] = i < end->budget ? ids[(size_t)i] : -1;
    if (rng) *rng = r;
    if (mu) *mu = u;
    *n_drawn = count;
    *ended_by = why;
    return 0;
}
int ggml_hip_decode_batch_requests(struct ggml_cgraph *const *graphs, int n_graphs, int n_steps, const ggml_hip_sampler_chain *const *chains,
                                   const ggml_hip_chain_end *ends, const int32_t *windows, const int32_t *window_n, uint64_t *rng, float *mu,
                                   int32_t *out_ids, int32_t *n_evaluated, int32_t *ended_by) {
    if (!graphs_ok(graphs, n_graphs, 2, BATCH_COLS_MAX, n_steps)) return -1;
    if (!n_evaluated || !ended_by || (n_steps > 1 && !out_ids)) return -1;
    if (!requests_ok(n_graphs, n_steps, chains, ends, windows, window_n, rng)) return -1;
    SlotLock lk;
    StateCopies st(n_graphs, rng, mu);
    std::vector<int32_t> count((size_t)n_graphs), why((size_t)n_graphs);
    const int rc = timed_compute([&] {
        ChainRequests req = {chains, ends, windows, window_n, st.r.data(), mu ? st.u.data() : nullptr, count.data(), why.data(), 1, {0, 0, 0, 0}};
        return decode_batch_steps(graphs, n_graphs, n_steps, out_ids, true, nullptr, &req);
    });
    if (rc != 0) return -1;
    st.commit(chains, rng, mu);
    for (int i = 0; i < n_graphs; i++) {
        n_evaluated[i] = count[(size_t)i];
        ended_by[i] = why[(size_t)i];
    }
    return 0;
}

// ---- the request pool: more requests than columns (plan_pool.inc) ----
int ggml_hip_decode_pool_requests(struct ggml_cgraph *const *graphs, int n_pool, int n_cols, int n_steps, const ggml_hip_sampler_chain *const *chains,
                                  const ggml_hip_chain_end *ends, const int32_t *windows, const int32_t *window_n, uint64_t *rng, float *mu,
                                  int32_t *out_ids, int32_t *col, int32_t *first_step, int32_t *n_evaluated, int32_t *ended_by, int32_t *steps_run) {
    if (n_cols < 2 || n_cols > BATCH_COLS_MAX || !graphs_ok(graphs, n_pool, n_cols, POOL_REQUESTS_MAX, n_steps)) return -1;
    if (!col || !first_step || !n_evaluated || !ended_by || !steps_run || (n_steps > 1 && !out_ids)) return -1;
    if (!requests_ok(n_pool, n_steps, chains, ends, windows, window_n, rng)) return -1;
    SlotLock lk;
    StateCopies st(n_pool, rng, mu);
    std::vector<int32_t> c((size_t)n_pool), f((size_t)n_pool), count((size_t)n_pool), why((size_t)n_pool);
    int32_t steps = 0;
    const int rc = timed_compute([&] {
        ChainRequests req = {chains, ends, windows, window_n, st.r.data(), mu ? st.u.data() : nullptr, count.data(), why.data(), 1, {0, 0, 0, 0}};
        const PoolResults res = {c.data(), f.data(), count.data(), why.data(), &steps};
        return decode_pool_requests(graphs, n_pool, n_cols, n_steps, out_ids, req, res);
    });
    if (rc != 0) return -1;
    st.commit(chains, rng, mu);
    for (int i = 0; i < n_pool; i++) {
        col[i] = c[(size_t)i];
        first_step[i] = f[(size_t)i];
        n_evaluated[i] = count[(size_t)i];
        ended_by[i] = why[(size_t)i];
    }
    *steps_run = steps;
    return 0;
}

// ---- the packed prompt batch: the prompt rows of several sessions as one pass of the prompt plan (plan_pack.inc) ----
int ggml_hip_prompt_pack(struct ggml_cgraph *const *graphs, int n_graphs) {
    if (!graphs_ok(graphs, n_graphs, 1, PACK_SEGS_MAX)) return -1;
    SlotLock lk;
    return timed_compute([&] { return prompt_pack(graphs, n_graphs); });
}

}  // extern "C"
