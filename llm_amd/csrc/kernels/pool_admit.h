// pool_admit.h — the request pool of ggml_hip_decode_pool_requests: more requests than columns.  k_pool_admit runs behind the tail
// kernels of every step of a pool call (kernels/sample.h, the REQ kernels): a column whose request has ended and whose last token has
// been evaluated (kernels/pool_rule.h) hands its request's results to that request's own slot and takes the next waiting request —
// token, position, caches, ring, sampler, end rule, generator — out of the tables the call staged once.  Every kernel of the batched
// step reads a column's token, position and caches from device memory and the tail kernels find their columns through the lists of
// the call's SampleReqs, so the SAME captured graph goes on with another session in that column: no host round trip, no recapture.
//
// The tables (PoolTable) lie in a buffer of their own.  The structures are compiled by the backend's host code too; the kernel is
// compiled into pool_admit.hip's code object alone (POOL_ADMIT_OBJECT), so the other code objects hold what they held.
#pragma once
#include "pool_rule.h"
#include "sample.h"

static_assert(POOL_COLS_MAX == BATCH_COLS_MAX, "pool_rule.h: the columns of a batched step");

struct PoolIn {  // what a column gets with request r: staged once per call, read-only on the device
    __half *mem_k, *mem_v;
    unsigned long long rng;
    float mu;
    int token, pos;  // its first token (drawn by the host) and the position that token is evaluated at
    int hist_n, max_draws, n_stop, cls;
    int stop_id[CHAIN_STOP_MAX];
    int hist[SAMPLER_WINDOW];
    SampleReqParams prm;
    SampleBias bias;
};
struct PoolOut {  // what comes back of request r
    unsigned long long rng;
    float mu;
    int n_drawn, ended_by;
    int col, first_step;  // -1, 0: it never left the queue
    int retired;          // 1: its logits and embedding rows are in its slot; 0 with col >= 0: still in its column
    int pad;
};
struct PoolHead {
    int cursor, n_pool, n_cols, step;  // the next waiting request; step: admissions so far = the step the last tail belongs to
    int busy;                          // behind an admission: a column is live or a request waits (the host's "done" test reads this)
    int pad;
    int owner[BATCH_COLS_MAX];         // the request in column c
    int was_live[BATCH_COLS_MAX];      // pool_rule.h
};
struct PoolTable {
    PoolHead head;  // first: what the host reads back behind a group of steps
    PoolOut out[POOL_REQUESTS_MAX];
    PoolIn in[POOL_REQUESTS_MAX];
};

#ifndef POOL_ADMIT_OBJECT
// pool_admit.hip; the tables as void *: their types are distinct types in the two objects (same definitions)
void launch_pool_admit(hipStream_t stream, void *table, void *reqs, void *sc, void *prm, void *bc, const float *logits, const float *emb, int V,
                       int E, float *slot_logits, float *slot_emb);
#else
// ONE workgroup of 1024 threads decides and does everything: two columns can become free behind one step, and with a single
// workgroup no word one column's admission writes (cursor, lists, live flags) is read by another workgroup of the launch.  Thread 0
// applies the rule to words only this launch writes; the assignment goes through LDS; every thread then moves the retiring requests'
// rows (logits [n_cols][V], emb [n_cols][E] -> slot_logits [n_pool][V], slot_emb [n_pool][E]); thread 0 writes the tables last.
// A launch that admits nothing — nearly every launch — reads 2 x n_cols flags, writes was_live, step and busy, and is done.
// Every index read from memory is clamped or checked before it addresses anything.
__global__ void __launch_bounds__(1024) k_pool_admit(PoolTable *pt, SampleReqs *rq, SampleCols *sc, DecParams *prm, BatchCols *bc,
                                                     const float *__restrict__ logits, const float *__restrict__ emb, int V, int E,
                                                     float *__restrict__ slot_logits, float *__restrict__ slot_emb) {
    __shared__ int s_take[BATCH_COLS_MAX], s_old[BATCH_COLS_MAX], s_ncols;
    if (blockIdx.x != 0) return;
    const int tid = threadIdx.x;
    if (tid == 0) {
        int n_cols = pt->head.n_cols, n_pool = pt->head.n_pool, cursor = pt->head.cursor;
        n_cols = n_cols < 0 ? 0 : (n_cols > BATCH_COLS_MAX ? BATCH_COLS_MAX : n_cols);
        n_pool = n_pool < 0 ? 0 : (n_pool > POOL_REQUESTS_MAX ? POOL_REQUESTS_MAX : n_pool);
        cursor = cursor < 0 ? n_pool : cursor;
        int live[BATCH_COLS_MAX], was[BATCH_COLS_MAX];
        for (int c = 0; c < BATCH_COLS_MAX; c++) {
            live[c] = c < n_cols ? rq->back.live[c] : 0;
            was[c] = c < n_cols ? pt->head.was_live[c] : 0;
            s_take[c] = -1;
        }
        pool_assign(live, was, n_cols, cursor, n_pool, s_take);
        for (int c = 0; c < BATCH_COLS_MAX; c++) {
            const int o = pt->head.owner[c];
            s_old[c] = (c < n_cols && o >= 0 && o < n_pool) ? o : -1;
        }
        s_ncols = n_cols;
    }
    __syncthreads();
    const int n_cols = s_ncols;
    bool any = false;
    for (int c = 0; c < n_cols; c++) {  // the retiring requests' rows: the ones their own last evaluation wrote
        if (s_take[c] < 0) continue;
        any = true;
        const int o = s_old[c];
        if (o < 0) continue;
        const float *ls = logits + (size_t)c * V, *es = emb + (size_t)c * E;
        float *ld = slot_logits + (size_t)o * V, *ed = slot_emb + (size_t)o * E;
        for (int i = tid; i < V; i += 1024) ld[i] = ls[i];
        for (int i = tid; i < E; i += 1024) ed[i] = es[i];
    }
    if (any) {  // the admitted requests' rings
        for (int c = 0; c < n_cols; c++) {
            const int r = s_take[c];
            if (r < 0) continue;
            if (tid < SAMPLER_WINDOW) sc->hist[c][tid] = pt->in[r].hist[tid];
            if (tid < SAMPLER_BIAS_MAX) {
                rq->bias[c].id[tid] = pt->in[r].bias.id[tid];
                rq->bias[c].b[tid] = pt->in[r].bias.b[tid];
            }
        }
    }
    if (tid != 0) return;
    int cursor = pt->head.cursor;
    for (int c = 0; c < n_cols; c++) {
        const int r = s_take[c];
        if (r >= 0) {
            const int o = s_old[c];
            if (o >= 0) {  // retire
                PoolOut &b = pt->out[o];
                b.rng = rq->back.state.rng[c];
                b.mu = rq->back.state.mu[c];
                b.n_drawn = rq->back.n_drawn[c];
                b.ended_by = rq->back.ended_by[c];
                b.retired = 1;
            }
            const PoolIn &in = pt->in[r];  // admit
            prm->tokens[c] = in.token;
            bc->pos[c] = in.pos;
            bc->mem_k[c] = in.mem_k;
            bc->mem_v[c] = in.mem_v;
            if (c == 0) {  // (as write_next_token keeps them)
                prm->token = in.token;
                prm->n_past = in.pos;
            }
            sc->hist_n[c] = in.hist_n;
            rq->prm[c] = in.prm;
            rq->n_stop[c] = in.n_stop;
            for (int j = 0; j < CHAIN_STOP_MAX; j++) rq->stop_id[c][j] = in.stop_id[j];
            rq->max_draws[c] = in.max_draws;
            rq->back.state.rng[c] = in.rng;
            rq->back.state.mu[c] = in.mu;
            rq->back.n_drawn[c] = 0;
            rq->back.live[c] = in.max_draws > 0;
            rq->back.ended_by[c] = in.max_draws > 0 ? CHAIN_END_NONE : CHAIN_END_BUDGET;
            pt->head.owner[c] = r;
            pt->out[r].col = c;
            pt->out[r].first_step = pt->head.step + 1;
            if (r + 1 > cursor) cursor = r + 1;
        }
    }
    if (any) {  // the lists of all four classes: an admitted request may be of a class no column had
        int n[SAMPLE_CLASSES] = {0, 0, 0, 0};
        for (int c = 0; c < n_cols; c++) {
            const int o = pt->head.owner[c];
            if (o < 0 || o >= POOL_REQUESTS_MAX) continue;
            const int cls = pt->in[o].cls;
            if (cls < 0 || cls >= SAMPLE_CLASSES) continue;
            rq->list[cls][n[cls]++] = c;
        }
        for (int s = 0; s < SAMPLE_CLASSES; s++) rq->n_list[s] = n[s];
    }
    bool busy = cursor < pt->head.n_pool;
    for (int c = 0; c < n_cols; c++) {
        const int l = rq->back.live[c];
        pt->head.was_live[c] = l;
        busy = busy || l;
    }
    pt->head.cursor = cursor;
    pt->head.step = pt->head.step + 1;
    pt->head.busy = busy;
}
#endif
