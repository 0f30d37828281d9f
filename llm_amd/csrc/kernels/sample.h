// sample.h — k_batch_sample_next: the tail of a SAMPLED batched decode step (ggml_hip_decode_batch_sampled, plan_run.inc).  What
// k_batch_argmax_next (decode.h) is to the greedy chain, with the sampler of kernels/sampler_math.h in place of the first maximum:
// repetition penalty over the column's last 64 tokens, top-k, top-p, temperature, one xorshift64* draw.  The arithmetic is that
// header's, which the host mirror (llm_sample_exact) compiles too: the chain draws the ids the stepped loop draws.
#pragma once
#include "common.h"
#include "decode.h"
#include "sampler_math.h"
#include "topk.h"

// Per-column sampler state of a batched plan, uploaded once per call: the history ring of each column (min(hist_n, 64) entries hold;
// the next token goes to slot hist_n % 64) and the chain's four parameters.  The generator states travel beside the sampled ids.
struct SampleCols {
    int hist[BATCH_COLS_MAX][SAMPLER_WINDOW];
    int hist_n[BATCH_COLS_MAX];
    int k;
    float top_p, temperature, penalty;
};

// Grid = B workgroups of 1024 threads; workgroup c works on row c of logits [B][V] and on entry c of every table — nothing is handed
// between workgroups, and entries from B on are not touched.
//   selection   topk_kth_key (k_topk's radix passes) finds the k-th largest raw key; the window's tokens (each id once) enter with
//               their penalised values, the raw top-k without the window's tokens beside them: <= k + 64 keys, bitonic-sorted in LDS
//               by (value descending, id ascending) — topk_key's order;
//   q, p        one thread per candidate (f32: sampler_q / sampler_p);
//   serial tail thread 0: sampler_pick, then the next replay's parameters (DecParams::tokens[c], BatchCols::pos[c] + 1, workgroup 0
//               also token / n_past), out[c], the id into the column's ring, the advanced generator state.
// k is 1 .. min(SAMPLER_K_MAX, V) (the host declines anything else; the kernel writes nothing then).
__global__ void __launch_bounds__(1024) k_batch_sample_next(const float *__restrict__ logits, int V, DecParams *prm, BatchCols *bc,
                                                            SampleCols *sc, unsigned long long *rng, int *__restrict__ out) {
    constexpr int PMAX = 512;  // power of two >= SAMPLER_K_MAX + SAMPLER_WINDOW
    static_assert(PMAX >= SAMPLER_K_MAX + SAMPLER_WINDOW, "k_batch_sample_next: LDS keys");
    __shared__ unsigned long long s_keys[PMAX];
    __shared__ float s_v[SAMPLER_K_MAX], s_q[SAMPLER_K_MAX], s_p[SAMPLER_K_MAX];
    __shared__ int s_id[SAMPLER_K_MAX], s_h[SAMPLER_WINDOW], s_win[SAMPLER_WINDOW];
    __shared__ int s_cnt, s_wn;
    const int c = blockIdx.x, tid = threadIdx.x;
    const int k = sc->k;
    if (c >= BATCH_COLS_MAX || k < 1 || k > SAMPLER_K_MAX || k > V) return;
    const float *x = logits + (size_t)c * V;
    const float penalty = sc->penalty, temperature = sc->temperature;
    const int hn = sc->hist_n[c];
    const int nw = hn < SAMPLER_WINDOW ? (hn < 0 ? 0 : hn) : SAMPLER_WINDOW;
    int P = 1;
    while (P < k + nw) P <<= 1;
    for (int i = tid; i < P; i += 1024) s_keys[i] = 0;  // (below every key of a row without NaN)
    if (tid < SAMPLER_WINDOW) s_h[tid] = tid < nw ? sc->hist[c][tid] : -1;
    if (tid == 0) {
        s_cnt = 0;
        s_wn = 0;
    }
    __syncthreads();
    if (tid < nw) {  // the window's tokens, each id once, with their penalised values
        const int id = s_h[tid];
        bool take = id >= 0 && id < V;
        for (int j = 0; j < tid; j++) take = take && s_h[j] != id;
        if (take) {
            s_win[atomicAdd(&s_wn, 1)] = id;
            s_keys[atomicAdd(&s_cnt, 1)] = topk_key(sampler_penalise(x[id], penalty), id);
        }
    }
    const unsigned long long kth = topk_kth_key(x, V, k);  // (opens with a barrier: s_win / s_wn are complete behind it)
    const int wn = s_wn;
    for (int i = tid; i < V; i += 1024) {  // the raw top-k, without the window's tokens
        const unsigned long long key = topk_key(x[i], i);
        if (key >= kth) {
            bool in_window = false;
            for (int j = 0; j < wn; j++) in_window = in_window || s_win[j] == i;
            if (!in_window) s_keys[atomicAdd(&s_cnt, 1)] = key;
        }
    }
    __syncthreads();
    topk_bitonic_desc(s_keys, P);
    if (tid < k) {  // at least k keys went in
        const unsigned long long key = s_keys[tid];
        const uint32_t o = (uint32_t)(key >> 32);
        const uint32_t u = (o & 0x80000000u) ? (o ^ 0x80000000u) : ~o;
        s_v[tid] = __builtin_bit_cast(float, u);
        s_id[tid] = (int)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull));
    }
    __syncthreads();
    if (tid < k) {
        const float v0 = s_v[0];
        s_q[tid] = sampler_q(s_v[tid], v0);
        s_p[tid] = sampler_p(s_v[tid], v0, temperature);
    }
    __syncthreads();
    if (tid == 0) {
        uint64_t state = rng[c];
        const int id = s_id[sampler_pick(s_q, s_p, k, sc->top_p, &state)];
        rng[c] = state;
        const int pos = bc->pos[c] + 1;
        prm->tokens[c] = id;
        bc->pos[c] = pos;
        out[c] = id;
        if (c == 0) {
            prm->token = id;
            prm->n_past = pos;
        }
        sc->hist[c][(unsigned)hn % SAMPLER_WINDOW] = id;
        sc->hist_n[c] = hn + 1;
    }
}
