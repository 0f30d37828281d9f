// sample.h — the device sampler of the sampled chains, 1 .. 8 sessions: k_sample_next, the kernel between two steps of
// ggml_hip_decode_sampled_chain (one session) and of ggml_hip_decode_batch_sampled (2 .. 8 sessions; plan_run.inc).  What k_argmax_next
// (decode.h) is to the greedy chains, with the sampler of kernels/sampler_math.h in place of the first maximum: repetition penalty
// over the column's last 64 tokens, top-k, top-p, temperature, one xorshift64* draw — and, as instantiations of their own, the rest of
// the reference's chain: flat bias, frequency / presence penalty, tail-free, locally typical, min-p, or Mirostat 2.  The arithmetic is
// that header's, which the host mirror (llm_sample_chain) compiles too: the chain draws the ids the stepped loop draws.
#pragma once
#include "common.h"
#include "decode.h"
#include "sampler_math.h"
#include "topk.h"

// Per-column sampler state of a plan (one session: column 0), uploaded once per call: the history ring of each column (min(hist_n, 64)
// entries hold; the next token goes to slot hist_n % 64), the chain's four parameters and the extras of the whole sampler
// (ggml_hip_sampler_chain; the default instantiations read none of them).  What comes back per column — SampleState: the generator
// states, then Mirostat's mu — travels in front of the sampled ids, and the bias table (SampleBias) lies in front of that, where the
// read-back does not reach: SampleCols keeps the 2304 bytes it has always had in a plan's pool, so that no buffer of a plan moves.
struct SampleCols {
    int hist[BATCH_COLS_MAX][SAMPLER_WINDOW];
    int hist_n[BATCH_COLS_MAX];
    int k;
    float top_p, temperature, penalty;
    float freq, presence, tail_free_z, typical_p, min_p;
    int mirostat;
    float tau, eta;
    int n_bias;
};
static_assert(sizeof(SampleCols) <= 2304, "SampleCols: its slot in the plan's pool");
struct SampleState {
    unsigned long long rng[BATCH_COLS_MAX];
    float mu[BATCH_COLS_MAX];
};
struct SampleBias {
    int id[SAMPLER_BIAS_MAX];
    float b[SAMPLER_BIAS_MAX];
};
// what heads a sampled chain's chain_out; k_sample_next's `rng` argument points at `state` (the default instantiations know no more)
struct SampleHead {
    SampleBias bias;
    SampleState state;
};
static_assert(sizeof(SampleHead) == sizeof(SampleBias) + sizeof(SampleState), "SampleHead: the bias table ends where the state begins");
// which stages an instantiation of k_sample_next carries: the default chain (the four parameters: today's kernel, registers and all),
// the whole truncating chain (specification A - D), Mirostat 2 (A, E; on chip only)
enum { SAMPLE_DEFAULT = 0, SAMPLE_FULL = 1, SAMPLE_MIROSTAT = 2 };
template <class Params>
__device__ __forceinline__ int sample_n_bias(const Params *sc) {  // (0 .. 64 whatever the table says)
    const int n = sc->n_bias;
    return n < 0 ? 0 : (n > SAMPLER_BIAS_MAX ? SAMPLER_BIAS_MAX : n);
}

// ---- chains that stop (ggml_hip_decode_chain_requests / ggml_hip_decode_batch_requests): every column carries its own request — its own
// sampler or the first maximum, its own stop ids, its own budget of draws.  SampleCols keeps the rings and nothing else of such a chain;
// the parameters it holds once are here per column, beside a bias table per column, and the table lies in a buffer of its own
// (DecodePlan::chain_req, allocated on first use).  What comes back with the ids is the head of the table, SampleReqBack: the generator
// states and Mirostat states where k_sample_next looks for them (its `rng` argument points at the table), the draws each column
// made, why it ended, and whether it is still live.  A column's entries are written by that column's own workgroup alone.
constexpr int CHAIN_STOP_MAX = 8;
enum { CHAIN_END_NONE = 0, CHAIN_END_BUDGET = 1, CHAIN_END_STOP = 2, CHAIN_END_CONTEXT = 3 };  // (the last: the host loop's alone)
enum { SAMPLE_GREEDY = 3, SAMPLE_CLASSES = 4 };  // the instantiation a column needs: SAMPLE_DEFAULT .. SAMPLE_MIROSTAT, or the first maximum
struct SampleReqParams {  // (SampleCols' parameters, by the same names)
    int k;
    float top_p, temperature, penalty;
    float freq, presence, tail_free_z, typical_p, min_p;
    int mirostat;
    float tau, eta;
    int n_bias;
};
struct SampleReqBack {
    SampleState state;
    int n_drawn[BATCH_COLS_MAX], ended_by[BATCH_COLS_MAX], live[BATCH_COLS_MAX];
};
struct SampleReqs {
    SampleReqBack back;                             // first: the table's address is its SampleState's
    int max_draws[BATCH_COLS_MAX];                  // the column ends with its max_draws-th draw (0: it never draws)
    int n_stop[BATCH_COLS_MAX];                     // ... or with a draw of one of its stop ids
    int stop_id[BATCH_COLS_MAX][CHAIN_STOP_MAX];
    int n_list[SAMPLE_CLASSES];                     // the columns of each class, compacted: the grid of class s is n_list[s] workgroups,
    int list[SAMPLE_CLASSES][BATCH_COLS_MAX];       // workgroup w of it works on column list[s][w].  Fixed for the whole call.
    SampleReqParams prm[BATCH_COLS_MAX];
    SampleBias bias[BATCH_COLS_MAX];
};
// whose parameters an instantiation reads: the one set of a SampleCols, or column c's request
template <bool REQ>
__device__ __forceinline__ auto sample_params_of(const SampleCols *sc, const void *table, int c) {
    if constexpr (REQ) return &static_cast<const SampleReqs *>(table)->prm[c];
    else return sc;
}
// the end of a live column's tail (one thread): the draw is counted, and the column stops being live if the id is one of its stop ids
// or its budget is used up.  The stop id wins: it is what the reference's loop would report (EndOfText, inference_session.rs:404-408).
__device__ __forceinline__ void chain_req_drawn(SampleReqs *rq, int c, int id) {
    const int n = rq->back.n_drawn[c] + 1;
    rq->back.n_drawn[c] = n;
    const int ns = rq->n_stop[c] < CHAIN_STOP_MAX ? rq->n_stop[c] : CHAIN_STOP_MAX;
    bool stop = false;
    for (int j = 0; j < ns; j++) stop = stop || rq->stop_id[c][j] == id;
    if (stop || n >= rq->max_draws[c]) {
        rq->back.ended_by[c] = stop ? CHAIN_END_STOP : CHAIN_END_BUDGET;
        rq->back.live[c] = 0;
    }
}

// ---- the selection: which keys of the row are its k largest.  Over global memory (topk_kth_key, k_topk's radix passes) the row is
// read nine times from L2 (eight passes of one dependent load per thread and iteration, then the gather); beside a 1.1 ms token that
// is most of the distance to the stepped loop.  On chip the row is fetched ONCE, eight independent 16-byte loads in flight per
// thread, and stays there for every pass and for the gather.
// On chip means REGISTERS, 32 values per thread (thread t: ids 32 t .. 32 t + 31), V <= SELECT_CAP = 32768: a 32000-float row in
// LDS would be 125 KB of the CU's 160 KB — no room beside k_topk's tables for a wider vocabulary than the registers take anyway,
// every pass would read it back through the LDS pipe the histogram's atomics already queue at, and __launch_bounds__(1024) leaves
// 128 VGPRs of which the row takes 32.  Wider rows (template argument ONCHIP = false; launch_sample_next picks by V alone, for every
// number of columns) take topk_kth_key over global memory.
//
// sample_select: which of this thread's values belong to the k largest keys of the row (topk_key order), as a bit mask.
//   value bits  four radix passes of 8 bits over the order-preserving image of the VALUE (the high word of topk_key), histogram in
//               LDS.  The first digit is the sign and seven exponent bits: a row of logits lands in three or four bins, and 64 lanes
//               of one atomic instruction on one word are served one after the other — with one 256-bin table the kernel took
//               72 us, with the copies 48.  Tables per WAVE would not help (the lanes that collide are lanes of one wave; the
//               instructions of 16 waves queue at one LDS pipe whichever table they name), so the table is replicated per LANE:
//               SELECT_COPIES = 32 copies, bin d of copy c at word d * 32 + c, lane l adds to copy l & 31 — the 32 lanes the pipe
//               serves together sit in 32 banks whatever their digits.  32 KB of LDS for a kernel that has the CU to itself.
//               Thread d < 256 sums bin d's copies (starting at copy d & 31, again one bank per lane); suffix sums by shuffles.
//   id bits     no passes.  Equal values differ in the low word only, ~id, and a thread's ids are consecutive and ascending with
//               its thread index: the r lowest ids among the keys equal to the k-th value are the first r in (thread, register)
//               order — one workgroup prefix sum of the threads' counts.  (All-equal rows, where every value pass keeps every key,
//               end here like any other row.)
constexpr int SELECT_PER_THREAD = 32;
constexpr int SELECT_CAP = 1024 * SELECT_PER_THREAD;
constexpr int SELECT_COPIES = 32;  // of the 256-bin histogram: one per lane of a half-wave

// the order-preserving image of a value: topk_key's high word
__device__ __forceinline__ uint32_t select_value_bits(float v) { return (uint32_t)(topk_key(v, 0) >> 32); }

// thread t's 32 values of x[0 .. V), V <= SELECT_CAP; entries from V on are never looked at (sample_select masks them by id)
__device__ __forceinline__ void sample_select_load(const float *__restrict__ x, int V, float (&v)[SELECT_PER_THREAD]) {
    const int base = (int)threadIdx.x * SELECT_PER_THREAD;
    const bool vec = (reinterpret_cast<uintptr_t>(x) & 15) == 0;  // (base is a multiple of 32 floats)
#pragma unroll
    for (int j = 0; j < SELECT_PER_THREAD / 4; j++) {
        const int i = base + 4 * j;
        float4 f = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (vec && i + 4 <= V) {
            f = *reinterpret_cast<const float4 *>(x + i);
        } else {
            if (i + 0 < V) f.x = x[i + 0];
            if (i + 1 < V) f.y = x[i + 1];
            if (i + 2 < V) f.z = x[i + 2];
            if (i + 3 < V) f.w = x[i + 3];
        }
        v[4 * j + 0] = f.x;
        v[4 * j + 1] = f.y;
        v[4 * j + 2] = f.z;
        v[4 * j + 3] = f.w;
    }
}
// bit i set: v[i] (id 32 t + i) is one of the k largest keys of the row, 1 <= k <= V <= SELECT_CAP.  One 1024-thread workgroup.
__device__ __forceinline__ uint32_t sample_select(const float (&v)[SELECT_PER_THREAD], int V, int k) {
    __shared__ unsigned int s_hist[256 * SELECT_COPIES];
    __shared__ unsigned int s_prefix, s_remaining, s_digits[4];
    __shared__ int s_wave[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int base = tid * SELECT_PER_THREAD;
    __syncthreads();  // (a caller's earlier use of these words is over)
    if (tid == 0) {
        s_prefix = 0;
        s_remaining = (unsigned int)k;
    }
    uint32_t mask = 0;
    for (int pass = 0; pass < 4; pass++) {
        const int shift = 24 - 8 * pass;
        for (int i = tid; i < 256 * SELECT_COPIES; i += 1024) s_hist[i] = 0;
        __syncthreads();
        const uint32_t prefix = s_prefix;
        unsigned int *copy = s_hist + (lane & (SELECT_COPIES - 1));
#pragma unroll
        for (int i = 0; i < SELECT_PER_THREAD; i++) {
            const uint32_t o = select_value_bits(v[i]);
            if (base + i < V && (o & mask) == prefix) atomicAdd(&copy[((o >> shift) & 255u) * SELECT_COPIES], 1u);
        }
        __syncthreads();
        // threads 0 .. 255 = waves 0 .. 3: `mine` = the keys of digit tid, `above` = those of the digits above it
        unsigned int above = 0, mine = 0;
        if (tid < 256) {
#pragma unroll
            for (int c = 0; c < SELECT_COPIES; c++) mine += s_hist[tid * SELECT_COPIES + ((c + tid) & (SELECT_COPIES - 1))];
            unsigned int inc = mine;  // inclusive suffix sum inside the wave
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned int down = __shfl_down(inc, off);
                if (lane + off < 64) inc += down;
            }
            if (lane == 0) s_digits[wave] = inc;
            above = inc - mine;
        }
        const unsigned int rem = s_remaining;
        __syncthreads();  // everyone has read s_remaining and the histogram
        if (tid < 256)
            for (int w = wave + 1; w < 4; w++) above += s_digits[w];
        if (tid < 256 && above < rem && rem <= above + mine) {  // exactly one digit
            s_prefix = prefix | ((uint32_t)tid << shift);
            s_remaining = rem - above;
        }
        mask |= 0xFFu << shift;
        __syncthreads();
    }
    const uint32_t kth = s_prefix;      // the k-th largest value; every key above it is in
    const int r = (int)s_remaining;     // ... and the r lowest ids of the keys that equal it, 1 <= r <= their number
    uint32_t gt = 0, eq = 0;
#pragma unroll
    for (int i = 0; i < SELECT_PER_THREAD; i++) {
        const uint32_t o = select_value_bits(v[i]);
        if (base + i < V) {
            gt |= (o > kth ? 1u : 0u) << i;
            eq |= (o == kth ? 1u : 0u) << i;
        }
    }
    // exclusive prefix sum of the threads' counts of equal keys, in thread order = id order
    const int cnt = __popc(eq);
    int inc = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int up = __shfl_up(inc, off);
        if (lane >= off) inc += up;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    int before = inc - cnt;
    for (int w = 0; w < wave; w++) before += s_wave[w];
    int room = r - before;  // how many of this thread's equal keys are in, lowest register first
#pragma unroll
    for (int i = 0; i < SELECT_PER_THREAD; i++) {
        if (((eq >> i) & 1u) && room > 0) {
            gt |= 1u << i;
            room--;
        }
    }
    return gt;
}

// Grid = B workgroups of 1024 threads; workgroup c works on row c of logits [B][V] and on entry c of every table (sc->hist[c],
// sc->hist_n[c], st->rng[c], st->mu[c], out[c]) — nothing is handed between workgroups, no workgroup waits for another, and entries
// from B on are not touched.  bc is the table of a batched step, or null for one session at DecParams::n_past (write_next_token, decode.h).
//   M           (SAMPLE_FULL / SAMPLE_MIROSTAT) the ids whose value the step adjusts, <= 128: threads 0 .. 63 take the window's tokens
//               (each id once, with its count and its bias), threads 64 .. 127 the bias entries that are not in the window;
//               sampler_adjust.  SAMPLE_DEFAULT: the window's tokens, sampler_penalise.
//   selection   the k largest raw keys of the row: sample_select over the row in registers (ONCHIP), or topk_kth_key over global
//               memory and a scan of the row against the k-th key.  M's tokens enter with their adjusted values, the raw top-k
//               without M's tokens beside them: <= k + 128 keys, bitonic-sorted in LDS by (value descending, id ascending) —
//               topk_key's order.  Both selections yield the same set of keys, so the same sorted keys;
//   q, p        one thread per candidate (f32: sampler_q / sampler_p);
//   filters     (SAMPLE_FULL) thread 0: tail-free and locally typical's mean (f64 sums in list order); one thread per entry: its
//               key, then its rank among the keys by (key, index) — 256 comparisons each, the order any sort would give; thread 0
//               again: sampler_pick_chain (the visit, top-p, min-p, the draw);
//   serial tail thread 0: sampler_pick (SAMPLE_DEFAULT) / sampler_pick_chain, then the next replay's parameters (write_next_token),
//               out[c], the id into the column's ring slot hist_n % 64, hist_n + 1, the advanced generator state.
//   Mirostat 2  (SAMPLE_MIROSTAT, ONCHIP only: no selection, no sort) the row stays in registers, 32 ids per thread = one block of
//               the specification: M's values patched in, a workgroup maximum with its lowest id, 32 exponentials per thread, the
//               thread's f64 block sum to LDS, thread 0 over the blocks in order (S), the retain mask per thread, block sums
//               again (S_R), thread 0 draws and walks the blocks; the thread that owns the block walks its registers and is the
//               tail: mu, the generator, the parameters, the ring.
// k is 1 .. min(SAMPLER_K_MAX, V) (not read by Mirostat 2), and V <= SELECT_CAP on chip (the host declines / picks so; the kernel
// writes nothing otherwise).
//
// REQ (the chains that stop): `rng` is the call's SampleReqs.  Workgroup w works on column list[CHAIN][w] with that column's own
// parameters, bias table and end rule; sc holds the rings alone.  A column that is not live touches nothing but out[c] = -1 — the test
// is uniform over the workgroup and comes before any barrier and before the row is loaded — so the step behind this launch evaluates
// the same token at the same position again.  A live column's tail also counts the draw and applies the end rule (chain_req_drawn).
template <bool ONCHIP, int CHAIN = SAMPLE_DEFAULT, bool REQ = false>
__global__ void __launch_bounds__(1024) k_sample_next(const float *__restrict__ logits, int V, DecParams *prm, BatchCols *bc,
                                                      SampleCols *sc, unsigned long long *rng, int *__restrict__ out) {
    constexpr int PMAX = 512;  // power of two >= SAMPLER_K_MAX + SAMPLER_M_MAX
    constexpr int NM = CHAIN == SAMPLE_DEFAULT ? SAMPLER_WINDOW : SAMPLER_M_MAX;
    static_assert(PMAX >= SAMPLER_K_MAX + SAMPLER_M_MAX, "k_sample_next: LDS keys");
    static_assert(CHAIN != SAMPLE_MIROSTAT || ONCHIP, "k_sample_next: Mirostat 2 works on the row in registers");
    static_assert(SAMPLER_BLOCK == SELECT_PER_THREAD, "k_sample_next: one thread, one block of Mirostat's sums");
    __shared__ unsigned long long s_keys[PMAX];
    __shared__ float s_v[SAMPLER_K_MAX], s_q[SAMPLER_K_MAX], s_p[SAMPLER_K_MAX];
    __shared__ int s_id[SAMPLER_K_MAX], s_h[SAMPLER_WINDOW], s_win[NM];
    __shared__ int s_cnt, s_wn;
    int c = blockIdx.x;
    const int tid = threadIdx.x;
    [[maybe_unused]] SampleReqs *rq = nullptr;
    if constexpr (REQ) {
        rq = reinterpret_cast<SampleReqs *>(rng);
        if (c >= BATCH_COLS_MAX || c >= rq->n_list[CHAIN]) return;
        c = rq->list[CHAIN][c];
        if (c < 0 || c >= BATCH_COLS_MAX) return;
        if (!rq->back.live[c]) {
            if (tid == 0) out[c] = -1;
            return;
        }
    }
    const auto *pp = sample_params_of<REQ>(sc, rng, c);
    const int k = pp->k;
    if (c >= BATCH_COLS_MAX || (ONCHIP && V > SELECT_CAP)) return;
    if (CHAIN != SAMPLE_MIROSTAT && (k < 1 || k > SAMPLER_K_MAX || k > V)) return;
    const float *x = logits + (size_t)c * V;
    [[maybe_unused]] float v[ONCHIP ? SELECT_PER_THREAD : 1];
    if constexpr (ONCHIP) sample_select_load(x, V, v);  // (in flight while the window is set up)
    const float penalty = pp->penalty, temperature = pp->temperature;
    const int hn = sc->hist_n[c];
    const int nw = hn < SAMPLER_WINDOW ? (hn < 0 ? 0 : hn) : SAMPLER_WINDOW;
    int P = 1;
    if constexpr (CHAIN != SAMPLE_MIROSTAT) {
        while (P < k + nw + (CHAIN == SAMPLE_DEFAULT ? 0 : sample_n_bias(pp))) P <<= 1;
        for (int i = tid; i < P; i += 1024) s_keys[i] = 0;  // (below every key of a row without NaN)
    }
    if (tid < SAMPLER_WINDOW) s_h[tid] = tid < nw ? sc->hist[c][tid] : -1;
    if (tid == 0) {
        s_cnt = 0;
        s_wn = 0;
    }
    if constexpr (CHAIN == SAMPLE_DEFAULT) {
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
    } else {
        __shared__ int s_bid[SAMPLER_BIAS_MAX];
        __shared__ float s_bv[SAMPLER_BIAS_MAX], s_adj[SAMPLER_M_MAX];
        const int nb = sample_n_bias(pp);
        const float freq = pp->freq, presence = pp->presence;
        if (tid < SAMPLER_BIAS_MAX) {
            const SampleBias *sb = reinterpret_cast<const SampleBias *>(rng) - 1;  // (SampleHead)
            if constexpr (REQ) sb = &rq->bias[c];
            s_bid[tid] = tid < nb ? sb->id[tid] : -1;
            s_bv[tid] = tid < nb ? sb->b[tid] : 0.0f;
        }
        __syncthreads();
        // M: thread t < 64 the window's token t (its first occurrence), thread 64 + j bias entry j unless the window holds its id
        int id = -1, count = 0, at = -1;
        if (tid < nw) {
            id = s_h[tid];
            for (int j = 0; j < tid; j++)
                if (s_h[j] == id) id = -1;
            for (int j = 0; j < nw; j++) count += s_h[j] == id;
            for (int j = 0; j < nb; j++)
                if (s_bid[j] == id) at = j;
        } else if (tid >= SAMPLER_WINDOW && tid < SAMPLER_WINDOW + nb) {
            at = tid - SAMPLER_WINDOW;
            id = s_bid[at];
            for (int j = 0; j < nw; j++)
                if (s_h[j] == id) id = -1;
        }
        if (id >= 0 && id < V) {
            const float val = sampler_adjust(x[id], at >= 0, at >= 0 ? s_bv[at] : 0.0f, count, penalty, freq, presence);
            const int slot = atomicAdd(&s_wn, 1);
            s_win[slot] = id;
            if constexpr (CHAIN == SAMPLE_MIROSTAT) s_adj[slot] = val;
            else s_keys[atomicAdd(&s_cnt, 1)] = topk_key(val, id);
        }
        if constexpr (CHAIN == SAMPLE_MIROSTAT) {
            __shared__ double s_blk[1024];
            __shared__ unsigned int s_mask[1024];
            __shared__ float s_wmax[16];
            __shared__ int s_wat[16], s_selb, s_walk;
            __shared__ double s_S, s_SR, s_urel;
            __shared__ unsigned long long s_x;
            SampleState *st = reinterpret_cast<SampleState *>(rng);
            const int base = tid * SELECT_PER_THREAD, lane = tid & 63, wave = tid >> 6;
            const int nblk = (V + SELECT_PER_THREAD - 1) / SELECT_PER_THREAD;
            __syncthreads();
            const int wn = s_wn;
            for (int j = 0; j < wn; j++) {  // a_i: M's values into the registers that hold their ids
                const int mid = s_win[j];
                if ((mid >> 5) == tid) {
                    const float val = s_adj[j];
#pragma unroll
                    for (int i = 0; i < SELECT_PER_THREAD; i++)
                        if (i == (mid & 31)) v[i] = val;
                }
            }
            // amax and the lowest id that holds it
            float mx = 0.0f;
            int first = 0x7FFFFFFF;
#pragma unroll
            for (int i = 0; i < SELECT_PER_THREAD; i++)
                if (base + i < V && (first == 0x7FFFFFFF || v[i] > mx)) {
                    mx = v[i];
                    first = base + i;
                }
            const auto better = [](float om, int oa, float m, int a) { return oa != 0x7FFFFFFF && (a == 0x7FFFFFFF || om > m || (om == m && oa < a)); };
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const float om = __shfl_xor(mx, off);
                const int oa = __shfl_xor(first, off);
                if (better(om, oa, mx, first)) {
                    mx = om;
                    first = oa;
                }
            }
            if (lane == 0) {
                s_wmax[wave] = mx;
                s_wat[wave] = first;
            }
            __syncthreads();
            mx = s_wmax[0];
            first = s_wat[0];
            for (int w = 1; w < 16; w++)
                if (better(s_wmax[w], s_wat[w], mx, first)) {
                    mx = s_wmax[w];
                    first = s_wat[w];
                }
            // e_i in place of a_i; the block's f64 sum in id order
            double sum = 0.0;
#pragma unroll
            for (int i = 0; i < SELECT_PER_THREAD; i++) {
                v[i] = base + i < V ? sampler_mirostat_e(v[i], mx, temperature) : 0.0f;
                if (base + i < V) sum += (double)v[i];
                __builtin_amdgcn_sched_barrier(0);  // (one exponential at a time: 32 interleaved would not fit beside the row)
            }
            s_blk[tid] = sum;
            __syncthreads();
            if (tid == 0) {
                double S = 0.0;
                for (int b = 0; b < nblk; b++) S += s_blk[b];
                s_S = S;
            }
            __syncthreads();
            const float mu = st->mu[c];
            uint32_t keep = 0;
            if (!(mu < 0.0f)) {
                const double least = sampler_mirostat_least(s_S, mu);
#pragma unroll
                for (int i = 0; i < SELECT_PER_THREAD; i++) {
                    keep |= (base + i < V && (double)v[i] >= least ? 1u : 0u) << i;
                    __builtin_amdgcn_sched_barrier(0);  // (one conversion at a time, as above)
                }
            }
            if ((first >> 5) == tid) keep |= 1u << (first & 31);
            sum = 0.0;
#pragma unroll
            for (int i = 0; i < SELECT_PER_THREAD; i++)
                if ((keep >> i) & 1u) {
                    sum += (double)v[i];
                    __builtin_amdgcn_sched_barrier(0);
                }
            s_blk[tid] = sum;
            s_mask[tid] = keep;
            __syncthreads();
            if (tid == 0) {  // S_R, the draw, the block it falls into (or, past them all, the last block that retains an id)
                double SR = 0.0;
                for (int b = 0; b < nblk; b++) SR += s_blk[b];
                const uint64_t xs = sampler_rng_step(st->rng[c]);
                const double u = sampler_rng_unit(xs) * SR;
                double run = 0.0, before = 0.0;
                int selb = -1;
                for (int b = 0; b < nblk; b++) {
                    before = run;
                    run += s_blk[b];
                    if (run > u) {
                        selb = b;
                        break;
                    }
                }
                s_walk = selb >= 0;
                for (int b = nblk - 1; b >= 0 && selb < 0; b--)
                    if (s_mask[b]) selb = b;
                s_selb = selb;
                s_urel = u - before;
                s_SR = SR;
                s_x = xs;
            }
            __syncthreads();
            if (tid == s_selb) {  // the block's owner walks its retained ids, and is the tail
                const double urel = s_urel;
                const bool walk = s_walk != 0;
                int sel = first;
                float e_sel = 0.0f;
                double acc = 0.0;
                bool done = false;
#pragma unroll
                for (int i = 0; i < SELECT_PER_THREAD; i++)
                    if (((keep >> i) & 1u) && !done) {
                        sel = base + i;  // (the block's last retained id, unless the walk stops before it)
                        e_sel = v[i];
                        acc += (double)v[i];
                        done = walk && urel < acc;
                    }
                st->mu[c] = sampler_mirostat_mu(mu, e_sel, s_SR, pp->tau, pp->eta);
                st->rng[c] = s_x;
                write_next_token(prm, bc, c, sel);
                out[c] = sel;
                sc->hist[c][(unsigned)hn % SAMPLER_WINDOW] = sel;
                sc->hist_n[c] = hn + 1;
                if constexpr (REQ) chain_req_drawn(rq, c, sel);
            }
            return;
        }
    }
    // the raw top-k, without M's tokens (both selections open with a barrier: s_win / s_wn are complete behind it)
    const auto gather = [&](unsigned long long key, int id, int wn) {
        bool in_window = false;
        for (int j = 0; j < wn; j++) in_window = in_window || s_win[j] == id;
        if (!in_window) s_keys[atomicAdd(&s_cnt, 1)] = key;
    };
    if constexpr (ONCHIP) {
        const uint32_t in = sample_select(v, V, k);
        const int wn = s_wn;
#pragma unroll
        for (int i = 0; i < SELECT_PER_THREAD; i++)
            if ((in >> i) & 1u) gather(topk_key(v[i], tid * SELECT_PER_THREAD + i), tid * SELECT_PER_THREAD + i, wn);
    } else {
        const unsigned long long kth = topk_kth_key(x, V, k);
        const int wn = s_wn;
        for (int i = tid; i < V; i += 1024) {
            const unsigned long long key = topk_key(x[i], i);
            if (key >= kth) gather(key, i, wn);
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
    if constexpr (CHAIN == SAMPLE_FULL) {
        __shared__ double s_t[SAMPLER_K_MAX], s_mean, s_Q;
        __shared__ int s_ord[SAMPLER_K_MAX], s_idx[SAMPLER_K_MAX], s_n1;
        const float typical_p = pp->typical_p;
        const bool typ = typical_p < 1.0f;  // (the same for every thread: the barriers below are taken by all or none)
        if (tid == 0) {
            const int n1 = sampler_tail_free(s_q, k, pp->tail_free_z);
            double Q = 0.0;
            if (typ) s_mean = sampler_typical_mean(s_v, s_q, n1, &Q);
            s_Q = Q;
            s_n1 = n1;
        }
        __syncthreads();
        const int n1 = s_n1;
        if (typ) {
            if (tid < n1) s_t[tid] = sampler_typical_key(s_v[0], s_v[tid], s_q[tid], s_mean);
            __syncthreads();
            if (tid < n1) {  // the entry's place in the order by (key ascending, index ascending): the keys below it, counted
                const double t = s_t[tid];
                int rank = 0;
                for (int j = 0; j < n1; j++) {
                    const double tj = s_t[j];
                    rank += (tj < t || (tj == t && j < tid)) ? 1 : 0;
                }
                s_ord[rank] = tid;
            }
            __syncthreads();
        }
        if (tid == 0) {
            uint64_t state = rng[c];
            const int id = s_id[sampler_pick_chain(s_q, s_p, n1, typ ? s_ord : nullptr, s_Q, typical_p, pp->top_p, pp->min_p, s_idx, &state)];
            rng[c] = state;
            write_next_token(prm, bc, c, id);
            out[c] = id;
            sc->hist[c][(unsigned)hn % SAMPLER_WINDOW] = id;
            sc->hist_n[c] = hn + 1;
            if constexpr (REQ) chain_req_drawn(rq, c, id);
        }
        return;
    }
    if (tid == 0) {
        uint64_t state = rng[c];
        const int id = s_id[sampler_pick(s_q, s_p, k, pp->top_p, &state)];
        rng[c] = state;
        write_next_token(prm, bc, c, id);
        out[c] = id;
        sc->hist[c][(unsigned)hn % SAMPLER_WINDOW] = id;
        sc->hist_n[c] = hn + 1;
        if constexpr (REQ) chain_req_drawn(rq, c, id);
    }
}
#ifdef SAMPLE_REQ_OBJECT
// k_argmax_next for the chains that stop: the columns whose request is "greedy", through the same table — the same live test in the same
// place, the first maximum, the same tail (the id goes to the column's ring too: one history whatever the column's class).
__global__ void __launch_bounds__(1024) k_argmax_next_req(const float *__restrict__ logits, int V, DecParams *prm, BatchCols *bc, SampleCols *sc,
                                                          SampleReqs *rq, int *__restrict__ out) {
    int c = blockIdx.x;
    if (c >= BATCH_COLS_MAX || c >= rq->n_list[SAMPLE_GREEDY]) return;
    c = rq->list[SAMPLE_GREEDY][c];
    if (c < 0 || c >= BATCH_COLS_MAX) return;
    if (!rq->back.live[c]) {
        if (threadIdx.x == 0) out[c] = -1;
        return;
    }
    const int bi = argmax_first_block(logits + (size_t)c * V, V);
    if (threadIdx.x == 0) {
        const int hn = sc->hist_n[c];
        write_next_token(prm, bc, c, bi);
        out[c] = bi;
        sc->hist[c][(unsigned)hn % SAMPLER_WINDOW] = bi;
        sc->hist_n[c] = hn + 1;
        chain_req_drawn(rq, c, bi);
    }
}
#endif
// The one launch of the sampler, for the chain, the batched chain and the test hook: B columns, the selection picked from V alone, the
// stages from the chain's parameters (`stages`: SAMPLE_DEFAULT for neutral extras — today's kernel).  rng is a SampleHead's state.
// The SAMPLE_FULL and SAMPLE_MIROSTAT instantiations are compiled into an object of their own (sample_ext.hip, which defines
// launch_sample_next_ext): the code object that holds every other kernel of the library keeps its contents and its addresses.
// The chains that stop launch through launch_next_token_req (sample_req.hip, a third object for the same reason): every class of
// columns that is present once, n_class[s] workgroups each, over the lists of the SampleReqs `reqs`.
#ifndef SAMPLE_EXT_OBJECT
void launch_next_token_req(hipStream_t stream, const int *n_class, const float *logits, int V, void *prm, void *bc, void *sc, void *reqs, int *out);
void launch_sample_next_ext(hipStream_t stream, int B, const float *logits, int V, void *prm, void *bc, void *sc, void *state, int *out, int stages);
static inline void launch_sample_next(hipStream_t stream, int B, const float *logits, int V, DecParams *prm, BatchCols *bc, SampleCols *sc,
                                      unsigned long long *rng, int *out, int stages = SAMPLE_DEFAULT) {
    if (stages != SAMPLE_DEFAULT)
        launch_sample_next_ext(stream, B, logits, V, prm, bc, sc, rng, out, stages);
    else if (V <= SELECT_CAP)
        hipLaunchKernelGGL((k_sample_next<true, SAMPLE_DEFAULT>), dim3((unsigned)B), dim3(1024), 0, stream, logits, V, prm, bc, sc, rng, out);
    else
        hipLaunchKernelGGL((k_sample_next<false, SAMPLE_DEFAULT>), dim3((unsigned)B), dim3(1024), 0, stream, logits, V, prm, bc, sc, rng, out);
}
#endif
