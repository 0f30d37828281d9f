// mpt_batch.h — what the batched MPT step (plan_mpt_batch.inc plan_launch_mpt_batch; option plan_mpt_batch) launches that no other plan
// does, compiled into a code object of its own (mpt_batch.hip, MPT_BATCH_OBJECT) so that every other code object holds what it held:
//   k_mmq_cols<QT, EPI_QKV_TM_BATCH>        the Wqkv mat-vec of B columns, K and V rows placed per column (kernels/mmq_cols.h)
//   k_attn_batch_{scores,vp,merge}_alibi    the batched ALiBi decode attention: column c against ITS session's cache, BatchCols on the device
// hip_backend.hip sees only the helpers and the launch functions declared at the end of this file.
#pragma once
#include <stddef.h>
#include <stdint.h>
// Workgroups per head of the batched attention (grid (H, W)): about CUs / H, 1 .. 16 — fixed when the plan is built
static inline int mpt_batch_W(int num_cus, int64_t H) {
    const int64_t w = num_cus / (H > 0 ? H : 1);
    return (int)(w < 1 ? 1 : w > 16 ? 16 : w);
}
// Tiles of 64 keys the longest share can hold: B columns of at most C keys each, dealt to W workgroups
static inline size_t mpt_batch_share_tiles(int64_t C, int B, int W) {
    const size_t total = (size_t)B * (size_t)((C + 63) / 64);
    return (total + (size_t)W - 1) / (size_t)W;
}
// LDS of launch 2: the share's p values as f16 (a segment never exceeds the share: Q tiles of 64 keys), dynamic; next to them the kernel's
// static arrays (the V.P partial sums of the key groups, 8 KiB, and the f64 sum's four words) — the bound the matcher holds to 150 KiB
static inline size_t mpt_batch_attn_lds_dyn(int64_t C, int B, int W) { return mpt_batch_share_tiles(C, B, W) * 64 * 2; }
static inline size_t mpt_batch_attn_lds(int64_t C, int B, int W) { return mpt_batch_attn_lds_dyn(C, B, W) + 8192 + 64; }
// one batched attention (the three launches below); hip_backend.hip fills it, it travels as void *
struct MptBatchAttnArgs {
    const float *q;      // [B] rows, ldq floats apart: the Q columns of the Wqkv product
    int64_t ldq;
    const void *bc;      // the step's BatchCols: pos[c], mem_k[c], mem_v[c] (both caches token-major [L][C][E] f16)
    int64_t kv_off;      // the layer's offset into every cache, elements
    const float *slopes;
    float scale;
    int B, D, H, W, f16d;
    int64_t E, C;
    float *sc;    // [B][H][C]
    float *pmax;  // [H][B][W]
    float *part;  // [H][B][W][D]
    float *out;   // [B][E] f32
    int8_t *lo, *hi;
    float *dq;
    int *sumq;
    float *dT;
    int *sT;
};
#ifdef MPT_BATCH_OBJECT
#include "mmq_cols.h"

// ---------------------------------------------------------------------------------------------------
// Batched ALiBi decode attention.  Column c is ONE query of session c at position pos[c], against rows 0 .. pos[c] of that session's
// token-major cache; the lengths differ (one session at 4000 positions next to seven at 100), so the work is not split per column but
// over the CONCATENATED keys: per head the B columns' keys form one list in column order, in tiles of 64 keys (column c:
// ceil((pos[c] + 1) / 64) tiles), and workgroup w of the grid (H, W) takes the tile range [w Q, (w + 1) Q), Q = ceil(total / W) — all
// derived from BatchCols on the device (batch_segment), so one captured graph serves every step of a chain that moves pos itself.  A
// share may end inside a column, hold whole short columns, or be empty; every workgroup walks the B columns and handles the segment
// (key range) of each that lies in its share.  ggml's rounding points are kept as k_attn_chunk_*_alibi keep them (no online softmax):
// three launches, every dependency a kernel boundary, nothing waits inside a launch.
//   1. k_attn_batch_scores_alibi  per segment: q . k with D / 8 lanes a key, 16 bytes of the key's row a lane (each K row is read once, in whole
//                                 rows), q and K as f16, their exact products added in f64 and the sum rounded to f32 ONCE — the value every
//                                 f32 accumulation order approximates; x = fadd(fmul((float)t, slope), fmul(s, scale)) -> sc[c][h][t]; the
//                                 segment's maximum -> pmax[h][c][w] (-inf: no key of c here).  Not the 32-key MFMA tile: with one query a
//                                 column it is 1/32 used, and its f32 sums differ from the executor's by an ulp here and there — one such
//                                 ulp that flips f16(x - mx) of a single key costs more than the whole error of a one-query row
//   2. k_attn_batch_vp_alibi      per segment: mx over pmax[h][c][..]; e = f16(exp(f16(x - mx))) and its f64 sum over the column's WHOLE
//                                 row, redone by every workgroup that holds keys of the column (every e a multiple of 2^-24 in [0, 1]:
//                                 exact in any order); inv = (float)(1 / sum); the segment's p = f16(e * inv) into LDS; V.P over the
//                                 segment on the VALU — one query makes P a single row, an MFMA tile would be 1/32 used: D / 8 lanes
//                                 a key (16 bytes of V each, f32 accumulation), the 256 / (D / 8) key groups added in group order
//                                 through LDS -> part[h][c][w][D] (no key of c here: zeros, from the same code)
//   3. k_attn_batch_merge_alibi   B workgroups: out[c][h D + d] = sum over w ascending of part; the row re-quantized to Q8 in the planar
//                                 and the [block][8] layouts out_proj's k_mmq_cols stages (k_attn_chunk_merge_alibi's tail)
// A position outside [0, C) gives its column no keys (never: the entry checks n_past + steps <= C).  Rows behind pos[c] are never read.
// ---------------------------------------------------------------------------------------------------
typedef _Float16 bt_f16x8 __attribute__((ext_vector_type(8)));
// the keys [t0, t1) of column c that lie in workgroup w's share; T: the column's keys (0 .. pos); all wave-uniform
__device__ __forceinline__ void batch_segment(const BatchCols *bc, int B, int W, int64_t C, int w, int c, int &t0, int &t1, int &T) {
    int total = 0, pre = 0, nc = 0;
    T = 0;
    for (int i = 0; i < B; i++) {
        const int p = bc->pos[i];
        const int Ti = p >= 0 && p < C ? p + 1 : 0;
        const int ni = (Ti + 63) >> 6;
        if (i < c) pre += ni;
        if (i == c) nc = ni, T = Ti;
        total += ni;
    }
    const int Q = (total + W - 1) / W;
    const int lo = max(w * Q, pre), hi = min(min((w + 1) * Q, total), pre + nc);
    t0 = t1 = 0;
    if (hi > lo) {
        t0 = (lo - pre) * 64;
        t1 = min((hi - pre) * 64, T);
    }
}
template <int D>
__global__ void __launch_bounds__(256) k_attn_batch_scores_alibi(const MptBatchAttnArgs a) {
    __shared__ float s_mx[BATCH_COLS_MAX][4];
    constexpr int LPK = D / 8, KPW = 64 / LPK;  // lanes a key, keys a wave and step
    const int h = blockIdx.x, w = blockIdx.y;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, piece = lane % LPK, kw = lane / LPK;
    const BatchCols *bc = (const BatchCols *)a.bc;
    const float slope = a.slopes[h];
    for (int c = 0; c < a.B; c++) {  // workgroup-uniform
        int t0, t1, T;
        batch_segment(bc, a.B, a.W, a.C, w, c, t0, t1, T);
        float m = -INFINITY;
        if (t1 > t0) {
            double qd[8];  // this lane's eight channels of the query, rounded to f16 as ggml rounds them
            const float *qp = a.q + (int64_t)c * a.ldq + (int64_t)h * D + piece * 8;
            const f32x4 x0 = *(const f32x4 *)qp, x1 = *(const f32x4 *)(qp + 4);
#pragma unroll
            for (int k = 0; k < 4; k++) qd[k] = (double)round_f16(x0[k]), qd[4 + k] = (double)round_f16(x1[k]);
            const __half *kg = bc->mem_k[c] + a.kv_off + (int64_t)h * D + piece * 8;
            float *sc = a.sc + ((int64_t)c * a.H + h) * a.C;
            const int nstep = (t1 - t0 + KPW - 1) / KPW;
            for (int j = wave; j < nstep; j += 4) {  // wave-uniform
                const int t = t0 + KPW * j + kw;
                const bool valid = t < t1;
                bt_f16x8 kb = {0, 0, 0, 0, 0, 0, 0, 0};
                if (valid) kb = *(const bt_f16x8 *)(kg + (int64_t)t * a.E);
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < 8; k++) acc = fma((double)(float)kb[k], qd[k], acc);  // (f16 x f16: exact; 128 of them in f64: exact)
#pragma unroll
                for (int o = 1; o < LPK; o <<= 1) acc += __shfl_xor(acc, o, 64);
                const float x = __fadd_rn(__fmul_rn((float)t, slope), __fmul_rn((float)acc, a.scale));
                if (valid && piece == 0) sc[t] = x;
                if (valid) m = fmaxf(m, x);
            }
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        if (lane == 0) s_mx[c][wave] = m;
    }
    __syncthreads();
    if (tid < a.B) a.pmax[((int64_t)h * a.B + tid) * a.W + w] = fmaxf(fmaxf(s_mx[tid][0], s_mx[tid][1]), fmaxf(s_mx[tid][2], s_mx[tid][3]));
}

template <int D>
__global__ void __launch_bounds__(256) k_attn_batch_vp_alibi(const MptBatchAttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    constexpr int LPK = D / 8, NG = 256 / LPK;  // lanes a key, key groups of the workgroup
    __shared__ __attribute__((aligned(16))) float s_red[NG][D];
    __shared__ double s_sum[4];
    _Float16 *s_p = (_Float16 *)lds;
    const int h = blockIdx.x, w = blockIdx.y;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int grp = tid / LPK, piece = tid % LPK;
    const BatchCols *bc = (const BatchCols *)a.bc;
    for (int c = 0; c < a.B; c++) {  // workgroup-uniform
        int t0, t1, T;
        batch_segment(bc, a.B, a.W, a.C, w, c, t0, t1, T);
        float *part = a.part + (((int64_t)h * a.B + c) * a.W + w) * D;
        if (t1 <= t0) {
            if (tid < D) part[tid] = 0.0f;
            continue;
        }
        const float *sc = a.sc + ((int64_t)c * a.H + h) * a.C;
        const float *pm = a.pmax + ((int64_t)h * a.B + c) * a.W;
        float mx = pm[0];
        for (int i = 1; i < a.W; i++) mx = fmaxf(mx, pm[i]);
        double sum = 0.0;
        for (int t = tid; t < T; t += 256) sum += (double)round_f16(expf(round_f16(sc[t] - mx)));
        sum = wave_sum_f64(sum);
        if (lane == 0) s_sum[wave] = sum;
        __syncthreads();  // (also: the previous column's reads of s_p and s_red are done)
        const float inv = (float)(1.0 / ((s_sum[0] + s_sum[1]) + (s_sum[2] + s_sum[3])));
        for (int t = t0 + tid; t < t1; t += 256) s_p[t - t0] = (_Float16)(round_f16(expf(round_f16(sc[t] - mx))) * inv);
        __syncthreads();
        // ---- V.P over the segment: lane `piece` of key group `grp` owns channels 8 piece .. 8 piece + 7 of the head ----
        const __half *vg = bc->mem_v[c] + a.kv_off + (int64_t)h * D + piece * 8;
        float acc[8];
#pragma unroll
        for (int k = 0; k < 8; k++) acc[k] = 0.0f;
#pragma unroll 4
        for (int t = t0 + grp; t < t1; t += NG) {
            const bt_f16x8 v = *(const bt_f16x8 *)(vg + (int64_t)t * a.E);
            const float p = (float)s_p[t - t0];
#pragma unroll
            for (int k = 0; k < 8; k++) acc[k] = __fmaf_rn((float)v[k], p, acc[k]);
        }
        *(f32x4 *)&s_red[grp][piece * 8] = f32x4{acc[0], acc[1], acc[2], acc[3]};
        *(f32x4 *)&s_red[grp][piece * 8 + 4] = f32x4{acc[4], acc[5], acc[6], acc[7]};
        __syncthreads();
        if (tid < D) {
            float v = s_red[0][tid];
#pragma unroll
            for (int g2 = 1; g2 < NG; g2++) v += s_red[g2][tid];
            part[tid] = v;
        }
    }
}

// one workgroup per column: the W partial rows added w ascending, then k_quant_row's quantizer per block of 32 lanes
__global__ void __launch_bounds__(256) k_attn_batch_merge_alibi(const MptBatchAttnArgs a) {
    const int n = blockIdx.x, tid = threadIdx.x, l = tid & 31;
    const int nblk = (int)(a.E >> 5);
    for (int b = tid >> 5; b < nblk; b += 8) {
        const int e = b * 32 + l, h = e / a.D, d = e - h * a.D;
        const float *pp = a.part + (((int64_t)h * a.B + n) * a.W) * a.D + d;
        float v = pp[0];
        for (int w = 1; w < a.W; w++) v += pp[(int64_t)w * a.D];
        a.out[(int64_t)n * a.E + e] = v;
        float amax = fabsf(v);
        amax = g32_max_f32(amax);
        const float dd = amax / 127.0f;
        const float id = act_id(amax, dd, aq_scalar());
        const int q = act_q(v * id, aq_scalar());
        int sq = q;
        sq = g32_sum_i32(sq);
        (l < 16 ? a.lo : a.hi)[((int64_t)n * nblk + b) * 16 + (l & 15)] = (int8_t)q;
        if (l == 0) {
            const float ds = a.f16d ? round_f16(dd) : dd;
            a.dq[(int64_t)n * nblk + b] = ds;
            a.sumq[(int64_t)n * nblk + b] = sq;
            a.dT[b * 8 + n] = ds;  // (B <= 8: one pass, one table)
            a.sT[b * 8 + n] = sq;
        }
    }
}
#else  // hip_backend.hip
// ---- what hip_backend.hip calls (defined in mpt_batch.hip; ColsArgs and BatchCols travel as void *) ----
// k_mmq_cols<qt, EPI_QKV_TM_BATCH> on G workgroups with `lds` bytes (cols_shape's); cols_args: a ColsArgs with ngroups / gq / gr, bc and
// kv_off set.  1: no such instantiation, or the LDS opt-in failed.
int launch_mpt_batch_cols(hipStream_t stream, int qt, const void *cols_args, int G, size_t lds);
// The batched attention (k_attn_batch_scores_alibi, k_attn_batch_vp_alibi on H x W workgroups, k_attn_batch_merge_alibi on B);
// args: an MptBatchAttnArgs, lds_dyn = mpt_batch_attn_lds_dyn.  1: head size not 32 / 64 / 128, or the LDS opt-in failed.
int launch_mpt_batch_attn(hipStream_t stream, const void *args, size_t lds_dyn);
// the quantizer branch of THIS code object's copy of c_act_quant_scalar (kernels/common.h): apply_act_quant sets every copy
int mpt_batch_set_act_quant(int v);
#endif
