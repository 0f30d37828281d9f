// mpt_chunk.h — what the MPT chunk plan (plan_mpt_chunk.inc plan_launch_mpt_chunk; option plan_mpt_chunk) launches that no other plan
// does, all of it compiled into a code object of its own (mpt_chunk.hip, MPT_CHUNK_OBJECT) so that hip_backend.hip's code object holds
// what it held:
//   k_lnorm_quant_cols                                        N rows of ggml's norm x gain -> the Q8 columns k_mmq_cols stages
//   k_mmq_cols<QT, EPI_QKV_TM | EPI_GELU | EPI_ADD_KS>        the cols mat-vec's MPT epilogues and its K-sliced form (kernels/mmq_cols.h)
// hip_backend.hip sees only the launch functions declared at the end of this file.
#pragma once
#include <stddef.h>
#include <stdint.h>
// LDS of launch 2 of the chunk attention for ranges of up to `chunk` keys (a multiple of 64): 32 p rows + the four waves' V staging
static inline int mpt_chunk_attn_row_bytes(size_t chunk) { return (int)(chunk * 2 + 16); }
static inline size_t mpt_chunk_attn_lds(size_t chunk) { return (size_t)32 * mpt_chunk_attn_row_bytes(chunk) + 4 * 2048; }
// one chunk attention (the three launches below); hip_backend.hip fills it, it travels as void *
struct MptChunkAttnArgs {
    const float *q;               // [N] rows, ldq floats apart: the Q columns of the Wqkv product
    int64_t ldq;
    const __half *mem_k, *mem_v;  // [C][E] f16, token-major, one layer
    const void *prm;              // the evaluation's DecParams (n_past is read on the device)
    const float *slopes;
    float scale;
    int N, D, S, f16d;
    int64_t E, C;
    float *sc;    // [H][32][C]
    float *pmax;  // [H][S][32]
    float *part;  // [H][S][32][D]
    float *out;   // [N][E] f32
    int8_t *lo, *hi;
    float *dq;
    int *sumq;
    float *dT;
    int *sT;
    int rb;       // LDS bytes per p row of launch 2
};
#ifdef MPT_CHUNK_OBJECT
#include "mmq_cols.h"

// ---- LayerNorm columns.  One 256-thread workgroup per row; the row (E <= 8192) in registers and in an LDS copy.  The arithmetic is
// k_p_lnorm_quant's (kernels/mpt_prompt.h) and so k_norm's and k_bin<MUL>'s, in their order: both f64 sums as thread t adds elements
// t, t + 256, ... ascending, wave_sum_f64, (s0 + s1) + (s2 + s3); mean = (float)(sum / E); f32 differences, their squares summed in
// f64; y = ((x - mean) * scale) * gain.  Then k_rmsnorm_quant's quantizer (kernels/decode.h: 32 lanes per block, both scale kinds) into
// the planar lo / hi / d / sum rows AND the [block][8] tables of the row's pass of 8 (row r: column r & 7 of table r >> 3), which is
// where k_mmq_cols' LDS-DMA reads them.  The last row's workgroup zeroes the columns behind it in its table.  y_f32 (nullable): the
// normed rows [N][E], the embedding result of the final norm.  Dynamic LDS: E floats.
template <bool F16_D>
__global__ void __launch_bounds__(256) k_lnorm_quant_cols(const float *__restrict__ x, const float *__restrict__ w, float eps, int E, int N,
                                                          float *y_f32, int8_t *lo, int8_t *hi, float *dq, int *sumq, float *dT, int *sT) {
    extern __shared__ __attribute__((aligned(16))) float s_row[];
    __shared__ double s_part[4];
    constexpr int MAXU = 8;
    const int64_t row = blockIdx.x;
    const int tid = threadIdx.x, E4 = E >> 2;
    const f32x4 *xr = (const f32x4 *)(x + row * E);
    const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 v[MAXU], wv[MAXU];
#pragma unroll
    for (int u = 0; u < MAXU; u++) {
        const int j = u * 256 + tid;
        v[u] = j < E4 ? xr[j] : zero4;
        wv[u] = j < E4 ? ((const f32x4 *)w)[j] : zero4;
        if (j < E4) ((f32x4 *)s_row)[j] = v[u];
    }
    __syncthreads();
    double s = 0.0;
    for (int i = tid; i < E; i += 256) s += (double)s_row[i];
    s = wave_sum_f64(s);
    if ((tid & 63) == 0) s_part[tid >> 6] = s;
    __syncthreads();
    const float mean = (float)(((s_part[0] + s_part[1]) + (s_part[2] + s_part[3])) / (double)E);
    double s2 = 0.0;
    for (int i = tid; i < E; i += 256) {
        const float d = s_row[i] - mean;
        s2 += (double)(d * d);
    }
    s2 = wave_sum_f64(s2);
    __syncthreads();  // (s_part and s_row are read no more)
    if ((tid & 63) == 0) s_part[tid >> 6] = s2;
    __syncthreads();
    const float variance = (float)(((s_part[0] + s_part[1]) + (s_part[2] + s_part[3])) / (double)E);
    const float scale = 1.0f / sqrtf(variance + eps);
#pragma unroll
    for (int u = 0; u < MAXU; u++) {
        const int j = u * 256 + tid;
        if (j < E4) {
            f32x4 y;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                float t = (v[u][k] - mean) * scale;
                t = t * wv[u][k];
                y[k] = t;
            }
            ((f32x4 *)s_row)[j] = y;
            if (y_f32) ((f32x4 *)(y_f32 + row * E))[j] = y;
        }
    }
    __syncthreads();
    const int nblk = E >> 5, l = tid & 31;
    lo += row * nblk * 16;
    hi += row * nblk * 16;
    dq += row * nblk;
    sumq += row * nblk;
    const int64_t tbl = (row >> 3) * nblk * 8;
    const int col = (int)(row & 7);
    const int tail0 = (int)row == N - 1 ? col + 1 : 8;  // the table's columns behind the chunk's last row: zeros
    for (int b = tid >> 5; b < nblk; b += 8) {
        const float yv = s_row[b * 32 + l];
        float amax = fabsf(yv);
        amax = g32_max_f32(amax);
        const float d = amax / 127.0f;
        const float id = act_id(amax, d, aq_scalar());
        const int q = act_q(yv * id, aq_scalar());
        int sq = q;
        sq = g32_sum_i32(sq);
        (l < 16 ? lo : hi)[b * 16 + (l & 15)] = (int8_t)q;
        if (l == 0) {
            const float ds = F16_D ? round_f16(d) : d;
            dq[b] = ds;
            sumq[b] = sq;
            dT[tbl + b * 8 + col] = ds;
            sT[tbl + b * 8 + col] = sq;
        }
        if (l >= tail0 && l < 8) {
            dT[tbl + b * 8 + l] = 0.0f;
            sT[tbl + b * 8 + l] = 0;
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// Chunk attention of MPT's graph, split over the positions as well as the heads: grid (H, S), each workgroup a contiguous range of keys
// (mpt_split_range of kernels/mpt_plan.h, restated: multiples of 64 but for the last, derived from prm->n_past + N on the device — one
// captured graph serves every position) and ALL N <= 31 queries of its head as one 32-row tile (rows behind N repeat the last query and
// are never stored), so the head's K and V are read once per chunk, by S CUs.  ggml's rounding points are kept (no online softmax):
// three launches, every dependency a kernel boundary, no workgroup waits inside a launch.
//   1. k_attn_chunk_scores_alibi   S = Q K^T on v_mfma_f32_32x32x16_f16 (A = the 32 queries, B = 32 keys of token-major K: the MFMA's k
//                                  runs along a key's row, 16 bytes a lane), x = fadd(fmul((float)t, slope), fmul(s, scale)); keys behind
//                                  n_past + n are masked for query n -> sc[h][n][t], range maxima -> pmax[h][s][n] (-inf: nothing visible)
//   2. k_attn_chunk_vp_alibi       per query: mx from the S partial maxima, e = f16(exp(f16(x - mx))) and its f64 sum over the WHOLE visible
//                                  row from sc (every e a multiple of 2^-24 in [0, 1]: exact in any order), inv = (float)(1 / sum), the own
//                                  range's p = f16(e * inv) into LDS (masked: 0); then V.P over the range: wave w owns channels 32 w .. of
//                                  the head, V in chunks of 16 keys through a wave-private LDS staging for ds_read_b64_tr_b16 (k_p_attn_alibi's
//                                  staging and lane mapping) -> part[h][s][n][D] (an empty range: zeros, from the same code)
//   3. k_attn_chunk_merge_alibi    out[n][h D + d] = sum over s ascending of part, f32; the row re-quantized to Q8 in the planar AND the
//                                  [block][8] layouts out_proj's k_mmq_cols reads (k_quant_row's quantizer), and the f32 row
// Rows at or behind n_past + N are never read.  Dynamic LDS of launch 2: 32 rows of the longest range's p (2 bytes a key + 16 bytes of
// pitch padding) + 4 x 2 KiB of V staging: mpt_chunk_attn_lds.
// ---------------------------------------------------------------------------------------------------
typedef _Float16 ch_f16x8 __attribute__((ext_vector_type(8)));
typedef float ch_f32x16 __attribute__((ext_vector_type(16)));
typedef short ch_s16x4 __attribute__((ext_vector_type(4)));
typedef short ch_s16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ void chunk_split_range(int T, int S, int s, int &t0, int &t1) {
    const int chunk = (((T + S - 1) / S) + 63) & ~63;
    t0 = s * chunk < T ? s * chunk : T;
    t1 = t0 + chunk < T ? t0 + chunk : T;
}
template <int D>
__global__ void __launch_bounds__(256) k_attn_chunk_scores_alibi(const MptChunkAttnArgs a) {
    __shared__ float s_mx[4][32];
    constexpr int KS = D / 16;
    const int h = blockIdx.x, s = blockIdx.y;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, fr = lane & 31, fh = lane >> 5;
    const int P = ((const DecParams *)a.prm)->n_past, T = P + a.N;
    if (P < 0 || T > a.C) return;  // (never: the plan runs positions inside the context only)
    int t0, t1;
    chunk_split_range(T, a.S, s, t0, t1);
    const float slope = a.slopes[h];
    ch_f16x8 qa[KS];
    {
        const float *qp = a.q + (int64_t)(fr < a.N ? fr : a.N - 1) * a.ldq + (int64_t)h * D + fh * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ks++) {
            const f32x4 x0 = *(const f32x4 *)(qp + ks * 16), x1 = *(const f32x4 *)(qp + ks * 16 + 4);
            qa[ks] = ch_f16x8{(_Float16)x0[0], (_Float16)x0[1], (_Float16)x0[2], (_Float16)x0[3], (_Float16)x1[0], (_Float16)x1[1], (_Float16)x1[2], (_Float16)x1[3]};
        }
    }
    float m[16];
#pragma unroll
    for (int r = 0; r < 16; r++) m[r] = -INFINITY;
    float *sc = a.sc + (int64_t)h * 32 * a.C;
    const int ntile = (t1 - t0 + 31) >> 5;
    const ch_f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int j = wave; j < ntile; j += 4) {  // wave-uniform
        const int t = t0 + 32 * j + fr;
        const bool valid = t < t1;
        const __half *kp = a.mem_k + (int64_t)t * a.E + (int64_t)h * D + fh * 8;
        ch_f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = 0.0f;
#pragma unroll
        for (int ks = 0; ks < KS; ks++) {
            const ch_f16x8 kb = valid ? *(const ch_f16x8 *)(kp + ks * 16) : zero8;
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(qa[ks], kb, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int n = (r & 3) + 8 * (r >> 2) + 4 * fh;
            const float x = __fadd_rn(__fmul_rn((float)t, slope), __fmul_rn(acc[r], a.scale));
            const bool vis = valid && t <= P + n;
            if (vis && n < a.N) sc[(int64_t)n * a.C + t] = x;
            m[r] = vis ? fmaxf(m[r], x) : m[r];
        }
    }
#pragma unroll
    for (int r = 0; r < 16; r++) {
        float v = m[r];
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
        if (fr == 0) s_mx[wave][(r & 3) + 8 * (r >> 2) + 4 * fh] = v;
    }
    __syncthreads();
    if (tid < 32) a.pmax[((int64_t)h * a.S + s) * 32 + tid] = fmaxf(fmaxf(s_mx[0][tid], s_mx[1][tid]), fmaxf(s_mx[2][tid], s_mx[3][tid]));
}

template <int D>
__global__ void __launch_bounds__(256) k_attn_chunk_vp_alibi(const MptChunkAttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int h = blockIdx.x, s = blockIdx.y;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, fr = lane & 31, fh = lane >> 5;
    const int P = ((const DecParams *)a.prm)->n_past, T = P + a.N;
    if (P < 0 || T > a.C) return;
    int t0, t1;
    chunk_split_range(T, a.S, s, t0, t1);
    const int npad = (t1 - t0 + 15) & ~15;  // (<= the range's full length, a multiple of 64: inside the p rows)
    const int rb = a.rb;
    // ---- soft_max of the tile's rows (wave w: rows w, w + 4, ..), the own range's p into LDS ----
    for (int n = wave; n < 32; n += 4) {
        _Float16 *prow = (_Float16 *)(lds + (size_t)n * rb);
        if (n >= a.N) {
            for (int i = lane; i < npad; i += 64) prow[i] = (_Float16)0.0f;
            continue;
        }
        const float *sc = a.sc + ((int64_t)h * 32 + n) * a.C;
        const float *pm = a.pmax + (int64_t)h * a.S * 32 + n;
        float mx = pm[0];
        for (int i = 1; i < a.S; i++) mx = fmaxf(mx, pm[i * 32]);
        const int Tn = P + n + 1;  // the keys query n sees
        double sum = 0.0;
        for (int t = lane; t < Tn; t += 64) sum += (double)round_f16(expf(round_f16(sc[t] - mx)));
        sum = wave_sum_f64(sum);
        const float inv = (float)(1.0 / sum);
        for (int i = lane; i < npad; i += 64) {
            const int t = t0 + i;
            float p = 0.0f;
            if (t < t1 && t < Tn) p = round_f16(expf(round_f16(sc[t] - mx))) * inv;
            prow[i] = (_Float16)p;
        }
    }
    __syncthreads();
    // ---- V.P over the range: wave w owns channels 32 w .. 32 w + 31 of the head ----
    if (wave * 32 >= D) return;
    const int d0 = wave * 32;
    char *vs = lds + (size_t)32 * rb + wave * 2048;  // this wave's two staging buffers
    const int srow = lane >> 2, spc = lane & 3;      // staging: key srow of the chunk, 16-byte piece spc of its 64 bytes
    const __half *vg = a.mem_v + (int64_t)h * D + d0 + spc * 8;
    auto load_v = [&](int c) {
        const int t = t0 + c * 16 + srow;            // rows behind the range may hold anything: zeros instead
        u32x4 v = {0, 0, 0, 0};
        if (t < t1) v = *(const u32x4 *)(vg + (int64_t)t * a.E);
        return v;
    };
    const int li = lane & 15, lg = lane >> 4;
    const int tr_off = (8 * (lg >> 1) + (li >> 2)) * 64 + (16 * (lg & 1) + 4 * (li & 3)) * 2;
    const char *pa = lds + (size_t)fr * rb + fh * 16;
    ch_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.0f;
    const int nch = npad >> 4;
    u32x4 vb = {0, 0, 0, 0};
    if (nch > 0) vb = load_v(0);
    for (int c = 0; c < nch; c++) {
        char *buf = vs + (c & 1) * 1024;
        *(u32x4 *)(buf + lane * 16) = vb;
        if (c + 1 < nch) vb = load_v(c + 1);
        asm volatile("" ::: "memory");  // the reads below take what OTHER lanes of this wave stored above
        const ch_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ch_s16x4 __attribute__((address_space(3))) *)(buf + tr_off));
        const ch_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((ch_s16x4 __attribute__((address_space(3))) *)(buf + tr_off + 256));
        asm volatile("" ::: "memory");
        const ch_s16x8 v8 = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        const ch_f16x8 pf = *(const ch_f16x8 *)(pa + c * 32);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(pf, __builtin_bit_cast(ch_f16x8, v8), acc, 0, 0, 0);
    }
    float *part = a.part + ((int64_t)h * a.S + s) * 32 * D + d0 + fr;
#pragma unroll
    for (int r = 0; r < 16; r++) part[(int64_t)((r & 3) + 8 * (r >> 2) + 4 * fh) * D] = acc[r];
}

// one workgroup per query row: the S partial rows added s ascending, then k_quant_row's quantizer per block of 32 lanes
__global__ void __launch_bounds__(256) k_attn_chunk_merge_alibi(const MptChunkAttnArgs a) {
    const int n = blockIdx.x, tid = threadIdx.x, l = tid & 31;
    const int nblk = (int)(a.E >> 5);
    const int64_t tbl = (int64_t)(n >> 3) * nblk * 8;
    for (int b = tid >> 5; b < nblk; b += 8) {
        const int e = b * 32 + l, h = e / a.D, d = e - h * a.D;
        const float *pp = a.part + ((int64_t)h * a.S * 32 + n) * a.D + d;
        float v = pp[0];
        for (int s = 1; s < a.S; s++) v += pp[(int64_t)s * 32 * a.D];
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
            a.dT[tbl + b * 8 + (n & 7)] = ds;
            a.sT[tbl + b * 8 + (n & 7)] = sq;
        }
    }
}
#else  // hip_backend.hip
// ---- what hip_backend.hip calls (defined in mpt_chunk.hip; ColsArgs is a distinct type in the two objects, same definition: it
// travels as void *) ----
// k_lnorm_quant_cols on N workgroups: rows [N][E] of x, gain w; the Q8 planes and tables of kernels/mpt_chunk.h.  E % 32 == 0, E <= 8192.
void launch_mpt_lnorm_cols(hipStream_t stream, bool f16d, const float *x, const float *w, float eps, int64_t E, int N, float *y_f32, int8_t *lo,
                           int8_t *hi, float *d, int *s, float *dT, int *sT);
// k_mmq_cols<qt, epi> on G workgroups with `lds` bytes (cols_shape's); epi: EPI_QKV_TM, EPI_GELU or EPI_ADD_KS; cols_args: a ColsArgs
// with ngroups / gq / gr set.  1: no such instantiation, or the LDS opt-in failed.
int launch_mpt_cols(hipStream_t stream, int qt, int epi, const void *cols_args, int G, size_t lds);
// The position-split chunk attention (k_attn_chunk_scores_alibi, k_attn_chunk_vp_alibi on H x S workgroups, k_attn_chunk_merge_alibi on N);
// args: an MptChunkAttnArgs (kernels/mpt_chunk.h: it travels as void *), lds = mpt_chunk_attn_lds.  1: head size not 32 / 64 / 128, or the LDS opt-in failed.
int launch_mpt_chunk_attn(hipStream_t stream, const void *args, int H, size_t lds);
// the quantizer branch of THIS code object's copy of c_act_quant_scalar (kernels/common.h): apply_act_quant sets every copy
int mpt_chunk_set_act_quant(int v);
#endif
