// mpt_prompt.h — what the MPT prompt plan (plan_mpt_prompt.inc plan_launch_mpt_prompt; option plan_mpt_prompt) launches between its
// GEMMs, all of it compiled into a code object of its own (mpt_prompt.hip, MPT_PROMPT_OBJECT) so that hip_backend.hip's code object
// holds what it held:
//   k_p_lnorm_quant          [x (+ second partial) + residual -> residual out ->] ggml's norm -> x gain -> Q8 round trip -> f16 operand
//   k_p_qkv_post_tm          the K and V columns of the Wqkv product as f16 rows of the token-major caches (no transpose, no rotation)
//   k_p_attn_alibi<D, QR>    K.Q, scale + ALiBi bias + causal mask + softmax and V.P of a query tile in one launch, scores in LDS
//   k_p_attn_alibi_stream<D> the same launch for rows of any length: three sweeps over the keys, no score row kept (LDS does not grow with T)
//   k_p_gelu_quant           gelu_table (+ second partial) -> Q8 round trip -> f16 operand
// hip_backend.hip sees the argument structure, the fit function and the launch functions at the end of this file.
#pragma once
#include <stdint.h>

// one attention launch: Q is read from the Wqkv product in place (row stride 3 E, columns 0 .. E - 1), K and V from the token-major
// caches of the layer ([C][E] f16 each)
struct MptAttnArgs {
    const float *qkv;     // [N][3 E] f32
    int64_t q_part;       // != 0: the GEMM split K, the second partial lies q_part floats on
    const void *mem_k, *mem_v;
    const float *slopes;  // [H]: alibi_slopes' values
    float *out;           // x16 == nullptr (the test hook): the merged heads [N][E] f32
    _Float16 *x16;        // else out_proj's operand: every 32-channel block of the merged row after its Q8 round trip, in the GEMM's k order
    int N, E, H, n_past, f16d;
    int row_bytes;        // LDS bytes per score row (mpt_attn_row_bytes)
    int r1;               // query-tile ranks dealt longest first; the ranks behind them go shortest first (k_p_attn's rule)
    int64_t C;
    float scale;
};
// LDS of a workgroup: QR score rows (the staged Q tile borrows them) + the V staging, 2 buffers x 16 keys x 64 bytes for each of the
// four waves.  Opted in above 64 KiB; 152 KiB is what the other launches of this library ask the CU's 160 KiB for at most.
#define MPT_ATTN_LDS_MAX ((size_t)152 * 1024)
#define MPT_ATTN_VSTAGE ((size_t)4 * 2 * 16 * 64)
static inline int mpt_attn_row_bytes(int64_t T) { return (int)(((T + 63) & ~(int64_t)63) * 4 + 16); }
static inline size_t mpt_attn_lds(int QR, int64_t D, int64_t T) {
    const size_t row = (size_t)mpt_attn_row_bytes(T), qrow = (size_t)(2 * D + 16);
    return (size_t)QR * (row > qrow ? row : qrow) + MPT_ATTN_VSTAGE;
}
// queries per workgroup for rows of T keys: 32, 16 (long rows), or 0 = no fit (k_p_attn_alibi_stream takes the launch; under option
// mpt_attn_stream = 0 the matcher declines and the executor runs the graph).
// D = 128: 32 up to T = 1088, 16 up to T = 2240.
static inline int mpt_attn_queries(int64_t D, int64_t T) {
    if (!(D == 128 || D == 64 || D == 32) || T < 1) return 0;
    if (mpt_attn_lds(32, D, T) <= MPT_ATTN_LDS_MAX) return 32;
    if (mpt_attn_lds(16, D, T) <= MPT_ATTN_LDS_MAX) return 16;
    return 0;
}
// LDS of a streaming workgroup (static in the kernel: the Q tile, two P buffers of 32 rows x 272 bytes, the V staging, the reduction scratch)
static inline size_t mpt_attn_stream_lds(int64_t D) { return (size_t)32 * (2 * D + 16) + 2 * 32 * 272 + MPT_ATTN_VSTAGE + 4 * 32 * 12; }

#ifdef MPT_PROMPT_OBJECT
#include "mmq.h"
#include "decode.h"
#include "kquant_big.h"
#include "prompt.h"
#include "prompt_attn.h"

// ---- LayerNorm operand.  One 256-thread workgroup per row, the row (E <= 8192) in registers and in an LDS copy, as k_p_norm_quant
// keeps it; both f64 sums take k_norm's order (thread t adds elements t, t + 256, ... ascending; wave_sum_f64; (s0 + s1) + (s2 + s3)),
// so mean, variance and every y = ((x - mean) * scale) * w are k_norm's and k_bin<MUL>'s bits.  ADD: xs = (x [+ x2]) + r first, written
// to xsum.  Dynamic LDS: E floats.
template <bool F16_D, bool ADD>
__global__ void __launch_bounds__(256) k_p_lnorm_quant(const float *__restrict__ x, const float *__restrict__ x2 /*nullable*/,
                                                       const float *__restrict__ r, float *xsum, const float *__restrict__ w, float eps,
                                                       int E, _Float16 *__restrict__ out) {
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
    }
    if constexpr (ADD) {
        if (x2) {  // uniform
            const f32x4 *x2r = (const f32x4 *)(x2 + row * E);
#pragma unroll
            for (int u = 0; u < MAXU; u++) {
                const int j = u * 256 + tid;
                v[u] = v[u] + (j < E4 ? x2r[j] : zero4);
            }
        }
        const f32x4 *rr = (const f32x4 *)(r + row * E);
        f32x4 *xs = (f32x4 *)(xsum + row * E);
#pragma unroll
        for (int u = 0; u < MAXU; u++) {
            const int j = u * 256 + tid;
            v[u] = v[u] + (j < E4 ? rr[j] : zero4);
            if (j < E4) xs[j] = v[u];
        }
    }
#pragma unroll
    for (int u = 0; u < MAXU; u++) {
        const int j = u * 256 + tid;
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
    __syncthreads();
    if ((tid & 63) == 0) s_part[tid >> 6] = s2;
    __syncthreads();
    const float variance = (float)(((s_part[0] + s_part[1]) + (s_part[2] + s_part[3])) / (double)E);
    const float scale = 1.0f / sqrtf(variance + eps);
    _Float16 *orow = out + row * E;
#pragma unroll
    for (int u = 0; u < MAXU; u++) {
        if (u * 256 >= E4) break;  // uniform: whole 8-lane groups take part in the block maximum
        const int j = u * 256 + tid;
        f32x4 y;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            float t = (v[u][k] - mean) * scale;
            t = t * wv[u][k];
            y[k] = t;
        }
        p_requant4_store<F16_D>(y, j, j < E4, orow);
    }
}

// ---- K/V store: columns E .. 3 E - 1 of the Wqkv product [N][3 E] (+ its second partial) as f16 into rows n_past .. n_past + N - 1 of
// the layer's token-major caches; four columns per thread, one 8-byte store.  Q stays where it is.
__global__ void __launch_bounds__(256) k_p_qkv_post_tm(const float *__restrict__ qkv, int64_t part, __half *__restrict__ mem_k,
                                                       __half *__restrict__ mem_v, int N, int E, int n_past) {
    const int per_tok = E >> 1;  // 4-vectors of K and V per token
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)N * per_tok) return;
    const int n = (int)(idx / per_tok), c = 4 * (int)(idx - (int64_t)n * per_tok);  // column E + c
    const float *p = qkv + (int64_t)n * 3 * E + E + c;
    f32x4 v = *(const f32x4 *)p;
    if (part) v = v + *(const f32x4 *)(p + part);
    const bool is_k = c < E;
    __half *dst = (is_k ? mem_k : mem_v) + ((int64_t)n_past + n) * E + (is_k ? c : c - E);
    __half2 h0, h1;
    h0.x = __float2half_rn(v[0]);
    h0.y = __float2half_rn(v[1]);
    h1.x = __float2half_rn(v[2]);
    h1.y = __float2half_rn(v[3]);
    ((__half2 *)dst)[0] = h0;
    ((__half2 *)dst)[1] = h1;
}

// ---- GELU operand: gelu_table of the up_proj product (+ its second partial), four values per lane, then the Q8 round trip
template <bool F16_D>
__global__ void __launch_bounds__(256) k_p_gelu_quant(const f32x4 *__restrict__ a, int64_t n4, int64_t part4, _Float16 *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < n4;
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (valid) {
        f32x4 x = a[i];
        if (part4) x = x + a[i + part4];
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = gelu_table(x[k]);
    }
    p_requant4_store<F16_D>(v, i, valid, out);
}

// ---- the epilogue of both attention kernels (k_p_attn's): a wave's accumulator (NR registers hold real query rows: row (r & 3) +
// 8 (r >> 2) + 4 fh of the tile, column col + fr of the merged row) as f32 merged heads, or as one Q8 block per row after its round trip
template <int NR>
__device__ __forceinline__ void mpt_attn_store(const MptAttnArgs &a, const f32x16 &acc, int q0, int col, int fr, int fh) {
    if (a.x16) {
        _Float16 *xp = a.x16 + (int64_t)(q0 + 4 * fh) * a.E + col + mmq_kperm_inv(fr);
#pragma unroll
        for (int r = 0; r < NR; r++) {
            const int row = (r & 3) + 8 * (r >> 2);
            const float v = acc[r];
            float amax = g16_max_f32(fabsf(v));
            {
                const int ai = __builtin_bit_cast(int, amax);
                const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(ai, 0));
                const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(ai, 16));
                const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(ai, 32));
                const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(ai, 48));
                amax = fh ? fmaxf(r2, r3) : fmaxf(r0, r1);
            }
            const float d = amax / 127.0f;
            const float id = act_id(amax, d, aq_scalar());
            const float dq = a.f16d ? round_f16(d) : d;
            const int qv = act_q(v * id, aq_scalar());
            float rq = dq * (float)qv;
            rq = fminf(fmaxf(rq, -65504.0f), 65504.0f);
            if (q0 + 4 * fh + row < a.N) xp[(int64_t)row * a.E] = (_Float16)rq;
        }
    } else {
        float *op = a.out + (int64_t)(q0 + 4 * fh) * a.E + col + fr;
#pragma unroll
        for (int r = 0; r < NR; r++) {
            const int row = (r & 3) + 8 * (r >> 2);
            if (q0 + 4 * fh + row < a.N) op[(int64_t)row * a.E] = acc[r];
        }
    }
}

// ---- Attention of a prompt batch of MPT's graph (crates/models/mpt/src/lib.rs:153-210) in one launch.  A workgroup of four waves owns
// QR queries of one head and keeps ALL their scores in LDS: ggml's softmax fixes its rounding points (row maximum first,
// e = f16(exp(f16(x - max))), exact f64 sum, p = f16(f32(e * inv))), so this is not an online softmax.
//   S phase   A = queries, B = keys on v_mfma_f32_32x32x16_f16; wave w takes key tiles w, w + 4, ..; token-major K has the MFMA's k
//             dimension (d) contiguous, fragments straight from global / L2, three tiles in flight.  Every score is stored as
//             __fadd_rn(__fmul_rn((float)t, slope), __fmul_rn(s, scale)): k_soft_max<true, true>'s expression, t the key's position.
//   softmax   wave w takes rows QR/4 w ..; all QR rows of LDS hold scores (queries behind N are the last query again), so no row is
//             special; a row sees keys 0 .. min(n_past + its query, T - 1), the columns behind are selected away, never multiplied.
//   V.P       wave w takes channels 32 w .. 32 w + 31 (D / 32 waves).  V is token-major: the MFMA's B operand wants eight consecutive
//             keys of one channel, 2 E bytes apart in memory.  Each wave stages ITS 32 channels of 16 keys through LDS: a lane loads 16
//             bytes of one key's row (four lanes = the 64 contiguous bytes of a key, 16 keys per load instruction, four chunks in flight
//             in registers), writes them to a 1 KiB buffer (two buffers, alternating) and the fragments come back through
//             ds_read_b64_tr_b16.  That instruction, in each group of 16 lanes: lane i receives element (i & 3) of what lanes
//             (i >> 2), 4 + (i >> 2), 8 + (i >> 2), 12 + (i >> 2) addressed.  With lane i of group g addressing key 8 (g >> 1) + (i >> 2),
//             channels 16 (g & 1) + 4 (i & 3) .., a lane gets keys 8 fh .. 8 fh + 3 of channel (lane & 31); a second read four rows on
//             gives keys + 4 .. + 7: the B fragment whose k slot j is key 8 fh + j, the slot the P fragment read from the score row has.
//             The staging is wave-private (LDS operations of a wave execute in order), so the loop has no workgroup barrier.  Rows of
//             64 bytes need no padding: a staging write is 1 KiB contiguous, and the 32 lanes of a transposed read cover four rows x 64
//             bytes = 256 contiguous bytes, every bank once.
//   epilogue  k_p_attn's: a wave's 32 channels are one Q8 block of the merged row.
// grid = ceil(N / QR) * H, 256 threads, dynamic LDS mpt_attn_lds(QR, D, n_past + N).
typedef short s16x4_t __attribute__((ext_vector_type(4)));
template <int D, int QR>
__global__ void __launch_bounds__(256, 2) k_p_attn_alibi(const MptAttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    constexpr int KS = D / 16, NWV = D / 32;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 31, fh = lane >> 5;
    const int ntile = (a.N + QR - 1) / QR;
    const int h = (int)blockIdx.x % a.H, rank = (int)blockIdx.x / a.H;
    const int qt = rank < a.r1 ? ntile - 1 - rank : rank - a.r1;
    const int q0 = qt * QR;
    const int Ttot = a.n_past + a.N;
    const int T_hi = min(a.n_past + q0 + QR, Ttot);  // keys 0 .. T_hi - 1 are visible to some query of the tile
    const int nkt = (T_hi + 31) >> 5;
    const int rb = a.row_bytes;
    const float slope = a.slopes[h];
    const __half *mem_k = (const __half *)a.mem_k, *mem_v = (const __half *)a.mem_v;

    auto load_k = [&](int kt, f16x8(&kb)[KS]) {
        const int64_t t = min((int64_t)kt * 32 + fr, a.C - 1);
        const __half *kp = mem_k + t * a.E + h * D + fh * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ks++) kb[ks] = *(const f16x8 *)(kp + ks * 16);
    };
    constexpr int KR = 3;
    f16x8 kb[KR][KS];
#pragma unroll
    for (int j = 0; j < KR - 1; j++)
        if (wave + 4 * j < nkt) load_k(wave + 4 * j, kb[j]);
    // ---- Q tile -> LDS once per workgroup as f16 (the score rows are not in use yet), every wave's A fragments from there
    constexpr int QROW = D * 2 + 16;
    char *s_q = lds;
    for (int idx = tid; idx < QR * (D / 16); idx += 256) {
        const int row = idx / (D / 16), c = idx % (D / 16);
        const int qn = min(q0 + row, a.N - 1);
        const float *qp = a.qkv + (int64_t)qn * 3 * a.E + h * D + c * 16;
        f32x4_u x[4];
#pragma unroll
        for (int k = 0; k < 4; k++) x[k] = *(const f32x4_u *)(qp + 4 * k);
        if (a.q_part) {  // uniform
#pragma unroll
            for (int k = 0; k < 4; k++) x[k] = x[k] + *(const f32x4_u *)(qp + a.q_part + 4 * k);
        }
        f16x8 h0, h1;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            h0[e] = (_Float16)x[0][e];
            h0[4 + e] = (_Float16)x[1][e];
            h1[e] = (_Float16)x[2][e];
            h1[4 + e] = (_Float16)x[3][e];
        }
        *(f16x8 *)(s_q + row * QROW + c * 32) = h0;
        *(f16x8 *)(s_q + row * QROW + c * 32 + 16) = h1;
    }
    __syncthreads();
    f16x8 qa[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ks++) qa[ks] = *(const f16x8 *)(s_q + (fr & (QR - 1)) * QROW + (fh * 8 + ks * 16) * 2);
    __syncthreads();  // the fragments are in registers: the S phase may overwrite the staging area
    // ---- S phase
    for (int kt0 = wave; kt0 < nkt; kt0 += 4 * KR) {
#pragma unroll
        for (int j = 0; j < KR; j++) {
            const int kt = kt0 + 4 * j;
            if (kt < nkt) {  // wave-uniform
                if (kt + 4 * (KR - 1) < nkt) load_k(kt + 4 * (KR - 1), kb[(j + KR - 1) % KR]);
                f32x16 acc;
#pragma unroll
                for (int r = 0; r < 16; r++) acc[r] = 0.0f;
#pragma unroll
                for (int ks = 0; ks < KS; ks++) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(qa[ks], kb[j][ks], acc, 0, 0, 0);
                const float bias = __fmul_rn((float)(kt * 32 + fr), slope);
                float *sp = (float *)(lds + 4 * fh * rb) + kt * 32 + fr;
#pragma unroll
                for (int r = 0; r < 16; r++)  // row (r & 3) + 8 (r >> 2) + 4 fh: below 16 exactly for r < 8
                    if (QR == 32 || r < 8) *(float *)((char *)sp + ((r & 3) + 8 * (r >> 2)) * rb) = __fadd_rn(bias, __fmul_rn(acc[r], a.scale));
            }
        }
    }
    __syncthreads();
    // ---- softmax, the wave's rows side by side; each row is then overwritten in place with its f16 probabilities
    const int npad = ((T_hi + 15) >> 4) << 4;  // V.P reads whole 16-key chunks: zeros behind the last visible key
    {
        constexpr int RW = QR / 4;
        const int row0 = wave * RW;
        const int lim0 = a.n_past + q0 + row0;
        const int lim_hi = min(lim0 + RW - 1, Ttot - 1);
        char *rp[RW];
        int lim[RW];
#pragma unroll
        for (int rr = 0; rr < RW; rr++) {
            rp[rr] = lds + (row0 + rr) * rb;
            lim[rr] = min(lim0 + rr, Ttot - 1);
        }
        float mx[RW];
#pragma unroll
        for (int rr = 0; rr < RW; rr++) mx[rr] = -INFINITY;
        for (int i = lane; i <= lim_hi; i += 64) {
            float x[RW];
#pragma unroll
            for (int rr = 0; rr < RW; rr++) x[rr] = ((const float *)rp[rr])[i];
#pragma unroll
            for (int rr = 0; rr < RW; rr++) mx[rr] = i <= lim[rr] ? fmaxf(mx[rr], x[rr]) : mx[rr];
        }
#pragma unroll
        for (int rr = 0; rr < RW; rr++) mx[rr] = wave_max_f32(mx[rr]);
        double sum[RW];
#pragma unroll
        for (int rr = 0; rr < RW; rr++) sum[rr] = 0.0;
        for (int i = lane; i <= lim_hi; i += 64) {
            float x[RW], e[RW];
#pragma unroll
            for (int rr = 0; rr < RW; rr++) x[rr] = ((const float *)rp[rr])[i];
#pragma unroll
            for (int rr = 0; rr < RW; rr++) e[rr] = round_f16(exp_le0(round_f16(x[rr] - mx[rr])));
#pragma unroll
            for (int rr = 0; rr < RW; rr++) {
                sum[rr] += (double)(i <= lim[rr] ? e[rr] : 0.0f);
                ((float *)rp[rr])[i] = e[rr];  // (a masked column's value is replaced by zero below without being read)
            }
        }
        float inv[RW];
#pragma unroll
        for (int rr = 0; rr < RW; rr++) {
            sum[rr] = wave_sum_f64(sum[rr]);
            inv[rr] = (float)(1.0 / sum[rr]);
        }
        // f16 element i lands on f32 element i / 2, which this wave has read in this or an earlier iteration
        for (int i0 = 0; i0 < npad; i0 += 64) {
            const int i = i0 + lane;
            float x[RW];
#pragma unroll
            for (int rr = 0; rr < RW; rr++) x[rr] = ((const float *)rp[rr])[min(i, npad - 1)];
            _Float16 pr[RW];
#pragma unroll
            for (int rr = 0; rr < RW; rr++) pr[rr] = f16_of_f32_product(i <= lim[rr] ? x[rr] : 0.0f, inv[rr]);
            if (i < npad) {
#pragma unroll
                for (int rr = 0; rr < RW; rr++) ((_Float16 *)rp[rr])[i] = pr[rr];
            }
        }
    }
    __syncthreads();
    // ---- V.P
    if (wave < NWV) {
        const int nch = npad >> 4;
        const int d0 = wave * 32;
        char *vs = lds + (size_t)QR * rb + wave * 2048;   // this wave's two staging buffers (the launcher's rows are >= the Q rows)
        const int srow = lane >> 2, spc = lane & 3;        // staging: key srow of the chunk, 16-byte piece spc of its 64 bytes
        const __half *vg = mem_v + h * D + d0 + spc * 8;
        auto load_v = [&](int c) {
            const int t = c * 16 + srow;                   // rows behind the last written key may hold anything: zeros instead
            u32x4 v = {0, 0, 0, 0};
            if (t < Ttot) v = *(const u32x4 *)(vg + (int64_t)t * a.E);
            return v;
        };
        const int li = lane & 15, lg = lane >> 4;
        const int tr_off = (8 * (lg >> 1) + (li >> 2)) * 64 + (16 * (lg & 1) + 4 * (li & 3)) * 2;
        const char *pa = lds + (fr & (QR - 1)) * rb + fh * 16;
        constexpr int NR = QR / 2;  // accumulator registers that hold real query rows
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = 0.0f;
        constexpr int PF = 4;  // chunks in flight
        u32x4 vb[PF];
#pragma unroll
        for (int k = 0; k < PF; k++)
            if (k < nch) vb[k] = load_v(k);
        for (int c0 = 0; c0 < nch; c0 += PF) {
#pragma unroll
            for (int k = 0; k < PF; k++) {
                const int c = c0 + k;
                if (c < nch) {  // wave-uniform
                    char *buf = vs + (c & 1) * 1024;
                    *(u32x4 *)(buf + lane * 16) = vb[k];
                    if (c + PF < nch) vb[k] = load_v(c + PF);
                    asm volatile("" ::: "memory");  // the reads below take what OTHER lanes of this wave stored above
                    const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4_t __attribute__((address_space(3))) *)(buf + tr_off));
                    const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4_t __attribute__((address_space(3))) *)(buf + tr_off + 256));
                    asm volatile("" ::: "memory");
                    typedef short s16x8_t __attribute__((ext_vector_type(8)));
                    const s16x8_t v8 = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    const f16x8 pf = *(const f16x8 *)(pa + c * 32);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(pf, __builtin_bit_cast(f16x8, v8), acc, 0, 0, 0);
                }
            }
        }
        mpt_attn_store<NR>(a, acc, q0, h * D + d0, fr, fh);
    }
}

// ---- The streaming form of that launch, for rows behind the LDS fit (any T): no score row is kept.  The rounding points above need the
// row maximum before the first e and the row sum before the first p, and a one-pass online softmax cannot have them; recomputing S can:
// the same MFMA chain on the same fragments gives the same bits every time.  So the workgroup (32 queries of one head, four waves, the
// same grid and dealing) sweeps the tile's visible keys three times:
//   sweep 1   wave w takes key tiles w, w + 4, .. as the S phase above; a lane keeps the running maximum of each of its 16 accumulator
//             rows (masked columns selected away), the 32 lanes of a row are reduced once at the end, the four waves through s_mx.  A
//             maximum does not depend on the order.
//   sweep 2   the same tiles; e = f16(exp(f16(x - max))) as above, f64 partial sums per lane, reduced the same way through s_sum.  Every
//             term is a multiple of 2^-24 not above 1, so an f64 sum of up to 2^29 of them is exact in any order: the sum, and so
//             inv = (float)(1 / sum), are k_p_attn_alibi's bits.
//   sweep 3   in blocks of 128 keys: wave w recomputes the S tile of keys 128 b + 32 w .., forms p = f16(f32(masked e * inv)) and writes
//             it as f16 into the block's P buffer (32 rows x 128 keys; the row pitch of 272 bytes puts the 16-byte A-fragment reads of 32
//             rows on distinct banks, as the Q tile's pitch does).  Behind ONE workgroup barrier the waves < D / 32 run the block's eight
//             16-key chunks of V.P from it: the staging, the transposed reads, the chunk order (ascending up to npad) and the accumulator
//             are those above, so the accumulation is the same chain.  Two P buffers: a wave that is through with block b computes the
//             S tile of block b + 1 while the others still read block b's; buffer b & 1 is written again only behind barrier b + 1,
//             which every wave passes after its V.P of block b.
// LDS does not grow with T: the Q tile + two P buffers (17 KiB) + the V staging (8 KiB) + 1.5 KiB of reduction scratch = 35 KiB at
// D = 128, static, below the 64 KiB default.  The price is the S phase three times (K three times from L2): paid only where the
// alternative is the executor (or where option mpt_attn_stream = 2 asks for it).  grid = ceil(N / 32) * H, 256 threads.
#define MPT_STREAM_PPITCH (128 * 2 + 16)
static_assert(MPT_STREAM_PPITCH % 16 == 0, "the A-fragment reads are 16-byte reads");
__device__ __forceinline__ double g32_sum_f64(double v) {
    v += dpp_f64<DPP_QUAD_XOR1>(v);
    v += dpp_f64<DPP_QUAD_XOR2>(v);
    v += dpp_f64<DPP_ROW_HALF_MIRROR>(v);
    v += dpp_f64<DPP_ROW_MIRROR>(v);
    return v + __shfl_xor(v, 16, 64);
}
template <int D>
__global__ void __launch_bounds__(256, 2) k_p_attn_alibi_stream(const MptAttnArgs a) {
    constexpr int QR = 32, KS = D / 16, NWV = D / 32, QROW = D * 2 + 16, PP = MPT_STREAM_PPITCH;
    __shared__ __attribute__((aligned(16))) char s_q[QR * QROW];
    __shared__ __attribute__((aligned(16))) char s_p[2][QR * PP];
    __shared__ __attribute__((aligned(16))) char s_v[MPT_ATTN_VSTAGE];
    __shared__ double s_sum[4][QR];
    __shared__ float s_mx[4][QR];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 31, fh = lane >> 5;
    const int ntile = (a.N + QR - 1) / QR;
    const int h = (int)blockIdx.x % a.H, rank = (int)blockIdx.x / a.H;
    const int qt = rank < a.r1 ? ntile - 1 - rank : rank - a.r1;
    const int q0 = qt * QR;
    const int Ttot = a.n_past + a.N;
    const int T_hi = min(a.n_past + q0 + QR, Ttot);
    const int nkt = (T_hi + 31) >> 5;
    const int npad = ((T_hi + 15) >> 4) << 4;
    const float slope = a.slopes[h];
    const __half *mem_k = (const __half *)a.mem_k, *mem_v = (const __half *)a.mem_v;

    // ---- Q tile -> LDS as f16, every wave's A fragments from there (queries behind N are the last query again)
    for (int idx = tid; idx < QR * (D / 16); idx += 256) {
        const int row = idx / (D / 16), c = idx % (D / 16);
        const int qn = min(q0 + row, a.N - 1);
        const float *qp = a.qkv + (int64_t)qn * 3 * a.E + h * D + c * 16;
        f32x4_u x[4];
#pragma unroll
        for (int k = 0; k < 4; k++) x[k] = *(const f32x4_u *)(qp + 4 * k);
        if (a.q_part) {  // uniform
#pragma unroll
            for (int k = 0; k < 4; k++) x[k] = x[k] + *(const f32x4_u *)(qp + a.q_part + 4 * k);
        }
        f16x8 h0, h1;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            h0[e] = (_Float16)x[0][e];
            h0[4 + e] = (_Float16)x[1][e];
            h1[e] = (_Float16)x[2][e];
            h1[4 + e] = (_Float16)x[3][e];
        }
        *(f16x8 *)(s_q + row * QROW + c * 32) = h0;
        *(f16x8 *)(s_q + row * QROW + c * 32 + 16) = h1;
    }
    __syncthreads();
    f16x8 qa[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ks++) qa[ks] = *(const f16x8 *)(s_q + fr * QROW + (fh * 8 + ks * 16) * 2);

    auto load_k = [&](int kt, f16x8(&kb)[KS]) {
        const int64_t t = min((int64_t)kt * 32 + fr, a.C - 1);
        const __half *kp = mem_k + t * a.E + h * D + fh * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ks++) kb[ks] = *(const f16x8 *)(kp + ks * 16);
    };
    // the scores of key tile kt, accumulator register r = query row (r & 3) + 8 (r >> 2) + 4 fh, key kt * 32 + fr
    auto scores = [&](int kt, const f16x8(&kb)[KS], float(&x)[16]) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = 0.0f;
#pragma unroll
        for (int ks = 0; ks < KS; ks++) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(qa[ks], kb[ks], acc, 0, 0, 0);
        const float bias = __fmul_rn((float)(kt * 32 + fr), slope);
#pragma unroll
        for (int r = 0; r < 16; r++) x[r] = __fadd_rn(bias, __fmul_rn(acc[r], a.scale));
    };
    // register r's row sees key t: t <= min(n_past + its query, T - 1)
    const int lim0 = a.n_past + q0 + 4 * fh;
    auto visible = [&](int t, int r) { return t < Ttot && t - lim0 <= (r & 3) + 8 * (r >> 2); };
    // the wave's key tiles w, w + 4, .., three in flight: use(key of this lane, its 16 scores)
    auto sweep = [&](auto &&use) {
        constexpr int KR = 3;
        f16x8 kb[KR][KS];
#pragma unroll
        for (int j = 0; j < KR - 1; j++)
            if (wave + 4 * j < nkt) load_k(wave + 4 * j, kb[j]);
        for (int kt0 = wave; kt0 < nkt; kt0 += 4 * KR) {
#pragma unroll
            for (int j = 0; j < KR; j++) {
                const int kt = kt0 + 4 * j;
                if (kt < nkt) {  // wave-uniform
                    if (kt + 4 * (KR - 1) < nkt) load_k(kt + 4 * (KR - 1), kb[(j + KR - 1) % KR]);
                    float x[16];
                    scores(kt, kb[j], x);
                    use(kt * 32 + fr, x);
                }
            }
        }
    };
    // ---- sweep 1: row maxima
    float mx[16];
#pragma unroll
    for (int r = 0; r < 16; r++) mx[r] = -INFINITY;
    sweep([&](int t, const float(&x)[16]) {
#pragma unroll
        for (int r = 0; r < 16; r++) mx[r] = visible(t, r) ? fmaxf(mx[r], x[r]) : mx[r];
    });
#pragma unroll
    for (int r = 0; r < 16; r++) {
        mx[r] = g32_max_f32(mx[r]);
        if (fr == 0) s_mx[wave][(r & 3) + 8 * (r >> 2) + 4 * fh] = mx[r];
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * fh;
        mx[r] = fmaxf(fmaxf(s_mx[0][row], s_mx[1][row]), fmaxf(s_mx[2][row], s_mx[3][row]));
    }
    // ---- sweep 2: row sums
    float inv[16];
    {
        double sum[16];
#pragma unroll
        for (int r = 0; r < 16; r++) sum[r] = 0.0;
        sweep([&](int t, const float(&x)[16]) {
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const float e = round_f16(exp_le0(round_f16(x[r] - mx[r])));
                sum[r] += (double)(visible(t, r) ? e : 0.0f);
            }
        });
#pragma unroll
        for (int r = 0; r < 16; r++) {
            sum[r] = g32_sum_f64(sum[r]);
            if (fr == 0) s_sum[wave][(r & 3) + 8 * (r >> 2) + 4 * fh] = sum[r];
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int row = (r & 3) + 8 * (r >> 2) + 4 * fh;
            inv[r] = (float)(1.0 / ((s_sum[0][row] + s_sum[1][row]) + (s_sum[2][row] + s_sum[3][row])));
        }
    }
    // ---- sweep 3: P block by block, V.P behind it
    const int nch = npad >> 4, nblk = (nch + 7) >> 3;
    const int d0 = wave * 32;
    char *vs = s_v + wave * 2048;                      // this wave's two staging buffers
    const int srow = lane >> 2, spc = lane & 3;        // staging: key srow of the chunk, 16-byte piece spc of its 64 bytes
    const __half *vg = mem_v + h * D + (wave < NWV ? d0 : 0) + spc * 8;
    auto load_v = [&](int c) {
        const int t = c * 16 + srow;                   // rows behind the last written key may hold anything: zeros instead
        u32x4 v = {0, 0, 0, 0};
        if (t < Ttot) v = *(const u32x4 *)(vg + (int64_t)t * a.E);
        return v;
    };
    const int li = lane & 15, lg = lane >> 4;
    const int tr_off = (8 * (lg >> 1) + (li >> 2)) * 64 + (16 * (lg & 1) + 4 * (li & 3)) * 2;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = 0.0f;
    constexpr int PF = 4;  // V chunks in flight
    u32x4 vb[PF];
    if (wave < NWV) {
#pragma unroll
        for (int k = 0; k < PF; k++)
            if (k < nch) vb[k] = load_v(k);
    }
    f16x8 kc[2][KS];  // this block's K tile and the next one's
    if (wave * 32 < npad) load_k(wave, kc[0]);
    for (int b0 = 0; b0 < nblk; b0 += 2) {
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int b = b0 + j;
            if (b < nblk) {  // uniform over the workgroup
                const int kt = 4 * b + wave;
                if (kt * 32 < npad) {  // wave-uniform; a tile wholly behind npad is read by no chunk
                    if ((kt + 4) * 32 < npad) load_k(kt + 4, kc[j ^ 1]);
                    float x[16];
                    scores(kt, kc[j], x);
                    const int t = kt * 32 + fr;
                    char *pp = s_p[j] + 4 * fh * PP + (wave * 32 + fr) * 2;
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const float e = round_f16(exp_le0(round_f16(x[r] - mx[r])));
                        *(_Float16 *)(pp + ((r & 3) + 8 * (r >> 2)) * PP) = f16_of_f32_product(visible(t, r) ? e : 0.0f, inv[r]);
                    }
                }
                __syncthreads();
                if (wave < NWV) {
                    const char *pa = s_p[j] + fr * PP + fh * 16;
#pragma unroll
                    for (int k = 0; k < 8; k++) {
                        const int c = 8 * b + k;
                        if (c < nch) {  // wave-uniform
                            char *buf = vs + (k & 1) * 1024;
                            *(u32x4 *)(buf + lane * 16) = vb[k % PF];
                            if (c + PF < nch) vb[k % PF] = load_v(c + PF);
                            asm volatile("" ::: "memory");  // the reads below take what OTHER lanes of this wave stored above
                            const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4_t __attribute__((address_space(3))) *)(buf + tr_off));
                            const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4_t __attribute__((address_space(3))) *)(buf + tr_off + 256));
                            asm volatile("" ::: "memory");
                            typedef short s16x8_t __attribute__((ext_vector_type(8)));
                            const s16x8_t v8 = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                            const f16x8 pf = *(const f16x8 *)(pa + k * 32);
                            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(pf, __builtin_bit_cast(f16x8, v8), acc, 0, 0, 0);
                        }
                    }
                }
            }
        }
    }
    if (wave < NWV) mpt_attn_store<16>(a, acc, q0, h * D + d0, fr, fh);
}
#else  // hip_backend.hip
// ---- what hip_backend.hip calls (defined in mpt_prompt.hip) ----
// k_p_lnorm_quant over N rows of E <= 8192 elements; r != nullptr: xsum = (x [+ x2]) + r is written and normed
void launch_mpt_lnorm_quant(hipStream_t stream, int f16d, const float *x, const float *x2, const float *r, float *xsum, const float *w, float eps,
                            int64_t E, int64_t N, _Float16 *out);
void launch_mpt_qkv_post_tm(hipStream_t stream, const float *qkv, int64_t part, void *mem_k, void *mem_v, int N, int64_t E, int n_past);
void launch_mpt_gelu_quant(hipStream_t stream, int f16d, const float *a, int64_t n4, int64_t part4, _Float16 *out);
// k_p_attn_alibi<D, QR> on `grid` workgroups with `lds` bytes; args: a MptAttnArgs (a distinct type in the two objects, same definition:
// it travels as void *); 1: no such instantiation, or the LDS opt-in failed
int launch_mpt_attn_alibi(hipStream_t stream, int D, int QR, const void *args, unsigned grid, size_t lds);
// k_p_attn_alibi_stream<D> on `grid` = ceil(N / 32) * H workgroups (static LDS; args.row_bytes is not read); 1: no such instantiation
int launch_mpt_attn_alibi_stream(hipStream_t stream, int D, const void *args, unsigned grid);
// the quantizer branch of THIS code object's copy of c_act_quant_scalar (kernels/common.h)
int mpt_prompt_set_act_quant(int v);
#endif
