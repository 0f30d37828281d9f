// flash_attn.h — GGML_OP_FLASH_ATTN (ggml_flash_attn, include/ggml_hip.h): attention as ONE graph node and one launch,
//   out[b][h][i][:] = sum_j softmax_j(scale * q_i . k_j)  v[:, j]        q [D, N, H, B], k [D, M, Hkv, B], v [M, D, Hkv, B] (transposed)
// with scale = 1 / sqrtf(D), P = M - N, `masked`: query i sees keys j <= P + i.  nb[0] of the operands is dense, every other
// stride is free (permuted views, views into a larger K/V cache).  ggml's softmax fixes its rounding points, as for soft_max:
//   s = f32(dot * scale); row max over the kept keys; arg = f16(f32(s - max)); e = f16(exp(arg)) (exp_le0); the sum of e exact
//   (f64); inv = f32(1 / sum); p = f32(e * inv); f16 K/V: p -> f16, f32 K/V: p stays f32; out = sum v * p in f32
// so neither kernel is an online softmax: the scores of a row are all held in LDS before the row's maximum is taken.  A key
// that is dropped (masked, or at / beyond M) is never read into a result: its column is SELECTED to zero, not multiplied.
//
//   k_flash_attn_tile<D, QR>: f16 K/V, D in {32, 64, 128}, 16-byte aligned K and V rows.  k_p_attn's structure (prompt_attn.h)
//       with every address taken through nb[1..3], a `masked` switch and the batch in blockIdx: QR = 32 (16 for long rows)
//       queries of one (h, b) per workgroup, their scores in LDS, both products on v_mfma_f32_32x32x16_f16 with ascending k.
//   k_flash_attn_row<KV16>: one workgroup per (i, h, b): decode (N == 1), every f32 graph, every other head size, every
//       layout the tile kernel's 16-byte loads cannot take.  The row's scores in LDS, dot products on the VALU.
// The launcher (backend_ops.inc op_flash_attn) chooses; the limits are FLASH_ATTN_* in internal.h.
#pragma once
#include "prompt_attn.h"

struct FlashAttnArgs {
    const char *q, *k, *v;  // first element of each view
    float *out;             // [B][H][N][D] f32, contiguous
    int64_t q_nb1, q_nb2, q_nb3, k_nb1, k_nb2, k_nb3, v_nb1, v_nb2, v_nb3;
    int D, N, M, H, B;
    int r;          // query heads per K/V head
    int P;          // M - N
    int masked;
    int q16;        // q holds f16 (else f32)
    int kvec, vvec; // row kernel: K rows / V rows may be read 16 bytes at a time (base and strides are multiples of 16)
    float scale;
    int row_bytes;  // tile kernel: LDS bytes per score row
};

typedef _Float16 f16x8_u __attribute__((ext_vector_type(8), aligned(2)));

template <int D, int QR>
__global__ void __launch_bounds__(256, 2) k_flash_attn_tile(const FlashAttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    constexpr int KS = D / 16;   // MFMA k steps of a K.Q tile
    constexpr int NWV = D / 32;  // waves that take part in V.P
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fr = lane & 31, fh = lane >> 5;
    const int ntile = (a.N + QR - 1) / QR;
    // blockIdx = h + H * (rank + ntile * b); the longest rows of a (masked) batch first
    const int h = (int)blockIdx.x % a.H, rest = (int)blockIdx.x / a.H;
    const int qt = ntile - 1 - rest % ntile, b = rest / ntile;
    const int hk = h / a.r;
    const int q0 = qt * QR;
    const int M = a.M;
    const int mstep = a.masked ? 1 : 0;                              // row i sees keys 0 .. (masked ? P + i : M - 1)
    const int T_hi = a.masked ? min(a.P + q0 + QR, M) : M;           // keys 0 .. T_hi - 1 are visible to some query of the tile
    const int nkt = (T_hi + 31) >> 5;
    const int rb = a.row_bytes;
    const char *kbase = a.k + (int64_t)hk * a.k_nb2 + (int64_t)b * a.k_nb3 + fh * 16;
    const char *vbase = a.v + (int64_t)hk * a.v_nb2 + (int64_t)b * a.v_nb3;
    const char *qbase = a.q + (int64_t)h * a.q_nb2 + (int64_t)b * a.q_nb3;

    auto load_k = [&](int kt, f16x8 (&kb)[KS]) {
        const int64_t t = min(kt * 32 + fr, M - 1);  // a row at or beyond M is never read: its column repeats key M - 1 and is dropped
        const char *kp = kbase + t * a.k_nb1;
#pragma unroll
        for (int ks = 0; ks < KS; ks++) kb[ks] = *(const f16x8 *)(kp + ks * 32);
    };
    constexpr int KR = 3;
    f16x8 kb[KR][KS];
#pragma unroll
    for (int j = 0; j < KR - 1; j++)
        if (wave + 4 * j < nkt) load_k(wave + 4 * j, kb[j]);
    // ---- Q tile -> LDS once per workgroup as f16 (an f32 q is rounded here, as mul_mat rounds its src1)
    constexpr int QROW = D * 2 + 16;  // bytes per staged row (+16: fragment reads of consecutive rows spread over the banks)
    char *s_q = lds;  // the score rows are not in use yet (32 x QROW <= 32 x row_bytes: row_bytes >= 272)
    for (int idx = tid; idx < QR * (D / 16); idx += 256) {
        const int row = idx / (D / 16), c = idx % (D / 16);
        const int qn = min(q0 + row, a.N - 1);
        const char *qp = qbase + (int64_t)qn * a.q_nb1;
        f16x8 h0, h1;
        if (a.q16) {  // uniform
            h0 = *(const f16x8_u *)(qp + c * 32);
            h1 = *(const f16x8_u *)(qp + c * 32 + 16);
        } else {
            f32x4_u x[4];
#pragma unroll
            for (int k = 0; k < 4; k++) x[k] = *(const f32x4_u *)(qp + c * 64 + 16 * k);
#pragma unroll
            for (int e = 0; e < 4; e++) {
                h0[e] = (_Float16)x[0][e];
                h0[4 + e] = (_Float16)x[1][e];
                h1[e] = (_Float16)x[2][e];
                h1[4 + e] = (_Float16)x[3][e];
            }
        }
        *(f16x8 *)(s_q + row * QROW + c * 32) = h0;
        *(f16x8 *)(s_q + row * QROW + c * 32 + 16) = h1;
    }
    __syncthreads();
    f16x8 qa[KS];  // A operand: row fr of the tile, 8 channels per k step and lane half
#pragma unroll
    for (int ks = 0; ks < KS; ks++) qa[ks] = *(const f16x8 *)(s_q + (fr & (QR - 1)) * QROW + (fh * 8 + ks * 16) * 2);
    __syncthreads();  // the fragments are in registers: the S phase may overwrite the staging area
    // ---- S phase: wave w takes key tiles w, w + 4, ...; K fragments of up to three of them in flight
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
                float *sp = (float *)(lds + 4 * fh * rb) + kt * 32 + fr;
#pragma unroll
                for (int r = 0; r < 16; r++)  // row (r & 3) + 8 (r >> 2) + 4 fh: below 16 exactly for r < 8
                    if (QR == 32 || r < 8) *(float *)((char *)sp + ((r & 3) + 8 * (r >> 2)) * rb) = acc[r];
            }
        }
    }
    __syncthreads();
    // ---- softmax: k_p_attn's, row by row (wave w takes rows RW w .. RW w + RW - 1 side by side); each row is then overwritten
    // with its f16 probabilities.  Row rr of the wave sees keys 0 .. lim0 + rr * mstep.
    const int npad = ((T_hi + 15) >> 4) << 4;  // V.P reads whole 16-key chunks: zeros behind the last visible key
    {
        constexpr int RW = QR / 4;
        const int row0 = wave * RW;
        const int nrow = min(RW, a.N - q0 - row0);  // rows of this wave that exist (ragged last tile), wave-uniform, may be <= 0
        const int lim0 = a.masked ? a.P + q0 + row0 : M - 1;
        const int lim_hi = lim0 + (nrow - 1) * mstep;  // nrow <= 0: the loops below do nothing that is kept
        // rows that do not exist alias the wave's first row for their reads and never write
        const char *rp[RW];
#pragma unroll
        for (int rr = 0; rr < RW; rr++) rp[rr] = lds + (row0 + (rr < nrow ? rr : 0)) * rb;
        if (nrow > 0) {
            float mx[RW];
#pragma unroll
            for (int rr = 0; rr < RW; rr++) mx[rr] = -INFINITY;
            for (int i = lane; i <= lim_hi; i += 64) {
                float x[RW];
#pragma unroll
                for (int rr = 0; rr < RW; rr++) x[rr] = ((const float *)rp[rr])[i];
#pragma unroll
                for (int rr = 0; rr < RW; rr++) {
                    const float v = x[rr] * a.scale;
                    mx[rr] = (rr < nrow && i <= lim0 + rr * mstep) ? fmaxf(mx[rr], v) : mx[rr];
                }
            }
#pragma unroll
            for (int rr = 0; rr < RW; rr++) mx[rr] = wave_max_f32(mx[rr]);
            double sum[RW];
#pragma unroll
            for (int rr = 0; rr < RW; rr++) sum[rr] = 0.0;
            // a dropped column's value (possibly NaN) is selected away from the sum and never stored
            for (int i = lane; i <= lim_hi; i += 64) {
                float x[RW], e[RW];
#pragma unroll
                for (int rr = 0; rr < RW; rr++) x[rr] = ((const float *)rp[rr])[i];
#pragma unroll
                for (int rr = 0; rr < RW; rr++) e[rr] = round_f16(exp_le0(round_f16(x[rr] * a.scale - mx[rr])));
#pragma unroll
                for (int rr = 0; rr < RW; rr++)
                    if (rr < nrow && i <= lim0 + rr * mstep) {
                        sum[rr] += (double)e[rr];
                        ((float *)(lds + (row0 + rr) * rb))[i] = e[rr];
                    }
            }
            float inv[RW];
#pragma unroll
            for (int rr = 0; rr < RW; rr++) {
                sum[rr] = wave_sum_f64(sum[rr]);
                inv[rr] = (float)(1.0 / sum[rr]);
            }
            // f16 element i lands on f32 element i / 2, which this wave read in an earlier (or this) iteration — LDS operations
            // of a wave execute in order
            for (int i0 = 0; i0 < npad; i0 += 64) {
                const int i = i0 + lane;
                float x[RW];
#pragma unroll
                for (int rr = 0; rr < RW; rr++) x[rr] = ((const float *)rp[rr])[min(i, npad - 1)];
#pragma unroll
                for (int rr = 0; rr < RW; rr++)
                    if (rr < nrow && i < npad) {
                        const float e = i <= lim0 + rr * mstep ? x[rr] : 0.0f;
                        ((_Float16 *)(lds + (row0 + rr) * rb))[i] = f16_of_f32_product(e, inv[rr]);
                    }
            }
        }
    }
    __syncthreads();
    // ---- V.P: wave w takes value channels 32 w .. 32 w + 31
    if (wave < NWV) {
        const int nch = npad >> 4;
        const int d0 = wave * 32;
        const char *vp = vbase + (int64_t)(d0 + fr) * a.v_nb1 + fh * 16;
        const char *pa = lds + (fr & (QR - 1)) * rb + fh * 16;
        constexpr int NR = QR / 2;  // accumulator registers that hold real query rows
        auto load_v = [&](int c) {
            const int valid = M - (c * 16 + fh * 8);  // keys of this group of 8 that exist; what lies behind them is never read
            f16x8 v;
#pragma unroll
            for (int e = 0; e < 8; e++) v[e] = (_Float16)0.0f;
            if (valid >= 8) {
                v = *(const f16x8 *)(vp + c * 32);
            } else if (valid > 0) {
                const _Float16 *sv = (const _Float16 *)(vp + c * 32);
#pragma unroll
                for (int e = 0; e < 8; e++)
                    if (e < valid) v[e] = sv[e];
            }
            return v;
        };
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = 0.0f;
        constexpr int PF = 8;  // chunks in flight
        f16x8 vb[PF];
#pragma unroll
        for (int k = 0; k < PF; k++)
            if (k < nch) vb[k] = load_v(k);
        for (int c0 = 0; c0 < nch; c0 += PF) {
#pragma unroll
            for (int k = 0; k < PF; k++) {
                if (c0 + k < nch) {
                    const f16x8 pf = *(const f16x8 *)(pa + (c0 + k) * 32);
                    const f16x8 v = vb[k];
                    if (c0 + k + PF < nch) vb[k] = load_v(c0 + k + PF);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(pf, v, acc, 0, 0, 0);
                }
            }
        }
        float *op = a.out + (((int64_t)b * a.H + h) * a.N + q0 + 4 * fh) * D + d0 + fr;
#pragma unroll
        for (int r = 0; r < NR; r++) {
            const int row = (r & 3) + 8 * (r >> 2);
            if (q0 + 4 * fh + row < a.N) op[(int64_t)row * D] = acc[r];
        }
    }
}

// ---- one query row per workgroup ----------------------------------------------------------------------------------------------
// Dynamic LDS: [0, 256) the block reductions' scratch; then D floats of q (f16-rounded when K/V are f16); then the row's scores
// (f32; later e, then p), ceil(keys / 4) * 16 bytes.  Every carve offset is a multiple of 16.
//   scores : a group of G lanes (G = 1 .. 64, a power of two: D / 8 lanes of 8 f16, or D / 4 lanes of 4 f32, so that a D = 128 f16
//            head keeps all 64 lanes busy on 4 keys) per key, 16-byte loads where a.kvec allows and the channels behind the last
//            whole vector one by one; G lanes of one element each otherwise.
//   softmax: 256 threads over the row.
//   V.P    : one wave per value channel at a time, its lanes along the keys (V is transposed: keys are contiguous).
#define FLASH_ROW_RED 256

template <typename T>
__device__ __forceinline__ T flash_block_reduce(T v, char *red, bool is_max) {
    // v: the wave's value in every lane
    const int tid = threadIdx.x;
    T *s = (T *)red;
    __syncthreads();  // the scratch may still be read from the reduction before
    if ((tid & 63) == 0) s[tid >> 6] = v;
    __syncthreads();
    T r = s[0];
    for (int w = 1; w < 4; w++) r = is_max ? (s[w] > r ? s[w] : r) : r + s[w];
    return r;
}

template <bool KV16>
__global__ void __launch_bounds__(256) k_flash_attn_row(const FlashAttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    typedef typename std::conditional<KV16, _Float16, float>::type kv_t;
    constexpr int VEC = KV16 ? 8 : 4;  // elements of a 16-byte load
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int D = a.D;
    const int i = (int)blockIdx.x % a.N, rest = (int)blockIdx.x / a.N;
    const int h = rest % a.H, b = rest / a.H;
    const int hk = h / a.r;
    const int nk = a.masked ? a.P + i + 1 : a.M;  // keys 0 .. nk - 1 are kept (1 <= nk <= M); no other key is read
    char *red = lds;
    float *s_q = (float *)(lds + FLASH_ROW_RED);
    float *s_s = (float *)(lds + FLASH_ROW_RED + ((D * 4 + 15) & ~15));
    const char *qp = a.q + (int64_t)i * a.q_nb1 + (int64_t)h * a.q_nb2 + (int64_t)b * a.q_nb3;
    const char *kbase = a.k + (int64_t)hk * a.k_nb2 + (int64_t)b * a.k_nb3;
    const char *vbase = a.v + (int64_t)hk * a.v_nb2 + (int64_t)b * a.v_nb3;
    for (int c = tid; c < D; c += 256) {
        float x = a.q16 ? (float)((const _Float16 *)qp)[c] : ((const float *)qp)[c];
        if (KV16) x = round_f16(x);  // f32 q against f16 K/V: rounded when loaded, as mul_mat rounds its src1
        s_q[c] = x;
    }
    __syncthreads();
    // ---- scores
    {
        const int Dv = a.kvec ? D / VEC * VEC : 0;  // channels read as whole vectors
        int G = 1;                                  // lanes per key
        const int want = a.kvec && Dv > 0 ? Dv / VEC : D;
        while (G < want && G < 64) G <<= 1;
        const int gl = lane & (G - 1), gi = lane / G, ng = 64 / G;
        for (int j0 = wave * ng; j0 < nk; j0 += 4 * ng) {
            const int j = j0 + gi;
            float acc = 0.0f;
            if (j < nk) {
                const char *kp = kbase + (int64_t)j * a.k_nb1;
                for (int c = gl * VEC; c < Dv; c += G * VEC) {
                    if constexpr (KV16) {
                        const f16x8 kv = *(const f16x8 *)(kp + c * 2);
                        const f32x4 q0 = *(const f32x4 *)(s_q + c), q1 = *(const f32x4 *)(s_q + c + 4);
#pragma unroll
                        for (int e = 0; e < 4; e++) acc = __builtin_fmaf((float)kv[e], q0[e], acc);
#pragma unroll
                        for (int e = 0; e < 4; e++) acc = __builtin_fmaf((float)kv[4 + e], q1[e], acc);
                    } else {
                        const f32x4 kv = *(const f32x4 *)(kp + c * 4);
                        const f32x4 q0 = *(const f32x4 *)(s_q + c);
#pragma unroll
                        for (int e = 0; e < 4; e++) acc = __builtin_fmaf(kv[e], q0[e], acc);
                    }
                }
                for (int c = Dv + gl; c < D; c += G) acc = __builtin_fmaf((float)((const kv_t *)kp)[c], s_q[c], acc);
            }
            for (int m = G >> 1; m > 0; m >>= 1) acc += __shfl_xor(acc, m);
            if (j < nk && gl == 0) s_s[j] = acc * a.scale;
        }
    }
    __syncthreads();
    // ---- softmax over s_s[0 .. nk - 1]
    float mx = -INFINITY;
    for (int j = tid; j < nk; j += 256) mx = fmaxf(mx, s_s[j]);
    mx = flash_block_reduce<float>(wave_max_f32(mx), red, true);
    double sum = 0.0;
    for (int j = tid; j < nk; j += 256) {
        const float e = round_f16(exp_le0(round_f16(s_s[j] - mx)));
        sum += (double)e;  // exact: f16-valued terms, fewer than 2^16 of them
        s_s[j] = e;
    }
    sum = flash_block_reduce<double>(wave_sum_f64(sum), red, false);
    const float inv = (float)(1.0 / sum);
    for (int j = tid; j < nk; j += 256) {
        if constexpr (KV16)
            s_s[j] = (float)f16_of_f32_product(s_s[j], inv);
        else
            s_s[j] = s_s[j] * inv;
    }
    __syncthreads();
    // ---- V.P
    {
        const int nv = a.vvec ? nk / VEC * VEC : 0;  // keys read as whole vectors
        float *op = a.out + (((int64_t)b * a.H + h) * a.N + i) * D;
        for (int d = wave; d < D; d += 4) {
            const char *vp = vbase + (int64_t)d * a.v_nb1;
            float acc = 0.0f;
            for (int j = lane * VEC; j < nv; j += 64 * VEC) {
                if constexpr (KV16) {
                    const f16x8 vv = *(const f16x8 *)(vp + j * 2);
                    const f32x4 p0 = *(const f32x4 *)(s_s + j), p1 = *(const f32x4 *)(s_s + j + 4);
#pragma unroll
                    for (int e = 0; e < 4; e++) acc = __builtin_fmaf((float)vv[e], p0[e], acc);
#pragma unroll
                    for (int e = 0; e < 4; e++) acc = __builtin_fmaf((float)vv[4 + e], p1[e], acc);
                } else {
                    const f32x4 vv = *(const f32x4 *)(vp + j * 4);
                    const f32x4 p0 = *(const f32x4 *)(s_s + j);
#pragma unroll
                    for (int e = 0; e < 4; e++) acc = __builtin_fmaf(vv[e], p0[e], acc);
                }
            }
            for (int j = nv + lane; j < nk; j += 64) acc = __builtin_fmaf((float)((const kv_t *)vp)[j], s_s[j], acc);
            acc = wave_sum_f32(acc);
            if (lane == 0) op[d] = acc;
        }
    }
}
