// bloom_plan.h — what the BLOOM decode plan (plan_decode.inc plan_launch_bloom) launches that neither the MPT plan nor a LLaMA plan does, all
// of it compiled into a code object of its own (bloom_plan.hip, BLOOM_PLAN_OBJECT) so that every other code object holds what it held:
//   k_get_rows_lnorm<QT>                                                the token's embedding row, dequantized, then LayerNorm with gain and bias
//   k_mmvq_big<QT, EPI_QKV_TM_B | EPI_GELU_B | EPI_STORE, XSRC_LNORM_B>  the mat-vecs behind a biased LayerNorm (kernels/decode_big.h)
//   k_mmvq_big<QT, EPI_ADD_B, XSRC_F32>                                  wo / w2: the dot, + bias, + residual
//   k_lnorm_b_stage_dump                                                 test hook: the Q8 blocks the biased LayerNorm staging leaves in LDS
// The attention between them is the MPT plan's, out of the MPT plan's code object (launch_mpt_attn, launch_mpt_attn_split).
// hip_backend.hip sees only the launch functions declared at the end of this file.
#pragma once
#ifdef BLOOM_PLAN_OBJECT
#include "decode_big.h"

// Elements 4 e4 .. 4 e4 + 3 of row `row` of a block-format weight as f32: k_get_rows_q's arithmetic (x * d, then + m: two roundings).
// Block e4 / 8; the low nibbles / first plane are elements 0..15 of a block, the high nibbles / second plane 16..31.
template <int QT>
__device__ __forceinline__ f32x4 bloom_embed4(const QWeight &w, int64_t row, int e4) {
    constexpr bool has_m = QT == QT_Q4_1 || QT == QT_Q5_1, has_h = QT == QT_Q5_0 || QT == QT_Q5_1;
    constexpr int zero = QT == QT_Q4_0 ? 8 : QT == QT_Q5_0 ? 16 : 0;
    const int64_t i = row * w.nb + (e4 >> 3);
    const int o = (e4 & 7) * 4, j0 = o & 15;
    const bool up = o >= 16;
    const float d = __half2float(w.d[i]);
    f32x4 v;
    if constexpr (QT == QT_Q8_0) {
        const uint32_t q = *(const uint32_t *)((up ? w.qs2 : w.qs) + i * 16 + j0);
#pragma unroll
        for (int u = 0; u < 4; u++) v[u] = (float)(int8_t)(q >> (8 * u)) * d;
    } else {
        const uint32_t q = *(const uint32_t *)(w.qs + i * 16 + j0);
        float m = 0.0f;
        uint32_t qh = 0;
        if constexpr (has_m) m = __half2float(w.m[i]);
        if constexpr (has_h) qh = w.qh[i];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int j = j0 + u;
            const uint32_t b = (q >> (8 * u)) & 0xFFu;
            const int xh = !has_h ? 0 : up ? (int)((qh >> (j + 12)) & 0x10u) : (int)(((qh >> j) << 4) & 0x10u);
            const int x = (int)((up ? (b >> 4) : (b & 0x0Fu)) | (uint32_t)xh) - zero;
            v[u] = has_m ? __fadd_rn(__fmul_rn((float)x, d), m) : __fmul_rn((float)x, d);
        }
    }
    return v;
}

// The opening of a BLOOM token (crates/models/bloom/src/lib.rs:140-147): x = add(mul(norm(get_rows(tok_embeddings, token)), norm.weight),
// norm.bias), ONE workgroup of 1024 threads.  The dequantized row never leaves the registers: thread t holds elements 4 i .. 4 i + 3 for
// i = t and i = 1024 + t (E <= 8192: the launcher's condition), the shape of BigX<XSRC_NORM>, and the LayerNorm over them is
// big_stage_lnorm's two passes in big_stage_lnorm's reduction order — per thread in element order, wave_sum_f64, the 16 partial sums in wave
// order; mean first, then the variance of the centred f32 values — so a row normed here and a row normed by the staging of the next launch
// see the same statistics for the same values.  Then (c * scale) * w and + b, each rounded.  Out: the residual row dst [E].
template <int QT>
__global__ void __launch_bounds__(1024) k_get_rows_lnorm(const QWeight w, const int *__restrict__ ids, const float *__restrict__ gain,
                                                         const float *__restrict__ bias, float eps, float *__restrict__ dst) {
    constexpr int MAXIT = 2, NT = 1024;
    __shared__ double s_part[NT / 64];
    const int tid = threadIdx.x;
    const int n4 = (int)w.nb * 8, n_el = (int)w.nb * 32;
    const int64_t row = ids[0];
    f32x4 v[MAXIT], gw[MAXIT], gb[MAXIT];
#pragma unroll
    for (int it = 0; it < MAXIT; it++) {
        const int i4 = it * NT + tid, ic = i4 < n4 ? i4 : 0;
        v[it] = bloom_embed4<QT>(w, row, ic);
        gw[it] = ((const f32x4 *)gain)[ic];
        gb[it] = ((const f32x4 *)bias)[ic];
    }
    const bool pow2 = (n_el & (n_el - 1)) == 0;  // uniform: the division is then an exact scaling
    auto mean_of = [&](double tot) {
        return pow2 ? (float)__builtin_ldexp(tot, -(31 - __builtin_clz((unsigned)n_el))) : (float)(tot / (double)n_el);
    };
    auto total = [&](double x) {
        x = wave_sum_f64(x);
        if ((tid & 63) == 0) s_part[tid >> 6] = x;
        __syncthreads();
        double tot = 0.0;
#pragma unroll
        for (int i = 0; i < NT / 64; i++) tot += s_part[i];
        return tot;
    };
    double s = 0.0;
#pragma unroll
    for (int it = 0; it < MAXIT; it++)
        if (it * NT + tid < n4) {
#pragma unroll
            for (int k = 0; k < 4; k++) s += (double)v[it][k];
        }
    const float mean = mean_of(total(s));
    __syncthreads();  // every wave has read the first set of partial sums
    f32x4 c[MAXIT];
    double s2 = 0.0;
#pragma unroll
    for (int it = 0; it < MAXIT; it++) {
        c[it] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (it * NT + tid < n4) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                c[it][k] = v[it][k] - mean;
                s2 += (double)(c[it][k] * c[it][k]);
            }
        }
    }
    const float variance = mean_of(total(s2));
    const float scale = 1.0f / sqrtf(variance + eps);
#pragma unroll
    for (int it = 0; it < MAXIT; it++) {
        const int i4 = it * NT + tid;
        if (i4 < n4) {
            f32x4 y;
#pragma unroll
            for (int k = 0; k < 4; k++) y[k] = __fadd_rn(__fmul_rn(c[it][k] * scale, gw[it][k]), gb[it][k]);
            ((f32x4 *)dst)[i4] = y;
        }
    }
}

// Test hook: one workgroup stages (norm(x) * w) + b as k_mmvq_big<.., XSRC_LNORM_B> stages it (the same BigX loads, the same big_stage_lnorm)
// and hands out what its LDS holds: the planar Q8 blocks (lo, hi: 16 int8 each), their scales and sums.
template <bool F16_D>
__global__ void __launch_bounds__(1024) k_lnorm_b_stage_dump(const BigArgs ba, i32x4 *lo, i32x4 *hi, float *d, int *sum) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ double s_part[16];
    const int nb = ba.nb, nbp = ((nb + 63) >> 6) * 64, tid = threadIdx.x;
    i32x4 *s_lo = (i32x4 *)smem;
    i32x4 *s_hi = s_lo + nbp;
    float *s_d = (float *)(s_hi + nbp);
    int *s_sum = (int *)(s_d + nbp);
    BigX<XSRC_LNORM_B> xr;
    xr.load(ba, nb, tid, 1024);
    big_stage_x<F16_D, XSRC_LNORM_B, false>(ba, xr, nb, nbp, tid, 1024, s_lo, s_hi, s_d, s_sum, s_part, nullptr);
    __syncthreads();
    for (int i = tid; i < nb; i += 1024) {
        lo[i] = s_lo[i];
        hi[i] = s_hi[i];
        d[i] = s_d[i];
        sum[i] = s_sum[i];
    }
}
#else  // hip_backend.hip
// ---- what hip_backend.hip calls (defined in bloom_plan.hip; BigArgs and QWeight are distinct types in the two objects, same
// definitions: they travel as void *) ----
// k_mmvq_big<qt, epi, xsrc> on G workgroups of `threads` threads; (epi, xsrc): (EPI_QKV_TM_B | EPI_GELU_B | EPI_STORE, XSRC_LNORM_B) or
// (EPI_ADD_B, XSRC_F32).  1: no such instantiation.
int launch_bloom_big(hipStream_t stream, int qt, int epi, int xsrc, const void *big_args, int G, int threads, size_t lds);
// k_get_rows_lnorm<qt> on one workgroup: row ids[0] of wte (a QWeight, nb <= 256), LayerNorm with gain and bias, into dst.  1: no such type.
int launch_bloom_embed(hipStream_t stream, int qt, const void *wte, const int *ids, const float *gain, const float *bias, float eps, float *dst);
int launch_bloom_stage_dump(hipStream_t stream, int f16d, const void *big_args, void *lo, void *hi, float *d, int *sum, size_t lds);
// the quantizer branch of THIS code object's copy of c_act_quant_scalar (kernels/common.h): apply_act_quant sets every copy
int bloom_plan_set_act_quant(int v);
#endif
