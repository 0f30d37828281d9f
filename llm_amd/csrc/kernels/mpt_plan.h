// mpt_plan.h — what the MPT decode plan (plan_decode.inc plan_launch_mpt) launches that no LLaMA plan does, all of it compiled into
// a code object of its own (mpt_plan.hip, MPT_PLAN_OBJECT) so that hip_backend.hip's code object holds what it held:
//   k_mmvq_big<QT, EPI_QKV_TM | EPI_GELU | EPI_STORE, XSRC_LNORM>   the mat-vecs behind a LayerNorm (kernels/decode_big.h)
//   k_attn_decode_alibi                                             decode attention over token-major K AND V, with the ALiBi bias
//   k_lnorm_stage_dump                                              test hook: the Q8 blocks big_stage_lnorm leaves in LDS
// hip_backend.hip sees only the launch functions declared at the end of this file.
#pragma once
#ifdef MPT_PLAN_OBJECT
#include "decode_big.h"

// Decode attention of MPT's graph (crates/models/mpt/src/lib.rs:153-210) for one query token: one 1024-thread workgroup per head.
//   s_t = Σ_d K[t][d]·f16(q[d])                       f32 accumulation, K f16 [C][E] (token-major)
//   x_t = (float)t * slope[h] + s_t * scale           k_alibi's / k_soft_max<true, true>'s expression: __fmul_rn twice, __fadd_rn
//   p   = soft_max(x_0 .. x_P)                        ggml's: maximum, f16-rounded exp of the f16-rounded difference, f64 sum, * (float)(1 / sum)
//   o_d = Σ_t V[t][d]·f16(p_t)                        V f16 [C][E] token-major too: read where the K/V store left it.  The reference's
//                                                     graph re-copies the whole V cache into a [T, D, H] tensor per layer and token
//                                                     first (lib.rs:185-205); that tensor has no other reader and is never made here.
// Positions beyond P = prm->n_past are never read.  Scores: 64 groups of 16 lanes, a lane holds 8 dims of a position, a group takes
// positions g, g + 64, ...; V·P has the same shape (a lane accumulates its 8 channels over its group's positions), then the four groups
// of a wave are added by shuffles and the 16 waves through LDS (s_acc, static), in a fixed order.  Dynamic LDS: Clds scores (f32) + Clds
// probabilities (f16); the launchers ask for attn_decode_lds(Clds, D), k_attn_decode's size, which is D floats more.  Clds >= P + 1, % 8 == 0.  D % 8 == 0, D <= 128 (the matcher asks % 32).
// out: the merged heads [n_head * D] f32 — out_proj stages it as a plain f32 row.
__global__ void __launch_bounds__(1024) k_attn_decode_alibi(const float *__restrict__ q, const __half *__restrict__ mem_k,
                                                            const __half *__restrict__ mem_v, const DecParams *prm, float scale,
                                                            const float *__restrict__ slopes, int D, int64_t E, float *__restrict__ out,
                                                            int64_t Clds) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *s_s = (float *)smem;             // Clds scores
    _Float16 *s_p = (_Float16 *)(s_s + Clds);  // Clds probabilities as f16 (src1 of the V matmul)
    __shared__ float s_red[16];
    __shared__ double s_redd[16];
    __shared__ float s_acc[16][128];
    const int h = blockIdx.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int T = prm->n_past + 1;
    if (T < 1 || T > Clds) return;  // (never: the plan runs positions inside the context only)
    const float slope = slopes[h];
    const int g = tid >> 4, gl = tid & 15;  // 64 groups of 16 lanes, lane gl owns dims gl*8 .. gl*8+7
    const int d0 = gl * 8;
    const bool act = d0 < D;
    const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    f16x2 qh2[4];  // ggml rounds src1 (Q) to f16; the products below are exact in f32 (v_dot2_f32_f16)
    {
        f32x4 q0 = {0.0f, 0.0f, 0.0f, 0.0f}, q1 = q0;
        if (act) {
            q0 = *(const f32x4 *)(q + (int64_t)h * D + d0);
            q1 = *(const f32x4 *)(q + (int64_t)h * D + d0 + 4);
        }
#pragma unroll
        for (int j = 0; j < 2; j++) {
            qh2[j] = f16x2{(_Float16)q0[2 * j], (_Float16)q0[2 * j + 1]};
            qh2[2 + j] = f16x2{(_Float16)q1[2 * j], (_Float16)q1[2 * j + 1]};
        }
    }
    // ---- scores, scaled and biased ----
    const __half *kbase = mem_k + (int64_t)h * D + d0;
#pragma unroll 1
    for (int t0 = g; t0 < T; t0 += 256) {
        f16x8 kv[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int t = t0 + 64 * u;
            kv[u] = zero8;
            if (act && t < T) kv[u] = *(const f16x8 *)(kbase + (int64_t)t * E);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int t = t0 + 64 * u;
            float s = 0.0f;
#pragma unroll
            for (int j = 0; j < 4; j++) s = __builtin_amdgcn_fdot2(f16x2{kv[u][2 * j], kv[u][2 * j + 1]}, qh2[j], s, false);
            s = g16_sum_f32(s);
            if (gl == 0 && t < T) s_s[t] = __fadd_rn(__fmul_rn((float)t, slope), __fmul_rn(s, scale));
        }
    }
    __syncthreads();
    // ---- soft_max over the T entries (the maximum and the f64 sum of f16-valued terms are exact: their order is immaterial) ----
    float mx = -INFINITY;
    for (int t = tid; t < T; t += 1024) mx = fmaxf(mx, s_s[t]);
    mx = wave_max_f32(mx);
    if (lane == 0) s_red[wave] = mx;
    __syncthreads();
    mx = s_red[0];
#pragma unroll
    for (int i = 1; i < 16; i++) mx = fmaxf(mx, s_red[i]);
    double sum = 0.0;
    for (int t = tid; t < T; t += 1024) {
        const float e = round_f16(expf(round_f16(s_s[t] - mx)));
        s_s[t] = e;
        sum += (double)e;
    }
    sum = wave_sum_f64(sum);
    if (lane == 0) s_redd[wave] = sum;
    __syncthreads();
    double tot = 0.0;
#pragma unroll
    for (int i = 0; i < 16; i++) tot += s_redd[i];
    const float inv = (float)(1.0 / tot);
    for (int t = tid; t < T; t += 1024) s_p[t] = (_Float16)(s_s[t] * inv);  // (the thread that wrote s_s[t])
    __syncthreads();
    // ---- V·P ----
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; j++) acc[j] = 0.0f;
    const __half *vbase = mem_v + (int64_t)h * D + d0;
#pragma unroll 1
    for (int t0 = g; t0 < T; t0 += 256) {
        f16x8 vv[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int t = t0 + 64 * u;
            vv[u] = zero8;
            if (act && t < T) vv[u] = *(const f16x8 *)(vbase + (int64_t)t * E);
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int t = t0 + 64 * u;
            if (t < T) {
                const float p = (float)s_p[t];
#pragma unroll
                for (int j = 0; j < 8; j++) acc[j] += (float)vv[u][j] * p;  // f16 x f16: exact in f32
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {  // the wave's four groups (lanes gl, gl + 16, gl + 32, gl + 48)
        acc[j] += __shfl_xor(acc[j], 16);
        acc[j] += __shfl_xor(acc[j], 32);
    }
    if (lane < 16 && act) {
#pragma unroll
        for (int j = 0; j < 8; j++) s_acc[wave][d0 + j] = acc[j];
    }
    __syncthreads();
    if (tid < D) {
        float o = 0.0f;
#pragma unroll
        for (int w = 0; w < 16; w++) o += s_acc[w][tid];
        out[(int64_t)h * D + tid] = o;
    }
}

// Test hook: one workgroup stages norm(x) * w as k_mmvq_big<.., XSRC_LNORM> stages it (the same BigX loads, the same big_stage_lnorm)
// and hands out what its LDS holds: the planar Q8 blocks (lo, hi: 16 int8 each), their scales and sums.
template <bool F16_D>
__global__ void __launch_bounds__(1024) k_lnorm_stage_dump(const BigArgs ba, i32x4 *lo, i32x4 *hi, float *d, int *sum) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ double s_part[16];
    const int nb = ba.nb, nbp = ((nb + 63) >> 6) * 64, tid = threadIdx.x;
    i32x4 *s_lo = (i32x4 *)smem;
    i32x4 *s_hi = s_lo + nbp;
    float *s_d = (float *)(s_hi + nbp);
    int *s_sum = (int *)(s_d + nbp);
    BigX<XSRC_LNORM> xr;
    xr.load(ba, nb, tid, 1024);
    big_stage_x<F16_D, XSRC_LNORM, false>(ba, xr, nb, nbp, tid, 1024, s_lo, s_hi, s_d, s_sum, s_part, nullptr);
    __syncthreads();
    for (int i = tid; i < nb; i += 1024) {
        lo[i] = s_lo[i];
        hi[i] = s_hi[i];
        d[i] = s_d[i];
        sum[i] = s_sum[i];
    }
}
#else  // hip_backend.hip
// ---- what hip_backend.hip calls (defined in mpt_plan.hip; BigArgs and DecParams are distinct types in the two objects, same
// definitions: they travel as void *) ----
// k_mmvq_big<qt, epi, XSRC_LNORM> on G workgroups of 1024 threads (BigArgs::wdeal of them take units); epi: EPI_QKV_TM, EPI_GELU or
// EPI_STORE.  1: no such instantiation.
int launch_mpt_big(hipStream_t stream, int qt, int epi, const void *big_args, int G, size_t lds);
// k_attn_decode_alibi on n_head workgroups; lds = attn_decode_lds(Clds, D).  1: the LDS opt-in failed.
int launch_mpt_attn(hipStream_t stream, int n_head, const float *q, const void *mem_k, const void *mem_v, const void *prm, float scale,
                    const float *slopes, int D, int64_t E, float *out, int64_t Clds, size_t lds);
int launch_mpt_stage_dump(hipStream_t stream, int f16d, const void *big_args, void *lo, void *hi, float *d, int *sum, size_t lds);
// the quantizer branch of THIS code object's copy of c_act_quant_scalar (kernels/common.h): apply_act_quant sets both
int mpt_plan_set_act_quant(int v);
#endif
