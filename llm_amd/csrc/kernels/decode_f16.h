// decode_f16.h — the decode / chunk mat-vec of a LLaMA whose matrices are F16 (file type 1: what every conversion writes before
// quantizing), as ONE wave of 1024-thread workgroups that stage the activation themselves: k_mmvq_kbig's skeleton
// (kernels/kquant_big.h) with a much simpler row dot and no weight re-layout — a weight is the tensor's own rows.
//
// Staging: the workgroup builds the NCOLS activation rows (KX_NORM: rms_norm(x) * w in k_rms_norm's f64 order, KX_F32: the row,
// KX_SILU_MUL: silu(a) * b) and rounds them to f16 (round to nearest even) into LDS — what ggml's F16 mul_mat does to src1
// (ggml_fp32_to_fp16_row).  LDS: NCOLS * K * 2 bytes.
//
// Row dot: a row is K / 8 chunks of 16 bytes.  DESIGN RULE — a row's result is a pure function of the row's bytes, the staged
// f16 activation column and K:
//   * lane l of the wave that owns the row takes chunks l, l + 64, l + 128, ... (chunk l + 64 i in step i);
//   * a lane adds its chunks in that order into ONE f32 accumulator per column, the four f16 pairs of a chunk in ascending
//     order through v_dot2_f32_f16 (exact products, f32 accumulation); lanes whose chunk lies past the row end add nothing;
//   * the 64 accumulators are summed by wave_sum_f32 (a fixed DPP tree).
// Nothing of that depends on the grid, on how many waves take rows, on NCOLS or on the column's index: a chunk of N tokens
// equals N single-token evaluations bit for bit, and a batched step equals the chunk (tests/test_f16_matvec_gpu.py,
// tests/test_f16_plan_gpu.py).  A matrix-core form would sum in the MFMA's order, which differs per tile shape: none here.
//
// The weight stream: a wave keeps F16_PF steps (16 bytes per lane each) requested ahead, over row boundaries — the ring of
// k_mmvq_kbig: every slot is refilled unconditionally (steps past the wave's last are dummy reads of one hot line), nothing is
// stored while the ring runs (results are parked in the lane of their unit until the epilogue), so every wait inside the loop
// has a compile-time count.
//
// Epilogues (expressions of k_mmvq_kbig's and of k_k_rope_store): KE_ROW store / store + res; KE_GATE silu(w1 x) * (w3 x) with the
// executor's f16-table SiLU; KE_QKV: a unit = two adjacent rows, RoPE of the pair, Q f32 in place of dst, K f16 into the cache row of
// the column's position, V f16 into the transposed cache.  The column's position and cache come from DecParams (n_past + col0 + c:
// a chunk) or from a BatchCols table + kv_off (a batched step).
#pragma once
#include "kquant_big.h"  // KX_* / KE_*, silu_table, DecParams, BatchCols

struct F16Args {
    const __half *w[3];  // up to three matrices that share the activation (rows of all of them dealt together)
    int64_t M[3];        // rows
    int64_t ld[3];       // row stride in elements (% 8 == 0; the base is 16-byte aligned)
    float *dst[3];       // [ncols][M[i]]
    int nseg;
    int K;               // % 8 == 0
    const float *res;    // KE_ROW, nullable: [ncols][M[0]]
    const float *xf;     // [ncols][K]: the f32 rows (KX_SILU_MUL: w1 x)
    const float *xw;     // KX_NORM: the norm weight [K];  KX_SILU_MUL: w3 x [ncols][K]
    float eps;
    float *y_out;        // KX_NORM + KE_ROW, nullable: [ncols][K] f32 copy of the normed rows, written by workgroup 0
    int seg_kind[3];     // KE_QKV: 0 / 1 / 2 = wq / wk / wv
    const float *rope;   // KE_QKV: [ncols][128] (cos, sin) tables (k_rope_table / k_rope_table_batch)
    const DecParams *prm;
    const BatchCols *bc;  // batched step: column c sits at bc->pos[col0 + c] of the caches bc->mem_k / mem_v[col0 + c] + kv_off
    int64_t kv_off;
    int col0;            // first column of this pass
    __half *mem_k, *mem_v;  // + layer offset (chunk form)
    int64_t Egqa, C;
    int D;
    const void *hot;     // 256 zero bytes the dummy ring steps read
};

#define F16_T 1024
// steps a wave keeps requested ahead: 8 x 1 KB x 16 waves = 128 KB per CU on its way (the dots are cheap: the depth is what keeps
// HBM busy); 8 columns with two parked results each still fit the registers of a 1024-thread workgroup without scratch
template <int NCOLS>
struct F16Ring {
    static constexpr int PF = 8;
};

__device__ __forceinline__ float f16_chunk_dot(const f16x8 w, const f16x8 x, float acc) {
#pragma unroll
    for (int j = 0; j < 4; j++) acc = __builtin_amdgcn_fdot2(f16x2{w[2 * j], w[2 * j + 1]}, f16x2{x[2 * j], x[2 * j + 1]}, acc, false);
    return acc;
}

template <int XSRC, int EPI, int NCOLS>
__global__ void __launch_bounds__(F16_T) k_mmvq_f16(const F16Args a) {
    constexpr int F16_PF = F16Ring<NCOLS>::PF;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ double s_part[NCOLS][4];
    _Float16 *s_x = (_Float16 *)smem;  // [NCOLS][K]
    const int bid = (int)blockIdx.x, G = (int)gridDim.x;
    const int K = a.K, nch = K >> 3;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int W = F16_T / 64;
    constexpr bool GATE = EPI == KE_GATE, PAIR = EPI != KE_ROW;
    const int nsteps = (nch + 63) >> 6;
    const int64_t Mall = a.M[0] + a.M[1] + a.M[2];  // (M of a matrix the launch does not have is 0)
    const int Mt = GATE ? (int)a.M[0] : EPI == KE_QKV ? (int)(Mall >> 1) : (int)Mall;
    // units of this wave, dealt wave-major: unit = wave * G + bid + G * W * i  (the launcher keeps nrw <= 64: one epilogue lane each)
    const int r_first = wave * G + bid, r_stride = G * W;
    const int nrw = r_first < Mt ? (Mt - r_first + r_stride - 1) / r_stride : 0;
    const int nhr = PAIR ? 2 * nrw : nrw;  // weight rows the wave walks
    const int S = nhr * nsteps;

    // global row `grow` of the launch's concatenated matrices -> its matrix and row there (M of a matrix the launch does not have is
    // 0: the comparisons alone decide; selects, no branches — a branch around a ring load costs the loop its counted waits)
    const int64_t M0 = a.M[0], M01 = a.M[0] + a.M[1];
    auto select = [&](int64_t grow, int &seg, int64_t &row) {
        const bool s1 = grow >= M0, s2 = grow >= M01;
        seg = s2 ? 2 : s1 ? 1 : 0;
        row = grow - (s2 ? M01 : s1 ? M0 : 0);
    };
    // ---- the load cursor: (row of the wave, step of the row); the row's base is wave-uniform and changes only at a row switch
    int li = 0, ls = 0;
    const __half *l_row = a.w[0];
    auto set_row = [&](int i) {
        if constexpr (GATE) {
            const int64_t row = (int64_t)(r_first + r_stride * (i >> 1));
            l_row = (i & 1) ? a.w[1] + row * a.ld[1] : a.w[0] + row * a.ld[0];
        } else {
            const int64_t grow = EPI == KE_QKV ? (int64_t)2 * (r_first + r_stride * (i >> 1)) + (i & 1) : (int64_t)(r_first + r_stride * i);
            int seg;
            int64_t row;
            select(grow, seg, row);
            const __half *wb = seg == 0 ? a.w[0] : seg == 1 ? a.w[1] : a.w[2];
            const int64_t ld = seg == 0 ? a.ld[0] : seg == 1 ? a.ld[1] : a.ld[2];
            l_row = wb + row * ld;
        }
    };
    auto load = [&](f16x8 &st, const bool dummy) {
        int ch = ls * 64 + lane;
        ch = ch < nch ? ch : nch - 1;  // lanes past the row end re-read the last chunk and are masked at the dot
        const __half *p = l_row + (int64_t)ch * 8;
        p = dummy ? (const __half *)a.hot : p;
        st = __builtin_nontemporal_load((const f16x8 *)p);
        if (!dummy && ++ls == nsteps) {  // the cursor moves on behind the load (a dummy step moves nothing)
            ls = 0;
            if (++li < nhr) set_row(li);
        }
    };
    // ---- 1. the weight stream starts before the activation is staged
    f16x8 ring[F16_PF];
    if (nhr > 0) set_row(0);
#pragma unroll
    for (int k = 0; k < F16_PF; k++) load(ring[k], k >= S);

    // ---- 2. stage the NCOLS rows as f16
    float scale[NCOLS];
#pragma unroll
    for (int c = 0; c < NCOLS; c++) scale[c] = 1.0f;
    if constexpr (XSRC == KX_NORM) {
        // k_rms_norm's order per row: thread t of 256 adds elements t, t + 256, ... in f64, waves by DPP, (s0 + s1) + (s2 + s3);
        // the 256-thread group tid >> 8 takes columns group, group + 4
        const int grp = tid >> 8, t = tid & 255;
#pragma unroll
        for (int c = 0; c < NCOLS; c++) {
            if ((c & 3) == grp) {  // uniform per wave
                const float *xr = a.xf + (int64_t)c * K;
                double s = 0.0;
                for (int i = t; i < K; i += 256) {
                    const float v = xr[i];
                    s += (double)(v * v);
                }
                s = wave_sum_f64(s);
                if (lane == 0) s_part[c][wave & 3] = s;
            }
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < NCOLS; c++) {
            const double tot = (s_part[c][0] + s_part[c][1]) + (s_part[c][2] + s_part[c][3]);
            const float mean = (float)(tot / (double)K);
            scale[c] = 1.0f / sqrtf(mean + a.eps);
        }
    }
    {
        const int K4 = K >> 2;
        for (int i4 = tid; i4 < K4; i4 += F16_T) {
            f32x4 w4 = {1.0f, 1.0f, 1.0f, 1.0f};
            if constexpr (XSRC == KX_NORM) w4 = ((const f32x4 *)a.xw)[i4];
#pragma unroll
            for (int c = 0; c < NCOLS; c++) {
                f32x4 v = ((const f32x4 *)(a.xf + (int64_t)c * K))[i4];
                if constexpr (XSRC == KX_NORM) {
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const float t = v[k] * scale[c];
                        v[k] = t * w4[k];
                    }
                    // (only the lm_head launch has the tap: a store that MAY be pending turns every later wait into a full one)
                    if constexpr (EPI == KE_ROW)
                        if (a.y_out && bid == 0) ((f32x4 *)(a.y_out + (int64_t)c * K))[i4] = v;
                } else if constexpr (XSRC == KX_SILU_MUL) {
                    const f32x4 b4 = ((const f32x4 *)(a.xw + (int64_t)c * K))[i4];
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const float t = silu_table(v[k]);
                        v[k] = t * b4[k];
                    }
                }
                *(f16x4 *)(s_x + (int64_t)c * K + 4 * i4) = f16x4{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
            }
        }
    }
    __syncthreads();

    // ---- 3. rows
    float acc[NCOLS], myv[NCOLS], myv3[PAIR ? NCOLS : 1];
#pragma unroll
    for (int c = 0; c < NCOLS; c++) {
        acc[c] = 0.0f;
        myv[c] = 0.0f;
        if constexpr (PAIR) myv3[c] = 0.0f;
    }
    int ri = 0, rs = 0;  // row index of the wave, step inside the row
    auto step = [&](const f16x8 &st) {
        const int ch = rs * 64 + lane;
        if (ch < nch) {
#pragma unroll
            for (int c = 0; c < NCOLS; c++) acc[c] = f16_chunk_dot(st, *(const f16x8 *)(s_x + (int64_t)c * K + ch * 8), acc[c]);
        }
        if (++rs == nsteps) {  // uniform
            rs = 0;
#pragma unroll
            for (int c = 0; c < NCOLS; c++) {
                const float v = wave_sum_f32(acc[c]);
                if constexpr (PAIR) {  // (two selects, not a branch between the arrays: that would index them at run time and put them in scratch)
                    const bool mine = lane == (ri >> 1), odd = (ri & 1) != 0;
                    myv[c] = mine && !odd ? v : myv[c];
                    myv3[c] = mine && odd ? v : myv3[c];
                } else {
                    myv[c] = lane == ri ? v : myv[c];
                }
                acc[c] = 0.0f;
            }
            ri++;
        }
    };
    int k0 = 0;
    for (; k0 + F16_PF < S; k0 += F16_PF) {
#pragma unroll
        for (int u = 0; u < F16_PF; u++) {
            step(ring[u]);
            load(ring[u], k0 + u + F16_PF >= S);
        }
    }
#pragma unroll
    for (int u = 0; u < F16_PF; u++)
        if (k0 + u < S) step(ring[u]);  // uniform

    // ---- 4. epilogue: lane i of the wave holds its i-th unit's results of every column
    if (lane >= nrw) return;
    const int unit = r_first + r_stride * lane;
    if constexpr (GATE) {
#pragma unroll
        for (int c = 0; c < NCOLS; c++) a.dst[0][(int64_t)c * a.M[0] + unit] = silu_table(myv[c]) * myv3[c];
        return;
    } else if constexpr (EPI == KE_QKV) {
        int seg;
        int64_t m0;
        select((int64_t)2 * unit, seg, m0);
        const int kind = seg == 0 ? a.seg_kind[0] : seg == 1 ? a.seg_kind[1] : a.seg_kind[2];
        const int kk = (int)(m0 % a.D) >> 1;
#pragma unroll
        for (int c = 0; c < NCOLS; c++) {
            const int col = a.col0 + c;
            const int p = a.bc ? a.bc->pos[col] : a.prm->n_past + col;
            __half *mk = a.bc ? a.bc->mem_k[col] + a.kv_off : a.mem_k;
            __half *mv = a.bc ? a.bc->mem_v[col] + a.kv_off : a.mem_v;
            if (kind == 2) {  // V: f16 into the transposed cache
                mv[m0 * a.C + p] = __float2half_rn(myv[c]);
                mv[(m0 + 1) * a.C + p] = __float2half_rn(myv3[c]);
            } else {
                const float cs = a.rope[c * 128 + 2 * kk], sn = a.rope[c * 128 + 2 * kk + 1];
                const float r0 = myv[c] * cs - myv3[c] * sn, r1 = myv[c] * sn + myv3[c] * cs;
                if (kind == 0) {
                    float *q = (seg == 0 ? a.dst[0] : seg == 1 ? a.dst[1] : a.dst[2]) + (int64_t)c * (seg == 0 ? a.M[0] : seg == 1 ? a.M[1] : a.M[2]);
                    q[m0] = r0;
                    q[m0 + 1] = r1;
                } else {
                    mk[(int64_t)p * a.Egqa + m0] = __float2half_rn(r0);
                    mk[(int64_t)p * a.Egqa + m0 + 1] = __float2half_rn(r1);
                }
            }
        }
        return;
    } else {
        int seg;
        int64_t row;
        select((int64_t)unit, seg, row);
        float *d = seg == 0 ? a.dst[0] : seg == 1 ? a.dst[1] : a.dst[2];
        const int64_t Ms = seg == 0 ? a.M[0] : seg == 1 ? a.M[1] : a.M[2];
#pragma unroll
        for (int c = 0; c < NCOLS; c++) d[(int64_t)c * Ms + row] = a.res ? myv[c] + a.res[(int64_t)c * a.M[0] + row] : myv[c];
    }
}
