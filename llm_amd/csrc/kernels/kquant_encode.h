// ggml_quantize_q2_K / q3_K / q4_K / q5_K / q6_K on the device: f32 (or f16) rows -> raw GGML super-blocks of 84 / 110 /
// 144 / 176 / 210 bytes, byte for byte what the host functions of the ABI (ggml_core.cpp) and the oracle's quantize_row_q*_K
// produce.  The fit is the oracle's (oracle/SEMANTICS.md): a min/max fit per sub-block for Q2_K / Q4_K / Q5_K, an abs-max fit
// for Q3_K / Q6_K — NOT upstream's iterative make_qkx / make_qx search, whose source is not available to restate
// (DESIGN.md §5, §8).
//
// One wave per super-block of 256 values, lane l holding elements 4l .. 4l + 3 (one 16-byte load, 1 KiB per wave), the layout
// of q8k_wave_block (kquant_big.h).  A 32-value sub-block is 8 lanes, a 16-value sub-block one quad: their extremes are DPP
// reductions (quad_perm x 2 [, row_half_mirror]), the super-block extremes the wave reductions of common.h.  Min and max are
// order-free.  The first-wins rules of the abs-max fit are not: inside a sub-block the FIRST element of largest magnitude
// supplies the signed value (the reduction carries (index, value) and keeps the lower index), across the 16 sub-blocks the
// FIRST scale of largest magnitude supplies max_sc (min reduction of the lane index, then v_readlane).
// Every f32 operation of the oracle is made once, in its order: correctly rounded divisions (__fdiv_rn, never a reciprocal
// and a multiply), nearest_int = round half to even (__float2int_rn), f16 conversions of a value pinned in a register
// (q_put_f16's reason, quantize.h), no contraction (the translation unit is built with -ffp-contract=off).
// Packing needs codes 32 / 64 / 96 elements apart (lanes 8 / 16 / 24 apart): the 256 codes (a u32 per lane) and the sub-block
// scale codes go through LDS, the finished block is assembled there in 32-bit words (every field of every K block starts on a
// 4-byte boundary) and leaves as 16-bit words (every block size is even; rows are 2-byte aligned).
// kq_encode_wave contains two __syncthreads(): every wave of the workgroup calls it, a wave past the end of the tensor with
// zeros and its loads and stores predicated off.
#pragma once
#include "kquant.h"
#include "kquant2.h"
#include "quantize.h"

template <int KT>
struct KBlock {
    static constexpr int bytes = KT == KT_Q2_K ? 84 : KT == KT_Q3_K ? 110 : KT == KT_Q4_K ? 144 : KT == KT_Q5_K ? 176 : 210;
};

// a wave's LDS: the staged block (raw input of the add, then the encoded output), the codes, the sub-block scale / min codes
struct KqWave {
    uint32_t blk[53];  // 212 bytes >= the largest block
    uint32_t codes[64];
    uint8_t sc[16], mn[16];
};

template <int GL>  // aligned groups of 4 or 8 lanes
__device__ __forceinline__ float kq_gmin_f32(float v) {
    v = fminf(v, dpp_f32<DPP_QUAD_XOR1>(v));
    v = fminf(v, dpp_f32<DPP_QUAD_XOR2>(v));
    if constexpr (GL == 8) v = fminf(v, dpp_f32<DPP_ROW_HALF_MIRROR>(v));
    return v;
}
template <int GL>
__device__ __forceinline__ float kq_gmax_f32(float v) {
    v = fmaxf(v, dpp_f32<DPP_QUAD_XOR1>(v));
    v = fmaxf(v, dpp_f32<DPP_QUAD_XOR2>(v));
    if constexpr (GL == 8) v = fmaxf(v, dpp_f32<DPP_ROW_HALF_MIRROR>(v));
    return v;
}
__device__ __forceinline__ int kq_wave_min_i32(int v) {  // wave-uniform
    v = min(v, dpp_i32<DPP_QUAD_XOR1>(v));
    v = min(v, dpp_i32<DPP_QUAD_XOR2>(v));
    v = min(v, dpp_i32<DPP_ROW_HALF_MIRROR>(v));
    v = min(v, dpp_i32<DPP_ROW_MIRROR>(v));
    const int r0 = __builtin_amdgcn_readlane(v, 0), r1 = __builtin_amdgcn_readlane(v, 16), r2 = __builtin_amdgcn_readlane(v, 32),
              r3 = __builtin_amdgcn_readlane(v, 48);
    return min(min(r0, r1), min(r2, r3));
}
__device__ __forceinline__ uint32_t kq_f16_bits(float f) {
    asm volatile("" : "+v"(f));  // one f32 rounding of the operand, then one f16 rounding (q_put_f16)
    return (uint32_t)__half_as_ushort(__float2half_rn(f));
}
__device__ __forceinline__ float kq_f16_val(uint32_t bits) {
    float f = __half2float(__ushort_as_half((unsigned short)bits));
    asm volatile("" : "+v"(f));
    return f;
}
__device__ __forceinline__ int kq_clamp(int q, int lo, int hi) { return q < lo ? lo : q > hi ? hi : q; }

// One super-block: v = this lane's four values.  On return (after the function's last barrier) w.blk holds the raw block.
template <int KT>
__device__ __forceinline__ void kq_encode_wave(const f32x4 v, const int lane, KqWave &w) {
    uint32_t codes = 0, dword = 0;  // dword: d | dmin << 16
    if constexpr (KT == KT_Q2_K || KT == KT_Q4_K || KT == KT_Q5_K) {
        // quantize_row_q2_K / q4_K / q5_K: lo <= 0 <= hi per sub-block, scale = (hi - lo) / qmax, min = -lo
        constexpr int GL = KT == KT_Q2_K ? 4 : 8;
        constexpr int QMAX = KT == KT_Q2_K ? 3 : KT == KT_Q4_K ? 15 : 31, SMAX = KT == KT_Q2_K ? 15 : 63;
        float lo = kq_gmin_f32<GL>(fminf(fminf(v[0], v[1]), fminf(v[2], v[3])));
        float hi = kq_gmax_f32<GL>(fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
        lo = lo < 0.0f ? lo : 0.0f;  // the scans start at +0 and take strictly smaller / larger values only
        hi = hi > 0.0f ? hi : 0.0f;
        const float scale = __fdiv_rn(__fsub_rn(hi, lo), (float)QMAX), mn = -lo;
        float max_scale = wave_max_f32(scale), max_min = wave_max_f32(mn);
        max_scale = max_scale > 0.0f ? max_scale : 0.0f;
        max_min = max_min > 0.0f ? max_min : 0.0f;
        const float inv_scale = max_scale > 0.0f ? __fdiv_rn((float)SMAX, max_scale) : 0.0f;
        const float inv_min = max_min > 0.0f ? __fdiv_rn((float)SMAX, max_min) : 0.0f;
        const int ls = min(SMAX, __float2int_rn(__fmul_rn(inv_scale, scale))), lm = min(SMAX, __float2int_rn(__fmul_rn(inv_min, mn)));
        const uint32_t d16 = kq_f16_bits(__fdiv_rn(max_scale, (float)SMAX)), dmin16 = kq_f16_bits(__fdiv_rn(max_min, (float)SMAX));
        dword = d16 | (dmin16 << 16);
        const float d = __fmul_rn(kq_f16_val(d16), (float)ls), dm = __fmul_rn(kq_f16_val(dmin16), (float)lm);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int q = d != 0.0f ? __float2int_rn(__fdiv_rn(__fadd_rn(v[k], dm), d)) : 0;
            codes |= (uint32_t)kq_clamp(q, 0, QMAX) << (8 * k);
        }
        if ((lane & (GL - 1)) == 0) {
            w.sc[lane / GL] = (uint8_t)ls;
            w.mn[lane / GL] = (uint8_t)lm;
        }
    } else {
        // quantize_row_q3_K / q6_K: the first value of largest magnitude of a sub-block maps to -4 / -32, the first
        // sub-block scale of largest magnitude to -32 / -128
        constexpr bool Q6 = KT == KT_Q6_K;
        const float a0 = fabsf(v[0]), a1 = fabsf(v[1]), a2 = fabsf(v[2]), a3 = fabsf(v[3]);
        const float amax = kq_gmax_f32<4>(fmaxf(fmaxf(a0, a1), fmaxf(a2, a3)));
        int idx = 4 * lane + (a0 == amax ? 0 : a1 == amax ? 1 : a2 == amax ? 2 : a3 == amax ? 3 : 1024);
        const int k0 = idx & 3;
        float vmax = k0 == 0 ? v[0] : k0 == 1 ? v[1] : k0 == 2 ? v[2] : v[3];
        {
            const int oi = dpp_i32<DPP_QUAD_XOR1>(idx);
            const float ov = dpp_f32<DPP_QUAD_XOR1>(vmax);
            if (oi < idx) idx = oi, vmax = ov;
        }
        {
            const int oi = dpp_i32<DPP_QUAD_XOR2>(idx);
            const float ov = dpp_f32<DPP_QUAD_XOR2>(vmax);
            if (oi < idx) idx = oi, vmax = ov;
        }
        const float sc = amax > 0.0f ? __fdiv_rn(vmax, Q6 ? -32.0f : -4.0f) : 0.0f;
        const float asc = fabsf(sc), max_abs = wave_max_f32(asc);
        const int first = kq_wave_min_i32(asc == max_abs ? lane : 64) & 63;
        const float max_sc = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, sc), first));
        constexpr int bias = Q6 ? 32 : 4;  // codes are q + bias, q in -bias .. bias - 1
        int lcode;
        if (max_abs == 0.0f) {  // wave-uniform.  Q6_K: 210 zero bytes; Q3_K: d = 0, scales coded 32, q = 0 (hmask 0xFF)
            lcode = Q6 ? 0 : 32;
            codes = Q6 ? 0u : 0x04040404u;
        } else {
            const float iscale = __fdiv_rn(Q6 ? -128.0f : -32.0f, max_sc);
            dword = kq_f16_bits(__fdiv_rn(1.0f, iscale));
            int l = __float2int_rn(__fmul_rn(iscale, sc));
            l = Q6 ? min(127, l) : kq_clamp(l, -32, 31);
            const float d = __fmul_rn(kq_f16_val(dword), (float)l);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int q = d != 0.0f ? __float2int_rn(__fdiv_rn(v[k], d)) : 0;
                codes |= (uint32_t)(kq_clamp(q, -bias, bias - 1) + bias) << (8 * k);
            }
            lcode = Q6 ? l : l + 32;
        }
        if ((lane & 3) == 0) w.sc[lane >> 2] = (uint8_t)lcode;
    }
    w.codes[lane] = codes;
    __syncthreads();

    const uint32_t *c = w.codes;
    uint8_t *bb = (uint8_t *)w.blk;
    const int r = lane & 7;
    if constexpr (KT == KT_Q4_K || KT == KT_Q5_K) {  // d, dmin, scales[12] (set_scale_min_k4), [qh[32],] qs[128]
        if (lane < 32) {
            const int g = 16 * (lane >> 3) + r;
            w.blk[(KT == KT_Q4_K ? 4 : 12) + lane] = (c[g] & 0x0F0F0F0Fu) | ((c[g + 8] & 0x0F0F0F0Fu) << 4);
        }
        if constexpr (KT == KT_Q5_K)
            if (lane < 8) {
                uint32_t qh = 0;
#pragma unroll
                for (int g = 0; g < 8; g++) qh |= ((c[8 * g + lane] >> 4) & 0x01010101u) << g;
                w.blk[4 + lane] = qh;
            }
        if (lane < 12) {
            const int j = lane & 3, kind = lane >> 2;
            const uint32_t s0 = w.sc[j], s1 = w.sc[j + 4], m0 = w.mn[j], m1 = w.mn[j + 4];
            bb[4 + lane] = (uint8_t)(kind == 0 ? (s0 | ((s1 >> 4) << 6)) : kind == 1 ? (m0 | ((m1 >> 4) << 6)) : ((s1 & 0xF) | ((m1 & 0xF) << 4)));
        }
        if (lane == 0) w.blk[0] = dword;
    } else if constexpr (KT == KT_Q6_K) {  // ql[128], qh[64], scales[16], d
        const int g = 32 * (lane >> 4) + (lane & 15);
        if (lane < 32) w.blk[lane] = (c[g] & 0x0F0F0F0Fu) | ((c[g + 16] & 0x0F0F0F0Fu) << 4);
        if (lane < 16) {
            const int h = 32 * (lane >> 3) + r;
            w.blk[32 + lane] = ((c[h] >> 4) & 0x03030303u) | (((c[h + 8] >> 4) & 0x03030303u) << 2) |
                               (((c[h + 16] >> 4) & 0x03030303u) << 4) | (((c[h + 24] >> 4) & 0x03030303u) << 6);
        }
        if (lane < 4) w.blk[48 + lane] = ((const uint32_t *)w.sc)[lane];
        if (lane == 0) w.blk[52] = dword;
    } else {  // Q2_K: scales[16], qs[64], d, dmin.  Q3_K: hmask[32], qs[64], scales[12], d
        if (lane < 16) {
            const int h = 32 * (lane >> 3) + r;
            w.blk[(KT == KT_Q2_K ? 4 : 8) + lane] = (c[h] & 0x03030303u) | ((c[h + 8] & 0x03030303u) << 2) |
                                                    ((c[h + 16] & 0x03030303u) << 4) | ((c[h + 24] & 0x03030303u) << 6);
        }
        if constexpr (KT == KT_Q2_K) {
            if (lane < 16) bb[lane] = (uint8_t)(w.sc[lane] | (w.mn[lane] << 4));
            if (lane == 0) w.blk[20] = dword;
        } else {
            if (lane < 8) {  // bit b of hmask[m]: element 32 b + m has code > 3
                uint32_t hm = 0;
#pragma unroll
                for (int b = 0; b < 8; b++) hm |= ((c[8 * b + lane] >> 2) & 0x01010101u) << b;
                w.blk[lane] = hm;
            }
            if (lane < 12) {  // w.sc: the 6-bit codes l + 32 of the 16 sub-blocks
                const int b = lane & 3;
                bb[96 + lane] = lane < 8 ? (uint8_t)((w.sc[lane] & 0xF) | ((w.sc[lane + 8] & 0xF) << 4))
                                         : (uint8_t)((w.sc[b] >> 4) | ((w.sc[b + 4] >> 4) << 2) | ((w.sc[b + 8] >> 4) << 4) | ((w.sc[b + 12] >> 4) << 6));
            }
            if (lane == 0) w.blk[27] = dword;
        }
    }
    __syncthreads();
}

// the staged block of w.blk -> global memory, as 16-bit words
template <int KT>
__device__ __forceinline__ void kq_store_block(const KqWave &w, const int lane, uint16_t *o, const bool active) {
    const uint16_t *s = (const uint16_t *)w.blk;
    if (active)
        for (int i = lane; i < KBlock<KT>::bytes / 2; i += 64) o[i] = s[i];
}

// dequantize_row_q*_K for this lane's four elements of the raw block staged in w.blk: `d * sc` first, then `d1 * q - m1`
// with separate roundings; `d * sc * q` left to right for Q3_K / Q6_K
template <int KT>
__device__ __forceinline__ f32x4 kq_decode4(const KqWave &w, const int lane) {
    const uint8_t *bb = (const uint8_t *)w.blk;
    const int r = lane & 7, j = lane >> 3;  // j: the 32-element group
    f32x4 y;
    if constexpr (KT == KT_Q4_K || KT == KT_Q5_K) {
        const float d = kq_f16_val(w.blk[0] & 0xFFFFu), dmin = kq_f16_val(w.blk[0] >> 16);
        const uint8_t *p = bb + 4;
        uint32_t sc, m;  // get_scale_min_k4(j)
        if (j < 4) {
            sc = p[j] & 63u;
            m = p[j + 4] & 63u;
        } else {
            sc = (p[j + 4] & 0xFu) | ((uint32_t)(p[j - 4] >> 6) << 4);
            m = (uint32_t)(p[j + 4] >> 4) | ((uint32_t)(p[j] >> 6) << 4);
        }
        const float d1 = __fmul_rn(d, (float)sc), m1 = __fmul_rn(dmin, (float)m);
        uint32_t q = (w.blk[(KT == KT_Q4_K ? 4 : 12) + 8 * (j >> 1) + r] >> (4 * (j & 1))) & 0x0F0F0F0Fu;
        if constexpr (KT == KT_Q5_K) q |= ((w.blk[4 + r] >> j) & 0x01010101u) << 4;
#pragma unroll
        for (int k = 0; k < 4; k++) y[k] = __fsub_rn(__fmul_rn(d1, (float)((q >> (8 * k)) & 0xFFu)), m1);
    } else if constexpr (KT == KT_Q6_K) {
        const int n = lane >> 5, k4 = j & 3;
        const float d = kq_f16_val(w.blk[52] & 0xFFFFu);
        const int sc = (int)(int8_t)bb[192 + (lane >> 2)];
        const uint32_t lo = (w.blk[16 * n + 8 * (k4 & 1) + r] >> (4 * (k4 >> 1))) & 0x0F0F0F0Fu;
        const uint32_t hi = (w.blk[32 + 8 * n + r] >> (2 * k4)) & 0x03030303u;
        const uint32_t q = lo | (hi << 4);
        const float dl = __fmul_rn(d, (float)sc);
#pragma unroll
        for (int k = 0; k < 4; k++) y[k] = __fmul_rn(dl, (float)((int)((q >> (8 * k)) & 0xFFu) - 32));
    } else {
        const int n = lane >> 5, k4 = j & 3, is = lane >> 2;
        const uint32_t q = (w.blk[(KT == KT_Q2_K ? 4 : 8) + 8 * n + r] >> (2 * k4)) & 0x03030303u;
        if constexpr (KT == KT_Q2_K) {
            const float d = kq_f16_val(w.blk[20] & 0xFFFFu), dmin = kq_f16_val(w.blk[20] >> 16);
            const uint32_t sc = bb[is];
            const float dl = __fmul_rn(d, (float)(sc & 0xFu)), ml = __fmul_rn(dmin, (float)(sc >> 4));
#pragma unroll
            for (int k = 0; k < 4; k++) y[k] = __fsub_rn(__fmul_rn(dl, (float)((q >> (8 * k)) & 0xFFu)), ml);
        } else {
            const float d = kq_f16_val(w.blk[27] & 0xFFFFu);
            const uint8_t *p = bb + 96;  // q3_unpack_scales
            const uint32_t low4 = is < 8 ? (p[is] & 0xFu) : (uint32_t)(p[is - 8] >> 4), high2 = (p[8 + (is & 3)] >> (2 * (is >> 2))) & 3u;
            const float dl = __fmul_rn(d, (float)((int)(low4 | (high2 << 4)) - 32));
            const uint32_t hm = (w.blk[r] >> (4 * n + k4)) & 0x01010101u;  // bit clear: subtract 4
#pragma unroll
            for (int k = 0; k < 4; k++)
                y[k] = __fmul_rn(dl, (float)((int)((q >> (8 * k)) & 0xFFu) - (((hm >> (8 * k)) & 1u) ? 0 : 4)));
        }
    }
    return y;
}

// contiguous rows of f32 (or f16, widened exactly) -> raw super-blocks; four super-blocks per 256-thread workgroup
template <int KT, bool F16_SRC>
__global__ void __launch_bounds__(256) k_quantize_k(const void *__restrict__ src, int64_t nsb, uint8_t *__restrict__ out) {
    __shared__ KqWave s_w[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t sb = (int64_t)blockIdx.x * 4 + wv;
    const bool active = sb < nsb;
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (active) {
        if constexpr (F16_SRC) {
            const f16x4 h = ((const f16x4 *)src)[sb * 64 + lane];
            v[0] = (float)h[0]; v[1] = (float)h[1]; v[2] = (float)h[2]; v[3] = (float)h[3];
        } else {
            v = ((const f32x4 *)src)[sb * 64 + lane];
        }
    }
    kq_encode_wave<KT>(v, lane, s_w[wv]);
    kq_store_block<KT>(s_w[wv], lane, (uint16_t *)(out + (active ? sb : 0) * KBlock<KT>::bytes), active);
}
