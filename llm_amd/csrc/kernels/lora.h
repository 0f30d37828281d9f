// ggml_add with a quantized or f16 src0 and an f32 src1: the last step of a LoRA patch, W = W + s·(B·A)
// (crates/llm-base/src/lora.rs:86-139; ggml's add_q_f32 / add_f16_f32, upstream ggml.c of the 2023-08 window).
//
// k_add_q<T>: one lane per 32-weight block of src0 (T = the ggml_type value: 2, 3, 6, 7, 8).  The lane reads the raw GGML
// block, dequantizes it as dequantize_row_q* does (`q * d`, `q * d + m`: separate multiply and add, the library is built
// with -ffp-contract=off), adds its 32 floats of src1 with one f32 rounding each, and requantizes with q_block
// (kernels/quantize.h): the `_reference` quantizers for the 4- and 5-bit types; for Q8_0 the branch the act_quant option
// selects (common.h), as every other from_float the device runs.  The block is held in registers between the read and
// the write, so dst may be src0 (ggml_add_inplace).
// k_add_f16: one lane per element, f16(f32(a) + b) with round to nearest even.
// k_add_k<KT>: the same for a K-quant src0 (Q2_K .. Q6_K), one wave per 256-weight super-block, four per workgroup.  The
// wave stages the raw super-block in LDS, each lane decodes its four elements as dequantize_row_q*_K does (kq_decode4),
// adds its four floats of src1 and the wave requantizes with kq_encode_wave (kernels/kquant_encode.h: the oracle's fit).
// The whole input block is in LDS before a byte of the output block is written, so dst may be src0 here too.
// Rows are addressed through nb[1..3] of each operand (the three have the same shape); elements within a row are
// contiguous.  k_add_q and k_add_f16 are memory bound, k_add_k by instruction issue at about half of k_add_q's bytes per
// second: bytes per block and per element, and the measurement, in DESIGN.md §4.7.
#pragma once
#include "kquant_encode.h"
#include "quantize.h"

template <int T>
struct AddQBlock {
    static constexpr int bytes = T == 2 ? 18 : T == 3 ? 20 : T == 6 ? 22 : T == 7 ? 24 : 34;
};

template <int T>
__global__ void __launch_bounds__(256) k_add_q(const TView a, const TView b, const TView d, int64_t blocks_per_row,
                                               int64_t nblocks) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= nblocks) return;
    const bool sc = aq_scalar();
    const int64_t blk = g % blocks_per_row, row = g / blocks_per_row;
    const int64_t i1 = row % a.ne[1], i23 = row / a.ne[1], i2 = i23 % a.ne[2], i3 = i23 / a.ne[2];
    constexpr int BS = AddQBlock<T>::bytes;
    const uint16_t *pa = (const uint16_t *)(a.p + i1 * a.nb[1] + i2 * a.nb[2] + i3 * a.nb[3] + blk * BS);
    const float *pb = (const float *)(b.p + i1 * b.nb[1] + i2 * b.nb[2] + i3 * b.nb[3]) + blk * 32;
    uint8_t *pd = (uint8_t *)(d.p + i1 * d.nb[1] + i2 * d.nb[2] + i3 * d.nb[3] + blk * BS);

    // the raw block, in 16-bit words (every block size is even; the host checked 2-byte alignment of rows and bases)
    uint16_t h[BS / 2];
#pragma unroll
    for (int i = 0; i < BS / 2; i++) h[i] = pa[i];
    auto byte = [&](int k) -> uint32_t { return (h[k >> 1] >> (8 * (k & 1))) & 0xFFu; };
    const float dd = __half2float(__ushort_as_half(h[0]));
    float y[32];
    if constexpr (T == 2) {  // Q4_0: d, qs[16]
#pragma unroll
        for (int j = 0; j < 16; j++) {
            y[j] = __fmul_rn((float)((int)(byte(2 + j) & 0x0F) - 8), dd);
            y[j + 16] = __fmul_rn((float)((int)(byte(2 + j) >> 4) - 8), dd);
        }
    } else if constexpr (T == 3) {  // Q4_1: d, m, qs[16]
        const float m = __half2float(__ushort_as_half(h[1]));
#pragma unroll
        for (int j = 0; j < 16; j++) {
            y[j] = __fadd_rn(__fmul_rn((float)(int)(byte(4 + j) & 0x0F), dd), m);
            y[j + 16] = __fadd_rn(__fmul_rn((float)(int)(byte(4 + j) >> 4), dd), m);
        }
    } else if constexpr (T == 6 || T == 7) {  // Q5_0: d, qh, qs[16] / Q5_1: d, m, qh, qs[16]
        constexpr bool one = T == 7;
        constexpr int oq = one ? 8 : 6;
        const uint32_t qh = one ? ((uint32_t)h[2] | ((uint32_t)h[3] << 16)) : ((uint32_t)h[1] | ((uint32_t)h[2] << 16));
        const float m = one ? __half2float(__ushort_as_half(h[1])) : 0.0f;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint32_t xh0 = ((qh >> j) << 4) & 0x10u, xh1 = (qh >> (j + 12)) & 0x10u;
            const int x0 = (int)((byte(oq + j) & 0x0F) | xh0), x1 = (int)((byte(oq + j) >> 4) | xh1);
            if constexpr (one) {
                y[j] = __fadd_rn(__fmul_rn((float)x0, dd), m);
                y[j + 16] = __fadd_rn(__fmul_rn((float)x1, dd), m);
            } else {
                y[j] = __fmul_rn((float)(x0 - 16), dd);
                y[j + 16] = __fmul_rn((float)(x1 - 16), dd);
            }
        }
    } else {  // Q8_0: d, qs[32] (int8)
#pragma unroll
        for (int j = 0; j < 32; j++) y[j] = __fmul_rn((float)(int8_t)byte(2 + j), dd);
    }
#pragma unroll
    for (int j = 0; j < 32; j++) y[j] = __fadd_rn(y[j], pb[j]);
    q_block(y, T, pd, nullptr, sc);
}

template <int KT>
__global__ void __launch_bounds__(256) k_add_k(const TView a, const TView b, const TView d, int64_t sb_per_row, int64_t nsb) {
    __shared__ KqWave s_w[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t g = (int64_t)blockIdx.x * 4 + wv;
    const bool active = g < nsb;  // a wave past the end runs the barriers on zeros; its loads and stores are predicated off
    const int64_t gg = active ? g : 0;
    const int64_t blk = gg % sb_per_row, row = gg / sb_per_row;
    const int64_t i1 = row % a.ne[1], i23 = row / a.ne[1], i2 = i23 % a.ne[2], i3 = i23 / a.ne[2];
    constexpr int BS = KBlock<KT>::bytes;
    const uint16_t *pa = (const uint16_t *)(a.p + i1 * a.nb[1] + i2 * a.nb[2] + i3 * a.nb[3] + blk * BS);
    const float *pb = (const float *)(b.p + i1 * b.nb[1] + i2 * b.nb[2] + i3 * b.nb[3]) + blk * 256 + 4 * lane;
    uint16_t *pd = (uint16_t *)(d.p + i1 * d.nb[1] + i2 * d.nb[2] + i3 * d.nb[3] + blk * BS);
    KqWave &w = s_w[wv];

    uint16_t *s16 = (uint16_t *)w.blk;
    for (int i = lane; i < BS / 2; i += 64) s16[i] = active ? pa[i] : (uint16_t)0;
    f32x4 x = {0.0f, 0.0f, 0.0f, 0.0f};
    if (active) x = f32x4{pb[0], pb[1], pb[2], pb[3]};  // rows of src1 are 4-byte aligned, no more is asserted
    __syncthreads();
    f32x4 y = kq_decode4<KT>(w, lane);
#pragma unroll
    for (int k = 0; k < 4; k++) y[k] = __fadd_rn(y[k], x[k]);
    kq_encode_wave<KT>(y, lane, w);  // its first barrier stands between the reads of w.blk above and the writes of the new block
    kq_store_block<KT>(w, lane, pd, active);
}

__global__ void __launch_bounds__(256) k_add_f16(const TView a, const TView b, const TView d, int64_t n) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const int64_t i0 = g % a.ne[0], row = g / a.ne[0];
    const int64_t i1 = row % a.ne[1], i23 = row / a.ne[1], i2 = i23 % a.ne[2], i3 = i23 / a.ne[2];
    const __half x = ((const __half *)(a.p + i1 * a.nb[1] + i2 * a.nb[2] + i3 * a.nb[3]))[i0];
    const float v = ((const float *)(b.p + i1 * b.nb[1] + i2 * b.nb[2] + i3 * b.nb[3]))[i0];
    float s = __fadd_rn(__half2float(x), v);
    asm volatile("" : "+v"(s));  // one f32 rounding, then one f16 rounding (no fused mixed-precision form)
    ((__half *)(d.p + i1 * d.nb[1] + i2 * d.nb[2] + i3 * d.nb[3]))[i0] = __float2half_rn(s);
}
