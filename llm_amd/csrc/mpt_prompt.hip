// mpt_prompt.hip — the kernels of the MPT prompt plan (kernels/mpt_prompt.h): the LayerNorm and GELU operands, the token-major K/V
// store and the ALiBi prompt attention (both forms), in an object and so a code object of their own, as mpt_plan.hip and prompt_pack.hip are and
// for their reason: hip_backend.hip's code object keeps its kernels at their addresses, and every other plan launches exactly what
// it launched.  The headers are included inside an unnamed namespace (see sample_ext.hip for what that costs and asks); this object's
// copy of c_act_quant_scalar is set with the others (mpt_prompt_set_act_quant).
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <atomic>

#define MPT_PROMPT_OBJECT
namespace {
#include "kernels/mpt_prompt.h"

// the dynamic LDS of an attention instantiation above the 64 KiB default: asked for once per device and instantiation
template <int D, int QR>
int attn_launch(hipStream_t stream, const MptAttnArgs &a, unsigned grid, size_t lds) {
    static std::atomic<bool> done[64] = {};
    if (lds > MPT_ATTN_LDS_MAX) return 1;
    if (lds > 64 * 1024) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return 1;
        if (!done[dev & 63].load(std::memory_order_acquire)) {
            if (hipFuncSetAttribute((const void *)k_p_attn_alibi<D, QR>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)MPT_ATTN_LDS_MAX) != hipSuccess)
                return 1;
            done[dev & 63].store(true, std::memory_order_release);
        }
    }
    hipLaunchKernelGGL((k_p_attn_alibi<D, QR>), dim3(grid), dim3(256), lds, stream, a);
    return 0;
}
template <bool F16_D>
void lnorm(hipStream_t stream, const float *x, const float *x2, const float *r, float *xsum, const float *w, float eps, int64_t E, int64_t N,
           _Float16 *out) {
    if (r)
        hipLaunchKernelGGL((k_p_lnorm_quant<F16_D, true>), dim3((unsigned)N), dim3(256), (size_t)E * 4, stream, x, x2, r, xsum, w, eps, (int)E, out);
    else
        hipLaunchKernelGGL((k_p_lnorm_quant<F16_D, false>), dim3((unsigned)N), dim3(256), (size_t)E * 4, stream, x, x2, r, xsum, w, eps, (int)E, out);
}
}  // namespace

void launch_mpt_lnorm_quant(hipStream_t stream, int f16d, const float *x, const float *x2, const float *r, float *xsum, const float *w, float eps,
                            int64_t E, int64_t N, _Float16 *out) {
    if (f16d)
        lnorm<true>(stream, x, x2, r, xsum, w, eps, E, N, out);
    else
        lnorm<false>(stream, x, x2, r, xsum, w, eps, E, N, out);
}
void launch_mpt_qkv_post_tm(hipStream_t stream, const float *qkv, int64_t part, void *mem_k, void *mem_v, int N, int64_t E, int n_past) {
    const int64_t n = (int64_t)N * (E / 2);
    hipLaunchKernelGGL(k_p_qkv_post_tm, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, qkv, part, (__half *)mem_k, (__half *)mem_v, N, (int)E,
                       n_past);
}
void launch_mpt_gelu_quant(hipStream_t stream, int f16d, const float *a, int64_t n4, int64_t part4, _Float16 *out) {
    const dim3 grid((unsigned)((n4 + 255) / 256));
    if (f16d)
        hipLaunchKernelGGL(k_p_gelu_quant<true>, grid, dim3(256), 0, stream, (const f32x4 *)a, n4, part4, out);
    else
        hipLaunchKernelGGL(k_p_gelu_quant<false>, grid, dim3(256), 0, stream, (const f32x4 *)a, n4, part4, out);
}
int launch_mpt_attn_alibi(hipStream_t stream, int D, int QR, const void *args, unsigned grid, size_t lds) {
    const MptAttnArgs &a = *(const MptAttnArgs *)args;
    if (QR == 32) {
        if (D == 128) return attn_launch<128, 32>(stream, a, grid, lds);
        if (D == 64) return attn_launch<64, 32>(stream, a, grid, lds);
        if (D == 32) return attn_launch<32, 32>(stream, a, grid, lds);
    } else if (QR == 16) {
        if (D == 128) return attn_launch<128, 16>(stream, a, grid, lds);
        if (D == 64) return attn_launch<64, 16>(stream, a, grid, lds);
        if (D == 32) return attn_launch<32, 16>(stream, a, grid, lds);
    }
    return 1;
}
int launch_mpt_attn_alibi_stream(hipStream_t stream, int D, const void *args, unsigned grid) {
    const MptAttnArgs &a = *(const MptAttnArgs *)args;
    if (D == 128)
        hipLaunchKernelGGL(k_p_attn_alibi_stream<128>, dim3(grid), dim3(256), 0, stream, a);
    else if (D == 64)
        hipLaunchKernelGGL(k_p_attn_alibi_stream<64>, dim3(grid), dim3(256), 0, stream, a);
    else if (D == 32)
        hipLaunchKernelGGL(k_p_attn_alibi_stream<32>, dim3(grid), dim3(256), 0, stream, a);
    else
        return 1;
    return 0;
}
int mpt_prompt_set_act_quant(int v) {
    return hipMemcpyToSymbol(HIP_SYMBOL(c_act_quant_scalar), &v, sizeof(v)) == hipSuccess ? 0 : 1;
}
