// mpt_plan.hip — the kernels of the MPT decode plan (kernels/mpt_plan.h): k_mmvq_big's LayerNorm-staged instantiations, the ALiBi
// decode attention over token-major K and V, and the staging dump of the test hook, in an object and so a code object of their own,
// as sample_ext.hip, sample_req.hip, pool_admit.hip and prompt_pack.hip are and for their reason: hip_backend.hip's code object keeps
// its kernels at their addresses, and every LLaMA plan launches exactly what it launched.  The headers are included inside an unnamed
// namespace (see sample_ext.hip for what that costs and asks).  One thing more than there: kernels/common.h's c_act_quant_scalar
// exists once per code object, so option act_quant is stored into this object's copy too (mpt_plan_set_act_quant).
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <atomic>

#define MPT_PLAN_OBJECT
namespace {
#include "kernels/mpt_plan.h"

template <int QT>
int big_lnorm(hipStream_t stream, int epi, const BigArgs &a, int G, size_t lds) {
    const dim3 grid((unsigned)G), block(BigX<XSRC_NORM>::NT);
    switch (epi) {
        case EPI_QKV_TM: hipLaunchKernelGGL((k_mmvq_big<QT, EPI_QKV_TM, XSRC_LNORM>), grid, block, lds, stream, a); return 0;
        case EPI_GELU: hipLaunchKernelGGL((k_mmvq_big<QT, EPI_GELU, XSRC_LNORM>), grid, block, lds, stream, a); return 0;
        case EPI_STORE: hipLaunchKernelGGL((k_mmvq_big<QT, EPI_STORE, XSRC_LNORM>), grid, block, lds, stream, a); return 0;
        default: return 1;
    }
}
// the dynamic LDS of the attention above the 64 KiB default: asked for once per device (two slots asking at once both ask: harmless)
int attn_opt_in(size_t lds) {
    static std::atomic<bool> done[64] = {};
    if (lds <= 64 * 1024) return 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 1;
    if (done[dev & 63].load(std::memory_order_acquire)) return 0;
    if (hipFuncSetAttribute((const void *)k_attn_decode_alibi, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024) != hipSuccess) return 1;
    done[dev & 63].store(true, std::memory_order_release);
    return 0;
}
}  // namespace

int launch_mpt_big(hipStream_t stream, int qt, int epi, const void *big_args, int G, size_t lds) {
    const BigArgs &a = *(const BigArgs *)big_args;
    switch (qt) {
        case QT_Q4_0: return big_lnorm<QT_Q4_0>(stream, epi, a, G, lds);
        case QT_Q4_1: return big_lnorm<QT_Q4_1>(stream, epi, a, G, lds);
        case QT_Q5_0: return big_lnorm<QT_Q5_0>(stream, epi, a, G, lds);
        case QT_Q5_1: return big_lnorm<QT_Q5_1>(stream, epi, a, G, lds);
        case QT_Q8_0: return big_lnorm<QT_Q8_0>(stream, epi, a, G, lds);
        default: return 1;
    }
}
int launch_mpt_attn(hipStream_t stream, int n_head, const float *q, const void *mem_k, const void *mem_v, const void *prm, float scale,
                    const float *slopes, int D, int64_t E, float *out, int64_t Clds, size_t lds) {
    if (attn_opt_in(lds)) return 1;
    hipLaunchKernelGGL(k_attn_decode_alibi, dim3((unsigned)n_head), dim3(1024), lds, stream, q, (const __half *)mem_k, (const __half *)mem_v,
                       (const DecParams *)prm, scale, slopes, D, E, out, Clds);
    return 0;
}
int launch_mpt_stage_dump(hipStream_t stream, int f16d, const void *big_args, void *lo, void *hi, float *d, int *sum, size_t lds) {
    const BigArgs &a = *(const BigArgs *)big_args;
    if (f16d)
        hipLaunchKernelGGL(k_lnorm_stage_dump<true>, dim3(1), dim3(1024), lds, stream, a, (i32x4 *)lo, (i32x4 *)hi, d, sum);
    else
        hipLaunchKernelGGL(k_lnorm_stage_dump<false>, dim3(1), dim3(1024), lds, stream, a, (i32x4 *)lo, (i32x4 *)hi, d, sum);
    return 0;
}
int mpt_plan_set_act_quant(int v) {
    return hipMemcpyToSymbol(HIP_SYMBOL(c_act_quant_scalar), &v, sizeof(v)) == hipSuccess ? 0 : 1;
}
