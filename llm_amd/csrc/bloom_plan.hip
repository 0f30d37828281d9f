// bloom_plan.hip — the kernels of the BLOOM decode plan (kernels/bloom_plan.h): k_mmvq_big's instantiations with the biased LayerNorm staging
// and the biased epilogues, the embedding launch with its LayerNorm, and the staging dump of the test hook, in an object and so a code object
// of their own, as mpt_plan.hip is and for its reason: every other code object keeps its kernels at their addresses, and every other plan
// launches exactly what it launched.  The headers are included inside an unnamed namespace (see sample_ext.hip for what that costs and
// asks); kernels/common.h's c_act_quant_scalar exists once per code object, so option act_quant is stored into this object's copy too
// (bloom_plan_set_act_quant).
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define BLOOM_PLAN_OBJECT
namespace {
#include "kernels/bloom_plan.h"

template <int QT>
int big_bloom(hipStream_t stream, int epi, int xsrc, const BigArgs &a, int G, int threads, size_t lds) {
    const dim3 grid((unsigned)G), block((unsigned)threads);
    if (xsrc == XSRC_F32 && epi == EPI_ADD_B) {
        hipLaunchKernelGGL((k_mmvq_big<QT, EPI_ADD_B, XSRC_F32>), grid, block, lds, stream, a);
        return 0;
    }
    if (xsrc != XSRC_LNORM_B || threads != BigX<XSRC_NORM>::NT) return 1;  // (the norm is staged by all 16 waves)
    switch (epi) {
        case EPI_QKV_TM_B: hipLaunchKernelGGL((k_mmvq_big<QT, EPI_QKV_TM_B, XSRC_LNORM_B>), grid, block, lds, stream, a); return 0;
        case EPI_GELU_B: hipLaunchKernelGGL((k_mmvq_big<QT, EPI_GELU_B, XSRC_LNORM_B>), grid, block, lds, stream, a); return 0;
        case EPI_STORE: hipLaunchKernelGGL((k_mmvq_big<QT, EPI_STORE, XSRC_LNORM_B>), grid, block, lds, stream, a); return 0;
        default: return 1;
    }
}
template <int QT>
int embed_bloom(hipStream_t stream, const QWeight &w, const int *ids, const float *gain, const float *bias, float eps, float *dst) {
    hipLaunchKernelGGL(k_get_rows_lnorm<QT>, dim3(1), dim3(1024), 0, stream, w, ids, gain, bias, eps, dst);
    return 0;
}
}  // namespace

int launch_bloom_big(hipStream_t stream, int qt, int epi, int xsrc, const void *big_args, int G, int threads, size_t lds) {
    const BigArgs &a = *(const BigArgs *)big_args;
    switch (qt) {
        case QT_Q4_0: return big_bloom<QT_Q4_0>(stream, epi, xsrc, a, G, threads, lds);
        case QT_Q4_1: return big_bloom<QT_Q4_1>(stream, epi, xsrc, a, G, threads, lds);
        case QT_Q5_0: return big_bloom<QT_Q5_0>(stream, epi, xsrc, a, G, threads, lds);
        case QT_Q5_1: return big_bloom<QT_Q5_1>(stream, epi, xsrc, a, G, threads, lds);
        case QT_Q8_0: return big_bloom<QT_Q8_0>(stream, epi, xsrc, a, G, threads, lds);
        default: return 1;
    }
}
int launch_bloom_embed(hipStream_t stream, int qt, const void *wte, const int *ids, const float *gain, const float *bias, float eps, float *dst) {
    const QWeight &w = *(const QWeight *)wte;
    if (w.nb < 1 || w.nb > 256) return 1;  // (two f32x4 per thread: rows up to 8192 wide)
    switch (qt) {
        case QT_Q4_0: return embed_bloom<QT_Q4_0>(stream, w, ids, gain, bias, eps, dst);
        case QT_Q4_1: return embed_bloom<QT_Q4_1>(stream, w, ids, gain, bias, eps, dst);
        case QT_Q5_0: return embed_bloom<QT_Q5_0>(stream, w, ids, gain, bias, eps, dst);
        case QT_Q5_1: return embed_bloom<QT_Q5_1>(stream, w, ids, gain, bias, eps, dst);
        case QT_Q8_0: return embed_bloom<QT_Q8_0>(stream, w, ids, gain, bias, eps, dst);
        default: return 1;
    }
}
int launch_bloom_stage_dump(hipStream_t stream, int f16d, const void *big_args, void *lo, void *hi, float *d, int *sum, size_t lds) {
    const BigArgs &a = *(const BigArgs *)big_args;
    if (f16d)
        hipLaunchKernelGGL(k_lnorm_b_stage_dump<true>, dim3(1), dim3(1024), lds, stream, a, (i32x4 *)lo, (i32x4 *)hi, d, sum);
    else
        hipLaunchKernelGGL(k_lnorm_b_stage_dump<false>, dim3(1), dim3(1024), lds, stream, a, (i32x4 *)lo, (i32x4 *)hi, d, sum);
    return 0;
}
int bloom_plan_set_act_quant(int v) {
    return hipMemcpyToSymbol(HIP_SYMBOL(c_act_quant_scalar), &v, sizeof(v)) == hipSuccess ? 0 : 1;
}
