// mpt_chunk.hip — the kernels of the MPT chunk plan (kernels/mpt_chunk.h): the LayerNorm that writes Q8 columns and k_mmq_cols' MPT
// instantiations (token-major Q|K|V store, GELU, the K-sliced residual add), in an object and so a code object of their own, as
// mpt_plan.hip and mpt_prompt.hip are and for their reason: hip_backend.hip's code object keeps its kernels at their addresses, and every
// other plan launches exactly what it launched.  The headers are included inside an unnamed namespace (see sample_ext.hip for what that
// costs and asks); this object's copy of c_act_quant_scalar is set with the others (mpt_chunk_set_act_quant).
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <atomic>

#define MPT_CHUNK_OBJECT
namespace {
#include "kernels/mpt_chunk.h"

// dynamic LDS above 64 KiB is asked for once per device and kernel (two slots asking at once both ask: harmless)
template <int QT, int EPI>
int cols_launch(hipStream_t stream, const ColsArgs &a, int G, size_t lds) {
    static std::atomic<bool> done[64] = {};
    if (lds > 64 * 1024) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return 1;
        if (!done[dev & 63].load(std::memory_order_acquire)) {
            if (hipFuncSetAttribute((const void *)k_mmq_cols<QT, EPI>, hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024) != hipSuccess) return 1;
            done[dev & 63].store(true, std::memory_order_release);
        }
    }
    hipLaunchKernelGGL((k_mmq_cols<QT, EPI>), dim3((unsigned)G), dim3(COLS_T), lds, stream, a);
    return 0;
}
template <int QT>
int cols_epi(hipStream_t stream, int epi, const ColsArgs &a, int G, size_t lds) {
    switch (epi) {
        case EPI_QKV_TM: return cols_launch<QT, EPI_QKV_TM>(stream, a, G, lds);
        case EPI_GELU: return cols_launch<QT, EPI_GELU>(stream, a, G, lds);
        case EPI_ADD_KS: return cols_launch<QT, EPI_ADD_KS>(stream, a, G, lds);
        default: return 1;
    }
}
template <int D>
int chunk_attn(hipStream_t stream, const MptChunkAttnArgs &a, int H, size_t lds) {
    static std::atomic<bool> done[64] = {};
    if (lds > 64 * 1024) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return 1;
        if (!done[dev & 63].load(std::memory_order_acquire)) {
            if (hipFuncSetAttribute((const void *)k_attn_chunk_vp_alibi<D>, hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024) != hipSuccess) return 1;
            done[dev & 63].store(true, std::memory_order_release);
        }
    }
    const dim3 grid((unsigned)H, (unsigned)a.S);
    hipLaunchKernelGGL(k_attn_chunk_scores_alibi<D>, grid, dim3(256), 0, stream, a);
    hipLaunchKernelGGL(k_attn_chunk_vp_alibi<D>, grid, dim3(256), lds, stream, a);
    hipLaunchKernelGGL(k_attn_chunk_merge_alibi, dim3((unsigned)a.N), dim3(256), 0, stream, a);
    return 0;
}
}  // namespace

int launch_mpt_chunk_attn(hipStream_t stream, const void *args, int H, size_t lds) {
    const MptChunkAttnArgs &a = *(const MptChunkAttnArgs *)args;
    switch (a.D) {
        case 32: return chunk_attn<32>(stream, a, H, lds);
        case 64: return chunk_attn<64>(stream, a, H, lds);
        case 128: return chunk_attn<128>(stream, a, H, lds);
        default: return 1;
    }
}
void launch_mpt_lnorm_cols(hipStream_t stream, bool f16d, const float *x, const float *w, float eps, int64_t E, int N, float *y_f32, int8_t *lo,
                           int8_t *hi, float *d, int *s, float *dT, int *sT) {
    const size_t lds = (size_t)E * 4;
    if (f16d)
        hipLaunchKernelGGL(k_lnorm_quant_cols<true>, dim3((unsigned)N), dim3(256), lds, stream, x, w, eps, (int)E, N, y_f32, lo, hi, d, s, dT, sT);
    else
        hipLaunchKernelGGL(k_lnorm_quant_cols<false>, dim3((unsigned)N), dim3(256), lds, stream, x, w, eps, (int)E, N, y_f32, lo, hi, d, s, dT, sT);
}
int launch_mpt_cols(hipStream_t stream, int qt, int epi, const void *cols_args, int G, size_t lds) {
    const ColsArgs &a = *(const ColsArgs *)cols_args;
    switch (qt) {
        case QT_Q4_0: return cols_epi<QT_Q4_0>(stream, epi, a, G, lds);
        case QT_Q4_1: return cols_epi<QT_Q4_1>(stream, epi, a, G, lds);
        case QT_Q5_0: return cols_epi<QT_Q5_0>(stream, epi, a, G, lds);
        case QT_Q5_1: return cols_epi<QT_Q5_1>(stream, epi, a, G, lds);
        case QT_Q8_0: return cols_epi<QT_Q8_0>(stream, epi, a, G, lds);
        default: return 1;
    }
}
int mpt_chunk_set_act_quant(int v) {
    return hipMemcpyToSymbol(HIP_SYMBOL(c_act_quant_scalar), &v, sizeof(v)) == hipSuccess ? 0 : 1;
}
