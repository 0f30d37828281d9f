// mpt_batch.hip — the kernels of the batched MPT step (kernels/mpt_batch.h): k_mmq_cols' per-column Q|K|V store and the batched ALiBi
// decode attention, in an object and so a code object of their own, as mpt_chunk.hip is and for its reason: every other code object
// keeps its kernels at their addresses, and every other plan launches exactly what it launched.  The headers are included inside an
// unnamed namespace (see sample_ext.hip for what that costs and asks); this object's copy of c_act_quant_scalar is set with the others
// (mpt_batch_set_act_quant).
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <atomic>

#define MPT_BATCH_OBJECT
namespace {
#include "kernels/mpt_batch.h"

// dynamic LDS above 64 KiB is asked for once per device and kernel (two slots asking at once both ask: harmless)
static int lds_opt_in(const void *fn, std::atomic<bool> *done, size_t lds) {
    if (lds <= 64 * 1024) return 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 1;
    if (!done[dev & 63].load(std::memory_order_acquire)) {
        if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024) != hipSuccess) return 1;
        done[dev & 63].store(true, std::memory_order_release);
    }
    return 0;
}
template <int QT>
int cols_launch(hipStream_t stream, const ColsArgs &a, int G, size_t lds) {
    static std::atomic<bool> done[64] = {};
    if (lds_opt_in((const void *)k_mmq_cols<QT, EPI_QKV_TM_BATCH>, done, lds)) return 1;
    hipLaunchKernelGGL((k_mmq_cols<QT, EPI_QKV_TM_BATCH>), dim3((unsigned)G), dim3(COLS_T), lds, stream, a);
    return 0;
}
template <int D>
int batch_attn(hipStream_t stream, const MptBatchAttnArgs &a, size_t lds_dyn) {
    static std::atomic<bool> done[64] = {};
    if (lds_opt_in((const void *)k_attn_batch_vp_alibi<D>, done, lds_dyn)) return 1;
    const dim3 grid((unsigned)a.H, (unsigned)a.W);
    hipLaunchKernelGGL(k_attn_batch_scores_alibi<D>, grid, dim3(256), 0, stream, a);
    hipLaunchKernelGGL(k_attn_batch_vp_alibi<D>, grid, dim3(256), lds_dyn, stream, a);
    hipLaunchKernelGGL(k_attn_batch_merge_alibi, dim3((unsigned)a.B), dim3(256), 0, stream, a);
    return 0;
}
}  // namespace

int launch_mpt_batch_attn(hipStream_t stream, const void *args, size_t lds_dyn) {
    const MptBatchAttnArgs &a = *(const MptBatchAttnArgs *)args;
    switch (a.D) {
        case 32: return batch_attn<32>(stream, a, lds_dyn);
        case 64: return batch_attn<64>(stream, a, lds_dyn);
        case 128: return batch_attn<128>(stream, a, lds_dyn);
        default: return 1;
    }
}
int launch_mpt_batch_cols(hipStream_t stream, int qt, const void *cols_args, int G, size_t lds) {
    const ColsArgs &a = *(const ColsArgs *)cols_args;
    switch (qt) {
        case QT_Q4_0: return cols_launch<QT_Q4_0>(stream, a, G, lds);
        case QT_Q4_1: return cols_launch<QT_Q4_1>(stream, a, G, lds);
        case QT_Q5_0: return cols_launch<QT_Q5_0>(stream, a, G, lds);
        case QT_Q5_1: return cols_launch<QT_Q5_1>(stream, a, G, lds);
        case QT_Q8_0: return cols_launch<QT_Q8_0>(stream, a, G, lds);
        default: return 1;
    }
}
int mpt_batch_set_act_quant(int v) {
    return hipMemcpyToSymbol(HIP_SYMBOL(c_act_quant_scalar), &v, sizeof(v)) == hipSuccess ? 0 : 1;
}
