// prompt_pack.hip — the three segment-aware launches of ggml_hip_prompt_pack (kernels/prompt_pack.h): k_rope_table_rows,
// k_p_qkv_post_seg and k_p_attn_seg, in an object and so a code object of their own, as sample_ext.hip,
// sample_req.hip and pool_admit.hip are and for their reason: the other code objects keep their kernels at their addresses, and the
// one-session prompt plan launches exactly what it launched.  The headers are included inside an unnamed namespace (see
// sample_ext.hip for what that costs and asks).
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define PROMPT_PACK_OBJECT
namespace {
#include "kernels/prompt_pack.h"

// the dynamic LDS of k_p_attn above the 64 KiB default: asked for once per device and kernel
template <int D>
int attn_seg_opt_in(size_t lds) {
    static bool done[64] = {};
    if (lds <= 64 * 1024) return 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 1;
    if (done[dev & 63]) return 0;
    if (hipFuncSetAttribute((const void *)k_p_attn_seg<D>, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024) != hipSuccess)
        return 1;
    done[dev & 63] = true;
    return 0;
}
template <int D>
int attn_seg(hipStream_t stream, const PAttnArgs &pa, const PackSeg *segs, const int *tiles, int n_tiles, size_t lds) {
    if (attn_seg_opt_in<D>(lds)) return 1;
    hipLaunchKernelGGL(k_p_attn_seg<D>, dim3((unsigned)(n_tiles * pa.H)), dim3(256), lds, stream, pa, segs, tiles);
    return 0;
}
}  // namespace

void launch_rope_table_rows(hipStream_t stream, int R, const int *pos, float theta_scale, float freq_scale, int half_d, float *out) {
    hipLaunchKernelGGL(k_rope_table_rows, dim3((unsigned)R), dim3(128), 0, stream, pos, theta_scale, freq_scale, half_d, out);
}
void launch_p_qkv_post_seg(hipStream_t stream, const void *args) {
    const PQkvPostSeg &a = *(const PQkvPostSeg *)args;
    hipLaunchKernelGGL(k_p_qkv_post_seg, dim3((unsigned)(a.nb_rope + a.vt_n * a.vt_m)), dim3(256), 0, stream, a);
}
int launch_p_attn_seg(hipStream_t stream, int D, const void *pattn_args, const void *segs_, const int *tiles, int n_tiles, size_t lds) {
    const PAttnArgs &pa = *(const PAttnArgs *)pattn_args;
    const PackSeg *segs = (const PackSeg *)segs_;
    if (D == 128) return attn_seg<128>(stream, pa, segs, tiles, n_tiles, lds);
    if (D == 64) return attn_seg<64>(stream, pa, segs, tiles, n_tiles, lds);
    if (D == 32) return attn_seg<32>(stream, pa, segs, tiles, n_tiles, lds);
    return 1;
}
