// sample_ext.hip — k_sample_next's instantiations for the whole sampler (kernels/sample.h: SAMPLE_FULL, the truncating chain with bias,
// frequency / presence penalty, tail-free, locally typical and min-p; SAMPLE_MIROSTAT, Mirostat 2), in an object and so a code object
// of their own.  hip_backend.hip's code object, which holds every other kernel, is then what it was before these existed: same
// kernels at the same addresses.  (With the three instantiations inside it every kernel behind them moved by 94 KB and the
// single-token plans ran 3 % slower at every leg of tests/tools/sample_chain.py, the greedy chain included — DESIGN section 3.)
// The kernel headers are included inside an unnamed namespace: everything in them gets internal linkage here, so nothing collides
// with hip_backend.hip's copies at link time.  The price: the 17 non-template kernels those headers define (k_norm, k_rope, k_argmax_next
// ...) are emitted into this code object a second time, never launched from here; and every system header they include must be included
// above the namespace first — a kernel header that gains an #include needs it added here too.  DecParams, BatchCols and SampleCols are
// therefore distinct types in the two objects (same definitions): launch_sample_next_ext takes them as void * on purpose.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define SAMPLE_EXT_OBJECT
namespace {
#include "kernels/sample.h"
}

// B columns; stages is SAMPLE_FULL or SAMPLE_MIROSTAT (which the callers decline beyond SELECT_CAP entries: nothing is launched there)
void launch_sample_next_ext(hipStream_t stream, int B, const float *logits, int V, void *prm_, void *bc_, void *sc_, void *state, int *out,
                            int stages) {
    DecParams *prm = (DecParams *)prm_;
    BatchCols *bc = (BatchCols *)bc_;
    SampleCols *sc = (SampleCols *)sc_;
    unsigned long long *rng = (unsigned long long *)state;
    const dim3 grid((unsigned)B), block(1024);
    if (stages == SAMPLE_MIROSTAT) {
        if (V <= SELECT_CAP) hipLaunchKernelGGL((k_sample_next<true, SAMPLE_MIROSTAT>), grid, block, 0, stream, logits, V, prm, bc, sc, rng, out);
    } else if (V <= SELECT_CAP) {
        hipLaunchKernelGGL((k_sample_next<true, SAMPLE_FULL>), grid, block, 0, stream, logits, V, prm, bc, sc, rng, out);
    } else {
        hipLaunchKernelGGL((k_sample_next<false, SAMPLE_FULL>), grid, block, 0, stream, logits, V, prm, bc, sc, rng, out);
    }
}
