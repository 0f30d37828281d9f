// sample_req.hip — the kernels between two steps of the chains that stop (ggml_hip_decode_chain_requests, ggml_hip_decode_batch_requests):
// k_sample_next's REQ instantiations, which read parameters, bias table, end rule and column index through the call's SampleReqs
// (kernels/sample.h), and k_argmax_next_req.  An object and so a code object of their own, as sample_ext.hip is and for its reason:
// hip_backend.hip's code object and sample_ext.hip's keep their kernels at their addresses, and the existing chains launch exactly
// what they launched.  The headers are included inside an unnamed namespace (see sample_ext.hip for what that costs and asks).
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define SAMPLE_EXT_OBJECT
#define SAMPLE_REQ_OBJECT
namespace {
#include "kernels/sample.h"
}

// One launch per class of columns that is present (n_class[SAMPLE_DEFAULT .. SAMPLE_GREEDY] columns each; the table's lists say
// which).  Classes touch disjoint entries of every table, so their order does not matter.  The selection by V alone, as everywhere;
// Mirostat 2 beyond SELECT_CAP entries is declined by the callers: nothing is launched there.
void launch_next_token_req(hipStream_t stream, const int *n_class, const float *logits, int V, void *prm_, void *bc_, void *sc_, void *reqs,
                           int *out) {
    DecParams *prm = (DecParams *)prm_;
    BatchCols *bc = (BatchCols *)bc_;
    SampleCols *sc = (SampleCols *)sc_;
    unsigned long long *rng = (unsigned long long *)reqs;
    const dim3 block(1024);
    const bool chip = V <= SELECT_CAP;
    if (const int n = n_class[SAMPLE_DEFAULT]) {
        if (chip) hipLaunchKernelGGL((k_sample_next<true, SAMPLE_DEFAULT, true>), dim3((unsigned)n), block, 0, stream, logits, V, prm, bc, sc, rng, out);
        else hipLaunchKernelGGL((k_sample_next<false, SAMPLE_DEFAULT, true>), dim3((unsigned)n), block, 0, stream, logits, V, prm, bc, sc, rng, out);
    }
    if (const int n = n_class[SAMPLE_FULL]) {
        if (chip) hipLaunchKernelGGL((k_sample_next<true, SAMPLE_FULL, true>), dim3((unsigned)n), block, 0, stream, logits, V, prm, bc, sc, rng, out);
        else hipLaunchKernelGGL((k_sample_next<false, SAMPLE_FULL, true>), dim3((unsigned)n), block, 0, stream, logits, V, prm, bc, sc, rng, out);
    }
    if (const int n = n_class[SAMPLE_MIROSTAT]) {
        if (chip) hipLaunchKernelGGL((k_sample_next<true, SAMPLE_MIROSTAT, true>), dim3((unsigned)n), block, 0, stream, logits, V, prm, bc, sc, rng, out);
    }
    if (const int n = n_class[SAMPLE_GREEDY])
        hipLaunchKernelGGL(k_argmax_next_req, dim3((unsigned)n), block, 0, stream, logits, V, prm, bc, sc, (SampleReqs *)reqs, out);
}
