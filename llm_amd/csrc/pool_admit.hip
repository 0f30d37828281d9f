// pool_admit.hip — k_pool_admit (kernels/pool_admit.h), the kernel behind the tail of every step of ggml_hip_decode_pool_requests, in an
// object and so a code object of its own, as sample_ext.hip and sample_req.hip are and for their reason: the code objects of
// hip_backend.hip, sample_ext.hip and sample_req.hip keep their kernels at their addresses.  The headers are included inside an
// unnamed namespace (see sample_ext.hip for what that costs and asks).
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define SAMPLE_EXT_OBJECT
#define POOL_ADMIT_OBJECT
namespace {
#include "kernels/pool_admit.h"
}

// One workgroup, whatever the number of columns (kernels/pool_admit.h says why).  The tables are passed as void *: their types are
// distinct types in the two objects (same definitions).
void launch_pool_admit(hipStream_t stream, void *table, void *reqs, void *sc, void *prm, void *bc, const float *logits, const float *emb, int V,
                       int E, float *slot_logits, float *slot_emb) {
    hipLaunchKernelGGL(k_pool_admit, dim3(1), dim3(1024), 0, stream, (PoolTable *)table, (SampleReqs *)reqs, (SampleCols *)sc, (DecParams *)prm,
                       (BatchCols *)bc, logits, emb, V, E, slot_logits, slot_emb);
}
