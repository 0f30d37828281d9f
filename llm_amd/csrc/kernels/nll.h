// Probability of ONE token per logits row on the device: prob[r] = util::softmax(x[r])[t[r]] of the reference
// (crates/llm-base/src/util.rs:143-151), which InferenceSession::perplexity (inference_session.rs:577-583) evaluates for every
// counted position after reading all n_vocab logits of the row to the host.  Here the row stays in HBM and 4 bytes come back.
//
//     prob[r] = expf(x[r][t] - max_r) / sum_j expf(x[r][j] - max_r)         max_r = max_j x[r][j]
//
// One 1024-thread workgroup per row.  Lane l owns the elements l, l + 1024, l + 2048, ... (coalesced dword loads: a row of
// 50257 floats is neither a multiple of 4 long nor 16-byte aligned).  KEEP: the row is read ONCE into ROW_PROB_KEEP registers
// per lane (V <= 32768: 32000 is 32 floats a lane); otherwise the second pass reads the row again (from L2: a row is <= a few
// hundred KB).  VEC (with KEEP; the host sets it when every row is 16-byte aligned and V % 4 == 0, LLaMA's 32000): lane l owns the
// float4s l, l + 1024, ... instead, 16 bytes per lane and load: 4 * ceil(V / 4096) elements per lane, added in index order.
// Max: per lane, wave_max_f32, 16 wave results through LDS.  Sum in f32: each lane adds its exponentials in sequence
// (ceil(V / 1024) of them; with VEC up to 4 * ceil(V / 4096), which exceeds that by at most 3 and only while V < 4096, where
// ceil(V / 4) < 1024 lanes hold anything and the tree over them is at least 2 levels shallower: sequential adds + tree levels
// never exceed ceil(V / 1024) + 10), then a tree of log2(1024) = 10 levels: 6 inside the wave (wave_sum_f32), 4 over the 16
// wave results, which lane 0 alone adds.  The accurate expf (1 ulp), no fast-math: the launch is bound by reading the row, not
// by the VALU.
//
// Edges, as the reference's expression gives them: fmaxf ignores NaN like f32::max, so a NaN entry reaches the sum and the row's
// result is NaN; -inf entries add exp(-inf) = 0; a target far below the maximum underflows to exactly 0 (the caller's -ln gives
// +inf); a row of -inf only, or one holding +inf, gives NaN (inf - inf).  A target outside [0, V) never reads: NaN (the host
// hook has refused it before the launch).
#pragma once
#include "common.h"

#define ROW_PROB_KEEP 32

template <bool KEEP, bool VEC>
__global__ void __launch_bounds__(1024) k_row_prob(const float *__restrict__ x, long long row_stride, int V,
                                                   const int *__restrict__ targets, float *__restrict__ out) {
    __shared__ float s_part[16];
    const int tid = threadIdx.x, wave = tid >> 6;
    const float *row = x + (long long)blockIdx.x * row_stride;
    float v[ROW_PROB_KEEP];
    float mx = -INFINITY;
    if (KEEP && VEC) {
        const float4 *row4 = (const float4 *)row;
#pragma unroll
        for (int k = 0; k < ROW_PROB_KEEP / 4; k++) {
            const int i = tid + k * 1024;
            const float4 q = i < (V >> 2) ? row4[i] : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
            v[4 * k] = q.x, v[4 * k + 1] = q.y, v[4 * k + 2] = q.z, v[4 * k + 3] = q.w;
            mx = fmaxf(fmaxf(mx, fmaxf(q.x, q.y)), fmaxf(q.z, q.w));
        }
    } else if (KEEP) {
#pragma unroll
        for (int k = 0; k < ROW_PROB_KEEP; k++) {
            const int i = tid + k * 1024;
            v[k] = i < V ? row[i] : -INFINITY;
            mx = fmaxf(mx, v[k]);
        }
    } else {
        for (long long i = tid; i < V; i += 1024) mx = fmaxf(mx, row[i]);
    }
    mx = wave_max_f32(mx);
    if ((tid & 63) == 0) s_part[wave] = mx;
    __syncthreads();
    mx = s_part[0];
#pragma unroll
    for (int w = 1; w < 16; w++) mx = fmaxf(mx, s_part[w]);
    __syncthreads();  // everyone has read the maxima: s_part is reused for the sums
    float s = 0.0f;
    if (KEEP) {
#pragma unroll
        for (int k = 0; k < ROW_PROB_KEEP; k++)
            if (VEC ? tid + (k >> 2) * 1024 < (V >> 2) : tid + k * 1024 < V) s += expf(v[k] - mx);
    } else {
        for (long long i = tid; i < V; i += 1024) s += expf(row[i] - mx);
    }
    s = wave_sum_f32(s);
    if ((tid & 63) == 0) s_part[wave] = s;
    __syncthreads();
    if (tid == 0) {
        float p[16];
#pragma unroll
        for (int w = 0; w < 16; w++) p[w] = s_part[w];
#pragma unroll
        for (int step = 1; step < 16; step <<= 1)
#pragma unroll
            for (int w = 0; w < 16; w += 2 * step) p[w] += p[w + step];
        const int t = targets[blockIdx.x];
        out[blockIdx.x] = (unsigned)t < (unsigned)V ? expf(row[t] - mx) / p[0] : NAN;
    }
}
