// prompt_attn.h — attention of a prompt batch in ONE launch: K.Q, scale + causal mask + softmax and V.P with the scores kept
// in LDS (crates/models/llama/src/lib.rs:246-299: mul_mat(K, Q) -> scale -> diag_mask_inf -> soft_max -> mul_mat(V, P) ->
// permute -> cpy, 7 graph nodes per layer).  The prompt plan ran them as three launches that moved the [H][N][T] scores
// through HBM twice (k_gemm_f16, k_p_soft_max, k_gemm_f16_b16: ~70 us of a 7B layer's ~480 at N = 512).
//
// ggml's softmax fixes its rounding points (row max first, e = f16(exp(f16(s*scale - max))), exact f64 sum, p = e * (1/sum),
// src1 of the V mat-mul rounded to f16), so this is not an online-softmax kernel: a workgroup owns 32 queries of one head,
// computes ALL their scores into LDS (32 rows x T f32), runs the row softmax there exactly as k_p_soft_max does, overwrites
// each row in place with its f16 probabilities and multiplies by V.  Both products use v_mfma_f32_32x32x16_f16 with the
// operand roles and k order of k_gemm_f16 (A = queries, B = keys / value channels, 16 k per instruction, ascending), so
// the result is bit-identical to the three-launch path (tests/test_prompt_plan_gpu.py).
//
//   grid = (ceil(N / 32) * H), 256 threads.  Dynamic LDS = 32 x (Tp * 4 + 16) bytes, Tp = (n_past + N) rounded up to 64,
//   (the staged Q tile, 32 x (2 D + 16) bytes, borrows the score rows before the S phase).
//   S phase: wave w takes key tiles w, w+4, ... of 32 keys (8 MFMAs for D = 128), K fragments straight from global / L2,
//            the next tile's fragments requested before the current tile's MFMAs.
//   softmax: wave w takes rows 8w .. 8w+7.
//   V.P    : wave w takes value channels 32w .. 32w+31 (D / 32 waves), V^T fragments from global, P fragments from LDS.
#pragma once
#include "gemm_f16.h"
#include "mmq.h"

struct PAttnArgs {
    const float *q;      // [N][E] f32, RoPE applied
    const __half *mem_k; // this layer: [C][Egqa]
    const __half *mem_v; // this layer: [Egqa][C]
    float *out;          // [N][E] f32, merged heads
    int N, E, Egqa, H, r, n_past;
    int64_t C;
    float scale;
    int row_bytes;       // LDS bytes per score row
    const float *rope;   // != nullptr: q is the raw wq product; RoPE (cos, sin per pair: 128 floats per token, k_rope_table) is
                         // applied while its fragments are loaded — k_p_qkv_post's operations on the same values
    int64_t q_part;      // != 0: ... and q is the first partial of a K-split GEMM, the second lies q_part floats on
    _Float16 *x16;       // != nullptr: the output goes out as wo's GEMM operand instead — every 32-channel block re-quantized to Q8
                         // and written as f16(d * q) in the GEMM's k order (what k_p_quant4 makes of `out`); `out` is not written
    int f16d;            // ... with the block scale rounded to f16 first (weight types whose vec_dot_type is Q8_0)
    int r1;              // query-tile ranks (blockIdx / H) dealt longest-first; the ranks behind them go shortest-first (see the kernel)
    long long *ts;       // INSTR build (option "timeline"): 8 x int64 per workgroup, see tests/tools/pattn_timeline.py
};

// a segment of a packed prompt batch (kernels/prompt_pack.h): rows [row0, row0 + N) of the packed activations are positions
// n_past .. n_past + N - 1 of the session whose caches (this layer's) are mem_k / mem_v
struct PackSeg {
    __half *mem_k, *mem_v;
    int row0, N, n_past, pad;
};

#define PATTN_Q 32

// expf for the softmax's arguments: x = f16(score - row maximum), so x <= 0 (or NaN for a masked column's garbage, which is selected
// away).  The operations of the device library's expf (ph = x * log2e rounded; pl = its error by two fmas with log2e's head and tail;
// e = rint(ph); 2^((ph - e) + pl) by v_exp_f32; ldexp by e) with ONE clamp in place of its two range checks (x < -103.28 -> 0,
// x > 88.72 -> inf: two compares, two selects and their wait states per element): the second cannot fire; below -104 (f16's -inf
// included: inf - inf inside the sequence would make a NaN of it) the argument is held at -104, whose result (7e-46) rounds to the
// same f16 zero the library's branch returns.  A NaN stays a NaN.  Same f16 bits as f16(expf(x)) for every f16 x <= 0 and every
// NaN: tests/test_prompt_plan_gpu.py checks all 2^15 + 1 of them on the device (ggml_hip_debug_exp_le0).
__device__ __forceinline__ float exp_le0(const float x0) {
    const float c = 0x1.715476p+0f, cc = 0x1.4ae0bep-26f;  // log2(e): head and tail
    const float x = x0 < -104.0f ? -104.0f : x0;
    const float ph = x * c;
    float pl = __builtin_fmaf(x, c, -ph);
    pl = __builtin_fmaf(x, cc, pl);
    const float e = __builtin_rintf(ph);
    const float a_ = (ph - e) + pl;
    return __builtin_amdgcn_ldexpf(__builtin_amdgcn_exp2f(a_), (int)e);
}

// p = f16(f32(e * inv)): ggml's soft_max stores the f32 product and the V mat-mul converts THAT to f16, two roundings.  Written as
// (_Float16)(e * inv) the compiler selects v_fma_mixlo_f16 — the product rounded ONCE, straight to f16 (-ffp-contract=off does not
// stop it: no addend is contracted) — which lands one f16 ulp off wherever the f32 rounding moves the product onto an f16 tie
// (tests/test_prompt_attn_gpu.py found it: exact scores, T = 17, p 0x1270 expected, 0x126f computed).  The empty asm makes the f32
// product a value of its own; k_p_soft_max's product already is one (it feeds an f32 store as well).
__device__ __forceinline__ _Float16 f16_of_f32_product(float a, float b) {
    float t = a * b;
    asm("" : "+v"(t));
    return (_Float16)t;
}

// QR = queries per workgroup: 32, or 16 for rows too long for 32 score rows in LDS (T up to ~2300 keys: the last chunks of a
// 2048-token context; the MFMA tiles stay 32 rows high, their upper half computes on duplicated queries and is dropped)
// The body is prompt_attn_body.h, shared with k_p_attn_seg below.  The segment flag is a constant of the including kernel, not a template
// parameter of this one: another parameter renames every instantiation, the longer names moved the code object's .text by 256 bytes,
// and kernels of this code object that move have cost the single-token plans 3 % before.  This way the code object
// is byte for byte what it was.
template <int D, bool INSTR = false, int QR = PATTN_Q>
__global__ void __launch_bounds__(256, 2) k_p_attn(const PAttnArgs a) {
    constexpr bool SEG = false;
    constexpr int seg_qt = 0;
#include "prompt_attn_body.h"
}
// The segment form (instantiated in prompt_pack.hip alone): the launch covers the rows of several sessions.  Workgroup rank
// blockIdx / H reads (segment, query tile) from `tiles` ([grid / H][2]; the host has put the table in dealing order, so r1 is not
// consulted), takes the caches, N and n_past from the segment (`segs`: this layer's table) and moves q / rope / out / x16 to the
// segment's first row; then the same body: same MFMA operand roles and k order, same rounding points, same epilogue.
template <int D>
__global__ void __launch_bounds__(256, 2) k_p_attn_seg(const PAttnArgs a_, const PackSeg *__restrict__ segs, const int *__restrict__ tiles) {
    constexpr bool SEG = true, INSTR = false;
    constexpr int QR = PATTN_Q;
    const int seg_rank = (int)blockIdx.x / a_.H;
    const PackSeg sg = segs[tiles[2 * seg_rank]];
    const int seg_qt = tiles[2 * seg_rank + 1];
    PAttnArgs a = a_;
    a.q = a_.q + (int64_t)sg.row0 * a_.E;
    if (a_.rope) a.rope = a_.rope + (int64_t)sg.row0 * 128;
    if (a_.out) a.out = a_.out + (int64_t)sg.row0 * a_.E;
    if (a_.x16) a.x16 = a_.x16 + (int64_t)sg.row0 * a_.E;
    a.mem_k = sg.mem_k;
    a.mem_v = sg.mem_v;
    a.N = sg.N;
    a.n_past = sg.n_past;
#include "prompt_attn_body.h"
}
