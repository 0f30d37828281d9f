// prompt_pack.h — the prompts of several sessions as ONE pass of the prompt plan (ggml_hip_prompt_pack, plan_pack.inc): R rows, segment
// i = rows [row0, row0 + N) of the packed activations = the N tokens session i appends at positions n_past .. n_past + N - 1 of its own
// cache.  Everything between the GEMMs of the prompt plan is row-local; the three launches that place a row in a sequence have their
// segment forms here:
//   k_rope_table_rows   row r's (cos, sin) table from a per-row position array (k_rope_table: "position n_past + r")
//   k_p_qkv_post_seg    k_p_qkv_post (kernels/prompt.h) with the rows' segments: K rows and V tiles go into each segment's own cache
//   k_p_attn_seg        kernels/prompt_attn.h: a workgroup reads (segment, query tile) from a table and runs the unchanged body
// The tables (PackSeg per layer, row -> segment and position, V tiles, attention tiles) are built on the host and uploaded once per call.
// The structures are compiled by the backend's host code too; the kernels are compiled into prompt_pack.hip's code object alone
// (PROMPT_PACK_OBJECT), so the other code objects hold what they held.
#pragma once
#include "decode.h"
#include "prompt_attn.h"

#define PACK_SEGS_MAX 64

// (PackSeg, the segment as the kernels read it — this layer's caches — is defined in prompt_attn.h, whose kernel takes it)
struct PackTile {
    int seg, at;  // V tiles: the tile's first token inside the segment (a multiple of 64); attention tiles: the query tile of the segment
};
struct PQkvPostSeg {
    float *q;
    const float *kf, *vf, *tab;  // [R][E], [R][Egqa], [R][Egqa] f32; tab [R][128] (k_rope_table_rows)
    const PackSeg *segs;         // this layer's
    const int *row_seg;          // [R]: the segment of row r
    const PackTile *vtiles;      // [vt_n]: 64-token tiles, none across two segments
    int R, E, Egqa, D;
    int64_t C;
    int nb_rope, vt_n, vt_m;
    int64_t part;
    int skip_q;
};

#ifndef PROMPT_PACK_OBJECT
// prompt_pack.hip; PQkvPostSeg and PAttnArgs as void *: their types are distinct types in the two objects (same definitions)
void launch_rope_table_rows(hipStream_t stream, int R, const int *pos, float theta_scale, float freq_scale, int half_d, float *out);
void launch_p_qkv_post_seg(hipStream_t stream, const void *args);
// D = 32 / 64 / 128, the 32-query form; segs: this layer's PackSeg table, tiles [n_tiles][2]; 0, or 1 = the LDS opt-in failed
int launch_p_attn_seg(hipStream_t stream, int D, const void *pattn_args, const void *segs, const int *tiles, int n_tiles, size_t lds);
#else
__global__ void __launch_bounds__(128) k_rope_table_rows(const int *__restrict__ pos, float theta_scale, float freq_scale, int half_d,
                                                         float *__restrict__ out) {
    const int kk = threadIdx.x, r = blockIdx.x;
    if (kk >= half_d) return;
    rope_table_pair(pos[r], r, kk, theta_scale, freq_scale, out);
}

// k_p_qkv_post with every row in its own segment.  Blocks [0, nb_rope): one thread per (row, two pairs) of Q and K, K stored at
// position n_past + n of the row's segment.  Blocks [nb_rope, ...): tile (vtiles[tn], channels 64 tm ..): up to 64 tokens of ONE
// segment, transposed through LDS; the paired store where the tile's first cache position is even.
__global__ void __launch_bounds__(256) k_p_qkv_post_seg(const PQkvPostSeg a) {
    __shared__ float s_t[64][65];
    const int b = blockIdx.x;
    if (b < a.nb_rope) {
        const int q4 = a.skip_q ? 0 : (a.E >> 2);
        const int per_tok = q4 + (a.Egqa >> 2);
        const int64_t idx = (int64_t)b * 256 + threadIdx.x;
        if (idx >= (int64_t)a.R * per_tok) return;
        const int n = (int)(idx / per_tok), pr = (int)(idx - (int64_t)n * per_tok);
        const bool is_k = pr >= q4;
        const int pi = 2 * (is_k ? pr - q4 : pr);
        const int kk = pi % (a.D >> 1);
        const f32x4 cs = *(const f32x4 *)(a.tab + (int64_t)n * 128 + 2 * kk);
        if (!is_k) {
            float *p = a.q + (int64_t)n * a.E + 2 * pi;
            f32x4 v = *(const f32x4 *)p;
            if (a.part) v = v + *(const f32x4 *)(p + a.part);
            f32x4 o;
            o[0] = v[0] * cs[0] - v[1] * cs[1];
            o[1] = v[0] * cs[1] + v[1] * cs[0];
            o[2] = v[2] * cs[2] - v[3] * cs[3];
            o[3] = v[2] * cs[3] + v[3] * cs[2];
            *(f32x4 *)p = o;
        } else {
            const PackSeg sg = a.segs[a.row_seg[n]];
            f32x4 v = *(const f32x4 *)(a.kf + (int64_t)n * a.Egqa + 2 * pi);
            if (a.part) v = v + *(const f32x4 *)(a.kf + a.part + (int64_t)n * a.Egqa + 2 * pi);
            const float o0 = v[0] * cs[0] - v[1] * cs[1], o1 = v[0] * cs[1] + v[1] * cs[0];
            const float o2 = v[2] * cs[2] - v[3] * cs[3], o3 = v[2] * cs[3] + v[3] * cs[2];
            __half2 h0, h1;
            h0.x = __float2half_rn(o0);
            h0.y = __float2half_rn(o1);
            h1.x = __float2half_rn(o2);
            h1.y = __float2half_rn(o3);
            __half2 *dst = (__half2 *)(sg.mem_k + ((int64_t)sg.n_past + (n - sg.row0)) * a.Egqa + 2 * pi);
            dst[0] = h0;
            dst[1] = h1;
        }
        return;
    }
    const int t = b - a.nb_rope, tn = t % a.vt_n, tm = t / a.vt_n;
    const PackTile tl = a.vtiles[tn];
    const PackSeg sg = a.segs[tl.seg];
    const int n0 = tl.at, m0 = tm * 64;  // n0: inside the segment
    const float *vf = a.vf + (int64_t)sg.row0 * a.Egqa;
    {
        const int c4 = threadIdx.x & 15, r = threadIdx.x >> 4;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int n = n0 + r + 16 * i, m = m0 + 4 * c4;
            f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
            if (n < sg.N && m < a.Egqa) {
                v = *(const f32x4 *)(vf + (int64_t)n * a.Egqa + m);
                if (a.part) v = v + *(const f32x4 *)(vf + a.part + (int64_t)n * a.Egqa + m);
            }
#pragma unroll
            for (int k = 0; k < 4; k++) s_t[r + 16 * i][4 * c4 + k] = v[k];
        }
    }
    __syncthreads();
    if ((((int64_t)sg.n_past + n0) & 1) == 0 && (a.C & 1) == 0) {  // uniform
        const int np = threadIdx.x & 31, mg = threadIdx.x >> 5;
        const int n = n0 + 2 * np;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int ml = mg + 8 * i, m = m0 + ml;
            if (m < a.Egqa && n < sg.N) {
                __half *dst = sg.mem_v + (int64_t)m * a.C + sg.n_past + n;
                const __half h0 = __float2half_rn(s_t[2 * np][ml]);
                if (n + 1 < sg.N) {
                    __half2 h2;
                    h2.x = h0;
                    h2.y = __float2half_rn(s_t[2 * np + 1][ml]);
                    *(__half2 *)dst = h2;
                } else {
                    *dst = h0;
                }
            }
        }
    } else {
        const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int m = m0 + ly + 4 * i, n = n0 + lx;
            if (n < sg.N && m < a.Egqa) sg.mem_v[(int64_t)m * a.C + sg.n_past + n] = __float2half_rn(s_t[lx][ly + 4 * i]);
        }
    }
}
#endif
