/*
 * ggml_hip.h — C ABI of libggml_hip.so, the MI355X-native drop-in for the one hot path of
 * rustformers/llm: ggml_compute_forward_mul_mat over Q4_0/Q4_1/Q5_0/Q5_1/Q8_0 (+F16 attention
 * matmuls), RMSNorm, RoPE, scale/mask/softmax, the KV-cache copy and the elementwise glue of the
 * LLaMA graph.
 *
 * Every declaration below replaces one `extern "C"` item of the reference's FFI layer
 * (crates/ggml/sys/src/lib.rs and crates/ggml/sys/src/cuda.rs — bindgen output); the comment on
 * each item names the reference line it stands in for.  Struct layouts are byte-identical to the
 * bindgen layout tests (sizes/offsets are static_assert'ed at the bottom of this file), so the
 * unmodified `crates/ggml` Rust wrapper can link against this library in place of the C sources
 * that crates/ggml/sys/build.rs:12-17 compiles.
 *
 * Plain C: pointers, sizes, POD structs.  No torch / HIP types cross this boundary.
 * Error behaviour follows ggml: no error returns — a failed assertion or HIP error prints a
 * message to stderr and abort()s (reference: SURVEY.md §8b "Errors").
 */
#ifndef GGML_HIP_H
#define GGML_HIP_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GGML_API __attribute__((visibility("default")))

/* ---- constants: crates/ggml/sys/src/lib.rs:16-33 ------------------------------------------- */
#define GGML_FILE_MAGIC 0x67676d6c
#define GGML_FILE_VERSION 1
#define GGML_QNT_VERSION 2
#define GGML_QNT_VERSION_FACTOR 1000
#define GGML_MAX_DIMS 4
#define GGML_MAX_NODES 4096
#define GGML_MAX_PARAMS 256
#define GGML_MAX_CONTEXTS 64
#define GGML_MAX_SRC 6
#define GGML_MAX_NAME 48
#define GGML_MAX_OP_PARAMS 32
#define GGML_DEFAULT_N_THREADS 4
#define GGML_EXIT_SUCCESS 0
#define GGML_EXIT_ABORTED 1
#define GGML_GRAPH_HASHTABLE_SIZE 8273
#define GGML_MEM_ALIGN 16

/* crates/ggml/sys/src/llama.rs:15 (LLAMA_DEFAULT_RMS_EPS) */
#define LLAMA_DEFAULT_RMS_EPS 5e-6f

typedef uint16_t ggml_fp16_t; /* lib.rs:34 */

/* ---- enums: lib.rs:51-160 ------------------------------------------------------------------ */
enum ggml_type {
    GGML_TYPE_F32 = 0,
    GGML_TYPE_F16 = 1,
    GGML_TYPE_Q4_0 = 2,
    GGML_TYPE_Q4_1 = 3,
    /* 4, 5: removed upstream (Q4_2, Q4_3) */
    GGML_TYPE_Q5_0 = 6,
    GGML_TYPE_Q5_1 = 7,
    GGML_TYPE_Q8_0 = 8,
    GGML_TYPE_Q8_1 = 9,
    GGML_TYPE_Q2_K = 10,
    GGML_TYPE_Q3_K = 11,
    GGML_TYPE_Q4_K = 12,
    GGML_TYPE_Q5_K = 13,
    GGML_TYPE_Q6_K = 14,
    GGML_TYPE_Q8_K = 15,
    GGML_TYPE_I8 = 16,
    GGML_TYPE_I16 = 17,
    GGML_TYPE_I32 = 18,
    GGML_TYPE_COUNT = 19,
};

enum ggml_backend { /* lib.rs:70-73 */
    GGML_BACKEND_CPU = 0,
    GGML_BACKEND_GPU = 10,
    GGML_BACKEND_GPU_SPLIT = 20,
};

enum ggml_ftype { /* lib.rs:74-88 */
    GGML_FTYPE_UNKNOWN = -1,
    GGML_FTYPE_ALL_F32 = 0,
    GGML_FTYPE_MOSTLY_F16 = 1,
    GGML_FTYPE_MOSTLY_Q4_0 = 2,
    GGML_FTYPE_MOSTLY_Q4_1 = 3,
    GGML_FTYPE_MOSTLY_Q4_1_SOME_F16 = 4,
    GGML_FTYPE_MOSTLY_Q8_0 = 7,
    GGML_FTYPE_MOSTLY_Q5_0 = 8,
    GGML_FTYPE_MOSTLY_Q5_1 = 9,
};

enum ggml_op { /* lib.rs:89-149 */
    GGML_OP_NONE = 0,
    GGML_OP_DUP,
    GGML_OP_ADD,
    GGML_OP_ADD1,
    GGML_OP_ACC,
    GGML_OP_SUB,
    GGML_OP_MUL,
    GGML_OP_DIV,
    GGML_OP_SQR,
    GGML_OP_SQRT,
    GGML_OP_LOG,
    GGML_OP_SUM,
    GGML_OP_SUM_ROWS,
    GGML_OP_MEAN,
    GGML_OP_ARGMAX,
    GGML_OP_REPEAT,
    GGML_OP_REPEAT_BACK,
    GGML_OP_SILU_BACK,
    GGML_OP_NORM,
    GGML_OP_RMS_NORM,
    GGML_OP_RMS_NORM_BACK,
    GGML_OP_MUL_MAT, /* = 21 */
    GGML_OP_OUT_PROD,
    GGML_OP_SCALE,
    GGML_OP_SET,
    GGML_OP_CPY,
    GGML_OP_CONT,
    GGML_OP_RESHAPE,
    GGML_OP_VIEW,
    GGML_OP_PERMUTE,
    GGML_OP_TRANSPOSE,
    GGML_OP_GET_ROWS,
    GGML_OP_GET_ROWS_BACK,
    GGML_OP_DIAG,
    GGML_OP_DIAG_MASK_INF,
    GGML_OP_DIAG_MASK_ZERO,
    GGML_OP_SOFT_MAX,
    GGML_OP_SOFT_MAX_BACK,
    GGML_OP_ROPE,
    GGML_OP_ROPE_BACK,
    GGML_OP_ALIBI,
    GGML_OP_CLAMP,
    GGML_OP_CONV_1D,
    GGML_OP_CONV_2D,
    GGML_OP_POOL_1D,
    GGML_OP_POOL_2D,
    GGML_OP_FLASH_ATTN,
    GGML_OP_FLASH_FF,
    GGML_OP_FLASH_ATTN_BACK,
    GGML_OP_WIN_PART,
    GGML_OP_WIN_UNPART,
    GGML_OP_UNARY, /* = 51 */
    GGML_OP_MAP_UNARY,
    GGML_OP_MAP_BINARY,
    GGML_OP_MAP_CUSTOM1,
    GGML_OP_MAP_CUSTOM2,
    GGML_OP_MAP_CUSTOM3,
    GGML_OP_CROSS_ENTROPY_LOSS,
    GGML_OP_CROSS_ENTROPY_LOSS_BACK,
    GGML_OP_COUNT, /* = 59 */
};

enum ggml_unary_op { /* lib.rs:150-160 */
    GGML_UNARY_OP_ABS = 0,
    GGML_UNARY_OP_SGN,
    GGML_UNARY_OP_NEG,
    GGML_UNARY_OP_STEP,
    GGML_UNARY_OP_TANH,
    GGML_UNARY_OP_ELU,
    GGML_UNARY_OP_RELU,
    GGML_UNARY_OP_GELU,
    GGML_UNARY_OP_GELU_QUICK,
    GGML_UNARY_OP_SILU,
};

enum ggml_object_type { /* lib.rs:161-164 */
    GGML_OBJECT_TENSOR = 0,
    GGML_OBJECT_GRAPH = 1,
    GGML_OBJECT_WORK_BUFFER = 2,
};

enum ggml_task_type { /* lib.rs:756-759 */
    GGML_TASK_INIT = 0,
    GGML_TASK_COMPUTE = 1,
    GGML_TASK_FINALIZE = 2,
};

/* ---- structs ------------------------------------------------------------------------------- */
struct ggml_context; /* opaque, lib.rs:47-50 */

struct ggml_object { /* lib.rs:167-173, 32 bytes */
    size_t offs;
    size_t size;
    struct ggml_object *next;
    enum ggml_object_type type;
    char padding[4];
};

struct ggml_tensor { /* lib.rs:242-260, 272 bytes */
    enum ggml_type type;
    enum ggml_backend backend;
    int n_dims;
    int64_t ne[GGML_MAX_DIMS]; /* number of elements */
    size_t nb[GGML_MAX_DIMS];  /* stride in bytes: nb[0]=type size, nb[i]=nb[i-1]*ne[i-1] (blocks for q) */
    enum ggml_op op;
    int32_t op_params[GGML_MAX_OP_PARAMS / sizeof(int32_t)];
    bool is_param;
    struct ggml_tensor *grad;
    struct ggml_tensor *src[GGML_MAX_SRC];
    int perf_runs;
    int64_t perf_cycles;
    int64_t perf_time_us;
    void *data;
    char name[GGML_MAX_NAME];
    void *extra; /* backend handle: device allocation record of the HIP backend */
    char padding[4];
};

struct ggml_cplan { /* lib.rs:449-457, 16424 bytes */
    size_t work_size;
    uint8_t *work_data;
    int n_threads;
    int n_tasks[GGML_MAX_NODES];
    bool (*abort_callback)(void *data);
    void *abort_callback_data;
};

struct ggml_cgraph { /* lib.rs:535-545, 164520 bytes */
    int n_nodes;
    int n_leafs;
    struct ggml_tensor *nodes[GGML_MAX_NODES];
    struct ggml_tensor *grads[GGML_MAX_NODES];
    struct ggml_tensor *leafs[GGML_MAX_NODES];
    void *visited_hash_table[GGML_GRAPH_HASHTABLE_SIZE];
    int perf_runs;
    int64_t perf_cycles;
    int64_t perf_time_us;
};

struct ggml_scratch { /* lib.rs:654-658 */
    size_t offs;
    size_t size;
    void *data;
};

struct ggml_init_params { /* lib.rs:706-710 */
    size_t mem_size;
    void *mem_buffer;
    bool no_alloc;
};

struct ggml_compute_params { /* lib.rs:762-768 */
    enum ggml_task_type type;
    int ith, nth;
    size_t wsize;
    void *wdata;
};

typedef void (*ggml_to_float_t)(const void *x, float *y, int k);   /* lib.rs:2884 */
typedef void (*ggml_from_float_t)(const float *x, void *y, int k); /* lib.rs:2887 */
typedef void (*ggml_vec_dot_t)(int n, float *s, const void *x, const void *y); /* lib.rs:2890 */
typedef struct { /* lib.rs:2900-2906, 40 bytes */
    ggml_to_float_t to_float;
    ggml_from_float_t from_float;
    ggml_from_float_t from_float_reference;
    ggml_vec_dot_t vec_dot;
    enum ggml_type vec_dot_type;
} ggml_type_traits_t;

typedef void (*ggml_unary_op_f32_t)(const int, float *, const float *);
typedef void (*ggml_binary_op_f32_t)(const int, float *, const float *, const float *);

/* ---- core: context / arena (lib.rs:36-45, 916-940) ----------------------------------------- */
GGML_API float ggml_fp16_to_fp32(ggml_fp16_t x);
GGML_API ggml_fp16_t ggml_fp32_to_fp16(float x);
GGML_API void ggml_fp16_to_fp32_row(const ggml_fp16_t *x, float *y, int n);
GGML_API void ggml_fp32_to_fp16_row(const float *x, ggml_fp16_t *y, int n);

GGML_API struct ggml_context *ggml_init(struct ggml_init_params params); /* lib.rs:916 */
GGML_API void ggml_free(struct ggml_context *ctx);
GGML_API size_t ggml_used_mem(const struct ggml_context *ctx);
GGML_API size_t ggml_set_scratch(struct ggml_context *ctx, struct ggml_scratch scratch); /* :925 */
GGML_API bool ggml_get_no_alloc(struct ggml_context *ctx);
GGML_API void ggml_set_no_alloc(struct ggml_context *ctx, bool no_alloc);
GGML_API void *ggml_get_mem_buffer(const struct ggml_context *ctx);
GGML_API size_t ggml_get_mem_size(const struct ggml_context *ctx);
GGML_API size_t ggml_get_max_tensor_size(const struct ggml_context *ctx);
GGML_API void ggml_print_objects(const struct ggml_context *ctx);

/* ---- core: type and tensor introspection ---------------------------------------------------- */
GGML_API int64_t ggml_nelements(const struct ggml_tensor *t);
GGML_API int64_t ggml_nrows(const struct ggml_tensor *t);
GGML_API size_t ggml_nbytes(const struct ggml_tensor *t);
GGML_API int ggml_blck_size(enum ggml_type type);
GGML_API size_t ggml_type_size(enum ggml_type type);
GGML_API float ggml_type_sizef(enum ggml_type type);
GGML_API const char *ggml_type_name(enum ggml_type type);
GGML_API const char *ggml_op_name(enum ggml_op op);
GGML_API size_t ggml_element_size(const struct ggml_tensor *t);
GGML_API bool ggml_is_quantized(enum ggml_type type);
GGML_API bool ggml_is_transposed(const struct ggml_tensor *t);
GGML_API bool ggml_is_contiguous(const struct ggml_tensor *t);
GGML_API bool ggml_is_permuted(const struct ggml_tensor *t);
GGML_API size_t ggml_tensor_overhead(void);
GGML_API void *ggml_get_data(const struct ggml_tensor *t);
GGML_API float *ggml_get_data_f32(const struct ggml_tensor *t);
GGML_API const char *ggml_get_name(const struct ggml_tensor *t);
GGML_API struct ggml_tensor *ggml_set_name(struct ggml_tensor *t, const char *name);

/* ---- core: tensor constructors -------------------------------------------------------------- */
GGML_API struct ggml_tensor *ggml_new_tensor(struct ggml_context *ctx, enum ggml_type type, int n_dims,
                                             const int64_t *ne);
GGML_API struct ggml_tensor *ggml_new_tensor_1d(struct ggml_context *ctx, enum ggml_type type, int64_t ne0);
GGML_API struct ggml_tensor *ggml_new_tensor_2d(struct ggml_context *ctx, enum ggml_type type, int64_t ne0,
                                                int64_t ne1);
GGML_API struct ggml_tensor *ggml_new_tensor_3d(struct ggml_context *ctx, enum ggml_type type, int64_t ne0,
                                                int64_t ne1, int64_t ne2);
GGML_API struct ggml_tensor *ggml_new_tensor_4d(struct ggml_context *ctx, enum ggml_type type, int64_t ne0,
                                                int64_t ne1, int64_t ne2, int64_t ne3);
GGML_API struct ggml_tensor *ggml_new_i32(struct ggml_context *ctx, int32_t value);
GGML_API struct ggml_tensor *ggml_new_f32(struct ggml_context *ctx, float value);
GGML_API struct ggml_tensor *ggml_dup_tensor(struct ggml_context *ctx, const struct ggml_tensor *src);
GGML_API struct ggml_tensor *ggml_view_tensor(struct ggml_context *ctx, const struct ggml_tensor *src);

/* ---- core: graph builders (the operator surface of crates/ggml/src/context.rs:276-626) ------- */
GGML_API struct ggml_tensor *ggml_dup(struct ggml_context *ctx, struct ggml_tensor *a);
GGML_API struct ggml_tensor *ggml_add(struct ggml_context *ctx, struct ggml_tensor *a, struct ggml_tensor *b);
GGML_API struct ggml_tensor *ggml_add_inplace(struct ggml_context *ctx, struct ggml_tensor *a,
                                              struct ggml_tensor *b);
GGML_API struct ggml_tensor *ggml_mul(struct ggml_context *ctx, struct ggml_tensor *a, struct ggml_tensor *b);
GGML_API struct ggml_tensor *ggml_repeat(struct ggml_context *ctx, struct ggml_tensor *a, struct ggml_tensor *b);
GGML_API struct ggml_tensor *ggml_silu(struct ggml_context *ctx, struct ggml_tensor *a);
GGML_API struct ggml_tensor *ggml_gelu(struct ggml_context *ctx, struct ggml_tensor *a);
GGML_API struct ggml_tensor *ggml_norm(struct ggml_context *ctx, struct ggml_tensor *a);
GGML_API struct ggml_tensor *ggml_rms_norm(struct ggml_context *ctx, struct ggml_tensor *a, float eps); /* :1265 */
GGML_API struct ggml_tensor *ggml_mul_mat(struct ggml_context *ctx, struct ggml_tensor *a,
                                          struct ggml_tensor *b); /* lib.rs:1283-1288 — THE hot op */
GGML_API struct ggml_tensor *ggml_scale(struct ggml_context *ctx, struct ggml_tensor *a, struct ggml_tensor *b);
GGML_API struct ggml_tensor *ggml_scale_inplace(struct ggml_context *ctx, struct ggml_tensor *a,
                                                struct ggml_tensor *b); /* :1304 */
GGML_API struct ggml_tensor *ggml_cpy(struct ggml_context *ctx, struct ggml_tensor *a, struct ggml_tensor *b);
GGML_API struct ggml_tensor *ggml_cont(struct ggml_context *ctx, struct ggml_tensor *a);
GGML_API struct ggml_tensor *ggml_reshape(struct ggml_context *ctx, struct ggml_tensor *a, struct ggml_tensor *b);
GGML_API struct ggml_tensor *ggml_reshape_1d(struct ggml_context *ctx, struct ggml_tensor *a, int64_t ne0);
GGML_API struct ggml_tensor *ggml_reshape_2d(struct ggml_context *ctx, struct ggml_tensor *a, int64_t ne0,
                                             int64_t ne1);
GGML_API struct ggml_tensor *ggml_reshape_3d(struct ggml_context *ctx, struct ggml_tensor *a, int64_t ne0,
                                             int64_t ne1, int64_t ne2);
GGML_API struct ggml_tensor *ggml_view_1d(struct ggml_context *ctx, struct ggml_tensor *a, int64_t ne0,
                                          size_t offset);
GGML_API struct ggml_tensor *ggml_view_2d(struct ggml_context *ctx, struct ggml_tensor *a, int64_t ne0,
                                          int64_t ne1, size_t nb1, size_t offset);
GGML_API struct ggml_tensor *ggml_view_3d(struct ggml_context *ctx, struct ggml_tensor *a, int64_t ne0,
                                          int64_t ne1, int64_t ne2, size_t nb1, size_t nb2,
                                          size_t offset); /* :1446 */
GGML_API struct ggml_tensor *ggml_permute(struct ggml_context *ctx, struct ggml_tensor *a, int axis0, int axis1,
                                          int axis2, int axis3);
GGML_API struct ggml_tensor *ggml_transpose(struct ggml_context *ctx, struct ggml_tensor *a);
GGML_API struct ggml_tensor *ggml_get_rows(struct ggml_context *ctx, struct ggml_tensor *a,
                                           struct ggml_tensor *b); /* :1485 */
GGML_API struct ggml_tensor *ggml_diag_mask_inf(struct ggml_context *ctx, struct ggml_tensor *a, int n_past);
GGML_API struct ggml_tensor *ggml_diag_mask_inf_inplace(struct ggml_context *ctx, struct ggml_tensor *a,
                                                        int n_past); /* :1510 */
GGML_API struct ggml_tensor *ggml_soft_max(struct ggml_context *ctx, struct ggml_tensor *a);
GGML_API struct ggml_tensor *ggml_soft_max_inplace(struct ggml_context *ctx, struct ggml_tensor *a);
GGML_API struct ggml_tensor *ggml_rope(struct ggml_context *ctx, struct ggml_tensor *a, int n_past, int n_dims,
                                       int mode, int n_ctx); /* :1561 */
GGML_API struct ggml_tensor *ggml_rope_inplace(struct ggml_context *ctx, struct ggml_tensor *a, int n_past,
                                               int n_dims, int mode, int n_ctx);
GGML_API struct ggml_tensor *ggml_rope_custom_inplace(struct ggml_context *ctx, struct ggml_tensor *a,
                                                      int n_past, int n_dims, int mode, int n_ctx,
                                                      float freq_base, float freq_scale); /* :1583 */
/* The rest of the reference surface (crates/ggml/src/context.rs:592-626, 385-427): ggml_alibi and ggml_flash_attn run on
 * the device in the layouts their comments state and abort with a message outside them; the host callbacks
 * (ggml_map_*) always abort. */
GGML_API struct ggml_tensor *ggml_alibi(struct ggml_context *ctx, struct ggml_tensor *a, int n_past, int n_head,
                                        float bias_max);
/* Fused attention as ONE node (context.rs:614 op_flash_attn; runs on the device: kernels/flash_attn.h).
 *   q [D, N, H, B]   k [D, M, Hkv, B]   v [M, D, Hkv, B] (transposed: the view LLaMA's graph builds)   P = M - N >= 0
 *   result: a fresh contiguous F32 tensor with q's n_dims and ne; op GGML_OP_FLASH_ATTN, src[0..2] = q, k, v,
 *   op_params[0] = masked.
 *   out[:, i, h, b] = sum_j p_j v[j, :, h / r, b],  p = soft_max_j(q_i . k_j / sqrtf(D)) over the keys j <= P + i (masked)
 *   or over all M keys (not masked), with soft_max's rounding points: scores and their scaling in f32, the exponential's
 *   argument and value rounded to f16, an exact sum, p = f32(e * f32(1 / sum)); with f16 k/v p is rounded to f16 before
 *   it meets v, with f32 k/v it stays f32; the products are accumulated in f32.
 * Types (q / k, v): F32 / F32 and F16 / F16 as upstream; F32 / F16 as an extension (q is rounded to f16 when loaded, as
 *   mul_mat rounds its src1: the layout every model of this library has).  A second extension: H may be a multiple r of
 *   Hkv (head h reads K/V head h / r); ne[3] must agree on all three.
 * Strides: nb[0] is the element size; nb[1..3] are free (multiples of the element size): permuted views and views into a
 *   larger K/V cache are the normal case.  Cache rows at and beyond M are never read.
 * Limits: D <= 1024 and M <= 37312 keys: a row's scores are held in the CU's 160 KB of LDS (internal.h FLASH_ATTN_*).
 * Anything else — another type mix, v.ne[0] != M, v.ne[1] != D, k.ne[0] != D, M < N, head or batch counts that do not
 *   divide / match, a sparse nb[0], a row beyond the limits — aborts HERE, while the graph is built, with a message that
 *   names ggml_flash_attn and the rule.  ggml_flash_attn_back and ggml_flash_ff are not part of this surface. */
GGML_API struct ggml_tensor *ggml_flash_attn(struct ggml_context *ctx, struct ggml_tensor *q,
                                             struct ggml_tensor *k, struct ggml_tensor *v, bool masked);
GGML_API struct ggml_tensor *ggml_map_unary_f32(struct ggml_context *ctx, struct ggml_tensor *a,
                                                ggml_unary_op_f32_t fun);
GGML_API struct ggml_tensor *ggml_map_binary_f32(struct ggml_context *ctx, struct ggml_tensor *a,
                                                 struct ggml_tensor *b, ggml_binary_op_f32_t fun);

/* ---- core: graph build / plan / compute (lib.rs:1877-1899; caller crates/ggml/src/lib.rs:332-376) */
GGML_API struct ggml_cgraph *ggml_new_graph(struct ggml_context *ctx);
GGML_API size_t ggml_graph_overhead(void);
GGML_API void ggml_build_forward_expand(struct ggml_cgraph *cgraph, struct ggml_tensor *tensor);
GGML_API struct ggml_cgraph ggml_build_forward(struct ggml_tensor *tensor);
GGML_API struct ggml_cplan ggml_graph_plan(struct ggml_cgraph *cgraph, int n_threads); /* by value (sret) */
/* Executes every node of the graph on the MI355X.  There is no CPU compute path in this library:
 * an op outside the supported set aborts with a message.  Returns GGML_EXIT_SUCCESS. */
GGML_API int ggml_graph_compute(struct ggml_cgraph *cgraph, struct ggml_cplan *cplan);
GGML_API void ggml_graph_reset(struct ggml_cgraph *cgraph);

/* ---- core: offline quantizer (lib.rs:2779-2822; caller crates/ggml/src/lib.rs:419-483) ------- */
GGML_API size_t ggml_quantize_q4_0(const float *src, void *dst, int n, int k, int64_t *hist);
GGML_API size_t ggml_quantize_q4_1(const float *src, void *dst, int n, int k, int64_t *hist);
GGML_API size_t ggml_quantize_q5_0(const float *src, void *dst, int n, int k, int64_t *hist);
GGML_API size_t ggml_quantize_q5_1(const float *src, void *dst, int n, int k, int64_t *hist);
GGML_API size_t ggml_quantize_q8_0(const float *src, void *dst, int n, int k, int64_t *hist);
/* The K types (bindgen: crates/ggml/sys/src/lib.rs:3472-3515): n values in rows of k, k % 256 == 0; returns the bytes
 * written.  The encoders follow this project's own fit (oracle/SEMANTICS.md: min/max per sub-block for Q2_K / Q4_K /
 * Q5_K, abs-max for Q3_K / Q6_K), not upstream's iterative scale search, whose source the reference tree does not
 * carry: blocks are valid and decode everywhere, parity with upstream's bytes is unpinned.  `hist` is left untouched. */
GGML_API size_t ggml_quantize_q2_K(const float *src, void *dst, int n, int k, int64_t *hist);
GGML_API size_t ggml_quantize_q3_K(const float *src, void *dst, int n, int k, int64_t *hist);
GGML_API size_t ggml_quantize_q4_K(const float *src, void *dst, int n, int k, int64_t *hist);
GGML_API size_t ggml_quantize_q5_K(const float *src, void *dst, int n, int k, int64_t *hist);
GGML_API size_t ggml_quantize_q6_K(const float *src, void *dst, int n, int k, int64_t *hist);
/* start % 32 == 0 (K types: start % 256 == 0) */
GGML_API size_t ggml_quantize_chunk(enum ggml_type type, const float *src, void *dst, int start, int n,
                                    int64_t *hist);
GGML_API ggml_type_traits_t ggml_internal_get_type_traits(enum ggml_type i); /* lib.rs:2973 */

GGML_API int ggml_cpu_has_blas(void);
GGML_API int ggml_cpu_has_gpublas(void);

/* ---- accelerator hooks: one per entry of crates/ggml/sys/src/cuda.rs:6-77 -------------------- */
#define GGML_HIP_MAX_DEVICES 16 /* cuda.rs:6 GGML_CUDA_MAX_DEVICES */

GGML_API void ggml_init_hipblas(void);                                 /* cuda.rs:8  ggml_init_cublas */
GGML_API void ggml_hip_set_tensor_split(const float *tensor_split);    /* cuda.rs:11 */
GGML_API void ggml_hip_mul(const struct ggml_tensor *src0, const struct ggml_tensor *src1,
                           struct ggml_tensor *dst);                   /* cuda.rs:14 */
GGML_API bool ggml_hip_can_mul_mat(const struct ggml_tensor *src0, const struct ggml_tensor *src1,
                                   struct ggml_tensor *dst);           /* cuda.rs:17-22 */
GGML_API size_t ggml_hip_mul_mat_get_wsize(const struct ggml_tensor *src0, const struct ggml_tensor *src1,
                                           struct ggml_tensor *dst);   /* cuda.rs:24-29 */
GGML_API void ggml_hip_mul_mat(const struct ggml_tensor *src0, const struct ggml_tensor *src1,
                               struct ggml_tensor *dst, void *wdata, size_t wsize); /* cuda.rs:31-38 */
GGML_API void *ggml_hip_host_malloc(size_t size);                      /* cuda.rs:41 */
GGML_API void ggml_hip_host_free(void *ptr);                           /* cuda.rs:44 */
GGML_API void ggml_hip_transform_tensor(void *data, struct ggml_tensor *tensor); /* cuda.rs:47 — H2D boundary */
GGML_API void ggml_hip_free_data(struct ggml_tensor *tensor);          /* cuda.rs:50 */
GGML_API void ggml_hip_assign_buffers(struct ggml_tensor *tensor);     /* cuda.rs:53 */
GGML_API void ggml_hip_assign_buffers_no_scratch(struct ggml_tensor *tensor);    /* cuda.rs:56 */
GGML_API void ggml_hip_assign_buffers_force_inplace(struct ggml_tensor *tensor); /* cuda.rs:59 */
GGML_API void ggml_hip_set_main_device(int main_device);               /* cuda.rs:62 */
GGML_API void ggml_hip_set_mul_mat_q(bool mul_mat_q);                  /* cuda.rs:65 */
GGML_API void ggml_hip_set_scratch_size(size_t scratch_size);          /* cuda.rs:68 */
GGML_API void ggml_hip_free_scratch(void);                             /* cuda.rs:71 */
GGML_API bool ggml_hip_compute_forward(struct ggml_compute_params *params, struct ggml_tensor *tensor); /* :73-76 */

/* The same 19 entry points under the names the reference's `cublas` cfg arms already bind
 * (crates/ggml/src/tensor.rs:68-71,89-92,106-109,214-217; accelerator/mod.rs:68-94), so the Rust
 * crate links against this library with zero source changes. */
GGML_API void ggml_init_cublas(void);
GGML_API void ggml_cuda_set_tensor_split(const float *tensor_split);
GGML_API void ggml_cuda_mul(const struct ggml_tensor *, const struct ggml_tensor *, struct ggml_tensor *);
GGML_API bool ggml_cuda_can_mul_mat(const struct ggml_tensor *, const struct ggml_tensor *, struct ggml_tensor *);
GGML_API size_t ggml_cuda_mul_mat_get_wsize(const struct ggml_tensor *, const struct ggml_tensor *,
                                            struct ggml_tensor *);
GGML_API void ggml_cuda_mul_mat(const struct ggml_tensor *, const struct ggml_tensor *, struct ggml_tensor *,
                                void *, size_t);
GGML_API void *ggml_cuda_host_malloc(size_t size);
GGML_API void ggml_cuda_host_free(void *ptr);
GGML_API void ggml_cuda_transform_tensor(void *data, struct ggml_tensor *tensor);
GGML_API void ggml_cuda_free_data(struct ggml_tensor *tensor);
GGML_API void ggml_cuda_assign_buffers(struct ggml_tensor *tensor);
GGML_API void ggml_cuda_assign_buffers_no_scratch(struct ggml_tensor *tensor);
GGML_API void ggml_cuda_assign_buffers_force_inplace(struct ggml_tensor *tensor);
GGML_API void ggml_cuda_set_main_device(int main_device);
GGML_API void ggml_cuda_set_mul_mat_q(bool mul_mat_q);
GGML_API void ggml_cuda_set_scratch_size(size_t scratch_size);
GGML_API void ggml_cuda_free_scratch(void);
GGML_API bool ggml_cuda_compute_forward(struct ggml_compute_params *params, struct ggml_tensor *tensor);

/* ---- HIP-backend extensions (no reference counterpart; measurement and multi-GPU plumbing) ---- */
/* Number of visible devices (0 when no GPU / HIP runtime unusable). Never aborts. */
GGML_API int ggml_hip_device_count(void);
/* The physical GPU a device slot drives (slot s -> (GGML_HIP_DEVICE + s) mod visible GPUs), -1 for a slot that does not exist. */
GGML_API int ggml_hip_slot_physical_device(int slot);
/* GGML_HIP_SESSION_SLOTS=n (opt-in): the first K/V memory a thread creates (ggml_hip_assign_buffers_no_scratch, i.e.
 * InferenceSession::new) assigns the thread one of the n sibling slots of the GPU and pins it there, so that sessions started on
 * several threads by an UNCHANGED caller (model.start_session() / infer()) overlap instead of sharing one slot's stream and lock.
 * Returns the calling thread's assignment, -1 before it has one. */
GGML_API int ggml_hip_thread_session_slot(void);
/* Several devices in one process (the ggml-style layer split of one InferenceSession).  A device
 * "slot" owns a stream, the device shadows of the host arenas, the weights uploaded while it was current and its plan cache;
 * ggml_hip_set_main_device (cuda.rs:62) makes a slot current for every following call.  GGML_HIP_VIRTUAL_DEVICES=n maps n
 * slots onto the visible GPUs round-robin (several slots on one GPU: how the split is tested on a 1-GPU box).
 * Threads: the current slot is per thread.  ggml_hip_set_main_device sets the process default (followed by every thread
 * that never chose a slot — the reference sets it once at load, accelerator/mod.rs:72) and pins the calling thread;
 * ggml_hip_bind_thread_device pins the calling thread only.  Entry points lock the slot they act on, not the library:
 * sessions on different slots run concurrently (crates/llm-base/src/inference_session.rs:43-48: sessions are Send and
 * one model serves several of them), calls on one slot are serialised.  ggml_hip_get_main_device = the caller's slot. */
GGML_API int ggml_hip_get_main_device(void);
GGML_API void ggml_hip_bind_thread_device(int device);
/* -1 while the calling thread follows the process default, else the slot it is pinned to; unbind drops the pin again (the
 * session mirror pins a model's slot around each call and must leave a thread that followed the default following it). */
GGML_API int ggml_hip_thread_pinned_device(void);
GGML_API void ggml_hip_unbind_thread_device(void);
/* ggml_hip_set_tensor_split / ggml_cuda_set_tensor_split read exactly ONE float: the reference passes the address of a
 * single stack f32 (crates/ggml/src/accelerator/mod.rs:74-75).  get returns that value (out[0]; 1 written). */
GGML_API int ggml_hip_get_tensor_split(float *out, int cap);
/* A split of ONE model over several device slots of this process, by LAYERS (ggml's fractions convention: slot i takes
 * fractions[i] / sum; all zero = equal shares; rows of one tensor are never split).  Explicit length, so nothing is read
 * past the caller's array.  NULL or n <= 0 clears it.  llm_llama_new applies it (also: env GGML_HIP_LAYER_SPLIT=G for G
 * equal shares).  get returns the number of fractions written. */
GGML_API void ggml_hip_set_layer_split(const float *fractions, int n);
GGML_API int ggml_hip_get_layer_split(float *out, int cap);
/* dst (on slot dst_device) = src (on slot src_device), ordered after src_device's enqueued work and before dst_device's
 * later work: the residual hop of a layer split inside one process (peer copy over xGMI between two GPUs). */
GGML_API void ggml_hip_copy_between_devices(int dst_device, void *dst, int src_device, const void *src, size_t nbytes);
/* Blocks until all device work queued by this library has finished. */
GGML_API void ggml_hip_synchronize(void);
/* Copies nbytes of a tensor's device mirror to/from host memory (host pointer != tensor->data allowed).
 * Used by tests to inspect interior nodes and by the layer-split driver to hand the residual to RCCL. */
GGML_API void ggml_hip_tensor_get(const struct ggml_tensor *tensor, void *host_dst, size_t offset, size_t nbytes);
GGML_API void ggml_hip_tensor_set(struct ggml_tensor *tensor, const void *host_src, size_t offset, size_t nbytes);
/* Raw synchronous copy on the backend stream; kind: 0 = host->device, 1 = device->host, 2 = device->device. */
GGML_API void ggml_hip_memcpy(void *dst, const void *src, size_t nbytes, int kind);
/* Device address of a tensor's mirror (for handing buffers to torch.distributed / RCCL). */
GGML_API void *ggml_hip_tensor_device_ptr(const struct ggml_tensor *tensor);
/* Per-kernel-class timing with HIP events on the backend's own stream (bench.py roofline leg).
 * classes: see GGML_HIP_KCLASS_*.  begin() resets and enables; end() disables; query returns
 * accumulated milliseconds and launch count for one class. */
enum ggml_hip_kclass {
    GGML_HIP_KCLASS_MMVQ = 0,    /* quantized mat-vec (decode hot kernel) */
    GGML_HIP_KCLASS_MMQ_MFMA,    /* quantized GEMM on MFMA (prefill) */
    GGML_HIP_KCLASS_ATTN,        /* f16 KV matmuls / fused attention */
    GGML_HIP_KCLASS_OTHER,       /* norm, rope, softmax, cpy, elementwise, quantize-activation */
    GGML_HIP_KCLASS_COUNT
};
GGML_API void ggml_hip_timing_begin(void);
GGML_API void ggml_hip_timing_end(void);
GGML_API void ggml_hip_timing_query(int kclass, double *ms, int64_t *launches, double *algo_bytes);
/* Runtime options, process-wide.  The keys, their meanings and their environment variables: INTEGRATION.md section 4 "Runtime
 * knobs"; the table they come from: g_options in llm_amd/csrc/backend_state.inc.  An unknown key aborts with a message.
 * get_option answers what the calling thread's slot holds (before that slot exists: the value that was set, else the default);
 * -1 for a key that is an action. */
GGML_API void ggml_hip_set_option(const char *key, int value);
GGML_API int ggml_hip_get_option(const char *key);
/* Replays the launches of one kernel class of the most recent fused decode plan `replays` times from a
 * dedicated hipGraph between two HIP events on the backend stream (bench.py roofline leg). 0 on success.
 * kclass may also be GGML_HIP_KKIND_BASE + {0 wq|wk|wv, 1 wo, 2 w1|w3, 3 w2, 4 lm_head}: that mat-vec alone; or
 * GGML_HIP_KKIND_BASE + 8 + the same: every mat-vec launch BUT that kind (all - all_but_k = what kind k costs in sequence). */
#define GGML_HIP_KKIND_BASE 16
GGML_API int ggml_hip_bench_plan_class(int kclass, int replays, double *ms_total, int64_t *launches_per_replay,
                                       double *algo_bytes_per_replay);
/* Layer split over RCCL (the reference has no multi-GPU path: LLAMA_MAX_DEVICES = 1,
 * crates/ggml/sys/src/llama.rs:3, and feeds ggml_cuda_set_tensor_split a single float, crates/ggml/src/accelerator/mod.rs:74-75).
 * One process per GPU; rank 0 draws the id, the launcher hands it to every rank, every rank calls init.  send / recv are
 * enqueued on the backend's stream (ordered with the kernels before and after them, no host synchronisation);
 * sendrecv = both in one RCCL group (needed when the peer is this rank itself).  librccl.so is opened on first use. */
#define GGML_HIP_COMM_ID_BYTES 128
GGML_API int ggml_hip_comm_unique_id(void *id_out /* GGML_HIP_COMM_ID_BYTES */);
GGML_API int ggml_hip_comm_init(int rank, int world, const void *id); /* returns the rank count RCCL reports; -1 (with a
                                                                          message) if the communicator cannot be formed */
GGML_API void ggml_hip_comm_destroy(void);
GGML_API int ggml_hip_comm_ranks(void); /* 0 = no communicator */
GGML_API void ggml_hip_comm_send(const void *dev_src, size_t nbytes, int peer);
GGML_API void ggml_hip_comm_recv(void *dev_dst, size_t nbytes, int peer);
GGML_API void ggml_hip_comm_sendrecv(const void *dev_src, int send_peer, void *dev_dst, int recv_peer, size_t nbytes);
/* Launch-floor probe (measurement only, tests/tools/launch_probe.py): a linear hipGraph of n_launch launches of a
 * kernel that only stamps the device wall clock, with the given launch shape.  out[3] = {us per launch, us from one
 * launch's end to the next launch's first instruction, us first instruction -> last kernel argument usable}. */
GGML_API int ggml_hip_bench_empty(int wgs, int threads, int lds_bytes, int kernarg_bytes, int n_launch, int replays,
                                  double *out);
/* Counters for tests: "plan_tokens" (tokens run by the fused decode plan), "attn_split_tokens", "graph_replays", "plans",
 * "generic_graphs".  -1 for an unknown key. */
GGML_API int64_t ggml_hip_get_stat(const char *key);
/* ggml_graph_compute split in two so that a caller can overlap host work (building the next token's graph) with
 * the device: begin() enqueues the graph and returns 1 if it is still running on the device (fused decode plan),
 * 0 if it already completed (any other graph runs synchronously); end() waits and completes the copy of the
 * host-visible results (CPU-backend nodes).  No result may be read, and no other graph computed, in between. */
GGML_API int ggml_hip_graph_compute_begin(struct ggml_cgraph *cgraph);
GGML_API void ggml_hip_graph_compute_end(void);
/* Optional companion of the pair above: a caller that builds the NEXT token's graph between begin() and end() may hand it over
 * right away; the structural match of that graph against the fused decode plan (~20 us of host work per token) then happens
 * while the device runs instead of between two tokens' device work.  Returns 1 if the graph was recognised and remembered (its
 * begin() then skips the match), 0 otherwise (nothing changes).  The remembered match is dropped by anything that could
 * invalidate it (ggml_init / ggml_free / ggml_set_scratch on any thread, an option change, freed weights).  The token id itself
 * is read at begin(), as always. */
GGML_API int ggml_hip_graph_prepare(struct ggml_cgraph *cgraph);
/* A caller that is greedy by construction says so before it computes a token's graph: "the evaluation after the one I compute next
 * will be of the first maximum of its logits".  It holds for that one graph of the calling thread's device slot.  A single-token
 * whole-model plan run then ends in k_token_tail (argmax, next parameters and the results' way to pinned host memory in one
 * kernel) and the next token's graph is launched right behind it; if the caller's next evaluation is that token, its results are
 * already on their way (stats "spec_hits", "tail_tokens").  What is computed never changes: any other next call simply runs
 * behind the ahead run.  Option speculate_next = 1 makes the same promise for every evaluation of an unchanged caller. */
GGML_API void ggml_hip_expect_greedy_next(void);
/* Greedy sampling on the device (the step after the path): decodes n more tokens — each the first
 * argmax of the previous logits, what `infer_next_token` with a greedy sampler yields (inference_session.rs:381-424,
 * samplers.rs:289-306) — without the per-token logits read-back and host sync.  `last` = the cgraph of the caller's
 * most recent ggml_graph_compute, which must have been a single-token LLaMA evaluation executed by the fused plan.
 * out_tokens[n] receives the ids; last_logits (V floats, may be NULL) the logits after the n-th token.  The K/V
 * memory advances by n positions; the caller adds n to its n_past.  Returns 0, or -1 if the precondition does not
 * hold (nothing was executed: decode token by token instead). */
GGML_API int ggml_hip_decode_greedy_chain(struct ggml_cgraph *last, int n, int32_t *out_tokens, float *last_logits);
/* One decode step of B single-token LLaMA graphs of ONE model on this slot, each the reference's unchanged graph for its own
 * session (own memory_k / memory_v, own n_past, own token), as one pass over the weights.  Same results as ggml_graph_compute
 * on each graph in turn (host-visible nodes filled: logits, embeddings).  Returns 0, or -1 with nothing executed.
 * -1 unless: 2 <= B <= 8; every graph is a whole-model single-token graph of a block-format or F16 model, or of a K-quant model
 * (Q2_K ... Q6_K, uniform or mixed) with options plan_batch_k (default 0) and plan_k on; all share the
 * weights, dimensions, context size and RoPE parameters; f16 K/V, all distinct; every n_past below the context size, which fits
 * the attention kernel's LDS; options plan and plan_batch on.  NULL or a B out of range is refused before any device is touched. */
GGML_API int ggml_hip_decode_batch(struct ggml_cgraph *const *graphs, int n_graphs);
/* n_steps greedy decode steps of those B sessions without a host round trip between them.  Step 0 is ggml_hip_decode_batch on the
 * graphs (they carry every session's first token); each further step evaluates, for every session, the first maximum of the
 * logits its previous step left — sampled on the device, which also moves the session's position on — as a replay of the same
 * step.  out_ids[(i - 1) * B + c] = the token session c evaluated in step i (i = 1 .. n_steps - 1); after the last step every
 * graph's logits and embedding nodes hold that step's results, as after ggml_hip_decode_batch.  Bit for bit what n_steps calls
 * of ggml_hip_decode_batch by a caller that takes the first maximum compute: logits, K/V memory.  Every K/V memory advances by
 * n_steps positions; the caller adds n_steps to each n_past.  Returns 0, or -1 with nothing executed: whatever
 * ggml_hip_decode_batch declines, n_steps < 1 or > 4096, a session with n_past + n_steps beyond the context, option
 * plan_batch_chain off.  n_steps == 1 is ggml_hip_decode_batch (out_ids may be NULL).  NULL, a B out of range or such an n_steps is
 * refused before any device is touched. */
GGML_API int ggml_hip_decode_batch_greedy(struct ggml_cgraph *const *graphs, int n_graphs, int n_steps, int32_t *out_ids);
/* The same chain with the shape of the reference's default sampler (crates/llm-base/src/samplers.rs:97-188) on the device instead
 * of the first maximum: repetition penalty `penalty` over a session's last 64 tokens, top-k `k`, top-p `top_p`, temperature
 * `temperature`, one xorshift64* draw — in the arithmetic of llm_amd/csrc/kernels/sampler_math.h (IEEE basic operations only, no
 * library exponential), which llm_sample_exact restates on the host: a caller that samples each step with that function from the
 * logits ggml_hip_decode_batch leaves draws the same ids, and the logits and K/V memory agree bit for bit.
 * windows [B][64]: session c's last window_n[c] (0 .. 64) tokens, oldest first, INCLUDING the token its graph evaluates; the device
 * keeps the window moving over the ids it samples.  rng [B]: the sessions' generator states, advanced by n_steps - 1 draws each on
 * return.  out_ids as above.  Returns 0, or -1 with nothing executed and no generator moved: whatever
 * ggml_hip_decode_batch_greedy declines, k < 1, k > 256 or k > n_vocab, temperature <= 0, top_p <= 0, penalty <= 0, a window
 * entry outside the vocabulary, option plan_batch_sample off.  Counted in batch_sample_steps / batch_sample_tokens (not in
 * batch_chain_*). */
typedef struct {
    int32_t k;
    float top_p, temperature, penalty;
} ggml_hip_sampler;
GGML_API int ggml_hip_decode_batch_sampled(struct ggml_cgraph *const *graphs, int n_graphs, int n_steps, const ggml_hip_sampler *params,
                                           const int32_t *windows, const int32_t *window_n, uint64_t *rng, int32_t *out_ids);
/* ggml_hip_decode_greedy_chain for ONE session that samples: n more tokens, each drawn on the device by that sampler (k_sample_next,
 * the arithmetic of sampler_math.h) from the logits the previous token left, between two replays of the single-token plan — no
 * logits read-back and no host round trip per token.  `last` as for the greedy chain: the cgraph of the most recent
 * ggml_graph_compute, a single-token whole-model LLaMA evaluation that ran as a fused plan (block-format, K-quant or F16 weights).
 * window: the session's last window_n (0 .. 64) tokens, oldest first, INCLUDING the token `last` evaluated; *rng: its generator
 * state, advanced by n draws on return.  out_tokens[n] receives the ids, last_logits (V floats, may be NULL) the logits after the
 * n-th.  The K/V memory advances by n positions; the caller adds n to its n_past.  Ids, logits and K/V memory are bit for bit what a
 * caller gets that draws each token with llm_sample_exact and evaluates it.  Returns 0, or -1 with nothing executed and *rng
 * unmoved: whatever ggml_hip_decode_greedy_chain declines (n_past + 1 + n beyond the context among it), k < 1, k > 256 or
 * k > n_vocab, temperature <= 0, top_p <= 0, penalty <= 0, window_n outside 0 .. 64, a window entry outside the vocabulary, option
 * plan_sample_chain off.  Option chain_k does not apply.  Counters: sample_chain_steps and sample_chain_tokens (n each), and what
 * the greedy chain moves — plan_tokens, fused_tokens, fused_heads_tokens, graph_replays; nothing of batch_* and none of the token
 * tail's (tail_tokens, spec_*). */
GGML_API int ggml_hip_decode_sampled_chain(struct ggml_cgraph *last, int n, const ggml_hip_sampler *params, const int32_t *window,
                                           int window_n, uint64_t *rng, int32_t *out_tokens, float *last_logits);
/* The whole sampler: the four parameters above and the reference's other samplers (crates/llm-base/src/samplers.rs:97-188 and the
 * flat bias of build_sampler, :308-345) — token bias, frequency / presence penalty over the same 64-token window, tail-free, locally
 * typical, min-p, Mirostat 2 — as specified at the head of llm_amd/csrc/kernels/sampler_math.h, which k_sample_next and the host's
 * llm_sample_chain both compile.  Neutral values: freq 0, presence 0, tail_free_z 1, typical_p 1, min_p 0, n_bias 0, mirostat 0, and ANY tau > 0 and eta >= 0,
 * such as 5 and 0.1: they are checked whatever mirostat is, so a zeroed struct with only the listed values set is declined —
 * with them every _ex entry below computes what its four-parameter sibling computes, bit for bit (the siblings forward to them).
 * mirostat is 0 or 2; with 2 the truncating samplers must be neutral (top_p >= 1 too; k is not read) and tau > 0, eta >= 0.
 * bias_id / bias: n_bias (0 .. 64) pairs, every id once; -inf bans a token.  Not representable: Mirostat 1, top-a, sequence
 * repetition, a window other than 64. */
typedef struct {
    ggml_hip_sampler base;
    float freq, presence, tail_free_z, typical_p, min_p;
    int32_t mirostat;
    float tau, eta;
    int32_t n_bias;
    int32_t bias_id[64];
    float bias[64];
} ggml_hip_sampler_chain;
/* ggml_hip_decode_sampled_chain / ggml_hip_decode_batch_sampled with that sampler.  mu: the sessions' Mirostat states (one / B floats,
 * in / out beside rng; a caller starts them at 2 * tau; may be NULL when mirostat == 0).  -1 with nothing executed and no state moved
 * for whatever the siblings decline and for: NaN in a parameter, tail_free_z <= 0, typical_p <= 0, min_p outside [0, 1], n_bias
 * outside 0 .. 64, a bias id outside the vocabulary or listed twice, a NaN or +inf bias, mirostat not 0 or 2, Mirostat 2 beside a
 * truncating sampler, tau <= 0, eta < 0, a NaN mu, Mirostat 2 on more than 32768 vocabulary entries.  Same options, same counters. */
GGML_API int ggml_hip_decode_sampled_chain_ex(struct ggml_cgraph *last, int n, const ggml_hip_sampler_chain *chain, const int32_t *window,
                                              int window_n, uint64_t *rng, float *mu, int32_t *out_tokens, float *last_logits);
GGML_API int ggml_hip_decode_batch_sampled_ex(struct ggml_cgraph *const *graphs, int n_graphs, int n_steps, const ggml_hip_sampler_chain *chain,
                                              const int32_t *windows, const int32_t *window_n, uint64_t *rng, float *mu, int32_t *out_ids);
/* Chains that stop: every column carries its own request — its own sampler (a NULL chain: the first maximum), up to 8 stop ids and
 * its own budget — and ends on its own: with the draw of one of its stop ids, which the next step still evaluates as the reference's
 * loop does (inference_session.rs:404-408: evaluate, then EndOfText), or when its budget is used up.  A column that has ended is
 * frozen while the others go on: the kernel between two steps leaves its token, position, ring, generator and mu alone, so every
 * further step evaluates the same token at the same position again and rewrites the same K/V rows and logits with the same bits.
 * The call ends as soon as no column is live: the steps are enqueued in groups of option chain_group, the columns' live flags come
 * back behind each group, and nothing more is launched once every column was found ended.  Each session is left exactly where its
 * own last evaluation left it: logits, K/V, generator, mu.
 * ended_by: 1 = the budget, 2 = a stop id.  Rows of the ids that belong to steps a column sat out frozen, or that were never
 * launched, hold -1. */
typedef struct {
    int32_t budget, n_stop, stop_id[8];
} ggml_hip_chain_end;
#define GGML_HIP_CHAIN_END_BUDGET 1
#define GGML_HIP_CHAIN_END_STOP 2
/* One session, as ggml_hip_decode_sampled_chain_ex (chain != NULL) or ggml_hip_decode_greedy_chain (chain == NULL; window, rng and mu
 * may then be NULL): at most end->budget (1 .. n) draws.  out_tokens[n]: the ids drawn, then -1; *n_drawn their number (every one
 * of them was evaluated: the caller adds it to its n_past); last_logits (V floats, may be NULL): the logits after the last of them.
 * Returns 0, or -1 with nothing executed and no state moved: whatever the sibling declines, with n_past + 1 + end->budget against the
 * context; n_stop outside 0 .. 8; a stop id outside the vocabulary; a budget outside 1 .. n.  Option chain_k does not apply.
 * Counters as the sibling's, for the steps that were launched; chain_stopped_columns, chain_frozen_steps, chain_steps_cut. */
GGML_API int ggml_hip_decode_chain_requests(struct ggml_cgraph *last, int n, const ggml_hip_sampler_chain *chain, const ggml_hip_chain_end *end,
                                            const int32_t *window, int window_n, uint64_t *rng, float *mu, int32_t *out_tokens,
                                            int32_t *n_drawn, int32_t *ended_by, float *last_logits);
/* B = 2 .. 8 sessions, as ggml_hip_decode_batch_sampled_ex / ggml_hip_decode_batch_greedy: chains [B] (entries may be NULL: that
 * column takes the first maximum), ends [B].  A column's budget is the number of evaluations it takes, counting step 0: 1 .. n_steps;
 * 1 = frozen from the first draw on (a session whose host-drawn first token was already its stop id).  n_evaluated [B]: the
 * evaluations each column took (the caller adds them to the session's n_past).  windows, window_n, rng may be NULL when every column
 * is greedy; mu when none runs Mirostat 2.  -1 with nothing executed and no state moved: whatever the siblings decline, checked per
 * column, with n_past + budget against the context; n_stop outside 0 .. 8; a stop id outside the vocabulary; a budget outside
 * 1 .. n_steps.  NULL pointers and counts out of range are refused before any device is touched. */
GGML_API int ggml_hip_decode_batch_requests(struct ggml_cgraph *const *graphs, int n_graphs, int n_steps,
                                            const ggml_hip_sampler_chain *const *chains, const ggml_hip_chain_end *ends, const int32_t *windows,
                                            const int32_t *window_n, uint64_t *rng, float *mu, int32_t *out_ids, int32_t *n_evaluated,
                                            int32_t *ended_by);
/* A POOL of n_pool = n_cols .. 64 requests over n_cols = 2 .. 8 columns: ggml_hip_decode_batch_requests where a column whose request
 * has ended is not frozen for the rest of the call but takes the next waiting request, on the device, between two replays of the
 * same captured graph.  graphs, chains, ends, windows, window_n, rng, mu: [n_pool], as the sibling's per column; graphs[r] is request
 * r's staged single-token graph (its first token, its session's caches and position).  Entries 0 .. n_cols - 1 start in columns
 * 0 .. n_cols - 1, the rest wait in order.  The admission rule (kernels/pool_rule.h): after step s and its tail a column is free when
 * its request is not live and was already not live before step s ran (its last drawn token, a stop id included, has been evaluated);
 * a request born ended (a budget of one evaluation) is free after its first step; free columns in ascending index take the waiting
 * requests in ascending pool index, and the admitted request's first token is evaluated at step s + 1.
 * Out: col [n_pool], first_step [n_pool]: request r ran in column col[r] from step first_step[r] (-1, 0: it never left the queue and
 * is untouched); n_evaluated [n_pool], ended_by [n_pool] (0: n_steps ran out with the request still live; its states are where its
 * last evaluation left them); out_ids [n_steps - 1][n_cols]: request r's k-th id (k = 1 .. n_evaluated - 1) is
 * out_ids[(first_step + k - 1) * n_cols + col]; *steps_run: the largest first_step + n_evaluated.  Every request that ran finds its
 * logits and embedding row at its graph's result nodes.  A budget is 1 .. n_steps and is checked, with the request's own position,
 * against the context.  -1 with nothing executed and no state moved: whatever the sibling declines for any request of the pool
 * (all checked up front), a session twice in the pool, option plan_batch_pool = 0.  NULL pointers and counts out of range are
 * refused before any device is touched.  Counters: the sibling's, and pool_calls, pool_admitted, pool_steps. */
#define GGML_HIP_POOL_MAX 64
GGML_API int ggml_hip_decode_pool_requests(struct ggml_cgraph *const *graphs, int n_pool, int n_cols, int n_steps,
                                           const ggml_hip_sampler_chain *const *chains, const ggml_hip_chain_end *ends, const int32_t *windows,
                                           const int32_t *window_n, uint64_t *rng, float *mu, int32_t *out_ids, int32_t *col,
                                           int32_t *first_step, int32_t *n_evaluated, int32_t *ended_by, int32_t *steps_run);
/* The PROMPTS of 1 .. 64 sessions of one model as one packed prompt batch: graphs[i] is the reference's unchanged N_i-token
 * Llama::evaluate graph of its own session (own memory_k / memory_v, own n_past, N_i >= 1), built and not computed.  The R = sum N_i
 * rows run as ONE pass of the prompt plan (f16-MFMA GEMMs over all R rows, the K split chosen at R rows); segment i is rows
 * [row0_i, row0_i + N_i) in graph order, and the three launches that place a row in a sequence — RoPE table, K/V store, fused
 * attention — read every row's position and cache from tables of the call (kernels/prompt_pack.h).  Results go where an evaluation of
 * graph i alone leaves them: its logits and embedding rows at its result nodes, K/V rows n_past_i .. n_past_i + N_i - 1 of its caches.
 * 0, or -1 with nothing executed and nothing written: option plan, plan_prompt or plan_prompt_pack (default 1, GGML_HIP_PLAN_PROMPT_PACK)
 * = 0, a graph that is not a whole-model LLaMA graph, a K-quant or F16 model (block formats Q4_0 .. Q8_0 only), K/V not f16, graphs of
 * different models, the same cache twice, a cache of another device slot, option attn_fused = 0 or a segment whose n_past_i + N_i does
 * not take the 32-query form of the fused attention, n_past_i + N_i beyond the context, R > 4096, rows of more than 8192 elements, a
 * token id outside the vocabulary.  NULL pointers and n_graphs outside 1 .. 64 are refused before any device is touched.  Counters:
 * prompt_pack_calls, prompt_pack_segments, prompt_pack_tokens; the rows count in prompt_plan_tokens too. */
#define GGML_HIP_PACK_MAX 64
GGML_API int ggml_hip_prompt_pack(struct ggml_cgraph *const *graphs, int n_graphs);
/* Top-k prefilter of a logits row on the device: the k (<= 1024, <= ne0) largest entries of row `row` of
 * the f32 tensor `t` — a node of the caller's most recent ggml_graph_compute, normally the logits — as (value, id) pairs,
 * value descending, lower id first among equal values, followed by the entries of `extra_ids` (n_extra ids, e.g. the
 * tokens a repetition penalty or a bias list touches) in the order given.  out_vals / out_ids hold k + n_extra entries.
 * For the reference's sampler chain (crates/llm-base/src/samplers.rs:289-306 sample_token; top-k after flat bias and
 * repetition penalty): the tokens that can be among the k best after the host has changed the n_extra listed logits
 * are all in {raw top-(k + n_extra)} U extra_ids, so a caller asks for k + n_extra and sorts at most k + 2 n_extra
 * pairs instead of n_vocab logits; only those pairs cross PCIe.  Returns 0, -1 on bad arguments. */
GGML_API int ggml_hip_topk(const struct ggml_tensor *t, int64_t row, int k, const int32_t *extra_ids, int n_extra,
                           float *out_vals, int32_t *out_ids);
/* Probability of one target per logits row on the device: out_probs[i] = util::softmax(row)[targets[i]] of the reference
 * (crates/llm-base/src/util.rs:143-151) for the rows row_begin .. row_begin + n_rows - 1 of the 2-D f32 tensor `logits` — a
 * node of the caller's most recent ggml_graph_compute, or a tensor handed to ggml_hip_transform_tensor.  What
 * InferenceSession::perplexity (inference_session.rs:577-583) takes from every counted position: n_rows floats cross PCIe
 * instead of n_rows * ne0.  A target whose probability underflows gives 0, a row holding NaN gives NaN.  Returns 0, or -1 on
 * bad arguments (NULL pointers, n_rows < 1, row_begin < 0, rows beyond ne1, a tensor that is not F32 / 2-D / on the device, a
 * target outside [0, ne0)); everything but the device image is checked before the device is touched. */
GGML_API int ggml_hip_row_probs(const struct ggml_tensor *logits, int64_t row_begin, int64_t n_rows, const int32_t *targets,
                                float *out_probs);
/* ggml_quantize_q4_0 / q4_1 / q5_0 / q5_1 / q8_0 (crates/ggml/src/lib.rs:419-483, called by
 * crates/llm-base/src/quantize.rs:363-379) computed on the device: n f32 values at `src` (host memory, rows
 * of k, k % 32 == 0) -> raw GGML blocks at `dst` (host memory), byte-identical to the host functions; the 16-bin
 * histogram is ADDED to hist (may be NULL).  Returns the bytes written.  PCIe-bound: ~1.2 bytes moved per weight.
 * Also ggml_quantize_q2_K .. q6_K (k % 256 == 0, one wave per super-block: kernels/kquant_encode.h), which leave hist
 * untouched. */
GGML_API size_t ggml_hip_quantize(enum ggml_type type, const float *src, void *dst, int64_t n, int64_t k, int64_t *hist);
/* The same for a matrix that already lives in HBM: `src` is a contiguous 2-D f32 or f16 tensor previously handed to
 * ggml_hip_transform_tensor; `dst` is a tensor of a 32-wide block type with the same shape whose data pointer names the
 * result (its host bytes are neither read nor written).  After the call dst is a device-resident quantized weight
 * (GGML_BACKEND_GPU, extra set) exactly as if the host-quantized blocks had been uploaded: mul_mat / get_rows accept
 * it; nothing crosses PCIe.  Returns 0, -1 if the precondition does not hold. */
GGML_API int ggml_hip_quantize_resident(const struct ggml_tensor *src, struct ggml_tensor *dst, int64_t *hist);
/* In-kernel timeline of the decode mat-vec launches (ggml_hip_set_option("timeline", 1), eager or graph mode):
 * records of 8 x int64 {entry, loads issued, x staged, barrier passed, first weights landed, exit (100 MHz
 * wall clock ticks), steps of wave 0, workgroup id}; 4 (or "timeline" = n) sampled workgroups per launch, launch order.
 * Returns the number of records copied. */
GGML_API size_t ggml_hip_read_timeline(int64_t *dst, size_t max_records);
/* Test hook (no reference counterpart): the attention of a prompt batch — mul_mat(K, Q), scale, diag_mask_inf, soft_max,
 * mul_mat(V, P), merge heads (crates/models/llama/src/lib.rs:246-307) — on host arrays, through the fused kernel
 * (fused != 0) or the three-launch path of the prompt plan.  q [N][E] f32 (RoPE applied), mem_k [C][Egqa] f16,
 * mem_v [Egqa][C] f16, out [N][E] f32.  0 on success, -1 if the shape is not accepted. */
GGML_API int ggml_hip_debug_prompt_attention(const float *q, const uint16_t *mem_k, const uint16_t *mem_v, float *out, int N, int E,
                                             int Egqa, int H, int n_past, int64_t C, float scale, int fused);
/* Test hook: the fused prompt attention in the form the prompt plan launches it: q_raw [N][E] f32 is the UN-rotated wq product,
 * q_raw2 (may be NULL) the second partial of a K-split GEMM, added first; rope [N][128] f32 holds (cos, sin) per pair and token
 * (the plan's RoPE table), applied while Q is staged; the result leaves as wo's GEMM operand x16 [N][E] f16: every 32-channel
 * block re-quantized to Q8 (block scale rounded to f16 first when f16d != 0) and stored as f16(d * q) in the GEMM's k order.
 * x16 and out (f32 [N][E], may be NULL: the plain form's output buffer, which this form leaves unwritten) hold their elements
 * and 256 bytes more; both are 0xFF bytes before the launch and come back whole.  0 on success, -1 if the shape is not accepted. */
GGML_API int ggml_hip_debug_prompt_attention_plan(const float *q_raw, const float *q_raw2, const float *rope, const uint16_t *mem_k,
                                                  const uint16_t *mem_v, uint16_t *x16, float *out, int N, int E, int Egqa, int H,
                                                  int n_past, int64_t C, float scale, int f16d);
/* Test hook: the fused prompt attention's exponential against expf over ALL f16 arguments: out_fast[i] = f16(exp_le0(x_i)),
 * out_ref[i] = f16(expf(x_i)) for the 65536 f16 bit patterns i (65536 f16 bit patterns each).  The softmax only ever passes
 * x <= 0 or NaN (crates/models/llama/src/lib.rs:272-280: soft_max over masked, scaled scores).  Returns 0. */
GGML_API int ggml_hip_debug_exp_le0(uint16_t *out_fast, uint16_t *out_ref);
/* Test hook: k_token_tail (the last kernel of a greedy token's graph) alone, beside k_argmax_next on the same logits.  logits[V]
 * and emb[E] (nullable) go to the device, each `misalign` (0..3) floats off a 16-byte boundary; both kernels start from the
 * parameters {n_past, token 0}.  Out: the id each kernel sampled, the logits and the row as they arrived in the pinned result
 * slot, prm_out[0..2] = n_past, token, tokens[0] as k_token_tail left them for the next replay.  0, or -1 for arguments it
 * cannot take. */
GGML_API int ggml_hip_debug_token_tail(const float *logits, int V, const float *emb, int E, int n_past, int misalign,
                                       int32_t *id_tail, int32_t *id_argmax, float *slot_logits, float *slot_emb, int32_t *prm_out);
/* Test hook: k_token_tail preparing the next token (option tail_prepare), beside the three launches it stands for.  logits[V];
 * wte_raw: V rows of E elements in the block format `wtype` (GGML_TYPE_Q4_0 .. Q8_0); mem_k [L][C][Egqa], mem_v [L][Egqa][C] f16.
 * The parameters start at position n_past (n_past + 1 < C), the granule epoch at epoch_in.  One launch of the tail of parity
 * `parity` (0 / 1) prepares position n_past + 1 — with `zeroed` != 0 the same launch is given a zeroed argument struct and must
 * write none of it; beside it k_argmax_next, then k_get_rows_q, k_rope_table and k_kv_row_save run on a second set of parameters.
 * Out, from the tail / from those launches (_ref): row [E], table [128] (the first 2 * half_d are written), the epoch, save
 * [2 * L * Egqa] f16 (K rows, then V columns) — 0xFF bytes where never written; id_out: the id in the tail's slot; prm_out[0..4] =
 * n_past, token, tokens[0] and the two position words of the tails as the launch left them.  0, or -1 for arguments it cannot take. */
GGML_API int ggml_hip_debug_token_tail_prepare(const float *logits, int V, const void *wte_raw, int wtype, int E, int n_past,
                                               uint32_t epoch_in, int parity, int zeroed, int L, int C, int Egqa,
                                               const uint16_t *mem_k, const uint16_t *mem_v, float theta_scale, float freq_scale,
                                               int half_d, int32_t *id_out, int32_t *prm_out, float *row, float *table,
                                               uint32_t *epoch_out, uint16_t *save, float *row_ref, float *table_ref,
                                               uint32_t *epoch_ref, uint16_t *save_ref);
/* Test hook: k_argmax_next with a BatchCols (the kernel between two steps of ggml_hip_decode_batch_greedy) alone.  logits [B][V], B = 1..8;
 * pos_in[8] and tokens_in[32] are the positions and token ids a step's parameters hold before it.  Out: ids_out[B] the sampled ids,
 * prm_out[34] = n_past, token, tokens[0..32) and pos_out[8] as the kernel left them.  0, or -1 for arguments it cannot take. */
GGML_API int ggml_hip_debug_batch_tail(const float *logits, int B, int V, const int32_t *pos_in, const int32_t *tokens_in,
                                       int32_t *ids_out, int32_t *prm_out, int32_t *pos_out);
/* Test hook: k_sample_next with a BatchCols (the kernel between two steps of ggml_hip_decode_batch_sampled) alone, n_draws (1 .. 4096) launches
 * on the same rows.  logits [B][V], B = 1..8; pos_in[8] / tokens_in[32] as above; hist [8][64] and hist_n[8] are the columns'
 * history rings (hist_n[c] tokens pushed so far: min(hist_n, 64) entries hold, the next goes to slot hist_n % 64), rng[8] the
 * generator states: all three in / out, all 8 entries.  Out: ids_out [n_draws][B], prm_out[34], pos_out[8] as above.  0, or -1
 * for arguments it cannot take (the sampler parameters ggml_hip_decode_batch_sampled declines among them). */
GGML_API int ggml_hip_debug_batch_sample(const float *logits, int B, int V, const ggml_hip_sampler *params, const int32_t *pos_in,
                                         const int32_t *tokens_in, int32_t *hist, int32_t *hist_n, uint64_t *rng, int n_draws,
                                         int32_t *ids_out, int32_t *prm_out, int32_t *pos_out);
/* Test hook: k_sample_next (the kernel between two replays of ggml_hip_decode_sampled_chain) alone, n_draws (1 .. 4096) launches on
 * one row logits [V], in the form the chain picks for that V.  n_past_in / tokens_in[32]: the DecParams before the first launch
 * (token = tokens_in[0]); hist[64], *hist_n and *rng: the ring, its count and the generator state, in / out.  Out: ids_out[n_draws],
 * prm_out[34] = n_past, token, tokens[0..32).  0, or -1 for arguments it cannot take (what the chain declines among them). */
GGML_API int ggml_hip_debug_sample_next(const float *logits, int V, const ggml_hip_sampler *params, int n_past_in,
                                        const int32_t *tokens_in, int32_t *hist, int32_t *hist_n, uint64_t *rng, int n_draws,
                                        int32_t *ids_out, int32_t *prm_out);
/* Test hook: the two hooks above with the whole sampler (one body): pos_in == NULL is ggml_hip_debug_sample_next's form (B = 1,
 * n_past_in, hist[64], one count, one rng, one mu), otherwise ggml_hip_debug_batch_sample's (n_past_in ignored; hist [8][64], hist_n[8],
 * rng[8], mu[8], all 8 entries in / out).  mu may be NULL when chain->mirostat == 0. */
GGML_API int ggml_hip_debug_next_token_ex(const float *logits, int B, int V, const ggml_hip_sampler_chain *chain, int n_past_in,
                                          const int32_t *pos_in, const int32_t *tokens_in, int32_t *hist, int32_t *hist_n, uint64_t *rng,
                                          float *mu, int n_draws, int32_t *ids_out, int32_t *prm_out, int32_t *pos_out);
/* Test hook: the kernel(s) between two steps of the chains that stop, alone, n_draws rounds on the same rows: the hook above with a
 * request per column — chains [B] (NULL entries: the first maximum) and ends [B], whose budget is here the number of DRAWS the
 * column may make (0 .. n_draws; 0 = frozen from the start).  Out besides the hook's: n_drawn [B] and ended_by [B]; a frozen column's
 * entries of ids_out are -1. */
GGML_API int ggml_hip_debug_next_token_req(const float *logits, int B, int V, const ggml_hip_sampler_chain *const *chains,
                                           const ggml_hip_chain_end *ends, int n_past_in, const int32_t *pos_in, const int32_t *tokens_in,
                                           int32_t *hist, int32_t *hist_n, uint64_t *rng, float *mu, int n_draws, int32_t *ids_out,
                                           int32_t *prm_out, int32_t *pos_out, int32_t *n_drawn, int32_t *ended_by);
/* Test hook: ONE launch of k_pool_admit (kernels/pool_admit.h) on the caller's tables, every table read back in place.  The tables
 * are the device structures byte for byte: table (PoolTable), reqs (SampleReqs), scols (SampleCols), prm (DecParams), bcols
 * (BatchCols; its pointers are copied, never followed); sizes [5] their sizes in that order, which must be the library's own
 * (ggml_hip_debug_pool_admit_sizes fills them in).  logits [n_cols][V], emb [n_cols][E]; slot_logits [n_pool][V] and slot_emb
 * [n_pool][E] go up and come back.  -1 before any device is touched: NULLs, wrong sizes, n_cols outside 2 .. 8, n_pool outside
 * n_cols .. 64, V or E < 1, a table whose head disagrees with n_cols / n_pool or whose cursor, owners or classes are out of range. */
GGML_API void ggml_hip_debug_pool_admit_sizes(int64_t *sizes);
GGML_API int ggml_hip_debug_pool_admit(void *table, void *reqs, void *scols, void *prm, void *bcols, const int64_t *sizes, int n_cols, int n_pool,
                                       const float *logits, const float *emb, int V, int E, float *slot_logits, float *slot_emb);
/* Test hook: w (quantized 2-D weight with a device copy) times N = 2..8 host rows x [N][K] through k_mmq_cols as the
 * multi-token plan launches it; out [N][M].  0, or -1 when that plan would not run this shape on k_mmq_cols. */
GGML_API int ggml_hip_debug_mul_mat_cols(const struct ggml_tensor *w, const float *x, float *out, int N);
/* Test hooks: ONE launch of the single-token plans' mat-vec — k_mmvq_big (Q4_0 .. Q8_0) / k_mmvq_kbig (K-quants) — with the
 * activation source and epilogue pairs the plans launch (xsrc / epi: 0 Q8 / 1 NORM / 2 F32 and 0 STORE / 1 ADD / 2 GATE / 3 QKV
 * for _big; 1 NORM / 2 F32 / 3 SILU_MUL and 0 ROW / 1 GATE / 2 QKV for _kbig).  w0 (w1, w2): weights with device copies; x, xw /
 * norm_w [K]; res; out, y_out (the normed row); QKV: n_past, head size D, RoPE base and scale, cache length C, mem_k [C][Egqa] /
 * mem_v [Egqa][C] f16 in-out.  Every output and in-out host buffer holds its elements and 256 bytes more: they come back from the
 * device as they were behind the elements (0xFF before the launch).  0, or -1 for what the plans would not launch. */
GGML_API int ggml_hip_debug_mat_vec_big(const struct ggml_tensor *w0, const struct ggml_tensor *w1, const struct ggml_tensor *w2,
                                        int xsrc, int epi, const float *x, const float *norm_w, float eps, const float *res, float *out,
                                        float *y_out, int n_past, int D, float freq_base, float freq_scale, int64_t C,
                                        uint16_t *mem_k, uint16_t *mem_v);
GGML_API int ggml_hip_debug_mat_vec_kbig(const struct ggml_tensor *w0, const struct ggml_tensor *w1, const struct ggml_tensor *w2,
                                         int xsrc, int epi, const float *x, const float *xw, float eps, const float *res, float *out,
                                         float *y_out, int n_past, int D, float freq_base, float freq_scale, int64_t C,
                                         uint16_t *mem_k, uint16_t *mem_v);
/* ... and of the F16 plan's mat-vec k_mmvq_f16 (kernels/decode_f16.h), xsrc / epi as for _kbig, with ncols columns as a chunk of
 * ncols tokens launches them: x [ncols][K], xw [K] (NORM) or [ncols][K] (SILU_MUL), res [ncols][M0], out [ncols][M], y_out [ncols][K];
 * QKV: column c sits at position n_past + c.  w0 (w1, w2): contiguous F16 matrices.  -1 for K % 8 != 0, an odd row count with QKV
 * and whatever else the plan would not launch. */
GGML_API int ggml_hip_debug_mat_vec_f16(const struct ggml_tensor *w0, const struct ggml_tensor *w1, const struct ggml_tensor *w2,
                                        int xsrc, int epi, const float *x, const float *xw, float eps, const float *res, float *out,
                                        float *y_out, int n_past, int D, float freq_base, float freq_scale, int64_t C,
                                        uint16_t *mem_k, uint16_t *mem_v, int ncols);
/* Test hook: ONE launch of an activation quantizer kernel (Q8_0 / Q8_1 planar rows, the int8 and f16 GEMM operands, Q8_K) on host
 * arrays, with the launch geometry of its call sites.  a [rows][K] f32 (the strided kinds: [rows][stride], stride >= K floats), b the
 * second input (SiLU kinds: w3 x; P_NORM_QUANT: the second K-split partial, nullable), r the residual (P_NORM_QUANT's ADD form,
 * nullable), w [K] and eps the norm's; part != 0 (P_SILU_MUL_QUANT): second partials `part` floats on in a and b; zp: the zero point
 * of QUANT_ACT_I8 (8, 16 or 0).  flags: 1 = d after its f16 round trip (the Q8_0 kind), 2 = with the [block][8] tables dT / sT, 4 = the
 * Q8_K round trip form of the P_* kinds.  outs: the kind's output buffers in the order listed at the definition
 * (llm_amd/csrc/debug_quant_attn.inc), each holding its elements and 256 bytes more, which come back as the device holds them (0xFF
 * before the launch).  0, or -1 for what no call site launches. */
enum ggml_hip_act_quant_kind {
    GGML_HIP_AQ_QUANTIZE_ACT = 0, GGML_HIP_AQ_QUANT_ROW, GGML_HIP_AQ_RMSNORM_QUANT, GGML_HIP_AQ_RMSNORM_QUANT_WARM,
    GGML_HIP_AQ_QUANT_ACT_I8, GGML_HIP_AQ_QUANT_ACT_F16, GGML_HIP_AQ_P_QUANT4, GGML_HIP_AQ_P_SILU_MUL_QUANT, GGML_HIP_AQ_P_NORM_QUANT,
    GGML_HIP_AQ_QUANT_ACT_F16_K, GGML_HIP_AQ_F32_TO_W16, GGML_HIP_AQ_QUANT_Q8K, GGML_HIP_AQ_K_NORM_QUANT, GGML_HIP_AQ_K_QUANT,
    GGML_HIP_AQ_K_SILU_MUL_QUANT
};
GGML_API int ggml_hip_debug_act_quant(int kind, int flags, int64_t rows, int64_t K, int64_t stride, const float *a, const float *b,
                                      const float *r, const float *w, float eps, int64_t part, int zp, void *const *outs);
/* Test hook of the MPT decode plan's two kernels with arithmetic of their own (option plan_mpt; llm_amd/csrc/kernels/mpt_plan.h), on
 * host arrays.  op 0: the LayerNorm staging of its mat-vecs — x [K], the gain w [K], eps; out[0..3] = the planar Q8 blocks one workgroup
 * stages: lo, hi [K/2] int8, d [K/32] f32 (flag 1: after its f16 round trip), sum [K/32] i32.  op 1: the ALiBi decode attention over
 * token-major caches — x = q [H*D], w = the slopes [H], mem_k / mem_v [C][H*D] f16, the token at n_past, scale; out[0] [H*D] f32.
 * op 2 (test-only state): flag != 0 = MPT plans built from now on carry a slope table with every head on the first sequence; cached
 * plans are dropped.  op 3: x = a ggml_cgraph *: 1 if the MPT matcher takes it under the current options, 0 if not; nothing is executed.
 * Every output is followed by 256 guard bytes (0xFF before the launch).  0, or -1 for what no call site launches. */
GGML_API int ggml_hip_debug_mpt(int op, int flag, const float *x, const float *w, float eps, int64_t K, const uint16_t *mem_k,
                                const uint16_t *mem_v, int H, int D, int n_past, int64_t C, float scale, void *const *out);
/* Extension (layer split inside one process): slot `slot` enqueues on slot `with_slot`'s stream (with_slot < 0: on its own again).
 * Only for slots of ONE physical GPU whose work never overlaps — the stages of one split session: a wait on another queue's event
 * costs tens of microseconds per stage boundary on this runtime, the same wait inside one queue nothing.  1 = now shared, 0 = not
 * (different GPUs, a slot not initialised).  The host mirror calls it from llm_start_session / llm_session_free. */
GGML_API int ggml_hip_share_stream(int slot, int with_slot);
GGML_API const char *ggml_hip_version(void);

#ifdef __cplusplus
}
#endif

/* ---- ABI layout checks: the numbers of the bindgen layout tests (lib.rs:174-238, 261-446, 458-533,
 * 546-651, 659-705, 711-755, 769-830, 2907-2972) ------------------------------------------------ */
#ifdef __cplusplus
#define GGML_ABI_ASSERT(c, m) static_assert(c, m)
#else
#define GGML_ABI_ASSERT(c, m) _Static_assert(c, m)
#endif
GGML_ABI_ASSERT(sizeof(struct ggml_object) == 32, "ggml_object size (lib.rs:239)");
GGML_ABI_ASSERT(offsetof(struct ggml_object, type) == 24, "ggml_object.type");
GGML_ABI_ASSERT(sizeof(struct ggml_tensor) == 272, "ggml_tensor size (lib.rs:446)");
GGML_ABI_ASSERT(offsetof(struct ggml_tensor, ne) == 16, "ggml_tensor.ne");
GGML_ABI_ASSERT(offsetof(struct ggml_tensor, nb) == 48, "ggml_tensor.nb");
GGML_ABI_ASSERT(offsetof(struct ggml_tensor, op) == 80, "ggml_tensor.op");
GGML_ABI_ASSERT(offsetof(struct ggml_tensor, op_params) == 84, "ggml_tensor.op_params");
GGML_ABI_ASSERT(offsetof(struct ggml_tensor, is_param) == 116, "ggml_tensor.is_param");
GGML_ABI_ASSERT(offsetof(struct ggml_tensor, grad) == 120, "ggml_tensor.grad");
GGML_ABI_ASSERT(offsetof(struct ggml_tensor, src) == 128, "ggml_tensor.src");
GGML_ABI_ASSERT(offsetof(struct ggml_tensor, perf_runs) == 176, "ggml_tensor.perf_runs");
GGML_ABI_ASSERT(offsetof(struct ggml_tensor, data) == 200, "ggml_tensor.data");
GGML_ABI_ASSERT(offsetof(struct ggml_tensor, name) == 208, "ggml_tensor.name");
GGML_ABI_ASSERT(offsetof(struct ggml_tensor, extra) == 256, "ggml_tensor.extra");
GGML_ABI_ASSERT(offsetof(struct ggml_tensor, padding) == 264, "ggml_tensor.padding");
GGML_ABI_ASSERT(sizeof(struct ggml_cplan) == 16424, "ggml_cplan size");
GGML_ABI_ASSERT(offsetof(struct ggml_cplan, n_tasks) == 20, "ggml_cplan.n_tasks");
GGML_ABI_ASSERT(offsetof(struct ggml_cplan, abort_callback) == 16408, "ggml_cplan.abort_callback");
GGML_ABI_ASSERT(sizeof(struct ggml_cgraph) == 164520, "ggml_cgraph size (lib.rs:651)");
GGML_ABI_ASSERT(offsetof(struct ggml_cgraph, nodes) == 8, "ggml_cgraph.nodes");
GGML_ABI_ASSERT(offsetof(struct ggml_cgraph, leafs) == 65544, "ggml_cgraph.leafs");
GGML_ABI_ASSERT(offsetof(struct ggml_cgraph, visited_hash_table) == 98312, "ggml_cgraph.visited_hash_table");
GGML_ABI_ASSERT(offsetof(struct ggml_cgraph, perf_runs) == 164496, "ggml_cgraph.perf_runs");
GGML_ABI_ASSERT(sizeof(struct ggml_scratch) == 24, "ggml_scratch size");
GGML_ABI_ASSERT(sizeof(struct ggml_init_params) == 24, "ggml_init_params size");
GGML_ABI_ASSERT(sizeof(struct ggml_compute_params) == 32, "ggml_compute_params size");
GGML_ABI_ASSERT(offsetof(struct ggml_compute_params, wsize) == 16, "ggml_compute_params.wsize");
GGML_ABI_ASSERT(sizeof(ggml_type_traits_t) == 40, "ggml_type_traits_t size");

#endif /* GGML_HIP_H */
