/* llm_host.h — C entry points of the host-side mirror (llm_session.hpp and the llm_*.cpp beside it) of the reference's
 * crates/llm-base InferenceSession + crates/models/llama, so that tests and bench.py (Python, ctypes)
 * can drive the SAME call sequence a Rust user of rustformers/llm drives:
 *   llm::load → Model::start_session → InferenceSession::{feed_prompt, infer_next_token} → Model::evaluate.
 * Not part of the ggml drop-in ABI (include/ggml_hip.h); exported from the same shared object. */
#ifndef LLM_HOST_H
#define LLM_HOST_H
#include <stddef.h>
#include <stdint.h>

#include "ggml_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* crates/models/llama/src/lib.rs:399-416 Hyperparameters (+ n_ff, which the reference derives from
 * the w1 tensor shape in the file) */
typedef struct {
    int32_t n_vocab, n_embd, n_mult, n_head, n_head_kv, n_layer, n_rot, file_type;
} llm_llama_hparams;

/* crates/llm-base/src/model/mod.rs:196-229 ModelParameters (the fields that touch this path) */
typedef struct {
    int32_t context_size;   /* default 2048 */
    int32_t use_gpu;        /* must be 1: this library has no CPU compute path */
    int32_t gpu_layers;     /* -1 = all */
    int32_t has_rope_overrides;
    float rope_frequency_scale;
    int32_t rope_frequency_base;
    /* layer-split extension: this process owns layers [layer_begin, layer_end) */
    int32_t layer_begin, layer_end; /* 0,-1 = all */
    /* ModelParameters::n_gqa (crates/llm-base/src/model/mod.rs:213-214): grouped-query factor, 0 = None.  As in the reference
     * (crates/models/llama/src/lib.rs:106-117) it is honoured for models of 80 layers and more only ("temporary fix for 70B"):
     * n_head_kv = n_head / n_gqa; the container carries no n_head_kv. */
    int32_t n_gqa;
} llm_model_params;

/* crates/llm-base/src/inference_session.rs:799-841 InferenceSessionConfig */
typedef struct {
    int32_t memory_k_type; /* ggml_type: F16 (default) or F32 */
    int32_t memory_v_type;
    int32_t n_batch;   /* default 8 */
    int32_t n_threads; /* default 8 (ignored by the device executor) */
} llm_session_config;

/* one tensor handed to the loader: the TensorLoader::load(name) contract of
 * crates/llm-base/src/loader.rs:651-678 — name, type, dims ([in, out]) and a host pointer to the GGML
 * bytes (an mmap'd file region or a caller-owned buffer that outlives the model). */
typedef struct {
    const char *name;
    int32_t type; /* ggml_type */
    int32_t n_dims;
    int64_t ne[2];
    void *data;
} llm_tensor_desc;

typedef struct llm_model llm_model;
typedef struct llm_session llm_session;

GGML_API llm_model *llm_llama_new(const llm_llama_hparams *hp, const llm_model_params *params,
                                  const llm_tensor_desc *tensors, int n_tensors);
GGML_API void llm_model_free(llm_model *m);
/* Layer split of ONE model over several device slots of this process: llm_llama_new / llm_llama_load
 * split the layers into contiguous ranges, one per slot, when ggml_hip_set_tensor_split gave more than one slot a
 * positive share (the reference's hook, crates/ggml/src/accelerator/mod.rs:68-77) or GGML_HIP_LAYER_SPLIT=G asks for
 * equal shares; sessions of such a model walk the stages, the residual crosses with ggml_hip_copy_between_devices.
 * Returns the number of stages and, for the first `cap`, their layer ranges [begin, end) and device slots. */
GGML_API int llm_model_stages(const llm_model *m, int *layer_begin, int *layer_end, int *device, int cap);

/* GGML / GGMF v1 / GGJT v1-3 container reader with an mmap'd tensor section:
 * crates/ggml/src/format/loader.rs:160-281 (container walk, 32-byte alignment of GGJT tensor data, the
 * dims[0] % 64 rule for Q4_0/Q4_1) + crates/llm-base/src/loader.rs:419-567, 702-755 (mmap loader) +
 * crates/models/llama/src/lib.rs:425-447 (LLaMA hyperparameters) + loader.rs:32-50 (ftype = format +
 * 1000 * quantization_version).  Returns NULL after printing the LoadError-style reason to stderr. */
typedef struct llm_ggml_file llm_ggml_file;
GGML_API llm_ggml_file *llm_ggml_file_open(const char *path);
GGML_API void llm_ggml_file_close(llm_ggml_file *f);
/* container: 0 ggml, 1 ggmf, 2 ggjt, 3 ggla (hp all zero: a ggla file carries r and alpha, llm_ggml_file_lora); hp may be NULL */
GGML_API void llm_ggml_file_info(const llm_ggml_file *f, int *container, int *version, llm_llama_hparams *hp,
                                 int *n_tensors, int *n_vocab_entries);
/* i-th tensor in file order; desc->name / desc->data point into the mapping (valid until close) */
GGML_API int llm_ggml_file_tensor(const llm_ggml_file *f, int i, llm_tensor_desc *desc);
/* i-th vocabulary entry: returns the token's byte length, copies at most cap bytes, *score nullable */
GGML_API int llm_ggml_file_vocab(const llm_ggml_file *f, int i, char *buf, int cap, float *score);
/* llm::load for LLaMA: open + Llama::new over the mapping (kept alive by the model); hyperparameters from the file */
GGML_API llm_model *llm_llama_load(const char *path, const llm_model_params *params);
/* A ggla file (a LoRA adapter): returns 0 and its LoraParameters r and alpha; -1 for every other container */
GGML_API int llm_ggml_file_lora(const llm_ggml_file *f, int *r, int *alpha);
/* llm::load for LLaMA with ModelParameters::lora_adapters (crates/llm-base/src/loader.rs:486-531, 651-670): opens every
 * adapter, reads the model into a buffer the model owns (no mmap), patches each tensor named by an adapter with
 * LoraAdapter::patch's graph (lora.rs:71-141: W = W + (alpha / r) * mul_mat(A, B), computed through this library's ggml
 * in a CPU context, every adapter in the order given), then Llama::new.  NULL after a LoadError-style message. */
GGML_API llm_model *llm_llama_load_lora(const char *path, const llm_model_params *params, const char *const *lora_paths,
                                        int n_lora);
/* Accumulated host ns of llm_llama_load_lora: [0] model read, [1] adapter open, [2] patching as a whole, [3] the copies of
 * the patched tensors over the weights (part of [2]); reset != 0 clears them after the read */
GGML_API void llm_lora_timing(double *out4, int reset);
GGML_API llm_session *llm_start_session(llm_model *m, const llm_session_config *cfg);
/* a session of an unsplit model on another device slot of the model's GPU: own stream / shadows / K/V / plans, shared weights */
GGML_API llm_session *llm_start_session_on(llm_model *m, const llm_session_config *cfg, int slot);
GGML_API void llm_session_seek(llm_session *s, int n_past);
GGML_API void llm_session_set_speculate(llm_session *s, int on);
GGML_API void llm_session_free(llm_session *s);
/* Model::evaluate (models/llama/src/lib.rs:144-368): feeds n tokens at the session's n_past.
 * all_logits (nullable): n*n_vocab floats (OutputRequest.all_logits); embeddings (nullable): n_embd floats. */
GGML_API void llm_evaluate(llm_model *m, llm_session *s, const int32_t *tokens, int n, float *all_logits,
                           float *embeddings);
/* InferenceSession::feed_prompt with Prompt::Tokens (inference_session.rs:299-349): chunks by n_batch */
GGML_API void llm_feed_prompt(llm_model *m, llm_session *s, const int32_t *tokens, int n);
/* InferenceSession::infer_next_token with a greedy (argmax) sampler; returns the sampled token id */
GGML_API int32_t llm_infer_next_token_greedy(llm_model *m, llm_session *s);
/* The same step with the shape of the reference's DEFAULT sampler (samplers.rs:97-188: repetition penalty over the last 64 tokens,
 * top-k, temperature) instead of argmax; device_topk = 1 leaves the logits in HBM and reads k + 64 pairs (llm_session_topk),
 * 0 reads all n_vocab logits back as the reference does.  Both draw the same tokens from the same xorshift64* state. */
GGML_API int32_t llm_infer_next_token_topk(llm_model *m, llm_session *s, int k, float temperature, uint64_t *rng, int device_topk);
/* InferenceSession::rewind (inference_session.rs:352-378) */
/* n greedy tokens with the argmax on the device (ggml_hip_decode_greedy_chain): same ids and final logits as n calls
 * of llm_infer_next_token_greedy, no per-token logits read-back; falls back to that loop when chaining is impossible */
GGML_API int llm_infer_tokens_greedy_device(llm_model *m, llm_session *s, int n, int32_t *out);
/* One decode step of B sessions of ONE model, token tokens[i] for sessions[i], as one pass over the weights where the backend can
 * (ggml_hip_decode_batch: 2..8 sessions of a block-format or F16 model, or of a K-quant model under backend option plan_batch_k,
 * f16 K/V; nothing on the host asks for the weights' type: the backend decides): each session's single-token graph is built exactly as
 * llm_evaluate builds it, and each session ends as after llm_evaluate(m, sessions[i], &tokens[i], 1, ...) — n_past, last_logits; the
 * token history stays the caller's, as there.  logits (nullable): B * n_vocab floats, row i = session i's.
 * Returns 1 if the step ran batched, 0 if the sessions were evaluated one after the other (the backend declined: same results),
 * -1 on bad arguments with nothing evaluated: a session listed twice, of another model, of a layer-split model or on another device
 * slot than the calling thread's, a token outside the vocabulary, a session whose context is full. */
GGML_API int llm_evaluate_batch(llm_model *m, llm_session *const *sessions, const int32_t *tokens, int B, float *logits);
/* llm_infer_next_token_greedy for B sessions in one such step: out_ids[i] = the first maximum of session i's last_logits, appended to
 * its token history and evaluated.  Returns what llm_evaluate_batch returns. */
GGML_API int llm_infer_next_tokens_greedy_batch(llm_model *m, llm_session *const *sessions, int B, int32_t *out_ids);
/* the two entries above with the backend's batched step as a parameter (NULL: always one by one).  llm_infer.cpp is also built against
 * backends without ggml_hip_decode_batch; host/llm_batch.cpp binds the library's own. */
typedef int (*llm_batch_entry)(struct ggml_cgraph *const *graphs, int n_graphs);
GGML_API int llm_evaluate_batch_via(llm_batch_entry entry, llm_model *m, llm_session *const *sessions, const int32_t *tokens, int B,
                                    float *logits);
GGML_API int llm_infer_next_tokens_greedy_batch_via(llm_batch_entry entry, llm_model *m, llm_session *const *sessions, int B,
                                                    int32_t *out_ids);
/* n greedy tokens for each of B sessions of one model, sampled on the device (ggml_hip_decode_batch_greedy: every step one pass
 * over the weights, no host round trip between steps).  out_ids [n][B]: row k holds the k-th token of every session; row 0 is
 * the first maximum of each session's current last_logits.  Every session ends exactly as after n calls of
 * llm_infer_next_tokens_greedy_batch: n_past, token history, last_logits (after the n-th token), K/V.  Returns 1 if the chain
 * ran, 0 if the backend declined and that loop ran instead (same results), -1 with nothing evaluated and no session moved: the
 * bad arguments of llm_evaluate_batch, n < 1, a session with n_past + n beyond the context size.  (Stop ids and
 * budgets per session: llm_infer_until_batch.) */
GGML_API int llm_infer_tokens_greedy_batch_device(llm_model *m, llm_session *const *sessions, int B, int n, int32_t *out_ids);
/* ... with the backend's single step and its chain as parameters (either may be NULL), as the two _via entries above */
typedef int (*llm_batch_chain_entry)(struct ggml_cgraph *const *graphs, int n_graphs, int n_steps, int32_t *out_ids);
GGML_API int llm_infer_tokens_greedy_batch_via(llm_batch_entry step, llm_batch_chain_entry chain, llm_model *m,
                                               llm_session *const *sessions, int B, int n, int32_t *out_ids);
/* The sampler of the sampled batched chain: {k, top_p, temperature, penalty} — repetition penalty over the last 64 tokens, top-k,
 * top-p, temperature, a xorshift64* draw, specified on IEEE basic operations only (llm_amd/csrc/kernels/sampler_math.h, which the
 * device kernel compiles too).  The reference's default chain (samplers.rs:97-188) is {40, 0.95, 0.8, 1.30}. */
typedef ggml_hip_sampler llm_sampler_params;
/* One draw from a row of V logits (free of NaN): `window` holds the most recent tokens, oldest first (its last 64 count, each id once).
 * Returns the id and steps *rng once; -1 (and *rng unmoved) for k outside 1 .. V, a non-positive temperature, top_p or
 * penalty, or a window token outside the vocabulary.  Needs no device. */
GGML_API int32_t llm_sample_exact(const float *logits, int V, const int32_t *window, int n_window, const llm_sampler_params *params,
                                  uint64_t *rng);
/* llm_infer_next_tokens_greedy_batch with that sampler: out_ids[i] is drawn from session i's last_logits and the last 64 tokens of
 * its history with generator rngs[i], appended to the history and evaluated.  Returns what llm_evaluate_batch returns; on -1 no
 * session and no generator has moved. */
GGML_API int llm_infer_next_tokens_sampled_batch(llm_model *m, llm_session *const *sessions, int B, const llm_sampler_params *params,
                                                 uint64_t *rngs, int32_t *out_ids);
/* n such tokens for each of B sessions, rows 1 .. n - 1 drawn on the device (ggml_hip_decode_batch_sampled).  out_ids [n][B].  Every
 * session ends exactly as after n calls of llm_infer_next_tokens_sampled_batch — n_past, token history, last_logits, K/V — and every
 * generator too.  Returns 1 if the chain ran, 0 if the backend declined and that loop ran instead (same results), -1 with nothing
 * evaluated and no session or generator moved: the bad arguments of the greedy chain and of llm_sample_exact. */
GGML_API int llm_infer_tokens_sampled_batch_device(llm_model *m, llm_session *const *sessions, int B, int n,
                                                   const llm_sampler_params *params, uint64_t *rngs, int32_t *out_ids);
/* ... with the backend's entries as parameters (either may be NULL), as the greedy _via entries */
typedef int (*llm_batch_sample_entry)(struct ggml_cgraph *const *graphs, int n_graphs, int n_steps, const ggml_hip_sampler *params,
                                      const int32_t *windows, const int32_t *window_n, uint64_t *rng, int32_t *out_ids);
GGML_API int llm_infer_next_tokens_sampled_batch_via(llm_batch_entry entry, llm_model *m, llm_session *const *sessions, int B,
                                                     const llm_sampler_params *params, uint64_t *rngs, int32_t *out_ids);
GGML_API int llm_infer_tokens_sampled_batch_via(llm_batch_entry step, llm_batch_sample_entry chain, llm_model *m,
                                                llm_session *const *sessions, int B, int n, const llm_sampler_params *params,
                                                uint64_t *rngs, int32_t *out_ids);
/* llm_infer_next_token_greedy for a caller that samples: one draw by llm_sample_exact from last_logits and the last 64 tokens of the
 * history, appended and evaluated.  Steps *rng once.  -1 with nothing moved (and *rng unmoved) on llm_sample_exact's bad arguments.
 * Never arms the backend's run-ahead (that is the greedy caller's). */
GGML_API int32_t llm_infer_next_token_sampled(llm_model *m, llm_session *s, const llm_sampler_params *params, uint64_t *rng);
/* n such tokens drawn on the device (ggml_hip_decode_sampled_chain: k_sample_next between two replays of the session's single-token
 * plan; block-format, K-quant and F16 models alike).  out[n].  The session ends exactly as after n calls of
 * llm_infer_next_token_sampled — tokens, n_past, last_logits, K/V — and so does *rng.  Returns the number of tokens the DEVICE drew:
 * n behind a single-token step, n - 1 behind a prompt chunk or on a fresh session (one stepped token arms the chain), 0 when the
 * backend declines throughout and the stepped loop ran (same results); -1 with nothing moved: bad arguments (those of
 * llm_sample_exact, n < 1) or no room for n tokens. */
GGML_API int llm_infer_tokens_sampled_device(llm_model *m, llm_session *s, int n, const llm_sampler_params *params, uint64_t *rng,
                                             int32_t *out);
/* ... with the backend's entry as a parameter (NULL: always the stepped loop), as the batched _via entries */
typedef int (*llm_sample_chain_entry)(struct ggml_cgraph *last, int n, const ggml_hip_sampler *params, const int32_t *window,
                                      int window_n, uint64_t *rng, int32_t *out_tokens, float *last_logits);
GGML_API int llm_infer_tokens_sampled_via(llm_sample_chain_entry entry, llm_model *m, llm_session *s, int n,
                                          const llm_sampler_params *params, uint64_t *rng, int32_t *out);
/* ---- the whole sampler (ggml_hip_sampler_chain: the four parameters and flat bias, frequency / presence penalty, tail-free, locally
 * typical, min-p, Mirostat 2; specified at the head of llm_amd/csrc/kernels/sampler_math.h).  Every entry above that takes an
 * llm_sampler_params forwards to its _chain sibling below with neutral extras: same ids, same states. ---- */
typedef ggml_hip_sampler_chain llm_sampler_chain;
/* llm_sample_exact with that sampler, on the host, for any V: returns the id, steps *rng once and (mirostat == 2) moves *mu; -1 with
 * *rng and *mu unmoved for what the specification declines.  mu may be NULL when mirostat == 0.  Needs no device. */
GGML_API int32_t llm_sample_chain(const float *logits, int V, const int32_t *window, int n_window, const llm_sampler_chain *chain,
                                  uint64_t *rng, float *mu);
/* test hook: sampler_log2 of sampler_math.h, n values */
GGML_API void llm_sampler_log2(const double *r, int n, float *out);
GGML_API int32_t llm_infer_next_token_sampled_chain(llm_model *m, llm_session *s, const llm_sampler_chain *chain, uint64_t *rng, float *mu);
GGML_API int llm_infer_tokens_sampled_chain_device(llm_model *m, llm_session *s, int n, const llm_sampler_chain *chain, uint64_t *rng,
                                                   float *mu, int32_t *out);
GGML_API int llm_infer_next_tokens_sampled_chain_batch(llm_model *m, llm_session *const *sessions, int B, const llm_sampler_chain *chain,
                                                       uint64_t *rngs, float *mus, int32_t *out_ids);
GGML_API int llm_infer_tokens_sampled_chain_batch_device(llm_model *m, llm_session *const *sessions, int B, int n,
                                                         const llm_sampler_chain *chain, uint64_t *rngs, float *mus, int32_t *out_ids);
/* ... with the backend's entries as parameters (any may be NULL), as the _via entries above */
typedef int (*llm_sample_chain_ex_entry)(struct ggml_cgraph *last, int n, const ggml_hip_sampler_chain *chain, const int32_t *window,
                                         int window_n, uint64_t *rng, float *mu, int32_t *out_tokens, float *last_logits);
typedef int (*llm_batch_sample_ex_entry)(struct ggml_cgraph *const *graphs, int n_graphs, int n_steps, const ggml_hip_sampler_chain *chain,
                                         const int32_t *windows, const int32_t *window_n, uint64_t *rng, float *mu, int32_t *out_ids);
GGML_API int llm_infer_tokens_sampled_chain_via(llm_sample_chain_ex_entry entry, llm_model *m, llm_session *s, int n,
                                                const llm_sampler_chain *chain, uint64_t *rng, float *mu, int32_t *out);
GGML_API int llm_infer_next_tokens_sampled_chain_batch_via(llm_batch_entry entry, llm_model *m, llm_session *const *sessions, int B,
                                                           const llm_sampler_chain *chain, uint64_t *rngs, float *mus, int32_t *out_ids);
GGML_API int llm_infer_tokens_sampled_chain_batch_via(llm_batch_entry step, llm_batch_sample_ex_entry chain_entry, llm_model *m,
                                                      llm_session *const *sessions, int B, int n, const llm_sampler_chain *chain,
                                                      uint64_t *rngs, float *mus, int32_t *out_ids);
/* ---- generation that stops, as InferenceSession::infer does (inference_session.rs:381-424, :487-507): draw, evaluate, and end when
 * the token is one of the request's stop ids (it is still evaluated first, :404-408), when max_tokens were drawn, or where the
 * reference's loop would return ContextFull (:388: n_past + 1 reaches the context size).  A request per session: its own sampler
 * (chain == NULL: the first maximum), its own budget, up to 8 stop ids (every one inside the vocabulary). ---- */
typedef struct {
    const llm_sampler_chain *chain;
    int32_t max_tokens, n_stop, stop_id[8];
} llm_until_request;
enum { LLM_ENDED_BY_BUDGET = 1, LLM_ENDED_BY_STOP = 2, LLM_ENDED_BY_CONTEXT = 3 };
/* One session.  out[max_tokens]: the ids drawn, then -1; *n_out their number; *ended_by one of the above.  On the device where the
 * backend can (ggml_hip_decode_chain_requests: the chain ends by itself at the stop id and leaves the session where the stop token's
 * evaluation left it), after one stepped token behind a prompt chunk as llm_infer_tokens_sampled_chain_device; the stepped loop with
 * the same rule runs when it declines.  Tokens, n_past, last_logits, K/V, *rng and *mu end as the stepped loop leaves them.  Returns 1
 * if the device chain ran, 0 if the stepped loop did it all, -1 with nothing moved on bad arguments (those of llm_sample_chain,
 * max_tokens < 1, n_stop outside 0 .. 8, a stop id outside the vocabulary).  rng may be NULL for a greedy request. */
GGML_API int llm_infer_until(llm_model *m, llm_session *s, const llm_until_request *req, uint64_t *rng, float *mu, int32_t *out,
                             int32_t *n_out, int32_t *ended_by);
/* B sessions of one model, requests [B], rngs [B] / mus [B] (either may be NULL when no request needs it).  out_ids [n][B] with n the
 * largest max_tokens: column i holds session i's ids, then -1; n_out [B], ended_by [B].  One call of ggml_hip_decode_batch_requests
 * where the backend can (the host draws row 0; a session whose first token is already a stop id enters with a budget of one
 * evaluation), otherwise steps of the sessions that are still going.  Returns 1 / 0 / -1 as llm_infer_tokens_sampled_chain_batch_device. */
GGML_API int llm_infer_until_batch(llm_model *m, llm_session *const *sessions, int B, const llm_until_request *reqs, uint64_t *rngs,
                                   float *mus, int32_t *out_ids, int32_t *n_out, int32_t *ended_by);
/* ... with the backend's entries as parameters (any may be NULL), as the _via entries above */
typedef int (*llm_chain_requests_entry)(struct ggml_cgraph *last, int n, const ggml_hip_sampler_chain *chain, const ggml_hip_chain_end *end,
                                        const int32_t *window, int window_n, uint64_t *rng, float *mu, int32_t *out_tokens, int32_t *n_drawn,
                                        int32_t *ended_by, float *last_logits);
typedef int (*llm_batch_requests_entry)(struct ggml_cgraph *const *graphs, int n_graphs, int n_steps, const ggml_hip_sampler_chain *const *chains,
                                        const ggml_hip_chain_end *ends, const int32_t *windows, const int32_t *window_n, uint64_t *rng,
                                        float *mu, int32_t *out_ids, int32_t *n_evaluated, int32_t *ended_by);
GGML_API int llm_infer_until_via(llm_chain_requests_entry entry, llm_model *m, llm_session *s, const llm_until_request *req, uint64_t *rng,
                                 float *mu, int32_t *out, int32_t *n_out, int32_t *ended_by);
GGML_API int llm_infer_until_batch_via(llm_batch_entry step, llm_batch_requests_entry entry, llm_model *m, llm_session *const *sessions, int B,
                                       const llm_until_request *reqs, uint64_t *rngs, float *mus, int32_t *out_ids, int32_t *n_out,
                                       int32_t *ended_by);
/* ---- the request pool: N >= 1 fed sessions of one model, a request each, over at most max_cols (1 .. 8) columns.  A column whose
 * request has ended takes the next waiting session — on the device through ggml_hip_decode_pool_requests, which is called again for
 * whatever it left unfinished or unstarted (more than 64 requests; the step cap); a lone remainder goes through llm_infer_until; the
 * stepped loop under the same admission rule (kernels/pool_rule.h) runs when the backend has no such entry or declines.  A session
 * with no room reports LLM_ENDED_BY_CONTEXT and never enters the pool.  out_ids [N][n] with n the largest max_tokens: ROW i holds
 * session i's ids, then -1; n_out [N], ended_by [N].  Every session ends as llm_infer_until leaves it alone.  Returns 1 if the device
 * ran requests, 0 if the stepped loop did it all, -1 with nothing moved (generator states included) on bad arguments: those of
 * llm_infer_until_batch, max_cols outside 1 .. 8. ---- */
GGML_API int llm_infer_until_pool(llm_model *m, llm_session *const *sessions, int N, const llm_until_request *reqs, uint64_t *rngs, float *mus,
                                  int max_cols, int32_t *out_ids, int32_t *n_out, int32_t *ended_by);
typedef int (*llm_pool_requests_entry)(struct ggml_cgraph *const *graphs, int n_pool, int n_cols, int n_steps,
                                       const ggml_hip_sampler_chain *const *chains, const ggml_hip_chain_end *ends, const int32_t *windows,
                                       const int32_t *window_n, uint64_t *rng, float *mu, int32_t *out_ids, int32_t *col, int32_t *first_step,
                                       int32_t *n_evaluated, int32_t *ended_by, int32_t *steps_run);
GGML_API int llm_infer_until_pool_via(llm_batch_entry step, llm_chain_requests_entry single, llm_pool_requests_entry entry, llm_model *m,
                                      llm_session *const *sessions, int N, const llm_until_request *reqs, uint64_t *rngs, float *mus, int max_cols,
                                      int32_t *out_ids, int32_t *n_out, int32_t *ended_by);
/* The admission rule alone: n requests of evals[i] >= 1 evaluations over n_cols (1 .. 8, <= n) columns; col_out [n], first_step_out [n]
 * (either may be NULL): request i runs in column col_out[i] from step first_step_out[i].  Returns the number of steps, -1 on bad
 * arguments.  Needs no device. */
GGML_API int llm_pool_schedule(const int32_t *evals, int n, int n_cols, int32_t *col_out, int32_t *first_step_out);
/* ---- feeding the prompts of B >= 1 sessions of one model as packed prompt batches (ggml_hip_prompt_pack): `tokens` is the prompts back
 * to back, counts [B] (all >= 1) their lengths, max_rows 1 .. 4096 the rows of one evaluation (0 means 512).  Rounds follow ONE rule
 * (llm_pack_schedule): in every round the sessions are visited in index order and a session with tokens left takes min(left, room)
 * rows, room being what is left of max_rows; the round goes to the backend as those sessions' graphs, one per session, built as
 * llm_evaluate builds them and not computed (more than 64 sessions in a round: pieces of 64 in index order); repeat until nothing is
 * left.  The sessions' own n_batch is NOT consulted: the round is the unit.  Afterwards every session has its tokens appended, n_past
 * advanced and last_logits equal to its last row's logits, as llm_feed_prompt leaves it.  If the backend declines a round, that
 * round's sessions and all later rounds are fed one by one through llm_feed_prompt (each session's remaining tokens as one call, so a
 * call that never packs leaves exactly what llm_feed_prompt alone leaves).  Returns 1 if every round ran packed, 0 if any was
 * stepped, -1 with nothing moved on bad arguments: B < 1, a NULL session, the same session twice, a session of another model, of a
 * layer-split model or on another device slot than the calling thread's, a count < 1, a token outside the vocabulary, max_rows out
 * of range, a session for which llm_feed_prompt would report ContextFull. ---- */
GGML_API int llm_feed_prompt_batch(llm_model *m, llm_session *const *sessions, int B, const int32_t *tokens, const int32_t *counts,
                                   int max_rows);
typedef int (*llm_pack_entry)(struct ggml_cgraph *const *graphs, int n_graphs);
GGML_API int llm_feed_prompt_batch_via(llm_pack_entry entry, llm_model *m, llm_session *const *sessions, int B, const int32_t *tokens,
                                       const int32_t *counts, int max_rows);
/* ONE evaluation of ggml_hip_prompt_pack over all B <= 64 sessions' tokens: no rounds, no fallback (tests and tools).  all_logits
 * (nullable): [sum counts][n_vocab], every row's logits in order; embeddings (nullable): [B][n_embd], each session's last row.
 * 0 = it ran and every session moved as above; -1 = bad arguments or the backend declined, nothing moved. */
GGML_API int llm_prompt_pack(llm_model *m, llm_session *const *sessions, int B, const int32_t *tokens, const int32_t *counts,
                             float *all_logits, float *embeddings);
GGML_API int llm_prompt_pack_via(llm_pack_entry entry, llm_model *m, llm_session *const *sessions, int B, const int32_t *tokens,
                                 const int32_t *counts, float *all_logits, float *embeddings);
/* test hook: the session's graph for these n tokens at its n_past, built as llm_evaluate builds it and not computed (for
 * ggml_hip_prompt_pack); the session does not move.  NULL on bad arguments. */
GGML_API struct ggml_cgraph *llm_session_stage_rows(llm_model *m, llm_session *s, const int32_t *tokens, int n);
/* The rule for rounds alone: take_out (nullable) [rounds][B], row r = the rows each session takes in round r.  Returns the number of
 * rounds, -1 on bad arguments (NULL counts, B < 1, a count < 1, max_rows outside 0 .. 4096).  Needs no device. */
GGML_API int llm_pack_schedule(const int32_t *counts, int B, int max_rows, int32_t *take_out);
/* test hook: the most steps llm_infer_until_pool asks of one call of the entry (1 .. 4096, the default); returns the previous cap */
GGML_API int llm_pool_step_cap(int cap);
/* test hook: the end rule alone, on recorded logits rows [n_rows][V] (row t stands for the logits the t-th draw sees; the window is
 * `window` followed by the ids drawn so far; n_past counts up from n_past0 with every draw against context_size).  Draws with
 * llm_sample_chain (or the first maximum) until the rule ends the run or the rows run out (*ended_by = 0 then).  Needs no device. */
GGML_API int llm_until_rule(const float *rows, int n_rows, int V, const llm_until_request *req, const int32_t *window, int n_window,
                            int n_past0, int context_size, uint64_t *rng, float *mu, int32_t *out, int32_t *n_out, int32_t *ended_by);
GGML_API size_t llm_session_read_node_host(const llm_session *s, int from_end, void *dst, size_t max_bytes);
GGML_API int llm_session_rewind(llm_session *s, int num);
/* host nanoseconds per phase of the decode loop, accumulated: [0] adopt/build graph, [1] token write + plan,
 * [2] compute begin (match + enqueue), [3] speculative build of the next graph, [4] compute end (wait + copy),
 * [5] greedy argmax, [6] evaluate as a whole. */
GGML_API void llm_host_timing(double *out8, int reset);
GGML_API const float *llm_session_last_logits(const llm_session *s);
GGML_API int llm_session_n_past(const llm_session *s);
GGML_API int llm_model_n_vocab(const llm_model *m);
/* graph statistics of the last evaluate (for tests): nodes, leafs */
GGML_API void llm_session_last_graph_stats(const llm_session *s, int *n_nodes, int *n_leafs);

/* layer split: device addresses of the residual hand-off buffers of a stage session (NULL if absent) */
GGML_API void llm_session_stage_buffers(llm_session *s, void **in_dev, void **out_dev, size_t *nbytes);
/* raw K/V memory of a session (which: 0 = memory_k, 1 = memory_v; set: 0 = read into buf, 1 = write from buf);
 * buf == NULL returns the size.  The InferenceSnapshot payload (inference_session.rs:599-646). */
/* test hook: the greedy sampler's index (first maximum under `>`, NaNs never win); which = 1: the scalar loop */
GGML_API int llm_argmax_first(const float *logits, int n, int which);
/* layer ranges of an in-process split over G device slots for the fractions `split` (NULL = equal): bounds_out[0..G] */
GGML_API void llm_split_layers(int n_layer, int G, const float *split, int *bounds_out);
GGML_API size_t llm_session_kv(llm_session *s, int which, int set, void *buf, size_t nbytes);
/* InferenceSession::get_snapshot / from_snapshot (inference_session.rs:590-646): npast, config, tokens, last_logits and
 * the K/V memory (read from / written to the device).  snapshot: buf == NULL or cap too small returns the size needed.
 * from_snapshot: NULL on a malformed buffer or SnapshotError::MemorySizeMismatch. */
GGML_API size_t llm_session_snapshot(llm_session *s, void *buf, size_t cap);
GGML_API llm_session *llm_session_from_snapshot(llm_model *m, const void *buf, size_t n);
/* test hook: reads the device contents of a node of the last evaluated graph (by index, or k-th node named `name`) */
/* top-k prefilter of the last token's logits on the device (ggml_hip_topk): k (value, id) pairs, best first, then the
 * raw logits of extra_ids; 0 on success, -1 if there is no evaluated graph or the arguments are out of range */
GGML_API int llm_session_topk(const llm_session *s, int k, const int32_t *extra_ids, int n_extra, float *out_vals,
                              int32_t *out_ids);
GGML_API size_t llm_session_read_node(const llm_session *s, int index, const char *name, int occurrence, void *dst,
                                      size_t max_bytes);
/* Model::evaluate with the extensions of OutputRequest as flags: 1 = logits_on_device (the logits stay in HBM, last_logits is
 * not refreshed), 2 = intermediate_chunk (only enqueued where feed_prompt would do so); all_logits nullable (n * n_vocab) */
GGML_API void llm_evaluate_flags(llm_model *m, llm_session *s, const int32_t *tokens, int n, int flags, float *all_logits);
/* the logits node ([n_vocab, n] f32) of the last evaluated graph and the device slot that owns it; NULL without a graph */
GGML_API const struct ggml_tensor *llm_session_logits_node(const llm_session *s, int *device_slot);
/* read_last_token after an evaluation that left its logits on the device: last row of the logits node -> last_logits */
GGML_API int llm_session_fetch_last_logits(llm_session *s);
/* the thread works on device slot `slot` until the scope is closed; the caller's main device is then as it was found */
typedef struct llm_device_scope llm_device_scope;
GGML_API llm_device_scope *llm_device_scope_open(int slot);
GGML_API void llm_device_scope_close(llm_device_scope *scope);
GGML_API int llm_model_context_size(const llm_model *m);
GGML_API int llm_session_n_batch(const llm_session *s);
/* InferenceSession::perplexity (inference_session.rs:519-589; host/llm_perplexity.cpp) over n token ids.  Returns
 * n_chunk = n / context_size; out_perplexity[i] (first `cap` chunks) is what the reference hands to perplexity_callback(i, .):
 * the RUNNING exp(nll / count); out_probs (nullable) receives the probability of every counted position in order,
 * n_chunk * (context_size - 1 - first) floats, first = min(512, context_size / 2).  bos_token replaces the first token of
 * every chunk for the evaluation (the reference's bot_token_id().unwrap_or(1)); `tokens` is unchanged on return.
 * -1 if bos_token or a token of a chunk lies outside [0, n_vocab) (nothing is evaluated then).
 * on_device = 1: the logits stay in HBM and ggml_hip_row_probs reduces each counted row to its target's probability;
 * 0: the reference's shape, all logits read back and util::softmax on the host.  Every chunk starts at n_past = 0. */
GGML_API int llm_session_perplexity(llm_model *m, llm_session *s, const int32_t *tokens, int n, int32_t bos_token,
                                    int on_device, float *out_perplexity, int cap, float *out_probs);
/* synthetic GGML blocks for full-size benchmarks (deterministic in seed and block index) */
GGML_API void llm_synth_blocks(int type, void *dst, int64_t nblocks, uint64_t seed, float d_scale);
/* BASELINE.md section 4 weights at full size: ne1 rows of ne0 gaussians N(0, std^2) (counter-based generator, deterministic
 * in (seed, row)), each row quantized by ggml_quantize_q* into raw GGML blocks of `type` at dst; multi-threaded. */
GGML_API void llm_synth_gaussian(int type, void *dst, int64_t ne0, int64_t ne1, uint64_t seed, float std);

#ifdef __cplusplus
}
#endif
#endif
