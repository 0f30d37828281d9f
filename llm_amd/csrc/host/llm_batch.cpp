// llm_batch.cpp — the batched multi-session decode step of the session mirror bound to this library's backend: llm_evaluate_batch and
// llm_infer_next_tokens_greedy_batch are llm_infer.cpp's llm_*_batch_via with ggml_hip_decode_batch as the entry, and
// llm_infer_tokens_greedy_batch_device the chained one with ggml_hip_decode_batch_greedy beside it; the sampled chains likewise, the
// single session's (llm_infer_tokens_sampled_device, ggml_hip_decode_sampled_chain) among them.  A file of its own so that
// llm_infer.cpp keeps linking against backends that have no such entries.
#include "ggml_hip.h"
#include "llm_host.h"

extern "C" {
int llm_evaluate_batch(llm_model *m, llm_session *const *sessions, const int32_t *tokens, int B, float *logits) {
    return llm_evaluate_batch_via(ggml_hip_decode_batch, m, sessions, tokens, B, logits);
}
int llm_infer_next_tokens_greedy_batch(llm_model *m, llm_session *const *sessions, int B, int32_t *out_ids) {
    return llm_infer_next_tokens_greedy_batch_via(ggml_hip_decode_batch, m, sessions, B, out_ids);
}
int llm_infer_tokens_greedy_batch_device(llm_model *m, llm_session *const *sessions, int B, int n, int32_t *out_ids) {
    return llm_infer_tokens_greedy_batch_via(ggml_hip_decode_batch, ggml_hip_decode_batch_greedy, m, sessions, B, n, out_ids);
}
int llm_infer_next_tokens_sampled_batch(llm_model *m, llm_session *const *sessions, int B, const llm_sampler_params *params, uint64_t *rngs,
                                        int32_t *out_ids) {
    return llm_infer_next_tokens_sampled_batch_via(ggml_hip_decode_batch, m, sessions, B, params, rngs, out_ids);
}
int llm_infer_tokens_sampled_batch_device(llm_model *m, llm_session *const *sessions, int B, int n, const llm_sampler_params *params,
                                          uint64_t *rngs, int32_t *out_ids) {
    return llm_infer_tokens_sampled_batch_via(ggml_hip_decode_batch, ggml_hip_decode_batch_sampled, m, sessions, B, n, params, rngs, out_ids);
}
int llm_infer_tokens_sampled_device(llm_model *m, llm_session *s, int n, const llm_sampler_params *params, uint64_t *rng, int32_t *out) {
    return llm_infer_tokens_sampled_via(ggml_hip_decode_sampled_chain, m, s, n, params, rng, out);
}
// ... and with the whole sampler (llm_sampler_chain): the _ex entries
int llm_infer_next_tokens_sampled_chain_batch(llm_model *m, llm_session *const *sessions, int B, const llm_sampler_chain *chain, uint64_t *rngs,
                                              float *mus, int32_t *out_ids) {
    return llm_infer_next_tokens_sampled_chain_batch_via(ggml_hip_decode_batch, m, sessions, B, chain, rngs, mus, out_ids);
}
int llm_infer_tokens_sampled_chain_batch_device(llm_model *m, llm_session *const *sessions, int B, int n, const llm_sampler_chain *chain,
                                                uint64_t *rngs, float *mus, int32_t *out_ids) {
    return llm_infer_tokens_sampled_chain_batch_via(ggml_hip_decode_batch, ggml_hip_decode_batch_sampled_ex, m, sessions, B, n, chain, rngs, mus,
                                                    out_ids);
}
int llm_infer_tokens_sampled_chain_device(llm_model *m, llm_session *s, int n, const llm_sampler_chain *chain, uint64_t *rng, float *mu,
                                          int32_t *out) {
    return llm_infer_tokens_sampled_chain_via(ggml_hip_decode_sampled_chain_ex, m, s, n, chain, rng, mu, out);
}
// ... and the generation that stops: the chains with a request per session
int llm_infer_until(llm_model *m, llm_session *s, const llm_until_request *req, uint64_t *rng, float *mu, int32_t *out, int32_t *n_out,
                    int32_t *ended_by) {
    return llm_infer_until_via(ggml_hip_decode_chain_requests, m, s, req, rng, mu, out, n_out, ended_by);
}
int llm_infer_until_batch(llm_model *m, llm_session *const *sessions, int B, const llm_until_request *reqs, uint64_t *rngs, float *mus,
                          int32_t *out_ids, int32_t *n_out, int32_t *ended_by) {
    return llm_infer_until_batch_via(ggml_hip_decode_batch, ggml_hip_decode_batch_requests, m, sessions, B, reqs, rngs, mus, out_ids, n_out,
                                     ended_by);
}
// ... and the request pool
int llm_infer_until_pool(llm_model *m, llm_session *const *sessions, int N, const llm_until_request *reqs, uint64_t *rngs, float *mus, int max_cols,
                         int32_t *out_ids, int32_t *n_out, int32_t *ended_by) {
    return llm_infer_until_pool_via(ggml_hip_decode_batch, ggml_hip_decode_chain_requests, ggml_hip_decode_pool_requests, m, sessions, N, reqs, rngs,
                                    mus, max_cols, out_ids, n_out, ended_by);
}
// ... and the packed prompt batch (llm_pack.cpp)
int llm_feed_prompt_batch(llm_model *m, llm_session *const *sessions, int B, const int32_t *tokens, const int32_t *counts, int max_rows) {
    return llm_feed_prompt_batch_via(ggml_hip_prompt_pack, m, sessions, B, tokens, counts, max_rows);
}
int llm_prompt_pack(llm_model *m, llm_session *const *sessions, int B, const int32_t *tokens, const int32_t *counts, float *all_logits,
                    float *embeddings) {
    return llm_prompt_pack_via(ggml_hip_prompt_pack, m, sessions, B, tokens, counts, all_logits, embeddings);
}
}
