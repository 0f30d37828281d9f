// llm_perplexity.cpp — InferenceSession::perplexity of the reference (crates/llm-base/src/inference_session.rs:519-589, the
// `llm perplexity` command) over the C entry points of llm_host.h (llm_state.cpp defines the ones written for it).  A translation
// unit of its own: it is the only host code that calls ggml_hip_row_probs, and the rest must keep linking against backends
// that do not have that hook.
//
// on_device = 1 keeps every batch's [n_vocab, N] logits in HBM (OutputRequest::logits_on_device) and asks the device for
// util::softmax(row)[target] of the counted rows only (kernels/nll.h): N floats cross the bus where the reference reads
// N * n_vocab and exponentiates all of them on the host.  on_device = 0 is the reference's shape, for comparison.
//
// One deliberate deviation: the reference never lowers n_past between chunks, so its second chunk writes the
// K/V views past context_size; here every chunk starts at n_past = 0, as the llama.cpp example it cites does.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "llm_host.h"

namespace {
// crates/llm-base/src/util.rs:143-151 softmax(logits)[target], in f32 with the reference's sequential sum
float softmax_entry(const float *logits, size_t n, size_t target) {
    float max_logit = -INFINITY;
    for (size_t i = 0; i < n; i++) max_logit = fmaxf(max_logit, logits[i]);  // f32::max: a NaN operand is ignored
    float sum = 0.0f;
    for (size_t i = 0; i < n; i++) sum += expf(logits[i] - max_logit);
    return expf(logits[target] - max_logit) / sum;
}
}  // namespace

extern "C" int llm_session_perplexity(llm_model *m, llm_session *s, const int32_t *tokens_in, int n, int32_t bos_token,
                                      int on_device, float *out_perplexity, int cap, float *out_probs) {
    if (!m || !s || !tokens_in || n < 0) return -1;
    std::vector<int32_t> tokens(tokens_in, tokens_in + n);  // :527 `let mut tokens`

    size_t count = 0;  // :529

    // :531 TODO of the reference: fewer than context_size tokens give no chunk
    if (llm_model_context_size(m) < 1) return -1;
    const size_t context_size = (size_t)llm_model_context_size(m);  // :532
    const size_t n_chunk = tokens.size() / context_size;            // :533
    const size_t n_vocab = (size_t)llm_model_n_vocab(m);            // :534
    const size_t n_batch = (size_t)std::max(1, llm_session_n_batch(s));  // :535
    if (bos_token < 0 || (size_t)bos_token >= n_vocab) return -1;  // (it goes into the embedding lookup like every other token)
    for (size_t i = 0; i < n_chunk * context_size; i++)
        if (tokens[i] < 0 || (size_t)tokens[i] >= n_vocab) return -1;  // (a target outside the row; the reference would panic on the index)

    float nll = 0.0f;  // :537

    const size_t first = std::min<size_t>(512, context_size / 2), last = context_size - 1;  // :577 the counted window [first, last)
    const size_t per_chunk = last > first ? last - first : 0;
    std::vector<float> logits, probs(per_chunk);
    std::vector<int32_t> targets;

    for (size_t i = 0; i < n_chunk; i++) {  // :539
        const size_t start = i * context_size;        // :540
        const size_t end = (i + 1) * context_size;    // :541

        const size_t num_batches = (context_size + n_batch - 1) / n_batch;  // :543

        llm_session_seek(s, 0);  // (the deviation: this chunk's K/V views start at position 0)

        for (size_t j = 0; j < num_batches; j++) {  // :547
            const size_t batch_start = start + j * n_batch;                     // :553
            const size_t batch_size = std::min(end - batch_start, n_batch);     // :554
            // the rows of this batch inside the counted window, as positions of the chunk: [lo, hi)
            const size_t lo = std::max(first, j * n_batch), hi = std::min(last, j * n_batch + batch_size);
            const bool counted = lo < hi;

            const int32_t token_org = tokens[batch_start];  // :557 save the original token at the start of the batch
            if (j == 0) tokens[batch_start] = bos_token;    // :560-562

            if (on_device) {
                // :564-568 Model::evaluate, the logits left in HBM; a batch nobody looks at is only enqueued, unless it is the
                // very last one (its last row becomes last_logits below)
                const bool final_batch = i + 1 == n_chunk && j + 1 == num_batches;
                llm_evaluate_flags(m, s, &tokens[batch_start], (int)batch_size, 1 | (!counted && !final_batch ? 2 : 0), nullptr);
            } else {
                logits.resize(batch_size * n_vocab);  // :548-551 OutputRequest { all_logits: Some(..) }
                llm_evaluate_flags(m, s, &tokens[batch_start], (int)batch_size, 0, logits.data());
            }

            tokens[batch_start] = token_org;  // :571 restore the original token

            if (!counted) continue;
            // :577-583, batch by batch instead of after the chunk (:574 keeps all logits of the chunk; nothing else reads them):
            // position p of the chunk is row p - j * n_batch of this batch, its target the ORIGINAL tokens[start + p + 1]
            const size_t row0 = lo - j * n_batch, rows = hi - lo;
            if (on_device) {
                targets.resize(rows);
                for (size_t p = lo; p < hi; p++) targets[p - lo] = tokens[start + p + 1];
                int slot = 0;
                const struct ggml_tensor *node = llm_session_logits_node(s, &slot);
                if (!node) return -1;
                llm_device_scope *scope = llm_device_scope_open(slot);  // the hook runs on the slot that owns the logits
                const int rc = ggml_hip_row_probs(node, (int64_t)row0, (int64_t)rows, targets.data(), probs.data() + (lo - first));
                llm_device_scope_close(scope);
                if (rc != 0) return -1;
            } else {
                for (size_t p = lo; p < hi; p++)  // :578-579
                    probs[p - first] = softmax_entry(&logits[(p - j * n_batch) * n_vocab], n_vocab, (size_t)tokens[start + p + 1]);
            }
        }

        for (size_t p = 0; p < per_chunk; p++) {  // :577
            nll += -logf(probs[p]);  // :580
            count += 1;              // :582
        }
        if (out_probs && per_chunk) memcpy(out_probs + i * per_chunk, probs.data(), per_chunk * sizeof(float));

        if (out_perplexity && (int)i < cap) out_perplexity[i] = expf(nll / (float)count);  // :585 perplexity_callback(i, ..)
    }
    // the session is where n_chunk * num_batches calls of Model::evaluate leave it: last_logits is the last row of the last batch
    if (on_device && n_chunk > 0 && llm_session_fetch_last_logits(s) != 0) return -1;
    return (int)n_chunk;
}
