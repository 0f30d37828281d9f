// perplexity_driver.cpp — the workload of the sanitizer job for InferenceSession::perplexity (tests/test_sanitize_perplexity.py):
// llm_amd/csrc/host/llm_perplexity.cpp with llm_host.cpp and ggml_core.cpp under ASan + UBSan, linked against
// tests/sanitize/stub_backend.cpp and tests/sanitize/stub_row_probs.cpp.  Walks the loop of crates/llm-base/src/
// inference_session.rs:519-589 over context_size = 64 with n_batch 8, 9, 24, 64 and 100: chunking, the BOS replace-and-restore,
// the window arithmetic and the indexing of out_probs are checked against the stub's (row, target) -> value function.
// usage: perplexity_driver <model.ggjt>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ggml_hip.h"
#include "host/llm_host.h"

#define CHECK(c)                                                                        \
    do {                                                                                \
        if (!(c)) {                                                                     \
            fprintf(stderr, "perplexity driver: CHECK failed at line %d: %s\n", __LINE__, #c); \
            exit(2);                                                                    \
        }                                                                               \
    } while (0)

extern "C" float stub_row_prob_value(int64_t row, int32_t target);
extern "C" long stub_row_probs_calls(void);
extern "C" long stub_row_probs_rows(void);

int main(int argc, char **argv) {
    CHECK(argc == 2);
    const int C = 64, FIRST = 32, PER = 31;  // the counted window of a 64-token chunk: positions 32..62
    llm_model_params mp = {C, 1, -1, 0, 1.0f, 10000, 0, -1, 0};
    llm_model *m = llm_llama_load(argv[1], &mp);
    CHECK(m && llm_model_context_size(m) == C);
    const int V = llm_model_n_vocab(m);
    std::vector<int32_t> toks(3 * C + 5);
    for (size_t i = 0; i < toks.size(); i++) toks[i] = (int32_t)((i * 37 + 11) % (size_t)V);
    const std::vector<int32_t> before = toks;
    for (int n_batch : {8, 9, 24, 64, 100}) {
        llm_session_config cfg = {GGML_TYPE_F16, GGML_TYPE_F16, n_batch, 4};
        llm_session *s = llm_start_session(m, &cfg);
        CHECK(s && llm_session_n_batch(s) == n_batch);
        CHECK(llm_session_logits_node(s, nullptr) == nullptr && llm_session_fetch_last_logits(s) == -1);  // nothing evaluated yet
        // ---- on the "device": exactly 3 * 31 floats of out_probs and 3 perplexities are written
        std::vector<float> ppl(3, -1.0f), probs(3 * PER, -1.0f);
        const long calls0 = stub_row_probs_calls(), rows0 = stub_row_probs_rows();
        CHECK(llm_session_perplexity(m, s, toks.data(), (int)toks.size(), 1, 1, ppl.data(), 3, probs.data()) == 3);
        CHECK(toks == before);
        CHECK(llm_session_n_past(s) == C);
        const int nb = n_batch < C ? n_batch : C;
        long want_calls = 0;
        for (int j = 0; j * nb < C; j++) {
            const int lo = j * nb > FIRST ? j * nb : FIRST, hi = (j + 1) * nb < C - 1 ? (j + 1) * nb : C - 1;
            if (lo < hi) want_calls++;
        }
        CHECK(stub_row_probs_calls() - calls0 == 3 * want_calls && stub_row_probs_rows() - rows0 == 3 * PER);
        float nll = 0.0f;
        int count = 0;
        for (int i = 0; i < 3; i++) {
            for (int p = FIRST; p < C - 1; p++) {  // position p: row p - j * n_batch of its batch, target the ORIGINAL token p + 1
                const float want = stub_row_prob_value(p % nb, before[(size_t)(i * C + p + 1)]);
                CHECK(probs[(size_t)(i * PER + p - FIRST)] == want);
                nll += -logf(want);
                count++;
            }
            CHECK(ppl[(size_t)i] == expf(nll / (float)count));  // running over the chunks, f32 in position order
        }
        int slot = -1;
        const struct ggml_tensor *node = llm_session_logits_node(s, &slot);
        CHECK(node && slot == 0 && node->ne[0] == V && node->ne[1] == C - (C - 1) / nb * nb);  // the last batch's logits
        CHECK(llm_session_last_logits(s) != nullptr);
        // ---- fewer outputs than chunks, no out_probs; a prompt shorter than the context; a token outside the vocabulary
        float one = -1.0f;
        CHECK(llm_session_perplexity(m, s, toks.data(), 2 * C + 63, 1, 1, &one, 1, nullptr) == 2 && one == ppl[0]);
        CHECK(llm_session_perplexity(m, s, toks.data(), 2 * C, 1, 1, nullptr, 0, nullptr) == 2);
        CHECK(llm_session_perplexity(m, s, toks.data(), C - 1, 1, 1, &one, 1, probs.data()) == 0);
        CHECK(llm_session_perplexity(m, s, toks.data(), 0, 1, 1, &one, 1, probs.data()) == 0);
        std::vector<int32_t> bad = before;
        bad[C + 40] = V;
        CHECK(llm_session_perplexity(m, s, bad.data(), (int)bad.size(), 1, 1, ppl.data(), 3, probs.data()) == -1);
        bad[C + 40] = -1;
        CHECK(llm_session_perplexity(m, s, bad.data(), (int)bad.size(), 1, 1, ppl.data(), 3, probs.data()) == -1);
        CHECK(llm_session_perplexity(m, s, toks.data(), (int)toks.size(), V, 1, ppl.data(), 3, probs.data()) == -1);   // a BOS outside the
        CHECK(llm_session_perplexity(m, s, toks.data(), (int)toks.size(), -1, 0, ppl.data(), 3, probs.data()) == -1);  // vocabulary
        // ---- the reference's shape: all logits on the host, util::softmax there (the stand-in's logits lie in [0, 1))
        std::vector<float> hp(3, -1.0f), hprobs(3 * PER, -1.0f);
        const long calls1 = stub_row_probs_calls();
        CHECK(llm_session_perplexity(m, s, toks.data(), (int)toks.size(), 1, 0, hp.data(), 3, hprobs.data()) == 3);
        CHECK(stub_row_probs_calls() == calls1 && llm_session_n_past(s) == C);
        for (float p : hprobs) CHECK(p > 0.0f && p < 1.0f);
        for (float p : hp) CHECK(p > 1.0f && p <= (float)V * 3.0f);
        // ---- and the session goes on: rewind one token and evaluate it again (ends exactly at the context's end)
        CHECK(llm_session_rewind(s, 1) == 0);
        llm_evaluate_flags(m, s, &toks[3 * C - 1], 1, 0, nullptr);
        CHECK(llm_session_n_past(s) == C);
        llm_session_free(s);
    }
    llm_model_free(m);
    printf("perplexity driver OK\n");
    return 0;
}
