// stub_row_probs.cpp — a HOST stand-in for ggml_hip_row_probs (hip_backend.hip), used ONLY by the sanitizer job of the
// perplexity loop (tests/test_sanitize_perplexity.py), next to tests/sanitize/stub_backend.cpp which stands in for the rest of
// the device backend.  Nothing is reduced: the "probability" of a row is a function of (row index, target id) alone, so that
// the driver can tell from out_probs which row and which target every counted position was given.  The argument checks are
// the real hook's; every call is counted.  Never linked into libggml_hip.so.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <atomic>

#include "ggml_hip.h"

namespace {
std::atomic<long> g_calls{0}, g_rows{0};
}

extern "C" {
float stub_row_prob_value(int64_t row, int32_t target) { return 1.0f / (2.0f + (float)(target % 7) + 0.125f * (float)(row % 5)); }
long stub_row_probs_calls(void) { return g_calls; }
long stub_row_probs_rows(void) { return g_rows; }

int ggml_hip_row_probs(const struct ggml_tensor *t, int64_t row_begin, int64_t n_rows, const int32_t *targets, float *out_probs) {
    if (!t || !targets || !out_probs || n_rows < 1 || row_begin < 0 || t->type != GGML_TYPE_F32 || t->ne[2] != 1 || t->ne[3] != 1 ||
        n_rows > t->ne[1] || row_begin > t->ne[1] - n_rows || t->data == nullptr)
        return -1;
    g_calls++;
    g_rows += n_rows;
    for (int64_t r = 0; r < n_rows; r++) {
        if (targets[r] < 0 || targets[r] >= t->ne[0]) return -1;
        // the element the kernel would read for the numerator: inside the tensor, or ASan says so
        volatile float touch = *(const float *)((const char *)t->data + (row_begin + r) * t->nb[1] + (size_t)targets[r] * 4);
        (void)touch;
        out_probs[r] = stub_row_prob_value(row_begin + r, targets[r]);
    }
    return 0;
}
}
