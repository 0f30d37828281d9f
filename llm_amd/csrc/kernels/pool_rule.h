// pool_rule.h — the admission rule of the request pools (ggml_hip_decode_pool_requests, llm_infer_until_pool), once, for the device
// (k_pool_admit, kernels/pool_admit.h), for the host mirror's stepped fallback and for llm_pool_schedule.  Host and device compile it.
//
// A pool call runs steps 0, 1, 2 ... of n_cols columns; behind every step comes its tail (every live column draws the token the next
// step evaluates, and stops being live with its last draw) and behind the tail the admission.  After step s and its tail
//   - a column is FREE when its request is not live and was already not live before step s ran: its last drawn token, a stop id
//     included, has then been evaluated, as InferenceSession::infer does;
//   - a column whose request ended in this very tail is not free yet: step s + 1 evaluates its last token;
//   - a request born ended (a budget of one evaluation: its host-drawn first token was a stop id) is free after its first step;
//   - free columns, in ascending index, take the waiting requests in ascending pool index;
//   - the admitted request's first token is evaluated at step s + 1: nothing idles in between.
// The admission keeps one word per column besides the live flag: was_live, the flag as it stood behind the previous admission, i.e.
// before step s ran.
#pragma once

#if defined(__HIPCC__)
#define POOL_FN __host__ __device__ inline
#else
#define POOL_FN inline
#endif

constexpr int POOL_COLS_MAX = 8;     // (BATCH_COLS_MAX)
constexpr int POOL_REQUESTS_MAX = 64;

POOL_FN bool pool_col_free(int live, int was_live) { return !live && !was_live; }
// Which waiting request each column takes behind a tail: take[c] = its pool index, or -1.  Returns the cursor behind the admissions.
POOL_FN int pool_assign(const int *live, const int *was_live, int n_cols, int cursor, int n_pool, int *take) {
    for (int c = 0; c < n_cols; c++) {
        take[c] = -1;
        if (cursor < n_pool && pool_col_free(live[c], was_live[c])) take[c] = cursor++;
    }
    return cursor;
}
// A request of `evals` evaluations draws evals - 1 times; it is live while draws are left.
POOL_FN int pool_draws_of(int evals) { return evals > 1 ? evals - 1 : 0; }

// The rule alone, on evaluation counts (evals[n] >= 1, n >= n_cols, 1 <= n_cols <= POOL_COLS_MAX): request r runs in column col[r]
// from step first_step[r] (either may be null).  Returns the number of steps, the largest first_step + evals.
POOL_FN int pool_schedule(const int *evals, int n, int n_cols, int *col, int *first_step) {
    int live[POOL_COLS_MAX], was_live[POOL_COLS_MAX], left[POOL_COLS_MAX], take[POOL_COLS_MAX];
    int cursor = n_cols, steps = 0;
    for (int c = 0; c < n_cols; c++) {
        left[c] = pool_draws_of(evals[c]);
        live[c] = was_live[c] = left[c] > 0;
        if (col) col[c] = c;
        if (first_step) first_step[c] = 0;
        if (evals[c] > steps) steps = evals[c];
    }
    for (int s = 0;; s++) {
        bool any = cursor < n;
        for (int c = 0; c < n_cols; c++) {  // the tail of step s
            if (live[c] && --left[c] == 0) live[c] = 0;
            any = any || live[c];
        }
        cursor = pool_assign(live, was_live, n_cols, cursor, n, take);
        for (int c = 0; c < n_cols; c++) {
            if (take[c] >= 0) {
                const int r = take[c];
                left[c] = pool_draws_of(evals[r]);
                live[c] = left[c] > 0;
                if (col) col[r] = c;
                if (first_step) first_step[r] = s + 1;
                if (s + 1 + evals[r] > steps) steps = s + 1 + evals[r];
            }
            was_live[c] = live[c];
        }
        if (!any) break;
    }
    return steps;
}
