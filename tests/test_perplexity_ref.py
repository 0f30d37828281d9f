"""The premises of the perplexity tests, without a device: what tests/perplexity_ref.py (a numpy restatement of
InferenceSession::perplexity, crates/llm-base/src/inference_session.rs:519-589) does with a recording fake Model::evaluate,
that the reference's own f32 arithmetic stays inside ITS bound of the exact value on the rows the GPU tests feed (so the
reference alone would pass what the device is asked to pass), and the argument checks of ggml_hip_row_probs that need no
device."""
import numpy as np
import pytest

import perplexity_ref as R

CTX, V = 64, 50


class FakeModel:
    """Model::evaluate: records every batch it is given, returns logits that depend on the call and the tokens."""

    def __init__(self):
        self.calls, self.logits, self.chunks = [], [], 0

    def evaluate(self, toks):
        self.calls.append(np.array(toks))
        rng = np.random.default_rng([len(self.calls), int(toks[0]), len(toks)])
        out = (3.0 * rng.standard_normal((len(toks), V))).astype(np.float32)
        self.logits.append(out)
        return out

    def new_chunk(self):
        self.chunks += 1


def _tokens(n, seed=1):
    return np.random.default_rng(seed).integers(2, V, n).astype(np.int32)  # (never 1: the BOS stands out)


@pytest.mark.parametrize("n_batch", [8, 9, 24, 64])
def test_chunk_and_batch_boundaries_bos_targets_and_window(n_batch):
    toks = _tokens(3 * CTX + 5)
    before = toks.copy()
    m = FakeModel()
    ppl, probs = R.perplexity(m.evaluate, toks, CTX, n_batch, bos=1, form="exact", new_chunk=m.new_chunk)
    assert np.array_equal(toks, before)  # the caller's tokens are untouched
    per_chunk = -(-CTX // n_batch)
    assert len(ppl) == 3 and m.chunks == 3 and len(m.calls) == 3 * per_chunk  # 5 tokens beyond the third chunk are ignored
    sizes = [n_batch] * (CTX // n_batch) + ([CTX % n_batch] if CTX % n_batch else [])
    assert {8: [8] * 8, 9: [9] * 7 + [1], 24: [24, 24, 16], 64: [64]}[n_batch] == sizes
    pos = 0
    for c, call in enumerate(m.calls):
        i, j = divmod(c, per_chunk)
        assert len(call) == sizes[j]
        want = before[pos:pos + len(call)].copy()
        if j == 0:
            want[0] = 1  # BOS in place of the chunk's first token, seen by evaluate ...
        assert np.array_equal(call, want), (i, j)  # ... and by no later batch: it was undone
        pos += len(call)
    assert pos == 3 * CTX
    # the window is 32..62, the target of position j the ORIGINAL token j + 1 of the chunk
    assert R.window(CTX) == (32, 63) and probs.shape == (3, 31)
    nll, count = 0.0, 0
    for i in range(3):
        logits = np.concatenate(m.logits[i * per_chunk:(i + 1) * per_chunk])
        for j in range(32, 63):
            x = logits[j].astype(np.float64)
            p = np.exp(x[before[i * CTX + j + 1]] - x.max()) / np.exp(x - x.max()).sum()
            assert probs[i, j - 32] == pytest.approx(p, rel=1e-14)
            nll -= np.log(p)
            count += 1
        assert ppl[i] == pytest.approx(np.exp(nll / count), rel=1e-12)  # nll and count run on across the chunks
    assert count == 93


def test_a_prompt_shorter_than_the_context_gives_no_chunk():
    m = FakeModel()
    ppl, probs = R.perplexity(m.evaluate, _tokens(CTX - 1), CTX, 8, form="f32_sequential", new_chunk=m.new_chunk)
    assert ppl == [] and probs.shape == (0, 31) and m.calls == [] and m.chunks == 0


def test_window_of_a_long_context():
    assert R.window(2048) == (512, 2047) and R.window(1024) == (512, 1023) and R.window(1000) == (500, 999)


@pytest.mark.parametrize("n_batch", [8, 64])
def test_the_f32_form_follows_the_exact_one(n_batch):
    toks = _tokens(2 * CTX)
    a, b = FakeModel(), FakeModel()
    pe, qe = R.perplexity(a.evaluate, toks, CTX, n_batch, form="exact")
    pf, qf = R.perplexity(b.evaluate, toks, CTX, n_batch, form="f32_sequential")
    assert qf.dtype == np.float32 and qe.dtype == np.float64
    per_chunk = len(a.logits) // 2
    worst = 0.0
    for i in range(2):
        logits = np.concatenate(a.logits[i * per_chunk:(i + 1) * per_chunk])
        for k in range(31):
            x = logits[32 + k]
            dt = float(x[toks[i * CTX + 33 + k]]) - float(x.max())
            worst = max(worst, R.bound_sequential(V, dt))
            assert abs(qf[i, k] - qe[i, k]) / qe[i, k] <= R.bound_sequential(V, dt)
        # f32 running sum of `count` positive terms, logf, the final expf
        count = 31 * (i + 1)
        assert abs(np.log(pf[i] / pe[i])) <= worst + (count + 4) * R.EPS * max(1.0, np.log(pe[i]))


@pytest.mark.parametrize("V_,n_rows,row_begin", R.OP_CASES)
def test_the_reference_form_passes_its_bound_on_the_rows_of_the_gpu_test(V_, n_rows, row_begin):
    """util::softmax in f32 with its sequential sum, on the very rows tests/test_perplexity_gpu.py feeds the device: inside
    (V + 3 + |x_t - max|) * 2^-24 of the exact value, 0 and NaN where the device must give 0 and NaN."""
    x, t, kinds = R.op_rows(V_, n_rows)
    if n_rows > 1 and V_ > 1:
        assert set(kinds) == set(R.KINDS8 if n_rows <= 8 else R.KINDS)
    got = np.array([R.prob_f32_sequential(x[r], int(t[r])) for r in range(n_rows)], dtype=np.float32)
    worst = R.check_op_rows(x, t, kinds, got, R.bound_sequential)
    print(f"V={V_} n_rows={n_rows}: worst error / bound of the f32 sequential form {worst:.3f}")
    # the device's bound is not vacuous either: it is far below one unit of the result for every row it applies to
    assert R.bound_device(V_, -80) < 1e-5


def test_row_probs_refuses_bad_arguments_without_a_device(G):
    """ggml_hip_row_probs returns -1 before it touches the device: NULL tensor, n_rows < 1, row_begin < 0, NULL targets /
    out_probs, a tensor that is not F32, rows beyond the tensor, a target outside the row."""
    L = G.lib()
    with G.Context(1 << 20) as ctx:
        x = ctx.tensor_from(np.zeros((4, 16), np.float32), G.TYPE_F32, (16, 4))
        h = ctx.tensor_from(np.zeros((4, 16), np.float16), G.TYPE_F16, (16, 4))
        t = np.zeros(4, np.int32)
        out = np.zeros(4, np.float32)
        tp, op = t.ctypes.data, out.ctypes.data
        assert L.ggml_hip_row_probs(None, 0, 4, tp, op) == -1
        assert L.ggml_hip_row_probs(x.ptr, 0, 0, tp, op) == -1
        assert L.ggml_hip_row_probs(x.ptr, 0, -1, tp, op) == -1
        assert L.ggml_hip_row_probs(x.ptr, -1, 4, tp, op) == -1
        assert L.ggml_hip_row_probs(x.ptr, 0, 4, None, op) == -1
        assert L.ggml_hip_row_probs(x.ptr, 0, 4, tp, None) == -1
        assert L.ggml_hip_row_probs(h.ptr, 0, 4, tp, op) == -1
        assert L.ggml_hip_row_probs(x.ptr, 1, 4, tp, op) == -1  # rows 1..4 of 4
        assert L.ggml_hip_row_probs(x.ptr, 0, 5, tp, op) == -1
        for bad in (-1, 16, 1 << 30):
            t[2] = bad
            assert L.ggml_hip_row_probs(x.ptr, 0, 4, tp, op) == -1
        t[2] = 0
        with pytest.raises(ValueError):
            G.row_probs(x, [0, 0, 0, 0, 0])
        with pytest.raises(ValueError):
            G.row_probs(x, [])
