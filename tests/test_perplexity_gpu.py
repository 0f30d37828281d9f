"""InferenceSession::perplexity (crates/llm-base/src/inference_session.rs:519-589) with the softmax reduced on the device:
k_row_prob (kernels/nll.h) behind ggml_hip_row_probs, llm_session_perplexity, Session.perplexity.

Expected values are the EXACT form (f64 throughout, tests/perplexity_ref.py).  The allowed relative error of one probability
comes from the kernel's arithmetic, not from a run:

    bound_r = (ceil(V / T) + log2(T) + 4 + |x[r][t] - max_r|) * 2^-24,     T = 1024

The kernel sums in f32: each of its T = 1024 lanes adds its strided share of the row in sequence (ceil(V / T) adds), a tree of
log2(T) = 10 levels joins them (6 inside a wave, 4 across the 16 waves).  Where it loads float4s (aligned rows, V % 4 == 0) a
lane adds 4 * ceil(V / 4096) values, up to 3 more than ceil(V / T), but only for V < 4096, where at most V / 4 < 1024 lanes hold
anything and the tree over them is at least 2 levels shallower: adds + levels stay within the first two terms.  Then 4 roundings for the two expf (the math library's
documented <= 1 ulp each), the subtraction and the division; the last term is the rounding of x_t - max carried through the
exponential.  It is asserted on every row whose target is within 80 of the maximum; targets that are -inf or >= 120 below the
maximum give exactly 0, a row holding a NaN gives NaN; no row is built in between (denormals, the flush mode).
tests/test_perplexity_ref.py shows that the reference's own f32 form passes ITS bound on the same rows."""
import os

import numpy as np
import pytest

import perplexity_ref as R

pytestmark = pytest.mark.gpu

CTX = 64
N_BATCHES = [8, 9, 24, 64]  # prompt chunks of 2-31 tokens; a last batch of ONE token (decode plan); a ragged last batch; one batch


@pytest.mark.parametrize("V,n_rows,row_begin", R.OP_CASES)
def test_row_probs_against_the_exact_softmax(G, V, n_rows, row_begin):
    x, t, kinds = R.op_rows(V, n_rows)
    rng = np.random.default_rng([V, n_rows, 5])
    full = np.concatenate([(3.0 * rng.standard_normal((row_begin, V))).astype(np.float32), x,
                           (3.0 * rng.standard_normal((2 if row_begin else 0, V))).astype(np.float32)])
    with G.Context(full.nbytes * 2 + (4 << 20)) as ctx:
        a = ctx.tensor_from(full, G.TYPE_F32, (V, full.shape[0]))
        y = ctx.op_scale(a, ctx.new_f32(1.0))  # a graph node: its device image is what the hook reads
        ctx.graph().build_forward_expand(y).compute()
        assert np.array_equal(y.device_get().view(np.uint32), full.reshape(-1).view(np.uint32))  # -inf and NaN arrived as they are
        got = G.row_probs(y, t, row_begin)
        worst = R.check_op_rows(x, t, kinds, got, R.bound_device)  # every row
        print(f"V={V} n_rows={n_rows} row_begin={row_begin}: worst error / bound {worst:.3f}")
        # a second call on a sub-range gives the same values (row_begin arithmetic; one workgroup per row, no cross-row state)
        if n_rows >= 8:
            assert np.array_equal(G.row_probs(y, t[5:8], row_begin + 5), got[5:8], equal_nan=True)
        with pytest.raises(ValueError):
            G.row_probs(y, np.full(n_rows, V, np.int32), row_begin)  # a target outside the row: refused, never read
        with pytest.raises(ValueError):
            G.row_probs(y, t, full.shape[0] - n_rows + 1)


@pytest.mark.parametrize("V,pad", [(1000, 24), (32001, 3), (50257, 7)])
def test_row_probs_of_a_view_with_a_padded_row_stride(G, V, pad):
    """The rows of a 2-D view whose stride exceeds its width (nb[1] = (V + pad) * 4, starting `pad` floats into the parent):
    the kernel's stride argument differs from V; what lies between the rows (+1e30 here) must not be read."""
    n_rows = 8
    x, t, kinds = R.op_rows(V, n_rows, seed=pad)
    full = np.full((n_rows + 1, V + pad), np.float32(1e30))
    flat = full.reshape(-1)
    for r in range(n_rows):
        flat[pad + r * (V + pad):pad + r * (V + pad) + V] = x[r]
    with G.Context(full.nbytes * 2 + (4 << 20)) as ctx:
        a = ctx.tensor_from(full, G.TYPE_F32, (V + pad, n_rows + 1))
        y = ctx.op_scale(a, ctx.new_f32(1.0))
        ctx.graph().build_forward_expand(y).compute()
        v = ctx.op_view_2d(y, V, n_rows, (V + pad) * 4, pad * 4)
        assert v.ne[:2] == (V, n_rows) and v.nb[1] == (V + pad) * 4
        got = G.row_probs(v, t)
        worst = R.check_op_rows(x, t, kinds, got, R.bound_device)
        print(f"view V={V} pad={pad}: worst error / bound {worst:.3f}")
        assert np.array_equal(G.row_probs(v, t[2:5], 2), got[2:5], equal_nan=True)


def _tokens(hp):
    return np.random.default_rng(21).integers(0, hp["n_vocab"], 3 * CTX + 5).astype(np.int32)


# Q4_0 and Q8_0.  No K-quant: its blocks are 256 wide and the tiny shape has rows of n_embd = 128 (and n_ff = 352).
WTYPES = [2, 8]


def _exact(model, toks, n_batch):
    """The exact form over the logits Session.evaluate(want_all_logits=True) returns for the same batches on a fresh session
    (seek to 0 per chunk, BOS in place).  Returns (ppl, probs, logits of every chunk [3, CTX, V])."""
    sess = model.start_session(n_batch=n_batch)
    rec = []

    def evaluate(batch):
        rec.append(sess.evaluate(batch, want_all_logits=True))
        return rec[-1]

    ppl, probs = R.perplexity(evaluate, toks, CTX, n_batch, bos=1, form="exact", new_chunk=lambda: sess.seek(0))
    sess.free()
    return ppl, probs, np.concatenate(rec).reshape(3, CTX, -1)


def _bounds(logits, toks, bound):
    """bound_r of every counted position [3, 31] from the logits it was computed from."""
    first, last = R.window(CTX)
    out = np.zeros((3, last - first))
    for i in range(3):
        for j in range(first, last):
            x = logits[i, j]
            out[i, j - first] = bound(x.size, float(x[toks[i * CTX + j + 1]]) - float(x.max()))
    return out


@pytest.mark.parametrize("n_batch", N_BATCHES)
@pytest.mark.parametrize("wtype", WTYPES)
def test_perplexity_on_device_against_the_exact_form(G, wtype, n_batch):
    from llm_amd import llama, synth
    assert synth.TINY["n_embd"] % 256 != 0 and (wtype == G.TYPE_Q4_0 or G.TYPE_NAMES[wtype] == "q8_0")
    hp, w = synth.make_llama(synth.TINY, wtype, seed=31)
    toks = _tokens(hp)
    before = toks.copy()
    model = llama.Llama(hp, w, context_size=CTX)
    try:
        ppl_x, probs_x, logits = _exact(model, toks, n_batch)
        sess = model.start_session(n_batch=n_batch)
        ppl, probs = sess.perplexity(toks, bos=1, on_device=True, return_probs=True)
        host_ppl, host_probs = sess.perplexity(toks, bos=1, on_device=False, return_probs=True)
        assert sess.perplexity(toks[:CTX - 1]) == []
        sess.free()
    finally:
        model.free()
    assert np.array_equal(toks, before)
    assert len(ppl) == 3 and probs.shape == (3, 31) and len(host_ppl) == 3
    b_dev = _bounds(logits, toks, R.bound_device)
    b_seq = _bounds(logits, toks, R.bound_sequential)
    assert np.all(probs_x > 0) and np.all(np.isfinite(probs))
    rel = np.abs(probs.astype(np.float64) - probs_x) / probs_x
    print(f"wtype {wtype} n_batch {n_batch}: worst position error / bound {np.max(rel / b_dev):.3f}; perplexity",
          ppl, "exact", ppl_x, "host", host_ppl)
    assert np.all(rel <= b_dev), (np.argmax(rel / b_dev), np.max(rel / b_dev))
    # chunk i's value is the RUNNING one: f32 running sum of `count` positive terms, logf, the final expf
    for i in range(3):
        count = 31 * (i + 1)
        tol = np.max(b_dev[:i + 1]) + (count + 4) * R.EPS * max(1.0, np.log(ppl_x[i]))
        assert abs(np.log(ppl[i] / ppl_x[i])) <= tol, (i, ppl[i], ppl_x[i], tol)
    assert not np.isclose(ppl[1], np.exp(-np.mean(np.log(probs_x[1]))), rtol=1e-4)  # (a per-chunk value would be this one)
    # on_device=False (the reference's shape) agrees with on_device=True within the sum of the two bounds, position by position
    assert np.all(np.abs(probs.astype(np.float64) - host_probs.astype(np.float64)) <= (b_dev + b_seq) * probs_x)
    for i in range(3):
        tol = np.max(b_seq[:i + 1]) + (31 * (i + 1) + 4) * R.EPS * max(1.0, np.log(ppl_x[i]))
        assert abs(np.log(host_ppl[i] / ppl_x[i])) <= tol


@pytest.mark.parametrize("n", [8, 24, 2])
def test_logits_left_on_the_device_are_the_logits_a_caller_reads(G, n):
    """OutputRequest::logits_on_device changes where the logits live and nothing else: read_node of the device logits after
    evaluate(want_all_logits=False) equals evaluate(want_all_logits=True) bit for bit (both come from the same plan)."""
    from llm_amd import llama, synth
    hp, w = synth.make_llama(synth.TINY, G.TYPE_Q4_0, seed=31)
    toks = _tokens(hp)
    model = llama.Llama(hp, w, context_size=CTX)
    a, b = model.start_session(n_batch=n), model.start_session(n_batch=n)
    try:
        for lo in (0, n, 2 * n):
            want = a.evaluate(toks[lo:lo + n], want_all_logits=True)
            assert b.evaluate(toks[lo:lo + n], want_all_logits=False) is None
            got = b.read_node(-1).reshape(n, -1)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    finally:
        a.free()
        b.free()
        model.free()


@pytest.mark.parametrize("n_batch", [9, 8, 64])
def test_session_state_after_perplexity(G, n_batch):
    """n_past, K/V memory and last_logits are what the evaluate calls of the last chunk leave (bit for bit against a session
    that was given that chunk, BOS in place, in the same batches); token history untouched; the session goes on: rewind(1) +
    evaluate of the removed token (binaries/llm-test/src/delete.rs) gives, bit for bit, what the companion session gives, and
    doing it a second time gives the first result bit for bit (the Delete test as the reference runs it: single-token evaluation
    against single-token evaluation).  Where the last batch of the chunk WAS that one token (n_batch = 9) the result also equals
    last_logits from before, bit for bit.  Where the last batch was a prompt batch (n_batch 8, 64) "the same logits as before"
    cannot hold bit for bit: before, position 63 was computed by the prompt plan's kernels, afterwards by the decode plan's
    ("Perplexity").  The K/V slot is pinned by the bit-for-bit checks above; the comparison with the logits
    from before is only a plausibility check there, at the repository's stated prompt-against-decode tolerance
    (tests/test_llama_gpu.py EDGE)."""
    from llm_amd import llama, synth
    hp, w = synth.make_llama(synth.TINY, G.TYPE_Q4_0, seed=31)
    toks = _tokens(hp)
    model = llama.Llama(hp, w, context_size=CTX)
    sess, ref = model.start_session(n_batch=n_batch), model.start_session(n_batch=n_batch)
    try:
        assert len(sess.perplexity(toks)) == 3
        assert sess.n_past == CTX
        chunk = toks[2 * CTX:3 * CTX].copy()
        chunk[0] = 1
        for lo in range(0, CTX, n_batch):
            ref.evaluate(chunk[lo:lo + n_batch])
        assert ref.n_past == CTX
        last = sess.last_logits()
        assert np.array_equal(last.view(np.uint32), ref.last_logits().view(np.uint32))
        for x, y in zip(sess.get_kv(), ref.get_kv()):
            assert np.array_equal(x, y)
        assert sess.rewind(1) == 0 and ref.rewind(1) == 0 and sess.n_past == CTX - 1
        again = sess.evaluate(chunk[-1:])[0]
        assert np.array_equal(again.view(np.uint32), ref.evaluate(chunk[-1:])[0].view(np.uint32))
        assert sess.n_past == CTX
        assert sess.rewind(1) == 0
        twice = sess.evaluate(chunk[-1:])[0]
        assert np.array_equal(twice.view(np.uint32), again.view(np.uint32))  # L1 == L2
        assert np.array_equal(sess.last_logits().view(np.uint32), again.view(np.uint32))
        for x, y in zip(sess.get_kv(), ref.get_kv()):
            assert np.array_equal(x, y)
        if CTX % n_batch == 1:
            assert np.array_equal(again.view(np.uint32), last.view(np.uint32))
        else:
            assert float(np.max(np.abs(again - last)) / last.std()) < 4e-2
    finally:
        sess.free()
        ref.free()
        model.free()


def test_perplexity_of_a_layer_split_model_is_bit_identical(G):
    """A model split over three virtual device slots (set up and torn down as tests/test_split_gpu.py does) returns the same
    probabilities and perplexities bit for bit as the unsplit one: the logits belong to the last stage, the hook runs on the
    slot that owns them."""
    from llm_amd import llama, synth
    HP = dict(n_vocab=256, n_embd=128, n_head=4, n_head_kv=4, n_layer=5, n_rot=32, n_ff=352, n_mult=32)
    assert G.lib().ggml_hip_get_main_device() == 0
    hp, w = synth.make_llama(HP, 2, seed=17)
    toks = _tokens(hp)

    def run(model):
        out = []
        for n_batch in (24, 9):
            s = model.start_session(n_batch=n_batch)
            out.append(s.perplexity(toks, return_probs=True) + (s.last_logits(), s.n_past))
            s.free()
        return out

    whole = llama.Llama(hp, w, context_size=CTX)
    assert whole.stages() == [(0, 5, 0)]
    ref = run(whole)
    whole.free()
    os.environ["GGML_HIP_VIRTUAL_DEVICES"] = "3"
    try:
        assert G.lib().ggml_hip_device_count() >= 3
        os.environ["GGML_HIP_LAYER_SPLIT"] = "3"
        split = llama.Llama(hp, w, context_size=CTX)
        assert split.stages() == [(0, 2, 0), (2, 3, 1), (3, 5, 2)]
        got = run(split)
        split.free()
    finally:
        os.environ.pop("GGML_HIP_LAYER_SPLIT", None)
        G.lib().ggml_hip_set_layer_split(None, 0)
        G.lib().ggml_hip_set_main_device(0)
        os.environ.pop("GGML_HIP_VIRTUAL_DEVICES", None)
    assert G.lib().ggml_hip_get_main_device() == 0
    for (pa, qa, la, na), (pb, qb, lb, nb) in zip(ref, got):
        assert pa == pb and na == nb == CTX
        assert np.array_equal(qa.view(np.uint32), qb.view(np.uint32)) and np.array_equal(la.view(np.uint32), lb.view(np.uint32))
