"""The request pool (ggml_hip_decode_pool_requests, Llama.infer_until_pool): more requests than the batched step has columns; a column
whose request has ended takes the next waiting request on the device, between two replays of the same captured step.

Every comparison is equality.  k_pool_admit alone, one launch through the hook ggml_hip_debug_pool_admit on tables filled with
sentinels, against a restatement of the admission rule (kernels/pool_rule.h) written here on the same words: every word of every
table, the retire slots included.  The pool against twins that run each session ALONE through the existing stepped entries (ids,
counts, reasons, generator states, the bits of mu, n_past, Session.snapshot() byte for byte), against infer_until_batch where there
are as many requests as columns, across a step cap that makes the mirror call the entry twice, and with the option off."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_ref as R  # noqa: E402
from test_chain_requests_gpu import CTX, _config, _first_new, _mk, _seed, _stats, _step, _stepped_until  # noqa: E402

pytestmark = pytest.mark.gpu

COLS, POOL, WIN, NBIAS, NSTOP, CLASSES = 8, 64, 64, 64, 8, 4
DEFAULT_CLS, FULL_CLS, MIRO_CLS, GREEDY_CLS = 0, 1, 2, 3


# ---- the device tables, word for word (kernels/decode.h, kernels/sample.h, kernels/pool_admit.h) ----
class DecParams(C.Structure):
    _fields_ = [("n_past", C.c_int32), ("token", C.c_int32), ("store_at", C.c_int32), ("pad1", C.c_int32), ("tokens", C.c_int32 * 32),
                ("pos_tail", C.c_int32 * 2)]


class BatchCols(C.Structure):
    _fields_ = [("pos", C.c_int32 * COLS), ("mem_k", C.c_uint64 * COLS), ("mem_v", C.c_uint64 * COLS)]


class SampleCols(C.Structure):
    _fields_ = [("hist", (C.c_int32 * WIN) * COLS), ("hist_n", C.c_int32 * COLS), ("params", C.c_int32 * 13)]


class ReqParams(C.Structure):
    _fields_ = [("w", C.c_int32 * 13)]


class Bias(C.Structure):
    _fields_ = [("id", C.c_int32 * NBIAS), ("b", C.c_float * NBIAS)]


class ReqBack(C.Structure):
    _fields_ = [("rng", C.c_uint64 * COLS), ("mu", C.c_float * COLS), ("n_drawn", C.c_int32 * COLS), ("ended_by", C.c_int32 * COLS),
                ("live", C.c_int32 * COLS)]


class SampleReqs(C.Structure):
    _fields_ = [("back", ReqBack), ("max_draws", C.c_int32 * COLS), ("n_stop", C.c_int32 * COLS), ("stop_id", (C.c_int32 * NSTOP) * COLS),
                ("n_list", C.c_int32 * CLASSES), ("list", (C.c_int32 * COLS) * CLASSES), ("prm", ReqParams * COLS), ("bias", Bias * COLS)]


class PoolIn(C.Structure):
    _fields_ = [("mem_k", C.c_uint64), ("mem_v", C.c_uint64), ("rng", C.c_uint64), ("mu", C.c_float), ("token", C.c_int32), ("pos", C.c_int32),
                ("hist_n", C.c_int32), ("max_draws", C.c_int32), ("n_stop", C.c_int32), ("cls", C.c_int32), ("stop_id", C.c_int32 * NSTOP),
                ("hist", C.c_int32 * WIN), ("prm", ReqParams), ("bias", Bias)]


class PoolOut(C.Structure):
    _fields_ = [("rng", C.c_uint64), ("mu", C.c_float), ("n_drawn", C.c_int32), ("ended_by", C.c_int32), ("col", C.c_int32),
                ("first_step", C.c_int32), ("retired", C.c_int32), ("pad", C.c_int32)]


class PoolHead(C.Structure):
    _fields_ = [("cursor", C.c_int32), ("n_pool", C.c_int32), ("n_cols", C.c_int32), ("step", C.c_int32), ("busy", C.c_int32), ("pad", C.c_int32),
                ("owner", C.c_int32 * COLS), ("was_live", C.c_int32 * COLS)]


class PoolTable(C.Structure):
    _fields_ = [("head", PoolHead), ("out", PoolOut * POOL), ("in_", PoolIn * POOL)]


TABLES = (PoolTable, SampleReqs, SampleCols, DecParams, BatchCols)


def _sentinels(obj, seed):
    """Every word of a table gets a value of its own (small positive ints: also valid floats), so that a word the launch should not
    have touched, or took from the wrong place, shows."""
    n = C.sizeof(obj) // 4
    words = (np.arange(n, dtype=np.uint32) * np.uint32(7) + np.uint32(seed * 1000003 + 11)) % np.uint32(1 << 20) + np.uint32(1 << 20)
    C.memmove(C.addressof(obj), words.ctypes.data, n * 4)


def _bytes(obj):
    return bytes((C.c_char * C.sizeof(obj)).from_address(C.addressof(obj)))


def _clone(obj):
    c = type(obj)()
    C.memmove(C.addressof(c), C.addressof(obj), C.sizeof(obj))
    return c


def _admit_ref(t, rq, sc, prm, bc, logits, emb, slot_l, slot_e):
    """The rule restated on the tables (in place).  After the tail of a step: column c is free when its request is not live and was
    not live before the step; free columns in ascending order take waiting requests in ascending pool order.  A column that changes
    hands first retires its request (rows into that request's slot; counts, reason, generator, mu into its back record), then takes
    everything the new request staged.  The lists of all four classes are rebuilt when anybody was admitted.  Every launch: was_live
    becomes live, step counts up, busy says whether a column is live or a request waits."""
    B, P = t.head.n_cols, t.head.n_pool
    free = [c for c in range(B) if not rq.back.live[c] and not t.head.was_live[c]]
    admitted = False
    for c in free:
        if t.head.cursor >= P:
            break
        r, o = t.head.cursor, t.head.owner[c]
        t.head.cursor += 1
        admitted = True
        if 0 <= o < P:
            slot_l[o], slot_e[o] = logits[c], emb[c]
            b = t.out[o]
            b.rng, b.mu, b.n_drawn, b.ended_by, b.retired = rq.back.rng[c], rq.back.mu[c], rq.back.n_drawn[c], rq.back.ended_by[c], 1
        i = t.in_[r]
        prm.tokens[c], bc.pos[c], bc.mem_k[c], bc.mem_v[c] = i.token, i.pos, i.mem_k, i.mem_v
        if c == 0:
            prm.token, prm.n_past = i.token, i.pos
        for j in range(WIN):
            sc.hist[c][j] = i.hist[j]
        sc.hist_n[c] = i.hist_n
        C.memmove(C.addressof(rq.prm[c]), C.addressof(i.prm), C.sizeof(ReqParams))
        C.memmove(C.addressof(rq.bias[c]), C.addressof(i.bias), C.sizeof(Bias))
        rq.n_stop[c], rq.max_draws[c] = i.n_stop, i.max_draws
        for j in range(NSTOP):
            rq.stop_id[c][j] = i.stop_id[j]
        rq.back.rng[c], rq.back.mu[c], rq.back.n_drawn[c] = i.rng, i.mu, 0
        rq.back.live[c] = int(i.max_draws > 0)
        rq.back.ended_by[c] = 0 if i.max_draws > 0 else 1
        t.head.owner[c] = r
        t.out[r].col, t.out[r].first_step = c, t.head.step + 1
    if admitted:
        counts = [0] * CLASSES
        for c in range(B):
            cls = t.in_[t.head.owner[c]].cls
            rq.list[cls][counts[cls]] = c
            counts[cls] += 1
        for s in range(CLASSES):
            rq.n_list[s] = counts[s]
    for c in range(B):
        t.head.was_live[c] = rq.back.live[c]
    t.head.step += 1
    t.head.busy = int(t.head.cursor < P or any(rq.back.live[c] for c in range(B)))


def _launch(G, B, P, live, was_live, cursor, owners, classes, max_draws=None, V=41, E=9, seed=1):
    """One launch on sentinel tables with the given flags, against the restatement: every word of every table and slot."""
    sizes = (C.c_int64 * 5)()
    G.lib().ggml_hip_debug_pool_admit_sizes(sizes)
    assert [int(s) for s in sizes] == [C.sizeof(T) for T in TABLES]
    t, rq, sc, prm, bc = (T() for T in TABLES)
    for k, obj in enumerate((t, rq, sc, prm, bc)):
        _sentinels(obj, seed * 10 + k)
    t.head.cursor, t.head.n_pool, t.head.n_cols, t.head.step = cursor, P, B, 17
    for c in range(COLS):
        t.head.owner[c] = owners[c] if c < B else -1
    for c in range(B):
        rq.back.live[c], t.head.was_live[c] = live[c], was_live[c]
    for r in range(POOL):
        t.in_[r].cls = classes[r] if r < P else 0
        if max_draws is not None and r < P:
            t.in_[r].max_draws = max_draws[r]
    g = np.random.default_rng([seed, V])
    logits, emb = g.standard_normal((B, V)).astype(np.float32), g.standard_normal((B, E)).astype(np.float32)
    slot_l, slot_e = g.standard_normal((P, V)).astype(np.float32), g.standard_normal((P, E)).astype(np.float32)
    want = [_clone(o) for o in (t, rq, sc, prm, bc)]
    want_l, want_e = slot_l.copy(), slot_e.copy()
    _admit_ref(*want, logits, emb, want_l, want_e)
    rc = G.lib().ggml_hip_debug_pool_admit(C.addressof(t), C.addressof(rq), C.addressof(sc), C.addressof(prm), C.addressof(bc), sizes, B, P,
                                           logits.ctypes.data, emb.ctypes.data, V, E, slot_l.ctypes.data, slot_e.ctypes.data)
    assert rc == 0
    for name, got, exp in zip(("PoolTable", "SampleReqs", "SampleCols", "DecParams", "BatchCols"), (t, rq, sc, prm, bc), want):
        a, b = np.frombuffer(_bytes(got), np.uint32), np.frombuffer(_bytes(exp), np.uint32)
        assert np.array_equal(a, b), (name, np.flatnonzero(a != b)[:16].tolist())
    assert np.array_equal(slot_l.view(np.uint32), want_l.view(np.uint32)) and np.array_equal(slot_e.view(np.uint32), want_e.view(np.uint32))
    return t, rq, prm, bc


GREEDY6 = [GREEDY_CLS] * 7


def test_nothing_is_free_and_nothing_moves(G):
    t, rq, _, _ = _launch(G, 3, 6, [1, 1, 1], [1, 1, 1], 3, [0, 1, 2], GREEDY6)
    assert t.head.cursor == 3 and t.head.step == 18 and t.head.busy == 1 and list(t.head.owner)[:3] == [0, 1, 2]


def test_a_column_that_ended_in_this_tail_is_not_free_yet(G):
    t, rq, _, _ = _launch(G, 3, 6, [1, 0, 1], [1, 1, 1], 3, [0, 1, 2], GREEDY6, seed=2)
    assert t.head.cursor == 3 and list(t.head.owner)[:3] == [0, 1, 2] and list(t.head.was_live)[:3] == [1, 0, 1]
    assert t.out[1].retired != 1


def test_one_free_column_takes_the_one_waiting_request(G):
    t, rq, _, _ = _launch(G, 3, 4, [1, 0, 1], [1, 0, 1], 3, [0, 1, 2], GREEDY6, max_draws=[4, 4, 4, 5, 0, 0, 0], seed=3)
    assert t.head.cursor == 4 and list(t.head.owner)[:3] == [0, 3, 2] and t.out[1].retired == 1
    assert (t.out[3].col, t.out[3].first_step) == (1, 18) and rq.back.live[1] == 1 and rq.max_draws[1] == 5


def test_columns_0_and_2_free_take_the_pool_in_order_and_column_0_keeps_token_and_n_past(G):
    t, rq, prm, bc = _launch(G, 3, 7, [0, 1, 0], [0, 1, 0], 4, [0, 1, 3], GREEDY6, max_draws=[1, 1, 1, 1, 3, 0, 2], seed=4)
    assert t.head.cursor == 6 and list(t.head.owner)[:3] == [4, 1, 5] and t.head.busy == 1
    assert (prm.token, prm.n_past) == (t.in_[4].token, t.in_[4].pos) == (prm.tokens[0], bc.pos[0])
    assert rq.back.live[0] == 1 and rq.back.live[2] == 0 and rq.back.ended_by[2] == 1  # request 5 is born ended
    assert list(t.head.was_live)[:3] == [1, 1, 0]


def test_two_free_columns_and_one_waiting_request_the_lower_column_gets_it(G):
    t, rq, _, _ = _launch(G, 4, 5, [1, 0, 0, 0], [1, 0, 1, 0], 4, [0, 1, 2, 3], GREEDY6, max_draws=[1, 1, 1, 1, 2, 0, 0], seed=5)
    assert t.head.cursor == 5 and list(t.head.owner)[:4] == [0, 4, 2, 3] and t.out[3].retired != 1 and t.out[2].retired != 1


def test_an_admitted_class_no_column_had_rebuilds_the_lists(G):
    classes = [GREEDY_CLS, FULL_CLS, MIRO_CLS, DEFAULT_CLS, DEFAULT_CLS, GREEDY_CLS, GREEDY_CLS]
    t, rq, _, _ = _launch(G, 3, 6, [0, 1, 0], [0, 1, 0], 3, [0, 1, 2], classes, max_draws=[1, 1, 1, 2, 2, 2, 0], seed=6)
    assert list(rq.n_list) == [2, 1, 0, 0] and list(rq.list[DEFAULT_CLS])[:2] == [0, 2] and rq.list[FULL_CLS][0] == 1


@pytest.mark.parametrize("V", [41, R.CAP + 1])
def test_the_retire_slots_hold_the_rows_of_the_retired_requests(G, V):
    """Both sizes of row: below one pass of the 1024 threads and beyond the on-chip selection's cap; E is no multiple of anything."""
    t, _, _, _ = _launch(G, 3, 6, [0, 0, 1], [0, 0, 1], 3, [2, 0, 1], GREEDY6, max_draws=[1, 1, 1, 2, 2, 2, 0], V=V, E=1031, seed=7)
    assert t.out[2].retired == 1 and t.out[0].retired == 1 and t.out[1].retired != 1


# ---- the pool against twins stepped alone ----
SIX = (("greedy", 8, 8, None),             # the first maximum, all eight
       ("truncating", 2, 8, ("new", 1, 5)),  # stops on a stop id found by a free run
       ("mirostat", 5, 2, None),           # Mirostat 2 with a budget of 2
       ("default", 4, 8, ("at", 0)),       # its first token is its stop id: born ended
       ("truncating", 61, 8, None),        # room for two draws only: ends on the context
       ("default", 6, 5, None))            # the default class: no column has it until this one enters
_twins = {}


def _prompts(cfg, plan, V):
    g = np.random.default_rng([cfg == "tiny", len(plan), 77])
    return [g.integers(0, V, p[1]).astype(np.int32) for p in plan]


def _want(G, O, cfg, plan):
    """Per request of the plan: (stop ids, ids, reason, (rng, mu bits), n_past, snapshot) of a twin stepped ALONE; computed once."""
    key = (cfg, plan)
    if key in _twins:
        return _twins[key]
    hp, model = _mk(G, O, cfg)
    V = hp["n_vocab"]
    out = []
    try:
        G.set_option("plan_batch_k", 1)
        for c, (p, prompt) in enumerate(zip(plan, _prompts(cfg, plan, V))):
            kw, mu0 = _config(p[0], V)
            stop = []
            if p[3] is not None:
                s = model.start_session(n_batch=8)
                s.feed_prompt(prompt)
                rng, mu = (None if kw is None else _seed(c)), (None if mu0 is None else np.array([mu0], np.float32))
                ids = [_step(s, kw, rng, mu) for _ in range(min(p[2], CTX - 1 - s.n_past))]
                stop = [ids[_first_new(ids, p[3][1], p[3][2])]] if p[3][0] == "new" else [ids[p[3][1]]]
                s.free()
            s = model.start_session(n_batch=8)
            s.feed_prompt(prompt)
            rng, mu = (None if kw is None else _seed(c)), (None if mu0 is None else np.array([mu0], np.float32))
            ids, why = _stepped_until(s, kw, rng, mu, p[2], stop)
            state = (None if kw is None else int(rng[0]), None if mu0 is None else int(mu.view(np.uint32)[0]))
            out.append((stop, ids, why, state, s.n_past, s.snapshot()))
            s.free()
    finally:
        G.set_option("plan_batch_k", 0)
    model.free()
    _twins[key] = out
    return out


POOL_COUNTERS = ("pool_calls", "pool_admitted", "pool_steps", "batch_decode_steps", "chain_steps_cut", "chain_frozen_steps", "chain_stopped_columns",
                 "batch_sample_steps", "batch_chain_steps", "plan_tokens")


def _pool(G, O, cfg, plan, max_cols, group=8, cap=None, options=(), batch=False):
    """The plan's sessions through infer_until_pool (batch: infer_until_batch), compared with the twins; returns (ran, movements)."""
    from llm_amd import llama
    want = _want(G, O, cfg, plan)
    hp, model = _mk(G, O, cfg)
    V, N = hp["n_vocab"], len(plan)
    cfgs = [_config(p[0], V) for p in plan]
    sessions = []
    try:
        G.set_option("plan_batch_k", 1)
        G.set_option("chain_group", group)
        for k, v in options:
            G.set_option(k, v)
        if cap is not None:
            llama._lib().llm_pool_step_cap(cap)
        sessions = [model.start_session(n_batch=8) for _ in range(N)]
        for s, pr in zip(sessions, _prompts(cfg, plan, V)):
            s.feed_prompt(pr)
        rngs = np.array([int(_seed(c)[0]) for c in range(N)], np.uint64)
        mus = np.array([6.0 if m is None else m for _, m in cfgs], np.float32)
        reqs = [dict(max_tokens=p[2], stop=want[c][0], sampler=cfgs[c][0]) for c, p in enumerate(plan)]
        s0 = _stats(G, POOL_COUNTERS)
        if batch:
            grid, counts, reasons, ran = model.infer_until_batch(sessions, reqs, rngs, mu=mus)
            ids = [grid[:counts[c], c] for c in range(N)]
        else:
            ids, counts, reasons, ran = model.infer_until_pool(sessions, reqs, rngs, mu=mus, max_cols=max_cols)
        moved = dict(zip(POOL_COUNTERS, [b - a for a, b in zip(s0, _stats(G, POOL_COUNTERS))]))
        for c in range(N):
            _, w_ids, w_why, w_state, w_past, w_snap = want[c]
            assert list(ids[c]) == w_ids and int(counts[c]) == len(w_ids) and reasons[c] == w_why, (c, list(ids[c]), w_ids, reasons[c], w_why)
            kw, mu0 = cfgs[c]
            got_state = (None if kw is None else int(rngs[c]), None if mu0 is None else int(mus[c:c + 1].view(np.uint32)[0]))
            assert got_state == w_state, (c, got_state, w_state)
            assert sessions[c].n_past == w_past, (c, sessions[c].n_past, w_past)
            assert sessions[c].snapshot() == w_snap, c
    finally:
        G.set_option("plan_batch_k", 0)
        G.set_option("chain_group", 8)
        for k, _ in options:
            G.set_option(k, 1)
        llama._lib().llm_pool_step_cap(4096)
        for s in sessions:
            s.free()
        model.free()
    return ran, moved, [len(w[1]) for w in want]


def _schedule(evals, n_cols):
    from llm_amd import llama
    e = np.ascontiguousarray(evals, np.int32)
    return llama._lib().llm_pool_schedule(e.ctypes.data, len(e), n_cols, None, None)


@pytest.mark.parametrize("cfg", ["tiny", "q4_k", "f16"])
def test_six_requests_over_three_columns_equal_each_session_alone(G, O, cfg):
    ran, moved, lens = _pool(G, O, cfg, SIX, 3)
    assert ran is True and lens[0] == 8 and lens[2] == 2 and lens[3] == 1 and lens[4] == 2 and lens[5] == 5 and 2 <= lens[1] <= 6, lens
    assert moved["pool_calls"] == 1 and moved["pool_admitted"] == 3, moved


def test_as_many_requests_as_columns_is_the_batched_chain_counters_included(G, O):
    plan = SIX[:3]
    _, pool, _ = _pool(G, O, "tiny", plan, 3, group=4)
    ran, batch, _ = _pool(G, O, "tiny", plan, 3, group=4, batch=True)
    assert ran is True and pool["pool_calls"] == 1 and pool["pool_admitted"] == 0
    for k in POOL_COUNTERS[3:]:
        assert pool[k] == batch[k], (k, pool, batch)


def test_the_steps_are_the_schedule_and_steps_behind_the_end_are_never_launched(G, O):
    """Groups of one step: the host sees the end one group late.  pool_steps is the call's steps_run: the schedule of the
    evaluations the requests took.  The budgets' schedule is what the mirror asked for; the rest was never launched."""
    ran, moved, lens = _pool(G, O, "tiny", SIX, 3, group=1)
    steps, asked = _schedule(lens, 3), _schedule([1 if i == 3 else min(p[2], 2 if i == 4 else 99) for i, p in enumerate(SIX)], 3)
    assert ran is True and moved["pool_steps"] == steps and moved["pool_admitted"] == len(SIX) - 3, (moved, steps)
    launched = min(asked, steps + 1)
    assert moved["batch_decode_steps"] == launched and moved["chain_steps_cut"] == asked - launched, (moved, steps, asked)
    assert moved["chain_frozen_steps"] == 3 * launched - sum(lens), (moved, lens)
    assert moved["chain_stopped_columns"] == 1, moved  # (the born-ended request's stop id was drawn by the host)


def test_a_step_cap_ends_the_first_call_mid_request_and_the_second_call_finishes_it(G, O):
    ran, moved, lens = _pool(G, O, "tiny", SIX, 3, cap=3)
    assert ran is True and moved["pool_calls"] >= 2, moved


@pytest.mark.parametrize("option", ["plan_batch_pool", "plan_batch_sample"])
def test_with_the_option_off_the_stepped_loop_gives_the_same_results(G, O, option):
    """The entry declines (nothing executed, no state moved: the stepped loop starts from untouched sessions and states, or its results
    would differ from the twins') and the stepped loop runs under the same admission rule."""
    ran, moved, _ = _pool(G, O, "tiny", SIX, 3, options=((option, 0),))
    assert ran is False and moved["pool_calls"] == 0 and moved["pool_admitted"] == 0 and moved["batch_sample_steps"] == 0, moved
