#!/usr/bin/env python
"""The chains that stop (Session.infer_until, Llama.infer_until_batch) beside the chains that do not, in tests/tools/sample_chain_ext.py's
protocol: synthetic LLaMA-7B Q4_0, every leg its own session(s) behind the same prompt at about 128 positions, windows of CHAIN_TOKENS
(64) tokens, CHAIN_REPS (7) windows per leg, the legs of a group alternating window by window (the order reversed every other round).
    python tests/tools/chain_requests.py [existing nostop group usecase launch]        (default: all five)
  existing  the unchanged paths: the default and the extended sampled chain and the greedy chain, one session and B = 8.  These legs
            use nothing this tool's tree added, so the same file runs on the parent commit's tree: run the two trees alternately and
            compare each leg with the parent's own min - max spread.
  nostop    the new entries with no stop possible (equal budgets, no stop ids) in the same groups as the existing entries.
  group     the new entries with a stop id that is never drawn, option chain_group = 8, 16, 32, 64, beside the no-stop run.
  usecase   B = 8 sessions with budgets spread over 32 .. 256 and one stop id, in aggregate useful tokens/s: the requests chain, the
            stepped loop under the same rule (option plan_batch_sample = 0) and the existing chain run to the longest budget and
            trimmed; and one session until its stop id against the stepped loop (option plan_sample_chain = 0).
  launch    the kernels between two steps alone, through the hook, at B = 8 and 32000 vocabulary entries with one, two and three
            classes of columns present: microseconds per round, from the difference of a long and a short run.
Reported per leg: the median with min and max and all windows.  Prints one JSON line; env CHAIN_REQ_OUT names a file to write it to
as well (profiles/chain_requests.json was assembled from such files)."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)

DEFAULT = dict(k=40, top_p=0.95, temperature=0.8, penalty=1.30)
EXT = dict(k=40, top_p=0.95, temperature=0.8, penalty=1.30, freq=0.3, presence=0.2, tail_free_z=0.9, typical_p=0.5, min_p=0.2,
           bias=[(0, float("-inf")), (1, -1.5), (7, 3.0), (1000, 2.0), (31999, 2.5)])
MIRO = dict(k=40, top_p=1.0, temperature=0.8, penalty=1.30, mirostat=2, tau=5.0, eta=0.1)
NEVER = 3  # a stop id for the runs that must not stop; a window that draws it anyway is reported short and says so


def summary(v):
    return {"tokens_per_s": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1), "windows": [round(x, 1) for x in v]}


def main():
    what = sys.argv[1:] or ["existing", "nostop", "group", "usecase", "launch"]
    n = int(os.environ.get("CHAIN_TOKENS", "64"))
    reps = int(os.environ.get("CHAIN_REPS", "7"))
    from llm_amd import ggml, llama, synth
    L = ggml.lib()
    new_api = hasattr(llama.Session, "infer_until")
    hp, w = synth.make_llama_fast(synth.LLAMA_7B, ggml.TYPE_Q4_0)
    V = hp["n_vocab"]
    model = llama.Llama(hp, w, context_size=2048)
    out = {"model": "LLaMA-7B Q4_0 (synthetic blocks)", "positions_at_start": 128, "tokens_per_window": n, "windows_per_leg": reps,
           "tree_has_the_requests_chains": new_api, "groups": {}}

    def sessions(B):
        ss = [model.start_session(n_batch=8) for _ in range(B)]
        for c, s in enumerate(ss):
            s.feed_prompt((np.arange(120, dtype=np.int32) * 7 + 5 + c) % V)
        return ss

    def rngs(B):
        return (np.arange(B, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x1234567)).astype(np.uint64)

    def run_group(title, B, legs):
        """legs: {name: f(sessions, rng, k) -> tokens drawn}; every leg on its own sessions and generator states"""
        state = {name: (sessions(B), rngs(B)) for name in legs}
        for name, f in legs.items():
            f(*state[name], 8)
        rates, short = {name: [] for name in legs}, {}
        names = list(legs)
        for r in range(reps):
            for name in (names if r % 2 == 0 else names[::-1]):
                L.ggml_hip_synchronize()
                t0 = time.perf_counter()
                got = legs[name](*state[name], n)
                L.ggml_hip_synchronize()
                rates[name].append(got / (time.perf_counter() - t0))
                if got != n * B:
                    short[name] = short.get(name, 0) + 1
        res = {name: summary(v) for name, v in rates.items()}
        for name, k in short.items():
            res[name]["windows_cut_short_by_the_stop_id"] = k
        out["groups"][title] = res
        print(json.dumps({title: res}), flush=True)
        for ss, _ in state.values():
            for s in ss:
                s.free()

    # ---- the legs
    def one_sampled(kw):
        def f(ss, r, k):
            on_dev, ids = ss[0].infer_tokens_sampled_device(k, r, **kw)
            assert on_dev >= k - 1, "the backend declined the chain"
            return k
        return f

    def one_greedy(ss, r, k):
        ss[0].infer_tokens_device(k)
        return k

    def one_until(kw, stop=(), group=None):
        def f(ss, r, k):
            if group:
                ggml.set_option("chain_group", group)
            ids, count, why, ran = ss[0].infer_until(k, r if kw is not None else None, stop=stop, **(kw or {}))
            return count
        return f

    def batch_sampled(kw):
        def f(ss, r, k):
            ran, ids = model.infer_tokens_sampled_batch(ss, k, r, **kw)
            assert ran, "the backend declined the chain"
            return k * len(ss)
        return f

    def batch_greedy(ss, r, k):
        ran, ids = model.infer_tokens_batch(ss, k)
        assert ran
        return k * len(ss)

    def batch_until(kw, stop=(), group=None):
        def f(ss, r, k):
            if group:
                ggml.set_option("chain_group", group)
            ids, counts, why, ran = model.infer_until_batch(ss, [dict(max_tokens=k, stop=stop, sampler=kw)] * len(ss), r if kw is not None else None)
            assert ran, "the backend declined the chain"
            return int(counts.sum())
        return f

    for B, title in ((1, "one_session"), (8, "eight_sessions")):
        legs = {}
        if "existing" in what:
            legs.update({"sampled_default": (one_sampled if B == 1 else batch_sampled)(DEFAULT),
                         "sampled_extended": (one_sampled if B == 1 else batch_sampled)(EXT), "greedy": one_greedy if B == 1 else batch_greedy})
        if "nostop" in what and new_api:
            u = one_until if B == 1 else batch_until
            legs.update({"until_default_no_stop": u(DEFAULT), "until_extended_no_stop": u(EXT), "until_greedy_no_stop": u(None)})
        if legs:
            run_group(title, B, legs)
        if "group" in what and new_api:
            u = one_until if B == 1 else batch_until
            legs = {"no_stop": u(DEFAULT)}
            legs.update({"chain_group_%d" % gsz: u(DEFAULT, stop=[NEVER], group=gsz) for gsz in (8, 16, 32, 64)})
            run_group(title + "_chain_group", B, legs)
            ggml.set_option("chain_group", 8)

    if "usecase" in what and new_api:
        B, budgets, stop_id = 8, [32, 64, 96, 128, 160, 192, 224, 256], 2
        res = {name: [] for name in ("requests_chain", "stepped_loop_same_rule", "existing_chain_to_256_trimmed")}
        useful = {}
        for r in range(3):
            for name in (list(res) if r % 2 == 0 else list(res)[::-1]):
                ss, rr = sessions(B), rngs(B)
                reqs = [dict(max_tokens=b, stop=[stop_id], sampler=DEFAULT) for b in budgets]
                L.ggml_hip_synchronize()
                t0 = time.perf_counter()
                if name == "existing_chain_to_256_trimmed":
                    ran, ids = model.infer_tokens_sampled_batch(ss, max(budgets), rr, **DEFAULT)
                    got = 0
                    for c, b in enumerate(budgets):  # the caller trims: up to and with the stop id, inside the budget
                        col = ids[:b, c].tolist()
                        got += col.index(stop_id) + 1 if stop_id in col else b
                else:
                    if name == "stepped_loop_same_rule":
                        ggml.set_option("plan_batch_sample", 0)
                    ids, counts, why, ran = model.infer_until_batch(ss, reqs, rr)
                    ggml.set_option("plan_batch_sample", 1)
                    assert ran == (name == "requests_chain")
                    got = int(counts.sum())
                L.ggml_hip_synchronize()
                res[name].append(got / (time.perf_counter() - t0))
                useful[name] = got
                for s in ss:
                    s.free()
        uc = {name: dict(summary(v), useful_tokens=useful[name]) for name, v in res.items()}
        # one session until its stop id: the id of the last draw up to 192 of a free run that is new there
        free = sessions(1)[0]
        rr = rngs(1)
        ids = [free.infer_next_token_sampled(rr, **DEFAULT) for _ in range(193)]
        new = [i for i in range(8, 193) if ids[i] not in ids[:i]]
        assert new, "the free run drew no new id behind its eighth draw"
        j = new[-1]
        free.free()
        one = {"chain": [], "stepped_loop": []}
        for r in range(3):
            for name in (list(one) if r % 2 == 0 else list(one)[::-1]):
                s, rr = sessions(1)[0], rngs(1)
                s.infer_next_token_sampled(rr, **DEFAULT)  # (as the free run began; also arms the chain)
                ggml.set_option("plan_sample_chain", 1 if name == "chain" else 0)
                L.ggml_hip_synchronize()
                t0 = time.perf_counter()
                got, count, why, ran = s.infer_until(256, rr, stop=[ids[j]], **DEFAULT)
                L.ggml_hip_synchronize()
                one[name].append(count / (time.perf_counter() - t0))
                ggml.set_option("plan_sample_chain", 1)
                assert why == "stop" and ran == (name == "chain"), (why, ran, count, j)
                s.free()
        uc["one_session_until_its_stop_id"] = dict({name: summary(v) for name, v in one.items()}, tokens=j)
        out["groups"]["use_case"] = uc
        print(json.dumps({"use_case": uc}), flush=True)

    if "launch" in what and new_api:
        B, Vh = 8, 32000
        rows = np.ascontiguousarray(np.random.default_rng(3).standard_normal((B, Vh)).astype(np.float32) * 3)
        lc = {"default": llama.sampler_chain(**DEFAULT), "extended": llama.sampler_chain(**{**EXT, "bias": [(0, float("-inf")), (1, -1.5)]}),
              "mirostat": llama.sampler_chain(**MIRO)}
        res = {}
        for title, cols in (("one_class", ["default"] * 8), ("two_classes", ["default"] * 4 + ["extended"] * 4),
                            ("three_classes", ["default"] * 3 + ["extended"] * 3 + ["mirostat"] * 2)):
            def run(n_draws):
                cptr = (C.c_void_p * B)(*[C.addressof(lc[c]) for c in cols])
                eptr = (llama.ChainEnd * B)(*[llama.chain_end(n_draws) for _ in range(B)])
                pos, tok = np.arange(8, dtype=np.int32), np.zeros(32, np.int32)
                hist, hist_n = np.zeros((8, 64), np.int32), np.zeros(8, np.int32)
                rr, mu = rngs(8), np.full(8, 10.0, np.float32)
                ids, prm, pos_out = np.zeros((n_draws, B), np.int32), np.zeros(34, np.int32), np.zeros(8, np.int32)
                cnt, why = np.zeros(B, np.int32), np.zeros(B, np.int32)
                t0 = time.perf_counter()
                rc = L.ggml_hip_debug_next_token_req(rows.ctypes.data, B, Vh, cptr, eptr, 0, pos.ctypes.data, tok.ctypes.data, hist.ctypes.data,
                                                     hist_n.ctypes.data, rr.ctypes.data, mu.ctypes.data, n_draws, ids.ctypes.data, prm.ctypes.data,
                                                     pos_out.ctypes.data, cnt.ctypes.data, why.ctypes.data)
                assert rc == 0 and cnt.tolist() == [n_draws] * B
                return time.perf_counter() - t0
            run(50)
            us = [(run(1050) - run(50)) / 1000 * 1e6 for _ in range(5)]
            res[title] = {"us_per_round": round(statistics.median(us), 1), "min": round(min(us), 1), "max": round(max(us), 1)}
        out["groups"]["launch_between_steps_B8_V32000"] = res
        print(json.dumps({"launch": res}), flush=True)

    model.free()
    path = os.environ.get("CHAIN_REQ_OUT")
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
