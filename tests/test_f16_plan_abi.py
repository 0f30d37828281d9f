"""CPU tests of the F16 plan's boundary (no GPU): the test hook ggml_hip_debug_mat_vec_f16 is exported and declared with the
signature the binding has, the option plan_f16 is in the options table with default 1 and is documented, and the synthetic weight
makers give F16 arrays of the right size and type.  Everything that loads the library runs in a child process."""
import json
import os
import re
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child_json(code):
    e = {k: v for k, v in os.environ.items() if not k.startswith("GGML_HIP_")}
    r = subprocess.run([sys.executable, "-c", textwrap.dedent(code)], cwd=ROOT, env=e, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_the_hook_is_exported_with_the_declared_signature():
    got = child_json("""
        import ctypes as C, json
        from llm_amd import ggml
        lib = C.CDLL(ggml.LIB_PATH)
        res, args = ggml.PROTOTYPES["ggml_hip_debug_mat_vec_f16"]
        kres, kargs = ggml.PROTOTYPES["ggml_hip_debug_mat_vec_kbig"]
        print(json.dumps({"symbol": hasattr(lib, "ggml_hip_debug_mat_vec_f16"), "res": res is C.c_int, "n_args": len(args),
                          "like_kbig": list(args[:-1]) == list(kargs) and res is kres, "last": args[-1] is C.c_int}))
    """)
    assert got == {"symbol": True, "res": True, "n_args": 19, "like_kbig": True, "last": True}
    # the header declares the same: ggml_hip_debug_mat_vec_kbig's parameters and one more int
    hdr = open(os.path.join(ROOT, "include", "ggml_hip.h")).read()

    def params(name):
        m = re.search(r"GGML_API int %s\(([^;]*)\);" % name, hdr)
        assert m, name
        return [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    pf, pk = params("ggml_hip_debug_mat_vec_f16"), params("ggml_hip_debug_mat_vec_kbig")
    assert pf[:-1] == pk and pf[-1] == "int ncols"


def test_the_option_is_in_the_table_with_default_1_and_has_an_environment_variable():
    got = child_json("""
        import json
        from llm_amd import ggml
        out = {"default": ggml.get_option("plan_f16")}
        ggml.set_option("plan_f16", 0)
        out["set"] = ggml.get_option("plan_f16")
        print(json.dumps(out))
    """)
    assert got == {"default": 1, "set": 0}
    src = open(os.path.join(ROOT, "llm_amd", "csrc", "backend_state.inc")).read()
    assert re.search(r'\{"plan_f16", &Backend::opt_plan_f16, OPT_ENV \| OPT_DROPS\}', src)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`plan_f16`" in doc


def test_the_synthetic_weight_makers_take_f16():
    got = child_json("""
        import json
        import numpy as np
        from llm_amd import ggml, synth
        out = {}
        for name, make in (("fast", synth.make_llama_fast), ("gaussian", synth.make_llama_gaussian), ("exact", synth.make_llama)):
            hp, w = make(synth.TINY, ggml.TYPE_F16)
            shapes = synth.tensor_shapes(synth.TINY)
            ok = hp["wtype"] == ggml.TYPE_F16 and set(w) == set(shapes)
            for k, (ne0, ne1) in shapes.items():
                a = w[k]
                if ne1 is None:
                    ok = ok and a.dtype == np.float32 and a.size == ne0
                else:
                    v = a.view(np.float16)
                    ok = ok and a.dtype == np.uint8 and a.size == 2 * ne0 * ne1 and bool(np.all(np.isfinite(v)))
                    ok = ok and 0.015 < float(v.astype(np.float64).std()) < 0.025
            out[name] = bool(ok)
        hq, wq = synth.make_llama_fast(synth.TINY, ggml.TYPE_Q4_0)  # the other types are as they were
        out["q4_0"] = wq["output.weight"].size == 256 * 128 // 32 * 18
        print(json.dumps(out))
    """)
    assert got == {"fast": True, "gaussian": True, "exact": True, "q4_0": True}
