"""What the sanitizer jobs (tests/test_sanitize*.py) share: the host sources of the product, the g++ command that builds a
stand-alone driver from them, the tiny model the drivers load, and the run of the binary.  The jobs run on the CPU (no GPU, no
HIP); nothing is loaded into python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the ggml C API and the host mirror's translation units that link without a device backend (llm_perplexity.cpp and llm_batch.cpp
# call backend hooks the stand-in does not have: a job that wants one names it, with a stand-in for the hook, in its extra sources)
GGML_CORE = "llm_amd/csrc/ggml_core.cpp"
HOST_SRCS = [GGML_CORE] + ["llm_amd/csrc/host/llm_%s.cpp" % u for u in ("host", "file", "infer", "state", "synth")]
STUB_BACKEND = "tests/sanitize/stub_backend.cpp"  # a host stand-in for the device backend: nothing is computed

ASAN_UBSAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
TSAN = ["-fsanitize=thread"]


def build(exe, extra_srcs, flags=ASAN_UBSAN, host_srcs=HOST_SRCS):
    """g++ `flags` over host_srcs, the stand-in backend and extra_srcs (the driver and whatever else the job links) -> exe"""
    cmd = ["g++", "-std=c++17", "-O1", "-g"] + flags + ["-fno-omit-frame-pointer", "-Iinclude", "-Illm_amd/csrc", "-pthread"]
    cmd += list(host_srcs) + [STUB_BACKEND] + list(extra_srcs) + ["-o", str(exe)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]


def write_tiny_model(path):
    """a two-layer LLaMA (Q4_0; n_ff a multiple of 64: the loader's dims[0] % 64 rule for Q4_0 / Q4_1) in the GGJT v3 container"""
    from llm_amd import ggml, synth
    hp0 = dict(n_vocab=256, n_embd=128, n_head=4, n_head_kv=4, n_layer=2, n_rot=32, n_ff=384, n_mult=32)
    hp, w = synth.make_llama(hp0, ggml.TYPE_Q4_0)
    synth.write_ggjt(str(path), hp, w)


def run(exe, args=()):
    """the ASan + UBSan binary, leaks checked where the sandbox lets LeakSanitizer work -> (completed process, tail of its output)"""
    cmd = [str(exe)] + [str(a) for a in args]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    tail = (r.stdout + r.stderr)[-4000:]
    if r.returncode != 0 and "LeakSanitizer has encountered a fatal error" in tail:  # ptrace-restricted sandbox: leaks unchecked
        env["ASAN_OPTIONS"] = "detect_leaks=0:halt_on_error=1"
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
        tail = (r.stdout + r.stderr)[-4000:]
    return r, tail


def run_tsan(exe, args=()):
    """the ThreadSanitizer binary; skips where the runtime cannot work -> (completed process, tail of its output)"""
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=0")
    r = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, timeout=600, env=env)
    tail = (r.stdout + r.stderr)[-4000:]
    if "FATAL: ThreadSanitizer" in tail:  # a sandbox whose memory layout the runtime does not support
        pytest.skip("ThreadSanitizer cannot run here: " + tail.strip().splitlines()[-1])
    return r, tail
