"""Sanitizer job for the perplexity loop (llm_amd/csrc/host/llm_perplexity.cpp: InferenceSession::perplexity,
crates/llm-base/src/inference_session.rs:519-589): chunking, the BOS replace-and-restore, the window arithmetic and the
indexing of out_probs are host pointer arithmetic of the kind tests/test_sanitize.py exists for.  The loop, llm_host.cpp and
ggml_core.cpp are compiled with g++ -fsanitize=address,undefined and linked against tests/sanitize/stub_backend.cpp plus
tests/sanitize/stub_row_probs.cpp (a host stand-in for ggml_hip_row_probs whose result names the row and the target it was
given); tests/sanitize/perplexity_driver.cpp runs it for n_batch 8, 9, 24, 64 and 100 over a 64-token context.  Any ASan /
UBSan / LeakSanitizer report fails the test.  Runs on the CPU (no GPU, no HIP)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_perplexity_loop_under_asan_and_ubsan(tmp_path):
    from llm_amd import ggml, synth
    exe = tmp_path / "perplexity_driver"
    srcs = ["llm_amd/csrc/ggml_core.cpp", "llm_amd/csrc/host/llm_host.cpp", "llm_amd/csrc/host/llm_perplexity.cpp",
            "tests/sanitize/stub_backend.cpp", "tests/sanitize/stub_row_probs.cpp", "tests/sanitize/perplexity_driver.cpp"]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-Iinclude", "-Illm_amd/csrc", "-pthread"] + srcs + ["-o", str(exe)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    hp0 = dict(n_vocab=256, n_embd=128, n_head=4, n_head_kv=4, n_layer=2, n_rot=32, n_ff=384, n_mult=32)
    hp, w = synth.make_llama(hp0, ggml.TYPE_Q4_0)
    path = tmp_path / "tiny.ggjt"
    synth.write_ggjt(str(path), hp, w)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=600, env=env)
    tail = (r.stdout + r.stderr)[-4000:]
    if r.returncode != 0 and "LeakSanitizer has encountered a fatal error" in tail:  # ptrace-restricted sandbox: leaks unchecked
        env["ASAN_OPTIONS"] = "detect_leaks=0:halt_on_error=1"
        r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=600, env=env)
        tail = (r.stdout + r.stderr)[-4000:]
    assert r.returncode == 0, tail
    assert "perplexity driver OK" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, tail
