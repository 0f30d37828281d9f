"""Sanitizer job for the host side of the sampled batched chain (llm_amd/csrc/host/llm_host.cpp: llm_sample_exact,
llm_infer_next_tokens_sampled_batch_via, llm_infer_tokens_sampled_batch_via): the sampler on edge rows and bad arguments, the
argument checks of the two entries, the staging of B graphs and windows for a chain entry that declines, a session whose history is
longer than the 64-token window, and the fall-back loop's indexing of out_ids [n][B].  llm_host.cpp and ggml_core.cpp are compiled
with g++ -fsanitize=address,undefined and linked against tests/sanitize/stub_backend.cpp, which has no batched entries at all;
tests/sanitize/sampler_driver.cpp is the stand-alone program that runs.  Any ASan / UBSan / LeakSanitizer report fails the test.
Runs on the CPU (no GPU, no HIP); nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_sampler_and_its_fall_back_under_asan_and_ubsan(tmp_path):
    from llm_amd import ggml, synth
    exe = tmp_path / "sampler_driver"
    srcs = ["llm_amd/csrc/ggml_core.cpp", "llm_amd/csrc/host/llm_host.cpp", "tests/sanitize/stub_backend.cpp",
            "tests/sanitize/sampler_driver.cpp"]
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
    assert "sampler driver OK" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, tail
