"""Sanitizer job for the host K-quant encoders (llm_amd/csrc/ggml_core.cpp: ggml_quantize_q2_K .. q6_K, the K branch of
ggml_quantize_chunk): the fits index 256 values by sub-block and the packings write 84 .. 210-byte blocks field by field,
host pointer arithmetic of the kind tests/test_sanitize.py exists for.  ggml_core.cpp is compiled with
g++ -fsanitize=address,undefined and linked against tests/sanitize/stub_backend.cpp and the stand-alone program
tests/sanitize/kquant_encode_driver.cpp, which encodes every type into heap buffers of the exact size.  Any ASan / UBSan /
LeakSanitizer report fails the test.  Runs on the CPU (no GPU, no HIP); nothing is loaded into python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_k_encoders_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "kquant_encode_driver"
    srcs = ["llm_amd/csrc/ggml_core.cpp", "tests/sanitize/stub_backend.cpp", "tests/sanitize/kquant_encode_driver.cpp"]
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-Iinclude", "-Illm_amd/csrc", "-pthread"] + srcs + ["-o", str(exe)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
    tail = (r.stdout + r.stderr)[-4000:]
    if r.returncode != 0 and "LeakSanitizer has encountered a fatal error" in tail:  # ptrace-restricted sandbox: leaks unchecked
        env["ASAN_OPTIONS"] = "detect_leaks=0:halt_on_error=1"
        r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=env)
        tail = (r.stdout + r.stderr)[-4000:]
    assert r.returncode == 0, tail
    assert "kquant encode driver OK" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, tail
