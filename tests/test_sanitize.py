"""Sanitizer job for the host C++ of the product (the reference's host side is Rust and gets its memory
safety from the compiler; the C++ restatement gets it from this job).  llm_amd/csrc/ggml_core.cpp (the ggml C API: arenas,
tensor builders, views, graph build / plan, quantizers) and the host mirror llm_amd/csrc/host/llm_{host,file,infer,state,synth}.cpp
(InferenceSession / models/llama, the GGML / GGMF / GGJT reader, snapshots, the greedy sampler) are compiled with
g++ -fsanitize=address,undefined and linked against tests/sanitize/stub_backend.cpp (a host stand-in for the device backend:
nothing is computed), then
tests/sanitize/driver.cpp walks the reference's call sequences — llm::load, two sessions on two threads over one model,
feed_prompt in n_batch chunks, infer_next_token, rewind, K/V out and in, snapshot / from_snapshot, top-k — the ggml wrapper's
context / scratch / view / graph calls, the five quantizers, and feeds the container reader truncated and corrupted copies
of a model file.  Any ASan / UBSan / LeakSanitizer report fails the test.  Runs on the CPU (no GPU, no HIP)."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sanitize_job  # noqa: E402

DRIVER = ["tests/sanitize/driver.cpp"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_host_cpp_under_asan_and_ubsan(tmp_path):
    sanitize_job.build(tmp_path / "sanitize_driver", DRIVER)
    sanitize_job.write_tiny_model(tmp_path / "tiny.ggjt")
    r, tail = sanitize_job.run(tmp_path / "sanitize_driver", [tmp_path / "tiny.ggjt"])
    assert r.returncode == 0, tail
    assert "sanitize driver OK" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, tail


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_host_cpp_under_tsan(tmp_path):
    """The same driver under ThreadSanitizer: its two-sessions-on-two-threads walk (the reference's "several sessions for one
    model on several threads", crates/llm-base/src/inference_session.rs:43-48) must not race in the host C++ — the shared model,
    the process-wide host timers, the ggml arenas of the two sessions."""
    sanitize_job.build(tmp_path / "tsan_driver", DRIVER, flags=sanitize_job.TSAN)
    sanitize_job.write_tiny_model(tmp_path / "tiny.ggjt")
    r, tail = sanitize_job.run_tsan(tmp_path / "tsan_driver", [tmp_path / "tiny.ggjt"])
    assert "WARNING: ThreadSanitizer" not in r.stderr, tail
    assert r.returncode == 0 and "sanitize driver OK" in r.stdout, tail
