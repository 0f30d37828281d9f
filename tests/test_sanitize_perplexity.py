"""Sanitizer job for the perplexity loop (llm_amd/csrc/host/llm_perplexity.cpp: InferenceSession::perplexity,
crates/llm-base/src/inference_session.rs:519-589): chunking, the BOS replace-and-restore, the window arithmetic and the
indexing of out_probs are host pointer arithmetic of the kind tests/test_sanitize.py exists for.  The loop, the host mirror and
ggml_core.cpp are compiled with g++ -fsanitize=address,undefined and linked against tests/sanitize/stub_backend.cpp plus
tests/sanitize/stub_row_probs.cpp (a host stand-in for ggml_hip_row_probs whose result names the row and the target it was
given); tests/sanitize/perplexity_driver.cpp runs it for n_batch 8, 9, 24, 64 and 100 over a 64-token context.  Any ASan /
UBSan / LeakSanitizer report fails the test.  Runs on the CPU (no GPU, no HIP)."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sanitize_job  # noqa: E402


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_perplexity_loop_under_asan_and_ubsan(tmp_path):
    sanitize_job.build(tmp_path / "perplexity_driver", ["llm_amd/csrc/host/llm_perplexity.cpp", "tests/sanitize/stub_row_probs.cpp",
                                                        "tests/sanitize/perplexity_driver.cpp"])
    sanitize_job.write_tiny_model(tmp_path / "tiny.ggjt")
    r, tail = sanitize_job.run(tmp_path / "perplexity_driver", [tmp_path / "tiny.ggjt"])
    assert r.returncode == 0, tail
    assert "perplexity driver OK" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, tail
