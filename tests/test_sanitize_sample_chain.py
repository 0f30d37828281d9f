"""Sanitizer job for the host side of one session's sampled chain (llm_amd/csrc/host/llm_infer.cpp: llm_infer_next_token_sampled,
llm_infer_tokens_sampled_via): the two attempts with a NULL entry, an entry that declines and an entry that accepts and fills ids,
generator state and logits; histories longer and shorter than the 64-token window; n = 1, 2 and 5 with `out` of the exact size; bad
arguments.  The host mirror and ggml_core.cpp are compiled with g++ -fsanitize=address,undefined and linked against
tests/sanitize/stub_backend.cpp, which has no ggml_hip_decode_sampled_chain; tests/sanitize/sample_chain_driver.cpp is the
stand-alone program that runs.  Any ASan / UBSan / LeakSanitizer report fails the test.  Runs on the CPU (no GPU, no HIP); nothing
is loaded into python."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sanitize_job  # noqa: E402


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_the_sampled_chain_and_its_stepped_loop_under_asan_and_ubsan(tmp_path):
    sanitize_job.build(tmp_path / "sample_chain_driver", ["tests/sanitize/sample_chain_driver.cpp"])
    sanitize_job.write_tiny_model(tmp_path / "tiny.ggjt")
    r, tail = sanitize_job.run(tmp_path / "sample_chain_driver", [tmp_path / "tiny.ggjt"])
    assert r.returncode == 0, tail
    assert "sample chain driver OK" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, tail
