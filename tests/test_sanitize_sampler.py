"""Sanitizer job for the host side of the sampled batched chain (llm_amd/csrc/host/llm_infer.cpp: llm_sample_exact,
llm_infer_next_tokens_sampled_batch_via, llm_infer_tokens_sampled_batch_via): the sampler on edge rows and bad arguments, the
argument checks of the two entries, the staging of B graphs and windows for a chain entry that declines, a session whose history is
longer than the 64-token window, the fall-back loop's indexing of out_ids [n][B], and the commit after a chain entry that accepts
(B = 2 and 3, n = 1, 2 and 5, out_ids and the generator states of the exact size).  The host mirror and ggml_core.cpp are compiled
with g++ -fsanitize=address,undefined and linked against tests/sanitize/stub_backend.cpp, which has no batched entries at all;
tests/sanitize/sampler_driver.cpp is the stand-alone program that runs.  Any ASan / UBSan / LeakSanitizer report fails the test.
Runs on the CPU (no GPU, no HIP); nothing is loaded into python."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sanitize_job  # noqa: E402


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_sampler_and_its_fall_back_under_asan_and_ubsan(tmp_path):
    sanitize_job.build(tmp_path / "sampler_driver", ["tests/sanitize/sampler_driver.cpp"])
    sanitize_job.write_tiny_model(tmp_path / "tiny.ggjt")
    r, tail = sanitize_job.run(tmp_path / "sampler_driver", [tmp_path / "tiny.ggjt"])
    assert r.returncode == 0, tail
    assert "sampler driver OK" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, tail
