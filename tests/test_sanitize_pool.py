"""Sanitizer job for the host side of the request pool (llm_amd/csrc/host/llm_infer.cpp: llm_infer_until_pool_via, llm_pool_schedule):
its argument checks (nothing moved, generator states untouched), the staging of the pool's graphs, the stepped loop under the
admission rule of kernels/pool_rule.h — without an entry and with one that declines — and the commit behind fake entries that accept
without computing: one that runs every request to its end and one that stops short of n_steps, so that the mirror calls again for what
is unfinished or unstarted and sends a lone remainder through llm_infer_until_via.  Checked against each session's ids, position and
token history.  The host mirror and ggml_core.cpp are compiled with g++ -fsanitize=address,undefined and linked against
tests/sanitize/stub_backend.cpp, which has no pool entry — the reason the entries are parameters; tests/sanitize/pool_driver.cpp is
the stand-alone program that runs.  Any ASan / UBSan / LeakSanitizer report fails the test.  Runs on the CPU (no GPU, no HIP); nothing
is loaded into python."""
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sanitize_job  # noqa: E402


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_the_pool_mirror_under_asan_and_ubsan(tmp_path):
    sanitize_job.build(tmp_path / "pool_driver", ["tests/sanitize/pool_driver.cpp"])
    sanitize_job.write_tiny_model(tmp_path / "tiny.ggjt")
    r, tail = sanitize_job.run(tmp_path / "pool_driver", [tmp_path / "tiny.ggjt"])
    assert r.returncode == 0, tail
    assert "pool driver OK" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, tail
