"""CPU tests of the LoRA adapter container (ggla, crates/ggml/src/format/loader.rs:160-209 and lora.rs:28-52) through the
library's C++ reader, of the adapter bookkeeping of crates/llm-base/src/loader.rs:494-528 (tensors_to_patch, scaling),
and of llm_llama_load_lora's LoadError path (nothing here reaches the device)."""
import ctypes as C
import struct

import numpy as np
import pytest

from llm_amd import ggml as G
from llm_amd import llama, lora, synth


def _adapter(rng):
    return {
        "layers.0.attention.wq.weight.loraA": rng.standard_normal((128, 8)).astype(np.float16),
        "layers.0.attention.wq.weight.loraB": rng.standard_normal((128, 8)).astype(np.float32),
        "layers.1.feed_forward.w2.weight.loraA": rng.standard_normal((352, 8)).astype(np.float32),
        "layers.1.feed_forward.w2.weight.loraB": rng.standard_normal((128, 8)).astype(np.float32),
    }


def test_ggla_round_trip(tmp_path):
    ts = _adapter(np.random.default_rng(1))
    path = tmp_path / "a.ggla"
    synth.write_ggla(path, 8, 16, ts)
    info = llama.inspect_file(path)
    assert info is not None
    assert (info["container"], info["version"]) == (3, 1)
    hp = info["hp"]
    assert [getattr(hp, f) for f, _ in hp._fields_] == [0] * 8  # no LLaMA hyperparameters in a ggla file
    assert info["vocab"] == []
    assert [t["name"] for t in info["tensors"]] == list(ts)
    for t, (name, arr) in zip(info["tensors"], ts.items()):
        assert t["type"] == (G.TYPE_F16 if arr.dtype == np.float16 else G.TYPE_F32)
        assert t["n_dims"] == 2 and t["ne"] == (arr.shape[1], arr.shape[0])
        assert t["offset_mod32"] == 0
        assert t["head"] == arr.tobytes()[:16]
    ad = lora.read_adapter(path)
    assert (ad["r"], ad["alpha"]) == (8, 16)
    for name, arr in ts.items():
        assert ad["tensors"][name].dtype == arr.dtype and np.array_equal(ad["tensors"][name], arr)


def test_ggla_other_versions_rejected(tmp_path):
    ts = _adapter(np.random.default_rng(2))
    for v in (0, 2):
        path = tmp_path / f"v{v}.ggla"
        synth.write_ggla(path, 8, 16, ts, version=v)
        assert llama.inspect_file(path) is None
        with pytest.raises(ValueError):
            lora.read_adapter(path)


def test_lora_query_is_ggla_only(tmp_path):
    hp, w = synth.make_llama(synth.TINY, G.TYPE_Q8_0)  # (TINY's n_ff breaks the dims[0] % 64 rule of Q4_0 files)
    path = tmp_path / "m.bin"
    synth.write_ggjt(path, hp, w)
    with pytest.raises(ValueError, match="not a ggla"):
        lora.read_adapter(path)
    info = llama.inspect_file(path)
    assert info["container"] == 2 and info["hp"].n_embd == hp["n_embd"]


def test_tensors_to_patch_and_scaling():
    names = ["layers.0.attention.wq.weight.loraA", "layers.0.attention.wq.weight.loraB", "output.weight.loraA", "noDot"]
    assert lora.tensors_to_patch(names) == {"layers.0.attention.wq.weight", "output.weight"}
    for r, alpha in ((16, 32), (16, 8), (3, 1), (64, 16), (7, 5)):
        s = lora.scaling(r, alpha)
        assert s.dtype == np.float32 and s == np.float32(alpha) / np.float32(r)
    assert lora.scaling(16, 16) == 1.0


def test_load_lora_missing_loraB_is_load_error(tmp_path, capfd):
    hp, w = synth.make_llama(synth.TINY, G.TYPE_Q8_0)  # (TINY's n_ff breaks the dims[0] % 64 rule of Q4_0 files)
    model = tmp_path / "m.bin"
    synth.write_ggjt(model, hp, w)
    bad = tmp_path / "bad.ggla"
    synth.write_ggla(bad, 4, 4, {"layers.0.attention.wq.weight.loraA": np.zeros((128, 4), np.float32)})
    L = llama._lib()
    mp = llama._MP(64, 1, -1, 0, 1.0, 10000, 0, -1, 0)
    paths = (C.c_char_p * 1)(str(bad).encode())
    assert not L.llm_llama_load_lora(str(model).encode(), C.byref(mp), paths, 1)
    assert "UnknownTensor" in capfd.readouterr().err
    with pytest.raises(KeyError, match="loraB"):
        lora.patch_weights(w, synth.tensor_shapes(hp), [str(bad)], G.TYPE_Q8_0)
    # a model file given as an adapter is not one
    paths = (C.c_char_p * 1)(str(model).encode())
    assert not L.llm_llama_load_lora(str(model).encode(), C.byref(mp), paths, 1)


def test_ggla_layout_bytes(tmp_path):
    """The writer's layout, byte by byte: magic, version, r, alpha, then the first tensor record and its padding."""
    a = np.arange(8, dtype=np.float32).reshape(2, 4)
    path = tmp_path / "x.ggla"
    synth.write_ggla(path, 4, 8, {"w.loraA": a})
    b = path.read_bytes()
    assert b[:16] == struct.pack("<IIii", 0x67676C61, 1, 4, 8)
    assert b[16:28] == struct.pack("<iiI", 2, 7, G.TYPE_F32) and b[28:36] == struct.pack("<2i", 4, 2)
    assert b[36:43] == b"w.loraA"
    assert b[64:] == a.tobytes() and set(b[43:64]) == {0}
