"""LoRA adapters (crates/llm-base/src/lora.rs, loader.rs:486-531, 651-670) for the graph builders of this package.

read_adapter() reads a ggla file through the library's container reader (llm_ggml_file_open / llm_ggml_file_lora).
patch_weights() applies adapters to a weight dict of the kind make_llama / make_bloom / ... return (raw GGML bytes for 2-D
weights), running LoraAdapter::patch's graph through the ggml ABI on the device:

    ba = mul_mat(A, B)                    A: .loraA [r, n_in] f32 or f16,  B: .loraB [r, n_out] f32
    ba = scale(ba, new_f32(alpha / r))    only when the scaling is not 1
    out = add(W, ba)                      requantized to W's type (kernels/lora.h), then copied over W

so every generic family (gptneox.py ... mpt.py) can take patched weights.  The LLaMA loader does the same in C++
(llm_llama_load_lora, llama.Llama.load(lora=...))."""
import ctypes as C

import numpy as np

from . import ggml as G


def scaling(r, alpha):
    """LoraParameters::calculate_scaling: (alpha as f32) / (r as f32), in f32."""
    return np.float32(np.float32(alpha) / np.float32(r))


def tensors_to_patch(names):
    """Every adapter tensor name minus its last '.'-component (rsplit_once('.')); names without a '.' are skipped."""
    return {n.rsplit(".", 1)[0] for n in names if "." in n}


def read_adapter(path):
    """{r, alpha, scaling, tensors: {name: ndarray [ne1, ne0] f32 / f16}, to_patch} of a ggla file.  ValueError if the
    reader rejects it or it is another container."""
    from .llama import _TD, _lib
    L = _lib()
    f = L.llm_ggml_file_open(str(path).encode())
    if not f:
        raise ValueError(f"{path}: rejected by the container reader")
    try:
        r, alpha, nt = C.c_int(), C.c_int(), C.c_int()
        if L.llm_ggml_file_lora(f, C.byref(r), C.byref(alpha)) != 0:
            raise ValueError(f"{path}: not a ggla LoRA adapter")
        L.llm_ggml_file_info(f, None, None, None, C.byref(nt), None)
        tensors = {}
        for i in range(nt.value):
            d = _TD()
            L.llm_ggml_file_tensor(f, i, C.byref(d))
            dt = {G.TYPE_F32: np.float32, G.TYPE_F16: np.float16}.get(d.type)
            if dt is None:
                raise ValueError(f"{path}: tensor {d.name.decode()} has type {d.type}; adapters hold f32 or f16")
            ne0, ne1 = d.ne[0], d.ne[1]
            n = ne0 * ne1 * np.dtype(dt).itemsize
            raw = (C.c_uint8 * n).from_address(d.data)
            tensors[d.name.decode()] = np.frombuffer(raw, dtype=dt).reshape(ne1, ne0).copy()
    finally:
        L.llm_ggml_file_close(f)
    return dict(r=r.value, alpha=alpha.value, scaling=scaling(r.value, alpha.value), tensors=tensors,
                to_patch=tensors_to_patch(tensors))


def _as_adapter(a):
    if isinstance(a, dict):
        a = dict(a)
        a.setdefault("scaling", scaling(a["r"], a["alpha"]))
        a.setdefault("to_patch", tensors_to_patch(a["tensors"]))
        return a
    return read_adapter(a)


def _wtype_of(nbytes, ne0, ne1):
    """The weight type of raw bytes whose type was not given, from their size: the first of Q4_0, Q4_1, Q5_0, Q5_1, Q8_0,
    F16, F32 that fits.  K types are never guessed: Q4_K stores 4.5 bits per weight as Q4_0 does and Q5_K 5.5 as Q5_0
    does, so sizes cannot tell them apart — name a K type (or a {name: type} dict) in patch_weights' `wtype`."""
    for t in (G.TYPE_Q4_0, G.TYPE_Q4_1, G.TYPE_Q5_0, G.TYPE_Q5_1, G.TYPE_Q8_0, G.TYPE_F16, G.TYPE_F32):
        if G.row_bytes(t, ne0) * ne1 == nbytes:
            return t
    raise ValueError(f"no weight type stores [{ne0}, {ne1}] in {nbytes} bytes")


def patch_one(W, wtype, ne0, ne1, A, B, s):
    """One LoraAdapter::patch: W raw bytes of [ne0, ne1] in `wtype`, A [ne0, r] and B [ne1, r] as stored (ne [r, ne0] /
    [r, ne1]).  Returns (patched raw bytes, the f32 operand the add consumed: `scaled`, or `ba` when s == 1)."""
    A, B = np.ascontiguousarray(A), np.ascontiguousarray(B)
    r = A.shape[1]
    nbytes = np.asarray(W).nbytes
    # the patch context (lora.rs:96-115 sizes it from the tensor sizes plus 5 %; here the graph's own size is added, so
    # that small tensors fit as well) and, apart, the target's context: in the reference W lives in the model's context
    with G.Context(A.nbytes + B.nbytes + nbytes + 2 * 4 * ne0 * ne1 + (1 << 20)) as ctx, G.Context(nbytes + 4096) as wctx:
        w = wctx.tensor_from(np.asarray(W).view(np.uint8), wtype, (ne0, ne1))
        a = ctx.tensor_from(A, G.TYPE_F16 if A.dtype == np.float16 else G.TYPE_F32, (r, ne0))
        b = ctx.tensor_from(B.astype(np.float32), G.TYPE_F32, (r, ne1))
        ba = ctx.op_mul_mat(a, b)
        if s != np.float32(1.0):
            ba = ctx.op_scale(ba, ctx.new_f32(float(s)))
        out = ctx.op_add(w, ba)
        ctx.graph().build_forward_expand(out).compute()
        return out.read_data(np.uint8), ba.read_data(np.float32).reshape(ne1, ne0)


def patch_weights(w, shapes, adapters, wtype=None):
    """A copy of the weight dict `w` with every adapter applied in the order given (loader.rs:660-667).  shapes: name ->
    (ne0, ne1 or None); adapters: paths of ggla files or dicts {r, alpha, tensors}.  A target without its .loraA /
    .loraB raises KeyError (LoadError::UnknownTensor).  wtype: the type of every 2-D weight (Q4_0 .. Q8_0, Q2_K .. Q6_K,
    F16), or a dict {name: type} for models that mix types as the *_K_S / *_K_M files do (names it lacks, and
    wtype=None, fall back to the size: _wtype_of, which never answers a K type)."""
    ads = [_as_adapter(a) for a in adapters]
    type_of = wtype.get if isinstance(wtype, dict) else (lambda name: wtype)
    out = dict(w)
    for name, (ne0, ne1) in shapes.items():
        for ad in ads:
            if name not in ad["to_patch"]:
                continue
            for part in (".loraA", ".loraB"):
                if name + part not in ad["tensors"]:
                    raise KeyError(f"LoadError::UnknownTensor: {name + part}")
            t = type_of(name)
            t = t if t is not None else _wtype_of(np.asarray(out[name]).nbytes, ne0, ne1 or 1)
            out[name], _ = patch_one(out[name], t, ne0, ne1 or 1, ad["tensors"][name + ".loraA"],
                                     ad["tensors"][name + ".loraB"], ad["scaling"])
    return out
