"""ctypes handle on the host mirror (llm_amd/csrc/host/llm_host.h): the call sequence of
crates/llm-base (Model::start_session, InferenceSession::feed_prompt / infer_next_token,
Model::evaluate) as a rustformers/llm user drives it."""
import ctypes as C

import numpy as np

from . import ggml


class _HP(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("n_vocab", "n_embd", "n_mult", "n_head", "n_head_kv", "n_layer", "n_rot", "file_type")]


class _MP(C.Structure):
    _fields_ = [("context_size", C.c_int32), ("use_gpu", C.c_int32), ("gpu_layers", C.c_int32),
                ("has_rope_overrides", C.c_int32), ("rope_frequency_scale", C.c_float),
                ("rope_frequency_base", C.c_int32), ("layer_begin", C.c_int32), ("layer_end", C.c_int32), ("n_gqa", C.c_int32)]


class _SC(C.Structure):
    _fields_ = [("memory_k_type", C.c_int32), ("memory_v_type", C.c_int32), ("n_batch", C.c_int32),
                ("n_threads", C.c_int32)]


class _TD(C.Structure):
    _fields_ = [("name", C.c_char_p), ("type", C.c_int32), ("n_dims", C.c_int32), ("ne", C.c_int64 * 2),
                ("data", C.c_void_p)]


_bound = False


def _lib():
    global _bound
    L = ggml.lib()
    if not _bound:
        L.llm_llama_new.restype = C.c_void_p
        L.llm_llama_new.argtypes = [C.POINTER(_HP), C.POINTER(_MP), C.POINTER(_TD), C.c_int]
        L.llm_model_free.argtypes = [C.c_void_p]
        L.llm_model_stages.restype = C.c_int
        L.llm_model_stages.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.llm_ggml_file_open.restype = C.c_void_p
        L.llm_ggml_file_open.argtypes = [C.c_char_p]
        L.llm_ggml_file_close.argtypes = [C.c_void_p]
        L.llm_ggml_file_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(_HP),
                                         C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.llm_ggml_file_tensor.restype = C.c_int
        L.llm_ggml_file_tensor.argtypes = [C.c_void_p, C.c_int, C.POINTER(_TD)]
        L.llm_ggml_file_vocab.restype = C.c_int
        L.llm_ggml_file_vocab.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_float)]
        L.llm_llama_load.restype = C.c_void_p
        L.llm_llama_load.argtypes = [C.c_char_p, C.POINTER(_MP)]
        L.llm_llama_load_lora.restype = C.c_void_p
        L.llm_llama_load_lora.argtypes = [C.c_char_p, C.POINTER(_MP), C.POINTER(C.c_char_p), C.c_int]
        L.llm_ggml_file_lora.restype = C.c_int
        L.llm_ggml_file_lora.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.llm_lora_timing.argtypes = [C.POINTER(C.c_double), C.c_int]
        L.llm_start_session.restype = C.c_void_p
        L.llm_start_session.argtypes = [C.c_void_p, C.POINTER(_SC)]
        L.llm_session_free.argtypes = [C.c_void_p]
        L.llm_start_session_on.restype = C.c_void_p
        L.llm_start_session_on.argtypes = [C.c_void_p, C.POINTER(_SC), C.c_int]
        L.llm_session_read_node_host.restype = C.c_size_t
        L.llm_session_read_node_host.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        L.llm_session_seek.argtypes = [C.c_void_p, C.c_int]
        L.llm_session_set_speculate.argtypes = [C.c_void_p, C.c_int]
        L.llm_evaluate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.llm_feed_prompt.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.llm_infer_next_token_greedy.restype = C.c_int32
        L.llm_infer_next_token_greedy.argtypes = [C.c_void_p, C.c_void_p]
        L.llm_infer_next_token_topk.restype = C.c_int32
        L.llm_infer_next_token_topk.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.POINTER(C.c_uint64), C.c_int]
        L.llm_session_snapshot.restype = C.c_size_t
        L.llm_session_snapshot.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.llm_session_from_snapshot.restype = C.c_void_p
        L.llm_session_from_snapshot.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.llm_infer_tokens_greedy_device.restype = C.c_int
        L.llm_infer_tokens_greedy_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.llm_host_timing.restype = None
        L.llm_host_timing.argtypes = [C.POINTER(C.c_double), C.c_int]
        L.llm_session_rewind.restype = C.c_int
        L.llm_session_rewind.argtypes = [C.c_void_p, C.c_int]
        L.llm_session_last_logits.restype = C.POINTER(C.c_float)
        L.llm_session_last_logits.argtypes = [C.c_void_p]
        L.llm_session_n_past.restype = C.c_int
        L.llm_session_n_past.argtypes = [C.c_void_p]
        L.llm_session_last_graph_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.llm_session_stage_buffers.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                                C.POINTER(C.c_size_t)]
        L.llm_session_kv.restype = C.c_size_t
        L.llm_session_kv.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t]
        L.llm_session_topk.restype = C.c_int
        L.llm_session_topk.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.llm_session_read_node.restype = C.c_size_t
        L.llm_session_read_node.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.c_void_p, C.c_size_t]
        L.llm_session_perplexity.restype = C.c_int
        L.llm_session_perplexity.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int32, C.c_int, C.c_void_p, C.c_int,
                                             C.c_void_p]
        L.llm_evaluate_batch.restype = C.c_int
        L.llm_evaluate_batch.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_void_p]
        L.llm_infer_next_tokens_greedy_batch.restype = C.c_int
        L.llm_infer_next_tokens_greedy_batch.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_void_p]
        L.llm_infer_tokens_greedy_batch_device.restype = C.c_int
        L.llm_infer_tokens_greedy_batch_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_void_p]
        L.llm_sample_exact.restype = C.c_int32
        L.llm_sample_exact.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.llm_infer_next_tokens_sampled_batch.restype = C.c_int
        L.llm_infer_next_tokens_sampled_batch.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.llm_infer_tokens_sampled_batch_device.restype = C.c_int
        L.llm_infer_tokens_sampled_batch_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                            C.c_void_p]
        L.llm_infer_next_token_sampled.restype = C.c_int32
        L.llm_infer_next_token_sampled.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.llm_infer_tokens_sampled_device.restype = C.c_int
        L.llm_infer_tokens_sampled_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.llm_sample_chain.restype = C.c_int32
        L.llm_sample_chain.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.llm_sampler_log2.restype = None
        L.llm_sampler_log2.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.llm_infer_next_token_sampled_chain.restype = C.c_int32
        L.llm_infer_next_token_sampled_chain.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.llm_infer_tokens_sampled_chain_device.restype = C.c_int
        L.llm_infer_tokens_sampled_chain_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.llm_infer_next_tokens_sampled_chain_batch.restype = C.c_int
        L.llm_infer_next_tokens_sampled_chain_batch.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                                                C.c_void_p]
        L.llm_infer_tokens_sampled_chain_batch_device.restype = C.c_int
        L.llm_infer_tokens_sampled_chain_batch_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                                                  C.c_void_p, C.c_void_p]
        L.llm_infer_until.restype = C.c_int
        L.llm_infer_until.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.llm_infer_until_batch.restype = C.c_int
        L.llm_infer_until_batch.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p, C.c_void_p]
        L.llm_infer_until_pool.restype = C.c_int
        L.llm_infer_until_pool.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_void_p]
        L.llm_pool_schedule.restype = C.c_int
        L.llm_pool_schedule.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        L.llm_feed_prompt_batch.restype = C.c_int
        L.llm_feed_prompt_batch.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        L.llm_prompt_pack.restype = C.c_int
        L.llm_prompt_pack.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.llm_session_stage_rows.restype = C.c_void_p
        L.llm_session_stage_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.llm_pack_schedule.restype = C.c_int
        L.llm_pack_schedule.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.llm_pool_step_cap.restype = C.c_int
        L.llm_pool_step_cap.argtypes = [C.c_int]
        L.llm_until_rule.restype = C.c_int
        L.llm_until_rule.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p]
        _bound = True
    return L


class SamplerParams(C.Structure):
    """llm_sampler_params / ggml_hip_sampler: the sampled batched chain's {k, top_p, temperature, penalty}."""
    _fields_ = [("k", C.c_int32), ("top_p", C.c_float), ("temperature", C.c_float), ("penalty", C.c_float)]


class SamplerChain(C.Structure):
    """llm_sampler_chain / ggml_hip_sampler_chain: the four parameters and the reference's other samplers (flat bias, frequency /
    presence penalty, tail-free, locally typical, min-p, Mirostat 2)."""
    _fields_ = [("base", SamplerParams), ("freq", C.c_float), ("presence", C.c_float), ("tail_free_z", C.c_float), ("typical_p", C.c_float),
                ("min_p", C.c_float), ("mirostat", C.c_int32), ("tau", C.c_float), ("eta", C.c_float), ("n_bias", C.c_int32),
                ("bias_id", C.c_int32 * 64), ("bias", C.c_float * 64)]


def sampler_chain(k=40, top_p=0.95, temperature=0.8, penalty=1.30, freq=0.0, presence=0.0, tail_free_z=1.0, typical_p=1.0, min_p=0.0,
                  bias=(), mirostat=0, tau=5.0, eta=0.1):
    """A SamplerChain from keywords; the defaults of everything behind `penalty` are neutral (the default chain).  bias: [(id, b), ...],
    at most 64 pairs, every id once (b = -inf bans a token); mirostat: 0 or 2 (with 2: tau, eta, and no truncating sampler — top_p 1
    too).  ValueError for more than 64 bias pairs; everything else is checked by the library."""
    bias = list(bias)
    if len(bias) > 64:
        raise ValueError("sampler_chain: at most 64 bias pairs")
    c = SamplerChain(SamplerParams(int(k), float(top_p), float(temperature), float(penalty)), float(freq), float(presence),
                     float(tail_free_z), float(typical_p), float(min_p), int(mirostat), float(tau), float(eta), len(bias))
    for i, (t, b) in enumerate(bias):
        c.bias_id[i] = int(t)
        c.bias[i] = float(b)
    return c


class UntilRequest(C.Structure):
    """llm_until_request: one session's request of a generation that stops — its sampler (NULL: the first maximum), its budget, up to
    8 stop ids."""
    _fields_ = [("chain", C.c_void_p), ("max_tokens", C.c_int32), ("n_stop", C.c_int32), ("stop_id", C.c_int32 * 8)]


class ChainEnd(C.Structure):
    """ggml_hip_chain_end: a column's end rule for ggml_hip_decode_chain_requests / ggml_hip_decode_batch_requests."""
    _fields_ = [("budget", C.c_int32), ("n_stop", C.c_int32), ("stop_id", C.c_int32 * 8)]


def chain_end(budget, stop=()):
    stop = [int(t) for t in stop]
    if len(stop) > 8:
        raise ValueError("chain_end: at most 8 stop ids")
    e = ChainEnd(int(budget), len(stop))
    for i, t in enumerate(stop):
        e.stop_id[i] = t
    return e


ENDED_BY = {1: "budget", 2: "stop", 3: "context"}


def until_request(max_tokens, stop=(), sampler=None):
    """(UntilRequest, the SamplerChain it points at or None — keep it alive beside the request).  sampler: sampler_chain's keywords
    as a dict, or None for the first maximum.  ValueError for more than 8 stop ids."""
    stop = [int(t) for t in stop]
    if len(stop) > 8:
        raise ValueError("until_request: at most 8 stop ids")
    chain = None if sampler is None else sampler_chain(**sampler)
    r = UntilRequest(None if chain is None else C.addressof(chain), int(max_tokens), len(stop))
    for i, t in enumerate(stop):
        r.stop_id[i] = t
    return r, chain


def _mu(mu, B, chain):
    """The Mirostat states: a contiguous float32 array of B elements, advanced in place (None without Mirostat)."""
    if mu is None:
        if chain.mirostat != 0:
            raise ValueError("mu: Mirostat needs its state, a float32 array with one element per session (start it at 2 * tau)")
        return None
    if not (isinstance(mu, np.ndarray) and mu.dtype == np.float32 and mu.size == B and mu.flags.c_contiguous):
        raise ValueError("mu: a contiguous float32 array with one Mirostat state per session (updated in place)")
    return mu.ctypes.data


def sample_chain(logits, window, rng, mu=None, **chain):
    """llm_sample_chain: one draw from a row of logits by the whole sampler (sampler_chain's keywords; no device needed).  rng: a
    uint64 array of one element, mu: a float32 array of one element (Mirostat 2's state; None otherwise), both stepped in place.
    Returns the id; ValueError, with nothing moved, on what the specification declines."""
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    window = np.ascontiguousarray(window, dtype=np.int32)
    if not (isinstance(rng, np.ndarray) and rng.dtype == np.uint64 and rng.size == 1 and rng.flags.c_contiguous):
        raise ValueError("sample_chain: rng is a uint64 array of one element")
    c = sampler_chain(**chain)
    rc = _lib().llm_sample_chain(logits.ctypes.data, logits.size, window.ctypes.data if window.size else None, window.size,
                                 C.addressof(c), rng.ctypes.data, _mu(mu, 1, c))
    if rc < 0:
        raise ValueError("llm_sample_chain: bad arguments")
    return int(rc)


def sample_exact(logits, window, rng, k=40, top_p=0.95, temperature=0.8, penalty=1.30):
    """llm_sample_exact: one draw from a row of logits by the sampled chain's sampler (no device needed).  window: the most recent
    tokens, oldest first; rng: a uint64 array of one element, stepped in place.  Returns the id; ValueError on bad arguments."""
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    window = np.ascontiguousarray(window, dtype=np.int32)
    if not (isinstance(rng, np.ndarray) and rng.dtype == np.uint64 and rng.size == 1 and rng.flags.c_contiguous):
        raise ValueError("sample_exact: rng is a uint64 array of one element")
    prm = SamplerParams(int(k), float(top_p), float(temperature), float(penalty))
    rc = _lib().llm_sample_exact(logits.ctypes.data, logits.size, window.ctypes.data if window.size else None, window.size,
                                 C.addressof(prm), rng.ctypes.data)
    if rc < 0:
        raise ValueError("llm_sample_exact: bad arguments")
    return int(rc)


def inspect_file(path):
    """Parses a GGML-family container with the C++ reader (no device needed): None if it is rejected, else
    {container, version, hp, vocab: [(bytes, score)], tensors: [{name, type, n_dims, ne, offset_mod32, head}]}."""
    L = _lib()
    f = L.llm_ggml_file_open(str(path).encode())
    if not f:
        return None
    try:
        c, v, nt, nv, hp = C.c_int(), C.c_int(), C.c_int(), C.c_int(), _HP()
        L.llm_ggml_file_info(f, C.byref(c), C.byref(v), C.byref(hp), C.byref(nt), C.byref(nv))
        vocab = []
        for i in range(nv.value):
            buf, sc = C.create_string_buffer(256), C.c_float()
            n = L.llm_ggml_file_vocab(f, i, buf, 256, C.byref(sc))
            vocab.append((buf.raw[:min(n, 256)], sc.value))
        tensors = []
        for i in range(nt.value):
            d = _TD()
            L.llm_ggml_file_tensor(f, i, C.byref(d))
            head = bytes((C.c_uint8 * 16).from_address(d.data))
            tensors.append(dict(name=d.name.decode(), type=d.type, n_dims=d.n_dims, ne=(d.ne[0], d.ne[1]),
                                offset_mod32=d.data % 32, head=head))
        return dict(container=c.value, version=v.value, hp=hp, vocab=vocab, tensors=tensors)
    finally:
        L.llm_ggml_file_close(f)


class Llama:
    """models/llama Llama + ModelParameters{use_gpu: true}.  `weights`: {name: ndarray} as produced by
    llm_amd.synth (raw GGML bytes for 2-D tensors) — must outlive the model (mmap semantics)."""

    def __init__(self, hp, weights, context_size=2048, gpu_layers=-1, rope_overrides=None, layer_range=None):
        from .synth import stage_tensor_names, tensor_shapes
        self.hp = dict(hp)
        self.weights = weights
        L = _lib()
        lb, le = layer_range if layer_range else (0, hp["n_layer"])
        self.layer_range = (lb, le)
        self.is_first, self.is_last = lb == 0, le == hp["n_layer"]
        keep = stage_tensor_names(hp, lb, le)
        shapes = {k: v for k, v in tensor_shapes(hp).items() if k in keep}
        descs = (_TD * len(shapes))()
        self._names = []
        for i, (name, (ne0, ne1)) in enumerate(shapes.items()):
            b = name.encode()
            self._names.append(b)
            descs[i].name = b
            wt = hp.get("wtypes", {}).get(name, hp["wtype"])  # per-tensor types of a mixed file (*_K_M: some tensors Q6_K)
            descs[i].type = ggml.TYPE_F32 if ne1 is None else wt
            descs[i].n_dims = 1 if ne1 is None else 2
            descs[i].ne[0] = ne0
            descs[i].ne[1] = 1 if ne1 is None else ne1
            arr = weights[name]
            exp = ne0 * 4 if ne1 is None else ggml.row_bytes(wt, ne0) * ne1
            assert arr.nbytes == exp, (name, arr.nbytes, exp)
            descs[i].data = arr.ctypes.data
        h = _HP(hp["n_vocab"], hp["n_embd"], hp.get("n_mult", 256), hp["n_head"], hp["n_head_kv"], hp["n_layer"],
                hp["n_rot"], 2 * 1000 + ggml.FTYPE_OF[hp["wtype"]])
        mp = _MP(context_size, 1, gpu_layers, 0, 1.0, 10000, lb, le, 0)
        if rope_overrides:
            mp.has_rope_overrides = 1
            mp.rope_frequency_scale = rope_overrides["frequency_scale"]
            mp.rope_frequency_base = rope_overrides["frequency_base"]
        self.context_size = context_size
        self.ptr = L.llm_llama_new(C.byref(h), C.byref(mp), descs, len(shapes))

    @classmethod
    def load(cls, path, context_size=2048, gpu_layers=-1, n_gqa=0, lora=()):
        """llm::load::<Llama>(path, …, ModelParameters{prefer_mmap: true, use_gpu: true}): the C++ container reader
        (llm_ggml_file_open) maps the GGML/GGMF/GGJT file and the tensors point into the mapping.
        lora: paths of ggla adapters (ModelParameters::lora_adapters), applied in order at load time
        (llm_llama_load_lora: the model is read into a buffer it owns, no mapping)."""
        L = _lib()
        info = inspect_file(path)
        if info is None:
            raise ValueError(f"{path}: not a loadable GGML-family container")
        self = cls.__new__(cls)
        mp = _MP(context_size, 1, gpu_layers, 0, 1.0, 10000, 0, -1, n_gqa)  # n_gqa: ModelParameters::n_gqa (80 layers and more)
        if lora:
            paths = (C.c_char_p * len(lora))(*[str(p).encode() for p in lora])
            self.ptr = L.llm_llama_load_lora(str(path).encode(), C.byref(mp), paths, len(lora))
        else:
            self.ptr = L.llm_llama_load(str(path).encode(), C.byref(mp))
        if not self.ptr:
            raise ValueError(f"{path}: load failed")
        h = info["hp"]
        wtype = next(t["type"] for t in info["tensors"] if t["n_dims"] == 2)
        n_ff = next(t["ne"][1] for t in info["tensors"] if t["name"].endswith("feed_forward.w1.weight"))
        if n_gqa > 0 and h.n_layer >= 80:
            h.n_head_kv = h.n_head // n_gqa
        self.hp = dict(n_vocab=h.n_vocab, n_embd=h.n_embd, n_mult=h.n_mult, n_head=h.n_head, n_head_kv=h.n_head_kv,
                       n_layer=h.n_layer, n_rot=h.n_rot, n_ff=n_ff, wtype=wtype)
        self.weights = None
        self.layer_range = (0, h.n_layer)
        self.is_first = self.is_last = True
        self.context_size = context_size
        return self

    def stages(self):
        """[(layer_begin, layer_end, device_slot)] — one entry for an unsplit model, one per device slot for a model that
        llm_llama_new split over the GPUs of this process (ggml_hip_set_tensor_split / GGML_HIP_LAYER_SPLIT)."""
        lb, le, dv = ((C.c_int * 16)() for _ in range(3))
        n = _lib().llm_model_stages(self.ptr, lb, le, dv, 16)
        return [(lb[i], le[i], dv[i]) for i in range(n)]

    def start_session(self, n_batch=8, kv_type=ggml.TYPE_F16):
        return Session(self, n_batch, kv_type)

    def start_session_on(self, slot, n_batch=8, kv_type=ggml.TYPE_F16):
        """A session of this (unsplit) model on another device slot of the model's GPU: its own stream, K/V and plans, the
        model's weights — sessions on different slots run concurrently (llm_start_session_on)."""
        return Session(self, n_batch, kv_type, slot=slot)

    def session_from_snapshot(self, blob):
        """InferenceSession::from_snapshot; None on SnapshotError."""
        blob = np.ascontiguousarray(np.frombuffer(blob, dtype=np.uint8))
        ptr = _lib().llm_session_from_snapshot(self.ptr, blob.ctypes.data, blob.size)
        if not ptr:
            return None
        s = Session.__new__(Session)
        s.model, s.ptr = self, ptr
        return s

    def evaluate_batch(self, sessions, tokens):
        """One decode step of several sessions of this model, tokens[i] for sessions[i], as ONE pass over the weights where the
        backend can (llm_evaluate_batch: 2..8 sessions with f16 K/V of a block-format or F16 model, or of a K-quant model — Q2_K …
        Q6_K, uniform or a *_K_M / *_K_S mix — once ggml.set_option("plan_batch_k", 1) is set (default 0); anything else is
        evaluated one session after the other, with the same results).  Returns (ran_batched, logits [B, n_vocab]); every session ends as
        after evaluate([token]).  ValueError, with nothing evaluated: a session listed twice, of another model or device slot,
        a token outside the vocabulary, a session whose context is full."""
        tokens = np.ascontiguousarray(tokens, dtype=np.int32)
        if tokens.size != len(sessions):
            raise ValueError("evaluate_batch: one token per session")
        ptrs = (C.c_void_p * len(sessions))(*[s.ptr for s in sessions])
        logits = np.zeros((len(sessions), self.hp["n_vocab"]), np.float32)
        rc = _lib().llm_evaluate_batch(self.ptr, ptrs, tokens.ctypes.data, len(sessions), logits.ctypes.data)
        if rc < 0:
            raise ValueError("llm_evaluate_batch: bad arguments (nothing was evaluated)")
        return bool(rc), logits

    def infer_next_tokens_batch(self, sessions):
        """Session.infer_next_token for several sessions of this model in one such step (llm_infer_next_tokens_greedy_batch):
        returns (ran_batched, ids)."""
        ptrs = (C.c_void_p * len(sessions))(*[s.ptr for s in sessions])
        out = np.zeros(len(sessions), np.int32)
        rc = _lib().llm_infer_next_tokens_greedy_batch(self.ptr, ptrs, len(sessions), out.ctypes.data)
        if rc < 0:
            raise ValueError("llm_infer_next_tokens_greedy_batch: bad arguments (nothing was evaluated)")
        return bool(rc), out

    def infer_tokens_batch(self, sessions, n):
        """n greedy tokens for each of several sessions of this model, sampled on the device where the backend can
        (llm_infer_tokens_greedy_batch_device: every step one pass over the weights, no host round trip between steps; the models
        evaluate_batch takes batched, K-quant models under option plan_batch_k included; anything else runs as n steps of
        infer_next_tokens_batch, with the same results).  Returns (ran_chained, ids [n, B]).  ValueError,
        with nothing evaluated: the bad arguments of evaluate_batch, n < 1, a session without room for n tokens."""
        ptrs = (C.c_void_p * len(sessions))(*[s.ptr for s in sessions])
        out = np.zeros((max(int(n), 0), len(sessions)), np.int32)
        rc = _lib().llm_infer_tokens_greedy_batch_device(self.ptr, ptrs, len(sessions), int(n), out.ctypes.data)
        if rc < 0:
            raise ValueError("llm_infer_tokens_greedy_batch_device: bad arguments (nothing was evaluated)")
        return bool(rc), out

    @staticmethod
    def _rngs(rngs, B):
        if not (isinstance(rngs, np.ndarray) and rngs.dtype == np.uint64 and rngs.size == B and rngs.flags.c_contiguous):
            raise ValueError("rngs: a contiguous uint64 array with one generator state per session (updated in place)")
        return rngs

    def infer_next_tokens_sampled_batch(self, sessions, rngs, k=40, top_p=0.95, temperature=0.8, penalty=1.30, mu=None, **extras):
        """infer_next_tokens_batch with the shape of the reference's default sampler instead of the first maximum
        (llm_infer_next_tokens_sampled_batch): repetition penalty over each session's last 64 tokens, top-k, top-p, temperature, one
        xorshift64* draw from rngs[i] (a uint64 array, updated in place).  Returns (ran_batched, ids).  ValueError, with nothing
        evaluated and no generator moved: the bad arguments of evaluate_batch, k outside 1 .. n_vocab, a non-positive top_p,
        temperature or penalty.  extras: sampler_chain's further keywords (freq, presence, tail_free_z, typical_p, min_p, bias,
        mirostat, tau, eta; neutral by default); mu: the sessions' Mirostat states, a float32 array advanced in place like rngs."""
        ptrs = (C.c_void_p * len(sessions))(*[s.ptr for s in sessions])
        rngs = self._rngs(rngs, len(sessions))
        prm = sampler_chain(k, top_p, temperature, penalty, **extras)
        out = np.zeros(len(sessions), np.int32)
        rc = _lib().llm_infer_next_tokens_sampled_chain_batch(self.ptr, ptrs, len(sessions), C.addressof(prm), rngs.ctypes.data,
                                                              _mu(mu, len(sessions), prm), out.ctypes.data)
        if rc < 0:
            raise ValueError("llm_infer_next_tokens_sampled_batch: bad arguments (nothing was evaluated)")
        return bool(rc), out

    def infer_tokens_sampled_batch(self, sessions, n, rngs, k=40, top_p=0.95, temperature=0.8, penalty=1.30, mu=None, **extras):
        """n such tokens for each session, all but the first drawn on the device where the backend can
        (llm_infer_tokens_sampled_batch_device: no host round trip between steps; k <= 256; the models evaluate_batch takes
        batched, K-quant models under option plan_batch_k included); anything else runs as n steps of
        infer_next_tokens_sampled_batch, with the same ids, sessions and generator states.  Returns (ran_chained, ids [n, B]).
        ValueError as above, and for n < 1 or a session without room for n tokens.  extras and mu as above (Mirostat 2 on the
        device: n_vocab <= 32768)."""
        ptrs = (C.c_void_p * len(sessions))(*[s.ptr for s in sessions])
        rngs = self._rngs(rngs, len(sessions))
        prm = sampler_chain(k, top_p, temperature, penalty, **extras)
        out = np.zeros((max(int(n), 0), len(sessions)), np.int32)
        rc = _lib().llm_infer_tokens_sampled_chain_batch_device(self.ptr, ptrs, len(sessions), int(n), C.addressof(prm), rngs.ctypes.data,
                                                                _mu(mu, len(sessions), prm), out.ctypes.data)
        if rc < 0:
            raise ValueError("llm_infer_tokens_sampled_batch_device: bad arguments (nothing was evaluated)")
        return bool(rc), out

    def infer_until_batch(self, sessions, requests, rngs, mu=None):
        """Generation that stops, for several sessions at once (llm_infer_until_batch): requests[i] is a dict for sessions[i] with
        max_tokens, stop (up to 8 ids, optional) and sampler (sampler_chain's keywords as a dict; None or absent: the first maximum).
        Every session draws and evaluates until it draws one of its stop ids (still evaluated, as the reference does), has drawn
        max_tokens, or its context is full; one device chain where the backend can (a session that has ended is frozen while the
        others go on, and the call ends when none is left), steps of the sessions still going otherwise — the same results.
        rngs: a uint64 array with one state per session (None when every request is greedy), mu: the Mirostat states (None without
        Mirostat 2); both advanced in place.  Returns (ids [n, B] with -1 behind a session's last token, counts [B], reasons [B] of
        "budget" / "stop" / "context", ran_chained).  ValueError with nothing moved on bad arguments."""
        B = len(sessions)
        if len(requests) != B:
            raise ValueError("infer_until_batch: one request per session")
        ptrs = (C.c_void_p * B)(*[s.ptr for s in sessions])
        built = [until_request(r["max_tokens"], r.get("stop", ()), r.get("sampler")) for r in requests]
        reqs = (UntilRequest * B)(*[b[0] for b in built])
        sampled = [b[1] for b in built if b[1] is not None]
        if sampled:
            rngs = self._rngs(rngs, B)
        if any(c.mirostat != 0 for c in sampled) or mu is not None:
            if not (isinstance(mu, np.ndarray) and mu.dtype == np.float32 and mu.size == B and mu.flags.c_contiguous):
                raise ValueError("mu: a contiguous float32 array with one Mirostat state per session (updated in place)")
        n = max([int(r["max_tokens"]) for r in requests] + [0])
        out = np.full((max(n, 0), B), -1, np.int32)
        counts, why = np.zeros(B, np.int32), np.zeros(B, np.int32)
        rc = _lib().llm_infer_until_batch(self.ptr, ptrs, B, C.addressof(reqs), None if rngs is None else rngs.ctypes.data,
                                          None if mu is None else mu.ctypes.data, out.ctypes.data, counts.ctypes.data, why.ctypes.data)
        if rc < 0:
            raise ValueError("llm_infer_until_batch: bad arguments (nothing was evaluated)")
        return out, counts, [ENDED_BY[int(w)] for w in why], bool(rc)

    def infer_until_pool(self, sessions, requests, rngs, mu=None, max_cols=8):
        """Generation that stops for MORE sessions than a batched step has columns (llm_infer_until_pool): infer_until_batch's
        requests, one per session, any number of them, over at most max_cols (1 .. 8) columns.  A column whose request has ended
        takes the next waiting session on the device, between two replays of the same step, so the columns stay busy; every session
        ends exactly as Session.infer_until leaves it alone.  Without the backend's pool (option plan_batch_pool = 0, a model it
        declines) the stepped loop runs under the same admission rule — the same results.  rngs, mu: as infer_until_batch, one entry
        per session.  Returns (ids: a list with one int32 array per request, counts [N], reasons [N], ran_chained).  ValueError with
        nothing moved on bad arguments."""
        N = len(sessions)
        if len(requests) != N or N < 1:
            raise ValueError("infer_until_pool: one request per session, at least one")
        ptrs = (C.c_void_p * N)(*[s.ptr for s in sessions])
        built = [until_request(r["max_tokens"], r.get("stop", ()), r.get("sampler")) for r in requests]
        reqs = (UntilRequest * N)(*[b[0] for b in built])
        sampled = [b[1] for b in built if b[1] is not None]
        if sampled:
            rngs = self._rngs(rngs, N)
        if any(c.mirostat != 0 for c in sampled) or mu is not None:
            if not (isinstance(mu, np.ndarray) and mu.dtype == np.float32 and mu.size == N and mu.flags.c_contiguous):
                raise ValueError("mu: a contiguous float32 array with one Mirostat state per session (updated in place)")
        n = max([int(r["max_tokens"]) for r in requests] + [0])
        out = np.full((N, max(n, 0)), -1, np.int32)
        counts, why = np.zeros(N, np.int32), np.zeros(N, np.int32)
        rc = _lib().llm_infer_until_pool(self.ptr, ptrs, N, C.addressof(reqs), None if rngs is None else rngs.ctypes.data,
                                         None if mu is None else mu.ctypes.data, int(max_cols), out.ctypes.data, counts.ctypes.data,
                                         why.ctypes.data)
        if rc < 0:
            raise ValueError("llm_infer_until_pool: bad arguments (nothing was evaluated)")
        return [out[i, :counts[i]].copy() for i in range(N)], counts, [ENDED_BY[int(w)] for w in why], bool(rc)

    @staticmethod
    def _packed(sessions, prompts):
        if len(prompts) != len(sessions) or len(sessions) < 1:
            raise ValueError("one prompt per session, at least one")
        prompts = [np.ascontiguousarray(p, dtype=np.int32).ravel() for p in prompts]
        counts = np.array([p.size for p in prompts], np.int32)
        tokens = np.ascontiguousarray(np.concatenate(prompts) if counts.sum() else np.zeros(1, np.int32), dtype=np.int32)
        return (C.c_void_p * len(sessions))(*[s.ptr for s in sessions]), tokens, counts

    def feed_prompt_batch(self, sessions, prompts, max_rows=512):
        """Session.feed_prompt for several sessions of this model at once (llm_feed_prompt_batch): prompts[i] goes to sessions[i], and
        the rows of all of them run as packed prompt batches of at most max_rows (1 .. 4096) rows — one pass over the weights per
        round instead of one per session and chunk (ggml_hip_prompt_pack: block-format models, f16 K/V).  Rounds: sessions in index
        order, each takes min(tokens left, room left in the round); the sessions' own n_batch is not consulted.  Every session ends
        as feed_prompt leaves it (tokens, n_past, last_logits of its last token).  Returns 1 if every round ran packed, 0 if the
        backend declined one: that round's and all later tokens were then fed one session after the other through feed_prompt.
        ValueError with nothing moved on bad arguments (a session twice, an empty prompt, a token outside the vocabulary, a prompt
        that does not fit its session's context)."""
        ptrs, tokens, counts = self._packed(sessions, prompts)
        rc = _lib().llm_feed_prompt_batch(self.ptr, ptrs, len(sessions), tokens.ctypes.data, counts.ctypes.data, int(max_rows))
        if rc < 0:
            raise ValueError("llm_feed_prompt_batch: bad arguments (nothing was evaluated)")
        return int(rc)

    def prompt_pack(self, sessions, prompts):
        """Test hook: ONE call of ggml_hip_prompt_pack over all the prompts (llm_prompt_pack; at most 64 sessions), no rounds and no
        fallback.  Returns (rc, logits, embeddings): rc 0 = it ran — logits[i] is [len(prompts[i]), n_vocab], embeddings[i] the
        final-norm row of session i's last token — or -1 = bad arguments or the backend declined: nothing moved, the rest is None."""
        ptrs, tokens, counts = self._packed(sessions, prompts)
        V, E = self.hp["n_vocab"], self.hp["n_embd"]
        logits = np.zeros((int(counts.sum()), V), np.float32)
        emb = np.zeros((len(sessions), E), np.float32)
        rc = _lib().llm_prompt_pack(self.ptr, ptrs, len(sessions), tokens.ctypes.data, counts.ctypes.data, logits.ctypes.data, emb.ctypes.data)
        if rc != 0:
            return -1, None, None
        ends = np.cumsum(counts)
        return 0, [logits[e - c:e] for c, e in zip(counts, ends)], [emb[i] for i in range(len(sessions))]

    def free(self):
        if self.ptr:
            _lib().llm_model_free(self.ptr)
            self.ptr = None


class Session:
    def __init__(self, model, n_batch, kv_type, slot=-1):
        self.model = model
        cfg = _SC(kv_type, kv_type, n_batch, 8)
        self.ptr = (_lib().llm_start_session(model.ptr, C.byref(cfg)) if slot < 0 else
                    _lib().llm_start_session_on(model.ptr, C.byref(cfg), slot))

    def seek(self, n_past):
        """The session continues at position n_past (the caller has put the K/V before it in place: set_kv)."""
        _lib().llm_session_seek(self.ptr, int(n_past))

    def set_speculate(self, on):
        """False = the reference's own call sequence per token (build the graph, then ggml_graph_compute); True = the next
        token's graph is built between ggml_hip_graph_compute_begin / _end while the device runs."""
        _lib().llm_session_set_speculate(self.ptr, 1 if on else 0)

    @property
    def n_past(self):
        return _lib().llm_session_n_past(self.ptr)

    def evaluate(self, tokens, want_all_logits=True, want_embeddings=False):
        """Model::evaluate: returns all logits [N, n_vocab] (OutputRequest.all_logits) if requested."""
        tokens = np.ascontiguousarray(tokens, dtype=np.int32)
        V, E = self.model.hp["n_vocab"], self.model.hp["n_embd"]
        if not self.model.is_last:
            want_all_logits = want_embeddings = False
        logits = np.zeros((tokens.size, V), np.float32) if want_all_logits else None
        emb = np.zeros(E, np.float32) if want_embeddings else None
        _lib().llm_evaluate(self.model.ptr, self.ptr, tokens.ctypes.data, tokens.size,
                            logits.ctypes.data if logits is not None else None,
                            emb.ctypes.data if emb is not None else None)
        if want_embeddings:
            return logits, emb
        return logits

    def feed_prompt(self, tokens):
        tokens = np.ascontiguousarray(tokens, dtype=np.int32)
        _lib().llm_feed_prompt(self.model.ptr, self.ptr, tokens.ctypes.data, tokens.size)

    def stage_rows(self, tokens):
        """Test hook: this session's graph for `tokens` at its n_past, built as evaluate builds it and NOT computed (llm_session_stage_rows);
        returns the ggml_cgraph pointer for ggml.prompt_pack.  The session does not move."""
        tokens = np.ascontiguousarray(tokens, dtype=np.int32)
        return _lib().llm_session_stage_rows(self.model.ptr, self.ptr, tokens.ctypes.data, tokens.size)

    def infer_next_token(self):
        return int(_lib().llm_infer_next_token_greedy(self.model.ptr, self.ptr))

    def infer_next_token_topk(self, rng, k=40, temperature=0.8, device_topk=True):
        """One token step with the shape of the reference's default sampler (llm_infer_next_token_topk); rng: ctypes c_uint64 state."""
        return int(_lib().llm_infer_next_token_topk(self.model.ptr, self.ptr, k, temperature, C.byref(rng), 1 if device_topk else 0))

    def snapshot(self):
        """InferenceSession::get_snapshot as bytes (npast, config, tokens, last_logits, memory_k, memory_v)."""
        n = _lib().llm_session_snapshot(self.ptr, None, 0)
        buf = np.zeros(n, np.uint8)
        _lib().llm_session_snapshot(self.ptr, buf.ctypes.data, n)
        return buf.tobytes()

    def infer_tokens_device(self, n):
        """n greedy tokens sampled on the device (llm_infer_tokens_greedy_device); returns their ids."""
        out = np.zeros(n, np.int32)
        _lib().llm_infer_tokens_greedy_device(self.model.ptr, self.ptr, n, out.ctypes.data)
        return out

    def infer_next_token_sampled(self, rng, k=40, top_p=0.95, temperature=0.8, penalty=1.30, mu=None, **extras):
        """One token step of a caller that samples (llm_infer_next_token_sampled): sample_exact on last_logits and the last 64 tokens
        of the history, the id appended and evaluated.  rng: a uint64 array of one element, stepped in place.  ValueError, with
        nothing moved, on sample_exact's bad arguments.  extras: sampler_chain's further keywords (freq, presence, tail_free_z,
        typical_p, min_p, bias, mirostat, tau, eta; neutral by default — sample_chain draws); mu: Mirostat 2's state, a float32 array
        of one element advanced in place like rng."""
        rng = Llama._rngs(rng, 1)
        prm = sampler_chain(k, top_p, temperature, penalty, **extras)
        rc = _lib().llm_infer_next_token_sampled_chain(self.model.ptr, self.ptr, C.addressof(prm), rng.ctypes.data, _mu(mu, 1, prm))
        if rc < 0:
            raise ValueError("llm_infer_next_token_sampled: bad arguments (nothing was evaluated)")
        return int(rc)

    def infer_tokens_sampled_device(self, n, rng, k=40, top_p=0.95, temperature=0.8, penalty=1.30, mu=None, **extras):
        """n such tokens drawn on the device where the backend can (llm_infer_tokens_sampled_device: no logits read-back and no host
        round trip per token; k <= 256); anything else runs as infer_next_token_sampled, with the same ids, session and generator
        state.  Returns (n_on_device, ids): n behind a single-token step, n - 1 behind a prompt, 0 when the backend declined.
        ValueError as above, and for n < 1 or a session without room for n tokens.  extras and mu as above (Mirostat 2 on the
        device: n_vocab <= 32768)."""
        rng = Llama._rngs(rng, 1)
        prm = sampler_chain(k, top_p, temperature, penalty, **extras)
        out = np.zeros(max(int(n), 0), np.int32)
        rc = _lib().llm_infer_tokens_sampled_chain_device(self.model.ptr, self.ptr, int(n), C.addressof(prm), rng.ctypes.data,
                                                          _mu(mu, 1, prm), out.ctypes.data)
        if rc < 0:
            raise ValueError("llm_infer_tokens_sampled_device: bad arguments (nothing was evaluated)")
        return int(rc), out

    def infer_until(self, max_tokens, rng, stop=(), mu=None, **sampler):
        """Generation that stops, as InferenceSession::infer (llm_infer_until): draw and evaluate until the token is one of `stop` (up
        to 8 ids; it is still evaluated), max_tokens were drawn or the context is full.  sampler: sampler_chain's keywords; with
        rng None (and no keywords) the first maximum is taken.  On the device where the backend can — the chain ends by itself and
        leaves the session where the stop token's evaluation left it — otherwise the stepped loop with the same rule: same ids,
        session, generator state and mu.  Returns (ids, count, reason, ran_chained) with reason "budget", "stop" or "context".
        ValueError with nothing moved on bad arguments."""
        if rng is None and sampler:
            raise ValueError("infer_until: a sampler needs rng, a uint64 array of one element")
        req, chain = until_request(max_tokens, stop, None if rng is None else sampler)
        if rng is not None:
            rng = Llama._rngs(rng, 1)
        out = np.full(max(int(max_tokens), 0), -1, np.int32)
        count, why = C.c_int32(0), C.c_int32(0)
        rc = _lib().llm_infer_until(self.model.ptr, self.ptr, C.addressof(req), None if rng is None else rng.ctypes.data,
                                    None if chain is None else _mu(mu, 1, chain), out.ctypes.data, C.addressof(count), C.addressof(why))
        if rc < 0:
            raise ValueError("llm_infer_until: bad arguments (nothing was evaluated)")
        return out[:count.value], int(count.value), ENDED_BY[int(why.value)], bool(rc)

    @staticmethod
    def host_timing(reset=False):
        """Accumulated host ns per phase of the decode loop (llm_host_timing)."""
        a = (C.c_double * 8)()
        _lib().llm_host_timing(a, 1 if reset else 0)
        return list(a)

    def rewind(self, num):
        return _lib().llm_session_rewind(self.ptr, num)

    def last_logits(self):
        V = self.model.hp["n_vocab"]
        return np.ctypeslib.as_array(_lib().llm_session_last_logits(self.ptr), shape=(V,)).copy()

    def stage_buffers(self):
        """(in_dev_ptr, out_dev_ptr, nbytes) of the layer-split residual hand-off buffers (None if absent)."""
        a, b, n = C.c_void_p(0), C.c_void_p(0), C.c_size_t(0)
        _lib().llm_session_stage_buffers(self.ptr, C.byref(a), C.byref(b), C.byref(n))
        return a.value, b.value, n.value

    def get_kv(self, dtype=np.uint16):
        """(memory_k, memory_v) raw contents — the InferenceSnapshot payload."""
        out = []
        for which in (0, 1):
            n = _lib().llm_session_kv(self.ptr, which, 0, None, 0)
            a = np.zeros(n // np.dtype(dtype).itemsize, dtype=dtype)
            _lib().llm_session_kv(self.ptr, which, 0, a.ctypes.data, a.nbytes)
            out.append(a)
        return out

    def set_kv(self, k, v):
        for which, a in ((0, k), (1, v)):
            a = np.ascontiguousarray(a)
            _lib().llm_session_kv(self.ptr, which, 1, a.ctypes.data, a.nbytes)

    def top_k(self, k, extra_ids=()):
        """(values, ids) of the k largest logits of the last evaluated token, best first (lower id first on ties), then
        the raw logits of extra_ids — computed on the device (llm_session_topk); only k + len(extra_ids) pairs are
        read back."""
        extra = np.ascontiguousarray(extra_ids, dtype=np.int32)
        vals = np.zeros(k + extra.size, dtype=np.float32)
        ids = np.zeros(k + extra.size, dtype=np.int32)
        rc = _lib().llm_session_topk(self.ptr, k, extra.ctypes.data if extra.size else None, extra.size, vals.ctypes.data,
                                     ids.ctypes.data)
        if rc != 0:
            raise ValueError("llm_session_topk: no evaluated graph or bad arguments")
        return vals, ids

    def perplexity(self, tokens, bos=1, on_device=True, return_probs=False):
        """InferenceSession::perplexity (inference_session.rs:519-589): one value per chunk of context_size tokens, each the
        RUNNING exp(nll / count) the reference hands to its callback; `bos` replaces the first token of every chunk for the
        evaluation.  on_device: the logits stay in HBM and the device reduces each counted row to its target's probability
        (ggml_hip_row_probs); False: all logits are read back and softmaxed on the host, as the reference does.
        return_probs: also the probability of every counted position, [n_chunk, context_size - 1 - min(512, context_size / 2)]."""
        tokens = np.ascontiguousarray(tokens, dtype=np.int32)
        ctx = self.model.context_size
        n_chunk = tokens.size // ctx
        per_chunk = max(ctx - 1 - min(512, ctx // 2), 0)
        ppl = np.zeros(max(n_chunk, 1), np.float32)
        probs = np.zeros((max(n_chunk, 1), per_chunk), np.float32)
        rc = _lib().llm_session_perplexity(self.model.ptr, self.ptr, tokens.ctypes.data, tokens.size, int(bos), 1 if on_device else 0,
                                           ppl.ctypes.data, n_chunk, probs.ctypes.data if return_probs else None)
        if rc != n_chunk:
            raise ValueError("llm_session_perplexity: a token id outside the vocabulary, or no logits on the device")
        out = [float(x) for x in ppl[:n_chunk]]
        return (out, probs[:n_chunk]) if return_probs else out

    def read_node(self, index=-1, name=None, occurrence=0, dtype=np.float32):
        """Test hook: device contents of a node of the last evaluated graph, by index (negative: from the end, -1 = the last
        node, the logits) or by name."""
        nm = name.encode() if name else None
        if nm is None and index < 0:
            index += self.graph_stats()[0]
        n = _lib().llm_session_read_node(self.ptr, index, nm, occurrence, None, 0)
        if n == 0:
            raise KeyError((index, name, occurrence))
        out = np.zeros(n // np.dtype(dtype).itemsize, dtype=dtype)
        _lib().llm_session_read_node(self.ptr, index, nm, occurrence, out.ctypes.data, out.nbytes)
        return out

    def read_node_host(self, from_end, dtype=np.float32):
        """Test hook: the HOST bytes of node n_nodes - 1 - from_end of the last evaluated graph (tensor->data)."""
        n = _lib().llm_session_read_node_host(self.ptr, from_end, None, 0)
        out = np.zeros(n // np.dtype(dtype).itemsize, dtype=dtype)
        _lib().llm_session_read_node_host(self.ptr, from_end, out.ctypes.data, out.nbytes)
        return out

    def graph_stats(self):
        a, b = C.c_int(0), C.c_int(0)
        _lib().llm_session_last_graph_stats(self.ptr, C.byref(a), C.byref(b))
        return a.value, b.value

    def free(self):
        if self.ptr:
            _lib().llm_session_free(self.ptr)
            self.ptr = None
