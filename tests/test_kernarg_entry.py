"""What a workgroup of the block-format decode launches waits for before it may ask for its first byte, read from the built library.

A scalar load of a 64-byte line of the kernarg segment that no earlier load of the workgroup has touched is a scalar-cache miss, and every
`s_waitcnt lgkmcnt(0)` behind a batch of such loads is a dependent round trip in front of the activation's loads or of the weight stream
(DESIGN.md section 4.2 "Kernarg lines"; kernels/decode_big.h BigArgs).  For the Q4_0 production instantiations of k_mmvq_big (w1|w3, w2,
lm_head), k_qkv_attn and k_qkv_attn_wo this walks the gfx950 disassembly from the kernel's first instruction (in the fused kernels: along
the side of the first branch that the mat-vec workgroups take) to the first `global_load` (the activation) and on to the first non-temporal load (the
weight stream), and holds the batches of kernarg loads to the shapes the layout was built for:

  k_mmvq_big      one wait before the activation's loads; its batch reads lines 0x00 and 0x40 and no other; no kernarg load at all between
                  that wait and the first weight request; the kernel has no hidden arguments (neither blockDim nor gridDim is read)
  fused kernels   two waits before the activation's loads; the second batch, and whatever is loaded up to the first weight request, reads
                  only lines the first batch read; the first batch reads lines 0x00, 0x40, 0x80 of BigArgs; no load from the hidden line

The limits are what hipcc gives for the layout as committed.  No GPU: the library is only read."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "llm_amd", "libggml_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"
BIG_ARGS_BYTES = 384  # sizeof(BigArgs), pinned by a static_assert next to the struct

GATE = "_Z10k_mmvq_bigILi0ELi2ELi1ELb0EEv7BigArgs"   # <Q4_0, EPI_GATE, XSRC_NORM>: w1|w3
DOWN = "_Z10k_mmvq_bigILi0ELi1ELi2ELb0EEv7BigArgs"   # <Q4_0, EPI_ADD, XSRC_F32>: w2
HEAD = "_Z10k_mmvq_bigILi0ELi0ELi1ELb0EEv7BigArgs"   # <Q4_0, EPI_STORE, XSRC_NORM>: lm_head
FUSED = "_Z10k_qkv_attnILi0ELb0EEv7BigArgs13FusedAttnArgs"
FUSED_WO = "_Z13k_qkv_attn_woILi0ELi2EEv7BigArgs13FusedAttnArgs10WoTailArgs"


def _tool(name):
    p = os.path.join(LLVM, name)
    return p if os.path.exists(p) else shutil.which(name)


@pytest.fixture(scope="module")
def code_object(tmp_path_factory):
    """the first gfx950 code object inside the library (hip_backend.hip's), as tests/tools/disasm.py takes it out"""
    if not _tool("llvm-objdump") or not _tool("llvm-readelf"):
        pytest.skip("llvm-objdump / llvm-readelf not found")
    if not os.path.exists(SO):
        pytest.fail("llm_amd/libggml_hip.so is not built")
    data = open(SO, "rb").read()
    for m in re.finditer(b"\x7fELF", data):
        i = m.start()
        if i and int.from_bytes(data[i + 18:i + 20], "little") == 0xE0:  # EM_AMDGPU
            shoff = int.from_bytes(data[i + 0x28:i + 0x30], "little")
            size = shoff + int.from_bytes(data[i + 0x3A:i + 0x3C], "little") * int.from_bytes(data[i + 0x3C:i + 0x3E], "little")
            path = tmp_path_factory.mktemp("co") / "hip_backend.co"
            path.write_bytes(data[i:i + size])
            return str(path)
    pytest.fail("no gfx950 code object in the library")


@pytest.fixture(scope="module")
def notes(code_object):
    return subprocess.run([_tool("llvm-readelf"), "--notes", code_object], capture_output=True, text=True, check=True).stdout


def _instructions(code_object, kernel):
    out = subprocess.run([_tool("llvm-objdump"), "-d", "--mcpu=gfx950", "--disassemble-symbols=" + kernel, code_object],
                         capture_output=True, text=True, check=True).stdout
    lines = [l for l in out.splitlines() if l.startswith("\t")]
    assert len(lines) > 100, f"{kernel}: not in the code object"
    return _mat_vec_path(lines)


def _mat_vec_path(lines):
    """The instructions a mat-vec workgroup runs, in order, up to where the walk ends.  k_mmvq_big: the kernel as it stands.  The fused
    kernels decide attention or mat-vec by comparing blockIdx.x (s2) with BigArgs::n_attn in front of their first conditional branch;
    the mat-vec side (blockIdx.x >= n_attn) is followed whichever way hipcc laid the two out, and a first branch of any other form
    fails here rather than let the walk count the attention workgroups' loads."""
    text = [l.split("//")[0].strip() for l in lines]
    first = next(i for i, t in enumerate(text) if t.startswith("s_cbranch"))
    cmps = [t for t in text[:first] if re.match(r"s_cmp_\w+ s2, s\d+$", t)]
    if not cmps:
        return text  # no comparison of the workgroup index in front of the first branch: not a fused kernel
    m = re.match(r"s_cmp_(ge|lt)_i32 s2, s\d+$", cmps[-1])
    b = re.match(r"s_cbranch_scc([01]) ", text[first])
    assert m and b, (cmps[-1], text[first])
    taken_is_mat_vec = (m.group(1) == "ge") == (b.group(1) == "1")
    if not taken_is_mat_vec:
        return text
    target = re.search(r"<[^>]*\+0x([0-9a-f]+)>", lines[first])
    addr = [int(re.search(r"// ([0-9A-F]+):", l).group(1), 16) for l in lines]
    assert target, lines[first]
    to = addr[0] + int(target.group(1), 16)
    assert to in addr, lines[first]
    return text[:first] + text[addr.index(to):]


def _entry(ins):
    """-> (batches before the first global_load, kernarg loads between that and the first nt load): a batch = the kernarg offsets of the
    scalar loads a `s_waitcnt lgkmcnt` waits for; scalar loads off other pointers (DecParams, the epoch) are none of this test's."""
    bases = {"s[0:1]": 0}  # the kernarg pointer, and pointers into the segment derived from it (s_add_u32 sN, s0, imm)
    batches, cur, later, seen_x = [], [], [], False
    for t in ins:
        m = re.match(r"s_add_u32 s(\d+), s0, (0x[0-9a-f]+|\d+)$", t)
        if m:
            bases["s[%d:%d]" % (int(m.group(1)), int(m.group(1)) + 1)] = int(m.group(2), 0)
        m = re.match(r"s_load_dword(x\d+)? (\S+), (s\[\d+:\d+\]), (0x[0-9a-f]+|\d+)", t)
        if m and m.group(3) in bases:
            n = int((m.group(1) or "x1")[1:]) * 4
            off = bases[m.group(3)] + int(m.group(4), 0)
            (later if seen_x else cur).append((off, n))
        elif t.startswith("s_waitcnt") and "lgkmcnt" in t and cur and not seen_x:
            batches.append(cur)
            cur = []
        elif t.startswith("global_load"):
            if t.endswith(" nt"):
                return batches, cur, later
            if not seen_x:
                seen_x = True
    raise AssertionError("no non-temporal load found")


def _lines(loads):
    return {o // 64 * 64 for off, n in loads for o in (off, off + n - 1)}


def _fmt(batches):
    return [[hex(o) for o, _ in b] for b in batches]


def _hidden_args(notes, kernel):
    at = notes.index(".name:           " + kernel + "\n")
    return re.findall(r"hidden_\w+", notes[notes.rindex("\n  - ", 0, at):at])


@pytest.mark.parametrize("kernel", [GATE, DOWN, HEAD], ids=["gate_norm", "add_f32", "store_norm"])
def test_mmvq_big_enters_on_one_round_trip_over_two_lines(code_object, notes, kernel):
    batches, pending, later = _entry(_instructions(code_object, kernel))
    print(kernel, _fmt(batches), "pending at x:", pending, "up to the first weight request:", later)
    assert batches and batches[0], "no kernarg load found: is the kernarg pointer still s[0:1]?"
    assert len(batches) == 1, _fmt(batches)
    assert _lines(batches[0]) == {0x00, 0x40}, _fmt(batches)
    assert not pending and not later, (pending, later)
    assert max(o + n for o, n in batches[0]) <= BIG_ARGS_BYTES
    assert _hidden_args(notes, kernel) == []


@pytest.mark.parametrize("kernel", [FUSED, FUSED_WO], ids=["k_qkv_attn", "k_qkv_attn_wo"])
def test_fused_mat_vec_path_enters_on_two_waits_the_second_a_hit(code_object, notes, kernel):
    batches, pending, later = _entry(_instructions(code_object, kernel))
    print(kernel, _fmt(batches), "pending at x:", pending, "up to the first weight request:", later)
    assert batches and batches[0], "no kernarg load found: is the kernarg pointer still s[0:1]?"
    assert len(batches) == 2, _fmt(batches)
    first = _lines(batches[0])
    assert {0x00, 0x40, 0x80} <= first, _fmt(batches)
    assert _lines(batches[1]) <= {0x00, 0x40, 0x80}, _fmt(batches)
    assert _lines(pending) | _lines(later) <= first, (pending, later)
    # the hidden arguments, if the kernel has any, lie behind the explicit ones: nothing on this path reads them
    at = notes.index(".name:           " + kernel + "\n")
    block = notes[notes.rindex("\n  - ", 0, at):at]
    hidden = [int(o) for o in re.findall(r"\.offset:\s+(\d+)\n\s+\.size:\s+\d+\n\s+\.value_kind:\s+hidden_", block)]
    if hidden:
        assert max(o + n for b in batches + [pending, later] for o, n in b) <= min(hidden)
