"""CPU: k_sha1_gather_lat's compiled gfx950 code: exactly two
instantiations, no scratch, the LDS DESIGN states (SLOTS x 20 KiB of W+K slots
+ 512 bytes of published block counts), and a round wave whose loop does
k_sha1_lat's work per block.  Reads resources and instruction counts only."""
import collections
import importlib.util
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = {2: "_ZN6btsha117k_sha1_gather_latILi2EE", 3: "_ZN6btsha117k_sha1_gather_latILi3EE"}
LDS = {2: 2 * 20480 + 512, 3: 3 * 20480 + 512}


def _isa_mix():
    spec = importlib.util.spec_from_file_location("isa_mix", os.path.join(REPO, "tools", "isa_mix.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def text(tmp_path_factory):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc absent")
    out = str(tmp_path_factory.mktemp("isa_gather_lat") / "k.s")
    _isa_mix().compile_asm(out)
    return open(out).read()


def _symbols(text):
    return sorted(set(re.findall(r"^(_ZN6btsha1\d+k_sha1_gather_lat\w*):", text, re.M)))


def _info(text, sym):
    body = text[text.index(sym + ":"):]
    body = body[body.index(".Lfunc_end"):]
    body = body[:body.index(".amdhsa_kernel") if ".amdhsa_kernel" in body else len(body)]
    return {k: int(v) for k, v in re.findall(r"; (ScratchSize|LDSByteSize|NumVgprs|NumAgprs|codeLenInByte)[:= ]+(\d+)",
                                             body)}


def _loops(text, sym):
    """(label, body) of every innermost loop of kernel `sym` (tests/test_isa.py's counting)."""
    body = text[text.index(sym + ":"):]
    body = body[:body.index(".Lfunc_end")]
    out = []
    for m in re.finditer(r"^(\.LBB\d+_\d+):[^\n]*(?:\n\s*;[^\n]*)?Inner Loop Header", body, re.M):
        label = m.group(1)
        end = re.search(r"s_cbranch_\w+ " + re.escape(label) + r"\b", body[m.end():])
        if end:
            out.append((label, body[m.end():m.end() + end.start()]))
    return out


def _ops(loop):
    return collections.Counter(l.strip().split()[0] for l in loop.splitlines()
                               if l.strip() and not l.strip().startswith((".", ";")))


def test_exactly_two_instantiations(text):
    syms = _symbols(text)
    assert len(syms) == 2, syms
    assert all(any(s.startswith(p) for s in syms) for p in SYMS.values()), syms


@pytest.mark.parametrize("slots", [2, 3])
def test_resources(text, slots):
    sym = [s for s in _symbols(text) if s.startswith(SYMS[slots])][0]
    info = _info(text, sym)
    print(f"k_sha1_gather_lat<{slots}>: {info}")
    assert info["ScratchSize"] == 0, info
    assert info["LDSByteSize"] == LDS[slots], info
    assert info["NumVgprs"] <= 256, info


def test_round_wave_structure(text):
    """R's loop (2-slot form, counted as test_latency_kernel_round_wave_structure
    counts k_sha1_lat's): one block per iteration, 20 ds_read_b128 from one
    slot, one s_barrier, 160 v_alignbit_b32 + 80 v_bitop3_b32, and 405 VALU of
    round work (5 per round + the 5 state adds).  The per-lane latch at the
    lane's own last block, which k_sha1_lat has not and k_sha1_lat_ragged has
    (its test allows 10 VALU for it), is counted apart: it is the loop's only
    compares and selects, at most 10 of them."""
    sym = [s for s in _symbols(text) if s.startswith(SYMS[2])][0]
    r_loops = [b for _, b in _loops(text, sym) if "ds_read_b128" in b]
    assert len(r_loops) == 1, len(r_loops)
    ops = _ops(r_loops[0])
    valu = sum(v for k, v in ops.items() if k.startswith("v_"))
    latch = sum(v for k, v in ops.items() if k.startswith(("v_cmp", "v_cndmask")))
    print(f"R loop: {valu} VALU of which latch {latch}; {dict(ops)}")
    assert valu - latch == 405, ops
    assert latch <= 10, ops
    assert ops["ds_read_b128"] == 20 and ops["s_barrier"] == 1, ops
    assert ops["v_alignbit_b32"] == 160 and ops["v_bitop3_b32"] == 80, ops
    assert not any(k.startswith(("global_load", "flat_load", "buffer_load")) for k in ops), ops


def test_three_slot_round_wave(text):
    """The 3-slot form's R runs two blocks per trip from registers, as
    k_sha1_lat_ragged<3>: 20 ds_read_b128 ahead of the loop and 20 per block
    in it (60 in the kernel, all R's: S only writes LDS), 160 v_bitop3_b32 of
    round work (80 per block; S's schedule has the other 64), no scratch."""
    sym = [s for s in _symbols(text) if s.startswith(SYMS[3])][0]
    body = text[text.index(sym + ":"):]
    ops = _ops(body[:body.index(".Lfunc_end")])
    assert ops["ds_read_b128"] == 60 and ops["ds_write_b128"] == 20, ops
    assert ops["v_bitop3_b32"] == 64 + 160, ops


@pytest.mark.parametrize("slots", [2, 3])
def test_loader_wave_keeps_a_block_in_flight(text, slots):
    """S's loop: the five 16-byte loads of block b + 1 are issued, then
    produce_block of block b runs (20 ds_write_b128) up to the block's
    s_barrier with NO vmcnt wait in between; the first wait behind the barrier
    is vmcnt(5) or more, i.e. it waits for the descriptor asked for ahead of
    the five and leaves them outstanding."""
    sym = [s for s in _symbols(text) if s.startswith(SYMS[slots])][0]
    body = text[text.index(sym + ":"):]
    lines = [l.strip() for l in body[:body.index(".Lfunc_end")].splitlines()]
    lines = [l for l in lines if l and not l.startswith((".", ";"))]
    found = []
    for i in range(len(lines) - 5):
        if all(l.startswith("global_load_dwordx4") for l in lines[i:i + 5]) and \
                not lines[i + 5].startswith("global_load_dwordx4"):
            writes, j = 0, i + 5
            while j < len(lines) and not lines[j].startswith(("s_barrier", "s_waitcnt vmcnt", "s_cbranch")):
                writes += lines[j].startswith("ds_write_b128")
                j += 1
            if j < len(lines) and lines[j].startswith("s_barrier") and writes == 20:
                wait = next(l for l in lines[j:] if l.startswith("s_waitcnt vmcnt"))
                found.append(int(re.match(r"s_waitcnt vmcnt\((\d+)\)", wait).group(1)))
    print(f"k_sha1_gather_lat<{slots}>: first waits behind the block barrier {found}")
    assert len(found) == 1 and found[0] >= 5, found
