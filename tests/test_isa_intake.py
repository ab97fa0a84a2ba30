"""CPU: the table-driven form of the resumable chain kernel keeps
k_sha1_resume's round wave in its compiled gfx950 code: every
instantiation of k_sha1_resume_table has exactly one round loop, with 408 VALU,
two ds_read_b128 and 71 DPP-fed adds per block, no scratch and the two 21 KiB
LDS slots."""
import collections
import importlib.util
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = "_ZN6btsha119k_sha1_resume_tableILb%dEE"  # k_sha1_resume_table<VERIFY>


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    assert os.path.exists("/opt/rocm/bin/hipcc"), "the ISA checks need hipcc"
    mod = _load("isa_mix", os.path.join(REPO, "tools", "isa_mix.py"))
    out = str(tmp_path_factory.mktemp("isa_intake") / "k.s")
    mod.compile_asm(out)
    return open(out).read()


def _symbols(text):
    return sorted(set(re.findall(r"^(_ZN6btsha119k_sha1_resume_table\w*):", text, re.M)))


def _loops(text, sym):
    """(header label, body text) of every innermost loop of kernel `sym` (as tests/test_isa_resume.py)."""
    body = text[text.index(sym + ":"):]
    body = body[:body.index(".Lfunc_end")]
    out = []
    for m in re.finditer(r"^(\.LBB\d+_\d+):[^\n]*(?:\n\s*;[^\n]*)?Inner Loop Header", body, re.M):
        label = m.group(1)
        end = re.search(r"s_cbranch_\w+ " + re.escape(label) + r"\b", body[m.end():])
        if end:
            out.append((label, body[m.end():m.end() + end.start()]))
    return out


def test_both_instantiations_exist(asm):
    syms = _symbols(asm)
    assert len(syms) == 2 and syms[0].startswith(TABLE % 0) and syms[1].startswith(TABLE % 1), syms


@pytest.mark.parametrize("verify", [0, 1])
def test_table_kernel_round_wave_structure(asm, verify):
    sym = [s for s in _symbols(asm) if s.startswith(TABLE % verify)]
    assert len(sym) == 1, sym
    loops = [b for _, b in _loops(asm, sym[0]) if "v_alignbit_b32" in b]
    assert len(loops) == 1, len(loops)
    ops = collections.Counter(l.strip().split()[0] for l in loops[0].splitlines()
                              if l.strip() and not l.strip().startswith((".", ";")))
    valu = sum(v for k, v in ops.items() if k.startswith("v_"))
    print("VALU", valu, dict(ops))
    assert valu == 408, ops
    assert ops["ds_read_b128"] == 2 and ops["v_add_u32_dpp"] == 71, ops
    assert ops["v_alignbit_b32"] == 160 and ops["v_bitop3_b32"] == 80, ops


@pytest.mark.parametrize("verify", [0, 1])
def test_table_kernel_uses_no_scratch_and_two_lds_slots(asm, verify):
    sym = [s for s in _symbols(asm) if s.startswith(TABLE % verify)][0]
    meta = asm[asm.index(sym + ":"):]
    assert int(re.search(r"; ScratchSize: (\d+)", meta).group(1)) == 0
    assert int(re.search(r"; LDSByteSize: (\d+)", meta).group(1)) == 43008  # two 21 KiB slots of 64 blocks
    print("NumVgprs", re.search(r"; NumVgprs: (\d+)", meta).group(1))

