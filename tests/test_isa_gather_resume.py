"""CPU: the chain-form gather kernels keep k_sha1_resume's round wave in their
compiled gfx950 code: both instantiations of
k_sha1_gather_resume and of k_sha1_gather_resume_table have exactly one round
loop, with 408 VALU, two ds_read_b128, 71 DPP-fed adds, 160 v_alignbit_b32 and
80 v_bitop3_b32 per block -- the same chain_rounds -- no scratch (the S wave's
gather_words selects stay in registers) and the two 21 KiB LDS slots."""
import collections
import importlib.util
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {"array": "_ZN6btsha120k_sha1_gather_resumeILb%dEE",        # k_sha1_gather_resume<VERIFY>
           "table": "_ZN6btsha126k_sha1_gather_resume_tableILb%dEE"}  # k_sha1_gather_resume_table<VERIFY>
CASES = [(form, verify) for form in KERNELS for verify in (0, 1)]


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    assert os.path.exists("/opt/rocm/bin/hipcc"), "the ISA checks need hipcc"
    mod = _load("isa_mix", os.path.join(REPO, "tools", "isa_mix.py"))
    out = str(tmp_path_factory.mktemp("isa_gather_resume") / "k.s")
    mod.compile_asm(out)
    return open(out).read()


def _symbols(text):
    return sorted(set(re.findall(r"^(_ZN6btsha12[06]k_sha1_gather_resume\w*):", text, re.M)))


def _symbol(text, form, verify):
    sym = [s for s in _symbols(text) if s.startswith(KERNELS[form] % verify)]
    assert len(sym) == 1, sym
    return sym[0]


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


def test_both_instantiations_of_both_kernels_exist(asm):
    syms = _symbols(asm)
    assert len(syms) == 4, syms
    for form, verify in CASES:
        _symbol(asm, form, verify)


@pytest.mark.parametrize("form,verify", CASES)
def test_round_wave_structure(asm, form, verify):
    loops = [b for _, b in _loops(asm, _symbol(asm, form, verify)) if "v_alignbit_b32" in b]
    assert len(loops) == 1, len(loops)
    ops = collections.Counter(l.strip().split()[0] for l in loops[0].splitlines()
                              if l.strip() and not l.strip().startswith((".", ";")))
    valu = sum(v for k, v in ops.items() if k.startswith("v_"))
    print("VALU", valu, dict(ops))
    assert valu == 408, ops
    assert ops["ds_read_b128"] == 2 and ops["v_add_u32_dpp"] == 71, ops
    assert ops["v_alignbit_b32"] == 160 and ops["v_bitop3_b32"] == 80, ops


@pytest.mark.parametrize("form,verify", CASES)
def test_no_scratch_and_two_lds_slots(asm, form, verify):
    sym = _symbol(asm, form, verify)
    meta = asm[asm.index(sym + ":"):]
    assert int(re.search(r"; ScratchSize: (\d+)", meta).group(1)) == 0
    assert int(re.search(r"; LDSByteSize: (\d+)", meta).group(1)) == 43008  # two 21 KiB slots of 64 blocks
    print("NumVgprs", re.search(r"; NumVgprs: (\d+)", meta).group(1),
          "NumAgprs", re.search(r"; NumAgprs: (\d+)", meta).group(1))
