"""CPU: the resumable chain kernel's compiled gfx950 code keeps the chain
kernel's round wave: every instantiation of k_sha1_resume has
exactly one round loop, with two ds_read_b128 per block and one DPP-fed add
per round (~405 VALU), and the kernel uses no scratch."""
import collections
import importlib.util
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESUME = "_ZN6btsha113k_sha1_resumeILb%dEE"  # k_sha1_resume<VERIFY>


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc absent")
    mod = _load("isa_mix", os.path.join(REPO, "tools", "isa_mix.py"))
    out = str(tmp_path_factory.mktemp("isa_resume") / "k.s")
    mod.compile_asm(out)
    return open(out).read()


def _symbols(text):
    return sorted(set(re.findall(r"^(_ZN6btsha113k_sha1_resume\w*):", text, re.M)))


def _loops(text, sym):
    """(header label, body text) of every innermost loop of kernel `sym` (as tests/test_isa.py)."""
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
    assert len(syms) == 2 and syms[0].startswith(RESUME % 0) and syms[1].startswith(RESUME % 1), syms


@pytest.mark.parametrize("verify", [0, 1])
def test_resume_kernel_round_wave_structure(asm, verify):
    sym = [s for s in _symbols(asm) if s.startswith(RESUME % verify)]
    assert len(sym) == 1, sym
    loops = [b for _, b in _loops(asm, sym[0]) if "v_alignbit_b32" in b]
    assert len(loops) == 1, len(loops)
    ops = collections.Counter(l.strip().split()[0] for l in loops[0].splitlines()
                              if l.strip() and not l.strip().startswith((".", ";")))
    valu = sum(v for k, v in ops.items() if k.startswith("v_"))
    assert 405 <= valu <= 410, ops
    assert ops["ds_read_b128"] == 2 and ops["v_add_u32_dpp"] >= 70, ops
    assert ops["v_alignbit_b32"] == 160 and ops["v_bitop3_b32"] == 80, ops


@pytest.mark.parametrize("verify", [0, 1])
def test_resume_kernel_uses_no_scratch(asm, verify):
    sym = [s for s in _symbols(asm) if s.startswith(RESUME % verify)][0]
    meta = asm[asm.index(sym + ":"):]
    assert int(re.search(r"; ScratchSize: (\d+)", meta).group(1)) == 0
    assert int(re.search(r"; LDSByteSize: (\d+)", meta).group(1)) == 2 * 21 * 64 * 16  # two 21 KiB slots of 64 blocks
