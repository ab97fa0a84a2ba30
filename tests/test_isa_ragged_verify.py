"""CPU: the ragged kernels' verify forms in the compiled gfx950 code.  Each
ragged kernel exists without and with the fused compare -- k_sha1_ragged /
k_sha1_ragged_verify, k_sha1_lat_ragged<SLOTS> / k_sha1_lat_ragged_verify<SLOTS>
for 2 and 3 slots -- the latency forms use no scratch and exactly the LDS of
their non-verify form, and the compare adds no barrier to either wave (the
kernels are correct only while S and R execute nbmax + SLOTS - 1 each)."""
import importlib.util
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES = "_ZN6btsha113k_sha1_raggedEPKh"
LANES_VERIFY = "_ZN6btsha120k_sha1_ragged_verifyEPKh"
LAT = "_ZN6btsha117k_sha1_lat_raggedILi%dEE"
LAT_VERIFY = "_ZN6btsha124k_sha1_lat_ragged_verifyILi%dEE"


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    assert os.path.exists("/opt/rocm/bin/hipcc"), "the ISA checks need hipcc"
    mod = _load("isa_mix", os.path.join(REPO, "tools", "isa_mix.py"))
    out = str(tmp_path_factory.mktemp("isa_ragged_verify") / "k.s")
    mod.compile_asm(out)
    return open(out).read()


def _sym(text, prefix):
    found = sorted(set(re.findall(r"^(" + re.escape(prefix) + r"\w*):", text, re.M)))
    assert len(found) == 1, (prefix, found)
    return found[0]


def _body(text, sym):
    b = text[text.index(sym + ":"):]
    return b[:b.index(".Lfunc_end")]


def _meta(text, sym, key):
    return int(re.search(r"; %s: (\d+)" % key, text[text.index(sym + ":"):]).group(1))


def test_both_forms_of_each_ragged_kernel_exist(asm):
    for prefix in (LANES, LANES_VERIFY, LAT % 2, LAT % 3, LAT_VERIFY % 2, LAT_VERIFY % 3):
        _sym(asm, prefix)
    # the verify forms take the two extra pointers: expected (PKh again) and ok (Ph again)
    assert _sym(asm, LANES_VERIFY).endswith("PKhPKmPKjmjmPhS1_S6_")
    assert not re.findall(r"^_ZN6btsha1\d+k_sha1_lat_ragged_verifyILi[^23]", asm, re.M)


@pytest.mark.parametrize("slots", [2, 3])
def test_latency_verify_form_keeps_scratch_lds_and_barriers(asm, slots):
    plain, verify = _sym(asm, LAT % slots), _sym(asm, LAT_VERIFY % slots)
    assert _meta(asm, verify, "ScratchSize") == 0 and _meta(asm, plain, "ScratchSize") == 0
    lds = _meta(asm, plain, "LDSByteSize")
    assert lds == slots * 20 * 1024 and _meta(asm, verify, "LDSByteSize") == lds
    print("NumVgprs", _meta(asm, plain, "NumVgprs"), _meta(asm, verify, "NumVgprs"))
    assert _meta(asm, verify, "NumVgprs") <= 256
    # the compare sits after the last barrier: the same s_barrier sites as the plain form
    assert _body(asm, verify).count("s_barrier") == _body(asm, plain).count("s_barrier") > 0


def test_lane_verify_form_uses_no_scratch_and_no_lds(asm):
    plain, verify = _sym(asm, LANES), _sym(asm, LANES_VERIFY)
    for s in (plain, verify):
        assert _meta(asm, s, "ScratchSize") == 0 and _meta(asm, s, "LDSByteSize") == 0, s

