"""CPU: resources of the gather kernels in the gfx950 ISA hipcc emits -- both
symbols exist, no scratch memory, no LDS, no barrier.  Resources only: the
listing is not searched for particular instructions."""
import os
import re
import sys

import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))
import isa_mix  # noqa: E402

KERNELS = ("k_sha1_gather", "k_sha1_gather_verify")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa_gather") / "k.s"
    isa_mix.compile_asm(str(out))
    return out.read_text()


@pytest.mark.parametrize("kernel", KERNELS)
def test_gather_kernel_resources(asm, kernel):
    syms = re.findall(r"^(_ZN6btsha1\d+%sE\w*):" % kernel, asm, re.M)
    assert len(syms) == 1, syms
    body = asm[asm.index(syms[0] + ":"):]
    code = body[:body.index(".Lfunc_end")]
    meta = body[:body.index("; Occupancy")]
    vgprs = int(re.search(r"; NumVgprs: (\d+)", meta).group(1))
    print(f"{kernel}: NumVgprs {vgprs}")
    assert int(re.search(r"; ScratchSize: (\d+)", meta).group(1)) == 0
    assert int(re.search(r"; LDSByteSize: (\d+)", meta).group(1)) == 0
    assert "s_barrier" not in code
    assert vgprs <= 256
