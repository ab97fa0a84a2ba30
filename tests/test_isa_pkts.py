"""CPU: facts about k_sha1_pkts read from the gfx950 listing hipcc emits for
csrc/sha1_kernels.hip (tools/isa_mix.py compiles it as the product build does).

  * one kernel symbol: one instantiation, the fused compare chosen at run time;
  * no scratch, no LDS, no s_barrier;
  * VALU instructions per whole block below k_sha1_gather's 716,
    the figure this kernel exists to beat;
  * a block's loads stay outstanding across the compress: no s_waitcnt
    vmcnt(0) inside the loop body.

The loop body is the text of the kernel's outer loop.  A whole block's path
through it is what a wave executes when none of its lanes is in its message's
padding: branches on an empty exec mask whose target lies in the loop are
taken (they skip the padding block, which a message runs at most twice),
everything else falls through until the loop's header comes round again.
"""
import os
import re
import sys

import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, "tools"))
import isa_mix  # noqa: E402

GATHER_VALU_PER_BLOCK = 716


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("isa") / "k.s")
    isa_mix.compile_asm(out)
    return open(out).read()


def kernel(listing):
    syms = set(re.findall(r"^(_ZN6btsha1\d+k_sha1_pkts\w*):", listing, re.M))
    assert len(syms) == 1, syms
    sym = syms.pop()
    body = listing[listing.index(sym + ":"):]
    return sym, body[:body.index(".Lfunc_end")], body


def loop(body):
    """(lines of the outer loop's text, index of its header in them)."""
    lines = [l.strip() for l in body.splitlines()]
    hdr = [i for i, l in enumerate(lines) if re.match(r"\.LBB\d+_\d+:.*=>This Loop Header: Depth=1", l)
           or re.match(r"\.LBB\d+_\d+:.*=>This Inner Loop Header: Depth=1", l)]
    assert len(hdr) == 1, hdr
    label = lines[hdr[0]].split(":")[0]
    member = [i for i, l in enumerate(lines) if re.search(r"(in Loop: Header=|Parent Loop )%s\b" % label[2:], l)]
    first = min(member + hdr)
    last = max(i for i, l in enumerate(lines) if re.match(r"s_c?branch\w* %s$" % re.escape(label), l)
               or (l.startswith("s_branch") and i > hdr[0] and re.search(r"\.LBB", l)))
    # the loop's text ends with the last branch back into it
    inside = {lines[i].split(":")[0] for i in member + hdr}
    last = max(i for i, l in enumerate(lines) if l.startswith(("s_branch", "s_cbranch")) and l.split()[-1] in inside)
    return lines[first:last + 1], hdr[0] - first


def test_one_kernel_no_scratch_no_lds_no_barrier(listing):
    sym, body, meta = kernel(listing)
    assert int(re.search(r"; ScratchSize: (\d+)", meta).group(1)) == 0
    assert int(re.search(r"; LDSByteSize: (\d+)", meta).group(1)) == 0
    assert "s_barrier" not in body and "scratch_" not in body and "ds_" not in body


def test_loads_stay_outstanding_across_the_compress(listing):
    _, body, _ = kernel(listing)
    text, _ = loop(body)
    assert sum(l.startswith("global_load_dwordx") for l in text) == 5, "the block's five loads"
    assert sum(l.startswith("v_bitop3_b32") for l in text) >= 80, "the loop holds the compress"
    waits = [l for l in text if "vmcnt" in l]
    assert waits and not [l for l in waits if "vmcnt(0)" in l], waits


def test_valu_per_whole_block_is_below_the_gather_kernels(listing):
    _, body, _ = kernel(listing)
    text, hdr = loop(body)
    labels = {l.split(":")[0]: i for i, l in enumerate(text) if l.startswith(".LBB")}
    total = sum(l.startswith("v_") for l in text)
    i, valu, steps = hdr + 1, 0, 0
    while True:
        steps += 1
        assert steps < 10 * len(text), "no way back to the header"
        l = text[i] if i < len(text) else ""
        if l.startswith("v_"):
            valu += 1
        m = re.match(r"(s_branch|s_cbranch_execz) (\.LBB\d+_\d+)$", l)
        if m and m.group(2) in labels:
            i = labels[m.group(2)]  # in the loop: back to its header, or past the padding block
        else:
            assert not l.startswith("s_cbranch") or l.startswith("s_cbranch_execz"), l  # leaves the loop: not taken
            i += 1
        if i == hdr:
            break
    print(f"k_sha1_pkts: {valu} VALU per whole block, {total} in the loop's text (padding block included)")
    assert 597 <= valu < GATHER_VALU_PER_BLOCK, valu
