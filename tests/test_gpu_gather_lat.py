"""GPU: the latency form of segment-list batches (k_sha1_gather_lat<2 / 3>
behind bt_sha1_set_seglist_latency_batch): digests and fused verdicts equal to
the oracle's and to the one-message-per-lane kernel's, at the seams of its two
waves (n around a workgroup, the longest message in the last lane, lanes past
n), from device and pinned tables, in both slot forms, and under a gather
verifier.  Every test sets the knob and restores it."""
import contextlib
import ctypes
import hashlib
import random

import numpy as np
import pytest

import gather_cases as gc
import gather_lat_cases as glc
import test_gpu_launch_forms as lf
from conftest import load_btsha1

pytestmark = pytest.mark.gpu
AUTO = 2**64 - 1


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "gpu tests need a HIP device"
    return t


@pytest.fixture(scope="module")
def bt(torch):
    m = load_btsha1()
    assert m.device_count() >= 1
    return m


@pytest.fixture(scope="module")
def cus(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


@contextlib.contextmanager
def knob(bt, value):
    prev = bt.set_seglist_latency_batch(value)
    try:
        yield
    finally:
        bt.set_seglist_latency_batch(prev)


def dev(torch, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).cuda()


def pinned(torch, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1).copy()).pin_memory()


@pytest.fixture(scope="module")
def mixed(torch):
    b = glc.mixed_batch()
    return b, dev(torch, b["blob"]), dev(torch, b["segs"])


def run(bt, torch, blob, segs, first, count, n, put=None, expected=None, with_digests=True):
    """One gather launch over n messages; returns (digests, ok) as the
    Guarded outputs (ok None without `expected`)."""
    put = put or dev
    d_first, d_count = put(torch, first), put(torch, count)
    dig = lf.Guarded(torch, n, 20, 1)
    if expected is None:
        bt.gather_dev(blob.data_ptr(), segs.data_ptr(), d_first.data_ptr(), d_count.data_ptr(), n, dig.ptr)
        torch.cuda.synchronize()
        return dig, None
    exp = dev(torch, np.frombuffer(expected, dtype=np.uint8))
    ok = lf.Guarded(torch, n, 1, 3)
    bt.gather_verify_dev(blob.data_ptr(), segs.data_ptr(), d_first.data_ptr(), d_count.data_ptr(), n,
                         exp.data_ptr(), ok.ptr, dig.ptr if with_digests else None)
    torch.cuda.synchronize()
    return dig, ok


def test_knob_and_name_follow_the_regime(bt, cus):
    assert bt.set_seglist_latency_batch(0) == 0  # off by default
    assert bt.seglist_kernel_name(1) == bt.seglist_kernel_name(64 * cus) == "k_sha1_gather"
    with knob(bt, AUTO):
        assert bt.seglist_kernel_name(1) == bt.seglist_kernel_name(64 * cus) == "k_sha1_gather_lat<2>"
        assert bt.seglist_kernel_name(64 * cus + 1) == bt.seglist_kernel_name(128 * cus) == "k_sha1_gather_lat<3>"
        assert bt.seglist_kernel_name(128 * cus + 1) == "k_sha1_gather"
    with knob(bt, 65):
        assert bt.seglist_kernel_name(65) == "k_sha1_gather_lat<2>" and bt.seglist_kernel_name(66) == "k_sha1_gather"
    assert bt.set_seglist_latency_batch(0) == 0


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 130])
@pytest.mark.parametrize("where", ["device", "pinned"])
def test_digests_equal_the_oracle_and_the_lane_kernel(bt, torch, mixed, n, where):
    """The walk's cases in turn, the longest message (77 blocks against at
    most 4) in lane n - 1: the last lane of a workgroup at n = 64, else a lane
    past which n ends.  n = 130 is the whole batch: messages 127 and 128,
    which list one segment both, run in the same launch.  Tables in device or
    pinned host memory; the segments of a message run against the address order."""
    b, blob, segs = mixed
    first, count, want, _ = glc.longest_last(b, n)
    put = dev if where == "device" else pinned
    d_segs = segs if where == "device" else pinned(torch, b["segs"])
    with knob(bt, 0):
        off, _ = run(bt, torch, blob, d_segs, first, count, n, put)
    with knob(bt, AUTO):
        assert bt.seglist_kernel_name(n) == "k_sha1_gather_lat<2>"
        on, _ = run(bt, torch, blob, d_segs, first, count, n, put)
    got = lf.settle(torch, ("gather_lat", n, where), [("off", off, want), ("on", on, want)])
    assert np.array_equal(got["off"], got["on"])


def test_three_slot_form_at_its_smallest_grid(bt, torch, cus):
    b = glc.small_batch()
    n = 64 * cus + 1
    first, count, want, lens = glc.tiled_with_seams(b, n)  # empty and one-segment messages among them
    assert sum(lens) < 8 << 20
    blob, segs = dev(torch, b["blob"]), dev(torch, b["segs"])
    with knob(bt, AUTO):
        assert bt.seglist_kernel_name(n) == "k_sha1_gather_lat<3>"
        on, _ = run(bt, torch, blob, segs, first, count, n)
    lf.settle(torch, "three slots", [("digests", on, want)])


@pytest.mark.parametrize("n", [64, 130])
@pytest.mark.parametrize("with_digests", [True, False])
def test_fused_compare(bt, torch, mixed, n, with_digests):
    """One single-bit mismatch planted in each of the five digest words, in
    five different lanes; nothing written past n; digests may be null."""
    b, blob, segs = mixed
    first, count, want, _ = glc.longest_last(b, n)
    exp = bytearray(want)
    planted = {3: (0, 31), 17: (1, 0), 31: (2, 13), 45: (3, 7), n - 1: (4, 24)}  # lane: (word, bit)
    for lane, (word, bit) in planted.items():
        exp[20 * lane + 4 * word + (3 - bit // 8)] ^= 1 << (bit % 8)
    want_ok = bytes(0 if i in planted else 1 for i in range(n))
    outs = {}
    for setting in (0, AUTO):
        with knob(bt, setting):
            dig, ok = run(bt, torch, blob, segs, first, count, n, expected=bytes(exp), with_digests=with_digests)
        outs[setting] = lf.settle(torch, ("verify", n, with_digests, setting),
                                  [("ok", ok, want_ok), ("digests", dig, want if with_digests else None)])
    assert np.array_equal(outs[0]["ok"], outs[AUTO]["ok"])


SLOT = 5 * gc.DGRAM


def verifier_run(bt):
    """130 slots through a gather verifier of batch 130: datagrams out of
    order with a duplicate, one slot released, every 9th chunk planted bad."""
    rng = random.Random(0x1A7E)
    v = bt.Verifier(chunk_len=SLOT, batch=130, nstreams=2, gather=True, max_segs=8)
    try:
        slots = [v.slot() for _ in range(130)]
        want = []
        for k, slot in enumerate(slots):
            if k == 77:
                v.release(slot)
                continue
            npay = 1 + k % 3  # with the last payload and the duplicate at most five datagrams: the slot
            pays = [rng.randbytes(gc.PAYLOAD) for _ in range(npay)] + [rng.randbytes(1 + (37 * k) % gc.LAST_PAYLOAD)]
            order = rng.sample(range(len(pays)), len(pays))
            where = {}
            for arrival, seq in enumerate(order + [order[0]]):  # the first to arrive comes again
                pkt = seq.to_bytes(4, "little") + bytes(12) + pays[seq]
                ctypes.memmove(slot + arrival * gc.DGRAM, pkt, len(pkt))
                where.setdefault(seq, arrival * gc.DGRAM + gc.HEADER)
            segs = [(where[s], len(pays[s])) for s in range(len(pays))]
            dg = hashlib.sha1(b"".join(pays)).digest()
            good = k % 9 != 4
            v.commit_gather(slot, segs, dg if good else dg[:11] + bytes([dg[11] ^ 2]) + dg[12:], k)
            want.append((k, good, dg))
        got = v.drain()
        return sorted(got), sorted(want), v.gather_stats(), v.stats()
    finally:
        v.close()


def test_gather_verifier_gives_the_same_verdicts_with_the_knob_on(bt):
    with knob(bt, 0):
        off = verifier_run(bt)
    with knob(bt, AUTO):
        assert bt.seglist_kernel_name(130) == "k_sha1_gather_lat<2>"
        on = verifier_run(bt)
    assert off[0] == off[1] and on[0] == on[1]
    assert off == on
    assert on[2]["gather_batches"] == 1 and on[2]["gather_chunks"] == 129 and on[3]["released"] == 1
