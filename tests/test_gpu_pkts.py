"""GPU: SHA-1 straight from fixed-size packet buffers (bt_sha1_pkts_dev /
bt_sha1_pkts_verify_dev, k_sha1_pkts).

1. Every geometry, length and order of pkts_cases at n = 1, 63, 64, 65, 257:
   digests equal the oracle's over the assembled messages.
2. Slots that are not 4-byte aligned still give the right digests.
3. The fused compare: every digest bit, no digest buffer, odd addresses,
   entries past n untouched.
4. The same messages as segment lists through bt_sha1_gather_verify_dev.
5. Order tables full of out-of-range entries read the clamped buffer.
6. The 256-thread form (at least one wave per SIMD).
"""
import numpy as np
import pytest

import pkts_cases as pc
import test_gpu_launch_forms as lf
import verdict_cases as vc
from conftest import load_btsha1

pytestmark = pytest.mark.gpu


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


def dev(torch, arr):
    return torch.from_numpy(arr.view(np.uint8).reshape(-1).copy()).cuda()


class Tables:
    def __init__(self, bt, torch, b, **replace):
        a = dict(b, **replace)
        self.geom = bt.PktGeom(*b["geom"], pc.SLOT_PKTS)
        self.keep = [dev(torch, a[k]) for k in ("blob", "slot_off", "len", "order", "order_first")]

    def args(self):
        blob, slot_off, length, order, order_first = (t.data_ptr() for t in self.keep)
        return blob, self.geom, slot_off, length, order, order_first


_tables = {}


def tables(bt, torch, orc, geom):
    if geom not in _tables:
        b = pc.batch(orc, geom)
        _tables[geom] = (b, Tables(bt, torch, b))
    return _tables[geom]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("geom", pc.GEOMETRIES, ids=lambda g: "%d-%d-%d" % g)
def test_pkts_digests_equal_the_oracle(bt, torch, oracle, geom, n):
    b, t = tables(bt, torch, oracle, geom)
    dig = lf.Guarded(torch, n, 20, 1)
    bt.pkts_dev(*t.args(), n, dig.ptr)
    lf.settle(torch, ("pkts_dev", geom, n), [("digests", dig, b["want"][:20 * n])])


def test_pkts_no_messages_touches_nothing(bt, torch, oracle):
    _, t = tables(bt, torch, oracle, pc.GEOMETRIES[1])
    dig, ok = lf.Guarded(torch, 4, 20), lf.Guarded(torch, 4, 1)
    bt.pkts_dev(*t.args(), 0, dig.ptr)
    bt.pkts_verify_dev(*t.args(), 0, t.keep[0].data_ptr(), ok.ptr, dig.ptr)
    lf.settle(torch, "n == 0", [("digests", dig, None), ("ok", ok, None)])


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_pkts_misaligned_slots(bt, torch, oracle, shift):
    """d_slot_off not a multiple of 4: outside the caller's contract for
    speed, inside it for the result."""
    b = pc.batch(oracle, pc.GEOMETRIES[1])
    t = Tables(bt, torch, b, blob=np.concatenate([np.full(shift, pc.POISON, np.uint8), b["blob"]]),
               slot_off=b["slot_off"] + np.uint64(shift))
    n = 65
    dig = lf.Guarded(torch, n, 20, 1)
    bt.pkts_dev(*t.args(), n, dig.ptr)
    lf.settle(torch, ("misaligned", shift), [("digests", dig, b["want"][:20 * n])])


def verdict_tables(bt, torch, orc):
    """vc.N messages of 64 bytes, each the second buffer of a slot of two."""
    stride, header, payload = 76, 4, 68
    rng = np.random.default_rng(pc.SEED)
    blob = np.full(vc.N * 2 * stride, pc.POISON, np.uint8)
    msgs = rng.integers(0, 256, (vc.N, 64), dtype=np.uint8)
    for i in range(vc.N):
        at = i * 2 * stride + stride + header
        blob[at:at + 64] = msgs[i]
    want = b"".join(orc.sha1(bytes(m)) for m in msgs)
    keep = [dev(torch, a) for a in (blob, np.arange(vc.N, dtype=np.uint64) * np.uint64(2 * stride),
                                    np.full(vc.N, 64, np.uint32), np.ones(vc.N, np.uint32),
                                    np.arange(vc.N, dtype=np.uint64))]
    return keep, bt.PktGeom(stride, header, payload, 2), want


@pytest.mark.parametrize("with_digests", [False, True])
def test_pkts_verify_every_digest_bit(bt, torch, oracle, with_digests):
    """One wrong bit at each of the 160 positions, as 160 messages of 64 bytes;
    expected hashes and verdicts at odd addresses; d_digests NULL or given."""
    keep, geom, want = verdict_tables(bt, torch, oracle)
    n = vc.N - 3  # the last workgroup partly filled: entries past n stay untouched
    exp_all = vc.expectations(want)[:n]
    expd = lf.Guarded(torch, n, 20, 1)
    expd.buf[expd.lead:expd.lead + expd.used] = torch.from_numpy(exp_all.reshape(-1).copy()).cuda()
    ok, dig = lf.Guarded(torch, n, 1, 1), lf.Guarded(torch, n, 20, 3)
    bt.pkts_verify_dev(*(k.data_ptr() if hasattr(k, "data_ptr") else k
                         for k in (keep[0], geom, keep[1], keep[2], keep[3], keep[4])),
                       n, expd.ptr, ok.ptr, dig.ptr if with_digests else None)
    got = lf.settle(torch, ("verify", with_digests),
                    [("ok", ok, vc.want_ok(vc.N)[:n].tobytes()),
                     ("digests", dig, want[:20 * n] if with_digests else None)])
    assert got["ok"][:vc.NBITS].sum() == 0 and got["ok"][vc.NBITS:].all()


@pytest.mark.parametrize("geom", pc.GEOMETRIES[:2], ids=lambda g: "%d-%d-%d" % g)
def test_pkts_agree_with_the_gather_path(bt, torch, oracle, geom):
    """The segment lists the orders imply, through bt_sha1_gather_verify_dev:
    identical digests and verdicts."""
    b, t = tables(bt, torch, oracle, geom)
    n = b["n"]
    exp = dev(torch, np.frombuffer(b["want"], dtype=np.uint8))
    segs, first, count = dev(torch, b["segs"]), dev(torch, b["first"]), dev(torch, b["count"])
    okg, digg = lf.Guarded(torch, n, 1), lf.Guarded(torch, n, 20)
    okp, digp = lf.Guarded(torch, n, 1), lf.Guarded(torch, n, 20)
    bt.gather_verify_dev(t.keep[0].data_ptr(), segs.data_ptr(), first.data_ptr(), count.data_ptr(), n,
                         exp.data_ptr(), okg.ptr, digg.ptr)
    bt.pkts_verify_dev(*t.args(), n, exp.data_ptr(), okp.ptr, digp.ptr)
    ones = bytes([1]) * n
    lf.settle(torch, ("gather", geom), [("ok", okg, ones), ("digests", digg, b["want"])])
    lf.settle(torch, ("pkts", geom), [("ok", okp, ones), ("digests", digp, b["want"])])


@pytest.mark.parametrize("geom", [pc.GEOMETRIES[2], pc.GEOMETRIES[3]], ids=lambda g: "%d-%d-%d" % g)
def test_pkts_out_of_range_orders_are_clamped(bt, torch, oracle, geom):
    """Every entry at or above slot_pkts: each position reads buffer
    slot_pkts - 1 of its own slot, the last bytes of the blob included (the
    geometries whose payload ends the buffer)."""
    b = pc.batch(oracle, geom)
    bad = np.where(np.arange(b["order"].size) % 3 == 0, 0xFFFFFFFF, pc.SLOT_PKTS + np.arange(b["order"].size))
    t = Tables(bt, torch, b, order=bad.astype(np.uint32))
    n = b["n"]
    dig = lf.Guarded(torch, n, 20, 1)
    bt.pkts_dev(*t.args(), n, dig.ptr)
    lf.settle(torch, ("clamped", geom), [("digests", dig, pc.clamped_want(oracle, b))])


def test_pkts_256_thread_form(bt, torch, oracle):
    """At least one wave per SIMD: 256-thread workgroups (chain_workgroup), the
    fused compare with the verdict batch planted on the last 168 messages."""
    geom = pc.GEOMETRIES[1]
    b = pc.batch(oracle, geom)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = cus * 256 + 1
    reps = -(-n // b["n"])
    t = Tables(bt, torch, b, **{k: np.tile(b[k], reps)[:n] for k in ("slot_off", "len", "order_first")})
    want = (b["want"] * reps)[:20 * n]
    exp = dev(torch, vc.expectations(want))
    ok, dig = lf.Guarded(torch, n, 1, 1), lf.Guarded(torch, n, 20, 1)
    bt.pkts_verify_dev(*t.args(), n, exp.data_ptr(), ok.ptr, dig.ptr)
    lf.settle(torch, "256 threads", [("ok", ok, vc.want_ok(n).tobytes()), ("digests", dig, want)])
