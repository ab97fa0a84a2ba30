"""Shared by tests/test_gpu_ragged_verify.py and its barrier-build twin
tests/test_gpu_ragged_verify_barriers.py: one ragged batch per launch form of
btsha1_launch_ragged_verify, and the three launches every form gets.

Forms (n messages, CUs = compute units of the device):
  chain     k_sha1_chain<false, true>, one workgroup per message       n = 300
  lat2      k_sha1_lat_ragged_verify<2>, up to CUs workgroups of 64    n = 300
  lat3      k_sha1_lat_ragged_verify<3>, more than CUs workgroups      n = 64 * CUs + 1
  lanes     k_sha1_ragged_verify in 64-thread workgroups               n = 300
  lanes256  the same in 256-thread workgroups (n >= 256 * CUs)         n = 256 * CUs + 65
Every n is odd against 64, 128 and 256, so the last workgroup is partly filled.

Lengths.  LENGTHS = 0, 1, 55, 56, 63, 64, 65, 119, 120, 127, 128, 191, 4097:
every padding residue around 55 / 56 / 63 / 64, with and without whole blocks,
and one message of 65 blocks.  Workgroup 0 cycles through all of them, so its
nbmax (66) differs from every other lane's nb and each lane's latch decides;
workgroup 1 holds only empty messages; the others rotate through the lengths up
to 191.  lanes256 has no 4097 (65 thousand messages stay at a few MiB).
Offsets hit every residue mod 16; `expected`, `ok` and the digests sit at odd
addresses inside sentinel-guarded buffers.

Launches per form: the verdict batch of verdict_cases.py planted on the last
168 messages (one flipped bit each for 160 of them), with and without a digest
buffer -- the verdicts must not depend on it -- then all expectations exact.
"""
import contextlib
import hashlib

import numpy as np

LENGTHS = (0, 1, 55, 56, 63, 64, 65, 119, 120, 127, 128, 191, 4097)
SHORT = LENGTHS[:-1]
FORMS = ("chain", "lat2", "lat3", "lanes", "lanes256")
SEED = 0x9A66


def n_for(form, cus):
    return {"chain": 300, "lat2": 300, "lat3": 64 * cus + 1, "lanes": 300, "lanes256": 256 * cus + 65}[form]


@contextlib.contextmanager
def pinned(bt, form, n, cus):
    """The two settings that send a ragged batch of n messages to `form`; restores them."""
    chain, lat = {"chain": (1 << 62, 0), "lat2": (0, 1 << 62), "lat3": (0, 1 << 62), "lanes": (0, 0),
                  "lanes256": (0, 0)}[form]
    grid = (n + 63) // 64
    assert {"lat2": grid <= cus, "lat3": grid > cus, "lanes": n < 256 * cus, "lanes256": n >= 256 * cus}.get(form, True)
    assert n % 64 and n % 128 and n % 256
    prev_chain, prev_lat = bt.set_chain_batch(chain), bt.set_latency_batch(lat)
    try:
        yield
    finally:
        bt.set_chain_batch(prev_chain)
        bt.set_latency_batch(prev_lat)


def lengths(n, longest=True):
    out = []
    for i in range(n):
        g, j = divmod(i, 64)
        if g == 0:
            out.append((LENGTHS if longest else SHORT)[j % (13 if longest else 12)])
        elif g == 1:
            out.append(0)
        else:
            out.append(SHORT[(j + g) % 12])
    return out


_batches = {}


def batch(orc, n, longest=True):
    """(blob, offsets, lengths, digests back to back) of the n-message batch, built once per n."""
    key = (n, longest)
    if key not in _batches:
        lens = lengths(n, longest)
        offs, pos = [], 0
        for i, ln in enumerate(lens):
            pos += 1 + (5 * i) % 15
            offs.append(pos)
            pos += ln
        assert {o % 16 for o in offs} == set(range(16))
        blob = orc.fill_synthetic(pos + 64, n, SEED)
        view = memoryview(blob)
        want = b"".join(hashlib.sha1(view[o:o + ln]).digest() for o, ln in zip(offs, lens))
        _batches[key] = (blob, offs, lens, want)
    return _batches[key]


def barrier_want(lens, slots, launches):
    """(waves checked, barriers executed) the barrier build must count for `launches`
    launches of k_sha1_lat_ragged_verify<slots> over these lengths: two waves per
    workgroup of 64 messages, nbmax + slots - 1 barriers each, nbmax the largest
    block count (whole blocks + one or two padding blocks) in the workgroup."""
    waves = barriers = 0
    for g in range(0, len(lens), 64):
        nbmax = max((ln >> 6) + (2 if (ln & 63) >= 56 else 1) for ln in lens[g:g + 64])
        waves += 2
        barriers += 2 * (nbmax + slots - 1)
    return launches * waves, launches * barriers


def run_form(bt, torch, lf, vc, orc, form, cus):
    """The three launches of `form`; returns (lengths, launches)."""
    n = n_for(form, cus)
    blob, offs, lens, want = batch(orc, n, longest=form != "lanes256")
    d = lf.upload(torch, blob)
    d_off = torch.tensor(offs, dtype=torch.int64, device="cuda")
    d_len = torch.tensor(lens, dtype=torch.int32, device="cuda")
    oks = {}
    with pinned(bt, form, n, cus):
        for exact, with_digests in ((False, True), (False, False), (True, True)):
            exp = vc.expectations(want, exact)
            d_exp = torch.zeros(20 * n + 1, dtype=torch.uint8, device="cuda")
            d_exp[1:] = torch.from_numpy(exp.reshape(-1)).cuda()
            ok, dig = lf.Guarded(torch, n, 1, 3), lf.Guarded(torch, n, 20, 1)
            assert (d_exp.data_ptr() + 1) % 2 == 1 and ok.ptr % 2 == 1 and dig.ptr % 2 == 1
            bt.ragged_verify_dev(d.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), n, d_exp.data_ptr() + 1, ok.ptr,
                                 dig.ptr if with_digests else None)
            run = (form, n, "exact" if exact else "planted", "digests" if with_digests else "no digest buffer")
            got = lf.settle(torch, run, [("ok", ok, lf.WRITTEN), ("digests", dig, want if with_digests else None)])
            bad = vc.problems(got["ok"], exact)
            assert not bad, (run, bad)
            oks[(exact, with_digests)] = got["ok"].copy()
    assert np.array_equal(oks[(False, True)], oks[(False, False)]), (form, "verdicts depend on the digest buffer")
    return lens, 3
