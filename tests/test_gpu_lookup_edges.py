"""GPU: every bit and every probe of the digest lookup (k_lookup_build /
k_lookup_query behind bt_sha1_lookup_dev).

Every other lookup test fills table and queries with real SHA-1 digests of
short strings: an absent query then differs from every entry in all five
words, no two entries share key[0], and a probe chain is as short as the load
factor makes it.  same_digest() could lose any of its five terms, in the
build or in the query, and the wrap of a chain from slot `mask` to slot 0 is
reached by chance only.  Here entries and queries are arbitrary 20-byte
strings (the kernels never hash them); the reference is the first-match
dictionary of test_gpu_parity.py:

  one-bit queries     168 entries; query i < 160 is entry i with bit i alone
                      flipped and must miss, the last 8 are exact; then 168
                      exact queries.  A failure names the bits whose flip
                      was accepted, as verdict_cases.problems does.
  one-bit neighbours  a base value and its 160 single-bit variants as table
                      entries: each found at its own index (the build must
                      not merge them), a true duplicate resolving to the first.
  shared key[0]       700 distinct entries with the same first four bytes,
                      key[0] & 2047 == 2045 under a capacity of 2048: ONE
                      chain of 700 slots that wraps past the end of the slot
                      array; every entry found, 50 absent values with the same
                      four bytes walk the whole chain, 30 duplicates far from
                      their originals give the original's index.
  capacity steps      512, 513, 1024 and 1025 random entries: load exactly
                      1/2 (capacity 1024, 2048) and the first table past it.

Table and queries start at addresses that are 4 mod 16 (the contract is
4-byte alignment); d_index lies behind canaries (test_gpu_launch_forms.Guarded).
"""
import random

import numpy as np
import pytest

import test_gpu_launch_forms as lf
import verdict_cases as vc
from conftest import load_btsha1

pytestmark = pytest.mark.gpu

Guarded, settle, WRITTEN = lf.Guarded, lf.settle, lf.WRITTEN


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


def at4(torch, entries):
    """20-byte strings back to back in device memory, the first at an address
    that is 4 mod 16.  Returns (the tensor, to be kept alive; the address)."""
    raw = b"".join(entries)
    t = torch.zeros(len(raw) + 32, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    t[4:4 + len(raw)] = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    return t, t.data_ptr() + 4


def first_match(table, queries):
    first = {}
    for i, d in enumerate(table):
        first.setdefault(d, i)
    return [first.get(q, -1) for q in queries]


def lookup(bt, torch, table, queries, label):
    assert all(len(x) == 20 for x in table) and all(len(x) == 20 for x in queries)
    keep_t, p_table = at4(torch, table)
    keep_q, p_queries = at4(torch, queries)
    out = Guarded(torch, len(queries), 8)
    assert p_table % 16 == 4 and p_queries % 16 == 4 and out.ptr % 8 == 0
    bt.lookup_dev(p_table, len(table), p_queries, len(queries), out.ptr)
    got = settle(torch, label, [("index", out, WRITTEN)])
    del keep_t, keep_q
    return [int(x) for x in got["index"].copy().view(np.int64)]


def flip(entry, bit):
    b = bytearray(entry)
    b[bit // 8] ^= 1 << (bit % 8)
    return bytes(b)


def random_entries(rng, n):
    out = [rng.randbytes(20) for _ in range(n)]
    assert len(set(out)) == n
    return out


def mismatches(got, want, limit=20):
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    return [f"{len(bad)} of {len(want)} answers differ: " +
            ", ".join(f"query {i}: {got[i]} want {want[i]}" for i in bad[:limit])] if bad else []


def test_lookup_one_bit_queries(bt, torch):
    rng = random.Random(0x10C)
    table = random_entries(rng, vc.N)
    planted = [flip(table[i], i) for i in range(vc.NBITS)] + table[vc.NBITS:]
    assert not set(planted[:vc.NBITS]) & set(table)
    for exact, queries in ((False, planted), (True, table)):
        want = first_match(table, queries)
        assert want == ([-1] * vc.NBITS + list(range(vc.NBITS, vc.N)) if not exact else list(range(vc.N)))
        got = lookup(bt, torch, table, queries, ("one-bit queries", "exact" if exact else "planted"))
        bad = []
        if not exact:
            accepted = [i for i in range(vc.NBITS) if got[i] != -1]
            if accepted:
                bad.append(f"{len(accepted)} one-bit differences not rejected: digest bits {vc.ranges(accepted)} "
                           f"(bytes {vc.ranges({i // 8 for i in accepted})}), answers {[got[i] for i in accepted[:20]]}")
            bad += mismatches(got[vc.NBITS:], want[vc.NBITS:])
        else:
            bad += mismatches(got, want)
        assert not bad, (exact, bad)


def test_lookup_one_bit_neighbours_in_the_table(bt, torch):
    rng = random.Random(0x10D)
    base = rng.randbytes(20)
    table = [base] + [flip(base, i) for i in range(vc.NBITS)]
    assert len(set(table)) == vc.NBITS + 1
    table.append(table[5])  # a true duplicate, at the end
    got = lookup(bt, torch, table, table, "one-bit neighbours")
    want = list(range(vc.NBITS + 1)) + [5]
    assert want == first_match(table, table)
    merged = [i - 1 for i in range(1, vc.NBITS + 1) if got[i] != i]
    bad = []
    if merged:
        bad.append(f"{len(merged)} entries one bit from the base not found at their own index: digest bits "
                   f"{vc.ranges(merged)} (bytes {vc.ranges({i // 8 for i in merged})}), "
                   f"answers {[got[i + 1] for i in merged[:20]]}")
    if got[0] != 0:
        bad.append(f"the base entry: {got[0]} want 0")
    if got[-1] != 5:
        bad.append(f"the duplicate of entry 5: {got[-1]} want 5")
    assert not bad, bad


SHARED = bytes([0xFD, 0x07, 0xA5, 0x3C])  # key[0] = 0x3CA507FD little-endian; & 2047 == 2045


def test_lookup_shared_first_word_chain_wraps(bt, torch):
    rng = random.Random(0x10E)
    assert int.from_bytes(SHARED, "little") & 2047 == 2045
    tails = set()
    while len(tails) < 750:
        tails.add(rng.randbytes(16))
    tails = sorted(tails)
    rng.shuffle(tails)
    distinct = [SHARED + t for t in tails[:700]]
    absent = [SHARED + t for t in tails[700:]]
    originals = [23 * j + 3 for j in range(30)]  # 3 .. 670: the copies at 700 .. 729 lie 30 to 697 entries away
    table = distinct + [distinct[o] for o in originals]
    n = len(table)
    assert n == 730 and 1024 < 2 * n <= 2048  # bt_sha1_lookup_dev: capacity 2048, the chain starts at slot 2045
    assert 2045 + 700 > 2048
    queries = table + absent
    want = first_match(table, queries)
    assert want == list(range(700)) + originals + [-1] * 50
    got = lookup(bt, torch, table, queries, "shared key[0]")
    bad = mismatches(got, want)
    assert not bad, bad


@pytest.mark.parametrize("n_table", [512, 513, 1024, 1025])
def test_lookup_capacity_steps(bt, torch, n_table):
    rng = random.Random(n_table)
    pool = random_entries(rng, n_table + 100)
    table, absent = pool[:n_table], pool[n_table:]
    queries = table + absent
    rng.shuffle(queries)
    want = first_match(table, queries)
    assert sorted(w for w in want if w >= 0) == list(range(n_table)) and want.count(-1) == 100
    got = lookup(bt, torch, table, queries, ("capacity", n_table))
    bad = mismatches(got, want)
    assert not bad, (n_table, bad)
