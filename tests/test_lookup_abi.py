"""CPU: bt_sha1_lookup_dev refuses a table it cannot index, before any device
call -- so this holds without a GPU.

The slot array of the lookup is a power of two of at least 2 * n_table
entries, counted in a uint32_t.  For 2^30 < n_table < 2^31 that power of two
is 2^32: the doubling loop `while (cap < 2 * n_table) cap <<= 1` took cap from
2^31 to 0 and never ended (the old guard refused only n_table >= 2^31).  The
limit is now 2^30, stated in include/bt_sha1.h, and checked first among the
arguments.

The calls run in a child process under a time limit: a library without the
check gets as far as the HIP calls -- "no device" where there is none, the
endless loop where there is one -- and neither is the message asked for here.
"""
import json
import subprocess
import sys

from conftest import PKG

CHILD = r"""
import ctypes, json, os, sys
lib = ctypes.CDLL(os.path.join(sys.argv[1], "libbtsha1.so"))
vp, u64 = ctypes.c_void_p, ctypes.c_uint64
f = lib.bt_sha1_lookup_dev
f.restype, f.argtypes = ctypes.c_int, [vp, u64, vp, u64, vp, vp]
lib.bt_sha1_last_error.restype = ctypes.c_char_p
table = (ctypes.c_uint32 * 10)()    # two 20-byte entries, 4-byte aligned
queries = (ctypes.c_uint32 * 5)()   # one query
index = (ctypes.c_int64 * 1)(7)
t, q, ix = (ctypes.addressof(a) for a in (table, queries, index))
assert t % 4 == 0 and q % 4 == 0
out = []
for n_table, d_index in ((2**30 + 1, ix), (2**31 - 1, ix), (2**31, ix), (2**63, ix), (2**30 + 1, None),
                         (2**30, None), (2, None)):
    rc = f(t, n_table, q, 1, d_index, None)
    out.append([n_table, d_index is not None, rc, lib.bt_sha1_last_error().decode(), index[0]])
out.append([2**31 - 1, True, f(t, 2**31 - 1, q, 0, ix, None), "", index[0]])  # no queries: nothing to do
print(json.dumps(out))
"""


def test_lookup_refuses_more_than_2_30_entries_before_any_device_call():
    r = subprocess.run([sys.executable, "-c", CHILD, PKG], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = json.loads(r.stdout.strip().splitlines()[-1])
    seen = {(n, real): (rc, msg, idx) for n, real, rc, msg, idx in rows[:-1]}
    # small real host arrays: refused with the message, nothing looked up, nothing written
    for n in (2**30 + 1, 2**31 - 1, 2**31, 2**63):
        assert seen[(n, True)] == (-1, "lookup table too large", 7), (n, seen[(n, True)])
    # the size is checked before the pointers ...
    assert seen[(2**30 + 1, False)][:2] == (-1, "lookup table too large")
    # ... so a null d_index shows, with no device call either, that 2^30 entries pass the size check
    for n in (2**30, 2):
        rc, msg, _ = seen[(n, False)]
        assert rc == -1 and "non-null" in msg and "too large" not in msg, (n, rc, msg)
    assert rows[-1][2] == 0 and rows[-1][4] == 7  # n_queries == 0 returns before every check
