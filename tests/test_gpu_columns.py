"""GPU: k_sha1_lat's column forms (FIRST / MIDDLE / LAST, with and without the
fused compare, 2 and 3 LDS slots) in the product library, launched one at a
time through bt_sha1_column_dev at shapes of a few MiB -- the public paths
reach them only with chunks of 64 KiB or more, and their 3-slot form only
past 1 GiB.

Every launch of a FIRST -> MIDDLE.. -> LAST sequence is compared with the
oracle (column_cases.run_case): the chaining state of every chunk after each
column, the digests and the fused compare's verdicts after the last, and the
canaries past the end of each output.  Columns hashed in place (pitch >
width) and gathered densely (pitch == width), widths of 1, 2, 3, 5 and 16
blocks, row counts that leave the last workgroup with 1, 2, 36 or 64 rows.
"""
import numpy as np
import pytest

import column_cases as cc
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


@pytest.fixture(scope="module")
def cus(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("idx", range(5), ids=["a", "b", "c-2slot", "c-3slot", "d"])
def test_column_sequence_matches_the_oracle(bt, torch, oracle, cus, idx):
    case = cc.cases(cus)[idx]
    grid = (case.n + 63) // 64
    assert (grid > cus) == ("3-slot" in case.name), (case.name, grid, cus)
    seen = []

    def on_launch(label, n, width, part, problems):
        seen.append(label)
        assert not problems, (label, problems)

    cc.run_case(bt, torch, oracle, case, on_launch)
    assert len(seen) == cc.launches_of(case), seen


def test_refused_arguments_launch_nothing(bt, torch, oracle):
    """Whatever btsha1_launch_column refuses is -1 with a message from
    bt_sha1_column_dev, and no kernel runs: d_state, the digests and ok keep
    their sentinel.  The 64-bit pitch / width of the entry point are refused
    when they exceed the launcher's 32 bits, never truncated into range."""
    n, w = 70, 128
    img = torch.zeros(n * 256 + 64, dtype=torch.uint8, device="cuda")
    state = torch.full((20 * n,), cc.SENT, dtype=torch.uint8, device="cuda")
    dig = torch.full((20 * n,), cc.SENT, dtype=torch.uint8, device="cuda")
    ok = torch.full((n,), cc.SENT, dtype=torch.uint8, device="cuda")
    exp = torch.zeros(20 * n, dtype=torch.uint8, device="cuda")
    p, s, d, k, e = (t.data_ptr() for t in (img, state, dig, ok, exp))
    F, M, L = cc.FIRST, cc.MIDDLE, cc.LAST
    refused = {
        "width 0": (p, n, 256, 0, F, s),
        "width no multiple of 64": (p, n, 256, 96, F, s),
        "width no multiple of 64 (LAST)": (p, n, 256, 100, L, s, 256, d),
        "pitch < width": (p, n, 64, w, F, s),
        "pitch no multiple of 16": (p, n, 136, w, M, s),
        "misaligned d_col": (p + 8, n, 256, w, F, s),
        "64 * pitch == 4 GiB": (p, n, 1 << 26, w, F, s),
        "pitch of 2^32 + 256": (p, n, (1 << 32) + 256, w, F, s),
        "width and pitch of 2^32 + 128": (p, n, (1 << 32) + 128, (1 << 32) + 128, M, s),
        "d_ok on FIRST": (p, n, 256, w, F, s, 0, None, e, k),
        "d_ok on MIDDLE": (p, n, 256, w, M, s, 0, None, e, k),
        "d_ok without d_expected": (p, n, 256, w, L, s, 256, d, None, k),
        "LAST with neither digests nor ok": (p, n, 256, w, L, s, 256, None, None, None),
        "LAST with misaligned digests": (p, n, 256, w, L, s, 256, d + 2),
        "part 3": (p, n, 256, w, 3, s),
        "part -1": (p, n, 256, w, -1, s),
        "null d_col": (None, n, 256, w, F, s),
        "null d_state": (p, n, 256, w, F, None),
    }
    accepted = []
    for name, args in refused.items():
        try:
            bt.column_dev(*args)
            accepted.append(name)
        except bt.BtSha1Error as err:
            assert "refused" in str(err) or "null pointer" in str(err), (name, str(err))
    torch.cuda.synchronize()
    assert not accepted, accepted
    for name, t in (("state", state), ("digests", dig), ("ok", ok)):
        assert bool((t == cc.SENT).all()), name
    bt.column_dev(p, 0, 256, w, F, s)  # no chunks: nothing to do, no error
    # the largest pitch the launcher takes (64 * pitch < 4 GiB) is not refused: one row, so nothing is strided
    bt.column_dev(p, 1, (1 << 26) - 16, w, F, s)
    torch.cuda.synchronize()
    got = state.cpu().numpy().view(np.uint32)
    assert [int(x) for x in got[:5]] == oracle.compress_blocks(cc.IV, bytes(w))
    assert bool((got[5:].view(np.uint8) == cc.SENT).all())
