"""GPU: the resumable chain kernel through bt_sha1_resume_dev /
bt_sha1_states_init_dev, against py_oracle.compress_blocks / py_oracle.sha1.

Advances of 0, 1, 63, 64, 65, 128 and 129 blocks (the 64-block loader
batches) singly and chained; finishes with tails r in {0, 1, 55, 56, 63} and
0, 1 or 64 whole blocks left (lens == 0 among them), after an advanced prefix
and from the IV (where the digest must also be bt_sha1_chunks_dev's); a mixed
launch of 7 at random alignments with planted mismatches; 0xFF right after
every launch's byte range; pinned host memory for the bytes and the states.
The cases live in resume_cases.py, shared with the barrier-accounting test.
"""
import pytest

import resume_cases as rc
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


@pytest.mark.parametrize("case", rc.DEVICE_CASES, ids=lambda f: f.__name__[4:])
def test_resume_dev_matches_the_oracle(bt, torch, oracle, case):
    seen = []

    def report(name, launches, problems):
        print(name, launches if len(launches) < 4 else len(launches), problems)
        seen.append(name)
        assert not problems, (name, problems)

    case(bt, torch, oracle, report)
    assert seen


def test_states_init_writes_the_iv(bt, torch):
    n = 300  # more than one block of the init kernel
    st = torch.full((5 * n + 5,), -1, dtype=torch.int32, device="cuda")
    bt.states_init_dev(st.data_ptr(), n)
    torch.cuda.synchronize()
    got = st.cpu().numpy().view("uint32")
    assert [int(x) for x in got[:5 * n]] == rc.IV * n
    assert all(int(x) == 0xFFFFFFFF for x in got[5 * n:])


def test_refused_arguments_launch_nothing(bt, torch):
    b = rc.Batch(torch, [bytes(64)])
    b.set_states([[1, 2, 3, 4, 5]])
    o = torch.zeros(1, dtype=torch.int64, device="cuda")
    ln = torch.full((1,), 64, dtype=torch.int32, device="cuda")
    tt = torch.full((1,), 64, dtype=torch.int64, device="cuda")
    args = [b.buf.data_ptr(), o.data_ptr(), ln.data_ptr(), tt.data_ptr(), 1, b.states.data_ptr(), b.dig.data_ptr(),
            None, None]
    for k in (0, 1, 2, 3, 5):
        a = list(args)
        a[k] = None
        with pytest.raises(bt.BtSha1Error, match="null pointer"):
            bt.resume_dev(*a)
    a = list(args)
    a[8] = b.ok.data_ptr()
    with pytest.raises(bt.BtSha1Error, match="d_ok needs d_expected"):
        bt.resume_dev(*a)
    a = list(args)
    a[4] = 1 << 31
    with pytest.raises(bt.BtSha1Error, match="grid limit"):
        bt.resume_dev(*a)
    torch.cuda.synchronize()
    assert b.get_states() == [[1, 2, 3, 4, 5]]
    assert b.digests() == ([bytes([rc.SENT]) * 20], rc.SENT)
