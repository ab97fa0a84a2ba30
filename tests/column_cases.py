"""Shared by test_gpu_columns.py (product library) and test_gpu_barriers.py
(barrier-accounting build): whole FIRST -> MIDDLE.. -> LAST sequences of
k_sha1_lat's column forms, one bt_sha1_column_dev call per launch, each checked
against the oracle.

A case is n chunks of chunk_len bytes cut into columns [(offset, width)].
"inplace": the columns are hashed where they lie in the row-major image
(pitch = chunk_len > width).  "dense": each column is gathered on the host
into its own column-major block (pitch == width), the blocks back to back in
one device buffer, as the host pipelines and the verifier lay them out.

Checked after every launch (run_case):
  FIRST / MIDDLE  all 5 x n words of d_state (word k of chunk i at
                  state[k*n + i]) == compress_blocks(IV, chunk[:prefix]);
  LAST            the digests == sha1(chunk), bit-exact; with the fused
                  compare, ok == the planted pattern (every 7th expectation is
                  wrong); d_state as the last MIDDLE / FIRST left it;
  always          the 64 entries past the end of d_state, the digests and ok
                  still hold the sentinel: lanes at or past nvalid store nothing.
"""
import collections

import numpy as np

IV = (0x67452301, 0xEFCDAB89, 0x98BADCFE, 0x10325476, 0xC3D2E1F0)
FIRST, MIDDLE, LAST = 0, 1, 2
GUARD = 64  # canary entries past each output
SENT = 0xA5  # canary byte
SEED = 0xC01C

Case = collections.namedtuple("Case", "name n chunk_len layout cols null_digest_run")


def cases(cus):
    """Cases a to d.  `wide` chunks fill one workgroup per CU: one more takes
    the 3-slot form (launch_column_m: ceil(n / 64) > CUs)."""
    wide = 64 * cus
    abc = [(0, 64), (64, 128), (192, 192)]  # 1, 2 and 3 blocks
    ring = [(320 * j, 320) for j in range(4)]  # 5 blocks: S's 4-deep ring wraps with nblocks % 4 == 1
    return [
        Case("a in place 2-slot", 100, 384, "inplace", abc, False),
        Case("b in place 3-slot odd row", wide + 1, 384, "inplace", abc, False),
        Case("c dense 2-slot", 130, 1280, "dense", ring, False),
        Case("c dense 3-slot", wide + 64, 1280, "dense", ring, False),
        # FIRST + LAST only, no MIDDLE; also LAST with the fused compare and no digest buffer
        Case("d two columns 3-slot", wide + 64, 2048, "inplace", [(0, 1024), (1024, 1024)], True),
    ]


def launches_of(case):
    """Launches run_case makes for a case: every column but the last once,
    LAST plain and with the fused compare (+ once without a digest buffer)."""
    return len(case.cols) - 1 + (3 if case.null_digest_run else 2)


_refs = {}


def reference(orc, case):
    """(image as an (n, chunk_len) uint8 array, digests as bytes, [state after
    column j as a (5, n) uint32 array]) -- computed once per case."""
    key = (case.n, case.chunk_len, tuple(case.cols))
    if key not in _refs:
        n, cl = case.n, case.chunk_len
        raw = orc.fill_synthetic(n * cl, 131 * n + cl, SEED)  # one stream of distinct words: every chunk distinct
        img = np.frombuffer(bytes(raw), dtype=np.uint8).reshape(n, cl)
        digests = b"".join(orc.hash_chunks(raw, cl, nthreads=8))
        states = []
        for off, w in case.cols[:-1]:
            st = np.empty((5, n), dtype=np.uint32)
            for i in range(n):
                st[:, i] = orc.compress_blocks(IV, img[i, :off + w].tobytes())
            states.append(st)
        img.setflags(write=False)
        _refs[key] = (img, digests, states)
    return _refs[key]


def barrier_want(n, width, part, cus):
    """(waves, barriers) one column launch adds to the barrier build's tallies."""
    grid = (n + 63) // 64
    slots = 3 if grid > cus else 2
    nb = width // 64 + (1 if part == LAST else 0)  # FIRST / MIDDLE: no padding block
    return (2 * grid, 2 * grid * (nb + slots - 1))


def run_case(bt, torch, orc, case, on_launch):
    """Runs the case's launches; after each, on_launch(label, n, width, part,
    problems) with the list of what differed from the reference (empty: all
    exact)."""
    n, cl = case.n, case.chunk_len
    img, want_dig, want_states = reference(orc, case)
    if case.layout == "inplace":
        d_img = torch.from_numpy(img.reshape(-1).copy()).cuda()
        cols = [(d_img.data_ptr() + off, cl, w) for off, w in case.cols]
    else:
        gathered = np.concatenate([np.ascontiguousarray(img[:, off:off + w]).reshape(-1) for off, w in case.cols])
        d_img = torch.from_numpy(gathered).cuda()
        at, cols = 0, []
        for off, w in case.cols:
            cols.append((d_img.data_ptr() + at, w, w))
            at += n * w
    state = torch.full((4 * (5 * n + GUARD),), SENT, dtype=torch.uint8, device="cuda")  # uint32 words

    def state_now():
        torch.cuda.synchronize()
        return state.cpu().numpy().view(np.uint32)

    def tail_ok(arr, used):
        return arr[used:].size == GUARD and bool((arr[used:].view(np.uint8) == SENT).all())

    for j, (ptr, pitch, w) in enumerate(cols[:-1]):
        part = FIRST if j == 0 else MIDDLE
        bt.column_dev(ptr, n, pitch, w, part, state.data_ptr())
        got = state_now()
        bad = []
        if not np.array_equal(got[:5 * n], want_states[j].reshape(-1)):
            wrong = np.nonzero(got[:5 * n] != want_states[j].reshape(-1))[0]
            bad.append(f"{len(wrong)} state words differ, first at word {wrong[0] // n} of chunk {wrong[0] % n}")
        if not tail_ok(got, 5 * n):
            bad.append("state written past 5 * n words")
        on_launch(f"{case.name}: {'FIRST' if j == 0 else 'MIDDLE'} column {j} width {w}", n, w, part, bad)

    ptr, pitch, w = cols[-1]
    state_in = state_now().copy()
    exp = bytearray(want_dig)
    for i in range(0, n, 7):
        exp[20 * i] ^= 1  # every 7th chunk must fail util.c:313's compare
    want_ok = np.array([0 if i % 7 == 0 else 1 for i in range(n)], dtype=np.uint8)
    d_exp = torch.from_numpy(np.frombuffer(bytes(exp), dtype=np.uint8).copy()).cuda()
    runs = [("LAST", True, False), ("LAST + verify", True, True)]
    if case.null_digest_run:
        runs.insert(0, ("LAST + verify, no digest buffer", False, True))
    for label, with_dig, verify in runs:
        dig = torch.full((20 * (n + GUARD),), SENT, dtype=torch.uint8, device="cuda")
        ok = torch.full((n + GUARD,), SENT, dtype=torch.uint8, device="cuda")
        bt.column_dev(ptr, n, pitch, w, LAST, state.data_ptr(), cl, dig.data_ptr() if with_dig else None,
                      d_exp.data_ptr() if verify else None, ok.data_ptr() if verify else None)
        torch.cuda.synchronize()
        got_dig, got_ok = dig.cpu().numpy(), ok.cpu().numpy()
        bad = []
        if with_dig and got_dig[:20 * n].tobytes() != want_dig:
            wrong = [i for i in range(n) if got_dig[20 * i:20 * i + 20].tobytes() != want_dig[20 * i:20 * i + 20]]
            bad.append(f"{len(wrong)} digests differ, first chunk {wrong[0]}")
        if not (got_dig[20 * n if with_dig else 0:] == SENT).all():
            bad.append("digest bytes written past 20 * n" if with_dig else "digests written without a digest buffer")
        if verify and not np.array_equal(got_ok[:n], want_ok):
            wrong = np.nonzero(got_ok[:n] != want_ok)[0]
            bad.append(f"{len(wrong)} verdicts differ, first chunk {wrong[0]}")
        if not (got_ok[n if verify else 0:] == SENT).all():
            bad.append("ok written past n" if verify else "ok written without the fused compare")
        if not np.array_equal(state_now(), state_in):
            bad.append("LAST changed d_state")
        on_launch(f"{case.name}: {label} column {len(cols) - 1} width {w}", n, w, LAST, bad)
