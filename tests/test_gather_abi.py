"""CPU: the scatter-gather surface -- bt_sha1_gather_dev,
bt_sha1_gather_verify_dev, bt_sha1_verifier_create_gather,
bt_sha1_verifier_commit_gather, bt_sha1_verifier_get_gather_stats -- is
exported by every build of the library, declared in include/bt_sha1.h where it
belongs, and refuses bad arguments with a message before any device call, so
all of this holds without a GPU."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import PKG, REPO, load_btsha1

LIBS = {"product": os.path.join(PKG, "libbtsha1.so"),
        "dbgbar": os.path.join(REPO, "build_variants", "dbgbar", "libbtsha1.so"),
        "experiments": os.path.join(REPO, "build_variants", "experiments", "libbtsha1.so")}
NEW = ["bt_sha1_gather_dev", "bt_sha1_gather_verify_dev", "bt_sha1_verifier_create_gather",
       "bt_sha1_verifier_commit_gather", "bt_sha1_verifier_get_gather_stats"]
CREATE_MSG = "slot_len must be in [1, 33 MiB], max_segs > 0, batch > 0 and batch x max_segs x 16 <= 256 MiB"


@pytest.mark.parametrize("name", LIBS)
def test_every_build_exports_the_gather_surface(name):
    assert os.path.exists(LIBS[name]), f"run make {name} first"
    out = subprocess.run(["nm", "-D", "--defined-only", LIBS[name]], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert not set(NEW) - exported, set(NEW) - exported
    # the launcher is hidden; besides the C functions only the kernels' handles carry the name
    other = [l.split()[-1] for l in out.splitlines() if re.search(r"gather", l)]
    assert all(s in NEW or re.fullmatch(r"_ZN6btsha1\d+(__device_stub__)?k_sha1_gather\w*", s) for s in other), other
    assert not any("launch_gather" in s for s in other)


def test_header_declares_them_in_place():
    header = open(os.path.join(REPO, "include", "bt_sha1.h")).read()
    assert all(re.search(r"\b%s\s*\(" % f, header) for f in NEW)
    pos = [header.index(f + "(") for f in ("bt_sha1_ragged_verify_dev", "bt_sha1_gather_dev",
                                           "bt_sha1_gather_verify_dev", "bt_sha1_resume_dev")]
    assert pos == sorted(pos)
    # directly after bt_sha1_ragged_verify_dev: no other function between them
    between = header[header.index(";", pos[0]):pos[1]]
    assert re.findall(r"^\w[\w \*]*\b(\w+)\(", between, re.M) == [], between


def test_gather_dev_refuses_before_any_device_call():
    bt = load_btsha1()
    lib = bt.lib
    assert lib.bt_sha1_gather_dev(None, None, None, None, 0, None, None) == 0
    assert lib.bt_sha1_gather_verify_dev(None, None, None, None, 0, None, None, None, None) == 0
    p = 4096  # never dereferenced: every call below is refused first
    for k, name in enumerate(("d_base", "d_segs", "d_seg_first", "d_seg_count", "d_digests")):
        args = [p] * 5
        args[k] = None
        lib.bt_sha1_verifier_create_gather(0, 0, 1, 1, 2)  # leaves another message behind
        assert "slot_len" in bt.last_error()
        assert lib.bt_sha1_gather_dev(args[0], args[1], args[2], args[3], 1, args[4], None) == -1, name
        assert "null pointer" in bt.last_error(), (name, bt.last_error())
        with pytest.raises(bt.BtSha1Error, match="null pointer"):
            bt.gather_dev(args[0], args[1], args[2], args[3], 1, args[4])
    for k, name in enumerate(("d_base", "d_segs", "d_seg_first", "d_seg_count", "d_expected", "d_ok")):
        args = [p] * 6
        args[k] = None
        lib.bt_sha1_verifier_create_gather(0, 0, 1, 1, 2)
        assert lib.bt_sha1_gather_verify_dev(*args[:4], 1, args[4], args[5], None, None) == -1, name
        assert "null pointer" in bt.last_error(), (name, bt.last_error())
        with pytest.raises(bt.BtSha1Error, match="null pointer"):
            bt.gather_verify_dev(*args[:4], 1, args[4], args[5])
    limit = 0x7fffffff * 64
    for n in (limit + 1, (1 << 64) - 1):
        assert lib.bt_sha1_gather_dev(p, p, p, p, n, p, None) == -1
        assert "grid limit" in bt.last_error() and str(n) in bt.last_error(), bt.last_error()
        assert lib.bt_sha1_gather_verify_dev(p, p, p, p, n, p, p, None, None) == -1
        assert "grid limit" in bt.last_error() and str(limit) in bt.last_error(), bt.last_error()


@pytest.mark.parametrize("slot_len,max_segs,batch", [(0, 8, 8), ((33 << 20) + 1, 8, 8), (7500, 0, 8), (7500, 8, 0),
                                                     (7500, 1 << 16, (1 << 8) + 1), (7500, 0xFFFFFFFF, 0xFFFFFFFF)])
def test_gather_verifier_create_refuses_before_any_device_call(slot_len, max_segs, batch):
    bt = load_btsha1()
    assert bt.lib.bt_sha1_verifier_create_gather(0, slot_len, max_segs, batch, 2) is None
    assert CREATE_MSG in bt.last_error()
    with pytest.raises(bt.BtSha1Error, match=re.escape(CREATE_MSG)):
        bt.Verifier(chunk_len=slot_len, batch=batch, gather=True, max_segs=max_segs)


def test_commit_gather_and_stats_refuse_null_pointers():
    bt = load_btsha1()
    s = bt.VerifierGatherStats()
    e = (ctypes.c_uint8 * 20)()
    seg = (bt.Seg * 1)()
    for call in (lambda: bt.lib.bt_sha1_verifier_get_gather_stats(None, ctypes.byref(s)),
                 lambda: bt.lib.bt_sha1_verifier_commit_gather(None, 4096, seg, 1, e, 0)):
        bt.lib.bt_sha1_verifier_create_gather(0, 0, 1, 1, 2)
        assert call() == -1
        assert "null pointer" in bt.last_error()


def c_layout(tmp_path, struct, fields):
    src = tmp_path / f"{struct}.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bt_sha1.h"\nint main(void) {\n'
                   f'  printf("size %zu\\n", sizeof({struct}));\n'
                   + "".join(f'  printf("{f} %zu\\n", offsetof({struct}, {f}));\n' for f in fields)
                   + "  return 0;\n}\n")
    exe = tmp_path / struct
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    return {k: int(v) for k, v in (l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                                     check=True).stdout.splitlines())}


def test_ctypes_layouts_equal_the_c_ones(tmp_path):
    bt = load_btsha1()
    for cls, struct, fields in ((bt.Seg, "bt_sha1_seg", ["off", "len", "reserved"]),
                                (bt.VerifierGatherStats, "bt_sha1_verifier_gather_stats",
                                 ["gather_batches", "gather_chunks", "segments", "payload_bytes", "copied_bytes"])):
        assert [f for f, _ in cls._fields_] == fields
        got = c_layout(tmp_path, struct, fields)
        assert got["size"] == ctypes.sizeof(cls), struct
        for f in fields:
            assert got[f] == getattr(cls, f).offset, (struct, f)
    assert ctypes.sizeof(bt.Seg) == 16
    # bt_sha1_verifier_stats keeps its five fields
    five = ["batches", "ragged_batches", "chunks", "short_chunks", "released"]
    assert [f for f, _ in bt.VerifierStats._fields_] == five
    assert c_layout(tmp_path, "bt_sha1_verifier_stats", five)["size"] == 40


def test_python_surface():
    import inspect
    bt = load_btsha1()
    assert callable(bt.gather_dev) and callable(bt.gather_verify_dev)
    assert callable(bt.Verifier.commit_gather) and callable(bt.Verifier.gather_stats)
    p = inspect.signature(bt.Verifier.__init__).parameters
    assert p["gather"].default is False and p["max_segs"].default == 0 and p["ragged"].default is False
    assert list(p)[:6] == ["self", "device", "chunk_len", "batch", "nstreams", "ragged"]
