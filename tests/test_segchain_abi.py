"""CPU: the chain form of whole segment lists -- its knob
bt_sha1_set_segchain_batch and its diagnostic launch bt_sha1_segchain_dev --
is exported by every build of the library and declared in include/bt_sha1.h,
its launcher is not exported, the knob moves bt_sha1_seglist_kernel_name as
documented, and bad arguments are refused with a message before any device
call, so all of this holds without a GPU."""
import os
import re
import subprocess
import sys

import pytest

from conftest import PKG, REPO, load_btsha1

LIBS = {"product": os.path.join(PKG, "libbtsha1.so"),
        "dbgbar": os.path.join(REPO, "build_variants", "dbgbar", "libbtsha1.so"),
        "experiments": os.path.join(REPO, "build_variants", "experiments", "libbtsha1.so")}
NEW = ["bt_sha1_set_segchain_batch", "bt_sha1_segchain_dev"]
AUTO = 2**64 - 1


@pytest.mark.parametrize("name", LIBS)
def test_every_build_exports_them_and_hides_the_launcher(name):
    assert os.path.exists(LIBS[name]), f"run make {name} first"
    out = subprocess.run(["nm", "-D", "--defined-only", LIBS[name]], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert not set(NEW) - exported, set(NEW) - exported
    other = [s for s in (l.split()[-1] for l in out.splitlines() if l.strip()) if "segchain" in s or "gather_chain" in s]
    assert all(s in NEW or re.fullmatch(r"_ZN6btsha1\d+(__device_stub__)?k_sha1_gather_chain\w*", s) for s in other), other
    assert not any("launch" in s for s in other)
    assert b"k_sha1_gather_chain" in open(LIBS[name], "rb").read()


def test_header_declares_them():
    header = open(os.path.join(REPO, "include", "bt_sha1.h")).read()
    assert re.search(r"uint64_t\s+bt_sha1_set_segchain_batch\s*\(\s*uint64_t", header)
    assert re.search(r"int\s+bt_sha1_segchain_dev\s*\(\s*const void \*d_base,\s*const bt_sha1_seg \*d_segs", header)
    assert re.search(r"uint32_t piece_bytes,\s*void \*stream\)", header)


def test_setter_returns_the_previous_value_and_names_follow_it():
    """In a fresh process: 0 at first, then each value that was set; the chain
    form is asked before the latency form; AUTO is two per compute unit (256
    where no device is visible); back at 0 the names are what they were."""
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import btsha1 as bt\n"
            "s, l, k = bt.set_segchain_batch, bt.set_seglist_latency_batch, bt.seglist_kernel_name\n"
            "print(s(4), k(1), k(4), k(5))\n"
            "print(l(2**64 - 1), k(4), k(5))\n"
            "print(l(0), s(2**64 - 1), k(512), k(513))\n"
            "print(s(0), k(1), k(64), k(128 * 1024 * 1024))\n"
            "print(l(5), k(1), k(5), k(6))\n"
            "print(s(0), l(0), k(1))\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-c", code, PKG], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l.split() for l in r.stdout.strip().splitlines()]
    assert lines[0] == ["0", "k_sha1_gather_chain", "k_sha1_gather_chain", "k_sha1_gather"]  # now 4
    assert lines[1] == ["0", "k_sha1_gather_chain", "k_sha1_gather_lat<2>"]  # the latency knob on as well
    assert lines[2] == [str(AUTO), "4", "k_sha1_gather_chain", "k_sha1_gather"]  # auto without a device: 512
    assert lines[3] == [str(AUTO), "k_sha1_gather", "k_sha1_gather", "k_sha1_gather"]  # now off
    assert lines[4] == ["0", "k_sha1_gather_lat<2>", "k_sha1_gather_lat<2>", "k_sha1_gather"]  # as test_seglist_lat_abi
    assert lines[5] == ["0", "5", "k_sha1_gather"]


def test_segchain_dev_refuses_before_any_device_call():
    bt = load_btsha1()
    lib = bt.lib
    p = 4096  # never dereferenced: every call below is refused first
    assert lib.bt_sha1_segchain_dev(None, None, None, None, 0, None, None, None, 0, None) == 0
    assert lib.bt_sha1_segchain_dev(p, p, p, p, 0, None, None, None, 32, None) == 0
    for k, name in enumerate(("d_base", "d_segs", "d_seg_first", "d_seg_count")):
        args = [p] * 4
        args[k] = None
        lib.bt_sha1_verifier_create_gather(0, 0, 1, 1, 2)  # leaves another message behind
        assert "slot_len" in bt.last_error()
        assert lib.bt_sha1_segchain_dev(*args, 1, p, p, p, 0, None) == -1, name
        assert "null pointer" in bt.last_error(), (name, bt.last_error())
        with pytest.raises(bt.BtSha1Error, match="null pointer"):
            bt.segchain_dev(*args, 1, d_digests=p)
    for exp, ok, dig, msg in ((None, p, p, "come together"), (p, None, p, "come together"),
                              (None, None, None, "nothing to write")):
        lib.bt_sha1_verifier_create_gather(0, 0, 1, 1, 2)
        assert lib.bt_sha1_segchain_dev(p, p, p, p, 1, exp, ok, dig, 0, None) == -1, msg
        assert msg in bt.last_error(), bt.last_error()
    for piece in (32, 96, 2**31 + 64):
        lib.bt_sha1_verifier_create_gather(0, 0, 1, 1, 2)
        assert lib.bt_sha1_segchain_dev(p, p, p, p, 1, p, p, p, piece, None) == -1, piece
        assert "64-byte multiple" in bt.last_error() and str(piece) in bt.last_error(), bt.last_error()
    for n in (2**31, 2**64 - 1):
        assert lib.bt_sha1_segchain_dev(p, p, p, p, n, p, p, p, 0, None) == -1
        assert "grid limit" in bt.last_error() and str(n) in bt.last_error(), bt.last_error()


def test_python_surface():
    import inspect
    bt = load_btsha1()
    assert callable(bt.set_segchain_batch) and callable(bt.segchain_dev)
    p = inspect.signature(bt.segchain_dev).parameters
    assert list(p) == ["d_base", "d_segs", "d_seg_first", "d_seg_count", "n", "d_expected", "d_ok", "d_digests",
                       "piece_bytes", "stream"]
    assert p["piece_bytes"].default == 0 and p["d_digests"].default is None
    assert bt.set_segchain_batch(0) == 0  # off by default, and left off


def test_verify_stream_takes_the_switch_only_with_datagram_slots(tmp_path):
    """-c without -G is refused with status 255 before any file is opened or a device touched."""
    exe = os.path.join(PKG, "bin", "verify-stream")
    assert os.path.exists(exe), "run make tools first"
    for args in (["-c"], ["-z", "-c"]):
        r = subprocess.run([exe, *args, str(tmp_path / "missing.img"), str(tmp_path / "missing.chunks")],
                           capture_output=True, text=True, timeout=60)
        assert r.returncode == 255 and "it needs -G" in r.stderr, (args, r.returncode, r.stderr)
    usage = subprocess.run([exe], capture_output=True, text=True, timeout=60).stderr
    assert "-G [-c]" in usage
