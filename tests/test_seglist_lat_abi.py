"""CPU: the knob of the latency-form gather -- bt_sha1_set_seglist_latency_batch
and bt_sha1_seglist_kernel_name -- is exported by every build of the library
and declared in include/bt_sha1.h, its launcher is not exported, and both
functions work without a device."""
import os
import re
import subprocess
import sys

import pytest

from conftest import PKG, REPO, load_btsha1

LIBS = {"product": os.path.join(PKG, "libbtsha1.so"),
        "dbgbar": os.path.join(REPO, "build_variants", "dbgbar", "libbtsha1.so"),
        "experiments": os.path.join(REPO, "build_variants", "experiments", "libbtsha1.so")}
NEW = ["bt_sha1_set_seglist_latency_batch", "bt_sha1_seglist_kernel_name"]
AUTO = 2**64 - 1


@pytest.mark.parametrize("name", LIBS)
def test_every_build_exports_the_knob_and_hides_the_launcher(name):
    assert os.path.exists(LIBS[name]), f"run make {name} first"
    out = subprocess.run(["nm", "-D", "--defined-only", LIBS[name]], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert not set(NEW) - exported, set(NEW) - exported
    other = [s for s in (l.split()[-1] for l in out.splitlines() if l.strip()) if "seglist" in s or "gather_lat" in s]
    assert all(s in NEW or re.fullmatch(r"_ZN6btsha1\d+(__device_stub__)?k_sha1_gather_lat\w*", s) for s in other), other
    assert not any("launch" in s for s in other)
    assert b"k_sha1_gather_lat" in open(LIBS[name], "rb").read()


def test_header_declares_them():
    header = open(os.path.join(REPO, "include", "bt_sha1.h")).read()
    assert re.search(r"uint64_t\s+bt_sha1_set_seglist_latency_batch\s*\(\s*uint64_t", header)
    assert re.search(r"const char \*bt_sha1_seglist_kernel_name\s*\(\s*uint64_t", header)


def test_setter_returns_the_previous_value_and_names_follow_it():
    """In a fresh process: 0 at first, then each value that was set; the name
    query follows the setting (256 compute units where no device is visible)."""
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import btsha1 as bt\n"
            "s, k = bt.set_seglist_latency_batch, bt.seglist_kernel_name\n"
            "print(s(5), k(1), k(5), k(6))\n"
            "print(s(2**64 - 1), k(5), k(6))\n"
            "print(s(0), k(1), k(64), k(128 * 1024 * 1024))\n"
            "print(s(0), k(1))\n")
    r = subprocess.run([sys.executable, "-c", code, PKG], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l.split() for l in r.stdout.strip().splitlines()]
    assert lines[0] == ["0", "k_sha1_gather_lat<2>", "k_sha1_gather_lat<2>", "k_sha1_gather"]  # now 5
    assert lines[1] == ["5", "k_sha1_gather_lat<2>", "k_sha1_gather_lat<2>"]  # now auto
    assert lines[2] == [str(AUTO), "k_sha1_gather", "k_sha1_gather", "k_sha1_gather"]  # now off
    assert lines[3] == ["0", "k_sha1_gather"]


def test_gather_dev_still_refuses_null_pointers_with_the_knob_on():
    bt = load_btsha1()
    prev = bt.set_seglist_latency_batch(AUTO)
    try:
        p = 4096  # never dereferenced: every call below is refused first
        for k in range(5):
            args = [p] * 5
            args[k] = None
            assert bt.lib.bt_sha1_gather_dev(args[0], args[1], args[2], args[3], 1, args[4], None) == -1, k
            assert "null pointer" in bt.last_error(), (k, bt.last_error())
        for k in range(6):
            args = [p] * 6
            args[k] = None
            assert bt.lib.bt_sha1_gather_verify_dev(*args[:4], 1, args[4], args[5], None, None) == -1, k
            assert "null pointer" in bt.last_error(), (k, bt.last_error())
        assert bt.lib.bt_sha1_gather_dev(None, None, None, None, 0, None, None) == 0
    finally:
        assert bt.set_seglist_latency_batch(prev) == AUTO
