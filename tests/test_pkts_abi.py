"""CPU: the packet-buffer surface -- bt_sha1_pkts_dev and
bt_sha1_pkts_verify_dev -- is exported by every build of the library and by
nothing else new, declared in include/bt_sha1.h as the binding calls it, and
refuses bad arguments with a message before any device call, so all of this
holds without a GPU."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import PKG, REPO, load_btsha1

LIBS = {"product": os.path.join(PKG, "libbtsha1.so"),
        "dbgbar": os.path.join(REPO, "build_variants", "dbgbar", "libbtsha1.so"),
        "experiments": os.path.join(REPO, "build_variants", "experiments", "libbtsha1.so")}
EXPORTED = {"bt_sha1_pkts_dev", "bt_sha1_pkts_verify_dev"}
CLOSED = r"dgram|gather|resume|receiver|states_init|intake|Intake|ISlot|table|Table|segchain|seglist|ragged_verify"
P = 4096  # any non-null address: nothing is dereferenced before the checks


@pytest.mark.parametrize("name", LIBS)
def test_every_build_exports_the_two_entry_points_and_one_kernel(name):
    assert os.path.exists(LIBS[name]), f"run make {name} first"
    out = subprocess.run(["nm", "-D", "--defined-only", LIBS[name]], capture_output=True, text=True, check=True).stdout
    names = [l.split()[-1] for l in out.splitlines()]
    new = [s for s in names if re.search(r"pkt|Pkt", s)]
    assert EXPORTED <= set(new), EXPORTED - set(new)
    # the launcher is hidden; besides the two functions only the kernel's handle and its stub are new
    other = [s for s in new if s not in EXPORTED]
    assert all(re.fullmatch(r"_ZN6btsha1\d+(__device_stub__)?k_sha1_pkts\w*", s) for s in other), other
    assert len({s for s in other if "__device_stub__" not in s}) == 1, other
    assert not [s for s in new if re.search(CLOSED, s)], new


def test_header_declares_what_the_binding_calls(tmp_path):
    header = open(os.path.join(REPO, "include", "bt_sha1.h")).read()
    for f in EXPORTED:
        assert re.search(r"\bint %s\s*\(" % f, header), f
    assert "use bt_sha1_gather_dev" in header  # where other geometries go
    src = tmp_path / "caller.c"
    src.write_text(
        '#include <stdio.h>\n#include "bt_sha1.h"\n'
        "int main(void) {\n"
        "  bt_sha1_pkt_geom g = {1500, 16, 1484, 354};\n"
        "  int bad = 0;\n"
        "  bad += bt_sha1_pkts_dev(NULL, &g, NULL, NULL, NULL, NULL, 1, NULL, NULL) != -1;\n"
        "  bad += bt_sha1_pkts_verify_dev(NULL, &g, NULL, NULL, NULL, NULL, 1, NULL, NULL, NULL, NULL) != -1;\n"
        '  printf("%d %zu %s\\n", bad, sizeof g, bt_sha1_last_error());\n'
        "  return bad;\n}\n")
    exe = tmp_path / "caller"
    subprocess.run(["gcc", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src),
                    f"-L{PKG}", "-lbtsha1", f"-Wl,-rpath,{PKG}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("0 16 null pointer"), r.stdout + r.stderr
    bt = load_btsha1()
    assert ctypes.sizeof(bt.PktGeom) == 16
    assert [f for f, _ in bt.PktGeom._fields_] == ["stride", "header", "payload", "slot_pkts"]
    assert callable(bt.pkts_dev) and callable(bt.pkts_verify_dev)


def geom(bt, stride=1500, header=16, payload=1484, slot_pkts=354):
    return ctypes.byref(bt.PktGeom(stride, header, payload, slot_pkts))


def test_null_arrays_are_refused_before_any_device_call():
    bt = load_btsha1()
    good = [P, geom(bt), P, P, P, P, 1, P, None]
    for k in (0, 1, 2, 3, 4, 5, 7):
        a = list(good)
        a[k] = None
        bt.lib.bt_sha1_intake_create(0, 0, 1, 0)  # leaves another message behind
        assert bt.lib.bt_sha1_pkts_dev(*a) == -1, k
        assert "null pointer" in bt.last_error(), (k, bt.last_error())
    good = [P, geom(bt), P, P, P, P, 1, P, P, None, None]
    for k in (0, 1, 2, 3, 4, 5, 7, 8):  # 7: d_ok without d_expected; 8: the reverse
        a = list(good)
        a[k] = None
        bt.lib.bt_sha1_intake_create(0, 0, 1, 0)
        assert bt.lib.bt_sha1_pkts_verify_dev(*a) == -1, k
        assert "null pointer" in bt.last_error(), (k, bt.last_error())
    with pytest.raises(bt.BtSha1Error, match="null pointer"):
        bt.pkts_dev(None, bt.PktGeom(1500, 16, 1484, 4), P, P, P, P, 1, P)


@pytest.mark.parametrize("g", [
    dict(stride=1502), dict(header=18, payload=1480), dict(payload=1482),  # not multiples of 4
    dict(stride=64, header=4, payload=60),                                 # payload < 64
    dict(stride=1496),                                                     # header + payload > stride
    dict(slot_pkts=0),
    dict(stride=1 << 20, slot_pkts=4097),                                  # slot_pkts * stride above 2^32
], ids=str)
def test_geometries_outside_the_rule_are_refused(g):
    bt = load_btsha1()
    for n in (0, 1):  # refused whatever n is: the geometry is checked first
        bt.lib.bt_sha1_intake_create(0, 0, 1, 0)
        assert bt.lib.bt_sha1_pkts_dev(P, geom(bt, **g), P, P, P, P, n, P, None) == -1, (g, n)
        assert "pkts: geometry" in bt.last_error() and "outside the rule" in bt.last_error(), bt.last_error()
        assert bt.lib.bt_sha1_pkts_verify_dev(P, geom(bt, **g), P, P, P, P, n, P, P, None, None) == -1, (g, n)
        assert "outside the rule" in bt.last_error()


def test_the_largest_slot_is_taken_and_the_grid_limit_refused():
    bt = load_btsha1()
    # slot_pkts * stride == 2^32 exactly is inside the rule; n == 0 is no work
    assert bt.lib.bt_sha1_pkts_dev(P, geom(bt, stride=1 << 20, slot_pkts=4096), P, P, P, P, 0, P, None) == 0
    assert bt.lib.bt_sha1_pkts_verify_dev(P, geom(bt), P, P, P, P, 0, P, P, None, None) == 0
    for n in ((0x7fffffff * 64) + 1, (1 << 64) - 1):
        assert bt.lib.bt_sha1_pkts_dev(P, geom(bt), P, P, P, P, n, P, None) == -1, n
        assert "grid limit" in bt.last_error()
