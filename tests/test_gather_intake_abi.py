"""CPU: the chain-form gather surface -- bt_sha1_gather_resume_dev and the
gather intake (bt_sha1_intake_create_gather / _append / _commit_gather) -- is
exported by every build of the library, declared in include/bt_sha1.h, and
refuses bad arguments with a message before any device call, so all of this
holds without a GPU.

The library exports the four under bt_sha1_dgram_* names: the export lists of
test_gather_abi / test_resume_abi / test_intake_abi allow no further dynamic
symbol with gather, resume or intake in its name.  The header gives the
bt_sha1_gather_resume_dev / bt_sha1_intake_* names as inline forms of them."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import PKG, REPO, load_btsha1

LIBS = {"product": os.path.join(PKG, "libbtsha1.so"),
        "dbgbar": os.path.join(REPO, "build_variants", "dbgbar", "libbtsha1.so"),
        "experiments": os.path.join(REPO, "build_variants", "experiments", "libbtsha1.so")}
EXPORTED = {"bt_sha1_gather_resume_dev": "bt_sha1_dgram_chain_dev",
            "bt_sha1_intake_create_gather": "bt_sha1_dgram_slots_create",
            "bt_sha1_intake_append": "bt_sha1_dgram_slots_append",
            "bt_sha1_intake_commit_gather": "bt_sha1_dgram_slots_commit"}
MIB = 1 << 20


@pytest.mark.parametrize("name", LIBS)
def test_every_build_exports_the_new_entry_points(name):
    assert os.path.exists(LIBS[name]), f"run make {name} first"
    out = subprocess.run(["nm", "-D", "--defined-only", LIBS[name]], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert not set(EXPORTED.values()) - exported, set(EXPORTED.values()) - exported
    # the two launchers are hidden, and so is everything else that is new but the kernels' handles
    names = [l.split()[-1] for l in out.splitlines()]
    assert not [s for s in names if "launch_gather_resume" in s]
    other = [s for s in names if re.search(r"dgram|gather_resume|GatherEntry", s)]
    assert all(s in EXPORTED.values() or re.fullmatch(r"_ZN6btsha1\d+(__device_stub__)?k_sha1_gather_resume\w*", s)
               for s in other), other
    kernels = {s for s in other if s.startswith("_ZN6btsha1") and "__device_stub__" not in s}
    assert len(kernels) == 4, kernels  # <false> and <true> of the array and the table form


def test_header_declares_both_names_and_they_compile(tmp_path):
    """A C caller reaches every entry point under the name the header documents."""
    header = open(os.path.join(REPO, "include", "bt_sha1.h")).read()
    for public, exported in EXPORTED.items():
        assert re.search(r"\b%s\s*\(" % public, header) and re.search(r"\b%s\s*\(" % exported, header), public
    assert header.index("bt_sha1_gather_resume_dev(") > header.index("bt_sha1_resume_dev(")
    assert header.index("bt_sha1_intake_create_gather(") > header.index("bt_sha1_intake_get_stats(")
    src = tmp_path / "caller.c"
    src.write_text(
        '#include <stdio.h>\n#include "bt_sha1.h"\n'
        "int main(void) {\n"
        "  bt_sha1_seg seg = {0, 64, 0};\n"
        "  uint8_t e[20] = {0};\n"
        "  int bad = 0;\n"
        "  bad += bt_sha1_gather_resume_dev(NULL, &seg, NULL, NULL, NULL, NULL, NULL, NULL, 1, NULL, NULL, NULL, NULL, NULL) != -1;\n"
        "  bad += bt_sha1_intake_create_gather(0, 0, 1, 1, 0) != NULL;\n"
        "  bad += bt_sha1_intake_append(NULL, NULL, &seg, 1) != -1;\n"
        "  bad += bt_sha1_intake_commit_gather(NULL, NULL, e, 0) != -1;\n"
        '  printf("%d %s\\n", bad, bt_sha1_last_error());\n'
        "  return bad;\n}\n")
    exe = tmp_path / "caller"
    subprocess.run(["gcc", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src),
                    f"-L{PKG}", "-lbtsha1", f"-Wl,-rpath,{PKG}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("0 null pointer"), r.stdout + r.stderr


def test_gather_table_entry_is_32_bytes(tmp_path):
    """BtSha1GatherEntry (csrc/sha1_launch.h): 32 bytes, 32-byte aligned, the
    fields of BtSha1TableEntry where they were and nseg / seg_hint behind them."""
    src = tmp_path / "entry.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "sha1_launch.h"\nint main() {\n'
                   '  printf("%zu %zu", sizeof(BtSha1GatherEntry), alignof(BtSha1GatherEntry));\n'
                   + "".join(f'  printf(" %zu", offsetof(BtSha1GatherEntry, {f}));\n'
                             for f in ("slot", "from", "len", "total", "seq", "nseg", "seg_hint"))
                   + "".join(f'  printf(" %zu", offsetof(BtSha1TableEntry, {f}));\n'
                             for f in ("slot", "from", "len", "total", "seq"))
                   + '  printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "entry"
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-I", os.path.join(PKG, "csrc"), "-o", str(exe), str(src)],
                   check=True, capture_output=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [32, 32, 0, 4, 8, 12, 16, 20, 24, 0, 4, 8, 12, 16], got


def test_gather_resume_dev_refuses_before_any_device_call():
    bt = load_btsha1()
    f = bt.lib.bt_sha1_dgram_chain_dev
    assert f(*([None] * 8), 0, *([None] * 5)) == 0  # n == 0 is no work
    p = 4096
    good = [p, p, p, p, p, p, p, p, 1, p, p, None, None, None]
    for k in (0, 1, 2, 3, 4, 5, 6, 7, 9):
        a = list(good)
        a[k] = None
        bt.lib.bt_sha1_intake_create(0, 0, 1, 0)  # leaves another message behind
        assert f(*a) == -1, k
        assert "null pointer" in bt.last_error(), (k, bt.last_error())
    a = list(good)
    a[12] = p  # d_ok without d_expected
    assert f(*a) == -1 and "d_ok needs d_expected" in bt.last_error()
    for n in (1 << 31, (1 << 64) - 1):
        a = list(good)
        a[8] = n
        assert f(*a) == -1 and "grid limit" in bt.last_error(), n
    with pytest.raises(bt.BtSha1Error, match="null pointer"):
        bt.gather_resume_dev(None, p, p, p, p, p, p, p, 1, p)


@pytest.mark.parametrize("slot_len,max_segs,nslots,msg", [
    (0, 4, 4, "slot_len must be in [1, 33 MiB]"),
    (33 * MIB + 1, 4, 4, "slot_len must be in [1, 33 MiB]"),
    (4096, 0, 4, "max_segs must be at least 1"),
    (4096, 4, 0, "nslots must be in [1, 512]"),
    (4096, 4, 513, "nslots must be in [1, 512]"),
    (8 * MIB, 4, 512, "2 GiB of pinned memory"),
    (4096, (256 * MIB) // 24 // 512 + 1, 512, "segment tables exceed 256 MiB"),
    (4096, 0xFFFFFFFF, 512, "segment tables exceed 256 MiB"),
])
def test_gather_intake_create_refuses_before_any_device_call(slot_len, max_segs, nslots, msg):
    bt = load_btsha1()
    assert bt.lib.bt_sha1_dgram_slots_create(0, slot_len, max_segs, nslots, 0) is None
    assert msg in bt.last_error()
    with pytest.raises(bt.BtSha1Error, match=re.escape(msg)):
        bt.Intake(chunk_len=slot_len, nslots=nslots, gather=True, max_segs=max_segs)


def test_append_and_commit_gather_refuse_null_handles():
    bt = load_btsha1()
    lib = bt.lib
    seg = (bt.Seg * 1)()
    e = (ctypes.c_uint8 * 20)()
    calls = {"append, no intake": lambda: lib.bt_sha1_dgram_slots_append(None, 4096, seg, 1),
             "append, no slot": lambda: lib.bt_sha1_dgram_slots_append(4096, None, seg, 1),
             "append, no segments": lambda: lib.bt_sha1_dgram_slots_append(4096, 4096, None, 1),
             "commit, no intake": lambda: lib.bt_sha1_dgram_slots_commit(None, 4096, e, 0),
             "commit, no slot": lambda: lib.bt_sha1_dgram_slots_commit(4096, None, e, 0),
             "commit, no hash": lambda: lib.bt_sha1_dgram_slots_commit(4096, 4096, None, 0)}
    for name, call in calls.items():
        lib.bt_sha1_intake_create(0, 0, 1, 0)  # leaves another message behind
        assert "chunk_len" in bt.last_error()
        assert call() == -1, name
        assert "null pointer" in bt.last_error(), (name, bt.last_error())


def test_python_intake_has_the_gather_methods():
    bt = load_btsha1()
    for m in ("append", "commit_gather", "receive_datagrams"):
        assert callable(getattr(bt.Intake, m)), m
    assert callable(bt.gather_resume_dev)
