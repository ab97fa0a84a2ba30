"""CPU: the many-chunk progressive receive object (bt_sha1_intake_*) is exported
by every build of the library, declared in include/bt_sha1.h, and refuses bad
arguments with a message before any device call -- so all of this holds
without a GPU."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import PKG, REPO, load_btsha1

LIBS = {"product": os.path.join(PKG, "libbtsha1.so"),
        "dbgbar": os.path.join(REPO, "build_variants", "dbgbar", "libbtsha1.so"),
        "experiments": os.path.join(REPO, "build_variants", "experiments", "libbtsha1.so")}
# every function the header's intake section declares
NEW = ["bt_sha1_intake_" + f for f in ("create", "destroy", "slot", "advance", "commit", "release", "kick", "sync",
                                       "poll", "drain", "pending", "get_stats")]


@pytest.mark.parametrize("name", LIBS)
def test_every_build_exports_the_intake(name):
    assert os.path.exists(LIBS[name]), f"run make {name} first"
    out = subprocess.run(["nm", "-D", "--defined-only", LIBS[name]], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert not set(NEW) - exported, set(NEW) - exported
    # the table launcher and the object's internals are hidden; only the new kernel's handles carry its name
    other = [l.split()[-1] for l in out.splitlines() if re.search(r"intake|Intake|ISlot|table|Table", l)]
    assert all(s in NEW or re.fullmatch(r"_ZN6btsha1\d+(__device_stub__)?k_sha1_\w+", s) for s in other), other
    header = open(os.path.join(REPO, "include", "bt_sha1.h")).read()
    assert all(re.search(r"\b%s\s*\(" % f, header) for f in NEW)
    assert header.index("bt_sha1_intake_create") > header.index("bt_sha1_receiver_get_stats")
    assert not [f for f in NEW if "receiver" in f or "resume" in f]


@pytest.mark.parametrize("chunk_len,nslots,msg", [
    (0, 4, "chunk_len must be in [1, 32 MiB]"),
    ((32 << 20) + 1, 4, "chunk_len must be in [1, 32 MiB]"),
    (4096, 0, "nslots must be in [1, 512]"),
    (4096, 513, "nslots must be in [1, 512]"),
    (8 << 20, 512, "2 GiB of pinned memory"),
])
def test_intake_create_refuses_before_any_device_call(chunk_len, nslots, msg):
    bt = load_btsha1()
    assert bt.lib.bt_sha1_intake_create(0, chunk_len, nslots, 0) is None
    assert msg in bt.last_error()
    with pytest.raises(bt.BtSha1Error, match=re.escape(msg)):
        bt.Intake(chunk_len=chunk_len, nslots=nslots)


def test_intake_calls_refuse_null_handles():
    bt = load_btsha1()
    lib = bt.lib
    out = (bt.Verdict * 1)()
    e = (ctypes.c_uint8 * 20)()
    calls = {"advance": lambda: lib.bt_sha1_intake_advance(None, 4096, 64),
             "commit": lambda: lib.bt_sha1_intake_commit(None, 4096, 64, e, 0),
             "release": lambda: lib.bt_sha1_intake_release(None, 4096),
             "kick": lambda: lib.bt_sha1_intake_kick(None),
             "sync": lambda: lib.bt_sha1_intake_sync(None),
             "poll": lambda: lib.bt_sha1_intake_poll(None, out, 1),
             "drain": lambda: lib.bt_sha1_intake_drain(None, out, 1),
             "pending": lambda: lib.bt_sha1_intake_pending(None),
             "get_stats": lambda: lib.bt_sha1_intake_get_stats(None, None)}
    for name, call in calls.items():
        lib.bt_sha1_intake_create(0, 0, 1, 0)  # leaves another message behind
        assert "chunk_len" in bt.last_error()
        assert call() == -1, name
        assert "null pointer" in bt.last_error(), (name, bt.last_error())
    lib.bt_sha1_intake_create(0, 0, 1, 0)
    assert lib.bt_sha1_intake_slot(None) is None and "null pointer" in bt.last_error()
    lib.bt_sha1_intake_destroy(None)  # like free(NULL)


def test_intake_stats_layout(tmp_path):
    """The ctypes mirror btsha1.IntakeStats has the C struct's size and offsets."""
    bt = load_btsha1()
    fields = [f for f, _ in bt.IntakeStats._fields_]
    assert fields == ["kicks", "launches", "entries", "max_entries", "advanced_bytes", "committed", "released",
                      "deferred"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bt_sha1.h"\nint main(void) {\n'
                   '  printf("size %zu\\n", sizeof(bt_sha1_intake_stats));\n'
                   + "".join(f'  printf("{f} %zu\\n", offsetof(bt_sha1_intake_stats, {f}));\n' for f in fields)
                   + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True)
               .stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(bt.IntakeStats)
    for f in fields:
        assert int(got[f]) == getattr(bt.IntakeStats, f).offset, f


def test_python_intake_has_the_receivers_methods_and_the_new_ones():
    bt = load_btsha1()
    for m in ("slot", "advance", "commit", "release", "receive", "poll", "drain", "pending", "stats", "close",
              "kick", "sync", "receive_all"):
        assert callable(getattr(bt.Intake, m)), m


def test_integration_intake_example_compiles(tmp_path):
    """The event-loop snippet of INTEGRATION.md's intake subsection (the ```c
    block that follows its heading, after the receiver's) compiles and links
    against include/ + libbtsha1.so as written, over the reference's Chunk layout."""
    text = open(os.path.join(REPO, "INTEGRATION.md")).read()
    first = text.index("Progressive receive")
    assert "bt_sha1_receiver_advance" in re.search(r"```c\n(.*?)```", text[first:], re.S).group(1)  # still the first
    sec = text[text.index("`bt_sha1_intake`", first):]
    body = re.search(r"```c\n(.*?)```", sec, re.S).group(1)
    assert "bt_sha1_intake_advance" in body and "bt_sha1_intake_commit" in body and "bt_sha1_intake_poll" in body
    assert "receiver" not in body
    body = "\n".join(l for l in body.splitlines() if not l.startswith("#include"))
    src = tmp_path / "intake.c"
    src.write_text(
        "#include <stdint.h>\n#include <stdlib.h>\n#include <string.h>\n#include \"bt_sha1.h\"\n#include \"chunk.h\"\n"
        "enum { NOT_STARTED, RECEIVING, VERIFYING, OWNED };\n"
        "struct Chunk { int id; uint8_t hash[20]; int state; char *data; int received_seq_number;\n"
        "               int received_byte_number; };\n"          # common.h:45-52
        "void intake_example(struct Chunk *chunk, const char *payload, int payload_len, int max_conn) {\n"
        + body + "\n}\nint main(void) { return 0; }\n")
    exe = tmp_path / "intake"
    r = subprocess.run(["gcc", "-Wall", "-Wno-unused-variable", "-Werror", "-I", os.path.join(REPO, "include"),
                        "-o", str(exe), str(src), f"-L{PKG}", "-lbtsha1", f"-Wl,-rpath,{PKG}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
