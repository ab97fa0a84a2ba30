"""CPU: the resumable entry points (bt_sha1_resume_dev,
bt_sha1_states_init_dev) and the progressive receiver (bt_sha1_receiver_*)
are exported by every build of the library, and refuse bad arguments with a
message before any device call -- so all of this holds without a GPU."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import PKG, REPO, load_btsha1

LIBS = {"product": os.path.join(PKG, "libbtsha1.so"),
        "dbgbar": os.path.join(REPO, "build_variants", "dbgbar", "libbtsha1.so"),
        "experiments": os.path.join(REPO, "build_variants", "experiments", "libbtsha1.so")}
NEW = ["bt_sha1_resume_dev", "bt_sha1_states_init_dev"] + ["bt_sha1_receiver_" + f for f in (
    "create", "destroy", "slot", "advance", "commit", "release", "poll", "drain", "pending", "get_stats")]


@pytest.mark.parametrize("name", LIBS)
def test_every_build_exports_the_new_entry_points(name):
    assert os.path.exists(LIBS[name]), f"run make {name} first"
    out = subprocess.run(["nm", "-D", "--defined-only", LIBS[name]], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert not set(NEW) - exported, set(NEW) - exported
    # the launchers and the receiver's internals are hidden; the kernels' handles carry their btsha1::k_ names
    other = [l.split()[-1] for l in out.splitlines() if re.search(r"resume|receiver|states_init|Receiver|RSlot", l)]
    assert all(s in NEW or re.fullmatch(r"_ZN6btsha1\d+(__device_stub__)?k_\w+", s) for s in other), other
    header = open(os.path.join(REPO, "include", "bt_sha1.h")).read()
    assert all(re.search(r"\b%s\s*\(" % f, header) for f in NEW)


def test_resume_dev_argument_checks_need_no_device():
    bt = load_btsha1()
    f = bt.lib.bt_sha1_resume_dev
    assert f(None, None, None, None, 0, None, None, None, None, None) == 0
    good = [4096, 4096, 4096, 4096, 1, 4096, 4096, None, None, None]
    for k in (0, 1, 2, 3, 5):
        a = list(good)
        a[k] = None
        assert f(*a) == -1, k
        assert "null pointer" in bt.last_error(), (k, bt.last_error())
    a = list(good)
    a[8] = 4096  # d_ok without d_expected
    assert f(*a) == -1 and "null pointer" in bt.last_error() and "d_expected" in bt.last_error()
    a = list(good)
    a[4] = 1 << 31  # one workgroup per message: the grid limit
    assert f(*a) == -1 and "grid limit" in bt.last_error()
    assert bt.lib.bt_sha1_states_init_dev(None, 0, None) == 0
    assert bt.lib.bt_sha1_states_init_dev(None, 3, None) == -1 and "null pointer" in bt.last_error()


@pytest.mark.parametrize("chunk_len,nslots,msg", [
    (0, 4, "chunk_len must be in [1, 32 MiB]"),
    ((32 << 20) + 1, 4, "chunk_len must be in [1, 32 MiB]"),
    (4096, 0, "nslots must be in [1, 64]"),
    (4096, 65, "nslots must be in [1, 64]"),
])
def test_receiver_create_refuses_before_any_device_call(chunk_len, nslots, msg):
    bt = load_btsha1()
    assert bt.lib.bt_sha1_receiver_create(0, chunk_len, nslots, 0) is None
    assert msg in bt.last_error()
    with pytest.raises(bt.BtSha1Error, match=re.escape(msg)):
        bt.Receiver(chunk_len=chunk_len, nslots=nslots)


def test_receiver_calls_refuse_null_handles():
    bt = load_btsha1()
    lib = bt.lib
    out = (bt.Verdict * 1)()
    e = (ctypes.c_uint8 * 20)()
    for rc in (lib.bt_sha1_receiver_advance(None, 4096, 64), lib.bt_sha1_receiver_commit(None, 4096, 64, e, 0),
               lib.bt_sha1_receiver_release(None, 4096), lib.bt_sha1_receiver_poll(None, out, 1),
               lib.bt_sha1_receiver_drain(None, out, 1), lib.bt_sha1_receiver_get_stats(None, None)):
        assert rc == -1 and "null pointer" in bt.last_error()
    assert lib.bt_sha1_receiver_slot(None) is None and "null pointer" in bt.last_error()
    assert lib.bt_sha1_receiver_pending(None) == -1
    lib.bt_sha1_receiver_destroy(None)  # like free(NULL)


def test_receiver_stats_layout(tmp_path):
    """The ctypes mirror btsha1.ReceiverStats has the C struct's size and offsets."""
    bt = load_btsha1()
    fields = [f for f, _ in bt.ReceiverStats._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bt_sha1.h"\nint main(void) {\n'
                   '  printf("size %zu\\n", sizeof(bt_sha1_receiver_stats));\n'
                   + "".join(f'  printf("{f} %zu\\n", offsetof(bt_sha1_receiver_stats, {f}));\n' for f in fields)
                   + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True)
               .stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(bt.ReceiverStats)
    for f in fields:
        assert int(got[f]) == getattr(bt.ReceiverStats, f).offset, f


def test_integration_progressive_example_compiles(tmp_path):
    """The progressive-receive snippet of INTEGRATION.md (the ```c block that
    follows "Progressive receive") compiles and links against include/ +
    libbtsha1.so as written, over the reference's Chunk layout."""
    text = open(os.path.join(REPO, "INTEGRATION.md")).read()
    sec = text[text.index("Progressive receive"):]
    body = re.search(r"```c\n(.*?)```", sec, re.S).group(1)
    assert "bt_sha1_receiver_advance" in body and "bt_sha1_receiver_commit" in body
    body = "\n".join(l for l in body.splitlines() if not l.startswith("#include"))
    src = tmp_path / "progressive.c"
    src.write_text(
        "#include <stdint.h>\n#include <stdlib.h>\n#include <string.h>\n#include \"bt_sha1.h\"\n#include \"chunk.h\"\n"
        "enum { NOT_STARTED, RECEIVING, VERIFYING, OWNED };\n"
        "struct Chunk { int id; uint8_t hash[20]; int state; char *data; int received_seq_number;\n"
        "               int received_byte_number; };\n"          # common.h:45-52
        "void progressive_example(struct Chunk *chunk, const char *payload, int payload_len, int max_conn) {\n"
        + body + "\n}\nint main(void) { return 0; }\n")
    exe = tmp_path / "progressive"
    r = subprocess.run(["gcc", "-Wall", "-Wno-unused-variable", "-Werror", "-I", os.path.join(REPO, "include"),
                        "-o", str(exe), str(src), f"-L{PKG}", "-lbtsha1", f"-Wl,-rpath,{PKG}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
