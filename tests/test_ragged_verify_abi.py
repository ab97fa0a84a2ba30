"""CPU: the verify forms for chunks of any length -- bt_sha1_ragged_verify_dev,
bt_sha1_verifier_create_ragged, bt_sha1_verifier_get_stats -- are exported by
every build of the library, declared in include/bt_sha1.h, and refuse bad
arguments with a message before any device call, so all of this holds without
a GPU."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import PKG, REPO, load_btsha1

LIBS = {"product": os.path.join(PKG, "libbtsha1.so"),
        "dbgbar": os.path.join(REPO, "build_variants", "dbgbar", "libbtsha1.so"),
        "experiments": os.path.join(REPO, "build_variants", "experiments", "libbtsha1.so")}
NEW = ["bt_sha1_ragged_verify_dev", "bt_sha1_verifier_create_ragged", "bt_sha1_verifier_get_stats"]


@pytest.mark.parametrize("name", LIBS)
def test_every_build_exports_the_ragged_verify_surface(name):
    assert os.path.exists(LIBS[name]), f"run make {name} first"
    out = subprocess.run(["nm", "-D", "--defined-only", LIBS[name]], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert not set(NEW) - exported, set(NEW) - exported
    # the new launcher is hidden; besides the C functions only the kernels' handles carry the name
    other = [l.split()[-1] for l in out.splitlines() if re.search(r"ragged_verify", l)]
    assert all(s in NEW or re.fullmatch(r"_ZN6btsha1\d+(__device_stub__)?k_sha1_\w+", s) for s in other), other
    header = open(os.path.join(REPO, "include", "bt_sha1.h")).read()
    assert all(re.search(r"\b%s\s*\(" % f, header) for f in NEW)
    assert header.index("bt_sha1_ragged_verify_dev") > header.index("bt_sha1_ragged_dev")


def test_ragged_verify_dev_refuses_before_any_device_call():
    """n == 0 is no work; a null d_base / d_offsets / d_lens / d_expected / d_ok
    and an n past the grid are -1 with a message; d_digests may be NULL."""
    bt = load_btsha1()
    lib = bt.lib
    assert lib.bt_sha1_ragged_verify_dev(None, None, None, 0, None, None, None, None) == 0
    p = 4096  # never dereferenced: every call below is refused first
    names = ("d_base", "d_offsets", "d_lens", "d_expected", "d_ok")
    for k, name in enumerate(names):
        args = [p] * 5
        args[k] = None
        lib.bt_sha1_verifier_create_ragged(0, 0, 1, 2)  # leaves another message behind
        assert "max_chunk_len" in bt.last_error()
        assert lib.bt_sha1_ragged_verify_dev(args[0], args[1], args[2], 1, args[3], args[4], None, None) == -1, name
        assert "null pointer" in bt.last_error(), (name, bt.last_error())
        with pytest.raises(bt.BtSha1Error, match="null pointer"):
            bt.ragged_verify_dev(args[0], args[1], args[2], 1, args[3], args[4])
    for n in (1 << 31, (1 << 64) - 1):
        assert lib.bt_sha1_ragged_verify_dev(p, p, p, n, p, p, None, None) == -1
        assert "grid limit" in bt.last_error() and str(n) in bt.last_error(), bt.last_error()


@pytest.mark.parametrize("max_chunk_len,batch", [(0, 8), ((32 << 20) + 1, 8), (4096, 0)])
def test_ragged_verifier_create_refuses_before_any_device_call(max_chunk_len, batch):
    bt = load_btsha1()
    msg = "max_chunk_len must be in [1, 32 MiB] and batch > 0"
    assert bt.lib.bt_sha1_verifier_create_ragged(0, max_chunk_len, batch, 2) is None
    assert msg in bt.last_error()
    with pytest.raises(bt.BtSha1Error, match=re.escape(msg)):
        bt.Verifier(chunk_len=max_chunk_len, batch=batch, ragged=True)


def test_classic_verifier_create_keeps_its_refusal():
    """bt_sha1_verifier_create still wants a 16-byte multiple: the ragged constructor is the only new way in."""
    bt = load_btsha1()
    assert bt.lib.bt_sha1_verifier_create(0, 65536 + 8, 8, 2) is None
    assert "chunk_len must be a 16-byte multiple <= 32 MiB and batch > 0" in bt.last_error()


def test_verifier_get_stats_refuses_null_pointers():
    bt = load_btsha1()
    s = bt.VerifierStats()
    bt.lib.bt_sha1_verifier_create_ragged(0, 0, 1, 2)
    assert bt.lib.bt_sha1_verifier_get_stats(None, ctypes.byref(s)) == -1
    assert "null pointer" in bt.last_error()


def test_verifier_stats_layout(tmp_path):
    """The ctypes mirror btsha1.VerifierStats has the C struct's size and offsets."""
    bt = load_btsha1()
    fields = [f for f, _ in bt.VerifierStats._fields_]
    assert fields == ["batches", "ragged_batches", "chunks", "short_chunks", "released"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "bt_sha1.h"\nint main(void) {\n'
                   '  printf("size %zu\\n", sizeof(bt_sha1_verifier_stats));\n'
                   + "".join(f'  printf("{f} %zu\\n", offsetof(bt_sha1_verifier_stats, {f}));\n' for f in fields)
                   + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(REPO, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True)
               .stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(bt.VerifierStats)
    for f in fields:
        assert int(got[f]) == getattr(bt.VerifierStats, f).offset, f


def test_python_surface():
    bt = load_btsha1()
    assert callable(bt.ragged_verify_dev) and callable(bt.Verifier.stats)
    import inspect
    assert inspect.signature(bt.Verifier.__init__).parameters["ragged"].default is False
