"""CPU: the block walk of k_sha1_pkts (csrc/sha1_pkt_walk.h), the text the
device compiles, run on the host under AddressSanitizer and UBSan.

tests/native/pkt_walk_check.cpp is a stand-alone program: each slot is a heap
allocation of exactly slot_pkts * stride bytes and each order table one of
exactly ceil(len / payload) entries, so an over-read of either is reported;
every address the walk fetches is recorded and must lie in a packet buffer's
payload area, and the blocks must equal the assembled message's, padding
included.  Built here with the host compiler and run as a child process; it
needs nothing preloaded."""
import os
import subprocess

from conftest import PKG, REPO


def check(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    last = r.stdout.strip().splitlines()[-1].split()
    assert last[0] == "pkt_walk_check:" and last[-1] == "ok" and int(last[1]) >= 400, last
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr and "FAIL" not in r.stderr, r.stderr[-3000:]


def test_pkt_walk_keeps_its_read_contract(tmp_path):
    exe = tmp_path / "pkt_walk_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", os.path.join(PKG, "csrc"),
                    "-o", str(exe), os.path.join(REPO, "tests", "native", "pkt_walk_check.cpp")], check=True)
    check(exe)


def test_make_target_builds_and_the_program_passes(tmp_path):
    """`make pkt_walk_check` with its object directory redirected: the recipe itself is run."""
    out = tmp_path / "walk"
    subprocess.run(["make", "-C", REPO, "pkt_walk_check", f"PKTDIR={out}"], check=True, capture_output=True)
    check(out / "pkt_walk_check")
