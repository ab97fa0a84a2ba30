"""CPU: the random access of the chain-form gather kernels (gather_seek,
gather_block_at, gather_tail_at in csrc/sha1_gather_walk.h), the text the
device compiles, run on the host under AddressSanitizer and UBSan.

tests/native/gather_seek_check.cpp is a stand-alone program: every segment is
a heap allocation of exactly its own size and the descriptor / pos tables end
at the listed prefix, so a read outside a listed segment or of a table entry
at or past nseg is reported.  For every list of gather_cases.WALK_CASES, every
listed prefix, every whole block inside it and every hint from 0 to the true
segment, the block must equal the concatenation's bytes; the finish tails of
0, 1, 55, 56 and 63 bytes too.  Built here with the host compiler and run as a
child process; it needs nothing preloaded."""
import os
import subprocess

import gather_cases
from conftest import PKG, REPO


def _check(exe, args, min_cases):
    r = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    cases, failed = int(lines[-1].split()[0]), int(lines[-1].split()[2])
    blocks, tails = int(lines[-2].split()[0]), int(lines[-2].split()[2])
    assert failed == 0 and cases >= min_cases and blocks > 1000 and tails > 1000, lines[-2:]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]


def test_gather_seek_reads_only_what_is_listed(tmp_path):
    exe = tmp_path / "gather_seek_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", os.path.join(PKG, "csrc"),
                    "-o", str(exe), os.path.join(REPO, "tests", "native", "gather_seek_check.cpp")], check=True)
    cases = tmp_path / "walk_cases.txt"
    cases.write_text("".join(" ".join(map(str, lens)) + "\n" for lens in gather_cases.WALK_CASES))
    _check(exe, [str(cases)], len(gather_cases.WALK_CASES) + 3)


def test_make_target_builds_and_the_program_passes(tmp_path):
    """`make gather_seek_check` with its object directory redirected: the recipe itself is run."""
    out = tmp_path / "seek"
    subprocess.run(["make", "-C", REPO, "gather_seek_check", f"SEEKDIR={out}"], check=True, capture_output=True)
    _check(out / "gather_seek_check", [], 70)
