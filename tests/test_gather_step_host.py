"""CPU: the stepper of k_sha1_gather_lat's loader wave (gather_step,
csrc/sha1_gather_walk.h), the text the device compiles, run on the host under
AddressSanitizer and UBSan.

tests/native/gather_step_check.cpp is a stand-alone program: every segment, the
descriptor table and the idle block are heap allocations of exactly their own
size; the stepper's blocks must equal gather_walk's, its padding blocks the
oracle's layout, and the calls past a message's end are made after the message
was freed.  Built here with the host compiler and run as a child process; it
needs nothing preloaded."""
import os
import subprocess

from conftest import PKG, REPO


def test_gather_step_yields_the_padded_message_and_reads_only_the_listed_segments(tmp_path):
    exe = tmp_path / "gather_step_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", os.path.join(PKG, "csrc"),
                    "-o", str(exe), os.path.join(REPO, "tests", "native", "gather_step_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    last = r.stdout.strip().splitlines()[-1]
    cases, failed = int(last.split()[0]), int(last.split()[2])
    assert failed == 0 and cases >= 450, last
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]


def test_make_target_builds_and_the_program_passes(tmp_path):
    """`make gather_step_check` with its object directory redirected: the recipe itself is run."""
    out = tmp_path / "step"
    subprocess.run(["make", "-C", REPO, "gather_step_check", f"STEPDIR={out}"], check=True, capture_output=True)
    r = subprocess.run([str(out / "gather_step_check")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith(" 0 failed"), r.stdout[-2000:] + r.stderr[-2000:]
