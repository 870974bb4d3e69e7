"""The staging arena's layout and the shared CSR validation, on the host alone.

tests/arena_main.cpp includes the layout half of csrc/kad_arena.h and first_bad / off_bad / csr_bad of
csrc/kad_ctx.h (KAD_HOST_ONLY: no HIP header, no device). It is compiled here with the host compiler under
AddressSanitizer and UndefinedBehaviorSanitizer and run as its own process; nothing is loaded into Python.
It checks that parts are 256-B aligned and disjoint, that empty parts keep a slot and absent ones give a null
pointer, that every bound pointer lands at its part's offset, that a field of 1, 4 or 8 bytes reserves its
count times its width, that only outputs bound to a host destination are fetched, total() of the consumer
layouts at n = 0, 1 and 65 537 (past first_bad's parallel threshold), and that csr_bad agrees with one serial pass on a non-zero start, a decrease at the first, a middle, the last
and the 65 536th offset, and an entry equal to lo - 1 and to hi."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_arena_layout_and_csr_checks_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "arena_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-pthread", os.path.join(HERE, "arena_main.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=120)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out
    assert out.startswith("ok: "), out
