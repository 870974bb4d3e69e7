"""The host's choice of prep_kernel's row access width (csrc/kad_route.h), without a GPU.

prep_kernel<true> (route PREP_VEC) moves a lane's four row words as two 16-byte accesses. That is only valid
where every lane owns four whole chunks (ceil(C / 64) % 4 == 0) and every table it reads or writes starts on a
16-byte boundary; the decision is made once per launch on the host from the device pointers
(rows_aligned16 -> RouteIn::rows16 -> route_schedule).

tests/prep_vec_main.cpp includes kad_route.h as host-only C++ and is compiled here with the host compiler under
AddressSanitizer and UndefinedBehaviorSanitizer and run as its own process (nothing is loaded into Python): the
alignment predicate on aligned, null and deliberately 8-byte aligned addresses (one bad base in each of the seven
positions), prep_vec_ok over every chunk count, and route_schedule's prep id for every C of the ABI with and
without aligned bases. The second test asks the built library the same through kad_route_eval.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_prep_route_decision_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "prep_vec_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-pthread",
                    os.path.join(HERE, "prep_vec_main.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=120)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out
    assert out.startswith("ok: "), out


# C -> chunks; the vector route needs a multiple of four
VEC_CS = {256: 4, 450: 8, 512: 8, 705: 12, 1000: 16, 1024: 16, 4096: 64, 32768: 512}
SCALAR_CS = {1: 1, 64: 1, 65: 2, 192: 3, 300: 5, 513: 9, 960: 15, 1025: 17, 32769: 513}


def test_library_route_follows_chunks_and_alignment():
    from kubeadmiral_amd import build, runtime
    build.build()
    base = dict(clean=1, fold=1, fitfold=1, W=1000, n_cu=256)
    for C, nch in VEC_CS.items():
        assert (C + 63) // 64 == nch and nch % 4 == 0
        assert runtime.route_eval(C=C, rows16=1, **base)["prep"] == "PREP_VEC", C
        assert runtime.route_eval(C=C, rows16=0, **base)["prep"] == "PREP", C  # an 8-byte aligned base somewhere
        assert runtime.route_eval(C=C, **base)["prep"] == "PREP", C  # the record's default: not known to be aligned
    for C, nch in SCALAR_CS.items():
        assert (C + 63) // 64 == nch and nch % 4 != 0
        assert runtime.route_eval(C=C, rows16=1, **base)["prep"] == "PREP", C
    # prep_wave_kernel's range is not touched
    assert runtime.route_eval(C=10000, rows16=1, **base)["prep"] == "PREP_WAVE3"
    assert runtime.route_eval(C=8192, rows16=1, prep_wave=0, **base)["prep"] == "PREP_VEC"
    # nothing else of the route depends on it
    a, b = runtime.route_eval(C=1000, rows16=0, **base), runtime.route_eval(C=1000, rows16=1, **base)
    assert {k: v for k, v in a.items() if k != "prep"} == {k: v for k, v in b.items() if k != "prep"}
