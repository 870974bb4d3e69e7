"""build.up_to_date(): libkad.so counts as current when its stamp holds the content hash of the sources it was
linked from — not when its modification time happens to be newer (copies and checkouts reset mtimes)."""
import os
import re

from kubeadmiral_amd import build


def test_stamp_decides_over_mtimes(tmp_path, monkeypatch):
    lib = tmp_path / "libkad.so"
    lib.write_bytes(b"\0")
    os.utime(lib, (0, 0))  # older than every source: the mtime rule alone would rebuild
    monkeypatch.setattr(build, "LIB", str(lib))
    monkeypatch.setattr(build, "STAMP", str(lib) + ".sha256")
    assert not build.up_to_date()
    build._write_stamp(build.inputs_hash())
    assert build.up_to_date()
    build._write_stamp("0" * 64)  # a library of other sources, however new its file
    os.utime(lib, None)
    assert not build.up_to_date()


def test_inputs_hash_covers_every_input():
    h = build.inputs_hash()
    assert len(h) == 64 and h == build.inputs_hash()
    names = {os.path.basename(p) for p in build._inputs()}
    assert set(build.SOURCES) <= names and "kad_sched.h" in names


def test_every_header_is_an_input():
    names = {os.path.basename(p) for p in build._inputs()}
    headers = {f for f in os.listdir(build.CSRC) if f.endswith(".h")}
    assert headers and headers <= names, sorted(headers - names)


def test_every_quoted_include_resolves_to_an_input():
    inputs = {os.path.realpath(p) for p in build._inputs()}
    seen = 0
    for f in sorted(os.listdir(build.CSRC)):
        if not f.endswith((".h", ".hip", ".cpp")):
            continue
        with open(os.path.join(build.CSRC, f)) as fh:
            for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', fh.read(), re.M):
                seen += 1
                assert os.path.realpath(os.path.join(build.CSRC, inc)) in inputs, (f, inc)
    assert seen > 20  # (the kernels' file alone includes more than a dozen headers)
