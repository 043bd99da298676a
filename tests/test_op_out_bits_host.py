"""The bit-offset bitmap append of the host output batch
(out_validity_append_bits, arroyo_amd/csrc/op_out.h) under AddressSanitizer
and UBSan: tests/op_out_bits_main.cpp is compiled as a stand-alone program
and run as a child process -- nothing is loaded into this interpreter.  It
appends at every destination bit offset 0..15 the lengths 0, 1, 7, 8, 9, 63,
64 and 65 from sources with dirty tail bits, against a bit-by-bit loop, in
buffers of exactly the contract's size."""
import os
import shutil
import subprocess

import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))


def test_validity_append_bits_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.fail("g++ not found: the host helper cannot be checked")
    exe = str(tmp_path / "op_out_bits_main")
    build = subprocess.run(
        [gxx, "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         "-Wall", "-Wextra", "-Werror",
         os.path.join(_HERE, "op_out_bits_main.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "op_out_bits: ok" in run.stdout
