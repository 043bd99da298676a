"""The map section of the CPU oracle (oracle/arroyo_oracle.c) under
AddressSanitizer and UBSan: tests/map_oracle_main.c is compiled together
with the oracle as a stand-alone program and run as a child process --
nothing is loaded into this interpreter.  It covers what used to be
undefined behaviour there (signed wrap, INT64_MIN / -1, F2I out of range,
an unvalidated out_reg) and the error return's output batch, which
LeakSanitizer watches."""
import os
import shutil
import subprocess

import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_ORACLE = os.path.join(os.path.dirname(_HERE), "oracle", "arroyo_oracle.c")


def test_map_oracle_under_sanitizers(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.fail("gcc not found: the oracle cannot be checked")
    exe = str(tmp_path / "map_oracle_main")
    build = subprocess.run(
        [gcc, "-g", "-O1", "-fno-omit-frame-pointer",
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         os.path.join(_HERE, "map_oracle_main.c"), _ORACLE, "-o", exe, "-lm"],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "map_oracle: ok" in run.stdout
