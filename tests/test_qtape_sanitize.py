"""CPU tier: the host compile of the quantile tape's routines (pyspeedy_amd/csrc/qtape_point.hpp, the body of spd_qtape_host) under
AddressSanitizer + UndefinedBehaviorSanitizer, in a stand-alone program with its own main (tests/sanitize/qtape_sanitize.cpp) that
is run directly, r = 2 and r = 64, with and without ties, as tests/test_verif_sanitize.py runs the verification tape's."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


def run(cmd, cwd):
    p = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=600, env=ENV)
    assert p.returncode == 0, "%s\n%s\n%s" % (" ".join(cmd), p.stdout[-3000:], p.stderr[-6000:])
    return p.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_qtape_host_routines_under_asan_ubsan(tmp_path):
    csrc = os.path.join(ROOT, "pyspeedy_amd", "csrc")
    run(["g++", "-std=c++17", "-ffp-contract=off", *SAN, "-I" + csrc, os.path.join(ROOT, "tests", "sanitize", "qtape_sanitize.cpp"), "-o",
         "qtape_sanitize"], tmp_path)
    assert "qtape sanitize ok" in run([str(tmp_path / "qtape_sanitize")], tmp_path)
