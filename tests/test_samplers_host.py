"""The table of samplers of the library's host code (gat_amd/csrc/gat_samplers.h) and the three predicates that read it:
tests/host/samplers_check.cpp, a stand-alone program compiled for the host alone with the address and undefined-behaviour
sanitizers.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_samplers_check(tmp_path):
    """ids 0..7 known; -1, 8, INT32_MAX unknown (nullptr, nothing read beyond the table); the predicates' values per id"""
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("no hipcc")
    exe = str(tmp_path / "samplers_check")
    cmd = [hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "gat_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "samplers_check.cpp"), "-o", exe]
    c = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert c.returncode == 0, "the check program does not compile:\n" + c.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "samplers_check failed (exit status %d):\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
