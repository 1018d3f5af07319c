"""The arithmetic of one (segment, feature) pair of k_metagene (gat_amd/csrc/gat_metagene_bins.h: the clip to the three regions
by strand, the flank pieces, the stepping of the body's edges, the bin of a midpoint, the reach helpers, the LDS sizing)
against the definition in 128-bit integers: tests/host/metagene_bins_check.cpp, a stand-alone program compiled for the host
alone with the address and undefined-behaviour sanitizers.  No GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_metagene_bins_check(tmp_path):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    if not hipcc:
        pytest.skip("no hipcc")
    exe = str(tmp_path / "metagene_bins_check")
    cmd = [hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "gat_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "metagene_bins_check.cpp"), "-o", exe]
    c = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert c.returncode == 0, "the check program does not compile:\n" + c.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "metagene_bins_check failed (exit status %d):\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
