"""The grouped dW kernel's ring arithmetic (csrc/gemm_dw_ring.h: slots, source rows, token slices,
the DMA image and the fragment addresses) replayed on the host by tools/dw_ring_check.cpp.  The
program is meant for a host sanitizer (its header gives the command); here it is built plainly and
must report every invariant held."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def _host_compiler():
    for c in ("c++", "g++", "clang++"):
        if shutil.which(c):
            return [c]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if Path(hipcc).exists():
        return [hipcc, "-x", "c++"]
    return None


def test_ring_invariants_on_the_host(tmp_path):
    cc = _host_compiler()
    if cc is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "dw_ring_check"
    subprocess.run([*cc, "-std=c++17", "-O1", "-I", str(ROOT / "genomics-lm_amd" / "csrc"),
                    str(ROOT / "tools" / "dw_ring_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "dw_ring_check: ok" in r.stdout, r.stdout[-2000:]
