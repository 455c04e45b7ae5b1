"""Build-container test (NOT under tests/, like tools/host_asan/: no run on the GPU pool may reach a sanitizer build): the 20-bit
unit-block entries' pack / unpack arithmetic (include/mgx/pack20.hpp) under AddressSanitizer + UndefinedBehaviorSanitizer on the
host.  usage: python -m pytest tools/host_pack20/test_host_pack20.py"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_pack20_round_trips_under_asan_and_ubsan():
    """every slot position x {0, 1, 0x7FFFF, 0x80000, 0xFFFFE, all ones -> -1}, random chunks in the kernels' arrangement, the
    slack behind the array -- equal to a bit-by-bit reference, no sanitizer report"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    r = subprocess.run(["bash", os.path.join(HERE, "run.sh")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "host_pack20: 0 failures" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
