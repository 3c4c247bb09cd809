"""csrc/device_own.h - DevBuf, PinnedBuf, Event: who owns what on the device - as tools/own_check.cpp, a stand-alone
program on the CPU under AddressSanitizer + UBSan with the runtime's functions defined on malloc / free: alloc, move,
grow (also the failing allocation), aliases by copy, adopt, the live counters; the sanitizer's leak check at exit is
part of it.  Run a second time with RTLFM_POISON=1 for the poison path."""
import os
import shutil
import subprocess

import pytest

from rtlsdr_amd import build as hipbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rocm_include():
    hipcc = hipbuild._hipcc()
    for c in (hipcc, os.path.realpath(hipcc)):
        inc = os.path.join(os.path.dirname(os.path.dirname(c)), "include")
        if os.path.exists(os.path.join(inc, "hip", "hip_runtime_api.h")):
            return inc
    return "/opt/rocm/include"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("own") / "own_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I" + rocm_include(), "-o", out,
                           os.path.join(ROOT, "tools", "own_check.cpp")])
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not on PATH")
@pytest.mark.parametrize("poison", ["", "1"])
def test_own_check_under_the_sanitizers(exe, poison):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, RTLFM_POISON=poison))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.startswith("own_check: ok"), r.stdout
    assert ("poisoned" in r.stdout) == bool(poison), r.stdout
