"""CPU: wfa_amd/csrc/wfa_hostpack.hpp (the 2-bit packer of the host entries, their thread-splitting loop and thread-count rule)
as a stand-alone program under the host sanitizers -- tests/hostpack_test.cpp holds the checks."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name,sanitize", [("asan_ubsan", "address,undefined"), ("tsan", "thread")])
def test_hostpack_under_sanitizers(name, sanitize):
    exe = os.path.join(ROOT, "build", "hostpack_test_" + name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=" + sanitize, "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "hostpack_test.cpp"), "-pthread"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
