"""CPU: wfa_amd/csrc/wfa_kinds.hpp (the kernel numbering and the traits table of the sub-wave forward kinds) and the table read
behind bound_row_pitch() as a stand-alone program under the host sanitizers -- tests/kinds_host_test.cpp holds the checks."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kinds_table_under_sanitizers():
    exe = os.path.join(ROOT, "build", "kinds_host_test_asan_ubsan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "kinds_host_test.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "kinds host test ok" in r.stdout
