"""CPU: wfa_amd/csrc/wfa_pile.hpp (the pileup's counting rule, one source for the kernels and the host entries) as a stand-alone
program, plain and under the host sanitizers -- tests/pile_host_test.cpp holds the checks."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pile_rule_under_sanitizers():
    src = os.path.join(ROOT, "tests", "pile_host_test.cpp")
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    for name, flags in (("pile_host_test", []), ("pile_host_test_asan_ubsan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = os.path.join(ROOT, "build", name)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", *flags, "-o", exe, src])
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "pile host test ok" in r.stdout
