"""CPU: wfa_amd/csrc/wfa_ladder.hpp (the plan of one job of the long-pair ladder: kernel, arena slots or paged pool, team geometry,
LDS) as a stand-alone program under the host sanitizers -- tests/ladder_host_test.cpp holds the literal plans, the slot sizes the
comments quote and the invariants over the grid (650 million jobs, each planned twice, on up to eight threads: hence -O2; twelve
minutes of one core under the sanitizers)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ladder_plan_under_sanitizers():
    exe = os.path.join(ROOT, "build", "ladder_host_test_asan_ubsan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "ladder_host_test.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ladder host test ok" in r.stdout
