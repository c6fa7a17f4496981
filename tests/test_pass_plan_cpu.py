"""The driver's host arithmetic without a GPU: how a slice is cut into passes, a resident range into the lanes' chunks, and
what a lane of a host run takes next (csrc/pass_plan.hpp).  Expected values are those the loops gave inside the driver before
they were moved out, pasted into tools/pass_plan_check.cpp as numbers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pass_plan_under_the_sanitizers(tmp_path):
    """properties on every case and the literal values of a fixed list, as a stand-alone program built with the address and
    undefined-behaviour sanitizers and run on the CPU"""
    exe = tmp_path / "pass_plan_check"
    cc = subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         os.path.join(ROOT, "tools", "pass_plan_check.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "pass_plan_check ok" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr
