"""The feeder's arithmetic of a host run without a GPU: the parts as one batch, the cut into copy chunks and input segments,
the narrowed offsets and the size of their table, what a lane may take (csrc/host_feed.hpp).  Expected values are those the
loop gave inside Batch::run_host_parts before it was moved out, pasted into tools/host_feed_check.cpp as numbers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_feed_under_the_sanitizers(tmp_path):
    """properties on every case and the literal values of a fixed list, as a stand-alone program built with the address and
    undefined-behaviour sanitizers and run on the CPU"""
    exe = tmp_path / "host_feed_check"
    cc = subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         os.path.join(ROOT, "tools", "host_feed_check.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "host_feed_check ok" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr
