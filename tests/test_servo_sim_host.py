"""The servo simulator's host side without a device (csrc/servo_sim_host.h): which descriptors lie behind a catppo_servo_sim,
what the entry point refuses, and the call of a launch with the descriptors that are present.  The entry point itself needs
a context and so a device; the header needs neither, and the refusals of tests/test_gpu_servo_*.py are restated against it.
The program is tests/servo_sim_host_main.cpp."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_compiler():
    for name in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(name)
        if path:
            return path
    return None


def test_host_side_walk_check_and_dispatch(tmp_path):
    """every level of ``reserved`` with every allowed set of optional blocks is accepted and walked as it is laid out; every
    buffer on every other buffer, every row field on every other field, and each refusal of the GPU suite is refused; the
    dispatch helper hands on exactly the descriptors that are there"""
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "servo_sim_host"
    csrc = os.path.join(ROOT, "constraints-as-terminations_amd", "csrc")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", f"-I{csrc}", f"-I{os.path.join(ROOT, 'include')}", "-o", str(exe),
                        os.path.join(ROOT, "tests", "servo_sim_host_main.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    last = r.stdout.strip().splitlines()[-1].split() if r.stdout.strip() else []
    assert r.returncode == 0 and len(last) == 4 and int(last[1]) > 2000 and last[2:] == ["bad", "0"], (r.stdout + r.stderr)[-4000:]
