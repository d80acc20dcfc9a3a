"""The plant level of the servo simulator's host side without a device (csrc/servo_sim_host.h; DESIGN section 9, "Robustness"):
the new level is accepted with every allowed set of optional blocks, with and without a history; refused for a NULL or
misaligned table, a non-zero reserved word, no evaluation pointer, a history without observations and the table on each other
range in turn; and the older levels run on the same bytes as before.  The program is tests/servo_plant_host_main.cpp, a
stand-alone one with its own main: it is built once plainly and once with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

from test_servo_sim_host import ROOT, _host_compiler

SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g"]


def _build_and_run(tmp_path, flags):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    if flags:                                                                 # a toolchain without the sanitizers' runtimes
        probe = tmp_path / "probe.cpp"
        probe.write_text("int main() { return 0; }\n")
        r = subprocess.run([cxx, *flags, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            pytest.skip("the host compiler cannot link the sanitizers' runtimes")
    exe = tmp_path / "servo_plant_host"
    csrc = os.path.join(ROOT, "constraints-as-terminations_amd", "csrc")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", *flags, f"-I{csrc}", f"-I{os.path.join(ROOT, 'include')}", "-o", str(exe),
                        os.path.join(ROOT, "tests", "servo_plant_host_main.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    last = r.stdout.strip().splitlines()[-1].split() if r.stdout.strip() else []
    assert r.returncode == 0 and len(last) == 4 and int(last[1]) > 1200 and last[2:] == ["bad", "0"], (r.stdout + r.stderr)[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def test_plant_level_walk_check_and_dispatch(tmp_path):
    _build_and_run(tmp_path, [])


def test_plant_level_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    _build_and_run(tmp_path, SANITIZE)
