"""The extended event block in the servo simulator's host side without a device (csrc/servo_sim_host.h; DESIGN section 9,
"Disturbances"): 64 words are accepted with and without ``off_ev_state``; 48 words (and every other count), a non-zero
``reserved`` under 32 words, a misaligned ``ev_state``, ``ev_state`` on each other row field and each base field, and the block on
each buffer in turn are refused.  The program is tests/servo_disturb_host_main.cpp, a stand-alone one with its own main: it is
built once plainly and once with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

from test_servo_plant_host import SANITIZE
from test_servo_sim_host import ROOT, _host_compiler


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
    exe = tmp_path / "servo_disturb_host"
    csrc = os.path.join(ROOT, "constraints-as-terminations_amd", "csrc")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", *flags, f"-I{csrc}", f"-I{os.path.join(ROOT, 'include')}", "-o", str(exe),
                        os.path.join(ROOT, "tests", "servo_disturb_host_main.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    last = r.stdout.strip().splitlines()[-1].split() if r.stdout.strip() else []
    assert r.returncode == 0 and len(last) == 4 and int(last[1]) > 150 and last[2:] == ["bad", "0"], (r.stdout + r.stderr)[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def test_extended_event_block_check(tmp_path):
    _build_and_run(tmp_path, [])


def test_extended_event_block_check_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    _build_and_run(tmp_path, SANITIZE)
