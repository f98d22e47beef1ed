"""CPU-only: what shstep_set_conic_tangential_spring (docs/SPEC.md §2.23) accepts, from check_conic_spring of
csrc/cone_check.hpp, and the switches a record with a k_t gives in either order of the two setters, in a stand-alone host
program (tests/host/test_conic_spring_check.cpp).  Built plainly, and once more under AddressSanitizer + UBSan; run as a
program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lammps-spherharm_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "test_conic_spring_check.cpp")

OK = ("accepted", "eight", "none")
WANT = {"count": "cone tangential spring: 3 coefficients for 2 cones (call it after shstep_set_cones)",
        "before the cones": "cone tangential spring: 2 coefficients for 0 cones (call it after shstep_set_cones)",
        "null table": "cone tangential spring: null array pointer",
        "negative": "cone 1: tangential spring k_t -2 must be finite and >= 0",
        "nan": "cone 0: tangential spring k_t nan must be finite", "inf": "cone 1: tangential spring k_t inf must be finite",
        "spring alone": "damp 0 fric 0 hist 0 roll 0 any 0", "friction alone": "damp 0 fric 0 hist 0 roll 0 any 0",
        "spring then mu": "damp 0 fric 0 hist 1 roll 0 any 1", "mu then spring": "damp 0 fric 0 hist 1 roll 0 any 1",
        "last mu to 0": "hist 0 roll 0 any 0", "every k_t to 0": "hist 0 roll 0 any 0", "reset": "hist 0 roll 0 any 0"}


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_the_cone_spring_coefficient_is_checked(tmp_path, flags):
    out = tmp_path / "test_conic_spring_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{CSRC}", SRC, "-o", str(out)])
    res = subprocess.run([str(out)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stderr == ""
    lines = dict(ln.split(": ", 1) for ln in res.stdout.strip().split("\n"))
    assert set(lines) == set(OK) | set(WANT)
    for label in OK:
        assert lines[label] == "ok", (label, lines[label])
    for label, part in WANT.items():
        assert part in lines[label], (label, lines[label])
