"""CPU-only: what shstep_set_rolling_con and shstep_set_twisting_con (docs/SPEC.md §2.24) accept, from
check_conic_resistance of csrc/cone_check.hpp, the words of the null-twist refusal, and the switches a record with the
four coefficients gives in either order of the two setters, in a stand-alone host program
(tests/host/test_conic_roll_check.cpp).  Built plainly, and once more under AddressSanitizer + UBSan; run as a program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lammps-spherharm_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "test_conic_roll_check.cpp")

OK = ("accepted", "eight", "none")
WANT = {"count": "cone twisting resistance: 3 coefficients for 2 cones (call it after shstep_set_cones)",
        "before the cones": "cone rolling resistance: 1 coefficients for 0 cones (call it after shstep_set_cones)",
        "null table": "cone rolling resistance: null array pointer",
        "negative": "cone 1: rolling coefficient mu_r -0.5 must be finite and >= 0",
        "nan": "cone 0: twisting coefficient gamma_tw nan must be finite",
        "inf": "cone 1: rolling coefficient gamma_r inf must be finite",
        "null twist": "cone rolling or twisting resistance: null twist pointer",
        "split rolling": "damp 0 fric 0 hist 0 roll 0 any 0", "rolling alone": "damp 0 fric 0 hist 0 roll 1 any 1",
        "twisting alone": "damp 0 fric 0 hist 0 roll 1 any 1", "rolling then twisting": "damp 0 fric 0 hist 0 roll 1 any 1",
        "twisting then rolling": "damp 0 fric 0 hist 0 roll 1 any 1", "rolling to 0": "damp 0 fric 0 hist 0 roll 1 any 1",
        "both to 0": "damp 0 fric 0 hist 0 roll 0 any 0", "rotation alone": "damp 0 fric 0 hist 0 roll 0 any 0",
        "spring and rolling": "damp 0 fric 0 hist 1 roll 1 any 1", "reset": "damp 0 fric 0 hist 0 roll 0 any 0"}


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_the_cone_rolling_coefficients_are_checked(tmp_path, flags):
    out = tmp_path / "test_conic_roll_check"
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
