"""CPU-only: what shstep_set_cones and the cone coefficient setters (docs/SPEC.md §2.22) accept, from csrc/cone_check.hpp
and csrc/surface_coefficients.hpp in a stand-alone host program (tests/host/test_cone_check.cpp): unit axis, the range of
the half-angle through its cosine and sine, the unit circle within 4 ulp, finite non-negative coefficients, the count.
Built plainly, and once more under AddressSanitizer + UBSan; run as a program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lammps-spherharm_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "test_cone_check.cpp")

OK = ("accepted", "none", "eight", "one ulp off", "near pi/2", "coefficients accepted", "negative rotation")
WANT = {"nine": "cones: 9 cones, 0..8 are accepted", "negative count": "0..8 are accepted", "null": "cones: null array pointer",
        "axis length": "cone 0: the axis has length", "cos < 0": "must both be > 0 (0 < theta < pi/2)",
        "cos 0": "must both be > 0", "sin 0": "must both be > 0", "off the circle": "not 1 within 4 ulp",
        "cos nan": "not finite", "apex inf": "not finite", "kn < 0": "cone 0: kn -1 < 0", "exponent < 1": "exponent 0.5 < 1",
        "kn nan": "not finite", "count": "cone damping: 3 coefficients for 2 cones (call it after shstep_set_cones)",
        "null table": "cone damping: null array pointer", "negative": "cone 1: damping coefficient -2 must be finite and >= 0",
        "nan": "cone 0: damping coefficient nan must be finite", "inf rotation": "cone 0: angular velocity inf must be finite"}


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_the_cone_record_and_its_coefficients_are_checked(tmp_path, flags):
    out = tmp_path / "test_cone_check"
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
