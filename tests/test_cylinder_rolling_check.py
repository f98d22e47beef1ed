"""CPU-only: what the cylinders' rolling and twisting setters (docs/SPEC.md §2.21) take from
csrc/surface_coefficients.hpp, in a stand-alone host program (tests/host/test_cylinder_rolling_check.cpp): the messages of
the two argument checks, the `roll` switch over a cylinder record and the [4][n] image of the device table.  Built plainly,
and once more under AddressSanitizer + UBSan; run as a program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lammps-spherharm_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "test_cylinder_rolling_check.cpp")

EXPECTED = """\
rolling accepted: ok
twisting accepted: ok
rolling accepted: ok
twisting accepted: ok
none set: ok
rolling count: cylinder rolling resistance: 3 coefficients for 2 cylinders (call it after shstep_set_cylinders)
twisting count before any cylinder: cylinder twisting resistance: 3 coefficients for 0 cylinders (call it after shstep_set_cylinders)
rolling null mu: cylinder rolling resistance: null array pointer
twisting null gamma: cylinder twisting resistance: null array pointer
rolling negative mu: cylinder 2: rolling coefficient mu_r -0.5 must be finite and >= 0
twisting negative mu: cylinder 2: twisting coefficient mu_tw -0.5 must be finite and >= 0
rolling negative gamma: cylinder 1: rolling coefficient gamma_r -2 must be finite and >= 0
twisting nan gamma: cylinder 1: twisting coefficient gamma_tw nan must be finite
rolling inf mu: cylinder 0: rolling coefficient mu_r inf must be finite
fresh: roll 0 any 0 damp 0 fric 0 hist 0
mu_r and gamma_r on different cylinders: roll 0 any 0 damp 0 fric 0 hist 0
rolling on cylinder 0: roll 1 any 1 damp 0 fric 0 hist 0
and a rotation: roll 1 any 1 damp 0 fric 0 hist 0
twisting alone on cylinder 2: roll 1 any 1 damp 0 fric 0 hist 0
and damping: roll 1 any 1 damp 1 fric 0 hist 0
reset: roll 0 any 0 damp 0 fric 0 hist 0
image 12: 1 2 3 4 5 6 7 8 9 10 11 12
"""


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_the_setters_checks_the_switch_and_the_image(tmp_path, flags):
    out = tmp_path / "test_cylinder_rolling_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{CSRC}", SRC, "-o", str(out)])
    res = subprocess.run([str(out)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout == EXPECTED
    assert res.stderr == ""
