"""CPU-only: the coefficient rules that the planar walls and the cylinders share (csrc/surface_coefficients.hpp: the
setters' argument check with both families' words, the record of the coefficients, the switches damp / fric / hist / roll
derived from it, the [k][n] images of the device tables), in a stand-alone host program
(tests/host/test_surface_coefficients.cpp): built plainly, and once more under AddressSanitizer + UBSan.  And neither
family's files spell the rules themselves."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lammps-spherharm_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "test_surface_coefficients.cpp")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_the_coefficient_rules_hold_for_walls_and_cylinders(tmp_path, flags):
    out = tmp_path / "test_surface_coefficients"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{CSRC}", SRC, "-o", str(out)])
    res = subprocess.run([str(out)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.strip() == "ok"
    assert res.stderr == ""


def test_the_header_is_host_only_and_neither_family_spells_the_rules_itself():
    with open(os.path.join(CSRC, "surface_coefficients.hpp")) as f:
        includes = re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", f.read())
    assert includes and not [i for i in includes if "hip" in i or i.endswith(".hpp")], includes
    for name in ("shstep_walls.hip", "shstep_cylinders.hip", "shstep_state.hpp", "cylinder_check.hpp"):
        with open(os.path.join(CSRC, name)) as f:
            text = re.sub(r"//[^\n]*", "", f.read())
        # an entry of a coefficient table compared with zero, the count refusal's words
        assert not re.search(r"\b(mu|gamma|kt|k_t|h)\w*\[[^\]]*\] != 0\.0|coefficients for %d", text), name
