"""CPU-only: the two pure rules of the surface history (csrc/surface_history.hpp: live words from an xi array, an xi array
masked by live words), which the planar walls (SPEC §2.15) and the cylinders (§2.19) share, in a stand-alone host program
(tests/host/test_surface_history.cpp) for both instantiations: built plainly, and once more under AddressSanitizer +
UBSan.  And neither family's files spell the shared rules themselves."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lammps-spherharm_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "test_surface_history.cpp")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_the_history_rules_hold_for_walls_and_cylinders(tmp_path, flags):
    out = tmp_path / "test_surface_history"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *flags, f"-I{CSRC}", SRC, "-o", str(out)])
    res = subprocess.run([str(out)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.strip() == "ok"
    assert res.stderr == ""


def test_neither_family_spells_the_shared_rules_itself():
    for name in ("wall_kernels.hpp", "cylinder_kernels.hpp", "shstep_walls.hip", "shstep_cylinders.hip"):
        with open(os.path.join(CSRC, name)) as f:
            text = f.read()
        # the queue's ballot, the live_dead rule, a memset of the live words
        assert not re.search(r"__ballot|live_dead = 1|hipMemset(Async)?\([^;]*live", text), name
