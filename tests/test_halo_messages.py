"""CPU check of the per-peer message list of the halo layer (csrc/halo_plan.hpp halo_peer_blocks, what every forward and
reverse exchange of csrc/shhalo_api.hip is built from): tests/host/test_halo_messages.cpp, built with g++ under
AddressSanitizer + UBSan together with the host planner (csrc/halo_plan.cpp), walks every rank of the grids 2x1x1, 2x2x1,
2x2x2 and 1x1x1 with seeded send counts that include zeros."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lammps-spherharm_amd", "csrc")


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    out = tmp_path_factory.mktemp("host") / "test_halo_messages"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           f"-I{CSRC}", os.path.join(ROOT, "tests", "host", "test_halo_messages.cpp"),
                           os.path.join(CSRC, "halo_plan.cpp"), "-o", str(out)])
    return str(out)


def test_message_lists_follow_the_layout_on_every_rank(binary):
    r = subprocess.run([binary], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.fullmatch(r"ok (\d+)\n", r.stdout)
    assert m and int(m.group(1)) == 2 * 8 * (2 + 4 + 8 + 1), r.stdout   # a forward and a reverse list per rank, 8 seeds per grid
