"""CPU checks of the contact kernel's launch planner (csrc/contact_plan.hpp): at every row of
tests/golden/contact_plans.csv — the plans a build reported through shpair_get_kernel_info on the GPU
(tools/record_contact_plans.py) — the planner, built with g++ under AddressSanitizer + UBSan, must pick exactly
the same kernel and sizes, given the two-wave kernels' VGPR counts read from the built library's code objects.
And PairSpec<L> must be what the planner picks at its shape, so the specialised instances cannot silently stop
running."""
import csv
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lammps-spherharm_amd", "csrc")
LIB = os.path.join(ROOT, "lammps-spherharm_amd", "shpair", "libshpair.so")
FIXTURE = os.path.join(ROOT, "tests", "golden", "contact_plans.csv")
# the option fields of ContactOptions, in the order tests/host/test_contact_plan.cpp reads them, at their defaults
OPTION_DEFAULTS = {"variant": 0, "rule": 0, "jpoly": -1, "split": -1, "ring_rows": 0, "waves_per_block": 0,
                   "queue_slack": 1, "spec": 1}


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", f"{name}.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def binary(tmp_path_factory):
    out = tmp_path_factory.mktemp("host") / "test_contact_plan"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           f"-I{CSRC}", os.path.join(ROOT, "tests", "host", "test_contact_plan.cpp"), "-o", str(out)])
    return str(out)


@pytest.fixture(scope="module")
def two_wave_vgprs():
    """{L: VGPRs of pair_contact_azimuth_kernel<L, true, 2>} (the general two-wave kernel with the volume path)."""
    pat = re.compile(r"_ZN3shp27pair_contact_azimuth_kernelILi(\d+)ELb1ELi2ELb0EEEvNS_10PairParamsE")
    out = {int(m.group(1)): k["vgprs"] for k in _tool("kernel_meta").kernels(LIB) for m in [pat.fullmatch(k["symbol"])] if m}
    assert sorted(out) == list(range(7, 13)), out
    return out


def test_planner_reproduces_recorded_plans(binary, two_wave_vgprs):
    rec = _tool("record_contact_plans")
    with open(FIXTURE) as fh:
        rows = list(csv.DictReader(fh))
    assert len(rows) == sum(1 for _ in rec.grid())
    cases = []
    for r in rows:
        o = dict(OPTION_DEFAULTS, **rec.OPTS[r["opts"]])
        L = int(r["lmax"])
        cases.append(" ".join(str(v) for v in [L, r["nq"], *o.values(), two_wave_vgprs.get(L, 0)]))
    out = subprocess.run([binary], input="\n".join(cases) + "\n", capture_output=True, text=True, check=True).stdout
    lines = out.strip().split("\n")
    assert len(lines) == len(rows)
    bad = []
    for r, ln in zip(rows, lines):
        got, _, msg = ln.partition(" | ")
        got = got.split()
        want = [r["rc"]] + ([r[f] for f in rec.FIELDS] if int(r["rc"]) == 0 else ["-1"] * len(rec.FIELDS))
        if got != want:
            bad.append(f"{r['opts']} L={r['lmax']} nq={r['nq']}: recorded {want}, planned {got}")
        if int(r["rc"]) != 0:
            assert re.fullmatch(r"the weighted rule needs lmax <= 12 and nq <= 32 \(have lmax \d+, nq \d+\)|"
                                r"lmax \d+ with nq \d+ needs \d+ bytes of LDS per pair, more than a CU has", msg), msg
    assert not bad, f"{len(bad)} of {len(rows)} plans differ:\n" + "\n".join(bad[:40])


def test_pair_spec_is_what_the_planner_picks(binary, two_wave_vgprs):
    out = subprocess.check_output([binary, "specs", str(two_wave_vgprs[12])], text=True)
    for ln in out.strip().split("\n"):
        spec, _, plan = ln.partition(" | ")
        L, nq, rr, qc, wpp = map(int, spec.split())
        rc, prr, pqc, pwpp = map(int, plan.split())
        assert rc == 0 and (prr, pqc, pwpp) == (rr, qc, wpp), f"PairSpec<{L}> (n_q {nq}): rr, qc, wpp {rr, qc, wpp}, planner {prr, pqc, pwpp}"
