"""bench.py's plain line and --dump-outputs: a plain N = 1 run carries the headline alone (everything else is behind
--full), and the arrays the timed path computed in its last step come out as float64 .npy files that two runs with the
same arguments reproduce (the bed is seeded; only the order of the FP64 atomic sums differs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "occupancy", "valu_f64", "utilisation", "host_path", "configs", "timestep", "scale_ref", "cpu_baseline")


def _last_json(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out[-2000:]
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def test_dump_outputs_writes_float64_and_samples_the_same_rows_of_every_array(tmp_path, monkeypatch):
    import bench
    rng = np.random.default_rng(1)
    arrays = {"f": rng.normal(size=(1000, 3)), "quat": rng.normal(size=(1000, 4)).astype(np.float32)}
    bench.dump_outputs(str(tmp_path / "all"), arrays)
    got = _load(tmp_path / "all")
    assert set(got) == {"f", "quat"} and all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["f"], arrays["f"]) and np.array_equal(got["quat"], arrays["quat"].astype(np.float64))
    # over the budget: one seeded sample of rows, ascending, the same in every array and in every run
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 20000)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), arrays)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(x.nbytes for x in a.values()) <= 20000 and a["f"].shape[0] == a["quat"].shape[0] > 0
    assert all(np.array_equal(a[k], b[k]) for k in a)
    rows = np.array([np.flatnonzero((arrays["f"] == r).all(axis=1))[0] for r in a["f"]])
    assert np.all(np.diff(rows) > 0) and np.array_equal(a["quat"], arrays["quat"][rows].astype(np.float64))


def test_full_is_off_and_the_dump_directory_is_absolute_by_default(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 5 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "some/dir"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == os.path.abspath("some/dir")


@pytest.mark.gpu
def test_plain_line_is_the_headline_alone_and_its_outputs_reproduce(tmp_path):
    runs = []
    for name in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--particles", "20000", "--steps", "7",
                            "--warmup", "2", "--ramp", "2", "--dump-outputs", str(tmp_path / name)],
                           capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        runs.append(_last_json(r.stdout))
    d = runs[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config"):
        assert k in d, k
    assert d["full"] is False and not set(FULL_ONLY) & set(d), set(FULL_ONLY) & set(d)
    assert d["metric"] == "contact_pairs_per_sec" and d["unit"] == "contact-pairs/s" and d["dtype"] == "f64"
    assert d["higher_is_better"] is True and d["steps"] == 7 and d["warmup"] == 2 and d["value"] > 1e7
    n_contact = d["config"]["contact_pairs_all_ranks"]
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 - n_contact) < 1e-6 * n_contact
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(a) == {"f", "torque", "x", "v", "quat", "angmom"} and set(b) == set(a)
    n = d["config"]["particles_per_gpu"]
    assert all(x.dtype == np.float64 and x.shape == (n, 4 if k == "quat" else 3) for k, x in a.items())
    assert all(np.all(np.isfinite(x)) for x in a.values()) and np.abs(a["f"]).max() > 0 and np.abs(a["v"]).max() > 0
    assert sum(os.path.getsize(tmp_path / "a" / (k + ".npy")) for k in a) <= 64 * 10 ** 6
    for k in a:     # same seeded bed, same steps: equal up to the order of the atomic force sums
        scale = max(np.abs(a[k]).max(), 1e-300)
        assert np.abs(a[k] - b[k]).max() <= 1e-9 * scale, k


@pytest.mark.gpu
def test_multi_rank_dump_holds_every_owned_atom_in_tag_order(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--transport", "local", "--particles", "5000",
                        "--steps", "4", "--warmup", "1", "--ramp", "1", "--peak-ms", "0", "--halo-overlap", "0", "--no-verify-overlap",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _last_json(r.stdout)
    got = _load(tmp_path)
    n = d["config"]["particles_all_ranks"]
    assert set(got) == {"f", "torque", "x", "v", "quat"} and d["steps"] == 4
    assert all(x.dtype == np.float64 and x.shape == (n, 4 if k == "quat" else 3) and np.all(np.isfinite(x)) for k, x in got.items())
    assert np.abs(got["f"]).max() > 0
