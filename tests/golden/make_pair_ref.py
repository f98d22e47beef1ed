"""Recorder of tests/golden/pair_ref_<name>.npz and tests/golden/root_shortcut.json.  CPU only, minutes in total:

    python tests/golden/make_pair_ref.py [case ...]

Each fixture holds a small bed (inputs) and, per list slot, the integrals of tests/pair_ref.py, whose inner radii are
exact roots.  root_shortcut.json records how far the CPU oracle -- which accepts the extrapolated inner radius of
docs/SPEC.md §2.6 without evaluating it -- sits from that reference: the cost of the shortcut, per case.  The tests hold
the oracle and the HIP kernels to 1.5 x these figures (tests/test_pair_ref.py, tests/test_gpu_pair_ref.py).

No case needed its amplitude lowered or its spacing raised to stay under the 5 % limit on ambiguous slots.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "lammps-spherharm_amd"), ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import pair_ref                                  # noqa: E402
from common import make_case, make_soup          # noqa: E402
from mixed_common import MIN_MIXED_SLOTS, make_mixed_case, pad_anm, slot_classes      # noqa: E402
from oracle import oracle as O                   # noqa: E402

# name: lmax, n_q, particles, spacing, amp, shapes, types
BEDS = {
    "l4_shallow": (4, 10, 30, 1.9, 0.1, 1, 1),
    "l6_shallow": (6, 16, 30, 1.9, 0.1, 2, 2),
    "l6_deep": (6, 16, 24, 1.6, 0.1, 1, 1),
    "l6_rough": (6, 16, 24, 1.7, 0.25, 1, 1),
    "l12_shallow": (12, 32, 16, 1.9, 0.1, 1, 1),
    "l9_general": (9, 12, 24, 1.8, 0.1, 1, 1),
    "l3_body": (3, 7, 30, 1.8, 0.1, 1, 1),
    "l14_loop": (14, 8, 16, 1.9, 0.1, 1, 1),
}
# name: orders (one per shape), n_q, particles, spacing, amp, seed.  The fixture stores the shapes zero-padded to the largest
# order (lmax, a_nm as in every other fixture) and the orders themselves in own_lmax; the bounding radii are those of the
# shapes at their own orders.
MIXED = {
    "l3_9_mixed": ((3, 9), 16, 48, 1.8, 0.1, 5),
}


def inputs(name):
    if name == "soup":
        s = make_soup(6, O.shape_rmax, npair=40)
        return dict(lmax=6, nq=16, a_nm=np.array(s["shapes"]), rmax=np.array(s["rmax"]), x=s["x"], quat=s["quat"],
                    type=s["type"], shtype=s["shtype"], ilist=s["ilist"], offsets=s["offsets"], jlist=s["jlist"],
                    nlocal=len(s["x"]), ntypes=1, newton=1)
    if name in MIXED:
        orders, nq, n, spacing, amp, seed = MIXED[name]
        c = make_mixed_case(n, orders, seed=seed, amp=amp, spacing=spacing, rmax_fn=O.shape_rmax)
        b, lmax = c["bed"], c["lmax"]
        return dict(lmax=lmax, nq=nq, a_nm=np.array([pad_anm(l, lmax, a) for l, a in zip(orders, c["shapes"])]),
                    rmax=np.array(c["rmax"]), x=b["x"], quat=b["quat"], type=b["type"], shtype=b["shtype"], ilist=c["ilist"],
                    offsets=c["offsets"], jlist=c["jlist"], nlocal=n, ntypes=1, newton=1, own_lmax=np.array(orders, np.int32))
    lmax, nq, n, spacing, amp, nshapes, ntypes = BEDS["l6_shallow" if name == "ghosts" else name]
    c = make_case(n, lmax, nshapes, seed=3, amp=amp, spacing=spacing, ntypes=ntypes, rmax_fn=O.shape_rmax)
    b = c["bed"]
    g = dict(lmax=lmax, nq=nq, a_nm=np.array(c["shapes"]), rmax=np.array(c["rmax"]), x=b["x"], quat=b["quat"],
             type=b["type"], shtype=b["shtype"], ilist=c["ilist"], offsets=c["offsets"], jlist=c["jlist"], nlocal=n,
             ntypes=ntypes, newton=1)
    if name == "ghosts":                         # rows of the first 15 atoms; the others are ghosts, newton off
        g.update(nlocal=15, newton=0, ilist=c["ilist"][:15], offsets=c["offsets"][:16],
                 jlist=c["jlist"][:c["offsets"][15]])
    return g


def record(name):
    g = inputs(name)
    table = [(g["lmax"], a, r) for a, r in zip(g["a_nm"], g["rmax"])]
    nlist = (g["ilist"], g["offsets"], g["jlist"])
    ref = pair_ref.pair_list(table, g["nq"], g["x"], g["quat"], g["shtype"], *nlist)
    touch = ref["V"] > 0
    flagged = touch & ref["multi"]
    # conditions on the inputs, from the reference alone
    if name == "soup":
        for br in (0, 1, 2):
            assert (touch & (ref["branch"] == br)).sum() >= 3, (name, "cap branch", br)
        assert (touch & ref["rin0"]).sum() >= 3, (name, "r_in = 0")
    else:
        assert touch.sum() >= 40, (name, int(touch.sum()))
    if name in MIXED:
        cls = slot_classes(g["own_lmax"], g["shtype"], *nlist, touch)
        assert cls["low-high"] >= MIN_MIXED_SLOTS and cls["high-low"] >= MIN_MIXED_SLOTS, (name, cls)
    rj = g["rmax"][g["shtype"][g["jlist"] & 0x1FFFFFFF]]
    assert (ref["resid"] <= 1e-12 * rj).all(), (name, (ref["resid"] / rj).max())
    assert flagged.sum() <= 0.05 * touch.sum(), (name, int(flagged.sum()), int(touch.sum()))

    # the oracle against the reference
    newton = bool(g["newton"])
    args = (g["nq"], g["nlocal"], g["x"], g["quat"], g["type"], g["shtype"])
    K, E = pair_ref.kn_table(g["ntypes"], 1.0)
    o = O.compute(table, K, E, *args, *nlist, newton_pair=newton, force_volume=True, want_pairs=True)
    assert ((o["pairs"][:, 0] > 0) == touch).all()
    cmp_v = touch & ~flagged
    vdev = np.abs(o["pairs"][cmp_v, 0] - ref["V"][cmp_v]) / ref["V"][cmp_v]
    ev = nin = 0.0
    for ii, i in enumerate(g["ilist"]):
        for p in range(g["offsets"][ii], g["offsets"][ii + 1]):
            j = int(g["jlist"][p])
            _, _, diag = O.pair(*table[g["shtype"][i]], *table[g["shtype"][j]], g["x"][i], g["quat"][i], g["x"][j],
                                g["quat"][j], g["nq"])
            if not ref["rin0"][p]:           # a centre of i inside j needs no search
                ev, nin = ev + diag[2], nin + diag[0]
    rec = dict(n_slots=int(touch.size), n_touching=int(touch.sum()), n_flagged=int(flagged.sum()),
               v_dev_max=float(vdev.max()), v_dev_median=float(np.median(vdev)), f_dev={}, tau_dev={},
               evals_per_node=float(ev / nin))
    short = pair_ref.without_slots(nlist, flagged)
    for m in pair_ref.EXPONENTS:
        K, E = pair_ref.kn_table(g["ntypes"], m)
        use, skip = (nlist, None) if m == 1.0 else (short, flagged)
        o = O.compute(table, K, E, *args, *use, newton_pair=newton, force_volume=True)
        f, tq, _ = pair_ref.assemble(ref, nlist, g["x"], g["type"], K, E, g["nlocal"], newton, skip=skip)
        df, dt = pair_ref.deviations(o["f"], o["torque"], f, tq)
        rec["f_dev"][repr(m)], rec["tau_dev"][repr(m)] = float(df), float(dt)
    np.savez_compressed(os.path.join(HERE, f"pair_ref_{name}.npz"), **g, **ref)
    return rec


def main(names):
    path = os.path.join(HERE, "root_shortcut.json")
    table = {}
    if os.path.exists(path):
        with open(path) as fh:
            table = json.load(fh)
    for name in names:
        table[name] = record(name)
        print(name, json.dumps(table[name]), flush=True)
    with open(path, "w") as fh:
        json.dump({k: table[k] for k in pair_ref.CASES if k in table}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:] or list(pair_ref.CASES))
