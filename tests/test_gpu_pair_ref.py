"""The HIP pair kernels, through the C ABI, against the exact-root numpy reference of tests/pair_ref.py on the committed
small beds (tests/golden/pair_ref_<name>.npz; recorder tests/golden/make_pair_ref.py).  Needs neither the oracle nor a
run of the reference: the slow part is committed data.

What depends on no inner radius -- classification, S_n, T_n, the m = 1 wrench and its assembly onto the atoms -- is held
to docs/SPEC.md §4's 1e-9 on every slot.  What depends on the accepted inner radii of §2.6 -- V, the wrench at m = 1.25
and m = 2, the energy -- is held to 1.5 x the deviation that tests/golden/root_shortcut.json records for the same
search run by the CPU oracle: that figure is the truncation error of one fixed search path, a libm or compiler change
moves single roots by ~1e-9 relative (SPEC §4), and a factor of 1.5 means another path through the search.  Slots with a
node whose bracket holds several roots (flagged in the fixture; 1 slot, in l6_rough) are left out of the second group
only, by leaving them out of the list.  l3_9_mixed holds shapes of the orders 3 and 9, stored zero-padded to 9: the context
gets each at its own order (own_lmax) with the fixture's bounding radius.

Each test: one context, one compute, at most 80 atoms."""
import numpy as np
import pytest

import pair_ref

pytestmark = pytest.mark.gpu
GATE = 1e-9
MARGIN = 1.5

ALL = pair_ref.CASES
COMPILED = tuple(n for n in ALL if n != "l14_loop")          # orders that have both compiled families
VARIANTS = ([(n, "own", ()) for n in ALL] +
            [(n, f"jpoly{jp}", (("jpoly", jp),)) for n in COMPILED for jp in (0, 1)] +
            [(n, "split", (("jpoly", 1), ("split", 1))) for n in ("l9_general", "l12_shallow")] +
            [(n, "spec0", (("spec", 0),)) for n in ("l4_shallow", "l6_shallow", "l12_shallow")] +
            [(n, "loop", (("variant", 1),)) for n in ("l6_shallow", "l3_body")] +
            [("l6_shallow", "wpb2", (("waves_per_block", 2),))] +
            [(n, "det", (("deterministic", 1),)) for n in ALL])


@pytest.fixture(scope="module")
def shortcut():
    return pair_ref.load_shortcut()


@pytest.fixture(scope="module")
def fixtures():
    return {n: pair_ref.load_fixture(n) for n in ALL}


def expect_kernel(name, tag, k):
    """The kernel the options ask for is the one that ran."""
    base = {"l4_shallow": (4, 10), "l6_shallow": (6, 16), "l12_shallow": (12, 32)}
    if tag.startswith("jpoly"):
        assert k["family"] == int(tag[-1])
    if tag == "split":
        assert k["family"] == 1 and k["waves_per_pair"] == 2
    if tag == "loop":
        assert k["compiled_order"] == 0
    if name == "l14_loop":
        assert k["compiled_order"] == 0 and k["lmax"] == 14
    if name == "l3_9_mixed":
        assert k["lmax"] == 9
    if name in base and tag in ("own", "spec0"):
        assert k["specialised"] == (tag == "own") and k["family"] == 1
        assert k["waves_per_pair"] == (2 if name == "l12_shallow" else 1)
    assert k["scratch_bytes"] == 0


@pytest.mark.parametrize("m", pair_ref.EXPONENTS)
@pytest.mark.parametrize("name,tag,opts", VARIANTS, ids=[f"{n}-{t}" for n, t, _ in VARIANTS])
def test_kernels_against_the_exact_root_reference(fixtures, shortcut, name, tag, opts, m):
    import torch
    from shpair import ShPair
    g, rec = fixtures[name], shortcut[name]
    newton = bool(g["newton"])
    touch = g["V"] > 0
    flagged = touch & g["multi"]
    drop = flagged if m != 1.0 else np.zeros_like(flagged)     # m = 1 leaves no slot out
    keep = ~drop
    ilist, offsets, jlist = pair_ref.without_slots(g["nlist"], drop)
    K, E = pair_ref.kn_table(g["ntypes"], m)

    sp = ShPair(0)
    sp.settings(g["nq"])
    sp.set_ntypes(g["ntypes"], len(g["a_nm"]))
    for s, a in enumerate(g["a_nm"]):
        if "own_lmax" in g:       # shapes of several orders, stored zero-padded: the library gets each at its own order
            l = int(g["own_lmax"][s])
            assert not a[(l + 1) * (l + 2):].any()
            sp.set_shape(s, l, a[:(l + 1) * (l + 2)], float(g["rmax"][s]))
        else:
            sp.set_shape(s, g["lmax"], a)
        assert abs(sp.rmax(s) - g["rmax"][s]) < 1e-14
    for a in range(1, g["ntypes"] + 1):
        for b in range(1, g["ntypes"] + 1):
            sp.coeff(a, b, K[a, b], E[a, b])
    sp.set_neighbors_csr(ilist, offsets, jlist)
    sp.set_option("force_volume", 1)
    sp.set_option("count", 1)
    for key, value in opts:
        sp.set_option(key, value)
    out = torch.zeros(max(jlist.size, 1), 7, dtype=torch.float64, device="cuda:0")
    sp.set_pair_output(out.data_ptr())
    nall = len(g["x"])
    f, tq = np.zeros((nall, 3)), np.zeros((nall, 3))
    _, _, eng, _ = sp.compute(g["nlocal"], g["x"], g["quat"], g["type"], g["shtype"], newton_pair=newton, eflag=True,
                              f=f, torque=tq)
    got = out.cpu().numpy()[:jlist.size]
    ntouch = sp.stats()["n_touching"]
    kinfo = sp.kernel_info()
    sp.set_pair_output(None)
    sp.close()
    expect_kernel(name, tag, kinfo)

    f_ref, tq_ref, e_ref = pair_ref.assemble(g, g["nlist"], g["x"], g["type"], K, E, g["nlocal"], newton, skip=drop)
    df, dt = pair_ref.deviations(f, tq, f_ref, tq_ref)
    V, S, T = g["V"][keep], g["S"][keep], g["T"][keep]
    dS = np.abs(got[:, 1:4] - S).max() / np.abs(g["S"]).max()
    dT = np.abs(got[:, 4:7] - T).max() / np.abs(g["T"]).max()
    tv = V > 0
    dV = (np.abs(got[tv, 0] - V[tv]) / V[tv]).max()
    dE = abs(eng - e_ref) / e_ref
    print(f"{name} {tag} m={m}: S {dS:.2e} T {dT:.2e} V {dV:.2e} (recorded {rec['v_dev_max']:.2e}) F {df:.2e} tau {dt:.2e} "
          f"(recorded {rec['f_dev'][repr(m)]:.2e} {rec['tau_dev'][repr(m)]:.2e}) E {dE:.2e}")

    # no root involved: every slot
    assert ntouch == tv.sum() and np.array_equal(got[:, 0] > 0, tv)
    assert dS <= GATE and dT <= GATE
    if not newton:
        assert not f[g["nlocal"]:].any() and not tq[g["nlocal"]:].any()
    if m == 1.0:
        assert df <= GATE and dt <= GATE
    else:
        assert df <= MARGIN * rec["f_dev"][repr(m)] and dt <= MARGIN * rec["tau_dev"][repr(m)]
    # the accepted inner radii.  V and the energy: on the unflagged slots, which at m = 1 are all slots only where the
    # fixture has no flagged one
    cmp_v = ~g["multi"][keep] & tv
    assert (np.abs(got[cmp_v, 0] - V[cmp_v]) / V[cmp_v]).max() <= MARGIN * rec["v_dev_max"]
    if not flagged[keep].any():
        assert dE <= MARGIN * rec["v_dev_max"] * m
