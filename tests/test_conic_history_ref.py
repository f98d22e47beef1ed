"""CPU pins of tests/conic_history_ref.py, the numpy restatement of docs/SPEC.md §2.23 that the GPU cone-history tests
compare against: the cylinder of §2.19 as the limit theta -> 0, the plane of §2.15 as the limit theta -> pi/2, the
development of a 30-degree cone as an independent reference of the transport, four wrong transports that these three
tell from the right one, the symmetries and the reset guards.  Passes on any tree that has the reference: it pins the
yardstick, not the kernels."""
import numpy as np
import pytest

import cone_ref as Co
import conic_history_cases as K
import conic_history_ref as CH
import cyl_history_ref as CyH
import wall_history_ref as WH
from shpair import shapes

NQ, NPASS = 16, 8
LIMIT_BAR, DEV_BAR = 1e-6, 1e-12          # the project's bar for the two limits (tests/test_cone_ref.py); the development
TW = np.array([0.3, -0.2, 0.1, 0.5, 0.4, -0.6])


def rough_shape(oracle, seed=3):
    anm = shapes.random_shape(6, seed, amp=0.1)
    return (6, anm, oracle.shape_rmax(6, anm))


def sphere_shape():
    return (0, shapes.sphere(1.0), 1.01)


def twists(npass, scale=1.0):
    """A twist per pass that turns slowly, so that the tangential velocity changes direction along the way."""
    return [scale * TW * (1 + 0.1 * k) * np.array([1, 1, 1, np.cos(0.3 * k), 1, np.sin(0.3 * k) + 1]) for k in range(npass)]


# ---- the cylinder limit ---------------------------------------------------------------------------------------------

def cylinder_limit(shape, q, law, mu, kt=4e3, omega=1.7, dt=0.01):
    """§2.22's slender set-up (theta = 2.5e-8, the apex 1e8 R_i down the axis, local radius 2.5 R_i, h = 0.7 R_i); eight
    passes that move the centre 0.875 rad round the axis and 0.35 R_i along it.  Returns the largest relative difference of
    F_t and of (xi_g, xi_theta) to cyl_history_ref over the passes, and the kinds seen."""
    rm, ax = shape[2], K.AXIS
    th, t0 = 2.5e-8, 1e8 * rm
    Rc = t0 * np.tan(th)
    co = Co.cone(-t0 * ax, ax, th)
    cyl = np.array([0.0, 0.0, 0.0, *ax, Rc])
    xs = [(Rc - 0.7 * rm) * K.radial(ax, 0.4 + 0.125 * k) + 0.05 * k * rm * ax for k in range(NPASS)]
    tws = twists(NPASS)
    coef = dict(kn=1000.0, m=1.25, gamma=3.0, mu=mu, gt=2.0, omega=omega, kt=kt)
    got = K.follow(shape, NQ, co, xs, [q] * NPASS, tws, coef, dt, law=law)
    xi, live = np.zeros((1, 1, 2)), np.zeros((1, 1), bool)
    eF = eX = 0.0
    kinds = set()
    for k in range(NPASS):
        r = CyH.cyl_forces_history([shape], NQ, xs[k][None], np.asarray(q)[None], [0], tws[k][None], [cyl], 1000.0, 1.25, 3.0, mu, 2.0,
                                   omega, kt, xi, live, dt)
        xi, live = r["xi"], r["live"]
        Fc = r["contacts"][0][2]
        assert got[k]["kind"][0, 0] == r["kind"][0, 0]
        kinds.add(r["kind"][0, 0])
        eF = max(eF, np.abs(K.tangential_force(got[k]) - Fc).max() / np.linalg.norm(Fc))
        eX = max(eX, np.abs(got[k]["xi"][0, 0, :2] - xi[0, 0]).max() / np.abs(xi).max())
    return eF, eX, kinds


@pytest.mark.parametrize("which", ["sphere", "rough"])
def test_the_cylinder_spring_is_the_limit_of_a_slender_cone(oracle, which):
    """F_t and (xi_g, xi_theta) against tests/cyl_history_ref.py's F_t and (xi_a, xi_theta) within 1e-6 over eight passes,
    Omega = 1.7, sticking (mu = 0.5) and sliding (mu = 0.02).  Reached: sphere 3.8e-8 (F_t) and 6.1e-8 (xi), rough 6.0e-8
    and 1.0e-7: the coordinates of the centre carry 1e8 R_i."""
    shape = sphere_shape() if which == "sphere" else rough_shape(oracle)
    q = K.unit([0.5, -0.3, 0.7, 0.4])
    seen = set()
    for mu in (0.5, 0.02):
        eF, eX, kinds = cylinder_limit(shape, q, CH.EXACT, mu)
        print(f"{which} mu {mu}: dF_t {eF:.2e} dxi {eX:.2e} kinds {sorted(kinds)}")
        seen |= kinds
        assert max(eF, eX) <= LIMIT_BAR
    assert seen == {CH.STICK, CH.SLIDE}


# ---- the plane limit ------------------------------------------------------------------------------------------------

def plane_limit(law, mu, kt=4e3, dt=0.01):
    """theta = pi/2 - 1e-8, a unit sphere whose foot point lies 3 R_i from the apex and moves 0.875 rad round the axis in eight
    passes, h = 0.7 R_i, the cone at rest (a plane of §2.15 cannot turn).  A sphere: the cone's node frame turns with the
    azimuth and the plane's does not, which the sums of a rough shape would see at the level of the quadrature error.
    Returns the largest relative difference of F_t and of the spring vector to wall_history_ref, and the kinds seen."""
    shape = sphere_shape()
    rm, n = shape[2], K.AXIS
    th = np.pi / 2 - 1e-8
    co = Co.cone(K.APEX, n, th)
    plane = (*n, n @ K.APEX)
    xs = K.motion(co, 2.9 + 0.125 * np.arange(NPASS), 3.0 * rm + 0.02 * np.arange(NPASS), [0.7 * rm] * NPASS)
    tws = twists(NPASS)
    q = np.array([1.0, 0.0, 0.0, 0.0])
    coef = dict(kn=1000.0, m=1.25, gamma=3.0, mu=mu, gt=2.0, omega=0.0, kt=kt)
    got = K.follow(shape, NQ, co, xs, [q] * NPASS, tws, coef, dt, law=law)
    xi, live = np.zeros((1, 1, 3)), np.zeros((1, 1), bool)
    one = np.ones(1)
    eF = eX = 0.0
    kinds = set()
    for k in range(NPASS):
        r = WH.wall_forces_history([shape], NQ, xs[k][None], q[None], [0], tws[k][None], [plane], 1000.0 * one, 1.25 * one, 3.0 * one,
                                   mu * one, 2.0 * one, kt * one, np.zeros((1, 3)), xi, live, dt)
        xi, live = r["xi"], r["live"]
        Fw = r["contacts"][0][5]
        kinds.add(r["kind"][0, 0])
        eF = max(eF, np.abs(K.tangential_force(got[k]) - Fw).max() / np.linalg.norm(Fw))
        eX = max(eX, np.abs(K.spring_vector(got[k], co) - xi[0, 0]).max() / np.abs(xi).max())
    return eF, eX, kinds


def test_the_plane_spring_is_the_limit_of_a_wide_cone():
    """xi_g g^_c + xi_theta t^_c and F_t against tests/wall_history_ref.py's xi_iw and F_t within 1e-6 over eight passes in
    which the azimuth changes by 0.875 rad, sticking (mu = 0.5) and sliding (mu = 0.02).  Reached: 1.4e-7 (F_t) and 1.6e-7
    (xi): the curvature scale is 1e-8, and the contact point's quadratic loses half the digits there."""
    seen = set()
    for mu in (0.5, 0.02):
        eF, eX, kinds = plane_limit(CH.EXACT, mu)
        print(f"plane mu {mu}: dF_t {eF:.2e} dxi {eX:.2e} kinds {sorted(kinds)}")
        seen |= kinds
        assert max(eF, eX) <= LIMIT_BAR
    assert seen == {CH.STICK, CH.SLIDE}


# ---- the development ------------------------------------------------------------------------------------------------

def development(oracle, law, omega=1.7, dt=0.01):
    """theta = 30 degrees, the oblique axis, a rough L = 6 shape, eight sticking passes (mu = 50) along a path that crosses
    the cut of the azimuth.  The independent reference: the contact points mapped into the developed plane (radius the
    slant distance, polar angle sin theta times the azimuth in the wall's material frame), the spring held there as a
    Cartesian vector to which dt v_t is added in the local polar basis.  Returns the largest difference of its polar
    components to the transported (xi_g, xi_theta), relative to the largest |xi|."""
    shape = rough_shape(oracle)
    rm = shape[2]
    th = np.pi / 6
    co = Co.cone(K.APEX, K.AXIS, th)
    xs = K.motion(co, np.pi - 0.45 + 0.125 * np.arange(NPASS), 6.0 * rm + 0.1 * np.arange(NPASS), [0.7 * rm] * NPASS)
    tws = twists(NPASS)
    q = K.unit([0.5, -0.3, 0.7, 0.4])
    coef = dict(kn=1000.0, m=1.25, gamma=3.0, mu=50.0, gt=2.0, omega=omega, kt=4e3)
    got = K.follow(shape, NQ, co, xs, [q] * NPASS, tws, coef, dt, law=law)
    Xi, psi, prev = np.zeros(2), 0.0, None
    err, big, points, cut = 0.0, 0.0, [], False
    for k, r in enumerate(got):
        (_, _, Ft, ri, rc, vt, N, kind, ratio), = r["contacts"]
        assert kind == CH.STICK
        phi = CH.azimuth(co, rc)
        if prev is not None:
            cut = cut or abs(phi - prev) > np.pi
            psi += CH.wrap(phi - prev) - omega * dt        # the azimuth against the wall's material
        prev = phi
        beta = np.sin(th) * psi
        er, eb = np.array([np.cos(beta), np.sin(beta)]), np.array([-np.sin(beta), np.cos(beta)])
        slant = np.sqrt(rc @ rc) / np.sin(th)
        points.append(slant * er)                          # the contact point in the developed plane
        eg, et = CH.surface_frame(co, rc)
        Xi = Xi + dt * ((vt @ eg) * er + (vt @ et) * eb)
        big = max(big, np.linalg.norm(Xi))
        err = max(err, abs(Xi @ er - r["xi"][0, 0, 0]), abs(Xi @ eb - r["xi"][0, 0, 1]))
    assert cut                                             # the path crossed the cut of atan2
    travelled = np.linalg.norm(points[-1] - points[0])
    assert travelled > 0.3 * rm
    return err / big


def test_the_transport_is_the_development_of_the_cone(oracle):
    """Reached 9.8e-17; the bar is 1e-12."""
    e = development(oracle, CH.EXACT)
    print(f"development: {e:.2e}")
    assert e <= DEV_BAR


@pytest.mark.parametrize("law", CH.WRONG_LAWS)
def test_a_wrong_transport_misses_a_check_by_more_than_100_bars(oracle, law):
    """No transport keeps the cylinder limit and misses the plane and the development; the full angle misses the cylinder
    limit; the opposite sign misses the plane and the development; ignoring Omega dt keeps both limits (theta -> 0 has no
    transport, the plane does not turn) and misses the development."""
    q = K.unit([0.5, -0.3, 0.7, 0.4])
    cyl = max(cylinder_limit(sphere_shape(), q, law, 0.5)[:2]) / LIMIT_BAR
    pla = max(plane_limit(law, 0.5)[:2]) / LIMIT_BAR
    dev = development(oracle, law) / DEV_BAR
    print(f"{law}: cylinder limit {cyl:.1e} bars, plane limit {pla:.1e} bars, development {dev:.1e} bars")
    assert max(cyl, pla, dev) > 100.0
    want = {CH.NO_TRANSPORT: (False, True, True), CH.FULL_ANGLE: (True, False, True), CH.OPPOSITE: (False, True, True),
            CH.NO_OMEGA: (False, False, True)}[law]
    assert (cyl > 100.0, pla > 100.0, dev > 100.0) == want


# ---- symmetries and guards ------------------------------------------------------------------------------------------

def _oblique(oracle):
    shape = rough_shape(oracle)
    co = Co.cone(K.APEX, K.AXIS, np.pi / 6)
    x = K.centre(co, 0.8, 6.0 * shape[2], 0.7 * shape[2])
    return shape, co, x, K.unit([0.5, -0.3, 0.7, 0.4])


def _one(shape, co, x, q, tw, state, live, dt, mu=0.5, gamma=3.0, omega=1.7, mask=None):
    return CH.cone_forces_history([shape], NQ, x[None], np.asarray(q)[None], [0], np.asarray(tw)[None], [co], 1000.0, 1.25, gamma, mu, 2.0,
                                  omega, 4e3, np.asarray(state, float).reshape(1, 1, 3), [[live]], dt, mask=mask)


def test_a_rotation_about_the_axis_keeps_the_components_and_shifts_the_azimuth(oracle):
    shape, co, x, q = _oblique(oracle)
    a, ax = co[:3], co[3:6]
    state = np.array([2e-3, -1e-3, 0.5])
    r = _one(shape, co, x, q, TW, state, True, 0.01)
    al = 2.9                                               # carries the azimuth over the cut
    g, G = K.turn(ax, al)
    state2 = np.array([state[0], state[1], CH.wrap(state[2] + al)])
    r2 = _one(shape, co, a + G @ (x - a), K.qmul(g, q), np.concatenate([G @ TW[:3], G @ TW[3:]]), state2, True, 0.01)
    sc = np.abs(r["f"]).max()
    dxi = np.abs(r2["xi"][0, 0, :2] - r["xi"][0, 0, :2]).max() / np.abs(r["xi"][0, 0, :2]).max()
    dphi = abs(CH.wrap(r2["xi"][0, 0, 2] - r["xi"][0, 0, 2] - al))
    dF = max(np.abs(r2["f"][0] - G @ r["f"][0]).max(), np.abs(r2["torque"][0] - G @ r["torque"][0]).max()) / sc
    print(f"rotation: dxi {dxi:.1e} dphi {dphi:.1e} wrench {dF:.1e} M_ax {abs(r2['cone_out'][0, 4] - r['cone_out'][0, 4]) / sc:.1e}")
    assert r["live"][0, 0] and np.linalg.norm(K.tangential_force(r)) > 0
    assert dxi <= 1e-12 and dphi <= 1e-12 and dF <= 1e-12 and abs(r2["cone_out"][0, 4] - r["cone_out"][0, 4]) <= 1e-12 * sc


def test_a_particle_carried_round_by_the_cone_keeps_its_spring(oracle):
    """x and quat turned by Omega dt per pass, w = Omega a^ x (x - a), omega = Omega a^: over 8 advancing passes (xi_g,
    xi_theta) stay what they were given to 1e-12 relative, and the wrench only rotates."""
    shape, co, x, q = _oblique(oracle)
    a, ax = co[:3], co[3:6]
    Om, dt = 2.0, 0.05
    tw = lambda x: np.concatenate([Om * np.cross(ax, x - a), Om * ax])
    look = _one(shape, co, x, q, tw(x), np.zeros(3), False, dt, omega=Om)
    phi0 = CH.azimuth(co, look["contacts"][0][4])
    state = np.array([2e-3, -1e-3, CH.wrap(phi0 - Om * dt)])   # as the pass before this one left it
    g, G = K.turn(ax, Om * dt)
    Gk, first = np.eye(3), None
    for k in range(8):
        r = _one(shape, co, x, q, tw(x), state, True, dt, omega=Om)
        assert r["kind"][0, 0] == CH.STICK
        if first is None:
            first = (r["f"][0], r["torque"][0])
        sc = np.linalg.norm(first[0])
        dx = np.abs(r["xi"][0, 0, :2] - [2e-3, -1e-3]).max() / 2e-3
        dw = max(np.abs(r["f"][0] - Gk @ first[0]).max(), np.abs(r["torque"][0] - Gk @ first[1]).max()) / sc
        print(f"co-rotation pass {k}: dxi {dx:.1e} wrench {dw:.1e}")
        assert dx <= 1e-12 and dw <= 1e-12
        state = r["xi"][0, 0]
        x, q, Gk = a + G @ (x - a), K.qmul(g, q), G @ Gk


def test_a_look_writes_nothing_and_transports_without_the_drive(oracle):
    shape, co, x, q = _oblique(oracle)
    state = np.array([2e-3, -1e-3, 0.5])
    r = _one(shape, co, x, q, TW, state, True, 0.0)
    assert np.array_equal(r["xi"][0, 0], state) and r["live"][0, 0]
    (_, _, Ft, ri, rc, vt, N, kind, ratio), = r["contacts"]
    eg, et = CH.surface_frame(co, rc)
    xi = CH.transported(state, CH.azimuth(co, rc), co[7], 1.7, 0.0)
    db = co[7] * (CH.azimuth(co, rc) - 0.5)
    assert np.allclose(xi, [state[0] * np.cos(db) + state[1] * np.sin(db), -state[0] * np.sin(db) + state[1] * np.cos(db)], rtol=0, atol=1e-18)
    assert kind == CH.STICK and np.abs(Ft - (-4e3 * (xi[0] * eg + xi[1] * et) - 2.0 * vt)).max() <= 1e-12 * np.linalg.norm(Ft)
    dead = _one(shape, co, x, q, TW, state, False, 0.0)       # a dead row reads as 0 whatever it holds
    assert np.abs(dead["contacts"][0][2] + 2.0 * vt).max() <= 1e-12 * np.linalg.norm(vt)


def test_every_guard_clears_the_bit_and_a_new_contact_starts_from_nothing(oracle, monkeypatch):
    shape, co, x, q = _oblique(oracle)
    rm = shape[2]
    state = np.array([2e-3, -1e-3, 0.5])
    ok = _one(shape, co, x, q, TW, state, True, 0.01)
    assert ok["live"][0, 0] and ok["kind"][0, 0] in (CH.STICK, CH.SLIDE)
    cases = {}
    cases["out of reach"] = _one(shape, co, K.centre(co, 0.8, 6.0 * rm, 1.2 * rm), q, TW, state, True, 0.01)
    cases["not in the group"] = _one(shape, co, x, q, TW, state, True, 0.01, mask=[2])
    sph = sphere_shape()
    cases["V = 0"] = _one(sph, co, K.centre(co, 0.8, 6.0, 1.005), q, TW, state, True, 0.01)
    away = np.concatenate([-50.0 * (co[7] * co[3:6] - co[6] * K.radial(co[3:6], 0.8)) * -1, np.zeros(3)])   # towards the axis
    cases["N = 0"] = _one(shape, co, x, q, away, state, True, 0.01, gamma=1e3)
    monkeypatch.setattr(Co, "contact_point", lambda *a: None)
    cases["a friction guard"] = _one(shape, co, x, q, TW, state, True, 0.01)
    monkeypatch.undo()
    for name, r in cases.items():
        assert not r["live"].any() and not r["xi"].any() and r["kind"][0, 0] == CH.RESET, name
        assert not r["contacts"], name
    assert cases["N = 0"]["ncontacts"] == 1 and not cases["N = 0"]["f"].any()       # V > 0, and the wall does not pull
    assert cases["V = 0"]["ncontacts"] == 0 and cases["a friction guard"]["f"].any()
    # re-entered: from nothing, whatever the row still holds
    back = _one(shape, co, x, q, TW, cases["out of reach"]["xi"][0, 0], cases["out of reach"]["live"][0, 0], 0.01)
    fresh = _one(shape, co, x, q, TW, np.array([9.0, 9.0, 9.0]), False, 0.01)
    (_, _, Ft, ri, rc, vt, N, kind, ratio), = back["contacts"]
    eg, et = CH.surface_frame(co, rc)
    assert np.array_equal(back["xi"], fresh["xi"]) and kind == CH.STICK
    assert np.allclose(back["xi"][0, 0, :2], [0.01 * (vt @ eg), 0.01 * (vt @ et)], rtol=1e-14, atol=0)
    assert not np.allclose(back["xi"][0, 0, :2], ok["xi"][0, 0, :2], rtol=1e-3, atol=0)
