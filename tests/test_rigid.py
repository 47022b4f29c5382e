"""CPU tests of the rigid-contact plant's numpy statement (trajectories.rigid_contact_acceleration, include/lmh.h) on the oracle's terms:
the 16 states of plant_step_cases.contact_states() x three support modes x kv in {0, 50}.  Oracle and numpy only.

Tolerances are the project's own (test_gpu_plant_step.py, test_gpu_terms.py): backward error 1e-12, forward error 1e-12 cond(KKT) against
a long-double-refined KKT solve, the constraint residual 1e-12 on the scale |A| |lam| + |g| of the system it is the residual of.
That the unpivoted Gauss-Jordan meets only positive pivots is checked here near standing (smallest 0.473) and by test_fall_rigid_cases.py
over the fall bands (smallest 0.399) and the pitch ladder (0.567)."""
import numpy as np

import plant_step_cases as pc
import rigid_cases as rc
from linearmpchumanoid_amd import capi
from linearmpchumanoid_amd.trajectories import rigid_contact_acceleration, rigid_modes, walk_plan


def test_statement_meets_the_three_bounds_on_every_case():
    S = rc.rigid_cases()
    worst = dict(backward=0.0, constraint=0.0, forward=0.0, cond=0.0, condA=0.0)
    min_pivot = np.inf
    for (i, m, kv), c in S["cases"].items():
        b = rc.bounds(S["terms"][i], S["tau"][i], m, kv, c["a"], c["lam"])
        for k in ("backward", "constraint", "forward", "cond"):
            worst[k] = max(worst[k], b[k])
        worst["condA"] = max(worst["condA"], float(np.linalg.cond(c["info"]["A"])))
        min_pivot = min(min_pivot, float(c["info"]["pivots"].min()))
        assert np.isfinite(c["a"]).all() and np.isfinite(c["lam"]).all()
        assert b["backward"] <= 1e-12 and b["constraint"] <= 1e-12 and b["forward"] <= 1e-12, ((i, m, kv), b)
    print("\nrigid statement, 96 cases: backward %.2e, constraint %.2e, forward/cond %.2e; cond(KKT) <= %.2e, cond(A) <= %.2e, smallest "
          "unpivoted pivot %.3g" % (worst["backward"], worst["constraint"], worst["forward"], worst["cond"], worst["condA"], min_pivot))
    assert min_pivot > 0.0                                         # no pivoting is needed


def test_flight_is_the_unconstrained_solve_and_a_free_foot_carries_nothing():
    S = rc.rigid_cases()
    for i in range(rc.B):
        tm = S["terms"][i]
        for kv in rc.KVS:
            a, lam, flags = rigid_contact_acceleration(tm["M"], tm["C"], tm["J"], tm["Jpqp"], tm["vhat"], S["tau"][i], capi.PHASE_FLIGHT, kv)
            assert np.array_equal(a, np.linalg.solve(tm["M"], S["tau"][i] - tm["C"])) and not lam.any() and flags == 0
            assert not S["cases"][(i, capi.PHASE_RIGHT, kv)]["lam"][6:].any()       # exactly zero, not small
            assert not S["cases"][(i, capi.PHASE_LEFT, kv)]["lam"][:6].any()
            assert S["cases"][(i, capi.PHASE_RIGHT, kv)]["lam"][:6].all() and S["cases"][(i, capi.PHASE_LEFT, kv)]["lam"][6:].all()
            # only the low two bits of the mode are read; tau30 = None is a passive robot
            a4, lam4, f4 = rigid_contact_acceleration(tm["M"], tm["C"], tm["J"], tm["Jpqp"], tm["vhat"], S["tau"][i], capi.PHASE_RIGHT + 4, kv)
            c = S["cases"][(i, capi.PHASE_RIGHT, kv)]
            assert np.array_equal(a4, c["a"]) and np.array_equal(lam4, c["lam"]) and f4 == c["flags"]
        ap, _, _ = rigid_contact_acceleration(tm["M"], tm["C"], tm["J"], tm["Jpqp"], tm["vhat"], None, 0, 0.0)
        az, _, _ = rigid_contact_acceleration(tm["M"], tm["C"], tm["J"], tm["Jpqp"], tm["vhat"], np.zeros(30), 0, 0.0)
        assert np.array_equal(ap, az)


def test_the_pull_flag_sees_both_outcomes():
    """A condition on the cases, not on the code: each of pull and no-pull occurs in at least 16 of the 96."""
    S = rc.rigid_cases()
    pull = sum(1 for c in S["cases"].values() if c["flags"] & capi.FLAG_CONTACT_PULL)
    slip = sum(1 for c in S["cases"].values() if c["flags"] & capi.FLAG_CONTACT_SLIP)
    print("\nrigid flags over the 96 cases: pull %d, no pull %d, slip %d" % (pull, 96 - pull, slip))
    assert pull >= 16 and 96 - pull >= 16
    for (i, m, kv), c in S["cases"].items():                       # the flag is the statement's sentence, foot by foot
        held = [ft for ft in range(2) if 6 * ft in c["info"]["rows"]]
        assert bool(c["flags"] & capi.FLAG_CONTACT_PULL) == any(c["lam"][6 * ft + 5] < 0.0 for ft in held)
        assert bool(c["flags"] & capi.FLAG_CONTACT_SLIP) == any(np.hypot(*c["lam"][6 * ft + 3:6 * ft + 5]) > rc.MU * c["lam"][6 * ft + 5] for ft in held)


def test_twenty_substeps_are_finite_and_the_held_twist_decays():
    """rk4_tick over the statement, both soles held.  The held soles' twist shrinks by e^(-kv 20 dt) within 1e-3 relative, at kv = 50 and
    (factor 1) at kv = 0, in the sense of rigid_cases.twist_decay_error: RK4's own error at kv dt = 0.05 is orders below, a wrong sign or
    a missing term orders above.  That sense: the angular part component by component, the linear part in magnitude -- the constraint's
    Jdot qdot is the sole's spatial acceleration turned to world axes, so the linear part also turns with the sole, and component by
    component it is 6.0e-3 (kv = 0) and 3.8e-3 (kv = 50) off on these states, which the test prints and does not assert; in magnitude it is
    1.8e-6 and 6.2e-6 off.  Prints the drift of the sole origins over the 20 substeps, a measured figure."""
    S = rc.rigid_cases()
    o = pc.make_oracle()
    n, tau = 20, rc.step_tau()
    worst, turn, drift = {0.0: 0.0, 50.0: 0.0}, {0.0: 0.0, 50.0: 0.0}, {0.0: 0.0, 50.0: 0.0}
    for i in (0, 5, 10, 15):
        x0 = np.concatenate([S["q"][i], S["v"][i]])
        w0, p0 = rc.sole_twist(o, x0), rc.sole_positions(o, x0)
        for kv in rc.KVS:
            x, flags, lam = rc.oracle_rigid_steps(o, x0, tau[i], capi.PHASE_DOUBLE, kv, n)
            assert np.isfinite(x).all() and np.isfinite(lam).all() and not flags & capi.FLAG_NONFINITE
            err, comp = rc.twist_decay_error(rc.sole_twist(o, x), w0, kv, n * rc.DT)
            worst[kv], turn[kv] = max(worst[kv], err), max(turn[kv], comp)
            drift[kv] = max(drift[kv], float(np.abs(rc.sole_positions(o, x) - p0).max()))
            assert err <= 1e-3, (i, kv, err)
    print("\nrigid plant, 20 substeps of 1 ms, both soles held: twist against e^(-kv t) w_0: %.2e (kv = 0), %.2e (kv = 50); linear part "
          "component by component %.2e, %.2e; drift of the sole origins %.3e m (kv = 0), %.3e m (kv = 50)"
          % (worst[0.0], worst[50.0], turn[0.0], turn[50.0], drift[0.0], drift[50.0]))


def test_rigid_modes_follow_the_plan():
    ph = walk_plan(2.0, 1e-2)["phase"]
    assert {int(p) for p in ph} == {capi.PHASE_DOUBLE, capi.PHASE_RIGHT, capi.PHASE_LEFT}
    assert rigid_modes(ph, 0) == capi.PHASE_DOUBLE and rigid_modes(ph, 0).dtype == np.int32
    for k in (0, len(ph) // 2, len(ph) - 1):
        assert rigid_modes(ph, k) == ph[k]
    assert rigid_modes(ph, -5) == ph[0] and rigid_modes(ph, 10 ** 9) == ph[-1]         # clamped into the arrays
    both = np.stack([ph, ph[::-1]])
    k = int(np.argmax(ph != ph[::-1]))
    assert np.array_equal(rigid_modes(both, k), np.array([ph[k], ph[::-1][k]], dtype=np.int32))
