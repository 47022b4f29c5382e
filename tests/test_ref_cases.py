"""CPU checks of the checker test_gpu_ref.py leans on (ref_cases.py): the numpy restatement with a supplied CoM reference.

1. RefMpc fed with Mpc.compute's own xRef / yRef gives the plain restatement's result exactly: the subclass changes where the six numbers
   come from and nothing else.
2. The restatement's distance to the C oracle on these states (built-in MPC step, the only form the oracle has), by the rules the GPU test
   applies to the same outputs (test_gpu_posture_sweep.py: tau and qdd relative to their own largest entry, f on the robot's weight).  It has
   to stay below a tenth of helpers.TOL_REL for the GPU test to use TOL_REL as it stands; measured 3.8e-11 (tau), 1.1e-11 (f), 1.6e-11 (qdd).
3. The off-manifold references are what they claim: inside their bands around the CoM state, and no LIPM step of the robot's state."""
import numpy as np

import ref_cases as rc
from helpers import TOL_REL, WEIGHT, oracle_system, vec_err


def test_supplied_own_values_reproduce_the_plain_restatement_exactly():
    plain = rc.plain_restatement()
    for i in range(rc.B):
        out = rc.with_reference(i, plain[i]["xref"], plain[i]["yref"])
        for key in ("tau", "f", "qpp", "x", "href", "g"):
            assert np.array_equal(out[key], plain[i]["out"][key]), (i, key)
        assert out["active"] == plain[i]["out"]["active"] and plain[i]["k"] == 0


def test_restatement_distance_to_the_oracle_is_below_a_tenth_of_the_tolerance():
    S, plain = rc.states(), rc.plain_restatement()
    worst = dict(tau=0.0, f=0.0, qdd=0.0)
    for i in range(rc.B):
        o = oracle_system(rc.DT, rc.TH)
        o.set_prev_velocity(S["vp"][i])
        e = o.eval(S["q"][i], S["v"][i], 0.0)
        assert e["qp_status"] == 0 and e["k"] == 0
        out = plain[i]["out"]
        worst["tau"] = max(worst["tau"], vec_err(out["tau"], e["tau"]))
        worst["qdd"] = max(worst["qdd"], vec_err(out["qpp"], e["qpp"]))
        worst["f"] = max(worst["f"], float(np.abs(out["f"] - e["f"]).max() / WEIGHT))
    print("\nrestatement vs oracle on the reference-test states:", {k: "%.2e" % v for k, v in worst.items()})
    for k, v in worst.items():
        assert v < 0.1 * TOL_REL, (k, v)


def test_off_manifold_references_are_inside_their_bands_and_off_the_lipm_step():
    plain, rec = rc.plain_restatement(), rc.off_manifold_refs()
    assert rec.shape == (rc.B, 16) and np.isfinite(rec).all()
    A, Bm = np.array([[1.0, rc.DT], [0.0, 1.0]]), np.array([rc.DT * rc.DT / 2, rc.DT])
    for i in range(rc.B):
        for ax in range(2):
            p, v, a = rec[i, 3 * ax:3 * ax + 3]
            assert abs(p - plain[i]["com"][ax]) <= rc.REF_POS and abs(v - plain[i]["comvel"][ax]) <= rc.REF_VEL and abs(a) <= rc.REF_ACC
            step = A @ np.array([plain[i]["com"][ax], plain[i]["comvel"][ax]]) + Bm * a
            assert max(abs(step[0] - p), abs(step[1] - v)) > 1e-4, (i, ax)     # no x+ = A x + B u with the supplied u
    # and they move the result: the supplied reference is not the one the built-in step would have formed
    offm = rc.off_manifold_results()
    assert all(vec_err(offm[i]["tau"], plain[i]["out"]["tau"]) > 1e-3 for i in range(rc.B))
