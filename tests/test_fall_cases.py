"""CPU side of the fall-parity tests: conditions on the draw of fall_cases.py, so that no case of test_gpu_fall_parity.py passes vacuously,
and the reference judged alone on those 32 states -- the C oracle against the independent numpy restatement, numpy's solve against a
long-double solve, the helper's Euler-rate map against a long-double one next to its singularity.  The figures printed here are the ones
DESIGN.md ("Fall parity") and the docstring of test_gpu_fall_parity.py quote; they decide whether a GPU tolerance may be wider than the
project's own (it may not: every figure is below a hundredth of its tolerance).  No GPU is used."""
import numpy as np
import pytest

import fall_cases as fc
import ground_cases as gc
import plant_step_cases as pc
from helpers import sincos_quadrants
from oracle import restatement_np as R


def _ninf(a):
    return float(np.abs(a).sum(axis=1).max()) if np.ndim(a) == 2 else float(np.abs(a).max())


# ------------------------------------------------------------------------------- the draw
@pytest.mark.parametrize("band", fc.BANDS)
def test_every_regime_on_each_foot_with_margin(band):
    """Flat ground and planes alike: every aimed vertex is in its aimed regime, all four regimes occur on each foot, every penetrating
    vertex is a factor two from the fn = 0 threshold and from the friction disc, no vertex is nearer than 10 um to its plane, and all 16
    states are there."""
    S, P = fc.fall_states(band), fc.fall_planes(band)
    o = pc.make_oracle()
    assert S["q"].shape == (fc.B, 30) and P["planes"].shape == (fc.B, 8) and len(S["aimed"]) == fc.B and len(P["aimed"]) == fc.B
    for name, aimed, regimes, planes in (("flat", S["aimed"], S["regimes"], None), ("planes", P["aimed"], P["regimes"], P["planes"])):
        seen = [dict.fromkeys(pc.REGIMES, 0), dict.fromkeys(pc.REGIMES, 0)]
        min_pen, min_fn, min_disc = np.inf, np.inf, np.inf
        for i, (foot, j, want) in enumerate(aimed):
            assert foot == i % 2 and want == pc.REGIMES[(i // 2) % 4] and j // 4 == foot
            pos, vel = pc.vertex_kinematics(o, S["q"][i], S["v"][i])              # (not the cached ones: from the state itself)
            assert np.array_equal(pos, S["pos"][i]) and np.array_equal(vel, S["vel"][i])
            rec = gc.FLAT if planes is None else planes[i]
            got = pc.classify(pos, vel, o.contact()[1]) if planes is None else fc.contact_of(pos, vel, rec)[1]
            assert list(got) == list(regimes[i]) and got[j] == want and "?" not in got, (name, i, j, want, got)
            for n, r in enumerate(got):
                seen[n // 4][r] += 1
            pen, m_fn, m_disc = gc.thresholds(pos, vel, rec)
            min_pen, min_fn, min_disc = min(min_pen, np.abs(pen).min()), min(min_fn, m_fn.min()), min(min_disc, m_disc.min())
        print("\nband %g %s: regimes right %s left %s; min |pen| %.3g m, margins fn %.3f disc %.3f" % (band, name, seen[0], seen[1], min_pen, min_fn, min_disc))
        for foot in range(2):
            assert all(seen[foot][r] > 0 for r in pc.REGIMES), (name, seen)
        assert min_pen >= fc.MIN_PEN, (name, min_pen)
        assert min_fn >= fc.MARGIN - fc.MARGIN_EPS and min_disc >= fc.MARGIN - fc.MARGIN_EPS, (name, min_fn, min_disc)
    normals = P["planes"].reshape(fc.B, 2, 4)[:, :, :3]
    tilt = np.rad2deg(np.arccos(normals[:, :, 2]))
    assert (np.abs((normals ** 2).sum(-1) - 1.0) <= 1e-12).all() and (tilt >= fc.TILT_DEG[0] - 1e-9).all() and (tilt <= fc.TILT_DEG[1] + 1e-9).all()
    print("band %g: attempts per state %s, plane draws %s" % (band, S["attempt"].tolist(), P["attempt"].tolist()))
    # the velocities of a fall, and tau30
    assert np.abs(S["v"][:, 0:3]).max() <= 2.0 and np.abs(S["v"][:, 3:]).max() <= 5.0
    assert np.abs(S["v"][:, 0:3]).max() > 1.5 and np.abs(S["v"][:, 3:6]).max() > 3.0 and np.abs(S["v"][:, 6:]).max() > 4.5
    assert (np.abs(np.cos(S["q"][:, 4])) >= fc.MIN_COS_PITCH).all()


def test_angles_cover_every_quadrant_and_soles_on_edge_and_upside_down():
    q = np.concatenate([fc.fall_states(b)["q"] for b in fc.BANDS])
    n = sincos_quadrants(q)[:, 24:27] & 3
    for k, name in enumerate(("roll", "pitch", "yaw")):
        count = np.bincount(n[:, k], minlength=4)
        print("%s: states per quadrant %s, largest |angle| %.2f rad" % (name, count.tolist(), np.abs(q[:, 3 + k]).max()))
        assert (count > 0).all(), (name, count)
    normals = np.concatenate([fc.fall_states(b)["normals"] for b in fc.BANDS])
    off = np.rad2deg(np.arccos(np.clip(normals[:, :, 2], -1.0, 1.0)))
    print("soles more than 60 degrees off vertical: %d of 64, more than 120: %d" % ((off > 60.0).sum(), (off > 120.0).sum()))
    assert (off > 60.0).sum() >= 4 and (off > 120.0).sum() >= 2


def test_conditioning():
    for band in fc.BANDS:
        S = fc.fall_states(band)
        print("\nband %g: cond(M) %s" % (band, " ".join("%.2e" % c for c in S["cond"])))
        print("band %g: cond(M) min %.2e max %.2e" % (band, S["cond"].min(), S["cond"].max()))
        assert np.isfinite(S["cond"]).all() and (S["cond"] < fc.COND_MAX).all()


# ------------------------------------------------------------------------------- the reference alone
def _solve_longdouble(A, b):
    """Gaussian elimination with partial pivoting in np.longdouble."""
    A, b = np.array(A, dtype=np.longdouble), np.array(b, dtype=np.longdouble)
    n = len(b)
    for c in range(n):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        if p != c:
            A[[c, p]], b[[c, p]] = A[[p, c]], b[[p, c]]
        f = A[c + 1:, c] / A[c, c]
        A[c + 1:] -= f[:, None] * A[c][None, :]
        b[c + 1:] -= f * b[c]
    x = np.zeros(n, dtype=np.longdouble)
    for r in range(n - 1, -1, -1):
        x[r] = (b[r] - A[r, r + 1:] @ x[r + 1:]) / A[r, r]
    return x


def test_the_reference_alone():
    """On the 32 states: the oracle's M, C, J, AG, Jpqp, AGpqp and CoM against oracle/restatement_np.py with the scale rules of
    test_independent_restatement.py (1e-12 there), and np.linalg.solve of the plant's system M a = tau30 + J'w - C against a long-double
    solve of the same doubles on the forward / cond scale.  Measured: terms 2.8e-15 at the worst (J), the solve 7.9e-20 -- every figure
    is below a hundredth of the GPU tolerance for its quantity (1e-11 -> 1e-13; 1e-12 -> 1e-14), which is asserted, so that the GPU
    tolerances stay the project's own."""
    assert np.finfo(np.longdouble).eps < 1e-18
    rb, dyn = R.Robot(), R.Dynamics()
    o = pc.make_oracle()
    worst, solve = {}, 0.0
    for band in fc.BANDS:
        S = fc.fall_states(band)
        for i in range(fc.B):
            q, v = S["q"][i], S["v"][i]
            o.set_prev_velocity(v)
            o.eval(q, v, 0.0)
            t, com = o.terms(), o.robot()["CoM"]
            rb.update_state(q)
            rb.v = v.copy()
            dyn.compute_all(rb)
            J = R.feet_jacobian(rb)
            cs = np.abs(t["C"]).max()
            err = dict(M=np.abs(dyn.M - t["M"]).max() / np.abs(t["M"]).max(), C=np.abs(dyn.C - t["C"]).max() / cs,
                       AG=np.abs(dyn.AG - t["AG"]).max() / np.abs(t["AG"]).max(), J=np.abs(J - t["J"]).max() / np.abs(t["J"]).max(),
                       CoM=np.abs(rb.CoM - com).max() / np.abs(com).max(), AGpqp=np.abs(dyn.AGpqp - t["AGpqp"]).max() / cs,
                       Jpqp=np.abs(dyn.Jpqp - t["Jpqp"]).max() / cs)
            for k, val in err.items():
                worst[k] = max(worst.get(k, 0.0), float(val))
            rhs = S["tau"][i] + t["J"].T @ S["w"][i] - t["C"]
            x64, xld = np.linalg.solve(t["M"], rhs), _solve_longdouble(t["M"], rhs)
            solve = max(solve, float(_ninf(x64 - xld) / (S["cond"][i] * _ninf(xld))))
    print("\noracle vs restatement on the 32 fall states: " + ", ".join("%s %.1e" % kv for kv in sorted(worst.items())))
    print("np.linalg.solve vs long double, forward / cond: %.1e" % solve)
    for k, val in worst.items():
        assert val < 1e-13, (k, val)                               # a hundredth of the 1e-11 the GPU terms are held to
    assert solve < 1e-14, solve                                    # a hundredth of the 1e-12 forward criterion


def test_the_helper_next_to_the_euler_rate_singularity():
    """qdot[3:6] of oracle_plant_xdot on the pitch ladder against E(rpy) w formed in long double from the same doubles: below 1e-14 at
    every rung (measured 2.1e-16 at the worst), so every rung is kept."""
    Ld, o = fc.pitch_ladder(), pc.make_oracle()
    assert len(Ld["q"]) == 10 and sorted(set(Ld["delta"])) == sorted(fc.LADDER_DELTAS)
    ld = np.longdouble
    for n in range(len(Ld["q"])):
        q, v = Ld["q"][n], Ld["v"][n]
        assert abs(abs(q[4]) - (0.5 * np.pi - Ld["delta"][n])) <= 1e-15 and np.sign(q[4]) == Ld["sign"][n]
        xdot, parts = pc.oracle_plant_xdot(o, q, v, Ld["tau"][n])
        pos, _ = pc.vertex_kinematics(o, q, v)
        assert pos[:, 2].min() > 0.04 and not parts["vf"].any()    # every vertex out
        p, y, w = ld(q[4]), ld(q[5]), v[3:6].astype(ld)
        cp, sy, cy, tp = np.cos(p), np.sin(y), np.cos(y), np.tan(p)
        want = np.array([cy / cp * w[0] + sy / cp * w[1], -sy * w[0] + cy * w[1], cy * tp * w[0] + sy * tp * w[1] + w[2]])
        err = float(np.abs(xdot[3:6].astype(ld) - want).max() / np.abs(want).max())
        print("pitch %+.6f (delta %.0e): 1 / cos %.3e, helper vs long double %.2e" % (q[4], Ld["delta"][n], 1.0 / np.cos(q[4]), err))
        assert np.isfinite(xdot).all() and err < 1e-14, (n, err)


# ------------------------------------------------------------------------------- the step references
@pytest.mark.parametrize("band", fc.BANDS)
def test_step_references_keep_their_regimes_under_perturbation(band):
    """The 20-substep references of the step test (velocities x 1/4), flat and planes: the state perturbed by 1e-12 relative, random signs,
    gives the same regime of every vertex at each of the 80 evaluations, on every one of the 16 states; and the flat reference is
    plant_step_cases.oracle_plant_steps' to the bit."""
    S, P, T = fc.fall_states(band), fc.fall_planes(band), fc.step_references(band)
    o = pc.make_oracle()
    assert np.array_equal(T["x0"][:, :30], S["q"]) and np.array_equal(T["x0"][:, 30:], S["v"] * fc.STEP_VSCALE)
    assert np.array_equal(pc.oracle_plant_steps(o, T["x0"][3], T["tau"][3], fc.STEP_N), T["flat"]["x"][3])
    assert np.array_equal(gc.ground_plant_steps(o, T["x0"][3], T["tau"][3], P["planes"][3], fc.STEP_N, pc.DT), T["planes"]["x"][3])
    changes = 0
    for name, planes in (("flat", None), ("planes", P["planes"])):
        for i in range(fc.B):
            sign = np.random.default_rng([fc.FALL_SEED, i, 4]).choice([-1.0, 1.0], 60)
            _, regimes, _, _ = fc.trace(o, T["x0"][i] * (1.0 + 1e-12 * sign), T["tau"][i], None if planes is None else planes[i])
            assert regimes == T[name]["regimes"][i], (name, i)
            changes += sum(a != b for a, b in zip(regimes[1:], regimes[:-1]))
        print("\nband %g %s: least |pen| %.2e m and least threshold margin %.2e over the 16 x 80 evaluations" % (band, name, T[name]["min_pen"], T[name]["min_margin"]))
        assert T[name]["min_pen"] >= fc.TRACE_PEN and T[name]["min_margin"] >= fc.TRACE_MARGIN and np.isfinite(T[name]["x"]).all()
    print("band %g: %d evaluations at which some vertex changed its regime (the references do cross thresholds, between evaluations)" % (band, changes))
