"""CPU tests of the box-constrained MPC's cases, bounds and numpy statement (mpc_box_cases.py, trajectories.lip_box_*, zmp_box): the drawn
cases hold what the kernels can get wrong, the statement stays inside every derived bound while three planted mistakes leave them by
mc.SENSITIVITY, zmp_box follows the plan, the rollout splits bit for bit, and the statement agrees with an independent bounded least-squares
solver.  test_gpu_mpc_box.py holds the kernels to the same cases and bounds."""
import re

import numpy as np
import pytest

import mpc_box_cases as bc
import mpc_cases as mc
from helpers import ROOT, same_bits
from linearmpchumanoid_amd import capi
from linearmpchumanoid_amd import trajectories as tj


@pytest.mark.parametrize("N,mpc_dt", bc.CASES)
def test_the_drawn_cases_hold_every_situation(N, mpc_dt):
    d = bc.draw(N, mpc_dt)
    own, shared = bc.statement(N, mpc_dt), bc.statement(N, mpc_dt, shared=True)
    both = own + shared
    n = N + 1
    assert all(pv["flags"] & ~capi.FLAG_ZMP_RANGE == 0 for pv in both)                      # the statement raises no flag of its own
    assert all(pv["rounds"].max() <= 2 * n for pv in both)
    assert (own[0]["active"] == 0).all() and (own[0]["rounds"] == 0).all()                  # no active bound
    assert max(pv["active"].max() for pv in both) == n                                      # every sample of an axis
    assert any(((pv["side"][ax] > 0).any() and (pv["side"][ax] < 0).any()) for pv in both for ax in range(2))
    assert np.isinf(own[4]["lo"]).any() and np.isinf(own[4]["hi"]).any() and own[4]["flags"] == 0
    assert own[0]["k"] == -3 and own[1]["k"] + N == d["n"] - 1 + mc.PAST_END                 # both clamps
    assert own[0]["flags"] == own[1]["flags"] == capi.FLAG_ZMP_RANGE
    assert any(pv["active"].sum() > 0 for pv in shared) and any(pv["active"].sum() > 0 for pv in own)
    strict = min(bc.strictness(pv, ax) for pv in both for ax in range(2))
    assert strict >= bc.STRICT, strict
    assert d["margins"].min() == 0.0 and d["margins"].max() == 0.023                          # the whole sole ... +-2 mm
    for pv in both:                                                                         # primal and dual feasibility, exactly
        for ax in range(2):
            s, lam, Z = pv["side"][ax], pv["lam"][ax], pv["Z"][ax]
            assert (Z >= pv["lo"][ax]).all() and (Z <= pv["hi"][ax]).all()
            assert (lam[s == 0] == 0).all() and (lam[s > 0] > 0).all() and (lam[s < 0] < 0).all()
            assert (Z[s > 0] == pv["hi"][ax][s > 0]).all() and (Z[s < 0] == pv["lo"][ax][s < 0]).all()


@pytest.mark.parametrize("shared", (False, True))
@pytest.mark.parametrize("N,mpc_dt", bc.CASES)
def test_the_statement_stays_inside_every_bound(N, mpc_dt, shared):
    worst = dict(a=0.0, b=0.0, c=0.0, d=0.0)
    for i, pv in enumerate(bc.statement(N, mpc_dt, shared)):
        for ax in range(2):
            r = bc.check_against_statement(N, mpc_dt, i, ax, pv, pv["U"][ax], pv["lam"][ax], pv["Z"][ax], pv["C"][ax], pv["Cv"][ax], shared)
            worst = {k: max(worst[k], r[k]) for k in worst}
    print(f"\nbox statement N = {N}, mpc_dt = {mpc_dt}, shared = {shared}: " + ", ".join(f"({k}) {v:.3g}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def _wrong_answers(N, mpc_dt, i, ax):
    """Robot i, axis ax (an axis with active bounds): the ratios error / bound of three planted mistakes."""
    pv = bc.statement(N, mpc_dt)[i]
    sy = bc.system(N, mpc_dt, i, ax)
    side = pv["side"][ax]
    _, bu = bc.solution_bounds(sy, side, pv["U"][ax], pv["lam"][ax])
    U_ld, lam_ld, _ = bc.solve_on_set_ld(sy, side)
    out = {}
    released = side.copy()
    released[np.flatnonzero(side)[-1]] = 0                          # one active sample released
    U1, _, _ = bc.solve_on_set_ld(sy, released)
    out["released"] = float(np.abs(U1 - U_ld).max()) / bu
    flipped = pv["lam"][ax].copy()
    j = int(np.argmax(np.abs(flipped)))
    flipped[j] = -flipped[j]                                       # one multiplier's sign flipped
    res, bound_a = bc.stationarity(sy, pv["U"][ax], flipped)
    out["flipped"] = res / bound_a
    late = bc.system(N, mpc_dt, i, ax, box_shift=1)                 # the window of the bounds one sample late
    H64, Pu = np.asarray(late["H"], dtype=np.float64), late["Pu"]
    sol = tj.box_exchange(H64, Pu, np.asarray(late["g"], dtype=np.float64), np.asarray(late["p"], dtype=np.float64), late["lo"], late["hi"])
    out["shifted"] = float(np.abs(sol["U"] - U_ld).max()) / bu
    return out


@pytest.mark.parametrize("N,mpc_dt", ((2, 1e-2), (16, 1e-2), (64, 1e-2)))
def test_three_wrong_answers_lie_outside_the_bounds(N, mpc_dt):
    r = _wrong_answers(N, mpc_dt, 3, 1)                             # robot 3's bounds jump inside its window: a late window reads other bounds
    print(f"\nN = {N}: " + ", ".join(f"{k} {v:.3g} bounds" for k, v in r.items()))
    assert min(r.values()) >= mc.SENSITIVITY, r


def test_zmp_box_follows_the_plan():
    plan = tj.walk_plan(2.6, 1e-2, num_steps=3, time_per_step=0.5, ds_time=0.1)
    xs, mg = 0.04, 0.004
    box = tj.zmp_box(plan, xs, margin=mg)
    wide = tj.zmp_box(plan, xs)
    ph, zx, zy = plan["phase"], plan["zmp_x"], plan["zmp_y"]
    assert box.shape == (4, len(zx)) and (box[0] < box[1]).all() and (box[2] < box[3]).all()
    ss = ph != capi.PHASE_DOUBLE
    assert ss.any() and (~ss).any()
    np.testing.assert_array_equal(wide[:, ss], np.stack([xs * zx - 0.05, xs * zx + 0.1, zy - 0.025, zy + 0.025])[:, ss])    # the stance sole
    np.testing.assert_allclose(box - wide, np.array([mg, -mg, mg, -mg])[:, None] * np.ones_like(box), atol=1e-15)             # the margin
    g = plan["segs"][plan["seg_of_sample"]]
    xr, xl = g[:, 1], g[:, 25]
    ds = ~ss
    np.testing.assert_allclose(wide[:, ds], np.stack([xs * np.minimum(xr, xl) - 0.05, xs * np.maximum(xr, xl) + 0.1,
                                                      np.full(len(zx), -0.075), np.full(len(zx), 0.075)])[:, ds], rtol=0, atol=1e-15)   # the hull
    assert (np.abs(xr - xl)[ds] > 0).any()                          # ... with one foot ahead of the other among them
    twice = tj.zmp_box(plan, 2 * xs)
    np.testing.assert_allclose((twice[1] - twice[0])[ss], (wide[1] - wide[0])[ss], rtol=0, atol=1e-15)   # a sole does not stretch with the step length
    np.testing.assert_allclose((twice[0] + 0.05)[ss], 2 * (wide[0] + 0.05)[ss], atol=1e-15)
    other = tj.zmp_box(plan, xs, fwd=0.08, back=0.03, half_width=0.02)
    np.testing.assert_allclose((other - wide)[:, ss], np.array([0.02, -0.02, 0.005, -0.005])[:, None] * np.ones((4, ss.sum())), atol=1e-15)
    jump = tj.jump_plan(1.0, 1e-2)
    jb = tj.zmp_box(jump)
    fl = jump["phase"] == capi.PHASE_FLIGHT
    assert fl.any() and (jb[0::2, fl] == -np.inf).all() and (jb[1::2, fl] == np.inf).all() and np.isfinite(jb[:, ~fl]).all()
    np.testing.assert_allclose(jb[:, ~fl], np.array([-0.05, 0.1, -0.075, 0.075])[:, None] * np.ones((4, (~fl).sum())), rtol=0, atol=1e-15)
    plans = tj.walk_plans(2.6, 1e-2, dict(num_steps=np.array([2, 3]), time_per_step=np.array([0.4, 0.5])))
    batch = tj.zmp_boxes(plans, np.array([0.03, 0.04]), margin=np.array([0.0, mg]))
    assert batch.shape == (2, 4, len(zx))
    np.testing.assert_array_equal(batch[0], tj.zmp_box({k: v[0] for k, v in plans.items()}, 0.03))
    np.testing.assert_array_equal(batch[1], tj.zmp_box({k: v[1] for k, v in plans.items()}, 0.04, margin=mg))


def test_lip_box_rollout_splits_bit_for_bit_and_is_the_loop_of_steps():
    N, mpc_dt = 16, 1e-2
    d = bc.draw(N, mpc_dt)
    i = 6
    args = (d["plans"]["zmp_x"][i], d["plans"]["zmp_y"][i], d["box"][i])
    kw = dict(N=N, mpc_dt=mpc_dt, z_com=d["zcoms"][i], xscale=d["xs"][i])
    end, tr = tj.lip_box_rollout(*args, d["lip"][i], 9, **kw)
    mid, ta = tj.lip_box_rollout(*args, d["lip"][i], 4, **kw)
    end2, tb = tj.lip_box_rollout(*args, mid, 5, **kw)
    assert same_bits(end, end2) and same_bits(tr, np.concatenate([ta, tb]))
    rec, pv = tj.lip_box_step(*args, d["lip"][i], **kw)
    assert same_bits(rec, tr[0]) and rec[15] == pv["active"].sum() > 0 and rec[2] == pv["U"][0, 0] and rec[7] == pv["Z"][1, 0]
    assert (tr[:, 15] > 0).any() and (tr[:, 14] == 0).all()
    assert same_bits(np.ascontiguousarray(tr[1:, 8]), np.ascontiguousarray(tr[:-1, 0]))      # the state moves on


def test_an_empty_or_nan_box_sample_is_flagged_and_a_capped_solve_too():
    N, mpc_dt = 16, 1e-2
    d = bc.draw(N, mpc_dt)
    i = 5
    k = mc.k_of(d["lip"][i, 4], mpc_dt)
    for bad in ((1, k + 3, -1.0), (2, k + N, np.nan)):
        box = d["box"][i].copy()
        box[bad[0], bad[1]] = bad[2]
        pv = tj.lip_box_preview(d["plans"]["zmp_x"][i], d["plans"]["zmp_y"][i], box, d["lip"][i], N, mpc_dt, d["zcoms"][i], xscale=d["xs"][i])
        assert pv["flags"] == capi.FLAG_BOX_EMPTY | capi.FLAG_NONFINITE and np.isnan(pv["U"]).all() and np.isnan(pv["lam"]).all()
    i = 2
    pv = tj.lip_box_preview(d["plans"]["zmp_x"][i], d["plans"]["zmp_y"][i], d["box"][i], d["lip"][i], N, mpc_dt, d["zcoms"][i], xscale=d["xs"][i],
                            max_rounds=0)
    assert pv["flags"] == capi.FLAG_QP_MAXITER and (pv["rounds"] == 0).all() and (pv["active"] == 0).all()


def test_the_statement_agrees_with_bvls():
    """An independent solver: in Z coordinates the problem is a bounded least-squares problem, min alpha |Pu^-1 (Z - p)|^2 + beta |Z - z|^2
    with lo <= Z <= hi.  1e-7 is BVLS's own tolerance, not ours."""
    scipy_optimize = pytest.importorskip("scipy.optimize")
    worst = 0.0
    for N, mpc_dt in ((2, 1e-2), (16, 1e-2), (64, 1e-2), (16, 1e-3)):
        d = bc.draw(N, mpc_dt)
        for i, pv in enumerate(bc.statement(N, mpc_dt)):
            for ax in range(2):
                sy = bc.system(N, mpc_dt, i, ax)
                Pi = np.linalg.inv(sy["Pu"])
                p = np.asarray(sy["p"], dtype=np.float64)
                z = (d["xs"][i] * d["plans"]["zmp_x"][i], d["plans"]["zmp_y"][i])[ax][np.clip(sy["k"] + np.arange(N + 1), 0, d["n"] - 1)]
                A = np.vstack([np.sqrt(mc.ALPHA) * Pi, np.sqrt(mc.BETA) * np.eye(N + 1)])
                b = np.concatenate([np.sqrt(mc.ALPHA) * Pi @ p, np.sqrt(mc.BETA) * z])
                ref = scipy_optimize.lsq_linear(A, b, bounds=(sy["lo"], sy["hi"]), method="bvls", tol=1e-14, max_iter=2000)
                worst = max(worst, float(np.abs(ref.x - pv["Z"][ax]).max()))
    print(f"\nagainst BVLS: {worst:.3g}")
    assert worst <= 1e-7


def test_prototypes_header_and_constants_agree():
    text = open(ROOT + "/include/lmh.h").read()
    for name, args in (("lmh_mpc_box_preview", 7), ("lmh_mpc_box_step", 7), ("lmh_mpc_box_rollout", 8)):
        assert len(capi.PROTOTYPES[name][1]) == args and name in capi.EXPORTS
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, text).group(1)
        assert len(decl.split(",")) == args
    define = lambda n: int(re.search(r"#define %s\s+(\d+)" % n, text).group(1))
    assert define("LMH_MPC_BOX_STRIDE") == capi.MPC_BOX_STRIDE == capi.MPC_PREVIEW_STRIDE + 2 * capi.MPC_PREVIEW_ARRAY
    assert define("LMH_FLAG_BOX_EMPTY") == capi.FLAG_BOX_EMPTY == 64
    assert define("LMH_MPC_BOX_MAX_ROUNDS") == capi.MPC_BOX_MAX_ROUNDS >= 2 * 65
    assert define("LMH_MPC_OFF_ACTIVE") == capi.MPC_OFF_ACTIVE == 15
    assert [define("LMH_BOX_" + k.upper()) for k in ("lo_x", "hi_x", "lo_y", "hi_y")] == [capi.BOX_ROWS[k] for k in ("lo_x", "hi_x", "lo_y", "hi_y")]
    assert (define("LMH_MPC_BOX_OFF_LAM_X"), define("LMH_MPC_BOX_OFF_LAM_Y")) == (capi.MPC_BOX_ARRAYS["lam_x"][0], capi.MPC_BOX_ARRAYS["lam_y"][0])
    assert [define("LMH_MPC_BOX_OFF_" + k.upper()) for k in capi.MPC_BOX_HEADER] == list(capi.MPC_BOX_HEADER.values())
