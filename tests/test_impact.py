"""CPU tests of the rigid plant's plastic impact: the numpy statement trajectories.rigid_contact_impact (include/lmh.h,
lmh_plant_impact_rigid) on the oracle's terms at the 16 states of plant_step_cases.contact_states() x three support modes, the bindings of
the two entry points, the refusal that needs no device, the Python wrapper's own checks, and the conditions the fixtures of the GPU tests
(impact_cases.py) are there for.  Oracle and numpy only; no GPU is used.

Tolerances are the project's own for the same figures (test_rigid.py): backward error 1e-12 on the scale of its terms, the constraint
residual 1e-12 on the scale |A| |Lam| + |w|, the forward error 1e-12 cond(KKT) against a long-double-refined KKT solve.  Measured on these
cases: constraint 1.6e-17, smallest unpivoted pivot 0.4726, a second impact 2.4e-15 of the first, the kinetic energy falls by 8.0 % or
more, M's asymmetry 1.6e-5 relative, largest |dvhat| 10.4."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import impact_cases as ic
import zoh_rigid_cases as zr
from linearmpchumanoid_amd import capi
from linearmpchumanoid_amd import trajectories as tj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_statement_meets_the_three_bounds_on_every_case():
    S = ic.impact_cases()
    worst = dict(backward=0.0, constraint=0.0, forward=0.0, cond=0.0)
    min_pivot, biggest = np.inf, 0.0
    assert len(S["cases"]) == 48
    for (i, m), c in S["cases"].items():
        b = ic.bounds(S["terms"][i], m, c["dvhat"], c["lam"])
        for k in worst:
            worst[k] = max(worst[k], b[k])
        min_pivot = min(min_pivot, float(c["info"]["pivots"].min()))
        biggest = max(biggest, float(np.abs(c["dvhat"]).max()))
        assert np.isfinite(c["dvhat"]).all() and np.isfinite(c["lam"]).all() and not c["flags"] & (capi.FLAG_NONFINITE | capi.FLAG_NOT_SPD)
        assert b["backward"] <= 1e-12 and b["constraint"] <= 1e-12 and b["forward"] <= 1e-12, ((i, m), b)
        assert (c["info"]["pivots"] > 0.0).all(), (i, m)           # no pivoting is needed
        # v_plus = v + dv, dv the statement's dvhat through the acceleration map
        assert np.array_equal(c["v_plus"], S["v"][i] + c["dv"]) and np.allclose(ic.dvhat_from_dv(c["dv"], S["terms"][i]["X"][0]), c["dvhat"], rtol=1e-12, atol=1e-13)
    print("\nimpact statement, 48 cases: backward %.2e, constraint %.2e, forward/cond %.2e; cond(KKT) <= %.2e, smallest unpivoted pivot %.4g, "
          "largest |dvhat| %.3g" % (worst["backward"], worst["constraint"], worst["forward"], worst["cond"], min_pivot, biggest))


def test_a_second_impact_changes_nothing_and_the_energy_does_not_rise():
    S = ic.impact_cases()
    again, least = 0.0, np.inf
    for (i, m), c in S["cases"].items():
        tm = S["terms"][i]
        vh1 = tm["vhat"] + c["dvhat"]
        d2, lam2, _ = tj.rigid_contact_impact(tm["M"], tm["J"], vh1, m)
        again = max(again, float(np.abs(d2).max() / np.abs(c["dvhat"]).max()))
        assert np.abs(d2).max() <= 1e-12 * np.abs(c["dvhat"]).max(), (i, m)
        e0, e1 = ic.energy(tm, tm["vhat"]), ic.energy(tm, vh1)
        least = min(least, (e0 - e1) / e0)
        assert e1 <= e0, (i, m, e0, e1)
    asym = max(float(np.abs(tm["M"] - tm["M"].T).max() / np.abs(tm["M"]).max()) for tm in S["terms"])
    print("\nimpact statement: a second impact moves v_plus by %.2e of the first; the kinetic energy falls by at least %.1f %%; M's asymmetry %.2e"
          % (again, 100.0 * least, asym))


def test_flight_is_exact_zeros_and_a_free_foot_carries_nothing():
    S = ic.impact_cases()
    for i in range(ic.B):
        tm = S["terms"][i]
        d, lam, flags = tj.rigid_contact_impact(tm["M"], tm["J"], tm["vhat"], capi.PHASE_FLIGHT)
        assert d.shape == (30,) and lam.shape == (12,) and not d.any() and not lam.any() and flags == 0
        assert not S["cases"][(i, capi.PHASE_RIGHT)]["lam"][6:].any() and S["cases"][(i, capi.PHASE_RIGHT)]["lam"][:6].all()       # exactly zero, not small
        assert not S["cases"][(i, capi.PHASE_LEFT)]["lam"][:6].any() and S["cases"][(i, capi.PHASE_LEFT)]["lam"][6:].all()
        d4, lam4, f4 = tj.rigid_contact_impact(tm["M"], tm["J"], tm["vhat"], capi.PHASE_RIGHT + 4)          # only the low two bits are read
        c = S["cases"][(i, capi.PHASE_RIGHT)]
        assert np.array_equal(d4, c["dvhat"]) and np.array_equal(lam4, c["lam"]) and f4 == c["flags"]
        # ALL held soles take part: into double support, both soles rest afterwards
        c0 = S["cases"][(i, capi.PHASE_DOUBLE)]
        assert np.abs(tm["J"] @ (tm["vhat"] + c0["dvhat"])).max() <= 1e-12 * np.abs(tm["J"] @ tm["vhat"]).max()


def test_the_pull_flag_sees_both_outcomes():
    """A condition on the cases, not on the code; and the flags are the statement's sentence, foot by foot."""
    S = ic.impact_cases()
    pull = sum(1 for c in S["cases"].values() if c["flags"] & capi.FLAG_IMPULSE_PULL)
    slip = sum(1 for c in S["cases"].values() if c["flags"] & capi.FLAG_IMPULSE_SLIP)
    print("\nimpact flags over the 48 cases: pull %d, no pull %d, slip %d" % (pull, 48 - pull, slip))
    assert pull >= 1 and 48 - pull >= 1
    for (i, m), c in S["cases"].items():
        held = [ft for ft in range(2) if 6 * ft in c["info"]["rows"]]
        assert bool(c["flags"] & capi.FLAG_IMPULSE_PULL) == any(c["lam"][6 * ft + 5] < 0.0 for ft in held)
        assert bool(c["flags"] & capi.FLAG_IMPULSE_SLIP) == any(np.hypot(*c["lam"][6 * ft + 3:6 * ft + 5]) > ic.MU * c["lam"][6 * ft + 5] for ft in held)
    assert capi.FLAG_IMPULSE_PULL == 1024 and capi.FLAG_IMPULSE_SLIP == 2048 and not (capi.FLAG_IMPULSE_PULL | capi.FLAG_IMPULSE_SLIP) & 15
    assert tj.FLAG_IMPULSE_PULL == 1024 and tj.FLAG_IMPULSE_SLIP == 2048
    assert {"rigid_contact_impact", "FLAG_IMPULSE_PULL", "FLAG_IMPULSE_SLIP"} <= set(tj.__all__)


# ------------------------------------------------------------------------------- header, binding, export
def test_entry_points_are_declared_bound_and_exported(hip_lib):
    from linearmpchumanoid_amd.controller import BatchedController
    raw = open(os.path.join(ROOT, "include", "lmh.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in ("lmh_plant_impact_rigid", "lmh_rollout_zoh_rigid_impact"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src) and name in capi.EXPORTS and hasattr(hip_lib, name), name
    assert capi.PROTOTYPES["lmh_plant_impact_rigid"] == (C.c_int, [C.c_void_p] * 8)
    args = capi.PROTOTYPES["lmh_rollout_zoh_rigid_impact"][1]
    assert len(args) == 11 and args[4:8] == [C.POINTER(capi.LmhZohOpts), C.POINTER(capi.LmhZohIo), C.POINTER(capi.LmhZohRigid), C.POINTER(capi.LmhZohImpact)]
    assert args[8:10] == [C.c_int, C.c_int] and callable(BatchedController.plant_impact_rigid)
    # the record: two pointers and two int32, in the header's order; lmh_zoh_rigid is as it was
    body = re.search(r"typedef struct lmh_zoh_impact \{(.*?)\} lmh_zoh_impact;", src, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*;", body) == [n for n, _ in capi.LmhZohImpact._fields_] == ["d_mode_prev", "d_impulse", "enable", "reserved"]
    assert [t for _, t in capi.LmhZohImpact._fields_] == [C.c_void_p] * 2 + [C.c_int32] * 2 and C.sizeof(capi.LmhZohImpact) == 2 * 8 + 2 * 4
    assert C.sizeof(capi.LmhZohRigid) == 2 * 8 + 8 + 2 * 4
    defs = dict(re.findall(r"#define\s+(LMH_\w+)\s+(\d+)", raw))
    assert (capi.FLAG_IMPULSE_PULL, capi.FLAG_IMPULSE_SLIP) == (int(defs["LMH_FLAG_IMPULSE_PULL"]), int(defs["LMH_FLAG_IMPULSE_SLIP"])) == (1024, 2048)
    # no new launcher symbol: the stand-alone host programs link one stub per launcher
    launch = open(os.path.join(ROOT, "linearmpchumanoid_amd", "csrc", "lmh_launch.h")).read()
    assert len(re.findall(r"void\s+lmh_launch_\w+\s*\(", launch)) == 19 and "PM_RIGID_IMPACT" in launch and "const LmhZohImpact *" in launch
    # the refusals' words are the library's
    lib_src = open(os.path.join(ROOT, "linearmpchumanoid_amd", "csrc", "lmh_capi.hip")).read()
    for words in ("enable must be 0 or 1", "reserved must be 0", "enable = 1 needs a rigid record with a source", "enable = 1 needs d_mode_prev"):
        assert '"lmh_rollout_zoh_rigid_impact: %s' % words in lib_src, words
    for words in ('"null d_q"', '"null d_v"', '"null d_v_plus"'):
        assert words in lib_src, words


def test_without_a_handle_both_calls_are_refused(hip_lib):
    buf = (C.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    p = C.cast(buf, C.c_void_p)
    for args in ((None,) * 6, (p,) * 6):
        assert hip_lib.lmh_plant_impact_rigid(None, *args, None) == -2 and hip_lib.lmh_last_error() == b"null handle"
    for im in (None, C.byref(capi.LmhZohImpact()), C.byref(capi.LmhZohImpact(d_mode_prev=p, d_impulse=p, enable=1)), C.byref(capi.LmhZohImpact(enable=5, reserved=3))):
        for rg in (None, C.byref(capi.LmhZohRigid(kv=float("nan"), source=7, reserved=3)), C.byref(capi.LmhZohRigid(source=1))):
            assert hip_lib.lmh_rollout_zoh_rigid_impact(None, p, p, p, None, None, rg, im, 3, 2, None) == -2 and hip_lib.lmh_last_error() == b"null handle"
    assert list(buf) == [7.0] * 4


def test_the_python_wrapper_checks_before_it_calls():
    import torch
    from linearmpchumanoid_amd.controller import BatchedController
    with pytest.raises(ValueError, match="n_ticks"):
        BatchedController.rollout_zoh_rigid(None, None, -1, 1, impact=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="impulse goes with impact"):
        BatchedController.rollout_zoh_rigid(None, None, 6, 1, impulse=True)
    for bad in (np.zeros(4, dtype=np.int32), torch.zeros(4, dtype=torch.int64), [0, 1, 2, 3], 1):
        with pytest.raises(ValueError, match="impact must be"):
            BatchedController.rollout_zoh_rigid(None, None, 6, 1, impact=bad)


# ------------------------------------------------------------------------------- the fixtures' stated conditions
def test_the_mode_words_of_the_gpu_loop_tests_hold_what_they_are_there_for():
    words, prev = zr.per_tick_modes(), ic.mode_prev_words()
    assert words.shape == (ic.NT, ic.B) and prev.shape == (ic.B,) and prev.dtype == np.int32
    assert ic.loop_condition(words, prev)
    td, last = ic.touchdowns(words, prev)
    assert td.any(axis=0).all() and (~td).any(axis=0).all()        # every robot: a tick with a touchdown and a tick without
    assert set((words & 3).ravel().tolist()) == {0, 1, 2, 3} and set((prev & 3).tolist()) == {0, 1, 2, 3}
    assert (words > 3).any() and (prev > 3).any()                  # junk above the low two bits, which is all the call reads
    assert np.array_equal(last, words[-1] & 3)
    # a split hands on what the first launch leaves
    td2, mid = ic.touchdowns(words[:2], prev)
    td4, _ = ic.touchdowns(words[2:], mid)
    assert np.array_equal(np.concatenate([td2, td4]), td)
    # FIXED: FLIGHT on the even robots makes every held foot a touchdown at tick 0 and nowhere else; the mode itself none at all
    fixed = zr.fixed_modes()
    tdf, _ = ic.touchdowns(np.tile(fixed, (ic.NT, 1)), ic.fixed_prev(fixed))
    assert tdf[0].tolist() == [i % 2 == 0 for i in range(ic.B)] and not tdf[1:].any()
    # by hand
    assert ic.touchdowns(np.array([[0], [1], [2], [3], [1]]), np.array([3]))[0][:, 0].tolist() == [True, False, True, False, True]
    assert ic.touchdowns(np.array([[1 + 8]]), np.array([1 + 4]))[0].tolist() == [[False]]


@pytest.mark.parametrize("n_substeps", [3, 1])
def test_the_plans_of_the_gpu_loop_tests_bring_touchdowns(n_substeps):
    """On the per-robot plans (walks and jumps) and on the shared walking plan, with impact_cases' d_mode_prev words, a touchdown occurs on
    the first tick (against d_mode_prev) and on a later one (a phase boundary of the plan), and ticks without one occur."""
    for phase in (zr.plans()["phase"], tj.walk_plan(zr.SIM_TIME, zr.DT)["phase"]):
        t0 = zr.start_clocks(phase, n_substeps)
        modes = zr.plan_modes(phase, zr.preview_indices(t0, ic.NT, n_substeps))
        td, last = ic.touchdowns(modes, ic.mode_prev_words())
        print("\ntouchdowns per tick on the plans, n_substeps %d: %s" % (n_substeps, td.sum(axis=1).tolist()), end="")
        assert td[0].any() and td[1:].any() and (~td).any() and np.array_equal(last, modes[-1] & 3)


def test_the_touchdown_of_the_cpu_closed_loop_moves_the_state():
    """The parity test's bound on the state is 1e-7: the impact of its touchdown has to change some velocity component by more than 1e-3 of
    the largest |v|, or a dropped impact could pass.  Both loops on the CPU: with the impact and without."""
    P = ic.parity_inputs()
    assert P["modes"].shape == (12, 4) and set(P["modes"][:6].ravel()) == {1} and set(P["modes"][6:].ravel()) == {0} and np.array_equal(P["prev"], P["modes"][0])
    assert (np.abs(P["v"]).max(axis=1) > 0.0).all()                # no robot starts from rest
    withi, without = ic.cpu_loop(True), ic.cpu_loop(False)
    for i, (a, b) in enumerate(zip(withi, without)):
        td = np.abs(a["impulse"]).max(axis=1) > 0.0
        assert td.tolist() == [j == ic.PARITY["touchdown"] for j in range(12)], (i, td)
        assert a["jump"] > 1e-3, (i, a["jump"])
        gap = np.abs(a["x"] - b["x"]).max() / np.abs(a["x"]).max()
        print("\ncpu loop, robot %d: the touchdown changes a velocity by %.3g of the largest |v|; the final states with and without it differ by %.3g relative"
              % (i, a["jump"], gap), end="")
        assert gap > 1e-5 and np.isfinite(a["x"]).all() and not a["flags"] & capi.FLAG_NONFINITE
    print()
