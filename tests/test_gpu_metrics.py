"""Rollout metrics (lmh_rollout_metrics): a 208-word record per robot -- tick count, first flag, first fall, extrema of the state and
the contact wrench, peak torque, the effort and tracking-error sums -- accumulated on chip during a launch.  The record is defined as a
fold of the every-tick trace, so the reference of every test is a second handle run with rollout_trace(.., every = 1) (pinned by
tests/test_gpu_trace.py) and folded on the host by linearmpchumanoid_amd.metrics.fold_trace (tests/metrics_cases.py).  "Equal" means
equal as bytes, all 208 words of every robot, except that a NaN reference word asks for a NaN."""
import os

import numpy as np
import pytest
import torch

from helpers import run_probe, same_bits
from linearmpchumanoid_amd import metrics as hm
from metrics_cases import (FLAG_MORE, FOLD_CASES, M_B, M_NT, POISON_FOLD_CASES, first_flag_case, fold_against_trace, measured,
                           reference_trace, words_differ)
from push_cases import bits_differ, walking_controller
from trace_cases import untraced

pytestmark = pytest.mark.gpu

_CHILD = r"""
import json, os, sys
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
from linearmpchumanoid_amd import capi
from metrics_cases import POISON_FOLD_CASES, first_flag_case, fold_against_trace
res = {"build_flags": capi.lib().lmh_debug_build_flags(), "fold": [fold_against_trace(*c) for c in POISON_FOLD_CASES], "flag": first_flag_case()}
print(json.dumps(res))
"""
# per-robot parameter sets of the PARAMS case (cycled over the robots): friction, joint gains and a force weight around the defaults
PARAM_SETS = [dict(), dict(mu=0.5), dict(kp_joints=350.0, kd_joints=36.0), dict(mu=0.55, w_force=2.0)]


def check_fold_result(res, precision, plant):
    print("metrics against the folded trace:", precision, plant, res)
    assert res["count"] == [M_NT, M_NT]
    assert res["finite"]                                            # numbers are compared, not NaNs
    assert res["joints_moving"] == res["joints"] and res["effort_positive"]     # ... of robots that move and push
    assert res["diff"] == [], res                                   # (robot, word) of the first differing words
    assert res["final_diff"] == [], res                             # the launch leaves what lmh_rollout leaves


def check_flag_result(res):
    print("first flag:", res)
    ff = res["first_flag"]
    assert res["finite"] and res["flags"] == [0, 4]                 # LMH_FLAG_ZMP_RANGE and nothing else; the run goes on
    # the reference itself: a robot flagged at its first tick, one inside the first chunk, one beyond tick 250, one never
    assert 0 in ff and any(0 < v < 250 for v in ff) and any(v > 250 for v in ff) and -1 in ff
    assert res["diff"] == [], res
    # the following launch's cumulative flags start again from 0: what was set stays, what was not is counted from the reset
    again = res["first_flag_again"]
    assert all(a == f for a, f in zip(again, ff) if f >= 0)
    assert any(f < 0 and M_NT <= a < M_NT + FLAG_MORE for a, f in zip(again, ff))
    assert res["diff_again"] == [], res


@pytest.fixture(scope="module")
def walking():
    """16 robots of the walking plan, fp64, no pushes: the every-tick reference trace of 520 ticks and its start posture"""
    ctl, q0 = walking_controller(B=M_B)
    trace = reference_trace(ctl, q0, M_NT)
    ctl.close()
    assert np.isfinite(trace).all()
    return dict(trace=trace, q0=q0)


@pytest.fixture(scope="module")
def poison_results():
    """Cases 1 (fp64, both plants) and 3 on the checker build that fills each robot's LDS with NaNs first, in ONE fresh child process."""
    from linearmpchumanoid_amd import build as hipbuild
    assert os.path.exists(hipbuild.build_variant("poison", ["-DLMH_POISON"]))
    res = run_probe(_CHILD, "poison", timeout=900)
    assert res["build_flags"] & 1 == 1, res["build_flags"]
    return res


# ------------------------------------------------------------------------------- 1. the record = the folded every-tick trace
@pytest.mark.parametrize("precision,plant,pushes", FOLD_CASES)
def test_record_equals_the_folded_trace(precision, plant, pushes):
    """fp64 on the walking plan with pushes at ticks 0, 6, 7, 8, 249, 250, 251 (trace_cases.push_schedule), fp64 with the plant on the
    standing robots, mixed and fp32 without the plant; 520 ticks = two chunks and a tail.  All 208 words of every robot; the final
    state / out / status / log equal a plain rollout's as bytes; the compared run is finite, every joint moved, every torque acted."""
    check_fold_result(fold_against_trace(precision, plant, pushes), precision, plant)


@pytest.mark.parametrize("precision,plant,pushes", POISON_FOLD_CASES)
def test_record_equals_the_folded_trace_on_the_poisoned_lds_build(poison_results, precision, plant, pushes):
    """no word of a record comes from LDS that nobody wrote"""
    check_fold_result(poison_results["fold"][POISON_FOLD_CASES.index((precision, plant, pushes))], precision, plant)


# ------------------------------------------------------------------------------- 2. composition
def test_two_launches_on_one_record_are_the_launch_of_the_whole(walking):
    """280 + 240 ticks on one record = 520 in one launch, as bytes (and both the folded trace); a reset between two launches leaves
    the second launch's own record."""
    ctl, q0 = walking_controller(B=M_B)
    whole = measured(ctl, q0, [M_NT])
    parts = measured(ctl, q0, [280, 240])
    assert same_bits(parts["metrics"], whole["metrics"]) and same_bits(parts["state"], whole["state"]) and same_bits(parts["out"], whole["out"])
    assert words_differ(whole["metrics"], hm.fold_trace(hm.identity(M_B), walking["trace"])) == []
    # reset between: launch 280, reset, launch 240 on the same state
    st, m = ctl.new_state(q0, np.zeros(30), t=0.0), ctl.new_metrics()
    out, status = ctl.new_out(), ctl.new_status()
    ctl.rollout_metrics(st, 280, m, out, status)
    first = m.cpu().numpy()
    ctl.metrics_reset(m)
    ctl.rollout_metrics(st, 240, m, out, status)
    torch.cuda.synchronize()
    second = m.cpu().numpy()
    ctl.close()
    assert words_differ(first, hm.fold_trace(hm.identity(M_B), walking["trace"][:280])) == []
    assert words_differ(second, hm.fold_trace(hm.identity(M_B), walking["trace"][280:])) == []
    assert not same_bits(second, whole["metrics"]) and (second[:, 0] == 240).all()


# ------------------------------------------------------------------------------- 3. first flag
def test_first_flag_is_the_tick_the_flag_was_raised():
    """Standing robots whose preview window leaves 1 s of stance references at t ~ 1.18 s (LMH_FLAG_ZMP_RANGE, clamped, the run goes on),
    start clocks 1.18 - 0.05 j: the reference trace has a robot flagged at tick 0, robots inside the first chunk and beyond tick 250 and
    robots never flagged.  FIRST_FLAG stays under a following launch, whose own cumulative flags start again from 0."""
    check_flag_result(first_flag_case())


def test_first_flag_on_the_poisoned_lds_build(poison_results):
    check_flag_result(poison_results["flag"])


# ------------------------------------------------------------------------------- 4. first fall, by construction
def _record_setting(series, seed, rising):
    """ticks at which `series` sets a strict new extreme (running extreme seeded with `seed`) with a threshold half-way to the previous
    extreme that separates the two as doubles -> (ticks, thresholds)"""
    s = -series if rising else series
    prev = np.minimum.accumulate(np.concatenate([[-seed if rising else seed], s]))[:-1]
    thr = 0.5 * (s + prev)
    ok = (s < thr) & (thr <= prev)
    return np.flatnonzero(ok), (-thr if rising else thr)[ok]


def test_first_fall_is_the_first_crossing_of_the_thresholds(walking):
    """Thresholds built from the reference trace so that the first crossing is a known tick: robot i's Z_MIN half-way between a strict
    new minimum of its base height at tick tau_i and the running minimum before it (the tau nearest to 0, 249, 250, 251 and 519 over the
    robots), one robot the same on |pitch| with TILT_MAX, the others left at -inf / inf."""
    trace, q0 = walking["trace"], walking["q0"]
    z_min, tilt_max, want = np.full(M_B, -np.inf), np.full(M_B, np.inf), np.full(M_B, -1, dtype=np.int64)
    free = list(range(M_B))
    for target in (0, 249, 250, 251, 519):
        best = None
        for i in free:
            ticks, thr = _record_setting(trace[:, i, 2], q0[2], rising=False)
            if ticks.size:
                j = int(np.argmin(np.abs(ticks - target)))
                if best is None or abs(ticks[j] - target) < abs(best[1] - target):
                    best = (i, int(ticks[j]), float(thr[j]))
        assert best is not None
        free.remove(best[0])
        z_min[best[0]], want[best[0]] = best[2], best[1]
    tilt_robot = free.pop(0)
    ticks, thr = _record_setting(np.abs(trace[:, tilt_robot, 4]), abs(q0[4]), rising=True)
    j = int(np.argmin(np.abs(ticks - 250)))
    tilt_max[tilt_robot], want[tilt_robot] = thr[j], ticks[j]
    print("first fall by construction: ticks", want.tolist())
    ref = hm.fold_trace(hm.identity(M_B, z_min, tilt_max), trace)
    # the reference holds what the construction says, in every chunk, and the robots without a threshold never fall
    assert ref[:, 2].astype(np.int64).tolist() == want.tolist()
    assert any(0 <= t < 250 for t in want) and any(250 <= t < 500 for t in want) and any(500 <= t < M_NT for t in want)
    assert len(free) >= 4 and (want[free] == -1).all()
    ctl, q0_ = walking_controller(B=M_B)
    got = measured(ctl, q0_, [M_NT], z_min=z_min, tilt_max=tilt_max)
    ctl.close()
    assert words_differ(got["metrics"], ref) == []
    assert got["metrics"][:, 3].tolist() == z_min.tolist() and got["metrics"][:, 4].tolist() == tilt_max.tolist()    # the thresholds are read, never written


# ------------------------------------------------------------------------------- 5. real fallers
def test_robots_that_really_fall():
    """16 robots of the walking plan on the compliant-contact plant over 1000 ticks: they fall from about tick 640 on and end non-finite
    (push_cases.scenario_controller).  Thresholds 0.8 x the initial base height and 0.5 rad; the record against the folded trace under
    the NaN rule; the reference has fallers."""
    nt = 1000
    ref_ctl, q0 = walking_controller(B=M_B, plant=1)
    trace = reference_trace(ref_ctl, q0, nt)
    ref_ctl.close()
    z_min, tilt_max = 0.8 * q0[2], 0.5
    ref = hm.fold_trace(hm.identity(M_B, z_min, tilt_max), trace)
    falls = ref[:, 2].astype(np.int64)
    print("real fallers: first fall", falls.tolist(), "non-finite robots", int((~np.isfinite(trace[-1, :, :60]).all(axis=1)).sum()))
    assert (falls >= 0).any() and (falls[falls >= 0] > 0).all()      # somebody falls, nobody starts down
    ctl, _ = walking_controller(B=M_B, plant=1)
    got = measured(ctl, q0, [nt], z_min=z_min, tilt_max=tilt_max)
    plain = untraced(ctl, q0, nt)
    ctl.close()
    assert words_differ(got["metrics"], ref) == []
    assert all(same_bits(got[k], plain[k]) for k in ("state", "out", "status", "log"))
    s = hm.summarise(got["metrics"], 1e-3)
    assert np.array_equal(s["t_first_fall"][falls >= 0], (falls[falls >= 0] + 1) * 1e-3) and np.isnan(s["t_first_fall"][falls < 0]).all()


# ------------------------------------------------------------------------------- 6. per-robot parameters
def test_record_on_a_handle_with_per_robot_parameters():
    """the walking robots with four parameter sets cycled over them (lmh_set_params): the PARAMS instantiation of the kernel"""
    ctl, _ = walking_controller(B=M_B)
    from params_cases import columns
    cols = columns([PARAM_SETS[i % len(PARAM_SETS)] for i in range(M_B)], ctl.cfg)
    ctl.close()
    res = fold_against_trace(0, 0, False, params=cols)
    print("metrics with per-robot parameters:", res)
    assert res["per_robot"] == 1 and res["count"] == [M_NT, M_NT]
    assert res["finite"] and res["joints_moving"] == res["joints"] and res["effort_positive"]
    assert res["diff"] == [] and res["final_diff"] == [], res


# ------------------------------------------------------------------------------- 7. arguments
def test_refused_arguments_take_no_launch_slot_and_zero_ticks_write_nothing():
    from linearmpchumanoid_amd import capi
    L, vp = capi.lib(), capi.C.c_void_p
    ctl, q0 = walking_controller(B=M_B)
    st, out, status = ctl.new_state(q0, np.zeros(30), t=0.0), ctl.new_out(), ctl.new_status()
    before = st.cpu().numpy().copy()
    rec = torch.full((M_B, capi.METRICS_STRIDE), float("nan"), dtype=torch.float64, device=ctl.device)

    def call(m, nt):
        return L.lmh_rollout_metrics(ctl._h, vp(st.data_ptr()), vp(out.data_ptr()), vp(status.data_ptr()), None, nt,
                                     None if m is None else vp(m.data_ptr()), ctl._stream())

    assert call(None, 20) == -2 and "lmh_rollout_metrics" in L.lmh_last_error().decode()      # LMH_ERR_BAD_ARG
    assert call(rec, -1) == -2
    assert call(rec, 0) == 0                                        # nothing enqueued, the record's bytes left alone
    torch.cuda.synchronize()
    assert same_bits(st.cpu().numpy(), before) and torch.isnan(rec).all()
    for z, a in ((float("nan"), 0.5), (0.2, float("nan"))):
        assert L.lmh_metrics_reset(ctl._h, vp(rec.data_ptr()), z, a, ctl._stream()) == -2 and "NaN" in L.lmh_last_error().decode()
    assert L.lmh_metrics_reset(ctl._h, None, 0.2, 0.5, ctl._stream()) == -2
    with pytest.raises(ValueError):
        ctl.new_metrics(z_min=float("nan"))
    torch.cuda.synchronize()
    assert torch.isnan(rec).all()
    assert same_bits(ctl.new_metrics(0.2, 0.5).cpu().numpy(), hm.identity(M_B, 0.2, 0.5))      # the reset writes the identity record
    zs = np.linspace(0.1, 0.25, M_B)
    assert same_bits(ctl.new_metrics(zs, np.inf).cpu().numpy(), hm.identity(M_B, zs, np.inf))
    # the refusals took no launch slot: the next plain rollout on this handle is the one a fresh handle runs
    a = untraced(ctl, q0, 300)
    fresh, _ = walking_controller(B=M_B)
    b = untraced(fresh, q0, 300)
    ctl.close(); fresh.close()
    assert np.isfinite(a["log"]).all() and bits_differ(a, b) == []


def test_two_metric_launches_in_flight_on_two_streams():
    """Two launches of one handle in flight on two streams, each with state, records and a metrics record of its own, equal their solo runs."""
    ctl, q0 = walking_controller(B=M_B)
    lengths = (M_NT, 300)
    solo = [measured(ctl, q0, [nt]) for nt in lengths]
    streams = [torch.cuda.Stream(device=ctl.device) for _ in range(2)]
    torch.cuda.synchronize()
    runs = []
    for s, nt in zip(streams, lengths):
        st, m = ctl.new_state(q0, np.zeros(30), t=0.0), ctl.new_metrics()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            runs.append((st, m) + ctl.rollout_metrics(st, nt, m, log=True))
    torch.cuda.synchronize()
    ctl.close()
    for (st, m, out, status, lg), ref in zip(runs, solo):
        assert same_bits(m.cpu().numpy(), ref["metrics"]) and np.isfinite(ref["metrics"][:, 5:]).all()
        assert same_bits(st.cpu().numpy(), ref["state"]) and same_bits(out.cpu().numpy(), ref["out"])
        assert same_bits(status.cpu().numpy(), ref["status"]) and same_bits(lg.cpu().numpy(), ref["log"])
    assert not same_bits(solo[0]["metrics"], solo[1]["metrics"])
