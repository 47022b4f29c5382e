"""The scenarios of the rollout-metrics tests (tests/test_gpu_metrics.py), importable by the test process and by the child process that
runs the NaN-filled-LDS checker build.

The record of lmh_rollout_metrics is DEFINED as a fold of the every-tick trace (include/lmh.h), so the reference of every case is a
second handle of the same set-up run with rollout_trace(.., every = 1) -- a path tests/test_gpu_trace.py pins against split launches and
the oracle -- folded on the host by linearmpchumanoid_amd.metrics.fold_trace.  "Equal" is equal as bytes wherever the reference word is
finite or +-inf; where the reference word is a NaN the device word must be a NaN too.
Shapes: 16 robots of the mixed per-robot walking plan over 520 ticks (two full 250-tick chunks and a tail), as in trace_cases; with the
plant, push_cases.scenario_controller's standing robots.
"""
import numpy as np
import torch

from helpers import same_bits
from plan_draw import DT, MPC_DT, N_PREVIEW
from push_cases import ik_posture, scenario_controller, walking_controller
from trace_cases import TRACE_B, TRACE_NT, push_schedule, traced, untraced

M_B, M_NT = TRACE_B, TRACE_NT
# (precision, plant, pushes): fp64 on the walking plan with trace_cases.push_schedule (pushes at ticks 0, 6, 7, 8, 249, 250, 251), fp64 with
# the plant on the standing robots, mixed and fp32 without the plant
FOLD_CASES = [(0, 0, True), (0, 1, False), (1, 0, False), (2, 0, False)]
POISON_FOLD_CASES = [c for c in FOLD_CASES if c[0] == 0]
FLAG_MORE = 60                           # ticks of the first-flag scenario's second launch
FLAG_T0, FLAG_STEP = 1.18, 0.05          # first-flag scenario: LMH_FLAG_ZMP_RANGE from t ~ 1.18 s on; robot j starts FLAG_STEP * j earlier


def case_controller(precision, plant, pushes=False):
    ctl, q0 = scenario_controller(1, precision=precision) if plant else walking_controller(B=M_B, precision=precision)
    if pushes:
        ctl.set_pushes(*push_schedule(ctl.B))
    return ctl, q0


def flag_controller(B=M_B):
    """Standing robots on 1 s of stance references (mpc_dt = 10 ms, N = 32): the preview window leaves the reference arrays at
    t ~ FLAG_T0, LMH_FLAG_ZMP_RANGE is raised from then on, the window is clamped and the run goes on.  Start clocks per robot."""
    from linearmpchumanoid_amd.controller import BatchedController, default_config
    q0, zcom = ik_posture()
    ctl = BatchedController(B, default_config(dt=DT, time_horizon=N_PREVIEW * MPC_DT + 1e-9, z_com=zcom, mpc_dt=MPC_DT, warm_start=1))
    ctl.set_refs_stance(1.0, 2)
    return ctl, q0, FLAG_T0 - FLAG_STEP * np.arange(B)


def words_differ(got, ref):
    """[(robot, word), ..] where two metrics records [B,208] are not equal under the rule above"""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    nan = np.isnan(ref)
    bad = np.where(nan, ~np.isnan(got), got.view(np.uint64) != ref.view(np.uint64))
    return [tuple(int(v) for v in iw) for iw in np.argwhere(bad)]


def measured(ctl, q0, launches, z_min=-np.inf, tilt_max=np.inf, t=0.0, metrics=None, log=True):
    """rollout_metrics launches of the given lengths, one after the other on one state and one record (a fresh one unless given).
    -> dict(state, out, status, log (of the last launch), metrics (host [B,208]), record (the device tensor))"""
    st = ctl.new_state(q0, np.zeros(30), t=t)
    m = ctl.new_metrics(z_min, tilt_max) if metrics is None else metrics
    out, status = ctl.new_out(), ctl.new_status()
    lg = None
    for nt in launches:
        _, _, lg = ctl.rollout_metrics(st, nt, m, out, status, log=log)
        torch.cuda.synchronize()
    return dict(state=st.cpu().numpy(), out=out.cpu().numpy(), status=status.cpu().numpy(), log=None if lg is None else lg.cpu().numpy(),
                metrics=m.cpu().numpy(), record=m)


def reference_trace(ctl, q0, nt, t=0.0):
    """the every-tick trace [nt, B, 180] of one launch from the start posture (start clocks t, a scalar or one per robot)"""
    state = ctl.new_state(q0, np.zeros(30), t=t).cpu().numpy()
    return traced(ctl, q0, nt, 1, state=state, log=False)["trace"]


def fold_against_trace(precision, plant, pushes, params=None):
    """One case of FOLD_CASES -> dict of the comparisons and of what makes them meaningful (JSON-serialisable).  params: set_params
    keyword arguments for both handles (the PARAMS instantiation)."""
    from linearmpchumanoid_amd import metrics as hm
    ctl, q0 = case_controller(precision, plant, pushes)
    if params:
        ctl.set_params(**params)
    got = measured(ctl, q0, [M_NT])
    plain = untraced(ctl, q0, M_NT)
    per_robot = int(ctl.params_per_instance())
    B = ctl.B
    ctl.close()
    ref_ctl, _ = case_controller(precision, plant, pushes)
    if params:
        ref_ctl.set_params(**params)
    trace = reference_trace(ref_ctl, q0, M_NT)
    ref_ctl.close()
    ref = hm.fold_trace(hm.identity(B), trace)
    f = _fields(ref)
    return dict(diff=words_differ(got["metrics"], ref)[:8], final_diff=[k for k in ("state", "out", "status", "log") if not same_bits(got[k], plain[k])],
                finite=bool(np.isfinite(trace).all() and np.isfinite(got["log"]).all() and np.isfinite(got["metrics"][:, 5:]).all()),
                joints_moving=int((f["xmax"][:, 6:30] > f["xmin"][:, 6:30]).sum()), joints=int(B * 24),
                effort_positive=bool((f["tau_sq"] > 0).all()), count=[int(got["metrics"][:, 0].min()), int(got["metrics"][:, 0].max())],
                robots=B, per_robot=per_robot, trace_flags=int(np.bitwise_or.reduce(trace[:, :, 178].astype(np.int64).ravel())))


def _fields(rec):
    from linearmpchumanoid_amd.controller import BatchedController
    return BatchedController.split_metrics(rec)


def first_flag_case():
    """Test 3's scenario -> dict: the record against the folded reference trace, the reference's own first-flag ticks, and FIRST_FLAG after
    FLAG_MORE more ticks in a second launch (whose cumulative flags start again from 0)."""
    from linearmpchumanoid_amd import metrics as hm
    ctl, q0, t0 = flag_controller()
    st = ctl.new_state(q0, np.zeros(30), t=t0)
    m = ctl.new_metrics()
    ctl.rollout_metrics(st, M_NT, m)
    torch.cuda.synchronize()
    got = m.cpu().numpy()
    ctl.rollout_metrics(st, FLAG_MORE, m)                             # the following launch goes on from where the first ended, on the same record
    torch.cuda.synchronize()
    again = m.cpu().numpy()
    ctl.close()
    ref_ctl, _, _ = flag_controller()
    first = traced(ref_ctl, q0, M_NT, 1, state=ref_ctl.new_state(q0, np.zeros(30), t=t0).cpu().numpy(), log=False)
    second = traced(ref_ctl, q0, FLAG_MORE, 1, state=first["state"], log=False)
    ref_ctl.close()
    ref = hm.fold_trace(hm.identity(M_B), first["trace"])
    ref2 = hm.fold_trace(ref, second["trace"])
    return dict(diff=words_differ(got, ref)[:8], diff_again=words_differ(again, ref2)[:8],
                first_flag=[int(v) for v in ref[:, 1]], first_flag_again=[int(v) for v in ref2[:, 1]],
                second_launch_first_flags=[int(v) for v in second["trace"][0, :, 178]],
                flags=sorted({int(v) for v in first["trace"][:, :, 178].ravel()}), finite=bool(np.isfinite(first["trace"]).all()))
