"""CPU side of lmh_rollout_zoh_rigid: the binding against the header, the refusal that needs no device, the Python wrapper's own checks, and
that the fixtures the GPU tests run (zoh_rigid_cases.py) hold what they are there for -- the per-tick mode words of test 3, the plans and
start clocks of test 4 -- with trajectories.rigid_modes held to the CPU oracle's own phase at k on those plans.  No GPU is used."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import plant_step_cases as pc
import zoh_rigid_cases as zr
from linearmpchumanoid_amd import trajectories as tj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_bound_and_exported(hip_lib):
    from linearmpchumanoid_amd import capi
    from linearmpchumanoid_amd.controller import BatchedController
    raw = open(os.path.join(ROOT, "include", "lmh.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\bint\s+lmh_rollout_zoh_rigid\s*\(", src) and "lmh_rollout_zoh_rigid" in capi.EXPORTS and hasattr(hip_lib, "lmh_rollout_zoh_rigid")
    args = capi.PROTOTYPES["lmh_rollout_zoh_rigid"][1]
    assert len(args) == 10 and args[4] == C.POINTER(capi.LmhZohOpts) and args[5] == C.POINTER(capi.LmhZohIo) and args[6] == C.POINTER(capi.LmhZohRigid)
    assert args[7:9] == [C.c_int, C.c_int] and callable(BatchedController.rollout_zoh_rigid)
    # the record: two pointers, a double, two int32, in the header's order
    body = re.search(r"typedef struct lmh_zoh_rigid \{(.*?)\} lmh_zoh_rigid;", src, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*;", body) == [n for n, _ in capi.LmhZohRigid._fields_] and C.sizeof(capi.LmhZohRigid) == 2 * 8 + 8 + 2 * 4
    assert [t for _, t in capi.LmhZohRigid._fields_] == [C.c_void_p] * 2 + [C.c_double] + [C.c_int32] * 2
    defs = dict(re.findall(r"#define\s+(LMH_\w+)\s+(\d+)", raw))
    assert (capi.RIGID_FIXED, capi.RIGID_PER_TICK, capi.RIGID_PLAN) == tuple(int(defs[k]) for k in ("LMH_RIGID_FIXED", "LMH_RIGID_PER_TICK", "LMH_RIGID_PLAN")) == (1, 2, 3)
    # what the header must state plainly
    text = re.sub(r"\s*\n \*\s*", " ", raw)
    for words in ("NO IMPACT MODEL", "e^(-kv t)", "BILATERAL", "trajectories.rigid_modes(phase, k) and nothing else"):
        assert words in text, words
    # the launcher is declared once and carries the new call (no new symbol: the stand-alone host programs link against one stub per launcher)
    launch = open(os.path.join(ROOT, "linearmpchumanoid_amd", "csrc", "lmh_launch.h")).read()
    decl = re.findall(r"void\s+lmh_launch_rollout_zoh\s*\(([^;]*)\)\s*;", launch)
    assert len(decl) == 1 and "const LmhZohRigid *" in decl[0] and len(re.findall(r"void\s+lmh_launch_\w+\s*\(", launch)) == 19
    # the refusals' words are the library's
    lib_src = open(os.path.join(ROOT, "linearmpchumanoid_amd", "csrc", "lmh_capi.hip")).read()
    for words in ("source must be 0, LMH_RIGID_FIXED, LMH_RIGID_PER_TICK or LMH_RIGID_PLAN", "reserved must be 0", "kv must be finite and >= 0",
                  "source LMH_RIGID_PER_TICK needs d_mode", "d_mode must be NULL with source LMH_RIGID_PLAN"):
        assert '"lmh_rollout_zoh_rigid: %s' % words in lib_src, words


def test_without_a_handle_the_call_is_refused(hip_lib):
    from linearmpchumanoid_amd import capi
    for rg in (None, C.byref(capi.LmhZohRigid()), C.byref(capi.LmhZohRigid(kv=float("nan"), source=7, reserved=3))):
        for io in (None, C.byref(capi.LmhZohIo(actuators=1))):
            assert hip_lib.lmh_rollout_zoh_rigid(None, None, None, None, None, io, rg, 3, 2, None) == -2 and hip_lib.lmh_last_error() == b"null handle"


def test_the_python_wrapper_checks_before_it_calls():
    from linearmpchumanoid_amd.controller import BatchedController
    with pytest.raises(ValueError, match="n_ticks"):
        BatchedController.rollout_zoh_rigid(None, None, -1, 1)
    with pytest.raises(ValueError, match='"plan"'):
        BatchedController.rollout_zoh_rigid(None, None, 6, 1, mode="walk")


def test_the_host_loop_shares_the_familys_helpers():
    import zoh_host_loop as zh
    import zoh_rigid_host_loop as zrh
    assert all(getattr(zrh, n) is getattr(zh, n) for n in ("fresh", "push_schedules", "wrench_and_refs", "assert_same", "actuate")) and callable(zrh.host_loop_rigid)


def test_the_per_tick_words_change_every_robot_twice_and_hold_all_four_modes():
    words = zr.per_tick_modes()
    changes, values = zr.mode_changes(words)
    assert words.shape == (zr.NT, zr.B) and words.dtype == np.int32
    assert (changes >= 2).all() and values == {tj.PHASE_DOUBLE, tj.PHASE_RIGHT, tj.PHASE_LEFT, tj.PHASE_FLIGHT}
    assert (words > 3).any() and (words >= 0).all()                # junk above the low two bits, which is all the call reads
    assert np.array_equal(zr.per_tick_modes(2), words[:2]) and np.array_equal(zr.per_tick_modes(4), words[:4])       # a split slices them
    fixed = zr.fixed_modes()
    assert fixed.dtype == np.int32 and fixed.tolist() == [i % 3 for i in range(zr.B)]


@pytest.mark.parametrize("n_substeps", [3, 1])
def test_the_plans_and_start_clocks_cross_phase_boundaries_inside_six_ticks(n_substeps):
    plans = zr.plans()
    assert plans["phase"].shape == (zr.B, int((zr.SIM_TIME + 0.5) / zr.DT)) and plans["phase"].dtype == np.uint8
    walk = tj.walk_plans(zr.SIM_TIME, zr.DT, zr.walk_specs(), zr.B)
    for i in range(zr.B):
        if i in zr.JUMP_ROBOTS:
            assert set(plans["phase"][i].tolist()) == {tj.PHASE_DOUBLE, tj.PHASE_FLIGHT}
        else:
            assert np.array_equal(plans["phase"][i], walk["phase"][i]) and set(plans["phase"][i].tolist()) == {tj.PHASE_DOUBLE, tj.PHASE_RIGHT, tj.PHASE_LEFT}
    t0 = zr.start_clocks(plans["phase"], n_substeps)
    assert (t0 >= 0.0).all() and all(t0[i] == 0.0 for i in zr.STILL_ROBOTS)
    ks = zr.preview_indices(t0, zr.NT, n_substeps)
    assert (np.diff(ks, axis=0) == n_substeps).all()               # half a sample off the grid: no k hangs on a quotient's rounding
    modes = zr.plan_modes(plans["phase"], ks)
    changes, values = zr.mode_changes(modes)
    assert zr.plan_condition(modes) and values == {0, 1, 2, 3} and int((changes > 0).sum()) >= 4
    assert all(changes[i] == 0 for i in zr.STILL_ROBOTS) and all(changes[i] == 1 for i in range(zr.B) if i not in zr.STILL_ROBOTS)
    # the shared plan of the GPU test: the three walking modes, four robots or more change
    shared = tj.walk_plan(zr.SIM_TIME, zr.DT)["phase"]
    ms = zr.plan_modes(shared, zr.preview_indices(zr.start_clocks(shared, n_substeps), zr.NT, n_substeps))
    cs, vs = zr.mode_changes(ms)
    assert vs == {tj.PHASE_DOUBLE, tj.PHASE_RIGHT, tj.PHASE_LEFT} and int((cs > 0).sum()) >= 4


def test_rigid_modes_is_the_oracles_phase_at_k_on_those_plans():
    """The oracle's evaluation reports the preview index and the support phase it used (info[0], info[1]); on every robot's plan, at every
    control tick's clock of the n_substeps = 3 run and beyond the end of the arrays, rigid_modes(phase, k) is that phase."""
    plans = zr.plans()
    S = pc.contact_states()
    t0 = zr.start_clocks(plans["phase"], 3)
    ks = zr.preview_indices(t0, zr.NT, 3)
    o = pc.make_oracle()
    seen = set()
    for i in range(zr.B):
        o.set_refs(plans["zmp_x"][i], plans["zmp_y"][i], plans["phase"][i])
        t = t0[i]
        for j in range(zr.NT):
            o.set_prev_velocity(np.zeros(30))
            e = o.eval(S["q0"], np.zeros(30), t)
            assert e["k"] == ks[j, i] == tj.preview_index(t, zr.DT), (i, j)
            assert e["phase"] == int(tj.rigid_modes(plans["phase"][i], e["k"])) == int(tj.rigid_modes(plans["phase"], e["k"])[i]), (i, j)
            seen.add(e["phase"])
            for _ in range(3):
                t = t + zr.DT
        e = o.eval(S["q0"], np.zeros(30), zr.SIM_TIME + 5.0)         # k beyond the arrays: clamped to the last sample, as the kernels clamp it
        assert e["k"] >= plans["phase"].shape[1] and e["phase"] == int(tj.rigid_modes(plans["phase"][i], e["k"])) == int(plans["phase"][i, -1])
    assert seen == {0, 1, 2, 3}
    # no phase array: double support, what LMH_RIGID_PLAN holds then
    o.set_refs(plans["zmp_x"][0], plans["zmp_y"][0], None)
    assert o.eval(S["q0"], np.zeros(30), 0.45)["phase"] == tj.PHASE_DOUBLE
