"""Per-robot plans without a GPU: the C ABI's new entry points exist and refuse a null handle before anything touches the device, and
trajectories.walk_plans / jump_plans are walk_plan / jump_plan per robot, stacked and zero-padded to one segment count."""
import ctypes as C

import numpy as np
import pytest

from plan_draw import MPC_DT, SIM_TIME, draw_jump_specs, draw_walk_specs, spec_i

NEW_SYMBOLS = ("lmh_gen_walk_batch", "lmh_gen_jump_batch", "lmh_set_plans", "lmh_plans_per_instance", "lmh_get_plan")
LMH_ERR_BAD_ARG = -2


def test_new_symbols_are_exported_and_refuse_a_null_handle(hip_lib):
    from linearmpchumanoid_amd import capi
    for name in NEW_SYMBOLS:
        assert name in capi.EXPORTS and hasattr(hip_lib, name), name
    walk = (capi.LmhWalkSpec * 2)()
    jump = (capi.LmhJumpSpec * 2)()
    z = np.zeros(8)
    zp = z.ctypes.data_as(C.c_void_p)
    assert hip_lib.lmh_gen_walk_batch(None, 1.0, walk, 2) == LMH_ERR_BAD_ARG
    assert b"null handle" in hip_lib.lmh_last_error()
    assert hip_lib.lmh_gen_jump_batch(None, 1.0, jump, 2) == LMH_ERR_BAD_ARG
    assert hip_lib.lmh_set_plans(None, zp, zp, None, 4, None, 0, None, 2) == LMH_ERR_BAD_ARG
    assert hip_lib.lmh_plans_per_instance(None) == LMH_ERR_BAD_ARG
    assert hip_lib.lmh_get_plan(None, 0, zp, zp, None, None, None) == LMH_ERR_BAD_ARG
    # the spec records are the header's: five doubles and two int32 / two doubles
    assert C.sizeof(capi.LmhWalkSpec) == 48 and C.sizeof(capi.LmhJumpSpec) == 16


def test_walk_plans_is_walk_plan_per_robot_zero_padded():
    from linearmpchumanoid_amd import trajectories
    B = 24
    sp, _ = draw_walk_specs(B)
    assert set(sp["num_steps"].tolist()) == {2, 3, 4} and set(sp["first_support"].tolist()) == {1, 2}     # a mixed draw
    plans = trajectories.walk_plans(SIM_TIME, MPC_DT, sp)
    n = int((SIM_TIME + 0.5) / MPC_DT)
    n_seg = 2 * int(sp["num_steps"].max()) + 2
    assert plans["zmp_x"].shape == (B, n) and plans["segs"].shape == (B, n_seg, 52) and plans["seg_of_sample"].shape == (B, n)
    assert plans["phase"].dtype == np.uint8 and plans["seg_of_sample"].dtype == np.uint16
    for i in range(B):
        p = trajectories.walk_plan(SIM_TIME, MPC_DT, **spec_i(sp, i))
        used = 2 * int(sp["num_steps"][i]) + 2
        assert p["segs"].shape[0] == used
        for k in ("zmp_x", "zmp_y", "phase", "seg_of_sample"):
            assert np.array_equal(plans[k][i], p[k]), (i, k)
        assert np.array_equal(plans["segs"][i, :used], p["segs"])
        assert not plans["segs"][i, used:].any()                      # the padding records are zero
        assert int(plans["seg_of_sample"][i].max()) < used            # and no sample selects one
    # scalars broadcast, missing fields take walk_plan's defaults
    q = trajectories.walk_plans(SIM_TIME, MPC_DT, dict(num_steps=[2, 4], time_per_step=0.4))
    assert np.array_equal(q["segs"][1], trajectories.walk_plan(SIM_TIME, MPC_DT, num_steps=4, time_per_step=0.4)["segs"])
    with pytest.raises(ValueError):
        trajectories.walk_plans(SIM_TIME, MPC_DT, dict(num_steps=[2, 4], time_per_step=[0.4, 0.5, 0.6]))
    with pytest.raises(KeyError):
        trajectories.walk_plans(SIM_TIME, MPC_DT, dict(step_length=[0.04]))


def test_jump_plans_is_jump_plan_per_robot():
    from linearmpchumanoid_amd import trajectories
    B = 12
    sp = draw_jump_specs(B)
    plans = trajectories.jump_plans(1.2, MPC_DT, sp)
    for i in range(B):
        p = trajectories.jump_plan(1.2, MPC_DT, stance_time=float(sp["stance_time"][i]), flight_time=float(sp["flight_time"][i]))
        for k in ("zmp_x", "zmp_y", "phase"):
            assert np.array_equal(plans[k][i], p[k]), (i, k)
    assert len({bytes(r) for r in plans["phase"]}) > 1                # the robots leave the ground in different ticks


def test_the_draw_desynchronises_sixteen_robots():
    """What the closed-loop GPU test asserts at tick 700, checked on the host plans: among the first sixteen robots of the draw all three
    support phases occur at samples 40, 70, 100 and 130."""
    from linearmpchumanoid_amd import trajectories
    sp, xs = draw_walk_specs(16)
    assert (xs >= 0.02).all() and (xs <= 0.05).all()
    plans = trajectories.walk_plans(SIM_TIME, MPC_DT, sp)
    for k in (40, 70, 100, 130):
        assert set(plans["phase"][:, k].tolist()) == {0, 1, 2}, k
