"""CPU side of lmh_rollout_zoh_box: the binding, the refusal that needs no device, the Python helpers, and that the cases the GPU tests run
hold what they are there for (zoh_box_cases.py).  No GPU is used."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import zoh_box_cases as zb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_bound_and_exported(hip_lib):
    from linearmpchumanoid_amd import capi
    from linearmpchumanoid_amd.controller import BatchedController
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lmh.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+lmh_rollout_zoh_box\s*\(", src) and "lmh_rollout_zoh_box" in capi.EXPORTS and hasattr(hip_lib, "lmh_rollout_zoh_box")
    args = capi.PROTOTYPES["lmh_rollout_zoh_box"][1]
    assert len(args) == 12 and args[4] == C.POINTER(capi.LmhZohOpts) and args[6:8] == [C.c_int, C.c_int] and args[9:11] == [C.c_int, C.c_int]
    assert callable(BatchedController.rollout_zoh_box)
    # the launcher is declared once, beside every other: lmh_launch_rollout_zoh's declaration carries the new call (no new symbol: the stand-alone host
    # programs under tests/host link against one stub per launcher)
    launch = open(os.path.join(ROOT, "linearmpchumanoid_amd", "csrc", "lmh_launch.h")).read()
    decl = re.findall(r"void\s+lmh_launch_rollout_zoh\s*\(([^;]*)\)\s*;", launch)
    assert len(decl) == 1 and "const LmhZohBox *" in decl[0]


def test_without_a_handle_the_call_is_refused(hip_lib):
    from linearmpchumanoid_amd import capi
    opts = capi.LmhZohOpts(pushes=1, trace_every=3)
    for o in (None, C.byref(opts)):
        assert hip_lib.lmh_rollout_zoh_box(None, None, None, None, o, None, 0, 1, None, 3, 2, None) == -2 and hip_lib.lmh_last_error() == b"null handle"


def test_lip_from_out_picks_the_measured_com_words():
    import torch
    from linearmpchumanoid_amd.controller import lip_from_out
    out = np.arange(3 * 80, dtype=np.float64).reshape(3, 80)
    t = np.array([0.5, 0.25, 0.125])
    lip = lip_from_out(out, t)
    assert lip.shape == (3, 8) and lip.dtype == np.float64
    assert np.array_equal(lip[:, 0:4], out[:, [66, 69, 67, 70]]) and np.array_equal(lip[:, 4], t) and not lip[:, 5:].any()
    assert np.array_equal(lip_from_out(out, 0.75)[:, 4], np.full(3, 0.75))
    lt = lip_from_out(torch.as_tensor(out), torch.as_tensor(t))
    assert isinstance(lt, torch.Tensor) and np.array_equal(lt.numpy(), lip)


def test_the_python_wrapper_rejects_a_reference():
    from linearmpchumanoid_amd.controller import BatchedController
    with pytest.raises(ValueError, match="exclusive"):
        BatchedController.rollout_zoh_box(None, None, None, 1, 1, ref=np.zeros((1, 6, 16)))


@pytest.mark.parametrize("N", sorted(zb.HORIZONS))
def test_the_moved_boxes_bind_and_robot_0_is_free(N):
    """The numpy statement at the start's reduced states, the velocity 20 % either way: robots 2 and 3 have active samples in the per-robot
    and in the shared sets, robot 0 has none in the per-robot sets, nothing runs out of rounds."""
    for t in (0.0, zb.T_MID):
        own, shared, flags = zb.binding(N, t)
        assert flags == 0
        assert (own[:, [2, 3]] > 0).all() and (shared[:, [2, 3]] > 0).all(), (N, t, own, shared)
        assert (own[:, 0] == 0).all(), (N, t, own)
    d = zb.draw(N)
    assert d["box"].shape == (zb.B, 4, d["n"]) and np.isinf(d["box"][0]).all() and np.array_equal(d["box"][2], d["shared"])
    k1 = int((zb.T_MID + 0.05) / d["mpc_dt"]) + N                    # the plan's own ZMP lies outside the moved box over every window of a run
    assert (d["plans"]["zmp_y"][2, 2:k1] < d["shared"][2, 2:k1]).all() and (d["plans"]["phase"][2, 2:k1] == 2).all()
    assert np.array_equal(d["box"][2, 2:4], d["box"][1, 2:4] + zb.SHIFT_Y) and np.array_equal(d["box"][2, 0:2], d["box"][1, 0:2] + zb.SHIFT_X)
    # robots 4 and 5 change phase inside the windows the tests run through
    k0 = int(zb.T_MID / d["mpc_dt"])
    for i in (4, 5):
        assert len(set(d["plans"]["phase"][i, k0:k0 + N + 1].tolist())) > 1
    e = zb.with_empty_sample(d["box"], 5)
    assert e[zb.EMPTY_ROBOT, 0, 5] > e[zb.EMPTY_ROBOT, 1, 5] and np.array_equal(np.delete(e, zb.EMPTY_ROBOT, 0), np.delete(d["box"], zb.EMPTY_ROBOT, 0))


def test_the_behaviour_push_takes_the_unconstrained_zmp_out_of_the_stance_box():
    zmp, inside = zb.behaviour_check()
    assert not inside, zmp
    assert zmp[1] > zb.STANCE_BOX["hi_y"] + 0.01, zmp                # by more than a centimetre: not a rounding matter
