"""The matrix-core tiles of the 15-row QP set-up with their guards folded: every tile epilogue forms what depends on the lane alone --
predicates, the selected 1 / D entries, base pointers with the zero / trash redirection folded in -- once, and its result registers
differ by immediates.  The cases where a folded guard can be wrong without the rest of the suite noticing (tests/qp_tiles_cases.py):
three distinct D^-1 blocks per robot against the CPU oracle, and every support phase of a compressed walking plan against the oracle,
against the NaN-filled-LDS checker build (a base plus immediate that lands on unwritten LDS) and against itself in split launches.
(The guarded Gauss-Jordan step with one DPP row switched off, whose pivot predicate is a constant lane mask now, is pinned by
tests/dpp_cases.guard_cases: use = 1 and use = 2.)"""
import os

import numpy as np
import pytest
import torch

from helpers import TOL_REL, WEIGHT, bits_differ, cfg2, close, run_probe, same_bits, vec_err  # noqa: F401
from params_cases import columns, make_controller
from qp_tiles_cases import (DT, TH, WALK_NT, WALK_SPLIT, WALK_XS, WEIGHT_NT, WEIGHT_SETS, walk_oracle, walk_plan, walk_run, weight_oracle,
                            weight_pushes)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------- 1. three distinct 1 / D blocks per robot
def test_distinct_weight_blocks_per_robot_against_the_oracle(cfg2):
    """Three robots, each with its own clearly distinct (w_base_pos, w_base_ang, w_joints) through lmh_set_params, 8 ticks of the rollout
    from the IK posture on stance references with two velocity pushes per robot inside the launch: tau and f of every tick (the log), the
    accelerations of the last evaluation (out[:, 36:66]) and k against one oracle per robot, at the tolerance of
    tests/test_gpu_params.py (helpers.close: 1e-6 relative, forces with the weight's floor)."""
    B = len(WEIGHT_SETS)
    for s in WEIGHT_SETS:                                           # the three blocks differ by more than a factor 2 within every robot
        w = sorted(s[k] for k in ("w_base_pos", "w_base_ang", "w_joints"))
        assert w[1] > 2.0 * w[0] and w[2] > 2.0 * w[1], s
    ticks, dv = weight_pushes()
    assert ticks.shape == (B, 2) and ticks.max() < WEIGHT_NT - 1
    refs = [weight_oracle(cfg2["q0"], WEIGHT_SETS[i], ticks[i], dv[i]) for i in range(B)]
    assert all(r["qp_status_seen"] == 0 for r in refs)
    ctl = make_controller(B, cfg2["dt"], cfg2["th"], cfg2["zcom"], warm_start=1)
    ctl.set_params(**columns(WEIGHT_SETS, ctl.cfg))
    assert ctl.params_per_instance()
    ctl.set_refs_stance(2.0, 2)
    ctl.set_pushes(ticks, dv)
    st = ctl.new_state(cfg2["q0"], np.zeros(30), t=0.0)
    out, status, log = ctl.rollout(st, WEIGHT_NT, log=True)
    torch.cuda.synchronize()
    out, status, log, stn = out.cpu().numpy(), status.cpu().numpy(), log.cpu().numpy(), st.cpu().numpy()
    ctl.close()
    assert (status[:, 2] == 0).all(), status[:, 2]
    worst = dict(tau=0.0, f=0.0, qdd=0.0)
    for i, r in enumerate(refs):
        worst["qdd"] = max(worst["qdd"], vec_err(out[i, 36:66], r["qpp"]))
        for tk in range(WEIGHT_NT):
            worst["tau"] = max(worst["tau"], vec_err(log[tk, i, :24], r["log"][tk, :24]))
            worst["f"] = max(worst["f"], float(np.abs(log[tk, i, 24:] - r["log"][tk, 24:]).max() / WEIGHT))
    print("distinct weight blocks against the oracle, worst relative errors:", worst)
    for i, r in enumerate(refs):
        assert status[i, 0] == r["k"][-1], i
        assert close(out[i, 36:66], r["qpp"]), (i, vec_err(out[i, 36:66], r["qpp"]))
        assert close(stn[i, :60], r["state"]), (i, vec_err(stn[i, :60], r["state"]))
        for tk in range(WEIGHT_NT):
            assert close(log[tk, i, :24], r["log"][tk, :24], TOL_REL), (i, tk)
            assert close(log[tk, i, 24:], r["log"][tk, 24:], TOL_REL, scale=WEIGHT), (i, tk)


# ------------------------------------------------------------------------------- 2. every support phase through the tiles
@pytest.fixture(scope="module")
def walk(cfg2):
    """the one 64-tick launch of the four walkers on the shipped library, shared by the three comparisons"""
    return walk_run(cfg2["q0"], cfg2["zcom"])


def test_compressed_walk_against_the_oracle(cfg2, walk):
    plan = walk_plan()
    ph = plan["phase"][1:WALK_NT + 1]                               # k of the ticks' fourth evaluations: 1..64
    assert set(int(p) for p in ph) == {0, 1, 2}
    touch_downs = int(((ph[:-1] != 0) & (ph[1:] == 0)).sum())
    assert touch_downs >= 1
    assert (walk["status"][:, 2] == 0).all(), walk["status"][:, 2]
    worst = dict(tau=0.0, f=0.0)
    refs = [walk_oracle(cfg2["q0"], cfg2["zcom"], plan, WALK_XS[i]) for i in range(len(WALK_XS))]
    for i, r in enumerate(refs):
        assert r["info"][3] == 0, i
        for tk in range(WALK_NT):
            worst["tau"] = max(worst["tau"], vec_err(walk["log"][tk, i, :24], r["log"][tk][:24]))
            worst["f"] = max(worst["f"], float(np.abs(walk["log"][tk, i, 24:] - r["log"][tk][24:]).max() / WEIGHT))
    print("compressed walk against the oracle, worst relative errors:", worst)
    off_l = np.abs(walk["log"][:, :, 24 + 6:24 + 12]).max(axis=2) == 0.0
    off_r = np.abs(walk["log"][:, :, 24:24 + 6]).max(axis=2) == 0.0
    assert off_l.any() and off_r.any() and (~(off_l | off_r)).any()      # each foot was unloaded at some tick, and both carried at others
    for i, r in enumerate(refs):
        assert walk["status"][i, 0] == r["k"][-1], i
        assert close(walk["state"][i, :60], r["state"], TOL_REL), (i, vec_err(walk["state"][i, :60], r["state"]))
        for tk in range(WALK_NT):
            assert close(walk["log"][tk, i, :24], r["log"][tk][:24], TOL_REL), (i, tk)
            assert close(walk["log"][tk, i, 24:], r["log"][tk][24:], TOL_REL, scale=WEIGHT), (i, tk)


_POISON_CHILD = r"""
import json, os, sys
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np, torch                     # torch before the library is loaded, as in the suite's other children
from linearmpchumanoid_amd import capi
from qp_tiles_cases import walk_run
q0 = np.load(sys.argv[1])
res = walk_run(q0["q0"], float(q0["zcom"]))
np.savez(sys.argv[2], **res)
print(json.dumps({"build_flags": capi.lib().lmh_debug_build_flags()}))
"""


def test_compressed_walk_on_nan_filled_lds_is_bit_equal(cfg2, walk, tmp_path):
    """The same launch on the checker build that fills every robot's LDS with NaNs first (a fresh child process; lmh_debug_build_flags
    bit 0 says which library ran): a tile address that lands on LDS nobody wrote, or on the other wave's live scratch, shows as a
    different bit somewhere in state, out, status or the log."""
    from linearmpchumanoid_amd import build as hipbuild
    assert os.path.exists(hipbuild.build_variant("poison", ["-DLMH_POISON"]))
    src, dst = str(tmp_path / "start.npz"), str(tmp_path / "poison.npz")
    np.savez(src, q0=cfg2["q0"], zcom=cfg2["zcom"])
    res = run_probe(_POISON_CHILD, variant="poison", timeout=300, args=(src, dst))
    assert res["build_flags"] & 1 == 1, res
    got = np.load(dst)
    assert np.isfinite(walk["log"]).all()
    for name in ("state", "out", "status", "log"):
        assert same_bits(walk[name], got[name]), name


def test_compressed_walk_in_three_launches_is_bit_equal(cfg2, walk):
    assert sum(WALK_SPLIT) == WALK_NT
    parts = walk_run(cfg2["q0"], cfg2["zcom"], split=WALK_SPLIT)
    assert bits_differ(walk, parts) == []
