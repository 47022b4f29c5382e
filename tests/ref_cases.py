"""Shared cases of the caller-supplied CoM reference tests (test_ref_cases.py on the CPU, test_gpu_ref.py on the GPU).

lmh_eval_ref is lmh_eval with Mpc3dLip::getXRef / getYRef replaced by six words the caller supplies (include/lmh.h).  The reference's
controller has no such door and the C oracle states the reference, so the checker here is the independent numpy restatement
(oracle/restatement_np.py) with RefMpc, a subclass of its Mpc whose compute() hands out supplied values: everything behind the MPC stage --
PDMomentumAcc, the QP, the outputs -- is the restatement's own code, unchanged.
States: helpers.posture_sweep at the narrowest band (the draw the restatement is already held to the C oracle on,
test_independent_restatement.py), B = 8, t = 0 on the stance plan.  References: position, velocity and acceleration of both axes drawn
independently of one another around the robot's own CoM state, so they satisfy no LIPM step x+ = A x + B u.
Results are cached per process and never written by a test."""
import numpy as np

from helpers import SWEEP_BANDS, oracle_system, posture_sweep
from oracle import restatement_np as R

DT, TH, B = 1e-3, 0.016, 8
BAND = SWEEP_BANDS[0]
REF_SEED = 20261026
REF_POS, REF_VEL, REF_ACC = 0.05, 0.3, 2.0      # half-widths [m, m/s, m/s^2] of the off-manifold draw


class RefMpc(R.Mpc):
    """restatement_np.Mpc whose step is not computed but supplied: compute() sets xRef, yRef to the values of supply() and
    k = int(t / dt), as lmh_eval_ref does."""

    def supply(self, xref, yref):
        self._x, self._y = np.array(xref, dtype=np.float64), np.array(yref, dtype=np.float64)

    def compute(self, pos, vel, zx, zy, t):
        self.xRef, self.yRef, self.k = self._x.copy(), self._y.copy(), int(t / self.dt)
        return self.k


def restatement_system(zcom, mpc=None, sim_time=2.0):
    """restatement_np.offline_system, with `mpc` in the place of its Mpc when given."""
    ctl = R.offline_system(DT, TH, zcom, sim_time=sim_time)
    if mpc is not None:
        ctl.mpc = mpc
    return ctl


_cache = {}


def states():
    """dict(q0, zcom, q [B,30], v [B,30], vp [B,30]): the first B robots of the narrowest band of the posture sweep."""
    if "states" not in _cache:
        o = oracle_system(DT, TH)
        q0, zcom = o.robot()["q"].copy(), o.zcom
        q, v, vp = posture_sweep(q0, B, BAND)
        _cache["states"] = dict(q0=q0, zcom=zcom, q=q, v=v, vp=vp)
    return _cache["states"]


def plain_restatement():
    """The restatement as it is on every state: list of dict(out, com, comvel, xref, yref) -- xref, yref are Mpc.compute's own."""
    if "plain" not in _cache:
        S, res = states(), []
        for i in range(B):
            ctl = restatement_system(S["zcom"])
            ctl.rb.v = S["vp"][i].copy()
            out = ctl.stand_step(S["q"][i], S["v"][i], 0.0)
            res.append(dict(out=out, com=ctl.rb.CoM.copy(), comvel=ctl.rb.comVel.copy(), xref=ctl.mpc.xRef.copy(), yref=ctl.mpc.yRef.copy(), k=ctl.mpc.k))
        _cache["plain"] = res
    return _cache["plain"]


def with_reference(i, xref, yref):
    """The restatement on state i tracking the supplied reference -> its wbc() result."""
    S = states()
    mpc = RefMpc(DT, TH, S["zcom"])
    mpc.supply(xref, yref)
    ctl = restatement_system(S["zcom"], mpc)
    ctl.rb.v = S["vp"][i].copy()
    out = ctl.stand_step(S["q"][i], S["v"][i], 0.0)
    assert mpc.k == 0
    return out


def off_manifold_refs():
    """[B,16] records: xRef | yRef within +-REF_POS, +-REF_VEL of the robot's CoM and CoM velocity and +-REF_ACC of zero acceleration, every
    word drawn on its own; the words a record carries beside them ([6, 16)) hold values lmh_eval_ref must not read."""
    if "refs" not in _cache:
        rng = np.random.default_rng(REF_SEED)
        plain = plain_restatement()
        rec = rng.normal(0.0, 1.0e3, (B, 16))
        for i in range(B):
            for ax in range(2):
                rec[i, 3 * ax + 0] = plain[i]["com"][ax] + rng.uniform(-REF_POS, REF_POS)
                rec[i, 3 * ax + 1] = plain[i]["comvel"][ax] + rng.uniform(-REF_VEL, REF_VEL)
                rec[i, 3 * ax + 2] = rng.uniform(-REF_ACC, REF_ACC)
        _cache["refs"] = rec
    return _cache["refs"]


def off_manifold_results():
    """The restatement's results on off_manifold_refs(), one per state (computed once, shared)."""
    if "offm" not in _cache:
        r = off_manifold_refs()
        _cache["offm"] = [with_reference(i, r[i, 0:3], r[i, 3:6]) for i in range(B)]
    return _cache["offm"]
