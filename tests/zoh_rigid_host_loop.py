"""The host loop that DEFINES lmh_rollout_zoh_rigid (include/lmh.h): zoh_host_loop.host_loop, as it stands, with every plant_step of a hold
replaced by plant_step_rigid(mode_j, kv).  host_loop is handed a controller whose stand_step fixes the mode of its control tick behind the
evaluation -- the caller's word, the caller's record of the tick, or trajectories.rigid_modes at the preview index the evaluation reports --
and whose plant_step is plant_step_rigid on it; every other piece (the pushes, the measurement, the actuator, the samples) is host_loop's
own, as in servo_host_loop.py.  The handle carries, like host_loop's, neither a push schedule nor actuator records."""
import numpy as np
import torch

from zoh_host_loop import actuate, assert_same, fresh, host_loop, push_schedules, wrench_and_refs        # noqa: F401  (shared with the tests)


class RigidLoopController:
    """What host_loop sees in the place of the controller: stand_step also fixes the mode of its control tick -- one word per robot for every
    piece of the hold --, plant_step is plant_step_rigid on it and keeps the multiplier of the tick's last piece (that of the first stage of
    the hold's last substep wherever the cuts fall); everything else is the controller's."""

    def __init__(self, ctl, n_ticks, mode, kv, phase):
        self._ctl, self._mode, self._kv, self._phase = ctl, mode, kv, phase
        self._tick, self._m = -1, None
        self.lam = torch.zeros((n_ticks, ctl.B, 12), dtype=torch.float64, device=ctl.device)
        self.modes = torch.zeros((n_ticks, ctl.B), dtype=torch.int32, device=ctl.device)

    def __getattr__(self, name):
        return getattr(self._ctl, name)

    def stand_step(self, state, out=None, status=None, **kw):
        from linearmpchumanoid_amd.trajectories import rigid_modes
        res = self._ctl.stand_step(state, out, status, **kw)
        self._tick += 1
        mode, m = self._mode, None
        if isinstance(mode, str):
            assert mode == "plan"
            if self._phase is not None:
                ph, ks = np.asarray(self._phase), res[1][:, 0].cpu().numpy()
                m = torch.as_tensor(np.array([int(rigid_modes(ph[i] if ph.ndim == 2 else ph, ks[i])) for i in range(len(ks))], dtype=np.int32)).to(self._ctl.device)
        elif mode is not None:
            m = (mode[self._tick] if mode.ndim == 2 else mode).contiguous()
        self._m = m
        self.modes[self._tick] = 0 if m is None else (m & 3)
        return res

    def plant_step(self, state, tau=None, n_substeps=1):
        state, lm, flags = self._ctl.plant_step_rigid(state, tau, self._m, self._kv, n_substeps)
        self.lam[self._tick] = lm
        return state, flags


def host_loop_rigid(ctl, st, status, n_ticks, n_substeps, *, mode=None, kv=0.0, phase=None, bw=None, sched=None, refs=None, meas=None, act=None):
    """The definition on a handle WITHOUT a schedule and WITHOUT actuator records.  mode: None (both soles) | int32 [B] | int32 [n_ticks,B]
    | "plan", then phase: None (no phase array: both soles) | array [n] (a shared plan) | array [B,n] (per-robot plans) and the mode of
    robot i on tick j is trajectories.rigid_modes(phase_i, status[i, 0]) of that tick's evaluation.  bw, sched, refs, meas, act: as
    zoh_host_loop.host_loop takes them.
    -> dict(out, status with [1] / [2] merged as max / OR over the ticks and the plant's flags, log [n_ticks,B,36], applied [n_ticks,B,24],
    trace [n_ticks,B,180], lam [n_ticks,B,12]: the multiplier the last piece of every tick's hold returned, modes [n_ticks,B])."""
    proxy = RigidLoopController(ctl, n_ticks, mode, kv, phase)
    res = host_loop(proxy, st, status, n_ticks, n_substeps, bw=bw, sched=sched, refs=refs, meas=meas, act=act)
    return dict(res, lam=proxy.lam, modes=proxy.modes)
