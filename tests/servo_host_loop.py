"""The host loop that DEFINES lmh_rollout_zoh_servo (include/lmh.h): zoh_host_loop.host_loop, as it stands, with every plant_step of a hold
replaced by plant_step_servo on the control tick's setpoint.  host_loop is handed a controller whose stand_step forms that setpoint behind
the evaluation -- from the joint words the evaluation READ and the joint rows of its out.qdd (LMH_SERVO_INTEGRATE), or from the caller's
record of the tick (LMH_SERVO_CALLER) -- and whose plant_step is plant_step_servo; every other piece (the pushes, the measurement, the
actuator, the samples) is host_loop's own.  The handle carries the servo table and, like host_loop's, neither a push schedule nor actuator
records."""
import torch

from zoh_host_loop import host_loop


def integrate_setpoint(read, out, n_substeps, dt):
    """trajectories.servo_setpoint in torch on the device: read [B,96] the record the evaluation read, out [B,80] its out record ->
    [B,48].  Every elementwise operation is a kernel of its own: the products and the sums are rounded one by one."""
    q_m, v_m, a = read[:, 6:30], read[:, 36:60], out[:, 42:66]
    T = float(int(n_substeps)) * float(dt)
    h2 = (0.5 * T) * T
    ta, tv, ha = T * a, T * v_m, h2 * a
    v_des = v_m + ta
    s1 = q_m + tv
    return torch.cat([s1 + ha, v_des], dim=1).contiguous()


class ServoLoopController:
    """What host_loop sees in the place of the controller: stand_step also forms the setpoint of its control tick, plant_step is
    plant_step_servo on it, everything else is the controller's."""

    def __init__(self, ctl, n_substeps, servo):
        self._ctl, self._n_substeps, self._servo = ctl, n_substeps, servo
        self._tick, self._setpoint = 0, None

    def __getattr__(self, name):
        return getattr(self._ctl, name)

    def stand_step(self, state, out=None, status=None, **kw):
        res = self._ctl.stand_step(state, out, status, **kw)
        if isinstance(self._servo, str):
            assert self._servo == "integrate"
            self._setpoint = integrate_setpoint(state, res[0], self._n_substeps, self._ctl.cfg.dt)      # (stand_step writes v_prev alone)
        else:
            self._setpoint = self._servo[self._tick].contiguous()
        self._tick += 1
        return res

    def plant_step(self, state, tau=None, n_substeps=1):
        return self._ctl.plant_step_servo(state, self._setpoint, tau, n_substeps)


def servo_host_loop(ctl, st, status, n_ticks, n_substeps, servo, **options):
    """host_loop(ctl, st, status, n_ticks, n_substeps, **options) with the servo in every hold; servo: "integrate" | [n_ticks,B,48]."""
    assert options.get("box") is None, "the box-constrained loop is not offered with a servo"
    return host_loop(ServoLoopController(ctl, n_substeps, servo), st, status, n_ticks, n_substeps, **options)
