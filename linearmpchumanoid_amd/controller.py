"""Host-side mirror of the reference's controller interface for B robots at once.

Names and argument meaning follow the reference classes (Controller::standStep / WBC,
Kinematics::compute, ZMP, footCoeffTrajectory, Mpc3dLip) so that tests read like calls into
the reference; every numeric result comes from the HIP kernels behind include/lmh.h.
torch is used only for device memory and streams.
"""
import ctypes as C

import numpy as np
import torch

from . import capi, trajectories
from .capi import LmhConfig, check


def default_config(dt=0.01, time_horizon=0.5, z_com=0.26, **overrides):
    """lmh_config with the reference literals (controller.hpp:80-124, mpcLinearPendulum.hpp:43-49).

    dt is the control step (Clock); mpc_dt=... (an override) is the MPC sample time / reference sample period
    (Mpc3dLip and ZMP constructor arguments, apps/offline/main.cpp:21,39); 0 or absent = dt."""
    cfg = LmhConfig()
    capi.lib().lmh_config_default(C.byref(cfg))
    cfg.dt, cfg.time_horizon, cfg.z_com = dt, time_horizon, z_com
    for k, v in overrides.items():
        if not hasattr(cfg, k):
            raise AttributeError(f"lmh_config has no field {k}")
        setattr(cfg, k, v)
    return cfg


def nominal_links():
    """createNaoParameters() table, [28][13] (mass | com | inertia), Aldebaran convention."""
    raw = np.zeros((28, 13), dtype=np.float64)
    capi.lib().lmh_nominal_links(raw.ctypes.data_as(C.c_void_p))
    return raw


def initial_configuration():
    """initialConfiguration() of the reference (src/Robot.cpp:242-251): posture the IK starts from."""
    return np.array([-0.0185, 0, 0.282, 0, 0, 0,
                     0, 0, -0.5, 0.8, -0.3, 0,
                     0, 0, -0.5, 0.8, -0.3, 0,
                     1.6, 0, 0, 0, 0,
                     -1.6, 0, 0, 0, 0,
                     0, 0], dtype=np.float64)


def ik_start_posture(device=0, com_target=(-0.02, 0.0, 0.26)):
    """apps/offline/main.cpp:24-39 on the GPU: IK to feet (0,-/+0.05,0) and the CoM target; returns (q[30], z_com)
    where z_com = Robot::getCoM()(2) after the IK (the Mpc3dLip constructor argument)."""
    ctl = BatchedController(1, default_config(), device=device)
    q = torch.as_tensor(initial_configuration()[None, :]).to(ctl.device)
    q, iters = ctl.ik(q, com_target=com_target)
    com = ctl.robot_com(q)
    torch.cuda.synchronize(ctl.device)
    out = q.cpu().numpy()[0].copy(), float(com.cpu().numpy()[0, 2])
    ctl.close()
    return out


def param_records(cfg, n_instances, **fields):
    """The [B,20] records BatchedController.set_params uploads (include/lmh.h, lmh_set_params): every field of capi.PARAM_FIELDS is a
    scalar or a length-B array, unnamed fields keep the value of cfg.  Unknown names, wrong lengths and non-finite values raise
    ValueError; nothing here touches the device."""
    B = int(n_instances)
    unknown = sorted(set(fields) - set(capi.PARAM_FIELDS))
    if unknown:
        raise ValueError(f"unknown parameter field(s) {unknown}; the per-robot fields are {sorted(capi.PARAM_FIELDS)}")
    rec = np.zeros((B, capi.PARAM_STRIDE), dtype=np.float64)
    for name, off in capi.PARAM_FIELDS.items():
        v = np.asarray(fields.get(name, getattr(cfg, name)), dtype=np.float64)
        if v.ndim > 1 or (v.ndim == 1 and v.shape[0] != B):
            raise ValueError(f"{name} must be a scalar or an array of length {B}")
        if not np.all(np.isfinite(v)):
            raise ValueError(f"{name} must be finite")
        rec[:, off] = v
    return rec


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _dev_ptr(t):
    """Device address of a tensor; None (an optional argument left out) stays None, the C side's NULL."""
    return None if t is None else C.c_void_p(t.data_ptr())


_NP_DTYPE = {torch.float64: np.float64, torch.int32: np.int32}     # the array dtype that becomes a tensor of the key's


# rollout_zoh_ex's option keywords and their defaults: what rollout_zoh_box, _io, _servo and _rigid take as they are
_ZOH_OPTIONS = dict(base_wrench=None, ref=None, pushes=False, log=False, trace_every=0, trace=None, metrics=None, out=None, status=None)


def _count(name, n):
    """A whole number >= 0, as an int."""
    if int(n) != n or n < 0:
        raise ValueError(f"{name} must be a whole number >= 0")
    return int(n)


def _split(rec, fields):
    """Named views of records [.., stride] (tensor or array) by one of the name -> (offset, shape) tables."""
    lead = tuple(rec.shape[:-1])
    return {k: rec[..., o:o + int(np.prod(s, dtype=np.int64))].reshape(lead + tuple(s)) for k, (o, s) in fields.items()}


class BatchedController:
    """B independent Robot+Mpc3dLip+Controller triples resident on one GPU.

    reference: Controller(Robot&, Mpc3dLip&, ZMP&, rFCoeff, lFCoeff) (controller.hpp:52-57).
    """

    def __init__(self, n_instances, config=None, device=0):
        if not torch.cuda.is_available():
            raise RuntimeError("BatchedController needs a HIP device (no CPU fallback)")
        self.B = int(n_instances)
        self.device_index = int(device)
        self.device = torch.device("cuda", self.device_index)
        self.cfg = config if config is not None else default_config()
        self._h = C.c_void_p()
        check(capi.lib().lmh_create(C.byref(self.cfg), self.B, self.device_index, C.byref(self._h)))
        self.N = capi.lib().lmh_horizon(self._h)

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            capi.lib().lmh_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ set-up
    def set_model(self, raw_links=None):
        """createNaoParameters + Robot ctor re-expression; raw_links [28,13] or [B,28,13]."""
        if raw_links is None:
            check(capi.lib().lmh_set_model(self._h, None, 1))
            return
        raw = np.ascontiguousarray(raw_links, dtype=np.float64)
        n = 1 if raw.ndim == 2 else raw.shape[0]
        check(capi.lib().lmh_set_model(self._h, _np_ptr(raw), n))

    def mass(self):
        out = np.zeros(self.B, dtype=np.float64)
        check(capi.lib().lmh_get_mass(self._h, _np_ptr(out)))
        return out

    def set_refs(self, zmp_x, zmp_y, phase=None):
        """ZMP reference arrays (ZMP::getZmpXRef/YRef) + optional per-sample support phase."""
        zx = np.ascontiguousarray(zmp_x, dtype=np.float64)
        zy = np.ascontiguousarray(zmp_y, dtype=np.float64)
        ph = None if phase is None else np.ascontiguousarray(phase, dtype=np.uint8)
        check(capi.lib().lmh_set_refs(self._h, _np_ptr(zx), _np_ptr(zy), None if ph is None else _np_ptr(ph), len(zx)))

    def set_refs_stance(self, simulation_time, support_foot=2):
        """ZMP(Task::Stand, simulationTime, timeStep, supportFoot) (zmpGeneration.cpp:12-23,39-60)."""
        check(capi.lib().lmh_set_refs_stance(self._h, float(simulation_time), int(support_foot)))

    def set_foot_coeffs(self, r_coeff, r_n, l_coeff, l_n):
        r = np.zeros((3, 8)); l = np.zeros((3, 8))
        r[:, :np.shape(r_coeff)[1]] = r_coeff
        l[:, :np.shape(l_coeff)[1]] = l_coeff
        rn = np.ascontiguousarray(r_n, dtype=np.int32); ln = np.ascontiguousarray(l_n, dtype=np.int32)
        check(capi.lib().lmh_set_foot_coeffs(self._h, _np_ptr(r), _np_ptr(rn), _np_ptr(l), _np_ptr(ln)))

    def set_segments(self, segs, seg_of_sample):
        """Walking extension: piecewise foot polynomials [n_seg,52] selected by seg_of_sample[k] (uint16)."""
        if segs is None:
            check(capi.lib().lmh_set_segments(self._h, None, 0, None, 0))
            return
        sg = np.ascontiguousarray(segs, dtype=np.float64)
        so = np.ascontiguousarray(seg_of_sample, dtype=np.uint16)
        check(capi.lib().lmh_set_segments(self._h, _np_ptr(sg), sg.shape[0], _np_ptr(so), len(so)))

    def gen_walk(self, simulation_time, num_steps=4, time_per_step=0.5, ds_time=0.1, step_height=0.02, settle_time=0.3,
                 first_support=capi.PHASE_RIGHT, foot_y=0.05):
        """lmh_gen_walk: the walking plan of trajectories.walk_plan generated by a device kernel (ZMP samples, support phase, swing
        polynomial segments); nothing is uploaded."""
        check(capi.lib().lmh_gen_walk(self._h, float(simulation_time), int(num_steps), float(time_per_step), float(ds_time), float(step_height),
                                      float(settle_time), int(first_support), float(foot_y)))

    def gen_jump(self, simulation_time, stance_time=0.4, flight_time=0.15):
        """lmh_gen_jump: stance references with a flight phase (trajectories.jump_plan), generated on the device."""
        check(capi.lib().lmh_gen_jump(self._h, float(simulation_time), float(stance_time), float(flight_time)))

    def get_refs(self):
        """The reference set the handle currently holds, read back from the device: dict(zmp_x, zmp_y, phase, segs, seg_of_sample).
        With per-robot plans it is robot 0's (lmh_get_refs is lmh_get_plan of robot 0)."""
        return self.get_plan(0)

    # -- one plan per robot (include/lmh.h, "Per-robot plans")
    def gen_walk_batch(self, simulation_time, specs):
        """lmh_gen_walk_batch: one walking plan per robot, generated on the device.  specs: dict of arrays of length B with gen_walk's
        keyword arguments (scalars broadcast, missing ones take gen_walk's defaults); the plans are trajectories.walk_plans(...)."""
        sp, _ = trajectories.broadcast_specs(specs, trajectories.WALK_SPEC_DEFAULTS, self.B)
        arr = (capi.LmhWalkSpec * self.B)()
        for i in range(self.B):
            for k, v in sp.items():
                setattr(arr[i], k, v[i].item())
        check(capi.lib().lmh_gen_walk_batch(self._h, float(simulation_time), arr, self.B))

    def gen_jump_batch(self, simulation_time, specs):
        """lmh_gen_jump_batch: one jumping schedule per robot (trajectories.jump_plans), generated on the device."""
        sp, _ = trajectories.broadcast_specs(specs, trajectories.JUMP_SPEC_DEFAULTS, self.B)
        arr = (capi.LmhJumpSpec * self.B)()
        for i in range(self.B):
            arr[i].stance_time, arr[i].flight_time = float(sp["stance_time"][i]), float(sp["flight_time"][i])
        check(capi.lib().lmh_gen_jump_batch(self._h, float(simulation_time), arr, self.B))

    def set_plans(self, zmp_x, zmp_y, phase=None, segs=None, seg_of_sample=None):
        """lmh_set_plans: one plan per robot uploaded from the host -- zmp_x, zmp_y [n,n_samples], phase [n,n_samples] or None,
        segs [n,n_seg,52] and seg_of_sample [n,n_samples] or None (trajectories.walk_plans / jump_plans return these as a dict:
        ctl.set_plans(**plans)).  n must be B (the library checks it)."""
        zx = np.ascontiguousarray(zmp_x, dtype=np.float64)
        zy = np.ascontiguousarray(zmp_y, dtype=np.float64)
        if zx.ndim != 2 or zy.shape != zx.shape:
            raise ValueError("zmp_x, zmp_y must be [n,n_samples]")
        ph = None if phase is None else np.ascontiguousarray(phase, dtype=np.uint8)
        if ph is not None and ph.shape != zx.shape:
            raise ValueError("phase must be [n,n_samples]")
        sg = so = None
        n_seg = 0
        if segs is not None:
            sg = np.ascontiguousarray(segs, dtype=np.float64)
            so = np.ascontiguousarray(seg_of_sample, dtype=np.uint16)
            if sg.ndim != 3 or sg.shape[0] != zx.shape[0] or sg.shape[2] != capi.SEG_STRIDE or so.shape != zx.shape:
                raise ValueError("segs must be [n,n_seg,52] and seg_of_sample [n,n_samples]")
            n_seg = sg.shape[1]
        check(capi.lib().lmh_set_plans(self._h, _np_ptr(zx), _np_ptr(zy), None if ph is None else _np_ptr(ph), zx.shape[1],
                                       None if sg is None else _np_ptr(sg), n_seg, None if so is None else _np_ptr(so), zx.shape[0]))

    @property
    def plans_per_instance(self):
        """True while every robot has a plan of its own (gen_walk_batch / gen_jump_batch / set_plans); any other setter ends it."""
        return bool(capi.lib().lmh_plans_per_instance(self._h))

    def get_plan(self, i):
        """Robot i's plan read back from the device (the shared one on a shared handle): the dict of get_refs."""
        n, ns = capi.lib().lmh_num_ref_samples(self._h), capi.lib().lmh_num_segments(self._h)
        zx, zy = np.zeros(n), np.zeros(n)
        ph = np.zeros(n, dtype=np.uint8)
        segs = np.zeros((ns, capi.SEG_STRIDE)); sos = np.zeros(n, dtype=np.uint16)
        check(capi.lib().lmh_get_plan(self._h, int(i), _np_ptr(zx), _np_ptr(zy), _np_ptr(ph), _np_ptr(segs) if ns else None, _np_ptr(sos) if ns else None))
        return dict(zmp_x=zx, zmp_y=zy, phase=ph, segs=segs, seg_of_sample=sos)

    # -- timed velocity pushes inside rollout (include/lmh.h, lmh_set_pushes)
    def set_pushes(self, ticks, dv=None):
        """lmh_set_pushes: velocity increments applied inside rollout at the start of given ticks.  ticks [B,n] or [n] (one schedule shared
        by all robots), whole numbers, -1 = unused; dv [..,n,30] laid out as state[:, 30:60].  trajectories.push_schedule sorts and pads
        them into records (and refuses what the library refuses, in the same words).  ticks=None clears the schedule."""
        if ticks is None:
            check(capi.lib().lmh_set_pushes(self._h, None, 0, 1))
            return
        rec = trajectories.push_schedule(ticks, dv, n_instances=self.B)
        check(capi.lib().lmh_set_pushes(self._h, _np_ptr(rec), rec.shape[1], rec.shape[0]))

    @property
    def pushes_per_instance(self):
        """True while every robot has a push schedule of its own."""
        return bool(capi.lib().lmh_pushes_per_instance(self._h))

    def get_pushes(self, i):
        """Robot i's schedule read back from the device (the shared one on a shared schedule): dict(ticks [n] int64, dv [n,30])."""
        n = capi.lib().lmh_num_pushes(self._h)
        rec = np.zeros((n, capi.PUSH_STRIDE))
        check(capi.lib().lmh_get_pushes(self._h, int(i), _np_ptr(rec) if n else None))
        return dict(ticks=rec[:, 0].astype(np.int64), dv=rec[:, 1:31].copy())

    # -- per-robot actuator records of rollout_zoh_io (include/lmh.h, lmh_set_actuators)
    def set_actuators(self, tau_max=None, alpha=None, delay=None):
        """lmh_set_actuators: what rollout_zoh_io(actuators=True) puts between the controller's torques and the plant.  tau_max (the torque
        limit, >= 0; None or inf: none) and alpha (the first-order lag coefficient in (0, 1]; None or 1: no lag) are scalars, [24] or
        [B,24]; delay (the latency in control ticks, a whole number 0 .. 7; None: 0) is a scalar or [B].  trajectories.actuator_records
        forms the records (and refuses what the library refuses, in the same words).  With no argument the table is cleared."""
        if tau_max is None and alpha is None and delay is None:
            check(capi.lib().lmh_set_actuators(self._h, None, 0))
            return
        rec = np.ascontiguousarray(trajectories.actuator_records(self.B, tau_max, alpha, delay))
        check(capi.lib().lmh_set_actuators(self._h, _np_ptr(rec), self.B))

    @property
    def actuators_per_instance(self):
        """True while every robot has an actuator record of its own."""
        return bool(capi.lib().lmh_actuators_per_instance(self._h))

    def get_actuators(self, i):
        """Robot i's actuator record: dict(tau_max [24], alpha [24], delay int); the defaults (inf, 1, 0) on a handle without records."""
        rec = np.zeros(capi.ACT_STRIDE)
        check(capi.lib().lmh_get_actuators(self._h, int(i), _np_ptr(rec)))
        return dict(tau_max=rec[0:24].copy(), alpha=rec[24:48].copy(), delay=int(rec[capi.ACT_OFF_DELAY]))

    def new_act_mem(self, tau0=None):
        """The actuator memory of rollout_zoh_io [B,192] on the device: PREV and every queue slot filled with tau0 [B,24] (None: zeros)."""
        mem = torch.zeros((self.B, capi.ACT_MEM_STRIDE), dtype=torch.float64, device=self.device)
        if tau0 is not None:
            t0 = tau0 if isinstance(tau0, torch.Tensor) else torch.as_tensor(np.asarray(tau0, dtype=np.float64))
            mem[:] = t0.to(self.device, torch.float64).expand(self.B, 24).repeat(1, 1 + capi.ACT_MAX_DELAY)
        return mem

    # -- per-robot joint servo of plant_step_servo and rollout_zoh_servo (include/lmh.h, lmh_set_servo)
    def set_servo(self, kp=None, kd=None):
        """lmh_set_servo: the per-joint PD gains the joint servo adds to the feed-forward torque inside every hold of plant_step_servo and
        rollout_zoh_servo.  kp (N m / rad) and kd (N m s / rad) are scalars, [24] or [B,24], finite and >= 0 (None: 0);
        trajectories.servo_records forms the records (and refuses what the library refuses, in the same words).  No other call reads the
        table.  With no argument the table is cleared."""
        if kp is None and kd is None:
            check(capi.lib().lmh_set_servo(self._h, None, 0))
            return
        rec = np.ascontiguousarray(trajectories.servo_records(self.B, 0.0 if kp is None else kp, 0.0 if kd is None else kd))
        check(capi.lib().lmh_set_servo(self._h, _np_ptr(rec), self.B))

    @property
    def servo_per_instance(self):
        """True while every robot has a servo record of its own."""
        return bool(capi.lib().lmh_servo_per_instance(self._h))

    def get_servo(self, i):
        """Robot i's servo record: dict(kp [24], kd [24]); zeros on a handle without records."""
        rec = np.zeros(capi.SERVO_STRIDE)
        check(capi.lib().lmh_get_servo(self._h, int(i), _np_ptr(rec)))
        return dict(kp=rec[0:24].copy(), kd=rec[24:48].copy())

    # -- per-robot ground planes under the soles (include/lmh.h, lmh_set_ground)
    def set_ground(self, records=None):
        """lmh_set_ground: the plane under each foot that the plant calls (contact_wrench, plant_derivative, plant_step) and rollout_zoh,
        rollout_zoh_ex and rollout_zoh_io press the sole vertices against, instead of z = 0.  records [8] (one for every robot) or [B,8]:
        n_R(3) | h_R | n_L(3) | h_L, the ground under a foot being n.x <= h with a unit normal n, n_z > 0 (trajectories.ground_planes forms
        them from a slope, its azimuth and per-foot offsets; nothing is normalised here).  The controller is not told: its foot references
        and friction pyramid stay the flat ones.  rollout_zoh_box is refused while a table is set; every other call ignores it.  None clears
        the table."""
        if records is None:
            check(capi.lib().lmh_set_ground(self._h, None, 0))
            return
        rec = np.ascontiguousarray(np.asarray(records, dtype=np.float64))
        if rec.ndim not in (1, 2) or rec.shape[-1] != capi.GROUND_STRIDE:
            raise ValueError(f"records must be [{capi.GROUND_STRIDE}] or [n_sets,{capi.GROUND_STRIDE}]")
        check(capi.lib().lmh_set_ground(self._h, _np_ptr(rec), 1 if rec.ndim == 1 else rec.shape[0]))

    @property
    def ground_per_instance(self):
        """True while every robot has a ground record of its own."""
        return bool(capi.lib().lmh_ground_per_instance(self._h))

    def get_ground(self, inst):
        """Robot inst's ground record [8], the bytes that were set; the flat record 0 0 1 0 | 0 0 1 0 on a handle without a table."""
        rec = np.zeros(capi.GROUND_STRIDE)
        check(capi.lib().lmh_get_ground(self._h, int(inst), _np_ptr(rec)))
        return rec

    # -- per-robot gains, QP weights, friction and contact parameters (include/lmh.h, lmh_set_params)
    def set_params(self, **fields):
        """lmh_set_params: one set of PD gains, QP weights, eps_coeff, mu and contact constants per robot, e.g.
        set_params(kp_joints=np.linspace(200, 400, B), mu=0.5).  With no arguments the handle goes back to the values of its config."""
        if not fields:
            check(capi.lib().lmh_set_params(self._h, None, 0))
            return
        rec = param_records(self.cfg, self.B, **fields)           # ValueError before any device call
        check(capi.lib().lmh_set_params(self._h, _np_ptr(rec), self.B))

    def params_per_instance(self):
        """True while every robot has a parameter set of its own (set_params with arguments, B > 1)."""
        return bool(capi.lib().lmh_params_per_instance(self._h))

    def get_params(self, i):
        """Robot i's parameters as a dict over capi.PARAM_FIELDS (the config's values on a handle without per-robot parameters)."""
        rec = np.zeros(capi.PARAM_STRIDE, dtype=np.float64)
        check(capi.lib().lmh_get_params(self._h, int(i), _np_ptr(rec)))
        return {name: float(rec[off]) for name, off in capi.PARAM_FIELDS.items()}

    def set_xscale(self, xscale):
        """Per-instance step-length scale of ZMP x and x-axis foot polynomials ([B] or None)."""
        if xscale is None:
            check(capi.lib().lmh_set_xscale(self._h, None, 0))
            return
        xs = np.ascontiguousarray(xscale, dtype=np.float64)
        check(capi.lib().lmh_set_xscale(self._h, _np_ptr(xs), len(xs)))

    def set_zcom(self, z_com):
        z = np.atleast_1d(np.ascontiguousarray(z_com, dtype=np.float64))
        check(capi.lib().lmh_set_zcom(self._h, _np_ptr(z), len(z)))

    def mpc_gain(self):
        K = np.zeros(self.N + 1, dtype=np.float64)
        check(capi.lib().lmh_get_mpc_gain(self._h, _np_ptr(K)))
        return K

    # ------------------------------------------------------------------ buffers
    def new_state(self, q, v, t=0.0, v_prev=None):
        """state records [B,96]: q | v | v_prev (Robot::v_, zeros after construction) | t."""
        st = torch.zeros((self.B, capi.STATE_STRIDE), dtype=torch.float64)
        st[:, 0:30] = torch.as_tensor(np.broadcast_to(np.asarray(q, dtype=np.float64), (self.B, 30)).copy())
        st[:, 30:60] = torch.as_tensor(np.broadcast_to(np.asarray(v, dtype=np.float64), (self.B, 30)).copy())
        if v_prev is not None:
            st[:, 60:90] = torch.as_tensor(np.broadcast_to(np.asarray(v_prev, dtype=np.float64), (self.B, 30)).copy())
        st[:, 90] = torch.as_tensor(np.broadcast_to(np.asarray(t, dtype=np.float64), (self.B,)).copy())
        return st.to(self.device)

    def new_out(self):
        return torch.zeros((self.B, capi.OUT_STRIDE), dtype=torch.float64, device=self.device)

    def new_status(self):
        return torch.zeros((self.B, capi.STATUS_STRIDE), dtype=torch.int32, device=self.device)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ------------------------------------------------------------------ hot path
    def _ref_records(self, ref, lead):
        """Caller-supplied CoM references (lmh_eval_ref): a tensor or array of shape lead + [B, 16] -> contiguous float64 records on this
        controller's device.  Words 0:3 | 3:6 of a record are xRef | yRef (position, velocity, acceleration); the others are not read."""
        shape = tuple(lead) + (self.B, capi.MPC_STRIDE)
        if isinstance(ref, np.ndarray):
            if ref.dtype != np.float64:
                raise ValueError(f"ref must be float64, not {ref.dtype}")
            ref = torch.from_numpy(np.ascontiguousarray(ref))
        if not isinstance(ref, torch.Tensor):
            raise ValueError("ref must be a tensor or an array")
        if ref.dtype != torch.float64:
            raise ValueError(f"ref must be float64, not {ref.dtype}")
        if tuple(ref.shape) != shape:
            raise ValueError(f"ref must have shape {list(shape)}, not {list(ref.shape)}")
        return ref.to(self.device).contiguous()

    def stand_step(self, state, out=None, status=None, debug=False, ref=None):
        """Controller::standStep(ControllerInput{q,dq,time}) for all instances (controller.cpp:48-79).

        Updates state[:, 60:90] (Robot::v_) in place like the reference mutates its Robot.
        ref [B,16] (lmh_eval_ref; None: the built-in preview step): the CoM reference the momentum task tracks, xRef | yRef in words 0:6 --
        a record of mpc_step / mpc_box_step or a tick of their rollouts' traj as it stands.  Not with debug."""
        if ref is not None:
            if debug:
                raise ValueError("stand_step: ref has no debug-dump variant")
            ref = self._ref_records(ref, ())
        out = self.new_out() if out is None else out
        status = self.new_status() if status is None else status
        if ref is not None:
            check(capi.lib().lmh_eval_ref(self._h, _dev_ptr(state), _dev_ptr(ref), _dev_ptr(out), _dev_ptr(status), self._stream()))
            return out, status
        if debug:
            dbg = torch.zeros((self.B, capi.DEBUG_STRIDE), dtype=torch.float64, device=self.device)
            check(capi.lib().lmh_eval_debug(self._h, _dev_ptr(state), _dev_ptr(out), _dev_ptr(status), _dev_ptr(dbg), self._stream()))
            return out, status, dbg
        check(capi.lib().lmh_eval(self._h, _dev_ptr(state), _dev_ptr(out), _dev_ptr(status), self._stream()))
        return out, status

    def _rollout_buffers(self, n_ticks, out, status, log):
        """out, status and log of a rollout: the caller's, or fresh ones (log=True: a zeroed [n_ticks,B,36]; False: none)."""
        out = self.new_out() if out is None else out
        status = self.new_status() if status is None else status
        lg = torch.zeros((n_ticks, self.B, 36), dtype=torch.float64, device=self.device) if log is True else (log if log is not False else None)
        return out, status, lg

    def rollout(self, state, n_ticks, out=None, status=None, log=False):
        """n_ticks of rk4Step(dynamics) + Clock::step (apps/offline/main.cpp:66-122), fused on chip."""
        out, status, lg = self._rollout_buffers(n_ticks, out, status, log)
        check(capi.lib().lmh_rollout(self._h, _dev_ptr(state), _dev_ptr(out), _dev_ptr(status), _dev_ptr(lg), int(n_ticks), self._stream()))
        return out, status, lg

    def rollout_trace(self, state, n_ticks, every, out=None, status=None, log=False, trace=None):
        """lmh_rollout_trace: rollout that also stores a sample [state(96) | out(80) | status(4, as doubles)] of every robot each time it
        has completed `every` more ticks of this launch -- what rollout(state, (j + 1) * every) would have left, bit for bit.
        trace: a [n_ticks // every, B, 180] float64 device tensor (or larger), allocated here when None.  -> (out, status, log, trace)."""
        out, status, lg = self._rollout_buffers(n_ticks, out, status, log)
        if trace is None:
            trace = torch.zeros((capi.lib().lmh_trace_samples(int(n_ticks), int(every)), self.B, capi.TRACE_STRIDE), dtype=torch.float64, device=self.device)
        check(capi.lib().lmh_rollout_trace(self._h, _dev_ptr(state), _dev_ptr(out), _dev_ptr(status), _dev_ptr(lg),
                                           int(n_ticks), _dev_ptr(trace), int(every), self._stream()))
        return out, status, lg, trace

    @staticmethod
    def split_trace(trace):
        """Named views of a trace [.., 180] (tensor or array): state, q, v, v_prev, t, the split_out fields tau, f, qpp and com, com_vel,
        x_ref, y_ref, out; k, qp_iterations, flags, active_mask as integer tensors / arrays (exact: they were stored from int32)."""
        s, o, w = trace[..., 0:96], trace[..., 96:176], trace[..., 176:180]
        wi = w.to(torch.int64) if isinstance(w, torch.Tensor) else np.asarray(w).astype(np.int64)
        return dict(state=s, q=s[..., 0:30], v=s[..., 30:60], v_prev=s[..., 60:90], t=s[..., 90],
                    out=o, tau=o[..., 0:24], f=o[..., 24:36], qpp=o[..., 36:66], com=o[..., 66:69], com_vel=o[..., 69:72],
                    x_ref=o[..., 72:75], y_ref=o[..., 75:78],
                    k=wi[..., 0], qp_iterations=wi[..., 1], flags=wi[..., 2], active_mask=wi[..., 3])

    # ------------------------------------------------------------------ per-robot metrics (lmh_rollout_metrics)
    def new_metrics(self, z_min=-np.inf, tilt_max=np.inf):
        """A reset record per robot, [B,208] on the device.  z_min / tilt_max: the "down" thresholds on the base height and on |roll|,
        |pitch|, scalars or arrays of length B (-inf / inf: never down)."""
        m = torch.empty((self.B, capi.METRICS_STRIDE), dtype=torch.float64, device=self.device)
        return self.metrics_reset(m, z_min, tilt_max)

    def metrics_reset(self, metrics, z_min=-np.inf, tilt_max=np.inf):
        """lmh_metrics_reset: the identity record for every robot; arrays of length B then overwrite words 3 / 4 (stream-ordered)."""
        z, a = np.asarray(z_min, dtype=np.float64), np.asarray(tilt_max, dtype=np.float64)
        for name, v in (("z_min", z), ("tilt_max", a)):
            if v.ndim > 1 or (v.ndim == 1 and v.shape[0] != self.B):
                raise ValueError(f"{name} must be a scalar or an array of length {self.B}")
            if np.isnan(v).any():
                raise ValueError(f"{name} must not be NaN")
        check(capi.lib().lmh_metrics_reset(self._h, _dev_ptr(metrics), float(z) if z.ndim == 0 else -np.inf, float(a) if a.ndim == 0 else np.inf,
                                           self._stream()))
        for (off, _), v in ((capi.METRICS_FIELDS["z_min"], z), (capi.METRICS_FIELDS["tilt_max"], a)):
            if v.ndim == 1:
                metrics[:, off] = torch.as_tensor(v.copy()).to(self.device)
        return metrics

    def rollout_metrics(self, state, n_ticks, metrics, out=None, status=None, log=False):
        """lmh_rollout_metrics: rollout that also folds every tick into the robots' records (new_metrics); the records are not reset by
        the call, so consecutive launches accumulate.  -> (out, status, log)"""
        out, status, lg = self._rollout_buffers(n_ticks, out, status, log)
        check(capi.lib().lmh_rollout_metrics(self._h, _dev_ptr(state), _dev_ptr(out), _dev_ptr(status), _dev_ptr(lg), int(n_ticks),
                                             _dev_ptr(metrics), self._stream()))
        return out, status, lg

    @staticmethod
    def split_metrics(m):
        """Named views of records [.., 208] (tensor or array) by capi.METRICS_FIELDS; count, first_flag and first_fall as integers
        (exact: whole numbers in doubles; -1 = never)."""
        f = _split(m, capi.METRICS_FIELDS)
        for k in ("count", "first_flag", "first_fall"):
            f[k] = f[k].to(torch.int64) if isinstance(f[k], torch.Tensor) else np.asarray(f[k]).astype(np.int64)
        return f

    def synchronize(self):
        """lmh_synchronize on the current stream: waits for it, and raises LmhError (code ERR_UNFINISHED) if a completed rollout of this
        handle left robots part-way (they carry FLAG_UNFINISHED in their status records)."""
        check(capi.lib().lmh_synchronize(self._h, self._stream()))

    def ik(self, q, com_target=(-0.02, 0.0, 0.26), rf=(0, -0.05, 0, 0, 0, 0), lf=(0, 0.05, 0, 0, 0, 0)):
        """Kinematics::desiredOperationalState + compute (invKinematics.cpp:11-52); q [B,30] device tensor, in place."""
        iters = torch.zeros((self.B,), dtype=torch.int32, device=self.device)
        ct = np.ascontiguousarray(com_target, dtype=np.float64)
        r6 = np.ascontiguousarray(rf, dtype=np.float64); l6 = np.ascontiguousarray(lf, dtype=np.float64)
        check(capi.lib().lmh_ik(self._h, _dev_ptr(q), _np_ptr(ct), _np_ptr(r6), _np_ptr(l6), _dev_ptr(iters), self._stream()))
        return q, iters

    def ik_batch(self, q, targets):
        """lmh_ik_batch: per-robot targets, and sequences of them solved one after the other in one launch (target j from the solution
        of target j-1).  q [B,30] device tensor (left as it is); targets [B,16] or [n,B,16] records (trajectories.ik_targets /
        start_targets; array or tensor).  -> (q [n,B,30], iters [n,B] int32, crit [n,B]); [B,30], [B], [B] when targets is [B,16]."""
        q = self._batch("q", q, 30)
        t = torch.as_tensor(targets, dtype=torch.float64).to(self.device).contiguous()
        if t.ndim not in (2, 3) or tuple(t.shape[-2:]) != (self.B, capi.IK_TARGET_STRIDE):
            raise ValueError(f"targets must be [{self.B},{capi.IK_TARGET_STRIDE}] or [n,{self.B},{capi.IK_TARGET_STRIDE}]")
        lead = tuple(t.shape[:-1])
        n = 1 if t.ndim == 2 else int(t.shape[0])
        out = torch.zeros(lead + (30,), dtype=torch.float64, device=self.device)
        iters = torch.zeros(lead, dtype=torch.int32, device=self.device)
        crit = torch.zeros(lead, dtype=torch.float64, device=self.device)
        if n > 0:                                                  # (an empty tensor has no address to pass)
            check(capi.lib().lmh_ik_batch(self._h, _dev_ptr(q), _dev_ptr(t), n, _dev_ptr(out), _dev_ptr(iters), _dev_ptr(crit), self._stream()))
        return out, iters, crit

    def robot_com(self, q):
        """Robot::updateState + getCoM (Robot.cpp:264-269,225-238) for q [B,30] (device tensor) -> [B,3]."""
        com = torch.zeros((self.B, 3), dtype=torch.float64, device=self.device)
        check(capi.lib().lmh_robot_com(self._h, _dev_ptr(q), _dev_ptr(com), self._stream()))
        return com

    # -- rigid-body terms, inverse and forward dynamics (include/lmh.h, lmh_terms): pure functions of the (q, v) given
    def _batch(self, name, t, width, optional=False, in_place=False):
        """A [B,width] float64 tensor on this controller's device, made contiguous; None passes when optional.  in_place: the call writes
        into t itself, so it has to be contiguous as it comes."""
        if t is None:
            if optional:
                return None
            raise ValueError(f"{name} is required")
        what = f"[{self.B},{width}] float64 tensor on {self.device}"
        if in_place:
            what = f"contiguous {what} (it is updated in place)"
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or tuple(t.shape) != (self.B, width) or t.device != self.device \
                or (in_place and not t.is_contiguous()):
            raise ValueError(f"{name} must be a {what}")
        return t.contiguous()

    def terms(self, q, v=None):
        """Dynamics::computeAll + its getters, Kinematics::feetJacobian and Robot::getT / getCoM / getComVel / getComAngMom for q, v
        [B,30] (device tensors; v=None is v = 0) -> [B,1840], one record per robot (split_terms names its fields).  Every
        velocity-dependent term is taken at the v given."""
        q, v = self._batch("q", q, 30), self._batch("v", v, 30, optional=True)
        t = torch.empty((self.B, capi.TERMS_STRIDE), dtype=torch.float64, device=self.device)
        check(capi.lib().lmh_terms(self._h, _dev_ptr(q), _dev_ptr(v), _dev_ptr(t), self._stream()))
        return t

    def inverse_dynamics(self, q, v, qdd, w=None):
        """tau30 = M qdd + C - J'w -> [B,30]: rows 0..5 the residual wrench on the base, 6..29 the joint torques.  qdd is in the
        coordinates of M (include/lmh.h); w [B,12] has the layout of out.f (w=None: no contact wrench); v=None is v = 0."""
        q, v = self._batch("q", q, 30), self._batch("v", v, 30, optional=True)
        qdd, w = self._batch("qdd", qdd, 30), self._batch("w", w, 12, optional=True)
        tau = torch.empty((self.B, 30), dtype=torch.float64, device=self.device)
        check(capi.lib().lmh_inverse_dynamics(self._h, _dev_ptr(q), _dev_ptr(v), _dev_ptr(qdd), _dev_ptr(w), _dev_ptr(tau), self._stream()))
        return tau

    def forward_dynamics(self, q, v, tau, w=None):
        """Solves M qdd = tau30 + J'w - C -> (qdd [B,30], flags [B] int32: FLAG_NOT_SPD / FLAG_NONFINITE per robot)."""
        q, v = self._batch("q", q, 30), self._batch("v", v, 30, optional=True)
        tau, w = self._batch("tau", tau, 30), self._batch("w", w, 12, optional=True)
        qdd = torch.empty((self.B, 30), dtype=torch.float64, device=self.device)
        flags = torch.zeros((self.B,), dtype=torch.int32, device=self.device)
        check(capi.lib().lmh_forward_dynamics(self._h, _dev_ptr(q), _dev_ptr(v), _dev_ptr(tau), _dev_ptr(w), _dev_ptr(qdd), _dev_ptr(flags), self._stream()))
        return qdd, flags

    @staticmethod
    def split_terms(t):
        """Named views of terms records [.., 1840] (tensor or array): M [..,30,30], C, Cg (first six), AG [..,6,30], AGpqp, J [..,12,30],
        Jpqp, CoM, comVel, angMom, mass [..], T [..,28,3,4] -- capi.TERMS_FIELDS."""
        return _split(t, capi.TERMS_FIELDS)

    # -- torque-driven plant (include/lmh.h, lmh_contact_wrench): the compliant-contact plant under torques the caller supplies
    def contact_wrench(self, q, v=None):
        """The ground's forces on the soles for q, v [B,30] (device tensors; v=None is v = 0) -> [B,40], one record per robot
        (split_contact names its fields): the spring-damper contact of lmh_config.plant with the robot's own contact constants, against
        the robot's planes of set_ground when there is a table (trajectories.ground_contact states the model), else against z = 0."""
        q, v = self._batch("q", q, 30), self._batch("v", v, 30, optional=True)
        c = torch.empty((self.B, capi.CONTACT_STRIDE), dtype=torch.float64, device=self.device)
        check(capi.lib().lmh_contact_wrench(self._h, _dev_ptr(q), _dev_ptr(v), _dev_ptr(c), self._stream()))
        return c

    def plant_derivative(self, q, v, tau=None):
        """xdot of the plant for q, v [B,30] under tau [B,30] in the coordinates of M (rows 6..29 joint torques, rows 0..5 an external wrench
        on the base; None: a passive robot) -> (xdot [B,60], contact [B,40], flags [B] int32: FLAG_NOT_SPD / FLAG_NONFINITE per robot).
        xdot[:, :30] is qdot from v, xdot[:, 30:] solves M a = tau + J'w_c - C(q, v) (state ordering, world frame).  w_c is
        contact_wrench's: the planes of set_ground are honoured."""
        q, v, tau = self._batch("q", q, 30), self._batch("v", v, 30), self._batch("tau", tau, 30, optional=True)
        xdot = torch.empty((self.B, 60), dtype=torch.float64, device=self.device)
        c = torch.empty((self.B, capi.CONTACT_STRIDE), dtype=torch.float64, device=self.device)
        flags = torch.zeros((self.B,), dtype=torch.int32, device=self.device)
        check(capi.lib().lmh_plant_derivative(self._h, _dev_ptr(q), _dev_ptr(v), _dev_ptr(tau), _dev_ptr(xdot), _dev_ptr(c),
                                              _dev_ptr(flags), self._stream()))
        return xdot, c, flags

    def plant_step(self, state, tau=None, n_substeps=1):
        """n_substeps RK4 steps of cfg.dt on (q, v) of the state records [B,96], in place, with tau [B,30] held (None: passive); t advances,
        v_prev stays.  The planes of set_ground are honoured.  -> (state, flags [B] int32, OR-ed over the substeps)."""
        tau, state = self._batch("tau", tau, 30, optional=True), self._batch("state", state, capi.STATE_STRIDE, in_place=True)
        flags = torch.zeros((self.B,), dtype=torch.int32, device=self.device)
        check(capi.lib().lmh_plant_step(self._h, _dev_ptr(state), _dev_ptr(tau), _count("n_substeps", n_substeps), _dev_ptr(flags), self._stream()))
        return state, flags

    def plant_step_servo(self, state, setpoint, tau=None, n_substeps=1):
        """lmh_plant_step_servo: plant_step with the joint servo of set_servo re-forming the joint torques at every RK4 stage -- row 6 + j
        of tau becomes tau + (kp_j (q_des_j - q_j) + kd_j (v_des_j - v_j)) at the stage's own q and v (trajectories.servo_torque).
        setpoint [B,48] = q_des[24] | v_des[24], held for the launch; tau [B,30] the feed-forward torques (None: zero).  A handle without
        a servo table runs with zero gains.  -> (state, flags [B] int32, OR-ed over the substeps)."""
        tau, state = self._batch("tau", tau, 30, optional=True), self._batch("state", state, capi.STATE_STRIDE, in_place=True)
        setpoint = self._batch("setpoint", setpoint, capi.SETPOINT_STRIDE)
        flags = torch.zeros((self.B,), dtype=torch.int32, device=self.device)
        check(capi.lib().lmh_plant_step_servo(self._h, _dev_ptr(state), _dev_ptr(tau), _dev_ptr(setpoint), _count("n_substeps", n_substeps), _dev_ptr(flags), self._stream()))
        return state, flags

    # -- rigid-contact plant (include/lmh.h, lmh_plant_derivative_rigid): the held soles as constraints, the contact wrench their multiplier
    def _rigid_args(self, mode, kv):
        if mode is not None and (not isinstance(mode, torch.Tensor) or mode.dtype != torch.int32 or tuple(mode.shape) != (self.B,) or mode.device != self.device):
            raise ValueError(f"mode must be a [{self.B}] int32 tensor on {self.device}")
        return (None if mode is None else mode.contiguous()), float(kv)

    def plant_derivative_rigid(self, q, v, tau=None, mode=None, kv=0.0):
        """xdot of the rigid-contact plant for q, v [B,30] under tau [B,30] (None: passive): the soles that mode holds (int32 [B] of
        PHASE_DOUBLE / PHASE_RIGHT / PHASE_LEFT / PHASE_FLIGHT, low two bits; None: both soles of every robot) are kinematic constraints
        with the velocity-level stabilisation kv >= 0 [1/s] -> (xdot [B,60], lam [B,12] the contact wrench as the constraint's multiplier,
        laid out like out.f and exactly 0 on a free foot, flags [B] int32: FLAG_CONTACT_PULL / FLAG_CONTACT_SLIP (informational), FLAG_NOT_SPD,
        FLAG_NONFINITE).  trajectories.rigid_contact_acceleration states the acceleration; the call reads no ground and no servo table."""
        q, v, tau = self._batch("q", q, 30), self._batch("v", v, 30), self._batch("tau", tau, 30, optional=True)
        mode, kv = self._rigid_args(mode, kv)
        xdot = torch.empty((self.B, 60), dtype=torch.float64, device=self.device)
        lam = torch.empty((self.B, 12), dtype=torch.float64, device=self.device)
        flags = torch.zeros((self.B,), dtype=torch.int32, device=self.device)
        check(capi.lib().lmh_plant_derivative_rigid(self._h, _dev_ptr(q), _dev_ptr(v), _dev_ptr(tau), _dev_ptr(mode), kv, _dev_ptr(xdot), _dev_ptr(lam),
                                                    _dev_ptr(flags), self._stream()))
        return xdot, lam, flags

    def plant_step_rigid(self, state, tau=None, mode=None, kv=0.0, n_substeps=1):
        """n_substeps RK4 steps of cfg.dt of the rigid-contact plant on (q, v) of the state records [B,96], in place, with tau [B,30] held
        (None: passive); t advances, v_prev stays.  mode and kv as in plant_derivative_rigid.  -> (state, lam [B,12] the multiplier at the
        first stage of the last substep -- zeros when n_substeps is 0 --, flags [B] int32 OR-ed over every stage)."""
        tau, state = self._batch("tau", tau, 30, optional=True), self._batch("state", state, capi.STATE_STRIDE, in_place=True)
        mode, kv = self._rigid_args(mode, kv)
        if int(n_substeps) != n_substeps:
            raise ValueError("n_substeps must be a whole number")
        lam = torch.zeros((self.B, 12), dtype=torch.float64, device=self.device)
        flags = torch.zeros((self.B,), dtype=torch.int32, device=self.device)
        check(capi.lib().lmh_plant_step_rigid(self._h, _dev_ptr(state), _dev_ptr(tau), _dev_ptr(mode), kv, int(n_substeps), _dev_ptr(lam), _dev_ptr(flags), self._stream()))
        return state, lam, flags

    def plant_impact_rigid(self, q, v, mode=None):
        """lmh_plant_impact_rigid: the plastic impact of the rigid-contact plant at q, v [B,30] -- the velocity jumps to the nearest one, in
        the metric of M, at which every sole that mode holds (as in plant_derivative_rigid; None: both soles) is at rest -> (v_plus [B,30],
        impulse [B,12] laid out like out.f and exactly 0 on a free foot, flags [B] int32: FLAG_IMPULSE_PULL / FLAG_IMPULSE_SLIP
        (informational), FLAG_NOT_SPD, FLAG_NONFINITE).  PHASE_FLIGHT leaves v bit for bit.  trajectories.rigid_contact_impact states it."""
        q, v = self._batch("q", q, 30), self._batch("v", v, 30)
        mode, _ = self._rigid_args(mode, 0.0)
        v_plus = torch.empty((self.B, 30), dtype=torch.float64, device=self.device)
        impulse = torch.empty((self.B, 12), dtype=torch.float64, device=self.device)
        flags = torch.zeros((self.B,), dtype=torch.int32, device=self.device)
        check(capi.lib().lmh_plant_impact_rigid(self._h, _dev_ptr(q), _dev_ptr(v), _dev_ptr(mode), _dev_ptr(v_plus), _dev_ptr(impulse), _dev_ptr(flags), self._stream()))
        return v_plus, impulse, flags

    # -- zero-order-hold closed loop (include/lmh.h, lmh_rollout_zoh): the argument handling the seven calls share
    def _tick_records(self, name, v, n, tail, dtype=torch.float64, out=False, at_least=False, also=()):
        """Per-tick records [n,B,*tail] of a launch (or one of the whole shapes `also`; at_least: [m,B,*tail] with m >= n) -> (the tensor the
        caller is handed back, the tensor whose address is passed: a one-word placeholder when the first is empty, since an empty tensor has
        no address and with no tick no record is touched).  None and False are (None, None).  An input (out=False) may be an array of the
        dtype and is made contiguous; an output is written in place, so it is contiguous as it comes, and True allocates zeros."""
        if v is None or (v is False and out):
            return None, None
        shape = (n, self.B) + tuple(tail)
        if v is True and out:
            t = torch.zeros(shape, dtype=dtype, device=self.device)
        else:
            t = v
            if not out and isinstance(t, np.ndarray) and t.dtype == _NP_DTYPE[dtype]:
                t = torch.from_numpy(np.ascontiguousarray(t)).to(self.device)
            has = tuple(t.shape) if isinstance(t, torch.Tensor) else None
            fits = has == shape or has in also or (at_least and has is not None and len(has) == len(shape) and has[1:] == shape[1:] and has[0] >= n)
            if not fits or t.dtype != dtype or t.device != self.device or (out and not t.is_contiguous()):
                what = " or ".join(str(list(x)) for x in (shape,) + tuple(also)) + (" (or longer)" if at_least else "")
                raise ValueError(f"{name} must be a {'contiguous ' if out else ''}{what} {str(dtype)[6:]} tensor on {self.device}")
            if not out:
                t = t.contiguous()
        return t, (t if t.numel() > 0 else torch.empty((1,), dtype=dtype, device=self.device))

    def rollout_zoh(self, state, n_ticks, n_substeps, base_wrench=None, log=False, out=None, status=None, ref=None):
        """lmh_rollout_zoh: n_ticks rounds of { stand_step ; plant_step([base_wrench | out.tau], n_substeps) } in one launch, bit for bit
        what that loop leaves; state [B,96] is updated in place.  The control period is n_substeps * cfg.dt.  base_wrench [B,6]: an external
        wrench on the base held for the launch ([angular | linear], base frame; None: zero).  status (given or fresh): [:, 3] is the active
        mask a warm-started handle continues from; afterwards [:, 1] is the maximum of the QP rounds and [:, 2] the OR of the controller's
        and the plant's flags over all ticks.  ref [n_ticks,B,16] (lmh_rollout_zoh_ref; None: the built-in preview step): record j is the
        CoM reference of control tick j of this launch, as in stand_step(ref=...) -- the traj of mpc_rollout / mpc_box_rollout as it stands.
        With a set_ground table the holds are plant_step's on that ground (so the loop statement holds as it reads), here and in
        rollout_zoh_ex and rollout_zoh_io; the evaluation is not told about the ground.
        -> (out, status), plus the log [n_ticks,B,36] (tau | f of every tick) when log is asked for."""
        state, bw = self._batch("state", state, capi.STATE_STRIDE, in_place=True), self._batch("base_wrench", base_wrench, 6, optional=True)
        n, ns = _count("n_ticks", n_ticks), _count("n_substeps", n_substeps)
        out, status, lg = self._rollout_buffers(n, out, status, log)
        args = (self._h, _dev_ptr(state), _dev_ptr(out), _dev_ptr(status), _dev_ptr(bw), _dev_ptr(lg))
        if ref is not None:
            ref = self._tick_records("ref", self._ref_records(ref, (n,)), n, (capi.MPC_STRIDE,))[1]
            check(capi.lib().lmh_rollout_zoh_ref(*args, _dev_ptr(ref), n, ns, self._stream()))
        else:
            check(capi.lib().lmh_rollout_zoh(*args, n, ns, self._stream()))
        return (out, status) if lg is None else (out, status, lg)

    def rollout_zoh_ex(self, state, n_ticks, n_substeps, base_wrench=None, ref=None, pushes=False, log=False, trace_every=0, trace=None,
                       metrics=None, out=None, status=None):
        """lmh_rollout_zoh_ex: rollout_zoh with the set_pushes schedule applied (pushes=True; push ticks are plant substeps of cfg.dt on the
        robot's clock, trajectories.zoh_hold_pieces states where each one falls), a wrench per control tick (base_wrench [n_ticks,B,6]
        instead of [B,6]), a trace (trace_every > 0: a sample [state | out | status] of every robot each time it has completed that many
        control ticks, as rollout_trace lays it out; trace: a [n_ticks // trace_every, B, 180] device tensor, allocated here when None;
        write_trace's sample_dt is trace_every * n_substeps * cfg.dt) and a metrics record (metrics: new_metrics' [B,208], folded once per
        control tick at the tick's end; the records accumulate over launches).  With none of them the call is rollout_zoh's launch.
        -> dict(out, status, log, trace); log and trace are None when not asked for."""
        return self._zoh_launch(state, n_ticks, n_substeps, dict(base_wrench=base_wrench, ref=ref, pushes=pushes, log=log, trace_every=trace_every, trace=trace,
                                                                 metrics=metrics, out=out, status=status), capi.lib().lmh_rollout_zoh_ex)

    def rollout_zoh_box(self, state, box, n_ticks, n_substeps, mpc=True, base_wrench=None, pushes=False, log=False, trace_every=0, trace=None,
                        metrics=None, out=None, status=None, ref=None):
        """lmh_rollout_zoh_box: rollout_zoh_ex with the box-constrained preview step closed around the measured CoM inside every control tick
        -- bit for bit the host loop { lip_from_out(stand_step on a scratch copy) ; mpc_box_step ; stand_step(ref=) ; plant_step } -- on one
        factorisation per launch.  box as mpc_box_step takes it ([4,n_samples] or [B,4,n_samples]).  mpc=True: the samples [n_ticks,B,16] of
        every tick's constrained step (split_mpc; word 15: the active samples) are returned under "mpc"; False: not stored; a tensor: filled.
        There is no ref: a reference and the box step are exclusive.  Refused on a handle with a set_ground table.
        -> rollout_zoh_ex's dict plus mpc."""
        if ref is not None:
            raise ValueError("rollout_zoh_box takes no ref: the box-constrained step is the reference (the two are exclusive)")
        bx, ns, sets = self._box(box)
        tr, tr_arg = self._tick_records("mpc", mpc, _count("n_ticks", n_ticks), (capi.MPC_STRIDE,), out=True, at_least=True)
        res = self._zoh_launch(state, n_ticks, n_substeps, dict(base_wrench=base_wrench, pushes=pushes, log=log, trace_every=trace_every, trace=trace, metrics=metrics,
                                                                out=out, status=status), capi.lib().lmh_rollout_zoh_box, _dev_ptr(bx), ns, sets, _dev_ptr(tr_arg))
        res["mpc"] = tr
        return res

    def _zoh_io(self, n, meas=None, actuators=False, act_mem=None, applied=False):
        """rollout_zoh_io's own arguments for a launch of n ticks -> (lmh_zoh_io record, the applied tensor or None)"""
        ms = self._tick_records("meas", meas, n, (60,))[1]
        ap, ap_arg = self._tick_records("applied", applied, n, (24,), out=True)
        if actuators and act_mem is None:
            raise ValueError("rollout_zoh_io: actuators=True needs act_mem (new_act_mem)")
        mem = self._batch("act_mem", act_mem, capi.ACT_MEM_STRIDE, optional=True, in_place=True)
        io = capi.LmhZohIo(d_meas=_dev_ptr(ms), d_act_mem=_dev_ptr(mem), d_applied=_dev_ptr(ap_arg), actuators=int(bool(actuators)), reserved=0)
        io.keep = (ms, mem, ap_arg)                                # (the record holds addresses only)
        return io, ap

    def _zoh_io_launch(self, state, n, n_substeps, kw, call, *records):
        """The calls that take rollout_zoh_io's keywords as they are (kw: its own arguments and rollout_zoh_ex's options together) with
        records of their own behind the io record -> rollout_zoh_ex's dict plus applied."""
        io, ap = self._zoh_io(n, kw.pop("meas", None), kw.pop("actuators", False), kw.pop("act_mem", None), kw.pop("applied", False))
        res = self._zoh_launch(state, n, n_substeps, kw, call, C.byref(io), *[C.byref(r) for r in records])
        res["applied"] = ap
        return res

    def rollout_zoh_servo(self, state, n_ticks, n_substeps, servo="integrate", **io):
        """lmh_rollout_zoh_servo: rollout_zoh_io (whose keywords it takes as they are) with the joint servo of set_servo inside every hold
        -- bit for bit that call's host loop with plant_step_servo in the place of plant_step.  servo="integrate": the setpoint of a
        control tick is where the evaluation's own joint accelerations take the joints it read by the end of the control period
        (trajectories.servo_setpoint; needs n_substeps > 0); a tensor [n_ticks,B,48]: the caller's setpoint for every control tick and
        robot; None: no servo, rollout_zoh_io's launch.  log and applied keep the commanded and the feed-forward torques: the PD part
        changes at every RK4 stage and is not recorded.  -> rollout_zoh_io's dict."""
        n = _count("n_ticks", n_ticks)
        if isinstance(servo, str) and servo != "integrate":
            raise ValueError('servo must be "integrate", a setpoint tensor [n_ticks,B,48] or None')
        sp = None if isinstance(servo, str) else self._tick_records("servo", servo, n, (capi.SETPOINT_STRIDE,))[1]
        mode = 0 if servo is None else capi.SERVO_INTEGRATE if sp is None else capi.SERVO_CALLER
        return self._zoh_io_launch(state, n, n_substeps, io, capi.lib().lmh_rollout_zoh_servo, capi.LmhZohServo(d_setpoint=_dev_ptr(sp), mode=mode, reserved=0))

    def rollout_zoh_rigid(self, state, n_ticks, n_substeps, mode=None, kv=0.0, lam=False, impact=None, impulse=False, **io):
        """lmh_rollout_zoh_rigid: rollout_zoh_io (whose keywords it takes as they are) with the rigid-contact plant in every hold -- bit for
        bit that call's host loop with plant_step_rigid(mode_j, kv) in the place of plant_step.  mode: None, both soles of every robot held
        for the launch; an int32 [B] tensor of PHASE_* words, held for the launch; an int32 [n_ticks,B] tensor, record j is control tick
        j's hold; "plan": the support phase of the robot's own plan at the preview index that tick's evaluation reports
        (trajectories.rigid_modes).  One mode serves every piece of a tick's hold.  lam=True: the multipliers [n_ticks,B,12] at the first
        stage of the last substep of every tick's hold are returned under "lam" (a tensor: filled).  The contact stays bilateral
        (include/lmh.h); the ground and servo tables are not read.
        impact=None: there is no impact model, a sole that becomes held while it moves loses its twist as e^(-kv t).  impact: an int32 [B]
        tensor, the mode of the hold before this launch's first tick (lmh_rollout_zoh_rigid_impact's d_mode_prev, updated in place to the
        last tick's mode and handed on from launch to launch): every tick whose mode holds a foot the hold before it did not runs
        plant_impact_rigid on the true state in front of its hold.  impulse=True: the impulses [n_ticks,B,12], zeros on a tick without a
        touchdown, are returned under "impulse" (a tensor: filled); only with impact.  -> rollout_zoh_io's dict plus lam (and impulse)."""
        n = _count("n_ticks", n_ticks)
        if isinstance(mode, str) and mode != "plan":
            raise ValueError('mode must be None, an int32 [B] or [n_ticks,B] tensor, or "plan"')
        if impact is None and impulse is not False:
            raise ValueError("impulse goes with impact (the int32 [B] tensor of the modes before the launch) only")
        if impact is not None and (not isinstance(impact, torch.Tensor) or impact.dtype != torch.int32):
            raise ValueError("impact must be None or a contiguous [B] int32 tensor on the handle's device")
        md = None if isinstance(mode, str) else self._tick_records("mode", mode, n, (), dtype=torch.int32, also=((self.B,),))[1]
        source = capi.RIGID_PLAN if isinstance(mode, str) else capi.RIGID_PER_TICK if (md is not None and mode.ndim == 2) else capi.RIGID_FIXED
        lm, lm_arg = self._tick_records("lam", lam, n, (12,), out=True)
        rg = capi.LmhZohRigid(d_mode=_dev_ptr(md), d_lambda=_dev_ptr(lm_arg), kv=float(kv), source=source, reserved=0)
        if impact is None:
            res = self._zoh_io_launch(state, n, n_substeps, io, capi.lib().lmh_rollout_zoh_rigid, rg)
        else:
            if tuple(impact.shape) != (self.B,) or impact.device != self.device or not impact.is_contiguous():
                raise ValueError(f"impact must be a contiguous [{self.B}] int32 tensor on {self.device}")
            ip, ip_arg = self._tick_records("impulse", impulse, n, (12,), out=True)
            im = capi.LmhZohImpact(d_mode_prev=_dev_ptr(impact), d_impulse=_dev_ptr(ip_arg), enable=1, reserved=0)
            res = self._zoh_io_launch(state, n, n_substeps, io, capi.lib().lmh_rollout_zoh_rigid_impact, rg, im)
            res["impulse"] = ip
        res["lam"] = lm
        return res

    def rollout_zoh_io(self, state, n_ticks, n_substeps, meas=None, actuators=False, act_mem=None, applied=False, **ex):
        """lmh_rollout_zoh_io: rollout_zoh_ex (whose keywords it takes as they are) with sensing and actuation between controller and plant.
        meas [n_ticks,B,60]: what is added to q | v as control tick j's evaluation sees them (the plant goes on from the true state; v_prev
        keeps the measured v).  actuators=True: the set_actuators records -- latency, torque limit, first-order lag -- stand between the
        evaluation's torques and the hold, with act_mem (new_act_mem's [B,192], changed in place and handed on from launch to launch;
        required).  applied=True: the torques the plant received [n_ticks,B,24] are returned under "applied" (a tensor: filled).  log, trace
        and metrics keep the COMMANDED torques; status[:, 2] & capi.FLAG_TAU_LIMIT: a torque was cut.  With none of the four the call is
        rollout_zoh_ex's launch.  trajectories.actuator_step states the actuator.  -> rollout_zoh_ex's dict plus applied."""
        n = _count("n_ticks", n_ticks)
        io, ap = self._zoh_io(n, meas, actuators, act_mem, applied)
        res = self._zoh_launch(state, n, n_substeps, ex, capi.lib().lmh_rollout_zoh_io, C.byref(io))
        res["applied"] = ap
        return res

    def _zoh_launch(self, state, n_ticks, n_substeps, kw, call, *own):
        """The one launch of rollout_zoh_ex, _box, _io, _servo and _rigid: forms lmh_zoh_opts from kw, rollout_zoh_ex's option keywords (another
        name is a TypeError), and makes the C call `call` with `own`, the arguments it has between the options and the counts.
        -> dict(out, status, log, trace)"""
        if not kw.keys() <= _ZOH_OPTIONS.keys():
            raise TypeError(f"{call.__name__[4:]}: unexpected keyword {sorted(kw.keys() - _ZOH_OPTIONS.keys())[0]!r}")
        o = {**_ZOH_OPTIONS, **kw}
        state = self._batch("state", state, capi.STATE_STRIDE, in_place=True)
        n, ns, every = _count("n_ticks", n_ticks), _count("n_substeps", n_substeps), _count("trace_every", o["trace_every"])
        per_tick = getattr(o["base_wrench"], "ndim", 0) == 3
        bw = self._tick_records("base_wrench", o["base_wrench"], n, (6,))[1] if per_tick else self._batch("base_wrench", o["base_wrench"], 6, optional=True)
        trace = tr_arg = None
        if o["trace"] is not None or every > 0:                    # the kernel writes lmh_trace_samples records: a smaller buffer is an out-of-bounds write
            trace, tr_arg = self._tick_records("trace", True if o["trace"] is None else o["trace"], capi.lib().lmh_trace_samples(n, every), (capi.TRACE_STRIDE,),
                                               out=True, at_least=True)
        out, status, lg = self._rollout_buffers(n, o["out"], o["status"], o["log"])
        ref = None if o["ref"] is None else self._tick_records("ref", self._ref_records(o["ref"], (n,)), n, (capi.MPC_STRIDE,))[1]
        metrics = self._batch("metrics", o["metrics"], capi.METRICS_STRIDE, optional=True, in_place=True)
        opts = capi.LmhZohOpts(d_base_wrench=_dev_ptr(bw), d_ref=_dev_ptr(ref), d_log=_dev_ptr(lg), d_trace=_dev_ptr(tr_arg), d_metrics=_dev_ptr(metrics),
                               trace_every=every, wrench_per_tick=int(per_tick), pushes=int(bool(o["pushes"])), reserved=0)
        check(call(self._h, _dev_ptr(state), _dev_ptr(out), _dev_ptr(status), C.byref(opts), *own, n, ns, self._stream()))
        return dict(out=out, status=status, log=lg, trace=trace)

    @staticmethod
    def split_contact(c):
        """Named views of contact records [.., 40] (tensor or array): w [..,12] (n_R f_R n_L f_L), vertex_force [..,8,3], pad [..,4] --
        capi.CONTACT_FIELDS."""
        return _split(c, capi.CONTACT_FIELDS)

    # -- LIPM preview MPC (include/lmh.h, lmh_mpc_step): the MPC stage of the controller on reduced states, as calls of its own
    def new_lip(self, com_xy=(0.0, 0.0), vel_xy=(0.0, 0.0), t=0.0):
        """LIP state records [B,8]: x | xdot | y | ydot | t | pad.  com_xy, vel_xy: [2] or [B,2]; t: a scalar or [B]."""
        lip = np.zeros((self.B, capi.LIP_STRIDE))
        lip[:, [0, 2]] = np.broadcast_to(np.asarray(com_xy, dtype=np.float64), (self.B, 2))
        lip[:, [1, 3]] = np.broadcast_to(np.asarray(vel_xy, dtype=np.float64), (self.B, 2))
        lip[:, 4] = np.broadcast_to(np.asarray(t, dtype=np.float64), (self.B,))
        return torch.as_tensor(lip).to(self.device)

    def mpc_step(self, lip):
        """lmh_mpc_step: Mpc3dLip::compute for every robot at its own clock; lip [B,8] (left as it is) -> samples [B,16] (split_mpc)."""
        lip = self._batch("lip", lip, capi.LIP_STRIDE)
        rec = torch.empty((self.B, capi.MPC_STRIDE), dtype=torch.float64, device=self.device)
        check(capi.lib().lmh_mpc_step(self._h, _dev_ptr(lip), _dev_ptr(rec), self._stream()))
        return rec

    def mpc_rollout(self, lip, n_ticks, traj=True):
        """lmh_mpc_rollout: n_ticks MPC steps of the reduced model in closed loop, in one launch; lip [B,8] is updated in place.
        traj=True: -> the samples [n_ticks,B,16]; False: -> None (only the final state); a tensor: filled and returned."""
        lip = self._batch("lip", lip, capi.LIP_STRIDE, in_place=True)
        n = _count("n_ticks", n_ticks)
        tr = torch.zeros((n, self.B, capi.MPC_STRIDE), dtype=torch.float64, device=self.device) if traj is True else (traj if traj is not False else None)
        if tr is not None and (tr.dtype != torch.float64 or tr.device != self.device or not tr.is_contiguous() or tr.numel() < n * self.B * capi.MPC_STRIDE):
            raise ValueError(f"traj must be a contiguous [{n},{self.B},{capi.MPC_STRIDE}] float64 tensor on {self.device}")
        if n > 0:                                                  # (an empty tensor has no address to pass)
            check(capi.lib().lmh_mpc_rollout(self._h, _dev_ptr(lip), n, _dev_ptr(tr), self._stream()))
        return tr

    def mpc_preview(self, lip):
        """lmh_mpc_preview: the whole unconstrained solution over the horizon at every robot's state; lip [B,8] (left as it is) ->
        records [B,536] (split_preview)."""
        lip = self._batch("lip", lip, capi.LIP_STRIDE)
        rec = torch.empty((self.B, capi.MPC_PREVIEW_STRIDE), dtype=torch.float64, device=self.device)
        check(capi.lib().lmh_mpc_preview(self._h, _dev_ptr(lip), _dev_ptr(rec), self._stream()))
        return rec

    # -- the box-constrained preview MPC (include/lmh.h, lmh_mpc_box_preview): the predicted ZMP kept inside per-sample bounds
    def _box(self, box):
        """box: [4,n_samples] (shared) or [B,4,n_samples] (per robot), rows lo_x | hi_x | lo_y | hi_y in metres (trajectories.zmp_box /
        zmp_boxes), a tensor or an array -> (contiguous float64 device tensor, n_samples, n_sets)."""
        t = box if isinstance(box, torch.Tensor) else torch.as_tensor(np.array(box, dtype=np.float64))
        if t.ndim == 2:
            t = t.unsqueeze(0)
        if t.ndim != 3 or t.shape[1] != 4 or t.shape[0] not in (1, self.B) or t.dtype != torch.float64:
            raise ValueError(f"box must be float64 [4,n_samples] or [{self.B},4,n_samples]")
        return t.to(self.device).contiguous(), int(t.shape[2]), int(t.shape[0])

    def mpc_box_step(self, lip, box):
        """lmh_mpc_box_step: the MPC step with the predicted ZMP held inside `box` over the horizon; lip [B,8] (left as it is) ->
        samples [B,16] (split_mpc; word 15: the active samples of both axes)."""
        lip = self._batch("lip", lip, capi.LIP_STRIDE)
        bx, ns, sets = self._box(box)
        rec = torch.empty((self.B, capi.MPC_STRIDE), dtype=torch.float64, device=self.device)
        check(capi.lib().lmh_mpc_box_step(self._h, _dev_ptr(lip), _dev_ptr(bx), ns, sets, _dev_ptr(rec), self._stream()))
        return rec

    def mpc_box_rollout(self, lip, box, n_ticks, traj=True):
        """lmh_mpc_box_rollout: n_ticks constrained steps of the reduced model in closed loop, in one launch on one factorisation;
        lip [B,8] is updated in place.  traj as in mpc_rollout."""
        lip = self._batch("lip", lip, capi.LIP_STRIDE, in_place=True)
        n = _count("n_ticks", n_ticks)
        bx, ns, sets = self._box(box)
        tr = torch.zeros((n, self.B, capi.MPC_STRIDE), dtype=torch.float64, device=self.device) if traj is True else (traj if traj is not False else None)
        if tr is not None and (tr.dtype != torch.float64 or tr.device != self.device or not tr.is_contiguous() or tr.numel() < n * self.B * capi.MPC_STRIDE):
            raise ValueError(f"traj must be a contiguous [{n},{self.B},{capi.MPC_STRIDE}] float64 tensor on {self.device}")
        if n > 0:
            check(capi.lib().lmh_mpc_box_rollout(self._h, _dev_ptr(lip), _dev_ptr(bx), ns, sets, n, _dev_ptr(tr), self._stream()))
        return tr

    def mpc_box_preview(self, lip, box):
        """lmh_mpc_box_preview: the whole constrained solution over the horizon with its multipliers; lip [B,8] (left as it is) ->
        records [B,668] (split_box_preview)."""
        lip = self._batch("lip", lip, capi.LIP_STRIDE)
        bx, ns, sets = self._box(box)
        rec = torch.empty((self.B, capi.MPC_BOX_STRIDE), dtype=torch.float64, device=self.device)
        check(capi.lib().lmh_mpc_box_preview(self._h, _dev_ptr(lip), _dev_ptr(bx), ns, sets, _dev_ptr(rec), self._stream()))
        return rec

    @staticmethod
    def split_box_preview(rec, N=None):
        """Named views of constrained preview records [.., 668]: what split_preview gives of the first 536 words, rounds_x, rounds_y,
        active_x, active_y as integers and the multipliers lam_x, lam_y (N + 1 entries: > 0 at an upper bound, < 0 at a lower one, 0 at
        an inactive sample) -- capi.MPC_BOX_HEADER, capi.MPC_BOX_ARRAYS."""
        as_int = (lambda v: v.to(torch.int64)) if isinstance(rec, torch.Tensor) else (lambda v: np.asarray(v).astype(np.int64))
        f = BatchedController.split_preview(rec, N)
        N = f["U_x"].shape[-1] - 1
        for name, off in capi.MPC_BOX_HEADER.items():
            f[name] = as_int(rec[..., off])
        for name in ("lam_x", "lam_y"):
            off, extra = capi.MPC_BOX_ARRAYS[name]
            f[name] = rec[..., off:off + N + extra]
        return f

    @staticmethod
    def split_mpc(rec):
        """Named views of MPC samples [.., 16] (tensor or array): x_ref [..,3], y_ref [..,3], zmp [..,2], state [..,4], t, and k, flags as
        integers (exact: whole numbers in doubles) -- capi.MPC_FIELDS."""
        f = _split(rec, capi.MPC_FIELDS)
        for k in ("k", "flags"):
            f[k] = f[k].to(torch.int64) if isinstance(f[k], torch.Tensor) else np.asarray(f[k]).astype(np.int64)
        return f

    @staticmethod
    def split_preview(rec, N=None):
        """Named views of preview records [.., 536] (tensor or array): k, flags, N as integers and the eight arrays U_x, U_y, Z_x, Z_y
        (N + 1 entries) and C_x, Cv_x, C_y, Cv_y (N + 2) cut to their used length -- capi.MPC_PREVIEW_ARRAYS.  N: the horizon (taken from
        the first record's header when None)."""
        as_int = (lambda v: v.to(torch.int64)) if isinstance(rec, torch.Tensor) else (lambda v: np.asarray(v).astype(np.int64))
        f = dict(k=as_int(rec[..., 0]), flags=as_int(rec[..., 1]), N=as_int(rec[..., 2]))
        if N is None:
            N = int(f["N"].reshape(-1)[0])
        for name, (off, extra) in capi.MPC_PREVIEW_ARRAYS.items():
            f[name] = rec[..., off:off + N + extra]
        return f

    def make_summary(self, state, out, status):
        """End-of-run summary [B,16] (include/lmh.h lmh_make_summary): the record the RCCL gather moves."""
        s = torch.empty((self.B, capi.SUMMARY_WIDTH), dtype=torch.float64, device=self.device)
        check(capi.lib().lmh_make_summary(self._h, _dev_ptr(state), _dev_ptr(out), _dev_ptr(status), _dev_ptr(s), self._stream()))
        return s

    @staticmethod
    def _write_record(write, path, name, a, shape, *scalars):
        """One writer for the three record files: a as a float64 array of the rank and record width of shape, e.g. ("ticks", "B", 36)."""
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.ndim != len(shape) or a.shape[-1] != shape[-1]:
            raise ValueError(f"{name} must be [{','.join(map(str, shape))}]")
        check(write(str(path).encode(), _np_ptr(a), *a.shape[:-1], *map(float, scalars)))

    @staticmethod
    def _read_record(read, path, width, per_tick=True):
        """One reader: the header alone (no buffer), then the payload -> (array, dt, t0).  A summary (per_tick=False) has no tick count, no t0."""
        nt, n, dt, t0 = C.c_uint64(0), C.c_uint64(0), C.c_double(0.0), C.c_double(0.0)
        header = (C.byref(nt), C.byref(n), C.byref(dt), C.byref(t0)) if per_tick else (C.byref(n), C.byref(dt))
        check(read(str(path).encode(), None, 0, *header))
        a = np.zeros((nt.value, n.value, width) if per_tick else (n.value, width), dtype=np.float64)
        check(read(str(path).encode(), _np_ptr(a), a.size, *header))
        return a, dt.value, t0.value

    @staticmethod
    def write_summary(path, summary, dt=0.0):
        """lmh_write_summary: [n,16] host array -> 64-byte header + raw f64 file."""
        BatchedController._write_record(capi.lib().lmh_write_summary, path, "summary", summary, ("n", capi.SUMMARY_WIDTH), dt)

    @staticmethod
    def read_summary(path):
        return BatchedController._read_record(capi.lib().lmh_read_summary, path, capi.SUMMARY_WIDTH, per_tick=False)[:2]

    @staticmethod
    def write_log(path, log, dt, t0=0.0):
        """lmh_write_log: [n_ticks,B,36] host array (lmh_rollout's d_log copied back)."""
        BatchedController._write_record(capi.lib().lmh_write_log, path, "log", log, ("ticks", "B", 36), dt, t0)

    @staticmethod
    def read_log(path):
        return BatchedController._read_record(capi.lib().lmh_read_log, path, 36)

    @staticmethod
    def write_trace(path, trace, sample_dt, t0=0.0):
        """lmh_write_trace: [n_samples,B,180] host array (lmh_rollout_trace's d_trace copied back); sample_dt = every * dt, t0 = the
        clock of the first sample.  A trace of rollout_zoh_ex: sample_dt = trace_every * n_substeps * dt."""
        BatchedController._write_record(capi.lib().lmh_write_trace, path, "trace", trace, ("samples", "B", capi.TRACE_STRIDE), sample_dt, t0)

    @staticmethod
    def read_trace(path):
        return BatchedController._read_record(capi.lib().lmh_read_trace, path, capi.TRACE_STRIDE)

    @staticmethod
    def split_out(out):
        """WBCOutput fields: tau [B,24], f [B,12] (n_R f_R n_L f_L), qpp [B,30]."""
        return out[:, 0:24], out[:, 24:36], out[:, 36:66]


# debug-dump layout (LMH_DEBUG_STRIDE record, see controller_eval in lmh_kernels.hip)
DEBUG_FIELDS = {
    "T": (0, (28, 3, 4)), "XE": (336, (28, 3, 3)), "Xp": (588, (28, 3)), "XB": (672, (28, 3, 3)),
    "C": (924, (30,)), "Cg6": (954, (6,)), "Mtop": (960, (6, 30)), "Hl": (1140, (24, 6)),
    "AG": (1284, (6, 30)), "AGpqp": (1464, (6,)), "Jpqp": (1470, (12,)), "Jc": (1482, (2, 6, 12)),
    "CoM": (1626, (3,)), "comVel": (1629, (3,)), "angMom": (1632, (3,)), "mpc": (1635, (8,)),
    "qppRef": (1643, (30,)), "hGpRef": (1673, (6,)), "footAccRef": (1679, (12,)),
    "Y": (1691, (30, 7)), "Si": (1901, (6, 6)), "W": (1937, (12, 12)), "h12": (2081, (12,)),
    "P": (2093, (32, 32)), "qv": (3117, (32,)), "c": (3149, (32,)), "a": (3181, (30,)),
}


def lip_from_out(out, t):
    """The LIP records [B,8] (x | xdot | y | ydot | t | pad) of out records [B,80] (tensor or array): the CoM and its velocity an evaluation
    measured, out[66] | out[69] | out[67] | out[70], at the clock(s) t (a scalar or [B]: state[:, 90]) -- what mpc_box_step takes in a host loop
    that closes the constrained step around the whole-body controller (rollout_zoh_box is that loop in one launch)."""
    if isinstance(out, torch.Tensor):
        lip = torch.zeros((out.shape[0], capi.LIP_STRIDE), dtype=out.dtype, device=out.device)
        lip[:, 0:4] = out[:, [66, 69, 67, 70]]
        lip[:, 4] = torch.as_tensor(t, dtype=out.dtype, device=out.device)
        return lip
    out = np.asarray(out)
    lip = np.zeros((out.shape[0], capi.LIP_STRIDE), dtype=out.dtype)
    lip[:, 0:4] = out[:, [66, 69, 67, 70]]
    lip[:, 4] = np.broadcast_to(np.asarray(t, dtype=out.dtype), (out.shape[0],))
    return lip


def unpack_debug(dbg_row):
    """numpy views of one instance's debug record."""
    return _split(np.asarray(dbg_row), DEBUG_FIELDS)
