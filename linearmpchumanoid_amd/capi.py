"""ctypes binding of the C ABI in include/lmh.h (linearmpchumanoid_amd/liblmh_hip.so).

The library is hand-written HIP for gfx950; there is no CPU implementation behind it.  If the
shared object is missing this module raises at load time -- it never falls back to anything.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# LMH_DIAG=1 selects the diagnostic build of the same sources (in-kernel phase stamps, scripts/gpu_phase_stamps.py)
# LMH_VARIANT=name selects an experiment build (linearmpchumanoid_amd/build.py); neither is the shipped library
_VAR = os.environ.get("LMH_VARIANT", "").split(":")[0]
SO_PATH = os.path.join(_HERE, "liblmh_hip_diag.so" if os.environ.get("LMH_DIAG") == "1" else ("liblmh_hip_var_%s.so" % _VAR if _VAR else "liblmh_hip.so"))

STATE_STRIDE = 96
OUT_STRIDE = 80
STATUS_STRIDE = 4
DEBUG_STRIDE = 4096
LINK_STRIDE = 13
SEG_STRIDE = 52
PUSH_STRIDE = 32              # one timed velocity push: tick (as a double) | dv[30] | pad (lmh_set_pushes)
MAX_PUSHES = 16               # push records per robot
ACT_STRIDE = 56               # one actuator record: tau_max[24] | alpha[24] | delay | pad (lmh_set_actuators)
ACT_OFF_TAU_MAX, ACT_OFF_ALPHA, ACT_OFF_DELAY = 0, 24, 48
ACT_MAX_DELAY = 7             # control ticks
ACT_MEM_STRIDE = 192          # one robot's actuator memory: PREV[24] | QUEUE[7][24], oldest command first (lmh_rollout_zoh_io)
SERVO_STRIDE = 48             # one servo record: kp[24] | kd[24] (lmh_set_servo)
SERVO_OFF_KP, SERVO_OFF_KD = 0, 24
SETPOINT_STRIDE = 48          # one setpoint record: q_des[24] | v_des[24] (lmh_plant_step_servo, lmh_rollout_zoh_servo)
SERVO_INTEGRATE, SERVO_CALLER = 1, 2      # lmh_zoh_servo.mode (0: off)
RIGID_FIXED, RIGID_PER_TICK, RIGID_PLAN = 1, 2, 3     # lmh_zoh_rigid.source (0: off)
GROUND_STRIDE = 8             # one ground record: n_R(3) | h_R | n_L(3) | h_L, the half space n.x <= h under each foot (lmh_set_ground)
GROUND_OFF_N_R, GROUND_OFF_H_R, GROUND_OFF_N_L, GROUND_OFF_H_L = 0, 3, 4, 7
IK_TARGET_STRIDE = 16         # one inverse-kinematics target record: rf6 | lf6 | com(3) | pad (lmh_ik_batch)
PARAM_STRIDE = 20             # one per-robot parameter record (lmh_set_params)
# name -> offset inside a parameter record: the LMH_PARAM_OFF_* defines of include/lmh.h (lmh_config's own order; [19] is a pad)
PARAM_FIELDS = {
    "mu": 0, "kp_joints": 1, "kd_joints": 2, "kp_mom": 3, "kd_mom": 4, "kp_feet": 5, "kd_feet": 6,
    "w_com_lin": 7, "w_com_ang": 8, "w_base_pos": 9, "w_base_ang": 10, "w_joints": 11, "w_force": 12, "w_foot": 13,
    "eps_coeff": 14, "contact_k": 15, "contact_d": 16, "contact_dt": 17, "contact_mu": 18,
}
TRACE_STRIDE = 180            # one trace sample: state(96) | out(80) | status(4, as doubles) (lmh_rollout_trace)
METRICS_STRIDE = 208          # one per-robot metrics record (lmh_rollout_metrics)
# name -> (offset, shape) inside a metrics record: the LMH_METRICS_OFF_* defines of include/lmh.h
METRICS_FIELDS = {
    "count": (0, ()), "first_flag": (1, ()), "first_fall": (2, ()), "z_min": (3, ()), "tilt_max": (4, ()),
    "xmin": (8, (60,)), "xmax": (68, (60,)), "wmin": (128, (12,)), "wmax": (140, (12,)),
    "tau_maxabs": (152, (24,)), "tau_sq": (176, (24,)), "err_maxabs": (200, (2,)), "err_sq": (202, (2,)),
}
METRICS_PADS = ((5, 8), (204, 208))   # zero
TERMS_STRIDE = 1840           # one rigid-body terms record (lmh_terms)
# name -> (offset, shape) inside a terms record: the LMH_TERMS_OFF_* defines of include/lmh.h, every array row-major
TERMS_FIELDS = {
    "M": (0, (30, 30)), "C": (900, (30,)), "Cg": (930, (6,)), "AG": (936, (6, 30)), "AGpqp": (1116, (6,)),
    "J": (1122, (12, 30)), "Jpqp": (1482, (12,)), "CoM": (1494, (3,)), "comVel": (1497, (3,)), "angMom": (1500, (3,)),
    "mass": (1503, ()), "T": (1504, (28, 3, 4)),
}

CONTACT_STRIDE = 40           # one contact record (lmh_contact_wrench, lmh_plant_derivative)
# name -> (offset, shape) inside a contact record: the LMH_CONTACT_OFF_* defines of include/lmh.h
CONTACT_FIELDS = {"w": (0, (12,)), "vertex_force": (12, (8, 3)), "pad": (36, (4,))}

LIP_STRIDE = 8                # the reduced (LIPM) state of one robot: x | xdot | y | ydot | t | pad(3) (lmh_mpc_step)
MPC_STRIDE = 16               # one MPC sample (lmh_mpc_step, lmh_mpc_rollout)
# name -> (offset, shape) inside an MPC sample: the LMH_MPC_OFF_* defines of include/lmh.h; [15] is a pad (zero)
MPC_FIELDS = {"x_ref": (0, (3,)), "y_ref": (3, (3,)), "zmp": (6, (2,)), "state": (8, (4,)), "t": (12, ()), "k": (13, ()), "flags": (14, ())}
MPC_PREVIEW_STRIDE = 536      # one horizon preview record (lmh_mpc_preview): header(8) | eight arrays of 66
MPC_PREVIEW_ARRAY = 66
# name -> (offset, entries used at horizon N as a function of N): the LMH_MPC_PREVIEW_OFF_* defines of include/lmh.h
MPC_PREVIEW_ARRAYS = {"U_x": (8, 1), "U_y": (74, 1), "Z_x": (140, 1), "Z_y": (206, 1),
                      "C_x": (272, 2), "Cv_x": (338, 2), "C_y": (404, 2), "Cv_y": (470, 2)}   # (offset, count - N)
MPC_BOX_STRIDE = 668          # one constrained preview record (lmh_mpc_box_preview): the preview record | LAM_x(66) | LAM_y(66)
# the box record's own words: rounds and active samples per axis in the header, the multipliers behind the preview record
MPC_BOX_HEADER = {"rounds_x": 3, "rounds_y": 4, "active_x": 5, "active_y": 6}
MPC_BOX_ARRAYS = dict(MPC_PREVIEW_ARRAYS, lam_x=(536, 1), lam_y=(602, 1))
MPC_OFF_ACTIVE = 15           # an lmh_mpc_box_step sample's active samples of both axes (zero in lmh_mpc_step's)
MPC_BOX_MAX_ROUNDS = 260      # exchange rounds per axis before LMH_FLAG_QP_MAXITER
BOX_ROWS = {"lo_x": 0, "hi_x": 1, "lo_y": 2, "hi_y": 3}      # the rows of one set of bounds [4][n_samples]: the LMH_BOX_* defines

FLAG_QP_MAXITER = 1
FLAG_NONFINITE = 2
FLAG_ZMP_RANGE = 4
FLAG_NOT_SPD = 8
FLAG_QP_FP64_ROUTE = 16
FLAG_BOX_EMPTY = 64           # lmh_mpc_box_*: a sample of the window has lo > hi or a NaN bound
FLAG_TAU_LIMIT = 128          # lmh_rollout_zoh_io, informational: a joint's torque was cut to its limit on some tick of the launch
FLAG_CONTACT_PULL = 256       # lmh_plant_*_rigid, informational: a held foot's multiplier pulls (f_z < 0)
FLAG_CONTACT_SLIP = 512       # lmh_plant_*_rigid, informational: a held foot's multiplier leaves the friction disc contact_mu f_z
FLAG_IMPULSE_PULL = 1024      # lmh_plant_impact_rigid, informational: a held foot's impulse pulls (f_z < 0)
FLAG_IMPULSE_SLIP = 2048      # lmh_plant_impact_rigid, informational: a held foot's impulse leaves the friction disc contact_mu f_z
FLAG_UNFINISHED = 32          # lmh_rollout: the robot did not get all its ticks (a wait of the kernel's work queue ran out)
ERR_UNFINISHED = -5

PHASE_DOUBLE, PHASE_RIGHT, PHASE_LEFT, PHASE_FLIGHT = 0, 1, 2, 3
PRECISION_FP64, PRECISION_MIXED, PRECISION_FP32 = 0, 1, 2   # lmh_config.precision (include/lmh.h)
SUMMARY_WIDTH = 16


class LmhConfig(C.Structure):
    """struct lmh_config (include/lmh.h); defaults are the reference's literals."""
    _fields_ = [(n, C.c_double) for n in (
        "dt", "time_horizon", "z_com", "gravity", "alpha", "beta", "mu",
        "kp_joints", "kd_joints", "kp_mom", "kd_mom", "kp_feet", "kd_feet",
        "w_com_lin", "w_com_ang", "w_base_pos", "w_base_ang", "w_joints", "w_force", "w_foot",
        "eps_coeff")] + [("warm_start", C.c_int32), ("max_qp_iters", C.c_int32), ("precision", C.c_int32), ("bpp_rounds", C.c_int32),
                                     ("plant", C.c_int32), ("reserved", C.c_int32)] + [(n, C.c_double) for n in ("contact_k", "contact_d", "contact_dt", "contact_mu", "mpc_dt")]


class LmhWalkSpec(C.Structure):
    """struct lmh_walk_spec (include/lmh.h): one robot's arguments of lmh_gen_walk."""
    _fields_ = [(n, C.c_double) for n in ("time_per_step", "ds_time", "step_height", "settle_time", "foot_y")] + \
               [("num_steps", C.c_int32), ("first_support", C.c_int32)]


class LmhJumpSpec(C.Structure):
    """struct lmh_jump_spec (include/lmh.h)."""
    _fields_ = [("stance_time", C.c_double), ("flight_time", C.c_double)]


class LmhZohOpts(C.Structure):
    """struct lmh_zoh_opts (include/lmh.h): the options of lmh_rollout_zoh_ex; all zero = lmh_rollout_zoh."""
    _fields_ = [(n, C.c_void_p) for n in ("d_base_wrench", "d_ref", "d_log", "d_trace", "d_metrics")] + \
               [(n, C.c_int32) for n in ("trace_every", "wrench_per_tick", "pushes", "reserved")]


class LmhZohIo(C.Structure):
    """struct lmh_zoh_io (include/lmh.h): what lmh_rollout_zoh_io puts between controller and plant; all zero = lmh_rollout_zoh_ex."""
    _fields_ = [(n, C.c_void_p) for n in ("d_meas", "d_act_mem", "d_applied")] + [("actuators", C.c_int32), ("reserved", C.c_int32)]


class LmhZohServo(C.Structure):
    """struct lmh_zoh_servo (include/lmh.h): the joint servo of lmh_rollout_zoh_servo; mode 0 = lmh_rollout_zoh_io."""
    _fields_ = [("d_setpoint", C.c_void_p), ("mode", C.c_int32), ("reserved", C.c_int32)]


class LmhZohRigid(C.Structure):
    """struct lmh_zoh_rigid (include/lmh.h): the rigid-contact hold of lmh_rollout_zoh_rigid; source 0 = lmh_rollout_zoh_io."""
    _fields_ = [("d_mode", C.c_void_p), ("d_lambda", C.c_void_p), ("kv", C.c_double), ("source", C.c_int32), ("reserved", C.c_int32)]


class LmhZohImpact(C.Structure):
    """struct lmh_zoh_impact (include/lmh.h): the plastic impact of lmh_rollout_zoh_rigid_impact; enable 0 = lmh_rollout_zoh_rigid."""
    _fields_ = [("d_mode_prev", C.c_void_p), ("d_impulse", C.c_void_p), ("enable", C.c_int32), ("reserved", C.c_int32)]


_vp, _ip, _dp, _str, _u64 = C.c_void_p, C.c_int, C.c_double, C.c_char_p, C.c_uint64
_u64p, _dpp = C.POINTER(C.c_uint64), C.POINTER(C.c_double)
# name -> (restype, argtypes) of every symbol include/lmh.h declares; tests/test_abi.py holds each row against its prototype
PROTOTYPES = {
    "lmh_config_default": (None, [C.POINTER(LmhConfig)]),
    "lmh_last_error": (_str, []),
    "lmh_device_count": (_ip, []),
    "lmh_create": (_ip, [C.POINTER(LmhConfig), _ip, _ip, C.POINTER(_vp)]),
    "lmh_destroy": (_ip, [_vp]),
    "lmh_num_instances": (_ip, [_vp]),
    "lmh_horizon": (_ip, [_vp]),
    "lmh_set_model": (_ip, [_vp, _vp, _ip]),
    "lmh_get_mass": (_ip, [_vp, _vp]),
    "lmh_nominal_links": (None, [_vp]),
    "lmh_set_refs": (_ip, [_vp, _vp, _vp, _vp, _ip]),
    "lmh_set_refs_stance": (_ip, [_vp, _dp, _ip]),
    "lmh_set_foot_coeffs": (_ip, [_vp, _vp, _vp, _vp, _vp]),
    "lmh_set_segments": (_ip, [_vp, _vp, _ip, _vp, _ip]),
    "lmh_gen_walk": (_ip, [_vp, _dp, _ip, _dp, _dp, _dp, _dp, _ip, _dp]),
    "lmh_gen_jump": (_ip, [_vp, _dp, _dp, _dp]),
    "lmh_gen_walk_batch": (_ip, [_vp, _dp, _vp, _ip]),
    "lmh_gen_jump_batch": (_ip, [_vp, _dp, _vp, _ip]),
    "lmh_set_plans": (_ip, [_vp, _vp, _vp, _vp, _ip, _vp, _ip, _vp, _ip]),
    "lmh_plans_per_instance": (_ip, [_vp]),
    "lmh_num_ref_samples": (_ip, [_vp]),
    "lmh_num_segments": (_ip, [_vp]),
    "lmh_get_refs": (_ip, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "lmh_get_plan": (_ip, [_vp, _ip, _vp, _vp, _vp, _vp, _vp]),
    "lmh_set_xscale": (_ip, [_vp, _vp, _ip]),
    "lmh_set_zcom": (_ip, [_vp, _vp, _ip]),
    "lmh_get_mpc_gain": (_ip, [_vp, _vp]),
    "lmh_set_pushes": (_ip, [_vp, _vp, _ip, _ip]),
    "lmh_num_pushes": (_ip, [_vp]),
    "lmh_pushes_per_instance": (_ip, [_vp]),
    "lmh_get_pushes": (_ip, [_vp, _ip, _vp]),
    "lmh_set_actuators": (_ip, [_vp, _vp, _ip]),
    "lmh_actuators_per_instance": (_ip, [_vp]),
    "lmh_get_actuators": (_ip, [_vp, _ip, _vp]),
    "lmh_set_servo": (_ip, [_vp, _vp, _ip]),
    "lmh_servo_per_instance": (_ip, [_vp]),
    "lmh_get_servo": (_ip, [_vp, _ip, _vp]),
    "lmh_set_ground": (_ip, [_vp, _vp, _ip]),
    "lmh_ground_per_instance": (_ip, [_vp]),
    "lmh_get_ground": (_ip, [_vp, _ip, _vp]),
    "lmh_set_params": (_ip, [_vp, _vp, _ip]),
    "lmh_params_per_instance": (_ip, [_vp]),
    "lmh_get_params": (_ip, [_vp, _ip, _vp]),
    "lmh_eval": (_ip, [_vp, _vp, _vp, _vp, _vp]),
    "lmh_eval_ref": (_ip, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "lmh_eval_debug": (_ip, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "lmh_rollout": (_ip, [_vp, _vp, _vp, _vp, _vp, _ip, _vp]),
    "lmh_rollout_trace": (_ip, [_vp, _vp, _vp, _vp, _vp, _ip, _vp, _ip, _vp]),
    "lmh_trace_samples": (_ip, [_ip, _ip]),
    "lmh_metrics_reset": (_ip, [_vp, _vp, _dp, _dp, _vp]),
    "lmh_rollout_metrics": (_ip, [_vp, _vp, _vp, _vp, _vp, _ip, _vp, _vp]),
    "lmh_ik": (_ip, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lmh_ik_batch": (_ip, [_vp, _vp, _vp, _ip, _vp, _vp, _vp, _vp]),
    "lmh_robot_com": (_ip, [_vp, _vp, _vp, _vp]),
    "lmh_terms": (_ip, [_vp, _vp, _vp, _vp, _vp]),
    "lmh_inverse_dynamics": (_ip, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lmh_forward_dynamics": (_ip, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lmh_contact_wrench": (_ip, [_vp, _vp, _vp, _vp, _vp]),
    "lmh_plant_derivative": (_ip, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lmh_plant_step": (_ip, [_vp, _vp, _vp, _ip, _vp, _vp]),
    "lmh_plant_step_servo": (_ip, [_vp, _vp, _vp, _vp, _ip, _vp, _vp]),
    "lmh_plant_derivative_rigid": (_ip, [_vp, _vp, _vp, _vp, _vp, _dp, _vp, _vp, _vp, _vp]),
    "lmh_plant_step_rigid": (_ip, [_vp, _vp, _vp, _vp, _dp, _ip, _vp, _vp, _vp]),
    "lmh_plant_impact_rigid": (_ip, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lmh_rollout_zoh": (_ip, [_vp, _vp, _vp, _vp, _vp, _vp, _ip, _ip, _vp]),
    "lmh_rollout_zoh_ref": (_ip, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _ip, _ip, _vp]),
    "lmh_rollout_zoh_ex": (_ip, [_vp, _vp, _vp, _vp, C.POINTER(LmhZohOpts), _ip, _ip, _vp]),
    "lmh_rollout_zoh_box": (_ip, [_vp, _vp, _vp, _vp, C.POINTER(LmhZohOpts), _vp, _ip, _ip, _vp, _ip, _ip, _vp]),
    "lmh_rollout_zoh_io": (_ip, [_vp, _vp, _vp, _vp, C.POINTER(LmhZohOpts), C.POINTER(LmhZohIo), _ip, _ip, _vp]),
    "lmh_rollout_zoh_servo": (_ip, [_vp, _vp, _vp, _vp, C.POINTER(LmhZohOpts), C.POINTER(LmhZohIo), C.POINTER(LmhZohServo), _ip, _ip, _vp]),
    "lmh_rollout_zoh_rigid": (_ip, [_vp, _vp, _vp, _vp, C.POINTER(LmhZohOpts), C.POINTER(LmhZohIo), C.POINTER(LmhZohRigid), _ip, _ip, _vp]),
    "lmh_rollout_zoh_rigid_impact": (_ip, [_vp, _vp, _vp, _vp, C.POINTER(LmhZohOpts), C.POINTER(LmhZohIo), C.POINTER(LmhZohRigid), C.POINTER(LmhZohImpact), _ip, _ip, _vp]),
    "lmh_mpc_step": (_ip, [_vp, _vp, _vp, _vp]),
    "lmh_mpc_rollout": (_ip, [_vp, _vp, _ip, _vp, _vp]),
    "lmh_mpc_preview": (_ip, [_vp, _vp, _vp, _vp]),
    "lmh_mpc_box_preview": (_ip, [_vp, _vp, _vp, _ip, _ip, _vp, _vp]),
    "lmh_mpc_box_step": (_ip, [_vp, _vp, _vp, _ip, _ip, _vp, _vp]),
    "lmh_mpc_box_rollout": (_ip, [_vp, _vp, _vp, _ip, _ip, _ip, _vp, _vp]),
    "lmh_eval_host": (_ip, [_vp, _vp, _vp, _dp, _vp, _vp, _vp, _vp]),
    "lmh_robot_com_host": (_ip, [_vp, _vp, _vp]),
    "lmh_last_out_host": (_ip, [_vp, _vp]),
    "lmh_ik_host": (_ip, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lmh_terms_host": (_ip, [_vp, _vp, _vp, _vp]),
    "lmh_mpc_step_host": (_ip, [_vp, _vp, _vp]),
    "lmh_set_prev_velocity_host": (_ip, [_vp, _vp]),
    "lmh_synchronize": (_ip, [_vp, _vp]),
    "lmh_make_summary": (_ip, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "lmh_write_summary": (_ip, [_str, _vp, _u64, _dp]),
    "lmh_read_summary": (_ip, [_str, _vp, _u64, _u64p, _dpp]),
    "lmh_write_log": (_ip, [_str, _vp, _u64, _u64, _dp, _dp]),
    "lmh_read_log": (_ip, [_str, _vp, _u64, _u64p, _u64p, _dpp, _dpp]),
    "lmh_write_trace": (_ip, [_str, _vp, _u64, _u64, _dp, _dp]),
    "lmh_read_trace": (_ip, [_str, _vp, _u64, _u64p, _u64p, _dpp, _dpp]),
}
EXPORTS = list(PROTOTYPES)
# the diagnostics csrc/lmh_launch.h declares beside the C ABI: bound where the loaded library has them (a build of an earlier tree may not)
DEBUG_PROTOTYPES = {"lmh_debug_build_flags": (_ip, []), "lmh_debug_rollout_occupancy": (_ip, [C.POINTER(C.c_int)] * 3)}

_lib = None


def lib():
    """Load the HIP library.  Fails loudly if it has not been built (python -m linearmpchumanoid_amd.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise RuntimeError(
            f"{SO_PATH} is missing: the MI355X HIP library has not been built "
            "(run `python __graft_entry__.py` or `python linearmpchumanoid_amd/build.py`). "
            "There is no CPU fallback.")
    L = C.CDLL(SO_PATH)
    for name, (restype, argtypes) in list(PROTOTYPES.items()) + [d for d in DEBUG_PROTOTYPES.items() if hasattr(L, d[0])]:
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


class LmhError(RuntimeError):
    def __init__(self, msg, code=0):
        super().__init__(msg)
        self.code = code


def check(rc):
    if rc != 0:
        raise LmhError(f"lmh error {rc}: {lib().lmh_last_error().decode()}", rc)
