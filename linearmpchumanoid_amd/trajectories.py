"""Set-up time reference generators (inputs of the hot path), host side.

Mirrors the reference's trajectory producers: ZMP::stanceZMP (src/zmpGeneration.cpp:39-60),
footCoeffTrajectory (src/footRefTrajectory.cpp:4-47) and findPolyCoeff
(src/generalizedFunctions.cpp:103-163).  The reference declares a walking generator
(zmpGeneration.hpp:15-22 walkZMP) but never defines it; walk_refs() below is the build's own
definition on top of the reference's conventions (SupportFoot -> ZMP y of -/+0.05).
"""
import numpy as np

from .capi import FLAG_CONTACT_PULL, FLAG_CONTACT_SLIP, FLAG_IMPULSE_PULL, FLAG_IMPULSE_SLIP, ACT_MAX_DELAY, ACT_MEM_STRIDE, ACT_OFF_ALPHA, ACT_OFF_DELAY, ACT_OFF_TAU_MAX, ACT_STRIDE, FLAG_BOX_EMPTY, FLAG_NONFINITE, FLAG_NOT_SPD, FLAG_QP_MAXITER, FLAG_ZMP_RANGE, GROUND_OFF_H_L, GROUND_OFF_H_R, GROUND_OFF_N_L, GROUND_OFF_N_R, GROUND_STRIDE, IK_TARGET_STRIDE, LIP_STRIDE, MAX_PUSHES, MPC_BOX_MAX_ROUNDS, MPC_STRIDE, PHASE_DOUBLE, PHASE_LEFT, PHASE_RIGHT, PHASE_FLIGHT, PUSH_STRIDE, SERVO_OFF_KD, SERVO_OFF_KP, SERVO_STRIDE, SETPOINT_STRIDE


def stance_zmp(simulation_time, time_step, support_foot=2):
    """ZMP::stanceZMP; support_foot 0 Right, 1 Left, 2 Double (Task.hpp:9-13)."""
    samples = int((simulation_time + 0.5) / time_step)
    zx = np.zeros(samples)
    zy = np.full(samples, -0.05 if support_foot == 0 else (0.05 if support_foot == 1 else 0.0))
    return zx, zy


def find_poly_coeff(pos, vel, acc):
    """findPolyCoeff(Pos, Vel, Acc): rows are (t, value); ascending-power coefficients."""
    pos, vel, acc = (np.atleast_2d(np.asarray(a, dtype=np.float64)) for a in (pos, vel, acc))
    n = len(pos) + len(vel) + len(acc)
    A = np.zeros((n, n)); b = np.zeros(n)
    row = 0
    for t, val in pos:
        A[row] = t ** np.arange(n); b[row] = val; row += 1
    for t, val in vel:
        for j in range(1, n):
            A[row, j] = j * t ** (j - 1)
        b[row] = val; row += 1
    for t, val in acc:
        for j in range(2, n):
            A[row, j] = j * (j - 1) * t ** (j - 2)
        b[row] = val; row += 1
    return np.linalg.solve(A, b)


def foot_coeff_trajectory(current_pos, des_pos, step_height, T):
    """footCoeffTrajectory: x, y 5th order (6 coefficients), z 7th order (8). Returns ([3,8], [3])."""
    cur = np.asarray(current_pos, dtype=np.float64); des = np.asarray(des_pos, dtype=np.float64)
    co = np.zeros((3, 8)); n = np.array([6, 6, 8], dtype=np.int32)
    vel2 = [(0, 0), (T, 0)]; acc2 = [(0, 0), (T, 0)]
    for ax in range(2):
        co[ax, :6] = find_poly_coeff([(0, cur[ax]), (T, des[ax])], vel2, acc2)
    co[2, :8] = find_poly_coeff([(0, cur[2]), (T / 2, step_height), (T, des[2])],
                                [(0, 0), (T / 2, 0), (T, 0)], acc2)
    return co, n


def walk_plan(simulation_time, time_step, num_steps=4, time_per_step=0.5, ds_time=0.1, step_height=0.02,
              settle_time=0.3, first_support=PHASE_RIGHT, foot_y=0.05):
    """Build-defined walking references on the reference's conventions (no reference semantics: the
    reference declares ZMP(Task, numSteps, timePerStep, simulationTime) / walkZMP but defines neither).

    x quantities are in units of the step length: the per-instance scale (set_xscale) turns them into
    metres on the device.  Returns dict(zmp_x, zmp_y, phase, segs[n_seg,52], seg_of_sample):
      * phase[k]: PHASE_DOUBLE / PHASE_RIGHT (right foot supports, left swings) / PHASE_LEFT;
      * ZMP: support-foot position in single support, mid-point of the feet in double support;
      * segment g = t0 | rF[3][8] | lF[3][8]: constant polynomials while a foot stands, the
        footCoeffTrajectory() polynomials (5th order x/y, 7th order z through step_height) while it swings,
        evaluated at t - t0.
    Sample grid and length follow ZMP::stanceZMP: int((T + 0.5) / dt) samples, sample k <-> t = k dt."""
    n = int((simulation_time + 0.5) / time_step)
    zx = np.zeros(n); zy = np.zeros(n); ph = np.full(n, PHASE_DOUBLE, dtype=np.uint8)
    sos = np.zeros(n, dtype=np.uint16)
    segs = []

    def hold(t0, xr, xl):
        g = np.zeros(52); g[0] = t0
        g[1 + 0] = xr; g[1 + 8] = -foot_y            # rF x, y constants (z = 0)
        g[1 + 24 + 0] = xl; g[1 + 24 + 8] = foot_y   # lF
        return g

    def idx(t):
        return min(n, max(0, int(round(t / time_step))))

    xr = xl = 0.0
    segs.append(hold(0.0, xr, xl))
    cur = 0
    sup = first_support
    t = settle_time
    for s in range(num_steps):
        stride = 1.0 if (s == 0 or s == num_steps - 1) else 2.0
        t_ss0, t_ss1 = t + ds_time, t + time_per_step
        a, b, c = idx(t), idx(t_ss0), idx(t_ss1)
        # double support [a, b): hold segment, ZMP at the mid-point
        segs.append(hold(t, xr, xl)); cur = len(segs) - 1
        sos[a:b] = cur; zx[a:b] = 0.5 * (xr + xl); zy[a:b] = 0.0
        # single support [b, c)
        T = (c - b) * time_step
        g = hold(b * time_step, xr, xl)
        if sup == PHASE_RIGHT:                        # left foot swings
            co, _ = foot_coeff_trajectory([xl, foot_y, 0.0], [xl + stride, foot_y, 0.0], step_height, T)
            g[1 + 24:1 + 48] = co.reshape(-1); zx[b:c] = xr; zy[b:c] = -foot_y; xl += stride
        else:
            co, _ = foot_coeff_trajectory([xr, -foot_y, 0.0], [xr + stride, -foot_y, 0.0], step_height, T)
            g[1:1 + 24] = co.reshape(-1); zx[b:c] = xl; zy[b:c] = foot_y; xr += stride
        segs.append(g); cur = len(segs) - 1
        sos[b:c] = cur; ph[b:c] = sup
        sup = PHASE_LEFT if sup == PHASE_RIGHT else PHASE_RIGHT
        t += time_per_step
    a = idx(t)
    segs.append(hold(t, xr, xl)); cur = len(segs) - 1
    sos[a:] = cur; zx[a:] = 0.5 * (xr + xl); zy[a:] = 0.0
    return dict(zmp_x=zx, zmp_y=zy, phase=ph, segs=np.array(segs), seg_of_sample=sos)


def jump_plan(simulation_time, time_step, stance_time=0.4, flight_time=0.15):
    """Build-defined jumping contact schedule (BASELINE config 5; the reference only hints at it: "0 reaction
    variables" in the comment at controller.hpp:98): double support for stance_time, PHASE_FLIGHT for
    flight_time (both feet forced out of the QP), double support afterwards.  ZMP references stay at the
    stance values of ZMP::stanceZMP(Double); the feet keep their constant polynomials.
    Returns dict(zmp_x, zmp_y, phase) on the ZMP::stanceZMP sample grid."""
    zx, zy = stance_zmp(simulation_time, time_step, 2)
    n = len(zx)
    ph = np.full(n, PHASE_DOUBLE, dtype=np.uint8)
    a = min(n, int(round(stance_time / time_step)))
    b = min(n, int(round((stance_time + flight_time) / time_step)))
    ph[a:b] = PHASE_FLIGHT
    return dict(zmp_x=zx, zmp_y=zy, phase=ph)


WALK_SPEC_DEFAULTS = dict(num_steps=4, time_per_step=0.5, ds_time=0.1, step_height=0.02, settle_time=0.3, first_support=PHASE_RIGHT,
                          foot_y=0.05)                 # the defaults of walk_plan / BatchedController.gen_walk
JUMP_SPEC_DEFAULTS = dict(stance_time=0.4, flight_time=0.15)


def broadcast_specs(specs, defaults, B=None):
    """specs: dict of arrays of one length B (scalars broadcast; missing fields take `defaults`) -> (dict of [B] arrays, B).
    Integer fields (num_steps, first_support) come back as int64, the others as float64."""
    unknown = set(specs) - set(defaults)
    if unknown:
        raise KeyError(f"unknown spec fields {sorted(unknown)}")
    vals = {k: np.asarray(specs.get(k, d)) for k, d in defaults.items()}
    sizes = {v.shape[0] for v in vals.values() if v.ndim == 1}
    if any(v.ndim > 1 for v in vals.values()) or len(sizes) > 1:
        raise ValueError("spec fields must be scalars or arrays of one length")
    n = sizes.pop() if sizes else (1 if B is None else B)
    if B is not None and n != B:
        raise ValueError(f"specs describe {n} robots, expected {B}")
    out = {}
    for k, v in vals.items():
        if isinstance(defaults[k], int):
            if not np.all(v == np.round(v)):                        # num_steps = 2.5 is a mistake, not a request to truncate
                raise ValueError(f"{k} must be whole numbers")
            out[k] = np.broadcast_to(v.astype(np.int64), (n,)).copy()
        else:
            out[k] = np.broadcast_to(v.astype(np.float64), (n,)).copy()
    return out, n


def spec_of(specs, i):
    """Robot i's keyword arguments of walk_plan / jump_plan from a broadcast spec dict."""
    return {k: (int(v[i]) if v.dtype.kind == "i" else float(v[i])) for k, v in specs.items()}


def walk_plans(simulation_time, time_step, specs, B=None):
    """One walk_plan per robot (the host statement of lmh_gen_walk_batch; what BatchedController.set_plans takes): specs is a dict of
    arrays of length B with walk_plan's keyword arguments (scalars broadcast, missing ones take walk_plan's defaults).
    Returns dict(zmp_x [B,n], zmp_y [B,n], phase [B,n], segs [B,n_seg,52], seg_of_sample [B,n]) with n_seg = 2 max(num_steps) + 2: a
    robot with fewer steps fills its first 2 num_steps + 2 records, the rest of its slice is zero and its seg_of_sample never points there."""
    sp, n = broadcast_specs(specs, WALK_SPEC_DEFAULTS, B)
    plans = [walk_plan(simulation_time, time_step, **spec_of(sp, i)) for i in range(n)]
    n_seg = max(p["segs"].shape[0] for p in plans)
    segs = np.zeros((n, n_seg, 52))
    for i, p in enumerate(plans):
        segs[i, :p["segs"].shape[0]] = p["segs"]
    out = {k: np.stack([p[k] for p in plans]) for k in ("zmp_x", "zmp_y", "phase", "seg_of_sample")}
    out["segs"] = segs
    return out


def jump_plans(simulation_time, time_step, specs, B=None):
    """One jump_plan per robot (the host statement of lmh_gen_jump_batch): dict(zmp_x, zmp_y, phase), each [B,n]."""
    sp, n = broadcast_specs(specs, JUMP_SPEC_DEFAULTS, B)
    plans = [jump_plan(simulation_time, time_step, **spec_of(sp, i)) for i in range(n)]
    return {k: np.stack([p[k] for p in plans]) for k in ("zmp_x", "zmp_y", "phase")}


# the default targets of lmh_ik / BatchedController.ik: CoM, right and left sole [x y z | roll pitch yaw]
IK_DEFAULT_COM = (-0.02, 0.0, 0.26)
IK_DEFAULT_RF = (0.0, -0.05, 0.0, 0.0, 0.0, 0.0)
IK_DEFAULT_LF = (0.0, 0.05, 0.0, 0.0, 0.0, 0.0)


def ik_targets(com=IK_DEFAULT_COM, rf=IK_DEFAULT_RF, lf=IK_DEFAULT_LF, B=None, n=None):
    """Target records of lmh_ik_batch / BatchedController.ik_batch: [n,B,16] float64, each record rf(6) | lf(6) | com(3) | pad (zero).
    com is a scalar, [3], [B,3] or [n,B,3]; rf and lf a scalar, [6], [B,6] or [n,B,6]; the smaller forms broadcast over robots and
    targets.  B and n are taken from the arrays that carry them (1 where none does) and must agree with the B, n given."""
    fields = (("rf", rf, 6), ("lf", lf, 6), ("com", com, 3))
    vals, Bs, ns = {}, set(), set()
    for name, v, w in fields:
        v = np.asarray(v, dtype=np.float64)
        if v.ndim > 3 or (v.ndim >= 1 and v.shape[-1] != w):
            raise ValueError(f"{name} must be a scalar, [{w}], [B,{w}] or [n,B,{w}]")
        if v.ndim >= 2:
            Bs.add(v.shape[-2])
        if v.ndim == 3:
            ns.add(v.shape[0])
        vals[name] = v
    if len(Bs) > 1 or len(ns) > 1:
        raise ValueError("target fields must describe one number of robots and one number of targets")
    nb = Bs.pop() if Bs else (1 if B is None else B)
    nn = ns.pop() if ns else (1 if n is None else n)
    if B is not None and nb != B:
        raise ValueError(f"targets describe {nb} robots, expected {B}")
    if n is not None and nn != n:
        raise ValueError(f"targets describe {nn} targets, expected {n}")
    rec = np.zeros((nn, nb, IK_TARGET_STRIDE))
    rec[..., 0:6], rec[..., 6:12], rec[..., 12:15] = vals["rf"], vals["lf"], vals["com"]
    return rec


def start_targets(z_com=None, foot_y=None, com_xy=(-0.02, 0.0), B=None):
    """Start-posture records [B,16] for ik_batch: robot i's CoM at (com_xy, z_com[i]) and its soles flat on the ground at y = -/+
    foot_y[i] -- the values the caller passes to set_zcom and to the walk specs' foot_y.  z_com, foot_y: scalars or [B] (None: lmh_ik's
    defaults 0.26 and 0.05); com_xy: [2] or [B,2]."""
    sp, nb = broadcast_specs({k: v for k, v in (("z_com", z_com), ("foot_y", foot_y)) if v is not None},
                             dict(z_com=IK_DEFAULT_COM[2], foot_y=IK_DEFAULT_LF[1]), B)
    xy = np.asarray(com_xy, dtype=np.float64)
    if xy.ndim not in (1, 2) or xy.shape[-1] != 2 or (xy.ndim == 2 and xy.shape[0] != nb):
        raise ValueError(f"com_xy must be [2] or [{nb},2]")
    rec = np.zeros((nb, IK_TARGET_STRIDE))
    rec[:, 1], rec[:, 7] = -sp["foot_y"], sp["foot_y"]
    rec[:, 12:14], rec[:, 14] = xy, sp["z_com"]
    return rec


def preview_index(t, mpc_dt):
    """k = (int)(t / mpc_dt) of mpcLinearPendulum.cpp:92 as the kernels form it: the fp64 quotient truncated towards zero, saturated to
    int32, 0 for a NaN."""
    q = np.float64(t) / np.float64(mpc_dt)
    if np.isnan(q):
        return 0
    return int(np.clip(np.trunc(q), -2147483648.0, 2147483647.0))


def lip_rollout(K, Px0, Px1, zx, zy, lip, n_ticks, mpc_dt, z_com, gravity=9.81, xscale=1.0):
    """The numpy statement of lmh_mpc_rollout (include/lmh.h) for ONE robot: n_ticks times { the MPC step at (x, xdot, y, ydot, t); the
    sample; x <- x_next, ..., t <- t + mpc_dt }.  K, Px0, Px1 [N+1]: the robot's gain row (lmh_get_mpc_gain) and the two columns of Px
    (Px0 = 1, Px1 = j mpc_dt accumulated); zx, zy [n]: its plan's samples; lip [8] (or [5]): x | xdot | y | ydot | t; z_com, xscale: its
    LIPM height and step-length scale.  -> (lip [8] after the last tick, samples [n_ticks,16] laid out as capi.MPC_FIELDS).
    The step: k = (int)(t / mpc_dt); w = sum_j K_j z[clip(k + j)]; u = -((K.Px0 x + K.Px1 xdot) - xscale w) (y: no xscale);
    x_ref = (x + mpc_dt xdot + mpc_dt^2 / 2 u, xdot + mpc_dt u, u); zmp = x + D u, D = -z_com / gravity; FLAG_ZMP_RANGE when k < 0 or
    k + N >= n.  The sums are numpy's, so the kernel agrees to rounding, not to the bit; everything else is the kernel's operation order."""
    K, Px0, Px1 = (np.asarray(a, dtype=np.float64) for a in (K, Px0, Px1))
    zx, zy = np.asarray(zx, dtype=np.float64), np.asarray(zy, dtype=np.float64)
    N, n = len(K) - 1, len(zx)
    if Px0.shape != K.shape or Px1.shape != K.shape or zy.shape != zx.shape or zx.ndim != 1 or n < 1:
        raise ValueError("K, Px0, Px1 must be [N+1] and zx, zy [n]")
    if int(n_ticks) != n_ticks or n_ticks < 0:
        raise ValueError("n_ticks must be a whole number >= 0")
    dt = np.float64(mpc_dt)
    a01, b0, b1 = dt, (dt * dt) / 2, dt
    D = -np.float64(z_com) / np.float64(gravity)
    kp0, kp1 = K @ Px0, K @ Px1
    st = np.zeros(LIP_STRIDE)
    st[:min(len(lip), LIP_STRIDE)] = np.asarray(lip, dtype=np.float64)[:LIP_STRIDE]
    x, xd, y, yd, t = (np.float64(v) for v in st[:5])
    out = np.zeros((int(n_ticks), MPC_STRIDE))
    j = np.arange(N + 1)
    with np.errstate(all="ignore"):
        for tick in range(int(n_ticks)):
            k = preview_index(t, dt)
            idx = np.clip(k + j, 0, n - 1)
            ux = -((kp0 * x + kp1 * xd) - np.float64(xscale) * (K @ zx[idx]))
            uy = -((kp0 * y + kp1 * yd) - (K @ zy[idx]))
            rec = out[tick]
            rec[0:3] = x + a01 * xd + b0 * ux, xd + b1 * ux, ux
            rec[3:6] = y + a01 * yd + b0 * uy, yd + b1 * uy, uy
            rec[6:8] = x + D * ux, y + D * uy
            rec[8:13] = x, xd, y, yd, t
            flags = FLAG_ZMP_RANGE if (k < 0 or k + N >= n) else 0
            if not np.isfinite(rec[0:8]).all():
                flags |= FLAG_NONFINITE
            rec[13], rec[14] = k, flags
            x, xd, y, yd = rec[0], rec[1], rec[3], rec[4]
            t = t + dt
    st[:5] = x, xd, y, yd, t
    return st, out


def com_targets(traj, z_com):
    """The `com` argument of ik_targets from an MPC trajectory (lmh_mpc_rollout / lip_rollout): traj [n,B,16] or [n,16] samples ->
    [n,B,3] (or [n,3]) with x = x_ref[0], y = y_ref[0] of every sample -- where the LIPM is at the END of that tick -- and z = z_com (a
    scalar or [B], the values given to set_zcom)."""
    tr = np.asarray(traj, dtype=np.float64)
    if tr.ndim not in (2, 3) or tr.shape[-1] != MPC_STRIDE:
        raise ValueError(f"traj must be [n,B,{MPC_STRIDE}] or [n,{MPC_STRIDE}]")
    z = np.asarray(z_com, dtype=np.float64)
    if z.ndim > 1 or (z.ndim == 1 and (tr.ndim != 3 or z.shape[0] != tr.shape[1])):
        raise ValueError("z_com must be a scalar or [B]")
    com = np.zeros(tr.shape[:-1] + (3,))
    com[..., 0], com[..., 1] = tr[..., 0], tr[..., 3]
    com[..., 2] = z
    return com


# ------------------------------------------------------------------------------- the box-constrained preview MPC (lmh_mpc_box_*)
def zmp_box(plan, xscale=1.0, fwd=0.1, back=0.05, half_width=0.025, margin=0.0):
    """The support region of every sample of a plan as an axis-aligned box, the `box` argument of mpc_box_step / _rollout / _preview:
    -> [4, n_samples], rows lo_x | hi_x | lo_y | hi_y in metres (capi.BOX_ROWS).
    Single support: the stance sole's rectangle (the sole of Robot.cpp:38-42: `fwd` ahead of the foot's origin, `back` behind it,
    `half_width` to either side) about the stance foot's position in the plan -- the plan's ZMP sample there --, x times xscale, every
    side moved inwards by `margin`.  Double support: the axis-aligned hull of both soles (the feet's positions from the plan's segment
    records; a plan without them, stance_zmp / jump_plan, has its feet at zmp_y -+ 0.05 beside zmp_x): exact with the feet side by side,
    an OUTER approximation of the support polygon with one foot ahead of the other, whose hull has two corners the polygon lacks.
    PHASE_FLIGHT: -inf | +inf, no bound.  A sole does not stretch with the step length: only the feet's x positions take xscale."""
    zx, zy = np.asarray(plan["zmp_x"], dtype=np.float64), np.asarray(plan["zmp_y"], dtype=np.float64)
    n = len(zx)
    ph = np.asarray(plan["phase"]) if plan.get("phase") is not None else np.full(n, PHASE_DOUBLE)
    xs = float(xscale)
    if plan.get("segs") is not None and plan.get("seg_of_sample") is not None:
        g = np.asarray(plan["segs"], dtype=np.float64)[np.asarray(plan["seg_of_sample"], dtype=np.int64)]
        xr, yr, xl, yl = g[:, 1], g[:, 1 + 8], g[:, 1 + 24], g[:, 1 + 24 + 8]
    else:
        xr, yr, xl, yl = zx, zy + IK_DEFAULT_RF[1], zx, zy + IK_DEFAULT_LF[1]
    single = (ph == PHASE_RIGHT) | (ph == PHASE_LEFT)
    x_lo = np.where(single, zx, np.minimum(xr, xl)) * xs
    x_hi = np.where(single, zx, np.maximum(xr, xl)) * xs
    y_lo = np.where(single, zy, np.minimum(yr, yl))
    y_hi = np.where(single, zy, np.maximum(yr, yl))
    box = np.stack([x_lo - back + margin, x_hi + fwd - margin, y_lo - half_width + margin, y_hi + half_width - margin])
    box[0::2, ph == PHASE_FLIGHT] = -np.inf
    box[1::2, ph == PHASE_FLIGHT] = np.inf
    return box


def zmp_boxes(plans, xscale=1.0, fwd=0.1, back=0.05, half_width=0.025, margin=0.0):
    """zmp_box for per-robot plans (walk_plans / jump_plans: every field [B, ...]) -> [B, 4, n_samples]; xscale and margin: scalars or [B]."""
    B = np.asarray(plans["zmp_x"]).shape[0]
    xs, mg = np.broadcast_to(np.asarray(xscale, dtype=np.float64), (B,)), np.broadcast_to(np.asarray(margin, dtype=np.float64), (B,))
    return np.stack([zmp_box({k: v[i] for k, v in plans.items()}, xs[i], fwd, back, half_width, mg[i]) for i in range(B)])


def lip_matrices(N, mpc_dt, z_com, gravity=9.81):
    """Px [N+1,2] and Pu [N+1,N+1] of the LIPM preview (Mpc3dLip::initialize): Px row j = (1, j mpc_dt); Pu lower triangular Toeplitz,
    D = -z_com / gravity on the diagonal and mpc_dt^2 / 2 + (m mpc_dt) mpc_dt below it, m = r - c - 1."""
    dt, n = np.float64(mpc_dt), N + 1
    j = np.arange(n, dtype=np.float64)
    Px = np.stack([np.ones(n), j * dt], axis=1)
    col = (dt * dt) / 2 + (j * dt) * dt
    Pu = np.zeros((n, n))
    for c in range(n):
        Pu[c, c] = -np.float64(z_com) / np.float64(gravity)
        Pu[c + 1:, c] = col[:n - c - 1]
    return Px, Pu


def box_exchange(H, Pu, g, p, lo, hi, max_rounds=MPC_BOX_MAX_ROUNDS):
    """One axis of the box-constrained preview problem, min 1/2 U'HU + g'U s.t. lo <= p + Pu U <= hi, by the kernels' exchange rule with
    dense fp64 solves.  -> dict(U, Z, lam, side [n] (-1 lower, +1 upper, 0 inactive), rounds, flags).
    An iterate belongs to a working set (each of its samples at one side): lam_W = S^-1 (Z0_W - b_W), S = Pu_W H^-1 Pu_W', Z0 = p + Pu U0,
    U0 = -H^-1 g; U = -H^-1 (g + Pu' lam); Z = p + Pu U with Z_W = b_W written as the bounds themselves.  It is wrong at an inactive
    sample with Z < lo or Z > hi and at an active one whose multiplier has the wrong sign (> 0 belongs to an upper bound, < 0 to a lower
    one), compared exactly.  Nothing wrong: done.  Otherwise a round: while the number of wrong samples has just reached a new minimum,
    or at most three rounds after it did, all violated samples enter and all wrong-signed ones leave together; after that only the wrong
    sample of the largest index changes (Judice-Pires, Kim-Park).  max_rounds rounds without an end: FLAG_QP_MAXITER, the last iterate."""
    n = len(g)
    U0 = -np.linalg.solve(H, g)
    Z0 = p + Pu @ U0
    G = Pu @ np.linalg.solve(H, Pu.T)
    side = np.zeros(n, dtype=np.int64)
    U, Z, lam = U0.copy(), Z0.copy(), np.zeros(n)
    rounds, best, block, flags = 0, n + 1, 3, 0
    while True:
        want = side.copy()
        off = side == 0
        want[off & (Z < lo)] = -1
        want[off & (Z > hi)] = 1
        want[((side > 0) & (lam < 0)) | ((side < 0) & (lam > 0))] = 0
        bad = np.flatnonzero(want != side)
        if len(bad) == 0:
            break
        if rounds >= max_rounds:
            flags |= FLAG_QP_MAXITER
            break
        rounds += 1
        single = False
        if len(bad) < best:
            best, block = len(bad), 3
        elif block > 0:
            block -= 1
        else:
            single = True
        if single:
            side[bad[-1]] = want[bad[-1]]
        else:
            side = want
        W = np.flatnonzero(side)
        b = np.where(side > 0, hi, lo)
        lam = np.zeros(n)
        if len(W):
            lam[W] = np.linalg.solve(G[np.ix_(W, W)], Z0[W] - b[W])
        U = -np.linalg.solve(H, g + Pu.T @ lam)
        Z = p + Pu @ U
        Z[W] = b[W]
    return dict(U=U, Z=Z, lam=lam, side=side, rounds=rounds, flags=flags)


def lip_box_preview(zx, zy, box, lip, N, mpc_dt, z_com, alpha=1e-3, beta=1.0, gravity=9.81, xscale=1.0, max_rounds=MPC_BOX_MAX_ROUNDS):
    """The numpy statement of lmh_mpc_box_preview for ONE robot: zx, zy [n] its plan, box [4,n] its bounds (zmp_box), lip [5..8] its state.
    -> dict(k, flags, rounds [2], active [2], U [2,N+1], Z [2,N+1], lam [2,N+1], side [2,N+1], C [2,N+2], Cv [2,N+2], lo [2,N+1], hi [2,N+1]).
    A window sample with not (lo <= hi) raises FLAG_BOX_EMPTY and leaves NaNs."""
    zx, zy, box = np.asarray(zx, dtype=np.float64), np.asarray(zy, dtype=np.float64), np.asarray(box, dtype=np.float64)
    n = len(zx)
    if box.shape != (4, n) or zy.shape != zx.shape:
        raise ValueError("zx, zy must be [n] and box [4,n]")
    x = np.asarray(lip, dtype=np.float64)
    k = preview_index(x[4], mpc_dt)
    idx = np.clip(k + np.arange(N + 1), 0, n - 1)
    flags = FLAG_ZMP_RANGE if (k < 0 or k + N >= n) else 0
    Px, Pu = lip_matrices(N, mpc_dt, z_com, gravity)
    H = np.float64(alpha) * np.eye(N + 1) + np.float64(beta) * (Pu.T @ Pu)
    lo, hi = box[0::2, idx], box[1::2, idx]
    out = dict(k=k, rounds=np.zeros(2, dtype=np.int64), lo=lo, hi=hi)
    nanv = np.full(N + 1, np.nan)
    sols = []
    with np.errstate(all="ignore"):
        if not (lo <= hi).all():
            flags |= FLAG_BOX_EMPTY
            sols = [dict(U=nanv, Z=nanv, lam=nanv, side=np.zeros(N + 1, dtype=np.int64), rounds=0, flags=0)] * 2
        else:
            for ax, (z, s) in enumerate(((zx, np.float64(xscale)), (zy, np.float64(1.0)))):
                p = Px @ x[2 * ax:2 * ax + 2]
                g = np.float64(beta) * (Pu.T @ (p - s * z[idx]))
                sols.append(box_exchange(H, Pu, g, p, lo[ax], hi[ax], max_rounds))
        dt = np.float64(mpc_dt)
        C, Cv = np.zeros((2, N + 2)), np.zeros((2, N + 2))
        for ax in range(2):
            c, cv = (x[2 * ax], x[2 * ax + 1]) if not flags & FLAG_BOX_EMPTY else (np.nan, np.nan)
            for j in range(N + 2):
                C[ax, j], Cv[ax, j] = c, cv
                if j <= N:
                    u = sols[ax]["U"][j]
                    c, cv = c + dt * cv + (dt * dt) / 2 * u, cv + dt * u
    for name in ("U", "Z", "lam", "side"):
        out[name] = np.stack([sols[0][name], sols[1][name]])
    out["rounds"] = np.array([sols[0]["rounds"], sols[1]["rounds"]])
    out["active"] = (out["side"] != 0).sum(axis=1)
    out["C"], out["Cv"] = C, Cv
    flags |= sols[0]["flags"] | sols[1]["flags"]
    if not all(np.isfinite(out[a]).all() for a in ("U", "Z", "lam", "C", "Cv")):
        flags |= FLAG_NONFINITE
    out["flags"] = flags
    return out


def lip_box_step(zx, zy, box, lip, N, mpc_dt, z_com, alpha=1e-3, beta=1.0, gravity=9.81, xscale=1.0, max_rounds=MPC_BOX_MAX_ROUNDS):
    """The numpy statement of lmh_mpc_box_step for ONE robot -> (sample [16], the lip_box_preview dict it was formed from): u = U[0] and
    zmp = Z[0] of the constrained solution per axis, x_ref = (x + mpc_dt xdot + mpc_dt^2 / 2 u, xdot + mpc_dt u, u), word 15 the active
    samples of both axes; flags: those of the solve, FLAG_NONFINITE when one of the first eight words is not finite."""
    pv = lip_box_preview(zx, zy, box, lip, N, mpc_dt, z_com, alpha, beta, gravity, xscale, max_rounds)
    st = np.zeros(LIP_STRIDE)
    st[:min(len(lip), LIP_STRIDE)] = np.asarray(lip, dtype=np.float64)[:LIP_STRIDE]
    dt = np.float64(mpc_dt)
    rec = np.zeros(MPC_STRIDE)
    with np.errstate(all="ignore"):
        for ax in range(2):
            x, xd, u = st[2 * ax], st[2 * ax + 1], pv["U"][ax, 0]
            rec[3 * ax:3 * ax + 3] = x + dt * xd + (dt * dt) / 2 * u, xd + dt * u, u
            rec[6 + ax] = pv["Z"][ax, 0]
    rec[8:13] = st[:5]
    flags = pv["flags"] & ~FLAG_NONFINITE
    if not np.isfinite(rec[0:8]).all():
        flags |= FLAG_NONFINITE
    rec[13], rec[14], rec[15] = pv["k"], flags, pv["active"].sum()
    return rec, pv


def lip_box_rollout(zx, zy, box, lip, n_ticks, N, mpc_dt, z_com, alpha=1e-3, beta=1.0, gravity=9.81, xscale=1.0, max_rounds=MPC_BOX_MAX_ROUNDS):
    """The numpy statement of lmh_mpc_box_rollout for ONE robot: n_ticks times { lip_box_step; its sample; x <- sample[0], xdot <-
    sample[1], y <- sample[3], ydot <- sample[4], t <- t + mpc_dt }, every tick from the empty working set.
    -> (lip [8] after the last tick, samples [n_ticks,16])."""
    if int(n_ticks) != n_ticks or n_ticks < 0:
        raise ValueError("n_ticks must be a whole number >= 0")
    st = np.zeros(LIP_STRIDE)
    st[:min(len(lip), LIP_STRIDE)] = np.asarray(lip, dtype=np.float64)[:LIP_STRIDE]
    out = np.zeros((int(n_ticks), MPC_STRIDE))
    for tick in range(int(n_ticks)):
        out[tick], _ = lip_box_step(zx, zy, box, st, N, mpc_dt, z_com, alpha, beta, gravity, xscale, max_rounds)
        st[0], st[1], st[2], st[3] = out[tick, 0], out[tick, 1], out[tick, 3], out[tick, 4]
        st[4] = st[4] + np.float64(mpc_dt)
    return st, out


# the refusals of lmh_set_pushes, word for word (lmh_capi.hip, push_schedule_error)
PUSH_ERR_TICK = "push ticks must be whole numbers in [0, 2^31), or -1 for an unused record"
PUSH_ERR_ORDER = "a used push record follows an unused one"
PUSH_ERR_INCREASING = "push ticks must be strictly increasing"
PUSH_ERR_DV = "push dv must be finite"
PUSH_ERR_COUNT = "n_push must be at most LMH_MAX_PUSHES (16)"
PUSH_ERR_SETS = "n_sets must be 1 or n_instances"


def check_push_records(records, n_instances=None):
    """The rules of lmh_set_pushes on records [n_sets, n_push, 32] as they stand (nothing is sorted): raises ValueError with the
    library's wording, the first offending robot named ("robot 7: ...")."""
    rec = np.asarray(records, dtype=np.float64)
    if rec.ndim != 3 or rec.shape[2] != PUSH_STRIDE:
        raise ValueError("push records must be [n_sets, n_push, 32]")
    if rec.shape[1] > MAX_PUSHES:
        raise ValueError(PUSH_ERR_COUNT)
    if n_instances is not None and rec.shape[0] not in (1, n_instances):
        raise ValueError(PUSH_ERR_SETS)
    for i, sched in enumerate(rec):
        prev, unused = -1.0, False
        for r in sched:
            tk = r[0]
            if tk == -1.0:
                unused = True
                continue
            if not (tk >= 0.0) or not (tk < 2147483648.0) or tk != np.floor(tk):
                raise ValueError(f"robot {i}: {PUSH_ERR_TICK}")
            if unused:
                raise ValueError(f"robot {i}: {PUSH_ERR_ORDER}")
            if not (tk > prev):
                raise ValueError(f"robot {i}: {PUSH_ERR_INCREASING}")
            if not np.isfinite(r[1:31]).all():
                raise ValueError(f"robot {i}: {PUSH_ERR_DV}")
            prev = tk
    return rec


def push_schedule(ticks, dv, n_instances=None):
    """Host statement of the push table of lmh_set_pushes: ticks [B,n] or [n] (whole numbers; -1 = unused), dv [..,n,30] laid out as the v
    half of the state record -> records [n_sets, n, 32] = tick (as a double) | dv[30] | pad, per robot sorted by tick with the unused
    records last (tick -1, dv zero).  A [n] schedule is one shared set (n_sets = 1).  Everything lmh_set_pushes refuses is refused here
    with the same words (check_push_records): a tick that is not a whole number >= 0, two pushes of one robot on one tick, a non-finite
    dv, more than MAX_PUSHES records, n_sets not in {1, n_instances}."""
    if ticks is None or dv is None:
        raise ValueError("push_schedule needs both ticks and dv (dv [..,n,30])")
    tk = np.asarray(ticks, dtype=np.float64)
    d = np.asarray(dv, dtype=np.float64)
    if tk.ndim == 1:
        tk, d = tk[None, :], (d[None, ...] if d.ndim == 2 else d)
    if tk.ndim != 2 or d.shape != tk.shape + (30,):
        raise ValueError("ticks must be [B,n] or [n] and dv [..,n,30]")
    n_sets, n = tk.shape
    rec = np.zeros((n_sets, n, PUSH_STRIDE))
    for i in range(n_sets):
        used = tk[i] != -1.0
        order = np.concatenate([np.flatnonzero(used)[np.argsort(tk[i][used], kind="stable")], np.flatnonzero(~used)])
        rec[i, :, 0] = tk[i][order]
        rec[i, :, 1:31] = np.where(used[order][:, None], d[i][order], 0.0)
    return check_push_records(rec, n_instances)


def draw_pushes(B, n, tick_range, amplitude, seed):
    """n planar base kicks per robot in the manner of tests/helpers.perturbed_velocities (BASELINE config 2): robot i draws from
    numpy.random.default_rng(seed + i), first its n ticks -- distinct integers of [tick_range[0], tick_range[1]), in drawing order --
    then dv[:, 0:2] ~ U(-amplitude, amplitude) m/s; every other component of dv is zero.  Robot i of a batch of 16 is robot i of a
    batch of 4096.  -> (ticks [B,n] int64, dv [B,n,30])."""
    lo, hi = int(tick_range[0]), int(tick_range[1])
    if hi - lo < n:
        raise ValueError("tick_range holds fewer than n ticks")
    ticks = np.zeros((B, n), dtype=np.int64)
    dv = np.zeros((B, n, 30))
    for i in range(B):
        rng = np.random.default_rng(seed + i)
        ticks[i] = lo + rng.choice(hi - lo, size=n, replace=False)
        dv[i, :, 0:2] = rng.uniform(-amplitude, amplitude, (n, 2))
    return ticks, dv


def zoh_hold_pieces(ticks, n0, n_ticks, n_substeps):
    """Host statement of where one robot's pushes fall in a launch of lmh_rollout_zoh_ex (include/lmh.h): ticks [n] is the robot's schedule
    as lmh_set_pushes keeps it (plant substep numbers, strictly increasing, unused trailing records -1), n0 = llrint(state[90] / dt) the
    robot's substep number at the start of the launch.  -> one (start, pieces) per control tick: `start` is the index of the record applied
    before that tick's evaluation (v += dv; None: none), `pieces` the hold as a list of (substeps, record or None) -- plant_step(substeps),
    then v += dv of that record; the substeps of a tick's pieces add up to n_substeps and only the last piece may end without a push.
    Records below n0 are in the past and appear nowhere; nor does one on the substep the launch ends on, n0 + n_ticks * n_substeps: the
    next launch applies it before its first evaluation."""
    n0, n_ticks, n_substeps = int(n0), int(n_ticks), int(n_substeps)
    if n_ticks < 0 or n_substeps < 0:
        raise ValueError("n_ticks and n_substeps must be >= 0")
    due = {int(tk): c for c, tk in enumerate(np.asarray(ticks, dtype=np.float64)) if tk >= 0.0}
    if len(due) and n_ticks > 0 and n_substeps == 0:
        raise ValueError("pushes need n_substeps > 0 (push ticks are plant substeps: with none the clock does not move)")
    result, n = [], n0
    for _ in range(n_ticks):
        start, pieces, r = due.get(n), [], n_substeps
        while r > 0:
            inside = [p for p in due if n < p < n + r]
            s = min(inside) - n if inside else r
            n, r = n + s, r - s
            pieces.append((s, due[n] if inside else None))
        result.append((start, pieces))
    return result


# the refusals of lmh_set_actuators, word for word (lmh_capi.hip, actuator_record_error)
ACT_ERR_LIMIT = "torque limits must be >= 0 (+inf: none)"
ACT_ERR_ALPHA = "alpha must be in (0, 1]"
ACT_ERR_DELAY = "delay must be a whole number in [0, LMH_ACT_MAX_DELAY (7)]"


def actuator_records(n_instances, tau_max=None, alpha=None, delay=None):
    """Host statement of the table of lmh_set_actuators: tau_max and alpha a scalar, [24] or [B,24] (None: inf / 1), delay a scalar or [B]
    (None: 0) -> records [B, 56] = tau_max[24] | alpha[24] | delay | pad.  Everything lmh_set_actuators refuses is refused here with the
    same words, the first offending robot named ("robot 7: ...")."""
    B = int(n_instances)
    rec = np.zeros((B, ACT_STRIDE))
    rec[:, ACT_OFF_TAU_MAX:ACT_OFF_TAU_MAX + 24] = np.broadcast_to(np.asarray(np.inf if tau_max is None else tau_max, dtype=np.float64), (B, 24))
    rec[:, ACT_OFF_ALPHA:ACT_OFF_ALPHA + 24] = np.broadcast_to(np.asarray(1.0 if alpha is None else alpha, dtype=np.float64), (B, 24))
    rec[:, ACT_OFF_DELAY] = np.broadcast_to(np.asarray(0.0 if delay is None else delay, dtype=np.float64), (B,))
    for i, r in enumerate(rec):
        if not (r[ACT_OFF_TAU_MAX:ACT_OFF_TAU_MAX + 24] >= 0.0).all():
            raise ValueError(f"robot {i}: {ACT_ERR_LIMIT}")
        a = r[ACT_OFF_ALPHA:ACT_OFF_ALPHA + 24]
        if not ((a > 0.0) & (a <= 1.0)).all():
            raise ValueError(f"robot {i}: {ACT_ERR_ALPHA}")
        d = r[ACT_OFF_DELAY]
        if not (d >= 0.0) or not (d <= ACT_MAX_DELAY) or d != np.floor(d):
            raise ValueError(f"robot {i}: {ACT_ERR_DELAY}")
    return rec


def actuator_step(record, mem, cmd):
    """Host statement of the actuator of lmh_rollout_zoh_io (include/lmh.h), one control tick: record [..,56] (lmh_set_actuators), mem
    [..,192] = PREV[24] | QUEUE[7][24] (changed IN PLACE), cmd [..,24] the torques the evaluation commands -> (y [..,24], the torques the
    plant receives; limited [..] bool, whether a joint's torque was cut: LMH_FLAG_TAU_LIMIT).  Latency in control ticks through the queue
    (slots at and above the delay are never touched), then the limit (a NaN passes through), then the first-order lag y = alpha * c +
    (1 - alpha) * PREV with every operation rounded on its own (PREV is not read where alpha is 1), and PREV <- y.  One robot or a batch."""
    rec, cmd_ = np.asarray(record, dtype=np.float64), np.asarray(cmd, dtype=np.float64)
    if not isinstance(mem, np.ndarray) or mem.dtype != np.float64 or not mem.flags.c_contiguous or mem.shape[-1] != ACT_MEM_STRIDE \
            or rec.shape[-1] != ACT_STRIDE or cmd_.shape[-1] != 24:
        raise ValueError("actuator_step takes record [..,56], mem [..,192] (a contiguous float64 array, changed in place) and cmd [..,24]")
    lead = mem.shape[:-1]
    rec2 = np.broadcast_to(rec, lead + (ACT_STRIDE,)).reshape(-1, ACT_STRIDE)
    cmd2 = np.broadcast_to(cmd_, lead + (24,)).reshape(-1, 24)
    mem2 = mem.reshape(-1, ACT_MEM_STRIDE)                           # a view: mem is contiguous
    y = np.empty((len(mem2), 24))
    limited = np.zeros(len(mem2), dtype=bool)
    with np.errstate(invalid="ignore"):
        for i in range(len(mem2)):
            lim, alpha, d = rec2[i, ACT_OFF_TAU_MAX:ACT_OFF_TAU_MAX + 24], rec2[i, ACT_OFF_ALPHA:ACT_OFF_ALPHA + 24], int(rec2[i, ACT_OFF_DELAY])
            prev, queue = mem2[i, 0:24], mem2[i, 24:].reshape(ACT_MAX_DELAY, 24)
            if d == 0:
                u = cmd2[i].copy()
            else:
                u = queue[0].copy()
                queue[0:d - 1] = queue[1:d].copy()
                queue[d - 1] = cmd2[i]
            c = np.where(u > lim, lim, np.where(u < -lim, -lim, u))
            limited[i] = bool((c != u).any())
            lag = alpha != 1.0
            yi = c.copy()
            yi[lag] = (alpha[lag] * c[lag]) + ((1.0 - alpha[lag]) * prev[lag])
            prev[:] = yi
            y[i] = yi
    return y.reshape(lead + (24,)), limited.reshape(lead)


# the refusal of lmh_set_servo, word for word (lmh_capi.hip, servo_record_error)
SERVO_ERR_GAIN = "servo gains must be finite and >= 0"


def servo_records(n_instances, kp=0.0, kd=0.0):
    """Host statement of the table of lmh_set_servo: kp (N m / rad) and kd (N m s / rad) a scalar, [24] or [B,24] -> records [B,48] =
    kp[24] | kd[24].  What lmh_set_servo refuses is refused here with the same words, the first offending robot named ("robot 7: ...")."""
    B = int(n_instances)
    rec = np.zeros((B, SERVO_STRIDE))
    rec[:, SERVO_OFF_KP:SERVO_OFF_KP + 24] = np.broadcast_to(np.asarray(kp, dtype=np.float64), (B, 24))
    rec[:, SERVO_OFF_KD:SERVO_OFF_KD + 24] = np.broadcast_to(np.asarray(kd, dtype=np.float64), (B, 24))
    for i, r in enumerate(rec):
        if not (np.isfinite(r) & (r >= 0.0)).all():
            raise ValueError(f"robot {i}: {SERVO_ERR_GAIN}")
    return rec


def servo_torque(rec, setpoint, q, v, tau):
    """Host statement of the joint servo (include/lmh.h): rec [..,48] (lmh_set_servo), setpoint [..,48] = q_des[24] | v_des[24], q and v
    [..,30] the stage's state, tau [..,30] the feed-forward tau30 -> the tau30 the derivative uses.  Rows 6..29 are
    tau + ((kp * (q_des - q)) + (kd * (v_des - v))), every operation rounded on its own in this order; rows 0..5 are tau's."""
    rec, sp = np.asarray(rec, dtype=np.float64), np.asarray(setpoint, dtype=np.float64)
    q, v, tau = np.asarray(q, dtype=np.float64), np.asarray(v, dtype=np.float64), np.asarray(tau, dtype=np.float64)
    if rec.shape[-1] != SERVO_STRIDE or sp.shape[-1] != SETPOINT_STRIDE or q.shape[-1] != 30 or v.shape[-1] != 30 or tau.shape[-1] != 30:
        raise ValueError("servo_torque takes rec [..,48], setpoint [..,48], q, v and tau [..,30]")
    kp, kd = rec[..., SERVO_OFF_KP:SERVO_OFF_KP + 24], rec[..., SERVO_OFF_KD:SERVO_OFF_KD + 24]
    out = np.array(np.broadcast_to(tau, np.broadcast_shapes(tau.shape, q.shape[:-1] + (30,), rec.shape[:-1] + (30,), sp.shape[:-1] + (30,))))
    with np.errstate(invalid="ignore"):
        out[..., 6:30] = tau[..., 6:30] + ((kp * (sp[..., 0:24] - q[..., 6:30])) + (kd * (sp[..., 24:48] - v[..., 6:30])))
    return out


def servo_setpoint(q_m, v_m, qdd, n_substeps, dt):
    """Host statement of the LMH_SERVO_INTEGRATE setpoint of lmh_rollout_zoh_servo (include/lmh.h): q_m, v_m, qdd [..,24] the joint words
    the evaluation read and the joint rows of its out.qdd -> setpoint [..,48] = q_des | v_des with T = n_substeps * dt, h2 = (0.5 * T) * T,
    v_des = v_m + (T * qdd), q_des = (q_m + (T * v_m)) + (h2 * qdd), every operation rounded on its own."""
    q_m, v_m, a = np.asarray(q_m, dtype=np.float64), np.asarray(v_m, dtype=np.float64), np.asarray(qdd, dtype=np.float64)
    T = np.float64(float(int(n_substeps))) * np.float64(dt)
    h2 = (np.float64(0.5) * T) * T
    with np.errstate(invalid="ignore", over="ignore"):
        return np.concatenate([(q_m + (T * v_m)) + (h2 * a), v_m + (T * a)], axis=-1)


def ground_planes(slope, azimuth, h_r=0.0, h_l=0.0):
    """Ground records of lmh_set_ground for a common slope and per-foot offsets: slope (radians, |slope| < pi / 2) is the tilt of the ground
    from the horizontal, azimuth (radians) the horizontal direction in which it RISES, h_r / h_l the offsets of the right and the left foot's
    plane along the common normal (metres; different values are a ledge).  Scalars or arrays of one entry per robot, broadcast against each
    other -> records [..., 8] = n | h_r | n | h_l with n = (-sin slope cos azimuth, -sin slope sin azimuth, cos slope).  ground_slope is
    the way back."""
    s, a, hr, hl = np.broadcast_arrays(*(np.asarray(x, dtype=np.float64) for x in (slope, azimuth, h_r, h_l)))
    if not (np.abs(s) < 0.5 * np.pi).all():
        raise ValueError("slope must be inside (-pi / 2, pi / 2): the normal points up")
    n = np.stack([-np.sin(s) * np.cos(a), -np.sin(s) * np.sin(a), np.cos(s)], axis=-1)
    rec = np.zeros(s.shape + (GROUND_STRIDE,))
    rec[..., GROUND_OFF_N_R:GROUND_OFF_N_R + 3], rec[..., GROUND_OFF_H_R] = n, hr
    rec[..., GROUND_OFF_N_L:GROUND_OFF_N_L + 3], rec[..., GROUND_OFF_H_L] = n, hl
    return rec


def ground_slope(records):
    """(slope >= 0, azimuth, h_r, h_l) of the right foot's plane of records [..., 8]: ground_planes' arguments for a record it made with
    slope >= 0 (the azimuth of a horizontal plane is 0)."""
    rec = np.asarray(records, dtype=np.float64)
    n = rec[..., GROUND_OFF_N_R:GROUND_OFF_N_R + 3]
    hor = np.hypot(n[..., 0], n[..., 1])
    return np.arctan2(hor, n[..., 2]), np.where(hor > 0.0, np.arctan2(-n[..., 1], -n[..., 0]), 0.0), rec[..., GROUND_OFF_H_R], rec[..., GROUND_OFF_H_L]


GROUND_REGIMES = ("out", "stick", "slide", "lifted")


def ground_contact(pos, vel, planes, k, d, dt, mu):
    """Host statement of the contact model of lmh_set_ground (include/lmh.h): pos, vel [8,3] the world positions and velocities of the sole
    vertices (foot-major, right foot first), planes [8] one ground record, k / d / dt / mu the robot's contact_k / contact_d / contact_dt /
    contact_mu -> (f [8,3] the force at every vertex, regimes [8]): "out" of the ground (exactly 0) | "lifted" (penetrating, the normal
    force clamped to 0: exactly 0 too) | "slide" (the tangential force scaled back onto the friction disc mu f_n) | "stick"."""
    pos, vel, rec = np.asarray(pos, dtype=np.float64), np.asarray(vel, dtype=np.float64), np.asarray(planes, dtype=np.float64)
    if pos.shape != (8, 3) or vel.shape != (8, 3) or rec.shape != (GROUND_STRIDE,):
        raise ValueError("ground_contact takes pos [8,3], vel [8,3] and one ground record [8]")
    f, regimes = np.zeros((8, 3)), []
    for i in range(8):
        off = GROUND_OFF_N_L if i >= 4 else GROUND_OFF_N_R
        n, h = rec[off:off + 3], rec[off + 3]
        pen = h - n @ pos[i]
        vn = n @ vel[i]
        fn = max(0.0, k * pen - d * vn)
        ft = -dt * (vel[i] - vn * n)
        mag = np.sqrt(ft @ ft)
        slide = mag > mu * fn
        if slide:
            ft = ft * (mu * fn / mag)
        if not pen > 0.0:
            regimes.append("out"); continue
        f[i] = ft + fn * n
        regimes.append("lifted" if fn == 0.0 else "slide" if slide else "stick")
    return f, regimes


RIGID_ROWS = {PHASE_DOUBLE: tuple(range(12)), PHASE_RIGHT: tuple(range(6)), PHASE_LEFT: tuple(range(6, 12)), PHASE_FLIGHT: ()}


def gauss_jordan_unpivoted(A, b):
    """x with A x = b by Gauss-Jordan elimination without pivoting, pivot after pivot in order, as the register solves of the kernels run
    it -> (x, pivots): pivots[j] is the j-th pivot as the elimination met it."""
    A, b = np.array(A, dtype=np.float64), np.array(b, dtype=np.float64)
    n = len(b)
    piv = np.zeros(n)
    for j in range(n):
        piv[j] = A[j, j]
        for i in range(n):
            if i != j:
                f = A[i, j] / A[j, j]
                A[i, j + 1:] -= f * A[j, j + 1:]
                b[i] -= f * b[j]
                A[i, j] = 0.0
    return b / np.diag(A), piv


def _rigid_multiplier(rows, M, Js, rhs, flag_pull, flag_slip, contact_mu):
    """What the two statements below share for the held rows (Js = J[rows]): Y = M^-1 Js', A = Js Y, lam[rows] = -A^-1 rhs by the unpivoted
    Gauss-Jordan, per held foot flag_pull (f_z < 0) | flag_slip (hypot(f_x, f_y) > contact_mu f_z) -> (Y, A, lam [12], pivots, bits)."""
    Y = np.linalg.solve(M, Js.T)
    A = Js @ Y
    x, piv = gauss_jordan_unpivoted(A, rhs)
    lam, bits = np.zeros(12), 0
    lam[rows] = -x
    for ft in range(2):
        if 6 * ft in rows:
            fx, fy, fz = lam[6 * ft + 3:6 * ft + 6]
            bits |= flag_pull if fz < 0.0 else 0
            bits |= flag_slip if np.hypot(fx, fy) > contact_mu * fz else 0
    return Y, A, lam, piv, bits


def rigid_contact_acceleration(M, C, J, Jpqp, vhat, tau30, mode, kv, contact_mu=0.7, info=None):
    """The numpy statement of the rigid-contact plant (include/lmh.h, lmh_plant_derivative_rigid) for ONE robot, in the coordinates of M:
    M [30,30], C [30], J [12,30], Jpqp [12] (the soles' Jdot qdot), vhat [30] (v in M's coordinates), tau30 [30] (None: passive), mode (only
    the low two bits are read) and kv >= 0 -> (a [30], lam [12], flags).  Schur form: a0 = M^-1 (tau30 - C), Y = M^-1 J_S', A = J_S Y,
    g = J_S a0 + Jpqp_S + kv J_S vhat, lam_S = -A^-1 g by the unpivoted Gauss-Jordan, a = a0 + Y lam_S; lam is exactly 0 on the rows that
    are not held and LMH_PHASE_FLIGHT is a0 itself.  flags: FLAG_CONTACT_PULL (a held foot's f_z < 0), FLAG_CONTACT_SLIP (hypot(f_x, f_y) >
    contact_mu f_z on a held foot), FLAG_NONFINITE.  info (a dict, optional) receives A, g, Y, a0, rows and the pivots."""
    M, C, J = np.asarray(M, dtype=np.float64), np.asarray(C, dtype=np.float64), np.asarray(J, dtype=np.float64)
    tau30 = np.zeros(30) if tau30 is None else np.asarray(tau30, dtype=np.float64)
    if not (kv >= 0.0 and np.isfinite(kv)):
        raise ValueError("kv must be finite and >= 0")
    rows = list(RIGID_ROWS[int(mode) & 3])
    a0 = np.linalg.solve(M, tau30 - C)
    lam, a, flags = np.zeros(12), a0, 0
    if rows:
        Js = J[rows]
        g = Js @ a0 + np.asarray(Jpqp, dtype=np.float64)[rows] + kv * (Js @ np.asarray(vhat, dtype=np.float64))
        Y, A, lam, piv, flags = _rigid_multiplier(rows, M, Js, g, FLAG_CONTACT_PULL, FLAG_CONTACT_SLIP, contact_mu)
        a = a0 + Y @ lam[rows]
        if info is not None:
            info.update(A=A, g=g, Y=Y, a0=a0, rows=rows, pivots=piv)
    if not (np.all(np.isfinite(a)) and np.all(np.isfinite(lam))):
        flags |= FLAG_NONFINITE
    return a, lam, flags


def rigid_contact_impact(M, J, vhat, mode, contact_mu=0.7, info=None):
    """The numpy statement of the rigid plant's plastic impact (include/lmh.h, lmh_plant_impact_rigid) for ONE robot, in the coordinates of
    M: M [30,30], J [12,30], vhat [30] (v in M's coordinates) and mode (only the low two bits are read) -> (dvhat [30], impulse [12],
    flags).  The velocity jumps to the nearest one, in the metric of M, at which every held sole rests: w = J_S vhat, Y = M^-1 J_S',
    A = J_S Y, Lam_S = -A^-1 w by the unpivoted Gauss-Jordan, dvhat = Y Lam_S; ALL rows the mode holds take part.  The impulse is exactly 0
    on the rows that are not held, and LMH_PHASE_FLIGHT gives exact zeros for both.  flags: FLAG_IMPULSE_PULL (a held foot's f_z < 0: the
    sole was leaving the ground), FLAG_IMPULSE_SLIP (hypot(f_x, f_y) > contact_mu f_z on a held foot), FLAG_NOT_SPD (a pivot of A was not
    positive), FLAG_NONFINITE.  info (a dict, optional) receives A, w, Y, rows and the pivots."""
    M, J, vhat = np.asarray(M, dtype=np.float64), np.asarray(J, dtype=np.float64), np.asarray(vhat, dtype=np.float64)
    rows = list(RIGID_ROWS[int(mode) & 3])
    lam, dvhat, flags = np.zeros(12), np.zeros(30), 0
    if rows:
        Js = J[rows]
        w = Js @ vhat
        Y, A, lam, piv, flags = _rigid_multiplier(rows, M, Js, w, FLAG_IMPULSE_PULL, FLAG_IMPULSE_SLIP, contact_mu)
        dvhat = Y @ lam[rows]
        if info is not None:
            info.update(A=A, w=w, Y=Y, rows=rows, pivots=piv)
        if not np.all(piv > 0.0):
            flags |= FLAG_NOT_SPD
    if not (np.all(np.isfinite(dvhat)) and np.all(np.isfinite(lam)) and np.all(np.isfinite(vhat))):
        flags |= FLAG_NONFINITE
    return dvhat, lam, flags


def rigid_modes(phase_samples, k):
    """The modes lmh_plant_step_rigid takes for a walking host loop: the support phase of the plan(s) at preview index k (preview_index(t,
    mpc_dt) of the controller evaluation the hold follows), clamped into the arrays as the kernels clamp it.  phase_samples [n] or [B,n]
    (walk_plan / jump_plan / walk_plans) -> int32 scalar array or [B]: PHASE_DOUBLE holds both soles, PHASE_RIGHT / PHASE_LEFT the
    supporting one, PHASE_FLIGHT none."""
    ph = np.asarray(phase_samples)
    if ph.ndim not in (1, 2) or ph.shape[-1] < 1:
        raise ValueError("phase_samples must be [n] or [B,n] with n >= 1")
    k = int(np.clip(int(k), 0, ph.shape[-1] - 1))
    return (ph[..., k].astype(np.int32) & 3).astype(np.int32)


__all__ = ["stance_zmp", "find_poly_coeff", "foot_coeff_trajectory", "walk_plan", "jump_plan", "walk_plans", "jump_plans",
           "push_schedule", "check_push_records", "draw_pushes", "zoh_hold_pieces", "actuator_records", "actuator_step", "ground_planes", "ground_slope", "ground_contact",
           "preview_index", "lip_rollout", "com_targets", "rigid_contact_acceleration", "rigid_contact_impact", "FLAG_IMPULSE_PULL", "FLAG_IMPULSE_SLIP", "rigid_modes", "gauss_jordan_unpivoted", "RIGID_ROWS",
           "PHASE_DOUBLE", "PHASE_RIGHT", "PHASE_LEFT", "PHASE_FLIGHT"]
