"""CPU side of the LMH_PRECISION_FP32 parity tests: a numpy statement of the fp32 QP set-up's algebra, the pivot classes of a free set and
the cases (states, plans, weights, models, incoming masks) with the oracle's evaluation of every robot.  Nothing here imports the HIP library.

The algebra (qp_setup_f32, pushthrough_solve_f32, cone_pushthrough_f32 and the fp32 recovery of phase_qp, from their comments and lmh.h).
With a = x[:30] the accelerations in the base frame, w = x[30:42] the contact wrench n_R f_R n_L f_L, c the 32 cone coefficients, w = G c:

    U = [AG_lin ; J] (15 rows; 18 with the angular rows of AG when w_com_ang != 0),  Om = diag(w_com_*, w_foot),  D = diag(w_base_*, w_joints)
    beta = [AGpqp - hGpRef ; Jpqp - footAccRef],   bp' = [-qppRef | D^-1 Mb'],   Mb = M[:6]
    Cm = Om^-1 + U D^-1 U'                         (Woodbury: (D + U' Om U)^-1 = D^-1 - D^-1 U' Cm^-1 U D^-1)
    Y  = bp' - D^-1 U' t'',  t'' = Cm^-1 (U bp' - [beta | 0])                                       (30 x 7: Y_g | Y_M)
    S | d = Mb Y_M | C[:6] - Mb Y_g,   Si = sym(S^-1),   Jb = J[:, :6]
    W = w_force I + Jb Si Jb',   h = Jb Si d
    (W + eps K_F^-1) w = h on the rows of the feet that carry free coefficients, one refinement step;  K_F = G_F G_F' per foot
    c_F = G_F' K_F^-1 w,   lam = -Si (Jb' w - d),   a = -(Y_g + Y_M lam),   tau = (M a + C - J' w)[6:]

t'' has a second form, Cm^-1 U (bp' + [D^-1 U' Om beta | 0]) - [Om beta | 0] (equal because U D^-1 U' = Cm - Om^-1), which the fp64 set-up
uses to shorten its critical path.  In float32 it is useless: Om beta = w_foot (Jpqp - footAccRef) is 1e6 .. 1e7 where t'' is 1e2, and the
difference keeps two or three digits (tau of the stance case: 7e-3 instead of 1e-3 of its largest entry; of the posture sweeps: 6e-2).

A foot whose K_F is rank deficient (a few rays of one sole edge) has no K_F^-1: the kernel then leaves the 12 x 12 form for its fp64 free-set
solve (LMH_FLAG_QP_FP64_ROUTE).  Here that case is the same 12 x 12 system on range(G_F) with the pseudo-inverse of K_F, always in float64 on
the W and h of the given dtype -- the same minimiser, the arithmetic the kernel's fall-back has."""
import functools

import numpy as np

from helpers import oracle_system, perturbed_velocities, posture_sweep
from oracle import pyoracle

DT, TH = 1e-3, 0.016                              # cfg2: dt = 1 ms, N = 16
NREF = 2500                                       # samples of an uploaded plan (as the existing phase tests)
FULL_RATIO, DEFICIENT_RATIO = 1e-2, 1e-8          # pivot classes; the kernel's rule (gj_lds_f32(.., 1e-4f)) lies between them
FIELDS = ("Y", "Si", "W", "h", "w", "lam", "a", "tau", "f", "qdd")


# ----------------------------------------------------------------------------- the algebra
def wrench_map(A):
    """G [12,32] with w = G c from the oracle's constraint matrix: rows 6..17 of A state -(a permutation) w + (generators) c = 0."""
    return np.linalg.solve(-A[6:18, 30:42], A[6:18, 42:74])


def _feet(F):
    return [ft for ft in range(2) if (int(F) >> (16 * ft)) & 0xFFFF]


def _free_columns(F, ft):
    return [16 * ft + j for j in range(16) if (int(F) >> (16 * ft + j)) & 1]


def pivot_ratio(K):
    """Smallest pivot of the in-order Gauss-Jordan elimination of K (no row exchanges) over its original diagonal entry, in float64: the
    quantity gj_lds_f32's `rel` argument tests.  The elimination stops at the first pivot that is not positive (ratio 0)."""
    A = np.array(K, dtype=np.float64)
    d0 = np.diag(A).copy()
    worst = np.inf
    for j in range(A.shape[0]):
        if not (A[j, j] > 0.0 and d0[j] > 0.0):
            return 0.0
        worst = min(worst, A[j, j] / d0[j])
        if worst <= DEFICIENT_RATIO:
            return worst
        f = A[:, j] / A[j, j]
        f[j] = 0.0
        A -= np.outer(f, A[j])
    return float(worst)


def pivot_class(F, G):
    """{foot: "full" | "deficient" | "unclear"} for every foot with free coefficients in F."""
    out = {}
    for ft in _feet(F):
        Gf = G[6 * ft:6 * ft + 6][:, _free_columns(F, ft)]
        r = pivot_ratio(Gf @ Gf.T)
        out[ft] = "full" if r >= FULL_RATIO else "deficient" if r <= DEFICIENT_RATIO else "unclear"
    return out


def set_ratio(F, G):
    """The smallest in-order pivot ratio over the feet of a free set (inf for the empty set)."""
    return min((pivot_ratio(G[6 * ft:6 * ft + 6][:, _free_columns(F, ft)] @ G[6 * ft:6 * ft + 6][:, _free_columns(F, ft)].T) for ft in _feet(F)), default=np.inf)


def solve_on(W, h, G, F, eps):
    """The float64 wrench of the cone problem's equality form on GIVEN W, h and free set (range(G_F), pseudo-inverse of K_F: both routes):
    what a solver that was handed this W and h should return."""
    W64, h64, G64 = np.asarray(W, dtype=np.float64), np.asarray(h, dtype=np.float64), np.asarray(G, dtype=np.float64)
    Q, Kp = np.zeros((12, 0)), np.zeros((12, 12))
    for ft in _feet(F):
        Gf = G64[6 * ft:6 * ft + 6][:, _free_columns(F, ft)]
        lamK, V = np.linalg.eigh(Gf @ Gf.T)
        Vk = V[:, lamK > 1e-10 * lamK.max()]
        Kp[6 * ft:6 * ft + 6, 6 * ft:6 * ft + 6] = (Vk / lamK[lamK > 1e-10 * lamK.max()]) @ Vk.T
        Qf = np.zeros((12, Vk.shape[1])); Qf[6 * ft:6 * ft + 6] = Vk
        Q = np.concatenate([Q, Qf], axis=1)
    if Q.shape[1] == 0:
        return np.zeros(12)
    return Q @ np.linalg.solve(Q.T @ (W64 + eps * Kp) @ Q, Q.T @ h64)


def set_class(F, G):
    """One word for a free set: "empty", "full" (every foot in it full), "deficient" (some foot deficient, none unclear) or "unclear"."""
    cls = list(pivot_class(F, G).values())
    if not cls:
        return "empty"
    if "unclear" in cls:
        return "unclear"
    return "deficient" if "deficient" in cls else "full"


def setup_algebra(dtype, terms, refs, G, F, params, refine=True):
    """The algebra of the module docstring as plain numpy in `dtype` (inputs are rounded to it first).
    terms: M [30,30], C [30], AG [6,30], AGpqp [6], J [12,30], Jpqp [12], X0 [6,6] (base velocity matrix, for qdd);
    refs: qppRef [30], hGpRef [6], footAccRef [12]; G [12,32]; F: the free set (bit j = coefficient j free) K_F^-1 is formed for;
    params: w_com_lin, w_com_ang, w_base_pos, w_base_ang, w_joints, w_force, w_foot, eps_coeff.
    Returns dict(Y, Si, W, h, w, lam, a, tau, f, qdd) (+ c [32]).  A foot without free coefficients (out of support, or every bound
    active) has no rows in the 12 x 12 solve and its wrench is exactly 0; with no free coefficient at all there is no solve.
    refine=False leaves the refinement step of the 12 x 12 solve out (what the step is worth in a case: test_fp32_cases)."""
    T = np.dtype(dtype).type
    cast = lambda x: np.asarray(x, dtype=np.float64).astype(dtype)
    M, C, AG, J = cast(terms["M"]), cast(terms["C"]), cast(terms["AG"]), cast(terms["J"])
    AGpqp, Jpqp = cast(terms["AGpqp"]), cast(terms["Jpqp"])
    qref, href, fref = cast(refs["qppRef"]), cast(refs["hGpRef"]), cast(refs["footAccRef"])
    Gd = cast(G)
    r0 = 3 if params["w_com_ang"] == 0.0 else 0
    U = np.concatenate([AG[r0:], J])
    om = np.concatenate([[params["w_com_ang"]] * 3, [params["w_com_lin"]] * 3, [params["w_foot"]] * 12])[r0:].astype(dtype)
    iD = (T(1) / np.concatenate([[params["w_base_pos"]] * 3, [params["w_base_ang"]] * 3, [params["w_joints"]] * 24]).astype(dtype)).astype(dtype)
    beta = np.concatenate([AGpqp - href, Jpqp - fref])[r0:]
    Mb = M[:6]
    bp = np.concatenate([-qref[:, None], Mb.T * iD[:, None]], axis=1)                 # 30 x 7
    UD = U * iD[None, :]
    Cm = np.diag(T(1) / om) + UD @ U.T
    V = U @ bp
    V[:, 0] -= beta                                                                    # (not U (bp'_g + D^-1 U' Om beta), then - Om beta: see above)
    t = np.linalg.solve(Cm, V)
    Y = bp - (U.T @ t) * iD[:, None]
    S = Mb @ Y[:, 1:]
    d = C[:6] - Mb @ Y[:, 0]
    Sinv = np.linalg.inv(S)
    Si = T(0.5) * (Sinv + Sinv.T)
    Jb = J[:, :6]
    T1 = Jb @ Si
    W = T1 @ Jb.T + T(params["w_force"]) * np.eye(12, dtype=dtype)
    W = T(0.5) * (W + W.T)
    h = T1 @ d
    eps = params["eps_coeff"]
    w = np.zeros(12, dtype=dtype)
    c = np.zeros(32, dtype=dtype)
    feet = _feet(F)
    if feet:
        cls = pivot_class(F, np.asarray(G, dtype=np.float64))
        rows = np.concatenate([np.arange(6 * ft, 6 * ft + 6) for ft in feet])
        if all(cls[ft] == "full" for ft in feet):                                      # the push-through system in `dtype`
            Ki = np.zeros((12, 12), dtype=dtype)
            for ft in feet:
                Gf = Gd[6 * ft:6 * ft + 6][:, _free_columns(F, ft)]
                Kinv = np.linalg.inv(Gf @ Gf.T)
                Ki[6 * ft:6 * ft + 6, 6 * ft:6 * ft + 6] = T(0.5) * (Kinv + Kinv.T)
            A = (W + T(eps) * Ki)[np.ix_(rows, rows)]
            w0 = np.linalg.solve(A, h[rows])
            res = (h[rows].astype(np.float64) - A.astype(np.float64) @ w0.astype(np.float64)).astype(dtype)
            w[rows] = w0 + np.linalg.solve(A, res) if refine else w0                   # one refinement step, residual in float64
            y = Ki @ w
            for ft in feet:
                cols = _free_columns(F, ft)
                c[cols] = Gd[6 * ft:6 * ft + 6][:, cols].T @ y[6 * ft:6 * ft + 6]
        else:                                                                          # rank-deficient set: float64 on range(G_F)
            G64, W64, h64 = np.asarray(G, dtype=np.float64), W.astype(np.float64), h.astype(np.float64)
            Q, Kp = np.zeros((12, 0)), np.zeros((12, 12))
            for ft in feet:
                Gf = G64[6 * ft:6 * ft + 6][:, _free_columns(F, ft)]
                lamK, V = np.linalg.eigh(Gf @ Gf.T)
                keep = lamK > 1e-10 * lamK.max()
                Vk = V[:, keep]
                Kp[6 * ft:6 * ft + 6, 6 * ft:6 * ft + 6] = (Vk / lamK[keep]) @ Vk.T
                Qf = np.zeros((12, Vk.shape[1])); Qf[6 * ft:6 * ft + 6] = Vk
                Q = np.concatenate([Q, Qf], axis=1)
            yq = np.linalg.solve(Q.T @ (W64 + eps * Kp) @ Q, Q.T @ h64)
            w64 = Q @ yq
            w = w64.astype(dtype)
            yk = Kp @ w64
            for ft in feet:
                cols = _free_columns(F, ft)
                c[cols] = (G64[6 * ft:6 * ft + 6][:, cols].T @ yk[6 * ft:6 * ft + 6]).astype(dtype)
    lam = -(Si @ (Jb.T @ w - d))
    a = -(Y[:, 0] + Y[:, 1:] @ lam)
    # outputs: float64 arithmetic on the values of `dtype` (the kernel's output phases are shared by every mode)
    a64, w64 = a.astype(np.float64), w.astype(np.float64)
    tau = (M.astype(np.float64) @ a64 + C.astype(np.float64) - J.astype(np.float64).T @ w64)[6:]
    acc = np.linalg.solve(np.asarray(terms["X0"], dtype=np.float64), a64[:6])
    qdd = np.concatenate([acc[3:], acc[:3], a64[6:]])
    return dict(Y=Y, Si=Si, W=W, h=h, w=w, lam=lam, a=a, tau=tau, f=w64, qdd=qdd, c=c)


def terms_from_debug(d):
    """(terms, refs) of setup_algebra from ONE device debug record (controller.unpack_debug): the device's own model terms and references,
    so that an fp64 evaluation of the algebra on them differs from the device's QP stages by the solver's error alone."""
    from helpers import dense_terms_from_debug
    dd = dense_terms_from_debug(d)
    terms = dict(M=dd["M"], J=dd["J"], X0=dd["X"][0], C=np.array(d["C"]), AG=np.array(d["AG"]), AGpqp=np.array(d["AGpqp"]), Jpqp=np.array(d["Jpqp"]))
    refs = dict(qppRef=np.array(d["qppRef"]), hGpRef=np.array(d["hGpRef"]), footAccRef=np.array(d["footAccRef"]))
    return terms, refs


def terms_from_oracle(r):
    """(terms, refs) of setup_algebra from a robot's oracle record of a case (`ref` entries below)."""
    t, qp = r["t"], r["qp"]
    terms = dict(M=t["M"], J=t["J"], X0=t["X"][0], C=t["C"], AG=t["AG"], AGpqp=t["AGpqp"], Jpqp=t["Jpqp"])
    refs = dict(qppRef=qp["qppRef"], hGpRef=qp["hGpRef"], footAccRef=qp["footAccRef"])
    return terms, refs


# ----------------------------------------------------------------------------- the cases
CASES = ("stance", "single_R", "single_L", "flight", "rows18", "models", "lowmu", "sweep03", "sweep10", "lawson", "warm")
FULL_CASES = ("stance", "single_R", "single_L", "rows18", "models", "lowmu", "warm", "lawson")      # the oracle's final sets must all be `full`
DEFICIENT_CASES = ("sweep03", "sweep10")                                                   # ... all `deficient` (or empty)
ALGEBRA_PARAMS = ("w_com_lin", "w_com_ang", "w_base_pos", "w_base_ang", "w_joints", "w_force", "w_foot", "eps_coeff")


@functools.lru_cache(maxsize=None)
def start():
    o = oracle_system(DT, TH)
    return dict(zcom=o.zcom, q0=o.robot()["q"].copy())


def stance_states(B):
    """The draw of test_fp32_mode_single_evaluations_against_fp64: start posture, small velocities, a previous velocity close to them."""
    v = perturbed_velocities(B, seed=77) * 0.2
    return np.tile(start()["q0"], (B, 1)), v, v - perturbed_velocities(B, seed=78) * 0.004


def model_links(B):
    """Per-robot link tables: mass x U(0.9, 1.1), CoM +- 5 mm (the draw of test_domain_randomised_models)."""
    raw = np.tile(pyoracle.nao_raw_links(), (B, 1, 1))
    rng = np.random.default_rng(20260004)
    raw[:, :, 0] *= rng.uniform(0.9, 1.1, (B, 28))
    raw[:, :, 1:4] += rng.uniform(-5e-3, 5e-3, (B, 28, 3)) * (raw[:, :, 0:1] > 0)
    return raw


def _oracle_for(case, i):
    if case["links"] is not None:
        o = pyoracle.Oracle(sim_time=2.0, dt=DT, horizon_time=TH, do_ik=False, raw_links=case["links"][i])
        o.set_zcom(start()["zcom"])
    else:
        o = oracle_system(DT, TH)
    if case["gains"]:
        o.set_gains(**case["gains"])
    if case["phase"]:
        o.set_refs(np.zeros(NREF), np.full(NREF, case["zmp_y"]), np.full(NREF, case["phase"], dtype=np.uint8))
    return o


def _evaluate(case, i, n_evals=1):
    o = _oracle_for(case, i)
    o.set_prev_velocity(case["vp"][i])
    for _ in range(n_evals):                                      # a repeated evaluation sees the first one's velocity as Robot::v_
        e = o.eval(case["q"][i], case["v"][i], 0.0)
    assert e["qp_status"] == 0, (case["name"], i, e["qp_status"])
    qp = o.qp()
    par = {k: v for k, v in o.gains().items() if k in ALGEBRA_PARAMS + ("mu",)}
    return dict(e=e, t=o.terms(), qp=qp, rb=o.robot(), G=wrench_map(qp["A"]), F=(~int(e["active_mask"])) & 0xFFFFFFFF, params=par)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(name, q, v, vp [B,30], phase (0 = the stance plan's double support; else a plan of NREF samples with zmp_x = 0, zmp_y and this
    phase throughout), gains (config overrides), links ([B,28,13] or None),
    config (further lmh_config fields), masks (incoming ACTIVE masks of `warm`, else None), n_evals, ref: the oracle's record per robot
    (e, t, qp, rb, G, F = its final free set, params)).  Treat what comes back as read-only."""
    c = dict(name=name, phase=0, zmp_y=0.0, gains={}, links=None, config=dict(warm_start=0), masks=None, n_evals=1)
    if name in ("sweep03", "sweep10"):
        c["q"], c["v"], c["vp"] = posture_sweep(start()["q0"], 16, 0.3 if name == "sweep03" else 1.0)
    else:
        B = 16 if name == "stance" else 8
        c["q"], c["v"], c["vp"] = stance_states(B)
    if name in ("single_R", "single_L", "flight"):
        c["phase"] = {"single_R": 1, "single_L": 2, "flight": 3}[name]
        # With the ZMP reference between the feet (0) the start posture's centre of pressure lies on the inner edge of the support sole on
        # every robot: free set 0f0f, two vertices, rank deficient.  A reference beyond the support foot's centre (the right foot stands at
        # y = -0.05) asks for a CoM acceleration that brings the centre of pressure inside the sole.  Every robot of both cases has a full-rank
        # set (3 or 4 vertices) for |zmp_y| = 0.085 .. 0.10; at 0.08 and at 0.11 some are back on an edge: the middle of that window.
        c["zmp_y"] = {"single_R": -0.095, "single_L": 0.095, "flight": 0.0}[name]
    elif name == "rows18":
        c["gains"] = dict(w_com_ang=50.0, mu=0.5)
    elif name == "models":
        c["links"] = model_links(8)
    elif name == "lowmu":
        # narrow cones: three of the oracle's sets (de22de22, ce22ce22, ee88e6c8) have an in-order pivot ratio of 0.044 .. 0.053, full rank
        # by the kernel's 1e-4 rule and by FULL_RATIO but not by a rule of 1e-1; the sets the other cases end on have 0.71 .. 0.93
        c["gains"] = dict(mu=0.07)
    elif name == "lawson":
        c["config"] = dict(warm_start=0, bpp_rounds=-1)
    elif name == "warm":
        # ONE state eight times (the first of the stance draw whose oracle set has active bounds), so that the eight incoming masks must
        # all lead to the same final set
        st = case("stance")
        i0 = next((i for i, r in enumerate(st["ref"]) if r["F"] != 0xFFFFFFFF), 0)
        c["q"], c["v"], c["vp"] = (np.tile(st[k][i0], (8, 1)) for k in ("q", "v", "vp"))
        c["config"] = dict(warm_start=1)
        c["n_evals"] = 2
    c["ref"] = [_evaluate(c, i, c["n_evals"]) for i in range(c["q"].shape[0])]
    if name == "warm":
        # incoming FREE sets: all free, all bound, the oracle's final set, its complement, four random ones; status[3] carries the complement
        rng = np.random.default_rng(20261019)
        Fo = c["ref"][0]["F"]
        free = [0xFFFFFFFF, 0x00000000, Fo, (~Fo) & 0xFFFFFFFF] + [int(x) for x in rng.integers(0, 2 ** 32, 4, dtype=np.uint64)]
        c["masks"] = [(~m) & 0xFFFFFFFF for m in free]
    return c


def algebra(case_name, i, dtype, source=None, F=None):
    """setup_algebra of robot i of a case in `dtype`, on the oracle's terms (source None) or on (terms, refs) given; F defaults to the
    oracle's final free set."""
    r = case(case_name)["ref"][i]
    terms, refs = terms_from_oracle(r) if source is None else source
    return setup_algebra(dtype, terms, refs, r["G"], r["F"] if F is None else F, r["params"])
