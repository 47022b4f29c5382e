"""LMH_PRECISION_FP32 held to the oracle stage by stage, robot by robot.

LMH_PRECISION_FP32 is a second implementation of the whole-body QP (qp_setup_f32, gj_lds_f32, pushthrough_solve_f32, cone_pushthrough_f32,
the F32 branches of cone_qp, the fp32 recovery of phase_qp) on the R = float model-term chain.  Here every case of tests/fp32_cases.py runs
once through lmh_eval_debug and once through lmh_eval on an FP32 handle, and every robot of it is compared

  A  with exact facts (k, flags, rounds, forces of a foot out of support, Robot::v_, the friction cone to the kernel's own TOLC),
  B  model terms of the record against the oracle's, on the scales of test_stage_parity_over_the_joint_range,
  C  QP stages of the record against fp32_cases.setup_algebra(float64) on the record's OWN terms (the solver's error alone),
  D  tau, f, qdd against the full-fp64 oracle,
  E  LMH_FLAG_QP_FP64_ROUTE against the pivot classes of the free sets the kernel visited,
  F  the final active set against the oracle's,

and then G the warm start from eight incoming masks, H the two schedules, I a short closed loop, J the debug evaluation of a MIXED handle.
No assertion is a rate, a percentile or a median, and no robot is left out of a comparison it is eligible for.

Tolerances.  A and E are exact or read off the code; F is the existing allowance for degenerate ties.  C and D are bounded by
M_MARGIN x E_emul, E_emul the worst error over the case's robots of setup_algebra(float32) against setup_algebra(float64) on the same inputs
(C: the record's terms, D: the oracle's), computed here on the CPU.  M_MARGIN exists because the device sums sequentially with fmaf and
eliminates without pivoting where numpy uses LAPACK and BLAS: the worst device / emulation ratio seen on the MI355X over all cases and
quantities, rounded up to a power of two, times two.  B and I have no emulation: the worst value measured against the oracle times four,
one number per quantity for all cases, capped by what the suite already asserts of this arithmetic (1e-4 for the model terms of
test_mixed_precision_mode; 5e-2 / 5e-3 on tau / f of test_fp32_mode_single_evaluations_against_fp64).  The measured values stand beside
the constants below and in profiles/r28_fp32_parity.txt; every test prints its figures before it asserts.

These tests found the fp32 set-up forming t'' as a difference of two numbers of size w_foot |beta| (fp32_cases, module docstring).  With
that association the same run gave, against the oracle: tau 8.4e-3 (stance) .. 4.9e-1 (sweep10) of its largest entry, f 6.7e-4 .. 1.5 of
the weight, final sets different from the oracle's on 12 of the 16 robots of sweep10; now tau 1.8e-3 .. 9.3e-4, f 1.9e-4 .. 1.8e-3, none."""
import numpy as np
import pytest
import torch

import fp32_cases as fc
from helpers import WEIGHT, make_controller, oracle_system, rel_err, same_bits, vec_err

pytestmark = pytest.mark.gpu

KP_FEET = 500.0
RF_Q0 = np.array([[0.0, 0, 1], [0, -1, 0], [1, 0, 0]])
HARD = 1 | 2 | 4 | 8                              # LMH_FLAG_QP_MAXITER | NONFINITE | ZMP_RANGE | NOT_SPD
ROUTE = 16                                        # LMH_FLAG_QP_FP64_ROUTE
TOLC = 1e-5                                       # cone_qp<true>: primal sign test relative to 1 + max|c|
BPP_ROUNDS = 10                                   # lmh_config.bpp_rounds by default: block pivoting hands over to Lawson-Hanson behind it

# ---- set from the run on the MI355X recorded in profiles/r28_fp32_parity.txt
# M_MARGIN: worst device / emulation ratio over all cases and quantities of C and D = 8.37 (rows18, qdd in D) -> 16, times two.  The
# ratios above 5 are all rows18's (Y 8.07, a and qdd 8.13, D: qdd 8.37; everything else <= 4.90): the 18-row Cm is eliminated in order,
# without row exchanges.  An in-order float32 Gauss-Jordan in numpy on the record's terms gives 2.3e-4 / 3.5e-4 / 1.5e-4 on robots 0..2
# where the device has 2.7e-4 / 4.2e-4 / 1.8e-4 and LAPACK 3.4e-5 / 5.2e-5 / 2.1e-5 (15 rows: 1.1e-4, device 4.9e-5, LAPACK 3.4e-5).
# The yardstick carries two floors (stage_rows): without the one on h, rows18's emulation of h, 4.0e-5, a tenth of its own Si error where
# every other case has 2.3e-4 .. 4.9e-3, made a ratio of 29 out of a device error (1.15e-3) that is the same in every case.
M_MARGIN = 32.0
# B: worst value over all cases x 4 (T 2.60e-7, X 6.06e-7, C 1.17e-6, M 1.27e-6, AG 1.36e-6, J 3.24e-6, CoM 1.55e-7, comVel 1.29e-6,
# angMom 5.66e-8, Cg6 2.99e-10, AGpqp 3.06e-10, Jpqp 1.38e-9, href 2.15e-6, footAccRef 8.90e-7, u0 3.33e-8), all below the 1e-4 cap.  qref = kp (q0 - q) - kd v
# is fp64 arithmetic on exact inputs in every mode (measured 2.1e-16): it keeps an fp64 bar
B_BOUNDS = dict(T=1.1e-6, X=2.5e-6, C=4.7e-6, M=5.1e-6, AG=5.5e-6, J=1.3e-5, CoM=6.2e-7, comVel=5.2e-6, angMom=2.3e-7, Cg6=1.2e-9, AGpqp=1.3e-9,
                Jpqp=5.6e-9, qref=1e-12, href=8.6e-6, footAccRef=3.6e-6, u0=1.4e-7)
# I: worst tick of the closed loop x 4 (tau 5.13e-3, f / weight 2.41e-4), below the 5e-2 / 5e-3 caps
I_BOUNDS = dict(tau=2.1e-2, f=9.7e-4)
# H: out, status and Robot::v_ of lmh_eval and lmh_eval_debug were bit-identical in every case
SCHEDULES_BIT_IDENTICAL = True

STAGES = ("Y", "Si", "W", "h", "w_own", "a", "Gc", "c_rowspace", "tau", "f", "qdd")
OUTPUTS = ("tau", "f", "qdd")


def _mask32(x):
    return int(x) & 0xFFFFFFFF


def _launch(name):
    from linearmpchumanoid_amd import capi
    c = fc.case(name)
    B = c["q"].shape[0]
    assert B <= 32
    ctl = make_controller(B, fc.DT, fc.TH, fc.start()["zcom"], precision=capi.PRECISION_FP32, **c["config"], **c["gains"])
    if c["phase"]:
        ctl.set_refs(np.zeros(fc.NREF), np.full(fc.NREF, c["zmp_y"]), np.full(fc.NREF, c["phase"], dtype=np.uint8))
    else:
        ctl.set_refs_stance(2.0, 2)
    if c["links"] is not None:
        ctl.set_model(c["links"])
    res = {"max_qp_iters": int(ctl.cfg.max_qp_iters)}
    for kind in ("debug", "plain"):
        st = ctl.new_state(c["q"], c["v"], t=0.0, v_prev=c["vp"])
        status = ctl.new_status()
        if c["masks"] is not None:
            status[:, 3] = torch.as_tensor(np.array(c["masks"], dtype=np.uint32).astype(np.int32)).to(status.device)
        first = None
        for n in range(c["n_evals"]):                             # a repeated evaluation starts from the first one's final set and velocity
            r = ctl.stand_step(st, status=status, debug=(kind == "debug"))
            if n == 0 and c["n_evals"] > 1:
                torch.cuda.synchronize()
                first = dict(out=r[0].cpu().numpy().copy(), status=r[1].cpu().numpy().copy())
        torch.cuda.synchronize()
        res[kind] = dict(first=first, out=r[0].cpu().numpy(), status=r[1].cpu().numpy(), state=st.cpu().numpy(), dbg=r[2].cpu().numpy() if kind == "debug" else None)
    return res


_runs = {}
_launch_error = []


def guarded(fn, *args):
    """fn(*args), unless a launch of this module has already raised: then nothing more is started on the device."""
    if _launch_error:
        pytest.fail("an earlier launch of this module failed (%r): no further launch" % (_launch_error[0],))
    try:
        return fn(*args)
    except Exception as exc:
        _launch_error.append(exc)
        raise


def run(name):
    """One lmh_eval_debug and one lmh_eval launch per evaluation of the case on an FP32 handle, and the CPU references of every robot
    (cached per module)."""
    if name in _runs:
        return _runs[name]
    from linearmpchumanoid_amd.controller import unpack_debug
    c = fc.case(name)
    R = guarded(_launch, name)
    rob = []
    for i, r in enumerate(c["ref"]):
        d = unpack_debug(R["debug"]["dbg"][i])
        F = (~_mask32(R["debug"]["status"][i, 3])) & 0xFFFFFFFF
        src = fc.terms_from_debug(d)
        s64 = fc.setup_algebra(np.float64, *src, r["G"], F, r["params"])
        s32 = fc.setup_algebra(np.float32, *src, r["G"], F, r["params"])
        o64 = fc.algebra(name, i, np.float64)
        o32 = fc.algebra(name, i, np.float32)
        out = R["debug"]["out"][i]
        dev = dict(Y=d["Y"], Si=d["Si"], W=d["W"], h=d["h12"], a=d["a"], c=d["c"], tau=out[:24], f=out[24:36], qdd=out[36:66])
        rob.append(dict(d=d, F=F, s64=s64, s32=s32, o64=o64, o32=o32, dev=dev))
    _runs[name] = dict(R, rob=rob, case=c)
    return _runs[name]


def stage_errors(x, ref, G, F, eps):
    """The error of every compared quantity of one robot: Y, Si, W, h, a relative to the reference's largest entry; the wrench G c on
    weight + max|G c| and the row-space part of c on 1 + max c (test_cone_qp_and_outputs_over_the_joint_range); tau and qdd relative to
    their own largest entry, f on the robot's weight.  w_own: x's wrench against the float64 solution of the cone problem's equality form
    on x's OWN W and h (fp32_cases.solve_on), on the weight: the error of the 12 x 12 solve and of w = G c alone, without what W and h carry."""
    e = {k: rel_err(x[k], ref[k]) for k in ("Y", "Si", "W", "h", "a")}
    e["w_own"] = float(np.abs(np.asarray(x["f"], dtype=np.float64) - fc.solve_on(x["W"], x["h"], G, F, eps)).max() / WEIGHT)
    cref = np.asarray(ref["c"], dtype=np.float64)
    dc = np.asarray(x["c"], dtype=np.float64) - cref
    Gp = np.linalg.pinv(G)
    e["Gc"] = float(np.abs(G @ dc).max() / (WEIGHT + np.abs(G @ cref).max()))
    e["c_rowspace"] = float(np.abs(Gp @ (G @ dc)).max() / (1.0 + cref.max()))
    e["c_nullspace"] = float(np.abs(dc - Gp @ (G @ dc)).max() / (1.0 + cref.max()))
    e.update(output_errors(x, ref))
    return e


def stage_rows(S):
    """Per robot the device's and the emulation's stage errors of a case, and the yardstick E_emul per quantity: the worst emulation error
    over the case's robots, with two floors that keep a lucky float32 run from standing for what fp32 arithmetic delivers:
    h = Jb Si d is linear in Si, so E_emul(h) is at least E_emul(Si) (rows18: the emulation's h came out at a tenth of its own Si error);
    w is a float32 result, so E_emul(w_own) is at least half an fp32 ulp, 2^-24, of the largest wrench entry."""
    ref = S["case"]["ref"]
    args = [(ref[i]["G"], x["F"], ref[i]["params"]["eps_coeff"]) for i, x in enumerate(S["rob"])]
    dev = [stage_errors(x["dev"], x["s64"], *args[i]) for i, x in enumerate(S["rob"])]
    emu = [stage_errors(x["s32"], x["s64"], *args[i]) for i, x in enumerate(S["rob"])]
    we = _worst(emu, STAGES + ("c_nullspace",))
    we["h"] = max(we["h"], we["Si"])
    we["w_own"] = max(we["w_own"], max(2.0 ** -24 * float(np.abs(x["s64"]["f"]).max()) / WEIGHT for x in S["rob"]))
    return dev, emu, we


def output_errors(x, ref):
    return dict(tau=vec_err(x["tau"], ref["tau"]), f=float(np.abs(np.asarray(x["f"]) - ref["f"]).max() / WEIGHT), qdd=vec_err(x["qdd"], ref["qdd"]))


def _worst(rows, keys):
    return {k: max(r[k] for r in rows) for k in keys}


def _table(title, keys, dev, emul):
    print("\n%s\n  %-12s %10s %10s %8s" % (title, "quantity", "device", "emulation", "ratio"))
    ratios = {}
    for k in keys:
        ratios[k] = dev[k] / emul[k] if emul[k] > 0.0 else (0.0 if dev[k] == 0.0 else float("inf"))
        print("  %-12s %10.2e %10.2e %8.2f" % (k, dev[k], emul[k], ratios[k]))
    return ratios


def oracle_out(r):
    return dict(tau=r["e"]["tau"], f=r["e"]["f"], qdd=r["e"]["qpp"])


# ----------------------------------------------------------------------------- A
@pytest.mark.parametrize("name", fc.CASES)
def test_exact_facts(name):
    """A.  k is the oracle's; no hard flag; rounds <= max_qp_iters; a foot out of support carries exactly 0.0 and flight twelve zeros;
    Robot::v_ <- v; the friction cone holds to the kernel's own primal tolerance: the accepted c satisfies c_j >= -TOLC (1 + max|c|), so
    f_z >= -s and |f_x|, |f_y| <= mu f_z + s with s = TOLC (1 + max c) (largest column 1-norm of G)."""
    S = run(name)
    c = S["case"]
    for kind in ("debug", "plain"):
        out, status, state = S[kind]["out"], S[kind]["status"], S[kind]["state"]
        for i, r in enumerate(c["ref"]):
            assert status[i, 0] == r["e"]["k"], (kind, i, status[i].tolist())
            assert (status[i, 2] & HARD) == 0, (kind, i, status[i].tolist())
            assert 0 <= status[i, 1] <= S["max_qp_iters"], (kind, i, status[i].tolist())
            assert np.array_equal(state[i, 60:90], c["v"][i])
            f = out[i, 24:36]
            if c["phase"] in (1, 3):
                assert np.all(f[6:] == 0.0), (kind, i)                # right support | flight: the left foot carries nothing
            if c["phase"] in (2, 3):
                assert np.all(f[:6] == 0.0), (kind, i)
            cc = S["rob"][i]["d"]["c"]
            s = TOLC * (1.0 + cc.max()) * np.abs(r["G"]).sum(axis=0).max()
            mu = r["params"]["mu"]
            for ft in range(2):
                fx, fy, fz = f[6 * ft + 3], f[6 * ft + 4], f[6 * ft + 5]
                assert fz >= -s and abs(fx) <= mu * fz + s and abs(fy) <= mu * fz + s, (kind, i, ft, fx, fy, fz, s)


# ----------------------------------------------------------------------------- B
def model_term_errors(d, r, v, kpx):
    """The R = float chain's taps against the oracle's terms on the scale rules of test_stage_parity_over_the_joint_range."""
    from helpers import dense_terms_from_debug
    from oracle import restatement_np as restatement
    dd = dense_terms_from_debug(d)
    t, qp, rb = r["t"], r["qp"], r["rb"]
    e = dict(T=rel_err(dd["T"], t["T"]), X=rel_err(dd["X"], t["X"]), C=rel_err(d["C"], t["C"]), M=rel_err(dd["M"], t["M"]), AG=rel_err(d["AG"], t["AG"]),
             J=rel_err(dd["J"], t["J"]), CoM=rel_err(d["CoM"], rb["CoM"]), qref=rel_err(d["qppRef"], qp["qppRef"]), href=rel_err(d["hGpRef"], qp["hGpRef"]))
    cs = np.abs(t["C"]).max()
    e["Cg6"] = float(np.abs(d["Cg6"] - t["Cg"][:6]).max() / cs)
    e["AGpqp"] = float(np.abs(d["AGpqp"] - t["AGpqp"]).max() / cs)
    e["Jpqp"] = float(np.abs(d["Jpqp"] - t["Jpqp"]).max() / cs)
    ms = np.abs(t["AG"]).max() * max(np.abs(v).max(), 1e-300)
    mass = t["M"][3, 3]                                            # the robot's own mass (per-robot models)
    e["comVel"] = float(np.abs(d["comVel"] - rb["comVel"]).max() * mass / ms)
    e["angMom"] = float(np.abs(d["angMom"] - rb["angMom"]).max() / ms)
    psole = max(np.abs(t["T"][7][:3, 3]).max(), np.abs(t["T"][14][:3, 3]).max())
    eori = max(np.abs(restatement.rot_to_axis_angle(RF_Q0.T @ t["T"][f][:3, :3])).max() for f in (7, 14))
    fs = KP_FEET * (0.05 + psole) + KP_FEET * eori + np.abs(qp["footAccRef"]).max()
    e["footAccRef"] = float(np.abs(d["footAccRef"] - qp["footAccRef"]).max() / fs)
    us = 9.81 / 0.26 * 0.05 + abs(kpx[0]) * np.abs(rb["CoM"][:2]).max() + abs(kpx[1]) * np.abs(rb["comVel"][:2]).max() + np.abs(qp["u0"]).max()
    e["u0"] = float(np.abs(d["mpc"][:2] - qp["u0"]).max() / us)
    return e


@pytest.fixture(scope="module")
def kpx():
    o = oracle_system(fc.DT, fc.TH)
    return o.gain_row() @ o.mpc_mats()[0]


@pytest.mark.parametrize("name", fc.CASES)
def test_model_terms_against_the_oracle(name, kpx):
    """B.  T, X, C, M, AG, J, CoM, comVel, angMom, Cg6, AGpqp, Jpqp (and the references formed from them: qppRef, hGpRef, footAccRef, u0)
    of every robot's record against the oracle.  One bound per quantity for all cases: B_BOUNDS."""
    S = run(name)
    rows = [model_term_errors(S["rob"][i]["d"], r, S["case"]["v"][i], kpx) for i, r in enumerate(S["case"]["ref"])]
    worst = _worst(rows, B_BOUNDS)
    print("\n%s: fp32 model terms vs oracle: " % name + ", ".join("%s %.2e" % (k, worst[k]) for k in B_BOUNDS))
    bad = [(i, k, row[k]) for i, row in enumerate(rows) for k in B_BOUNDS if not row[k] <= B_BOUNDS[k]]
    assert not bad, bad[:12]
    assert max(worst[k] for k in ("T", "X", "M", "J")) > 1e-12       # fp32-sized: the R = float chain ran


# ----------------------------------------------------------------------------- C
@pytest.mark.parametrize("name", fc.CASES)
def test_qp_stages_against_the_float64_algebra_on_the_records_own_terms(name):
    """C.  Y, Si, W, h12, a, the wrench G c, the row-space part of c (the null-space part is printed), tau, f, qdd of every robot against
    setup_algebra(float64) on the terms and references of that robot's own record, with the device's final free set: the solver's error
    alone; and w_own, the wrench against the float64 solve on the record's own W and h.  Bound: M_MARGIN x the worst error of
    setup_algebra(float32) on the same inputs over the case's robots (stage_rows)."""
    S = run(name)
    dev, emu, we = stage_rows(S)
    wd = _worst(dev, STAGES + ("c_nullspace",))
    ratios = _table("%s: C, QP stages vs float64 algebra on the record's terms (c_nullspace is not asserted)" % name, STAGES + ("c_nullspace",), wd, we)
    print("  worst ratio %.2f" % max(ratios[k] for k in STAGES))
    bad = [(i, k, row[k], we[k]) for i, row in enumerate(dev) for k in STAGES if not row[k] <= M_MARGIN * we[k]]
    assert not bad, bad[:12]


# ----------------------------------------------------------------------------- D
@pytest.mark.parametrize("name", fc.CASES)
def test_outputs_against_the_oracle(name):
    """D.  tau (own largest entry), f (weight), qdd of every robot against the full-fp64 oracle.  Bound: M_MARGIN x the worst error of
    setup_algebra(float32) on the oracle's terms against the oracle over the case's robots.  The worst error is fp32-sized (> 1e-9): the
    fp32 path really ran."""
    S = run(name)
    ref = S["case"]["ref"]
    dev = [output_errors(x["dev"], oracle_out(ref[i])) for i, x in enumerate(S["rob"])]
    emu = [output_errors(x["o32"], oracle_out(ref[i])) for i, x in enumerate(S["rob"])]
    wd, we = _worst(dev, OUTPUTS), _worst(emu, OUTPUTS)
    ratios = _table("%s: D, outputs vs oracle" % name, OUTPUTS, wd, we)
    print("  worst ratio %.2f" % max(ratios.values()))
    bad = [(i, k, row[k], we[k]) for i, row in enumerate(dev) for k in OUTPUTS if not row[k] <= M_MARGIN * we[k]]
    assert not bad, bad[:12]
    assert max(wd.values()) > 1e-9


# ----------------------------------------------------------------------------- E
def visited_sets(S, i):
    """The free sets robot i's last evaluation solved on: the round trace of the debug record (rounds 1 .. 12 of the block-pivoting loop,
    dbg[3960 + it]), the all-free first solve (it is not traced; it runs when nothing is forced and the incoming set is all free) and the
    final set.  An untraced or empty round reads 0, which has no foot to classify."""
    c = S["case"]
    rounds = int(S["debug"]["status"][i, 1])
    dbg = S["debug"]["dbg"][i]
    sets = [S["rob"][i]["F"]] + [_mask32(dbg[3960 + it]) for it in range(1, min(rounds, 12) + 1)]
    if c["phase"] == 0 and c["masks"] is None and c["config"].get("bpp_rounds", BPP_ROUNDS) >= 0:
        sets.append(0xFFFFFFFF)
    return [F for F in sets if F]


@pytest.mark.parametrize("name", fc.CASES)
def test_route_flag(name):
    """E.  LMH_FLAG_QP_FP64_ROUTE is raised by exactly one statement: a round whose set cone_pushthrough_f32 refuses (a foot of it fails the
    1e-4 pivot rule) or that belongs to the Lawson-Hanson pass.  With the pivot classes of fp32_cases (full >= 1e-2, deficient <= 1e-8):
    in the cases whose oracle sets are full the flag is set iff a visited set is deficient or the block pivoting ran out of its
    bpp_rounds (then the Lawson-Hanson pass visited rank-deficient sets on its way up from the empty one) -- and every robot whose block
    pivoting settled must have visited full sets only and carry no flag; in the sweeps the final set is deficient or empty and the flag is set whenever it is not empty; with bpp_rounds < 0
    the flag is set on every robot.  A robot with an `unclear` set is exempt, at most 1/8 of a case's."""
    S = run(name)
    c = S["case"]
    B = len(S["rob"])
    exempt, bad, lines, n_lh = 0, [], [], 0
    for i, r in enumerate(c["ref"]):
        flag = bool(S["debug"]["status"][i, 2] & ROUTE)
        assert flag == bool(S["plain"]["status"][i, 2] & ROUTE), i
        classes = [fc.set_class(F, r["G"]) for F in visited_sets(S, i)]
        final = fc.set_class(S["rob"][i]["F"], r["G"])
        lines.append("%08x:%s%s/%d" % (S["rob"][i]["F"], final, "*" if flag else "", S["debug"]["status"][i, 1]))
        if "unclear" in classes:
            exempt += 1
            continue
        if name == "lawson":
            ok = flag
        elif name in fc.DEFICIENT_CASES:
            ok = final in ("deficient", "empty") and (flag or final == "empty")
        else:
            ran_out = int(S["debug"]["status"][i, 1]) > BPP_ROUNDS      # block pivoting did not settle: the Lawson-Hanson pass ran, from the
            n_lh += int(ran_out)                                        # empty set through single rays (rank-deficient sets, not traced)
            ok = flag == ("deficient" in classes or ran_out)
            if name in fc.FULL_CASES and not ran_out:
                ok = ok and not flag and all(k == "full" for k in classes)
        if not ok:
            bad.append((i, flag, classes))
    print("\n%s: final free sets (* = LMH_FLAG_QP_FP64_ROUTE) / rounds: %s | exempt %d, Lawson-Hanson after %d rounds %d" % (name, " ".join(lines), exempt, BPP_ROUNDS, n_lh))
    assert not bad, bad[:12]
    assert exempt <= B // 8, exempt


def test_lawson_hanson_and_block_pivoting_reach_one_minimiser():
    """E, lawson: bpp_rounds = -1 sends every robot through the fp64 free-set route on the fp32 W and h; the fp32 push-through route of
    `stance` on the same eight states lands on the same tau, f, qdd within bound C.  W and h of the two launches are the same bits, so
    the routes differ in the 12 x 12 solve alone: f also agrees within M_MARGIN x the sum of the two cases' E_emul(w_own)."""
    L, S = run("lawson"), run("stance")
    n = len(L["rob"])
    emu = _worst([output_errors(x["s32"], x["s64"]) for x in S["rob"][:n]] + [output_errors(x["s32"], x["s64"]) for x in L["rob"]], OUTPUTS)
    rows = [output_errors(L["rob"][i]["dev"], S["rob"][i]["dev"]) for i in range(n)]
    worst = _worst(rows, OUTPUTS)
    _table("lawson vs stance, same states: two routes", OUTPUTS, worst, emu)
    for i in range(n):
        assert np.array_equal(L["rob"][i]["d"]["W"], S["rob"][i]["d"]["W"]) and np.array_equal(L["rob"][i]["d"]["h12"], S["rob"][i]["d"]["h12"])
    bad = [(i, k, row[k]) for i, row in enumerate(rows) for k in OUTPUTS if not row[k] <= M_MARGIN * emu[k]]
    assert not bad, bad
    own = stage_rows(L)[2]["w_own"] + stage_rows(S)[2]["w_own"]
    print("  f between the routes %.2e, E_emul(w_own) of the two cases %.2e" % (worst["f"], own))
    assert worst["f"] <= M_MARGIN * own, (worst["f"], own)


# ----------------------------------------------------------------------------- F
@pytest.mark.parametrize("name", fc.CASES)
def test_final_active_set_against_the_oracle(name):
    """F.  The device's final ACTIVE mask equals the oracle's, up to B // 6 robots with degenerate (c_j = 0) ties (measured: no mismatch
    in any case).  `lawson` first ended on fff8fff8 and ff0fff0f on robots 1 and 6 where the oracle has fffcfffc and ff2fff2f: the
    Lawson-Hanson pass stopped with multipliers of -1.8e-9 and -1.5e-9 left, below its stopping tolerance 1e-14 (1 + max|q|) = 2.2e-9,
    and coefficients of 3 % and 2 % of max c left out (the wrench did not move: the multiplier of a coefficient on a foot that has
    free ones is -eps_coeff s_j).  The fp32 pass now ends with the push-through form of those multipliers, as block pivoting tests them."""
    S = run(name)
    mism = [i for i, r in enumerate(S["case"]["ref"]) if _mask32(S["debug"]["status"][i, 3]) != r["e"]["active_mask"]]
    print("\n%s: mask mismatches %s" % (name, [(i, "%08x" % S["rob"][i]["F"], "%08x" % S["case"]["ref"][i]["F"]) for i in mism]))
    assert len(mism) <= len(S["rob"]) // 6, mism


# ----------------------------------------------------------------------------- G
def test_warm_start_from_any_mask_reaches_the_same_set():
    """G.  One state, eight incoming masks (all free, all bound, the oracle's final set, its complement, four random ones), two
    consecutive evaluations with warm_start = 1: bounds C and D hold for every robot (the `warm` case of the tests above); here the eight
    final masks agree with one another up to the tie allowance, on both schedules.  The second evaluation starts from the first one's
    final set, so the incoming masks act on the FIRST evaluation: its final masks must agree with one another and with the oracle's
    single evaluation up to the same allowance, with no hard flag, and its tau, f, qdd lie within bound D."""
    S = run("warm")
    c = S["case"]
    # the FIRST evaluation is the one the eight masks come into: its final masks agree, and its outputs lie within bound D of the oracle's
    # single evaluation of that state
    r1 = fc._evaluate(c, 0, 1)
    src = fc.terms_from_oracle(r1)
    e1 = output_errors(fc.setup_algebra(np.float32, *src, r1["G"], r1["F"], r1["params"]), oracle_out(r1))
    for kind in ("debug", "plain"):
        out, st1 = S[kind]["first"]["out"], S[kind]["first"]["status"]
        masks = [_mask32(x) for x in st1[:, 3]]
        common = max(set(masks), key=masks.count)
        rows = [output_errors(dict(tau=out[i, :24], f=out[i, 24:36], qdd=out[i, 36:66]), oracle_out(r1)) for i in range(len(masks))]
        print("\nwarm (%s), first evaluation: final %s (oracle %08x), rounds %s, worst tau %.2e f %.2e qdd %.2e" % (
            kind, " ".join("%08x" % m for m in masks), r1["e"]["active_mask"], st1[:, 1].tolist(), *(max(r[k] for r in rows) for k in OUTPUTS)))
        assert ((st1[:, 2] & HARD) == 0).all()
        assert sum(m != common for m in masks) <= len(masks) // 6, masks
        assert sum(m != r1["e"]["active_mask"] for m in masks) <= len(masks) // 6, masks
        bad = [(i, k, r[k]) for i, r in enumerate(rows) for k in OUTPUTS if not r[k] <= M_MARGIN * e1[k]]
        assert not bad, bad
    for kind in ("debug", "plain"):
        masks = [_mask32(x) for x in S[kind]["status"][:, 3]]
        common = max(set(masks), key=masks.count)
        print("\nwarm (%s): incoming %s -> final %s, rounds %s" % (kind, " ".join("%08x" % m for m in S["case"]["masks"]), " ".join("%08x" % m for m in masks),
                                                                 S[kind]["status"][:, 1].tolist()))
        assert sum(m != common for m in masks) <= len(masks) // 6, masks


# ----------------------------------------------------------------------------- H
@pytest.mark.parametrize("name", fc.CASES)
def test_two_wave_and_single_wave_schedules(name):
    """H.  lmh_eval (two waves; the fp32 QP runs on wave 0 alone) and lmh_eval_debug (one wave) on the same FP32 handle and states: the
    plain launch's tau, f, qdd within bounds C (against the float64 algebra on the record's terms) and D (against the oracle), and out,
    status and Robot::v_ bit-identical to the debug launch's, as test_two_wave_schedule_is_deterministic_and_equals_the_single_wave_schedule
    asserts of fp64."""
    S = run(name)
    ref = S["case"]["ref"]
    po = S["plain"]["out"]
    plain = [dict(tau=po[i, :24], f=po[i, 24:36], qdd=po[i, 36:66]) for i in range(len(ref))]
    eC = _worst([output_errors(x["s32"], x["s64"]) for x in S["rob"]], OUTPUTS)
    eD = _worst([output_errors(x["o32"], oracle_out(ref[i])) for i, x in enumerate(S["rob"])], OUTPUTS)
    bad = []
    for i, x in enumerate(S["rob"]):
        c_, d_ = output_errors(plain[i], x["s64"]), output_errors(plain[i], oracle_out(ref[i]))
        bad += [(i, "C", k, c_[k]) for k in OUTPUTS if not c_[k] <= M_MARGIN * eC[k]] + [(i, "D", k, d_[k]) for k in OUTPUTS if not d_[k] <= M_MARGIN * eD[k]]
    same = (same_bits(S["plain"]["out"][:, :78], S["debug"]["out"][:, :78]) and same_bits(S["plain"]["status"], S["debug"]["status"])
            and same_bits(S["plain"]["state"], S["debug"]["state"]))
    print("\n%s: lmh_eval and lmh_eval_debug bit-identical: %s" % (name, same))
    assert not bad, bad[:12]
    assert same == SCHEDULES_BIT_IDENTICAL


# ----------------------------------------------------------------------------- I
def test_closed_loop_against_the_oracle_rollout():
    """I.  lmh_rollout of 12 ticks, 16 robots of the stance draw, FP32 handle with warm_start = 1 (lmh_rollout_kernel<float, true, ..>, the
    schedule without the pipelined look-ahead) against Oracle.rollout's log: k bit-exact, no hard flag, tau (own largest entry) and f
    (weight) of EVERY tick of EVERY robot inside I_BOUNDS."""
    from linearmpchumanoid_amd import capi
    B, nt = 16, 12
    q, v, vp = fc.stance_states(B)

    def launch():
        ctl = make_controller(B, fc.DT, fc.TH, fc.start()["zcom"], warm_start=1, precision=capi.PRECISION_FP32)
        ctl.set_refs_stance(2.0, 2)
        st = ctl.new_state(q, v, t=0.0, v_prev=vp)
        out, status, log = ctl.rollout(st, nt, log=True)
        torch.cuda.synchronize()
        return log.cpu().numpy(), status.cpu().numpy()
    log, status = guarded(launch)
    worst, bad = dict(tau=0.0, f=0.0), []
    for i in range(B):
        o = oracle_system(fc.DT, fc.TH, sim_time=1.0)
        o.set_prev_velocity(vp[i])
        r = o.rollout(np.concatenate([q[i], v[i]]), 0.0, nt, log=True)
        if status[i, 0] != r["k"][-1] or (status[i, 2] & HARD):
            bad.append((i, "status", status[i].tolist()))
        for tk in range(nt):
            e = dict(tau=rel_err(log[tk, i, :24], r["log"][tk][:24]), f=float(np.abs(log[tk, i, 24:] - r["log"][tk][24:]).max() / WEIGHT))
            for k in e:
                worst[k] = max(worst[k], e[k])
                if not e[k] <= I_BOUNDS[k]:
                    bad.append((i, tk, k, e[k]))
    print("\nclosed loop, FP32, %d ticks x %d robots vs oracle: tau %.2e, f/weight %.2e" % (nt, B, worst["tau"], worst["f"]))
    assert not bad, (len(bad), bad[:12])
    assert worst["tau"] > 1e-9


# ----------------------------------------------------------------------------- J
def test_debug_evaluation_of_a_mixed_handle_is_the_fp64_one():
    """J.  lmh_eval_debug has an fp64 and an FP32 instantiation: on a MIXED handle it evaluates in fp64 (include/lmh.h), so its out and
    status are the bits of an FP64 handle's, and so is its record; the fp32 model-term taps are read on an FP32 handle (B above)."""
    from linearmpchumanoid_amd import capi
    q, v, vp = fc.stance_states(8)
    def launch(prec):
        ctl = make_controller(8, fc.DT, fc.TH, fc.start()["zcom"], warm_start=0, precision=prec)
        ctl.set_refs_stance(2.0, 2)
        st = ctl.new_state(q, v, t=0.0, v_prev=vp)
        out, status, dbg = ctl.stand_step(st, debug=True)
        torch.cuda.synchronize()
        return out.cpu().numpy(), status.cpu().numpy(), dbg.cpu().numpy()[:, :3211]
    res = {prec: guarded(launch, prec) for prec in (capi.PRECISION_FP64, capi.PRECISION_MIXED)}
    a, b = res[capi.PRECISION_FP64], res[capi.PRECISION_MIXED]
    assert same_bits(a[0][:, :78], b[0][:, :78]) and same_bits(a[1], b[1])
    assert same_bits(a[2], b[2])                                   # every named field of the record (the words behind them are clock stamps)
