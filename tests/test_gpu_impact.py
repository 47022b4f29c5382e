"""The rigid plant's plastic touchdown impact on the GPU: lmh_plant_impact_rigid against the numpy statement
(trajectories.rigid_contact_impact) on the CPU oracle's terms and on the device's own, and lmh_rollout_zoh_rigid_impact against the host loop
that DEFINES it (impact_cases.host_loop_impact: zoh_rigid_host_loop's proxy with plant_impact_rigid in front of a hold's first piece), bit
for bit on a second copy of the same buffers; only test_parity_with_the_cpu_loop goes to the CPU oracle for a loop.

Inputs: plant_step_cases.contact_states(), 16 states around touch-down, v_prev = v, warm_start = 1; six control ticks; n_substeps 3 and 1;
zoh_rigid_cases' mode words and plans, impact_cases' d_mode_prev words (their conditions are pinned on the CPU, test_impact.py, and checked
again here before a launch).  Tolerances are the project's own for the same figures (test_gpu_rigid.py, test_gpu_zoh_rigid.py): the three
figures 1e-12, the closed loop state 1e-7, tau and f 1e-6, k exact.  "Bit for bit" is helpers.same_bits.  Every test fails on a library
without the entry points: the methods and the symbols do not exist there."""
import ctypes as C

import numpy as np
import pytest
import torch

import impact_cases as ic
import plant_step_cases as pc
import zoh_io_cases as zi
import zoh_rigid_cases as zr
from helpers import TOL_REL, WEIGHT, close, make_controller, rel_err, same_bits as _same, to_device, vec_err
from rigid_support import against_the_statement, device_terms as _device_terms, imode as _imode, randomised_links
from zoh_rigid_host_loop import assert_same as _assert_same, fresh, push_schedules, wrench_and_refs

pytestmark = pytest.mark.gpu
DT, TH, B, NT = ic.DT, ic.TH, ic.B, ic.NT
CASES = [(3, 50.0), (1, 0.0)]
CASE_IDS = ["3 substeps, kv 50", "1 substep, kv 0"]


def _fresh(ctl, S, t=0.0):
    return fresh(ctl, S["q"], S["v"], t)


# =============================================================================== lmh_plant_impact_rigid
def _impact_against(terms_of, tag):
    """Modes mixed over the batch (mode[i] = (i + s) % 3, s = 0, 1, 2) against the statement on terms_of(i): the three figures <= 1e-12,
    the flags the statement's."""
    from linearmpchumanoid_amd import trajectories as tj
    S = ic.impact_cases()
    ctl = make_controller(B, DT, TH, S["zcom"])
    q, v = to_device(ctl, S["q"]), to_device(ctl, S["v"])

    def robot(i, mode, kv, v_plus, imp, flags, where):
        tm, info = terms_of(i), {}
        _, lam_s, flags_s = tj.rigid_contact_impact(tm["M"], tm["J"], tm["vhat"], mode, contact_mu=ic.MU, info=info)
        assert imp[info["rows"]].all() and flags == flags_s, (where, flags, flags_s)
        return ic.bounds(tm, mode, ic.dvhat_from_dv(v_plus - S["v"][i], S["terms"][i]["X"][0]), imp), info["rows"], flags_s, 0

    against_the_statement(ctl, "impact", tag, (None,), lambda mode, kv: ctl.plant_impact_rigid(q, v, mode), robot)
    ctl.close()


def test_impact_against_the_statement_on_the_oracles_terms():
    S = ic.impact_cases()
    _impact_against(lambda i: S["terms"][i], "the oracle's terms")


def test_impact_against_the_statement_on_the_devices_terms():
    S = ic.impact_cases()
    ctl = make_controller(B, DT, TH, S["zcom"])
    dev = _device_terms(ctl, S)
    ctl.close()
    _impact_against(lambda i: dev[i], "the device's terms")


def test_flight_defaults_mode_bits_and_permutation():
    S = ic.impact_cases()
    ctl = make_controller(B, DT, TH, S["zcom"])
    q, v = to_device(ctl, S["q"]), to_device(ctl, S["v"])
    v_plus, imp, flags = ctl.plant_impact_rigid(q, v, _imode(ctl, np.full(B, 3)))
    torch.cuda.synchronize()
    assert _same(v_plus, v) and float(imp.abs().max()) == 0.0 and int(flags.abs().max()) == 0          # FLIGHT: v bit for bit, exact zeros
    vz = v.clone(); vz[0] = 0.0; vz[1] = -0.0
    assert _same(ctl.plant_impact_rigid(q, vz, _imode(ctl, np.full(B, 3 + 8)))[0], vz)                  # signed zeros included
    mode_np = np.array([(i * 7 + 1) % 4 for i in range(B)], dtype=np.int32)        # all four modes
    res = ctl.plant_impact_rigid(q, v, _imode(ctl, mode_np))
    for name, a, b in (("mode None = all DOUBLE", ctl.plant_impact_rigid(q, v, None), ctl.plant_impact_rigid(q, v, _imode(ctl, np.zeros(B)))),
                       ("only the low two bits", res, ctl.plant_impact_rigid(q, v, _imode(ctl, mode_np + 4))),
                       ("only the low two bits, high ones", res, ctl.plant_impact_rigid(q, v, _imode(ctl, mode_np.astype(np.int64) - 2 ** 31 + 1024)))):
        torch.cuda.synchronize()
        assert all(_same(x, y) for x, y in zip(a, b)), name
    assert not _same(res[0], ctl.plant_impact_rigid(q, v, None)[0])
    perm = np.random.default_rng(20261201).permutation(B)
    pt = torch.as_tensor(perm).to(ctl.device)
    pres = ctl.plant_impact_rigid(q[pt].contiguous(), v[pt].contiguous(), _imode(ctl, mode_np[perm]))
    torch.cuda.synchronize()
    assert all(_same(x[pt], y) for x, y in zip(res, pres))
    # a free foot's six words are exact zeros, a held foot's are not; a flying robot keeps its velocity
    lam, m = res[1].cpu().numpy(), mode_np & 3
    rows = np.array([[1] * 12, [1] * 6 + [0] * 6, [0] * 6 + [1] * 6, [0] * 12])[m]
    assert not lam[rows == 0].any() and lam[rows == 1].all() and _same(res[0][m == 3], v[m == 3])
    # the NULL outputs are legal and change nothing
    L = __import__("linearmpchumanoid_amd.capi", fromlist=["lib"]).lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    vo = torch.empty((B, 30), dtype=torch.float64, device=ctl.device)
    assert L.lmh_plant_impact_rigid(ctl._h, p(q), p(v), p(_imode(ctl, mode_np)), p(vo), None, None, ctl._stream()) == 0
    torch.cuda.synchronize()
    assert _same(vo, res[0])
    ctl.close()


def test_a_second_impact_changes_nothing_and_the_energy_does_not_rise():
    """On the device's own terms: a second impact moves v_plus by at most 1e-12 of the first, and vhat' M vhat / 2 does not rise."""
    S = ic.impact_cases()
    ctl = make_controller(B, DT, TH, S["zcom"])
    dev = _device_terms(ctl, S)
    q, v = to_device(ctl, S["q"]), to_device(ctl, S["v"])
    again, least = 0.0, np.inf
    for s in range(3):
        mode = _imode(ctl, [(i + s) % 3 for i in range(B)])
        v1, _, _ = ctl.plant_impact_rigid(q, v, mode)
        v2, _, f2 = ctl.plant_impact_rigid(q, v1, mode)
        torch.cuda.synchronize()
        a1, a2 = v1.cpu().numpy(), v2.cpu().numpy()
        for i in range(B):
            first, second = np.abs(a1[i] - S["v"][i]).max(), np.abs(a2[i] - a1[i]).max()
            again = max(again, second / first)
            assert second <= 1e-12 * first, (s, i, second, first)
            vh0 = dev[i]["vhat"]
            vh1 = vh0 + ic.dvhat_from_dv(a1[i] - S["v"][i], dev[i]["X"][0])
            e0, e1 = ic.energy(dev[i], vh0), ic.energy(dev[i], vh1)
            least = min(least, (e0 - e1) / e0)
            assert e1 <= e0, (s, i, e0, e1)
    print("\nimpact on the device: a second impact moves v_plus by %.2e of the first; the kinetic energy falls by at least %.1f %%" % (again, 100.0 * least))
    ctl.close()


def test_per_robot_models_and_friction_and_a_nan_flags_its_robot_alone():
    """Four robots with four models (set_model) and four contact_mu (set_params) in one handle equal four handles of one robot, bit for
    bit; the coefficients are chosen around the impulse's own ratio so that the slip flag differs between them."""
    from linearmpchumanoid_amd import capi
    S = ic.impact_cases()
    n, idx = 4, [1, 6, 11, 12]
    raw = randomised_links(n)
    mode_np = np.array([0, 1, 2, 0], dtype=np.int32)
    q, v = S["q"][idx], S["v"][idx]
    probe = make_controller(n, DT, TH, S["zcom"])
    probe.set_model(raw)
    _, lam0, _ = probe.plant_impact_rigid(to_device(probe, q), to_device(probe, v), _imode(probe, mode_np))
    lam0 = lam0.cpu().numpy()
    held = [[ft for ft in range(2) if mode_np[i] in (0, 1 + ft)] for i in range(n)]
    ratio = [[np.hypot(lam0[i, 6 * ft + 3], lam0[i, 6 * ft + 4]) / abs(lam0[i, 6 * ft + 5]) for ft in held[i]] for i in range(n)]
    pulls = [any(lam0[i, 6 * ft + 5] < 0.0 for ft in held[i]) for i in range(n)]
    mu = np.array([max(ratio[i]) * 2.0 if i % 2 == 0 else min(ratio[i]) * 0.5 for i in range(n)])      # inside every held foot's disc | outside
    ctl = make_controller(n, DT, TH, S["zcom"])
    ctl.set_model(raw)
    ctl.set_params(contact_mu=mu)
    v_plus, lam, flags = ctl.plant_impact_rigid(to_device(ctl, q), to_device(ctl, v), _imode(ctl, mode_np))
    torch.cuda.synchronize()
    for i in range(n):
        one = make_controller(1, DT, TH, S["zcom"], contact_mu=float(mu[i]))
        one.set_model(raw[i])
        v1, l1, f1 = one.plant_impact_rigid(to_device(one, q[i:i + 1]), to_device(one, v[i:i + 1]), _imode(one, mode_np[i:i + 1]))
        torch.cuda.synchronize()
        assert _same(v1[0], v_plus[i]) and _same(l1[0], lam[i]) and _same(f1[0], flags[i]), i
        one.close()
    fl = flags.cpu().numpy()
    for i in range(n):                                             # a pulling foot is outside every disc; otherwise mu decides
        assert bool(fl[i] & capi.FLAG_IMPULSE_SLIP) == (pulls[i] or mu[i] < max(ratio[i])), (i, fl[i], mu[i], ratio[i])
        assert bool(fl[i] & capi.FLAG_IMPULSE_PULL) == pulls[i], (i, fl[i])
    nominal = make_controller(n, DT, TH, S["zcom"])
    assert not _same(nominal.plant_impact_rigid(to_device(nominal, q), to_device(nominal, v), _imode(nominal, mode_np))[0], v_plus)       # the models matter
    for c in (probe, ctl, nominal):
        c.close()
    # a NaN flags its robot alone
    ctl = make_controller(B, DT, TH, S["zcom"])
    q, v = to_device(ctl, S["q"]), to_device(ctl, S["v"])
    mode = _imode(ctl, [i % 3 for i in range(B)])
    clean = ctl.plant_impact_rigid(q, v, mode)
    keep = torch.as_tensor([i for i in range(B) if i != 9]).to(ctl.device)
    for what in ("q", "v"):
        qn, vn = q.clone(), v.clone()
        (qn if what == "q" else vn)[9, 11] = float("nan")
        bad = ctl.plant_impact_rigid(qn, vn, mode)
        torch.cuda.synchronize()
        assert int(bad[2][9]) & capi.FLAG_NONFINITE and not (bad[2][keep].cpu().numpy() & capi.FLAG_NONFINITE).any(), what
        assert all(_same(a[keep], b[keep]) for a, b in zip(clean, bad)), what
    ctl.close()


# =============================================================================== lmh_rollout_zoh_rigid_impact
def _core(tag, sa, ra, sb, rb, pa, pb, more=()):
    _assert_same(tag, (("state", sa, sb), ("out", ra["out"], rb["out"]), ("status", ra["status"], rb["status"]), ("log", ra["log"], rb["log"]),
                       ("applied", ra["applied"], rb["applied"]), ("lam", ra["lam"], rb["lam"]), ("impulse", ra["impulse"], rb["impulse"]),
                       ("trace", ra["trace"], rb["trace"])) + tuple(more))
    assert torch.equal(pa, pb), (tag, "d_mode_prev", pa.tolist(), pb.tolist())


def _no_impulse_without_a_touchdown(tag, impulse, td):
    """d_impulse is exactly zero on every tick without a newly held foot, and carries an impulse on every tick with one."""
    big = impulse.abs().amax(dim=2).cpu().numpy()
    assert not big[~td].any() and big[td].all(), (tag, np.argwhere((big != 0.0) != td)[:8].tolist())


def host_loop_impact_(plain, st, n_ticks, n_substeps, prev, **kw):
    return ic.host_loop_impact(plain, st, plain.new_status(), n_ticks, n_substeps, prev, **kw)


@pytest.fixture(scope="module")
def zim():
    S = pc.contact_states()
    ticks, dv = push_schedules()
    mk = lambda: make_controller(B, DT, TH, S["zcom"], warm_start=1)
    ctl, plain = mk(), mk()                                        # push schedules and actuator records | neither: the host loop's handle
    for c in (ctl, plain):
        c.set_refs_stance(2.0, 2)
    ctl.set_pushes(ticks, dv)
    dev = ctl.device
    tau_max = 0.05 + 0.1 * ((np.arange(B)[:, None] + np.arange(24)[None, :]) % 5)
    tau_max[0::4] = np.inf
    rec = zi.robot_records(tau_max)
    rec[:, 48] = np.arange(B) % 4
    ctl.set_actuators(tau_max=rec[:, 0:24], alpha=rec[:, 24:48], delay=rec[:, 48])
    meas = torch.as_tensor(zi.measurement_noise(20261202, NT)).to(dev)
    bw_seq, refs, out0 = wrench_and_refs(plain, _fresh(plain, S), NT)
    tau0 = out0[:, 0:24].contiguous() * 0.5
    words, prev = zr.per_tick_modes(), ic.mode_prev_words()
    assert ic.loop_condition(words, prev)                          # on the host, before any launch
    yield dict(S=S, ctl=ctl, plain=plain, ticks=ticks, dv=dv, bw_seq=bw_seq, meas=meas, refs=refs, rec=torch.as_tensor(rec).to(dev), rec_np=rec, tau0=tau0,
               mode3=_imode(ctl, zr.fixed_modes()), per_tick=_imode(ctl, words), words=words, prev=prev)
    for c in (ctl, plain):
        c.close()


@pytest.mark.parametrize("n_substeps,kv", CASES, ids=CASE_IDS)
def test_fixed_modes_with_flight_before_half_the_robots(zim, n_substeps, kv):
    """d_mode_prev = LMH_PHASE_FLIGHT on the even robots -- every foot they hold is a touchdown at tick 0 --, the mode itself on the odd
    ones -- no impact at all, lmh_rollout_zoh_rigid's bytes for them."""
    ctl, plain, S = zim["ctl"], zim["plain"], zim["S"]
    fixed = zr.fixed_modes()
    prev = ic.fixed_prev(fixed)
    td, last = ic.touchdowns(np.tile(fixed, (NT, 1)), prev)
    assert td[0].tolist() == [i % 2 == 0 for i in range(B)] and not td[1:].any()
    sa, sb, sc = _fresh(ctl, S), _fresh(plain, S), _fresh(ctl, S)
    pa, pb = _imode(ctl, prev), _imode(plain, prev)
    kw = dict(kv=kv, lam=True, applied=True, log=True, trace_every=1)
    ra = ctl.rollout_zoh_rigid(sa, NT, n_substeps, mode=zim["mode3"], impact=pa, impulse=True, **kw)
    rb = host_loop_impact_(plain, sb, NT, n_substeps, pb, mode=zim["mode3"], kv=kv)
    rc_ = ctl.rollout_zoh_rigid(sc, NT, n_substeps, mode=zim["mode3"], **kw)
    torch.cuda.synchronize()
    _core(("fixed", n_substeps, kv), sa, ra, sb, rb, pa, pb)
    assert pa.cpu().numpy().tolist() == last.tolist()
    _no_impulse_without_a_touchdown("fixed", ra["impulse"], td)
    odd, even = torch.arange(1, B, 2, device=ctl.device), torch.arange(0, B, 2, device=ctl.device)
    assert _same(sa[odd], sc[odd]) and _same(ra["trace"][:, odd], rc_["trace"][:, odd]) and _same(ra["lam"][:, odd], rc_["lam"][:, odd])
    assert all(not _same(sa[i], sc[i]) for i in even.tolist())     # the impact is not nothing


def _everything(ctl, zim, n_ticks, n_substeps, kv, prev, t0=0.0, every=1, metrics=None, st=None, status=None, mem=None, first_tick=0, mode="per_tick", impact=True):
    """Pushes, the wrench sequence, the reference sequence, the measurement, the actuator, the log, applied, lam and impulse on; the sequences sliced from first_tick."""
    st = _fresh(ctl, zim["S"], t0) if st is None else st
    mem = ctl.new_act_mem(zim["tau0"]) if mem is None else mem
    cut = slice(first_tick, first_tick + n_ticks)
    md = zim[mode][cut].contiguous() if mode == "per_tick" else zim[mode]
    more = dict(impact=prev, impulse=True) if impact else {}
    r = ctl.rollout_zoh_rigid(st, n_ticks, n_substeps, mode=md, kv=kv, lam=True, meas=zim["meas"][cut].contiguous(), actuators=True, act_mem=mem, applied=True,
                              base_wrench=zim["bw_seq"][cut], ref=zim["refs"][cut], pushes=True, log=True, trace_every=every, metrics=metrics, status=status, **more)
    return dict(r, state=st, mem=mem)


def _everything_on_the_host(zim, n_ticks, n_substeps, kv, prev, t0=0.0, mode="per_tick"):
    plain = zim["plain"]
    st, mem = _fresh(plain, zim["S"], t0), plain.new_act_mem(zim["tau0"])
    r = ic.host_loop_impact(plain, st, plain.new_status(), n_ticks, n_substeps, prev, mode=zim[mode], kv=kv, bw=zim["bw_seq"], sched=(zim["ticks"], zim["dv"]),
                            refs=zim["refs"], meas=zim["meas"], act=(zim["rec"], mem))
    torch.cuda.synchronize()
    return dict(r, state=st, mem=mem)


@pytest.mark.parametrize("n_substeps,kv", CASES, ids=CASE_IDS)
def test_per_tick_modes_alone_and_with_every_option_at_once(zim, n_substeps, kv):
    """The per-tick words (every robot meets a touchdown and a tick without one; d_mode_prev with junk above the low two bits), first with
    nothing else set, then with the 16 push schedules (pushes inside holds split the pieces), a wrench per tick, ref=, meas, actuators
    with delays 0 .. 3, the every-tick trace and the metrics."""
    from linearmpchumanoid_amd import metrics as hm
    ctl, plain, S = zim["ctl"], zim["plain"], zim["S"]
    td, last = ic.touchdowns(zim["words"], zim["prev"])
    sa, sb = _fresh(ctl, S), _fresh(plain, S)
    pa, pb = _imode(ctl, zim["prev"]), _imode(plain, zim["prev"])
    ra = ctl.rollout_zoh_rigid(sa, NT, n_substeps, mode=zim["per_tick"], kv=kv, lam=True, applied=True, log=True, trace_every=1, impact=pa, impulse=True)
    rb = host_loop_impact_(plain, sb, NT, n_substeps, pb, mode=zim["per_tick"], kv=kv)
    torch.cuda.synchronize()
    _core(("per tick", n_substeps, kv), sa, ra, sb, rb, pa, pb)
    assert pa.cpu().numpy().tolist() == last.tolist()              # the last tick's mode, its junk gone
    _no_impulse_without_a_touchdown("per tick", ra["impulse"], td)
    # a free foot's words of an impulse are exact zeros
    rows = np.array([[1] * 12, [1] * 6 + [0] * 6, [0] * 6 + [1] * 6, [0] * 12])[zim["words"] & 3]
    assert not ra["impulse"].cpu().numpy()[rows == 0].any()
    # with everything else on as well
    pa, pb = _imode(ctl, zim["prev"]), _imode(plain, zim["prev"])
    m1 = ctl.new_metrics(0.3, 0.2)
    r1 = _everything(ctl, zim, NT, n_substeps, kv, pa, metrics=m1)
    host = _everything_on_the_host(zim, NT, n_substeps, kv, pb)
    torch.cuda.synchronize()
    _core(("per tick, everything", n_substeps, kv), r1["state"], r1, host["state"], host, pa, pb, (("act_mem", r1["mem"], host["mem"]),))
    assert _same(m1.cpu().numpy(), hm.fold_trace(hm.identity(B, 0.3, 0.2), host["trace"].cpu().numpy()))
    _no_impulse_without_a_touchdown("per tick, everything", r1["impulse"], td)


def _plan_handles(S, plans):
    hs = []
    for _ in range(2):
        c = make_controller(B, DT, TH, S["zcom"], warm_start=1)
        c.gen_walk_batch(zr.SIM_TIME, zr.walk_specs())
        got = [c.get_plan(i) for i in range(B)]
        stack = {k: np.stack([g[k] for g in got]) for k in ("zmp_x", "zmp_y", "phase", "segs", "seg_of_sample")}
        stack["phase"] = plans["phase"]
        c.set_plans(**stack)
        hs.append(c)
    return hs


@pytest.mark.parametrize("n_substeps,kv", CASES, ids=CASE_IDS)
def test_plan_modes_on_per_robot_walking_and_jump_plans(zim, n_substeps, kv):
    S = zim["S"]
    plans = zr.plans()
    t0 = zr.start_clocks(plans["phase"], n_substeps)
    want = zr.plan_modes(plans["phase"], zr.preview_indices(t0, NT, n_substeps))
    td, last = ic.touchdowns(want, zim["prev"])
    assert zr.plan_condition(want) and int(td[1:].any(axis=0).sum()) >= 1 and td[0].any() and (~td).any()       # before the launch
    ctl, plain = _plan_handles(S, plans)
    sa, sb = _fresh(ctl, S, t0), _fresh(plain, S, t0)
    pa, pb = _imode(ctl, zim["prev"]), _imode(plain, zim["prev"])
    ra = ctl.rollout_zoh_rigid(sa, NT, n_substeps, mode="plan", kv=kv, lam=True, applied=True, log=True, trace_every=1, impact=pa, impulse=True)
    rb = host_loop_impact_(plain, sb, NT, n_substeps, pb, mode="plan", phase=plans["phase"], kv=kv)
    torch.cuda.synchronize()
    _core(("plan", n_substeps, kv), sa, ra, sb, rb, pa, pb)
    assert np.array_equal(rb["modes"].cpu().numpy(), want) and pa.cpu().numpy().tolist() == last.tolist()
    _no_impulse_without_a_touchdown("plan", ra["impulse"], td)
    for c in (ctl, plain):
        c.close()


def test_plan_modes_on_a_shared_plan_and_without_a_phase_array(zim):
    from linearmpchumanoid_amd import trajectories as tj
    S, n_substeps, kv = zim["S"], 3, 50.0
    kw = dict(kv=kv, lam=True, applied=True, log=True, trace_every=1)
    ctl, plain = (make_controller(B, DT, TH, S["zcom"], warm_start=1) for _ in range(2))
    for c in (ctl, plain):
        c.gen_walk(zr.SIM_TIME)
    phase = ctl.get_refs()["phase"]
    t0 = zr.start_clocks(phase, n_substeps)
    want = zr.plan_modes(phase, zr.preview_indices(t0, NT, n_substeps))
    td, last = ic.touchdowns(want, zim["prev"])
    assert td.any() and (~td).any()
    sa, sb = _fresh(ctl, S, t0), _fresh(plain, S, t0)
    pa, pb = _imode(ctl, zim["prev"]), _imode(plain, zim["prev"])
    ra = ctl.rollout_zoh_rigid(sa, NT, n_substeps, mode="plan", impact=pa, impulse=True, **kw)
    rb = host_loop_impact_(plain, sb, NT, n_substeps, pb, mode="plan", phase=phase, kv=kv)
    torch.cuda.synchronize()
    _core("shared plan", sa, ra, sb, rb, pa, pb)
    assert np.array_equal(rb["modes"].cpu().numpy(), want) and pa.cpu().numpy().tolist() == last.tolist()
    _no_impulse_without_a_touchdown("shared plan", ra["impulse"], td)
    # a plan without a phase array: DOUBLE on every tick -- a touchdown at tick 0 for every robot whose d_mode_prev is not DOUBLE
    zx, zy = tj.stance_zmp(zr.SIM_TIME, DT, 2)
    for c in (ctl, plain):
        c.set_refs(zx, zy, None)
    td, last = ic.touchdowns(np.zeros((NT, B), dtype=np.int32), zim["prev"])
    sa, sb = _fresh(ctl, S, t0), _fresh(plain, S, t0)
    pa, pb = _imode(ctl, zim["prev"]), _imode(plain, zim["prev"])
    ra = ctl.rollout_zoh_rigid(sa, NT, n_substeps, mode="plan", impact=pa, impulse=True, **kw)
    rb = host_loop_impact_(plain, sb, NT, n_substeps, pb, mode="plan", phase=None, kv=kv)
    torch.cuda.synchronize()
    _core("no phase array", sa, ra, sb, rb, pa, pb)
    assert not pa.any() and td[0].tolist() == [(int(w) & 3) != 0 for w in zim["prev"]]
    _no_impulse_without_a_touchdown("no phase array", ra["impulse"], td)
    for c in (ctl, plain):
        c.close()


def test_no_touchdown_enable_0_and_no_tick_are_the_rigid_call(zim):
    """A launch in which no foot ever becomes held (FIXED, d_mode_prev = the mode) leaves rollout_zoh_rigid's bytes; enable = 0 and
    impact = NULL launch that call's kernel and leave exactly its bytes; n_ticks = 0 leaves d_mode_prev and every buffer untouched."""
    from linearmpchumanoid_amd import capi
    ctl, S = zim["ctl"], zim["S"]
    L = capi.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    fixed = zr.fixed_modes()
    ref = _everything(ctl, zim, NT, 3, 50.0, None, mode="mode3", metrics=ctl.new_metrics(0.3, 0.2), impact=False)
    pa = _imode(ctl, fixed + 4 * (np.arange(B) % 3))               # the mode itself under junk
    keep = pa.clone()
    r = _everything(ctl, zim, NT, 3, 50.0, pa, mode="mode3", metrics=ctl.new_metrics(0.3, 0.2))
    torch.cuda.synchronize()
    _assert_same("no touchdown", (("state", r["state"], ref["state"]), ("out", r["out"], ref["out"]), ("status", r["status"], ref["status"]), ("log", r["log"], ref["log"]),
                                  ("applied", r["applied"], ref["applied"]), ("lam", r["lam"], ref["lam"]), ("trace", r["trace"], ref["trace"]), ("act_mem", r["mem"], ref["mem"])))
    assert float(r["impulse"].abs().max()) == 0.0 and pa.cpu().numpy().tolist() == fixed.tolist() and not torch.equal(pa, keep)
    # enable = 0 (whatever else the record holds) and impact = NULL
    junk = torch.full((NT, B, 12), -7.0, dtype=torch.float64, device=ctl.device)
    prev = _imode(ctl, np.full(B, 3))
    for im in (None, capi.LmhZohImpact(), capi.LmhZohImpact(d_mode_prev=p(prev), d_impulse=p(junk), enable=0)):
        sa, ma, mem_a = _fresh(ctl, S), ctl.new_metrics(0.3, 0.2), ctl.new_act_mem(zim["tau0"])
        out, status = ctl.new_out(), ctl.new_status()
        log, applied, trace, lam = torch.zeros_like(ref["log"]), torch.zeros_like(ref["applied"]), torch.zeros_like(ref["trace"]), torch.zeros_like(ref["lam"])
        opts = capi.LmhZohOpts(d_base_wrench=p(zim["bw_seq"]), d_ref=p(zim["refs"]), d_log=p(log), d_trace=p(trace), d_metrics=p(ma), trace_every=1, wrench_per_tick=1, pushes=1)
        io = capi.LmhZohIo(d_meas=p(zim["meas"]), d_act_mem=p(mem_a), d_applied=p(applied), actuators=1)
        rg = capi.LmhZohRigid(d_mode=p(zim["mode3"]), d_lambda=p(lam), kv=50.0, source=capi.RIGID_FIXED)
        assert L.lmh_rollout_zoh_rigid_impact(ctl._h, p(sa), p(out), p(status), C.byref(opts), C.byref(io), C.byref(rg), None if im is None else C.byref(im), NT, 3, ctl._stream()) == 0
        torch.cuda.synchronize()
        _assert_same("enable 0", (("state", sa, ref["state"]), ("out", out, ref["out"]), ("status", status, ref["status"]), ("log", log, ref["log"]), ("applied", applied, ref["applied"]),
                                  ("lam", lam, ref["lam"]), ("trace", trace, ref["trace"]), ("act_mem", mem_a, ref["mem"])))
        assert bool((junk == -7.0).all()) and bool((prev == 3).all())
    # n_ticks = 0
    sa, out, status = _fresh(ctl, S), torch.full((B, 80), -7.0, dtype=torch.float64, device=ctl.device), ctl.new_status()
    status0 = status.clone()
    im = capi.LmhZohImpact(d_mode_prev=p(prev), d_impulse=p(junk), enable=1)
    rg = capi.LmhZohRigid(d_mode=p(zim["mode3"]), d_lambda=p(junk), kv=50.0, source=capi.RIGID_FIXED)
    assert L.lmh_rollout_zoh_rigid_impact(ctl._h, p(sa), p(out), p(status), None, None, C.byref(rg), C.byref(im), 0, 3, ctl._stream()) == 0
    torch.cuda.synchronize()
    assert _same(sa, _fresh(ctl, S)) and bool((out == -7.0).all()) and bool((junk == -7.0).all()) and bool((prev == 3).all()) and torch.equal(status, status0)


def test_six_ticks_are_two_then_four_with_everything_carried(zim):
    """The per-tick arrays (d_impulse included) are advanced by two records, d_mode_prev and act_mem are handed on."""
    ctl = zim["ctl"]
    td, _ = ic.touchdowns(zim["words"], zim["prev"])
    assert td[2].any() and (~td[2]).any()                          # the second launch's first tick: some robots land on it, some do not
    p6, p24 = _imode(ctl, zim["prev"]), _imode(ctl, zim["prev"])
    m6, m24 = ctl.new_metrics(0.3, 0.2), ctl.new_metrics(0.3, 0.2)
    r6 = _everything(ctl, zim, NT, 3, 50.0, p6, every=2, metrics=m6)
    r2 = _everything(ctl, zim, 2, 3, 50.0, p24, every=2, metrics=m24)
    torch.cuda.synchronize()
    status2 = r2["status"].clone()
    assert p24.cpu().numpy().tolist() == (zim["words"][1] & 3).tolist()
    r4 = _everything(ctl, zim, 4, 3, 50.0, p24, every=2, metrics=m24, st=r2["state"], status=r2["status"].clone(), mem=r2["mem"], first_tick=2)
    torch.cuda.synchronize()
    tb = r4["trace"].clone()                                       # status [1] / [2] of a sample count from its launch's start
    tb[:, :, 177] = torch.maximum(tb[:, :, 177], status2[None, :, 1].double())
    tb[:, :, 178] = (tb[:, :, 178].long() | status2[None, :, 2].long()).double()
    _assert_same("split", (("state", r6["state"], r4["state"]), ("out", r6["out"], r4["out"]), ("log", r6["log"], torch.cat([r2["log"], r4["log"]])),
                           ("applied", r6["applied"], torch.cat([r2["applied"], r4["applied"]])), ("lam", r6["lam"], torch.cat([r2["lam"], r4["lam"]])),
                           ("impulse", r6["impulse"], torch.cat([r2["impulse"], r4["impulse"]])),
                           ("act_mem", r6["mem"], r4["mem"]), ("trace", r6["trace"], torch.cat([r2["trace"], tb])), ("metrics", m6, m24)))
    assert torch.equal(p6, p24)
    s6, s4 = r6["status"], r4["status"]
    assert torch.equal(s6[:, 0], s4[:, 0]) and torch.equal(s6[:, 3], s4[:, 3])
    assert torch.equal(s6[:, 1], torch.maximum(status2[:, 1], s4[:, 1])) and torch.equal(s6[:, 2], status2[:, 2] | s4[:, 2])


def test_parity_with_the_cpu_loop():
    """4 robots x 12 control ticks, the right sole held for six ticks and both from the seventh on -- a touchdown of a moving left sole into
    double support in the middle --, kv = 50, n_substeps = 1, in ONE launch against the CPU loop (oracle evaluation + the numpy statements
    of the impact and of the hold; impact_cases.cpu_loop) at the project's bounds: state 1e-7, tau and f at TOL_REL (f with the weight's
    floor), k exact, no controller flag.  The touchdown changes a velocity by more than 1e-3 of the largest |v| (pinned on the CPU)."""
    P = ic.parity_inputs()
    n, nt, kv = ic.PARITY["n"], ic.PARITY["nt"], ic.PARITY["kv"]
    ctl = make_controller(n, DT, TH, P["zcom"], warm_start=0)
    ctl.set_refs_stance(2.0, 2)
    st = ctl.new_state(P["q"], P["v"], t=0.0, v_prev=P["v"])
    prev = _imode(ctl, P["prev"])
    r = ctl.rollout_zoh_rigid(st, nt, 1, mode=_imode(ctl, P["modes"]), kv=kv, lam=True, impact=prev, impulse=True)
    torch.cuda.synchronize()
    a, o_, s, lam, imp = st.cpu().numpy(), r["out"].cpu().numpy(), r["status"].cpu().numpy(), r["lam"][-1].cpu().numpy(), r["impulse"].cpu().numpy()
    refs = ic.cpu_loop(True)
    rows = []
    for i in range(n):
        c = refs[i]
        rows.append((i, rel_err(a[i, :60], c["x"]), vec_err(o_[i, 0:24], c["last"]["tau"]), vec_err(o_[i, 24:36], c["last"]["f"]), vec_err(lam[i], c["lam"]),
                     vec_err(imp[:, i].ravel(), c["impulse"].ravel()), int(s[i, 0]), c["last"]["k"], int(s[i, 2])))
        print("\nzoh_rigid_impact vs the CPU loop, robot %d: state %.2e  tau %.2e  f %.2e  lambda %.2e  impulse %.2e  k %d (oracle %d)  flags %d" % rows[-1], end="")
    print()
    for i in range(n):
        c = refs[i]
        assert c["jump"] > 1e-3
        assert close(a[i, :60], c["x"], 1e-7) and a[i, 90] == c["t"], rows[i]
        assert close(o_[i, 0:24], c["last"]["tau"], TOL_REL) and close(o_[i, 24:36], c["last"]["f"], TOL_REL, scale=WEIGHT), rows[i]
        assert close(imp[:, i].ravel(), c["impulse"].ravel(), TOL_REL), rows[i]
        assert s[i, 0] == c["last"]["k"] and (s[i, 2] & 31) == 0, rows[i]          # no controller flag (the plant's informational ones lie above)
        assert (np.abs(imp[:, i]).max(axis=1) > 0.0).tolist() == [j == ic.PARITY["touchdown"] for j in range(nt)]
    assert prev.cpu().numpy().tolist() == [0] * n
    ctl.close()


def test_refusals_and_tables(zim):
    from linearmpchumanoid_amd import capi, trajectories as tj
    S, ctl = zim["S"], zim["ctl"]
    L = capi.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    err = lambda: L.lmh_last_error().decode()
    dev = ctl.device
    sent = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device=dev)
    st, out, status = _fresh(ctl, S), ctl.new_out(), ctl.new_status()
    lam, impulse, v_plus, imp1 = sent(NT, B, 12), sent(NT, B, 12), sent(B, 30), sent(B, 12)
    prev, flags = _imode(ctl, zim["prev"]), torch.full((B,), -7, dtype=torch.int32, device=dev)
    q, v = st[:, 0:30].contiguous(), st[:, 30:60].contiguous()
    torch.cuda.synchronize()
    bufs = (st, out, status, lam, impulse, v_plus, imp1, prev, flags)
    sentinels = tuple(x.clone() for x in bufs)

    def untouched():
        torch.cuda.synchronize()
        return all(_same(x, y) for x, y in zip(bufs, sentinels))

    s = ctl._stream()
    # lmh_plant_impact_rigid
    P = L.lmh_plant_impact_rigid
    assert P(ctl._h, None, p(v), None, p(v_plus), p(imp1), p(flags), s) == -2 and err() == "lmh_plant_impact_rigid: null d_q"
    assert P(ctl._h, p(q), None, None, p(v_plus), p(imp1), p(flags), s) == -2 and err() == "lmh_plant_impact_rigid: null d_v"
    assert P(ctl._h, p(q), p(v), None, None, p(imp1), p(flags), s) == -2 and err() == "lmh_plant_impact_rigid: null d_v_plus"
    assert P(None, p(q), p(v), None, p(v_plus), p(imp1), p(flags), s) == -2 and err() == "null handle"
    assert untouched()
    # lmh_rollout_zoh_rigid_impact
    Z = L.lmh_rollout_zoh_rigid_impact

    def call(rigid, impact, n_ticks=NT, n_substeps=3, state=st, handle=ctl, io=None):
        rg = None if rigid is None else C.byref(capi.LmhZohRigid(**{"d_lambda": p(lam), **rigid}))
        im = None if impact is None else C.byref(capi.LmhZohImpact(**impact))
        return Z(handle._h, None if state is None else p(state), p(out), p(status), None, None if io is None else C.byref(capi.LmhZohIo(**io)), rg, im, n_ticks, n_substeps, s)

    on, im_on = dict(source=capi.RIGID_PER_TICK, d_mode=p(zim["per_tick"]), kv=50.0), dict(d_mode_prev=p(prev), d_impulse=p(impulse), enable=1)
    own = [(on, dict(im_on, enable=2), "lmh_rollout_zoh_rigid_impact: enable must be 0 or 1"),
           (on, dict(im_on, enable=-1), "lmh_rollout_zoh_rigid_impact: enable must be 0 or 1"),
           (on, dict(im_on, reserved=1), "lmh_rollout_zoh_rigid_impact: reserved must be 0"),
           (on, dict(enable=0, reserved=2), "lmh_rollout_zoh_rigid_impact: reserved must be 0"),
           (dict(source=0), im_on, "lmh_rollout_zoh_rigid_impact: enable = 1 needs a rigid record with a source (the impact is the rigid plant's)"),
           (None, im_on, "lmh_rollout_zoh_rigid_impact: enable = 1 needs a rigid record with a source (the impact is the rigid plant's)"),
           (on, dict(d_impulse=p(impulse), enable=1), "lmh_rollout_zoh_rigid_impact: enable = 1 needs d_mode_prev"),
           # every refusal of lmh_rollout_zoh_rigid, in its words and in front of the impact's own
           (dict(on, source=4), dict(im_on, enable=2), "lmh_rollout_zoh_rigid: source must be 0, LMH_RIGID_FIXED, LMH_RIGID_PER_TICK or LMH_RIGID_PLAN"),
           (dict(on, reserved=1), im_on, "lmh_rollout_zoh_rigid: reserved must be 0"),
           (dict(on, kv=-1.0), im_on, "lmh_rollout_zoh_rigid: kv must be finite and >= 0"),
           (dict(source=capi.RIGID_PER_TICK), im_on, "lmh_rollout_zoh_rigid: source LMH_RIGID_PER_TICK needs d_mode"),
           (dict(on, source=capi.RIGID_PLAN), im_on, "lmh_rollout_zoh_rigid: d_mode must be NULL with source LMH_RIGID_PLAN (the robot's own plan decides)")]
    for rigid, impact, words in own:
        assert call(rigid, impact) == -2 and err() == words, (rigid, impact)
    assert call(on, im_on, io=dict(actuators=1)) == -2 and err() == "lmh_rollout_zoh_io: actuators = 1 needs d_act_mem"
    assert call(on, im_on, state=None) == -2 and err() == "lmh_rollout_zoh: null device pointer"
    for n_ticks, n_sub in ((-1, 1), (1, -1)):
        assert call(on, im_on, n_ticks=n_ticks, n_substeps=n_sub) == -2 and err() == "lmh_rollout_zoh: n_ticks and n_substeps must be >= 0"
    assert Z(None, p(st), p(out), p(status), None, None, C.byref(capi.LmhZohRigid(**on)), C.byref(capi.LmhZohImpact(**im_on)), NT, 3, s) == -2 and err() == "null handle"
    assert call(on, im_on, n_ticks=0) == 0                         # no tick: nothing enqueued
    assert untouched()
    for prec in (capi.PRECISION_MIXED, capi.PRECISION_FP32):
        other = make_controller(B, DT, TH, S["zcom"], precision=prec)
        other.set_refs_stance(2.0, 2)
        assert call(on, im_on, handle=other) == -2 and "lmh_rollout_zoh: LMH_PRECISION_FP64 handles only" in err()
        # the impact call works on a handle of any precision
        vp, _, fl = other.plant_impact_rigid(q, v, None)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(vp).all()) and not (fl.cpu().numpy() & 10).any()
        other.close()
    assert untouched()
    # Python: shapes and kinds before the C call
    for bad_call in (lambda: ctl.rollout_zoh_rigid(st, NT, 1, impact=prev[0:3].contiguous()), lambda: ctl.rollout_zoh_rigid(st, NT, 1, impact=prev.long()),
                     lambda: ctl.rollout_zoh_rigid(st, NT, 1, impact=prev.cpu()), lambda: ctl.rollout_zoh_rigid(st, NT, 1, impulse=True),
                     lambda: ctl.rollout_zoh_rigid(st, NT, 1, impact=prev, impulse=impulse[0:3]), lambda: ctl.rollout_zoh_rigid(st, NT, 1, impact=prev, impulse=impulse.float()),
                     lambda: ctl.plant_impact_rigid(q[0:3], v), lambda: ctl.plant_impact_rigid(q, v, prev.long())):
        with pytest.raises(ValueError):
            bad_call()
    assert untouched()

    # the ground and the servo table, set and cleared, change no byte of either call; no table of the handle changes
    def tables():
        return [(ctl.get_ground(i).tobytes(), ctl.get_servo(i)["kp"].tobytes(), ctl.get_servo(i)["kd"].tobytes(), ctl.get_actuators(i)["tau_max"].tobytes(),
                 ctl.get_actuators(i)["alpha"].tobytes(), ctl.get_actuators(i)["delay"], ctl.get_pushes(i)["ticks"].tobytes(), ctl.get_pushes(i)["dv"].tobytes(),
                 tuple(sorted(ctl.get_params(i).items())), ctl.get_plan(i)["zmp_x"].tobytes(), ctl.get_plan(i)["phase"].tobytes()) for i in (0, 5, B - 1)]

    before = tables()
    runs = []
    for step in ("none", "ground and servo", "cleared"):
        if step == "ground and servo":
            ctl.set_ground(tj.ground_planes(0.05, 0.3, 0.002, -0.001))
            ctl.set_servo(kp=np.full((B, 24), 3.0), kd=0.1)
        elif step == "cleared":
            ctl.set_ground(None)
            ctl.set_servo()
        t_in = tables()
        pr = _imode(ctl, zim["prev"])
        r = _everything(ctl, zim, NT, 3, 50.0, pr, metrics=ctl.new_metrics(0.3, 0.2))
        one = ctl.plant_impact_rigid(q, v, zim["mode3"])
        torch.cuda.synchronize()
        assert tables() == t_in, step
        runs.append((r, pr, one))
    for r, pr, one in runs[1:]:
        _core("tables", runs[0][0]["state"], runs[0][0], r["state"], r, runs[0][1], pr, (("act_mem", runs[0][0]["mem"], r["mem"]),))
        assert all(_same(a, b) for a, b in zip(runs[0][2], one))
    assert tables() == before


def test_both_calls_captured_on_a_fresh_handle_replay_to_the_eager_bytes(zim):
    """A plain single-stream capture, each call as the first call on a fresh handle."""
    from linearmpchumanoid_amd import capi, metrics as hm
    S = zim["S"]
    L = capi.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    # ---- lmh_rollout_zoh_rigid_impact
    ctl = make_controller(B, DT, TH, S["zcom"], warm_start=1)     # fresh: no launch before the capture
    ctl.set_refs_stance(2.0, 2)
    ctl.set_pushes(zim["ticks"], zim["dv"])
    rec = zim["rec_np"]
    ctl.set_actuators(tau_max=rec[:, 0:24], alpha=rec[:, 24:48], delay=rec[:, 48])
    dev = ctl.device
    ident = torch.as_tensor(hm.identity(B, 0.3, 0.2)).to(dev)     # (not new_metrics: no launch of the handle's before the capture)
    st0 = _fresh(ctl, S)
    mem0 = zim["tau0"].repeat(1, 8).contiguous()
    sent = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device=dev)
    prev0 = _imode(ctl, zim["prev"])
    st, out, status, log, trace, m, mem, applied, lam, impulse, prev = (st0.clone(), sent(B, 80), ctl.new_status(), sent(NT, B, 36), sent(3, B, 180), ident.clone(), mem0.clone(),
                                                                        sent(NT, B, 24), sent(NT, B, 12), sent(NT, B, 12), prev0.clone())
    bw, refs, meas, modes = zim["bw_seq"].contiguous(), zim["refs"].contiguous(), zim["meas"].contiguous(), zim["per_tick"].to(dev).contiguous()
    opts = capi.LmhZohOpts(d_base_wrench=p(bw), d_ref=p(refs), d_log=p(log), d_trace=p(trace), d_metrics=p(m), trace_every=2, wrench_per_tick=1, pushes=1, reserved=0)
    io = capi.LmhZohIo(d_meas=p(meas), d_act_mem=p(mem), d_applied=p(applied), actuators=1, reserved=0)
    rg = capi.LmhZohRigid(d_mode=p(modes), d_lambda=p(lam), kv=50.0, source=capi.RIGID_PER_TICK, reserved=0)
    im = capi.LmhZohImpact(d_mode_prev=p(prev), d_impulse=p(impulse), enable=1, reserved=0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc_ = L.lmh_rollout_zoh_rigid_impact(ctl._h, p(st), p(out), p(status), C.byref(opts), C.byref(io), C.byref(rg), C.byref(im), NT, 3, ctl._stream())
    assert rc_ == 0
    torch.cuda.synchronize()
    assert _same(st, st0) and bool((out == -7).all()) and bool((impulse == -7).all()) and _same(m, ident) and _same(mem, mem0) and torch.equal(prev, prev0)       # captured, not run
    g.replay()
    torch.cuda.synchronize()
    got = [x.clone() for x in (st, out, status, log, trace, m, mem, applied, lam, impulse, prev)]
    del g
    e_st, e_m, e_mem, e_prev = st0.clone(), ident.clone(), mem0.clone(), prev0.clone()
    e = ctl.rollout_zoh_rigid(e_st, NT, 3, mode=modes, kv=50.0, lam=sent(NT, B, 12), meas=meas, actuators=True, act_mem=e_mem, applied=sent(NT, B, 24), base_wrench=bw,
                              ref=refs, pushes=True, log=sent(NT, B, 36), trace_every=2, trace=sent(3, B, 180), metrics=e_m, out=sent(B, 80), impact=e_prev, impulse=sent(NT, B, 12))
    torch.cuda.synchronize()
    for name, a, b in zip(("state", "out", "status", "log", "trace", "metrics", "act_mem", "applied", "lam", "impulse", "mode_prev"), got,
                          (e_st, e["out"], e["status"], e["log"], e["trace"], e_m, e_mem, e["applied"], e["lam"], e["impulse"], e_prev)):
        assert _same(a, b), name
    assert not bool((got[9] == -7).any()) and float(got[5][0, 0]) == NT and not torch.equal(got[10], prev0)
    ctl.close()
    # ---- lmh_plant_impact_rigid
    ctl = make_controller(B, DT, TH, S["zcom"])
    q, v, mode = st0[:, 0:30].contiguous(), st0[:, 30:60].contiguous(), zim["mode3"].to(dev)
    vp, imp, fl = sent(B, 30), sent(B, 12), torch.full((B,), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc_ = L.lmh_plant_impact_rigid(ctl._h, p(q), p(v), p(mode), p(vp), p(imp), p(fl), ctl._stream())
    assert rc_ == 0
    torch.cuda.synchronize()
    assert bool((vp == -7).all()) and bool((imp == -7).all()) and bool((fl == -7).all())
    g.replay()
    torch.cuda.synchronize()
    del g
    e = ctl.plant_impact_rigid(q, v, mode)
    torch.cuda.synchronize()
    assert _same(vp, e[0]) and _same(imp, e[1]) and _same(fl, e[2]) and not bool((vp == -7).any())
    ctl.close()
