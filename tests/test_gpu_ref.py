"""Caller-supplied CoM references on the GPU: lmh_eval_ref and lmh_rollout_zoh_ref (include/lmh.h), through stand_step(ref=...) and
rollout_zoh(ref=...).

lmh_eval_ref is lmh_eval with the six words xRef | yRef taken from the caller's record instead of the built-in preview step, so most cases
are identities against lmh_eval itself, byte for byte (helpers.same_bits): the built-in step's own words handed back (1), handed to a
handle with other ZMP samples (2), a launch's words replayed (5).  Where the reference is one no preview step produces the checker is the
numpy restatement with a supplied reference (3, ref_cases.py); lmh_rollout_zoh_ref is held to the host loop that defines it (4,
zoh_host_loop.py); the box-constrained MPC's trajectory goes in as it stands (6); refusals, isolation of a bad record and graph capture (7).
B = 8 everywhere.  States: the first eight of plant_step_cases.contact_states() (the zero-order-hold tests' inputs, v_prev = v), except (3)
which uses ref_cases.states().  A record's words [6, 16) hold a sentinel the calls must not read."""
import ctypes as C

import numpy as np
import pytest
import torch

import params_cases as pcs
import plant_step_cases as pc
import ref_cases as rc
from helpers import TOL_REL, WEIGHT, close, make_controller, same_bits as _same, vec_err
from zoh_host_loop import host_loop

pytestmark = pytest.mark.gpu
DT, TH, B = pc.DT, pc.TH, 8
FLAG_QP_MAXITER, FLAG_NONFINITE, FLAG_NOT_SPD = 1, 2, 8


def _states():
    S = pc.contact_states()
    return dict(q=S["q"][:B], v=S["v"][:B], q0=S["q0"], zcom=S["zcom"])


def _fresh(ctl, S, t=0.0):
    st = ctl.new_state(S["q"], S["v"], t=t, v_prev=S["v"])
    st[:, 91:96] = torch.arange(1.0, 6.0, dtype=torch.float64, device=ctl.device)          # the pads: left alone
    return st


def _records(ctl, six, lead=()):
    """Records lead + [B,16] on the device with words 0:6 = six and a sentinel in the words the calls ignore."""
    rec = torch.full(tuple(lead) + (B, 16), -7.0e3, dtype=torch.float64, device=ctl.device)
    rec[..., 0:6] = six
    return rec


def _walk_specs():
    """The per-robot plans of test_gpu_zoh.test_per_robot_everything_bit_for_bit, for eight robots."""
    return dict(num_steps=4, time_per_step=0.006 + 0.001 * (np.arange(B) % 5), ds_time=0.002 + 0.001 * (np.arange(B) % 3), step_height=0.002,
                settle_time=0.001 * (1 + np.arange(B) % 7), first_support=1 + np.arange(B) % 2)


def _single_support_times(ctl):
    """A clock per robot half a sample inside the first single-support sample of its own plan -> (t [B], the phases there)."""
    t, ph = np.zeros(B), []
    for i in range(B):
        phase = ctl.get_plan(i)["phase"]
        k = int(np.nonzero(phase != 0)[0][0]) + 1
        assert phase[k] in (1, 2)
        t[i] = (k + 0.5) * DT
        ph.append(int(phase[k]))
    return t, ph


def _randomised_links(n):
    """test_gpu_zoh's per-robot models."""
    from linearmpchumanoid_amd.controller import nominal_links
    raw = np.tile(nominal_links(), (n, 1, 1))
    rng = np.random.default_rng(20260004)
    raw[:, :, 0] *= rng.uniform(0.9, 1.1, (n, 28))
    raw[:, :, 1:4] += rng.uniform(-5e-3, 5e-3, (n, 28, 3)) * (raw[:, :, 0:1] > 0)
    return raw


def _two_steps(ctl, st, refs=None):
    """Two evaluations in a row on one state and status record (the second starts from the first's v_prev and active mask); refs: None =
    lmh_eval, else the two record sets.  -> list of (out, status, state) snapshots."""
    status, snaps = ctl.new_status(), []
    for j in range(2):
        out, status = ctl.stand_step(st, status=status, ref=None if refs is None else refs[j])
        snaps.append((out.clone(), status.clone(), st.clone()))
    torch.cuda.synchronize()
    return snaps


def _assert_same_snaps(a, b, tag):
    for j, (sa, sb) in enumerate(zip(a, b)):
        for name, x, y in zip(("out", "status", "state"), sa, sb):
            assert _same(x, y), (tag, "evaluation", j, name)


# ------------------------------------------------------------------------------- 1. self-identity
@pytest.mark.parametrize("case", ["stance", "walking plans", "params and models", "mixed", "fp32"])
def test_own_reference_handed_back_is_the_same_evaluation(case):
    """stand_step(ref = the words out[:, 72:78] a plain stand_step left) from the same state and status leaves the same bytes in out, status
    and state; twice in a row, so v_prev and the warm start's mask are carried by both."""
    from linearmpchumanoid_amd import capi
    S = _states()
    cfg = dict(warm_start=1)
    if case == "mixed":
        cfg["precision"] = capi.PRECISION_MIXED
    if case == "fp32":
        cfg["precision"] = capi.PRECISION_FP32
    ctl = make_controller(B, DT, TH, S["zcom"], **cfg)
    t = 0.0
    if case == "stance":
        ctl.set_refs_stance(2.0, 2)
    else:
        if case == "params and models":
            ctl.set_model(_randomised_links(B))
            ctl.set_params(**pcs.columns([dict(pcs.SIX_SETS[i % 6], **pcs.PLANT_SETS[i % 4]) for i in range(B)], ctl.cfg))
            ctl.set_zcom(S["zcom"] + 0.002 * np.arange(B))
        ctl.gen_walk_batch(0.2, _walk_specs())
        ctl.set_xscale(0.002 + 0.0005 * np.arange(B))
        t, phases = _single_support_times(ctl)
        assert set(phases) == {1, 2}                               # right and left support in one launch
    plain = _two_steps(ctl, _fresh(ctl, S, t))
    refs = [_records(ctl, snap[0][:, 72:78]) for snap in plain]
    again = _two_steps(ctl, _fresh(ctl, S, t), refs)
    _assert_same_snaps(plain, again, case)
    assert float(plain[0][0][:, 0:24].abs().max()) > 0.0
    if case != "stance":
        assert len({int(k) for k in plain[0][1][:, 0].tolist()}) >= 4      # the robots sit at different preview indices
    ctl.close()


# ------------------------------------------------------------------------------- 2. cross-handle identity
@pytest.mark.parametrize("plan", ["shared refs", "per-robot plans"])
def test_reference_of_another_handle_reproduces_that_handle(plan):
    """Handles A and B differ in their ZMP samples alone, which enter an evaluation through the MPC sums only (oracle/orc_controller.c,
    refs_prepare): B tracking A's xRef | yRef leaves A's 80 output words, status and state; B on its own does not."""
    from linearmpchumanoid_amd import trajectories
    S = _states()
    a, b = (make_controller(B, DT, TH, S["zcom"], warm_start=1) for _ in range(2))
    if plan == "shared refs":
        a.set_refs_stance(2.0, 2)
        b.set_refs_stance(2.0, 2)
        r = a.get_refs()
        n = len(r["zmp_x"])
        k = np.arange(n)
        zx, zy = r["zmp_x"] * 0.7 + 0.004 * np.sin(0.05 * k) + 0.003, r["zmp_y"] * 1.3 - 0.002 * np.cos(0.03 * k) - 0.004
        a.set_refs(r["zmp_x"], r["zmp_y"], r["phase"])
        b.set_refs(zx, zy, r["phase"])
        t = 0.0
    else:
        plans = trajectories.walk_plans(0.2, DT, _walk_specs(), B)
        n = plans["zmp_x"].shape[1]
        k = np.arange(n)[None, :]
        scale, shift = 1.0 + 0.05 * np.arange(1, B + 1)[:, None], 0.002 * np.arange(1, B + 1)[:, None]
        other = dict(plans, zmp_x=plans["zmp_x"] * scale + 0.1 * np.sin(0.07 * k), zmp_y=plans["zmp_y"] * (2.0 - scale) + shift * np.cos(0.05 * k))
        a.set_plans(**plans)
        b.set_plans(**other)
        for c in (a, b):
            c.set_xscale(0.002 + 0.0005 * np.arange(B))
        t, phases = _single_support_times(a)
        assert set(phases) == {1, 2} and np.array_equal(a.get_plan(3)["phase"], b.get_plan(3)["phase"])
    sa, sb, sc = _fresh(a, S, t), _fresh(b, S, t), _fresh(b, S, t)
    out_a, status_a = a.stand_step(sa)
    out_b, status_b = b.stand_step(sb, ref=_records(b, out_a[:, 72:78]))
    out_c, status_c = b.stand_step(sc)
    torch.cuda.synchronize()
    assert _same(out_a, out_b) and _same(status_a, status_b) and _same(sa, sb)
    assert int((status_a[:, 2] & (FLAG_QP_MAXITER | FLAG_NONFINITE | FLAG_NOT_SPD)).max()) == 0
    differ = (out_c[:, 0:24] != out_a[:, 0:24]).any(dim=1) & (out_c[:, 72:78] != out_a[:, 72:78]).any(dim=1)
    assert bool(differ.all()), differ.tolist()                     # not vacuous: B's own ZMP samples give every robot other torques
    a.close(); b.close()


# ------------------------------------------------------------------------------- 3. off-manifold parity
def test_off_manifold_reference_against_the_restatement():
    """References no MPC step produces (ref_cases.off_manifold_refs) against the numpy restatement tracking the same values: tau and qdd
    at helpers.TOL_REL of their own largest entry, f at TOL_REL with the weight's floor -- the rules of test_gpu_posture_sweep for the same
    outputs.  The restatement's own distance to the C oracle on these states is below a tenth of that (test_ref_cases.py), so nothing is
    added to the bound.  out[72:78] carry the supplied words exactly, k = 0, no flag, v_prev <- v.  Measured on one MI355X: tau 2.8e-10,
    f 7.0e-11 of the weight, qdd 8.5e-11 at most."""
    S, rec, want = rc.states(), rc.off_manifold_refs(), rc.off_manifold_results()
    assert rc.B == B
    ctl = make_controller(B, rc.DT, rc.TH, S["zcom"], warm_start=0)
    ctl.set_refs_stance(2.0, 2)
    st = ctl.new_state(S["q"], S["v"], t=0.0, v_prev=S["vp"])
    out, status = ctl.stand_step(st, ref=rec)                      # an array is taken as it is
    torch.cuda.synchronize()
    o, s, stn = out.cpu().numpy(), status.cpu().numpy(), st.cpu().numpy()
    ctl.close()
    rows = []
    for i in range(B):
        rows.append((i, vec_err(o[i, 0:24], want[i]["tau"]), float(np.abs(o[i, 24:36] - want[i]["f"]).max() / WEIGHT), vec_err(o[i, 36:66], want[i]["qpp"]),
                     int(s[i, 0]), int(s[i, 2])))
        print("\noff-manifold reference, robot %d: tau %.2e  f/weight %.2e  qdd %.2e  k %d  flags %d" % rows[-1], end="")
    print()
    for i in range(B):
        assert s[i, 0] == 0 and s[i, 2] == 0, rows[i]
        assert np.array_equal(o[i, 72:78], rec[i, 0:6]) and np.array_equal(stn[i, 60:90], S["v"][i]), rows[i]
        assert vec_err(o[i, 0:24], want[i]["tau"]) < TOL_REL and vec_err(o[i, 36:66], want[i]["qpp"]) < TOL_REL, rows[i]
        assert close(o[i, 24:36], want[i]["f"], TOL_REL, scale=WEIGHT), rows[i]


# ------------------------------------------------------------------------------- 4. the zero-order-hold definition
def _zoh_refs(ctl, S, n_ticks, seed):
    """[n_ticks,B,16]: the built-in step's words at the start state, moved per tick and robot by up to 1 cm, 5 cm/s and 0.5 m/s^2."""
    out, _ = ctl.stand_step(_fresh(ctl, S))
    rng = np.random.default_rng(seed)
    d = rng.uniform(-1.0, 1.0, (n_ticks, B, 6)) * np.array([0.01, 0.05, 0.5, 0.01, 0.05, 0.5])
    return _records(ctl, out[:, 72:78].unsqueeze(0) + torch.as_tensor(d).to(ctl.device), (n_ticks,))


@pytest.fixture(scope="module")
def zoh():
    S = _states()
    ctl = make_controller(B, DT, TH, S["zcom"], warm_start=1)
    ctl.set_refs_stance(2.0, 2)
    bw = torch.as_tensor(np.random.default_rng(20261024).normal(0.0, 1.0, (B, 6))).to(ctl.device)
    yield dict(S=S, ctl=ctl, bw=bw, refs=_zoh_refs(ctl, S, 6, 20261027))
    ctl.close()


@pytest.mark.parametrize("wrench", [False, True])
@pytest.mark.parametrize("n_substeps", [0, 1, 3])
def test_zoh_is_the_host_loop_bit_for_bit(zoh, n_substeps, wrench):
    ctl, S, refs, bw = zoh["ctl"], zoh["S"], zoh["refs"], zoh["bw"] if wrench else None
    sa, sb = _fresh(ctl, S), _fresh(ctl, S)
    out_a, status_a, log_a = ctl.rollout_zoh(sa, 6, n_substeps, base_wrench=bw, log=True, ref=refs)
    rb = host_loop(ctl, sb, ctl.new_status(), 6, n_substeps, bw=bw, refs=refs)
    out_b, status_b, log_b = rb["out"], rb["status"], rb["log"]
    torch.cuda.synchronize()
    for name, a, b in (("state", sa, sb), ("out", out_a, out_b), ("status", status_a, status_b), ("log", log_a, log_b)):
        assert _same(a, b), (n_substeps, wrench, name)
    assert _same(out_a[:, 72:78].contiguous(), refs[5, :, 0:6].contiguous())             # the last tick's record, not the first's
    assert float(sa[0, 90]) == sum([DT] * (6 * n_substeps))


def test_zoh_splits_with_the_reference_slices(zoh):
    """6 = 2 + 4 with ref[0:2] and ref[2:6] and the status record handed on."""
    ctl, S, refs, bw = zoh["ctl"], zoh["S"], zoh["refs"], zoh["bw"]
    s6, sp = _fresh(ctl, S), _fresh(ctl, S)
    out6, status6, log6 = ctl.rollout_zoh(s6, 6, 2, base_wrench=bw, log=True, ref=refs)
    out2, status2, log2 = ctl.rollout_zoh(sp, 2, 2, base_wrench=bw, log=True, ref=refs[0:2])
    status2 = status2.clone()
    out4, status4, log4 = ctl.rollout_zoh(sp, 4, 2, base_wrench=bw, log=True, status=status2.clone(), ref=refs[2:6])
    torch.cuda.synchronize()
    assert _same(s6, sp) and _same(out6, out4) and _same(log6, torch.cat([log2, log4]))
    assert torch.equal(status6[:, 0], status4[:, 0]) and torch.equal(status6[:, 3], status4[:, 3])
    assert torch.equal(status6[:, 1], torch.maximum(status2[:, 1], status4[:, 1])) and torch.equal(status6[:, 2], status2[:, 2] | status4[:, 2])


# ------------------------------------------------------------------------------- 5. replay identity
def test_replaying_a_launch_own_references_reproduces_it(zoh):
    """The built-in loop one tick per launch collects out[:, 72:78] of every tick; one rollout_zoh(ref = that sequence) launch from the same
    start leaves the bytes of the built-in 8-tick launch."""
    ctl, S, bw = zoh["ctl"], zoh["S"], zoh["bw"]
    st, status, seq = _fresh(ctl, S), ctl.new_status(), []
    for _ in range(8):
        out, status = ctl.rollout_zoh(st, 1, 2, base_wrench=bw, status=status)
        seq.append(out[:, 72:78].clone())
    sa, sb = _fresh(ctl, S), _fresh(ctl, S)
    out_a, status_a, log_a = ctl.rollout_zoh(sa, 8, 2, base_wrench=bw, log=True)
    out_b, status_b, log_b = ctl.rollout_zoh(sb, 8, 2, base_wrench=bw, log=True, ref=_records(ctl, torch.stack(seq), (8,)))
    torch.cuda.synchronize()
    assert _same(sa, st) and _same(sa, sb) and _same(out_a, out_b) and _same(status_a, status_b) and _same(log_a, log_b)
    assert not _same(seq[0], seq[7])


# ------------------------------------------------------------------------------- 6. the pipeline
def test_box_constrained_plan_is_tracked_as_it_stands():
    """mpc_box_rollout on the plans' ZMP boxes from the robots' own CoM state, its traj passed unmodified as ref: accepted, the last tick's
    out[:, 72:78] are traj[-1, :, 0:6] exactly, and no robot raises QP_MAXITER, NONFINITE or NOT_SPD over the five ticks."""
    from linearmpchumanoid_amd import trajectories
    S = _states()
    ctl = make_controller(B, DT, TH, S["zcom"], warm_start=1)
    plans = trajectories.walk_plans(0.2, DT, _walk_specs(), B)
    xs = 0.002 + 0.0005 * np.arange(B)
    ctl.set_plans(**plans)
    ctl.set_xscale(xs)
    st = ctl.new_state(S["q0"], S["v"] * 0.2, t=0.0, v_prev=S["v"] * 0.2)
    terms = ctl.split_terms(ctl.terms(st[:, 0:30].contiguous(), st[:, 30:60].contiguous()))
    torch.cuda.synchronize()
    com, comv = terms["CoM"].cpu().numpy(), terms["comVel"].cpu().numpy()
    lip = ctl.new_lip(com[:, 0:2], comv[:, 0:2], t=0.0)
    traj = ctl.mpc_box_rollout(lip, trajectories.zmp_boxes(plans, xscale=xs), 5)
    assert traj.shape == (5, B, 16)
    out, status = ctl.rollout_zoh(st, 5, 1, ref=traj)
    torch.cuda.synchronize()
    assert _same(out[:, 72:78].contiguous(), traj[4, :, 0:6].contiguous())
    assert int((status[:, 2] & (FLAG_QP_MAXITER | FLAG_NONFINITE | FLAG_NOT_SPD)).max()) == 0, status[:, 2].tolist()
    assert bool(torch.isfinite(st).all()) and bool(torch.isfinite(traj).all())
    ctl.close()


# ------------------------------------------------------------------------------- 7. isolation, refusals, capture
def test_a_non_finite_record_flags_its_robot_alone(zoh):
    ctl, S, refs = zoh["ctl"], zoh["S"], zoh["refs"]
    bad = refs.clone()
    bad[0, 2, 1] = float("nan")                                    # robot 2: xRef velocity
    bad[0, 5, 5] = float("inf")                                    # robot 5: yRef acceleration
    others = [0, 1, 3, 4, 6, 7]

    def step(r):
        st = _fresh(ctl, S)
        out, status = ctl.stand_step(st, ref=r[0])
        return st, out, status

    def loop(r):
        st = _fresh(ctl, S)
        out, status, log = ctl.rollout_zoh(st, 3, 1, log=True, ref=r[0:3])
        return st, out, status, log

    for run in (step, loop):
        good, got = run(refs), run(bad)
        torch.cuda.synchronize()
        flags = got[2][:, 2].tolist()
        assert flags[2] & FLAG_NONFINITE and flags[5] & FLAG_NONFINITE, flags
        assert all(not (int(good[2][i, 2]) & FLAG_NONFINITE) for i in range(B))
        for x, y in zip(good, got):
            assert _same(x[..., others, :].contiguous(), y[..., others, :].contiguous())


def test_the_handle_is_untouched_by_the_new_calls(zoh):
    ctl, S, refs = zoh["ctl"], zoh["S"], zoh["refs"]

    def plain():
        st = _fresh(ctl, S)
        out, status = ctl.stand_step(st)
        torch.cuda.synchronize()
        return st, out, status

    before = plain()
    ctl.stand_step(_fresh(ctl, S), ref=refs[1])
    ctl.rollout_zoh(_fresh(ctl, S), 3, 2, ref=refs[0:3])
    after = plain()
    assert all(_same(x, y) for x, y in zip(before, after))


def test_refusals():
    from linearmpchumanoid_amd import capi
    S = _states()
    L = capi.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    err = lambda: L.lmh_last_error().decode()
    ctl = make_controller(B, DT, TH, S["zcom"])
    ctl.set_refs_stance(2.0, 2)
    st, out, status = _fresh(ctl, S), ctl.new_out(), ctl.new_status()
    ref = _records(ctl, 0.0, (2,))
    sentinels = (st.clone(), out.clone(), status.clone())

    def untouched():
        torch.cuda.synchronize()
        return all(_same(x, y) for x, y in zip((st, out, status), sentinels))

    s = ctl._stream()
    # lmh_eval_ref: its own refusal, then lmh_eval's word for word
    assert L.lmh_eval_ref(ctl._h, p(st), None, p(out), p(status), s) == -2 and err() == "lmh_eval_ref: null d_ref"
    for args in ((None, p(ref), p(out), p(status)), (p(st), p(ref), None, p(status)), (p(st), p(ref), p(out), None)):
        assert L.lmh_eval_ref(ctl._h, *args, s) == -2 and err() == "null device pointer"
    assert L.lmh_eval(ctl._h, None, p(out), p(status), s) == -2 and err() == "null device pointer"
    assert L.lmh_eval_ref(None, p(st), p(ref), p(out), p(status), s) == -2 and err() == "null handle"
    # lmh_rollout_zoh_ref: its own refusal, then lmh_rollout_zoh's word for word
    Z, Z0 = L.lmh_rollout_zoh_ref, L.lmh_rollout_zoh
    assert Z(ctl._h, p(st), p(out), p(status), None, None, None, 2, 1, s) == -2 and err() == "lmh_rollout_zoh_ref: null d_ref"
    for args in ((None, p(out), p(status)), (p(st), None, p(status)), (p(st), p(out), None)):
        assert Z(ctl._h, *args, None, None, p(ref), 2, 1, s) == -2
        mine = err()
        assert Z0(ctl._h, *args, None, None, 2, 1, s) == -2 and err() == mine == "lmh_rollout_zoh: null device pointer"
    for n_ticks, n_sub in ((-1, 1), (1, -1)):
        assert Z(ctl._h, p(st), p(out), p(status), None, None, p(ref), n_ticks, n_sub, s) == -2
        mine = err()
        assert Z0(ctl._h, p(st), p(out), p(status), None, None, n_ticks, n_sub, s) == -2 and err() == mine and "must be >= 0" in mine
    assert Z(None, p(st), p(out), p(status), None, None, p(ref), 2, 1, s) == -2 and err() == "null handle"
    assert Z(ctl._h, p(st), p(out), p(status), None, None, p(ref), 0, 3, s) == 0           # no ticks: LMH_OK, nothing written
    assert untouched()
    # Python: shape and dtype before the C call
    for bad_call in (lambda: ctl.stand_step(st, ref=ref), lambda: ctl.stand_step(st, ref=ref[0, :, 0:6]), lambda: ctl.stand_step(st, ref=ref[0].float()),
                     lambda: ctl.stand_step(st, ref=np.zeros((B, 16), dtype=np.float32)), lambda: ctl.stand_step(st, ref=[[0.0] * 16] * B),
                     lambda: ctl.stand_step(st, ref=ref[0], debug=True), lambda: ctl.rollout_zoh(st, 2, 1, ref=ref[0]),
                     lambda: ctl.rollout_zoh(st, 3, 1, ref=ref), lambda: ctl.rollout_zoh(st, 2, 1, ref=ref.float())):
        with pytest.raises(ValueError):
            bad_call()
    assert untouched()
    ctl.close()
    mixed = make_controller(B, DT, TH, S["zcom"], precision=capi.PRECISION_MIXED)
    mixed.set_refs_stance(2.0, 2)
    with pytest.raises(capi.LmhError) as e:
        mixed.rollout_zoh(st, 2, 2, out=out, status=status, ref=ref)
    assert e.value.code == -2 and "lmh_rollout_zoh: LMH_PRECISION_FP64 handles only" in str(e.value) and untouched()
    mixed.close()
    bad = make_controller(B, DT, TH, S["zcom"], plant=0, contact_k=-1.0)
    bad.set_refs_stance(2.0, 2)
    for n_ticks in (2, 0):
        with pytest.raises(capi.LmhError) as e:
            bad.rollout_zoh(st, n_ticks, 2, out=out, status=status, ref=ref[0:n_ticks] if n_ticks else ref[0:0])
        assert e.value.code == -2 and "contact_k" in str(e.value)
    assert untouched()
    bad.close()


def test_both_calls_captured_on_a_fresh_handle_replay_to_the_eager_bytes():
    from linearmpchumanoid_amd import capi
    S = _states()
    L = capi.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    ctl = make_controller(B, DT, TH, S["zcom"], warm_start=1)     # fresh: no launch before the capture
    ctl.set_refs_stance(2.0, 2)
    rng = np.random.default_rng(20261028)
    ref = _records(ctl, torch.as_tensor(rng.uniform(-0.01, 0.01, (4, B, 6))).to(ctl.device), (4,))
    st0 = _fresh(ctl, S)
    st, out1, out2 = st0.clone(), torch.full((B, 80), -7.0, dtype=torch.float64, device=ctl.device), torch.full((B, 80), -7.0, dtype=torch.float64, device=ctl.device)
    x1, x2 = ctl.new_status(), ctl.new_status()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rcs = (L.lmh_eval_ref(ctl._h, p(st), p(ref[0]), p(out1), p(x1), ctl._stream()),
               L.lmh_rollout_zoh_ref(ctl._h, p(st), p(out2), p(x2), None, None, p(ref[1:]), 3, 2, ctl._stream()))
    assert rcs == (0, 0)
    torch.cuda.synchronize()
    assert _same(st, st0) and bool((out1 == -7).all()) and bool((out2 == -7).all())       # captured, not run
    g.replay()
    torch.cuda.synchronize()
    got = [x.clone() for x in (st, out1, x1, out2, x2)]
    del g
    e_st = st0.clone()
    sent = lambda: torch.full((B, 80), -7.0, dtype=torch.float64, device=ctl.device)           # (the record's two pad words are never written)
    e_out1, e_x1 = ctl.stand_step(e_st, out=sent(), ref=ref[0])
    e_out2, e_x2 = ctl.rollout_zoh(e_st, 3, 2, out=sent(), ref=ref[1:])
    torch.cuda.synchronize()
    for a, b in zip(got, (e_st, e_out1, e_x1, e_out2, e_x2)):
        assert _same(a, b)
    ctl.close()
