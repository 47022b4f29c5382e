"""lmh_rollout_zoh_box on the GPU: the zero-order-hold loop with the box-constrained preview step closed around the measured CoM.

The call is DEFINED by a host loop of calls that exist (include/lmh.h), so the reference of every bit-for-bit case is that loop on a second
copy of the same buffers (zoh_host_loop.host_loop with box=: stand_step on a scratch copy for the CoM state, mpc_box_step, stand_step(ref=),
plant_step in the pieces trajectories.zoh_hold_pieces gives, v += dv in torch).  Inputs: zoh_box_cases.py -- six robots at the start posture,
per-robot plans and boxes built so that robots 2 and 3 have active bounds on every tick and robot 0 (an infinite box) never has.  "Bit for
bit" is helpers.same_bits.
Every bit-for-bit case also asserts that on the samples, and that no sample ran out of rounds."""
import ctypes as C

import numpy as np
import pytest
import torch

import zoh_box_cases as zb
from helpers import make_controller, same_bits as _same
from zoh_host_loop import assert_same as _assert_same, fresh, host_loop

pytestmark = pytest.mark.gpu
B, DT, NT = zb.B, zb.DT, zb.N_TICKS
# per-robot push schedules (plant substep numbers from the run's first substep): a control tick's start, inside a hold, the launch's last
# substep (n_substeps = 3, six ticks: substeps 0 .. 17), the launch's end substep (not applied), none
SCHEDULES = [[6], [7], [3, 9], [17], [18], [-1]]
SCHEDULES_1 = [[2], [3], [1, 4], [5], [6], [-1]]                   # n_substeps = 1, six ticks: every push on a control tick's start; 6 is the end substep


def _controller(N, **cfg):
    from linearmpchumanoid_amd import capi
    d, s = zb.draw(N), zb.start()
    ctl = make_controller(B, DT, d["th"], s["zcom"], mpc_dt=d["mpc_dt"], warm_start=1, **cfg)
    assert ctl.N == N
    p = d["plans"]
    ctl.set_plans(p["zmp_x"], p["zmp_y"], p["phase"], p["segs"], p["seg_of_sample"])
    ctl.set_xscale(d["xs"])
    assert capi.lib().lmh_num_ref_samples(ctl._h) == d["n"]
    return ctl


def _fresh(ctl, t=0.0):
    return fresh(ctl, np.tile(zb.start()["q0"], (B, 1)), zb.velocities(), t)


def _schedules(n_substeps=3):
    ticks = np.full((B, 2), -1, dtype=np.int64)
    for i, s in enumerate(SCHEDULES if n_substeps == 3 else SCHEDULES_1):
        ticks[i, :len(s)] = s
    rng = np.random.default_rng(20261202)
    dv = np.zeros((B, 2, 30))
    dv[:, :, 0:3] = rng.uniform(-0.03, 0.03, (B, 2, 3))
    dv[:, :, 6:] = rng.normal(0.0, 0.1, (B, 2, 24))
    return ticks, dv


def _assert_binding(mpc, per_robot_sets=True):
    """Robots 2 and 3 have active bounds at every tick, robot 0 (its infinite box) never, and no sample ran out of rounds."""
    from linearmpchumanoid_amd import capi
    m = mpc.cpu().numpy()
    assert (m[:, [2, 3], capi.MPC_OFF_ACTIVE] > 0).all(), m[:, :, capi.MPC_OFF_ACTIVE]
    if per_robot_sets:
        assert (m[:, 0, capi.MPC_OFF_ACTIVE] == 0).all(), m[:, 0, capi.MPC_OFF_ACTIVE]
    assert not (m[:, :, 14].astype(np.int64) & capi.FLAG_QP_MAXITER).any()


@pytest.fixture(scope="module")
def ctls():
    made = {}

    def get(N, pushes=0):
        """pushes: 0 = a handle without a schedule, 1 | 3 = the schedules made for that n_substeps"""
        if (N, pushes) not in made:
            c = _controller(N)
            if pushes:
                c.set_pushes(*_schedules(pushes))
            made[(N, pushes)] = c
        return made[(N, pushes)]

    yield get
    for c in made.values():
        c.close()


def _box(ctl, N, shared=False):
    d = zb.draw(N)
    return torch.as_tensor(np.array(d["shared"] if shared else d["box"])).to(ctl.device)


# ------------------------------------------------------------------------------- 1. the host loop
@pytest.mark.parametrize("t0", [0.0, zb.T_MID], ids=["from t = 0", "mid-plan"])
@pytest.mark.parametrize("shared", [False, True], ids=["per-robot sets", "one shared set"])
@pytest.mark.parametrize("n_substeps", [1, 3])
@pytest.mark.parametrize("N", [8, 32, 64])
def test_the_call_is_the_host_loop_bit_for_bit(ctls, N, n_substeps, shared, t0):
    ctl = ctls(N)
    box = _box(ctl, N, shared)
    n_ticks = NT if N == 32 else 6
    sa, sb = _fresh(ctl, t0), _fresh(ctl, t0)
    ra = ctl.rollout_zoh_box(sa, box, n_ticks, n_substeps, log=True)
    rb = host_loop(ctl, sb, ctl.new_status(), n_ticks, n_substeps, box=box)
    torch.cuda.synchronize()
    _assert_same((N, n_substeps, shared, t0), (("mpc", ra["mpc"], rb["mpc"]), ("state", sa, sb), ("out", ra["out"], rb["out"]), ("status", ra["status"], rb["status"]),
                                               ("log", ra["log"], rb["log"])))
    _assert_binding(ra["mpc"], not shared)
    assert _same(ra["out"][:, 72:78].contiguous(), ra["mpc"][n_ticks - 1, :, 0:6].contiguous())   # the reference words are the sample's
    assert float(sa[0, 90]) == sum([t0] + [DT] * (n_ticks * n_substeps))
    k = ra["mpc"][:, :, 13].cpu().numpy()
    assert (k[0] == int(t0 / zb.HORIZONS[N])).all()
    # mpc=False stores no sample and changes nothing else
    sc = _fresh(ctl, t0)
    rc = ctl.rollout_zoh_box(sc, box, n_ticks, n_substeps, mpc=False, log=True)
    assert rc["mpc"] is None
    _assert_same("no d_mpc", (("state", sc, sa), ("out", rc["out"], ra["out"]), ("status", rc["status"], ra["status"]), ("log", rc["log"], ra["log"])))


# ------------------------------------------------------------------------------- 2. pushes and a wrench per tick
@pytest.mark.parametrize("n_substeps", [1, 3])
def test_pushes_and_a_wrench_sequence_are_the_host_loop_of_pieces(ctls, n_substeps):
    N, n_ticks = 32, 6
    ctl, plain = ctls(N, pushes=n_substeps), ctls(N)
    box = _box(ctl, N)
    ticks, dv = _schedules(n_substeps)
    bw = torch.as_tensor(np.random.default_rng(20261203).normal(0.0, 1.0, (n_ticks, B, 6))).to(ctl.device)
    sa, sb, sc = _fresh(ctl), _fresh(plain), _fresh(ctl)
    ra = ctl.rollout_zoh_box(sa, box, n_ticks, n_substeps, base_wrench=bw, pushes=True, log=True)
    rb = host_loop(plain, sb, plain.new_status(), n_ticks, n_substeps, bw=bw, sched=(ticks, dv), box=box)
    rc = ctl.rollout_zoh_box(sc, box, n_ticks, n_substeps, base_wrench=bw, pushes=False, log=True)
    torch.cuda.synchronize()
    _assert_same(("pushes", n_substeps), (("mpc", ra["mpc"], rb["mpc"]), ("state", sa, sb), ("out", ra["out"], rb["out"]), ("status", ra["status"], rb["status"]),
                                          ("log", ra["log"], rb["log"])))
    _assert_binding(ra["mpc"])
    from linearmpchumanoid_amd.trajectories import zoh_hold_pieces
    pushed = [i for i in range(B) if any(s is not None or any(r is not None for _, r in h) for s, h in zoh_hold_pieces(ticks[i], 0, n_ticks, n_substeps))]
    assert len(pushed) >= 3 and 5 not in pushed
    for i in range(B):
        assert _same(sa[i], sc[i]) == (i not in pushed), (i, "a pushed robot differs from pushes=False, an unpushed one does not")
    if n_substeps == 3:
        # robot 0's push falls on the start of control tick 2: that tick's sample holds the pushed CoM velocity (its state words), tick 1's does not
        a, c = ra["mpc"].cpu().numpy(), rc["mpc"].cpu().numpy()
        assert SCHEDULES[0] == [6] and np.array_equal(a[:2, 0], c[:2, 0]) and not np.array_equal(a[2, 0, [9, 11]], c[2, 0, [9, 11]])
        assert np.array_equal(a[2, 0, [8, 10]], c[2, 0, [8, 10]])                       # the CoM itself has not moved yet
        # robot 4's push is due on the launch's end substep: not applied
        assert SCHEDULES[4] == [18] and 4 not in pushed and 3 in pushed


# ------------------------------------------------------------------------------- 3. trace and metrics
def _everything(ctl, box, n_ticks, every=0, trace=None, metrics=None, status=None, st=None, first_tick=0, bw=None):
    st = _fresh(ctl) if st is None else st
    r = ctl.rollout_zoh_box(st, box, n_ticks, 3, base_wrench=bw[first_tick:first_tick + n_ticks], pushes=True, log=True, trace_every=every, trace=trace,
                            metrics=metrics, status=status)
    return dict(r, state=st)


@pytest.fixture(scope="module")
def full(ctls):
    ctl = ctls(32, pushes=3)
    bw = torch.as_tensor(np.random.default_rng(20261204).normal(0.0, 1.0, (6, B, 6))).to(ctl.device)
    return dict(ctl=ctl, box=_box(ctl, 32), bw=bw)


@pytest.mark.parametrize("every", [1, 4])
def test_trace_samples_are_the_records_of_shorter_launches(full, every):
    ctl, box, bw = full["ctl"], full["box"], full["bw"]
    n = 6 // every
    buf = torch.full((n + 1, B, 180), -7.0, dtype=torch.float64, device=ctl.device)          # one sample more than the call may write
    r = _everything(ctl, box, 6, every, trace=buf, bw=bw)
    whole = _everything(ctl, box, 6, bw=bw)
    torch.cuda.synchronize()
    _assert_same("the launch itself", (("state", r["state"], whole["state"]), ("out", r["out"], whole["out"]), ("status", r["status"], whole["status"]),
                                       ("log", r["log"], whole["log"]), ("mpc", r["mpc"], whole["mpc"])))
    assert bool((buf[n:] == -7.0).all())
    for j in range(n):
        m = (j + 1) * every
        short = _everything(ctl, box, m, bw=bw)
        torch.cuda.synchronize()
        want = torch.cat([short["state"], short["out"], short["status"].double()], dim=1)
        _assert_same(("sample", every, j), (("against the shorter launch", buf[j], want),))
        assert _same(buf[j, :, 96 + 72:96 + 78].contiguous(), r["mpc"][m - 1, :, 0:6].contiguous())     # out[72:78] of the sample are m[0:6]


def test_metrics_are_the_fold_of_the_every_tick_trace(full):
    from linearmpchumanoid_amd import metrics as hm
    ctl, box, bw = full["ctl"], full["box"], full["bw"]
    m_alone, m_both = ctl.new_metrics(0.3, 0.2), ctl.new_metrics(0.3, 0.2)
    alone = _everything(ctl, box, 6, metrics=m_alone, bw=bw)
    both = _everything(ctl, box, 6, every=1, metrics=m_both, bw=bw)
    torch.cuda.synchronize()
    ref = hm.fold_trace(hm.identity(B, 0.3, 0.2), both["trace"].cpu().numpy())
    assert _same(m_both.cpu().numpy(), ref) and _same(m_alone, m_both)
    _assert_same("metrics change nothing else", (("state", alone["state"], both["state"]), ("out", alone["out"], both["out"]), ("status", alone["status"], both["status"]),
                                                 ("mpc", alone["mpc"], both["mpc"])))
    assert ctl.split_metrics(m_alone.cpu().numpy())["count"].tolist() == [6] * B


# ------------------------------------------------------------------------------- 4. split
def test_six_ticks_are_two_then_four_with_everything_on(full):
    ctl, box, bw = full["ctl"], full["box"], full["bw"]
    m6, m24 = ctl.new_metrics(0.3, 0.2), ctl.new_metrics(0.3, 0.2)
    r6 = _everything(ctl, box, 6, every=2, metrics=m6, bw=bw)
    r2 = _everything(ctl, box, 2, every=2, metrics=m24, bw=bw)
    status2 = r2["status"].clone()
    r4 = _everything(ctl, box, 4, every=2, metrics=m24, st=r2["state"], status=r2["status"].clone(), first_tick=2, bw=bw)
    torch.cuda.synchronize()
    tb = r4["trace"].clone()
    tb[:, :, 177] = torch.maximum(tb[:, :, 177], status2[None, :, 1].double())
    tb[:, :, 178] = (tb[:, :, 178].long() | status2[None, :, 2].long()).double()
    _assert_same("split", (("state", r6["state"], r4["state"]), ("out", r6["out"], r4["out"]), ("log", r6["log"], torch.cat([r2["log"], r4["log"]])),
                           ("mpc", r6["mpc"], torch.cat([r2["mpc"], r4["mpc"]])), ("trace", r6["trace"], torch.cat([r2["trace"], tb])), ("metrics", m6, m24)))
    s6, s4 = r6["status"], r4["status"]
    assert torch.equal(s6[:, 0], s4[:, 0]) and torch.equal(s6[:, 3], s4[:, 3])
    assert torch.equal(s6[:, 1], torch.maximum(status2[:, 1], s4[:, 1])) and torch.equal(s6[:, 2], status2[:, 2] | s4[:, 2])
    assert SCHEDULES[0] == [6]                                       # a push on the substep the first launch ends on (2 x 3)
    _assert_binding(r6["mpc"])


# ------------------------------------------------------------------------------- 5. an empty box sample
def test_an_empty_box_sample_flags_its_robot_alone(ctls):
    from linearmpchumanoid_amd import capi
    N = 32
    ctl = ctls(N)
    d = zb.draw(N)
    good_box = _box(ctl, N)
    bad_box = torch.as_tensor(zb.with_empty_sample(d["box"], 5)).to(ctl.device)              # sample 5: inside the window [0, 32] of every tick
    bad, others = zb.EMPTY_ROBOT, [i for i in range(B) if i != zb.EMPTY_ROBOT]
    sg, sb = _fresh(ctl), _fresh(ctl)
    good = ctl.rollout_zoh_box(sg, good_box, 6, 3, log=True, trace_every=1)
    got = ctl.rollout_zoh_box(sb, bad_box, 6, 3, log=True, trace_every=1)
    torch.cuda.synchronize()
    want = capi.FLAG_NONFINITE | capi.FLAG_BOX_EMPTY
    assert int(got["status"][bad, 2]) & want == want and all((int(got["status"][i, 2]) & want) == 0 for i in others)
    assert bool(torch.isnan(got["mpc"][:, bad, 0:8]).all()) and all(int(v) & want == want for v in got["mpc"][:, bad, 14].tolist())
    assert bool(torch.isnan(got["out"][bad, 72:78]).all())
    for k, a, b in (("state", sg, sb), ("out", good["out"], got["out"]), ("status", good["status"], got["status"])):
        assert _same(a[others], b[others]), k
    for k in ("log", "trace", "mpc"):
        assert _same(good[k][:, others], got[k][:, others]), k


# ------------------------------------------------------------------------------- 6. behaviour
def test_a_pushed_robots_zmp_stays_inside_the_stance_box():
    """A sideways push of zoh_box_cases.PUSH_DV_Y at the start of control tick PUSH_TICK (tests/test_zoh_box.py holds the amplitude to the
    oracle).  Under rollout_zoh_ex the ZMP the built-in step commands on that tick, CoM + D u from the out record, is outside the stance box;
    under rollout_zoh_box every sample's ZMP is inside the bounds of its own sample k, exactly, on both axes."""
    from linearmpchumanoid_amd import trajectories as tj
    N, n_sub, n_ticks = 32, 3, 6
    d, s = zb.draw(N), zb.start()
    ctl = make_controller(B, DT, d["th"], s["zcom"], mpc_dt=d["mpc_dt"], warm_start=1)
    ctl.set_refs_stance(2.0, 2)
    zx, zy = tj.stance_zmp(2.0, d["mpc_dt"], 2)
    box = tj.zmp_box(dict(zmp_x=zx, zmp_y=zy, phase=None))
    sb = zb.STANCE_BOX
    assert np.allclose(box[:, 0], [sb["lo_x"], sb["hi_x"], sb["lo_y"], sb["hi_y"]], rtol=0.0, atol=1e-15)     # (-0.05 - 0.025 is an ulp off -0.075)
    dv = np.zeros((1, 30))
    dv[0, 1] = zb.PUSH_DV_Y
    ctl.set_pushes(np.array([zb.PUSH_TICK * n_sub]), dv)
    fresh = lambda: ctl.new_state(np.tile(s["q0"], (B, 1)), np.zeros((B, 30)), t=0.0)
    plain = ctl.rollout_zoh_ex(fresh(), n_ticks, n_sub, pushes=True, trace_every=1)
    boxed = ctl.rollout_zoh_box(fresh(), box, n_ticks, n_sub, pushes=True)
    torch.cuda.synchronize()
    D = -s["zcom"] / zb.GRAVITY
    o = plain["trace"][zb.PUSH_TICK, :, 96:176].cpu().numpy()
    zmp_plain = np.stack([o[:, 66] + D * o[:, 74], o[:, 67] + D * o[:, 77]], axis=1)
    print("\nthe built-in step's ZMP on the pushed tick:", zmp_plain[0], " box y:", sb["lo_y"], sb["hi_y"])
    assert (zmp_plain[:, 1] > sb["hi_y"]).all()                     # the test is meaningful: the unconstrained command leaves the sole
    m = boxed["mpc"].cpu().numpy()
    k = np.clip(m[:, :, 13].astype(np.int64), 0, box.shape[1] - 1)
    print("the constrained step's ZMP on the pushed tick:", m[zb.PUSH_TICK, 0, 6:8], " active:", m[:, 0, 15])
    assert (box[0][k] <= m[:, :, 6]).all() and (m[:, :, 6] <= box[1][k]).all() and (box[2][k] <= m[:, :, 7]).all() and (m[:, :, 7] <= box[3][k]).all()
    assert (m[zb.PUSH_TICK, :, 15] > 0).all() and (m[:, :, 14] == 0).all()
    ctl.close()


# ------------------------------------------------------------------------------- 7. handle untouched
def test_the_handle_is_untouched():
    N = 32
    fresh_ctl, used = _controller(N), _controller(N)
    box = _box(used, N)
    for _ in range(2):
        used.rollout_zoh_box(_fresh(used), box, 6, 3, trace_every=2, metrics=used.new_metrics())
    torch.cuda.synchronize()
    res = []
    for c in (fresh_ctl, used):
        st = _fresh(c)
        out, status = c.rollout_zoh(st, 6, 3)
        torch.cuda.synchronize()
        res.append((st.clone(), out.clone(), status.clone()))
    for a, b in zip(*res):
        assert _same(a, b)
    fresh_ctl.close(); used.close()


# ------------------------------------------------------------------------------- 8. graph capture
@pytest.mark.parametrize("N", [32, 64])
def test_captured_on_a_fresh_handle_replays_to_the_eager_bytes(N):
    from linearmpchumanoid_amd import capi, metrics as hm
    L = capi.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    ctl = _controller(N)                                          # fresh: no launch before the capture
    ctl.set_pushes(*_schedules())
    dev = ctl.device
    box = _box(ctl, N)
    ident = torch.as_tensor(hm.identity(B, 0.3, 0.2)).to(dev)     # (not new_metrics: no launch of the handle's before the capture)
    st0 = _fresh(ctl)
    sent = lambda *shape: torch.full(shape, -7.0, dtype=torch.float64, device=dev)
    st, out, status, log, trace, m, mpc = st0.clone(), sent(B, 80), ctl.new_status(), sent(6, B, 36), sent(3, B, 180), ident.clone(), sent(6, B, 16)
    bw = torch.as_tensor(np.random.default_rng(20261205).normal(0.0, 1.0, (6, B, 6))).to(dev)
    opts = capi.LmhZohOpts(d_base_wrench=p(bw), d_ref=None, d_log=p(log), d_trace=p(trace), d_metrics=p(m), trace_every=2, wrench_per_tick=1, pushes=1, reserved=0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = L.lmh_rollout_zoh_box(ctl._h, p(st), p(out), p(status), C.byref(opts), p(box), box.shape[2], B, p(mpc), 6, 3, ctl._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert _same(st, st0) and bool((out == -7).all()) and bool((mpc == -7).all()) and _same(m, ident)       # captured, not run
    g.replay()
    torch.cuda.synchronize()
    got = [x.clone() for x in (st, out, status, log, trace, m, mpc)]
    del g
    e_st, e_m = st0.clone(), ident.clone()
    e = ctl.rollout_zoh_box(e_st, box, 6, 3, mpc=sent(6, B, 16), base_wrench=bw, pushes=True, log=sent(6, B, 36), trace_every=2, trace=sent(3, B, 180), metrics=e_m,
                            out=sent(B, 80))
    torch.cuda.synchronize()
    for name, a, b in zip(("state", "out", "status", "log", "trace", "metrics", "mpc"), got, (e_st, e["out"], e["status"], e["log"], e["trace"], e_m, e["mpc"])):
        assert _same(a, b), name
    assert not bool((got[6][:, :, 0:15] == -7).any()) and float(got[5][0, 0]) == 6
    ctl.close()


# ------------------------------------------------------------------------------- 9. refusals
def test_refusals(ctls):
    from linearmpchumanoid_amd import capi
    N = 32
    L = capi.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    err = lambda: L.lmh_last_error().decode()
    ctl = ctls(N)
    dev, d = ctl.device, zb.draw(N)
    box = _box(ctl, N)
    ns = d["n"]
    st, out, status = _fresh(ctl), ctl.new_out(), ctl.new_status()
    mpc, m = torch.full((6, B, 16), -7.0, dtype=torch.float64, device=dev), ctl.new_metrics()
    ref = torch.zeros((6, B, 16), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    bufs = (st, out, status, mpc, m)
    canaries = tuple(x.clone() for x in bufs)

    def untouched():
        torch.cuda.synchronize()
        return all(_same(x, y) for x, y in zip(bufs, canaries))

    s = ctl._stream()
    Z = L.lmh_rollout_zoh_box

    def call(n_ticks=6, n_substeps=3, state=st, handle=ctl, d_box=box, n_samples=ns, n_sets=B, **fields):
        o = capi.LmhZohOpts(**{k: (p(v) if isinstance(v, torch.Tensor) else v) for k, v in fields.items()})
        return Z(handle._h, None if state is None else p(state), p(out), p(status), C.byref(o), None if d_box is None else p(d_box), n_samples, n_sets, p(mpc),
                 n_ticks, n_substeps, s)

    assert call(d_box=None, d_metrics=m) == -2 and err() == "lmh_rollout_zoh_box: null d_box"
    assert call(n_samples=ns - 1, d_metrics=m) == -2 and err() == "lmh_rollout_zoh_box: n_samples must be lmh_num_ref_samples"
    for n_sets in (0, 2, B + 1):
        assert call(n_sets=n_sets, d_metrics=m) == -2 and err() == "lmh_rollout_zoh_box: n_sets must be 1 or n_instances"
    assert call(d_ref=ref, d_metrics=m) == -2 and err().startswith("lmh_rollout_zoh_box: opts->d_ref must be NULL")
    assert untouched()
    # lmh_rollout_zoh_ex's own, in its words
    for fields, words in ((dict(wrench_per_tick=2), "lmh_rollout_zoh_ex: wrench_per_tick must be 0 or 1"), (dict(pushes=2), "lmh_rollout_zoh_ex: pushes must be 0 or 1"),
                          (dict(reserved=1), "lmh_rollout_zoh_ex: reserved must be 0"), (dict(wrench_per_tick=1), "lmh_rollout_zoh_ex: wrench_per_tick = 1 needs d_base_wrench"),
                          (dict(trace_every=2), "lmh_rollout_zoh_ex: d_trace and trace_every > 0 go together (NULL and 0: no trace)")):
        assert call(d_metrics=m, **fields) == -2 and err() == words, fields
    assert call(n_substeps=0, pushes=1, d_metrics=m) == -2 and err().startswith("lmh_rollout_zoh_ex: pushes = 1 needs n_substeps > 0")
    assert call(state=None) == -2 and err() == "lmh_rollout_zoh: null device pointer"
    for n_ticks, n_sub in ((-1, 1), (1, -1)):
        assert call(n_ticks=n_ticks, n_substeps=n_sub, d_metrics=m) == -2 and "must be >= 0" in err()
    assert Z(None, p(st), p(out), p(status), None, p(box), ns, B, p(mpc), 6, 3, s) == -2 and err() == "null handle"
    assert call(n_ticks=0, d_metrics=m) == 0                        # no tick: nothing enqueued
    assert untouched()
    # Python: a reference, a malformed box, a sample buffer the launch would overrun
    for bad_call in (lambda: ctl.rollout_zoh_box(st, box, 6, 3, ref=ref), lambda: ctl.rollout_zoh_box(st, box[:, 0:3], 6, 3), lambda: ctl.rollout_zoh_box(st, box[0:2], 6, 3),
                     lambda: ctl.rollout_zoh_box(st, box, 6, 3, mpc=mpc[0:5]), lambda: ctl.rollout_zoh_box(st, box, -1, 3)):
        with pytest.raises(ValueError):
            bad_call()
    assert untouched()
    s0 = zb.start()
    for precision in (capi.PRECISION_MIXED, capi.PRECISION_FP32):
        other = _controller(N, precision=precision)
        assert call(handle=other, d_metrics=m) == -2 and "LMH_PRECISION_FP64 handles only" in err()
        other.close()
    bad = make_controller(B, DT, d["th"], s0["zcom"], mpc_dt=d["mpc_dt"], plant=0, contact_k=-1.0)
    p_ = d["plans"]
    bad.set_plans(p_["zmp_x"], p_["zmp_y"], p_["phase"], p_["segs"], p_["seg_of_sample"])
    assert call(handle=bad, d_metrics=m) == -2 and "contact_k" in err()
    bad.close()
    assert untouched()
