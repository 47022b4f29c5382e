"""CPU side of lmh_rollout_zoh_io: the host statement of the actuator (trajectories.actuator_step) against a walk one joint at a time, the
records' rules in the library's words, the oracle statement of the loop the GPU parity test rests on, and the binding.  No GPU is used."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import plant_step_cases as pc
import zoh_cases as zc
import zoh_ex_cases as zx
import zoh_io_cases as zi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_declared_bound_and_exported(hip_lib):
    from linearmpchumanoid_amd import capi
    from linearmpchumanoid_amd.controller import BatchedController
    raw = open(os.path.join(ROOT, "include", "lmh.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name, n_args in (("lmh_rollout_zoh_io", 9), ("lmh_set_actuators", 3), ("lmh_actuators_per_instance", 1), ("lmh_get_actuators", 3)):
        assert re.search(r"\bint\s+%s\s*\(" % name, src) and name in capi.EXPORTS and hasattr(hip_lib, name), name
        assert len(capi.PROTOTYPES[name][1]) == n_args, name
    args = capi.PROTOTYPES["lmh_rollout_zoh_io"][1]
    assert args[4] == C.POINTER(capi.LmhZohOpts) and args[5] == C.POINTER(capi.LmhZohIo)
    for m in ("rollout_zoh_io", "set_actuators", "get_actuators", "new_act_mem"):
        assert callable(getattr(BatchedController, m)), m
    # the record: three pointers, two int32, in the header's order
    body = re.search(r"typedef struct lmh_zoh_io \{(.*?)\} lmh_zoh_io;", src, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*;", body) == [n for n, _ in capi.LmhZohIo._fields_] and C.sizeof(capi.LmhZohIo) == 3 * 8 + 2 * 4
    assert [t for _, t in capi.LmhZohIo._fields_] == [C.c_void_p] * 3 + [C.c_int32] * 2
    # the strides and the flag are the header's
    defs = dict(re.findall(r"#define\s+(LMH_\w+)\s+(\d+)", raw))
    assert (capi.ACT_STRIDE, capi.ACT_OFF_TAU_MAX, capi.ACT_OFF_ALPHA, capi.ACT_OFF_DELAY, capi.ACT_MAX_DELAY, capi.ACT_MEM_STRIDE, capi.FLAG_TAU_LIMIT) == tuple(
        int(defs[k]) for k in ("LMH_ACT_STRIDE", "LMH_ACT_OFF_TAU_MAX", "LMH_ACT_OFF_ALPHA", "LMH_ACT_OFF_DELAY", "LMH_ACT_MAX_DELAY", "LMH_ACT_MEM_STRIDE", "LMH_FLAG_TAU_LIMIT"))
    assert capi.ACT_MEM_STRIDE == 24 * (1 + capi.ACT_MAX_DELAY) and capi.FLAG_TAU_LIMIT & 15 == 0
    assert (zi.ACT_STRIDE, zi.ACT_MEM_STRIDE, zi.MAX_DELAY) == (capi.ACT_STRIDE, capi.ACT_MEM_STRIDE, capi.ACT_MAX_DELAY)
    # the launcher is declared once and carries the new call (no new symbol: the stand-alone host programs link against one stub per launcher)
    launch = open(os.path.join(ROOT, "linearmpchumanoid_amd", "csrc", "lmh_launch.h")).read()
    decl = re.findall(r"void\s+lmh_launch_rollout_zoh\s*\(([^;]*)\)\s*;", launch)
    assert len(decl) == 1 and "const LmhZohIo *" in decl[0] and len(re.findall(r"void\s+lmh_launch_\w+\s*\(", launch)) == 19


def test_without_a_handle_the_calls_are_refused(hip_lib):
    from linearmpchumanoid_amd import capi
    io = capi.LmhZohIo(actuators=1, reserved=3)
    for i in (None, C.byref(io)):
        assert hip_lib.lmh_rollout_zoh_io(None, None, None, None, None, i, 3, 2, None) == -2 and hip_lib.lmh_last_error() == b"null handle"
    rec = np.zeros(capi.ACT_STRIDE)
    assert hip_lib.lmh_set_actuators(None, rec.ctypes.data_as(C.c_void_p), 1) == -2 and hip_lib.lmh_last_error() == b"null handle"
    assert hip_lib.lmh_get_actuators(None, 0, rec.ctypes.data_as(C.c_void_p)) == -2 and hip_lib.lmh_last_error() == b"null handle"
    assert hip_lib.lmh_actuators_per_instance(None) == 0


def _record(delay, alpha, limit, rng):
    rec = np.zeros(zi.ACT_STRIDE)
    rec[0:24] = limit
    rec[24:48] = alpha
    rec[48] = delay
    rec[49:] = rng.normal(0.0, 1.0, 7)                              # the pad is ignored
    return rec


@pytest.mark.parametrize("limit", [0.8, np.inf], ids=["a limit that binds", "no limit"])
@pytest.mark.parametrize("alpha", zi.ALPHAS)
@pytest.mark.parametrize("delay", zi.DELAYS)
def test_actuator_step_against_the_walk_one_joint_at_a_time(delay, alpha, limit):
    """Ten control ticks of commands of order one (so that 0.8 cuts some joints on every tick and not others) from a memory of random
    words: y, the flag and the whole memory after every tick, bit for bit; the queue split across two calls is the one-robot call twice."""
    from linearmpchumanoid_amd.trajectories import actuator_step
    rng = np.random.default_rng(20261210 + 100 * delay + int(10 * alpha))
    rec = _record(delay, alpha, limit, rng)
    rec[24 + 5] = 1.0 if alpha != 1.0 else 0.6                      # one joint on the other branch of the lag
    mem0 = rng.normal(0.0, 1.0, zi.ACT_MEM_STRIDE)
    cmds = rng.normal(0.0, 1.0, (10, 24))
    mem, brute = mem0.copy(), mem0.tolist()
    cut = 0
    for j, cmd in enumerate(cmds):
        y, limited = actuator_step(rec, mem, cmd)
        yb, lb = zi.brute_actuator(rec.tolist(), brute, cmd.tolist())
        assert y.shape == (24,) and y.dtype == np.float64 and np.array_equal(y, np.array(yb)) and bool(limited) == lb, j
        assert np.array_equal(mem, np.array(brute)), j
        assert np.array_equal(mem[0:24], y)                         # PREV <- y
        assert np.array_equal(mem[24 + 24 * delay:], mem0[24 + 24 * delay:])      # slots at and above the delay are never touched
        cut += int(limited)
        if np.isfinite(limit):
            assert (np.abs(y[rec[24:48] == 1.0]) <= limit).all()     # without a lag the limit holds exactly
    assert cut == (10 if np.isfinite(limit) else 0)
    # the delay itself: with no limit and no lag on joint 7, tick j receives the command of tick j - delay, before that the memory's words
    rec2 = _record(delay, 1.0, np.inf, rng)
    mem = mem0.copy()
    got = np.array([actuator_step(rec2, mem, cmd)[0] for cmd in cmds])
    want = np.concatenate([mem0[24:24 + 24 * delay].reshape(delay, 24), cmds])[:10]
    assert np.array_equal(got, want)
    # the same ten ticks as 4 + 6 with the memory handed on, and as a batch of two robots of which this is the second
    mem_a, mem_b = mem0.copy(), np.stack([np.zeros(zi.ACT_MEM_STRIDE), mem0])
    recs = np.stack([_record(0, 1.0, np.inf, rng), rec])
    first = [actuator_step(rec, mem_a, cmd)[0] for cmd in cmds[:4]]
    rest = [actuator_step(rec, mem_a, cmd)[0] for cmd in cmds[4:]]
    batch = [actuator_step(recs, mem_b, np.stack([cmd, cmd])) for cmd in cmds]
    mem = mem0.copy()
    whole = [actuator_step(rec, mem, cmd)[0] for cmd in cmds]
    assert np.array_equal(np.array(first + rest), np.array(whole)) and np.array_equal(mem_a, mem)
    assert np.array_equal(np.array([y[1] for y, _ in batch]), np.array(whole)) and np.array_equal(mem_b[1], mem)
    assert np.array_equal(np.array([y[0] for y, _ in batch]), cmds) and not any(l[0] for _, l in batch)


def test_actuator_step_passes_a_nan_through_and_flags_it():
    from linearmpchumanoid_amd.trajectories import actuator_step
    rng = np.random.default_rng(20261211)
    rec, mem = _record(0, 1.0, 0.5, rng), np.zeros(zi.ACT_MEM_STRIDE)
    cmd = np.full(24, 0.1)
    cmd[3] = np.nan
    y, limited = actuator_step(rec, mem, cmd)
    assert np.isnan(y[3]) and np.array_equal(np.delete(y, 3), np.delete(cmd, 3)) and bool(limited)     # c != u holds for a NaN: the definition's words
    with pytest.raises(ValueError):
        actuator_step(rec, mem.astype(np.float32), cmd)
    with pytest.raises(ValueError):
        actuator_step(rec, np.zeros(100), cmd)


def test_actuator_records_and_their_refusals():
    from linearmpchumanoid_amd import trajectories as tj
    rec = tj.actuator_records(4)
    assert rec.shape == (4, zi.ACT_STRIDE) and np.isinf(rec[:, 0:24]).all() and (rec[:, 24:48] == 1.0).all() and not rec[:, 48:].any()
    rec = tj.actuator_records(4, tau_max=np.arange(24.0), alpha=0.5, delay=[0, 1, 7, 3])
    assert np.array_equal(rec[2, 0:24], np.arange(24.0)) and (rec[:, 24:48] == 0.5).all() and rec[:, 48].tolist() == [0, 1, 7, 3]
    rec = tj.actuator_records(4, tau_max=np.arange(96.0).reshape(4, 24), delay=2)
    assert rec[3, 23] == 95.0 and rec[:, 48].tolist() == [2] * 4
    bad_limit = np.full((4, 24), 1.0); bad_limit[2, 5] = -0.1
    nan_limit = np.full((4, 24), 1.0); nan_limit[1, 0] = np.nan
    bad_alpha = np.full((4, 24), 1.0); bad_alpha[3, 1] = 0.0
    for kw, who, words in ((dict(tau_max=bad_limit), 2, tj.ACT_ERR_LIMIT), (dict(tau_max=nan_limit), 1, tj.ACT_ERR_LIMIT), (dict(alpha=bad_alpha), 3, tj.ACT_ERR_ALPHA),
                           (dict(alpha=1.5), 0, tj.ACT_ERR_ALPHA), (dict(alpha=np.nan), 0, tj.ACT_ERR_ALPHA), (dict(delay=[0, 8, 0, 0]), 1, tj.ACT_ERR_DELAY),
                           (dict(delay=[0, 0, 1.5, 0]), 2, tj.ACT_ERR_DELAY), (dict(delay=-1), 0, tj.ACT_ERR_DELAY), (dict(delay=np.nan), 0, tj.ACT_ERR_DELAY)):
        with pytest.raises(ValueError, match=re.escape(f"robot {who}: {words}")):
            tj.actuator_records(4, **kw)
    # the same words in the library's source
    src = open(os.path.join(ROOT, "linearmpchumanoid_amd", "csrc", "lmh_capi.hip")).read()
    for words in (tj.ACT_ERR_LIMIT, tj.ACT_ERR_ALPHA, tj.ACT_ERR_DELAY):
        assert '"%s"' % words in src, words


def test_oracle_loop_is_the_zoh_ex_loop_with_the_added_statements():
    S = pc.contact_states()
    i = 3
    x0 = np.concatenate([S["q"][i], S["v"][i]])
    bw = zx.wrench_sequence(5, 3, 1)[:, 0]
    dv = zx.push_dv(11, 1)
    ref = zx.oracle_zoh_ex(pc.make_oracle(), x0, 3, 2, base_wrench=bw, ticks=[3], dv=dv)
    # nothing set, and the default record on a zeroed memory: oracle_zoh_ex's numbers exactly
    from linearmpchumanoid_amd.trajectories import actuator_records
    for kw in (dict(), dict(record=actuator_records(1)[0]), dict(meas=np.zeros((3, 60)))):
        r = zi.oracle_zoh_io(pc.make_oracle(), x0, 3, 2, base_wrench=bw, ticks=[3], dv=dv, **kw)
        for k in ("state", "v_prev", "tau", "f", "qpp", "taus", "k"):
            assert np.array_equal(r[k], ref[k]), (k, list(kw))
        assert r["t"] == ref["t"] and np.array_equal(r["applied"], ref["taus"]) and not r["limited"].any()
    # a measurement error: the evaluation changes, v_prev is the measured v, and the plant went on from the true state -- by hand for one tick
    meas = zi.measurement_noise(7, 3, 1)[:, 0]
    r = zi.oracle_zoh_io(pc.make_oracle(), x0, 1, 2, meas=meas)
    o = pc.make_oracle()
    o.set_prev_velocity(x0[30:])
    e = o.eval(x0[:30] + meas[0, :30], x0[30:] + meas[0, 30:], 0.0)
    x1 = pc.oracle_plant_steps(o, x0, np.concatenate([np.zeros(6), e["tau"]]), 2)
    assert np.array_equal(r["state"], x1) and np.array_equal(r["v_prev"], x0[30:] + meas[0, 30:]) and np.array_equal(r["tau"], e["tau"])
    assert not np.array_equal(r["tau"], zc.oracle_zoh(pc.make_oracle(), x0, 1, 2)["tau"])
    # a delay of two ticks from a memory holding tau0: the plant receives tau0 twice, then the first command
    tau0 = ref["taus"][0] * 0.5
    mem = np.tile(tau0, 8)
    r = zi.oracle_zoh_io(pc.make_oracle(), x0, 3, 2, record=actuator_records(1, delay=2)[0], mem=mem)
    assert np.array_equal(r["applied"][0], tau0) and np.array_equal(r["applied"][1], tau0) and np.array_equal(r["applied"][2], r["taus"][0])
    assert np.array_equal(mem[24:72].reshape(2, 24), r["taus"][1:3]) and np.array_equal(mem[0:24], r["taus"][0])
    # (2) then (1) with the memory handed on is (3)
    o, mem2 = pc.make_oracle(), np.tile(tau0, 8)
    a = zi.oracle_zoh_io(o, x0, 2, 2, record=actuator_records(1, delay=2)[0], mem=mem2)
    b = zi.oracle_zoh_io(o, a["state"], 1, 2, record=actuator_records(1, delay=2)[0], mem=mem2, t0=a["t"], v_prev=a["v_prev"])
    assert np.array_equal(b["state"], r["state"]) and np.array_equal(mem2, mem)


def test_the_compared_run_is_a_usable_reference():
    """The run test_gpu_zoh_io.py holds against the oracle: finite, the QP solved at every evaluation, every option matters on the robots
    that have it, and the limit binds on every robot that has one (the oracle's own commanded torques exceed it)."""
    runs, plain, I = zi.oracle_io_run(), zc.oracle_run(), zi.oracle_io_inputs()
    assert len(runs) == zi.B == 16 and zi.ORACLE_IO_RUN == (3, 2)
    for i, r in enumerate(runs):
        assert np.isfinite(r["state"]).all() and np.isfinite(r["taus"]).all() and np.isfinite(r["f"]).all() and np.isfinite(r["applied"]).all(), i
        assert not r["qp_status"].any(), (i, r["qp_status"])
        assert not np.array_equal(r["state"], plain[i]["state"]) and not np.array_equal(r["taus"][0], plain[i]["taus"][0])
        d = int(I["records"][i, 48])
        assert d == i % 3 and not r["applied"][:d].any()             # the zeroed memory's words while the first commands are on their way
        if i % 2 == 1:
            assert (np.abs(r["taus"]).max(axis=1) > zi.ORACLE_IO_LIMIT).all() and r["limited"][d:].all(), i
            if I["records"][i, 24] == 1.0:                           # without a lag the limit holds exactly
                assert np.abs(r["applied"]).max() <= zi.ORACLE_IO_LIMIT, i
        else:
            assert not r["limited"].any(), i
