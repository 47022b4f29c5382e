"""CPU side of lmh_rollout_zoh_ex: the host statement of where a robot's pushes fall in a launch (trajectories.zoh_hold_pieces) against a
walk one substep at a time, the oracle statement of the loop the GPU parity test rests on, and the binding.  No GPU is used."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import plant_step_cases as pc
import zoh_cases as zc
import zoh_ex_cases as zx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_bound_and_exported(hip_lib):
    from linearmpchumanoid_amd import capi
    from linearmpchumanoid_amd.controller import BatchedController
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lmh.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+lmh_rollout_zoh_ex\s*\(", src) and "lmh_rollout_zoh_ex" in capi.EXPORTS and hasattr(hip_lib, "lmh_rollout_zoh_ex")
    assert len(capi.PROTOTYPES["lmh_rollout_zoh_ex"][1]) == 8 and callable(BatchedController.rollout_zoh_ex)
    # the record: five pointers, four int32, in the header's order
    body = re.search(r"typedef struct lmh_zoh_opts \{(.*?)\} lmh_zoh_opts;", src, flags=re.S).group(1)
    names = re.findall(r"(\w+)\s*;", body)
    assert names == [n for n, _ in capi.LmhZohOpts._fields_] and C.sizeof(capi.LmhZohOpts) == 5 * 8 + 4 * 4
    assert [t for _, t in capi.LmhZohOpts._fields_] == [C.c_void_p] * 5 + [C.c_int32] * 4


def test_without_a_handle_the_call_is_refused(hip_lib):
    from linearmpchumanoid_amd import capi
    opts = capi.LmhZohOpts(pushes=1, trace_every=3)
    for o in (None, C.byref(opts)):
        assert hip_lib.lmh_rollout_zoh_ex(None, None, None, None, o, 3, 2, None) == -2 and hip_lib.lmh_last_error() == b"null handle"


@pytest.mark.parametrize("case", zx.PIECE_CASES, ids=[c[0] for c in zx.PIECE_CASES])
def test_hold_pieces_against_the_walk_one_substep_at_a_time(case):
    from linearmpchumanoid_amd.trajectories import zoh_hold_pieces
    _, ticks, n0, n_ticks, n_substeps = case
    pieces = zoh_hold_pieces(ticks, n0, n_ticks, n_substeps)
    assert len(pieces) == n_ticks
    for start, hold in pieces:
        assert sum(s for s, _ in hold) == n_substeps and all(s > 0 for s, _ in hold)
        assert all(rec is not None for _, rec in hold[:-1]) and hold[-1][1] is None      # a push ends a piece, never a hold
    assert zx.flatten_pieces(pieces) == zx.brute_events(ticks, n0, n_ticks, n_substeps)


def test_hold_pieces_name_the_cases():
    """What the list above is there for, written out: which records are applied, and where."""
    from linearmpchumanoid_amd.trajectories import zoh_hold_pieces
    P = {c[0]: zoh_hold_pieces(*c[1:]) for c in zx.PIECE_CASES}
    applied = lambda p: sorted([s for s, _ in p if s is not None] + [r for _, h in p for _, r in h if r is not None])
    assert P["a push at substep 0"][0] == (0, [(3, None)])
    assert P["a push on a control-tick boundary"][2] == (0, [(3, None)]) and P["a push on a control-tick boundary"][1] == (None, [(3, None)])
    assert P["a push just behind a boundary"][2] == (None, [(1, 0), (2, None)])
    assert P["two pushes in one hold"][1] == (None, [(1, 0), (1, 1), (1, None)])
    assert P["a push at the last substep"][5] == (None, [(2, 0), (1, None)])
    assert applied(P["a push at the launch's end substep (absent)"]) == []
    assert applied(P["a push in the past with n0 > 0 (absent)"]) == [1]
    assert applied(P["trailing -1 records"]) == [0, 1]
    assert [s for s, _ in P["n_substeps = 1"]] == [0, 1, None, 2, None, 3] and all(h == [(1, None)] for _, h in P["n_substeps = 1"])
    assert applied(P["boundary, inside and end together from a later clock"]) == [0, 1, 2, 3] and applied(P["no push at all"]) == []
    # the launch that follows applies the push the first one ended on, before its first evaluation
    assert zoh_hold_pieces([18], 18, 1, 3)[0] == (0, [(3, None)])
    with pytest.raises(ValueError):
        zoh_hold_pieces([2], 0, 3, 0)
    assert zoh_hold_pieces([-1], 0, 2, 0) == [(None, []), (None, [])] and zoh_hold_pieces([2], 0, 0, 0) == []


def test_oracle_loop_is_the_zoh_loop_with_pushes_in_their_places():
    S = pc.contact_states()
    i = 3
    x0 = np.concatenate([S["q"][i], S["v"][i]])
    bw = np.array([0.1, -0.2, 0.05, 1.0, -0.5, 2.0])
    # without pushes and with a constant wrench: oracle_zoh's numbers exactly (as a [6] wrench and as three copies of it)
    ref = zc.oracle_zoh(pc.make_oracle(), x0, 3, 2, base_wrench=bw)
    for w in (bw, np.tile(bw, (3, 1))):
        r = zx.oracle_zoh_ex(pc.make_oracle(), x0, 3, 2, base_wrench=w)
        for k in ("state", "v_prev", "tau", "f", "qpp", "taus", "k"):
            assert np.array_equal(r[k], ref[k]), k
        assert r["t"] == ref["t"]
    # a wrench sequence is not its first record
    seq = np.tile(bw, (3, 1)); seq[1] *= -1.0
    assert not np.array_equal(zx.oracle_zoh_ex(pc.make_oracle(), x0, 3, 2, base_wrench=seq)["state"], ref["state"])
    # a push inside the second hold (substep 3) against the same push at the next boundary (substep 4) and against none
    dv = zx.push_dv(11, 1)
    inside = zx.oracle_zoh_ex(pc.make_oracle(), x0, 3, 2, base_wrench=bw, ticks=[3], dv=dv)
    at_boundary = zx.oracle_zoh_ex(pc.make_oracle(), x0, 3, 2, base_wrench=bw, ticks=[4], dv=dv)
    assert not np.array_equal(inside["state"], at_boundary["state"]) and not np.array_equal(inside["state"], ref["state"])
    assert np.array_equal(inside["taus"][:2], ref["taus"][:2]) and not np.array_equal(inside["taus"][2], ref["taus"][2])
    # the boundary push is seen by the third evaluation, whose v_prev <- v then holds the pushed velocity; written out by hand
    o = pc.make_oracle()
    a = zc.oracle_zoh(o, x0, 2, 2, base_wrench=bw)
    xa = a["state"].copy(); xa[30:] += dv[0]
    b = zc.oracle_zoh(o, xa, 1, 2, base_wrench=bw, t0=a["t"], v_prev=a["v_prev"])
    assert np.array_equal(b["state"], at_boundary["state"]) and np.array_equal(at_boundary["v_prev"], xa[30:])
    # a push on the launch's end substep is the next launch's: (2) then (1) is (3)
    o = pc.make_oracle()
    first = zx.oracle_zoh_ex(o, x0, 2, 2, base_wrench=bw, ticks=[4], dv=dv)
    assert np.array_equal(first["state"], a["state"])
    second = zx.oracle_zoh_ex(o, first["state"], 1, 2, base_wrench=bw, ticks=[4], dv=dv, t0=first["t"], v_prev=first["v_prev"])
    assert np.array_equal(second["state"], at_boundary["state"])


def test_the_compared_run_is_a_usable_reference():
    """The run test_gpu_zoh_ex.py holds against the oracle: finite, the QP solved at every evaluation (no counted flag can come from the
    definition itself), and the push and the wrench sequence both matter."""
    runs, plain = zx.oracle_ex_run(), zc.oracle_run()
    assert len(runs) == zx.B == 16 and zx.ORACLE_EX_RUN == (3, 2) and zx.ORACLE_EX_TICK == 3
    for i, r in enumerate(runs):
        assert np.isfinite(r["state"]).all() and np.isfinite(r["taus"]).all() and np.isfinite(r["f"]).all(), i
        assert not r["qp_status"].any(), (i, r["qp_status"])
        assert not np.array_equal(r["state"], plain[i]["state"]) and not np.array_equal(r["taus"][1], plain[i]["taus"][1])
