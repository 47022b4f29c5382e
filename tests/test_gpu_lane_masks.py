"""LANE_IS (csrc/lmh_device.h): predicates of the lane id alone as compile-time lane masks.

Two things are held here.  (1) The mask form and the run-time form of a predicate agree lane by lane, and agree with numpy: a harness kernel
of its own (tests/kernels/lane_mask_harness.hip) evaluates sixteen predicates taken from lmh_kernels.hip both ways on two waves.  (2) The
shipped library and the checker build `lanert` (-DLMH_LANE_RUNTIME: every LANE_IS evaluated at run time on the kernel's lane id, the form
the masks replaced) compute the same BYTES -- state, out, status and the tau | f log -- on the walking, balance and jump workloads as
bench.py sets them up and on the other entry points that share the device functions (lmh_eval in double and single support,
lmh_rollout_zoh, lmh_plant_step).  Arithmetic is untouched by the masks, so equality is `==` on the byte images; no hard status flag may
appear in either library, or equality would say nothing.  One child process per library runs every case once (a process that has loaded
one build cannot run another); the cases share its arrays."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import run_probe

pytestmark = pytest.mark.gpu

HARD_FLAGS = 1 | 2 | 4 | 8 | 32      # bench.py's: QP_MAXITER | NONFINITE | ZMP_RANGE | NOT_SPD | UNFINISHED (16, the fp64-route note, is informational)


# ------------------------------------------------------------------------------- (1) both forms of a predicate, lane by lane
def _lane_maps(lane):
    ln = np.minimum(lane, 62)
    fr = (ln * 57) >> 9
    e9 = ln - 9 * fr
    col = e9 - 3 * ((e9 * 11) >> 5)
    fr3 = (ln * 43) >> 7
    l60 = np.where(lane < 60, lane, lane - 60)
    lfr = (l60 * 43) >> 9
    lel = l60 - 12 * lfr
    dup = np.array([(0x5210543210543210 >> (4 * int(l & 15))) & 15 for l in lane])
    return dict(ln=ln, fr=fr, e9=e9, col=col, fr3=fr3, l60=l60, lfr=lfr, lel=lel, dup=dup)


def _numpy_predicates(lane):
    """The list LANE_PREDICATES of the harness, in numpy.  The division-by-multiplication maps are also held to the plain quotients."""
    m = _lane_maps(lane)
    assert np.array_equal(m["fr"], m["ln"] // 9) and np.array_equal(m["col"], (m["ln"] % 9) % 3) and np.array_equal(m["fr3"], m["ln"] // 3)
    assert np.array_equal(m["lfr"], m["l60"] // 12) and np.array_equal(m["lel"], m["l60"] % 12)
    return [lane < 30,
            (lane >= 30) & (lane < 36),
            (lane & 15) < 6,
            (lane & 15) == 3,
            (lane >> 4) < 2,
            ((lane >> 4) == 2) & ((lane & 3) == 2),
            m["col"] == 1,
            m["fr"] < 3,
            m["fr3"] < 14,
            (m["lel"] == 0) | (m["lel"] == 5) | (m["lel"] == 9),
            m["lfr"] < 2,
            m["dup"] == 2,
            (lane < 48) & ((lane & 15) == 2 * (lane >> 4)),
            (lane == 0) | (lane >= 30),
            lane < 0,
            lane < 64]


def test_mask_form_and_run_time_form_agree_lane_by_lane():
    from linearmpchumanoid_amd import build as hipbuild
    lib = C.CDLL(hipbuild.build_lane_mask_harness())
    lib.lane_mask_harness_run.argtypes = [C.c_void_p, C.c_void_p]
    lib.lane_mask_harness_run.restype = C.c_int
    npred = lib.lane_mask_harness_npred()
    lane = np.arange(128) & 63
    want = _numpy_predicates(lane)
    assert npred == len(want) == 16
    out = torch.full((2 * npred, 128), -1, dtype=torch.int32, device="cuda:0")
    assert lib.lane_mask_harness_run(out.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for p in range(npred):
        ref = want[p].astype(np.int32)
        assert np.array_equal(got[2 * p], got[2 * p + 1]), (p, "mask form != run-time form", np.nonzero(got[2 * p] != got[2 * p + 1])[0][:8])
        assert np.array_equal(got[2 * p], ref), (p, "mask form != numpy", np.nonzero(got[2 * p] != ref)[0][:8])
    assert not want[14].any() and want[15].all()                   # the empty and the full mask are among them


# ------------------------------------------------------------------------------- (2) the shipped library and `lanert`: the same bytes
_PROBE = r"""
import json, os, sys
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np, torch
import bench
from linearmpchumanoid_amd import capi
from linearmpchumanoid_amd.controller import BatchedController, default_config, ik_start_posture

arrays, flags = {}, {}

def keep(case, **named):
    for k, a in named.items():
        arrays[case + "." + k] = a.detach().cpu().numpy().copy()

def bench_rollout(case, config, B, ticks):
    # the workload of `bench.py --config C` on B robots, one launch of `ticks` ticks (250-tick chunks: 1300 ticks cross five boundaries)
    args = bench.parse(["--config", str(config), "--instances", str(B), "--ticks", str(ticks)])
    cfg = default_config(dt=args.dt, time_horizon=args.horizon * args.mpc_dt + 1e-9, z_com=0.26, mpc_dt=args.mpc_dt, warm_start=1, precision=0)
    ctl = BatchedController(B, cfg, device=0)
    state, _ = bench.build_workload(args, ctl, 0, B, ticks)
    out, status, log = ctl.rollout(state, ticks, log=True)
    torch.cuda.synchronize(); ctl.synchronize()
    keep(case, state=state, out=out, status=status, log=log)
    flags[case] = int(np.bitwise_or.reduce(status.cpu().numpy()[:, 2]))

bench_rollout("walk", 3, 16, 1300)
bench_rollout("balance", 2, 8, 300)
bench_rollout("jump", 5, 8, 700)

# the other entry points: dt = 1 ms, N = 16 (BASELINE config 2's constants), 8 robots
B, DT, TH = 8, 1e-3, 0.016
q0, zcom = ik_start_posture(0)
v = 0.3 * bench.perturbed_velocities(0, B, seed=31)
n = 2500
for case, ph in (("eval_double", 0), ("eval_single", 1)):
    ctl = BatchedController(B, default_config(dt=DT, time_horizon=TH, z_com=zcom, warm_start=0), device=0)
    ctl.set_refs(np.zeros(n), np.zeros(n), np.full(n, ph, dtype=np.uint8))
    st = ctl.new_state(q0, v, t=0.0)
    out, status = ctl.stand_step(st)
    torch.cuda.synchronize()
    keep(case, state=st, out=out, status=status)
    flags[case] = int(np.bitwise_or.reduce(status.cpu().numpy()[:, 2]))

q = np.tile(q0, (B, 1)); q[:, 2] -= 5.0e-4                        # every sole vertex half a millimetre in the ground
vz = 0.2 * bench.perturbed_velocities(0, B, seed=20261022)
ctl = BatchedController(B, default_config(dt=DT, time_horizon=TH, z_com=zcom, warm_start=1), device=0)
ctl.set_refs_stance(2.0, 2)
st = ctl.new_state(q, vz, t=0.0, v_prev=vz)
out, status, log = ctl.rollout_zoh(st, 20, 2, log=True)
torch.cuda.synchronize()
keep("zoh", state=st, out=out, status=status, log=log)
flags["zoh"] = int(np.bitwise_or.reduce(status.cpu().numpy()[:, 2]))

ctl = BatchedController(B, default_config(dt=DT, time_horizon=TH, z_com=zcom, warm_start=0), device=0)
ctl.set_refs_stance(2.0, 2)
st = ctl.new_state(q, vz, t=0.0)
zero6 = torch.zeros((B, 6), dtype=torch.float64, device=ctl.device)
pf_all = torch.zeros((B,), dtype=torch.int32, device=ctl.device)
cf_all = torch.zeros((B,), dtype=torch.int32, device=ctl.device)
for _ in range(20):
    out, status = ctl.stand_step(st)
    st, pf = ctl.plant_step(st, torch.cat([zero6, out[:, 0:24]], dim=1).contiguous(), 1)
    pf_all |= pf; cf_all |= status[:, 2]
torch.cuda.synchronize()
keep("plant_step", state=st, out=out, status=status, plant_flags=pf_all)
flags["plant_step"] = int(np.bitwise_or.reduce((pf_all | cf_all).cpu().numpy()))

np.savez(sys.argv[1], **arrays)
print(json.dumps({"build_flags": capi.lib().lmh_debug_build_flags(), "flags": flags}))
"""
CASES = ("walk", "balance", "jump", "eval_double", "eval_single", "zoh", "plant_step")


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    """-> {variant: (the child's JSON line, its arrays)} for the shipped library ("") and `lanert`."""
    from linearmpchumanoid_amd import build as hipbuild
    hipbuild.build_variant("lanert")
    d = tmp_path_factory.mktemp("lane_masks")
    res = {}
    for variant in ("", "lanert"):
        path = str(d / ("arrays_%s.npz" % (variant or "shipped")))
        line = run_probe(_PROBE, variant, timeout=900, args=(path,))
        with np.load(path) as z:
            res[variant] = (line, {k: z[k] for k in z.files})
    return res


def test_the_two_libraries_are_the_two_builds(both):
    """lmh_debug_build_flags bit 6 = built with -DLMH_LANE_RUNTIME: a `lanert` library built without its flag cannot pass."""
    assert both[""][0]["build_flags"] & 64 == 0
    assert both["lanert"][0]["build_flags"] & 64 == 64


@pytest.mark.parametrize("case", CASES)
def test_no_hard_flag_in_either_library(both, case):
    for variant in ("", "lanert"):
        f = both[variant][0]["flags"][case]
        assert f & HARD_FLAGS == 0, (variant or "shipped", case, f)


@pytest.mark.parametrize("case", CASES)
def test_shipped_and_lanert_give_the_same_bytes(both, case):
    a, b = both[""][1], both["lanert"][1]
    names = sorted(k for k in a if k.startswith(case + "."))
    assert names and names == sorted(k for k in b if k.startswith(case + ".")), names
    assert any(k.endswith(".state") for k in names) and any(k.endswith(".out") for k in names) and any(k.endswith(".status") for k in names)
    if case in ("walk", "balance", "jump", "zoh"):
        assert case + ".log" in names
    for k in names:
        x, y = a[k], b[k]
        assert x.shape == y.shape and x.dtype == y.dtype, k
        assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes(), (k, "elements that differ", int((x != y).sum()))
    out = a[case + ".out"]
    assert np.isfinite(out[:, :36]).all() and np.abs(out[:, :24]).max() > 0.0      # the case computed torques: not two empty buffers
