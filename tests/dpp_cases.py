"""Cases and references of the DPP-layer tests (test_dpp_cases.py on the CPU, test_gpu_dpp.py on the GPU): csrc/lmh_dpp.h through the
harness tests/kernels/dpp_harness.hip, one wave and one case per block.

  exact        fma() is the correctly rounded a * b + c (exact rational arithmetic, rounded once); every broadcast-FMA chain has a
               lane-level emulator that applies it in the order the header states, wave_sum one with plain adds in the header's order.
               The GPU must match these bit for bit.
  to a bound   the register solves, against the solution in np.longdouble (solve_ref): backward error <= BWD * N * u (LDL'), forward
               error <= FWD * kappa_inf * N * u (all), u = 2^-53.  LDL' without pivoting is backward stable on an SPD matrix
               (Higham, Accuracy and Stability of Numerical Algorithms, theorem 10.3 with the growth factor 1 of the SPD case), so
               its residual is a small multiple of N u at every condition number; Gauss-Jordan without pivoting is forward stable
               only (ibid. section 14.4), its residual grows with kappa, so it is held to the forward bound alone.  The plain fp64
               restatements below (same pivot order, no lanes, no fused multiply-adds) are no expected values: the CPU test holds them
               to ONE EIGHTH of the bounds on the same tables, which shows the bounds neither vacuous nor tight on these inputs.

A lane vector is a numpy array of 64 entries; lane l belongs to the 16-lane DPP row l >> 4."""
import ctypes
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
BWD = 4.0                        # backward error of the LDL' solves <= BWD * N * u
FWD = 8.0                        # forward error of every solve <= FWD * kappa_inf * N * u
RESTATEMENT_SHARE = 0.125        # the fp64 restatements stay within this share of the bounds
SEED = 20261019
LANES = np.arange(64)

# ---------------------------------------------------------------- the harness: launcher -> per-case element counts of its buffers
F64, F32, U32, I32 = np.float64, np.float32, np.uint32, np.int32


def _ldl(n, m):
    return dict(ins=[(n * n, F64), (m * n, F64), (1, U32), (1, F64)], outs=[(m * 64, F64), (64, I32)])


def _gj(n, m):
    return dict(ins=[(n * n, F64), (4 * m * 16, F64), (1, U32)], outs=[(m * 64, F64), (64, I32)])


LAUNCHERS = {
    "dpph_lanes_f64": dict(ins=[(64, F64)], outs=[(148 * 64, F64)]),
    "dpph_lanes_f32": dict(ins=[(64, F32)], outs=[(4 * 64, F32)]),
    "dpph_fmac_one": dict(ins=[(3 * 64, F64)], outs=[(6 * 64, F64)]),
    "dpph_fmac_range": dict(ins=[(34 * 64, F64)], outs=[((16 * 32 + 15 * 16) * 64, F64)]),
    "dpph_fmac_self": dict(ins=[(17 * 64, F64)], outs=[(26 * 16 * 64, F64)]),
    "dpph_dots": dict(ins=[(18 * 64, F64)], outs=[(9 * 64, F64)]),
    "dpph_bdot6_f32": dict(ins=[(8 * 64, F32)], outs=[(64, F32)]),
    "dpph_reduce_f64": dict(ins=[(64, F64)], outs=[(2 * 64, F64)]),
    "dpph_reduce_f32": dict(ins=[(64, F32)], outs=[(64, F32)]),
    "dpph_rcp": dict(ins=[(64, F64)], outs=[(3 * 64, F64)]),
    "dpph_ldl_8_1": _ldl(8, 1), "dpph_ldl_16_1": _ldl(16, 1), "dpph_ldl_15_7": _ldl(15, 7), "dpph_ldl_6_6": _ldl(6, 6),
    "dpph_ldl_8_1_dadd": _ldl(8, 1), "dpph_ldl_18_7": _ldl(18, 7), "dpph_ldl_24_2": _ldl(24, 2),
    "dpph_ldl2": dict(ins=[(32 * 32, F64), (32, F64), (1, U32)], outs=[(2 * 64, F64), (64, I32)]),
    "dpph_gj_6_1": _gj(6, 1), "dpph_gj_6_2": _gj(6, 2), "dpph_gj_12_1": _gj(12, 1), "dpph_gj_15_2": _gj(15, 2),
    "dpph_gj_15_7": _gj(15, 7), "dpph_gj_16_1": _gj(16, 1),
    "dpph_gj16_guard": dict(ins=[(72, F64), (1, U32), (2, I32)], outs=[(4 * 64, F64), (2 * 64, I32)]),
}
# (18, 7) and (24, 2) take ldl_solve_regs' v_readlane form for 16 < N <= 32; (18, 7) is what the two-wave QP set-up instantiates
LDL_SHAPES = {"dpph_ldl_8_1": (8, 1), "dpph_ldl_16_1": (16, 1), "dpph_ldl_15_7": (15, 7), "dpph_ldl_6_6": (6, 6), "dpph_ldl_18_7": (18, 7),
              "dpph_ldl_24_2": (24, 2)}
GJ_SHAPES = {"dpph_gj_6_1": (6, 1), "dpph_gj_6_2": (6, 2), "dpph_gj_12_1": (12, 1), "dpph_gj_15_2": (15, 2), "dpph_gj_15_7": (15, 7),
             "dpph_gj_16_1": (16, 1)}


def harness():
    """The harness library, built if stale, with the launchers' argument types set: pointers..., int ncase, void *stream -> int."""
    from linearmpchumanoid_amd import build as hipbuild
    lib = ctypes.CDLL(hipbuild.build_dpp_harness())
    for name, spec in LAUNCHERS.items():
        fn = getattr(lib, name)
        fn.argtypes = [ctypes.c_void_p] * (len(spec["ins"]) + len(spec["outs"])) + [ctypes.c_int, ctypes.c_void_p]
        fn.restype = ctypes.c_int
    return lib


# ---------------------------------------------------------------- exact fused multiply-add and the lane permutations
def fma(a, b, c):
    """a * b + c rounded once (round to nearest even): the rational result is exact, float() of a Fraction is correctly rounded."""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def fma_v(a, b, c):
    return np.array([fma(x, y, z) for x, y, z in zip(a, b, c)], dtype=np.float64)


PERM = {0xB1: LANES ^ 1, 0x4E: LANES ^ 2, 0x141: (LANES & ~7) | (7 - (LANES & 7)), 0x140: (LANES & ~15) | (15 - (LANES & 15))}
CTRLS = (0xB1, 0x4E, 0x141, 0x140)


def bcast16(x, c):
    """Lane l reads lane c of its own 16-lane row."""
    return np.asarray(x)[(LANES & ~15) | c]


def emu_fmac_one(acc, src, m, j):
    return fma_v(bcast16(src, j), m, acc)


def emu_fmac_range(a, src, m, a0, b0, cnt):
    a = np.array(a, dtype=np.float64)
    for k in range(cnt):
        a[a0 + k] = fma_v(bcast16(src, b0 + k), m, a[a0 + k])
    return a


def emu_fmac_self(a, m, c0, cnt, j):
    a = np.array(a, dtype=np.float64)
    for c in range(c0, c0 + cnt):
        a[c] = fma_v(bcast16(a[c], j), m, a[c])
    return a


def emu_dot(acc, src, m, lanes):
    """acc += sum_k lane_(lanes[k])(src) m[k], in k order."""
    acc = np.array(acc, dtype=np.float64)
    for k, ln in enumerate(lanes):
        acc = fma_v(bcast16(src, ln), m[k], acc)
    return acc


def emu_dots(acc0, acc1, src, m):
    """The nine results of the harness's dot kernel, in its order."""
    ev, od = list(range(0, 12, 2)), list(range(1, 12, 2))
    return np.stack([
        emu_dot(acc0, src, m, range(6)), emu_dot(acc0, src, m, range(12)), emu_dot(acc0, src, m, range(15)),
        emu_dot(acc0, src, m, range(6)), emu_dot(acc1, src, m, range(6, 12)),
        emu_dot(acc0, src, [m[k] for k in ev], ev), emu_dot(acc1, src, [m[k] for k in od], od),
        emu_dot(acc0, src, [m[0]] * 8, range(0, 16, 2)), emu_dot(acc1, src, [m[0]] * 8, range(1, 16, 2))])


def emu_wave_sum(v):
    """Plain adds in the header's order: lane ^ 1, lane ^ 2, row_half_mirror, row_mirror, then (r0 + r16) + (r32 + r48).  Works in the
    dtype of v (float64 or float32)."""
    v = np.array(v)
    for ctrl in CTRLS:
        v = v + v[PERM[ctrl]]
    return np.full(64, (v[0] + v[16]) + (v[32] + v[48]), dtype=v.dtype)


def emu_wave_max(v):
    return np.full(64, np.fmax.reduce(np.asarray(v)))


SELF_CNT = (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16)          # dpp_fmac_self<0, CNT, (5 CNT) & 15> of the harness


def lane_tags():
    """64 distinct doubles whose high and low words both differ per lane (normal, finite)."""
    l = LANES.astype(np.uint64)
    hi = np.uint64(0x3FF00000) + np.uint64(0x1111) * (l + np.uint64(1))
    lo = (np.uint64(0x9E3779B9) * (l + np.uint64(1))) & np.uint64(0xFFFFFFFF)
    return ((hi << np.uint64(32)) | lo).view(np.float64)


def lane_tags_f32():
    """64 distinct floats in [1, 2)."""
    return (np.uint32(0x3F800000) + np.uint32(0x012345) * (LANES.astype(np.uint32) + np.uint32(1))).view(np.float32)


def full_mantissa(rng, shape):
    """Full-mantissa doubles of mixed sign and magnitude 2^-20 .. 2^20, all different."""
    return rng.standard_normal(shape) * np.exp2(rng.uniform(-20.0, 20.0, shape))


def exact_inputs(rng, shape):
    """Small integers times powers of two: every product and every partial sum of a chain of <= 16 terms is exact in fp64."""
    return rng.integers(-64, 65, shape).astype(np.float64) * np.exp2(rng.integers(-4, 5, shape).astype(np.float64))


def f32_exact_inputs(rng):
    """bdot6 (float): acc, src, m[0..5] of <= 8 significant bits on one binary scale each, so every product and partial sum is exact in
    fp32 (products: multiples of 1/2 below 2^15; seven terms stay below 2^18 halves)."""
    x = rng.integers(-255, 256, (8, 64)).astype(np.float64)
    x[0] *= 0.5
    x[1] *= 0.125
    x[2:] *= 4.0
    return x.astype(np.float32)


def rcp_inputs(rng, ncase):
    """d = +-m 2^e, m in [1, 2), e in [-500, 500]; the exact powers of two and the ends of the range included."""
    d = np.ldexp(rng.uniform(1.0, 2.0, (ncase, 64)), rng.integers(-500, 501, (ncase, 64))) * rng.choice([-1.0, 1.0], (ncase, 64))
    d[0, :8] = [1.0, -1.0, 2.0 ** -500, 2.0 ** 500, np.nextafter(2.0, 1.0), -np.nextafter(2.0, 1.0) * 2.0 ** 499, 3.0, 1.0 + 2.0 ** -52]
    return d


def ulp_error(y, d):
    """|y - 1 / d| in units of the last place of the correctly rounded fp64 quotient, the quotient formed in longdouble."""
    q = np.longdouble(1.0) / np.asarray(d, dtype=np.longdouble)
    ulp = np.spacing(np.abs(q.astype(np.float64))).astype(np.longdouble)
    return np.abs(np.asarray(y, dtype=np.longdouble) - q) / ulp


# ---------------------------------------------------------------- solve cases
LDL_CONDS = (1.0, 1e4, 1e8, 1e11, 1e13)
GJ_CONDS = (1.0, 1e2, 1e4, 1e6)


def spd(rng, n, cond):
    """Q diag(s) Q', symmetrised, s log-spaced from 1 down to 1 / cond."""
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    s = np.logspace(0.0, -np.log10(cond), n) if n > 1 else np.ones(1)
    a = (q * s) @ q.T
    return 0.5 * (a + a.T)


def mixed_rhs(rng, shape):
    return rng.standard_normal(shape) * 10.0 ** rng.uniform(-6.0, 6.0, shape)


def prefix(n):
    return (1 << n) - 1


def nonprefix_masks(N):
    """Three masks with holes, allowed by the header's contract (rows and columns outside the mask are zero); for N = 32 each has bits
    on both sides of the seam at 16."""
    rng = np.random.default_rng([SEED, N, 77])
    out = []
    while len(out) < 3:
        bits = rng.random(N) < 0.6
        m = int(sum(1 << i for i in range(N) if bits[i]))
        ok = m != prefix(bin(m).count("1")) and bin(m).count("1") >= 2 and m not in out
        if N == 32:
            ok = ok and (m & 0xFFFF) and (m >> 16)
        if ok:
            out.append(m)
    return out


def embed(N, mask, sub, rhs):
    """The |mask| x |mask| system on the rows / columns of `mask` inside an N x N one, zeros outside.  rhs: [M, |mask|] -> [M, N]."""
    idx = [i for i in range(N) if (mask >> i) & 1]
    A = np.zeros((N, N))
    A[np.ix_(idx, idx)] = sub
    B = np.zeros((rhs.shape[0], N))
    B[:, idx] = rhs
    return A, B


def solve_table(N, M, conds, tag, extra_sizes=()):
    """Seeded cases of one instantiation: every prefix mask n = 1 .. N (the condition numbers in rotation), the full size and
    `extra_sizes` at every condition number, three non-prefix masks.  -> list of dict(A [N,N], B [M,N], live, cond)."""
    rng = np.random.default_rng([SEED, N, M, tag])
    plan = [(prefix(n), conds[n % len(conds)]) for n in range(1, N + 1)]
    plan += [(prefix(n), c) for n in (N,) + tuple(extra_sizes) for c in conds]
    plan += [(m, conds[(i + 1) % len(conds)]) for i, m in enumerate(nonprefix_masks(N))]
    cases = []
    for mask, cond in plan:
        n = bin(mask).count("1")
        A, B = embed(N, mask, spd(rng, n, cond), mixed_rhs(rng, (M, n)))
        cases.append(dict(A=A, B=B, live=mask, cond=cond))
    return cases


def ldl_table(N, M):
    return solve_table(N, M, LDL_CONDS, 1)


def ldl2_table():
    return solve_table(32, 1, LDL_CONDS, 2, extra_sizes=(17, 24))


def gj_table(N, M):
    return solve_table(N, M, GJ_CONDS, 3)


DADDS = (1e-9, 1e-3, 0.5)


def ldl_dadd_table():
    """(8, 1) with a constant on the diagonal: the system solved is A + dadd I on the live rows."""
    cases = solve_table(8, 1, LDL_CONDS, 4)
    for i, c in enumerate(cases):
        c["dadd"] = DADDS[i % len(DADDS)]
    return cases


def live_idx(case):
    N = case["A"].shape[0]
    return [i for i in range(N) if (case["live"] >> i) & 1]


def live_system(case):
    """The system on the live rows: A_FF (+ dadd I), B_F [n, M]."""
    idx = live_idx(case)
    A = case["A"][np.ix_(idx, idx)] + case.get("dadd", 0.0) * np.eye(len(idx))
    return A, case["B"][:, idx].T.copy()


def solve_ref(A, B):
    """x* in np.longdouble: an fp64 solve, then iterative refinement with longdouble residuals until it stops moving."""
    Al, Bl = A.astype(np.longdouble), B.astype(np.longdouble)
    x = np.linalg.solve(A, B).astype(np.longdouble)
    for _ in range(100):
        r = Bl - Al @ x
        dx = np.linalg.solve(A, r.astype(np.float64)).astype(np.longdouble)
        x = x + dx
        if np.all(np.abs(dx) <= np.longdouble(2.0) ** -62 * np.abs(x).max(axis=0)):
            break
    return x


def reference(case):
    """(x* [n, M] longdouble, kappa_inf) of the live system, cached on the case."""
    if "_ref" not in case:
        A, B = live_system(case)
        case["_ref"] = (solve_ref(A, B), float(np.linalg.cond(A, np.inf)))
    return case["_ref"]


def errors(case, x):
    """x [n, M] (fp64) on the live rows -> (backward error / (N u), forward error / (kappa_inf N u)), the worst column of each; N is the
    size of the instantiation.  Residual and differences in longdouble."""
    A, B = live_system(case)
    N = case["A"].shape[0]
    xs, kappa = reference(case)
    Al, Bl, xl = A.astype(np.longdouble), B.astype(np.longdouble), np.asarray(x, dtype=np.float64).astype(np.longdouble)
    if not np.all(np.isfinite(xl)):
        return np.inf, np.inf
    res = np.abs(Al @ xl - Bl).max(axis=0)
    normA = np.abs(Al).sum(axis=1).max()
    bwd = res / (normA * np.abs(xl).max(axis=0) + np.abs(Bl).max(axis=0))
    fwd = np.abs(xl - xs).max(axis=0) / np.abs(xs).max(axis=0)
    return float(bwd.max() / (N * U)), float(fwd.max() / (kappa * N * U))


# ---------------------------------------------------------------- plain fp64 restatements (same pivot order, no lanes, no fma)
def ldl_restatement(A, B, live, dadd=0.0):
    """LDL' without pivoting over the live pivots in ascending order, forward substitution, D^-1, backward substitution.
    A [N,N], B [M,N] -> (x [M,N], zero on rows that are not live; bad)."""
    N = A.shape[0]
    a, b = np.tril(A).copy(), B.T.copy()
    inv = np.zeros(N)
    bad = 0
    piv = [j for j in range(N) if (live >> j) & 1]
    with np.errstate(divide="ignore", invalid="ignore"):          # (a zero or NaN pivot of the return-value cases)
        for j in piv:
            d = a[j, j] + dadd
            bad |= int(not d > 0.0)
            inv[j] = 1.0 / d
            f = a[:, j] * inv[j]
            for c in range(j + 1, N):
                a[c:, c] -= f[c:] * a[c, j]
            b[j + 1:] -= np.outer(f[j + 1:], b[j])
            a[j + 1:, j] = f[j + 1:]
        b *= inv[:, None]
        for j in reversed(piv):
            b[:j] -= np.outer(a[j, :j], b[j])
    return b.T, bad


def gj_restatement(A, B, live, on=True, dmin=None):
    """Gauss-Jordan without pivoting, multipliers through the reciprocal of the pivot.  dmin given: the guarded form (a pivot that is
    not above dmin -- every pivot when `on` is false -- is replaced by 1; reported only when `on`).  -> (x [M,N], bad)."""
    N = A.shape[0]
    a, b = A.copy(), B.T.copy()
    inv = np.zeros(N)
    bad = 0
    with np.errstate(divide="ignore", invalid="ignore"):
        for j in [j for j in range(N) if (live >> j) & 1]:
            d = a[j, j]
            if dmin is not None:
                bad |= int(on and not d > dmin)
                d = d if (on and d > dmin) else 1.0
            inv[j] = 1.0 / d
            nf = -(a[:, j] * inv[j])
            nf[j] = 0.0
            a[:, j + 1:] += np.outer(nf, a[j, j + 1:])
            b += np.outer(nf, b[j])
        if dmin is None:
            bad = int(any(not (inv[j] > 0.0 and inv[j] <= np.finfo(np.float64).max) for j in range(N) if (live >> j) & 1))
        return (b * inv[:, None]).T, bad


# ---------------------------------------------------------------- return-value cases
def indefinite(rng, n, j, dj=-1.0):
    """L D L' with unit lower-triangular L and positive D except D_j = dj: the elimination without pivoting meets pivot j = dj (to
    rounding) after j positive ones."""
    Lm = np.tril(rng.uniform(-0.5, 0.5, (n, n)), -1) + np.eye(n)
    D = rng.uniform(0.5, 2.0, n)
    D[j] = dj
    a = (Lm * D) @ Lm.T
    return 0.5 * (a + a.T)


def bad_pivot_cases(N, M, nF, pivots, tag):
    """For one instantiation and free-set size nF: an SPD case | pivot j non-positive for each j of `pivots` | a zero live diagonal at
    row 0 | a NaN on the diagonal of row nF // 2 | the SPD case again.  -> (cases, expect), expect[i] = the case must return non-zero."""
    rng = np.random.default_rng([SEED, N, M, nF, tag])
    good_sub, good_rhs = spd(rng, nF, 1e2), mixed_rhs(rng, (M, nF))
    mk = lambda sub: dict(zip(("A", "B"), embed(N, prefix(nF), sub, good_rhs)), live=prefix(nF), cond=1e2)
    cases, expect = [mk(good_sub)], [False]
    for j in pivots:
        cases.append(mk(indefinite(rng, nF, j))); expect.append(True)
    z = good_sub.copy(); z[0, 0] = 0.0
    cases.append(mk(z)); expect.append(True)
    z = good_sub.copy(); z[nF // 2, nF // 2] = np.nan
    cases.append(mk(z)); expect.append(True)
    cases.append(mk(good_sub)); expect.append(False)
    return cases, expect


def guard_cases():
    """Guarded gj16_step as kinv_compute uses it.  Each case: K [2,6,6] (SPD 6 x 6, entries O(1e-3 .. 10)), use (bit f = system f on),
    dd [2] (pinned row / column, -1 = none), rank5 = the system made rank 5 (or None)."""
    rng = np.random.default_rng([SEED, 6, 5])
    cases = []
    for use, rank5, dd in ((3, None, (-1, -1)), (1, None, (-1, -1)), (2, None, (-1, -1)), (3, 0, (-1, -1)), (3, 1, (-1, -1)),
                           (3, None, (2, -1)), (3, None, (-1, 4)), (0, None, (-1, -1))):
        K = np.stack([spd(rng, 6, c) * s for c, s in ((1e2, 3.0), (1e4, 0.5))])
        if rank5 is not None:
            g = rng.standard_normal((6, 5))
            K[rank5] = g @ g.T
        cases.append(dict(K=K, use=use, dd=np.array(dd, dtype=np.int32), rank5=rank5))
    return cases


def pinned(K, dd):
    """K with row / column dd replaced by the unit row / column (dd < 0: K)."""
    K = K.copy()
    if dd >= 0:
        K[dd, :] = 0.0; K[:, dd] = 0.0; K[dd, dd] = 1.0
    return K
