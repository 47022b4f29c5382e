// lmh_mpc_qp.h -- the maths of the box-constrained LIPM preview step, one copy for the two places that run it: lmh_mpc_qp_kernel (lmh_mpc.hip:
// one 64-thread workgroup per robot) and the helper wave of lmh_rollout_zoh_box_kernel (lmh_kernels.hip: one wave of a 128-thread workgroup,
// inside the evaluation's reference chain).  lmh_mpc.hip has the derivation and the LDS layout; this file holds the statements.
//   WV      how the 64 lanes that run a function meet: false = the workgroup barrier (they are the whole workgroup), true = the wave-scope
//           fence WSYNC() (they are one wave of a larger workgroup, which must not pass a workgroup barrier on its own).
//   strides the row strides of the two tiles are parameters: ld >= n for the tile T, ldb >= n + 1 for the packed L | G tile, both odd (a column
//           sweep then falls on distinct banks).  lmh_mpc_qp_kernel passes its constants; the fused loop sizes them by the handle's horizon.
//           No result depends on a stride.
// The includer defines WSYNC() and includes include/lmh.h first.  Every sum of two products is written as the fma it becomes, and every
// `s += a * b` contracts to one fma whatever surrounds it, so the two places agree bit for bit.
#pragma once

// a * b + c with the product and the sum rounded separately (numpy's c + a * b): the product goes through an opaque register, which the
// contraction of the build's default (fused multiply-add) cannot see through
__device__ __forceinline__ double mul_then_add(double a, double b, double c)
{
    double p = a * b;
    asm volatile("" : "+v"(p));
    return c + p;
}

__device__ __forceinline__ bool finite_f64(double v) { return fabs(v) <= 1.7976931348623157e308; }      // false for NaN and Inf

__device__ __forceinline__ int mpc_clamp(int kk, int ns) { return (kk < 0) ? 0 : (kk >= ns ? ns - 1 : kk); }

struct MpcSample {
    double xp, xv, ux, yp, yv, uy, zmx, zmy;
    int k, flags;
};

// the LIPM literals of the parameter block: x_next = A x + B u
struct LipAB {
    double a00, a01, a10, a11, b0, b1;
};

// one sample record (LMH_MPC_STRIDE words, pads zero), word `lane` by lane `lane`
__device__ __forceinline__ void mpc_store_sample(double *rec, int lane, const MpcSample &S, double cxp, double vxp, double cyp, double vyp, double t)
{
    if (lane < LMH_MPC_STRIDE) {
        double w = 0.0;
        w = (lane == LMH_MPC_OFF_XREF) ? S.xp : w; w = (lane == LMH_MPC_OFF_XREF + 1) ? S.xv : w; w = (lane == LMH_MPC_OFF_XREF + 2) ? S.ux : w;
        w = (lane == LMH_MPC_OFF_YREF) ? S.yp : w; w = (lane == LMH_MPC_OFF_YREF + 1) ? S.yv : w; w = (lane == LMH_MPC_OFF_YREF + 2) ? S.uy : w;
        w = (lane == LMH_MPC_OFF_ZMP) ? S.zmx : w; w = (lane == LMH_MPC_OFF_ZMP + 1) ? S.zmy : w;
        w = (lane == LMH_MPC_OFF_STATE) ? cxp : w; w = (lane == LMH_MPC_OFF_STATE + 1) ? vxp : w;
        w = (lane == LMH_MPC_OFF_STATE + 2) ? cyp : w; w = (lane == LMH_MPC_OFF_STATE + 3) ? vyp : w;
        w = (lane == LMH_MPC_OFF_T) ? t : w; w = (lane == LMH_MPC_OFF_K) ? (double)S.k : w; w = (lane == LMH_MPC_OFF_FLAGS) ? (double)S.flags : w;
        rec[lane] = w;
    }
}

template <bool WV>
__device__ __forceinline__ void qp_sync()
{
    if constexpr (WV) WSYNC();
    else __syncthreads();
}

// A = L L' in place on the leading n x n lower triangle, right-looking; every lane sees the same pivot.  false: a pivot was not positive.
template <bool WV>
__device__ __forceinline__ bool pv_factor(double *A, const int ld, int n, int lane)
{
    for (int j = 0; j < n; j++) {
        qp_sync<WV>();
        const double d = A[ld * j + j];
        if (!(d > 0.0)) return false;
        const double r = sqrt(d);
        qp_sync<WV>();
        for (int i = lane; i < n; i += 64) {
            if (i == j) A[ld * i + j] = r;
            if (i > j) A[ld * i + j] = A[ld * i + j] / r;
        }
        qp_sync<WV>();
        for (int i = lane; i < n; i += 64)
            if (i > j) {
                const double lij = A[ld * i + j];
                for (int c = j + 1; c <= i; c++) A[ld * i + c] -= lij * A[ld * c + j];
            }
    }
    return true;
}

// b <- (L L')^-1 b for one (bx) or two (bx, by) right-hand sides
template <bool TWO, bool WV>
__device__ __forceinline__ void pv_solve(const double *A, const int ld, int n, int lane, double *bx, double *by)
{
    for (int j = 0; j < n; j++) {                                  // L w = b
        qp_sync<WV>();
        const double ljj = A[ld * j + j];
        const double wx = bx[j] / ljj, wy = TWO ? by[j] / ljj : 0.0;
        qp_sync<WV>();
        for (int i = lane; i < n; i += 64) {
            if (i == j) { bx[i] = wx; if (TWO) by[i] = wy; }
            if (i > j) { const double lij = A[ld * i + j]; bx[i] -= lij * wx; if (TWO) by[i] -= lij * wy; }
        }
    }
    for (int j = n - 1; j >= 0; j--) {                             // L' v = w
        qp_sync<WV>();
        const double ljj = A[ld * j + j];
        const double vx = bx[j] / ljj, vy = TWO ? by[j] / ljj : 0.0;
        qp_sync<WV>();
        for (int i = lane; i < n; i += 64) {
            if (i == j) { bx[i] = vx; if (TWO) by[i] = vy; }
            if (i < j) { const double lji = A[ld * j + i]; bx[i] -= lji * vx; if (TWO) by[i] -= lji * vy; }
        }
    }
    qp_sync<WV>();
}

// pt[m] = B0 + (m dt) dt of m = lane, with m dt accumulated by m additions (the caller stores it: pt[m], m <= N - 1, is all that is read)
__device__ __forceinline__ double pv_pt_entry(double dt, double b0, int lane)
{
    double s = 0.0, mine = 0.0;
    for (int m = 0; m < 64; m++) { mine = (m == lane) ? s : mine; s = s + dt; }
    return mul_then_add(mine, dt, b0);
}

// the lower triangle of H = alpha I + beta Pu'Pu, row i by lane i
__device__ __forceinline__ void pv_form_h(double *H, const int ldh, const double *pt, double D, double alpha, double beta, int n, int lane)
{
    for (int i = lane; i < n; i += 64)
        for (int j = 0; j <= i; j++) {
            double s = ((i == j) ? D : pt[i - j - 1]) * D;         // l = i: Pu[i][j] Pu[i][i]
            for (int l = i + 1; l < n; l++) s += pt[l - j - 1] * pt[l - i - 1];
            H[ldh * i + j] = ((i == j) ? alpha : 0.0) + beta * s;
        }
}

// r = Px x_k - z over the clamped, scaled window; BOX: the bounds of the same samples, in metres as they are, row a at bw + bws * a.
// -> this lane met an empty or NaN box sample
template <bool BOX>
__device__ __forceinline__ bool qp_residual(int n, int ns, int lane, int k, double xs, const double *zx, const double *zy, const double *px0, const double *px1,
                                            double x, double xd, double y, double yd, double *rx, double *ry, const double *boxp, double *bw, const int bws)
{
    bool empty = false;
    for (int l = lane; l < n; l += 64) {
        const int kk = mpc_clamp(k + l, ns);
        rx[l] = fma(-xs, zx[kk], fma(px0[l], x, px1[l] * xd));
        ry[l] = fma(px0[l], y, px1[l] * yd) - zy[kk];
        if constexpr (BOX) {
            const double *bp = boxp + kk;
#pragma unroll
            for (int a = 0; a < 4; a++) bw[bws * a + l] = bp[(size_t)a * ns];
            empty = empty || !(bw[l] <= bw[bws + l]) || !(bw[bws * 2 + l] <= bw[bws * 3 + l]);
        }
    }
    return empty;
}

// g = beta Pu' r into bx | by (BOX: kept in gk | gk + gks as well)
template <bool BOX>
__device__ __forceinline__ void qp_gradient(int n, int lane, double D, double beta, const double *pt, const double *rx, const double *ry, double *bx, double *by,
                                            double *gk, const int gks)
{
    for (int j = lane; j < n; j += 64) {
        double sx = D * rx[j], sy = D * ry[j];
        for (int l = j + 1; l < n; l++) { const double p = pt[l - j - 1]; sx += p * rx[l]; sy += p * ry[l]; }
        bx[j] = beta * sx; by[j] = beta * sy;
        if constexpr (BOX) { gk[j] = bx[j]; gk[gks + j] = by[j]; }
    }
}

// U = -H^-1 g from the solve's result
__device__ __forceinline__ void qp_negate(int n, int lane, bool spd, double *bx, double *by)
{
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (int i = lane; i < n; i += 64) {
        bx[i] = spd ? -bx[i] : nan; by[i] = spd ? -by[i] : nan;
    }
}

// Z = Px x_k + Pu U
__device__ __forceinline__ void qp_predict(int n, int lane, double D, const double *pt, const double *px0, const double *px1, double x, double xd, double y, double yd,
                                           const double *bx, const double *by, double *rx, double *ry)
{
    for (int l = lane; l < n; l += 64) {
        double sx = fma(D, bx[l], fma(px0[l], x, px1[l] * xd)), sy = fma(D, by[l], fma(px0[l], y, px1[l] * yd));
        for (int j = 0; j < l; j++) { const double p = pt[l - j - 1]; sx += p * bx[j]; sy += p * by[j]; }
        rx[l] = sx; ry[l] = sy;
    }
}

// G = Pu H^-1 Pu' = Y'Y into the upper triangle of the packed tile, Y = L^-1 Pu' through the second tile (lmh_mpc.hip, header comment)
template <bool WV>
__device__ __forceinline__ void box_form_g(double *HG, const int ldb, double *T, const int ld, const double *pt, double D, int n, int lane)
{
    qp_sync<WV>();
    for (int c = lane; c < n; c += 64)                             // Y, column c by lane c (Pu'[i][c] = Pu[c][i], zero below the diagonal)
        for (int i = 0; i < n; i++) {
            double s = (i == c) ? D : ((i < c) ? pt[c - i - 1] : 0.0);
            for (int j = 0; j < i; j++) s = fma(-HG[ldb * i + j], T[ld * j + c], s);
            T[ld * i + c] = s / HG[ldb * i + i];
        }
    qp_sync<WV>();
    for (int c = lane; c < n; c += 64)                             // G = Y'Y, the upper triangle, column c by lane c
        for (int r = 0; r <= c; r++) {
            double s = 0.0;
            for (int i = 0; i < n; i++) s = fma(T[ld * i + r], T[ld * i + c], s);
            HG[ldb * r + c + 1] = s;
        }
    qp_sync<WV>();
}

// The working-set rounds of one axis on the factor (lmh_mpc.hip, header comment; include/lmh.h has the exchange rule).  In: u = U0,
// z = Z0 = p + Pu U0, g, the window's bounds lo / hi.  Out: u, z, lam, side (-1 lower, +1 upper, 0 inactive) of the last iterate; -> rounds, active, flags.
struct BoxLds {
    double *T;                                                     // n x ld: the factor of S
    double *z0, *v, *rhs;                                          // [n] each
    int *side, *want, *widx;                                       // [n] each
};

template <bool WV>
__device__ __forceinline__ void box_rounds(double *HG, const int ldb, const int ld, const double *pt, double D, int n, int lane, const double *p0, const double *p1,
                                           double s0, double s1, const double *g, const double *lo, const double *hi, double *u, double *z,
                                           double *lam, const BoxLds &W, bool &have_g, int &rounds_out, int &active_out, int &flags)
{
    for (int i = lane; i < n; i += 64) { W.side[i] = 0; W.z0[i] = z[i]; lam[i] = 0.0; }
    int rounds = 0, active = 0, best = n + 1, block = 3;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (;;) {
        qp_sync<WV>();
        for (int i = lane; i < n; i += 64) {                       // what is wrong with this iterate: exact fp64 compares
            const int s = W.side[i];
            int w = s;
            if (s == 0) w = (z[i] < lo[i]) ? -1 : ((z[i] > hi[i]) ? 1 : 0);
            else if ((s > 0 && lam[i] < 0.0) || (s < 0 && lam[i] > 0.0)) w = 0;
            W.want[i] = w;
        }
        qp_sync<WV>();
        int nbad = 0, last = -1;
        for (int i = 0; i < n; i++) if (W.want[i] != W.side[i]) { nbad++; last = i; }
        if (nbad == 0) break;
        if (rounds >= LMH_MPC_BOX_MAX_ROUNDS) { flags |= LMH_FLAG_QP_MAXITER; break; }
        rounds++;
        if (!have_g) { box_form_g<WV>(HG, ldb, W.T, ld, pt, D, n, lane); have_g = true; }
        bool single = false;
        if (nbad < best) { best = nbad; block = 3; }
        else if (block > 0) block--;
        else single = true;
        qp_sync<WV>();
        for (int i = lane; i < n; i += 64) if (!single || i == last) W.side[i] = W.want[i];
        qp_sync<WV>();
        int m = 0;
        for (int i = 0; i < n; i++) if (W.side[i] != 0) { if (lane == 0) W.widx[m] = i; m++; }
        active = m;
        qp_sync<WV>();
        for (int a = lane; a < m; a += 64) {                       // S = G[W][W], lower triangle (W ascends); rhs = Z0_W - b_W
            const int ia = W.widx[a];
            for (int b = 0; b <= a; b++) W.T[ld * a + b] = HG[ldb * W.widx[b] + ia + 1];
            W.rhs[a] = W.z0[ia] - ((W.side[ia] > 0) ? hi[ia] : lo[ia]);
        }
        for (int i = lane; i < n; i += 64) lam[i] = 0.0;
        const bool spd = pv_factor<WV>(W.T, ld, m, lane);
        if (!spd) {
            flags |= LMH_FLAG_NOT_SPD;
            qp_sync<WV>();
            for (int i = lane; i < n; i += 64) { u[i] = nan; z[i] = nan; lam[i] = nan; }
            break;
        }
        pv_solve<false, WV>(W.T, ld, m, lane, W.rhs, nullptr);
        for (int a = lane; a < m; a += 64) lam[W.widx[a]] = W.rhs[a];
        qp_sync<WV>();
        for (int j = lane; j < n; j += 64) {                       // v = g + Pu' lambda
            double s = D * lam[j];
            for (int l = j + 1; l < n; l++) s = fma(pt[l - j - 1], lam[l], s);
            W.v[j] = g[j] + s;
        }
        pv_solve<false, WV>(HG, ldb, n, lane, W.v, nullptr);
        for (int i = lane; i < n; i += 64) u[i] = -W.v[i];
        qp_sync<WV>();
        for (int l = lane; l < n; l += 64) {                       // Z = p + Pu U; an active sample sits on its bound
            double s = fma(D, u[l], fma(p0[l], s0, p1[l] * s1));
            for (int j = 0; j < l; j++) s = fma(pt[l - j - 1], u[j], s);
            const int sd = W.side[l];
            z[l] = (sd == 0) ? s : ((sd > 0) ? hi[l] : lo[l]);
        }
    }
    qp_sync<WV>();
    rounds_out = rounds; active_out = active;
}

// The arrays of one robot's constrained problem: two tiles and sixteen [n] arrays of doubles, three of ints.
struct BoxArrays {
    double *H, *T;                                                 // n x ldb (L | G packed), n x ld
    int ldb, ld;
    double *pt, *rx, *ry, *bx, *by;
    double *bw; int bws;                                           // the window's bounds, row a at bw + bws * a
    double *gk; int gks;                                           // g of both axes
    double *lm; int lms;                                           // the multipliers of both axes
    double *wk; int wks;                                           // z0 | v | rhs
    int *iw; int iws;                                              // side | want | widx
};

// The constrained part of a tick on U0 (bx | by) and Z0 (rx | ry): an empty or NaN box sample fills the solution with NaN, otherwise the rounds
// of both axes.  -> act_x + act_y through act, the rounds through rounds_x / rounds_y.
template <bool WV>
__device__ __forceinline__ void box_solve(const BoxArrays &A, const double *px0, const double *px1, double D, int n, int lane, bool empty, bool spd,
                                          double x, double xd, double y, double yd, bool &have_g, int &rounds_x, int &rounds_y, int &act_x, int &act_y, int &flags)
{
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (__any(empty)) {                                            // an empty or NaN box sample: nothing to solve
        flags |= LMH_FLAG_BOX_EMPTY;
        for (int i = lane; i < n; i += 64) { A.bx[i] = nan; A.by[i] = nan; A.rx[i] = nan; A.ry[i] = nan; A.lm[i] = nan; A.lm[A.lms + i] = nan; }
    } else if (spd) {
        const BoxLds W = {A.T, A.wk, A.wk + A.wks, A.wk + 2 * A.wks, A.iw, A.iw + A.iws, A.iw + 2 * A.iws};
        box_rounds<WV>(A.H, A.ldb, A.ld, A.pt, D, n, lane, px0, px1, x, xd, A.gk, A.bw, A.bw + A.bws, A.bx, A.rx, A.lm, W, have_g, rounds_x, act_x, flags);
        box_rounds<WV>(A.H, A.ldb, A.ld, A.pt, D, n, lane, px0, px1, y, yd, A.gk + A.gks, A.bw + 2 * A.bws, A.bw + 3 * A.bws, A.by, A.ry, A.lm + A.lms, W, have_g, rounds_y, act_y, flags);
    } else {
        for (int i = lane; i < n; i += 64) { A.lm[i] = nan; A.lm[A.lms + i] = nan; }
    }
    qp_sync<WV>();
}

// the sample of lmh_mpc_step from U[0] and Z[0] (mpc_step_one's expressions)
__device__ __forceinline__ void qp_sample(const LipAB &M, const double *bx, const double *by, const double *rx, const double *ry, double x, double xd, double y, double yd,
                                          int k, int flags, MpcSample &S)
{
    const double ux = bx[0], uy = by[0];
    S.ux = ux; S.uy = uy; S.zmx = rx[0]; S.zmy = ry[0];
    S.xp = fma(M.b0, ux, fma(M.a00, x, M.a01 * xd)); S.xv = fma(M.b1, ux, fma(M.a10, x, M.a11 * xd));
    S.yp = fma(M.b0, uy, fma(M.a00, y, M.a01 * yd)); S.yv = fma(M.b1, uy, fma(M.a10, y, M.a11 * yd));
    const bool fin = finite_f64(S.xp) && finite_f64(S.xv) && finite_f64(ux) && finite_f64(S.yp) && finite_f64(S.yv) && finite_f64(uy) &&
                     finite_f64(S.zmx) && finite_f64(S.zmy);
    S.k = k; S.flags = flags | (fin ? 0 : LMH_FLAG_NONFINITE);
}

// One constrained step from the factor to the sample: lmh_mpc_qp_kernel<QP_BOX_STEP>'s tick.  `spd`: what pv_factor made of H.
template <bool WV>
__device__ __forceinline__ int box_tick(const BoxArrays &A, const LipAB &M, int n, int ns, int lane, int k, int flags, double xs, const double *zx, const double *zy,
                                        const double *px0, const double *px1, double D, double beta, const double *boxp, bool spd, bool &have_g,
                                        double x, double xd, double y, double yd, MpcSample &S)
{
    const bool empty = qp_residual<true>(n, ns, lane, k, xs, zx, zy, px0, px1, x, xd, y, yd, A.rx, A.ry, boxp, A.bw, A.bws);
    qp_sync<WV>();
    qp_gradient<true>(n, lane, D, beta, A.pt, A.rx, A.ry, A.bx, A.by, A.gk, A.gks);
    if (spd) pv_solve<true, WV>(A.H, A.ldb, n, lane, A.bx, A.by);
    qp_sync<WV>();
    qp_negate(n, lane, spd, A.bx, A.by);
    qp_sync<WV>();
    qp_predict(n, lane, D, A.pt, px0, px1, x, xd, y, yd, A.bx, A.by, A.rx, A.ry);
    qp_sync<WV>();
    int rounds_x = 0, rounds_y = 0, act_x = 0, act_y = 0;
    box_solve<WV>(A, px0, px1, D, n, lane, empty, spd, x, xd, y, yd, have_g, rounds_x, rounds_y, act_x, act_y, flags);
    if (!spd) flags |= LMH_FLAG_NOT_SPD;
    qp_sample(M, A.bx, A.by, A.rx, A.ry, x, xd, y, yd, k, flags, S);
    return act_x + act_y;
}
