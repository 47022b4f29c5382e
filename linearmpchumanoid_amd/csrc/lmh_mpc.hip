// lmh_mpc.hip -- the LIPM preview MPC (Mpc3dLip::compute, src/mpcLinearPendulum.cpp:78-109) as a kernel family of its own:
//   lmh_mpc_step     one preview step per robot at the robot's own clock
//   lmh_mpc_rollout  the reduced model in closed loop, n_ticks steps with the robot on chip
//   lmh_mpc_preview  the whole unconstrained solution U = -H^-1 g over the horizon, the predicted ZMP and CoM
//   lmh_mpc_box_preview / _step / _rollout  the same problem with the predicted ZMP held inside per-sample bounds: working-set rounds
//                    on the preview's factor
// (include/lmh.h has the records and the definitions).  One wave per robot, fp64.  The kernels read the handle's gain records, plan,
// xscale and LIPM literals through the parameter block, which travels by value in the kernel arguments, and write nothing but the
// caller's buffers: no launch slot, no host staging, capturable from the first call.
//
// The step is the controller evaluation's, operation for operation: the window sum is refs_prepare's (lane i takes j = i, i + 64, then
// wave_sum), the two sums K.Px are load_common's, the six expressions are refs_chain_a's (lmh_kernels.hip).  They are copied here, not
// shared, so that the code object of lmh_kernels.hip is the one it was; tests/test_gpu_mpc.py holds the copies to the evaluation bit for bit.
// Where the evaluation's source says a * b + c * d the build's contraction makes fma(a, b, c * d) of it there; here every such operation is
// written out as the fma it becomes, because which product the compiler fuses depends on the code around the expression: left to it, the
// tick loop of the rollout fused the x axis the other way round and differed from the step in the last bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/lmh.h"
#include "lmh_device.h"
#include "lmh_launch.h"

#define LANE ((int)(threadIdx.x & 63u))
#define WSYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)
#define WSTAMP(i) do { } while (0)
#include "lmh_dpp.h"

// a * b + c with the product and the sum rounded separately (numpy's c + a * b): the product goes through an opaque register, which the
// contraction of the build's default (fused multiply-add) cannot see through
__device__ __forceinline__ double mul_then_add(double a, double b, double c)
{
    double p = a * b;
    asm volatile("" : "+v"(p));
    return c + p;
}

__device__ __forceinline__ bool finite_f64(double v) { return fabs(v) <= 1.7976931348623157e308; }      // false for NaN and Inf

// What a wave keeps of its robot's gain record for a whole launch: K_lane (lane <= N) and K_64 (lane 0, N = 64: the second trip of the
// window loop), the two state-independent sums, the model's output gain D = -z_com / gravity (the record's first pad word, formed on the
// host where the gain row is) and the robot's step-length scale.
struct MpcGain {
    double K0, K1, kp0, kp1, D, xs;
};

__device__ __forceinline__ void mpc_load_gain(const LmhDevParams &P, int inst, int lane, MpcGain &G)
{
    const double *mp = P.mpc + (size_t)P.mpc_stride_inst * inst;
    const int N = P.horizon;
    G.K0 = (lane <= N) ? mp[lane] : 0.0;
    G.K1 = (lane + 64 <= N) ? mp[lane + 64] : 0.0;
    double s0 = 0.0, s1 = 0.0;                                     // sum K Px0, sum K Px1 (load_common)
    for (int i = lane; i <= N; i += 64) { s0 = fma(mp[i], mp[(N + 1) + i], s0); s1 = fma(mp[i], mp[2 * (N + 1) + i], s1); }
    s0 = wave_sum(s0); s1 = wave_sum(s1);
    G.kp0 = s0; G.kp1 = s1;
    G.D = mp[3 * (N + 1) + 1];
    G.xs = P.xscale ? P.xscale[inst] : 1.0;
}

// the preview index of a clock (mpcLinearPendulum.cpp:92, fp64, same operation order) and whether its window [k, k + N] leaves the arrays
__device__ __forceinline__ int mpc_index(const LmhDevParams &P, double t, int &flags)
{
    const int k = (int)(t / P.mpc_dt);
    flags = (k < 0 || k >= P.n_samples - P.horizon) ? LMH_FLAG_ZMP_RANGE : 0;   // k + N >= n_samples, without the sum
    return k;
}

__device__ __forceinline__ int mpc_clamp(int kk, int ns) { return (kk < 0) ? 0 : (kk >= ns ? ns - 1 : kk); }

// sum_j K_j z[k + j] of both axes over the clamped window (refs_prepare): a coalesced window load per axis and trip
__device__ __forceinline__ void mpc_window(const LmhDevParams &P, const double *zx, const double *zy, const MpcGain &G, int k, int lane, double &wx, double &wy)
{
    const int N = P.horizon, ns = P.n_samples;
    double sx = 0.0, sy = 0.0;
    for (int i = lane; i <= N; i += 64) {                          // only N = 64 reaches a second round
        const int kk = mpc_clamp(k + i, ns);
        const double K = (i < 64) ? G.K0 : G.K1;
        sx = fma(K, zx[kk], sx); sy = fma(K, zy[kk], sy);
    }
    wx = wave_sum(sx); wy = wave_sum(sy);
}

struct MpcSample {
    double xp, xv, ux, yp, yv, uy, zmx, zmy;
    int k, flags;
};

// Mpc3dLip::compute at (cxp, vxp | cyp, vyp, t): u0 = -K (Px x_k - z[k : k + N + 1]), then x_next = A x + B u (refs_chain_a's expressions)
__device__ __forceinline__ void mpc_step_one(const LmhDevParams &P, const double *zx, const double *zy, const MpcGain &G, int lane,
                                             double cxp, double vxp, double cyp, double vyp, double t, MpcSample &S)
{
    int flags;
    const int k = mpc_index(P, t, flags);
    double wx, wy;
    mpc_window(P, zx, zy, G, k, lane, wx, wy);
    const double kp0 = G.kp0, kp1 = G.kp1;
    // ux = -((kp0 * cxp + kp1 * vxp) - xs * wx), uy = -((kp0 * cyp + kp1 * vyp) - wy); xp = a00 * cxp + a01 * vxp + b0 * ux, ... as contracted
    const double ux = -fma(-G.xs, wx, fma(kp0, cxp, kp1 * vxp));
    const double uy = -(fma(kp0, cyp, kp1 * vyp) - wy);
    const double xp = fma(P.b0, ux, fma(P.a00, cxp, P.a01 * vxp)), xv = fma(P.b1, ux, fma(P.a10, cxp, P.a11 * vxp));
    const double yp = fma(P.b0, uy, fma(P.a00, cyp, P.a01 * vyp)), yv = fma(P.b1, uy, fma(P.a10, cyp, P.a11 * vyp));
    S.xp = xp; S.xv = xv; S.ux = ux; S.yp = yp; S.yv = yv; S.uy = uy;
    S.zmx = mul_then_add(G.D, ux, cxp); S.zmy = mul_then_add(G.D, uy, cyp);     // the model's output row C x + D u
    const bool fin = finite_f64(xp) && finite_f64(xv) && finite_f64(ux) && finite_f64(yp) && finite_f64(yv) && finite_f64(uy) &&
                     finite_f64(S.zmx) && finite_f64(S.zmy);
    S.k = k; S.flags = flags | (fin ? 0 : LMH_FLAG_NONFINITE);
}

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

// lmh_mpc_step (ROLL = false: one sample into out[inst], the state is left alone) and lmh_mpc_rollout (ROLL = true: n_ticks samples into
// out[j][inst] when out is given, x <- x_next, t <- t + mpc_dt -- one fp64 add per tick, Clock::step's accumulation order -- and the state
// written back at the end).  The gain row stays in registers for the launch; a tick is two window loads, the DPP reductions and ten flops.
template <bool ROLL>
__global__ void __launch_bounds__(64) lmh_mpc_kernel(LmhDevParams P, double *lip, int n_ticks, double *out)
{
    const int inst = blockIdx.x;
    if (inst >= P.n_instances) return;
    const int lane = LANE;
    MpcGain G;
    mpc_load_gain(P, inst, lane, G);
    const size_t ro = (size_t)P.ref_stride * (size_t)inst;        // per-robot plans: the robot's slice; 0 on a shared plan
    const double *zx = P.zmpx + ro, *zy = P.zmpy + ro;
    double *st = lip + (size_t)LMH_LIP_STRIDE * inst;
    double cxp = st[LMH_LIP_OFF_X], vxp = st[LMH_LIP_OFF_XDOT], cyp = st[LMH_LIP_OFF_Y], vyp = st[LMH_LIP_OFF_YDOT], t = st[LMH_LIP_OFF_T];
    const size_t B = (size_t)P.n_instances;
    MpcSample S;
    if (!ROLL) {
        mpc_step_one(P, zx, zy, G, lane, cxp, vxp, cyp, vyp, t, S);
        mpc_store_sample(out + (size_t)LMH_MPC_STRIDE * inst, lane, S, cxp, vxp, cyp, vyp, t);
        return;
    }
#pragma unroll 1
    for (int j = 0; j < n_ticks; j++) {
        mpc_step_one(P, zx, zy, G, lane, cxp, vxp, cyp, vyp, t, S);
        if (out) mpc_store_sample(out + (size_t)LMH_MPC_STRIDE * ((size_t)j * B + inst), lane, S, cxp, vxp, cyp, vyp, t);
        cxp = S.xp; vxp = S.xv; cyp = S.yp; vyp = S.yv;
        t = t + P.mpc_dt;
    }
    if (lane < 5) {
        double w = cxp;
        w = (lane == LMH_LIP_OFF_XDOT) ? vxp : w; w = (lane == LMH_LIP_OFF_Y) ? cyp : w; w = (lane == LMH_LIP_OFF_YDOT) ? vyp : w;
        w = (lane == LMH_LIP_OFF_T) ? t : w;
        st[lane] = w;
    }
}

// ---------------------------------------------------------------------------- lmh_mpc_preview and the box-constrained family
// One wave per robot forms Pu and H = alpha I + beta Pu'Pu from mpc_dt and the robot's D in LDS, factors H = L L' there and solves both
// axes.  Nothing of it is kept per robot in the handle.
//   Pu is lower triangular Toeplitz: D on the diagonal, Pu[r][c] = C A^m B = B0 + (m dt) dt below it, m = r - c - 1, with m dt accumulated
//   by m additions as Mpc3dLip::initialize's matrix powers accumulate it (build_gain_row, lmh_capi.hip) -- one column of it, pt[m], is all
//   that is stored.
//   The tile: row i of H at ld * i.  ld is odd, so a column sweep (lane i at H[i][j]) puts the 32 lanes of a ds_read_b64 group on
//   the 32 distinct even banks of 64, and the 16 lanes of a ds_write_b64 group on the 16 distinct even banks of 32: no conflicts; a row
//   sweep (lane i at H[j][i]) is contiguous.  Lane i owns row i; lane 0 owns row 64 as well (N = 64).
//   Cost: the right-looking factorisation is n^3 / 3 multiply-adds of which a lane does at most n^2 / 2, the set-up of H as many again.
//
// The box-constrained calls (lmh_mpc_box_preview / _step / _rollout, include/lmh.h) are the same kernel template: the set-up, the
// factorisation, the solve of U0 = -H^-1 g and the prediction Z = Px x_k + Pu U are one copy of source for all four instantiations, and
// every sum of two products in it is written out as the fma it becomes, so that the instantiations agree bit for bit (identities I1-I3).
// On top of the factor a box instantiation keeps G = Pu H^-1 Pu' = Y'Y, Y = L^-1 Pu' (state independent, formed once per launch, by the
// first round that any tick of it needs: a robot whose bounds never bind pays the preview's cost): the
// Schur complement of a working set W is the principal submatrix S = G[W][W], so a round is: gather S (m x m), factor it, lambda_W =
// S^-1 (Z0_W - b_W), U = -H^-1 (g + Pu' lambda), Z = Px x_k + Pu U.
//   LDS: L sits in the lower triangle of the tile and G in the upper one, moved one column right (G[r][c], r <= c, at ld r + c + 1),
//   which takes ld = 67; a second tile holds Y during the set-up and the factor of S during the rounds.  Two tiles, not three.
#define PV_MAXN (LMH_MAX_HORIZON + 1)
#define PV_LD 65
#define PV_LDB 67                                                  // the tile's row stride with G in its upper triangle
#define PV_ARR 66                                                  // entries per array of the record
static_assert(PV_LD >= PV_MAXN && (PV_LD & 1) == 1, "the tile's row stride must hold a row and be odd");
static_assert(PV_LDB >= PV_MAXN + 1 && (PV_LDB & 1) == 1, "the packed tile's row stride must hold a row of L or G and the shift, and be odd");
static_assert(LMH_MPC_PREVIEW_STRIDE == 8 + 8 * PV_ARR, "preview record: header + eight arrays");
static_assert(LMH_MPC_BOX_STRIDE == LMH_MPC_PREVIEW_STRIDE + 2 * PV_ARR, "box record: the preview record + two multiplier arrays");
static_assert(LMH_MPC_BOX_OFF_LAM_X == LMH_MPC_PREVIEW_STRIDE && LMH_MPC_BOX_OFF_LAM_Y == LMH_MPC_PREVIEW_STRIDE + PV_ARR, "multiplier arrays");
static_assert(4 * PV_ARR <= PV_MAXN * PV_LD, "the CoM arrays are staged in a tile");
static_assert(LMH_MPC_BOX_MAX_ROUNDS >= 2 * PV_MAXN, "the round cap must allow every sample to enter and leave once");

enum { QP_PLAIN, QP_BOX_PREVIEW, QP_BOX_STEP, QP_BOX_ROLL };

// A = L L' in place on the leading n x n lower triangle, right-looking; every lane sees the same pivot.  false: a pivot was not positive.
__device__ __forceinline__ bool pv_factor(double *A, const int ld, int n, int lane)
{
    for (int j = 0; j < n; j++) {
        __syncthreads();
        const double d = A[ld * j + j];
        if (!(d > 0.0)) return false;
        const double r = sqrt(d);
        __syncthreads();
        for (int i = lane; i < n; i += 64) {
            if (i == j) A[ld * i + j] = r;
            if (i > j) A[ld * i + j] = A[ld * i + j] / r;
        }
        __syncthreads();
        for (int i = lane; i < n; i += 64)
            if (i > j) {
                const double lij = A[ld * i + j];
                for (int c = j + 1; c <= i; c++) A[ld * i + c] -= lij * A[ld * c + j];
            }
    }
    return true;
}

// b <- (L L')^-1 b for one (bx) or two (bx, by) right-hand sides
template <bool TWO>
__device__ __forceinline__ void pv_solve(const double *A, const int ld, int n, int lane, double *bx, double *by)
{
    for (int j = 0; j < n; j++) {                                  // L w = b
        __syncthreads();
        const double ljj = A[ld * j + j];
        const double wx = bx[j] / ljj, wy = TWO ? by[j] / ljj : 0.0;
        __syncthreads();
        for (int i = lane; i < n; i += 64) {
            if (i == j) { bx[i] = wx; if (TWO) by[i] = wy; }
            if (i > j) { const double lij = A[ld * i + j]; bx[i] -= lij * wx; if (TWO) by[i] -= lij * wy; }
        }
    }
    for (int j = n - 1; j >= 0; j--) {                             // L' v = w
        __syncthreads();
        const double ljj = A[ld * j + j];
        const double vx = bx[j] / ljj, vy = TWO ? by[j] / ljj : 0.0;
        __syncthreads();
        for (int i = lane; i < n; i += 64) {
            if (i == j) { bx[i] = vx; if (TWO) by[i] = vy; }
            if (i < j) { const double lji = A[ld * j + i]; bx[i] -= lji * vx; if (TWO) by[i] -= lji * vy; }
        }
    }
    __syncthreads();
}

// G = Pu H^-1 Pu' = Y'Y into the upper triangle of the packed tile, Y = L^-1 Pu' through the second tile (header comment)
__device__ __forceinline__ void box_form_g(double *HG, double *T, const double *pt, double D, int n, int lane)
{
    __syncthreads();
    for (int c = lane; c < n; c += 64)                             // Y, column c by lane c (Pu'[i][c] = Pu[c][i], zero below the diagonal)
        for (int i = 0; i < n; i++) {
            double s = (i == c) ? D : ((i < c) ? pt[c - i - 1] : 0.0);
            for (int j = 0; j < i; j++) s = fma(-HG[PV_LDB * i + j], T[PV_LD * j + c], s);
            T[PV_LD * i + c] = s / HG[PV_LDB * i + i];
        }
    __syncthreads();
    for (int c = lane; c < n; c += 64)                             // G = Y'Y, the upper triangle, column c by lane c
        for (int r = 0; r <= c; r++) {
            double s = 0.0;
            for (int i = 0; i < n; i++) s = fma(T[PV_LD * i + r], T[PV_LD * i + c], s);
            HG[PV_LDB * r + c + 1] = s;
        }
    __syncthreads();
}

// The working-set rounds of one axis on the factor (header comment; include/lmh.h has the exchange rule).  In: u = U0, z = Z0 = p + Pu U0,
// g, the window's bounds lo / hi.  Out: u, z, lam, side (-1 lower, +1 upper, 0 inactive) of the last iterate; -> rounds, active, flags.
struct BoxLds {
    double *T;                                                     // PV_MAXN x PV_LD: the factor of S
    double *z0, *v, *rhs;                                          // [PV_MAXN] each
    int *side, *want, *widx;                                       // [PV_MAXN] each
};

__device__ __forceinline__ void box_rounds(double *HG, const double *pt, double D, int n, int lane, const double *p0, const double *p1,
                                           double s0, double s1, const double *g, const double *lo, const double *hi, double *u, double *z,
                                           double *lam, const BoxLds &W, bool &have_g, int &rounds_out, int &active_out, int &flags)
{
    for (int i = lane; i < n; i += 64) { W.side[i] = 0; W.z0[i] = z[i]; lam[i] = 0.0; }
    int rounds = 0, active = 0, best = n + 1, block = 3;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    for (;;) {
        __syncthreads();
        for (int i = lane; i < n; i += 64) {                       // what is wrong with this iterate: exact fp64 compares
            const int s = W.side[i];
            int w = s;
            if (s == 0) w = (z[i] < lo[i]) ? -1 : ((z[i] > hi[i]) ? 1 : 0);
            else if ((s > 0 && lam[i] < 0.0) || (s < 0 && lam[i] > 0.0)) w = 0;
            W.want[i] = w;
        }
        __syncthreads();
        int nbad = 0, last = -1;
        for (int i = 0; i < n; i++) if (W.want[i] != W.side[i]) { nbad++; last = i; }
        if (nbad == 0) break;
        if (rounds >= LMH_MPC_BOX_MAX_ROUNDS) { flags |= LMH_FLAG_QP_MAXITER; break; }
        rounds++;
        if (!have_g) { box_form_g(HG, W.T, pt, D, n, lane); have_g = true; }
        bool single = false;
        if (nbad < best) { best = nbad; block = 3; }
        else if (block > 0) block--;
        else single = true;
        __syncthreads();
        for (int i = lane; i < n; i += 64) if (!single || i == last) W.side[i] = W.want[i];
        __syncthreads();
        int m = 0;
        for (int i = 0; i < n; i++) if (W.side[i] != 0) { if (lane == 0) W.widx[m] = i; m++; }
        active = m;
        __syncthreads();
        for (int a = lane; a < m; a += 64) {                       // S = G[W][W], lower triangle (W ascends); rhs = Z0_W - b_W
            const int ia = W.widx[a];
            for (int b = 0; b <= a; b++) W.T[PV_LD * a + b] = HG[PV_LDB * W.widx[b] + ia + 1];
            W.rhs[a] = W.z0[ia] - ((W.side[ia] > 0) ? hi[ia] : lo[ia]);
        }
        for (int i = lane; i < n; i += 64) lam[i] = 0.0;
        const bool spd = pv_factor(W.T, PV_LD, m, lane);
        if (!spd) {
            flags |= LMH_FLAG_NOT_SPD;
            __syncthreads();
            for (int i = lane; i < n; i += 64) { u[i] = nan; z[i] = nan; lam[i] = nan; }
            break;
        }
        pv_solve<false>(W.T, PV_LD, m, lane, W.rhs, nullptr);
        for (int a = lane; a < m; a += 64) lam[W.widx[a]] = W.rhs[a];
        __syncthreads();
        for (int j = lane; j < n; j += 64) {                       // v = g + Pu' lambda
            double s = D * lam[j];
            for (int l = j + 1; l < n; l++) s = fma(pt[l - j - 1], lam[l], s);
            W.v[j] = g[j] + s;
        }
        pv_solve<false>(HG, PV_LDB, n, lane, W.v, nullptr);
        for (int i = lane; i < n; i += 64) u[i] = -W.v[i];
        __syncthreads();
        for (int l = lane; l < n; l += 64) {                       // Z = p + Pu U; an active sample sits on its bound
            double s = fma(D, u[l], fma(p0[l], s0, p1[l] * s1));
            for (int j = 0; j < l; j++) s = fma(pt[l - j - 1], u[j], s);
            const int sd = W.side[l];
            z[l] = (sd == 0) ? s : ((sd > 0) ? hi[l] : lo[l]);
        }
    }
    __syncthreads();
    rounds_out = rounds; active_out = active;
}

// MODE QP_PLAIN: lmh_mpc_preview.  QP_BOX_PREVIEW: its record with the bounds enforced, the round and active counts in the header and the
// multipliers behind it.  QP_BOX_STEP: one sample per robot from the same solution.  QP_BOX_ROLL: n_ticks of them in closed loop on one
// factorisation, the state written back.  box: the robot's bounds at box + box_stride * inst, four rows of n_samples.
template <int MODE>
__global__ void __launch_bounds__(64) lmh_mpc_qp_kernel(LmhDevParams P, double alpha, double beta, double *lip, const double *box, size_t box_stride,
                                                        int n_ticks, double *out)
{
    constexpr bool BOX = MODE != QP_PLAIN, ROLL = MODE == QP_BOX_ROLL, RECORD = MODE == QP_PLAIN || MODE == QP_BOX_PREVIEW;
    constexpr int LDH = BOX ? PV_LDB : PV_LD;
    __shared__ double H[PV_MAXN * LDH];
    __shared__ double T[BOX ? PV_MAXN * PV_LD : 1];
    __shared__ double pt[PV_MAXN], rx[PV_MAXN], ry[PV_MAXN], bx[PV_MAXN], by[PV_MAXN];
    __shared__ double bw[BOX ? 4 : 1][PV_MAXN], gk[BOX ? 2 : 1][PV_MAXN], lm[BOX ? 2 : 1][PV_MAXN], wk[BOX ? 3 : 1][PV_MAXN];
    __shared__ int iw[BOX ? 3 : 1][PV_MAXN];
    const int inst = blockIdx.x;
    if (inst >= P.n_instances) return;
    const int lane = LANE;
    const int N = P.horizon, n = N + 1, ns = P.n_samples;
    const double *mp = P.mpc + (size_t)P.mpc_stride_inst * inst;
    const double *px0 = mp + n, *px1 = mp + 2 * n;
    const double D = mp[3 * n + 1];
    const double xs = P.xscale ? P.xscale[inst] : 1.0;
    const size_t ro = (size_t)P.ref_stride * (size_t)inst;
    const double *zx = P.zmpx + ro, *zy = P.zmpy + ro;
    double *st = lip + (size_t)LMH_LIP_STRIDE * inst;
    double x = st[LMH_LIP_OFF_X], xd = st[LMH_LIP_OFF_XDOT], y = st[LMH_LIP_OFF_Y], yd = st[LMH_LIP_OFF_YDOT], t = st[LMH_LIP_OFF_T];
    const double dt = P.mpc_dt;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const size_t B = (size_t)P.n_instances;

    {                                                              // pt[m], m = lane; pt[64] is never read (m <= N - 1)
        double s = 0.0, mine = 0.0;
        for (int m = 0; m < 64; m++) { mine = (m == lane) ? s : mine; s = s + dt; }
        pt[lane] = mul_then_add(mine, dt, P.b0);
        if (lane == 0) pt[PV_MAXN - 1] = 0.0;
    }
    __syncthreads();
    for (int i = lane; i < n; i += 64)                             // the lower triangle of H, row i
        for (int j = 0; j <= i; j++) {
            double s = ((i == j) ? D : pt[i - j - 1]) * D;         // l = i: Pu[i][j] Pu[i][i]
            for (int l = i + 1; l < n; l++) s += pt[l - j - 1] * pt[l - i - 1];
            H[LDH * i + j] = ((i == j) ? alpha : 0.0) + beta * s;
        }
    const bool spd = pv_factor(H, LDH, n, lane);
    __syncthreads();
    bool have_g = false;                                           // G is formed by the first round of the launch, if there is one

#pragma unroll 1
    for (int tick = 0; tick < (ROLL ? n_ticks : 1); tick++) {
        int flags;
        const int k = mpc_index(P, t, flags);
        bool empty = false;
        for (int l = lane; l < n; l += 64) {                       // r = Px x_k - z over the clamped, scaled window
            const int kk = mpc_clamp(k + l, ns);
            rx[l] = fma(-xs, zx[kk], fma(px0[l], x, px1[l] * xd));
            ry[l] = fma(px0[l], y, px1[l] * yd) - zy[kk];
            if constexpr (BOX) {                                   // the bounds of the same samples, in metres as they are
                const double *bp = box + box_stride * (size_t)inst + kk;
#pragma unroll
                for (int a = 0; a < 4; a++) bw[a][l] = bp[(size_t)a * ns];
                empty = empty || !(bw[0][l] <= bw[1][l]) || !(bw[2][l] <= bw[3][l]);
            }
        }
        __syncthreads();
        for (int j = lane; j < n; j += 64) {                       // g = beta Pu' r
            double sx = D * rx[j], sy = D * ry[j];
            for (int l = j + 1; l < n; l++) { const double p = pt[l - j - 1]; sx += p * rx[l]; sy += p * ry[l]; }
            bx[j] = beta * sx; by[j] = beta * sy;
            if constexpr (BOX) { gk[0][j] = bx[j]; gk[1][j] = by[j]; }
        }
        if (spd) pv_solve<true>(H, LDH, n, lane, bx, by);
        __syncthreads();
        for (int i = lane; i < n; i += 64) {                       // U = -H^-1 g
            bx[i] = spd ? -bx[i] : nan; by[i] = spd ? -by[i] : nan;
        }
        __syncthreads();
        for (int l = lane; l < n; l += 64) {                       // Z = Px x_k + Pu U
            double sx = fma(D, bx[l], fma(px0[l], x, px1[l] * xd)), sy = fma(D, by[l], fma(px0[l], y, px1[l] * yd));
            for (int j = 0; j < l; j++) { const double p = pt[l - j - 1]; sx += p * bx[j]; sy += p * by[j]; }
            rx[l] = sx; ry[l] = sy;
        }
        __syncthreads();
        int rounds_x = 0, rounds_y = 0, act_x = 0, act_y = 0;
        if constexpr (BOX) {
            if (__any(empty)) {                                    // an empty or NaN box sample: nothing to solve
                flags |= LMH_FLAG_BOX_EMPTY;
                for (int i = lane; i < n; i += 64) { bx[i] = nan; by[i] = nan; rx[i] = nan; ry[i] = nan; lm[0][i] = nan; lm[1][i] = nan; }
            } else if (spd) {
                const BoxLds W = {T, wk[0], wk[1], wk[2], iw[0], iw[1], iw[2]};
                box_rounds(H, pt, D, n, lane, px0, px1, x, xd, gk[0], bw[0], bw[1], bx, rx, lm[0], W, have_g, rounds_x, act_x, flags);
                box_rounds(H, pt, D, n, lane, px0, px1, y, yd, gk[1], bw[2], bw[3], by, ry, lm[1], W, have_g, rounds_y, act_y, flags);
            } else {
                for (int i = lane; i < n; i += 64) { lm[0][i] = nan; lm[1][i] = nan; }
            }
            __syncthreads();
        }
        if (!spd) flags |= LMH_FLAG_NOT_SPD;
        if (RECORD) {
            double *cs = BOX ? T : H;                              // c_0 = x_k, c_{j+1} = A c_j + B u_j: N + 2 states, staged in a tile
            {                                                      // (plain: the factor is not read again; box: the factor of S is not)
                const bool ok = spd && !(flags & LMH_FLAG_BOX_EMPTY);
                double cx = ok ? x : nan, cvx = ok ? xd : nan, cy = ok ? y : nan, cvy = ok ? yd : nan;
                for (int j = 0; j <= n; j++) {
                    if (lane == (j & 63)) { cs[j] = cx; cs[PV_ARR + j] = cvx; cs[2 * PV_ARR + j] = cy; cs[3 * PV_ARR + j] = cvy; }
                    if (j < n) {
                        const double ux = bx[j], uy = by[j];
                        const double nx = fma(P.b0, ux, fma(P.a00, cx, P.a01 * cvx)), nvx = fma(P.b1, ux, fma(P.a10, cx, P.a11 * cvx));
                        const double ny = fma(P.b0, uy, fma(P.a00, cy, P.a01 * cvy)), nvy = fma(P.b1, uy, fma(P.a10, cy, P.a11 * cvy));
                        cx = nx; cvx = nvx; cy = ny; cvy = nvy;
                    }
                }
            }
            __syncthreads();
            double *pv = out + (size_t)(BOX ? LMH_MPC_BOX_STRIDE : LMH_MPC_PREVIEW_STRIDE) * inst;
            bool bad = false;
            for (int e = lane; e < PV_ARR; e += 64) {                  // the eight arrays, unused tails zero
                const bool u = e < n, c = e <= n;
                const double v[8] = {u ? bx[e] : 0.0, u ? by[e] : 0.0, u ? rx[e] : 0.0, u ? ry[e] : 0.0,
                                     c ? cs[e] : 0.0, c ? cs[PV_ARR + e] : 0.0, c ? cs[2 * PV_ARR + e] : 0.0, c ? cs[3 * PV_ARR + e] : 0.0};
#pragma unroll
                for (int a = 0; a < 8; a++) { pv[LMH_MPC_PREVIEW_OFF_U_X + PV_ARR * a + e] = v[a]; bad = bad || !finite_f64(v[a]); }
                if constexpr (BOX) {
                    const double lx = u ? lm[0][e] : 0.0, ly = u ? lm[1][e] : 0.0;
                    pv[LMH_MPC_BOX_OFF_LAM_X + e] = lx; pv[LMH_MPC_BOX_OFF_LAM_Y + e] = ly;
                    bad = bad || !finite_f64(lx) || !finite_f64(ly);
                }
            }
            if (__any(bad)) flags |= LMH_FLAG_NONFINITE;
            if (lane < 8) {
                double w = (lane == 0) ? (double)k : (lane == 1) ? (double)flags : (lane == 2) ? (double)N : 0.0;
                if (BOX) w = (lane == 3) ? (double)rounds_x : (lane == 4) ? (double)rounds_y : (lane == 5) ? (double)act_x : (lane == 6) ? (double)act_y : w;
                pv[lane] = w;
            }
        } else {                                                   // the sample of lmh_mpc_step from U[0] and Z[0] (mpc_step_one's expressions)
            MpcSample S;
            const double ux = bx[0], uy = by[0];
            S.ux = ux; S.uy = uy; S.zmx = rx[0]; S.zmy = ry[0];
            S.xp = fma(P.b0, ux, fma(P.a00, x, P.a01 * xd)); S.xv = fma(P.b1, ux, fma(P.a10, x, P.a11 * xd));
            S.yp = fma(P.b0, uy, fma(P.a00, y, P.a01 * yd)); S.yv = fma(P.b1, uy, fma(P.a10, y, P.a11 * yd));
            const bool fin = finite_f64(S.xp) && finite_f64(S.xv) && finite_f64(ux) && finite_f64(S.yp) && finite_f64(S.yv) && finite_f64(uy) &&
                             finite_f64(S.zmx) && finite_f64(S.zmy);
            S.k = k; S.flags = flags | (fin ? 0 : LMH_FLAG_NONFINITE);
            double *rec = ROLL ? (out ? out + (size_t)LMH_MPC_STRIDE * ((size_t)tick * B + inst) : nullptr) : out + (size_t)LMH_MPC_STRIDE * inst;
            if (rec) {
                mpc_store_sample(rec, lane, S, x, xd, y, yd, t);
                if (lane == LMH_MPC_OFF_ACTIVE) rec[lane] = (double)(act_x + act_y);
            }
            if (ROLL) {
                x = S.xp; xd = S.xv; y = S.yp; yd = S.yv;
                t = t + P.mpc_dt;
            }
            __syncthreads();
        }
    }
    if (ROLL && lane < 5) {
        double w = x;
        w = (lane == LMH_LIP_OFF_XDOT) ? xd : w; w = (lane == LMH_LIP_OFF_Y) ? y : w; w = (lane == LMH_LIP_OFF_YDOT) ? yd : w;
        w = (lane == LMH_LIP_OFF_T) ? t : w;
        st[lane] = w;
    }
}

extern "C" void lmh_launch_mpc_step(const LmhDevParams *P, double alpha, double beta, const double *lip, const double *box, size_t box_stride, double *mpc, hipStream_t s)
{
    if (box) hipLaunchKernelGGL(lmh_mpc_qp_kernel<QP_BOX_STEP>, dim3(P->n_instances), dim3(64), 0, s, *P, alpha, beta, const_cast<double *>(lip), box, box_stride, 1, mpc);
    else hipLaunchKernelGGL(lmh_mpc_kernel<false>, dim3(P->n_instances), dim3(64), 0, s, *P, const_cast<double *>(lip), 1, mpc);
}
extern "C" void lmh_launch_mpc_rollout(const LmhDevParams *P, double alpha, double beta, double *lip, const double *box, size_t box_stride, int n_ticks, double *traj, hipStream_t s)
{
    if (box) hipLaunchKernelGGL(lmh_mpc_qp_kernel<QP_BOX_ROLL>, dim3(P->n_instances), dim3(64), 0, s, *P, alpha, beta, lip, box, box_stride, n_ticks, traj);
    else hipLaunchKernelGGL(lmh_mpc_kernel<true>, dim3(P->n_instances), dim3(64), 0, s, *P, lip, n_ticks, traj);
}
extern "C" void lmh_launch_mpc_preview(const LmhDevParams *P, double alpha, double beta, const double *lip, const double *box, size_t box_stride, double *record, hipStream_t s)
{
    if (box) hipLaunchKernelGGL(lmh_mpc_qp_kernel<QP_BOX_PREVIEW>, dim3(P->n_instances), dim3(64), 0, s, *P, alpha, beta, const_cast<double *>(lip), box, box_stride, 1, record);
    else hipLaunchKernelGGL(lmh_mpc_qp_kernel<QP_PLAIN>, dim3(P->n_instances), dim3(64), 0, s, *P, alpha, beta, const_cast<double *>(lip), nullptr, (size_t)0, 1, record);
}
