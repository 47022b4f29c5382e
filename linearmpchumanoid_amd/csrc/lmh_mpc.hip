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
#include "lmh_mpc_qp.h"                                            // the maths the fused closed loop shares (lmh_kernels.hip)

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

    pt[lane] = pv_pt_entry(dt, P.b0, lane);                        // pt[m], m = lane; pt[64] is never read (m <= N - 1)
    if (lane == 0) pt[PV_MAXN - 1] = 0.0;
    __syncthreads();
    pv_form_h(H, LDH, pt, D, alpha, beta, n, lane);
    const bool spd = pv_factor<false>(H, LDH, n, lane);
    __syncthreads();
    bool have_g = false;                                           // G is formed by the first round of the launch, if there is one
    const BoxArrays A = {H, T, LDH, PV_LD, pt, rx, ry, bx, by, &bw[0][0], PV_MAXN, &gk[0][0], PV_MAXN, &lm[0][0], PV_MAXN, &wk[0][0], PV_MAXN, &iw[0][0], PV_MAXN};

#pragma unroll 1
    for (int tick = 0; tick < (ROLL ? n_ticks : 1); tick++) {
        int flags;
        const int k = mpc_index(P, t, flags);
        const bool empty = qp_residual<BOX>(n, ns, lane, k, xs, zx, zy, px0, px1, x, xd, y, yd, rx, ry, BOX ? box + box_stride * (size_t)inst : nullptr, A.bw, A.bws);
        __syncthreads();
        qp_gradient<BOX>(n, lane, D, beta, pt, rx, ry, bx, by, A.gk, A.gks);
        if (spd) pv_solve<true, false>(H, LDH, n, lane, bx, by);
        __syncthreads();
        qp_negate(n, lane, spd, bx, by);
        __syncthreads();
        qp_predict(n, lane, D, pt, px0, px1, x, xd, y, yd, bx, by, rx, ry);
        __syncthreads();
        int rounds_x = 0, rounds_y = 0, act_x = 0, act_y = 0;
        if constexpr (BOX) box_solve<false>(A, px0, px1, D, n, lane, empty, spd, x, xd, y, yd, have_g, rounds_x, rounds_y, act_x, act_y, flags);
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
            const LipAB M = {P.a00, P.a01, P.a10, P.a11, P.b0, P.b1};
            qp_sample(M, bx, by, rx, ry, x, xd, y, yd, k, flags, S);
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
