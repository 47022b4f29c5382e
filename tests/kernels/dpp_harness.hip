// Test harness of the DPP layer (csrc/lmh_dpp.h): one kernel per primitive / chain / solve, so that tests/test_gpu_dpp.py can compare each
// with an exact or high-precision reference.  Test infrastructure: built into liblmh_dpp_harness.so (build.build_dpp_harness), never part
// of liblmh_hip.so.
//
// Every kernel is one wave per block and one test case per block (a case table is one launch), has wave-uniform control flow only, reads
// and writes at addresses formed from blockIdx, the lane and compile-time constants alone (rows outside a system read a clamped, valid
// address and are masked by value, as the production callers do), and writes every lane's result registers back.  The per-case element
// counts of every buffer are listed in tests/dpp_cases.py (LAUNCHERS), which sizes the buffers.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <type_traits>

#define LANE ((int)(threadIdx.x & 63))
#define WSYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)
#define WSTAMP(i) do { } while (0)
#include "lmh_dpp.h"

#define HK extern "C" __global__ __launch_bounds__(64) void

template <int I, int E, class F>
__device__ __forceinline__ void static_for(F &&f)
{
    if constexpr (I < E) { f(std::integral_constant<int, I>{}); static_for<I + 1, E>(f); }
}
#define IC(ic) (decltype(ic)::value)

// ---- lane movement.  out[case][148][64]: dpp_row<0xB1, 0x4E, 0x141, 0x140> | bcast16<0..15> | bcast_lane(x, 0..63) | read_lane_f64(x, 0..63)
HK k_lanes_f64(const double *in, double *out)
{
    const int lane = LANE;
    const size_t cs = blockIdx.x;
    const double x = in[cs * 64 + lane];
    double *o = out + cs * (148 * 64) + lane;
    o[0 * 64] = dpp_row<0xB1>(x); o[1 * 64] = dpp_row<0x4E>(x); o[2 * 64] = dpp_row<0x141>(x); o[3 * 64] = dpp_row<0x140>(x);
    static_for<0, 16>([&](auto c) { o[(4 + IC(c)) * 64] = bcast16<IC(c)>(x); });
#pragma unroll
    for (int l = 0; l < 64; l++) { o[(20 + l) * 64] = bcast_lane(x, l); o[(84 + l) * 64] = read_lane_f64(x, l); }
}
// out[case][4][64]: dpp_row<0xB1, 0x4E, 0x141, 0x140> of a float
HK k_lanes_f32(const float *in, float *out)
{
    const int lane = LANE;
    const size_t cs = blockIdx.x;
    const float x = in[cs * 64 + lane];
    float *o = out + cs * (4 * 64) + lane;
    o[0 * 64] = dpp_row<0xB1>(x); o[1 * 64] = dpp_row<0x4E>(x); o[2 * 64] = dpp_row<0x141>(x); o[3 * 64] = dpp_row<0x140>(x);
}

// ---- dpp_fmac_one<J>, J = 0, 7, 15.  in[case][3][64] = acc, src, m; out[case][6][64]: acc += lane_J(src) m | x += lane_J(x) m with x = src
HK k_fmac_one(const double *in, double *out)
{
    const int lane = LANE;
    const size_t cs = blockIdx.x;
    const double acc = in[cs * 192 + lane], src = in[cs * 192 + 64 + lane], m = in[cs * 192 + 128 + lane];
    double *o = out + cs * (6 * 64) + lane;
    { double r = acc; dpp_fmac_one<0>(r, src, m); o[0 * 64] = r; }
    { double r = acc; dpp_fmac_one<7>(r, src, m); o[1 * 64] = r; }
    { double r = acc; dpp_fmac_one<15>(r, src, m); o[2 * 64] = r; }
    { double r = src; dpp_fmac_one<0>(r, r, m); o[3 * 64] = r; }
    { double r = src; dpp_fmac_one<7>(r, r, m); o[4 * 64] = r; }
    { double r = src; dpp_fmac_one<15>(r, r, m); o[5 * 64] = r; }
}

// ---- dpp_fmac_range.  in[case][34][64] = a[0..31], src, m.
// out[case][16][32][64]: <16, 0, CNT> on a[32], CNT = 1..16 (ldl2_forward's columns 16..N-1: A0 != B0)
// then  [15][16][64]:   <J + 1, J + 1, 15 - J> on a[16], J = 0..14 (the pivots of ldl16_forward)
HK k_fmac_range(const double *in, double *out)
{
    const int lane = LANE;
    const size_t cs = blockIdx.x;
    const double *ip = in + cs * (34 * 64) + lane;
    const double src = ip[32 * 64], m = ip[33 * 64];
    double *o = out + cs * ((16 * 32 + 15 * 16) * 64) + lane;
    static_for<1, 17>([&](auto cnt) {
        double a[32];
#pragma unroll
        for (int c = 0; c < 32; c++) a[c] = ip[c * 64];
        dpp_fmac_range<16, 0, IC(cnt)>(a, src, m);
#pragma unroll
        for (int c = 0; c < 32; c++) o[((IC(cnt) - 1) * 32 + c) * 64] = a[c];
    });
    double *o2 = o + 16 * 32 * 64;
    static_for<0, 15>([&](auto j) {
        double a[16];
#pragma unroll
        for (int c = 0; c < 16; c++) a[c] = ip[c * 64];
        dpp_fmac_range<IC(j) + 1, IC(j) + 1, 15 - IC(j)>(a, src, m);
#pragma unroll
        for (int c = 0; c < 16; c++) o2[(IC(j) * 16 + c) * 64] = a[c];
    });
}

// ---- dpp_fmac_self.  in[case][17][64] = a[0..15], m.
// out[case][11][16][64]: <0, CNT, (5 CNT) & 15> for CNT = 1..8, 9, 15, 16
// then  [15][16][64]:   <J + 1, 15 - J, J>, J = 0..14 (the columns of a Gauss-Jordan pivot)
template <int CNT>
__device__ __forceinline__ void self_case(const double *ip, double *o, double m)
{
    double a[16];
#pragma unroll
    for (int c = 0; c < 16; c++) a[c] = ip[c * 64];
    dpp_fmac_self<0, CNT, (5 * CNT) & 15>(a, m);
#pragma unroll
    for (int c = 0; c < 16; c++) o[c * 64] = a[c];
}
HK k_fmac_self(const double *in, double *out)
{
    const int lane = LANE;
    const size_t cs = blockIdx.x;
    const double *ip = in + cs * (17 * 64) + lane;
    const double m = ip[16 * 64];
    double *o = out + cs * (26 * 16 * 64) + lane;
    static_for<1, 10>([&](auto cnt) { self_case<IC(cnt)>(ip, o + (IC(cnt) - 1) * 16 * 64, m); });
    self_case<15>(ip, o + 9 * 16 * 64, m);
    self_case<16>(ip, o + 10 * 16 * 64, m);
    double *o2 = o + 11 * 16 * 64;
    static_for<0, 15>([&](auto j) {
        double a[16];
#pragma unroll
        for (int c = 0; c < 16; c++) a[c] = ip[c * 64];
        dpp_fmac_self<IC(j) + 1, 15 - IC(j), IC(j)>(a, m);
#pragma unroll
        for (int c = 0; c < 16; c++) o2[(IC(j) * 16 + c) * 64] = a[c];
    });
}

// ---- dot chains.  in[case][18][64] = acc0, acc1, src, m[0..14].
// out[case][9][64]: bdot6 | dpp_dot12 | dpp_dot15 | dpp_dot6x2 r, l | dpp_dot12_alt a0, a1 | dpp_sum16_alt a0, a1 (m = m[0])
HK k_dots(const double *in, double *out)
{
    const int lane = LANE;
    const size_t cs = blockIdx.x;
    const double *ip = in + cs * (18 * 64) + lane;
    const double acc0 = ip[0], acc1 = ip[64], src = ip[128];
    double m15[15], m12[12], m6[6];
#pragma unroll
    for (int k = 0; k < 15; k++) m15[k] = ip[(3 + k) * 64];
#pragma unroll
    for (int k = 0; k < 12; k++) m12[k] = m15[k];
#pragma unroll
    for (int k = 0; k < 6; k++) m6[k] = m15[k];
    double *o = out + cs * (9 * 64) + lane;
    { double r = acc0; bdot6(r, src, m6); o[0 * 64] = r; }
    { double r = acc0; dpp_dot12(r, src, m12); o[1 * 64] = r; }
    { double r = acc0; dpp_dot15(r, src, m15); o[2 * 64] = r; }
    { double r = acc0, l = acc1; dpp_dot6x2(r, l, src, m6); o[3 * 64] = r; o[4 * 64] = l; }
    { double r = acc0, l = acc1; dpp_dot12_alt(r, l, src, m12); o[5 * 64] = r; o[6 * 64] = l; }
    { double r = acc0, l = acc1; dpp_sum16_alt(r, l, src, m15[0]); o[7 * 64] = r; o[8 * 64] = l; }
}
// in[case][8][64] = acc, src, m[0..5] (float); out[case][64]: bdot6
HK k_bdot6_f32(const float *in, float *out)
{
    const int lane = LANE;
    const size_t cs = blockIdx.x;
    const float *ip = in + cs * (8 * 64) + lane;
    float r = ip[0], m[6];
    const float src = ip[64];
#pragma unroll
    for (int k = 0; k < 6; k++) m[k] = ip[(2 + k) * 64];
    bdot6(r, src, m);
    out[cs * 64 + lane] = r;
}

// ---- reductions.  out[case][2][64]: wave_sum | wave_max
HK k_reduce_f64(const double *in, double *out)
{
    const int lane = LANE;
    const size_t cs = blockIdx.x;
    const double x = in[cs * 64 + lane];
    out[cs * 128 + lane] = wave_sum(x);
    out[cs * 128 + 64 + lane] = wave_max(x);
}
HK k_reduce_f32(const float *in, float *out)
{
    const int lane = LANE;
    const size_t cs = blockIdx.x;
    out[cs * 64 + lane] = wave_sum(in[cs * 64 + lane]);
}
// ---- reciprocals.  out[case][3][64]: fast_rcp | fast_rcp1 | the raw v_rcp_f64 both start from, every lane its own argument
HK k_rcp(const double *in, double *out)
{
    const int lane = LANE;
    const size_t cs = blockIdx.x;
    const double d = in[cs * 64 + lane];
    out[cs * 192 + lane] = fast_rcp(d);
    out[cs * 192 + 64 + lane] = fast_rcp1(d);
    out[cs * 192 + 128 + lane] = __builtin_amdgcn_rcp(d);
}

// ---- ldl_solve_regs<N, M>, loaded as solve_compact does: lane i < N holds the lower triangle of row i, zeros elsewhere.
// A[case][N][N], B[case][M][N], live[case], dadd[case] (read only if DADD); X[case][M][64] = b[] of every lane, ret[case][64].
// Ls has 64 doubles of slack behind the N (N + 1) of L: the 16 < N form reads L[j][lane] under a per-lane condition, and a load
// hoisted over it would reach up to lane 63 past row N - 1.
template <int N, int M, bool DADD>
__device__ __forceinline__ void ldl_case(const double *A, const double *B, const unsigned *live, const double *dadd, double *X, int *ret, double *Ls)
{
    const int lane = LANE;
    const size_t cs = blockIdx.x;
    const bool on = lane < N;
    const int lr = on ? lane : 0;
    double a[N], b[M];
#pragma unroll
    for (int c = 0; c < N; c++) { const double v = A[cs * (N * N) + lr * N + c]; a[c] = (on && c <= lane) ? v : 0.0; }
#pragma unroll
    for (int r = 0; r < M; r++) { const double v = B[cs * (M * N) + r * N + lr]; b[r] = on ? v : 0.0; }
    const unsigned lv = (unsigned)__builtin_amdgcn_readfirstlane((int)live[cs]);
    int bad;
    if constexpr (DADD) bad = ldl_solve_regs<N, M>(a, b, lv, Ls, dadd[cs]);
    else bad = ldl_solve_regs<N, M>(a, b, lv, Ls);
#pragma unroll
    for (int r = 0; r < M; r++) X[cs * (M * 64) + r * 64 + lane] = b[r];
    ret[cs * 64 + lane] = bad;
}
#define LDL_KERNEL(name, N, M, DADD) \
    HK name(const double *A, const double *B, const unsigned *live, const double *dadd, double *X, int *ret) \
    { __shared__ double Ls[N * (N + 1) + 64]; ldl_case<N, M, DADD>(A, B, live, dadd, X, ret, Ls); }
LDL_KERNEL(k_ldl_8_1, 8, 1, false)
LDL_KERNEL(k_ldl_16_1, 16, 1, false)
LDL_KERNEL(k_ldl_15_7, 15, 7, false)
LDL_KERNEL(k_ldl_6_6, 6, 6, false)
LDL_KERNEL(k_ldl_8_1_dadd, 8, 1, true)
LDL_KERNEL(k_ldl_18_7, 18, 7, false)         // the v_readlane form (16 < N <= 32): qp_setup<18, 2>'s 7 right-hand sides
LDL_KERNEL(k_ldl_24_2, 24, 2, false)

// ---- ldl2_solve_regs<16>, loaded as solve_compact2 does: lane i < 16 holds row i in a0 and row 16 + i in a1 (lower triangles).
// A[case][32][32], B[case][32], live[case]; X[case][2][64] = b0 | b1 of every lane, ret[case][64]
HK k_ldl2(const double *A, const double *B, const unsigned *live, double *X, int *ret)
{
    __shared__ double Ls[32 * 33];
    const int lane = LANE;
    const size_t cs = blockIdx.x;
    const bool on = lane < 16;
    const int lr = on ? lane : 0;
    double a0[16], a1[32], b0, b1;
#pragma unroll
    for (int c = 0; c < 16; c++) { const double v = A[cs * 1024 + lr * 32 + c]; a0[c] = (on && c <= lane) ? v : 0.0; }
#pragma unroll
    for (int c = 0; c < 32; c++) { const double v = A[cs * 1024 + (16 + lr) * 32 + c]; a1[c] = (on && c <= 16 + lane) ? v : 0.0; }
    { const double v0 = B[cs * 32 + lr], v1 = B[cs * 32 + 16 + lr]; b0 = on ? v0 : 0.0; b1 = on ? v1 : 0.0; }
    const unsigned lv = (unsigned)__builtin_amdgcn_readfirstlane((int)live[cs]);
    const int bad = ldl2_solve_regs<16>(a0, a1, b0, b1, lv, Ls);
    X[cs * 128 + lane] = b0;
    X[cs * 128 + 64 + lane] = b1;
    ret[cs * 64 + lane] = bad;
}

// ---- gj_solve_regs<N, M>, loaded as the Woodbury / push-through callers do: lane l holds the full row l & 15 (rows >= N: a copy of
// row 0) and DPP row l >> 4 its own M right-hand sides.  A[case][N][N], B[case][4][M][16], live[case]; X[case][M][64], ret[case][64]
template <int N, int M>
__device__ __forceinline__ void gj_case(const double *A, const double *B, const unsigned *live, double *X, int *ret)
{
    const int lane = LANE, l16 = lane & 15, row = lane >> 4;
    const size_t cs = blockIdx.x;
    const int lr = (l16 < N) ? l16 : 0;
    double a[N], b[M];
#pragma unroll
    for (int c = 0; c < N; c++) a[c] = A[cs * (N * N) + lr * N + c];
#pragma unroll
    for (int r = 0; r < M; r++) b[r] = B[((cs * 4 + row) * M + r) * 16 + l16];
    const unsigned lv = (unsigned)__builtin_amdgcn_readfirstlane((int)live[cs]);
    const int bad = gj_solve_regs<N, M>(a, b, lv);
#pragma unroll
    for (int r = 0; r < M; r++) X[cs * (M * 64) + r * 64 + lane] = b[r];
    ret[cs * 64 + lane] = bad;
}
#define GJ_KERNEL(name, N, M) \
    HK name(const double *A, const double *B, const unsigned *live, double *X, int *ret) { gj_case<N, M>(A, B, live, X, ret); }
GJ_KERNEL(k_gj_6_1, 6, 1)
GJ_KERNEL(k_gj_6_2, 6, 2)
GJ_KERNEL(k_gj_12_1, 12, 1)
GJ_KERNEL(k_gj_15_2, 15, 2)
GJ_KERNEL(k_gj_15_7, 15, 7)
GJ_KERNEL(k_gj_16_1, 16, 1)

// ---- guarded gj16_step as kinv_compute uses it: two 6 x 6 systems, DPP rows 0 and 2 = system 0, rows 1 and 3 = system 1; DPP row k
// carries unit right-hand sides 3 (k >> 1) .. 3 (k >> 1) + 2; a system is switched off by its bit of `use` being clear; row / column dd
// of a system (-1: none) is pinned to the unit row / column.  K[case][2][36], use[case], dd[case][2];
// X[case][4][64] = bb[0..2] * myinv | myinv, flag[case][2][64] = the lane's `bad` | the ballot kinv_compute returns
HK k_gj16_guard(const double *K, const unsigned *use, const int *dd2, double *X, int *flag)
{
    const int lane = LANE, l16 = lane & 15, row = lane >> 4;
    const size_t cs = blockIdx.x;
    const int ft = row & 1, c0 = 3 * (row >> 1);
    const unsigned us = (unsigned)__builtin_amdgcn_readfirstlane((int)use[cs]);
    const bool rowon = ((us >> ft) & 1u) != 0u;
    const int lr = (l16 < 6) ? l16 : 0;
    const int dd = dd2[cs * 2 + ft];
    double a[6], bb[3], myinv = 0.0;
    int bad = 0;
#pragma unroll
    for (int c = 0; c < 6; c++) {
        const double kv = K[cs * 72 + 36 * ft + 6 * lr + c];
        a[c] = (l16 == dd || c == dd) ? ((l16 == c) ? 1.0 : 0.0) : kv;
    }
#pragma unroll
    for (int s = 0; s < 3; s++) bb[s] = (l16 == c0 + s) ? 1.0 : 0.0;
    gj16_step<0>(a, bb, 0x3Fu, l16, rowon, 1e-12, bad, myinv);
#pragma unroll
    for (int s = 0; s < 3; s++) X[cs * 256 + s * 64 + lane] = bb[s] * myinv;
    X[cs * 256 + 3 * 64 + lane] = myinv;
    flag[cs * 128 + lane] = bad;
    flag[cs * 128 + 64 + lane] = (__ballot(bad != 0) != 0ull) ? 1 : 0;
}

// ---- launchers: device pointers, the case count (= blocks), a stream.  Return the launch's hipError_t (0 = ok), -1 for ncase < 1.
#define GO(k, ...) do { if (ncase < 1) return -1; hipLaunchKernelGGL(k, dim3((unsigned)ncase), dim3(64), 0, (hipStream_t)stream, __VA_ARGS__); return (int)hipGetLastError(); } while (0)
extern "C" {
int dpph_lanes_f64(const double *in, double *out, int ncase, void *stream) { GO(k_lanes_f64, in, out); }
int dpph_lanes_f32(const float *in, float *out, int ncase, void *stream) { GO(k_lanes_f32, in, out); }
int dpph_fmac_one(const double *in, double *out, int ncase, void *stream) { GO(k_fmac_one, in, out); }
int dpph_fmac_range(const double *in, double *out, int ncase, void *stream) { GO(k_fmac_range, in, out); }
int dpph_fmac_self(const double *in, double *out, int ncase, void *stream) { GO(k_fmac_self, in, out); }
int dpph_dots(const double *in, double *out, int ncase, void *stream) { GO(k_dots, in, out); }
int dpph_bdot6_f32(const float *in, float *out, int ncase, void *stream) { GO(k_bdot6_f32, in, out); }
int dpph_reduce_f64(const double *in, double *out, int ncase, void *stream) { GO(k_reduce_f64, in, out); }
int dpph_reduce_f32(const float *in, float *out, int ncase, void *stream) { GO(k_reduce_f32, in, out); }
int dpph_rcp(const double *in, double *out, int ncase, void *stream) { GO(k_rcp, in, out); }
#define LDL_LAUNCH(name, k) \
    int name(const double *A, const double *B, const unsigned *live, const double *dadd, double *X, int *ret, int ncase, void *stream) \
    { GO(k, A, B, live, dadd, X, ret); }
LDL_LAUNCH(dpph_ldl_8_1, k_ldl_8_1)
LDL_LAUNCH(dpph_ldl_16_1, k_ldl_16_1)
LDL_LAUNCH(dpph_ldl_15_7, k_ldl_15_7)
LDL_LAUNCH(dpph_ldl_6_6, k_ldl_6_6)
LDL_LAUNCH(dpph_ldl_8_1_dadd, k_ldl_8_1_dadd)
LDL_LAUNCH(dpph_ldl_18_7, k_ldl_18_7)
LDL_LAUNCH(dpph_ldl_24_2, k_ldl_24_2)
int dpph_ldl2(const double *A, const double *B, const unsigned *live, double *X, int *ret, int ncase, void *stream) { GO(k_ldl2, A, B, live, X, ret); }
#define GJ_LAUNCH(name, k) \
    int name(const double *A, const double *B, const unsigned *live, double *X, int *ret, int ncase, void *stream) { GO(k, A, B, live, X, ret); }
GJ_LAUNCH(dpph_gj_6_1, k_gj_6_1)
GJ_LAUNCH(dpph_gj_6_2, k_gj_6_2)
GJ_LAUNCH(dpph_gj_12_1, k_gj_12_1)
GJ_LAUNCH(dpph_gj_15_2, k_gj_15_2)
GJ_LAUNCH(dpph_gj_15_7, k_gj_15_7)
GJ_LAUNCH(dpph_gj_16_1, k_gj_16_1)
int dpph_gj16_guard(const double *K, const unsigned *use, const int *dd, double *X, int *flag, int ncase, void *stream) { GO(k_gj16_guard, K, use, dd, X, flag); }
}
