// DPP layer of the kernels: lane primitives, the row_newbcast fused multiply-add chains and the register-resident SPD solves (LDL',
// Gauss-Jordan) built on them.  Included by lmh_kernels.hip, which defines before it:
//   LANE    lane index inside the wave (0..63)
//   WSYNC() fence between the LDS stores and loads of one wave
//   WSTAMP(i) per-wave diagnostic stamp (empty in the shipped build)
// Everything here needs a full exec mask (wave-uniform control flow only).
#ifndef LMH_DPP_H
#define LMH_DPP_H
#include "lmh_device.h"     // LANE_IS: predicates of the lane id alone as constant lane masks (every `lane` below is the caller's LANE)
// Lane exchange inside a 16-lane row through DPP (two 32-bit v_mov_dpp per double, ~10 cycles) instead of
// ds_bpermute (an LDS round trip per step).  CTRL: 0xB1 = quad_perm[1,0,3,2] (lane ^ 1), 0x4E = quad_perm[2,3,0,1]
// (lane ^ 2), 0x141 = row_half_mirror, 0x140 = row_mirror.  Needs a full exec mask (wave-uniform control flow).
template <int CTRL>
__device__ __forceinline__ double dpp_row(double x)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}
template <int CTRL>
__device__ __forceinline__ float dpp_row(float x)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ double read_lane_f64(double x, int l)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l), __builtin_amdgcn_readlane(__double2loint(x), l));
}
// all-reduce over the 64 lanes: four DPP steps leave every lane with its row's total, the four row totals are
// combined through SGPRs in a fixed order (wave-uniform result)
__device__ __forceinline__ double wave_sum(double v)
{
    v += dpp_row<0xB1>(v); v += dpp_row<0x4E>(v); v += dpp_row<0x141>(v); v += dpp_row<0x140>(v);
    return (read_lane_f64(v, 0) + read_lane_f64(v, 16)) + (read_lane_f64(v, 32) + read_lane_f64(v, 48));
}
__device__ __forceinline__ float wave_sum(float v)
{
    v += dpp_row<0xB1>(v); v += dpp_row<0x4E>(v); v += dpp_row<0x141>(v); v += dpp_row<0x140>(v);
    return (__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0)) + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16)))
         + (__int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32)) + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48)));
}
__device__ __forceinline__ double wave_max(double v)
{
    v = fmax(v, dpp_row<0xB1>(v)); v = fmax(v, dpp_row<0x4E>(v)); v = fmax(v, dpp_row<0x141>(v)); v = fmax(v, dpp_row<0x140>(v));
    return fmax(fmax(read_lane_f64(v, 0), read_lane_f64(v, 16)), fmax(read_lane_f64(v, 32), read_lane_f64(v, 48)));
}

__device__ __forceinline__ double fast_rcp(double d)
{
    double y = __builtin_amdgcn_rcp(d);            // v_rcp_f64 (2^-24.1 measured on gfx950) + two Newton steps -> full fp64 (0.5 ulp measured)
    y = fma(fma(-d, y, 1.0), y, y);
    y = fma(fma(-d, y, 1.0), y, y);
    return y;
}

// one Newton step: the square of v_rcp_f64's error plus one rounding -- up to ~10 ulp on gfx950 (measured 10.3 ulp over 32768 arguments,
// tests/test_gpu_dpp.py; this comment used to say ~2 ulp, which would need a 2^-26 v_rcp_f64, and the instruction is good to 2^-24.1).
// For the multipliers of a Gauss-Jordan elimination that is as good as the exact quotient (the error is a 1e-15
// relative perturbation of the row operation; the eliminated column is never read again), and it takes two instructions off the dependent
// chain pivot -> reciprocal -> multiplier -> update of every pivot.  (gj_solve_regs also scales the solution by this reciprocal:
// x_i = b_i / d_i carries its ~10 ulp, which is what a well-conditioned system's forward error then consists of.)
__device__ __forceinline__ double fast_rcp1(double d)
{
    const double y = __builtin_amdgcn_rcp(d);
    return fma(fma(-d, y, 1.0), y, y);
}

__device__ __forceinline__ double bcast_lane(double x, int l)     // l is a compile-time constant after unrolling
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), l);
    return __hiloint2double(hi, lo);
}

// ---- DPP row broadcast (gfx90a+: 64-bit DPP with row_newbcast): lane l of every 16-lane row reads lane C of
// its own row.  One instruction, no SGPR round trip (v_readlane needs two per double plus the VALU->SGPR hazard).
extern "C" __device__ double lmh_update_dpp_f64(double, double, int, int, int, bool) __asm("llvm.amdgcn.update.dpp.f64");
template <int C>
__device__ __forceinline__ double bcast16(double x)               // compiler-visible v_mov_b64_dpp (hazards handled by llc)
{
    return lmh_update_dpp_f64(x, x, 0x150 + C, 0xf, 0xf, true);
}
// ---- Broadcast-FMA chains: acc += lane_C(src) * m as v_fmac_f64_dpp with row_newbcast (lane C of the own 16-lane row supplies src).
// A DPP operand needs two wait states behind a VALU write of its register, and the compiler's hazard recognizer does not look inside
// inline asm.  So EVERY statement of this family holds its whole chain and begins with s_nop 1: the wait covers whatever the compiler
// placed in front of the statement (the producer of src, or a copy of it made by a live-range split), and nothing inside a statement
// writes a register that a later instruction of it reads through DPP (the "self" shape reads and writes the same register in one
// instruction only).  No helper emits a DPP read without the wait.  Four shapes:
//   one   : acc += lane_J(src) m                         dpp_fmac_one
//   range : a[A0 + k] += lane_(B0 + k)(src) m            dpp_fmac_range (chunks: dpp_fmac_cols)
//   self  : a[c] += lane_J(a[c]) m                       dpp_fmac_self
//   dot   : acc += sum_k lane_k(src) m[k]                bdot6, dpp_dot12, dpp_dot15, dpp_dot6x2, dpp_dot12_alt, dpp_sum16_alt
// Operands of LMH_DPPF: destination, source, multiplier (operand numbers) and the lane (a literal, or %n for an "n" operand).
#define LMH_DPPF(op, d, s, m, c) op " %" #d ", %" #s ", %" #m " row_newbcast:" #c " row_mask:0xf bank_mask:0xf\n\t"
#define LMH_FD(d, s, m, c) LMH_DPPF("v_fmac_f64_dpp", d, s, m, c)
// acc += bcast16<J>(src) * m (acc and src may be the same register)
template <int J>
__device__ __forceinline__ void dpp_fmac_one(double &acc, double src, double m)
{
    asm volatile("s_nop 1\n\t" LMH_FD(0, 1, 2, %3) : "+v"(acc) : "v"(src), "v"(m), "n"(J));
}
template <int A0, int B0, int K, int N>
__device__ __forceinline__ void dpp_fmac_cols(double (&a)[N], double src, double m)    // a[A0 + k] += bcast16<B0 + k>(src) * m for k < K
{
    static_assert(K == 1 || K == 2 || K == 4 || K == 8, "chunk size");
    constexpr int C0 = A0;
    if constexpr (K == 8)
        asm volatile("s_nop 1\n\t" LMH_FD(0, 8, 9, %10) LMH_FD(1, 8, 9, %11) LMH_FD(2, 8, 9, %12) LMH_FD(3, 8, 9, %13)
                     LMH_FD(4, 8, 9, %14) LMH_FD(5, 8, 9, %15) LMH_FD(6, 8, 9, %16) LMH_FD(7, 8, 9, %17)
                     : "+v"(a[C0]), "+v"(a[C0 + 1]), "+v"(a[C0 + 2]), "+v"(a[C0 + 3]), "+v"(a[C0 + 4]), "+v"(a[C0 + 5]), "+v"(a[C0 + 6]), "+v"(a[C0 + 7])
                     : "v"(src), "v"(m), "n"(B0), "n"(B0 + 1), "n"(B0 + 2), "n"(B0 + 3), "n"(B0 + 4), "n"(B0 + 5), "n"(B0 + 6), "n"(B0 + 7));
    else if constexpr (K == 4)
        asm volatile("s_nop 1\n\t" LMH_FD(0, 4, 5, %6) LMH_FD(1, 4, 5, %7) LMH_FD(2, 4, 5, %8) LMH_FD(3, 4, 5, %9)
                     : "+v"(a[C0]), "+v"(a[C0 + 1]), "+v"(a[C0 + 2]), "+v"(a[C0 + 3])
                     : "v"(src), "v"(m), "n"(B0), "n"(B0 + 1), "n"(B0 + 2), "n"(B0 + 3));
    else if constexpr (K == 2)
        asm volatile("s_nop 1\n\t" LMH_FD(0, 2, 3, %4) LMH_FD(1, 2, 3, %5)
                     : "+v"(a[C0]), "+v"(a[C0 + 1]) : "v"(src), "v"(m), "n"(B0), "n"(B0 + 1));
    else
        asm volatile("s_nop 1\n\t" LMH_FD(0, 1, 2, %3) : "+v"(a[C0]) : "v"(src), "v"(m), "n"(B0));
}
// a[A0 + k] += bcast16<B0 + k>(src) * m for k < CNT
template <int A0, int B0, int CNT, int N>
__device__ __forceinline__ void dpp_fmac_range(double (&a)[N], double src, double m)
{
    if constexpr (CNT >= 8) { dpp_fmac_cols<A0, B0, 8>(a, src, m); dpp_fmac_range<A0 + 8, B0 + 8, CNT - 8>(a, src, m); }
    else if constexpr (CNT >= 4) { dpp_fmac_cols<A0, B0, 4>(a, src, m); dpp_fmac_range<A0 + 4, B0 + 4, CNT - 4>(a, src, m); }
    else if constexpr (CNT >= 2) { dpp_fmac_cols<A0, B0, 2>(a, src, m); dpp_fmac_range<A0 + 2, B0 + 2, CNT - 2>(a, src, m); }
    else if constexpr (CNT == 1) { dpp_fmac_cols<A0, B0, 1>(a, src, m); }
}
// a[c] += bcast16<J>(a[c]) * m for c in [C0, C0 + CNT): every register broadcasts its own lane-J entry (the columns of a Gauss-Jordan
// pivot; the right-hand sides of a forward / backward substitution)
template <int C0, int CNT, int J, int N>
__device__ __forceinline__ void dpp_fmac_self(double (&a)[N], double m)
{
    if constexpr (CNT >= 8) {
        asm volatile("s_nop 1\n\t" LMH_FD(0, 0, 8, %9) LMH_FD(1, 1, 8, %9) LMH_FD(2, 2, 8, %9) LMH_FD(3, 3, 8, %9)
                     LMH_FD(4, 4, 8, %9) LMH_FD(5, 5, 8, %9) LMH_FD(6, 6, 8, %9) LMH_FD(7, 7, 8, %9)
                     : "+v"(a[C0]), "+v"(a[C0 + 1]), "+v"(a[C0 + 2]), "+v"(a[C0 + 3]), "+v"(a[C0 + 4]), "+v"(a[C0 + 5]), "+v"(a[C0 + 6]), "+v"(a[C0 + 7])
                     : "v"(m), "n"(J));
        dpp_fmac_self<C0 + 8, CNT - 8, J>(a, m);
    } else if constexpr (CNT == 7) {
        asm volatile("s_nop 1\n\t" LMH_FD(0, 0, 7, %8) LMH_FD(1, 1, 7, %8) LMH_FD(2, 2, 7, %8) LMH_FD(3, 3, 7, %8) LMH_FD(4, 4, 7, %8) LMH_FD(5, 5, 7, %8) LMH_FD(6, 6, 7, %8)
                     : "+v"(a[C0]), "+v"(a[C0 + 1]), "+v"(a[C0 + 2]), "+v"(a[C0 + 3]), "+v"(a[C0 + 4]), "+v"(a[C0 + 5]), "+v"(a[C0 + 6]) : "v"(m), "n"(J));
    } else if constexpr (CNT == 6) {
        asm volatile("s_nop 1\n\t" LMH_FD(0, 0, 6, %7) LMH_FD(1, 1, 6, %7) LMH_FD(2, 2, 6, %7) LMH_FD(3, 3, 6, %7) LMH_FD(4, 4, 6, %7) LMH_FD(5, 5, 6, %7)
                     : "+v"(a[C0]), "+v"(a[C0 + 1]), "+v"(a[C0 + 2]), "+v"(a[C0 + 3]), "+v"(a[C0 + 4]), "+v"(a[C0 + 5]) : "v"(m), "n"(J));
    } else if constexpr (CNT == 5) {
        asm volatile("s_nop 1\n\t" LMH_FD(0, 0, 5, %6) LMH_FD(1, 1, 5, %6) LMH_FD(2, 2, 5, %6) LMH_FD(3, 3, 5, %6) LMH_FD(4, 4, 5, %6)
                     : "+v"(a[C0]), "+v"(a[C0 + 1]), "+v"(a[C0 + 2]), "+v"(a[C0 + 3]), "+v"(a[C0 + 4]) : "v"(m), "n"(J));
    } else if constexpr (CNT == 4) {
        asm volatile("s_nop 1\n\t" LMH_FD(0, 0, 4, %5) LMH_FD(1, 1, 4, %5) LMH_FD(2, 2, 4, %5) LMH_FD(3, 3, 4, %5)
                     : "+v"(a[C0]), "+v"(a[C0 + 1]), "+v"(a[C0 + 2]), "+v"(a[C0 + 3]) : "v"(m), "n"(J));
    } else if constexpr (CNT == 3) {
        asm volatile("s_nop 1\n\t" LMH_FD(0, 0, 3, %4) LMH_FD(1, 1, 3, %4) LMH_FD(2, 2, 3, %4) : "+v"(a[C0]), "+v"(a[C0 + 1]), "+v"(a[C0 + 2]) : "v"(m), "n"(J));
    } else if constexpr (CNT == 2) {
        asm volatile("s_nop 1\n\t" LMH_FD(0, 0, 2, %3) LMH_FD(1, 1, 2, %3) : "+v"(a[C0]), "+v"(a[C0 + 1]) : "v"(m), "n"(J));
    } else if constexpr (CNT == 1) {
        asm volatile("s_nop 1\n\t" LMH_FD(0, 0, 1, %2) : "+v"(a[C0]) : "v"(m), "n"(J));
    }
}
// Dot products of a lane's multipliers with the entries the lanes of its own 16-lane row hold in `src`.  Terms accumulate in k order with
// fused multiply-adds (the order and form of a plain `acc += m[k] * x[k]` loop); with two accumulators each keeps its own k order.
// acc += sum_k lane_k(src) m[k] (k < 6), double and float
#define LMH_DOT6(op) LMH_DPPF(op, 0, 1, 2, 0) LMH_DPPF(op, 0, 1, 3, 1) LMH_DPPF(op, 0, 1, 4, 2) LMH_DPPF(op, 0, 1, 5, 3) LMH_DPPF(op, 0, 1, 6, 4) LMH_DPPF(op, 0, 1, 7, 5)
__device__ __forceinline__ void bdot6(double &acc, double src, const double (&m)[6])
{
    asm volatile("s_nop 1\n\t" LMH_DOT6("v_fmac_f64_dpp") : "+v"(acc) : "v"(src), "v"(m[0]), "v"(m[1]), "v"(m[2]), "v"(m[3]), "v"(m[4]), "v"(m[5]));
}
__device__ __forceinline__ void bdot6(float &acc, float src, const float (&m)[6])
{
    asm volatile("s_nop 1\n\t" LMH_DOT6("v_fmac_f32_dpp") : "+v"(acc) : "v"(src), "v"(m[0]), "v"(m[1]), "v"(m[2]), "v"(m[3]), "v"(m[4]), "v"(m[5]));
}
// acc += sum_k lane_k(src) m[k] (k < 12)
__device__ __forceinline__ void dpp_dot12(double &acc, double src, const double (&m)[12])
{
    asm volatile("s_nop 1\n\t" LMH_FD(0, 1, 2, 0) LMH_FD(0, 1, 3, 1) LMH_FD(0, 1, 4, 2) LMH_FD(0, 1, 5, 3) LMH_FD(0, 1, 6, 4) LMH_FD(0, 1, 7, 5)
                 LMH_FD(0, 1, 8, 6) LMH_FD(0, 1, 9, 7) LMH_FD(0, 1, 10, 8) LMH_FD(0, 1, 11, 9) LMH_FD(0, 1, 12, 10) LMH_FD(0, 1, 13, 11)
                 : "+v"(acc) : "v"(src), "v"(m[0]), "v"(m[1]), "v"(m[2]), "v"(m[3]), "v"(m[4]), "v"(m[5]),
                   "v"(m[6]), "v"(m[7]), "v"(m[8]), "v"(m[9]), "v"(m[10]), "v"(m[11]));
}
// acc += sum_k lane_k(src) m[k] (k < 15)
__device__ __forceinline__ void dpp_dot15(double &acc, double src, const double (&m)[15])
{
    asm volatile("s_nop 1\n\t" LMH_FD(0, 1, 2, 0) LMH_FD(0, 1, 3, 1) LMH_FD(0, 1, 4, 2) LMH_FD(0, 1, 5, 3) LMH_FD(0, 1, 6, 4) LMH_FD(0, 1, 7, 5)
                 LMH_FD(0, 1, 8, 6) LMH_FD(0, 1, 9, 7) LMH_FD(0, 1, 10, 8) LMH_FD(0, 1, 11, 9) LMH_FD(0, 1, 12, 10) LMH_FD(0, 1, 13, 11)
                 LMH_FD(0, 1, 14, 12) LMH_FD(0, 1, 15, 13) LMH_FD(0, 1, 16, 14)
                 : "+v"(acc) : "v"(src), "v"(m[0]), "v"(m[1]), "v"(m[2]), "v"(m[3]), "v"(m[4]), "v"(m[5]), "v"(m[6]), "v"(m[7]),
                   "v"(m[8]), "v"(m[9]), "v"(m[10]), "v"(m[11]), "v"(m[12]), "v"(m[13]), "v"(m[14]));
}
// r += sum_k lane_k(src) m[k], l += sum_k lane_(6 + k)(src) m[k] (k < 6): one foot's six entries each, interleaved
__device__ __forceinline__ void dpp_dot6x2(double &r, double &l, double src, const double (&m)[6])
{
    asm volatile("s_nop 1\n\t" LMH_FD(0, 2, 3, 0) LMH_FD(1, 2, 3, 6) LMH_FD(0, 2, 4, 1) LMH_FD(1, 2, 4, 7) LMH_FD(0, 2, 5, 2) LMH_FD(1, 2, 5, 8)
                 LMH_FD(0, 2, 6, 3) LMH_FD(1, 2, 6, 9) LMH_FD(0, 2, 7, 4) LMH_FD(1, 2, 7, 10) LMH_FD(0, 2, 8, 5) LMH_FD(1, 2, 8, 11)
                 : "+v"(r), "+v"(l) : "v"(src), "v"(m[0]), "v"(m[1]), "v"(m[2]), "v"(m[3]), "v"(m[4]), "v"(m[5]));
}
// a0 += sum_(k even) lane_k(src) m[k], a1 += sum_(k odd) lane_k(src) m[k] (k < 12): two independent chains of half the length
__device__ __forceinline__ void dpp_dot12_alt(double &a0, double &a1, double src, const double (&m)[12])
{
    asm volatile("s_nop 1\n\t" LMH_FD(0, 2, 3, 0) LMH_FD(1, 2, 4, 1) LMH_FD(0, 2, 5, 2) LMH_FD(1, 2, 6, 3) LMH_FD(0, 2, 7, 4) LMH_FD(1, 2, 8, 5)
                 LMH_FD(0, 2, 9, 6) LMH_FD(1, 2, 10, 7) LMH_FD(0, 2, 11, 8) LMH_FD(1, 2, 12, 9) LMH_FD(0, 2, 13, 10) LMH_FD(1, 2, 14, 11)
                 : "+v"(a0), "+v"(a1) : "v"(src), "v"(m[0]), "v"(m[1]), "v"(m[2]), "v"(m[3]), "v"(m[4]), "v"(m[5]),
                   "v"(m[6]), "v"(m[7]), "v"(m[8]), "v"(m[9]), "v"(m[10]), "v"(m[11]));
}
// a0 += m sum_(k even) lane_k(src), a1 += m sum_(k odd) lane_k(src) (k < 16; m = 1: the sum over a 16-lane row, on every lane of it)
__device__ __forceinline__ void dpp_sum16_alt(double &a0, double &a1, double src, double m)
{
    asm volatile("s_nop 1\n\t" LMH_FD(0, 2, 3, 0) LMH_FD(1, 2, 3, 1) LMH_FD(0, 2, 3, 2) LMH_FD(1, 2, 3, 3) LMH_FD(0, 2, 3, 4) LMH_FD(1, 2, 3, 5)
                 LMH_FD(0, 2, 3, 6) LMH_FD(1, 2, 3, 7) LMH_FD(0, 2, 3, 8) LMH_FD(1, 2, 3, 9) LMH_FD(0, 2, 3, 10) LMH_FD(1, 2, 3, 11)
                 LMH_FD(0, 2, 3, 12) LMH_FD(1, 2, 3, 13) LMH_FD(0, 2, 3, 14) LMH_FD(1, 2, 3, 15)
                 : "+v"(a0), "+v"(a1) : "v"(src), "v"(m));
}
// One pivot of the row-per-lane LDL' for N <= 16 (all rows inside DPP row 0), then the next (compile-time recursion).
// `dadd`: a constant on the diagonal of the matrix, added where the pivot is read (the diagonal entry is touched nowhere else: lane J's own
// column entry is only ever used through this broadcast), so that the caller does not have to place it with a select per column.
template <int J, int N, int M>
__device__ __forceinline__ void ldl16_forward(double (&a)[N], double (&b)[M], unsigned live, int lane, int &bad, double &myinv, double dadd = 0.0)
{
    if constexpr (J < N) {
        if ((live >> J) & 1u) {                                   // wave-uniform
            // (DPP rows 1..3 hold no matrix rows: whatever they compute -- possibly non-finite -- stays in their lanes; `bad` is read from lane 0)
            const double d = bcast16<J>(a[J]) + dadd;
            if (!(d > 0.0)) bad = 1;
            const double invd = fast_rcp(d);
            const double f = a[J] * invd;                         // L_iJ in lanes i > J
            const double nfm = LANE_IS(lane > J) ? -f : 0.0;
            if (LANE_IS(lane == J)) myinv = invd;
            dpp_fmac_range<J + 1, J + 1, N - 1 - J>(a, a[J], -f);                 // a[c] -= f * (d_J L_cJ held by lane c)
            dpp_fmac_self<0, M, J>(b, nfm);                       // forward substitution
            a[J] = f;                                             // (rows <= J keep a don't-care there: only L_iJ, i > J, is read back)
        }
        ldl16_forward<J + 1>(a, b, live, lane, bad, myinv, dadd);
    }
}
template <int J, int N, int M>
__device__ __forceinline__ void ldl16_backward(double (&b)[M], unsigned live, int lane, const double *Ls)
{
    if constexpr (J > 0) {
        if ((live >> J) & 1u) {
            const double lv = Ls[J * (N + 1) + (LANE_IS(lane < N) ? lane : 0)];      // unconditional load (clamped), masked by value: no exec branch
            const double nl = LANE_IS(lane < J) ? -lv : 0.0;
            dpp_fmac_self<0, M, J>(b, nl);
        }
        ldl16_backward<J - 1, N>(b, live, lane, Ls);
    }
}

// ---- 16 < N <= 32, one right-hand side: TWO matrix rows per lane so that every row lives in DPP row 0 and the
// pivot broadcast is again a row_newbcast.  Lane i < 16 holds row i in a0[0..15] and row 16 + i in a1[0..N-1]
// (lower triangles), rhs entries b0 / b1.  Pivot J < 16: the scaled pivot column sits in a0[J] (rows < 16, lane c)
// and a1[J] (rows >= 16, lane c - 16); pivot J >= 16: in a1[J].
template <int J, int N2>
__device__ __forceinline__ void ldl2_forward(double (&a0)[16], double (&a1)[16 + N2], double &b0, double &b1, unsigned live, int lane,
                                             int &bad, double &inv0, double &inv1)
{
    constexpr int N = 16 + N2;
    if constexpr (J < N) {
        if ((live >> J) & 1u) {                                   // wave-uniform
            if constexpr (J < 16) {
                double d = bcast16<J>(a0[J]);
                d = LANE_IS(lane < 16) ? d : 1.0;
                if (!(d > 0.0)) bad = 1;
                const double invd = fast_rcp(d);
                const double f0 = a0[J] * invd, f1 = a1[J] * invd;     // L_iJ (rows < 16, valid for lane > J) | L_(16+i)J
                const double nfm0 = LANE_IS(lane > J) ? -f0 : 0.0;
                if (LANE_IS(lane == J)) inv0 = invd;
                dpp_fmac_range<J + 1, J + 1, 15 - J>(a0, a0[J], -f0);  // columns J+1..15: lane c holds d_J L_cJ in a0[J]
                dpp_fmac_range<J + 1, J + 1, 15 - J>(a1, a0[J], -f1);
                dpp_fmac_range<16, 0, N2>(a1, a1[J], -f1);             // columns 16..N-1: lane c - 16 holds d_J L_cJ in a1[J]
                dpp_fmac_one<J>(b1, b0, -f1);                          // forward substitution (lane J's b0 is z_J, untouched below)
                dpp_fmac_one<J>(b0, b0, nfm0);
                if (LANE_IS(lane > J)) a0[J] = f0;
                a1[J] = f1;
            } else {
                constexpr int Jp = J - 16;
                double d = bcast16<Jp>(a1[J]);
                d = LANE_IS(lane < 16) ? d : 1.0;
                if (!(d > 0.0)) bad = 1;
                const double invd = fast_rcp(d);
                const double f1 = a1[J] * invd;
                const double nfm1 = LANE_IS(lane > Jp) ? -f1 : 0.0;
                if (LANE_IS(lane == Jp)) inv1 = invd;
                dpp_fmac_range<J + 1, Jp + 1, N - 1 - J>(a1, a1[J], -f1);
                dpp_fmac_one<Jp>(b1, b1, nfm1);
                if (LANE_IS(lane > Jp)) a1[J] = f1;
            }
        }
        ldl2_forward<J + 1, N2>(a0, a1, b0, b1, live, lane, bad, inv0, inv1);
    }
}
template <int J, int N2>
__device__ __forceinline__ void ldl2_backward(double &b0, double &b1, unsigned live, int lane, const double *Ls)
{
    constexpr int N = 16 + N2;
    if constexpr (J > 0) {
        if ((live >> J) & 1u) {
            const int l16 = LANE_IS(lane < 16) ? lane : 0;         // lanes outside DPP row 0 read a valid address
            if constexpr (J >= 16) {
                constexpr int Jp = J - 16;
                const double l0 = LANE_IS(lane < 16) ? Ls[J * (N + 1) + l16] : 0.0;      // L[J][lane], rows < 16
                const double l1 = LANE_IS(lane < Jp) ? Ls[J * (N + 1) + 16 + l16] : 0.0;        // L[J][16 + lane], rows 16 .. J-1
                dpp_fmac_one<Jp>(b0, b1, -l0);
                dpp_fmac_one<Jp>(b1, b1, -l1);
            } else {
                const double l0 = LANE_IS(lane < J) ? Ls[J * (N + 1) + l16] : 0.0;
                dpp_fmac_one<J>(b0, b0, -l0);
            }
        }
        ldl2_backward<J - 1, N2>(b0, b1, live, lane, Ls);
    }
}
// On exit b0 of lane i < 16 holds x_i and b1 holds x_(16+i).  Returns non-zero (wave-uniform) if a pivot was not positive.
template <int N2>
__device__ __forceinline__ int ldl2_solve_regs(double (&a0)[16], double (&a1)[16 + N2], double &b0, double &b1, unsigned live, double *Ls)
{
    constexpr int N = 16 + N2;
    const int lane = LANE;
    int bad = 0;
    double inv0 = 0.0, inv1 = 0.0;
    ldl2_forward<0, N2>(a0, a1, b0, b1, live, lane, bad, inv0, inv1);
    bad = __builtin_amdgcn_readfirstlane(bad);
    b0 *= inv0; b1 *= inv1;                                       // w = D^-1 z
    WSYNC();
    if (LANE_IS(lane < 16)) {
#pragma unroll
        for (int c = 0; c < 15; c++) Ls[lane * (N + 1) + c] = a0[c];                 // L[lane][c], c < lane
    }
    if (LANE_IS(lane < N2)) {
#pragma unroll
        for (int c = 0; c < N - 1; c++) Ls[(16 + lane) * (N + 1) + c] = a1[c];       // L[16 + lane][c], c < 16 + lane
    }
    WSYNC();
    ldl2_backward<N - 1, N2>(b0, b1, live, lane, Ls);
    return bad;
}

// Register-resident LDL' solve of an SPD system with M right-hand sides, N <= 32.
// Lane i < N holds row i of the matrix in a[] (entries a[c], c <= i, are used; rows / columns whose
// bit is clear in `live` must be zero and are skipped) and its rhs entries in b[].  The pivot column
// is broadcast lane to lane (DPP row broadcast for N <= 16, v_readlane above; no LDS round trip inside the
// factorisation); the rows of L are parked once in Ls (row stride N+1, conflict free) for the backward
// substitution.  On exit b[r] of lane i holds x_i.  Returns non-zero (wave-uniform) if a pivot was not positive.
template <int N, int M>
__device__ __forceinline__ int ldl_solve_regs(double (&a)[N], double (&b)[M], unsigned live, double *Ls, double dadd = 0.0)
{
    const int lane = LANE;
    int bad = 0;
    double myinv = 0.0;                                           // 1 / d_lane (0 on rows that are not live)
    if constexpr (N <= 16) {
        WSTAMP(40);
        ldl16_forward<0>(a, b, live, lane, bad, myinv, dadd);
        bad = __builtin_amdgcn_readfirstlane(bad);
#pragma unroll
        for (int r = 0; r < M; r++) b[r] *= myinv;                // w = D^-1 z
        WSTAMP(41);
        WSYNC();
        if (LANE_IS(lane < N)) {
#pragma unroll
            for (int c = 0; c < N - 1; c++) Ls[lane * (N + 1) + c] = a[c];          // L[lane][c], c < lane
        }
        WSYNC();
        WSTAMP(42);
        ldl16_backward<N - 1, N>(b, live, lane, Ls);
        WSTAMP(43);
        return bad;
    }
#pragma unroll
    for (int j = 0; j < N; j++) {
        if (!((live >> j) & 1u)) continue;                        // wave-uniform
        const double d = bcast_lane(a[j], j);
        if (!(d > 0.0)) bad = 1;
        const double invd = fast_rcp(d);
        const double f = a[j] * invd;                             // L_ij in lanes i > j
        const double fm = (lane > j) ? f : 0.0;
        if (lane == j) myinv = invd;
#pragma unroll
        for (int c = j + 1; c < N; c++) a[c] = fma(-f, bcast_lane(a[j], c), a[c]);   // lane c still holds d_j L_cj
#pragma unroll
        for (int r = 0; r < M; r++) b[r] = fma(-fm, bcast_lane(b[r], j), b[r]);      // forward substitution
        if (lane > j) a[j] = f;
    }
#pragma unroll
    for (int r = 0; r < M; r++) b[r] *= myinv;                    // w = D^-1 z
    WSYNC();
    if (LANE_IS(lane < N)) {
#pragma unroll
        for (int c = 0; c < N - 1; c++) Ls[lane * (N + 1) + c] = a[c];              // L[lane][c], c < lane
    }
    WSYNC();
#pragma unroll
    for (int j = N - 1; j > 0; j--) {
        if (!((live >> j) & 1u)) continue;
        const double lji = (lane < j) ? Ls[j * (N + 1) + lane] : 0.0;
#pragma unroll
        for (int r = 0; r < M; r++) b[r] = fma(-lji, bcast_lane(b[r], j), b[r]);
    }
    return bad;
}

// ---- Gauss-Jordan form of the register-resident SPD solve for N <= 16 (the well-conditioned systems of the QP set-up: Woodbury core,
// Schur complement, push-through system, K_f).  Lane i < N holds the FULL row i in a[]; pivot J eliminates column J from every other
// row, rows above the pivot included: a[c] += bcast16<J>(a[c]) * nf, b[r] += bcast16<J>(b[r]) * nf with nf = -a_iJ / d_J (0 on row J) --
// every register broadcasts its own lane-J entry, one v_fmac_f64_dpp each.  The instruction count per pivot equals the LDL' forward
// step's, and there is no backward substitution, no L parked in LDS and no fence: x_i = b_i / d_i at the end.  Without pivoting this is
// as accurate as LDL' on an SPD matrix (measured on the Woodbury core: 7e-14 both, condition 1e4).
// (A software-pipelined form of the pivots was measured slower and removed: DESIGN section 5.)
// One pivot, then the next.  GUARD = true: `rowon` switches a whole 16-lane DPP row off (its pivots are replaced by 1) and a pivot that is
// not above `dmin` is replaced by 1 and reported in `bad` (kinv_compute: each foot on two DPP rows, a rank-deficient K_f is an expected
// outcome).  GUARD = false (gj_solve_regs): every DPP row carries a copy of the system, so the pivot a lane sees is always the true one --
// no guard selects, no test per pivot: lane J keeps 1 / d_J, and the caller looks at the signs once at the end.
// `l16` MUST be lane & 15 of the calling lane: the pivot-lane predicate l16 == J is taken from the constant lane mask 0x0001000100010001 << J
// (two scalar moves instead of a vector compare per pivot), so the argument only states the layout the callers have to be in.
template <int J, int N, int M, bool GUARD = true>
__device__ __forceinline__ void gj16_step(double (&a)[N], double (&b)[M], unsigned live, int l16, bool rowon, double dmin, int &bad, double &myinv)
{
    if constexpr (J < N) {
        if ((live >> J) & 1u) {                                   // wave-uniform
            double d = bcast16<J>(a[J]);
            if constexpr (GUARD) {
                if (rowon && !(d > dmin)) bad = 1;
                d = (rowon && d > dmin) ? d : 1.0;
            }
            const double invd = fast_rcp1(d);
            const bool piv = LANE_IS((lane & 15) == J);           // l16 == J as a constant lane mask: no compare per pivot
            const double nf = piv ? 0.0 : -(a[J] * invd);
            myinv = piv ? invd : myinv;
            dpp_fmac_self<J + 1, N - 1 - J, J>(a, nf);
            dpp_fmac_self<0, M, J>(b, nf);
        }
        gj16_step<J + 1, N, M, GUARD>(a, b, live, l16, rowon, dmin, bad, myinv);
    }
}
// Lane l holds row l & 15 of the system (rows >= N: any finite copy, e.g. row 0 -- they are eliminated like every other row and never read):
// all four 16-lane DPP rows then run the same elimination.  The right-hand sides need not be the same in every DPP row: b[r] is updated
// from the lane-J entry of its own row only, so a caller can give each DPP row its own slice of the columns (M per row) and every column
// sees the same fused multiply-adds in the same order as in a full copy.  On exit b[r] of lane i < N holds x_i.  Returns non-zero
// (wave-uniform) if a pivot was not positive (d_i > 0 <=> 0 < 1 / d_i < inf on the lane that kept it; the caller flags LMH_FLAG_NOT_SPD,
// and the non-finite values that follow a bad pivot are flagged LMH_FLAG_NONFINITE by the evaluation's own check).
template <int N, int M>
__device__ __forceinline__ int gj_solve_regs(double (&a)[N], double (&b)[M], unsigned live)
{
    static_assert(N <= 16, "one DPP row");
    const int l16 = LANE & 15;                                     // (what gj16_step's pivot masks assume)
    int bad = 0;
    double myinv = 0.0;
    gj16_step<0, N, M, false>(a, b, live, l16, true, 0.0, bad, myinv);
#pragma unroll
    for (int r = 0; r < M; r++) b[r] *= myinv;
    const bool pivot_lane = ((live >> l16) & 1u) != 0u;            // (bits >= N of `live` are clear)
    return (__ballot(pivot_lane && !(myinv > 0.0 && myinv <= 1.7976931348623157e308)) != 0ull) ? 1 : 0;
}

#endif
