// Test harness of LANE_IS (csrc/lmh_device.h): one kernel that evaluates a list of lane-only predicates taken from lmh_kernels.hip twice per
// thread -- as the constant lane mask LANE_IS forms at compile time and as the plain expression at run time -- so that
// tests/test_gpu_lane_masks.py can hold the two to each other and to numpy's evaluation.  Test infrastructure: built into
// liblmh_lane_mask_harness.so (build.build_lane_mask_harness), never part of liblmh_hip.so.
//
// One block of 128 threads (two waves, as the rollout kernel's workgroup): thread t writes out[2 p][t] (mask form) and out[2 p + 1][t]
// (run-time form) of predicate p, one int each, at addresses formed from threadIdx and compile-time constants alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define LANE ((int)(threadIdx.x & 63))
#include "lmh_device.h"

// the lane maps of phase_com_x and phase_fk (division by multiplication, exact on their ranges), as functions of the lane id
constexpr int h_ln(int lane) { return lane < 62 ? lane : 62; }                       // phase_com_x: lane 63 repeats lane 62
constexpr int h_fr(int lane) { return (h_ln(lane) * 57) >> 9; }                      // ln / 9
constexpr int h_e9(int lane) { return h_ln(lane) - 9 * h_fr(lane); }                 // ln % 9
constexpr int h_col(int lane) { return h_e9(lane) - 3 * ((h_e9(lane) * 11) >> 5); }  // e9 % 3
constexpr int h_fr3(int lane) { return (h_ln(lane) * 43) >> 7; }                     // ln / 3
constexpr int h_l60(int lane) { return lane < 60 ? lane : lane - 60; }               // phase_fk: lanes 60..63 repeat lanes 0..3
constexpr int h_lfr(int lane) { return (h_l60(lane) * 43) >> 9; }                    // l60 / 12
constexpr int h_lel(int lane) { return h_l60(lane) - 12 * h_lfr(lane); }             // l60 % 12
constexpr int h_dup(int lane) { return (int)((0x5210543210543210ull >> (4 * (lane & 15))) & 15ull); }     // tree_dup: component of a lane

// (index, expression): tests/test_gpu_lane_masks.py keeps the same list for numpy
#define LANE_PREDICATES(X) \
    X(0, lane < 30) \
    X(1, lane >= 30 && lane < 36) \
    X(2, (lane & 15) < 6) \
    X(3, (lane & 15) == 3) \
    X(4, (lane >> 4) < 2) \
    X(5, (lane >> 4) == 2 && (lane & 3) == 2) \
    X(6, h_col(lane) == 1) \
    X(7, h_fr(lane) < 3) \
    X(8, h_fr3(lane) < 14) \
    X(9, h_lel(lane) == 0 || h_lel(lane) == 5 || h_lel(lane) == 9) \
    X(10, h_lfr(lane) < 2) \
    X(11, h_dup(lane) == 2) \
    X(12, lane < 48 && (lane & 15) == 2 * (lane >> 4)) \
    X(13, lane == 0 || lane >= 30) \
    X(14, lane < 0) \
    X(15, lane < 64)
#define LANE_NPRED 16

extern "C" __global__ __launch_bounds__(128) void k_lane_masks(int *out)
{
    const int t = (int)threadIdx.x;
#define X(p, expr) { out[(2 * (p)) * 128 + t] = LANE_IS(expr) ? 1 : 0; const int lane = LANE; out[(2 * (p) + 1) * 128 + t] = (expr) ? 1 : 0; }
    LANE_PREDICATES(X)
#undef X
}

// out: [2 LANE_NPRED][128] ints on the device.  Returns the launch's hipError_t.
extern "C" int lane_mask_harness_run(int *out, void *stream)
{
    hipLaunchKernelGGL(k_lane_masks, dim3(1), dim3(128), 0, (hipStream_t)stream, out);
    return (int)hipGetLastError();
}
extern "C" int lane_mask_harness_npred(void) { return LANE_NPRED; }
