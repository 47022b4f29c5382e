// lmh_device.h -- parameter block shared by the host launcher and the gfx950 kernels.
#pragma once
#include <stdint.h>

#define LMH_MODEL_STRIDE 400  // per model: 28 x 14 doubles (Ibar 9 | m*c 3 | m | Robot::desiredPosture of coordinate i, the record's spare slot) + [392] total mass
#define LMH_BODY_STRIDE 14
#define LMH_SEG_STRIDE 52
#define LMH_PARAM_STRIDE 20   // one per-robot parameter record (include/lmh.h, lmh_set_params)
#define LMH_GCOL_STRIDE 228   // one friction table: generators [16][6] | (G G')^-1 [6][6] | G'(G G')^-1 [16][6]
#define LMH_PUSH_STRIDE 32    // one velocity push: tick (as a double) | dv[30] | pad (include/lmh.h, lmh_set_pushes)
#define LMH_ROLLOUT_THREADS 128   // fused rollout: two waves per robot (lmh_kernels.hip, bsync)

// ---- predicates of the lane id alone, as constant lane masks.  In the 64-lane kernels (lane = threadIdx.x & 63) a condition such as
// lane < 30 or (lane & 15) < 6 is a compile-time 64-bit constant: LANE_IS(expr) evaluates `expr` for lane = 0 .. 63 while compiling and
// hands the mask to the wave as a lane predicate -- two scalar moves where it is used, instead of a vector compare (plus the integer work
// that formed its operand) on the wave that carries the critical path, and nothing to keep alive in an SGPR pair across a phase.  The
// lambda captures nothing, so an `expr` that mentions anything but `lane`, literals, enumerators and constexpr values does not compile:
// a predicate with a run-time factor keeps that factor outside the macro (LANE_IS(lane < 12) && ((F >> l16) & 1)).
// -DLMH_LANE_RUNTIME (the `lanert` checker build): the same expression evaluated at run time on the kernel's LANE, the form the masks
// replaced -- tests/test_gpu_lane_masks.py holds the two libraries to the same bytes.
template <class F>
constexpr uint64_t lane_mask_of(F f)
{
    uint64_t m = 0;
    for (int l = 0; l < 64; l++) m |= f(l) ? (uint64_t)1 << l : (uint64_t)0;
    return m;
}
#ifdef LMH_LANE_RUNTIME
#define LANE_IS(expr) ([](int lane) -> bool { return (expr); }(LANE))
#else
#define LANE_IS(expr) ({ constexpr uint64_t lane_mask_ = lane_mask_of([](int lane) constexpr -> bool { return (expr); }); \
                         __builtin_amdgcn_inverse_ballot_w64(lane_mask_); })
#endif
static_assert(lane_mask_of([](int lane) constexpr -> bool { return lane < 30; }) == 0x3FFFFFFFull, "lane < 30");
static_assert(lane_mask_of([](int lane) constexpr -> bool { return (lane & 15) == 3; }) == 0x0008000800080008ull, "(lane & 15) == 3");
static_assert(lane_mask_of([](int lane) constexpr -> bool { return (lane >> 4) < 2; }) == 0x00000000FFFFFFFFull, "lane >> 4 < 2");
static_assert(lane_mask_of([](int lane) constexpr -> bool { return lane >= 30 && lane < 36; }) == 0x0000000FC0000000ull, "30 <= lane < 36");
static_assert(lane_mask_of([](int lane) constexpr -> bool { return lane < 0; }) == 0ull && lane_mask_of([](int lane) constexpr -> bool { return lane < 64; }) == ~0ull, "empty and full");

struct LmhIkTarget { double v[16]; };   // rF(6) | lF(6) | com(3) | pad: passed by value in the IK kernel's arguments

struct LmhDevParams {
    // ---- device buffers
    const double *model;        // [n_models][LMH_MODEL_STRIDE]
    const double *mpc;          // [n_gain][mpc_stride]: K(N+1) | Px0(N+1) | Px1(N+1) | zcom | D = -zcom / gravity (the lmh_mpc_* kernels) | pad(2)
    const double *zmpx;         // [n_samples]
    const double *zmpy;
    const uint8_t *phase;       // [n_samples] or nullptr
    const double *gcol;         // [16][6] friction-cone generators of one foot | (G G')^-1 | G'(G G')^-1
    const double *segs;         // [n_seg][LMH_SEG_STRIDE] walking segments: t0 | rF[3][8] | lF[3][8] | pad, or nullptr
    const uint16_t *seg_of_sample; // [n_samples] segment of preview index k
    const double *xscale;       // [n_instances] per-instance scale of ZMP x and x-axis foot polynomials, or nullptr
    const double *pushes;       // [n_sets][n_push][LMH_PUSH_STRIDE] timed velocity pushes (lmh_rollout, lmh_rollout_zoh_ex), or nullptr while n_push = 0
    const double *lcoef;        // [336][3] local-transform coefficients of the forward kinematics (build_lcoef): one table per handle
    const LmhDevParams *inst_blocks;   // per-robot parameters (lmh_set_params): [n_instances] whole blocks, block i = this block with robot i's 19
                                // scalars, the five inv_w_* and gcol -> robot i's friction table (lmh_params_expand_kernel); nullptr = this block
                                // serves every robot.  The controller kernels pick the robot's block once and read everything through it
    int32_t model_stride;       // 0 = shared model
    int32_t mpc_stride_inst;    // 0 = shared gain row
    int32_t mpc_stride;         // 3*(N+1)+4
    int32_t n_samples;
    int32_t n_seg;
    int32_t horizon;            // N
    int32_t n_instances;
    int32_t warm_start;
    int32_t max_qp_iters;
    int32_t precision;          // 0: fp64 throughout; 1: mixed (fp32 model terms, fp64 references + QP); 2: fp32
    int32_t bpp_max;            // block-pivoting rounds before the Lawson-Hanson pass (< 0: Lawson-Hanson only)
    int32_t plant;              // 1: compliant-contact plant driven by the torques (lmh_config.plant)
    int32_t ref_stride;         // per-robot plans: samples per robot in zmpx / zmpy / phase / seg_of_sample (= n_samples); 0 = one shared plan
    int32_t seg_stride;         // per-robot plans: segment records per robot in segs (= n_seg); 0 = shared
    int32_t push_stride;        // push records per robot in pushes (= n_push); 0 = one schedule shared by all robots
    int32_t n_push;             // push records per schedule (<= LMH_MAX_PUSHES); 0 = no schedule
    // ---- scalars (reference literals, see include/lmh.h lmh_config)
    double dt;                  // control step (RK4 step of the fused rollout, Clock::step)
    double mpc_dt;              // MPC sample time: k = int(t / mpc_dt), sample period of the reference arrays (lmh_config.mpc_dt; = dt when that is 0)
    double kp_joints, kd_joints, kp_mom, kd_mom, kp_feet, kd_feet;
    double w_com_lin, w_com_ang, w_base_pos, w_base_ang, w_joints, w_force, w_foot;
    double eps_coeff;
    double inv_w_base_pos, inv_w_base_ang, inv_w_joints, inv_w_com_lin, inv_w_foot;   // 1.0 / weight, divided once on the host (the same IEEE quotient the kernels used to form per evaluation)
    double contact_k, contact_d, contact_dt, contact_mu;
    double a00, a01, a10, a11, b0, b1;   // LIPM A, B (mpcLinearPendulum.cpp:45-47)
    // ---- foot reference polynomials (shared), ascending powers
    double rF[3][8];
    double lF[3][8];
    int32_t rFn[3];
    int32_t lFn[3];
};

// lmh_rollout_zoh_ex (include/lmh.h, lmh_zoh_opts): what the launch takes beyond lmh_rollout_zoh's own arguments, by value in the kernel arguments
struct LmhZohEx {
    double *trace;              // [n_ticks / trace_every][n_instances][LMH_TRACE_STRIDE], or nullptr
    double *metrics;            // [n_instances][LMH_METRICS_STRIDE], or nullptr
    int32_t trace_every;        // control ticks per sample (> 0 whenever trace is there)
    int32_t wrench_per_tick;    // 1: base_wrench is [n_ticks][n_instances][6]
    int32_t pushes;             // 1: the block's push schedule is applied, ticks counted in plant substeps (n_ticks * n_substeps < 2^30 - 1)
    int32_t pad;
};

// lmh_rollout_zoh_box (include/lmh.h): what the launch takes beyond lmh_rollout_zoh_ex's -- lmh_mpc_box_step's bounds and weights, where the samples go.
// prepare: nothing is launched; the kernel's dynamic shared memory limit is set on the current device for the largest horizon and the runtime's
// answer (a hipError_t) is stored through `answer`.  Once per handle, when it is created: never inside the call, which is captured into graphs.
struct LmhZohBox {
    const double *box;          // the robot's [4][n_samples] bounds at box + box_stride * robot (box_stride 0: one shared set)
    size_t box_stride;
    double *mpc;                // [n_ticks][n_instances][LMH_MPC_STRIDE], or nullptr
    double alpha, beta;         // the preview problem's weights (lmh_config)
    int32_t prepare;
    int32_t *answer;
};

// lmh_rollout_zoh_io (include/lmh.h, lmh_zoh_io): what the launch takes beyond lmh_rollout_zoh_ex's -- what the controller measures and what the
// plant receives.  act: the handle's lmh_set_actuators table, the robot's record at act + act_stride * robot (act_stride 0: one shared record);
// nullptr with actuators = 1: the defaults (no limit, no lag, no delay).
struct LmhZohIo {
    const double *meas;         // [n_ticks][n_instances][60], or nullptr
    double *act_mem;            // [n_instances][LMH_ACT_MEM_STRIDE]; read and written with actuators = 1 only
    double *applied;            // [n_ticks][n_instances][24], or nullptr
    const double *act;
    size_t act_stride;
    int32_t actuators;
    int32_t pad;
};

// lmh_rollout_zoh_servo (include/lmh.h): what the launch takes beyond lmh_rollout_zoh_io's -- the handle's servo table (servo NULL: zero gains;
// servo_stride 0: one shared record) and, with mode LMH_SERVO_CALLER, the caller's setpoints.  mode is never 0 here: that is the launch without.
struct LmhZohServo {
    const double *setpoint;     // [n_ticks][n_instances][LMH_SETPOINT_STRIDE] with LMH_SERVO_CALLER, else nullptr
    const double *servo;        // [n_sets][LMH_SERVO_STRIDE], or nullptr
    size_t servo_stride;
    int32_t mode;               // LMH_SERVO_INTEGRATE | LMH_SERVO_CALLER
    int32_t pad;
};

// lmh_rollout_zoh_rigid (include/lmh.h, lmh_zoh_rigid): what the launch takes beyond lmh_rollout_zoh_io's -- which soles every control tick's hold
// keeps and where its multipliers go.  source is never 0 here: that is the launch without.
struct LmhZohRigid {
    const int32_t *mode;        // LMH_RIGID_FIXED: [n_instances] or nullptr (both soles); LMH_RIGID_PER_TICK: [n_ticks][n_instances]; LMH_RIGID_PLAN: nullptr
    double *lambda;             // [n_ticks][n_instances][12], or nullptr
    double kv;                  // plant_derivative_rigid's velocity-level stabilisation
    int32_t source;             // LMH_RIGID_FIXED | LMH_RIGID_PER_TICK | LMH_RIGID_PLAN
    int32_t pad;
};

// lmh_rollout_zoh_rigid_impact (include/lmh.h, lmh_zoh_impact): what the launch takes beyond lmh_rollout_zoh_rigid's -- the mode of the hold before
// each robot's next one, and where the impulses go.  Passed with enable = 1 only: without it the launch is lmh_rollout_zoh_rigid's.
struct LmhZohImpact {
    int32_t *mode_prev;         // [n_instances], read and written once per control tick by the robot's own wave 0
    double *impulse;            // [n_ticks][n_instances][12], or nullptr
};

// walking-plan generator (lmh_gen_walk): arguments of the device kernel
#define LMH_GEN_MAX_STEPS 1022
struct LmhWalkSpec {
    double time_step, time_per_step, ds_time, step_height, settle_time, foot_y;
    int32_t n_samples, num_steps, first_support, pad;
};
struct LmhJumpSpec { double stance_time, flight_time; };   // lmh_gen_jump_batch: one robot's schedule
