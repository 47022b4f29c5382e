// lmh_launch.h -- the seam between the host layer (lmh_capi.hip) and the kernels (lmh_kernels.hip, lmh_mpc.hip): every kernel launcher and the two
// lmh_debug_* diagnostics, declared once.  All three files include it, so a definition that disagrees with its declaration does not compile.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "lmh_device.h"

enum { TM_TERMS, TM_INVDYN, TM_FWDDYN };    // lmh_launch_terms: the dense terms record | inverse dynamics | forward dynamics (lmh_terms_kernel)
enum { PM_CONTACT, PM_DERIV, PM_STEP,       // lmh_launch_plant: contact wrench | derivative | RK4 step (lmh_plant_kernel)
       PM_RIGID_DERIV, PM_RIGID_STEP,       //                   derivative | RK4 step of the rigid-contact plant (lmh_plant_kernel's RIGID instantiations)
       PM_RIGID_IMPACT };                   //                   its plastic impact (lmh_plant_impact_rigid)

extern "C" void lmh_launch_model(const double *raw, double *model, int n_models, const double *lcoef, hipStream_t s);
extern "C" void lmh_launch_params_expand(const LmhDevParams *P, const double *d_rec, const double *d_gcol_tab, LmhDevParams *d_blocks, int n, hipStream_t s);
extern "C" void lmh_launch_gen_walk(const LmhWalkSpec *W, double *zx, double *zy, uint8_t *phase, double *segs, uint16_t *sos, hipStream_t s);
extern "C" void lmh_launch_gen_jump(int n, double time_step, double stance_time, double flight_time, double *zx, double *zy, uint8_t *phase, hipStream_t s);
// d_specs: DEVICE [n_plans], each with n_samples set to the shared grid; seg_stride: segment records per robot
extern "C" void lmh_launch_gen_walk_batch(const LmhWalkSpec *d_specs, int n_plans, int seg_stride, double *zx, double *zy, uint8_t *phase, double *segs, uint16_t *sos, hipStream_t s);
extern "C" void lmh_launch_gen_jump_batch(int n, double time_step, const LmhJumpSpec *d_specs, int n_plans, double *zx, double *zy, uint8_t *phase, hipStream_t s);
// ref (lmh_eval_ref, lmh_rollout_zoh_ref): NULL = the built-in CoM reference of lmh_eval / lmh_rollout_zoh; otherwise the caller's CoM references,
// [B][LMH_MPC_STRIDE] for the evaluation (never with `debug`) and [n_ticks][B][LMH_MPC_STRIDE] for the closed loop
extern "C" void lmh_launch_eval(const LmhDevParams *P, double *state, double *out, int32_t *status, double *debug, const double *ref, hipStream_t s);
// d_P: device copy of *P (the rollout kernel reads its parameters through a pointer, see lmh_rollout_kernel)
// d_ticket: zero-initialised device memory owned by this launch until it completes (work-unit counters, ring, progress: see the kernel)
// trace, trace_every: the samples of lmh_rollout_trace, NULL and 0 = none; metrics: the records of lmh_rollout_metrics, NULL = none; never both
extern "C" void lmh_launch_rollout(const LmhDevParams *P, const LmhDevParams *d_P, int *d_ticket, double *state, double *out, int32_t *status, double *log, int n_ticks,
                                   double *trace, int trace_every, double *metrics, hipStream_t s);
// One launch of one kernel of the zero-order-hold family, all instantiations of one body (lmh_rollout_zoh_ex_body); the later option in this list wins:
// ex (lmh_rollout_zoh_ex): lmh_rollout_zoh_ex_kernel with these options (base_wrench is then [n_ticks][B][6] when ex->wrench_per_tick); NULL = none of them,
// which is lmh_rollout_zoh / lmh_rollout_zoh_ref: the same kernel with an all-zero record.
// bx (lmh_rollout_zoh_box; ex is then never NULL and ref is): NULL = not that call; otherwise lmh_rollout_zoh_box_kernel, the loop with lmh_mpc_box_step at
// the measured CoM state inside every evaluation -- or, with bx->prepare, no launch at all (LmhZohBox, lmh_device.h).  The same launcher, not a new symbol: the
// stand-alone host programs under tests/host link lmh_capi.hip against one stub per launcher.
// io (lmh_rollout_zoh_io; ex is then never NULL and bx is): NULL = not that call; otherwise lmh_rollout_zoh_io_kernel, the loop with a measurement added to
// what the evaluation reads and an actuator in front of the hold (LmhZohIo, lmh_device.h).
// ground (lmh_set_ground; bx is then NULL): NULL = the flat ground; otherwise ground + ground_stride * robot is that robot's LMH_GROUND_STRIDE words
// (ground_stride 0: one shared record) and the launch is lmh_rollout_zoh_ground_kernel's whatever ex and io ask for (either may be NULL = nothing).
// sv (lmh_rollout_zoh_servo; bx is then NULL, ex, io and ground may each be NULL): NULL = no servo; otherwise lmh_rollout_zoh_servo_kernel, the IO body
// with the joint servo inside every hold (LmhZohServo, lmh_device.h).
// rg (lmh_rollout_zoh_rigid; bx, ground and sv are then NULL, ex and io may each be NULL): NULL = not that call; otherwise lmh_rollout_zoh_rigid_kernel, the IO
// body with the rigid-contact plant in every hold (LmhZohRigid, lmh_device.h).
// im (lmh_rollout_zoh_rigid_impact with enable = 1; rg is then never NULL): NULL = not that call; otherwise lmh_rollout_zoh_rigid_impact_kernel, the rigid
// kernel's body with the plastic impact in front of every hold that holds a foot more than the hold before it (LmhZohImpact, lmh_device.h).
extern "C" void lmh_launch_rollout_zoh(const LmhDevParams *P, double *state, double *out, int32_t *status, const double *base_wrench, double *log, const double *ref, int n_ticks, int n_substeps,
                                       const LmhZohEx *ex, const LmhZohBox *bx, const LmhZohIo *io, const double *ground, size_t ground_stride, const LmhZohServo *sv, const LmhZohRigid *rg,
                                       const LmhZohImpact *im, hipStream_t s);
extern "C" void lmh_launch_metrics_reset(double *metrics, int n_instances, double z_min, double tilt_max, hipStream_t s);
extern "C" void lmh_launch_summary(int n, const double *state, const double *out, const int32_t *status, double *summary, hipStream_t s);
extern "C" void lmh_launch_com(const LmhDevParams *P, const double *q, double *com, hipStream_t s);
extern "C" void lmh_launch_ik(const LmhDevParams *P, double *q, const LmhIkTarget *target, int32_t *iters, hipStream_t s);
extern "C" void lmh_launch_ik_batch(const LmhDevParams *P, const double *q_start, const double *targets, int n_targets, double *q, int32_t *iters, double *crit, hipStream_t s);
extern "C" void lmh_launch_terms(const LmhDevParams *P, int mode, const double *q, const double *v, const double *x, const double *w, double *res, int32_t *flags, hipStream_t s);
// One launch of one instantiation of lmh_plant_kernel<MODE, GROUND, SERVO, RIGID>:
// ground, ground_stride: as in lmh_launch_rollout_zoh; NULL = the flat ground, otherwise the GROUND instantiation of the mode
// setpoint (lmh_plant_step_servo; PM_STEP only): NULL = no servo; otherwise [n_instances][LMH_SETPOINT_STRIDE] and the launch is the SERVO instantiation's,
// with servo + servo_stride * robot that robot's LMH_SERVO_STRIDE gains (servo NULL: zero gains; stride 0: one shared record)
// PM_RIGID_DERIV, PM_RIGID_STEP (lmh_plant_derivative_rigid, lmh_plant_step_rigid): the RIGID instantiations with hold ([n_instances] support modes, NULL = both
// soles held), kv and lambda ([n_instances][12], may be NULL); ground, servo and setpoint are not read.  The other modes read none of the three.  The same
// launcher, not a new symbol, for the reason given at lmh_launch_rollout_zoh.
// PM_RIGID_IMPACT (lmh_plant_impact_rigid): the RIGID instantiation that runs plant_impact_rigid at (q, v) under hold; xdot takes v_plus
// ([n_instances][30]) and lambda the impulse ([n_instances][12], may be NULL); tau30, state, contact, n_substeps and kv are not read.
extern "C" void lmh_launch_plant(const LmhDevParams *P, int mode, const double *q, const double *v, const double *tau30, double *state, double *xdot, double *contact, int32_t *flags,
                                 int n_substeps, const double *ground, size_t ground_stride, const double *servo, size_t servo_stride, const double *setpoint, const int32_t *hold, double kv,
                                 double *lambda, hipStream_t s);
// The three MPC launchers carry the box-constrained variants (lmh_mpc_box_*): box NULL = the unconstrained kernels exactly as they are (alpha, beta and
// box_stride are then not read by step and rollout); otherwise box + box_stride * robot is that robot's [4][n_samples] bounds (box_stride 0: one shared set)
// and `mpc` / `traj` / `record` take the constrained call's records (record: LMH_MPC_BOX_STRIDE words per robot instead of LMH_MPC_PREVIEW_STRIDE).
extern "C" void lmh_launch_mpc_step(const LmhDevParams *P, double alpha, double beta, const double *lip, const double *box, size_t box_stride, double *mpc, hipStream_t s);
extern "C" void lmh_launch_mpc_rollout(const LmhDevParams *P, double alpha, double beta, double *lip, const double *box, size_t box_stride, int n_ticks, double *traj, hipStream_t s);
extern "C" void lmh_launch_mpc_preview(const LmhDevParams *P, double alpha, double beta, const double *lip, const double *box, size_t box_stride, double *record, hipStream_t s);
// Diagnostics exported beside the C ABI of include/lmh.h, not part of it (capi.DEBUG_PROTOTYPES binds them): see their definitions
extern "C" int lmh_debug_rollout_occupancy(int *groups_per_cu, int *num_regs, int *static_lds_bytes);
extern "C" int lmh_debug_build_flags(void);
