/*
 * lmh.h -- C ABI of the MI355X-native batched NAO whole-body controller
 *          (LIPM preview MPC -> whole-body QP -> rigid-body terms -> torques).
 *
 * This is the drop-in boundary for the per-tick hot path of Ema158/linearMpcHumanoid.
 * The reference has no FFI/plugin layer: its boundary is the C++ call surface used by
 * apps/offline/main.cpp.  Each entry point below names the reference interface it
 * replaces (paths relative to the reference root).  The C++ classes with the reference's
 * own names (Robot, Controller, Mpc3dLip, ZMP, ...) in
 * linearmpchumanoid_amd/csrc/shim/linearMpcHumanoid/ are thin wrappers over this ABI.
 *
 * All compute runs in hand-written HIP kernels (gfx950).  There is NO CPU fallback:
 * every call fails with LMH_ERR_NO_DEVICE if no HIP device is usable.
 *
 * Layouts (fp64, instance-major, contiguous):
 *   state  [B][LMH_STATE_STRIDE]  : q(30) | v(30) | v_prev(30) | t | pad(5)
 *       q = [p_base(3) world, rpy(3), qJ(24)], v = [v_lin(3), omega(3), qdJ(24)]
 *       (include/linearMpcHumanoid/controller/controller.hpp:20-31).
 *       v_prev is Robot::v_ as the previous Controller::standStep left it: the reference
 *       evaluates C, Cg and Jdot*qdot BEFORE it stores the new velocity
 *       (src/controller.cpp:56 vs :59), so those terms see the previous call's velocity.
 *   out    [B][LMH_OUT_STRIDE]    : tau(24) | f(12: n_R f_R n_L f_L) | qdd(30) | CoM(3) | comVel(3) |
 *                                   xRef(3) | yRef(3) | pad(2)
 *       (WBCOutput, controller.hpp:43-48; Robot::getCoM/getComVel; Mpc3dLip::getXRef/getYRef)
 *   status [B][LMH_STATUS_STRIDE] int32 : k | qp_iterations | flags | active_mask
 *       k = int(t/mpc_dt) of the last evaluation (src/mpcLinearPendulum.cpp:92), bit-exact.
 */
#ifndef LMH_H
#define LMH_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LMH_NQ 30
#define LMH_NJ 24
#define LMH_NFRAMES 28
#define LMH_STATE_STRIDE 96
#define LMH_OUT_STRIDE 80
#define LMH_STATUS_STRIDE 4
#define LMH_LINK_STRIDE 13        /* mass | com(3) | inertia(9 row-major), linkInertia.hpp:4-9 */
#define LMH_MAX_HORIZON 64
#define LMH_DEBUG_STRIDE 4096
#define LMH_SEG_STRIDE 52
#define LMH_PUSH_STRIDE 32        /* one timed velocity push: tick (as a double) | dv[30] | pad, see lmh_set_pushes */
#define LMH_MAX_PUSHES 16         /* push records per robot */
#define LMH_IK_TARGET_STRIDE 16   /* one inverse-kinematics target record: rf6 (x y z | roll pitch yaw) | lf6 | com(3) | pad, see lmh_ik_batch */
#define LMH_PARAM_STRIDE 20       /* one per-robot parameter record, see lmh_set_params */
/* offsets into one parameter record (doubles, in lmh_config's own order) */
#define LMH_PARAM_OFF_MU 0
#define LMH_PARAM_OFF_KP_JOINTS 1
#define LMH_PARAM_OFF_KD_JOINTS 2
#define LMH_PARAM_OFF_KP_MOM 3
#define LMH_PARAM_OFF_KD_MOM 4
#define LMH_PARAM_OFF_KP_FEET 5
#define LMH_PARAM_OFF_KD_FEET 6
#define LMH_PARAM_OFF_W_COM_LIN 7
#define LMH_PARAM_OFF_W_COM_ANG 8
#define LMH_PARAM_OFF_W_BASE_POS 9
#define LMH_PARAM_OFF_W_BASE_ANG 10
#define LMH_PARAM_OFF_W_JOINTS 11
#define LMH_PARAM_OFF_W_FORCE 12
#define LMH_PARAM_OFF_W_FOOT 13
#define LMH_PARAM_OFF_EPS_COEFF 14
#define LMH_PARAM_OFF_CONTACT_K 15
#define LMH_PARAM_OFF_CONTACT_D 16
#define LMH_PARAM_OFF_CONTACT_DT 17
#define LMH_PARAM_OFF_CONTACT_MU 18   /* [19] pad */
#define LMH_TRACE_STRIDE 180      /* one trace sample: state(96) | out(80) | status(4, as doubles), see lmh_rollout_trace */
#define LMH_METRICS_STRIDE 208     /* one per-robot metrics record, see lmh_rollout_metrics */
/* offsets into one metrics record (doubles) */
#define LMH_METRICS_OFF_COUNT       0   /* ticks accumulated since the reset (a whole number in a double) */
#define LMH_METRICS_OFF_FIRST_FLAG  1   /* COUNT before the first accumulated tick at whose end (launch-cumulative flags & 15) != 0; -1: none */
#define LMH_METRICS_OFF_FIRST_FALL  2   /* COUNT before the first accumulated tick at whose end the robot is "down" (lmh_rollout_metrics); -1: none */
#define LMH_METRICS_OFF_Z_MIN       3   /* threshold: written by the reset (or the caller), read by the kernel, never written by a rollout */
#define LMH_METRICS_OFF_TILT_MAX    4   /* threshold, same rule; [5, 8) pad, zero */
#define LMH_METRICS_OFF_XMIN        8   /* [60] min of every state component q | v at the end of a tick */
#define LMH_METRICS_OFF_XMAX       68   /* [60] max */
#define LMH_METRICS_OFF_WMIN      128   /* [12] min of the k4 contact wrench n_R f_R n_L f_L (out.f, the log's words) */
#define LMH_METRICS_OFF_WMAX      140   /* [12] max */
#define LMH_METRICS_OFF_TAU_MAXABS 152  /* [24] max |tau_j| of the k4 torques */
#define LMH_METRICS_OFF_TAU_SQ    176   /* [24] sum of tau_j^2 (times dt: the effort integral) */
#define LMH_METRICS_OFF_ERR_MAXABS 200  /* [2] max |CoM_x - xRef[0]|, max |CoM_y - yRef[0]| (out[66] - out[72], out[67] - out[75]) */
#define LMH_METRICS_OFF_ERR_SQ    202   /* [2] sums of their squares; [204, 208) pad, zero */
#define LMH_TERMS_STRIDE 1840     /* one rigid-body terms record, see lmh_terms */
/* offsets into one terms record (doubles, every array row-major) */
#define LMH_TERMS_OFF_M 0         /* [30][30] mass matrix, structural zeros written (Dynamics::getM) */
#define LMH_TERMS_OFF_C 900       /* [30] Coriolis / centrifugal / gravity vector (getC) */
#define LMH_TERMS_OFF_CG 930      /* [6] base rows of the same vector without gravity (getCg; the rows the controller reads) */
#define LMH_TERMS_OFF_AG 936      /* [6][30] centroidal momentum matrix, angular rows first (getAG) */
#define LMH_TERMS_OFF_AGPQP 1116  /* [6] its velocity product AGdot qdot (getAGpqp) */
#define LMH_TERMS_OFF_J 1122      /* [12][30] feet Jacobian, rows n_R f_R n_L f_L like out.f (Kinematics::feetJacobian) */
#define LMH_TERMS_OFF_JPQP 1482   /* [12] Jdot qdot of the soles (getJpqp) */
#define LMH_TERMS_OFF_COM 1494    /* [3] Robot::getCoM */
#define LMH_TERMS_OFF_COMVEL 1497 /* [3] Robot::getComVel */
#define LMH_TERMS_OFF_ANGMOM 1500 /* [3] Robot::getComAngMom */
#define LMH_TERMS_OFF_MASS 1503   /* Robot::getMass of the robot's model */
#define LMH_TERMS_OFF_T 1504      /* [28][3][4] world transform of every frame, rows 0..2 of Robot::getT (row 3 is 0 0 0 1) */
#define LMH_CONTACT_STRIDE 40     /* one contact record, see lmh_contact_wrench */
/* offsets into one contact record (doubles) */
#define LMH_CONTACT_OFF_W 0       /* [12] contact wrench n_R f_R n_L f_L about the sole origins, world axes, like out.f */
#define LMH_CONTACT_OFF_VF 12     /* [8][3] force at every sole vertex, foot-major (right foot first), vertices in the order of Robot.cpp:38-42 */
#define LMH_CONTACT_OFF_PAD 36    /* [4] zero */
#define LMH_GROUND_STRIDE 8       /* one ground record n_R(3) | h_R | n_L(3) | h_L, see lmh_set_ground */
/* offsets into one ground record (doubles) */
#define LMH_GROUND_OFF_N_R 0      /* [3] unit normal of the plane under the right foot, world axes */
#define LMH_GROUND_OFF_H_R 3      /* its offset along the normal, metres: the ground is n.x <= h */
#define LMH_GROUND_OFF_N_L 4      /* [3] the same under the left foot */
#define LMH_GROUND_OFF_H_L 7
#define LMH_LIP_STRIDE 8          /* the reduced (LIPM) state of one robot, see lmh_mpc_step */
/* offsets into one LIP state record (doubles) */
#define LMH_LIP_OFF_X 0           /* CoM x */
#define LMH_LIP_OFF_XDOT 1        /* CoM velocity x */
#define LMH_LIP_OFF_Y 2
#define LMH_LIP_OFF_YDOT 3
#define LMH_LIP_OFF_T 4           /* the robot's clock; [5, 8) pad */
#define LMH_MPC_STRIDE 16         /* one MPC sample, see lmh_mpc_step */
/* offsets into one MPC sample (doubles) */
#define LMH_MPC_OFF_XREF 0        /* [3] Mpc3dLip::getXRef: x_next, xdot_next, u_x */
#define LMH_MPC_OFF_YREF 3        /* [3] Mpc3dLip::getYRef */
#define LMH_MPC_OFF_ZMP 6         /* [2] zmp_x, zmp_y = x_k + D u: the model's output row C x + D u, D = -z_com / gravity */
#define LMH_MPC_OFF_STATE 8       /* [4] the LIP state the sample was computed from: x, xdot, y, ydot */
#define LMH_MPC_OFF_T 12          /* its clock */
#define LMH_MPC_OFF_K 13          /* the preview index k = (int)(t / mpc_dt), as a double */
#define LMH_MPC_OFF_FLAGS 14      /* this sample's flags (LMH_FLAG_ZMP_RANGE, LMH_FLAG_NONFINITE), as a double; [15] zero */
#define LMH_MPC_OFF_ACTIVE 15     /* lmh_mpc_box_step / lmh_mpc_box_rollout only: the active samples of both axes, as a double */
#define LMH_MPC_PREVIEW_STRIDE 536 /* one horizon preview record, see lmh_mpc_preview: a header of 8, then eight arrays of 66 */
/* offsets into one preview record (doubles); of every array the entries beyond the count named are zero */
#define LMH_MPC_PREVIEW_OFF_K 0       /* the preview index, as a double */
#define LMH_MPC_PREVIEW_OFF_FLAGS 1   /* LMH_FLAG_ZMP_RANGE, LMH_FLAG_NOT_SPD, LMH_FLAG_NONFINITE, as a double */
#define LMH_MPC_PREVIEW_OFF_N 2       /* the horizon N, as a double; [3, 8) pad, zero */
#define LMH_MPC_PREVIEW_OFF_U_X 8     /* [N + 1] the unconstrained solution U = -H^-1 g, x axis */
#define LMH_MPC_PREVIEW_OFF_U_Y 74    /* [N + 1] */
#define LMH_MPC_PREVIEW_OFF_Z_X 140   /* [N + 1] the predicted ZMP Px x_k + Pu U */
#define LMH_MPC_PREVIEW_OFF_Z_Y 206   /* [N + 1] */
#define LMH_MPC_PREVIEW_OFF_C_X 272   /* [N + 2] the predicted CoM position: c_0 = x_k, c_{j+1} = A c_j + B u_j */
#define LMH_MPC_PREVIEW_OFF_CV_X 338  /* [N + 2] its velocity */
#define LMH_MPC_PREVIEW_OFF_C_Y 404   /* [N + 2] */
#define LMH_MPC_PREVIEW_OFF_CV_Y 470  /* [N + 2] */
#define LMH_MPC_BOX_STRIDE 668     /* one constrained preview record, see lmh_mpc_box_preview: the preview record, then two arrays of 66 */
/* the words a constrained preview record has beyond the LMH_MPC_PREVIEW_OFF_* layout (doubles; [7] stays zero) */
#define LMH_MPC_BOX_OFF_ROUNDS_X 3    /* exchange rounds taken in x, as a double */
#define LMH_MPC_BOX_OFF_ROUNDS_Y 4
#define LMH_MPC_BOX_OFF_ACTIVE_X 5    /* active samples in x, as a double */
#define LMH_MPC_BOX_OFF_ACTIVE_Y 6
#define LMH_MPC_BOX_OFF_LAM_X 536     /* [N + 1] multipliers of the x bounds: > 0 at an upper bound, < 0 at a lower one, 0 exactly at an inactive sample */
#define LMH_MPC_BOX_OFF_LAM_Y 602     /* [N + 1] */
/* the rows of one set of bounds d_box[set][4][n_samples], see lmh_mpc_box_preview */
#define LMH_BOX_LO_X 0
#define LMH_BOX_HI_X 1
#define LMH_BOX_LO_Y 2
#define LMH_BOX_HI_Y 3
/* exchange rounds per axis and solve before lmh_mpc_box_* give up with LMH_FLAG_QP_MAXITER and keep the last iterate: four times the largest
 * number of samples, twice what lets every sample of a window enter and leave its working set once (2 (N + 1)) */
#define LMH_MPC_BOX_MAX_ROUNDS 260

/* status flags */
#define LMH_FLAG_QP_MAXITER 1     /* active-set iteration cap hit (reference: "QP failed", controller.cpp:472-476) */
#define LMH_FLAG_NONFINITE 2      /* NaN/Inf in the solution (reference aborts, controller.cpp:448-466) */
#define LMH_FLAG_ZMP_RANGE 4      /* preview window [k, k+N] left the reference arrays */
#define LMH_FLAG_NOT_SPD 8        /* a Cholesky pivot was not positive */
#define LMH_FLAG_UNFINISHED 32    /* lmh_rollout only: a wait of the kernel's work queue ran out and this robot did not get all its ticks (its state / out
                                   * records are those of the last chunk it completed); the call reports LMH_ERR_UNFINISHED, see lmh_rollout */
#define LMH_FLAG_BOX_EMPTY 64      /* lmh_mpc_box_* only: a sample of the window has lo > hi or a NaN bound; the robot's results are NaN */
#define LMH_FLAG_QP_FP64_ROUTE 16 /* LMH_PRECISION_FP32 only, informational: a contact-force solve of this instance met a rank-deficient free set
                                   * (or the Lawson-Hanson pass) and went the fp64 general route -- that system (cond ~1e13) has no fp32 form */

/* support phase per preview sample (build-defined extension; reference: Task.hpp:9-13 SupportFoot) */
#define LMH_PHASE_DOUBLE 0
#define LMH_PHASE_RIGHT 1         /* right foot in support, left foot carries no force */
#define LMH_PHASE_LEFT 2
#define LMH_PHASE_FLIGHT 3

/* arithmetic of the model-term phases (BASELINE config 5 tolerance sweep; build-defined, the reference is fp64 only) */
#define LMH_PRECISION_FP64 0
#define LMH_PRECISION_MIXED 1
#define LMH_PRECISION_FP32 2      /* model terms AND the whole-body QP in fp32 (one fp64 residual refinement of the 12 x 12 contact solve) */
#define LMH_SUMMARY_WIDTH 16      /* end-of-run summary record (doubles per instance), see lmh_make_summary */

enum {
    LMH_OK = 0,
    LMH_ERR_NO_DEVICE = -1,
    LMH_ERR_BAD_ARG = -2,
    LMH_ERR_HIP = -3,
    LMH_ERR_NOT_READY = -4,
    LMH_ERR_UNFINISHED = -5       /* an earlier lmh_rollout on this handle left robots part-way (LMH_FLAG_UNFINISHED in their status records) */
};

/* Literals of the reference, gathered in one record (the reference has no config layer):
 * include/linearMpcHumanoid/controller/controller.hpp:80-124, mpcLinearPendulum.hpp:43-49,
 * src/controller.cpp:117, apps/offline/main.cpp:13-14,38-39. */
typedef struct lmh_config {
    double dt;             /* control step: Clock(timeStep, ...) of the caller (apps/offline/main.cpp:18), the RK4 step of lmh_rollout;
                              also the MPC sample time when mpc_dt == 0 (the reference's own app passes the same value to both)   */
    double time_horizon;   /* N = (int)(time_horizon / mpc_dt)  (mpcLinearPendulum.cpp:43)                                       */
    double z_com;          /* LIPM height: Mpc3dLip ctor argument (main.cpp:39)              */
    double gravity, alpha, beta;
    double mu;
    double kp_joints, kd_joints, kp_mom, kd_mom, kp_feet, kd_feet;
    double w_com_lin, w_com_ang, w_base_pos, w_base_ang, w_joints, w_force, w_foot;
    double eps_coeff;
    int32_t warm_start;    /* 1: start the active set from the previous evaluation's (same minimiser) */
    int32_t max_qp_iters;
    int32_t precision;     /* LMH_PRECISION_FP64 (reference arithmetic) | LMH_PRECISION_MIXED: model terms (kinematics, C, M, J) in
                              fp32 arithmetic, references + QP in fp64 | LMH_PRECISION_FP32: the QP too (Woodbury core, Schur
                              complement, push-through contact solves with one fp64 residual refinement; a rank-deficient contact set
                              falls back to the fp64 general route and raises LMH_FLAG_QP_FP64_ROUTE).  References, RK4 state and
                              k = int(t/dt) are fp64 in every mode */
    int32_t bpp_rounds;    /* block-principal-pivoting rounds of the contact-force QP before the Lawson-Hanson pass takes over:
                              0 = default (10); n > 0 = cap at n rounds; < 0 = skip block pivoting, solve by Lawson-Hanson from the
                              empty set (diagnostic: exercises the finite fall-back) */
    /* Build-defined plant.  plant = 0: the reference's closed loop, which integrates the controller's own acceleration
     * and throws the torques away (apps/offline/main.cpp:118-121).  plant = 1: the RK4 derivative is the forward dynamics
     * M qdd = S'tau + J'w_contact - C driven by the torques the WBC returns, with a spring-damper contact at the four vertices of each sole
     * (Robot.cpp:38-42) against the plane z = 0: normal force max(0, k d - c zdot) on penetration d, tangential force -c_t (xdot, ydot)
     * scaled back onto the friction disc mu f_n.  M, C, J are the terms the controller evaluated in the same call.  out.qdd then carries the
     * plant's acceleration.  (The reference's intended route, MuJoCo feedback, is commented out at apps/mujoco/main.cpp:115-122.) */
    int32_t plant;
    int32_t reserved;
    double contact_k;      /* normal stiffness per vertex [N/m]; the light distal links bound it for explicit RK4 (ankle inertia 1.4e-5 kg m^2) */
    double contact_d;      /* normal damping per vertex [N s/m]  */
    double contact_dt;     /* tangential damping per vertex [N s/m] */
    double contact_mu;     /* friction coefficient of the plant's ground */
    /* MPC sample time: the `dt` argument of Mpc3dLip(dt, timeHorizon, zCom) (apps/offline/main.cpp:39, mpcLinearPendulum.hpp:10-13) and the
     * `timeStep` of ZMP(task, simulationTime, timeStep, supportFoot) (main.cpp:21) -- the reference's caller picks them independently of the
     * Clock's step (main.cpp:18).  It sets k = int(t / mpc_dt) on the float-accumulated clock (mpcLinearPendulum.cpp:92), the LIPM A, B
     * (:45-47), the horizon N and the sample period of every reference array (ZMP x/y, support phase, segment index).
     * 0 (the default) = dt: one value for both, as apps/offline/main.cpp passes.  E.g. dt = 1e-3, mpc_dt = 1e-2, time_horizon = 0.32:
     * 1 kHz control with a 32 x 10 ms preview. */
    double mpc_dt;
} lmh_config;

typedef struct lmh_handle lmh_handle;

/* fills the reference literals; dt = 0.01, mpc_dt = 0 (= dt), time_horizon = 0.5, z_com = 0.26 */
void lmh_config_default(lmh_config *cfg);
const char *lmh_last_error(void);
int lmh_device_count(void);

/* replaces: Robot::Robot + Mpc3dLip::Mpc3dLip + Controller::Controller
 * (src/Robot.cpp:5-43, src/mpcLinearPendulum.cpp:10-76, src/controller.cpp:5-46) for
 * n_instances robots on HIP device `device`.  Loads the nominal NAO model and a constant
 * (stance) reference set covering `default_ref_samples` samples. */
int lmh_create(const lmh_config *cfg, int n_instances, int device, lmh_handle **out);
int lmh_destroy(lmh_handle *h);
int lmh_num_instances(const lmh_handle *h);
int lmh_horizon(const lmh_handle *h);

/* replaces: createNaoParameters (src/robotParameters.cpp:8-229) + the joint-frame
 * re-expression of Robot::Robot (src/Robot.cpp:14-22).  raw_links: HOST pointer,
 * [n_models][28][13] in the Aldebaran (world-aligned at q=0) convention; n_models is 1
 * (shared) or n_instances (domain randomisation).  NULL restores the nominal table. */
int lmh_set_model(lmh_handle *h, const double *raw_links, int n_models);
/* total mass per model, HOST out [n_models] (Robot::getMass) */
int lmh_get_mass(lmh_handle *h, double *mass);
/* nominal raw table (HOST out [28][13]) */
void lmh_nominal_links(double *raw_links);

/* replaces: ZMP::getZmpXRef/getZmpYRef arrays copied into Controller (src/zmpGeneration.cpp:39-60,
 * src/controller.cpp:14) + the support-phase extension.  HOST pointers, n_samples each;
 * phase may be NULL (all double support).
 * This and the seven other reference setters (lmh_set_refs_stance, lmh_set_segments, lmh_gen_walk, lmh_gen_jump, lmh_gen_walk_batch,
 * lmh_gen_jump_batch, lmh_set_plans) follow one rule: the arguments are checked first, the new plan is built in buffers of its own and
 * replaces the current one in a single step at the end.  A refused or failed call (bad argument, failed allocation, copy or generator
 * launch) leaves the handle on its previous plan, samples and segments, shared or per robot.  lmh_set_model, lmh_set_zcom and
 * lmh_set_xscale replace their tables the same way. */
int lmh_set_refs(lmh_handle *h, const double *zmp_x, const double *zmp_y, const uint8_t *phase, int n_samples);
/* replaces: ZMP::stanceZMP (src/zmpGeneration.cpp:39-60) with timeStep = mpc_dt; support_foot: 0 Right,1 Left,2 Double */
int lmh_set_refs_stance(lmh_handle *h, double simulation_time, int support_foot);
/* replaces: footCoeffTrajectory output copied into Controller (src/footRefTrajectory.cpp:4-47,
 * src/controller.cpp:15-16).  coeff: HOST [3][8] ascending powers, n: [3] counts. */
int lmh_set_foot_coeffs(lmh_handle *h, const double *r_coeff, const int32_t *r_n, const double *l_coeff, const int32_t *l_n);
/* Build-defined walking extension (the reference declares ZMP::walkZMP, zmpGeneration.hpp:22, but never
 * defines it; footCoeffTrajectory produces one polynomial set per step).  Piecewise foot references:
 * segment record = LMH_SEG_STRIDE doubles: t0 | rF[3][8] | lF[3][8] | pad(3), ascending powers, evaluated
 * at (t - t0); seg_of_sample[k] selects the segment from the preview index k.  HOST pointers;
 * n_seg = 0 restores the single polynomial set of lmh_set_foot_coeffs.  n_samples must be the current sample count and every
 * seg_of_sample entry < n_seg; a call refused for either reason (or for a NULL table) releases nothing: the segments in place stay. */
int lmh_set_segments(lmh_handle *h, const double *segs, int n_seg, const uint16_t *seg_of_sample, int n_samples);
/* Reference generators ON THE DEVICE (no host arrays are uploaded): the same plans as the host statement in
 * linearmpchumanoid_amd/trajectories.py.  lmh_gen_walk: ZMP(Task, numSteps, timePerStep, simulationTime) as the reference declares it
 * (zmpGeneration.hpp:15-19; walkZMP is never defined there) + one footCoeffTrajectory polynomial set per step
 * (footRefTrajectory.cpp:4-47, in closed form): settle_time of stance, then num_steps x [ds_time double support | single support],
 * first_support = LMH_PHASE_RIGHT or LMH_PHASE_LEFT, feet at y = -/+ foot_y; x in units of the step length (lmh_set_xscale).
 * Fills the ZMP / phase samples ((int)((simulation_time + 0.5) / mpc_dt) of them, as ZMP::stanceZMP counts; sample k <-> t = k mpc_dt)
 * and 2 num_steps + 2 segments.
 * lmh_gen_jump: stance references with LMH_PHASE_FLIGHT in [stance_time, stance_time + flight_time) (BASELINE config 5). */
int lmh_gen_walk(lmh_handle *h, double simulation_time, int num_steps, double time_per_step, double ds_time, double step_height,
                 double settle_time, int first_support, double foot_y);
int lmh_gen_jump(lmh_handle *h, double simulation_time, double stance_time, double flight_time);
/* Per-robot plans (build-defined): every robot of the handle walks / jumps on a schedule of its own.  The sample grid is
 * shared -- n_samples = (int)((simulation_time + 0.5) / mpc_dt) for every robot, as lmh_gen_walk counts; mpc_dt, the horizon and
 * simulation_time stay per handle -- and so is the stride of the segment table: n_seg = 2 max(num_steps) + 2 records per robot (what
 * lmh_num_segments then returns); a robot with fewer steps uses its first 2 num_steps + 2 records, the rest of its slice is zero and no
 * seg_of_sample entry of that robot points there.  Device layout: zmp_x, zmp_y, phase, seg_of_sample [n][n_samples], segs
 * [n][n_seg][LMH_SEG_STRIDE]; a robot reads its slice when its preview index moves, nothing else in an evaluation changes.
 * n must be n_instances.  A failed call leaves the handle on its previous plan (see lmh_set_refs).  On a handle of one robot a
 * per-robot plan IS the shared plan: lmh_plans_per_instance reports 0 there.
 * Every other reference setter (lmh_set_refs, lmh_set_refs_stance, lmh_set_segments, lmh_gen_walk, lmh_gen_jump) puts the handle back on
 * ONE shared plan (lmh_set_segments alone on a per-robot handle keeps robot 0's samples as the shared ones); lmh_set_xscale keeps its
 * meaning: robot i's x quantities are its own plan's times xscale[i]. */
typedef struct lmh_walk_spec {   /* one robot's arguments of lmh_gen_walk */
    double time_per_step, ds_time, step_height, settle_time, foot_y;
    int32_t num_steps, first_support;
} lmh_walk_spec;
typedef struct lmh_jump_spec { double stance_time, flight_time; } lmh_jump_spec;   /* one robot's arguments of lmh_gen_jump */
/* one plan per robot generated ON THE DEVICE (one workgroup per robot; no host arrays are uploaded).  specs: HOST [n].  Every spec is
 * checked by the rules of lmh_gen_walk / lmh_gen_jump; the error text names the first offending robot ("robot 7: ..."). */
int lmh_gen_walk_batch(lmh_handle *h, double simulation_time, const lmh_walk_spec *specs, int n);
int lmh_gen_jump_batch(lmh_handle *h, double simulation_time, const lmh_jump_spec *specs, int n);
/* one plan per robot uploaded from the host (what linearmpchumanoid_amd/trajectories.walk_plans / jump_plans state): zmp_x, zmp_y
 * [n][n_samples], phase [n][n_samples] or NULL (all double support), segs [n][n_seg][LMH_SEG_STRIDE] and seg_of_sample [n][n_samples], or
 * NULL / 0 / NULL for no segments.  The checks of lmh_set_refs / lmh_set_segments apply to every robot (seg_of_sample < n_seg; the
 * error text names the robot). */
int lmh_set_plans(lmh_handle *h, const double *zmp_x, const double *zmp_y, const uint8_t *phase, int n_samples,
                  const double *segs, int n_seg, const uint16_t *seg_of_sample, int n);
int lmh_plans_per_instance(const lmh_handle *h);          /* 0: one shared plan, 1: one plan per robot */
/* read the current reference set back (HOST out; any pointer may be NULL): n_samples doubles / bytes / uint16, n_seg x LMH_SEG_STRIDE doubles.
 * lmh_get_refs on a handle with per-robot plans returns robot 0's plan (as lmh_get_mpc_gain reports instance 0); lmh_get_plan reads robot
 * `inst`'s (on a shared plan every inst in [0, n_instances) returns the shared one). */
int lmh_num_ref_samples(const lmh_handle *h);
int lmh_num_segments(const lmh_handle *h);
int lmh_get_refs(lmh_handle *h, double *zmp_x, double *zmp_y, uint8_t *phase, double *segs, uint16_t *seg_of_sample);
int lmh_get_plan(lmh_handle *h, int inst, double *zmp_x, double *zmp_y, uint8_t *phase, double *segs, uint16_t *seg_of_sample);
/* per-instance scale of the ZMP x samples and of the x-axis foot polynomials (step length): HOST [n_instances]
 * or NULL for 1.0 */
int lmh_set_xscale(lmh_handle *h, const double *xscale, int n);
/* per-instance LIPM height (domain randomisation): HOST [n_instances]; rebuilds the gain rows */
int lmh_set_zcom(lmh_handle *h, const double *z_com, int n);
/* MPC gain row K (HOST out [N+1]) with u0 = -K (Px x_k - zmp[k:k+N+1]); instance 0 */
int lmh_get_mpc_gain(lmh_handle *h, double *K);

/* Timed velocity pushes inside lmh_rollout (build-defined; BASELINE config 2's perturbation at any tick instead of at t = 0 only).
 * A push is a tick number n >= 0 and an increment dv[30] of the generalised velocity, laid out as the v half of the state record
 * (dv[0:2] is the planar base kick).  A robot's tick number is absolute: n = llrint(t / dt) of its own clock state[90] at the start of a
 * tick (the kernel rounds with rint and compares in fp64: the same whole number).  At the start of tick n, before that tick's first controller evaluation, v += dv; q, v_prev (Robot::v_) and t are not touched:
 * exactly what a host does that stops lmh_rollout when the robot's clock reaches n dt, adds dv to state[i][30:60] and goes on.  Hence
 * lmh_rollout(a + b) is still lmh_rollout(a) followed by lmh_rollout(b) bit for bit: a record written to d_state never holds a push
 * whose tick has not started (a push at tick a is applied by the second call when it loads the robot; the 250-tick hand-overs inside a
 * launch follow the same rule).  A push whose tick is below the robot's tick number at the start of the launch is in the past and is
 * ignored; one beyond the last tick is never applied.  Same with plant = 0 and 1 and in every precision.  External forces on the plant
 * are not part of lmh_rollout; lmh_plant_derivative / lmh_plant_step take an external wrench on the base (rows 0..5 of their tau30).  lmh_eval, lmh_eval_debug and lmh_eval_host do not integrate and ignore the schedule.
 * records: HOST [n_sets][n_push][LMH_PUSH_STRIDE], n_sets = 1 (one schedule shared by all robots) or n_instances; per schedule the
 * ticks are whole numbers below 2^31, strictly increasing, dv finite; unused trailing records carry tick -1 (their dv is ignored).
 * n_push <= LMH_MAX_PUSHES.  records = NULL or n_push = 0 clears the schedule.  A refused call (the error text names the first offending
 * robot, "robot 7: ...") leaves the previous schedule in place, as every table setter does (see lmh_set_refs). */
int lmh_set_pushes(lmh_handle *h, const double *records, int n_push, int n_sets);
int lmh_num_pushes(const lmh_handle *h);                  /* records per schedule; 0: none set */
int lmh_pushes_per_instance(const lmh_handle *h);         /* 0: none or one shared schedule, 1: one schedule per robot */
/* robot `inst`'s schedule (the shared one on a shared schedule): HOST out [lmh_num_pushes][LMH_PUSH_STRIDE] */
int lmh_get_pushes(lmh_handle *h, int inst, double *records);

/* Per-robot controller parameters (build-defined; the reference's gains, weights and friction coefficient are compile-time literals,
 * controller.hpp:80-124): every robot of the handle runs its own PD gains, QP weights, eps_coeff, friction coefficient and -- with
 * plant = 1 -- contact constants, in one launch.  A gain or weight sweep, or a friction / ground-stiffness randomisation beside per-robot
 * models, is one handle.
 * records: HOST [n][LMH_PARAM_STRIDE], n must be n_instances; one record is, in lmh_config's own order (LMH_PARAM_OFF_*),
 *   mu | kp_joints kd_joints kp_mom kd_mom kp_feet kd_feet | w_com_lin w_com_ang w_base_pos w_base_ang w_joints w_force w_foot | eps_coeff |
 *   contact_k contact_d contact_dt contact_mu | pad (ignored).
 * Every record is checked by the rules lmh_create applies to the same fields of its lmh_config (weights positive, w_com_ang >= 0, mu and
 * eps_coeff positive, gains finite; the contact constants only when the handle's plant is 1); the error text names the first offending
 * robot ("robot 7: ...").  A refused or failed call leaves the handle on its previous parameters, under the rule of lmh_set_refs: check
 * first, build aside, replace in one step.  records = NULL or n = 0 puts the handle back on the values of its lmh_config.
 * Robot i then computes, bit for bit, what robot i of a handle created with record i in its lmh_config computes: it reads the same
 * friction generators (built on the host by the routine lmh_create uses) and the same quotients 1 / w.  w_com_ang chooses between the 15-
 * and the 18-row QP set-up per robot.  lmh_eval, lmh_eval_debug, lmh_eval_host and lmh_rollout honour the records; lmh_ik, lmh_robot_com and
 * the lmh_terms family read none of these fields.
 * These stay per handle, because they select kernel instantiations or size tables every robot shares: dt, mpc_dt, time_horizon, alpha, beta,
 * gravity, warm_start, max_qp_iters, bpp_rounds, precision, plant (z_com is per robot through lmh_set_zcom).
 * Device side: the handle keeps one whole parameter block per robot, rewritten by a small kernel whenever another setter (lmh_set_model,
 * lmh_set_zcom, the reference setters, lmh_set_foot_coeffs, lmh_set_pushes, lmh_set_xscale) moves a table, in any order with this call; such
 * a setter waits for that kernel, and if the rewrite itself fails (LMH_ERR_HIP) the setter fails as a whole: its own change is not applied.
 * On a handle of one robot a per-robot set IS the shared set: lmh_params_per_instance reports 0 there. */
int lmh_set_params(lmh_handle *h, const double *records, int n);
int lmh_params_per_instance(const lmh_handle *h);         /* 0: the config's one set, 1: one set per robot */
/* robot `inst`'s record (the config's values for every inst on a handle without per-robot parameters): HOST out [LMH_PARAM_STRIDE], pad 0 */
int lmh_get_params(lmh_handle *h, int inst, double *record);

/* replaces: Controller::standStep + Controller::WBC (src/controller.cpp:48-154) for all
 * instances.  DEVICE pointers; d_state is read AND updated (v_prev <- v, as Robot::v_ is);
 * stream is a hipStream_t (NULL = default stream).  Asynchronous. */
int lmh_eval(lmh_handle *h, double *d_state, double *d_out, int32_t *d_status, void *stream);
/* same, additionally dumping intermediate terms for unit parity (DEVICE [B][LMH_DEBUG_STRIDE]).  The debug evaluation exists in fp64 and
 * for LMH_PRECISION_FP32: on an LMH_PRECISION_MIXED handle it evaluates in fp64 (out, status and the record are an FP64 handle's, bit for
 * bit); the taps of the fp32 model-term chain that MIXED shares are read on an FP32 handle.  In FP32 the record's cone Hessian (words
 * 2093..3116) is only formed on the fp64 free-set route; W and h12 are always there. */
int lmh_eval_debug(lmh_handle *h, double *d_state, double *d_out, int32_t *d_status, double *d_debug, void *stream);

/* replaces: the closed loop of apps/offline/main.cpp:66-122 (rk4Step, rk4.hpp:5-18, of
 * dynamics(); Clock::step, Clock.hpp:11) for n_ticks ticks, state resident on chip.
 * d_out receives the k4-stage evaluation of the last tick; d_log (optional, DEVICE
 * [n_ticks][B][36]) receives tau|f of the k4 stage of every tick.  d_status: [0] k and [3] the active set of the last
 * tick, [1] the maximum of the QP rounds and [2] the OR of the flags over ALL ticks of the call.  Asynchronous.
 * Inside the call a robot is advanced in chunks of 250 ticks by whichever resident workgroup claims it next (its record in
 * d_state / d_out / d_status is the hand-over); the result does not depend on that: lmh_rollout(.., a + b, ..) equals
 * lmh_rollout(.., a, ..) followed by lmh_rollout(.., b, ..) bit for bit (with [1], [2] merged as max / OR).
 * The velocity pushes of lmh_set_pushes are applied here, at the start of their ticks.
 * Host side of "asynchronous": the call only enqueues (one small parameter copy + the kernel) on `stream`, except that a handle keeps
 * EIGHT launches in flight -- the ninth lmh_rollout waits on the host until the first has completed -- and that the first eight calls
 * allocate their launch slot (hipMalloc): not capturable into a hipGraph before every slot has been used once.  A slot is acquired whole
 * or not at all: if one of its allocations fails the call returns LMH_ERR_HIP without launching, and the next call tries again.
 * Incomplete launches are loud: the queue's waits are bounded, and if one runs out (a workgroup stalled for minutes: preemption, a
 * debugger) the robots that did not get all their ticks carry LMH_FLAG_UNFINISHED in d_status[.][2], and lmh_synchronize -- or the next
 * lmh_rollout that reuses the launch slot -- returns LMH_ERR_UNFINISHED once (the reference prints and aborts, src/controller.cpp:448-476).
 * The launch slot is clean again afterwards; the caller decides whether to re-run those robots. */
int lmh_rollout(lmh_handle *h, double *d_state, double *d_out, int32_t *d_status, double *d_log,
                int n_ticks, void *stream);
/* lmh_rollout that also records where every robot was DURING the launch (build-defined; the reference prints CoM x per tick and keeps
 * nothing, apps/offline/main.cpp:86).  d_trace: DEVICE [n_samples][B][LMH_TRACE_STRIDE], sample-major like d_log, n_samples =
 * lmh_trace_samples(n_ticks, trace_every) = n_ticks / trace_every.  Sample j of robot i is taken when the robot has completed
 * (j + 1) * trace_every ticks OF THIS LAUNCH (sample ticks are relative to the launch, not to the robot's clock) and holds exactly what
 * lmh_rollout(.., (j + 1) * trace_every, ..) would have left in that robot's three records, bit for bit:
 *   [0, 96)    the state record: q | v | v_prev | t, pads zero;
 *   [96, 176)  the out record of that tick's k4 evaluation: tau | f | qdd (the plant's acceleration when plant = 1) | CoM | comVel | xRef |
 *              yRef, pads [174, 176) zero;
 *   [176, 180) the status record as doubles: k | the maximum of the QP rounds so far in this launch | the OR of the flags so far in this
 *              launch | the active mask as its int32 value (all exact in a double).
 * Pushes (lmh_set_pushes): a sample never holds a push whose tick has not started -- one scheduled at tick n is absent from the sample
 * taken at the end of tick n - 1 and present in every later one.
 * Restart: the state part of any sample is a valid d_state row, and a launch started from it continues the same rollout bit for bit --
 * except with warm_start = 1, where the active mask (sample[179], as int32 into d_status[.][3]) must be restored as well.
 * Launch splitting: when a is a multiple of trace_every, the trace of lmh_rollout_trace(.., a + b, ..) is the traces of a and of b
 * one after the other.
 * d_trace == NULL together with trace_every == 0 means no trace: the call is lmh_rollout exactly (lmh_rollout is this call with NULL, 0).
 * Exactly one of the two given, or trace_every < 0, returns LMH_ERR_BAD_ARG before a launch slot is taken; nothing is enqueued.
 * trace_every > n_ticks is legal: zero samples, nothing is written.  The caller sizes the buffer; the call writes the samples and
 * nothing else to it, and the samples a robot flagged LMH_FLAG_UNFINISHED did not reach are left untouched.  The launch-slot rules are
 * lmh_rollout's (eight in flight, stream ordering, LMH_ERR_UNFINISHED reporting).  Each wave of a robot stores its share of a sample
 * from where the values are at the fourth stage of the tick; a launch without a trace runs a kernel instantiation that holds none of it. */
int lmh_rollout_trace(lmh_handle *h, double *d_state, double *d_out, int32_t *d_status, double *d_log,
                      int n_ticks, double *d_trace, int trace_every, void *stream);
int lmh_trace_samples(int n_ticks, int trace_every);      /* n_ticks / trace_every; 0 when trace_every <= 0 */

/* lmh_rollout that also scores every robot DURING the launch (build-defined): d_metrics, DEVICE [B][LMH_METRICS_STRIDE], one small record per
 * robot, accumulated on chip -- what a gain or weight sweep needs to rank its robots without an every-tick trace (1440 B per robot and
 * tick).  The record is DEFINED as a reduction of that trace.  Let sample s = 0 .. n - 1 be the samples of
 * lmh_rollout_trace(.., n_ticks = n, .., trace_every = 1) of the same launch; they are folded into the robot's record in order:
 *   down_s        = !(q[2] >= Z_MIN) || !(|q[3]| <= TILT_MAX) || !(|q[4]| <= TILT_MAX) on sample s (base height, roll, pitch; a NaN pose
 *                   therefore counts as down);
 *   FIRST_FALL    = COUNT, if FIRST_FALL < 0 and down_s;
 *   FIRST_FLAG    = COUNT, if FIRST_FLAG < 0 and ((int)sample[178] & 15) != 0 -- the flags are the launch-cumulative ones of the sample;
 *                   the informational LMH_FLAG_QP_FP64_ROUTE and LMH_FLAG_UNFINISHED do not count;
 *   XMIN / XMAX   = min / max with sample[0, 60), WMIN / WMAX with sample[96 + 24, 96 + 36).  The state words are those of the sample, so
 *                   a push whose tick has not started is not in them (lmh_rollout_trace's rule);
 *   TAU_MAXABS    = max(acc, |tau_j|), ERR_MAXABS = max(acc, |e|) with e = sample[96 + 66] - sample[96 + 72] and sample[96 + 67] - sample[96 + 75];
 *   TAU_SQ, ERR_SQ: acc = acc + v * v, the product and the sum rounded separately (no fused multiply-add), in tick order -- numpy's
 *                   acc += v * v gives the same bits;
 *   COUNT        += 1, last.
 * min and max are IEEE fmin / fmax: a NaN operand is ignored (v < acc ? v : acc, v > acc ? v : acc -- of two zeros of different sign the
 * accumulator's is kept; the accumulator itself is never a NaN).  A sum that meets a NaN is a NaN from then on.
 * The record is NOT reset by the call: metrics(a + b) is metrics(a) followed by metrics(b) on the same record, bit for bit, and FIRST_FLAG /
 * FIRST_FALL, once set, stay -- a sweep scored over several launches needs nothing special (COUNT counts the ticks since the reset, while
 * the flags of a sample count from its launch's start).
 * lmh_metrics_reset writes the identity record of every robot of the handle: COUNT 0, FIRST_FLAG and FIRST_FALL -1, the two thresholds as
 * given, minima +inf, maxima -inf, MAXABS words and sums 0, pads 0.  z_min = -INFINITY together with tilt_max = +INFINITY: the robot is never
 * down (a NaN pose excepted).  A NaN threshold returns LMH_ERR_BAD_ARG.  It is one small kernel on `stream`: asynchronous, capturable, no
 * launch slot.  Per-robot thresholds: overwrite words LMH_METRICS_OFF_Z_MIN and LMH_METRICS_OFF_TILT_MAX of the records after the reset
 * (stream-ordered in front of the rollout) -- that is legal; a rollout reads the two words every tick and never writes them.
 * lmh_rollout_metrics is lmh_rollout exactly -- the same launch-slot rules (eight in flight, LMH_ERR_UNFINISHED), the pushes applied, byte
 * for byte the same d_state, d_out, d_status and d_log -- and additionally folds every tick of the launch.  d_metrics == NULL returns
 * LMH_ERR_BAD_ARG before a launch slot is taken; the other argument checks are lmh_rollout's; n_ticks == 0 enqueues nothing and leaves
 * the record's bytes alone.  There is no entry point for a trace and metrics together: a caller who wants both launches the trace and
 * folds it (linearmpchumanoid_amd/metrics.py: fold_trace).  Each wave of a robot folds what it produced itself, where the trace takes its
 * words; a launch without a record runs a kernel instantiation that holds none of it. */
int lmh_metrics_reset(lmh_handle *h, double *d_metrics, double z_min, double tilt_max, void *stream);
int lmh_rollout_metrics(lmh_handle *h, double *d_state, double *d_out, int32_t *d_status, double *d_log,
                        int n_ticks, double *d_metrics, void *stream);

/* replaces: Kinematics::desiredOperationalState + Kinematics::compute
 * (src/invKinematics.cpp:11-52): Newton IK to feet (0,-/+0.05,0), com target, per instance.
 * DEVICE d_q [B][30] in/out (start posture in, solution out); com_target HOST [3]; rf6, lf6 HOST [6]: the soles' targets
 * [x y z | roll pitch yaw], the angles those of R * Rf_q0 (invKinematics.cpp:256-267).  d_iters [B] (optional): Newton steps taken.
 * The iteration stops when max|e| <= 1e-10 or after 200 steps (the reference has no cap).  Not converged: d_iters[i] == 200, or a
 * non-finite entry in d_q[i] (a target out of reach drives the iteration through singular postures; a NaN criterion also ends it).
 * Either way the call returns and the other robots of the launch are not affected; there is no error code for it. */
int lmh_ik(lmh_handle *h, double *d_q, const double *com_target, const double *rf6, const double *lf6,
           int32_t *d_iters, void *stream);

/* lmh_ik with the targets on the DEVICE, one record per robot, and n_targets of them solved one after the other in one launch: the robot
 * stays on chip, target j starts from the solution of target j-1 and target 0 from d_q_start.  Build-defined composition (the reference
 * solves one posture per call).  All pointers are DEVICE pointers; sequences are sample-major like d_log and d_trace:
 *   d_q_start [B][30]                                  start postures
 *   d_targets [n_targets][B][LMH_IK_TARGET_STRIDE]     rf6 | lf6 | com(3) | pad (ignored), the fields of lmh_ik
 *   d_q       [n_targets][B][30]                       solutions
 *   d_iters   [n_targets][B]   (may be NULL)           Newton steps taken
 *   d_crit    [n_targets][B]   (may be NULL)           the criterion max|e| the kernel held when it left the Newton loop of that solve
 * d_q may alias d_q_start only when n_targets == 1 (lmh_ik's in-place use).  Every solve follows lmh_ik's rules: the arm and head rows
 * hold the posture's CURRENT arm and head joints (a sequence keeps the start's arms throughout), the base-attitude target is zero, the
 * loop stops at max|e| <= 1e-10 or after 200 steps, a NaN criterion ends it.
 * Definition, bit for bit: for every robot, the call with n_targets = n leaves in d_q[j], d_iters[j], d_crit[j] what n calls with
 * n_targets = 1 leave, call j starting from d_q[j-1] and call 0 from d_q_start; where all robots' records at step j are equal, d_q[j]
 * and d_iters[j] are the bits of lmh_ik from the same starts with that target (the two kernels share one copy of the iteration).
 * A robot that does not converge goes on to its next target from whatever it has; a NaN posture gives a NaN criterion, zero steps and
 * NaN out.  No other robot is affected.  Not converged: d_iters == 200, a non-finite posture, or d_crit not <= 1e-10.
 * NULL d_q_start, d_targets or d_q, n_targets < 0, or n_targets > 1 with d_q == d_q_start return LMH_ERR_BAD_ARG before anything is
 * enqueued; n_targets == 0 is legal and enqueues nothing.  Asynchronous on `stream`; reads the handle's model tables (per-robot models
 * honoured) and writes nothing into the handle: a later lmh_eval or lmh_rollout is bit for bit unaffected.  No host staging and no launch
 * slot: the call can be captured into a graph from the first call on. */
int lmh_ik_batch(lmh_handle *h, const double *d_q_start, const double *d_targets, int n_targets,
                 double *d_q, int32_t *d_iters, double *d_crit, void *stream);

/* replaces: Robot::updateState + Robot::getCoM (src/Robot.cpp:264-269,225-238).
 * DEVICE d_q [B][30] in, d_com [B][3] out. */
int lmh_robot_com(lmh_handle *h, const double *d_q, double *d_com, void *stream);

/* ---- Rigid-body terms, inverse and forward dynamics for a batch of states (one kernel family of its own, one wave per robot, fp64).
 * Velocity semantics: these are PURE functions of the (q, v) given.  Every velocity-dependent term (C, Cg, AGpqp, Jpqp, comVel, angMom) is
 * evaluated at that one v.  lmh_eval evaluates C, Cg and Jdot*qdot at the stale v_prev (Robot::v_, see the state layout above), so the two
 * agree when the state's v_prev equals v.
 * Coordinates: M, C, AG and J are in the reference's own generalised velocity, which is not the state's v: the six base entries are
 * [angular(3) | linear(3)] expressed in the BASE frame, followed by the 24 joint rates (Robot::swapBaseVelocityAndRefToWorldFrame; the QP's
 * acceleration variable, controller.cpp:138).  qdd and tau30 of the two dynamics calls are in that ordering too; out.qdd of lmh_eval is the
 * same acceleration turned back to the state's ordering and the world frame.
 * DEVICE pointers: d_q, d_v, d_qdd, d_tau30 [B][30], d_w [B][12], d_terms [B][LMH_TERMS_STRIDE], d_flags [B] (may be NULL).  d_v == NULL means
 * v = 0; d_w == NULL means no contact wrench; w has the layout of out.f (n_R f_R n_L f_L) and multiplies J' as is.  Per-robot models
 * (lmh_set_model with n_models = n_instances) are honoured.  The calls are asynchronous on `stream`, read nothing of the handle but its
 * model tables and write nothing into it: a later lmh_eval or lmh_rollout is bit for bit unaffected.  NULL for a required pointer returns
 * LMH_ERR_BAD_ARG before anything is enqueued.
 *
 * lmh_terms replaces: Dynamics::computeAll + getM / getC / getCg / getAG / getAGpqp / getJpqp (controller/Dynamics.hpp, src/Dynamics.cpp),
 * Kinematics::feetJacobian (src/invKinematics.cpp:72-149) and Robot::getT / getCoM / getComVel / getComAngMom (robotInfo/Robot.hpp) for every
 * robot of the handle.  The record is laid out by the LMH_TERMS_OFF_* offsets above; row and column order of every array is the reference's
 * Eigen shape.  Cg is its first six entries only: the kernels form only those, and the controller uses only those. */
int lmh_terms(lmh_handle *h, const double *d_q, const double *d_v, double *d_terms, void *stream);
/* Build-defined (the reference has no general inverse dynamics: forwardNewtonEuler never uses its qDD, src/Dynamics.cpp:124-146, and tau
 * comes only from M qdd + C - J'f of the QP's own solution, src/controller.cpp:138).  tau30 = M qdd + C - J'w for ANY qdd and w:
 * all 30 rows are returned, rows 0..5 are the residual wrench on the floating base, rows 6..29 the joint torques. */
int lmh_inverse_dynamics(lmh_handle *h, const double *d_q, const double *d_v, const double *d_qdd, const double *d_w, double *d_tau30, void *stream);
/* Build-defined, the inverse of the call above: solves M qdd = tau30 + J'w - C by an LDL' factorisation of the dense mass matrix without
 * pivoting (M is symmetric positive definite).  d_flags[i]: LMH_FLAG_NOT_SPD when a pivot of robot i's matrix was not positive,
 * LMH_FLAG_NONFINITE when its result holds a NaN / Inf; neither stops the other robots. */
int lmh_forward_dynamics(lmh_handle *h, const double *d_q, const double *d_v, const double *d_tau30, const double *d_w, double *d_qdd, int32_t *d_flags, void *stream);

/* ---- Torque-driven plant (build-defined): the compliant-contact plant of lmh_config.plant = 1 as calls of its own, driven by torques the CALLER
 * supplies -- a learned policy, the controller of lmh_eval held over several physics steps (zero-order hold), or none (a passive robot).
 * One kernel family of its own, one wave per robot, fp64.  The calls are asynchronous on `stream`, read the handle's model tables (per-robot
 * models honoured) and the robot's contact constants -- lmh_config's contact_k / contact_d / contact_dt / contact_mu, or the robot's record of
 * lmh_set_params -- and write nothing into the handle: a later lmh_eval or lmh_rollout is bit for bit unaffected.  They work on a handle
 * with plant = 0 too; such a handle never had its contact constants checked, so every call checks the host copy (the config, or every
 * per-robot record) by lmh_create's rules for plant = 1 and refuses with LMH_ERR_BAD_ARG, naming the robot ("robot 7: ..."), before anything
 * is enqueued.  NULL for a required pointer returns LMH_ERR_BAD_ARG before anything is enqueued.
 * Contact model: see lmh_config.plant.  Vertex v of a sole at x = o_sole + r_v moving with xdot = v_o + w x r_v (the sole's twist J vhat at the
 * v given): penetration d = -x_z > 0 gives the normal force max(0, k d - c xdot_z) and the tangential force -c_t xdot_xy scaled back onto the
 * friction disc mu f_n; a vertex out of the ground carries exactly 0.
 * DEVICE pointers: d_q, d_v [B][30] (the state's ordering), d_tau30 [B][30], d_contact [B][LMH_CONTACT_STRIDE], d_xdot [B][60], d_state
 * [B][LMH_STATE_STRIDE], d_flags [B].
 * d_tau30 is in the coordinates of M, exactly as lmh_forward_dynamics takes it: rows 6..29 are the joint torques, rows 0..5 an EXTERNAL WRENCH
 * ON THE BASE ([angular | linear], base frame) -- this is how external forces enter the plant.  NULL means zero: a passive robot.
 *
 * lmh_contact_wrench: the ground's forces for a batch of states.  d_v == NULL means v = 0.  Record (LMH_CONTACT_OFF_*): w(12: n_R f_R n_L f_L,
 * about the sole origins, world axes, like out.f) | vertex force [8][3] | pad(4) = 0. */
int lmh_contact_wrench(lmh_handle *h, const double *d_q, const double *d_v, double *d_contact, void *stream);
/* xdot = d/dt (q, v) of the plant: xdot[0:30] is qdot from v (v_lin + omega x p_base, the Euler rates Omega(rpy) omega, the joint rates:
 * apps/offline/main.cpp:107-116); xdot[30:60] is the acceleration solving M a = tau30 + J'w_c - C(q, v), turned back to the state's ordering
 * and the world frame -- what out.qdd carries with plant = 1.  Every velocity product is taken at the v given, as in lmh_terms.  The solve
 * uses the structure of M (four limb blocks, the head's, a 6 x 6 Schur complement on the base).  d_contact (may be NULL) receives the
 * contact record of the state.  d_flags[i] (may be NULL): LMH_FLAG_NOT_SPD when a pivot of robot i's solve was rejected, LMH_FLAG_NONFINITE
 * when its result holds a NaN / Inf; neither stops the other robots. */
int lmh_plant_derivative(lmh_handle *h, const double *d_q, const double *d_v, const double *d_tau30, double *d_xdot, double *d_contact, int32_t *d_flags, void *stream);
/* n_substeps classic RK4 steps (rk4.hpp:5-18) of lmh_config.dt on (q, v) of the state records with the torques held, state on chip for the
 * whole launch; t += dt after every substep (Clock::step's accumulation order).  v_prev and the pads of the record are left untouched: a
 * caller alternating lmh_eval and this call sees the stale-velocity convention of a zero-order-hold loop (lmh_eval stores v_prev <- v).
 * n_substeps = 0 is legal and enqueues nothing; a negative value returns LMH_ERR_BAD_ARG.  lmh_plant_step(a + b) equals lmh_plant_step(a)
 * followed by lmh_plant_step(b) bit for bit.  d_flags[i] (may be NULL): the flags of lmh_plant_derivative, OR-ed over the substeps. */
int lmh_plant_step(lmh_handle *h, double *d_state, const double *d_tau30, int n_substeps, int32_t *d_flags, void *stream);

/* ---- Rigid-contact plant (build-defined): constrained forward dynamics with held soles.  The same robot under the same tau30 as the two
 * calls above, but the held soles are kinematic constraints and the contact wrench is their multiplier: no stiffness, no penetration, no
 * step-size bound from the ground, and a wrench lambda that can be laid directly beside the controller's planned out.f.
 * DEFINITION, per robot, in the coordinates of M as lmh_forward_dynamics uses them.  The mode m = d_mode[i] & 3 selects the held rows S of
 * the feet Jacobian J (rows n_R f_R n_L f_L, as in out.f): LMH_PHASE_DOUBLE rows 0..11, LMH_PHASE_RIGHT rows 0..5, LMH_PHASE_LEFT rows
 * 6..11, LMH_PHASE_FLIGHT none.
 *         r   = tau30 - C(q, v)                        every velocity product at the v given, as lmh_plant_derivative
 *         a0  = M^-1 r
 *         Y   = M^-1 J_S'        A = J_S Y             (M is not exactly symmetric -- the reference's inertia typos -- so neither is A)
 *         g   = J_S a0 + (Jdot qdot)_S + kv (J_S vhat)       vhat: v in M's coordinates; J vhat is the sole twist
 *         lambda_S = -A^-1 g     (Gauss-Jordan without pivoting)      lambda = 0 on the rows that are not held
 *         a   = a0 + Y lambda_S
 * M^-1 uses the structure of M as lmh_plant_derivative does (limb blocks, the head's, the 6 x 6 Schur complement on the base) with the
 * twelve columns of J' riding along; the first right-hand side sees lmh_plant_derivative's operations in their order, so with
 * LMH_PHASE_FLIGHT and every vertex out of the ground xdot is lmh_plant_derivative's bit for bit.  trajectories.rigid_contact_acceleration
 * is the numpy statement.  That every pivot of the unpivoted elimination of A is positive is checked on the statement near standing
 * (tests/test_rigid.py, smallest pivot 0.473) and over the postures and velocities of a fall (tests/test_fall_rigid_cases.py: 0.399 over
 * both bands, 0.567 on the pitch ladder).  xdot[0:30] is lmh_plant_derivative's qdot, xdot[30:60] is a turned back to the state's ordering and the world
 * frame, as there.
 * kv >= 0 [1/s] is a velocity-level stabilisation: the constraint is d/dt (J_S vhat) = -kv J_S vhat, so the held soles' twist decays as
 * e^(-kv t) (kv = 0: it is kept).  Jdot qdot is the reference's -- the sole's spatial acceleration turned to world axes --, so this holds
 * component by component for the angular part and in magnitude for the linear part, which also turns with the sole (d/dt v = -kv v +
 * omega x v; about |omega_0| / kv radians in all); a sole at rest stays at rest.  There is NO position-level term: a held sole stays
 * where its twist leaves it, so a sole that starts with a twist w_0 travels about w_0 / kv before it rests (w_0 t with kv = 0), and the
 * integrator's own error accumulates in its position undamped (measured drift: DESIGN.md, round 33).
 * The contact is BILATERAL.  Whether a ground could supply lambda is reported, not enforced: LMH_FLAG_CONTACT_PULL when a held foot's f_z
 * (rows 5, 11 of lambda) is negative, LMH_FLAG_CONTACT_SLIP when hypot(f_x, f_y) > contact_mu f_z on a held foot, with the robot's own
 * contact_mu (lmh_config's or the robot's record of lmh_set_params).  Both are informational, like LMH_FLAG_TAU_LIMIT.  LMH_FLAG_NOT_SPD (a
 * pivot of M's blocks or of A was not positive) and LMH_FLAG_NONFINITE keep their meaning; neither stops the other robots.
 * A constraint knows no plane and no servo: the two calls read NOTHING of lmh_set_ground and NOTHING of lmh_set_servo, and give the same
 * bytes with and without either table.
 * d_mode: DEVICE int32 [B]; only the low two bits of a word are read; NULL = every robot LMH_PHASE_DOUBLE.  d_tau30: NULL = a passive
 * robot.  d_lambda (DEVICE [B][12]) and d_flags (DEVICE [B]) may be NULL.
 * lmh_plant_step_rigid: everything else is lmh_plant_step's -- n_substeps RK4 steps of lmh_config.dt, t += dt per substep, v_prev and the
 * pads untouched, (a + b) equals (a) followed by (b) bit for bit, the flags of the derivative OR-ed over every stage, n_substeps = 0
 * enqueues nothing.  d_lambda receives the multiplier at the FIRST stage of the LAST substep: with n_substeps = 1 that is
 * lmh_plant_derivative_rigid's lambda at the input state, bit for bit.  Both calls work on any handle, write nothing into it, are
 * asynchronous and capturable from the first call, honour per-robot models and check the contact constants as lmh_plant_step does.
 * Refused with LMH_ERR_BAD_ARG before anything is enqueued: NULL for d_q, d_v, d_xdot or d_state; kv negative or not finite;
 * n_substeps < 0.
 * Cost (one MI355X, 4096 standing robots x 200 control ticks, kv = 50; scripts/rigid_rate.py; other batch sizes not
 * measured): lmh_plant_step_rigid 45.29 against lmh_plant_step's 35.85 ms (x 1.26) at 200 x 1 substeps and 449.4 against 356.5 ms (x 1.26) at
 * 200 x 10, the same with the modes mixed over the batch (45.08 / 449.0 ms).  lmh_plant_step runs at the parent commit's rate: its kernel is
 * the parent's, instruction for instruction.
 * What the rigid plant says about the closed loop (scripts/rigid_stand.py, profiles/r33_rigid_stand.txt): from rest, both soles held, default
 * gains, stand_step ; lmh_plant_step_rigid(1 substep) is down at control tick 728 (|pitch| > 0.5 rad; the height alone: 816), as the CPU loop
 * of the oracle and the numpy statement is -- earlier than on the compliant ground (1655), with |lambda - out.f| <= 0.03 N for the first
 * hundred ticks: the ground's compliance is not what brings the loop down.  With kp_joints raised a hundredfold and kd_joints tenfold (the
 * damping ratio kept), whatever kp_mom between 0.03 and 30 times its default, the robot is up after 2000 ticks, without pulling on the
 * ground or leaving the friction disc; no cell with kp_joints up to 19 times its default stands. */
#define LMH_FLAG_CONTACT_PULL 256  /* informational: a held foot's multiplier pulls (f_z < 0) */
#define LMH_FLAG_CONTACT_SLIP 512  /* informational: a held foot's multiplier leaves the friction disc contact_mu f_z */
int lmh_plant_derivative_rigid(lmh_handle *h, const double *d_q, const double *d_v, const double *d_tau30, const int32_t *d_mode, double kv, double *d_xdot, double *d_lambda,
                               int32_t *d_flags, void *stream);
int lmh_plant_step_rigid(lmh_handle *h, double *d_state, const double *d_tau30, const int32_t *d_mode, double kv, int n_substeps, double *d_lambda, int32_t *d_flags, void *stream);

/* ---- Rigid-contact plant: plastic touchdown impact (build-defined).  What the two calls above lack at the instant a sole BECOMES held: the
 * velocity jumps to the nearest velocity, in the metric of M, that satisfies the mode's constraints, and the impulse is the multiplier of that
 * projection.  Without it a sole that lands moving is braked over about 1 / kv seconds and drifts by about w_0 / kv meanwhile.
 * DEFINITION, per robot, in the coordinates of M as lmh_plant_derivative_rigid uses them; S: the rows d_mode[i] & 3 holds (NULL:
 * LMH_PHASE_DOUBLE), exactly as there.
 *         w      = J_S vhat                     the held soles' twist at (q, v)
 *         Y      = M^-1 J_S'       A = J_S Y
 *         Lam_S  = -A^-1 w         (Gauss-Jordan without pivoting, as the derivative's solve)      Lam = 0 on the rows that are not held
 *         dvhat  = Y Lam_S
 *         dv     = dvhat turned back to the state's ordering and the world frame, by the map the derivative applies to its acceleration
 *         v_plus = v + dv
 * ALL soles the mode holds take part, not only a newly held one: a touchdown into double support keeps the stance sole at rest.  There is no
 * kv, no torque, no C and no Jdot qdot in it; M, J, Y and A are the derivative's, operation for operation.  The update is v + dv and not a
 * round trip of vhat, so LMH_PHASE_FLIGHT gives v_plus == v bit for bit and an impulse of exact zeros.  J_S (vhat + dvhat) = 0 to rounding;
 * the kinetic energy vhat' M vhat / 2 does not rise; a second impact on v_plus changes nothing beyond rounding.  No restitution.
 * trajectories.rigid_contact_impact is the numpy statement (tests/test_impact.py: backward, constraint and forward figures <= 1e-12 on 48
 * cases, every pivot of A positive, smallest 0.473).
 * d_v_plus: DEVICE [B][30].  d_impulse: DEVICE [B][12] in the layout of out.f (N s and N m s), may be NULL.  d_flags: DEVICE [B], may be
 * NULL: LMH_FLAG_NOT_SPD and LMH_FLAG_NONFINITE (of v_plus) as in the derivative, and two informational flags, reported and not enforced,
 * both outside the mask (& 15) of the metrics' FIRST_FLAG: LMH_FLAG_IMPULSE_PULL when a held foot's impulse has f_z < 0 -- the sole was
 * moving away from the ground, a real contact would not have closed --, LMH_FLAG_IMPULSE_SLIP when hypot(f_x, f_y) > contact_mu f_z on a held
 * foot, with the robot's own contact_mu.
 * As the two rigid calls: works on any handle and writes nothing into it, reads nothing of the ground or servo table, honours per-robot
 * models, checks the contact constants, is asynchronous and capturable as the first call.  Refused with LMH_ERR_BAD_ARG before anything is
 * enqueued, each with a message of its own: NULL d_q, NULL d_v, NULL d_v_plus. */
#define LMH_FLAG_IMPULSE_PULL 1024 /* informational: a held foot's impulse pulls (f_z < 0): the sole was leaving the ground */
#define LMH_FLAG_IMPULSE_SLIP 2048 /* informational: a held foot's impulse leaves the friction disc contact_mu f_z */
int lmh_plant_impact_rigid(lmh_handle *h, const double *d_q, const double *d_v, const int32_t *d_mode, double *d_v_plus, double *d_impulse, int32_t *d_flags, void *stream);

/* ---- Ground planes under the soles (build-defined; lmh_set_ground, a table of the handle like the actuator records): how steep a slope, or
 * how high a ledge under one foot, the controller survives -- per robot, so that a sweep is one launch.
 * records: HOST [n_sets][LMH_GROUND_STRIDE], n_sets = 1 (one record for every robot) or n_instances; NULL or n_sets = 0 clears the table.
 * One record is n_R(3) | h_R | n_L(3) | h_L: the ground under a foot is the half space n.x <= h, world coordinates and metres, n a unit normal
 * and h the plane's offset along it.  The same plane under both feet is a slope; horizontal planes with different h are a ledge under one foot.
 * CONTACT MODEL.  Per vertex at x with velocity xdot, on its foot's plane (n, h), with the robot's contact_k, contact_d, contact_dt (c_t),
 * contact_mu:
 *     pen = h - n.x
 *     vn  = n.xdot
 *     fn  = max(0, k pen - d vn)
 *     vt  = xdot - vn n
 *     ft  = -c_t vt
 *     if |ft| > mu fn:  ft *= mu fn / |ft|
 *     f   = ft + fn n   if pen > 0,   else exactly 0
 * The wrench is formed as before: r_v x f_v | f_v about the sole origin, world axes, vertices summed in the same order; the contact record
 * (LMH_CONTACT_*) keeps its layout.  With n = (0, 0, 1) and h = 0 this is the model of lmh_contact_wrench above (to a few ulps of |ft|: the
 * table's kernels form their sums with explicit fused multiply-adds).  trajectories.ground_contact is the same statement in numpy.
 * WHO READS IT.  lmh_contact_wrench, lmh_plant_derivative and lmh_plant_step; lmh_rollout_zoh, _ref, _ex and _io, by their definitions: the
 * host loops written out below are made of lmh_eval and lmh_plant_step, and their bit-for-bit statements stay true word for word.
 * lmh_rollout_zoh_box on a handle with a table returns LMH_ERR_BAD_ARG before anything is enqueued.  Every other call (lmh_eval*,
 * lmh_rollout*, the terms, IK and MPC families) reads nothing of the table and is bit for bit what it is without it.  A handle without a
 * table, or whose table was cleared, launches exactly the kernels it launches without this feature.
 * THE CONTROLLER IS NOT TOLD.  Its foot references and its friction pyramid stay the flat ones: standing on ground it does not know about is
 * the point of a robustness test.  The thresholds Z_MIN and TILT_MAX of the metrics stay the caller's.
 * CHECKS, each LMH_ERR_BAD_ARG naming the first offending robot ("robot 7: ..."): every word finite; | |n|^2 - 1 | <= 1e-12 (the host does
 * not normalise, and lmh_get_ground returns the bytes that were set); n_z > 0; n_sets 1 or n_instances.  A handle created with plant = 1 is
 * refused with a message of its own: the RK4 reference loop (lmh_rollout, lmh_eval with plant = 1) is not offered with a ground.
 * lmh_set_refs' rule: check first, build aside, replace in one step -- a refused or failed call leaves the previous table in place.  The
 * table is a device buffer of its own (64 B per robot): the parameter blocks of lmh_set_params are not rebuilt.
 * COST (MI355X, 4096 standing robots, 200 control ticks, a record per robot, against the same build without a table; other batch sizes not
 * measured): lmh_plant_step 36.26 against 36.19 ms (+0.2 %) at 200 x 1 substeps and 357.2 against 357.1 ms (+0.0 %) at 200 x 10;
 * lmh_rollout_zoh 65.0 against 61.7 ms (+5.4 %) at n_substeps = 1 and 477.0 against 474.6 ms (+0.5 %) at 10 -- with a table all four
 * zero-order-hold entry points run lmh_rollout_zoh_io's loop, so the figure at one substep per tick holds that loop's own cost beside
 * the planes' loads (not profiled apart).
 * Without a table both calls run at the parent commit's rate (scripts/ground_rate.py). */
int lmh_set_ground(lmh_handle *h, const double *records, int n_sets);
int lmh_ground_per_instance(const lmh_handle *h);                    /* 0: none or one shared record, 1: one per robot */
int lmh_get_ground(lmh_handle *h, int inst, double *record);         /* HOST [LMH_GROUND_STRIDE]; 0 0 1 0 | 0 0 1 0 on a handle without a table */

/* ---- Zero-order-hold closed loop (build-defined; what apps/mujoco/main.cpp:115-122 intended before its feedback path was commented out):
 * the controller at its own rate, the torque-driven plant at a finer step with the torques held, n_ticks control ticks in ONE launch with
 * every robot on chip from the first tick to the last.
 * DEFINITION.  For every robot the call leaves exactly what this host loop leaves, bit for bit:
 *     repeat n_ticks times:
 *         lmh_eval(h, d_state, d_out, d_status, s)                  reads t = state[90], stores v_prev <- v
 *         tau30 = [ base_wrench[i] (6) | out.tau (24) ]
 *         lmh_plant_step(h, d_state, tau30, n_substeps, d_flags, s)
 * d_state: the state after the last hold (v_prev = the v the last evaluation saw; pads untouched).  d_out: the out record of the last
 * evaluation.  d_status: [0] k and [3] the active mask of the last evaluation, [1] the maximum of the QP rounds over all ticks of the call,
 * [2] the OR of the controller's flags and of lmh_plant_step's flags over all ticks.  d_log (DEVICE [n_ticks][B][36], may be NULL): tau | f of
 * every tick's evaluation, as in lmh_rollout.  d_base_wrench (DEVICE [B][6], may be NULL = zero): rows 0..5 of lmh_plant_step's tau30, an
 * external wrench on the base ([angular | linear], base frame), held for the whole launch -- this is how a disturbance enters this loop.
 * d_state, d_out and d_status have lmh_eval's layout and meaning.
 * Consequence: lmh_rollout_zoh(a + b) equals (a) followed by (b) bit for bit, with [1] and [2] merged as max / OR; with warm_start = 1 too,
 * because d_status[.][3] carries the mask across the split.
 * The control period is n_substeps * lmh_config.dt; mpc_dt keeps its meaning.  Per-robot models, plans, xscale, z_com and lmh_set_params
 * records are honoured as the two composed calls honour them.  The velocity pushes of lmh_set_pushes are NOT applied (as in lmh_eval; lmh_rollout_zoh_ex
 * applies them).
 * This is not lmh_rollout with plant = 1, which evaluates the controller at all four RK4 stages of every step (the reference's loop); on a
 * plant = 1 handle the evaluation here is whatever lmh_eval does there.
 * n_ticks < 0 or n_substeps < 0, or NULL for d_state / d_out / d_status, return LMH_ERR_BAD_ARG before anything is enqueued; n_ticks = 0
 * enqueues nothing; n_substeps = 0 is legal (n_ticks evaluations of a state that does not move).  The contact constants are checked as
 * lmh_plant_step checks them, on a plant = 0 handle too ("robot 7: ...").  LMH_PRECISION_FP64 handles only: another precision is refused
 * with LMH_ERR_BAD_ARG.  Asynchronous on `stream`; the parameter block travels in the kernel arguments (no launch slot, no work queue), so
 * the call can be captured into a hipGraph from the first call on and writes nothing into the handle. */
int lmh_rollout_zoh(lmh_handle *h, double *d_state, double *d_out, int32_t *d_status, const double *d_base_wrench, double *d_log,
                    int n_ticks, int n_substeps, void *stream);

/* ---- Caller-supplied CoM references (build-defined; the reference has no counterpart): the whole-body controller tracking a CoM plan that
 * was made elsewhere -- the box-constrained preview MPC below, a capture-point or DCM plan, a learned policy, a plan computed once and
 * replayed -- instead of the unconstrained preview step lmh_eval forms itself from the robot's measured CoM state.
 * d_ref: DEVICE, records of LMH_MPC_STRIDE doubles, [B][LMH_MPC_STRIDE] for lmh_eval_ref and [n_ticks][B][LMH_MPC_STRIDE] (sample-major like
 * d_log; record j serves control tick j of THIS launch) for lmh_rollout_zoh_ref.  Only words LMH_MPC_OFF_XREF .. + 2 and LMH_MPC_OFF_YREF .. + 2
 * are read: position, velocity and acceleration reference of the axis, in metres, absolute (not multiplied by xscale), fp64 in every
 * precision; words [6, 16) are ignored.  A d_traj of lmh_mpc_rollout / lmh_mpc_box_rollout, or a d_mpc of the step calls, is a valid d_ref as
 * it stands.
 * DEFINITION of lmh_eval_ref.  lmh_eval with the six values Mpc3dLip::getXRef / getYRef would have returned replaced by the record's: posRef,
 * velRef and accRef of axes x and y of PDMomentumAcc (controller.cpp:310-325), and out[72:78], which then carry the supplied words.
 * Everything else is lmh_eval's: k = (int)(t / mpc_dt), the support phase, the foot polynomials and LMH_FLAG_ZMP_RANGE still come from the
 * handle's plan at the robot's clock; the z reference stays the robot's z_com and the angular-momentum reference zero; v_prev <- v, the warm
 * start through status[3], per-robot models, plans, xscale, z_com and lmh_set_params records, every precision lmh_eval supports.  A
 * non-finite word among the six raises LMH_FLAG_NONFINITE for that robot (checked on the words themselves, whatever the solver makes of
 * them) and disturbs no other robot.  There is no debug-dump variant.
 * DEFINITION of lmh_rollout_zoh_ref.  For every robot the call leaves exactly what this host loop leaves, bit for bit:
 *     for j in 0 .. n_ticks - 1:
 *         lmh_eval_ref(h, d_state, d_ref + j * B * LMH_MPC_STRIDE, d_out, d_status, s)
 *         tau30 = [ base_wrench[i] (6) | out.tau (24) ]
 *         lmh_plant_step(h, d_state, tau30, n_substeps, d_flags, s)
 * d_out, d_status and d_log keep lmh_rollout_zoh's meaning.  Consequence: (a + b) equals (a) followed by (b) with d_ref advanced by a records
 * per robot (a * B * LMH_MPC_STRIDE doubles).  lmh_rollout_zoh's other rules apply as they are: LMH_PRECISION_FP64 handles only, the contact
 * constants checked, no launch slot, capturable into a hipGraph from the first call on, nothing written into the handle.
 * d_ref == NULL returns LMH_ERR_BAD_ARG before anything is enqueued, in both calls; the other refusals are those of lmh_eval /
 * lmh_rollout_zoh, word for word; n_ticks = 0 enqueues nothing.  The caller supplies one record per control tick: nothing is interpolated.
 * lmh_rollout (the RK4 reference loop, which evaluates the controller at four stage times per tick) is not offered with an external
 * reference, nor are its _trace and _metrics forms. */
int lmh_eval_ref(lmh_handle *h, double *d_state, const double *d_ref, double *d_out, int32_t *d_status, void *stream);
int lmh_rollout_zoh_ref(lmh_handle *h, double *d_state, double *d_out, int32_t *d_status, const double *d_base_wrench, double *d_log,
                        const double *d_ref, int n_ticks, int n_substeps, void *stream);

/* ---- The zero-order-hold loop with timed pushes, a wrench per control tick, a trace and a metrics record (build-defined): what a push-recovery
 * study or a scored sweep on the torque-driven plant needs, in the one launch, instead of a host loop around lmh_eval and lmh_plant_step.
 * One options record, one entry point; an all-zero record, or opts == NULL, is lmh_rollout_zoh(h, state, out, status, NULL, NULL, n_ticks,
 * n_substeps, s) exactly (the same kernel), and a record with only d_base_wrench, d_ref and d_log set is lmh_rollout_zoh / lmh_rollout_zoh_ref
 * with those arguments.  d_ref == NULL means the built-in preview step.
 * DEFINITION.  For every robot the call leaves, bit for bit, what this host loop leaves (B = n_instances; n is a whole number):
 *     n = llrint(state[90] / dt)                 the robot's plant substep number at the start of the launch; counted in integers from here on
 *     for j in 0 .. n_ticks - 1:
 *         if pushes and the robot's schedule has a record with tick == n:  state.v += dv      before the evaluation; q, v_prev, t untouched
 *         lmh_eval (d_ref == NULL)  or  lmh_eval_ref(d_ref + j * B * LMH_MPC_STRIDE)
 *         tau30 = [ wrench (6) | out.tau (24) ]      wrench = d_base_wrench[i], or d_base_wrench[j][i] when wrench_per_tick
 *         r = n_substeps
 *         while r > 0:
 *             p = the smallest schedule tick with n < p < n + r   (pushes only; else none)
 *             s = p - n if p exists else r
 *             lmh_plant_step(s substeps);  n += s;  r -= s
 *             if p exists:  state.v += dv(p)
 *         the sample / the fold of this control tick (below)
 * PUSHES (pushes = 1: the handle's lmh_set_pushes schedule).  A push tick is a PLANT SUBSTEP number, in units of lmh_config.dt on the robot's
 * own clock -- the meaning it has in lmh_rollout, where a tick is one step of dt.  A push that falls on the start of a control tick is seen by
 * that tick's evaluation (whose v_prev <- v then stores the pushed v); one inside a hold is applied between two substeps and the controller
 * meets it at its next evaluation.  A record whose tick equals the substep number the launch ends on is not applied: the next launch applies it
 * when it loads the robot, so (a + b) is (a) followed by (b) bit for bit, with d_ref advanced by a records and d_base_wrench too when it is per
 * tick.  A state record or a sample never holds a push whose substep has not started; records in the past at the start of the launch are
 * ignored; pushes = 1 on a handle without a schedule is legal and changes nothing.  pushes = 1 with n_substeps == 0 and n_ticks > 0 returns
 * LMH_ERR_BAD_ARG (the clock does not move, the rule has no meaning), and so does pushes = 1 with n_ticks * n_substeps >= 2^30 - 1.
 * TRACE (d_trace with trace_every > 0; lmh_rollout_trace's layout and rules as they are).  Sample j is taken when the robot has completed
 * (j + 1) * trace_every CONTROL ticks of this launch and holds what the same call with n_ticks = (j + 1) * trace_every would have left in the
 * robot's three records: the state words after that tick's hold, q | v | v_prev (the v the evaluation saw) | t, pads written as zeros; the out
 * record of that tick's evaluation (out.qdd is the evaluation's, not the plant's); the status words as doubles: k, the maximum of the QP rounds
 * so far in this launch, the OR of the controller's and the plant's flags so far in this launch including this tick's hold, the active mask.  Exactly one of d_trace /
 * trace_every given, or trace_every < 0, returns LMH_ERR_BAD_ARG; trace_every > n_ticks writes nothing; the trace of (a + b) is the trace of
 * (a) followed by the trace of (b) when trace_every divides a.  lmh_write_trace's sample_dt of such a trace is trace_every * n_substeps * dt.
 * METRICS (d_metrics: lmh_metrics_reset's records, the same 208 doubles and the same accumulation over launches as lmh_rollout_metrics).  The
 * record is the fold (lmh_rollout_metrics; linearmpchumanoid_amd/metrics.py: fold_trace) of the every-control-tick trace of the same launch.
 * COUNT counts control ticks.  The state extrema XMIN / XMAX (and FIRST_FALL) are taken at the ENDS OF CONTROL TICKS, not at every plant
 * substep: an excursion inside a hold that has decayed by its end is not in them.  WMIN / WMAX are the CONTROLLER'S contact wrench out.f, as
 * in the trace, not the wrench the plant's compliant contact produced.  d_trace and d_metrics may both be given.  n_ticks == 0 enqueues
 * nothing and leaves the record's bytes alone.
 * Everything else is lmh_rollout_zoh's: LMH_PRECISION_FP64 handles only, the contact constants checked on the host before anything is
 * enqueued, no launch slot, no work queue, no host staging, capturable into a hipGraph from the first call on a fresh handle, nothing written
 * into the handle, the meaning of d_state / d_out / d_status, per-robot models, plans, xscale, z_com and lmh_set_params records honoured.
 * Refusals, each LMH_ERR_BAD_ARG before anything is enqueued and with a message of its own: wrench_per_tick, pushes or reserved outside its
 * values; wrench_per_tick = 1 with a NULL wrench; the trace rules and the pushes rules above.  The others are lmh_rollout_zoh's, word for word.
 * Cost (one MI355X, 4096 standing robots x 200 control ticks): with no option set the call launches lmh_rollout_zoh's
 * kernel; at n_substeps = 1 each option alone costs 1.6 .. 2.6 % (inside the plain loop's own range of timings) and all of them with an
 * every-tick trace 5.8 %; at n_substeps = 10 every combination lies inside the plain loop's own range of timings.  Other batch sizes and
 * anything multi-GPU were not measured. */
typedef struct lmh_zoh_opts {
    const double *d_base_wrench;  /* DEVICE [B][6], or [n_ticks][B][6] when wrench_per_tick = 1; NULL = zero */
    const double *d_ref;          /* DEVICE [n_ticks][B][LMH_MPC_STRIDE] as lmh_rollout_zoh_ref takes it; NULL = the built-in preview step */
    double *d_log;                /* DEVICE [n_ticks][B][36] or NULL, as lmh_rollout_zoh */
    double *d_trace;              /* DEVICE [lmh_trace_samples(n_ticks, trace_every)][B][LMH_TRACE_STRIDE] or NULL */
    double *d_metrics;            /* DEVICE [B][LMH_METRICS_STRIDE] or NULL; lmh_metrics_reset's records */
    int32_t trace_every;          /* control ticks per sample; 0 together with d_trace == NULL: no trace */
    int32_t wrench_per_tick;      /* 0 | 1 */
    int32_t pushes;               /* 0 | 1: apply the handle's lmh_set_pushes schedule */
    int32_t reserved;             /* must be 0 */
} lmh_zoh_opts;
int lmh_rollout_zoh_ex(lmh_handle *h, double *d_state, double *d_out, int32_t *d_status, const lmh_zoh_opts *opts,
                       int n_ticks, int n_substeps, void *stream);

/* ---- The zero-order-hold loop with the box-constrained preview step (lmh_mpc_box_step, below) closed around the MEASURED CoM inside it
 * (build-defined): the predicted ZMP stays inside the caller's bounds while the robot is pushed, which a replayed plan (lmh_mpc_box_rollout's
 * traj handed to lmh_rollout_zoh_ref) cannot do, in one launch and on one factorisation of the preview Hessian instead of a host loop of four
 * launches per control tick that factors it on every tick.
 * d_box, n_samples, n_sets: exactly what lmh_mpc_box_step takes ([n_sets][4][n_samples], rows LMH_BOX_*, metres, not scaled by xscale; n_sets 1
 * or n_instances; n_samples == lmh_num_ref_samples).  d_mpc: DEVICE [n_ticks][B][LMH_MPC_STRIDE], sample-major, or NULL: the sample of every
 * control tick's constrained step (xRef | yRef | zmp | state | t | k | flags | active).  opts: lmh_rollout_zoh_ex's record as it stands, or NULL;
 * opts->d_ref must be NULL (a reference and the box step are exclusive).
 * DEFINITION.  For every robot the call leaves, bit for bit, what lmh_rollout_zoh_ex's host loop (above) leaves with its line
 *         lmh_eval (d_ref == NULL)  or  lmh_eval_ref(...)
 * replaced by
 *         x, xdot, y, ydot = out[66], out[69], out[67], out[70] of lmh_eval at the robot's current state record (pure functions of q and v: an
 *                            lmh_eval on a scratch copy of the record gives them; behind a push that falls on the tick's start)
 *         lip = x | xdot | y | ydot | state[90]
 *         m   = lmh_mpc_box_step(lip, d_box, n_samples, n_sets)          -> d_mpc[j][i] when d_mpc != NULL
 *         lmh_eval_ref(state, ref = m)
 *         the tick's flags |= (int)m[LMH_MPC_OFF_FLAGS]                  (QP_MAXITER, NOT_SPD, BOX_EMPTY, ZMP_RANGE, NONFINITE)
 * Everything else is lmh_rollout_zoh_ex's, word for word: the hold pieces, where pushes fall, the trace sample (whose out words are
 * lmh_eval_ref's: out[72:78] are m[0:6]), the metrics fold, the status words, (a + b) equals (a) then (b) with d_mpc advanced by a records, the
 * contact-constant checks, LMH_PRECISION_FP64 handles only, no launch slot, nothing written into the handle, capturable into a hipGraph from
 * the first call on a fresh handle.  A robot whose window holds an empty or NaN box sample gets NaN reference words and so, by lmh_eval_ref's
 * rule, LMH_FLAG_NONFINITE | LMH_FLAG_BOX_EMPTY; it disturbs no other robot.  Every tick starts from the empty working set.
 * Refusals, each LMH_ERR_BAD_ARG before anything is enqueued and with a message of its own: NULL d_box, another n_samples, n_sets not 1 or
 * n_instances, opts->d_ref != NULL; all of lmh_rollout_zoh_ex's apply as well.  n_ticks == 0 enqueues nothing.
 * LDS: the constrained problem's tiles sit behind the evaluation's 40.9 KB and are sized by the handle's horizon N (7.3 KB at N = 16, 22.6 KB
 * at N = 32, 77.8 KB at N = 64), which leaves three, two and one robot per CU where the plain loop has four.
 * Cost: (one MI355X, 4096 standing robots x 200 control ticks, N = 32 x 10 ms): lmh_rollout_zoh itself is unchanged.  At
 * n_substeps = 1 the call takes 141.7 ms under an infinite box and 269.0 ms with bounds active on every tick, against 62.1 ms for
 * lmh_rollout_zoh and 227.8 / 467.0 ms for the host loop of four launches it replaces: 1.61 / 1.74 times faster than that loop.  At
 * n_substeps = 10 the call is NOT faster than the host loop, it is slower: 770.6 / 813.5 ms against 581.9 / 658.5 ms, because the hold
 * runs at two robots per CU where lmh_plant_step has four.  N = 16: 92.2 / 136.2 ms at n_substeps = 1; N = 64: 405 / 1462 ms.  Other batch
 * sizes, walking plans and anything multi-GPU were not measured. */
int lmh_rollout_zoh_box(lmh_handle *h, double *d_state, double *d_out, int32_t *d_status, const lmh_zoh_opts *opts,
                        const double *d_box, int n_samples, int n_sets, double *d_mpc, int n_ticks, int n_substeps, void *stream);

/* ---- Sensing and actuation between the controller and the plant of the zero-order-hold loop (build-defined; the reference QP has no torque
 * bounds and its loop no sensor or motor model): measurement error on what the controller reads, and a latency, a torque limit and a
 * first-order lag on what the plant receives, per robot and per joint, inside the one launch -- so a gain sweep or a push-recovery margin can
 * be taken with them without giving up the pushes inside holds, the trace and the on-chip metrics to a host loop.
 * ACTUATOR RECORDS (lmh_set_actuators; a table of the handle like the push schedule).  records: HOST [n_sets][LMH_ACT_STRIDE], n_sets = 1 (one
 * record shared by all robots) or n_instances; records = NULL or n_sets = 0 clears the table.  One record: TAU_MAX[24], the torque limit of
 * every joint, >= 0, +INFINITY = none | ALPHA[24], the lag coefficient of every joint, in (0, 1], 1 = no lag | DELAY, the latency in control
 * ticks, a whole number 0 .. LMH_ACT_MAX_DELAY | pad, ignored.  A NaN or negative limit, an alpha outside (0, 1] and a delay that is not a
 * whole number in range are refused (LMH_ERR_BAD_ARG; the text names the first offending robot, "robot 7: ..."); a refused or failed call
 * leaves the previous table in place (see lmh_set_refs: check first, build aside, replace in one step).  The table is a buffer of its own: it
 * travels in lmh_rollout_zoh_io's kernel arguments only, the parameter block and the per-robot blocks of lmh_set_params are not rebuilt,
 * and no other call reads it -- lmh_eval, lmh_rollout*, lmh_plant_* and lmh_rollout_zoh, _ref, _ex and _box are bit for bit what they are
 * without it.  lmh_get_actuators: robot `inst`'s record (the shared one on a shared table; the defaults inf | 1 | 0 on a handle without one).
 * ACTUATOR MEMORY (d_act_mem, DEVICE [B][LMH_ACT_MEM_STRIDE], the caller's, in/out): PREV[24], the torques the plant received on the last
 * control tick | QUEUE[LMH_ACT_MAX_DELAY][24], the commands on their way, oldest first; a robot of delay d uses slots 0 .. d-1 and touches no
 * other.  The caller fills it before the first launch (zeros, or a holding torque) and hands it on from launch to launch.
 * DEFINITION.  For every robot i the call leaves, bit for bit, what lmh_rollout_zoh_ex's host loop (above) leaves with its evaluation line
 * replaced and the torques of its tau30 taken from y (B = n_instances; control tick j of this launch):
 *         [the push due at the tick's start, as in lmh_rollout_zoh_ex]
 *         scratch = the state record;  if d_meas:  scratch[0:60] = state[0:60] + d_meas[j][i][0:60]        one fp64 add per word
 *         lmh_eval / lmh_eval_ref on scratch -> out, status           (the warm start through status[3] as ever)
 *         state[60:90] = scratch[60:90]                               v_prev is the controller's memory: the v it MEASURED
 *         cmd = out.tau
 *         if actuators (d = the robot's delay; for every joint):
 *             u = cmd                                                            if d == 0
 *             u = QUEUE[0];  QUEUE[0 .. d-2] = QUEUE[1 .. d-1];  QUEUE[d-1] = cmd     otherwise
 *             c = u > lim ? lim : (u < -lim ? -lim : u)               a NaN passes through; c != u on any joint raises LMH_FLAG_TAU_LIMIT
 *             y = c                                                   if alpha == 1 (PREV is not read)
 *             y = (alpha * c) + ((1 - alpha) * PREV)                  otherwise: the difference, both products and the sum each rounded, no
 *                                                                     fused multiply-add (numpy's expression gives the same bits)
 *             PREV = y
 *         else y = cmd
 *         d_applied[j][i] = y                                         when d_applied != NULL
 *         tau30 = [ wrench (6) | y (24) ];  the hold pieces, the pushes inside them, the sample and the fold: lmh_rollout_zoh_ex's, on the TRUE state
 * Consequences.  (a + b) equals (a) followed by (b) bit for bit with d_meas and d_applied advanced by a records per robot and d_act_mem handed
 * on, also when the delay is longer than a.  A trace sample holds the TRUE state after the hold; its v_prev words hold the measured v and its
 * out words are the evaluation's, so CoM and comVel there are those of the measured state.  d_log and the metrics' torque words stay the
 * COMMANDED torques (the fold of the trace is unchanged); XMIN, XMAX and FIRST_FALL are the true state's.  LMH_FLAG_TAU_LIMIT is informational:
 * it is outside the mask (& 15) of the metrics' FIRST_FLAG.  A NaN in a robot's d_meas words flags that robot as lmh_eval flags a NaN state
 * and disturbs no other.  actuators = 1 on a handle without records is legal and applies the defaults.
 * io == NULL, or a record of NULLs and zeros, is lmh_rollout_zoh_ex(h, ..., opts, ...) exactly: the same kernel is launched.  The
 * box-constrained loop (lmh_rollout_zoh_box) is NOT offered with these options.
 * Refusals, each LMH_ERR_BAD_ARG before anything is enqueued and with a message of its own: actuators or reserved outside its values;
 * actuators = 1 without d_act_mem; every refusal of lmh_rollout_zoh_ex.  The launch rules are lmh_rollout_zoh_ex's: LMH_PRECISION_FP64 handles
 * only, no launch slot, nothing written into the handle, capturable into a hipGraph as the first call on a fresh handle.  During the launch
 * words [0, 60) of a robot's d_state record hold its true state (the kernel parks it there across the evaluation).
 * Cost (one MI355X, 4096 standing robots x 200 control ticks): with nothing set the call launches lmh_rollout_zoh_ex's
 * kernel (62.3 against 62.1 ms, the parent commit's own timings: 61.4 .. 62.6 ms).  At n_substeps = 1 the measurement alone costs 1.5 %, the
 * actuator (delays 0 .. 3, a lag and a limit on every joint) 2.0 %, the applied torques 1.2 %, all three 2.4 % (63.6 ms: one millisecond above
 * the parent's slowest launch), and on top of every option of lmh_rollout_zoh_ex with an every-tick trace 3.3 % of that launch; at
 * n_substeps = 10 every row lies inside the parent's own range of timings (471 .. 487 ms).  Other batch sizes and anything multi-GPU were
 * not measured. */
#define LMH_ACT_STRIDE 56         /* one actuator record (doubles) */
#define LMH_ACT_OFF_TAU_MAX 0      /* [24] torque limit per joint, >= 0, +INFINITY = none */
#define LMH_ACT_OFF_ALPHA 24       /* [24] first-order lag coefficient per joint, in (0, 1]; 1 = no lag */
#define LMH_ACT_OFF_DELAY 48       /* latency in CONTROL ticks, a whole number 0 .. LMH_ACT_MAX_DELAY, as a double; [49, 56) pad, ignored */
#define LMH_ACT_MAX_DELAY 7
#define LMH_ACT_MEM_STRIDE 192     /* one robot's actuator memory (doubles): PREV[24] | QUEUE[7][24], oldest command first */
#define LMH_FLAG_TAU_LIMIT 128     /* informational: on some tick of the launch a joint's torque was cut to its limit */
int lmh_set_actuators(lmh_handle *h, const double *records, int n_sets);
int lmh_actuators_per_instance(const lmh_handle *h);      /* 0: none or one shared record, 1: one record per robot */
int lmh_get_actuators(lmh_handle *h, int inst, double *record);
typedef struct lmh_zoh_io {
    const double *d_meas;         /* DEVICE [n_ticks][B][60] or NULL: what is ADDED to q | v as control tick j's evaluation sees them */
    double *d_act_mem;            /* DEVICE [B][LMH_ACT_MEM_STRIDE], in/out; required when actuators = 1 */
    double *d_applied;            /* DEVICE [n_ticks][B][24] or NULL: the joint torques the plant received on every control tick */
    int32_t actuators;            /* 0 | 1: apply the handle's lmh_set_actuators records */
    int32_t reserved;             /* must be 0 */
} lmh_zoh_io;
int lmh_rollout_zoh_io(lmh_handle *h, double *d_state, double *d_out, int32_t *d_status, const lmh_zoh_opts *opts,
                       const lmh_zoh_io *io, int n_ticks, int n_substeps, void *stream);

/* ---- Joint servo inside the hold (build-defined; lmh_set_servo, a table of the handle like the actuator records): what a torque-controlled
 * humanoid has between its whole-body controller and its motors.  It runs at the plant's rate, not the controller's: a feed-forward torque
 * plus a per-joint PD law on a setpoint, re-formed at every derivative evaluation of the hold -- all four RK4 stages of every substep.
 * records: HOST [n_sets][LMH_SERVO_STRIDE], n_sets = 1 (one record for every robot) or n_instances; NULL or n_sets = 0 clears the table.
 * One record is KP[24] (N m / rad) | KD[24] (N m s / rad), a gain per joint.  CHECKS, each LMH_ERR_BAD_ARG naming the first offending robot
 * ("robot 7: ..."): every word finite and >= 0; n_sets 1 or n_instances.  lmh_set_refs' rule: check first, build aside, replace in one
 * step -- a refused or failed call leaves the previous table in place.  The table is a device buffer of its own (384 B per robot): the
 * parameter blocks of lmh_set_params are not rebuilt, and no call but the two below reads it -- lmh_eval*, lmh_rollout*, lmh_plant_step and
 * lmh_rollout_zoh, _ref, _ex, _io and _box are bit for bit what they are without it.  lmh_get_servo: robot `inst`'s record (the shared one
 * on a shared table; zeros on a handle without one).
 * THE SERVO'S TORQUE.  At a stage whose state is (q, v), row 6 + j of the tau30 the derivative uses is
 *         tau30[6+j] + ((kp_j * (q_des_j - q[6+j])) + (kd_j * (v_des_j - v[6+j])))
 * in this order: the two differences, the two products, their sum, then the sum with the feed-forward torque, each rounded by itself, no
 * fused multiply-add (numpy's expression gives the same bits; trajectories.servo_torque).  Rows 0..5, the wrench on the base, are untouched.
 * Zero gains add +0 to the feed-forward torque.  The device has ONE copy of the expression, used by both calls below.
 *
 * lmh_plant_step_servo: lmh_plant_step with that torque.  d_setpoint: DEVICE [B][LMH_SETPOINT_STRIDE], Q_DES[24] | V_DES[24], held for the
 * launch; required (NULL: LMH_ERR_BAD_ARG).  Everything else is lmh_plant_step's, word for word: t advances and v_prev stays, the flags,
 * (a + b) equals (a) followed by (b) bit for bit, n_substeps = 0 enqueues nothing, the contact-constant checks on a plant = 0 handle, per-robot
 * models and lmh_set_params contact constants, and the ground table of lmh_set_ground is honoured.  A handle without a servo table runs with
 * zero gains.  A NaN setpoint word of a joint with a gain makes that robot's state non-finite (LMH_FLAG_NONFINITE) and disturbs no other.
 *
 * lmh_rollout_zoh_servo.  DEFINITION.  For every robot the call leaves, bit for bit, what lmh_rollout_zoh_io's host loop (above) leaves with
 * every lmh_plant_step(s substeps) of a hold replaced by lmh_plant_step_servo(s substeps, setpoint_j):
 *         [the push due at the tick's start;  scratch, the measurement, lmh_eval / lmh_eval_ref on scratch -> out, status;  v_prev;  the
 *          actuator -> y;  d_applied[j][i] = y:  all as in lmh_rollout_zoh_io]
 *         setpoint_j = d_setpoint[j][i]                               LMH_SERVO_CALLER
 *         setpoint_j = (q_des | v_des) of                             LMH_SERVO_INTEGRATE
 *             q_m = scratch[6:30], v_m = scratch[36:60]               the joint words the evaluation READ: with d_meas the measured ones
 *             a   = out[42:66]                                        the joint rows of out.qdd of this tick's evaluation
 *             T   = (double)n_substeps * dt;   h2 = (0.5 * T) * T
 *             v_des = v_m + (T * a)
 *             q_des = (q_m + (T * v_m)) + (h2 * a)                    every product and sum rounded by itself, no fused multiply-add
 *                                                                     (numpy's expressions give the same bits; trajectories.servo_setpoint)
 *         tau30 = [ wrench (6) | y (24) ]
 *         for every piece of the hold (s substeps; the pushes inside the hold between the pieces, as in lmh_rollout_zoh_ex):
 *             lmh_plant_step_servo(state, tau30, setpoint_j, s)       the same setpoint serves every piece of control tick j's hold
 *         [the sample and the fold: lmh_rollout_zoh_ex's, on the TRUE state]
 * LMH_SERVO_INTEGRATE holds as the servo's target the state the controller's own acceleration reaches at the end of the control period.
 * Consequences.  The setpoint is not sent through the actuator's delay queue.  d_applied and d_log stay what they are, the feed-forward and
 * the commanded torques: the PD part changes at every stage and is not recorded.  The trace, the metrics fold, the status words and (a + b) =
 * (a) then (b) are lmh_rollout_zoh_io's; for (a + b), d_setpoint is advanced by a records per robot and d_act_mem is handed on.  The ground
 * table is honoured.  LMH_PRECISION_FP64 handles only; the call takes no launch slot, writes nothing into the handle and is capturable into
 * a hipGraph as the first call on a fresh handle.
 * servo == NULL or mode == 0 is lmh_rollout_zoh_io(h, ..., opts, io, ...) exactly: the same kernel is launched.  The box-constrained loop
 * (lmh_rollout_zoh_box) is NOT offered with a servo.
 * Refusals, each LMH_ERR_BAD_ARG before anything is enqueued and with a message of its own: a mode outside its values; a non-zero reserved;
 * LMH_SERVO_CALLER without d_setpoint; d_setpoint with another mode; LMH_SERVO_INTEGRATE with n_substeps == 0; every refusal of
 * lmh_rollout_zoh_io.
 * Cost (one MI355X, 4096 standing robots x 200 control ticks, a record per robot; scripts/servo_rate.py; other batch
 * sizes not measured): lmh_plant_step_servo 36.55 against lmh_plant_step's 36.48 ms (+0.2 %) at 200 x 1 substeps and 360.3 against 359.3 ms
 * (+0.3 %) at 200 x 10; lmh_rollout_zoh_servo against the same call with mode 0 (62.45 ms): LMH_SERVO_INTEGRATE 63.59 ms (+1.8 %),
 * LMH_SERVO_CALLER 63.13 ms (+1.1 %) at n_substeps = 1, and 479.0 / 478.9 against 469.9 ms (+1.9 %) at 10, where single launches spread
 * by 4 %.  Without a servo lmh_plant_step and lmh_rollout_zoh_io run at the parent commit's rate: their kernels are the parent's,
 * instruction for instruction.
 * What the servo does to the closed loop (scripts/servo_sweep.py, profiles/r32_servo_sweep.txt): on flat ground, from rest, with the
 * controller's default gains and LMH_SERVO_INTEGRATE, NO cell of a 16 x 15 grid of gains (kp_j = a m_j / dt^2, a = 0 and 1e-4 .. 1;
 * kd_j = b m_j / dt, b = 0 and 1e-3 .. 2.5; m_j the joint's own inertia) keeps a robot up for 2000 control ticks, at n_substeps = 1 or
 * 10.  Damping delays the fall -- from control tick 1655 without a servo to 1889 at best (a = 0.072, b = 0.75) at n_substeps = 1, from 165
 * to 248 at 10 -- and stiffness above a = 0.02 or damping above b = 1 brings it forward.  The zero-order-hold loop still does not stand. */
#define LMH_SERVO_STRIDE 48        /* one servo record (doubles) */
#define LMH_SERVO_OFF_KP 0         /* [24] proportional gain per joint, N m / rad, finite and >= 0 */
#define LMH_SERVO_OFF_KD 24        /* [24] derivative gain per joint, N m s / rad, finite and >= 0 */
#define LMH_SETPOINT_STRIDE 48     /* one setpoint record (doubles): Q_DES[24] | V_DES[24] */
#define LMH_SERVO_INTEGRATE 1      /* lmh_zoh_servo.mode: the setpoint integrated from the evaluation's own acceleration */
#define LMH_SERVO_CALLER 2         /* lmh_zoh_servo.mode: the caller's setpoints, one record per control tick and robot */
int lmh_set_servo(lmh_handle *h, const double *records, int n_sets);
int lmh_servo_per_instance(const lmh_handle *h);          /* 0: none or one shared record, 1: one record per robot */
int lmh_get_servo(lmh_handle *h, int inst, double *record);
int lmh_plant_step_servo(lmh_handle *h, double *d_state, const double *d_tau30, const double *d_setpoint, int n_substeps, int32_t *d_flags, void *stream);
typedef struct lmh_zoh_servo {
    const double *d_setpoint;     /* DEVICE [n_ticks][B][LMH_SETPOINT_STRIDE] with mode LMH_SERVO_CALLER, else NULL */
    int32_t mode;                 /* 0 off | LMH_SERVO_INTEGRATE 1 | LMH_SERVO_CALLER 2 */
    int32_t reserved;             /* must be 0 */
} lmh_zoh_servo;
int lmh_rollout_zoh_servo(lmh_handle *h, double *d_state, double *d_out, int32_t *d_status, const lmh_zoh_opts *opts,
                          const lmh_zoh_io *io, const lmh_zoh_servo *servo, int n_ticks, int n_substeps, void *stream);

/* ---- Rigid-contact plant inside the zero-order-hold loop (build-defined): lmh_rollout_zoh_io's loop with lmh_plant_step_rigid in every hold,
 * in one launch -- so the timed pushes inside holds, the wrench per tick, the trace, the on-chip metrics fold, caller-supplied CoM
 * references, measurement error, the actuator model and n_substeps > 1 can be used on the plant that stands, and the held set can change from
 * control tick to control tick without a return to the host.
 * lmh_rollout_zoh_rigid.  DEFINITION.  For every robot i the call leaves, bit for bit, what lmh_rollout_zoh_io's host loop (above) leaves with
 * every lmh_plant_step(s substeps) of a hold replaced by lmh_plant_step_rigid(state, tau30, mode_j, kv, s) (B = n_instances; control tick j of
 * this launch):
 *         [the push due at the tick's start;  scratch, the measurement, lmh_eval / lmh_eval_ref on scratch -> out, status;  v_prev;  the
 *          actuator -> y;  d_applied[j][i] = y:  all as in lmh_rollout_zoh_io]
 *         mode_j = d_mode[i]  (d_mode NULL: LMH_PHASE_DOUBLE)          LMH_RIGID_FIXED
 *         mode_j = d_mode[j][i]                                        LMH_RIGID_PER_TICK
 *         mode_j = phase[min(max(k, 0), n_samples - 1)]                LMH_RIGID_PLAN: the support phase of the robot's own plan (the shared one,
 *                                                                     or robot i's of lmh_gen_walk_batch / lmh_set_plans) at the preview index k
 *                                                                     this tick's evaluation reports in status[0], clamped into the arrays as
 *                                                                     the kernels clamp it; a plan without a phase array: LMH_PHASE_DOUBLE.
 *                                                                     This is trajectories.rigid_modes(phase, k) and nothing else.
 *         tau30 = [ wrench (6) | y (24) ]
 *         for every piece of the hold (s substeps; the pushes inside the hold between the pieces, as in lmh_rollout_zoh_ex):
 *             lmh_plant_step_rigid(state, tau30, mode_j, kv, s) -> lambda      one mode serves every piece of control tick j's hold
 *         d_lambda[j][i] = lambda of the LAST piece                   when d_lambda != NULL: the multiplier at the first stage of the last
 *                                                                     substep of tick j's hold (zeros when n_substeps == 0)
 *         [the sample and the fold: lmh_rollout_zoh_ex's, on the TRUE state]
 * Only the low two bits of a mode word are read, as in lmh_plant_step_rigid.
 * Inherited from lmh_rollout_zoh_io, word for word: where pushes fall, including inside holds; d_ref, the wrench sequence, d_meas, the
 * actuator and d_applied; the trace sample and the metrics fold, on the true state (WMIN / WMAX stay the controller's out.f, not the
 * multiplier); status[2] ORs the plant's flags over every stage, so LMH_FLAG_CONTACT_PULL and LMH_FLAG_CONTACT_SLIP arrive there, and both stay
 * outside the mask (& 15) of the metrics' FIRST_FLAG; (a + b) equals (a) followed by (b) bit for bit with the per-tick arrays advanced by a
 * records per robot -- d_mode (LMH_RIGID_PER_TICK) and d_lambda included -- and d_act_mem handed on.
 * THERE IS NO IMPACT MODEL.  A sole that becomes held while it moves keeps its twist and loses it as e^(-kv t): with kv = 0 it keeps it for
 * good.  The contact stays BILATERAL: a held sole that the ground would have to pull on is held all the same, and reported
 * (LMH_FLAG_CONTACT_PULL, LMH_FLAG_CONTACT_SLIP), never released.  Which soles are held is the caller's (or the plan's) decision alone.
 * lmh_rollout_zoh_rigid_impact (below) is this loop with the plastic impact at every touchdown; this call itself still has none.
 * Tables.  As the two rigid plant calls, the call reads nothing from the ground table (lmh_set_ground) and nothing from the servo table
 * (lmh_set_servo): it gives the same bytes with or without either.
 * rigid == NULL or source == 0 is lmh_rollout_zoh_io(h, ..., opts, io, ...) exactly: the same kernel is launched (on that handle's ground
 * table, then).  The box-constrained loop (lmh_rollout_zoh_box) and the joint servo (lmh_rollout_zoh_servo) are NOT offered with it.
 * Refusals, each LMH_ERR_BAD_ARG before anything is enqueued and with a message of its own: a source outside its values; a non-zero
 * reserved; a kv that is negative or not finite; LMH_RIGID_PER_TICK without d_mode; LMH_RIGID_PLAN with d_mode; every refusal of
 * lmh_rollout_zoh_io.  n_ticks == 0 enqueues nothing.  LMH_PRECISION_FP64 handles only; the call takes no launch slot, writes nothing into
 * the handle and is capturable into a hipGraph as the first call on a fresh handle.
 * Cost (one MI355X, 4096 standing robots x 200 control ticks, both soles held, kv = 50; scripts/zoh_rigid_rate.py; other
 * batch sizes and anything multi-GPU were not measured): the call is SLOWER than the host loop it replaces, stand_step ; plant_step_rigid --
 * 73.95 against 70.13 ms (x 1.054) at n_substeps = 1 and 597.8 against 491.3 ms (x 1.217) at 10 -- and x 1.19 / x 1.25 of lmh_rollout_zoh_io
 * with nothing set (62.03 / 478.7 ms); storing d_lambda adds 1.4 % / 0.1 %, LMH_RIGID_PER_TICK modes cost nothing measurable.  The hold runs
 * on one wave of the evaluation's two-wave workgroup; the plant kernel of the host loop is a one-wave workgroup.  What the call offers is the
 * family's options on this plant and one launch, not time.  lmh_rollout_zoh_io and lmh_plant_step_rigid run at the parent commit's rate:
 * their kernels are the parent's, instruction for instruction. */
#define LMH_RIGID_FIXED 1          /* lmh_zoh_rigid.source: d_mode [B], held for the launch; NULL = LMH_PHASE_DOUBLE for every robot */
#define LMH_RIGID_PER_TICK 2       /* lmh_zoh_rigid.source: d_mode [n_ticks][B], record j is control tick j's hold */
#define LMH_RIGID_PLAN 3           /* lmh_zoh_rigid.source: d_mode must be NULL, the robot's own plan decides */
typedef struct lmh_zoh_rigid {
    const int32_t *d_mode;        /* DEVICE, low two bits read, as lmh_plant_step_rigid */
    double *d_lambda;             /* DEVICE [n_ticks][B][12] or NULL */
    double kv;                    /* >= 0, finite: lmh_plant_step_rigid's */
    int32_t source;               /* 0 off | LMH_RIGID_FIXED 1 | LMH_RIGID_PER_TICK 2 | LMH_RIGID_PLAN 3 */
    int32_t reserved;             /* must be 0 */
} lmh_zoh_rigid;
int lmh_rollout_zoh_rigid(lmh_handle *h, double *d_state, double *d_out, int32_t *d_status, const lmh_zoh_opts *opts,
                          const lmh_zoh_io *io, const lmh_zoh_rigid *rigid, int n_ticks, int n_substeps, void *stream);

/* ---- The plastic impact inside the zero-order-hold loop (build-defined): lmh_rollout_zoh_rigid with lmh_plant_impact_rigid at every control
 * tick whose hold keeps a foot the hold before it did not.
 * lmh_rollout_zoh_rigid_impact.  DEFINITION.  lmh_rollout_zoh_rigid's host loop, as written out above, with one step between mode_j and the
 * hold of control tick j (held(m): the feet m & 3 holds; prev_i: d_mode_prev[i] & 3 on the launch's first tick):
 *         if held(mode_j) \ held(prev_i) is not empty:                                   a foot becomes held
 *             (v_plus, Lam, fl) = lmh_plant_impact_rigid(q, v of the TRUE state, mode_j)
 *             v <- v_plus ;  status flags |= fl ;  d_impulse[j][i] = Lam
 *         else:
 *             d_impulse[j][i] = 0  (all twelve words)
 *         prev_i = mode_j & 3
 * The push due at the tick's start, the measurement, the evaluation, v_prev, the actuator and d_applied all come before the impact, as in
 * lmh_rollout_zoh_rigid (the mode of LMH_RIGID_PLAN is only known behind the evaluation): the torques of tick j are those computed on the
 * pre-impact state, and v_prev, q and t are not touched by the impact.  The hold's pieces and the pushes inside it come after it; the trace
 * sample and the metrics fold are lmh_rollout_zoh_rigid's, on the state behind the hold.  The impact holds ALL the feet of mode_j, so a
 * touchdown into double support keeps the stance sole at rest.
 * d_mode_prev[i] leaves the launch with the last tick's mode & 3; n_ticks == 0 leaves it alone; only the low two bits of a word are read.
 * (a + b) equals (a) followed by (b) bit for bit with the per-tick arrays advanced (d_impulse included) and d_mode_prev handed on.  A caller
 * who wants no impact on the first tick hands in that tick's mode; LMH_PHASE_FLIGHT makes every foot held at tick 0 a touchdown.
 * impact == NULL or enable == 0 is lmh_rollout_zoh_rigid exactly: the same kernel and the same bytes.
 * Refusals, each LMH_ERR_BAD_ARG before anything is enqueued and with a message of its own: enable outside {0, 1}; a non-zero reserved;
 * enable without a rigid record whose source != 0; enable without d_mode_prev; every refusal of lmh_rollout_zoh_rigid.
 * LMH_PRECISION_FP64 handles only; no launch slot, nothing written into the handle, capturable as the first call on a fresh handle.
 * Not offered: restitution, friction-limited or unilateral impulses (LMH_FLAG_IMPULSE_PULL and LMH_FLAG_IMPULSE_SLIP report them in
 * status[2], nothing enforces them), a position-level term.
 * Cost (one MI355X, 4096 standing robots x 200 control ticks, kv = 50, n_substeps = 1 / 10; scripts/rigid_impact_rate.py, DESIGN.md round
 * 38; other batch sizes and anything multi-GPU were not measured): with enable = 1 and no foot ever newly held -- the price of the check, one
 * word loaded and stored per control tick -- 75.38 / 599.2 ms beside lmh_rollout_zoh_rigid's 75.50 / 596.7 ms in the same run, inside the
 * parent commit's own range of timings for that call (73.27 .. 77.85 and 596.9 .. 606.5 ms).  With the left sole landing on every second
 * control tick 81.86 / 598.5 ms against 77.31 / 593.6 ms for the same modes without the impact: about 0.05 ms per landing of 4096 robots,
 * 12 % of a control tick of one substep and 1.7 % of one of ten.  lmh_plant_impact_rigid alone: 0.0695 ms per launch beside
 * lmh_plant_derivative_rigid's 0.0791 ms (x 0.88: no Newton-Euler pass).  lmh_rollout_zoh_rigid runs at the parent commit's rate: its kernel
 * is the parent's, instruction for instruction.
 * What it says about walking on this plant (scripts/rigid_stand.py --zoh --impact, profiles/r38_rigid_stand.txt): on round 36's mode = "plan"
 * sweep the impact changes next to nothing -- no cell stands, first falls at control ticks 649 .. 1024 with and without it, 250 of 256
 * cells at the same tick -- and 245 of 256 cells raise LMH_FLAG_IMPULSE_PULL: the soles the plan puts down are moving away from the ground. */
typedef struct lmh_zoh_impact {
    int32_t *d_mode_prev;         /* DEVICE [B], in and out: the mode of the hold before this launch's first tick; after the launch, the last tick's */
    double *d_impulse;            /* DEVICE [n_ticks][B][12] or NULL */
    int32_t enable;               /* 0 off | 1 */
    int32_t reserved;             /* must be 0 */
} lmh_zoh_impact;
int lmh_rollout_zoh_rigid_impact(lmh_handle *h, double *d_state, double *d_out, int32_t *d_status, const lmh_zoh_opts *opts,
                                 const lmh_zoh_io *io, const lmh_zoh_rigid *rigid, const lmh_zoh_impact *impact, int n_ticks, int n_substeps, void *stream);

/* ---- LIPM preview MPC for a batch of reduced states (one kernel family of its own, one wave per robot, fp64): the stage of the controller
 * that lmh_eval runs between the momentum and the PD law, as calls of its own.
 * replaces: Mpc3dLip::compute (src/mpcLinearPendulum.cpp:78-109) for every robot of the handle, at that robot's own clock.
 * The calls read the handle's gain records (lmh_create's z_com, or per robot through lmh_set_zcom), its plan (shared or per robot), xscale,
 * mpc_dt, alpha, beta, gravity and the horizon, and write nothing into the handle: a later lmh_eval or lmh_rollout is bit for bit
 * unaffected.  They work on a handle of any precision and plant.  All pointers are DEVICE pointers; the calls are asynchronous on `stream`,
 * stage nothing on the host and take no launch slot, so they can be captured into a hipGraph from the first call on.  NULL for a required
 * pointer or a negative count returns LMH_ERR_BAD_ARG before anything is enqueued; a count of 0 enqueues nothing.
 *   d_lip     [B][LMH_LIP_STRIDE]            x | xdot | y | ydot | t | pad(3)   (LMH_LIP_OFF_*)
 *   d_mpc     [B][LMH_MPC_STRIDE]            one sample per robot                 (LMH_MPC_OFF_*)
 *   d_traj    [n_ticks][B][LMH_MPC_STRIDE]   sample-major like d_log
 *   d_preview [B][LMH_MPC_PREVIEW_STRIDE]    header | U_x U_y Z_x Z_y C_x Cv_x C_y Cv_y   (LMH_MPC_PREVIEW_OFF_*)
 *
 * lmh_mpc_step: k = (int)(t / mpc_dt);  u = -((sum K Px0 * x + sum K Px1 * xdot) - xscale_i * sum_j K_j z[k + j]) per axis (the y axis has
 * no xscale; every index k + j is pinned to the robot's sample array, as in lmh_eval);  xRef = (a00 x + a01 xdot + b0 u, a10 x + a11 xdot +
 * b1 u, u).  d_lip is read only.  The sample: xRef(3) | yRef(3) | zmp_x zmp_y | the state it was computed from (4) | its t | k | flags | 0.
 * zmp = x + D * u with D = -z_com / gravity of the robot's own z_com (the fp64 quotient the gain row was built from), the product and the
 * sum rounded separately (no fused multiply-add): numpy's x + D * u gives the same bits.  Flags: LMH_FLAG_ZMP_RANGE exactly as lmh_eval
 * raises it (k < 0 || k + N >= n_samples), LMH_FLAG_NONFINITE when one of the first eight words is not finite.
 * Definition, bit for bit: take a state on which lmh_eval leaves CoM, comVel, xRef, yRef in out[66:78] and k and the flags in status[0],
 * status[2]; the call with x = out[66], xdot = out[69], y = out[67], ydot = out[70] and that state's t leaves out[72:78] in words [0, 6), k
 * in word 13 and LMH_FLAG_ZMP_RANGE as status[2] & 4 (the step's kernel repeats the evaluation's window sum, gain sums and six
 * expressions operation for operation). */
int lmh_mpc_step(lmh_handle *h, const double *d_lip, double *d_mpc, void *stream);
/* The reduced model in closed loop, on chip: the CoM trajectory the LIPM tracks under the plan -- what trajectories.ik_targets / lmh_ik_batch
 * take as their com sequence, without a whole-body rollout.  Definition, bit for bit: n_ticks times { lmh_mpc_step, its sample to d_traj[j]
 * (d_traj may be NULL: no samples); x <- sample[0], xdot <- sample[1], y <- sample[3], ydot <- sample[4], t <- t + mpc_dt (one fp64 add per
 * tick, Clock::step's accumulation order: k is taken from the accumulated clock) }.  d_lip is updated in place (its pads are left alone).
 * Hence lmh_mpc_rollout(a + b) is lmh_mpc_rollout(a) followed by lmh_mpc_rollout(b).  A robot whose window runs off its plan keeps going on
 * the clamped window and carries LMH_FLAG_ZMP_RANGE in those samples only.  The gain row stays in registers for the launch; a tick is two
 * coalesced window loads, the wave reductions and ten flops. */
int lmh_mpc_rollout(lmh_handle *h, double *d_lip, int n_ticks, double *d_traj, void *stream);
/* The whole unconstrained solution at each robot's state, for plotting the predicted ZMP and CoM against the plan: H = alpha I + beta Pu'Pu,
 * g = beta Pu'(Px x_k - z) with z the same clamped, xscale-scaled window, U = -H^-1 g per axis, Z = Px x_k + Pu U and the N + 2 CoM states
 * c_0 = x_k, c_{j+1} = A c_j + B u_j.  d_lip is read only.  The handle keeps the gain row K = beta e0' H^-1 Pu' alone (U[0] = -K (Px x_k - z)
 * is lmh_mpc_step's u to rounding); here every robot's wave forms Pu and H from mpc_dt and its own D in LDS, factors H = L L' there and
 * solves both axes -- no (N + 1)^2 table per robot is kept.  About (N + 1)^3 / 3 multiply-adds per robot: a diagnostic call, of the cost
 * of a controller evaluation.  A pivot that is not positive raises LMH_FLAG_NOT_SPD in the header and leaves NaNs in the arrays (lmh_create
 * and lmh_set_zcom refuse such a Hessian, so a handle that exists does not get there); LMH_FLAG_NONFINITE: an entry is not finite. */
int lmh_mpc_preview(lmh_handle *h, const double *d_lip, double *d_preview, void *stream);

/* ---- The preview problem with the predicted ZMP held inside the support polygon (the reference hands its QP solver no bounds,
 * src/mpcLinearPendulum.cpp:120-127; build-defined).  Per robot and axis, with n = N + 1, p = Px x_k and z the clamped, xscale-scaled window
 * of lmh_mpc_preview:
 *     min_U  1/2 alpha |U|^2 + 1/2 beta |p + Pu U - z|^2     s.t.   lo_j <= (p + Pu U)_j <= hi_j,  j = 0 .. N
 * Pu is lower triangular with D != 0 on its diagonal, so the problem is feasible whenever lo_j <= hi_j, strictly convex (one solution), and
 * the Schur complement of every working set is positive definite.
 *   d_box  DEVICE [n_sets][4][n_samples], rows lo_x | hi_x | lo_y | hi_y (LMH_BOX_*), read at the same clamped indices k + j as z.  Metres,
 *          absolute: NOT multiplied by xscale (a sole does not stretch with the step length).  -INFINITY / +INFINITY: no bound.
 *          n_sets = 1: one set for every robot; n_sets = n_instances: one per robot.  n_samples must be lmh_num_ref_samples(h).
 * The wording and refusal rules are those of the lmh_mpc_* block above: NULL for a required pointer, a negative count, another n_samples or
 * an n_sets other than 1 or n_instances returns LMH_ERR_BAD_ARG before anything is enqueued; a count of 0 enqueues nothing; asynchronous on
 * `stream`, no launch slot, no host staging, nothing written into the handle (the bounds travel in the kernel arguments and the handle
 * keeps nothing of them), capturable from the first call.  One wave per robot, fp64, the factor of H and the working set's system in LDS.
 * Method: working-set rounds on lmh_mpc_preview's factor.  An iterate belongs to a working set W (each of its samples at one side, b_W the
 * bounds there): lambda_W = S^-1 (Z0_W - b_W) with S = Pu_W H^-1 Pu_W' and Z0 = p + Pu U0, U0 = -H^-1 g; U = -H^-1 (g + Pu' lambda);
 * Z = p + Pu U.  It is wrong at an inactive sample with Z_j < lo_j or Z_j > hi_j and at an active one whose multiplier has the wrong sign,
 * compared exactly in fp64.  Nothing wrong: done.  Otherwise a round: while the number of wrong samples has just reached a new minimum, or
 * at most three rounds after it did, all violated samples enter and all wrong-signed ones leave together; after that only the wrong sample
 * of the largest index changes (Judice-Pires, Kim-Park; the whole-body solver's bpp_rounds follows the same idea).  Every solve starts
 * from the empty working set.  After LMH_MPC_BOX_MAX_ROUNDS rounds of an axis without an end: LMH_FLAG_QP_MAXITER and the last iterate.
 * A window sample with !(lo <= hi) in either axis (a NaN bound included): LMH_FLAG_BOX_EMPTY, and NaNs for U, Z, lambda and the CoM
 * arrays.  Neither disturbs another robot.
 *
 * lmh_mpc_box_preview: d_record [B][LMH_MPC_BOX_STRIDE].  Words [0, 536) have lmh_mpc_preview's layout with U, Z and the CoM arrays of the
 * constrained solution; [3], [4]: rounds taken in x, in y; [5], [6]: active samples in x, in y; [7]: 0; then LAM_X and LAM_Y
 * (LMH_MPC_BOX_OFF_*), N + 1 used entries each, tails zero.  A multiplier is > 0 at an upper bound, < 0 at a lower bound and 0 exactly at
 * an inactive sample; for an active sample Z_j is written as the bound itself; without LMH_FLAG_QP_MAXITER every Z_j satisfies
 * lo_j <= Z_j <= hi_j exactly.  Flags: lmh_mpc_preview's, LMH_FLAG_QP_MAXITER, LMH_FLAG_BOX_EMPTY (LMH_FLAG_NONFINITE covers the
 * multipliers too; LMH_FLAG_NOT_SPD also when a working set's S has a pivot that is not positive).
 * Identities, bit for bit:
 *   (I1) lmh_mpc_box_step's words [0, 8) are formed from this record at the same state: u = U_X[0] / U_Y[0], x_next = A x + B u by
 *        lmh_mpc_step's expressions, the zmp words Z_X[0] / Z_Y[0].
 *   (I2) lmh_mpc_box_rollout is the host loop { lmh_mpc_box_step, move the state on, t += mpc_dt }; hence (a + b) is (a) followed by (b).
 *   (I3) where no bound ever enters a working set (rounds 0 in both axes, an all-infinite box for instance), the first 536 words are byte
 *        for byte lmh_mpc_preview's record: one copy of the set-up, factorisation and solves serves both kernels. */
int lmh_mpc_box_preview(lmh_handle *h, const double *d_lip, const double *d_box, int n_samples, int n_sets, double *d_record, void *stream);
/* One constrained step per robot: an LMH_MPC_STRIDE sample like lmh_mpc_step's with u = U[0] and zmp = Z[0] of the constrained solution
 * (I1), word LMH_MPC_OFF_ACTIVE the active samples of both axes, and LMH_FLAG_QP_MAXITER / LMH_FLAG_BOX_EMPTY / LMH_FLAG_NOT_SPD among
 * the flags (LMH_FLAG_NONFINITE: one of the first eight words is not finite).  d_lip is read only.  Unlike lmh_mpc_step, which applies a
 * stored gain row, every call forms and factors H: about 2 (N + 1)^3 multiply-adds per robot before the first round. */
int lmh_mpc_box_step(lmh_handle *h, const double *d_lip, const double *d_box, int n_samples, int n_sets, double *d_mpc, void *stream);
/* The closed loop of lmh_mpc_rollout with the constrained step (I2): d_lip is updated in place, d_traj [n_ticks][B][LMH_MPC_STRIDE] may be
 * NULL.  H does not depend on the state, so it is factored once per launch and stays in LDS with G = Pu H^-1 Pu'; every tick starts from
 * the empty working set (no warm start across ticks: it would break (I2)). */
int lmh_mpc_box_rollout(lmh_handle *h, double *d_lip, const double *d_box, int n_samples, int n_sets, int n_ticks, double *d_traj, void *stream);

/* host-buffer convenience used by the C++ shim (B instances, staged through internal
 * device buffers, synchronous): q/dq [B][30], t, outputs tau[B][24], f[B][12], qdd[B][30] */
int lmh_eval_host(lmh_handle *h, const double *q, const double *dq, double t,
                  double *tau, double *f, double *qdd, int32_t *status);
/* Robot::updateState + getCoM through host buffers: q [B][30] in, com [B][3] out */
int lmh_robot_com_host(lmh_handle *h, const double *q, double *com);
/* full out records of the last lmh_eval_host call: HOST [B][LMH_OUT_STRIDE] */
int lmh_last_out_host(lmh_handle *h, double *out);
/* Kinematics::compute + Robot::getCoM through host buffers: q [B][30] in/out, com [B][3] out, iters [B] out */
int lmh_ik_host(lmh_handle *h, double *q, const double *com_target, const double *rf6, const double *lf6, double *com, int32_t *iters);
/* lmh_terms through host buffers (Dynamics::computeAll of the shim): q [B][30], v [B][30] or NULL (= 0) in, terms [B][LMH_TERMS_STRIDE] out.
 * Staged through a device buffer the handle allocates on the first call; synchronous. */
int lmh_terms_host(lmh_handle *h, const double *q, const double *v, double *terms);
/* lmh_mpc_step through host buffers (Mpc3dLip::compute of the shim): lip [B][LMH_LIP_STRIDE] in, mpc [B][LMH_MPC_STRIDE] out.  Staged through a
 * device buffer the handle allocates on the first call; synchronous. */
int lmh_mpc_step_host(lmh_handle *h, const double *lip, double *mpc);
/* overwrite the staged Robot::v_ (v_prev) used by the next lmh_eval_host call: HOST [B][30] */
int lmh_set_prev_velocity_host(lmh_handle *h, const double *v);
/* hipStreamSynchronize(stream), then LMH_ERR_UNFINISHED if a completed lmh_rollout of this handle reported an incomplete launch (see there) */
int lmh_synchronize(lmh_handle *h, void *stream);

/* ---- end-of-run summary and on-disk records (the reference writes nothing but stdout,
 * apps/offline/main.cpp:86, so these formats are the build's own).
 * lmh_make_summary: DEVICE in (state/out/status as lmh_rollout leaves them), DEVICE out [B][LMH_SUMMARY_WIDTH]:
 *   base pose(6) | t | max|tau| | f_z R + f_z L | f_z R | f_z L | k | qp iterations | flags | active-bound count |
 *   checksum (sum of the 60 state doubles, in index order).  This record is what the one RCCL gather moves. */
int lmh_make_summary(lmh_handle *h, const double *d_state, const double *d_out, const int32_t *d_status, double *d_summary, void *stream);
/* Files: 64-byte little-endian header { char magic[8] "LMHSUM1\0" | "LMHLOG1\0" | "LMHTRJ1\0"; uint32 version = 1; uint32 dtype = 1 (f64);
 * uint64 n_instances; uint64 n_ticks (0 for a summary; the sample count of a trace); uint32 width (16 | 36 | 180); uint32 0; double dt
 * (a trace: the sample period trace_every * dt); double t0 (a trace: the clock of the first sample); uint64 0 }
 * followed by the raw f64 payload: summary [n][16]; log [n_ticks][n][36] = lmh_rollout's d_log copied to the host; trace
 * [n_samples][n][180] = lmh_rollout_trace's d_trace copied to the host.
 * HOST pointers.  Readers return LMH_ERR_BAD_ARG on a bad magic / version / size; `capacity` is in doubles. */
int lmh_write_summary(const char *path, const double *summary, uint64_t n_instances, double dt);
int lmh_read_summary(const char *path, double *summary, uint64_t capacity, uint64_t *n_instances, double *dt);
int lmh_write_log(const char *path, const double *log, uint64_t n_ticks, uint64_t n_instances, double dt, double t0);
int lmh_read_log(const char *path, double *log, uint64_t capacity, uint64_t *n_ticks, uint64_t *n_instances, double *dt, double *t0);
int lmh_write_trace(const char *path, const double *trace, uint64_t n_samples, uint64_t n_instances, double sample_dt, double t0);
int lmh_read_trace(const char *path, double *trace, uint64_t capacity, uint64_t *n_samples, uint64_t *n_instances, double *sample_dt, double *t0);

#ifdef __cplusplus
}
#endif
#endif
