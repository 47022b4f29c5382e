// lmh_capi.hip -- host side of the C ABI in include/lmh.h: owns the device-resident tables
// (model, MPC gain rows, ZMP / phase references, friction generators), launches the gfx950
// kernels in lmh_kernels.hip.  No CPU compute path exists: without a HIP device every entry
// point fails with LMH_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <utility>
#include <string>
#include <vector>
#include "../../include/lmh.h"
#include "lmh_device.h"
#include "lmh_nao_model.h"
#include "lmh_launch.h"

static thread_local std::string g_err;
static int fail(int code, const std::string &msg) { g_err = msg; return code; }
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(LMH_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

// The one owner of device memory in this file: move-only, freed in the destructor.  A buffer that is in use is never refilled: its
// replacement is built aside and move-assigned over it, so a call that fails half-way leaves the handle as it was.
template <class T> struct DevBuf {
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DevBuf &operator=(DevBuf &&o) noexcept { DevBuf old(std::move(o)); std::swap(p_, old.p_); return *this; }   // safe on itself
    ~DevBuf() { release(); }
    hipError_t alloc(size_t n) { release(); return hipMalloc(&p_, sizeof(T) * n); }
    hipError_t upload(const T *host, size_t n)
    {
        const hipError_t e = alloc(n);
        return (e != hipSuccess) ? e : hipMemcpy(p_, host, sizeof(T) * n, hipMemcpyHostToDevice);
    }
    T *get() const { return p_; }
private:
    void release() { if (p_) (void)hipFree(p_); p_ = nullptr; }
    T *p_ = nullptr;
};

// The reference plan of a handle: ZMP / phase samples and the piecewise foot references.  n_plans = 1: one plan shared by all robots;
// n_plans = n_instances > 1: every buffer holds one slice per robot.  phase may be empty on a shared plan (all double support); segs and
// seg_of_sample are empty while n_seg = 0 (the single polynomial set of lmh_set_foot_coeffs).
struct RefPlan {
    DevBuf<double> zx, zy, segs;
    DevBuf<uint8_t> phase;
    DevBuf<uint16_t> sos;
    int n_samples = 0, n_seg = 0, n_plans = 1;
    bool per_robot() const { return n_plans > 1; }
};

// A table of records the kernels read through their arguments (no part of the parameter block): [n_sets][width] on the device and on the host
// (what get returns), n_sets = 1 shared by all robots or n_instances, empty while n_sets = 0.  set and get are defined with the three tables below.
struct RecordTable {
    DevBuf<double> d;
    std::vector<double> h;
    int n_sets = 0;
    const double *device() const { return d.get(); }
    size_t stride(int width) const { return (n_sets > 1) ? (size_t)width : 0; }   // 0: shared or empty
    int set(const lmh_handle *hd, const char *who, const double *records, int n, int width, const char *(*rule)(const double *));
    int get(const lmh_handle *hd, int inst, double *record, int width, double (*default_word)(int)) const;
};

struct lmh_handle {
    int zoh_box_prepared = -1;   // what the runtime answered when lmh_create asked for lmh_rollout_zoh_box_kernel's dynamic LDS limit (hipSuccess = 0)
    lmh_config cfg;
    double mpc_dt = 0.0;              // resolved MPC sample time (cfg.mpc_dt, or cfg.dt when that is 0)
    int B = 0, device = 0, N = 0, n_models = 0, n_gain = 0;
    DevBuf<double> d_model, d_raw, d_mpc, d_gcol, d_xscale;
    RefPlan plan;                     // replaced as a whole, by commit_plan only
    DevBuf<double> d_pushes;          // timed velocity pushes [n_push_sets][n_push][LMH_PUSH_STRIDE] (lmh_set_pushes); empty while n_push = 0
    int n_push = 0, n_push_sets = 1;
    RecordTable act;                  // lmh_set_actuators, LMH_ACT_STRIDE: read by the io records of the zero-order-hold family alone
    RecordTable servo;                // lmh_set_servo, LMH_SERVO_STRIDE: read by lmh_plant_step_servo and lmh_rollout_zoh_servo alone
    RecordTable ground;               // lmh_set_ground, LMH_GROUND_STRIDE: read by the plant calls and the zero-order-hold family (the rigid plant apart)
    // Per-robot parameters (lmh_set_params): the records, one friction table per robot and the table of whole parameter blocks the controller
    // kernels select from.  All empty while the handle runs on its config's one set.  The block table is rebuilt by fill_params, i.e. by
    // every setter that moves a pointer or a stride, and replaces the previous one in one step.
    struct InstParams {
        std::vector<double> h_rec;    // [B][LMH_PARAM_STRIDE], what lmh_get_params returns
        DevBuf<double> d_rec, d_gcol; // the same on the device | [B][LMH_GCOL_STRIDE]
        DevBuf<LmhDevParams> d_blocks;
        bool on() const { return d_rec.get() != nullptr; }
    } inst;
    // staging for the host-buffer convenience calls
    DevBuf<double> d_state, d_out;
    DevBuf<double> d_terms;           // lmh_terms_host only: q | v | terms records, allocated on its first call
    DevBuf<double> d_mpc_host;        // lmh_mpc_step_host only: lip | mpc records, allocated on its first call
    DevBuf<int32_t> d_status;
    std::vector<double> h_state, h_out, h_gain;
    std::vector<int32_t> h_status;
    LmhDevParams P;
    // Launch slots of lmh_rollout: the kernel reads its parameter block through a pointer and draws robots from a ticket word, so every
    // launch in flight needs its own copy of both.  Slot i is reused by launch i + kSlots, after the event recorded behind launch i has
    // completed (normally long ago): launches on different streams of one handle never share a block that is being rewritten.
    static constexpr int kSlots = 8;
    struct Slot {
        DevBuf<LmhDevParams> d_P;     // device copy read by the rollout kernel
        DevBuf<int> d_ticket;         // work-unit counters, ring queue of robots, ticks done per robot (4 + 2 B ints, all zero between launches: the kernel leaves them so)
        hipEvent_t done = nullptr;    // recorded behind the last launch that used this slot; non-null = the slot has all three
        LmhDevParams P_dev;           // what d_P currently holds
        bool valid = false, used = false;
        bool checked = true;          // the error word of the last launch on this slot (d_ticket[3]) has been read
        ~Slot() { if (done) (void)hipEventDestroy(done); }
        bool ready() const { return done != nullptr; }
        // acquires the parameter block, the zeroed ticket words and the event, or nothing: a failure releases what it got so far and leaves
        // the slot empty, and the next lmh_rollout that draws it tries again
        hipError_t init(int n_instances, hipStream_t s)
        {
            const size_t words = 4 + 2 * (size_t)n_instances;          // counters | error word | ring of robots | ticks done per robot
            DevBuf<LmhDevParams> p;
            DevBuf<int> t;
            hipEvent_t ev = nullptr;
            hipError_t e = p.alloc(1);
            if (e == hipSuccess) e = t.alloc(words);
            if (e == hipSuccess) e = hipMemsetAsync(t.get(), 0, words * sizeof(int), s);   // stream-ordered in front of the first launch on the slot
            if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);  // last, so that nothing is left to undo by hand
            if (e == hipSuccess) { d_P = std::move(p); d_ticket = std::move(t); done = ev; }
            return e;
        }
    } slot[kSlots];
    unsigned next_slot = 0;
};

extern "C" const char *lmh_last_error(void) { return g_err.c_str(); }

extern "C" int lmh_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" void lmh_config_default(lmh_config *c)
{
    std::memset(c, 0, sizeof(*c));
    c->dt = 0.01; c->time_horizon = 0.5; c->z_com = 0.26;          // apps/offline/main.cpp:13-14,31,38
    c->gravity = 9.81; c->alpha = 1e-3; c->beta = 1.0;              // mpcLinearPendulum.hpp:46-48
    c->mu = 0.7;                                                    // controller.hpp:81
    c->kp_joints = 300; c->kd_joints = 34;                          // controller.hpp:102-103
    c->kp_mom = 10; c->kd_mom = 6.32;                               // :106-107
    c->kp_feet = 500; c->kd_feet = 44;                              // :110-111
    c->w_com_lin = 4000; c->w_com_ang = 0; c->w_base_pos = 10; c->w_base_ang = 10;   // :118-121
    c->w_joints = 1; c->w_force = 1; c->w_foot = 100000;            // :122-124
    c->eps_coeff = 1e-8;                                            // controller.cpp:117
    c->warm_start = 1; c->max_qp_iters = 64; c->precision = LMH_PRECISION_FP64; c->bpp_rounds = 0;
    c->plant = 0; c->contact_k = 2.0e4; c->contact_d = 3.0; c->contact_dt = 3.0; c->contact_mu = 0.7;
    c->mpc_dt = 0.0;                                                // = dt (apps/offline/main.cpp:18,21,39 pass one value to Clock, ZMP and Mpc3dLip)
}

extern "C" void lmh_nominal_links(double *raw) { std::memcpy(raw, kLmhNaoLinks, sizeof(kLmhNaoLinks)); }

// ---- Mpc3dLip::initialize (src/mpcLinearPendulum.cpp:41-68) + the algebraic gain row:
// u = -H^-1 g, g = beta Pu'(Px x - z), H = alpha I + beta Pu'Pu  =>  u0 = -K (Px x - z),
// K = beta e0' H^-1 Pu'.  Record layout: K | Px[:,0] | Px[:,1] | zcom | D | pad(2); D = -zcom / gravity is the quotient Pu is built from
// here, carried for the lmh_mpc_* kernels (the controller kernels and lmh_get_mpc_gain do not read that word).
static int build_gain_row(const lmh_config &c, double dt /* MPC sample time */, double zcom, int N, double *rec)
{
    const int n = N + 1;
    std::vector<double> Pu((size_t)n * n, 0.0), H((size_t)n * n), h0(n, 0.0);
    double A[4] = {1, dt, 0, 1}, B[2] = {(dt * dt) / 2, dt}, Ap[4] = {1, 0, 0, 1};
    const double D = -zcom / c.gravity;
    double *K = rec, *px0 = rec + n, *px1 = rec + 2 * n;
    px0[0] = 1; px1[0] = 0;
    Pu[0] = D;
    for (int i = 1; i <= N; i++) {
        double t[4] = {Ap[0] * A[0] + Ap[1] * A[2], Ap[0] * A[1] + Ap[1] * A[3], Ap[2] * A[0] + Ap[3] * A[2], Ap[2] * A[1] + Ap[3] * A[3]};
        std::memcpy(Ap, t, sizeof(t));
        px0[i] = Ap[0]; px1[i] = Ap[1];                             // C = [1 0]
        Pu[(size_t)i * n + i - 1] = B[0];
        Pu[(size_t)i * n + i] = D;
        double Aj[4] = {1, 0, 0, 1};
        for (int j = 1; j <= N - i; j++) {
            double u[4] = {Aj[0] * A[0] + Aj[1] * A[2], Aj[0] * A[1] + Aj[1] * A[3], Aj[2] * A[0] + Aj[3] * A[2], Aj[2] * A[1] + Aj[3] * A[3]};
            std::memcpy(Aj, u, sizeof(u));
            Pu[(size_t)(i + j) * n + i - 1] = Aj[0] * B[0] + Aj[1] * B[1];
        }
    }
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
            double s = 0;
            for (int l = 0; l < n; l++) s += Pu[(size_t)l * n + i] * Pu[(size_t)l * n + j];
            H[(size_t)i * n + j] = ((i == j) ? c.alpha : 0.0) + c.beta * s;
        }
    for (int j = 0; j < n; j++) {                                   // Cholesky (lower)
        double d = H[(size_t)j * n + j];
        for (int k = 0; k < j; k++) d -= H[(size_t)j * n + k] * H[(size_t)j * n + k];
        if (!(d > 0)) return 1;
        d = std::sqrt(d);
        H[(size_t)j * n + j] = d;
        for (int i = j + 1; i < n; i++) {
            double s = H[(size_t)i * n + j];
            for (int k = 0; k < j; k++) s -= H[(size_t)i * n + k] * H[(size_t)j * n + k];
            H[(size_t)i * n + j] = s / d;
        }
    }
    std::vector<double> y(n, 0.0);
    for (int i = 0; i < n; i++) {                                   // H h0 = e0
        double s = (i == 0) ? 1.0 : 0.0;
        for (int k = 0; k < i; k++) s -= H[(size_t)i * n + k] * y[k];
        y[i] = s / H[(size_t)i * n + i];
    }
    for (int i = n - 1; i >= 0; i--) {
        double s = y[i];
        for (int k = i + 1; k < n; k++) s -= H[(size_t)k * n + i] * h0[k];
        h0[i] = s / H[(size_t)i * n + i];
    }
    for (int i = 0; i < n; i++) {
        double s = 0;
        for (int j = 0; j < n; j++) s += Pu[(size_t)i * n + j] * h0[j];
        K[i] = c.beta * s;
    }
    rec[3 * n] = zcom; rec[3 * n + 1] = D; rec[3 * n + 2] = rec[3 * n + 3] = 0.0;
    return 0;
}

// friction-cone generators: column j = 16 foot + 4 vertex + edge  ->  [p_v x ray_e ; ray_e]
// (src/controller.cpp:33-36,185-270, vertices src/Robot.cpp:38-42; same for both feet)
static void build_gcol(double mu, double *g /*[16][6] (one foot; both feet are identical) | (G G')^-1 [6][6] | G'(G G')^-1 [16][6]*/)
{
    const double ray[4][3] = {{mu, 0, 1}, {0, mu, 1}, {-mu, 0, 1}, {0, -mu, 1}};
    const double vtx[4][3] = {{0.1, 0.025, 0}, {0.1, -0.025, 0}, {-0.05, 0.025, 0}, {-0.05, -0.025, 0}};
    {
        for (int v = 0; v < 4; v++)
            for (int e = 0; e < 4; e++) {
                double *o = g + 6 * (4 * v + e);
                const double *p = vtx[v], *r = ray[e];
                // crossMatrix(p) * ray, term by term as the dense product does
                o[0] = 0 * r[0] + (-p[2]) * r[1] + p[1] * r[2];
                o[1] = p[2] * r[0] + 0 * r[1] + (-p[0]) * r[2];
                o[2] = (-p[1]) * r[0] + p[0] * r[1] + 0 * r[2];
                o[3] = r[0]; o[4] = r[1]; o[5] = r[2];
            }
    }
    // Gamma = G_f G_f' (6x6, identical for both feet), its inverse and the min-norm map G_f' Gamma^-1
    double Gm[36] = {0}, A[6][12];
    for (int a = 0; a < 6; a++)
        for (int b = 0; b < 6; b++)
            for (int j = 0; j < 16; j++) Gm[6 * a + b] += g[6 * j + a] * g[6 * j + b];
    for (int a = 0; a < 6; a++)
        for (int b = 0; b < 12; b++) A[a][b] = (b < 6) ? Gm[6 * a + b] : ((b - 6 == a) ? 1.0 : 0.0);
    for (int c = 0; c < 6; c++) {                                   // Gauss-Jordan with partial pivoting
        int pv = c;
        for (int rr = c + 1; rr < 6; rr++) if (std::fabs(A[rr][c]) > std::fabs(A[pv][c])) pv = rr;
        for (int b = 0; b < 12; b++) std::swap(A[c][b], A[pv][b]);
        const double d = A[c][c];
        for (int b = 0; b < 12; b++) A[c][b] /= d;
        for (int rr = 0; rr < 6; rr++)
            if (rr != c) { const double f = A[rr][c]; for (int b = 0; b < 12; b++) A[rr][b] -= f * A[c][b]; }
    }
    double *gi = g + 96, *gp = g + 96 + 36;
    for (int a = 0; a < 6; a++)
        for (int b = 0; b < 6; b++) gi[6 * a + b] = 0.5 * (A[a][6 + b] + A[b][6 + a]);
    for (int j = 0; j < 16; j++)
        for (int b = 0; b < 6; b++) {
            double sacc = 0;
            for (int a = 0; a < 6; a++) sacc += g[6 * j + a] * gi[6 * a + b];
            gp[6 * j + b] = sacc;
        }
}

// Local-transform coefficient table: entry e = 12 slot + 4 row + col of slot's 3x4 transform equals
// c0 + c1 cos(theta_slot) + c2 sin(theta_slot).  Slots 0..24 are the Khalil modified-DH transforms of
// matTrans (src/Robot.cpp:176-223; tables :180-196) with the shoulder / head offsets of :134,143,152 folded
// into the translations of slots 12, 17, 22; slots 25..27 are auxT01, auxT09 (0.7071 literals, :92-103) and
// the sole offset (:106-117).  cos/sin(alpha) are libm's values for the reference's pi literal.
static void build_lcoef(double *t /*[336][3]*/)
{
    const double pi = 3.14159265358979323846, h = pi / 2;
    const double r[25] = {-0.07071, 0, 0, 0, 0, 0, 0.07071, 0, 0, 0, 0, 0, 0, 0, 0.105, 0, 0.05595, 0, 0, 0.105, 0, 0.05595, 0, 0, 0};
    const double d[25] = {0, 0, 0, -0.1, -0.1029, 0, 0, 0, 0, -0.1, -0.1029, 0, 0, 0, -0.015, 0, 0, 0, 0, -0.015, 0, 0, 0, 0, 0.030};
    const double al[25] = {0, h, h, 0, 0, -h, -h, -h, h, 0, 0, -h, -h, h, h, -h, h, h, h, h, -h, h, 0, -h, 0};
    const double aux[3][12] = {{0, -1, 0, 0, 0.7071, 0, 0.7071, 0, -0.7071, 0, 0.7071, 0},
                               {1, 0, 0, 0, 0, 0.7071, 0.7071, 0, 0, -0.7071, 0.7071, 0},
                               {1, 0, 0, -0.0452, 0, 1, 0, 0, 0, 0, 1, 0}};
    std::memset(t, 0, sizeof(double) * 3 * 336);
    for (int s = 0; s < 25; s++) {
        const double ca = std::cos(al[s]), sa = std::sin(al[s]);
        double *e = t + 3 * 12 * s;
        // row 0: ct, -st, 0, d
        e[3 * 0 + 1] = 1.0; e[3 * 1 + 2] = -1.0; e[3 * 3 + 0] = d[s];
        // row 1: ca st, ca ct, -sa, -r sa
        e[3 * 4 + 2] = ca; e[3 * 5 + 1] = ca; e[3 * 6 + 0] = -sa; e[3 * 7 + 0] = -r[s] * sa;
        // row 2: sa st, sa ct, ca, r ca
        e[3 * 8 + 2] = sa; e[3 * 9 + 1] = sa; e[3 * 10 + 0] = ca; e[3 * 11 + 0] = r[s] * ca;
        if (s == 12 || s == 17 || s == 22) {
            e[3 * 3 + 0] = e[3 * 3 + 0] + 0.0;
            e[3 * 7 + 0] = e[3 * 7 + 0] + ((s == 12) ? -0.098 : (s == 17) ? 0.098 : 0.0);
            e[3 * 11 + 0] = e[3 * 11 + 0] + ((s == 22) ? 0.1615 : 0.13591);
        }
    }
    for (int s = 25; s < 28; s++)
        for (int k = 0; k < 12; k++) t[3 * (12 * s + k)] = aux[s - 25][k];
}

// the table of per-robot blocks from the block `base` (its inst_blocks aside): built aside, complete when this returns
static int expand_blocks(const lmh_handle *h, LmhDevParams base, const double *d_rec, const double *d_gcol, DevBuf<LmhDevParams> &table)
{
    base.inst_blocks = nullptr;
    HIPCHK(table.alloc((size_t)h->B));
    lmh_launch_params_expand(&base, d_rec, d_gcol, table.get(), h->B, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());                                  // the setter waits for the kernel; no launch in flight reads the old table either
    return LMH_OK;
}

// Every setter that moves a pointer, a stride or a shared scalar ends here: it has put its new buffers into the handle, and this forms the
// block that goes with them.  With per-robot parameters on, the block table is written again from that block, into a table of its own, so
// that no robot's block ever holds a stale pointer.  The handle's block and table are replaced together at the end; if the table cannot be
// built (allocation or launch) neither is touched, and the setter puts its previous buffers back: the call fails as a whole.
// the FK coefficient table sits behind the handle's friction table (create_body): the one statement of where
static const double *lcoef_of(const lmh_handle *h) { return h->d_gcol.get() + LMH_GCOL_STRIDE; }

static int fill_params(lmh_handle *h)
{
    LmhDevParams P = h->P;                                           // (the foot polynomials live in the block alone)
    const lmh_config &c = h->cfg;
    const RefPlan &r = h->plan;
    P.model = h->d_model.get(); P.mpc = h->d_mpc.get(); P.gcol = h->d_gcol.get(); P.xscale = h->d_xscale.get();
    P.lcoef = lcoef_of(h);
    P.zmpx = r.zx.get(); P.zmpy = r.zy.get(); P.phase = r.phase.get(); P.segs = r.segs.get(); P.seg_of_sample = r.sos.get();
    P.n_seg = r.n_seg; P.ref_stride = r.per_robot() ? r.n_samples : 0; P.seg_stride = r.per_robot() ? r.n_seg : 0;
    P.pushes = h->d_pushes.get(); P.n_push = h->n_push; P.push_stride = (h->n_push_sets > 1) ? h->n_push : 0;
    P.model_stride = (h->n_models > 1) ? LMH_MODEL_STRIDE : 0;
    P.mpc_stride = 3 * (h->N + 1) + 4;
    P.mpc_stride_inst = (h->n_gain > 1) ? P.mpc_stride : 0;
    P.n_samples = r.n_samples; P.horizon = h->N; P.n_instances = h->B;
    P.warm_start = c.warm_start; P.max_qp_iters = c.max_qp_iters; P.precision = c.precision;
    P.bpp_max = (c.bpp_rounds == 0) ? 10 : c.bpp_rounds;            // < 0: Lawson-Hanson from the empty set (diagnostic)
    P.plant = c.plant; P.contact_k = c.contact_k; P.contact_d = c.contact_d; P.contact_dt = c.contact_dt; P.contact_mu = c.contact_mu;
    P.dt = c.dt; P.mpc_dt = h->mpc_dt;
    P.kp_joints = c.kp_joints; P.kd_joints = c.kd_joints; P.kp_mom = c.kp_mom; P.kd_mom = c.kd_mom;
    P.kp_feet = c.kp_feet; P.kd_feet = c.kd_feet;
    P.w_com_lin = c.w_com_lin; P.w_com_ang = c.w_com_ang; P.w_base_pos = c.w_base_pos; P.w_base_ang = c.w_base_ang;
    P.w_joints = c.w_joints; P.w_force = c.w_force; P.w_foot = c.w_foot; P.eps_coeff = c.eps_coeff;
    P.inv_w_base_pos = 1.0 / c.w_base_pos; P.inv_w_base_ang = 1.0 / c.w_base_ang; P.inv_w_joints = 1.0 / c.w_joints;
    P.inv_w_com_lin = 1.0 / c.w_com_lin; P.inv_w_foot = 1.0 / c.w_foot;
    const double md = h->mpc_dt;                                     // mpcLinearPendulum.cpp:45-47 with the Mpc3dLip ctor's dt
    P.a00 = 1; P.a01 = md; P.a10 = 0; P.a11 = 1; P.b0 = (md * md) / 2; P.b1 = md;
    P.inst_blocks = nullptr;
    if (h->inst.on()) {
        DevBuf<LmhDevParams> table;
        const int rc = expand_blocks(h, P, h->inst.d_rec.get(), h->inst.d_gcol.get(), table);
        if (rc != LMH_OK) return rc;                                 // the handle still has its previous block and table
        h->inst.d_blocks = std::move(table);
        P.inst_blocks = h->inst.d_blocks.get();
    }
    h->P = P;
    return LMH_OK;
}

// The one setter transaction.  swap() exchanges members of the handle with what the caller has just built aside, so the one statement is
// both the change and its undo: if the block (or, with per-robot parameters, the block table) cannot be formed for the new members, the
// second swap() puts the previous ones back and the call fails as a whole.  What ends up in the caller's locals dies with them.
template <class Swap> static int commit(lmh_handle *h, Swap swap)
{
    swap();
    const int rc = fill_params(h);
    if (rc != LMH_OK) swap();
    return rc;
}

static int upload_gain(lmh_handle *h, const double *zcom, int n)
{
    const int stride = 3 * (h->N + 1) + 4;
    std::vector<double> rows((size_t)n * stride, 0.0);
    for (int i = 0; i < n; i++)
        if (build_gain_row(h->cfg, h->mpc_dt, zcom[i], h->N, rows.data() + (size_t)i * stride))
            return fail(LMH_ERR_BAD_ARG, "MPC Hessian not positive definite");
    DevBuf<double> d;
    HIPCHK(d.upload(rows.data(), rows.size()));
    return commit(h, [&] { std::swap(h->d_mpc, d); h->h_gain.swap(rows); std::swap(h->n_gain, n); });
}

// ---------------------------------------------------------------------------- the rules of a configuration
// the config's values in the record's order (LMH_PARAM_OFF_*)
static void config_record(const lmh_config &c, double *r)
{
    const double v[LMH_PARAM_STRIDE] = {c.mu, c.kp_joints, c.kd_joints, c.kp_mom, c.kd_mom, c.kp_feet, c.kd_feet,
                                        c.w_com_lin, c.w_com_ang, c.w_base_pos, c.w_base_ang, c.w_joints, c.w_force, c.w_foot, c.eps_coeff,
                                        c.contact_k, c.contact_d, c.contact_dt, c.contact_mu, 0.0};
    std::memcpy(r, v, sizeof(v));
}

// The rules of one parameter record, stated once: lmh_create applies them to its config's record, lmh_set_params to every robot's, the
// plant calls the contact rule alone.  nullptr = fine.  Every literal the kernels divide by or take a Cholesky pivot from must be positive
// (a zero weight is 1/0 in the Woodbury set-up; the reference has no such check because its literals are compile-time constants).
static const char *contact_error(const double *r)
{
    if (!(r[LMH_PARAM_OFF_CONTACT_K] > 0.0) || !(r[LMH_PARAM_OFF_CONTACT_D] >= 0.0) || !(r[LMH_PARAM_OFF_CONTACT_DT] >= 0.0) || !(r[LMH_PARAM_OFF_CONTACT_MU] >= 0.0))
        return "contact_k must be positive, contact_d / contact_dt / contact_mu non-negative";
    return nullptr;
}

static const char *param_record_error(const double *r, bool plant)
{
    if (!(r[LMH_PARAM_OFF_MU] > 0.0)) return "mu must be positive";
    if (!(r[LMH_PARAM_OFF_EPS_COEFF] > 0.0)) return "eps_coeff must be positive";
    for (int o : {LMH_PARAM_OFF_W_COM_LIN, LMH_PARAM_OFF_W_BASE_POS, LMH_PARAM_OFF_W_BASE_ANG, LMH_PARAM_OFF_W_JOINTS, LMH_PARAM_OFF_W_FORCE, LMH_PARAM_OFF_W_FOOT})
        if (!(r[o] > 0.0)) return "weights w_com_lin, w_base_pos, w_base_ang, w_joints, w_force, w_foot must be positive";
    if (!(r[LMH_PARAM_OFF_W_COM_ANG] >= 0.0)) return "w_com_ang must be >= 0";
    for (int o = LMH_PARAM_OFF_KP_JOINTS; o <= LMH_PARAM_OFF_KD_FEET; o++) if (!std::isfinite(r[o])) return "PD gains must be finite";
    return plant ? contact_error(r) : nullptr;
}

// The fields that are not in the record, around the record's rules.  The order of the refusals is part of the interface: the contact
// rule is asked after max_qp_iters and plant, as it always was, so the record is walked without it first.
static const char *validate_config(const lmh_config *c)
{
    if (!(c->dt > 0.0) || !(c->time_horizon > 0.0)) return "dt and time_horizon must be positive";
    if (!(c->mpc_dt >= 0.0) || !std::isfinite(c->mpc_dt)) return "mpc_dt must be >= 0 (0 = dt)";
    if (!(c->z_com > 0.0) || !(c->gravity > 0.0)) return "z_com and gravity must be positive";
    if (!(c->alpha > 0.0) || !(c->beta > 0.0)) return "alpha and beta must be positive";
    double rec[LMH_PARAM_STRIDE];
    config_record(*c, rec);
    if (const char *why = param_record_error(rec, false)) return why;
    if (c->max_qp_iters < 1) return "max_qp_iters must be >= 1";
    if (c->plant != 0 && c->plant != 1) return "plant must be 0 or 1";
    if (const char *why = c->plant ? contact_error(rec) : nullptr) return why;
    if (c->precision != LMH_PRECISION_FP64 && c->precision != LMH_PRECISION_MIXED && c->precision != LMH_PRECISION_FP32)
        return "precision must be LMH_PRECISION_FP64, LMH_PRECISION_MIXED or LMH_PRECISION_FP32";
    return nullptr;
}

static int create_body(lmh_handle *h, const lmh_config *cfg, int n_instances)
{
    std::memset(&h->P, 0, sizeof(h->P));
    double g[LMH_GCOL_STRIDE + 3 * 336];
    build_gcol(cfg->mu, g);
    build_lcoef(g + LMH_GCOL_STRIDE);
    HIPCHK(h->d_gcol.upload(g, sizeof(g) / sizeof(double)));
    HIPCHK(h->d_state.alloc(LMH_STATE_STRIDE * (size_t)n_instances));
    HIPCHK(h->d_out.alloc(LMH_OUT_STRIDE * (size_t)n_instances));
    HIPCHK(h->d_status.alloc(LMH_STATUS_STRIDE * (size_t)n_instances));
    HIPCHK(hipMemset(h->d_state.get(), 0, sizeof(double) * LMH_STATE_STRIDE * (size_t)n_instances));
    HIPCHK(hipMemset(h->d_status.get(), 0, sizeof(int32_t) * LMH_STATUS_STRIDE * (size_t)n_instances));
    h->h_state.assign((size_t)LMH_STATE_STRIDE * n_instances, 0.0);
    h->h_out.assign((size_t)LMH_OUT_STRIDE * n_instances, 0.0);
    h->h_status.assign((size_t)LMH_STATUS_STRIDE * n_instances, 0);
    int rc = lmh_set_model(h, nullptr, 1);
    if (rc == LMH_OK) rc = upload_gain(h, &cfg->z_com, 1);
    if (rc == LMH_OK) rc = lmh_set_refs_stance(h, 5.0, 2);
    if (rc == LMH_OK) {                                             // constant foot references at (0, -/+0.05, 0)
        double r[24] = {0}, l[24] = {0};
        int32_t n[3] = {6, 6, 8};
        r[8] = -0.05; l[8] = 0.05;
        rc = lmh_set_foot_coeffs(h, r, n, l, n);
    }
    return rc;
}

extern "C" int lmh_create(const lmh_config *cfg, int n_instances, int device, lmh_handle **out)
{
    if (!cfg || !out || n_instances < 1) return fail(LMH_ERR_BAD_ARG, "lmh_create: bad argument");
    *out = nullptr;
    if (const char *why = validate_config(cfg)) return fail(LMH_ERR_BAD_ARG, std::string("lmh_create: ") + why);
    const double mpc_dt = (cfg->mpc_dt > 0.0) ? cfg->mpc_dt : cfg->dt;
    const int N = (int)(cfg->time_horizon / mpc_dt);                // mpcLinearPendulum.cpp:43
    if (N < 1 || N > LMH_MAX_HORIZON) return fail(LMH_ERR_BAD_ARG, "horizon N = time_horizon/mpc_dt must be in [1, 64]");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(LMH_ERR_NO_DEVICE, "no HIP device: the controller has no CPU path");
    if (device < 0 || device >= ndev) return fail(LMH_ERR_BAD_ARG, "lmh_create: device index out of range");
    HIPCHK(hipSetDevice(device));
    lmh_handle *h = new lmh_handle();
    h->cfg = *cfg; h->B = n_instances; h->device = device; h->N = N; h->mpc_dt = mpc_dt;
    const int rc = create_body(h, cfg, n_instances);                // every failure path releases what was allocated so far
    if (rc != LMH_OK) { std::string keep = g_err; lmh_destroy(h); g_err = keep; return rc; }
    {                                                               // lmh_rollout_zoh_box's dynamic LDS: asked for here, never inside the (capturable) call
        int32_t answer = -1;
        const LmhZohBox prep = {nullptr, 0, nullptr, 0.0, 0.0, 1, &answer};
        lmh_launch_rollout_zoh(&h->P, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, &prep, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr);
        h->zoh_box_prepared = answer;
    }
    (void)hipGetLastError();                                        // an answer other than hipSuccess is that call's to report, not a sticky error of this one
    *out = h;
    return LMH_OK;
}

extern "C" int lmh_destroy(lmh_handle *h)
{
    if (!h) return LMH_OK;
    (void)hipSetDevice(h->device);
    for (auto &sl : h->slot) if (sl.used) (void)hipEventSynchronize(sl.done);   // no launch still reads a slot
    delete h;                                                       // the buffers and events go with their owners
    return LMH_OK;
}

extern "C" int lmh_num_instances(const lmh_handle *h) { return h ? h->B : 0; }
extern "C" int lmh_horizon(const lmh_handle *h) { return h ? h->N : 0; }

extern "C" int lmh_set_model(lmh_handle *h, const double *raw, int n_models)
{
    if (!h) return fail(LMH_ERR_BAD_ARG, "null handle");
    if (!raw) { raw = &kLmhNaoLinks[0][0]; n_models = 1; }
    if (n_models != 1 && n_models != h->B) return fail(LMH_ERR_BAD_ARG, "n_models must be 1 or n_instances");
    // frames 7, 14 (soles) and 27 (extra head frame) are massless virtual frames in createNaoParameters (src/robotParameters.cpp); the
    // kernels' tree recursions rely on that (they carry no body force and no inertia there)
    for (int m = 0; m < n_models; m++)
        for (int f : {7, 14, 27})
            for (int e = 0; e < LMH_LINK_STRIDE; e++)
                if (raw[((size_t)m * 28 + f) * LMH_LINK_STRIDE + e] != 0.0) return fail(LMH_ERR_BAD_ARG, "lmh_set_model: frames 7, 14, 27 are massless virtual frames: their records must be zero");
    HIPCHK(hipSetDevice(h->device));
    DevBuf<double> d_raw, d_model;
    HIPCHK(d_raw.upload(raw, 28 * LMH_LINK_STRIDE * (size_t)n_models));
    HIPCHK(d_model.alloc(LMH_MODEL_STRIDE * (size_t)n_models));
    lmh_launch_model(d_raw.get(), d_model.get(), n_models, lcoef_of(h), nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    return commit(h, [&] { std::swap(h->d_raw, d_raw); std::swap(h->d_model, d_model); std::swap(h->n_models, n_models); });
}

extern "C" int lmh_get_mass(lmh_handle *h, double *mass)
{
    if (!h || !mass) return fail(LMH_ERR_BAD_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    for (int i = 0; i < h->n_models; i++)
        HIPCHK(hipMemcpy(mass + i, h->d_model.get() + (size_t)i * LMH_MODEL_STRIDE + 392, sizeof(double), hipMemcpyDeviceToHost));
    return LMH_OK;
}

// ---------------------------------------------------------------------------- the reference plan
// Every setter validates its arguments on the host, builds a fresh RefPlan aside (allocation, upload or generator launch, sync) and
// commits it here: the one place where a handle changes plan.  Whatever fails before that leaves the handle on its previous plan.
// The plan that loses dies with p: the new one after a failure, else the previous one, after P (and every robot's block) has left it.
static int commit_plan(lmh_handle *h, RefPlan p) { return commit(h, [&] { std::swap(h->plan, p); }); }

static std::string robot_msg(int i, const char *msg) { return "robot " + std::to_string(i) + ": " + msg; }

// seg_of_sample < n_seg in every slice of n_samples entries: the first slice at fault, or -1
static int sos_out_of_range(const uint16_t *sos, int n_seg, int n_samples, int n_plans)
{
    for (int i = 0; i < n_plans; i++)
        for (int k = 0; k < n_samples; k++)
            if (sos[(size_t)i * n_samples + k] >= n_seg) return i;
    return -1;
}

// lmh_set_refs / lmh_set_refs_stance (one slice) and lmh_set_plans (n_instances slices); the arguments have been checked
static int upload_plan(lmh_handle *h, const double *zx, const double *zy, const uint8_t *phase, int n_samples,
                       const double *segs, int n_seg, const uint16_t *sos, int n_plans)
{
    HIPCHK(hipSetDevice(h->device));
    RefPlan p;
    const size_t ns = (size_t)n_samples * (size_t)n_plans;
    HIPCHK(p.zx.upload(zx, ns));
    HIPCHK(p.zy.upload(zy, ns));
    if (phase) HIPCHK(p.phase.upload(phase, ns));
    else if (n_plans > 1) {                                          // per-robot plans always carry a phase slice per robot
        HIPCHK(p.phase.alloc(ns));
        HIPCHK(hipMemset(p.phase.get(), 0, ns));
    }
    if (n_seg > 0) {
        HIPCHK(p.segs.upload(segs, LMH_SEG_STRIDE * (size_t)n_seg * (size_t)n_plans));
        HIPCHK(p.sos.upload(sos, ns));
    }
    p.n_samples = n_samples; p.n_seg = n_seg; p.n_plans = n_plans;
    return commit_plan(h, std::move(p));
}

extern "C" int lmh_set_refs(lmh_handle *h, const double *zx, const double *zy, const uint8_t *phase, int n)
{
    if (!h || !zx || !zy || n < 1) return fail(LMH_ERR_BAD_ARG, "bad argument");
    return upload_plan(h, zx, zy, phase, n, nullptr, 0, nullptr, 1);  // no segments: they are tied to the sample grid
}

// (int)((simulation_time + 0.5) / mpc_dt): zmpGeneration.cpp:41 with timeStep_ = the MPC sample time
static int sample_count(const lmh_handle *h, double simulation_time) { return (int)((simulation_time + 0.5) / h->mpc_dt); }

extern "C" int lmh_set_refs_stance(lmh_handle *h, double simulation_time, int support_foot)
{
    if (!h) return fail(LMH_ERR_BAD_ARG, "null handle");
    const int samples = sample_count(h, simulation_time);
    if (samples < 1) return fail(LMH_ERR_BAD_ARG, "no samples");
    std::vector<double> zx((size_t)samples, 0.0), zy((size_t)samples, (support_foot == 0) ? -0.05 : (support_foot == 1) ? 0.05 : 0.0);
    return lmh_set_refs(h, zx.data(), zy.data(), nullptr, samples);
}

extern "C" int lmh_set_foot_coeffs(lmh_handle *h, const double *r, const int32_t *rn, const double *l, const int32_t *ln)
{
    if (!h || !r || !rn || !l || !ln) return fail(LMH_ERR_BAD_ARG, "bad argument");
    for (int a = 0; a < 3; a++)
        if (rn[a] < 1 || rn[a] > 8 || ln[a] < 1 || ln[a] > 8) return fail(LMH_ERR_BAD_ARG, "coefficient count must be 1..8");
    double rF[3][8], lF[3][8];
    int32_t rFn[3], lFn[3];
    for (int a = 0; a < 3; a++) {
        rFn[a] = rn[a]; lFn[a] = ln[a];
        // entries beyond the count are stored as zeros: the kernels evaluate all eight terms (a zero coefficient adds an exact zero)
        for (int k = 0; k < 8; k++) { rF[a][k] = (k < rn[a]) ? r[8 * a + k] : 0.0; lF[a][k] = (k < ln[a]) ? l[8 * a + k] : 0.0; }
    }
    LmhDevParams &P = h->P;                                          // the polynomials live in the block alone, and in every robot's copy of it
    auto swap = [&] { std::swap(P.rF, rF); std::swap(P.lF, lF); std::swap(P.rFn, rFn); std::swap(P.lFn, lFn); };
    if (!h->inst.on()) { swap(); return LMH_OK; }                    // no table to rewrite: no HIP call at all
    HIPCHK(hipSetDevice(h->device));
    return commit(h, swap);
}

extern "C" int lmh_set_segments(lmh_handle *h, const double *segs, int n_seg, const uint16_t *sos, int n_samples)
{
    if (!h || n_seg < 0) return fail(LMH_ERR_BAD_ARG, "bad argument");
    if (n_seg > 0) {
        if (!segs || !sos) return fail(LMH_ERR_BAD_ARG, "null segment table");
        if (n_samples != h->plan.n_samples) return fail(LMH_ERR_BAD_ARG, "seg_of_sample must cover the ZMP reference samples (call lmh_set_refs first)");
        if (sos_out_of_range(sos, n_seg, n_samples, 1) >= 0) return fail(LMH_ERR_BAD_ARG, "seg_of_sample entry out of range");
    }
    HIPCHK(hipSetDevice(h->device));
    RefPlan p;                                                       // one shared plan: the new table ...
    if (n_seg > 0) {
        HIPCHK(p.segs.upload(segs, LMH_SEG_STRIDE * (size_t)n_seg));
        HIPCHK(p.sos.upload(sos, (size_t)n_samples));
    }
    RefPlan &cur = h->plan;                                          // ... on the current samples (of a per-robot set, robot 0's slice); nothing below fails
    p.zx = std::move(cur.zx); p.zy = std::move(cur.zy); p.phase = std::move(cur.phase);
    p.n_samples = cur.n_samples; p.n_seg = n_seg;
    return commit_plan(h, std::move(p));
}

// ---------------------------------------------------------------------------- timed velocity pushes (lmh_rollout)
// the rules of one schedule (n_push records): nullptr = fine.  trajectories.push_schedule states the same rules with the same words.
static const char *push_schedule_error(const double *rec, int n_push)
{
    double prev = -1.0;
    bool unused = false;
    for (int j = 0; j < n_push; j++, rec += LMH_PUSH_STRIDE) {
        const double tk = rec[0];
        if (tk == -1.0) { unused = true; continue; }                // padding: its dv is ignored
        if (!(tk >= 0.0) || !(tk < 2147483648.0) || tk != std::floor(tk)) return "push ticks must be whole numbers in [0, 2^31), or -1 for an unused record";
        if (unused) return "a used push record follows an unused one";
        if (!(tk > prev)) return "push ticks must be strictly increasing";
        for (int e = 1; e <= LMH_NQ; e++) if (!std::isfinite(rec[e])) return "push dv must be finite";
        prev = tk;
    }
    return nullptr;
}

extern "C" int lmh_set_pushes(lmh_handle *h, const double *records, int n_push, int n_sets)
{
    if (!h) return fail(LMH_ERR_BAD_ARG, "null handle");
    if (n_push < 0) return fail(LMH_ERR_BAD_ARG, "n_push must be >= 0");
    if (!records) n_push = 0;
    if (n_push > LMH_MAX_PUSHES) return fail(LMH_ERR_BAD_ARG, "n_push must be at most LMH_MAX_PUSHES (16)");
    if (n_push == 0) n_sets = 1;
    if (n_sets != 1 && n_sets != h->B) return fail(LMH_ERR_BAD_ARG, "n_sets must be 1 or n_instances");
    for (int i = 0; i < n_sets && n_push > 0; i++)
        if (const char *msg = push_schedule_error(records + (size_t)LMH_PUSH_STRIDE * n_push * i, n_push)) return fail(LMH_ERR_BAD_ARG, robot_msg(i, msg));
    HIPCHK(hipSetDevice(h->device));
    DevBuf<double> d;
    if (n_push > 0) HIPCHK(d.upload(records, (size_t)LMH_PUSH_STRIDE * n_push * n_sets));
    return commit(h, [&] { std::swap(h->d_pushes, d); std::swap(h->n_push, n_push); std::swap(h->n_push_sets, n_sets); });
}

extern "C" int lmh_num_pushes(const lmh_handle *h) { return h ? h->n_push : 0; }
extern "C" int lmh_pushes_per_instance(const lmh_handle *h) { return (h && h->n_push > 0 && h->n_push_sets > 1) ? 1 : 0; }

extern "C" int lmh_get_pushes(lmh_handle *h, int inst, double *records)
{
    if (!h) return fail(LMH_ERR_BAD_ARG, "null handle");
    if (inst < 0 || inst >= h->B) return fail(LMH_ERR_BAD_ARG, "instance out of range");
    if (h->n_push == 0) return LMH_OK;
    if (!records) return fail(LMH_ERR_BAD_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    const size_t n = (size_t)LMH_PUSH_STRIDE * h->n_push;
    HIPCHK(hipMemcpy(records, h->d_pushes.get() + ((h->n_push_sets > 1) ? n * (size_t)inst : 0), sizeof(double) * n, hipMemcpyDeviceToHost));
    return LMH_OK;
}

// ---------------------------------------------------------------------------- actuator records (lmh_rollout_zoh_io)
// the rules of one record: nullptr = fine.  trajectories.actuator_records states the same rules with the same words.
static const char *actuator_record_error(const double *rec)
{
    for (int j = 0; j < 24; j++) if (!(rec[LMH_ACT_OFF_TAU_MAX + j] >= 0.0)) return "torque limits must be >= 0 (+inf: none)";
    for (int j = 0; j < 24; j++) if (!(rec[LMH_ACT_OFF_ALPHA + j] > 0.0) || !(rec[LMH_ACT_OFF_ALPHA + j] <= 1.0)) return "alpha must be in (0, 1]";
    const double d = rec[LMH_ACT_OFF_DELAY];
    if (!(d >= 0.0) || !(d <= (double)LMH_ACT_MAX_DELAY) || d != std::floor(d)) return "delay must be a whole number in [0, LMH_ACT_MAX_DELAY (7)]";
    return nullptr;
}

// The shared work of lmh_set_actuators, lmh_set_servo and lmh_set_ground behind their handle checks: NULL records clear the table, n is 0, 1 or
// n_instances (who: the call's prefix of that refusal), every record passes `rule` (the first offending robot is named), then both copies are built
// aside and put in place together.  Whatever fails leaves the previous table: the parameter block does not hold it, so nothing after the upload can.
int RecordTable::set(const lmh_handle *hd, const char *who, const double *records, int n, int width, const char *(*rule)(const double *))
{
    if (n < 0) return fail(LMH_ERR_BAD_ARG, "n_sets must be >= 0");
    if (!records) n = 0;
    if (n != 0 && n != 1 && n != hd->B) return fail(LMH_ERR_BAD_ARG, std::string(who) + "n_sets must be 1 or n_instances");
    for (int i = 0; i < n; i++)
        if (const char *msg = rule(records + (size_t)width * i)) return fail(LMH_ERR_BAD_ARG, robot_msg(i, msg));
    HIPCHK(hipSetDevice(hd->device));
    DevBuf<double> dev;
    std::vector<double> host;
    if (n > 0) {
        host.assign(records, records + (size_t)width * n);
        HIPCHK(dev.upload(records, host.size()));
    }
    d = std::move(dev); h.swap(host); n_sets = n;
    return LMH_OK;
}

// robot inst's record: the defaults word by word from an empty table, the one record of a shared table, else the robot's own
int RecordTable::get(const lmh_handle *hd, int inst, double *record, int width, double (*default_word)(int)) const
{
    if (inst < 0 || inst >= hd->B) return fail(LMH_ERR_BAD_ARG, "instance out of range");
    if (!record) return fail(LMH_ERR_BAD_ARG, "bad argument");
    if (n_sets == 0) for (int j = 0; j < width; j++) record[j] = default_word(j);
    else std::memcpy(record, h.data() + (size_t)width * ((n_sets > 1) ? inst : 0), sizeof(double) * width);
    return LMH_OK;
}

extern "C" int lmh_set_actuators(lmh_handle *h, const double *records, int n_sets)
{
    if (!h) return fail(LMH_ERR_BAD_ARG, "null handle");
    return h->act.set(h, "", records, n_sets, LMH_ACT_STRIDE, actuator_record_error);
}

extern "C" int lmh_actuators_per_instance(const lmh_handle *h) { return (h && h->act.n_sets > 1) ? 1 : 0; }

extern "C" int lmh_get_actuators(lmh_handle *h, int inst, double *record)
{
    if (!h) return fail(LMH_ERR_BAD_ARG, "null handle");
    return h->act.get(h, inst, record, LMH_ACT_STRIDE, [](int j) { return (j < 24) ? (double)INFINITY : (j < 48) ? 1.0 : 0.0; });   // inf | 1 | 0
}

// ---------------------------------------------------------------------------- servo records (lmh_plant_step_servo, lmh_rollout_zoh_servo)
// the rules of one record: nullptr = fine.  trajectories.servo_records states the same rule with the same words.
static const char *servo_record_error(const double *rec)
{
    for (int j = 0; j < LMH_SERVO_STRIDE; j++) if (!std::isfinite(rec[j]) || !(rec[j] >= 0.0)) return "servo gains must be finite and >= 0";
    return nullptr;
}

extern "C" int lmh_set_servo(lmh_handle *h, const double *records, int n_sets)
{
    if (!h) return fail(LMH_ERR_BAD_ARG, "null handle");
    return h->servo.set(h, "lmh_set_servo: ", records, n_sets, LMH_SERVO_STRIDE, servo_record_error);
}

extern "C" int lmh_servo_per_instance(const lmh_handle *h) { return (h && h->servo.n_sets > 1) ? 1 : 0; }

extern "C" int lmh_get_servo(lmh_handle *h, int inst, double *record)
{
    if (!h) return fail(LMH_ERR_BAD_ARG, "null handle");
    return h->servo.get(h, inst, record, LMH_SERVO_STRIDE, [](int) { return 0.0; });
}

// ---------------------------------------------------------------------------- ground records (the plant calls and the zero-order-hold family)
// the rules of one record: nullptr = fine
static const char *ground_record_error(const double *rec)
{
    for (int j = 0; j < LMH_GROUND_STRIDE; j++) if (!std::isfinite(rec[j])) return "every word of a ground record must be finite";
    for (int off : {LMH_GROUND_OFF_N_R, LMH_GROUND_OFF_N_L}) {
        const double *n = rec + off;
        if (!(std::fabs((n[0] * n[0] + n[1] * n[1] + n[2] * n[2]) - 1.0) <= 1e-12)) return "a ground normal must have unit length (| |n|^2 - 1 | <= 1e-12; nothing is normalised here)";
        if (!(n[2] > 0.0)) return "a ground normal must point up (n_z > 0)";
    }
    return nullptr;
}

extern "C" int lmh_set_ground(lmh_handle *h, const double *records, int n_sets)
{
    if (!h) return fail(LMH_ERR_BAD_ARG, "null handle");
    if (h->cfg.plant) return fail(LMH_ERR_BAD_ARG, "lmh_set_ground: not offered on a plant = 1 handle (the RK4 reference loop of lmh_rollout keeps the plane z = 0)");
    return h->ground.set(h, "lmh_set_ground: ", records, n_sets, LMH_GROUND_STRIDE, ground_record_error);
}

extern "C" int lmh_ground_per_instance(const lmh_handle *h) { return (h && h->ground.n_sets > 1) ? 1 : 0; }

extern "C" int lmh_get_ground(lmh_handle *h, int inst, double *record)
{
    if (!h) return fail(LMH_ERR_BAD_ARG, "null handle");
    return h->ground.get(h, inst, record, LMH_GROUND_STRIDE, [](int j) { return (j == LMH_GROUND_OFF_N_R + 2 || j == LMH_GROUND_OFF_N_L + 2) ? 1.0 : 0.0; });   // 0 0 1 0 | 0 0 1 0
}

extern "C" int lmh_set_xscale(lmh_handle *h, const double *xscale, int n)
{
    if (!h) return fail(LMH_ERR_BAD_ARG, "null handle");
    if (xscale && n != h->B) return fail(LMH_ERR_BAD_ARG, "n must be n_instances");
    HIPCHK(hipSetDevice(h->device));
    DevBuf<double> d;
    if (xscale) HIPCHK(d.upload(xscale, (size_t)n));
    return commit(h, [&] { std::swap(h->d_xscale, d); });
}

extern "C" int lmh_set_zcom(lmh_handle *h, const double *z, int n)
{
    if (!h || !z || (n != 1 && n != h->B)) return fail(LMH_ERR_BAD_ARG, "n must be 1 or n_instances");
    HIPCHK(hipSetDevice(h->device));
    return upload_gain(h, z, n);
}

extern "C" int lmh_get_mpc_gain(lmh_handle *h, double *K)
{
    if (!h || !K) return fail(LMH_ERR_BAD_ARG, "bad argument");
    std::memcpy(K, h->h_gain.data(), sizeof(double) * (size_t)(h->N + 1));
    return LMH_OK;
}

// ---------------------------------------------------------------------------- per-robot controller parameters
extern "C" int lmh_set_params(lmh_handle *h, const double *records, int n)
{
    if (!h) return fail(LMH_ERR_BAD_ARG, "null handle");
    if (n < 0) return fail(LMH_ERR_BAD_ARG, "n must be >= 0");
    HIPCHK(hipSetDevice(h->device));
    if (!records || n == 0) {                                        // back on the config's one set
        h->P.inst_blocks = nullptr;                                  // first: nothing may launch on a table that is about to go
        h->inst = lmh_handle::InstParams();
        return fill_params(h);
    }
    if (n != h->B) return fail(LMH_ERR_BAD_ARG, "n must be n_instances");
    for (int i = 0; i < n; i++)
        if (const char *msg = param_record_error(records + (size_t)LMH_PARAM_STRIDE * i, h->cfg.plant != 0)) return fail(LMH_ERR_BAD_ARG, robot_msg(i, msg));
    // built aside: the records (pad zeroed), one friction table per robot by the routine lmh_create uses, the block table
    lmh_handle::InstParams p;
    p.h_rec.assign(records, records + (size_t)LMH_PARAM_STRIDE * n);
    std::vector<double> g((size_t)LMH_GCOL_STRIDE * n);
    for (int i = 0; i < n; i++) {
        p.h_rec[(size_t)LMH_PARAM_STRIDE * i + LMH_PARAM_STRIDE - 1] = 0.0;
        build_gcol(records[(size_t)LMH_PARAM_STRIDE * i + LMH_PARAM_OFF_MU], g.data() + (size_t)LMH_GCOL_STRIDE * i);
    }
    HIPCHK(p.d_rec.upload(p.h_rec.data(), p.h_rec.size()));
    HIPCHK(p.d_gcol.upload(g.data(), g.size()));
    const int rc = expand_blocks(h, h->P, p.d_rec.get(), p.d_gcol.get(), p.d_blocks);
    if (rc != LMH_OK) return rc;
    h->P.inst_blocks = p.d_blocks.get();                             // nothing above changed the handle; nothing below fails
    h->inst = std::move(p);
    return LMH_OK;
}

extern "C" int lmh_params_per_instance(const lmh_handle *h) { return (h && h->B > 1 && h->inst.on()) ? 1 : 0; }

extern "C" int lmh_get_params(lmh_handle *h, int inst, double *record)
{
    if (!h || !record) return fail(LMH_ERR_BAD_ARG, "bad argument");
    if (inst < 0 || inst >= h->B) return fail(LMH_ERR_BAD_ARG, "instance out of range");
    if (h->inst.on()) std::memcpy(record, h->inst.h_rec.data() + (size_t)LMH_PARAM_STRIDE * inst, sizeof(double) * LMH_PARAM_STRIDE);
    else config_record(h->cfg, record);
    return LMH_OK;
}

static int ready(lmh_handle *h)
{
    if (!h) return fail(LMH_ERR_BAD_ARG, "null handle");
    if (!h->d_model.get() || !h->d_mpc.get() || !h->plan.zx.get() || h->plan.n_samples < 1) return fail(LMH_ERR_NOT_READY, "model / references not set");
    return LMH_OK;
}

// The one launch path of the asynchronous entry points: the handle is ready, the entry point's own argument check did not fire
// (refusal: its message, nullptr = fine), then the device, the launch and the launch's error.  Nothing is enqueued by a refused call.
template <class Launch> static int launch(lmh_handle *h, const char *refusal, Launch go)
{
    const int rc = ready(h); if (rc) return rc;
    if (refusal) return fail(LMH_ERR_BAD_ARG, refusal);
    HIPCHK(hipSetDevice(h->device));
    go();
    HIPCHK(hipGetLastError());
    return LMH_OK;
}

// with_ref (lmh_eval_ref): d_ref is required too, refused behind lmh_eval's own pointers with a message of its own
static int eval_body(lmh_handle *h, double *d_state, double *d_out, int32_t *d_status, double *d_debug, bool debug, const double *d_ref, bool with_ref, void *stream)
{
    return launch(h, (!d_state || !d_out || !d_status || (debug && !d_debug)) ? "null device pointer" : (with_ref && !d_ref) ? "lmh_eval_ref: null d_ref" : nullptr,
                  [&] { lmh_launch_eval(&h->P, d_state, d_out, d_status, d_debug, d_ref, (hipStream_t)stream); });
}

extern "C" int lmh_eval(lmh_handle *h, double *d_state, double *d_out, int32_t *d_status, void *stream)
{
    return eval_body(h, d_state, d_out, d_status, nullptr, false, nullptr, false, stream);
}

extern "C" int lmh_eval_debug(lmh_handle *h, double *d_state, double *d_out, int32_t *d_status, double *d_debug, void *stream)
{
    return eval_body(h, d_state, d_out, d_status, d_debug, true, nullptr, false, stream);
}

extern "C" int lmh_eval_ref(lmh_handle *h, double *d_state, const double *d_ref, double *d_out, int32_t *d_status, void *stream)
{
    return eval_body(h, d_state, d_out, d_status, nullptr, false, d_ref, true, stream);
}

// The error word of a COMPLETED launch on this slot (d_ticket[3], lmh_rollout_kernel): read once, cleared, reported.  The kernel has already
// flagged the robots concerned and put the slot's ring / progress words back to zero.
static int slot_take_error(lmh_handle::Slot &sl)
{
    if (sl.checked) return LMH_OK;
    int err = 0;
    HIPCHK(hipMemcpy(&err, sl.d_ticket.get() + 3, sizeof(int), hipMemcpyDeviceToHost));
    sl.checked = true;
    if (err == 0) return LMH_OK;
    HIPCHK(hipMemset(sl.d_ticket.get() + 3, 0, sizeof(int)));
    return fail(LMH_ERR_UNFINISHED, "lmh_rollout: a wait of the kernel's work queue ran out (error word " + std::to_string(err) +
                "); the robots that did not get all their ticks carry LMH_FLAG_UNFINISHED in their status records");
}

extern "C" int lmh_trace_samples(int n_ticks, int trace_every)
{
    return (trace_every <= 0 || n_ticks <= 0) ? 0 : n_ticks / trace_every;
}

// The one launch path of lmh_rollout, lmh_rollout_trace and lmh_rollout_metrics, behind their own argument checks: a launch slot, the
// parameter block, the kernel (a trace, a metrics record or neither), the slot's event
static int rollout_launch(lmh_handle *h, double *d_state, double *d_out, int32_t *d_status, double *d_log, int n_ticks, double *d_trace, int trace_every,
                          double *d_metrics, void *stream)
{
    int rc = LMH_OK;
    HIPCHK(hipSetDevice(h->device));
    lmh_handle::Slot &sl = h->slot[h->next_slot % lmh_handle::kSlots];
    if (!sl.ready()) HIPCHK(sl.init(h->B, (hipStream_t)stream));
    if (sl.used) {
        HIPCHK(hipEventSynchronize(sl.done));                       // the launch that last used this slot (kSlots launches ago) has left it
        rc = slot_take_error(sl);                                // ... and if it was incomplete, this call reports it instead of launching
        if (rc) return rc;
    }
    h->next_slot++;
    if (!sl.valid || std::memcmp(&sl.P_dev, &h->P, sizeof(LmhDevParams)) != 0) {   // set-up calls changed the block since this slot was filled
        std::memcpy(&sl.P_dev, &h->P, sizeof(LmhDevParams));
        HIPCHK(hipMemcpyAsync(sl.d_P.get(), &sl.P_dev, sizeof(LmhDevParams), hipMemcpyHostToDevice, (hipStream_t)stream));   // stream-ordered in front of the launch; the slot is idle
        sl.valid = true;
    }
    lmh_launch_rollout(&h->P, sl.d_P.get(), sl.d_ticket.get(), d_state, d_out, d_status, d_log, n_ticks, d_trace, trace_every, d_metrics, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(sl.done, (hipStream_t)stream));
    sl.used = true;
    sl.checked = false;
    return LMH_OK;
}

extern "C" int lmh_rollout_trace(lmh_handle *h, double *d_state, double *d_out, int32_t *d_status, double *d_log, int n_ticks,
                                 double *d_trace, int trace_every, void *stream)
{
    const int rc = ready(h); if (rc) return rc;
    if (!d_state || !d_out || !d_status || n_ticks < 0) return fail(LMH_ERR_BAD_ARG, "bad argument");
    // decided before a launch slot is taken: the buffer and its period come together or not at all
    if (trace_every < 0 || (d_trace != nullptr) != (trace_every > 0))
        return fail(LMH_ERR_BAD_ARG, "lmh_rollout_trace: d_trace and trace_every > 0 go together (NULL and 0: no trace)");
    if (n_ticks == 0) return LMH_OK;
    return rollout_launch(h, d_state, d_out, d_status, d_log, n_ticks, d_trace, trace_every, nullptr, stream);
}

extern "C" int lmh_rollout_metrics(lmh_handle *h, double *d_state, double *d_out, int32_t *d_status, double *d_log, int n_ticks, double *d_metrics, void *stream)
{
    const int rc = ready(h); if (rc) return rc;
    if (!d_state || !d_out || !d_status || n_ticks < 0) return fail(LMH_ERR_BAD_ARG, "bad argument");
    if (!d_metrics) return fail(LMH_ERR_BAD_ARG, "lmh_rollout_metrics: d_metrics is NULL (lmh_rollout is the call without a record)");      // before a launch slot is taken
    if (n_ticks == 0) return LMH_OK;
    return rollout_launch(h, d_state, d_out, d_status, d_log, n_ticks, nullptr, 0, d_metrics, stream);
}

extern "C" int lmh_metrics_reset(lmh_handle *h, double *d_metrics, double z_min, double tilt_max, void *stream)
{
    if (!h) return fail(LMH_ERR_BAD_ARG, "null handle");
    if (!d_metrics) return fail(LMH_ERR_BAD_ARG, "lmh_metrics_reset: d_metrics is NULL");
    if (std::isnan(z_min) || std::isnan(tilt_max)) return fail(LMH_ERR_BAD_ARG, "lmh_metrics_reset: a threshold is NaN (-INFINITY / +INFINITY: never down)");
    HIPCHK(hipSetDevice(h->device));
    lmh_launch_metrics_reset(d_metrics, h->B, z_min, tilt_max, (hipStream_t)stream);
    HIPCHK(hipGetLastError());
    return LMH_OK;
}

extern "C" int lmh_rollout(lmh_handle *h, double *d_state, double *d_out, int32_t *d_status, double *d_log, int n_ticks, void *stream)
{
    return lmh_rollout_trace(h, d_state, d_out, d_status, d_log, n_ticks, nullptr, 0, stream);
}

extern "C" int lmh_ik(lmh_handle *h, double *d_q, const double *com_target, const double *rf6, const double *lf6, int32_t *d_iters, void *stream)
{
    return launch(h, (!d_q || !com_target || !rf6 || !lf6) ? "bad argument" : nullptr, [&] {
        LmhIkTarget tgt;                                             // travels by value in the kernel arguments: no shared staging buffer, no sync
        for (int k = 0; k < 6; k++) { tgt.v[k] = rf6[k]; tgt.v[6 + k] = lf6[k]; }
        for (int k = 0; k < 3; k++) tgt.v[12 + k] = com_target[k];
        tgt.v[15] = 0.0;
        lmh_launch_ik(&h->P, d_q, &tgt, d_iters, (hipStream_t)stream);
    });
}

extern "C" int lmh_ik_batch(lmh_handle *h, const double *d_q_start, const double *d_targets, int n_targets, double *d_q, int32_t *d_iters, double *d_crit, void *stream)
{
    const char *refusal = nullptr;
    if (!d_q_start || !d_targets || !d_q) refusal = "lmh_ik_batch: null device pointer";
    else if (n_targets < 0) refusal = "lmh_ik_batch: n_targets must be >= 0";
    else if (n_targets > 1 && d_q == d_q_start) refusal = "lmh_ik_batch: d_q may alias d_q_start only when n_targets == 1";
    // the records are read on the device and no launch slot is taken: nothing of the handle is written, nothing is staged on the host
    return launch(h, refusal, [&] { if (n_targets > 0) lmh_launch_ik_batch(&h->P, d_q_start, d_targets, n_targets, d_q, d_iters, d_crit, (hipStream_t)stream); });
}

// ---------------------------------------------------------------------------- LIPM preview MPC (lmh_mpc.hip)
// the records are read on the device and no launch slot is taken: nothing of the handle is written, nothing is staged on the host
extern "C" int lmh_mpc_step(lmh_handle *h, const double *d_lip, double *d_mpc, void *stream)
{
    return launch(h, (!d_lip || !d_mpc) ? "lmh_mpc_step: null device pointer" : nullptr, [&] { lmh_launch_mpc_step(&h->P, h->cfg.alpha, h->cfg.beta, d_lip, nullptr, 0, d_mpc, (hipStream_t)stream); });
}

extern "C" int lmh_mpc_rollout(lmh_handle *h, double *d_lip, int n_ticks, double *d_traj, void *stream)
{
    const char *refusal = nullptr;
    if (!d_lip) refusal = "lmh_mpc_rollout: null device pointer";
    else if (n_ticks < 0) refusal = "lmh_mpc_rollout: n_ticks must be >= 0";
    return launch(h, refusal, [&] { if (n_ticks > 0) lmh_launch_mpc_rollout(&h->P, h->cfg.alpha, h->cfg.beta, d_lip, nullptr, 0, n_ticks, d_traj, (hipStream_t)stream); });
}

extern "C" int lmh_mpc_preview(lmh_handle *h, const double *d_lip, double *d_preview, void *stream)
{
    return launch(h, (!d_lip || !d_preview) ? "lmh_mpc_preview: null device pointer" : nullptr, [&] { lmh_launch_mpc_preview(&h->P, h->cfg.alpha, h->cfg.beta, d_lip, nullptr, 0, d_preview, (hipStream_t)stream); });
}

// the box-constrained calls: the refusal of the bounds' shape (nullptr = fine) and the stride from one robot's bounds to the next
static const char *box_refusal(const lmh_handle *h, const void *d_box, int n_samples, int n_sets, const char *null_text, const char *samples_text, const char *sets_text)
{
    if (!d_box) return null_text;
    if (h && n_samples != h->plan.n_samples) return samples_text;
    if (h && n_sets != 1 && n_sets != h->B) return sets_text;
    return nullptr;
}
static size_t box_stride(const lmh_handle *h, int n_sets) { return (n_sets > 1) ? (size_t)4 * (size_t)h->plan.n_samples : 0; }

extern "C" int lmh_mpc_box_preview(lmh_handle *h, const double *d_lip, const double *d_box, int n_samples, int n_sets, double *d_record, void *stream)
{
    const char *refusal = (!d_lip || !d_record) ? "lmh_mpc_box_preview: null device pointer"
                        : box_refusal(h, d_box, n_samples, n_sets, "lmh_mpc_box_preview: null device pointer",
                                      "lmh_mpc_box_preview: n_samples must be lmh_num_ref_samples", "lmh_mpc_box_preview: n_sets must be 1 or n_instances");
    return launch(h, refusal, [&] { lmh_launch_mpc_preview(&h->P, h->cfg.alpha, h->cfg.beta, d_lip, d_box, box_stride(h, n_sets), d_record, (hipStream_t)stream); });
}

extern "C" int lmh_mpc_box_step(lmh_handle *h, const double *d_lip, const double *d_box, int n_samples, int n_sets, double *d_mpc, void *stream)
{
    const char *refusal = (!d_lip || !d_mpc) ? "lmh_mpc_box_step: null device pointer"
                        : box_refusal(h, d_box, n_samples, n_sets, "lmh_mpc_box_step: null device pointer",
                                      "lmh_mpc_box_step: n_samples must be lmh_num_ref_samples", "lmh_mpc_box_step: n_sets must be 1 or n_instances");
    return launch(h, refusal, [&] { lmh_launch_mpc_step(&h->P, h->cfg.alpha, h->cfg.beta, d_lip, d_box, box_stride(h, n_sets), d_mpc, (hipStream_t)stream); });
}

extern "C" int lmh_mpc_box_rollout(lmh_handle *h, double *d_lip, const double *d_box, int n_samples, int n_sets, int n_ticks, double *d_traj, void *stream)
{
    const char *refusal = !d_lip ? "lmh_mpc_box_rollout: null device pointer"
                        : box_refusal(h, d_box, n_samples, n_sets, "lmh_mpc_box_rollout: null device pointer",
                                      "lmh_mpc_box_rollout: n_samples must be lmh_num_ref_samples", "lmh_mpc_box_rollout: n_sets must be 1 or n_instances");
    if (!refusal && n_ticks < 0) refusal = "lmh_mpc_box_rollout: n_ticks must be >= 0";
    return launch(h, refusal, [&] { if (n_ticks > 0) lmh_launch_mpc_rollout(&h->P, h->cfg.alpha, h->cfg.beta, d_lip, d_box, box_stride(h, n_sets), n_ticks, d_traj, (hipStream_t)stream); });
}

extern "C" int lmh_eval_host(lmh_handle *h, const double *q, const double *dq, double t, double *tau, double *f, double *qdd, int32_t *status)
{
    int rc = ready(h); if (rc) return rc;
    if (!q || !dq) return fail(LMH_ERR_BAD_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    // keep v_prev / active set from the previous call (Robot::v_ semantics): read-modify-write
    for (int i = 0; i < h->B; i++) {
        double *s = h->h_state.data() + (size_t)LMH_STATE_STRIDE * i;
        std::memcpy(s, q + 30 * (size_t)i, 30 * sizeof(double));
        std::memcpy(s + 30, dq + 30 * (size_t)i, 30 * sizeof(double));
        s[90] = t;
    }
    HIPCHK(hipMemcpy(h->d_state.get(), h->h_state.data(), sizeof(double) * h->h_state.size(), hipMemcpyHostToDevice));
    lmh_launch_eval(&h->P, h->d_state.get(), h->d_out.get(), h->d_status.get(), nullptr, nullptr, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(h->h_state.data(), h->d_state.get(), sizeof(double) * h->h_state.size(), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(h->h_out.data(), h->d_out.get(), sizeof(double) * h->h_out.size(), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(h->h_status.data(), h->d_status.get(), sizeof(int32_t) * h->h_status.size(), hipMemcpyDeviceToHost));
    for (int i = 0; i < h->B; i++) {
        const double *o = h->h_out.data() + (size_t)LMH_OUT_STRIDE * i;
        if (tau) std::memcpy(tau + 24 * (size_t)i, o, 24 * sizeof(double));
        if (f) std::memcpy(f + 12 * (size_t)i, o + 24, 12 * sizeof(double));
        if (qdd) std::memcpy(qdd + 30 * (size_t)i, o + 36, 30 * sizeof(double));
        if (status) std::memcpy(status + 4 * (size_t)i, h->h_status.data() + 4 * (size_t)i, 4 * sizeof(int32_t));
    }
    return LMH_OK;
}

extern "C" int lmh_robot_com(lmh_handle *h, const double *d_q, double *d_com, void *stream)
{
    return launch(h, (!d_q || !d_com) ? "null device pointer" : nullptr, [&] { lmh_launch_com(&h->P, d_q, d_com, (hipStream_t)stream); });
}

extern "C" int lmh_robot_com_host(lmh_handle *h, const double *q, double *com)
{
    int rc = ready(h); if (rc) return rc;
    if (!q || !com) return fail(LMH_ERR_BAD_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpy(h->d_state.get(), q, sizeof(double) * 30 * (size_t)h->B, hipMemcpyHostToDevice));
    rc = lmh_robot_com(h, h->d_state.get(), h->d_out.get(), nullptr);
    if (rc) return rc;
    HIPCHK(hipMemcpy(com, h->d_out.get(), sizeof(double) * 3 * (size_t)h->B, hipMemcpyDeviceToHost));
    return LMH_OK;
}

// ---------------------------------------------------------------------------- rigid-body terms, inverse / forward dynamics
// The kernels read h->P's model tables only.
static int terms_body(lmh_handle *h, int mode, const double *d_q, const double *d_v, const double *d_x, const double *d_w, double *d_res, int32_t *d_flags, void *stream)
{
    return launch(h, (!d_q || !d_res || (mode != TM_TERMS && !d_x)) ? "null device pointer" : nullptr,
                  [&] { lmh_launch_terms(&h->P, mode, d_q, d_v, d_x, d_w, d_res, d_flags, (hipStream_t)stream); });
}

extern "C" int lmh_terms(lmh_handle *h, const double *d_q, const double *d_v, double *d_terms, void *stream)
{
    return terms_body(h, TM_TERMS, d_q, d_v, nullptr, nullptr, d_terms, nullptr, stream);
}

extern "C" int lmh_inverse_dynamics(lmh_handle *h, const double *d_q, const double *d_v, const double *d_qdd, const double *d_w, double *d_tau30, void *stream)
{
    return terms_body(h, TM_INVDYN, d_q, d_v, d_qdd, d_w, d_tau30, nullptr, stream);
}

extern "C" int lmh_forward_dynamics(lmh_handle *h, const double *d_q, const double *d_v, const double *d_tau30, const double *d_w, double *d_qdd, int32_t *d_flags, void *stream)
{
    return terms_body(h, TM_FWDDYN, d_q, d_v, d_tau30, d_w, d_qdd, d_flags, stream);
}

// ---------------------------------------------------------------------------- torque-driven plant
// A handle with plant = 0 never had its contact constants checked (validate_config, lmh_set_params): the plant calls check the host copy
static int plant_constants_ok(const lmh_handle *h)
{
    if (!h->inst.on()) {
        double rec[LMH_PARAM_STRIDE];
        config_record(h->cfg, rec);
        const char *why = contact_error(rec);
        return why ? fail(LMH_ERR_BAD_ARG, why) : LMH_OK;
    }
    for (int i = 0; i < h->B; i++)
        if (const char *why = contact_error(h->inst.h_rec.data() + (size_t)LMH_PARAM_STRIDE * i)) return fail(LMH_ERR_BAD_ARG, robot_msg(i, why));
    return LMH_OK;
}

// One plant call: the mode, the pointers its launch takes (those a call does not have stay NULL) and the step count.
// servo (lmh_plant_step_servo): d_setpoint is required and the handle's servo table rides along; without one the launcher never reads it.
// d_hold, kv, d_lambda (PM_RIGID_*): the rigid plant's; it reads neither the ground nor the servo table, so neither rides along.
// PM_RIGID_IMPACT (lmh_plant_impact_rigid): d_q, d_v, d_hold; d_xdot is d_v_plus and d_lambda the impulse; no torque, no kv, no count.
struct PlantCall {
    int mode, n_substeps;
    const double *d_q, *d_v, *d_tau30, *d_setpoint;
    double *d_state, *d_xdot, *d_contact, *d_lambda;
    int32_t *d_flags;
    const int32_t *d_hold;
    double kv;
    bool servo;
};
static bool kv_ok(double kv) { return kv >= 0.0 && kv <= 1.7976931348623157e308; }     // finite and >= 0 (a NaN fails both)

// The eight plant calls behind their names.  Refusals in this order: the handle, the pointers the mode requires, the servo's setpoint, the rigid
// plant's kv, the count, the contact constants; a step call with no substep enqueues nothing but still answers for all of them.
static int plant_body(lmh_handle *h, const char *name, const PlantCall &c, void *stream)
{
    const int rc = ready(h); if (rc) return rc;
    const std::string who = std::string(name) + ": ";
    const bool step = c.mode == PM_STEP || c.mode == PM_RIGID_STEP, impact = c.mode == PM_RIGID_IMPACT, rigid = c.mode == PM_RIGID_DERIV || c.mode == PM_RIGID_STEP || impact;
    if (impact && !c.d_q) return fail(LMH_ERR_BAD_ARG, who + "null d_q");
    if (impact && !c.d_v) return fail(LMH_ERR_BAD_ARG, who + "null d_v");
    if (impact && !c.d_xdot) return fail(LMH_ERR_BAD_ARG, who + "null d_v_plus");
    if (step ? !c.d_state : (c.mode == PM_CONTACT) ? (!c.d_q || !c.d_contact) : (!c.d_q || !c.d_v || !c.d_xdot)) return fail(LMH_ERR_BAD_ARG, who + "null device pointer");
    if (c.servo && !c.d_setpoint) return fail(LMH_ERR_BAD_ARG, who + "null d_setpoint");
    if (rigid && !kv_ok(c.kv)) return fail(LMH_ERR_BAD_ARG, who + "kv must be finite and >= 0");
    if (c.n_substeps < 0) return fail(LMH_ERR_BAD_ARG, who + "n_substeps must be >= 0");
    const int bad = plant_constants_ok(h);
    if (bad || (step && c.n_substeps == 0)) return bad;              // no substep: nothing to enqueue
    return launch(h, nullptr, [&] { lmh_launch_plant(&h->P, c.mode, c.d_q, c.d_v, c.d_tau30, c.d_state, c.d_xdot, c.d_contact, c.d_flags, c.n_substeps, rigid ? nullptr : h->ground.device(),
                                                     rigid ? 0 : h->ground.stride(LMH_GROUND_STRIDE), c.servo ? h->servo.device() : nullptr, h->servo.stride(LMH_SERVO_STRIDE), c.d_setpoint,
                                                     c.d_hold, c.kv, c.d_lambda, (hipStream_t)stream); });
}

extern "C" int lmh_contact_wrench(lmh_handle *h, const double *d_q, const double *d_v, double *d_contact, void *stream)
{
    PlantCall c = {}; c.mode = PM_CONTACT; c.d_q = d_q; c.d_v = d_v; c.d_contact = d_contact;
    return plant_body(h, "lmh_contact_wrench", c, stream);
}

extern "C" int lmh_plant_derivative(lmh_handle *h, const double *d_q, const double *d_v, const double *d_tau30, double *d_xdot, double *d_contact, int32_t *d_flags, void *stream)
{
    PlantCall c = {}; c.mode = PM_DERIV; c.d_q = d_q; c.d_v = d_v; c.d_tau30 = d_tau30; c.d_xdot = d_xdot; c.d_contact = d_contact; c.d_flags = d_flags;
    return plant_body(h, "lmh_plant_derivative", c, stream);
}

extern "C" int lmh_plant_step(lmh_handle *h, double *d_state, const double *d_tau30, int n_substeps, int32_t *d_flags, void *stream)
{
    PlantCall c = {}; c.mode = PM_STEP; c.d_state = d_state; c.d_tau30 = d_tau30; c.n_substeps = n_substeps; c.d_flags = d_flags;
    return plant_body(h, "lmh_plant_step", c, stream);
}

// lmh_plant_step with the joint servo re-forming the joint torques at every derivative evaluation (include/lmh.h)
extern "C" int lmh_plant_step_servo(lmh_handle *h, double *d_state, const double *d_tau30, const double *d_setpoint, int n_substeps, int32_t *d_flags, void *stream)
{
    PlantCall c = {}; c.mode = PM_STEP; c.d_state = d_state; c.d_tau30 = d_tau30; c.n_substeps = n_substeps; c.d_flags = d_flags; c.servo = true; c.d_setpoint = d_setpoint;
    return plant_body(h, "lmh_plant_step_servo", c, stream);
}

// The rigid-contact plant (include/lmh.h): the held soles as constraints, the contact wrench their multiplier.  lmh_plant_step's rule set, with
// kv between the pointers and the count.
extern "C" int lmh_plant_derivative_rigid(lmh_handle *h, const double *d_q, const double *d_v, const double *d_tau30, const int32_t *d_mode, double kv, double *d_xdot, double *d_lambda,
                                          int32_t *d_flags, void *stream)
{
    PlantCall c = {}; c.mode = PM_RIGID_DERIV; c.d_q = d_q; c.d_v = d_v; c.d_tau30 = d_tau30; c.d_xdot = d_xdot; c.d_flags = d_flags; c.d_hold = d_mode; c.kv = kv; c.d_lambda = d_lambda;
    return plant_body(h, "lmh_plant_derivative_rigid", c, stream);
}

extern "C" int lmh_plant_step_rigid(lmh_handle *h, double *d_state, const double *d_tau30, const int32_t *d_mode, double kv, int n_substeps, double *d_lambda, int32_t *d_flags, void *stream)
{
    PlantCall c = {}; c.mode = PM_RIGID_STEP; c.d_state = d_state; c.d_tau30 = d_tau30; c.n_substeps = n_substeps; c.d_flags = d_flags; c.d_hold = d_mode; c.kv = kv; c.d_lambda = d_lambda;
    return plant_body(h, "lmh_plant_step_rigid", c, stream);
}

// The rigid plant's plastic impact (include/lmh.h): the two rigid calls' rule set without a torque, a kv or a count
extern "C" int lmh_plant_impact_rigid(lmh_handle *h, const double *d_q, const double *d_v, const int32_t *d_mode, double *d_v_plus, double *d_impulse, int32_t *d_flags, void *stream)
{
    PlantCall c = {}; c.mode = PM_RIGID_IMPACT; c.d_q = d_q; c.d_v = d_v; c.d_xdot = d_v_plus; c.d_flags = d_flags; c.d_hold = d_mode; c.d_lambda = d_impulse;
    return plant_body(h, "lmh_plant_impact_rigid", c, stream);
}

// ---------------------------------------------------------------------------- zero-order-hold closed loop
// n_ticks rounds of { lmh_eval ; lmh_plant_step(tau30 = [base_wrench | out.tau], n_substeps) } in one launch (lmh_kernels.hip,
// lmh_rollout_zoh_ex_body's kernels).  The parameter block travels by value, so the call takes no launch slot.
// One call of the family: the records its entry point was given, NULL for those it does not have (and for those its caller left out: either is the
// all-zero record).  lmh_rollout_zoh and lmh_rollout_zoh_ref hand their three pointers over in an options record of their own.
struct ZohBoxCall { const double *d_box; int n_samples, n_sets; double *d_mpc; };
struct ZohCall {
    const lmh_zoh_opts *opts;
    const ZohBoxCall *box;        // lmh_rollout_zoh_box: never with io, servo or rigid
    const lmh_zoh_io *io;
    const lmh_zoh_servo *servo;   // lmh_rollout_zoh_servo: never with rigid
    const lmh_zoh_rigid *rigid;
    const lmh_zoh_impact *impact; // lmh_rollout_zoh_rigid_impact: only with a rigid record that is on
    bool d_ref_required;          // lmh_rollout_zoh_ref
};
static const lmh_zoh_opts kNoOpts = {}; static const lmh_zoh_io kNoIo = {}; static const lmh_zoh_servo kNoServo = {}; static const lmh_zoh_rigid kNoRigid = {};
static const lmh_zoh_impact kNoImpact = {};

// The refusals of each record, in the words and the order they always had; nullptr = fine
static const char *zoh_box_refusal(const lmh_handle *h, const ZohBoxCall &bx, const lmh_zoh_opts &o)
{
    if (const char *why = box_refusal(h, bx.d_box, bx.n_samples, bx.n_sets, "lmh_rollout_zoh_box: null d_box",
                                      "lmh_rollout_zoh_box: n_samples must be lmh_num_ref_samples", "lmh_rollout_zoh_box: n_sets must be 1 or n_instances"))
        return why;
    if (o.d_ref) return "lmh_rollout_zoh_box: opts->d_ref must be NULL (the box-constrained step is the reference: the two are exclusive)";
    if (h->ground.n_sets > 0) return "lmh_rollout_zoh_box: not offered on a handle with a ground table (lmh_set_ground(NULL) clears it)";
    return nullptr;
}
static const char *zoh_opts_refusal(const lmh_zoh_opts &o, int n_ticks, int n_substeps)
{
    if ((o.wrench_per_tick | 1) != 1) return "lmh_rollout_zoh_ex: wrench_per_tick must be 0 or 1";
    if ((o.pushes | 1) != 1) return "lmh_rollout_zoh_ex: pushes must be 0 or 1";
    if (o.reserved != 0) return "lmh_rollout_zoh_ex: reserved must be 0";
    if (o.wrench_per_tick && !o.d_base_wrench) return "lmh_rollout_zoh_ex: wrench_per_tick = 1 needs d_base_wrench";
    if (o.trace_every < 0 || (o.d_trace != nullptr) != (o.trace_every > 0)) return "lmh_rollout_zoh_ex: d_trace and trace_every > 0 go together (NULL and 0: no trace)";
    if (o.pushes && n_substeps == 0 && n_ticks > 0)
        return "lmh_rollout_zoh_ex: pushes = 1 needs n_substeps > 0 (push ticks are plant substeps: with none the clock does not move)";
    if (o.pushes && (long long)n_ticks * n_substeps >= 0x3fffffffll) return "lmh_rollout_zoh_ex: pushes = 1 needs n_ticks * n_substeps < 2^30 - 1";
    return nullptr;
}
static const char *zoh_io_refusal(const lmh_zoh_io &io)
{
    if ((io.actuators | 1) != 1) return "lmh_rollout_zoh_io: actuators must be 0 or 1";
    if (io.reserved != 0) return "lmh_rollout_zoh_io: reserved must be 0";
    if (io.actuators && !io.d_act_mem) return "lmh_rollout_zoh_io: actuators = 1 needs d_act_mem";
    return nullptr;
}
static const char *zoh_servo_refusal(const lmh_zoh_servo &sv, int n_substeps)
{
    if (sv.mode != 0 && sv.mode != LMH_SERVO_INTEGRATE && sv.mode != LMH_SERVO_CALLER) return "lmh_rollout_zoh_servo: mode must be 0, LMH_SERVO_INTEGRATE or LMH_SERVO_CALLER";
    if (sv.reserved != 0) return "lmh_rollout_zoh_servo: reserved must be 0";
    if (sv.mode == LMH_SERVO_CALLER && !sv.d_setpoint) return "lmh_rollout_zoh_servo: mode LMH_SERVO_CALLER needs d_setpoint";
    if (sv.mode != LMH_SERVO_CALLER && sv.d_setpoint) return "lmh_rollout_zoh_servo: d_setpoint goes with mode LMH_SERVO_CALLER only";
    if (sv.mode == LMH_SERVO_INTEGRATE && n_substeps == 0)
        return "lmh_rollout_zoh_servo: mode LMH_SERVO_INTEGRATE needs n_substeps > 0 (the setpoint is the end of a control period: with no substep there is none)";
    return nullptr;
}
static const char *zoh_rigid_refusal(const lmh_zoh_rigid &rg)
{
    if (rg.source != 0 && rg.source != LMH_RIGID_FIXED && rg.source != LMH_RIGID_PER_TICK && rg.source != LMH_RIGID_PLAN)
        return "lmh_rollout_zoh_rigid: source must be 0, LMH_RIGID_FIXED, LMH_RIGID_PER_TICK or LMH_RIGID_PLAN";
    if (rg.reserved != 0) return "lmh_rollout_zoh_rigid: reserved must be 0";
    if (!kv_ok(rg.kv)) return "lmh_rollout_zoh_rigid: kv must be finite and >= 0";
    if (rg.source == LMH_RIGID_PER_TICK && !rg.d_mode) return "lmh_rollout_zoh_rigid: source LMH_RIGID_PER_TICK needs d_mode";
    if (rg.source == LMH_RIGID_PLAN && rg.d_mode) return "lmh_rollout_zoh_rigid: d_mode must be NULL with source LMH_RIGID_PLAN (the robot's own plan decides)";
    return nullptr;
}

static const char *zoh_impact_refusal(const lmh_zoh_impact &im, const lmh_zoh_rigid &rg)
{
    if ((im.enable | 1) != 1) return "lmh_rollout_zoh_rigid_impact: enable must be 0 or 1";
    if (im.reserved != 0) return "lmh_rollout_zoh_rigid_impact: reserved must be 0";
    if (im.enable && rg.source == 0) return "lmh_rollout_zoh_rigid_impact: enable = 1 needs a rigid record with a source (the impact is the rigid plant's)";
    if (im.enable && !im.d_mode_prev) return "lmh_rollout_zoh_rigid_impact: enable = 1 needs d_mode_prev";
    return nullptr;
}

// Refusals in the order of the two calls the loop composes, every record's own behind the counts they depend on: the handle, the pointers, d_ref
// where it is required, the box, the counts, the options, io, servo, rigid, impact, then the precision and the contact constants.
static int zoh_body(lmh_handle *h, double *d_state, double *d_out, int32_t *d_status, int n_ticks, int n_substeps, void *stream, const ZohCall &c)
{
    int rc = ready(h); if (rc) return rc;                            // no record is read before this
    const lmh_zoh_opts &o = c.opts ? *c.opts : kNoOpts;
    const lmh_zoh_io &io = c.io ? *c.io : kNoIo;
    const lmh_zoh_servo &sv = c.servo ? *c.servo : kNoServo;
    const lmh_zoh_rigid &rg = c.rigid ? *c.rigid : kNoRigid;
    const lmh_zoh_impact &im = c.impact ? *c.impact : kNoImpact;
    const char *why = nullptr;
    if (!d_state || !d_out || !d_status) why = "lmh_rollout_zoh: null device pointer";
    else if (c.d_ref_required && !o.d_ref) why = "lmh_rollout_zoh_ref: null d_ref";
    if (!why && c.box) why = zoh_box_refusal(h, *c.box, o);
    if (!why && (n_ticks < 0 || n_substeps < 0)) why = "lmh_rollout_zoh: n_ticks and n_substeps must be >= 0";
    if (!why) why = zoh_opts_refusal(o, n_ticks, n_substeps);
    if (!why) why = zoh_io_refusal(io);
    if (!why) why = zoh_servo_refusal(sv, n_substeps);
    if (!why) why = zoh_rigid_refusal(rg);
    if (!why) why = zoh_impact_refusal(im, rg);
    if (!why && h->cfg.precision != LMH_PRECISION_FP64) why = "lmh_rollout_zoh: LMH_PRECISION_FP64 handles only (this handle's precision has no instantiation of the kernel)";
    if (why) return fail(LMH_ERR_BAD_ARG, why);
    rc = plant_constants_ok(h); if (rc) return rc;
    if (n_ticks == 0) return LMH_OK;                                 // nothing to enqueue
    if (c.box && h->zoh_box_prepared != 0 && h->N > 33)              // N >= 34: above 64 KB of LDS in all, only with the limit lmh_create asked for
        return fail(LMH_ERR_HIP, "lmh_rollout_zoh_box: the runtime refused the kernel's dynamic shared memory limit when the handle was created");
    // What the one launch is given, and with it which kernel of the family runs (lmh_launch.h); the options record always rides along:
    //   box                     the box record; ref is NULL and the handle has no ground table (both refused above); no io, servo, rigid
    //   rigid, source != 0      the io record always and the rigid record; no ground, no servo
    //   impact, enable != 0     the rigid launch's records and the impact record (never without rigid: refused above)
    //   servo, mode != 0        the io record always, the ground as the handle has it, the servo record with the handle's table and stride
    //   io that asks something  the io record, the ground
    //   otherwise               no io record, the ground
    const bool rigid = rg.source != 0, servo = sv.mode != 0;
    const bool with_io = rigid || servo || io.d_meas || io.d_applied || io.actuators;
    LmhZohEx ex = {};
    ex.trace = o.d_trace; ex.metrics = o.d_metrics; ex.trace_every = o.trace_every; ex.wrench_per_tick = o.wrench_per_tick; ex.pushes = o.pushes;
    const LmhZohBox zb = {c.box ? c.box->d_box : nullptr, c.box ? box_stride(h, c.box->n_sets) : 0, c.box ? c.box->d_mpc : nullptr, h->cfg.alpha, h->cfg.beta, 0, nullptr};
    const LmhZohIo zi = {io.d_meas, io.actuators ? io.d_act_mem : nullptr, io.d_applied, h->act.device(), h->act.stride(LMH_ACT_STRIDE), io.actuators, 0};
    const LmhZohServo zs = {sv.d_setpoint, h->servo.device(), h->servo.stride(LMH_SERVO_STRIDE), sv.mode, 0};
    const LmhZohRigid zr = {rg.d_mode, rg.d_lambda, rg.kv, rg.source, 0};
    const LmhZohImpact zm = {im.d_mode_prev, im.d_impulse};
    return launch(h, nullptr, [&] { lmh_launch_rollout_zoh(&h->P, d_state, d_out, d_status, o.d_base_wrench, o.d_log, o.d_ref, n_ticks, n_substeps, &ex, c.box ? &zb : nullptr, with_io ? &zi : nullptr,
                                                           rigid ? nullptr : h->ground.device(), rigid ? 0 : h->ground.stride(LMH_GROUND_STRIDE), servo ? &zs : nullptr, rigid ? &zr : nullptr,
                                                           im.enable ? &zm : nullptr, (hipStream_t)stream); });
}

extern "C" int lmh_rollout_zoh(lmh_handle *h, double *d_state, double *d_out, int32_t *d_status, const double *d_base_wrench, double *d_log,
                               int n_ticks, int n_substeps, void *stream)
{
    lmh_zoh_opts o = {}; o.d_base_wrench = d_base_wrench; o.d_log = d_log;
    ZohCall c = {}; c.opts = &o;
    return zoh_body(h, d_state, d_out, d_status, n_ticks, n_substeps, stream, c);
}
extern "C" int lmh_rollout_zoh_ref(lmh_handle *h, double *d_state, double *d_out, int32_t *d_status, const double *d_base_wrench, double *d_log, const double *d_ref,
                                   int n_ticks, int n_substeps, void *stream)
{
    lmh_zoh_opts o = {}; o.d_base_wrench = d_base_wrench; o.d_log = d_log; o.d_ref = d_ref;
    ZohCall c = {}; c.opts = &o; c.d_ref_required = true;
    return zoh_body(h, d_state, d_out, d_status, n_ticks, n_substeps, stream, c);
}
// the wrench, the reference and the log ride in the record: NULL there is what NULL is in the two calls above (d_ref NULL: the built-in preview step)
extern "C" int lmh_rollout_zoh_ex(lmh_handle *h, double *d_state, double *d_out, int32_t *d_status, const lmh_zoh_opts *opts, int n_ticks, int n_substeps, void *stream)
{
    ZohCall c = {}; c.opts = opts;
    return zoh_body(h, d_state, d_out, d_status, n_ticks, n_substeps, stream, c);
}

// lmh_rollout_zoh_ex with a measurement in front of the evaluation and an actuator behind it (include/lmh.h)
extern "C" int lmh_rollout_zoh_io(lmh_handle *h, double *d_state, double *d_out, int32_t *d_status, const lmh_zoh_opts *opts, const lmh_zoh_io *io, int n_ticks, int n_substeps,
                                  void *stream)
{
    ZohCall c = {}; c.opts = opts; c.io = io;
    return zoh_body(h, d_state, d_out, d_status, n_ticks, n_substeps, stream, c);
}

// lmh_rollout_zoh_io with the joint servo inside every hold (include/lmh.h)
extern "C" int lmh_rollout_zoh_servo(lmh_handle *h, double *d_state, double *d_out, int32_t *d_status, const lmh_zoh_opts *opts, const lmh_zoh_io *io, const lmh_zoh_servo *servo,
                                     int n_ticks, int n_substeps, void *stream)
{
    ZohCall c = {}; c.opts = opts; c.io = io; c.servo = servo;
    return zoh_body(h, d_state, d_out, d_status, n_ticks, n_substeps, stream, c);
}

// lmh_rollout_zoh_io with the rigid-contact plant in every hold (include/lmh.h)
extern "C" int lmh_rollout_zoh_rigid(lmh_handle *h, double *d_state, double *d_out, int32_t *d_status, const lmh_zoh_opts *opts, const lmh_zoh_io *io, const lmh_zoh_rigid *rigid,
                                     int n_ticks, int n_substeps, void *stream)
{
    ZohCall c = {}; c.opts = opts; c.io = io; c.rigid = rigid;
    return zoh_body(h, d_state, d_out, d_status, n_ticks, n_substeps, stream, c);
}

// lmh_rollout_zoh_rigid with the plastic impact in front of every hold that holds a foot more than the hold before it (include/lmh.h)
extern "C" int lmh_rollout_zoh_rigid_impact(lmh_handle *h, double *d_state, double *d_out, int32_t *d_status, const lmh_zoh_opts *opts, const lmh_zoh_io *io, const lmh_zoh_rigid *rigid,
                                            const lmh_zoh_impact *impact, int n_ticks, int n_substeps, void *stream)
{
    ZohCall c = {}; c.opts = opts; c.io = io; c.rigid = rigid; c.impact = impact;
    return zoh_body(h, d_state, d_out, d_status, n_ticks, n_substeps, stream, c);
}

// lmh_rollout_zoh_ex with lmh_mpc_box_step closing the loop inside every evaluation (include/lmh.h)
extern "C" int lmh_rollout_zoh_box(lmh_handle *h, double *d_state, double *d_out, int32_t *d_status, const lmh_zoh_opts *opts, const double *d_box, int n_samples, int n_sets,
                                   double *d_mpc, int n_ticks, int n_substeps, void *stream)
{
    const ZohBoxCall bx = {d_box, n_samples, n_sets, d_mpc};
    ZohCall c = {}; c.opts = opts; c.box = &bx;
    return zoh_body(h, d_state, d_out, d_status, n_ticks, n_substeps, stream, c);
}

extern "C" int lmh_terms_host(lmh_handle *h, const double *q, const double *v, double *terms)
{
    int rc = ready(h); if (rc) return rc;
    if (!q || !terms) return fail(LMH_ERR_BAD_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    const size_t n = (size_t)h->B;
    if (!h->d_terms.get()) HIPCHK(h->d_terms.alloc((60 + LMH_TERMS_STRIDE) * n));
    double *d_q = h->d_terms.get(), *d_v = d_q + 30 * n, *d_t = d_q + 60 * n;
    HIPCHK(hipMemcpy(d_q, q, sizeof(double) * 30 * n, hipMemcpyHostToDevice));
    if (v) HIPCHK(hipMemcpy(d_v, v, sizeof(double) * 30 * n, hipMemcpyHostToDevice));
    rc = lmh_terms(h, d_q, v ? d_v : nullptr, d_t, nullptr);
    if (rc) return rc;
    HIPCHK(hipMemcpy(terms, d_t, sizeof(double) * LMH_TERMS_STRIDE * n, hipMemcpyDeviceToHost));
    return LMH_OK;
}

extern "C" int lmh_mpc_step_host(lmh_handle *h, const double *lip, double *mpc)
{
    int rc = ready(h); if (rc) return rc;
    if (!lip || !mpc) return fail(LMH_ERR_BAD_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    const size_t n = (size_t)h->B;
    if (!h->d_mpc_host.get()) HIPCHK(h->d_mpc_host.alloc((LMH_LIP_STRIDE + LMH_MPC_STRIDE) * n));
    double *d_lip = h->d_mpc_host.get(), *d_rec = d_lip + LMH_LIP_STRIDE * n;
    HIPCHK(hipMemcpy(d_lip, lip, sizeof(double) * LMH_LIP_STRIDE * n, hipMemcpyHostToDevice));
    rc = lmh_mpc_step(h, d_lip, d_rec, nullptr);
    if (rc) return rc;
    HIPCHK(hipMemcpy(mpc, d_rec, sizeof(double) * LMH_MPC_STRIDE * n, hipMemcpyDeviceToHost));
    return LMH_OK;
}

extern "C" int lmh_last_out_host(lmh_handle *h, double *out)
{
    if (!h || !out) return fail(LMH_ERR_BAD_ARG, "bad argument");
    std::memcpy(out, h->h_out.data(), sizeof(double) * h->h_out.size());
    return LMH_OK;
}

extern "C" int lmh_ik_host(lmh_handle *h, double *q, const double *com_target, const double *rf6, const double *lf6, double *com, int32_t *iters)
{
    int rc = ready(h); if (rc) return rc;
    if (!q || !com_target || !rf6 || !lf6) return fail(LMH_ERR_BAD_ARG, "bad argument");
    HIPCHK(hipSetDevice(h->device));
    double *d_q = h->d_state.get();                                       // staging: reuse the state buffer
    double *d_com = h->d_out.get();
    HIPCHK(hipMemcpy(d_q, q, sizeof(double) * 30 * (size_t)h->B, hipMemcpyHostToDevice));
    rc = lmh_ik(h, d_q, com_target, rf6, lf6, h->d_status.get(), nullptr);
    if (rc) return rc;
    rc = lmh_robot_com(h, d_q, d_com, nullptr);
    if (rc) return rc;
    HIPCHK(hipMemcpy(q, d_q, sizeof(double) * 30 * (size_t)h->B, hipMemcpyDeviceToHost));
    if (com) HIPCHK(hipMemcpy(com, d_com, sizeof(double) * 3 * (size_t)h->B, hipMemcpyDeviceToHost));
    if (iters) HIPCHK(hipMemcpy(iters, h->d_status.get(), sizeof(int32_t) * (size_t)h->B, hipMemcpyDeviceToHost));
    HIPCHK(hipMemset(h->d_status.get(), 0, sizeof(int32_t) * LMH_STATUS_STRIDE * (size_t)h->B));
    return LMH_OK;
}

extern "C" int lmh_set_prev_velocity_host(lmh_handle *h, const double *v /*[B][30]*/)
{
    if (!h || !v) return fail(LMH_ERR_BAD_ARG, "bad argument");
    for (int i = 0; i < h->B; i++) std::memcpy(h->h_state.data() + (size_t)LMH_STATE_STRIDE * i + 60, v + 30 * (size_t)i, 30 * sizeof(double));
    return LMH_OK;
}

extern "C" int lmh_synchronize(lmh_handle *h, void *stream)
{
    if (!h) return fail(LMH_ERR_BAD_ARG, "null handle");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    int rc = LMH_OK;
    for (auto &sl : h->slot)                                         // launches that have completed (on this stream or any other) and were not looked at yet
        if (sl.used && !sl.checked && hipEventQuery(sl.done) == hipSuccess) { const int e = slot_take_error(sl); if (e) rc = e; }
    return rc;
}

// ---------------------------------------------------------------------------- end-of-run summary + on-disk records
extern "C" int lmh_make_summary(lmh_handle *h, const double *d_state, const double *d_out, const int32_t *d_status, double *d_summary, void *stream)
{
    if (!h || !d_state || !d_out || !d_status || !d_summary) return fail(LMH_ERR_BAD_ARG, "bad argument");
    return launch(h, nullptr, [&] { lmh_launch_summary(h->B, d_state, d_out, d_status, d_summary, (hipStream_t)stream); });
}

namespace {
#pragma pack(push, 1)
struct RecHeader {                                                   // 64 bytes, little-endian (include/lmh.h)
    char magic[8]; uint32_t version, dtype; uint64_t n_instances, n_ticks; uint32_t width, pad0; double dt, t0; uint64_t pad1;
};
#pragma pack(pop)
static_assert(sizeof(RecHeader) == 64, "record header is 64 bytes");
const char kMagicSum[8] = {'L', 'M', 'H', 'S', 'U', 'M', '1', 0}, kMagicLog[8] = {'L', 'M', 'H', 'L', 'O', 'G', '1', 0},
           kMagicTrace[8] = {'L', 'M', 'H', 'T', 'R', 'J', '1', 0};

int write_rec(const char *path, const char *magic, const double *data, uint64_t n_inst, uint64_t n_ticks, uint32_t width, double dt, double t0)
{
    if (!path || !data) return fail(LMH_ERR_BAD_ARG, "bad argument");
    FILE *f = std::fopen(path, "wb");
    if (!f) return fail(LMH_ERR_BAD_ARG, std::string("cannot open ") + path);
    RecHeader hd;
    std::memset(&hd, 0, sizeof(hd));
    std::memcpy(hd.magic, magic, 8);
    hd.version = 1; hd.dtype = 1; hd.n_instances = n_inst; hd.n_ticks = n_ticks; hd.width = width; hd.dt = dt; hd.t0 = t0;
    const size_t count = (size_t)n_inst * width * (size_t)(n_ticks ? n_ticks : 1);
    const bool ok = std::fwrite(&hd, sizeof(hd), 1, f) == 1 && (count == 0 || std::fwrite(data, sizeof(double), count, f) == count);
    if (std::fclose(f) != 0 || !ok) return fail(LMH_ERR_BAD_ARG, std::string("short write to ") + path);
    return LMH_OK;
}

// per_tick: a log or a trace, one record per robot and tick / sample; else a summary, one record per robot
int read_rec(const char *path, const char *magic, uint32_t width, bool per_tick, double *data, uint64_t capacity, RecHeader *hd)
{
    if (!path) return fail(LMH_ERR_BAD_ARG, "bad argument");
    FILE *f = std::fopen(path, "rb");
    if (!f) return fail(LMH_ERR_BAD_ARG, std::string("cannot open ") + path);
    int rc = LMH_OK;
    if (std::fread(hd, sizeof(*hd), 1, f) != 1) rc = fail(LMH_ERR_BAD_ARG, "truncated header");
    else if (std::memcmp(hd->magic, magic, 8) != 0) rc = fail(LMH_ERR_BAD_ARG, "bad magic");
    else if (hd->version != 1 || hd->dtype != 1 || hd->width != width) rc = fail(LMH_ERR_BAD_ARG, "unsupported version / dtype / width");
    else {
        const uint64_t count = hd->n_instances * width * (per_tick ? hd->n_ticks : 1);
        long pos = std::ftell(f);
        std::fseek(f, 0, SEEK_END);
        const long end = std::ftell(f);
        std::fseek(f, pos, SEEK_SET);
        if ((uint64_t)(end - pos) != count * sizeof(double)) rc = fail(LMH_ERR_BAD_ARG, "payload size does not match the header");
        else if (data) {
            if (capacity < count) rc = fail(LMH_ERR_BAD_ARG, "buffer too small");
            else if (count && std::fread(data, sizeof(double), (size_t)count, f) != count) rc = fail(LMH_ERR_BAD_ARG, "short read");
        }
    }
    std::fclose(f);
    return rc;
}

// what a reader reports beside the payload: every out-pointer is optional
void header_out(const RecHeader &hd, uint64_t *n_ticks, uint64_t *n_instances, double *dt, double *t0)
{
    if (n_ticks) *n_ticks = hd.n_ticks;
    if (n_instances) *n_instances = hd.n_instances;
    if (dt) *dt = hd.dt;
    if (t0) *t0 = hd.t0;
}
}  // namespace

extern "C" int lmh_write_summary(const char *path, const double *summary, uint64_t n_instances, double dt)
{
    return write_rec(path, kMagicSum, summary, n_instances, 0, LMH_SUMMARY_WIDTH, dt, 0.0);
}
extern "C" int lmh_read_summary(const char *path, double *summary, uint64_t capacity, uint64_t *n_instances, double *dt)
{
    RecHeader hd;
    const int rc = read_rec(path, kMagicSum, LMH_SUMMARY_WIDTH, false, summary, capacity, &hd);
    if (rc == LMH_OK) header_out(hd, nullptr, n_instances, dt, nullptr);
    return rc;
}
extern "C" int lmh_write_log(const char *path, const double *log, uint64_t n_ticks, uint64_t n_instances, double dt, double t0)
{
    if (n_ticks == 0) return fail(LMH_ERR_BAD_ARG, "a log holds at least one tick");
    return write_rec(path, kMagicLog, log, n_instances, n_ticks, 36, dt, t0);
}
extern "C" int lmh_read_log(const char *path, double *log, uint64_t capacity, uint64_t *n_ticks, uint64_t *n_instances, double *dt, double *t0)
{
    RecHeader hd;
    const int rc = read_rec(path, kMagicLog, 36, true, log, capacity, &hd);
    if (rc == LMH_OK) header_out(hd, n_ticks, n_instances, dt, t0);
    return rc;
}
extern "C" int lmh_write_trace(const char *path, const double *trace, uint64_t n_samples, uint64_t n_instances, double sample_dt, double t0)
{
    if (n_samples == 0) return fail(LMH_ERR_BAD_ARG, "a trace holds at least one sample");
    return write_rec(path, kMagicTrace, trace, n_instances, n_samples, LMH_TRACE_STRIDE, sample_dt, t0);
}
extern "C" int lmh_read_trace(const char *path, double *trace, uint64_t capacity, uint64_t *n_samples, uint64_t *n_instances, double *sample_dt, double *t0)
{
    RecHeader hd;
    const int rc = read_rec(path, kMagicTrace, LMH_TRACE_STRIDE, true, trace, capacity, &hd);
    if (rc == LMH_OK) header_out(hd, n_samples, n_instances, sample_dt, t0);
    return rc;
}

// ---------------------------------------------------------------------------- reference generators on the device
// fresh buffers for a generator kernel to fill: every plan has a phase slice, segments only where n_seg > 0
static int alloc_plan(RefPlan &p, int n_samples, int n_seg, int n_plans)
{
    const size_t ns = (size_t)n_samples * (size_t)n_plans;
    HIPCHK(p.zx.alloc(ns));
    HIPCHK(p.zy.alloc(ns));
    HIPCHK(p.phase.alloc(ns));
    if (n_seg > 0) {
        HIPCHK(p.segs.alloc(LMH_SEG_STRIDE * (size_t)n_seg * (size_t)n_plans));
        HIPCHK(p.sos.alloc(ns));
    }
    p.n_samples = n_samples; p.n_seg = n_seg; p.n_plans = n_plans;
    return LMH_OK;
}

// the argument rules of lmh_gen_walk (one spec of lmh_gen_walk_batch): nullptr = fine
static const char *walk_spec_error(double simulation_time, const lmh_walk_spec &s)
{
    if (s.num_steps < 1 || s.num_steps > LMH_GEN_MAX_STEPS) return "num_steps must be in [1, 1022]";
    if (!(s.time_per_step > 0.0) || !(s.ds_time >= 0.0) || !(s.ds_time < s.time_per_step) || !(s.settle_time >= 0.0) || !(simulation_time > 0.0))
        return "need 0 <= ds_time < time_per_step, settle_time >= 0, simulation_time > 0";
    if (s.first_support != LMH_PHASE_RIGHT && s.first_support != LMH_PHASE_LEFT) return "first_support must be LMH_PHASE_RIGHT or LMH_PHASE_LEFT";
    return nullptr;
}

// lmh_gen_walk (batch = false: specs[0], today's single-plan launch) and lmh_gen_walk_batch (one spec and one workgroup per robot)
static int gen_walk(lmh_handle *h, double simulation_time, const lmh_walk_spec *specs, int n, bool batch)
{
    const int ns = sample_count(h, simulation_time);                // one sample grid for all robots
    int max_steps = 0;
    std::vector<LmhWalkSpec> W((size_t)n);
    for (int i = 0; i < n; i++) {
        const lmh_walk_spec &s = specs[i];
        if (const char *msg = walk_spec_error(simulation_time, s)) return fail(LMH_ERR_BAD_ARG, batch ? robot_msg(i, msg) : msg);
        W[(size_t)i] = LmhWalkSpec{h->mpc_dt, s.time_per_step, s.ds_time, s.step_height, s.settle_time, s.foot_y, ns, s.num_steps, s.first_support, 0};
        if (s.num_steps > max_steps) max_steps = s.num_steps;
    }
    if (ns < 1) return fail(LMH_ERR_BAD_ARG, "no samples");
    HIPCHK(hipSetDevice(h->device));
    RefPlan p;
    const int rc = alloc_plan(p, ns, 2 * max_steps + 2, n);         // one segment stride for all robots
    if (rc != LMH_OK) return rc;
    DevBuf<LmhWalkSpec> d_specs;
    if (batch) {
        HIPCHK(d_specs.upload(W.data(), W.size()));
        lmh_launch_gen_walk_batch(d_specs.get(), n, p.n_seg, p.zx.get(), p.zy.get(), p.phase.get(), p.segs.get(), p.sos.get(), nullptr);
    } else lmh_launch_gen_walk(&W[0], p.zx.get(), p.zy.get(), p.phase.get(), p.segs.get(), p.sos.get(), nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    return commit_plan(h, std::move(p));
}

extern "C" int lmh_gen_walk(lmh_handle *h, double simulation_time, int num_steps, double time_per_step, double ds_time, double step_height,
                            double settle_time, int first_support, double foot_y)
{
    if (!h) return fail(LMH_ERR_BAD_ARG, "null handle");
    const lmh_walk_spec s = {time_per_step, ds_time, step_height, settle_time, foot_y, num_steps, first_support};
    return gen_walk(h, simulation_time, &s, 1, false);
}

extern "C" int lmh_gen_walk_batch(lmh_handle *h, double simulation_time, const lmh_walk_spec *specs, int n)
{
    if (!h) return fail(LMH_ERR_BAD_ARG, "null handle");
    if (!specs) return fail(LMH_ERR_BAD_ARG, "null spec array");
    if (n != h->B) return fail(LMH_ERR_BAD_ARG, "n must be n_instances");
    return gen_walk(h, simulation_time, specs, n, true);
}

static const char *jump_spec_error(double simulation_time, const lmh_jump_spec &s)
{
    if (!(s.stance_time >= 0.0) || !(s.flight_time >= 0.0) || !(simulation_time > 0.0)) return "times must be non-negative";
    return nullptr;
}

// lmh_gen_jump (batch = false: specs[0], today's single-plan launch) and lmh_gen_jump_batch
static int gen_jump(lmh_handle *h, double simulation_time, const lmh_jump_spec *specs, int n, bool batch)
{
    std::vector<LmhJumpSpec> J((size_t)n);
    for (int i = 0; i < n; i++) {
        if (const char *msg = jump_spec_error(simulation_time, specs[i])) return fail(LMH_ERR_BAD_ARG, batch ? robot_msg(i, msg) : msg);
        J[(size_t)i] = LmhJumpSpec{specs[i].stance_time, specs[i].flight_time};
    }
    const int ns = sample_count(h, simulation_time);
    if (ns < 1) return fail(LMH_ERR_BAD_ARG, "no samples");
    HIPCHK(hipSetDevice(h->device));
    RefPlan p;
    const int rc = alloc_plan(p, ns, 0, n);
    if (rc != LMH_OK) return rc;
    DevBuf<LmhJumpSpec> d_specs;
    if (batch) {
        HIPCHK(d_specs.upload(J.data(), J.size()));
        lmh_launch_gen_jump_batch(ns, h->mpc_dt, d_specs.get(), n, p.zx.get(), p.zy.get(), p.phase.get(), nullptr);
    } else lmh_launch_gen_jump(ns, h->mpc_dt, J[0].stance_time, J[0].flight_time, p.zx.get(), p.zy.get(), p.phase.get(), nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    return commit_plan(h, std::move(p));
}

extern "C" int lmh_gen_jump(lmh_handle *h, double simulation_time, double stance_time, double flight_time)
{
    if (!h) return fail(LMH_ERR_BAD_ARG, "null handle");
    const lmh_jump_spec s = {stance_time, flight_time};
    return gen_jump(h, simulation_time, &s, 1, false);
}

extern "C" int lmh_gen_jump_batch(lmh_handle *h, double simulation_time, const lmh_jump_spec *specs, int n)
{
    if (!h) return fail(LMH_ERR_BAD_ARG, "null handle");
    if (!specs) return fail(LMH_ERR_BAD_ARG, "null spec array");
    if (n != h->B) return fail(LMH_ERR_BAD_ARG, "n must be n_instances");
    return gen_jump(h, simulation_time, specs, n, true);
}

// ---------------------------------------------------------------------------- one plan per robot, uploaded / read back
extern "C" int lmh_set_plans(lmh_handle *h, const double *zx, const double *zy, const uint8_t *phase, int n_samples,
                             const double *segs, int n_seg, const uint16_t *sos, int n)
{
    if (!h) return fail(LMH_ERR_BAD_ARG, "null handle");
    if (!zx || !zy || n_samples < 1 || n_seg < 0) return fail(LMH_ERR_BAD_ARG, "bad argument");
    if (n != h->B) return fail(LMH_ERR_BAD_ARG, "n must be n_instances");
    if (n_seg > 0) {
        if (!segs || !sos) return fail(LMH_ERR_BAD_ARG, "null segment table");
        if (n_seg > 65536) return fail(LMH_ERR_BAD_ARG, "seg_of_sample is 16 bits wide: at most 65536 segments");
        const int bad = sos_out_of_range(sos, n_seg, n_samples, n);
        if (bad >= 0) return fail(LMH_ERR_BAD_ARG, robot_msg(bad, "seg_of_sample entry out of range"));
    }
    return upload_plan(h, zx, zy, phase, n_samples, segs, n_seg, sos, n);
}

extern "C" int lmh_plans_per_instance(const lmh_handle *h)
{
    if (!h) return fail(LMH_ERR_BAD_ARG, "null handle");
    return h->plan.per_robot() ? 1 : 0;
}

extern "C" int lmh_get_plan(lmh_handle *h, int inst, double *zx, double *zy, uint8_t *phase, double *segs, uint16_t *sos)
{
    if (!h) return fail(LMH_ERR_BAD_ARG, "null handle");
    if (inst < 0 || inst >= h->B) return fail(LMH_ERR_BAD_ARG, "instance out of range");
    HIPCHK(hipSetDevice(h->device));
    const RefPlan &r = h->plan;
    const size_t n = (size_t)r.n_samples;
    const size_t ro = (size_t)h->P.ref_stride * (size_t)inst, so = (size_t)LMH_SEG_STRIDE * (size_t)h->P.seg_stride * (size_t)inst;   // 0 on a shared plan
    if (zx) HIPCHK(hipMemcpy(zx, r.zx.get() + ro, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (zy) HIPCHK(hipMemcpy(zy, r.zy.get() + ro, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (phase) {
        if (r.phase.get()) HIPCHK(hipMemcpy(phase, r.phase.get() + ro, n, hipMemcpyDeviceToHost));
        else std::memset(phase, 0, n);
    }
    if (segs && r.n_seg > 0) HIPCHK(hipMemcpy(segs, r.segs.get() + so, sizeof(double) * LMH_SEG_STRIDE * (size_t)r.n_seg, hipMemcpyDeviceToHost));
    if (sos && r.n_seg > 0) HIPCHK(hipMemcpy(sos, r.sos.get() + ro, sizeof(uint16_t) * n, hipMemcpyDeviceToHost));
    return LMH_OK;
}

extern "C" int lmh_num_ref_samples(const lmh_handle *h) { return h ? h->plan.n_samples : 0; }
extern "C" int lmh_num_segments(const lmh_handle *h) { return h ? h->plan.n_seg : 0; }

extern "C" int lmh_get_refs(lmh_handle *h, double *zx, double *zy, uint8_t *phase, double *segs, uint16_t *sos)
{
    return lmh_get_plan(h, 0, zx, zy, phase, segs, sos);
}
