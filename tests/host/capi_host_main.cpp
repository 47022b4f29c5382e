// Stand-alone check of the C ABI's host layer (linearmpchumanoid_amd/csrc/lmh_capi.hip), built with the address and undefined-behaviour
// sanitizers by tests/test_host_sanitized.py.  It calls nothing that reaches a HIP runtime function, so it runs the same with or without
// a device: refusals of lmh_create that come before the device is looked for, null-handle refusals, and the record files.
// Usage: capi_host_main <scratch directory>.  Exit status 0 = every check held; each failure is printed.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <string>
#include <vector>
#include "lmh.h"

// every kernel launcher of csrc/lmh_launch.h is a stub here (a missing one does not link): nothing in this program may get as far as a launch
#define LAUNCH_STUB(name) extern "C" void name(void) { std::fprintf(stderr, #name " was reached\n"); std::abort(); }
LAUNCH_STUB(lmh_launch_eval) LAUNCH_STUB(lmh_launch_rollout) LAUNCH_STUB(lmh_launch_model) LAUNCH_STUB(lmh_launch_com)
LAUNCH_STUB(lmh_launch_ik) LAUNCH_STUB(lmh_launch_gen_walk) LAUNCH_STUB(lmh_launch_gen_jump) LAUNCH_STUB(lmh_launch_gen_walk_batch)
LAUNCH_STUB(lmh_launch_gen_jump_batch) LAUNCH_STUB(lmh_launch_terms) LAUNCH_STUB(lmh_launch_plant) LAUNCH_STUB(lmh_launch_params_expand)
LAUNCH_STUB(lmh_launch_summary) LAUNCH_STUB(lmh_launch_rollout_zoh) LAUNCH_STUB(lmh_launch_metrics_reset) LAUNCH_STUB(lmh_launch_ik_batch)
LAUNCH_STUB(lmh_launch_mpc_step) LAUNCH_STUB(lmh_launch_mpc_rollout) LAUNCH_STUB(lmh_launch_mpc_preview)

static int g_failures = 0;
static void expect(bool ok, const std::string &what)
{
    if (!ok) { std::printf("FAILED: %s (last error: \"%s\")\n", what.c_str(), lmh_last_error()); g_failures++; }
}
static void expect_refusal(int rc, const std::string &text, const std::string &what)
{
    expect(rc == LMH_ERR_BAD_ARG && text == lmh_last_error(), what + ": want -2 \"" + text + "\", got " + std::to_string(rc));
}

// ---------------------------------------------------------------------------- a. lmh_create's refusals, text and order
static const double kInf = std::numeric_limits<double>::infinity(), kNan = std::numeric_limits<double>::quiet_NaN();
struct BadConfig { const char *name; void (*spoil)(lmh_config &); const char *text; };
static const BadConfig kBadConfigs[] = {
    // one row per rule (every field of a rule that names several)
    {"dt = 0", [](lmh_config &c) { c.dt = 0; }, "lmh_create: dt and time_horizon must be positive"},
    {"dt = NaN", [](lmh_config &c) { c.dt = kNan; }, "lmh_create: dt and time_horizon must be positive"},
    {"time_horizon < 0", [](lmh_config &c) { c.time_horizon = -0.5; }, "lmh_create: dt and time_horizon must be positive"},
    {"mpc_dt < 0", [](lmh_config &c) { c.mpc_dt = -1; }, "lmh_create: mpc_dt must be >= 0 (0 = dt)"},
    {"mpc_dt = inf", [](lmh_config &c) { c.mpc_dt = kInf; }, "lmh_create: mpc_dt must be >= 0 (0 = dt)"},
    {"z_com = 0", [](lmh_config &c) { c.z_com = 0; }, "lmh_create: z_com and gravity must be positive"},
    {"gravity < 0", [](lmh_config &c) { c.gravity = -9.81; }, "lmh_create: z_com and gravity must be positive"},
    {"alpha = 0", [](lmh_config &c) { c.alpha = 0; }, "lmh_create: alpha and beta must be positive"},
    {"beta = NaN", [](lmh_config &c) { c.beta = kNan; }, "lmh_create: alpha and beta must be positive"},
    {"mu = 0", [](lmh_config &c) { c.mu = 0; }, "lmh_create: mu must be positive"},
    {"eps_coeff = 0", [](lmh_config &c) { c.eps_coeff = 0; }, "lmh_create: eps_coeff must be positive"},
    {"w_com_lin = 0", [](lmh_config &c) { c.w_com_lin = 0; }, "lmh_create: weights w_com_lin, w_base_pos, w_base_ang, w_joints, w_force, w_foot must be positive"},
    {"w_base_pos = 0", [](lmh_config &c) { c.w_base_pos = 0; }, "lmh_create: weights w_com_lin, w_base_pos, w_base_ang, w_joints, w_force, w_foot must be positive"},
    {"w_base_ang < 0", [](lmh_config &c) { c.w_base_ang = -1; }, "lmh_create: weights w_com_lin, w_base_pos, w_base_ang, w_joints, w_force, w_foot must be positive"},
    {"w_joints = NaN", [](lmh_config &c) { c.w_joints = kNan; }, "lmh_create: weights w_com_lin, w_base_pos, w_base_ang, w_joints, w_force, w_foot must be positive"},
    {"w_force = 0", [](lmh_config &c) { c.w_force = 0; }, "lmh_create: weights w_com_lin, w_base_pos, w_base_ang, w_joints, w_force, w_foot must be positive"},
    {"w_foot = 0", [](lmh_config &c) { c.w_foot = 0; }, "lmh_create: weights w_com_lin, w_base_pos, w_base_ang, w_joints, w_force, w_foot must be positive"},
    {"w_com_ang < 0", [](lmh_config &c) { c.w_com_ang = -1; }, "lmh_create: w_com_ang must be >= 0"},
    {"kp_joints = inf", [](lmh_config &c) { c.kp_joints = kInf; }, "lmh_create: PD gains must be finite"},
    {"kd_joints = NaN", [](lmh_config &c) { c.kd_joints = kNan; }, "lmh_create: PD gains must be finite"},
    {"kp_mom = -inf", [](lmh_config &c) { c.kp_mom = -kInf; }, "lmh_create: PD gains must be finite"},
    {"kd_mom = NaN", [](lmh_config &c) { c.kd_mom = kNan; }, "lmh_create: PD gains must be finite"},
    {"kp_feet = inf", [](lmh_config &c) { c.kp_feet = kInf; }, "lmh_create: PD gains must be finite"},
    {"kd_feet = NaN", [](lmh_config &c) { c.kd_feet = kNan; }, "lmh_create: PD gains must be finite"},
    {"max_qp_iters = 0", [](lmh_config &c) { c.max_qp_iters = 0; }, "lmh_create: max_qp_iters must be >= 1"},
    {"plant = 2", [](lmh_config &c) { c.plant = 2; }, "lmh_create: plant must be 0 or 1"},
    {"plant = -1", [](lmh_config &c) { c.plant = -1; }, "lmh_create: plant must be 0 or 1"},
    {"plant, contact_k = 0", [](lmh_config &c) { c.plant = 1; c.contact_k = 0; }, "lmh_create: contact_k must be positive, contact_d / contact_dt / contact_mu non-negative"},
    {"plant, contact_d < 0", [](lmh_config &c) { c.plant = 1; c.contact_d = -1; }, "lmh_create: contact_k must be positive, contact_d / contact_dt / contact_mu non-negative"},
    {"plant, contact_dt = NaN", [](lmh_config &c) { c.plant = 1; c.contact_dt = kNan; }, "lmh_create: contact_k must be positive, contact_d / contact_dt / contact_mu non-negative"},
    {"plant, contact_mu < 0", [](lmh_config &c) { c.plant = 1; c.contact_mu = -0.1; }, "lmh_create: contact_k must be positive, contact_d / contact_dt / contact_mu non-negative"},
    {"precision = 3", [](lmh_config &c) { c.precision = 3; }, "lmh_create: precision must be LMH_PRECISION_FP64, LMH_PRECISION_MIXED or LMH_PRECISION_FP32"},
    {"N = 700", [](lmh_config &c) { c.dt = 1e-3; c.time_horizon = 0.7; }, "horizon N = time_horizon/mpc_dt must be in [1, 64]"},
    {"N = 70 by mpc_dt", [](lmh_config &c) { c.dt = 1e-3; c.time_horizon = 0.7; c.mpc_dt = 1e-2; }, "horizon N = time_horizon/mpc_dt must be in [1, 64]"},
    {"N = 0", [](lmh_config &c) { c.time_horizon = 0.005; }, "horizon N = time_horizon/mpc_dt must be in [1, 64]"},
    // two rules broken at once: the one stated first is the one reported
    {"dt, mu", [](lmh_config &c) { c.dt = 0; c.mu = 0; }, "lmh_create: dt and time_horizon must be positive"},
    {"mpc_dt, z_com", [](lmh_config &c) { c.mpc_dt = -1; c.z_com = 0; }, "lmh_create: mpc_dt must be >= 0 (0 = dt)"},
    {"gravity, alpha", [](lmh_config &c) { c.gravity = 0; c.alpha = 0; }, "lmh_create: z_com and gravity must be positive"},
    {"beta, contact_k", [](lmh_config &c) { c.beta = 0; c.plant = 1; c.contact_k = 0; }, "lmh_create: alpha and beta must be positive"},
    {"mu, eps_coeff", [](lmh_config &c) { c.mu = -1; c.eps_coeff = 0; }, "lmh_create: mu must be positive"},
    {"mu, contact_mu", [](lmh_config &c) { c.mu = 0; c.plant = 1; c.contact_mu = -1; }, "lmh_create: mu must be positive"},
    {"eps_coeff, w_joints", [](lmh_config &c) { c.eps_coeff = 0; c.w_joints = 0; }, "lmh_create: eps_coeff must be positive"},
    {"w_foot, w_com_ang", [](lmh_config &c) { c.w_foot = 0; c.w_com_ang = -1; }, "lmh_create: weights w_com_lin, w_base_pos, w_base_ang, w_joints, w_force, w_foot must be positive"},
    {"w_com_ang, kp_joints", [](lmh_config &c) { c.w_com_ang = kNan; c.kp_joints = kInf; }, "lmh_create: w_com_ang must be >= 0"},
    {"kd_feet, max_qp_iters", [](lmh_config &c) { c.kd_feet = kNan; c.max_qp_iters = 0; }, "lmh_create: PD gains must be finite"},
    {"kd_feet, contact_k", [](lmh_config &c) { c.kd_feet = kNan; c.plant = 1; c.contact_k = 0; }, "lmh_create: PD gains must be finite"},
    {"max_qp_iters, contact_k", [](lmh_config &c) { c.max_qp_iters = 0; c.plant = 1; c.contact_k = 0; }, "lmh_create: max_qp_iters must be >= 1"},
    {"plant = 2, contact_k", [](lmh_config &c) { c.plant = 2; c.contact_k = 0; }, "lmh_create: plant must be 0 or 1"},
    {"contact_d, precision", [](lmh_config &c) { c.plant = 1; c.contact_d = -1; c.precision = -1; }, "lmh_create: contact_k must be positive, contact_d / contact_dt / contact_mu non-negative"},
    {"precision, N = 700", [](lmh_config &c) { c.precision = 7; c.dt = 1e-3; c.time_horizon = 0.7; }, "lmh_create: precision must be LMH_PRECISION_FP64, LMH_PRECISION_MIXED or LMH_PRECISION_FP32"},
};

static void check_create_refusals()
{
    lmh_config c;
    lmh_config_default(&c);
    expect(c.dt == 0.01 && c.time_horizon == 0.5 && c.mpc_dt == 0.0 && c.plant == 0 && c.precision == LMH_PRECISION_FP64 && c.max_qp_iters == 64, "defaults");
    int sentinel = 0;
    lmh_handle *const untouched = reinterpret_cast<lmh_handle *>(&sentinel);
    lmh_handle *h = untouched;
    expect_refusal(lmh_create(nullptr, 1, 0, &h), "lmh_create: bad argument", "null config");
    expect_refusal(lmh_create(&c, 1, 0, nullptr), "lmh_create: bad argument", "null out pointer");
    expect_refusal(lmh_create(&c, 0, 0, &h), "lmh_create: bad argument", "no instances");
    expect(h == untouched, "a call refused for its arguments leaves *out alone");
    for (const BadConfig &b : kBadConfigs) {
        lmh_config_default(&c);
        b.spoil(c);
        h = untouched;
        expect_refusal(lmh_create(&c, 3, 0, &h), b.text, std::string("config with ") + b.name);
        expect(h == nullptr, std::string("no handle for ") + b.name);
    }
}

// ---------------------------------------------------------------------------- null handles
static void check_null_handles()
{
    double x[LMH_STATE_STRIDE] = {0};
    int32_t n3[3] = {1, 1, 1}, i4[4] = {0};
    uint8_t ph[1] = {0};
    uint16_t so[1] = {0};
    lmh_walk_spec ws = {0.5, 0.1, 0.02, 0.3, 0.05, 4, LMH_PHASE_RIGHT};
    lmh_jump_spec js = {0.4, 0.15};
    expect(lmh_destroy(nullptr) == LMH_OK, "lmh_destroy(NULL)");
    expect(lmh_num_instances(nullptr) == 0 && lmh_horizon(nullptr) == 0 && lmh_num_pushes(nullptr) == 0 && lmh_pushes_per_instance(nullptr) == 0 &&
           lmh_params_per_instance(nullptr) == 0 && lmh_num_ref_samples(nullptr) == 0 && lmh_num_segments(nullptr) == 0, "counts of a null handle are 0");
#define TEXT(text, call) expect_refusal((call), text, #call)
    TEXT("null handle", lmh_set_model(nullptr, nullptr, 1));
    TEXT("bad argument", lmh_get_mass(nullptr, x));
    TEXT("bad argument", lmh_set_refs(nullptr, x, x, ph, 1));
    TEXT("null handle", lmh_set_refs_stance(nullptr, 5.0, 2));
    TEXT("bad argument", lmh_set_foot_coeffs(nullptr, x, n3, x, n3));
    TEXT("bad argument", lmh_set_segments(nullptr, x, 1, so, 1));
    TEXT("null handle", lmh_gen_walk(nullptr, 5.0, 4, 0.5, 0.1, 0.02, 0.3, LMH_PHASE_RIGHT, 0.05));
    TEXT("null handle", lmh_gen_jump(nullptr, 5.0, 0.4, 0.15));
    TEXT("null handle", lmh_gen_walk_batch(nullptr, 5.0, &ws, 1));
    TEXT("null handle", lmh_gen_jump_batch(nullptr, 5.0, &js, 1));
    TEXT("null handle", lmh_set_plans(nullptr, x, x, ph, 1, nullptr, 0, nullptr, 1));
    TEXT("null handle", lmh_plans_per_instance(nullptr));
    TEXT("null handle", lmh_get_refs(nullptr, x, x, ph, nullptr, nullptr));
    TEXT("null handle", lmh_get_plan(nullptr, 0, x, x, ph, nullptr, nullptr));
    TEXT("null handle", lmh_set_xscale(nullptr, x, 1));
    TEXT("n must be 1 or n_instances", lmh_set_zcom(nullptr, x, 1));
    TEXT("bad argument", lmh_get_mpc_gain(nullptr, x));
    TEXT("null handle", lmh_set_pushes(nullptr, x, 1, 1));
    TEXT("null handle", lmh_get_pushes(nullptr, 0, x));
    TEXT("null handle", lmh_set_params(nullptr, x, 1));
    TEXT("bad argument", lmh_get_params(nullptr, 0, x));
    TEXT("null handle", lmh_eval(nullptr, x, x, i4, nullptr));
    TEXT("null handle", lmh_ik(nullptr, x, x, x, x, i4, nullptr));
    TEXT("null handle", lmh_robot_com(nullptr, x, x, nullptr));
    TEXT("null handle", lmh_terms(nullptr, x, x, x, nullptr));
    TEXT("null handle", lmh_plant_step(nullptr, x, x, 1, i4, nullptr));
    TEXT("bad argument", lmh_make_summary(nullptr, x, x, i4, x, nullptr));
    TEXT("null handle", lmh_eval_debug(nullptr, x, x, i4, x, nullptr));
    TEXT("null handle", lmh_rollout(nullptr, x, x, i4, nullptr, 1, nullptr));
    TEXT("null handle", lmh_rollout_trace(nullptr, x, x, i4, nullptr, 1, x, 1, nullptr));
    TEXT("null handle", lmh_inverse_dynamics(nullptr, x, x, x, x, x, nullptr));
    TEXT("null handle", lmh_forward_dynamics(nullptr, x, x, x, x, x, i4, nullptr));
    TEXT("null handle", lmh_contact_wrench(nullptr, x, x, x, nullptr));
    TEXT("null handle", lmh_plant_derivative(nullptr, x, x, x, x, x, i4, nullptr));
    TEXT("null handle", lmh_eval_host(nullptr, x, x, 0.0, x, x, x, i4));
    TEXT("null handle", lmh_robot_com_host(nullptr, x, x));
    TEXT("bad argument", lmh_last_out_host(nullptr, x));
    TEXT("null handle", lmh_ik_host(nullptr, x, x, x, x, x, i4));
    TEXT("null handle", lmh_terms_host(nullptr, x, x, x));
    TEXT("bad argument", lmh_set_prev_velocity_host(nullptr, x));
    TEXT("null handle", lmh_synchronize(nullptr, nullptr));
    TEXT("null handle", lmh_rollout_zoh(nullptr, x, x, i4, nullptr, nullptr, 1, 1, nullptr));
    TEXT("null handle", lmh_rollout_metrics(nullptr, x, x, i4, nullptr, 1, x, nullptr));
    TEXT("null handle", lmh_metrics_reset(nullptr, x, 0.1, 0.5, nullptr));
    TEXT("null handle", lmh_ik_batch(nullptr, x, x, 1, x + 30, i4, x, nullptr));
    TEXT("null handle", lmh_mpc_step(nullptr, x, x, nullptr));
    TEXT("null handle", lmh_mpc_rollout(nullptr, x, 1, x, nullptr));
    TEXT("null handle", lmh_mpc_preview(nullptr, x, x, nullptr));
    TEXT("null handle", lmh_mpc_step_host(nullptr, x, x));
#undef TEXT
    expect(lmh_trace_samples(10, 3) == 3 && lmh_trace_samples(10, 0) == 0 && lmh_trace_samples(0, 3) == 0 && lmh_trace_samples(2, 3) == 0 &&
           lmh_trace_samples(10, -1) == 0, "lmh_trace_samples");
    double raw[LMH_NFRAMES * LMH_LINK_STRIDE];
    lmh_nominal_links(raw);
    bool massless = true;
    for (int f : {7, 14, 27}) for (int e = 0; e < LMH_LINK_STRIDE; e++) massless = massless && raw[f * LMH_LINK_STRIDE + e] == 0.0;
    expect(massless && raw[0] > 0.0, "nominal links: frames 7, 14, 27 are massless, the torso is not");
}

// ---------------------------------------------------------------------------- b, c. record files
static std::vector<unsigned char> slurp(const std::string &path)
{
    std::vector<unsigned char> b;
    if (FILE *f = std::fopen(path.c_str(), "rb")) {
        for (int ch; (ch = std::fgetc(f)) != EOF;) b.push_back((unsigned char)ch);
        std::fclose(f);
    }
    return b;
}
static void spit(const std::string &path, const std::vector<unsigned char> &b, size_t n)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(b.data(), 1, n, f) != n) { std::perror(path.c_str()); std::exit(2); }
    std::fclose(f);
}

// One kind of record file through the common signature: a summary has no tick count and no t0
struct Kind {
    const char *name; uint32_t width; uint64_t n_ticks, n_inst;
    std::function<int(const char *, const double *, uint64_t, uint64_t, double, double)> write;
    std::function<int(const char *, double *, uint64_t, uint64_t *, uint64_t *, double *, double *)> read;
};

static void check_record_kind(const std::string &dir, const Kind &k, const Kind &other)
{
    const std::string path = dir + "/" + k.name + ".bin", what = std::string(k.name) + ": ";
    const uint64_t count = k.width * k.n_inst * (k.n_ticks ? k.n_ticks : 1);
    std::vector<double> data(count), back(count + 1, -7.0);
    for (uint64_t i = 0; i < count; i++) data[i] = 0.25 * (double)i - 3.0;
    data[count - 1] = kNan;                                          // a payload is raw bits
    expect(k.write(path.c_str(), data.data(), k.n_ticks, k.n_inst, 0.004, 1.5) == LMH_OK, what + "write");
    expect(slurp(path).size() == 64 + 8 * count, what + "64-byte header + raw f64 payload");
    // header only, then the payload, into a buffer of exactly the capacity given
    uint64_t nt = 99, ni = 99;
    double dt = -1, t0 = -1;
    expect(k.read(path.c_str(), nullptr, 0, &nt, &ni, &dt, &t0) == LMH_OK && nt == k.n_ticks && ni == k.n_inst && dt == 0.004 && (t0 == 1.5 || !k.n_ticks), what + "header-only read");
    nt = ni = 99;
    expect(k.read(path.c_str(), back.data(), count, &nt, &ni, &dt, &t0) == LMH_OK && nt == k.n_ticks && ni == k.n_inst, what + "full read");
    expect(std::memcmp(back.data(), data.data(), 8 * count) == 0 && back[count] == -7.0, what + "payload round trip, nothing written past it");
    expect(k.read(path.c_str(), back.data(), count, nullptr, nullptr, nullptr, nullptr) == LMH_OK, what + "every out-pointer is optional");
    // refusals; the out-pointers keep what they held
    nt = ni = 99;
    expect_refusal(k.read(path.c_str(), back.data(), count - 1, &nt, &ni, &dt, &t0), "buffer too small", what + "capacity one short");
    expect(nt == 99 && ni == 99, what + "a refused read leaves the out-pointers alone");
    expect_refusal(other.read(path.c_str(), nullptr, 0, &nt, &ni, &dt, &t0), "bad magic", what + "read as a " + other.name);
    expect_refusal(k.read(nullptr, nullptr, 0, &nt, &ni, &dt, &t0), "bad argument", what + "null path");
    expect_refusal(k.write(nullptr, data.data(), k.n_ticks, k.n_inst, 0.004, 1.5), "bad argument", what + "write, null path");
    expect_refusal(k.write(path.c_str(), nullptr, k.n_ticks, k.n_inst, 0.004, 1.5), "bad argument", what + "write, null data");
    const std::string missing = dir + "/no_such_dir/" + k.name + ".bin";
    expect_refusal(k.read(missing.c_str(), nullptr, 0, &nt, &ni, &dt, &t0), "cannot open " + missing, what + "missing file");
    expect_refusal(k.write(missing.c_str(), data.data(), k.n_ticks, k.n_inst, 0.004, 1.5), "cannot open " + missing, what + "write into a missing directory");
    const std::vector<unsigned char> good = slurp(path);
    const std::string bad = dir + "/" + k.name + "_bad.bin";
    for (size_t n : {(size_t)0, (size_t)7, (size_t)63}) {
        spit(bad, good, n);
        expect_refusal(k.read(bad.c_str(), back.data(), count, &nt, &ni, &dt, &t0), "truncated header", what + std::to_string(n) + " bytes of header");
    }
    for (size_t n : {(size_t)64, good.size() - 8, good.size() - 1}) {
        spit(bad, good, n);
        expect_refusal(k.read(bad.c_str(), back.data(), count, &nt, &ni, &dt, &t0), "payload size does not match the header", what + "payload cut to " + std::to_string(n - 64) + " bytes");
    }
    std::vector<unsigned char> b = good;
    b.insert(b.end(), 8, 0);
    spit(bad, b, b.size());
    expect_refusal(k.read(bad.c_str(), back.data(), count, &nt, &ni, &dt, &t0), "payload size does not match the header", what + "one double too many");
    const struct { size_t offset; unsigned char value; const char *text, *name; } patches[] = {
        {0, 'X', "bad magic", "magic"}, {7, 1, "bad magic", "magic terminator"},
        {8, 2, "unsupported version / dtype / width", "version"}, {12, 0, "unsupported version / dtype / width", "dtype"},
        {32, (unsigned char)(k.width + 1), "unsupported version / dtype / width", "width"},
        {16, (unsigned char)(k.n_inst + 1), "payload size does not match the header", "n_instances"},
    };
    for (const auto &p : patches) {
        b = good;
        b[p.offset] = p.value;
        spit(bad, b, b.size());
        expect_refusal(k.read(bad.c_str(), back.data(), count, &nt, &ni, &dt, &t0), p.text, what + "patched " + p.name);
    }
    expect(nt == 99 && ni == 99 && back[count] == -7.0, what + "no refusal wrote anything");
}

static void check_records(const std::string &dir)
{
    const Kind sum = {"summary", LMH_SUMMARY_WIDTH, 0, 5,
                      [](const char *p, const double *d, uint64_t, uint64_t n, double dt, double) { return lmh_write_summary(p, d, n, dt); },
                      [](const char *p, double *d, uint64_t cap, uint64_t *nt, uint64_t *n, double *dt, double *) {
                          const int rc = lmh_read_summary(p, d, cap, n, dt);
                          if (rc == LMH_OK && nt) *nt = 0;
                          return rc;
                      }};
    const Kind log = {"log", 36, 3, 2, lmh_write_log, lmh_read_log};
    const Kind trace = {"trace", LMH_TRACE_STRIDE, 2, 3, lmh_write_trace, lmh_read_trace};
    check_record_kind(dir, sum, log);
    check_record_kind(dir, log, trace);
    check_record_kind(dir, trace, sum);
    // a log or a trace of zero ticks is refused when written; as a file it is a header with no payload and reads back as such
    const double one = 1.0;
    const std::string path = dir + "/empty.bin";
    std::remove(path.c_str());
    expect_refusal(lmh_write_log(path.c_str(), &one, 0, 2, 0.001, 0.0), "a log holds at least one tick", "log of zero ticks");
    expect_refusal(lmh_write_trace(path.c_str(), &one, 0, 2, 0.001, 0.0), "a trace holds at least one sample", "trace of zero samples");
    expect(slurp(path).empty(), "a refused write creates no file");
    expect(lmh_write_summary(path.c_str(), &one, 0, 0.001) == LMH_OK && slurp(path).size() == 64, "a summary of zero robots is a bare header");
    uint64_t n = 99;
    expect(lmh_read_summary(path.c_str(), nullptr, 0, &n, nullptr) == LMH_OK && n == 0, "... and reads back");
}

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s <scratch directory>\n", argv[0]); return 2; }
    check_create_refusals();
    check_null_handles();
    check_records(argv[1]);
    std::printf(g_failures ? "%d check(s) failed\n" : "all host-layer checks held\n", g_failures);
    return g_failures ? 1 : 0;
}
