// Stand-alone check of the joint servo's host layer (lmh_set_servo, lmh_get_servo, lmh_servo_per_instance, lmh_plant_step_servo and
// lmh_rollout_zoh_servo; linearmpchumanoid_amd/csrc/lmh_capi.hip), built with the address and undefined-behaviour sanitizers by
// tests/test_host_servo_sanitized.py.  Without a handle no call may get as far as a check of a record, a read of its words, a device or a
// launch: whatever the records and the servo's options hold -- gains, a negative one, a NaN, no record at all, every mode and a mode that
// does not exist --, the refusal is the null handle's, word for word, and no launcher is reached.
// (The record and option refusals themselves need a handle, that is a device: tests/test_gpu_servo.py holds them to their words.)
// Exit status 0 = every check held; each failure is printed.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <string>
#include "lmh.h"

// every kernel launcher of csrc/lmh_launch.h is a stub here (a missing one does not link): nothing in this program may get as far as a launch
#define LAUNCH_STUB(name) extern "C" void name(void) { std::fprintf(stderr, #name " was reached\n"); std::abort(); }
LAUNCH_STUB(lmh_launch_eval) LAUNCH_STUB(lmh_launch_rollout) LAUNCH_STUB(lmh_launch_model) LAUNCH_STUB(lmh_launch_com)
LAUNCH_STUB(lmh_launch_ik) LAUNCH_STUB(lmh_launch_gen_walk) LAUNCH_STUB(lmh_launch_gen_jump) LAUNCH_STUB(lmh_launch_gen_walk_batch)
LAUNCH_STUB(lmh_launch_gen_jump_batch) LAUNCH_STUB(lmh_launch_terms) LAUNCH_STUB(lmh_launch_plant) LAUNCH_STUB(lmh_launch_params_expand)
LAUNCH_STUB(lmh_launch_summary) LAUNCH_STUB(lmh_launch_rollout_zoh) LAUNCH_STUB(lmh_launch_metrics_reset) LAUNCH_STUB(lmh_launch_ik_batch)
LAUNCH_STUB(lmh_launch_mpc_step) LAUNCH_STUB(lmh_launch_mpc_rollout) LAUNCH_STUB(lmh_launch_mpc_preview)

static int g_failures = 0;
static void expect_null_handle(int rc, const char *what)
{
    if (rc != LMH_ERR_BAD_ARG || std::string("null handle") != lmh_last_error()) {
        std::printf("FAILED: %s: want -2 \"null handle\", got %d \"%s\"\n", what, rc, lmh_last_error());
        g_failures++;
    }
}

int main()
{
    static_assert(LMH_SERVO_STRIDE == 48 && LMH_SERVO_OFF_KP == 0 && LMH_SERVO_OFF_KD == 24 && LMH_SETPOINT_STRIDE == 48, "KP[24] | KD[24]; Q_DES[24] | V_DES[24]");
    static_assert(LMH_SERVO_INTEGRATE == 1 && LMH_SERVO_CALLER == 2, "0 off | integrate | caller");
    static_assert(sizeof(lmh_zoh_servo) == 16 && offsetof(lmh_zoh_servo, mode) == 8 && offsetof(lmh_zoh_servo, reserved) == 12, "pointer | mode | reserved");
    struct Row { const char *name; double word; };
    const Row rows[] = {{"gains", 3.0}, {"zero gains", 0.0}, {"a negative gain", -1.0}, {"a NaN gain", NAN}, {"an infinite gain", INFINITY}};
    for (const Row &r : rows) {
        double rec[3 * LMH_SERVO_STRIDE];
        for (double &w : rec) w = 3.0;
        rec[LMH_SERVO_STRIDE + LMH_SERVO_OFF_KD + 5] = r.word;
        for (int n_sets : {-1, 0, 1, 2, 3, 2147483647}) {
            const std::string what = std::string("lmh_set_servo, ") + r.name + ", n_sets = " + std::to_string(n_sets);
            expect_null_handle(lmh_set_servo(nullptr, rec, n_sets), what.c_str());
        }
    }
    expect_null_handle(lmh_set_servo(nullptr, nullptr, 0), "lmh_set_servo, clearing");
    expect_null_handle(lmh_set_servo(nullptr, nullptr, 5), "lmh_set_servo, no records but a count");
    double rec[LMH_SERVO_STRIDE];
    for (double &w : rec) w = 7.0;
    for (int inst : {-1, 0, 1, 2147483647}) expect_null_handle(lmh_get_servo(nullptr, inst, rec), "lmh_get_servo");
    expect_null_handle(lmh_get_servo(nullptr, 0, nullptr), "lmh_get_servo, null record");
    for (double w : rec)
        if (w != 7.0) { std::printf("FAILED: lmh_get_servo wrote into the record of a refused call\n"); g_failures++; break; }
    if (lmh_servo_per_instance(nullptr) != 0) { std::printf("FAILED: lmh_servo_per_instance(NULL) must be 0\n"); g_failures++; }

    double buf[8] = {0};
    int32_t ibuf[4] = {0};
    double *x = buf;                                               // never dereferenced: the calls are refused first
    int32_t *s = ibuf;
    for (int n : {-1, 0, 1, 20}) {
        expect_null_handle(lmh_plant_step_servo(nullptr, x, x, x, n, s, nullptr), "lmh_plant_step_servo");
        expect_null_handle(lmh_plant_step_servo(nullptr, x, x, nullptr, n, s, nullptr), "lmh_plant_step_servo, null setpoint");
    }
    expect_null_handle(lmh_plant_step_servo(nullptr, nullptr, nullptr, nullptr, 1, nullptr, nullptr), "lmh_plant_step_servo, null records");
    const lmh_zoh_opts every = {x, x, x, x, x, 2, 1, 1, 0}, none = {nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0};
    const lmh_zoh_io io = {x, x, x, 1, 0}, no_io = {nullptr, nullptr, nullptr, 0, 0};
    const lmh_zoh_servo servos[] = {{nullptr, 0, 0}, {nullptr, LMH_SERVO_INTEGRATE, 0}, {x, LMH_SERVO_CALLER, 0}, {nullptr, LMH_SERVO_CALLER, 0}, {x, LMH_SERVO_INTEGRATE, 0},
                                    {x, 0, 0}, {nullptr, 3, 0}, {nullptr, -1, 0}, {nullptr, LMH_SERVO_INTEGRATE, 1}};
    const int counts[][2] = {{6, 3}, {0, 3}, {6, 0}, {-1, 3}, {6, -1}};
    for (const auto &c : counts)
        for (const lmh_zoh_opts *o : {&every, &none, (const lmh_zoh_opts *)nullptr})
            for (const lmh_zoh_io *i : {&io, &no_io, (const lmh_zoh_io *)nullptr}) {
                for (const lmh_zoh_servo &sv : servos) expect_null_handle(lmh_rollout_zoh_servo(nullptr, x, x, s, o, i, &sv, c[0], c[1], nullptr), "lmh_rollout_zoh_servo");
                expect_null_handle(lmh_rollout_zoh_servo(nullptr, x, x, s, o, i, nullptr, c[0], c[1], nullptr), "lmh_rollout_zoh_servo, no servo record");
                expect_null_handle(lmh_rollout_zoh_io(nullptr, x, x, s, o, i, c[0], c[1], nullptr), "lmh_rollout_zoh_io");
            }
    expect_null_handle(lmh_rollout_zoh_servo(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 6, 3, nullptr), "lmh_rollout_zoh_servo, null records");
    if (g_failures) { std::printf("%d check(s) FAILED\n", g_failures); return 1; }
    std::printf("all servo host-layer checks held\n");
    return 0;
}
