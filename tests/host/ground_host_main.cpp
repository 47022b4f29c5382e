// Stand-alone check of the ground table's host layer (lmh_set_ground and the calls that honour it; linearmpchumanoid_amd/csrc/lmh_capi.hip),
// built with the address and undefined-behaviour sanitizers by tests/test_host_ground_sanitized.py.  Without a handle no call may get as far
// as a check of a record, a read of its words, a device or a launch: whatever the records hold -- the flat record, a slope, a normal that is
// not a unit vector or points down, a NaN, no record at all --, the refusal is the null handle's, word for word, and no launcher is reached.
// (The record refusals themselves need a handle, that is a device: tests/test_gpu_ground.py holds them to their words.)
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
    static_assert(LMH_GROUND_STRIDE == 8 && LMH_GROUND_OFF_N_R == 0 && LMH_GROUND_OFF_H_R == 3 && LMH_GROUND_OFF_N_L == 4 && LMH_GROUND_OFF_H_L == 7,
                  "n_R(3) | h_R | n_L(3) | h_L");
    const double s5 = std::sin(5.0 * M_PI / 180.0), c5 = std::cos(5.0 * M_PI / 180.0);
    struct Row { const char *name; double rec[2 * LMH_GROUND_STRIDE]; };
    const Row rows[] = {
        {"the flat record", {0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0}},
        {"a slope and a ledge", {-s5, 0, c5, 0.003, -s5, 0, c5, -0.002, 0, 0, 1, 0.003, 0, 0, 1, -0.002}},
        {"a normal of length 2", {0, 0, 2, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0}},
        {"a normal that points down", {0, 0, -1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0}},
        {"a NaN word", {0, 0, 1, NAN, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0}},
        {"an infinite offset", {0, 0, 1, 0, 0, 0, 1, INFINITY, 0, 0, 1, 0, 0, 0, 1, 0}},
    };
    for (const Row &r : rows)
        for (int n_sets : {-1, 0, 1, 2, 3, 2147483647}) {
            const std::string what = std::string("lmh_set_ground, ") + r.name + ", n_sets = " + std::to_string(n_sets);
            expect_null_handle(lmh_set_ground(nullptr, r.rec, n_sets), what.c_str());
        }
    expect_null_handle(lmh_set_ground(nullptr, nullptr, 0), "lmh_set_ground, clearing");
    expect_null_handle(lmh_set_ground(nullptr, nullptr, 5), "lmh_set_ground, no records but a count");
    double rec[LMH_GROUND_STRIDE] = {7, 7, 7, 7, 7, 7, 7, 7};
    for (int inst : {-1, 0, 1, 2147483647}) expect_null_handle(lmh_get_ground(nullptr, inst, rec), "lmh_get_ground");
    expect_null_handle(lmh_get_ground(nullptr, 0, nullptr), "lmh_get_ground, null record");
    for (double w : rec)
        if (w != 7.0) { std::printf("FAILED: lmh_get_ground wrote into the record of a refused call\n"); g_failures++; break; }
    if (lmh_ground_per_instance(nullptr) != 0) { std::printf("FAILED: lmh_ground_per_instance(NULL) must be 0\n"); g_failures++; }

    double buf[8] = {0};
    int32_t ibuf[4] = {0};
    double *x = buf;                                               // never dereferenced: the calls are refused first
    int32_t *s = ibuf;
    // the calls that honour the table keep the null handle's refusal, with and without their pointers
    expect_null_handle(lmh_contact_wrench(nullptr, x, x, x, nullptr), "lmh_contact_wrench");
    expect_null_handle(lmh_contact_wrench(nullptr, nullptr, nullptr, nullptr, nullptr), "lmh_contact_wrench, null records");
    expect_null_handle(lmh_plant_derivative(nullptr, x, x, x, x, x, s, nullptr), "lmh_plant_derivative");
    expect_null_handle(lmh_plant_derivative(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "lmh_plant_derivative, null records");
    for (int n : {-1, 0, 1, 20}) expect_null_handle(lmh_plant_step(nullptr, x, x, n, s, nullptr), "lmh_plant_step");
    expect_null_handle(lmh_plant_step(nullptr, nullptr, nullptr, 1, nullptr, nullptr), "lmh_plant_step, null records");
    const lmh_zoh_opts every = {x, x, x, x, x, 2, 1, 1, 0}, none = {nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0};
    const lmh_zoh_io io = {x, x, x, 1, 0}, no_io = {nullptr, nullptr, nullptr, 0, 0};
    const int counts[][2] = {{6, 3}, {0, 3}, {6, 0}, {-1, 3}, {6, -1}};
    for (const auto &c : counts) {
        expect_null_handle(lmh_rollout_zoh(nullptr, x, x, s, x, x, c[0], c[1], nullptr), "lmh_rollout_zoh");
        expect_null_handle(lmh_rollout_zoh_ref(nullptr, x, x, s, x, x, x, c[0], c[1], nullptr), "lmh_rollout_zoh_ref");
        for (const lmh_zoh_opts *o : {&every, &none, (const lmh_zoh_opts *)nullptr}) {
            expect_null_handle(lmh_rollout_zoh_ex(nullptr, x, x, s, o, c[0], c[1], nullptr), "lmh_rollout_zoh_ex");
            for (const lmh_zoh_io *i : {&io, &no_io, (const lmh_zoh_io *)nullptr})
                expect_null_handle(lmh_rollout_zoh_io(nullptr, x, x, s, o, i, c[0], c[1], nullptr), "lmh_rollout_zoh_io");
            expect_null_handle(lmh_rollout_zoh_box(nullptr, x, x, s, o, x, 64, 1, x, c[0], c[1], nullptr), "lmh_rollout_zoh_box");
        }
    }
    if (g_failures) { std::printf("%d check(s) FAILED\n", g_failures); return 1; }
    std::printf("all ground host-layer checks held\n");
    return 0;
}
