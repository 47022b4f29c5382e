// Stand-alone check of lmh_rollout_zoh_rigid's host layer (linearmpchumanoid_amd/csrc/lmh_capi.hip), built with the address and
// undefined-behaviour sanitizers by tests/test_host_zoh_rigid_sanitized.py.  Without a handle no call may get as far as a check of a record,
// a read of a mode word, a device or a launch: whatever the records hold -- a NaN kv, a source outside its values, a non-zero reserved, a
// mode pointer where none belongs, no pointer at all --, the refusal is the null handle's, word for word, nothing is written through a
// pointer and no launcher is reached.
// (The record's own refusals need a handle, that is a device: tests/test_gpu_zoh_rigid.py holds them to their words.)
// Exit status 0 = every check held; each failure is printed.
#include <cmath>
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

static int g_failures = 0, g_calls = 0;
static void expect_null_handle(int rc, const std::string &what)
{
    g_calls++;
    if (rc != LMH_ERR_BAD_ARG || std::string("null handle") != lmh_last_error()) {
        std::printf("FAILED: %s: want -2 \"null handle\", got %d \"%s\"\n", what.c_str(), rc, lmh_last_error());
        g_failures++;
    }
}

int main()
{
    static_assert(LMH_RIGID_FIXED == 1 && LMH_RIGID_PER_TICK == 2 && LMH_RIGID_PLAN == 3, "the three sources; 0 is off");
    static_assert(sizeof(lmh_zoh_rigid) == 2 * sizeof(void *) + sizeof(double) + 2 * sizeof(int32_t), "two pointers, kv, two words: no padding");
    double buf[16];
    int32_t ibuf[4], mode[4] = {0, 1, 2, 3};
    for (double &w : buf) w = 7.0;
    for (int32_t &w : ibuf) w = 7;
    double *x = buf;                                               // never dereferenced: the calls are refused first
    int32_t *s = ibuf;
    const double kvs[] = {0.0, 50.0, -0.0, -1.0, NAN, INFINITY, -INFINITY, 1.7976931348623157e308};
    const int32_t sources[] = {0, LMH_RIGID_FIXED, LMH_RIGID_PER_TICK, LMH_RIGID_PLAN, 4, -1, 2147483647, -2147483647 - 1};
    const int32_t reserveds[] = {0, 1, -1};
    const lmh_zoh_opts opts_on = {x, x, x, x, x, 2, 1, 1, 0}, opts_bad = {nullptr, nullptr, nullptr, x, nullptr, -3, 2, 2, 5};
    const lmh_zoh_io io_on = {x, x, x, 1, 0}, io_bad = {nullptr, nullptr, nullptr, 2, 9};
    const lmh_zoh_opts *optss[] = {nullptr, &opts_on, &opts_bad};
    const lmh_zoh_io *ios[] = {nullptr, &io_on, &io_bad};
    for (double kv : kvs)
        for (int32_t source : sources)
            for (int32_t reserved : reserveds)
                for (int mp = 0; mp < 2; mp++)
                    for (int lp = 0; lp < 2; lp++) {
                        const lmh_zoh_rigid rg = {mp ? mode : nullptr, lp ? x : nullptr, kv, source, reserved};
                        const std::string what = "kv = " + std::to_string(kv) + ", source = " + std::to_string(source) + ", reserved = " + std::to_string(reserved) +
                                                 (mp ? ", d_mode" : ", no d_mode") + (lp ? ", d_lambda" : ", no d_lambda");
                        for (int o = 0; o < 3; o++)
                            for (int i = 0; i < 3; i++)
                                expect_null_handle(lmh_rollout_zoh_rigid(nullptr, x, x, s, optss[o], ios[i], &rg, 6, 3, nullptr), what + ", records " + std::to_string(o) + std::to_string(i));
                        expect_null_handle(lmh_rollout_zoh_rigid(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &rg, 6, 3, nullptr), what + ", no pointer");
                        for (int n : {-2147483647 - 1, -1, 0, 2147483647}) {
                            expect_null_handle(lmh_rollout_zoh_rigid(nullptr, x, x, s, &opts_on, &io_on, &rg, n, 3, nullptr), what + ", n_ticks = " + std::to_string(n));
                            expect_null_handle(lmh_rollout_zoh_rigid(nullptr, x, x, s, &opts_on, &io_on, &rg, 6, n, nullptr), what + ", n_substeps = " + std::to_string(n));
                        }
                    }
    expect_null_handle(lmh_rollout_zoh_rigid(nullptr, x, x, s, nullptr, nullptr, nullptr, 6, 3, nullptr), "no record");
    expect_null_handle(lmh_rollout_zoh_rigid(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr), "nothing at all");
    for (double w : buf)
        if (w != 7.0) { std::printf("FAILED: a refused call wrote through a pointer\n"); g_failures++; break; }
    for (int32_t w : ibuf)
        if (w != 7) { std::printf("FAILED: a refused call wrote into the status\n"); g_failures++; break; }
    if (mode[0] != 0 || mode[1] != 1 || mode[2] != 2 || mode[3] != 3) { std::printf("FAILED: a refused call wrote into the modes\n"); g_failures++; }
    if (g_failures) { std::printf("%d check(s) FAILED\n", g_failures); return 1; }
    std::printf("all zoh-rigid host-layer checks held (%d calls)\n", g_calls);
    return 0;
}
