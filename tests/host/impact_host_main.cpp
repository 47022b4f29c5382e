// Stand-alone check of the plastic impact's host layer (lmh_plant_impact_rigid and lmh_rollout_zoh_rigid_impact;
// linearmpchumanoid_amd/csrc/lmh_capi.hip), built with the address and undefined-behaviour sanitizers by tests/test_host_impact_sanitized.py.
// Without a handle no call may get as far as a check of a record, a read of a mode word, a device or a launch: whatever the records and the
// arguments hold -- an enable outside its values, a non-zero reserved, no d_mode_prev, a rigid record that is off or broken, no pointer at
// all --, the refusal is the null handle's, word for word, nothing is written through a pointer and no launcher is reached.
// (The records' own refusals need a handle, that is a device: tests/test_gpu_impact.py holds them to their words.)
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
    static_assert(LMH_FLAG_IMPULSE_PULL == 1024 && LMH_FLAG_IMPULSE_SLIP == 2048, "the two informational flags");
    static_assert(((LMH_FLAG_IMPULSE_PULL | LMH_FLAG_IMPULSE_SLIP) & (15 | LMH_FLAG_QP_FP64_ROUTE | LMH_FLAG_UNFINISHED | LMH_FLAG_BOX_EMPTY | LMH_FLAG_TAU_LIMIT |
                                                                      LMH_FLAG_CONTACT_PULL | LMH_FLAG_CONTACT_SLIP)) == 0, "bits of their own, outside FIRST_FLAG's mask");
    static_assert(sizeof(lmh_zoh_impact) == 2 * sizeof(void *) + 2 * sizeof(int32_t), "two pointers, two words: no padding");
    static_assert(sizeof(lmh_zoh_rigid) == 2 * sizeof(void *) + sizeof(double) + 2 * sizeof(int32_t), "lmh_zoh_rigid is as it was");
    double buf[16];
    int32_t ibuf[4], mode[4] = {0, 1, 2, 3}, prev[4] = {3, 6, 9, 12};
    for (double &w : buf) w = 7.0;
    for (int32_t &w : ibuf) w = 7;
    double *x = buf;                                               // never dereferenced: the calls are refused first
    int32_t *s = ibuf;
    // ---- lmh_plant_impact_rigid: every pattern of present and absent pointers
    for (int bits = 0; bits < 64; bits++) {
        const double *q = (bits & 1) ? x : nullptr, *v = (bits & 2) ? x : nullptr;
        const int32_t *m = (bits & 4) ? mode : nullptr;
        double *vp = (bits & 8) ? x : nullptr, *imp = (bits & 16) ? x : nullptr;
        int32_t *fl = (bits & 32) ? s : nullptr;
        expect_null_handle(lmh_plant_impact_rigid(nullptr, q, v, m, vp, imp, fl, nullptr), "lmh_plant_impact_rigid, pointers " + std::to_string(bits));
    }
    // ---- lmh_rollout_zoh_rigid_impact: a grid of record contents and argument sets
    const int32_t enables[] = {0, 1, 2, -1, 2147483647, -2147483647 - 1};
    const int32_t reserveds[] = {0, 1, -1};
    const int32_t sources[] = {0, LMH_RIGID_FIXED, LMH_RIGID_PER_TICK, LMH_RIGID_PLAN, 4, -1};
    const double kvs[] = {0.0, 50.0, -1.0, NAN, INFINITY};
    const lmh_zoh_opts opts_on = {x, x, x, x, x, 2, 1, 1, 0}, opts_bad = {nullptr, nullptr, nullptr, x, nullptr, -3, 2, 2, 5};
    const lmh_zoh_io io_on = {x, x, x, 1, 0}, io_bad = {nullptr, nullptr, nullptr, 2, 9};
    const lmh_zoh_opts *optss[] = {nullptr, &opts_on, &opts_bad};
    const lmh_zoh_io *ios[] = {nullptr, &io_on, &io_bad};
    for (int32_t enable : enables)
        for (int32_t reserved : reserveds)
            for (int pp = 0; pp < 2; pp++)
                for (int ip = 0; ip < 2; ip++) {
                    const lmh_zoh_impact im = {pp ? prev : nullptr, ip ? x : nullptr, enable, reserved};
                    const std::string what = "enable = " + std::to_string(enable) + ", reserved = " + std::to_string(reserved) + (pp ? ", d_mode_prev" : ", no d_mode_prev") +
                                             (ip ? ", d_impulse" : ", no d_impulse");
                    for (int32_t source : sources)
                        for (double kv : kvs) {
                            const lmh_zoh_rigid rg = {(source == LMH_RIGID_PLAN) ? nullptr : mode, x, kv, source, 0};
                            const std::string w2 = what + ", source = " + std::to_string(source) + ", kv = " + std::to_string(kv);
                            for (int o = 0; o < 3; o++)
                                for (int i = 0; i < 3; i++)
                                    expect_null_handle(lmh_rollout_zoh_rigid_impact(nullptr, x, x, s, optss[o], ios[i], &rg, &im, 6, 3, nullptr), w2 + ", records " + std::to_string(o) + std::to_string(i));
                        }
                    expect_null_handle(lmh_rollout_zoh_rigid_impact(nullptr, x, x, s, &opts_on, &io_on, nullptr, &im, 6, 3, nullptr), what + ", no rigid record");
                    expect_null_handle(lmh_rollout_zoh_rigid_impact(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &im, 6, 3, nullptr), what + ", no pointer");
                    for (int n : {-2147483647 - 1, -1, 0, 2147483647}) {
                        const lmh_zoh_rigid rg = {mode, x, 50.0, LMH_RIGID_PER_TICK, 0};
                        expect_null_handle(lmh_rollout_zoh_rigid_impact(nullptr, x, x, s, &opts_on, &io_on, &rg, &im, n, 3, nullptr), what + ", n_ticks = " + std::to_string(n));
                        expect_null_handle(lmh_rollout_zoh_rigid_impact(nullptr, x, x, s, &opts_on, &io_on, &rg, &im, 6, n, nullptr), what + ", n_substeps = " + std::to_string(n));
                    }
                }
    {
        const lmh_zoh_rigid rg = {mode, x, 50.0, LMH_RIGID_PER_TICK, 0};
        expect_null_handle(lmh_rollout_zoh_rigid_impact(nullptr, x, x, s, nullptr, nullptr, &rg, nullptr, 6, 3, nullptr), "no impact record");
        expect_null_handle(lmh_rollout_zoh_rigid_impact(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr), "nothing at all");
    }
    for (double w : buf)
        if (w != 7.0) { std::printf("FAILED: a refused call wrote through a pointer\n"); g_failures++; break; }
    for (int32_t w : ibuf)
        if (w != 7) { std::printf("FAILED: a refused call wrote into the status or the flags\n"); g_failures++; break; }
    if (mode[0] != 0 || mode[1] != 1 || mode[2] != 2 || mode[3] != 3) { std::printf("FAILED: a refused call wrote into the modes\n"); g_failures++; }
    if (prev[0] != 3 || prev[1] != 6 || prev[2] != 9 || prev[3] != 12) { std::printf("FAILED: a refused call wrote into d_mode_prev\n"); g_failures++; }
    if (g_failures) { std::printf("%d check(s) FAILED\n", g_failures); return 1; }
    std::printf("all impact host-layer checks held (%d calls)\n", g_calls);
    return 0;
}
