// Stand-alone check of the caller-supplied CoM reference entry points of the C ABI's host layer (lmh_eval_ref, lmh_rollout_zoh_ref in
// linearmpchumanoid_amd/csrc/lmh_capi.hip), built with the address and undefined-behaviour sanitizers by tests/test_host_ref_sanitized.py.
// Without a handle no call may get as far as an argument check, a device or a launch: whatever the other arguments are -- good, a null
// d_ref, null required pointers, negative counts --, the refusal is the null handle's, word for word, and no launcher is reached.  (The
// argument refusals themselves need a handle, that is a device: tests/test_gpu_ref.py holds them to their words.)
// Exit status 0 = every check held; each failure is printed.
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
    static_assert(LMH_MPC_STRIDE == 16 && LMH_MPC_OFF_XREF == 0 && LMH_MPC_OFF_YREF == 3, "the record lmh_eval_ref reads");
    static_assert(LMH_MPC_OFF_XREF + 3 <= LMH_MPC_OFF_ZMP && LMH_MPC_OFF_YREF + 3 <= LMH_MPC_OFF_ZMP, "xRef | yRef are words [0, 6)");
    double buf[8] = {0};
    int32_t ibuf[4] = {0};
    double *x = buf;                                               // never dereferenced: the calls are refused first
    int32_t *s = ibuf;
    struct Args { const char *name; double *state, *ref, *out; int32_t *status; int n_ticks, n_substeps; };
    const Args rows[] = {
        {"good arguments", x, x, x, s, 3, 2},        {"null d_ref", x, nullptr, x, s, 3, 2},    {"null state", nullptr, x, x, s, 3, 2},
        {"null out", x, x, nullptr, s, 3, 2},        {"null status", x, x, x, nullptr, 3, 2},   {"n_ticks < 0", x, x, x, s, -1, 2},
        {"n_substeps < 0", x, x, x, s, 3, -1},       {"n_ticks = 0", x, x, x, s, 0, 2},         {"n_substeps = 0", x, x, x, s, 3, 0},
        {"everything wrong", nullptr, nullptr, nullptr, nullptr, -1, -1},
    };
    for (const Args &a : rows) {
        expect_null_handle(lmh_eval_ref(nullptr, a.state, a.ref, a.out, a.status, nullptr), (std::string("lmh_eval_ref, ") + a.name).c_str());
        expect_null_handle(lmh_rollout_zoh_ref(nullptr, a.state, a.out, a.status, nullptr, nullptr, a.ref, a.n_ticks, a.n_substeps, nullptr),
                           (std::string("lmh_rollout_zoh_ref, ") + a.name).c_str());
        expect_null_handle(lmh_rollout_zoh_ref(nullptr, a.state, a.out, a.status, x, x, a.ref, a.n_ticks, a.n_substeps, nullptr),
                           (std::string("lmh_rollout_zoh_ref with wrench and log, ") + a.name).c_str());
    }
    expect_null_handle(lmh_eval(nullptr, x, x, s, nullptr), "lmh_eval");                     // the calls whose launchers grew keep their refusal
    expect_null_handle(lmh_eval_debug(nullptr, x, x, s, x, nullptr), "lmh_eval_debug");
    expect_null_handle(lmh_rollout_zoh(nullptr, x, x, s, nullptr, nullptr, 3, 2, nullptr), "lmh_rollout_zoh");
    if (g_failures) { std::printf("%d check(s) FAILED\n", g_failures); return 1; }
    std::printf("all reference host-layer checks held\n");
    return 0;
}
