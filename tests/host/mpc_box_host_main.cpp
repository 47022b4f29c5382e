// Stand-alone check of the box-constrained MPC entry points of the C ABI's host layer (lmh_mpc_box_preview / _step / _rollout in
// linearmpchumanoid_amd/csrc/lmh_capi.hip), built with the address and undefined-behaviour sanitizers by tests/test_host_mpc_box_sanitized.py.
// Without a handle no call may get as far as an argument check, a device or a launch: whatever the other arguments are -- good, null, a
// negative count, a wrong n_samples or n_sets --, the refusal is the null handle's, word for word, and no launcher is reached.  (The
// argument refusals themselves need a handle, that is a device: tests/test_gpu_mpc_box.py holds them to their words.)
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
    static_assert(LMH_MPC_BOX_STRIDE == LMH_MPC_PREVIEW_STRIDE + 2 * 66, "box record");
    static_assert(LMH_MPC_BOX_MAX_ROUNDS >= 2 * (LMH_MAX_HORIZON + 1), "round cap");
    static_assert(LMH_FLAG_BOX_EMPTY == 64 && LMH_BOX_LO_X == 0 && LMH_BOX_HI_X == 1 && LMH_BOX_LO_Y == 2 && LMH_BOX_HI_Y == 3, "box defines");
    double buf[8] = {0};
    double *x = buf;                                               // never dereferenced: the calls are refused first
    struct Args { const char *name; double *lip, *box, *out; int n_samples, n_sets, n_ticks; };
    const Args rows[] = {
        {"good arguments", x, x, x, 100, 1, 3},      {"null lip", nullptr, x, x, 100, 1, 3},   {"null box", x, nullptr, x, 100, 1, 3},
        {"null output", x, x, nullptr, 100, 1, 3},   {"n_samples = 0", x, x, x, 0, 1, 3},      {"n_samples < 0", x, x, x, -5, 1, 3},
        {"n_sets = 0", x, x, x, 100, 0, 3},          {"n_sets < 0", x, x, x, 100, -1, 3},      {"n_ticks < 0", x, x, x, 100, 1, -1},
        {"n_ticks = 0", x, x, x, 100, 1, 0},         {"everything wrong", nullptr, nullptr, nullptr, -1, -1, -1},
    };
    for (const Args &a : rows) {
        expect_null_handle(lmh_mpc_box_preview(nullptr, a.lip, a.box, a.n_samples, a.n_sets, a.out, nullptr), (std::string("lmh_mpc_box_preview, ") + a.name).c_str());
        expect_null_handle(lmh_mpc_box_step(nullptr, a.lip, a.box, a.n_samples, a.n_sets, a.out, nullptr), (std::string("lmh_mpc_box_step, ") + a.name).c_str());
        expect_null_handle(lmh_mpc_box_rollout(nullptr, a.lip, a.box, a.n_samples, a.n_sets, a.n_ticks, a.out, nullptr), (std::string("lmh_mpc_box_rollout, ") + a.name).c_str());
    }
    expect_null_handle(lmh_mpc_preview(nullptr, x, x, nullptr), "lmh_mpc_preview");       // the calls whose launchers grew keep their refusal
    expect_null_handle(lmh_mpc_step(nullptr, x, x, nullptr), "lmh_mpc_step");
    expect_null_handle(lmh_mpc_rollout(nullptr, x, 1, x, nullptr), "lmh_mpc_rollout");
    if (g_failures) { std::printf("%d check(s) FAILED\n", g_failures); return 1; }
    std::printf("all box host-layer checks held\n");
    return 0;
}
