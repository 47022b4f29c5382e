// Stand-alone check of lmh_rollout_zoh_ex's host layer (linearmpchumanoid_amd/csrc/lmh_capi.hip), built with the address and
// undefined-behaviour sanitizers by tests/test_host_zoh_ex_sanitized.py.  Without a handle no call may get as far as an argument check, a
// read of the options record's pointers' targets, a device or a launch: whatever the record holds -- nothing, every option, values outside
// their ranges, a trace buffer without a period --, and with no record at all, the refusal is the null handle's, word for word, and no
// launcher is reached.  (The argument refusals themselves need a handle, that is a device: tests/test_gpu_zoh_ex.py holds them to their words.)
// Exit status 0 = every check held; each failure is printed.
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
    static_assert(sizeof(lmh_zoh_opts) == 5 * sizeof(void *) + 4 * sizeof(int32_t), "five pointers, four int32: no hidden padding");
    static_assert(offsetof(lmh_zoh_opts, trace_every) == 5 * sizeof(void *) && offsetof(lmh_zoh_opts, reserved) == sizeof(lmh_zoh_opts) - sizeof(int32_t), "the record's layout");
    static_assert(LMH_TRACE_STRIDE == LMH_STATE_STRIDE + LMH_OUT_STRIDE + LMH_STATUS_STRIDE, "a sample is the three records");
    double buf[8] = {0};
    int32_t ibuf[4] = {0};
    double *x = buf;                                               // never dereferenced: the calls are refused first
    int32_t *s = ibuf;
    struct Row { const char *name; lmh_zoh_opts o; };
    const Row rows[] = {
        {"all zero", {nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 0}},
        {"every option", {x, x, x, x, x, 2, 1, 1, 0}},
        {"pushes alone", {nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 1, 0}},
        {"wrench_per_tick without a wrench", {nullptr, nullptr, nullptr, nullptr, nullptr, 0, 1, 0, 0}},
        {"wrench_per_tick = 2", {x, nullptr, nullptr, nullptr, nullptr, 0, 2, 0, 0}},
        {"pushes = -1", {nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, -1, 0}},
        {"reserved = 7", {nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, 7}},
        {"a trace buffer without a period", {nullptr, nullptr, nullptr, x, nullptr, 0, 0, 0, 0}},
        {"a period without a trace buffer", {nullptr, nullptr, nullptr, nullptr, nullptr, 3, 0, 0, 0}},
        {"trace_every < 0", {nullptr, nullptr, nullptr, x, nullptr, -1, 0, 0, 0}},
        {"metrics alone", {nullptr, nullptr, nullptr, nullptr, x, 0, 0, 0, 0}},
    };
    const int counts[][2] = {{6, 3}, {0, 3}, {6, 0}, {-1, 3}, {6, -1}, {2147483647, 2147483647}};
    for (const Row &r : rows)
        for (const auto &c : counts) {
            const std::string what = std::string("lmh_rollout_zoh_ex, ") + r.name + ", " + std::to_string(c[0]) + " x " + std::to_string(c[1]);
            expect_null_handle(lmh_rollout_zoh_ex(nullptr, x, x, s, &r.o, c[0], c[1], nullptr), what.c_str());
            expect_null_handle(lmh_rollout_zoh_ex(nullptr, nullptr, nullptr, nullptr, &r.o, c[0], c[1], nullptr), (what + ", null records").c_str());
        }
    expect_null_handle(lmh_rollout_zoh_ex(nullptr, x, x, s, nullptr, 6, 3, nullptr), "lmh_rollout_zoh_ex without a record");
    expect_null_handle(lmh_rollout_zoh_ex(nullptr, nullptr, nullptr, nullptr, nullptr, -1, -1, nullptr), "lmh_rollout_zoh_ex, everything wrong");
    expect_null_handle(lmh_rollout_zoh(nullptr, x, x, s, nullptr, nullptr, 3, 2, nullptr), "lmh_rollout_zoh");      // the calls that share zoh_body keep their refusal
    expect_null_handle(lmh_rollout_zoh_ref(nullptr, x, x, s, nullptr, nullptr, x, 3, 2, nullptr), "lmh_rollout_zoh_ref");
    if (g_failures) { std::printf("%d check(s) FAILED\n", g_failures); return 1; }
    std::printf("all zoh_ex host-layer checks held\n");
    return 0;
}
