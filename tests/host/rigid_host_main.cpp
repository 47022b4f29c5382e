// Stand-alone check of the rigid-contact plant's host layer (lmh_plant_derivative_rigid and lmh_plant_step_rigid;
// linearmpchumanoid_amd/csrc/lmh_capi.hip), built with the address and undefined-behaviour sanitizers by tests/test_host_rigid_sanitized.py.
// Without a handle no call may get as far as a check of kv or of a count, a read of a mode word, a device or a launch: whatever the
// arguments hold -- a negative kv, a NaN, an infinity, a negative count, no state, no pointer at all --, the refusal is the null handle's,
// word for word, nothing is written through a pointer and no launcher is reached.
// (The argument refusals themselves need a handle, that is a device: tests/test_gpu_rigid.py holds them to their words.)
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
    static_assert(LMH_FLAG_CONTACT_PULL == 256 && LMH_FLAG_CONTACT_SLIP == 512, "the two informational flags");
    static_assert((LMH_FLAG_CONTACT_PULL & (LMH_FLAG_QP_MAXITER | LMH_FLAG_NONFINITE | LMH_FLAG_ZMP_RANGE | LMH_FLAG_NOT_SPD | LMH_FLAG_QP_FP64_ROUTE | LMH_FLAG_UNFINISHED |
                                            LMH_FLAG_BOX_EMPTY | LMH_FLAG_TAU_LIMIT | LMH_FLAG_CONTACT_SLIP)) == 0, "a bit of its own");
    static_assert(LMH_PHASE_DOUBLE == 0 && LMH_PHASE_RIGHT == 1 && LMH_PHASE_LEFT == 2 && LMH_PHASE_FLIGHT == 3, "the low two bits of a mode word");
    double buf[16];
    int32_t ibuf[4], mode[4] = {0, 1, 2, 3};
    for (double &w : buf) w = 7.0;
    for (int32_t &w : ibuf) w = 7;
    double *x = buf;                                               // never dereferenced: the calls are refused first
    int32_t *s = ibuf;
    const double kvs[] = {0.0, 50.0, -0.0, -1.0, -1e-300, NAN, INFINITY, -INFINITY, 1.7976931348623157e308};
    for (double kv : kvs) {
        const std::string k = ", kv = " + std::to_string(kv);
        expect_null_handle(lmh_plant_derivative_rigid(nullptr, x, x, x, mode, kv, x, x, s, nullptr), ("lmh_plant_derivative_rigid" + k).c_str());
        expect_null_handle(lmh_plant_derivative_rigid(nullptr, x, x, nullptr, nullptr, kv, x, nullptr, nullptr, nullptr), ("lmh_plant_derivative_rigid, optional pointers left out" + k).c_str());
        expect_null_handle(lmh_plant_derivative_rigid(nullptr, nullptr, x, x, mode, kv, x, x, s, nullptr), ("lmh_plant_derivative_rigid, null q" + k).c_str());
        expect_null_handle(lmh_plant_derivative_rigid(nullptr, x, nullptr, x, mode, kv, x, x, s, nullptr), ("lmh_plant_derivative_rigid, null v" + k).c_str());
        expect_null_handle(lmh_plant_derivative_rigid(nullptr, x, x, x, mode, kv, nullptr, x, s, nullptr), ("lmh_plant_derivative_rigid, null xdot" + k).c_str());
        expect_null_handle(lmh_plant_derivative_rigid(nullptr, nullptr, nullptr, nullptr, nullptr, kv, nullptr, nullptr, nullptr, nullptr), ("lmh_plant_derivative_rigid, no pointer" + k).c_str());
        for (int n : {-2147483647 - 1, -1, 0, 1, 20, 2147483647}) {
            const std::string kn = k + ", n_substeps = " + std::to_string(n);
            expect_null_handle(lmh_plant_step_rigid(nullptr, x, x, mode, kv, n, x, s, nullptr), ("lmh_plant_step_rigid" + kn).c_str());
            expect_null_handle(lmh_plant_step_rigid(nullptr, x, nullptr, nullptr, kv, n, nullptr, nullptr, nullptr), ("lmh_plant_step_rigid, optional pointers left out" + kn).c_str());
            expect_null_handle(lmh_plant_step_rigid(nullptr, nullptr, x, mode, kv, n, x, s, nullptr), ("lmh_plant_step_rigid, null state" + kn).c_str());
        }
    }
    for (double w : buf)
        if (w != 7.0) { std::printf("FAILED: a refused call wrote through a pointer\n"); g_failures++; break; }
    for (int32_t w : ibuf)
        if (w != 7) { std::printf("FAILED: a refused call wrote into the flags\n"); g_failures++; break; }
    if (mode[0] != 0 || mode[1] != 1 || mode[2] != 2 || mode[3] != 3) { std::printf("FAILED: a refused call wrote into the modes\n"); g_failures++; }
    if (g_failures) { std::printf("%d check(s) FAILED\n", g_failures); return 1; }
    std::printf("all rigid host-layer checks held\n");
    return 0;
}
