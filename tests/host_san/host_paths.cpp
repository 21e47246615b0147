// tests/host_san/host_paths.cpp — the host-only paths of libmetagym_hip, walked by a program with its own main so that they can
// run under AddressSanitizer and UBSan (metagym_amd/build.py: build_host_checked links this file with every csrc/*.hip, host side
// sanitized). TEST INFRASTRUCTURE. Nothing here needs a device: every call is refused on the host before a launch, or is one of
// the pure-host helpers. The expected codes are the contract of include/metagym_hip.h; a mismatch is printed and the exit status
// is 1. Device pointers are the address of a small host buffer: the library must never read through them on these paths, and
// ASan would say so if it did past the buffer.
//
// Covered: every entry point of the header. For each launching one: every required pointer NULL in turn (members of descriptors,
// states and carries included), every size and configuration refusal the header documents, one thing wrong per call. The
// pure-host helpers are run for real: the quadrotor config, plan, fold and task rows, every *_param_count over its whole
// accepted range and one past it, mg_liftsim_layout over every accepted (floors, elevators), the maze view tables, the
// walker topology at each MG_WALKER_MAX_* and one past. No call here is complete: a complete one would reach the device.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "metagym_hip.h"

static int g_checks = 0, g_failed = 0;

static void expect(long got, long want, const char *what, int line) {
    ++g_checks;
    if (got != want) {
        ++g_failed;
        std::printf("MISMATCH line %d: %s -> %ld, expected %ld (%s)\n", line, what, got, want, mg_last_error());
    }
}
#define EXPECT(call, want) expect((long)(call), (long)(want), #call, __LINE__)
#define EXPECT_TRUE(cond) expect((long)((cond) ? 1 : 0), 1L, #cond, __LINE__)

alignas(16) static unsigned char g_fake[256];       // stands for device memory that must not be touched
template <class T> static T *fake() { return reinterpret_cast<T *>(g_fake); }

// ---- quadrotor -----------------------------------------------------------------------------------------------------------------

static mg_quadrotor_state fake_state(bool episode) {
    mg_quadrotor_state st;
    st.pos = fake<float>(); st.vel = fake<double>(); st.omega = fake<double>(); st.propw = fake<float>(); st.rot = fake<float>();
    st.ct = fake<int32_t>(); st.episode = episode ? fake<uint32_t>() : nullptr;
    return st;
}

static void quadrotor() {
    EXPECT(mg_abi_version(), MG_ABI_VERSION);
    EXPECT_TRUE(std::strcmp(mg_target_arch(), "gfx950") == 0);
    EXPECT(mg_quadrotor_default_config(nullptr), MG_ERR_NULL_POINTER);
    mg_quadrotor_config cfg;
    EXPECT(mg_quadrotor_default_config(&cfg), MG_OK);
    EXPECT_TRUE(cfg.precision == 0.001 && cfg.dt == 0.01 && cfg.nt == 1000 && cfg.map_d == nullptr);
    mg_quadrotor_state st = fake_state(false), none;
    std::memset(&none, 0, sizeof(none));
    // the step: every required pointer NULL in turn (reward, reward64 and failed are optional)
    EXPECT(mg_quadrotor_step(nullptr, 4, &st, fake<float>(), fake<float>(), nullptr, nullptr, fake<uint8_t>(), nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_step(&cfg, 4, nullptr, fake<float>(), fake<float>(), nullptr, nullptr, fake<uint8_t>(), nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_step(&cfg, 4, &none, fake<float>(), fake<float>(), nullptr, nullptr, fake<uint8_t>(), nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_step(&cfg, 4, &st, nullptr, fake<float>(), nullptr, nullptr, fake<uint8_t>(), nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_step(&cfg, 4, &st, fake<float>(), nullptr, nullptr, nullptr, fake<uint8_t>(), nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_step(&cfg, 4, &st, fake<float>(), fake<float>(), nullptr, nullptr, nullptr, nullptr, nullptr), MG_ERR_NULL_POINTER);
    // plans: used before they are made, made from every incomplete argument list, made for real (host only), folded
    mg_quadrotor_plan plan;
    std::memset(&plan, 0, sizeof(plan));
    EXPECT(mg_quadrotor_plan_step(&plan, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), MG_ERR_BAD_CONFIG);
    EXPECT(mg_quadrotor_plan_step(nullptr, 1, fake<float>(), fake<float>(), nullptr, nullptr, fake<uint8_t>(), nullptr, nullptr), MG_ERR_NULL_POINTER);
    mg_quadrotor_fold fold;
    EXPECT(mg_quadrotor_plan_fold(&plan, &fold), MG_ERR_BAD_CONFIG);
    EXPECT(mg_quadrotor_plan_fold(nullptr, &fold), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_plan_init(nullptr, &cfg, nullptr, 4, &st), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_plan_init(&plan, nullptr, nullptr, 4, &st), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_plan_init(&plan, &cfg, nullptr, 4, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_plan_init(&plan, &cfg, nullptr, 4, &none), MG_ERR_NULL_POINTER);
    for (int k = 0; k < 6; ++k) {                       // each state array NULL in turn
        mg_quadrotor_state s = st;
        void **field[6] = {(void **)&s.pos, (void **)&s.vel, (void **)&s.omega, (void **)&s.propw, (void **)&s.rot, (void **)&s.ct};
        *field[k] = nullptr;
        EXPECT(mg_quadrotor_plan_init(&plan, &cfg, nullptr, 4, &s), MG_ERR_NULL_POINTER);
    }
    EXPECT(mg_quadrotor_plan_init(&plan, &cfg, nullptr, 0, &st), MG_ERR_BAD_SIZE);
    EXPECT(mg_quadrotor_plan_init(&plan, &cfg, nullptr, -3, &st), MG_ERR_BAD_SIZE);
    mg_quadrotor_autoreset ar;
    std::memset(&ar, 0, sizeof(ar));
    ar.init_velocity_noisy = 2.0; ar.init_angular_velocity_noisy = 5.0;
    EXPECT(mg_quadrotor_plan_init(&plan, &cfg, &ar, 4, &st), MG_ERR_NULL_POINTER);          // the fused reset needs state->episode
    mg_quadrotor_state ste = fake_state(true);
    EXPECT(mg_quadrotor_plan_init(&plan, &cfg, &ar, 4, &ste), MG_OK);
    EXPECT(mg_quadrotor_plan_fold(&plan, &fold), MG_OK);
    EXPECT_TRUE(fold.one_wave_form >= 0 && fold.one_wave_form <= 2);
    EXPECT(mg_quadrotor_plan_fold(&plan, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_plan_step(&plan, 0, fake<float>(), fake<float>(), nullptr, nullptr, fake<uint8_t>(), nullptr, nullptr), MG_ERR_BAD_SIZE);
    EXPECT(mg_quadrotor_plan_step(&plan, 1, nullptr, fake<float>(), nullptr, nullptr, fake<uint8_t>(), nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_plan_step(&plan, 1, fake<float>(), nullptr, nullptr, nullptr, fake<uint8_t>(), nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_plan_step(&plan, 1, fake<float>(), fake<float>(), nullptr, nullptr, nullptr, nullptr, nullptr), MG_ERR_NULL_POINTER);
    // every threshold the reference accepts folds (tests/test_quadrotor_edges.py: SPECIAL), with and without the fused reset
    const double inf = INFINITY, nan = NAN;
    const double ranges[] = {-1.0, -0.0, 0.0, 1e-30, 3e38, inf, 1e39, -inf, nan}, rates[] = {-1.0, 0.0, inf, nan, 1.0, 1.5};
    for (double r : ranges) {
        mg_quadrotor_config c = cfg;
        c.fail_range = r;
        EXPECT(mg_quadrotor_plan_init(&plan, &c, nullptr, 4, &st), MG_OK);
        EXPECT(mg_quadrotor_plan_init(&plan, &c, &ar, 4, &ste), MG_OK);
        EXPECT(mg_quadrotor_plan_fold(&plan, &fold), MG_OK);
    }
    for (double v : rates) {
        mg_quadrotor_config c = cfg;
        c.fail_velocity = v;
        EXPECT(mg_quadrotor_plan_init(&plan, &c, &ar, 4, &ste), MG_OK);
        c = cfg;
        c.fail_w = v;
        EXPECT(mg_quadrotor_plan_init(&plan, &c, &ar, 4, &ste), MG_OK);
        EXPECT(mg_quadrotor_plan_fold(&plan, &fold), MG_OK);
    }
    {                                                    // precision > dt (quadrotorsim.py:299-300), and below the documented 1e-8
        mg_quadrotor_config c = cfg;
        c.precision = 1.0;
        EXPECT(mg_quadrotor_plan_init(&plan, &c, nullptr, 4, &st), MG_ERR_BAD_CONFIG);
        c.precision = 1e-9;
        EXPECT(mg_quadrotor_plan_init(&plan, &c, nullptr, 4, &st), MG_ERR_BAD_CONFIG);
        c.precision = nan;
        EXPECT(mg_quadrotor_plan_init(&plan, &c, nullptr, 4, &st), MG_ERR_BAD_CONFIG);
    }
    // task rows
    const int32_t row_bytes = mg_quadrotor_tasks_row_bytes();
    EXPECT_TRUE(row_bytes > 0 && row_bytes % 16 == 0);
    std::vector<unsigned char> row((size_t)row_bytes);          // exactly a row: a fold that writes past it is ASan's to find
    EXPECT(mg_quadrotor_tasks_fold(nullptr, &ar, row.data()), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_tasks_fold(&cfg, &ar, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_tasks_fold(&cfg, nullptr, row.data()), MG_OK);
    EXPECT(mg_quadrotor_tasks_fold(&cfg, &ar, row.data()), MG_OK);
    mg_quadrotor_task_fold tf;
    EXPECT(mg_quadrotor_tasks_describe(nullptr, &tf), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_tasks_describe(row.data(), nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_tasks_describe(row.data(), &tf), MG_OK);
    EXPECT_TRUE(tf.times == 10 && tf.simple == 1 && tf.precision == 0.001 && tf.dt == 0.01 && tf.init_velocity_noisy == 2.0 &&
                tf.init_angular_velocity_noisy == 5.0 && tf.half_dt2 == 0.5 * 0.001 * 0.001);
    {
        mg_quadrotor_config c = cfg;
        c.precision = 1.0;
        EXPECT(mg_quadrotor_tasks_fold(&c, &ar, row.data()), MG_ERR_BAD_CONFIG);
        c = cfg;
        c.inertia[1] = c.inertia[3] = 0.0004f;             // an off-diagonal inertia term: not the stock structure
        EXPECT(mg_quadrotor_tasks_fold(&c, &ar, row.data()), MG_OK);
        EXPECT(mg_quadrotor_tasks_describe(row.data(), &tf), MG_OK);
        EXPECT_TRUE(tf.simple == 0);
    }
}

// every other launching entry point of the family: each required pointer NULL in turn, each size and configuration refusal
static void quadrotor_launches() {
    mg_quadrotor_config cfg;
    EXPECT(mg_quadrotor_default_config(&cfg), MG_OK);
    mg_quadrotor_state st = fake_state(false), ste = fake_state(true), none;
    std::memset(&none, 0, sizeof(none));
    mg_quadrotor_autoreset ar;
    std::memset(&ar, 0, sizeof(ar));
    float *f = fake<float>();
    uint8_t *u = fake<uint8_t>();
    mg_quadrotor_config bad = cfg;
    bad.precision = 1.0;                                // precision > dt
    EXPECT(mg_selftest_philox(nullptr, fake<uint32_t>(), 4, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_selftest_philox(fake<uint32_t>(), nullptr, 4, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_selftest_philox(fake<uint32_t>(), fake<uint32_t>(), 0, nullptr), MG_ERR_BAD_SIZE);
    // reset
    EXPECT(mg_quadrotor_reset(nullptr, 4, &st, nullptr, nullptr, nullptr, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_reset(&cfg, 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_reset(&cfg, 4, &none, nullptr, nullptr, nullptr, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_reset(&cfg, 0, &st, nullptr, nullptr, nullptr, nullptr, nullptr), MG_ERR_BAD_SIZE);
    EXPECT(mg_quadrotor_reset(&bad, 4, &st, nullptr, nullptr, nullptr, nullptr, nullptr), MG_ERR_BAD_CONFIG);
    // the velocity-control trajectory
    EXPECT(mg_quadrotor_velocity_targets(nullptr, 8, f, f, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_velocity_targets(&cfg, 8, nullptr, f, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_velocity_targets(&cfg, 8, f, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_velocity_targets(&cfg, 0, f, f, nullptr), MG_ERR_BAD_SIZE);
    EXPECT(mg_quadrotor_velocity_targets(&bad, 8, f, f, nullptr), MG_ERR_BAD_CONFIG);
    // rollout and the fused auto-reset
    EXPECT(mg_quadrotor_rollout(nullptr, 4, 2, &st, f, f, nullptr, nullptr, u, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_rollout(&cfg, 4, 2, nullptr, f, f, nullptr, nullptr, u, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_rollout(&cfg, 4, 2, &none, f, f, nullptr, nullptr, u, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_rollout(&cfg, 4, 2, &st, nullptr, f, nullptr, nullptr, u, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_rollout(&cfg, 4, 2, &st, f, nullptr, nullptr, nullptr, u, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_rollout(&cfg, 4, 2, &st, f, f, nullptr, nullptr, nullptr, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_rollout(&cfg, 0, 2, &st, f, f, nullptr, nullptr, u, nullptr, nullptr), MG_ERR_BAD_SIZE);
    EXPECT(mg_quadrotor_rollout(&cfg, 4, 0, &st, f, f, nullptr, nullptr, u, nullptr, nullptr), MG_ERR_BAD_SIZE);
    EXPECT(mg_quadrotor_rollout(&bad, 4, 2, &st, f, f, nullptr, nullptr, u, nullptr, nullptr), MG_ERR_BAD_CONFIG);
    EXPECT(mg_quadrotor_step_autoreset(nullptr, 4, 2, &ste, &ar, f, f, nullptr, nullptr, u, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_step_autoreset(&cfg, 4, 2, nullptr, &ar, f, f, nullptr, nullptr, u, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_step_autoreset(&cfg, 4, 2, &ste, nullptr, f, f, nullptr, nullptr, u, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_step_autoreset(&cfg, 4, 2, &st, &ar, f, f, nullptr, nullptr, u, nullptr, nullptr), MG_ERR_NULL_POINTER);   // no episode
    EXPECT(mg_quadrotor_step_autoreset(&cfg, 4, 2, &ste, &ar, nullptr, f, nullptr, nullptr, u, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_step_autoreset(&cfg, 4, 2, &ste, &ar, f, nullptr, nullptr, nullptr, u, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_step_autoreset(&cfg, 4, 2, &ste, &ar, f, f, nullptr, nullptr, nullptr, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_step_autoreset(&cfg, -1, 2, &ste, &ar, f, f, nullptr, nullptr, u, nullptr, nullptr), MG_ERR_BAD_SIZE);
    EXPECT(mg_quadrotor_step_autoreset(&cfg, 4, 0, &ste, &ar, f, f, nullptr, nullptr, u, nullptr, nullptr), MG_ERR_BAD_SIZE);
    EXPECT(mg_quadrotor_step_autoreset(&bad, 4, 2, &ste, &ar, f, f, nullptr, nullptr, u, nullptr, nullptr), MG_ERR_BAD_CONFIG);
    // the task table
    mg_quadrotor_tasks tk;
    std::memset(&tk, 0, sizeof(tk));
    tk.rows_d = g_fake; tk.task_id_d = fake<int32_t>(); tk.n_tasks = 3; tk.dt = cfg.dt;
    auto tstep = [&](const mg_quadrotor_config *c, const mg_quadrotor_tasks *t, int n, int steps, const mg_quadrotor_state *s,
                     const mg_quadrotor_autoreset *a, const float *act, float *obs, uint8_t *done) {
        return mg_quadrotor_tasks_step(c, t, n, steps, s, a, act, obs, nullptr, nullptr, done, nullptr, nullptr);
    };
    EXPECT(tstep(nullptr, &tk, 4, 2, &st, nullptr, f, f, u), MG_ERR_NULL_POINTER);
    EXPECT(tstep(&cfg, nullptr, 4, 2, &st, nullptr, f, f, u), MG_ERR_NULL_POINTER);
    EXPECT(tstep(&cfg, &tk, 4, 2, nullptr, nullptr, f, f, u), MG_ERR_NULL_POINTER);
    EXPECT(tstep(&cfg, &tk, 4, 2, &none, nullptr, f, f, u), MG_ERR_NULL_POINTER);
    EXPECT(tstep(&cfg, &tk, 4, 2, &st, nullptr, nullptr, f, u), MG_ERR_NULL_POINTER);
    EXPECT(tstep(&cfg, &tk, 4, 2, &st, nullptr, f, nullptr, u), MG_ERR_NULL_POINTER);
    EXPECT(tstep(&cfg, &tk, 4, 2, &st, nullptr, f, f, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(tstep(&cfg, &tk, 4, 2, &st, &ar, f, f, u), MG_ERR_NULL_POINTER);                  // the fused reset without episode
    EXPECT(tstep(&cfg, &tk, 0, 2, &st, nullptr, f, f, u), MG_ERR_BAD_SIZE);
    EXPECT(tstep(&cfg, &tk, 4, 0, &st, nullptr, f, f, u), MG_ERR_BAD_SIZE);
    EXPECT(tstep(&bad, &tk, 4, 2, &st, nullptr, f, f, u), MG_ERR_BAD_CONFIG);
    EXPECT(mg_quadrotor_tasks_reset(nullptr, &tk, 4, &st, nullptr, nullptr, nullptr, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_tasks_reset(&cfg, nullptr, 4, &st, nullptr, nullptr, nullptr, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_tasks_reset(&cfg, &tk, 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_tasks_reset(&cfg, &tk, 4, &none, nullptr, nullptr, nullptr, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_quadrotor_tasks_reset(&cfg, &tk, 0, &st, nullptr, nullptr, nullptr, nullptr, nullptr), MG_ERR_BAD_SIZE);
    EXPECT(mg_quadrotor_tasks_reset(&bad, &tk, 4, &st, nullptr, nullptr, nullptr, nullptr, nullptr), MG_ERR_BAD_CONFIG);
    for (int k = 0; k < 5; ++k) {                       // what is wrong with a table, the same for both entry points
        mg_quadrotor_tasks t = tk;
        mg_quadrotor_config c = cfg;
        int want = MG_ERR_NULL_POINTER;
        switch (k) {
        case 0: t.rows_d = nullptr; break;
        case 1: t.task_id_d = nullptr; break;
        case 2: t.n_tasks = 0; want = MG_ERR_BAD_SIZE; break;
        case 3: t.dt = 0.02; want = MG_ERR_BAD_CONFIG; break;
        default: c.task = MG_QUADROTOR_TASK_VELOCITY_CONTROL; break;      // needs tasks->velocity_targets_d
        }
        EXPECT(tstep(&c, &t, 4, 2, &st, nullptr, f, f, u), want);
        EXPECT(mg_quadrotor_tasks_reset(&c, &t, 4, &st, nullptr, nullptr, nullptr, nullptr, nullptr), want);
    }
    // closed-loop rollouts, feed-forward and recurrent
    mg_quadrotor_policy pol;
    std::memset(&pol, 0, sizeof(pol));
    pol.params_d = f; pol.policy_id_d = fake<int32_t>(); pol.n_policies = 2; pol.hidden = 8; pol.obs_dim = 16;
    mg_quadrotor_policy_last last;
    std::memset(&last, 0, sizeof(last));
    last.obs = f; last.done = u;
    mg_quadrotor_rpolicy_carry carry;
    carry.h = f; carry.prev_action = f; carry.prev_reward = f; carry.prev_done = u;
    double *d = fake<double>();
    int32_t *i32 = fake<int32_t>();
    for (int rec = 0; rec < 2; ++rec) {
        auto roll = [&](const mg_quadrotor_config *c, const mg_quadrotor_tasks *t, int n, int steps, const mg_quadrotor_state *s,
                        const mg_quadrotor_autoreset *a, const mg_quadrotor_policy *p, const mg_quadrotor_rpolicy_carry *cy, int episodic,
                        double *rt, double *re, int32_t *el, const mg_quadrotor_policy_last *l) {
            return rec ? mg_quadrotor_rpolicy_rollout(c, t, n, steps, s, a, p, cy, episodic, rt, re, el, nullptr, l, nullptr)
                       : mg_quadrotor_policy_rollout(c, t, n, steps, s, a, p, rt, re, el, nullptr, l, nullptr);
        };
        EXPECT(roll(nullptr, nullptr, 4, 2, &st, nullptr, &pol, &carry, 0, d, d, i32, &last), MG_ERR_NULL_POINTER);
        EXPECT(roll(&cfg, nullptr, 4, 2, nullptr, nullptr, &pol, &carry, 0, d, d, i32, &last), MG_ERR_NULL_POINTER);
        EXPECT(roll(&cfg, nullptr, 4, 2, &none, nullptr, &pol, &carry, 0, d, d, i32, &last), MG_ERR_NULL_POINTER);
        EXPECT(roll(&cfg, nullptr, 4, 2, &st, nullptr, nullptr, &carry, 0, d, d, i32, &last), MG_ERR_NULL_POINTER);
        EXPECT(roll(&cfg, nullptr, 4, 2, &st, nullptr, &pol, &carry, 0, nullptr, d, i32, &last), MG_ERR_NULL_POINTER);
        EXPECT(roll(&cfg, nullptr, 4, 2, &st, nullptr, &pol, &carry, 0, d, nullptr, i32, &last), MG_ERR_NULL_POINTER);
        EXPECT(roll(&cfg, nullptr, 4, 2, &st, nullptr, &pol, &carry, 0, d, d, nullptr, &last), MG_ERR_NULL_POINTER);
        EXPECT(roll(&cfg, nullptr, 4, 2, &st, nullptr, &pol, &carry, 0, d, d, i32, nullptr), MG_ERR_NULL_POINTER);
        EXPECT(roll(&cfg, nullptr, 4, 2, &st, &ar, &pol, &carry, 0, d, d, i32, &last), MG_ERR_NULL_POINTER);          // no episode
        {
            mg_quadrotor_policy_last l = last;
            l.obs = nullptr;
            EXPECT(roll(&cfg, nullptr, 4, 2, &st, nullptr, &pol, &carry, 0, d, d, i32, &l), MG_ERR_NULL_POINTER);
            l = last; l.done = nullptr;
            EXPECT(roll(&cfg, nullptr, 4, 2, &st, nullptr, &pol, &carry, 0, d, d, i32, &l), MG_ERR_NULL_POINTER);
            mg_quadrotor_policy p = pol;
            p.params_d = nullptr;
            EXPECT(roll(&cfg, nullptr, 4, 2, &st, nullptr, &p, &carry, 0, d, d, i32, &last), MG_ERR_NULL_POINTER);
            p = pol; p.policy_id_d = nullptr;
            EXPECT(roll(&cfg, nullptr, 4, 2, &st, nullptr, &p, &carry, 0, d, d, i32, &last), MG_ERR_NULL_POINTER);
            p = pol; p.n_policies = 0;
            EXPECT(roll(&cfg, nullptr, 4, 2, &st, nullptr, &p, &carry, 0, d, d, i32, &last), MG_ERR_BAD_SIZE);
            p = pol; p.hidden = rec ? 65 : 257;            // one past the supported path
            EXPECT(roll(&cfg, nullptr, 4, 2, &st, nullptr, &p, &carry, 0, d, d, i32, &last), MG_ERR_BAD_SIZE);
            p = pol; p.hidden = rec ? 0 : -1;
            EXPECT(roll(&cfg, nullptr, 4, 2, &st, nullptr, &p, &carry, 0, d, d, i32, &last), MG_ERR_BAD_SIZE);
            p = pol; p.obs_dim = 19;                        // not the task's
            EXPECT(roll(&cfg, nullptr, 4, 2, &st, nullptr, &p, &carry, 0, d, d, i32, &last), MG_ERR_BAD_CONFIG);
            p = pol; p.params_d = f + 1;                    // not 16-byte aligned
            EXPECT(roll(&cfg, nullptr, 4, 2, &st, nullptr, &p, &carry, 0, d, d, i32, &last), MG_ERR_BAD_CONFIG);
        }
        EXPECT(roll(&cfg, nullptr, 0, 2, &st, nullptr, &pol, &carry, 0, d, d, i32, &last), MG_ERR_BAD_SIZE);
        EXPECT(roll(&cfg, nullptr, 4, 0, &st, nullptr, &pol, &carry, 0, d, d, i32, &last), MG_ERR_BAD_SIZE);
        EXPECT(roll(&bad, nullptr, 4, 2, &st, nullptr, &pol, &carry, 0, d, d, i32, &last), MG_ERR_BAD_CONFIG);
        {
            mg_quadrotor_tasks t = tk;                     // what the step entry points refuse about a table
            t.n_tasks = 0;
            EXPECT(roll(&cfg, &t, 4, 2, &st, nullptr, &pol, &carry, 0, d, d, i32, &last), MG_ERR_BAD_SIZE);
            t = tk; t.rows_d = nullptr;
            EXPECT(roll(&cfg, &t, 4, 2, &st, nullptr, &pol, &carry, 0, d, d, i32, &last), MG_ERR_NULL_POINTER);
            t = tk; t.dt = 0.02;
            EXPECT(roll(&cfg, &t, 4, 2, &st, nullptr, &pol, &carry, 0, d, d, i32, &last), MG_ERR_BAD_CONFIG);
        }
        if (rec) {
            EXPECT(roll(&cfg, nullptr, 4, 2, &st, nullptr, &pol, nullptr, 0, d, d, i32, &last), MG_ERR_NULL_POINTER);
            for (int k = 0; k < 4; ++k) {
                mg_quadrotor_rpolicy_carry cy = carry;
                void **field[4] = {(void **)&cy.h, (void **)&cy.prev_action, (void **)&cy.prev_reward, (void **)&cy.prev_done};
                *field[k] = nullptr;
                EXPECT(roll(&cfg, nullptr, 4, 2, &st, nullptr, &pol, &cy, 0, d, d, i32, &last), MG_ERR_NULL_POINTER);
            }
            mg_quadrotor_rpolicy_carry cy = carry;
            cy.prev_action = f + 1;
            EXPECT(roll(&cfg, nullptr, 4, 2, &st, nullptr, &pol, &cy, 0, d, d, i32, &last), MG_ERR_BAD_CONFIG);
            EXPECT(roll(&cfg, nullptr, 4, 2, &st, nullptr, &pol, &carry, 1, d, d, i32, &last), MG_ERR_BAD_CONFIG);      // episodic without ar
        }
    }
}

// ---- parameter counts ----------------------------------------------------------------------------------------------------------

static void param_counts() {
    for (int h = 0; h <= 256; ++h)
        for (int d : {16, 19}) EXPECT(mg_quadrotor_policy_param_count(h, d), h ? 4 + 24 * h : 4 + 4 * d);
    EXPECT_TRUE(mg_quadrotor_policy_param_count(-1, 16) < 0 && mg_quadrotor_policy_param_count(257, 16) < 0);
    EXPECT_TRUE(mg_quadrotor_policy_param_count(8, 17) < 0 && mg_quadrotor_policy_param_count(8, 0) < 0);
    for (int h = 1; h <= 64; ++h)
        for (int d : {16, 19}) EXPECT_TRUE(mg_quadrotor_rpolicy_param_count(h, d) > 0);
    EXPECT_TRUE(mg_quadrotor_rpolicy_param_count(0, 16) < 0 && mg_quadrotor_rpolicy_param_count(65, 16) < 0 &&
                mg_quadrotor_rpolicy_param_count(8, 18) < 0);
    for (int h = 1; h <= 64; ++h) {
        for (int v = 1; v <= 3; ++v) EXPECT_TRUE(mg_maze2d_policy_param_count(h, v) > 0);
        for (int g = 1; g <= 16; ++g)
            EXPECT_TRUE(mg_maze3d_policy_param_count(h, g, 17 - g, 0) > 0 && mg_maze3d_policy_param_count(h, g, g, 1) > 0);
        for (int a = 2; a <= 64; ++a) EXPECT_TRUE(mg_bandits_policy_param_count(h, a) > 0);
    }
    EXPECT_TRUE(mg_maze2d_policy_param_count(0, 1) < 0 && mg_maze2d_policy_param_count(65, 1) < 0);
    EXPECT_TRUE(mg_maze2d_policy_param_count(8, 0) < 0 && mg_maze2d_policy_param_count(8, 4) < 0);
    EXPECT_TRUE(mg_maze3d_policy_param_count(0, 4, 4, 0) < 0 && mg_maze3d_policy_param_count(65, 4, 4, 0) < 0);
    EXPECT_TRUE(mg_maze3d_policy_param_count(8, 0, 4, 0) < 0 && mg_maze3d_policy_param_count(8, 4, 17, 1) < 0);
    EXPECT(mg_bandits_policy_param_count(8, 65), MG_ERR_BAD_SIZE);                           // 65 arms
    EXPECT(mg_bandits_policy_param_count(8, 1), MG_ERR_BAD_SIZE);
    EXPECT(mg_bandits_policy_param_count(0, 8), MG_ERR_BAD_SIZE);
    EXPECT(mg_bandits_policy_param_count(65, 8), MG_ERR_BAD_SIZE);
    const int max_obs = 8 + 2 * MG_WALKER_MAX_JOINTS + MG_WALKER_MAX_FEET;
    for (int h = 0; h <= 256; ++h)
        for (int a : {1, 8, 17, MG_WALKER_MAX_JOINTS})
            for (int d : {1, 28, 44, max_obs}) {
                EXPECT_TRUE(mg_walker_policy_param_count(h, d, a) > 0);
                if (h) EXPECT(mg_walker_rpolicy_param_count(h, d, a), h + (d + a + 2 + h) * h + a + h * a);
            }
    EXPECT_TRUE(mg_walker_policy_param_count(-1, 28, 8) < 0 && mg_walker_policy_param_count(257, 28, 8) < 0);
    EXPECT_TRUE(mg_walker_policy_param_count(8, 0, 8) < 0 && mg_walker_policy_param_count(8, max_obs + 1, 8) < 0);
    EXPECT_TRUE(mg_walker_policy_param_count(8, 28, 0) < 0 && mg_walker_policy_param_count(8, 28, MG_WALKER_MAX_JOINTS + 1) < 0);
    EXPECT_TRUE(mg_walker_rpolicy_param_count(0, 28, 8) < 0 && mg_walker_rpolicy_param_count(257, 28, 8) < 0);
    for (int h : {1, 7, 64})
        for (int f = 2; f <= MG_LIFTSIM_MAX_FLOORS; ++f)
            for (int e = 1; e <= MG_LIFTSIM_MAX_ELEVATORS; ++e)
                EXPECT_TRUE(mg_liftsim_policy_param_count(h, f, e) > 0 && mg_liftsim_rpolicy_param_count(h, f, e) > 0);
    for (int h = 1; h <= 64; ++h) EXPECT_TRUE(mg_liftsim_policy_param_count(h, 10, 4) > 0 && mg_liftsim_rpolicy_param_count(h, 10, 4) > 0);
    EXPECT(mg_liftsim_policy_param_count(0, 10, 4), MG_ERR_BAD_SIZE);
    EXPECT(mg_liftsim_policy_param_count(65, 10, 4), MG_ERR_BAD_SIZE);
    EXPECT(mg_liftsim_policy_param_count(8, 1, 4), MG_ERR_BAD_SIZE);
    EXPECT(mg_liftsim_policy_param_count(8, 129, 4), MG_ERR_BAD_SIZE);
    EXPECT(mg_liftsim_policy_param_count(8, 10, 0), MG_ERR_BAD_SIZE);
    EXPECT(mg_liftsim_policy_param_count(8, 10, 33), MG_ERR_BAD_SIZE);
    EXPECT(mg_liftsim_rpolicy_param_count(0, 10, 4), MG_ERR_BAD_SIZE);
    EXPECT(mg_liftsim_rpolicy_param_count(8, 129, 4), MG_ERR_BAD_SIZE);
    EXPECT(mg_liftsim_rpolicy_param_count(8, 10, 33), MG_ERR_BAD_SIZE);
    EXPECT_TRUE(mg_maze_distance_queue_capacity() > 0);
}

// ---- liftsim -------------------------------------------------------------------------------------------------------------------

static mg_liftsim_config lift_config(int floors, int elevators) {
    mg_liftsim_config c;
    std::memset(&c, 0, sizeof(c));
    c.floors = floors; c.elevators = elevators; c.generator = MG_LIFTSIM_UNIFORM; c.queue_capacity = 64; c.window = 1200;
    c.particle_number = 12; c.floor_height = 4.0; c.dt = 0.5; c.generation_interval = 150.0; c.nv_magic = 1.7155277699214135;
    return c;
}

static void liftsim() {
    int64_t off[MG_LS_NFIELDS], total = 0;
    for (int f = 2; f <= MG_LIFTSIM_MAX_FLOORS; ++f)
        for (int e = 1; e <= MG_LIFTSIM_MAX_ELEVATORS; ++e) {
            const mg_liftsim_config c = lift_config(f, e);
            const int n = 1 + (f * 7 + e) % 130;
            EXPECT(mg_liftsim_layout(&c, n, off, &total), MG_OK);
            bool ok = off[0] >= 0 && total > off[MG_LS_NFIELDS - 1];
            for (int k = 0; k < MG_LS_NFIELDS; ++k) ok = ok && off[k] % 256 == 0 && (k == 0 || off[k] > off[k - 1]);
            EXPECT_TRUE(ok);
        }
    mg_liftsim_config c = lift_config(10, 4);
    EXPECT(mg_liftsim_layout(nullptr, 4, off, &total), MG_ERR_NULL_POINTER);
    EXPECT(mg_liftsim_layout(&c, 4, nullptr, &total), MG_ERR_NULL_POINTER);
    EXPECT(mg_liftsim_layout(&c, 4, off, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_liftsim_layout(&c, 0, off, &total), MG_ERR_BAD_SIZE);
    for (int bad = 0; bad < 9; ++bad) {
        mg_liftsim_config b = lift_config(10, 4);
        switch (bad) {
        case 0: b.floors = 1; break;
        case 1: b.floors = MG_LIFTSIM_MAX_FLOORS + 1; break;
        case 2: b.elevators = 0; break;
        case 3: b.elevators = MG_LIFTSIM_MAX_ELEVATORS + 1; break;
        case 4: b.dt = 1.5; break;
        case 5: b.floor_height = 0.0; break;
        case 6: b.queue_capacity = 4097; break;
        case 7: b.window = 0; break;
        default: b.generator = 7; break;
        }
        EXPECT(mg_liftsim_layout(&b, 4, off, &total), MG_ERR_BAD_CONFIG);
    }
    c.generator = MG_LIFTSIM_CUSTOM;                    // CUSTOM without its tables, and with more than 16 floors
    c.table_len = 3;
    EXPECT(mg_liftsim_layout(&c, 4, off, &total), MG_ERR_BAD_CONFIG);
    // the launching entry points refuse the same things before they launch
    EXPECT(mg_liftsim_step(&c, 4, g_fake, fake<int32_t>(), nullptr), MG_ERR_BAD_CONFIG);
    c = lift_config(10, 4);
    EXPECT(mg_liftsim_step(&c, 0, g_fake, fake<int32_t>(), nullptr), MG_ERR_BAD_SIZE);
    EXPECT(mg_liftsim_step(nullptr, 4, g_fake, fake<int32_t>(), nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_liftsim_step(&c, 4, nullptr, fake<int32_t>(), nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_liftsim_step(&c, 4, g_fake, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_liftsim_reset(&c, 4, nullptr, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_liftsim_seed(&c, 4, nullptr, 1u, nullptr, nullptr), MG_ERR_NULL_POINTER);
}

// ---- maze ----------------------------------------------------------------------------------------------------------------------

// The other maze entry points. F is a complete ESCAPE table of n = 9, S a complete state, V a complete view: every call below
// is refused for the one thing it changes.
static void maze_launches(const mg_maze_tasks &F, const mg_maze_state &S, const mg_maze_view &Vin) {
    mg_maze_view V = Vin;
    V.res_h = V.res_v = 32; V.max_ray_records = 0;
    int32_t *i32 = fake<int32_t>();
    float *f = fake<float>();
    double *d = fake<double>();
    uint8_t *u = fake<uint8_t>();
    mg_maze_tasks small = F, notasks = F, nowalls = F;
    small.n = 2; notasks.n_tasks = 0; nowalls.walls = nullptr;
    mg_maze_state nogrid = S;
    nogrid.grid = nullptr;
    // reset
    EXPECT(mg_maze_reset(nullptr, MG_MAZE_ESCAPE, 4, &S, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_maze_reset(&F, MG_MAZE_ESCAPE, 4, nullptr, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_maze_reset(&F, MG_MAZE_ESCAPE, 0, &S, nullptr, nullptr), MG_ERR_BAD_SIZE);
    EXPECT(mg_maze_reset(&small, MG_MAZE_ESCAPE, 4, &S, nullptr, nullptr), MG_ERR_BAD_SIZE);
    EXPECT(mg_maze_reset(&notasks, MG_MAZE_ESCAPE, 4, &S, nullptr, nullptr), MG_ERR_BAD_SIZE);
    EXPECT(mg_maze_reset(&nowalls, MG_MAZE_ESCAPE, 4, &S, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_maze_reset(&F, MG_MAZE_ESCAPE, 4, &nogrid, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_maze_reset(&F, MG_MAZE_SURVIVAL, 4, &S, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_maze_reset(&F, 2, 4, &S, nullptr, nullptr), MG_ERR_BAD_CONFIG);
    // the sampler: MazeTaskManager.sample_task's own asserts, and the sizes the kernel supports
    mg_maze_sample_params sp;
    std::memset(&sp, 0, sizeof(sp));
    sp.n = 15; sp.n_texts = 7; sp.cell_size = 2.0; sp.wall_height = 3.2; sp.agent_height = 1.6; sp.step_reward = -0.01; sp.food_reward = 0.5;
    sp.initial_life = 1.0; sp.max_life = 2.0; sp.food_density = 0.01; sp.crowd_ratio = 0.0;
    auto sample = [&](const mg_maze_sample_params *p, int n_tasks, int null_at) {
        void *a[7] = {i32, i32, g_fake, u, d, i32, d};
        if (null_at >= 0) a[null_at] = nullptr;
        return mg_maze_sample_tasks(p, n_tasks, 1u, nullptr, (int32_t *)a[0], (int32_t *)a[1], (int8_t *)a[2], (uint8_t *)a[3], (double *)a[4],
                                    (int32_t *)a[5], (double *)a[6], nullptr);
    };
    EXPECT(sample(nullptr, 4, -1), MG_ERR_NULL_POINTER);
    for (int k = 0; k < 7; ++k) EXPECT(sample(&sp, 4, k), MG_ERR_NULL_POINTER);
    EXPECT(sample(&sp, 0, -1), MG_ERR_BAD_SIZE);
    EXPECT(sample(&sp, -2, -1), MG_ERR_BAD_SIZE);
    for (int n = -1; n <= 70; ++n) {                    // n <= 6, even n, n > 63; every accepted n is left to the GPU tests
        if (n >= 7 && n <= 63 && n % 2 == 1) continue;
        mg_maze_sample_params p = sp;
        p.n = n;
        EXPECT(sample(&p, 4, -1), n <= 6 || n % 2 == 0 ? MG_ERR_BAD_CONFIG : MG_ERR_UNSUPPORTED);
    }
    for (int nt : {1, 256, 0, -1}) {
        mg_maze_sample_params p = sp;
        p.n_texts = nt;
        EXPECT(sample(&p, 4, -1), MG_ERR_BAD_CONFIG);
    }
    {
        mg_maze_sample_params p = sp;
        p.step_reward = 0.0;
        EXPECT(sample(&p, 4, -1), MG_ERR_BAD_CONFIG);
        p = sp; p.has_goal_reward = 1; p.goal_reward = 0.0;
        EXPECT(sample(&p, 4, -1), MG_ERR_BAD_CONFIG);
        p = sp; p.food_reward = 0.05;
        EXPECT(sample(&p, 4, -1), MG_ERR_UNSUPPORTED);
        p = sp; p.food_density = -0.1;
        EXPECT(sample(&p, 4, -1), MG_ERR_BAD_CONFIG);
        p = sp; p.crowd_ratio = -0.1;
        EXPECT(sample(&p, 4, -1), MG_ERR_BAD_CONFIG);
    }
    // the 2-D rollout
    auto roll2 = [&](const mg_maze_tasks *t, int tt, int vg, int n, const mg_maze_state *s, int steps, int every, const int32_t *act, float *obs,
                     uint8_t *done) { return mg_maze2d_rollout(t, tt, 100, vg, 0, n, s, steps, every, act, obs, nullptr, nullptr, done, nullptr); };
    EXPECT(roll2(nullptr, MG_MAZE_ESCAPE, 1, 4, &S, 3, 0, i32, f, u), MG_ERR_NULL_POINTER);
    EXPECT(roll2(&F, MG_MAZE_ESCAPE, 1, 4, nullptr, 3, 0, i32, f, u), MG_ERR_NULL_POINTER);
    EXPECT(roll2(&F, MG_MAZE_ESCAPE, 1, 4, &S, 3, 0, nullptr, f, u), MG_ERR_NULL_POINTER);
    EXPECT(roll2(&F, MG_MAZE_ESCAPE, 1, 4, &S, 3, 0, i32, nullptr, u), MG_ERR_NULL_POINTER);
    EXPECT(roll2(&F, MG_MAZE_ESCAPE, 1, 4, &S, 3, 0, i32, f, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(roll2(&F, MG_MAZE_ESCAPE, 1, 0, &S, 3, 0, i32, f, u), MG_ERR_BAD_SIZE);
    EXPECT(roll2(&F, MG_MAZE_ESCAPE, -1, 4, &S, 3, 0, i32, f, u), MG_ERR_BAD_SIZE);
    EXPECT(roll2(&F, MG_MAZE_ESCAPE, 1, 4, &S, 0, 0, i32, f, u), MG_ERR_BAD_SIZE);
    EXPECT(roll2(&F, MG_MAZE_ESCAPE, 1, 4, &S, 3, -1, i32, f, u), MG_ERR_BAD_SIZE);
    EXPECT(roll2(&small, MG_MAZE_ESCAPE, 1, 4, &S, 3, 0, i32, f, u), MG_ERR_BAD_SIZE);
    EXPECT(roll2(&nowalls, MG_MAZE_ESCAPE, 1, 4, &S, 3, 0, i32, f, u), MG_ERR_NULL_POINTER);
    EXPECT(roll2(&F, MG_MAZE_ESCAPE, 1, 4, &nogrid, 3, 0, i32, f, u), MG_ERR_NULL_POINTER);
    EXPECT(roll2(&F, MG_MAZE_SURVIVAL, 1, 4, &S, 3, 0, i32, f, u), MG_ERR_NULL_POINTER);
    EXPECT(roll2(&F, 2, 1, 4, &S, 3, 0, i32, f, u), MG_ERR_BAD_CONFIG);
    // the 3-D step's own arguments, through the check that launches nothing, and the 3-D rollout
    auto check3 = [&](const mg_maze_tasks *t, const mg_maze_view *v, int tt, int cont, int n, const mg_maze_state *s, void *obs) {
        return mg_maze3d_step_check(t, v, tt, 100, cont, 0, n, s, obs, nullptr);
    };
    EXPECT(check3(nullptr, &V, MG_MAZE_ESCAPE, 0, 4, &S, g_fake), MG_ERR_NULL_POINTER);
    EXPECT(check3(&F, nullptr, MG_MAZE_ESCAPE, 0, 4, &S, g_fake), MG_ERR_NULL_POINTER);
    EXPECT(check3(&F, &V, MG_MAZE_ESCAPE, 0, 4, nullptr, g_fake), MG_ERR_NULL_POINTER);
    EXPECT(check3(&F, &V, MG_MAZE_ESCAPE, 0, 4, &S, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(check3(&F, &V, MG_MAZE_ESCAPE, 0, 0, &S, g_fake), MG_ERR_BAD_SIZE);
    EXPECT(check3(&small, &V, MG_MAZE_ESCAPE, 0, 4, &S, g_fake), MG_ERR_BAD_SIZE);
    EXPECT(check3(&F, &V, MG_MAZE_ESCAPE, 0, 4, &nogrid, g_fake), MG_ERR_NULL_POINTER);
    EXPECT(check3(&F, &V, MG_MAZE_SURVIVAL, 0, 4, &S, g_fake), MG_ERR_NULL_POINTER);
    {
        mg_maze_state s = S;
        s.ori_idx = nullptr;
        EXPECT(check3(&F, &V, MG_MAZE_ESCAPE, 0, 4, &s, g_fake), MG_ERR_NULL_POINTER);
        s = S; s.ori = nullptr;
        EXPECT(check3(&F, &V, MG_MAZE_ESCAPE, 1, 4, &s, g_fake), MG_ERR_NULL_POINTER);
        s = S; s.loc = nullptr;
        EXPECT(check3(&F, &V, MG_MAZE_ESCAPE, 1, 4, &s, g_fake), MG_ERR_NULL_POINTER);
        mg_maze_view v = V;
        v.res_h = 0;
        EXPECT(check3(&F, &v, MG_MAZE_ESCAPE, 0, 4, &S, g_fake), MG_ERR_BAD_SIZE);
        v = V; v.res_v = 0;
        EXPECT(check3(&F, &v, MG_MAZE_ESCAPE, 0, 4, &S, g_fake), MG_ERR_BAD_SIZE);
        v = V; v.col_cos = nullptr;
        EXPECT(check3(&F, &v, MG_MAZE_ESCAPE, 0, 4, &S, g_fake), MG_ERR_NULL_POINTER);
        v = V; v.col_sin = nullptr;
        EXPECT(check3(&F, &v, MG_MAZE_ESCAPE, 0, 4, &S, g_fake), MG_ERR_NULL_POINTER);
        v = V; v.textures = nullptr;
        EXPECT(check3(&F, &v, MG_MAZE_ESCAPE, 0, 4, &S, g_fake), MG_ERR_NULL_POINTER);
        v = V; v.ceil_texture = nullptr;
        EXPECT(check3(&F, &v, MG_MAZE_ESCAPE, 0, 4, &S, g_fake), MG_ERR_NULL_POINTER);
        v = V; v.tex_size = 0;
        EXPECT(check3(&F, &v, MG_MAZE_ESCAPE, 0, 4, &S, g_fake), MG_ERR_BAD_SIZE);
        v = V; v.n_textures = 0;
        EXPECT(check3(&F, &v, MG_MAZE_ESCAPE, 0, 4, &S, g_fake), MG_ERR_BAD_SIZE);
    }
    auto roll3 = [&](const mg_maze_tasks *t, const mg_maze_view *v, int n, const mg_maze_state *s, int steps, int every, const void *act, void *obs,
                     uint8_t *done) {
        return mg_maze3d_rollout(t, v, MG_MAZE_ESCAPE, 100, 0, 0, n, s, steps, every, act, obs, nullptr, nullptr, done, nullptr);
    };
    EXPECT(roll3(nullptr, &V, 4, &S, 3, 0, i32, g_fake, u), MG_ERR_NULL_POINTER);
    EXPECT(roll3(&F, nullptr, 4, &S, 3, 0, i32, g_fake, u), MG_ERR_NULL_POINTER);
    EXPECT(roll3(&F, &V, 4, nullptr, 3, 0, i32, g_fake, u), MG_ERR_NULL_POINTER);
    EXPECT(roll3(&F, &V, 4, &S, 3, 0, nullptr, g_fake, u), MG_ERR_NULL_POINTER);
    EXPECT(roll3(&F, &V, 4, &S, 3, 0, i32, nullptr, u), MG_ERR_NULL_POINTER);
    EXPECT(roll3(&F, &V, 4, &S, 3, 0, i32, g_fake, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(roll3(&F, &V, 0, &S, 3, 0, i32, g_fake, u), MG_ERR_BAD_SIZE);
    EXPECT(roll3(&F, &V, 4, &S, 0, 0, i32, g_fake, u), MG_ERR_BAD_SIZE);
    EXPECT(roll3(&F, &V, 4, &S, 3, -1, i32, g_fake, u), MG_ERR_BAD_SIZE);
    EXPECT(roll3(&small, &V, 4, &S, 3, 0, i32, g_fake, u), MG_ERR_BAD_SIZE);
    // distance fields and the experts
    EXPECT(mg_maze_distance_field(nullptr, MG_MAZE_FIELD_TURNS, nullptr, i32, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_maze_distance_field(&F, MG_MAZE_FIELD_TURNS, nullptr, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_maze_distance_field(&F, 3, nullptr, i32, nullptr), MG_ERR_BAD_CONFIG);
    EXPECT(mg_maze_distance_field(&F, -1, nullptr, i32, nullptr), MG_ERR_BAD_CONFIG);
    for (int kind = 0; kind < 3; ++kind) {
        EXPECT(mg_maze_distance_field(&small, kind, nullptr, i32, nullptr), MG_ERR_BAD_SIZE);
        EXPECT(mg_maze_distance_field(&notasks, kind, nullptr, i32, nullptr), MG_ERR_BAD_SIZE);
        EXPECT(mg_maze_distance_field(&nowalls, kind, nullptr, i32, nullptr), MG_ERR_NULL_POINTER);
    }
    EXPECT(mg_maze_expert_action(nullptr, MG_MAZE_FIELD_TURNS, i32, 4, &S, i32, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_maze_expert_action(&F, MG_MAZE_FIELD_TURNS, nullptr, 4, &S, i32, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_maze_expert_action(&F, MG_MAZE_FIELD_TURNS, i32, 4, nullptr, i32, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_maze_expert_action(&F, MG_MAZE_FIELD_TURNS, i32, 4, &S, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_maze_expert_action(&F, 3, i32, 4, &S, i32, nullptr), MG_ERR_BAD_CONFIG);
    EXPECT(mg_maze_expert_action(&F, MG_MAZE_FIELD_CELLS_3D, i32, 4, &S, i32, nullptr), MG_ERR_BAD_CONFIG);
    EXPECT(mg_maze_expert_action(&F, MG_MAZE_FIELD_MOVES_2D, i32, 0, &S, i32, nullptr), MG_ERR_BAD_SIZE);
    EXPECT(mg_maze_expert_action(&small, MG_MAZE_FIELD_MOVES_2D, i32, 4, &S, i32, nullptr), MG_ERR_BAD_SIZE);
    EXPECT(mg_maze_expert_action(&F, MG_MAZE_FIELD_MOVES_2D, i32, 4, &nogrid, i32, nullptr), MG_ERR_NULL_POINTER);
    {
        mg_maze_state s = S;
        s.ori_idx = nullptr;
        EXPECT(mg_maze_expert_action(&F, MG_MAZE_FIELD_TURNS, i32, 4, &s, i32, nullptr), MG_ERR_NULL_POINTER);
        EXPECT(mg_maze_steer_action(nullptr, i32, 4, &S, f, nullptr), MG_ERR_NULL_POINTER);
        EXPECT(mg_maze_steer_action(&F, nullptr, 4, &S, f, nullptr), MG_ERR_NULL_POINTER);
        EXPECT(mg_maze_steer_action(&F, i32, 4, nullptr, f, nullptr), MG_ERR_NULL_POINTER);
        EXPECT(mg_maze_steer_action(&F, i32, 4, &S, nullptr, nullptr), MG_ERR_NULL_POINTER);
        EXPECT(mg_maze_steer_action(&F, i32, 0, &S, f, nullptr), MG_ERR_BAD_SIZE);
        EXPECT(mg_maze_steer_action(&small, i32, 4, &S, f, nullptr), MG_ERR_BAD_SIZE);
        s = S; s.loc = nullptr;
        EXPECT(mg_maze_steer_action(&F, i32, 4, &s, f, nullptr), MG_ERR_NULL_POINTER);
        s = S; s.ori = nullptr;
        EXPECT(mg_maze_steer_action(&F, i32, 4, &s, f, nullptr), MG_ERR_NULL_POINTER);
    }
    for (int k = -1; k < 7; ++k) {                      // the 2-D expert rollout: k = 0..6 makes one required pointer NULL
        const void *a[7] = {&F, &S, i32, f, d, d, i32};
        if (k >= 0) a[k] = nullptr;
        int32_t *episodes = k == -1 ? nullptr : i32;
        EXPECT(mg_maze2d_expert_rollout((const mg_maze_tasks *)a[0], MG_MAZE_ESCAPE, 100, 1, 0, 4, (const mg_maze_state *)a[1], 3, 0,
                                        (const int32_t *)a[2], (float *)a[3], (double *)a[4], (double *)a[5], (int32_t *)a[6], episodes, nullptr,
                                        nullptr, nullptr, nullptr, nullptr, nullptr), MG_ERR_NULL_POINTER);
    }
    auto xroll2 = [&](const mg_maze_tasks *t, int tt, int vg, int n, const mg_maze_state *s, int steps, int every) {
        return mg_maze2d_expert_rollout(t, tt, 100, vg, 0, n, s, steps, every, i32, f, d, d, i32, i32, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    };
    EXPECT(xroll2(&F, MG_MAZE_ESCAPE, 1, 0, &S, 3, 0), MG_ERR_BAD_SIZE);
    EXPECT(xroll2(&F, MG_MAZE_ESCAPE, 1, 4, &S, 0, 0), MG_ERR_BAD_SIZE);
    EXPECT(xroll2(&F, MG_MAZE_ESCAPE, 1, 4, &S, 3, -1), MG_ERR_BAD_SIZE);
    EXPECT(xroll2(&F, MG_MAZE_ESCAPE, -1, 4, &S, 3, 0), MG_ERR_BAD_CONFIG);
    EXPECT(xroll2(&small, MG_MAZE_ESCAPE, 1, 4, &S, 3, 0), MG_ERR_BAD_SIZE);
    EXPECT(xroll2(&F, MG_MAZE_ESCAPE, 1, 4, &nogrid, 3, 0), MG_ERR_NULL_POINTER);
    EXPECT(xroll2(&F, MG_MAZE_SURVIVAL, 1, 4, &S, 3, 0), MG_ERR_NULL_POINTER);
    for (int k = 0; k < 9; ++k) {                       // the 3-D expert rollout
        const void *a[9] = {&F, &V, &S, i32, g_fake, d, d, i32, i32};
        a[k] = nullptr;
        EXPECT(mg_maze3d_expert_rollout((const mg_maze_tasks *)a[0], (const mg_maze_view *)a[1], MG_MAZE_ESCAPE, 100, 0, 0, 4,
                                        (const mg_maze_state *)a[2], 3, 0, (const int32_t *)a[3], (void *)a[4], (double *)a[5], (double *)a[6],
                                        (int32_t *)a[7], (int32_t *)a[8], nullptr, nullptr, nullptr, nullptr, nullptr), MG_ERR_NULL_POINTER);
    }
    auto xroll3 = [&](const mg_maze_tasks *t, int n, int steps, int every) {
        return mg_maze3d_expert_rollout(t, &V, MG_MAZE_ESCAPE, 100, 0, 0, n, &S, steps, every, i32, g_fake, d, d, i32, i32, nullptr, nullptr, nullptr,
                                        nullptr, nullptr);
    };
    EXPECT(xroll3(&F, 0, 3, 0), MG_ERR_BAD_SIZE);
    EXPECT(xroll3(&F, 4, 0, 0), MG_ERR_BAD_SIZE);
    EXPECT(xroll3(&F, 4, 3, -1), MG_ERR_BAD_SIZE);
    EXPECT(xroll3(&small, 4, 3, 0), MG_ERR_BAD_SIZE);
    // the recurrent 2-D policy rollout
    mg_maze_policy P;
    std::memset(&P, 0, sizeof(P));
    P.n_policies = 2; P.hidden = 8; P.view_grid = 1; P.params = f;
    mg_maze_policy_carry K;
    K.h = f; K.prev_action = i32; K.prev_reward = f; K.prev_done = u;
    for (int k = 0; k < 10; ++k) {
        const void *a[10] = {&F, &S, &P, i32, &K, f, d, d, i32, i32};
        a[k] = nullptr;
        EXPECT(mg_maze2d_policy_rollout((const mg_maze_tasks *)a[0], MG_MAZE_ESCAPE, 100, 1, 0, 4, (const mg_maze_state *)a[1], 3, 0,
                                        (const mg_maze_policy *)a[2], (const int32_t *)a[3], (const mg_maze_policy_carry *)a[4], 1u, 0u, 0,
                                        (float *)a[5], (double *)a[6], (double *)a[7], (int32_t *)a[8], (int32_t *)a[9], nullptr, nullptr, nullptr,
                                        nullptr, nullptr, nullptr), MG_ERR_NULL_POINTER);
    }
    auto proll2 = [&](const mg_maze_tasks *t, int tt, int vg, int n, const mg_maze_state *s, int steps, int every, const mg_maze_policy *p,
                      const mg_maze_policy_carry *c) {
        return mg_maze2d_policy_rollout(t, tt, 100, vg, 0, n, s, steps, every, p, i32, c, 1u, 0u, 0, f, d, d, i32, i32, nullptr, nullptr, nullptr,
                                        nullptr, nullptr, nullptr);
    };
    for (int k = 0; k < 4; ++k) {
        mg_maze_policy_carry c = K;
        void **field[4] = {(void **)&c.h, (void **)&c.prev_action, (void **)&c.prev_reward, (void **)&c.prev_done};
        *field[k] = nullptr;
        EXPECT(proll2(&F, MG_MAZE_ESCAPE, 1, 4, &S, 3, 0, &P, &c), MG_ERR_NULL_POINTER);
    }
    EXPECT(proll2(&F, MG_MAZE_ESCAPE, 1, 0, &S, 3, 0, &P, &K), MG_ERR_BAD_SIZE);
    EXPECT(proll2(&F, MG_MAZE_ESCAPE, 1, 4, &S, 0, 0, &P, &K), MG_ERR_BAD_SIZE);
    EXPECT(proll2(&F, MG_MAZE_ESCAPE, 1, 4, &S, 3, -1, &P, &K), MG_ERR_BAD_SIZE);
    EXPECT(proll2(&F, MG_MAZE_ESCAPE, 0, 4, &S, 3, 0, &P, &K), MG_ERR_BAD_CONFIG);
    EXPECT(proll2(&F, MG_MAZE_ESCAPE, 4, 4, &S, 3, 0, &P, &K), MG_ERR_BAD_CONFIG);
    EXPECT(proll2(&F, MG_MAZE_ESCAPE, 2, 4, &S, 3, 0, &P, &K), MG_ERR_BAD_CONFIG);       // not the policy's view_grid
    EXPECT(proll2(&small, MG_MAZE_ESCAPE, 1, 4, &S, 3, 0, &P, &K), MG_ERR_BAD_SIZE);
    EXPECT(proll2(&F, MG_MAZE_ESCAPE, 1, 4, &nogrid, 3, 0, &P, &K), MG_ERR_NULL_POINTER);
    EXPECT(proll2(&F, MG_MAZE_SURVIVAL, 1, 4, &S, 3, 0, &P, &K), MG_ERR_NULL_POINTER);
    {
        mg_maze_policy p = P;
        p.params = nullptr;
        EXPECT(proll2(&F, MG_MAZE_ESCAPE, 1, 4, &S, 3, 0, &p, &K), MG_ERR_NULL_POINTER);
        p = P; p.params = f + 1;
        EXPECT(proll2(&F, MG_MAZE_ESCAPE, 1, 4, &S, 3, 0, &p, &K), MG_ERR_BAD_CONFIG);
        p = P; p.n_policies = 0;
        EXPECT(proll2(&F, MG_MAZE_ESCAPE, 1, 4, &S, 3, 0, &p, &K), MG_ERR_BAD_SIZE);
        p = P; p.hidden = 0;
        EXPECT(proll2(&F, MG_MAZE_ESCAPE, 1, 4, &S, 3, 0, &p, &K), MG_ERR_BAD_SIZE);
        p = P; p.hidden = 65;                               // one past the supported path
        EXPECT(proll2(&F, MG_MAZE_ESCAPE, 1, 4, &S, 3, 0, &p, &K), MG_ERR_BAD_SIZE);
    }
    // pooling and the 3-D policy rollout
    EXPECT(mg_maze3d_pool_features(nullptr, 4, g_fake, 4, 4, 1.0f, f, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_maze3d_pool_features(&V, 4, nullptr, 4, 4, 1.0f, f, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_maze3d_pool_features(&V, 4, g_fake, 4, 4, 1.0f, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_maze3d_pool_features(&V, 0, g_fake, 4, 4, 1.0f, f, nullptr), MG_ERR_BAD_SIZE);
    EXPECT(mg_maze3d_pool_features(&V, 4, g_fake, 0, 4, 1.0f, f, nullptr), MG_ERR_BAD_SIZE);
    EXPECT(mg_maze3d_pool_features(&V, 4, g_fake, 4, 17, 1.0f, f, nullptr), MG_ERR_BAD_SIZE);
    EXPECT(mg_maze3d_pool_features(&V, 4, g_fake, 5, 4, 1.0f, f, nullptr), MG_ERR_BAD_CONFIG);       // 5 does not divide 32
    EXPECT(mg_maze3d_pool_features(&V, 4, g_fake, 4, 3, 1.0f, f, nullptr), MG_ERR_BAD_CONFIG);
    mg_maze3d_policy Q;
    std::memset(&Q, 0, sizeof(Q));
    Q.n_policies = 2; Q.hidden = 8; Q.grid_h = Q.grid_v = 4; Q.continuous = 0; Q.scale = (float)(1.0 / (255.0 * 8 * 8)); Q.params = f;
    for (int k = 0; k < 11; ++k) {
        const void *a[11] = {&F, &V, &S, &Q, i32, &K, g_fake, d, d, i32, i32};
        a[k] = nullptr;
        EXPECT(mg_maze3d_policy_rollout((const mg_maze_tasks *)a[0], (const mg_maze_view *)a[1], MG_MAZE_ESCAPE, 100, 0, 0, 4,
                                        (const mg_maze_state *)a[2], 3, 0, (const mg_maze3d_policy *)a[3], (const int32_t *)a[4],
                                        (const mg_maze_policy_carry *)a[5], 1u, 0u, 0, (void *)a[6], nullptr, (double *)a[7], (double *)a[8],
                                        (int32_t *)a[9], (int32_t *)a[10], nullptr, nullptr, nullptr, nullptr, nullptr), MG_ERR_NULL_POINTER);
    }
    auto proll3 = [&](const mg_maze_tasks *t, const mg_maze_view *v, int cont, int n, int steps, int every, const mg_maze3d_policy *p,
                      const mg_maze_policy_carry *c) {
        return mg_maze3d_policy_rollout(t, v, MG_MAZE_ESCAPE, 100, cont, 0, n, &S, steps, every, p, i32, c, 1u, 0u, 0, g_fake, nullptr, d, d, i32, i32,
                                        nullptr, nullptr, nullptr, nullptr, nullptr);
    };
    for (int k = 0; k < 4; ++k) {
        mg_maze_policy_carry c = K;
        void **field[4] = {(void **)&c.h, (void **)&c.prev_action, (void **)&c.prev_reward, (void **)&c.prev_done};
        *field[k] = nullptr;
        EXPECT(proll3(&F, &V, 0, 4, 3, 0, &Q, &c), MG_ERR_NULL_POINTER);
    }
    EXPECT(proll3(&F, &V, 0, 0, 3, 0, &Q, &K), MG_ERR_BAD_SIZE);
    EXPECT(proll3(&F, &V, 0, 4, 0, 0, &Q, &K), MG_ERR_BAD_SIZE);
    EXPECT(proll3(&F, &V, 0, 4, 3, -1, &Q, &K), MG_ERR_BAD_SIZE);
    EXPECT(proll3(&F, &V, 1, 4, 3, 0, &Q, &K), MG_ERR_BAD_CONFIG);                         // a discrete policy on the continuous env
    EXPECT(proll3(&small, &V, 0, 4, 3, 0, &Q, &K), MG_ERR_BAD_SIZE);
    {
        mg_maze3d_policy p = Q;
        p.params = nullptr;
        EXPECT(proll3(&F, &V, 0, 4, 3, 0, &p, &K), MG_ERR_NULL_POINTER);
        p = Q; p.params = f + 1;
        EXPECT(proll3(&F, &V, 0, 4, 3, 0, &p, &K), MG_ERR_BAD_CONFIG);
        p = Q; p.n_policies = 0;
        EXPECT(proll3(&F, &V, 0, 4, 3, 0, &p, &K), MG_ERR_BAD_SIZE);
        p = Q; p.hidden = 0;
        EXPECT(proll3(&F, &V, 0, 4, 3, 0, &p, &K), MG_ERR_BAD_SIZE);
        p = Q; p.hidden = 65;
        EXPECT(proll3(&F, &V, 0, 4, 3, 0, &p, &K), MG_ERR_BAD_SIZE);
        p = Q; p.grid_h = 17;
        EXPECT(proll3(&F, &V, 0, 4, 3, 0, &p, &K), MG_ERR_BAD_SIZE);
        p = Q; p.grid_v = 0;
        EXPECT(proll3(&F, &V, 0, 4, 3, 0, &p, &K), MG_ERR_BAD_SIZE);
        p = Q; p.grid_h = 5;
        EXPECT(proll3(&F, &V, 0, 4, 3, 0, &p, &K), MG_ERR_BAD_CONFIG);
        p = Q; p.scale = 1.0f;                              // not float32(1 / (255 * bh * bv))
        EXPECT(proll3(&F, &V, 0, 4, 3, 0, &p, &K), MG_ERR_BAD_CONFIG);
    }
}

static void maze() {
    std::vector<double> scalars(5 * 8, 0.0);
    for (int t = 0; t < 5; ++t) scalars[8 * t] = 2.0;
    mg_maze_tasks T;
    std::memset(&T, 0, sizeof(T));
    T.n = 9; T.n_tasks = 5; T.scalars = scalars.data();       // a host pointer: read directly (header, mg_maze_check_uniform_cell_size)
    EXPECT(mg_maze_check_uniform_cell_size(&T, 2.0, nullptr), MG_OK);
    EXPECT(mg_maze_check_uniform_cell_size(&T, 1.0, nullptr), MG_ERR_BAD_CONFIG);
    scalars[8 * 3] = 2.0000000000000004;
    EXPECT(mg_maze_check_uniform_cell_size(&T, 2.0, nullptr), MG_ERR_BAD_CONFIG);
    EXPECT(mg_maze_check_uniform_cell_size(&T, 0.0, nullptr), MG_ERR_BAD_CONFIG);
    EXPECT(mg_maze_check_uniform_cell_size(&T, NAN, nullptr), MG_ERR_BAD_CONFIG);
    EXPECT(mg_maze_check_uniform_cell_size(nullptr, 2.0, nullptr), MG_ERR_NULL_POINTER);
    T.scalars = nullptr;
    EXPECT(mg_maze_check_uniform_cell_size(&T, 2.0, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_maze_forget_tasks(&T), MG_OK);
    T.scalars = scalars.data();
    T.n_tasks = 0;
    EXPECT(mg_maze_check_uniform_cell_size(&T, 2.0, nullptr), MG_ERR_BAD_SIZE);
    T.n_tasks = 5;
    EXPECT(mg_maze_forget_tasks(&T), MG_OK);
    EXPECT(mg_maze_forget_tasks(&T), MG_OK);
    EXPECT(mg_maze_forget_tasks(nullptr), MG_ERR_NULL_POINTER);
    // the column tables: every width up to 256, exactly res_h doubles each
    for (int H = 1; H <= 256; ++H) {
        std::vector<double> cc((size_t)H), ss((size_t)H);
        EXPECT(mg_maze_view_tables(H, std::tan(0.3 * 3.1415926), 0.20, cc.data(), ss.data()), MG_OK);
        bool ok = true;
        for (int d = 0; d < H; ++d) ok = ok && std::fabs(cc[d] * cc[d] + ss[d] * ss[d] - 1.0) < 1e-12 && cc[d] > 0.0;
        EXPECT_TRUE(ok);
    }
    double one[1];
    EXPECT(mg_maze_view_tables(0, 1.0, 0.2, one, one), MG_ERR_BAD_SIZE);
    EXPECT(mg_maze_view_tables(1, 1.0, 0.2, nullptr, one), MG_ERR_NULL_POINTER);
    EXPECT(mg_maze_view_tables(1, 1.0, 0.2, one, nullptr), MG_ERR_NULL_POINTER);
    // the table checks every maze entry point starts with: sizes, then arrays, then the task type
    mg_maze_state S;
    std::memset(&S, 0, sizeof(S));
    S.task_id = fake<int32_t>(); S.grid = fake<int32_t>(); S.steps = fake<int32_t>();
    auto step2d = [&](const mg_maze_tasks *t, int task_type, int vg, int n_envs, const mg_maze_state *s) {
        return mg_maze2d_step(t, task_type, 100, vg, 0, n_envs, s, fake<int32_t>(), fake<float>(), nullptr, nullptr, fake<uint8_t>(), nullptr);
    };
    mg_maze_tasks F;
    std::memset(&F, 0, sizeof(F));
    F.n = 9; F.n_tasks = 2; F.start = F.goal = fake<int32_t>(); F.walls = fake<int8_t>(); F.texts = fake<uint8_t>(); F.scalars = fake<double>();
    EXPECT(step2d(nullptr, MG_MAZE_ESCAPE, 1, 4, &S), MG_ERR_NULL_POINTER);
    EXPECT(step2d(&F, MG_MAZE_ESCAPE, 1, 4, nullptr), MG_ERR_NULL_POINTER);
    for (int n : {2, 256, -1, 0}) {
        mg_maze_tasks t = F;
        t.n = n;
        EXPECT(step2d(&t, MG_MAZE_ESCAPE, 1, 4, &S), MG_ERR_BAD_SIZE);
    }
    for (int nt : {0, -4}) {
        mg_maze_tasks t = F;
        t.n_tasks = nt;
        EXPECT(step2d(&t, MG_MAZE_ESCAPE, 1, 4, &S), MG_ERR_BAD_SIZE);
    }
    for (int k = 0; k < 5; ++k) {                       // each required array of the table NULL in turn
        mg_maze_tasks t = F;
        const void **field[5] = {(const void **)&t.start, (const void **)&t.goal, (const void **)&t.walls, (const void **)&t.texts,
                                 (const void **)&t.scalars};
        *field[k] = nullptr;
        EXPECT(step2d(&t, MG_MAZE_ESCAPE, 1, 4, &S), MG_ERR_NULL_POINTER);
    }
    EXPECT(step2d(&F, MG_MAZE_SURVIVAL, 1, 4, &S), MG_ERR_NULL_POINTER);      // SURVIVAL needs the food arrays
    EXPECT(step2d(&F, 2, 1, 4, &S), MG_ERR_BAD_CONFIG);
    {
        mg_maze_tasks t = F;                               // int16 food lists on a table of more than 32 768 cells
        t.n = 182; t.food_cells = fake<int16_t>();
        EXPECT(step2d(&t, MG_MAZE_ESCAPE, 1, 4, &S), MG_ERR_BAD_SIZE);
    }
    for (int k = 0; k < 3; ++k) {                       // each required array of the state NULL in turn
        mg_maze_state s = S;
        void **field[3] = {(void **)&s.task_id, (void **)&s.grid, (void **)&s.steps};
        *field[k] = nullptr;
        EXPECT(step2d(&F, MG_MAZE_ESCAPE, 1, 4, &s), MG_ERR_NULL_POINTER);
    }
    // the 3-D renderer's record bound and LDS need, decided before anything runs (tests/test_maze_large.py)
    mg_maze_view V;
    std::memset(&V, 0, sizeof(V));
    V.res_h = 32; V.res_v = 4000; V.max_vision = 12.0; V.l_focal = 0.2; V.text_size = 1.0; V.tan_half_fov = std::tan(0.3 * 3.1415926);
    V.collision_dist = 0.2; V.col_cos = V.col_sin = fake<double>(); V.textures = V.ceil_texture = fake<uint32_t>(); V.n_textures = 7; V.tex_size = 64;
    S.ori_idx = fake<int32_t>(); S.ori = fake<double>(); S.loc = fake<float>();
    const int cases[][3] = {{63, 0, 0}, {64, 0, 1}, {65, 127, 0}, {65, 128, 1}, {101, 245, 1}, {101, 125, 0}, {255, 0, 1}, {255, 17, 0}};
    for (const auto &c : cases) {
        mg_maze_tasks t = F;
        t.n = c[0];
        V.max_ray_records = c[1];
        EXPECT(mg_maze3d_step(&t, &V, MG_MAZE_ESCAPE, 10, 0, 0, 4, &S, fake<int32_t>(), fake<int32_t>(), nullptr, nullptr, fake<uint8_t>(), nullptr),
               c[2] ? MG_ERR_UNSUPPORTED : MG_ERR_BAD_SIZE);
    }
    maze_launches(F, S, V);
}

// ---- walker --------------------------------------------------------------------------------------------------------------------

struct Walker {
    mg_walker_topology tp;
    mg_walker_models ms;
    mg_walker_params prm;
    mg_walker_state st;
    Walker(int nb, int nj, int ns, int nf, int ng, int np) {
        std::memset(&tp, 0, sizeof(tp)); std::memset(&ms, 0, sizeof(ms)); std::memset(&prm, 0, sizeof(prm)); std::memset(&st, 0, sizeof(st));
        tp.n_bodies = nb; tp.n_joints = nj; tp.n_spheres = ns; tp.n_feet = nf; tp.n_geoms = ng; tp.n_pairs = np;
        for (int b = 0; b < nb && b < MG_WALKER_MAX_BODIES; ++b) tp.body_parent[b] = b == 0 ? -1 : 0;
        for (int j = 0; j < nj && j < MG_WALKER_MAX_JOINTS; ++j) tp.joint_body[j] = nb > 1 ? 1 + j * (nb - 1) / (nj > 0 ? nj : 1) : 0;
        for (int g = 0; g < ns && g < MG_WALKER_MAX_SPHERES; ++g) tp.sphere_foot[g] = -1;
        ms.table = fake<double>(); ms.n_tasks = 1; ms.model_stride = 25 * nb + 12 * nj + 4 * ns + 7 * ng;
        prm.time_step = 0.005; prm.frame_skip = 4; prm.solver_iterations = 5; prm.mapping = 1;
        st.task_id = fake<int32_t>(); st.pos = st.rot = st.vel = st.omega = st.q = st.qd = st.potential = fake<double>();
        st.feet_contact = fake<float>(); st.steps = fake<int32_t>();
    }
    int step(int n = 4) {
        return mg_walker_step(&tp, &ms, &prm, n, &st, fake<float>(), fake<float>(), fake<float>(), nullptr, fake<uint8_t>(), nullptr);
    }
};

static void walker() {
    {   // tests/test_abi.py: 16 welded bodies overflow the wave mapping's assembly scratch; a body listed before its parent
        Walker w(16, 0, 0, 0, 0, 0);
        for (int b = 0; b < 16; ++b) w.tp.body_parent[b] = b - 1;
        EXPECT(w.step(), MG_ERR_UNSUPPORTED);
        EXPECT_TRUE(std::strstr(mg_last_error(), "mapping = lane") != nullptr);
        Walker v(3, 2, 0, 0, 0, 0);
        v.tp.body_parent[0] = -1; v.tp.body_parent[1] = 2; v.tp.body_parent[2] = 0;
        v.tp.joint_body[0] = 1; v.tp.joint_body[1] = 2;
        EXPECT(v.step(), MG_ERR_BAD_CONFIG);
        EXPECT_TRUE(std::strstr(mg_last_error(), "parents come first") != nullptr);
    }
    // every count one past its limit is a size error; AT its limit the range check passes and the next defect is reported
    // (a NULL state array, checked after the counts and the table)
    const int lim[6] = {MG_WALKER_MAX_BODIES, MG_WALKER_MAX_JOINTS, MG_WALKER_MAX_SPHERES, MG_WALKER_MAX_FEET, MG_WALKER_MAX_GEOMS, MG_WALKER_MAX_PAIRS};
    for (int k = 0; k < 6; ++k) {
        int n[6] = {2, 1, 1, 0, 0, 0};
        n[k] = lim[k];
        Walker at(n[0], n[1], n[2], n[3], n[4], n[5]);
        at.st.steps = nullptr;
        EXPECT(at.step(), MG_ERR_NULL_POINTER);
        n[k] = lim[k] + 1;
        Walker past(n[0], n[1], n[2], n[3], n[4], n[5]);
        EXPECT(past.step(), MG_ERR_BAD_SIZE);
        n[k] = -1;
        Walker neg(n[0], n[1], n[2], n[3], n[4], n[5]);
        EXPECT(neg.step(), MG_ERR_BAD_SIZE);
    }
    {
        Walker w(2, 1, 1, 0, 0, 0);
        EXPECT(w.step(0), MG_ERR_BAD_SIZE);
        EXPECT(mg_walker_step(nullptr, &w.ms, &w.prm, 4, &w.st, fake<float>(), fake<float>(), fake<float>(), nullptr, fake<uint8_t>(), nullptr), MG_ERR_NULL_POINTER);
        EXPECT(mg_walker_step(&w.tp, nullptr, &w.prm, 4, &w.st, fake<float>(), fake<float>(), fake<float>(), nullptr, fake<uint8_t>(), nullptr), MG_ERR_NULL_POINTER);
        EXPECT(mg_walker_step(&w.tp, &w.ms, nullptr, 4, &w.st, fake<float>(), fake<float>(), fake<float>(), nullptr, fake<uint8_t>(), nullptr), MG_ERR_NULL_POINTER);
        EXPECT(mg_walker_step(&w.tp, &w.ms, &w.prm, 4, nullptr, fake<float>(), fake<float>(), fake<float>(), nullptr, fake<uint8_t>(), nullptr), MG_ERR_NULL_POINTER);
        for (int k = 0; k < 10; ++k) {                  // each required state array NULL in turn
            Walker s(2, 1, 1, 0, 0, 0);
            void **field[10] = {(void **)&s.st.task_id, (void **)&s.st.pos, (void **)&s.st.rot, (void **)&s.st.vel, (void **)&s.st.omega,
                                (void **)&s.st.q, (void **)&s.st.qd, (void **)&s.st.potential, (void **)&s.st.feet_contact, (void **)&s.st.steps};
            *field[k] = nullptr;
            EXPECT(s.step(), MG_ERR_NULL_POINTER);
        }
        Walker t(2, 1, 1, 0, 0, 0);
        t.ms.model_stride -= 1;                            // a table row one double short
        EXPECT(t.step(), MG_ERR_BAD_SIZE);
        t.ms.model_stride += 1;
        t.prm.sphere_margin_in_table = 1;                  // ... and short of the margins the parameters announce
        EXPECT(t.step(), MG_ERR_BAD_SIZE);
        t.prm.sphere_margin_in_table = 0;
        t.ms.table = nullptr;
        EXPECT(t.step(), MG_ERR_BAD_SIZE);
        Walker p(2, 1, 1, 0, 0, 0);
        p.prm.time_step = 0.0;
        EXPECT(p.step(), MG_ERR_BAD_CONFIG);
        p.prm.time_step = NAN;
        EXPECT(p.step(), MG_ERR_BAD_CONFIG);
        p.prm.time_step = 0.005; p.prm.frame_skip = 0;
        EXPECT(p.step(), MG_ERR_BAD_CONFIG);
        // sphere_foot (ABI 4): a zero-initialised table on a robot without feet, and a foot on another body
        Walker f(2, 1, 1, 0, 0, 0);
        f.tp.sphere_foot[0] = 0;
        EXPECT(f.step(), MG_ERR_BAD_CONFIG);
        f.tp.n_feet = 1; f.tp.foot_body[0] = 1; f.tp.sphere_body[0] = 0;
        EXPECT(f.step(), MG_ERR_BAD_CONFIG);
        f.tp.sphere_foot[0] = -2;
        EXPECT(f.step(), MG_ERR_BAD_CONFIG);
        // terrain: a negative count, a NULL table, the lane mapping
        Walker r(2, 1, 1, 0, 0, 0);
        r.prm.n_terrain_boxes = -1;
        EXPECT(r.step(), MG_ERR_BAD_SIZE);
        r.prm.n_terrain_boxes = 3;
        EXPECT(r.step(), MG_ERR_NULL_POINTER);
        r.prm.terrain = fake<double>(); r.prm.mapping = 0;
        EXPECT(r.step(), MG_ERR_UNSUPPORTED);
        // rollouts: n_steps, obs_every, the lane mapping
        Walker o(2, 1, 1, 0, 0, 0);
        EXPECT(mg_walker_rollout(&o.tp, &o.ms, &o.prm, 4, &o.st, 0, 0, fake<float>(), fake<float>(), fake<float>(), nullptr, fake<uint8_t>(), nullptr), MG_ERR_BAD_SIZE);
        EXPECT(mg_walker_rollout(&o.tp, &o.ms, &o.prm, 4, &o.st, 2, -1, fake<float>(), fake<float>(), fake<float>(), nullptr, fake<uint8_t>(), nullptr), MG_ERR_BAD_SIZE);
        o.prm.mapping = 0;
        EXPECT(mg_walker_rollout(&o.tp, &o.ms, &o.prm, 4, &o.st, 2, 0, fake<float>(), fake<float>(), fake<float>(), nullptr, fake<uint8_t>(), nullptr), MG_ERR_UNSUPPORTED);
    }
}

// reset, the rollout's own pointers and the two closed-loop rollouts
static void walker_launches() {
    float *f = fake<float>();
    double *d = fake<double>();
    int32_t *i32 = fake<int32_t>();
    uint8_t *u = fake<uint8_t>();
    Walker w(2, 1, 1, 0, 0, 0), nosteps(2, 1, 1, 0, 0, 0), past(MG_WALKER_MAX_BODIES + 1, 1, 1, 0, 0, 0), notime(2, 1, 1, 0, 0, 0);
    nosteps.st.steps = nullptr;
    notime.prm.time_step = 0.0;
    EXPECT(mg_walker_reset(nullptr, &w.ms, &w.prm, 4, &w.st, nullptr, nullptr, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_walker_reset(&w.tp, nullptr, &w.prm, 4, &w.st, nullptr, nullptr, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_walker_reset(&w.tp, &w.ms, nullptr, 4, &w.st, nullptr, nullptr, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_walker_reset(&w.tp, &w.ms, &w.prm, 4, nullptr, nullptr, nullptr, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_walker_reset(&w.tp, &w.ms, &w.prm, 0, &w.st, nullptr, nullptr, nullptr, nullptr), MG_ERR_BAD_SIZE);
    EXPECT(mg_walker_reset(&w.tp, &w.ms, &w.prm, 4, &nosteps.st, nullptr, nullptr, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_walker_reset(&past.tp, &past.ms, &past.prm, 4, &past.st, nullptr, nullptr, nullptr, nullptr), MG_ERR_BAD_SIZE);
    EXPECT(mg_walker_reset(&w.tp, &w.ms, &notime.prm, 4, &w.st, nullptr, nullptr, nullptr, nullptr), MG_ERR_BAD_CONFIG);
    // the step's outputs and its in-launch actuators
    EXPECT(mg_walker_step(&w.tp, &w.ms, &w.prm, 4, &w.st, nullptr, f, f, nullptr, u, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_walker_step(&w.tp, &w.ms, &w.prm, 4, &w.st, f, nullptr, f, nullptr, u, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_walker_step(&w.tp, &w.ms, &w.prm, 4, &w.st, f, f, nullptr, nullptr, u, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_walker_step(&w.tp, &w.ms, &w.prm, 4, &w.st, f, f, f, nullptr, nullptr, nullptr), MG_ERR_NULL_POINTER);
    {
        Walker a(2, 1, 1, 0, 0, 0);
        a.prm.actuation = 5;
        EXPECT(a.step(), MG_ERR_BAD_CONFIG);
        a.prm.actuation = 1;
        EXPECT(a.step(), MG_ERR_NULL_POINTER);             // no pd_command
        a.prm.mapping = 0;
        EXPECT(a.step(), MG_ERR_UNSUPPORTED);
    }
    // the rollout
    auto roll = [&](Walker &x, int n, int steps, int every, const float *act, float *obs, float *rew, uint8_t *done) {
        return mg_walker_rollout(&x.tp, &x.ms, &x.prm, n, &x.st, steps, every, act, obs, rew, nullptr, done, nullptr);
    };
    EXPECT(mg_walker_rollout(nullptr, &w.ms, &w.prm, 4, &w.st, 2, 0, f, f, f, nullptr, u, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_walker_rollout(&w.tp, nullptr, &w.prm, 4, &w.st, 2, 0, f, f, f, nullptr, u, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_walker_rollout(&w.tp, &w.ms, nullptr, 4, &w.st, 2, 0, f, f, f, nullptr, u, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_walker_rollout(&w.tp, &w.ms, &w.prm, 4, nullptr, 2, 0, f, f, f, nullptr, u, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(roll(w, 4, 2, 0, nullptr, f, f, u), MG_ERR_NULL_POINTER);
    EXPECT(roll(w, 4, 2, 0, f, nullptr, f, u), MG_ERR_NULL_POINTER);
    EXPECT(roll(w, 4, 2, 0, f, f, nullptr, u), MG_ERR_NULL_POINTER);
    EXPECT(roll(w, 4, 2, 0, f, f, f, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(roll(w, 0, 2, 0, f, f, f, u), MG_ERR_BAD_SIZE);
    EXPECT(roll(nosteps, 4, 2, 0, f, f, f, u), MG_ERR_NULL_POINTER);
    EXPECT(roll(past, 4, 2, 0, f, f, f, u), MG_ERR_BAD_SIZE);
    {
        Walker a(2, 1, 1, 0, 0, 0);
        a.prm.actuation = 1; a.prm.pd_command = d;
        EXPECT(roll(a, 4, 2, 0, f, f, f, u), MG_ERR_UNSUPPORTED);
        Walker l(2, 1, 1, 0, 0, 0);
        l.prm.substep_log = d;
        EXPECT(roll(l, 4, 2, 0, f, f, f, u), MG_ERR_BAD_CONFIG);
    }
    // closed-loop rollouts, feed-forward and recurrent; the robot has one joint and no foot: D = 10, A = 1
    mg_walker_policy pol;
    std::memset(&pol, 0, sizeof(pol));
    pol.params_d = f; pol.policy_id_d = i32; pol.n_policies = 2; pol.hidden = 8; pol.obs_dim = 10; pol.n_act = 1;
    mg_walker_rpolicy_carry carry;
    carry.h = f; carry.prev_action = f; carry.prev_reward = f; carry.prev_done = u;
    for (int rec = 0; rec < 2; ++rec) {
        auto proll = [&](Walker &x, int n, int steps, int every, const mg_walker_policy *p, const mg_walker_rpolicy_carry *c, int episodic,
                         const float *obs0, float *obs, double *rt, double *re, int32_t *el) {
            return rec ? mg_walker_rpolicy_rollout(&x.tp, &x.ms, &x.prm, n, &x.st, steps, every, p, c, episodic, obs0, obs, rt, re, el, nullptr,
                                                   nullptr, nullptr, nullptr, nullptr)
                       : mg_walker_policy_rollout(&x.tp, &x.ms, &x.prm, n, &x.st, steps, every, p, obs0, obs, rt, re, el, nullptr, nullptr, nullptr,
                                                  nullptr, nullptr);
        };
        EXPECT(proll(w, 4, 2, 0, nullptr, &carry, 0, f, f, d, d, i32), MG_ERR_NULL_POINTER);
        EXPECT(proll(w, 4, 2, 0, &pol, &carry, 0, nullptr, f, d, d, i32), MG_ERR_NULL_POINTER);
        EXPECT(proll(w, 4, 2, 0, &pol, &carry, 0, f, nullptr, d, d, i32), MG_ERR_NULL_POINTER);
        EXPECT(proll(w, 4, 2, 0, &pol, &carry, 0, f, f, nullptr, d, i32), MG_ERR_NULL_POINTER);
        EXPECT(proll(w, 4, 2, 0, &pol, &carry, 0, f, f, d, nullptr, i32), MG_ERR_NULL_POINTER);
        EXPECT(proll(w, 4, 2, 0, &pol, &carry, 0, f, f, d, d, nullptr), MG_ERR_NULL_POINTER);
        EXPECT(proll(w, 0, 2, 0, &pol, &carry, 0, f, f, d, d, i32), MG_ERR_BAD_SIZE);
        EXPECT(proll(w, 4, 0, 0, &pol, &carry, 0, f, f, d, d, i32), MG_ERR_BAD_SIZE);
        EXPECT(proll(w, 4, 2, -1, &pol, &carry, 0, f, f, d, d, i32), MG_ERR_BAD_SIZE);
        EXPECT(proll(nosteps, 4, 2, 0, &pol, &carry, 0, f, f, d, d, i32), MG_ERR_NULL_POINTER);
        EXPECT(proll(past, 4, 2, 0, &pol, &carry, 0, f, f, d, d, i32), MG_ERR_BAD_SIZE);
        {
            Walker l(2, 1, 1, 0, 0, 0);
            l.prm.mapping = 0;
            EXPECT(proll(l, 4, 2, 0, &pol, &carry, 0, f, f, d, d, i32), MG_ERR_UNSUPPORTED);
            Walker a(2, 1, 1, 0, 0, 0);
            a.prm.actuation = 1; a.prm.pd_command = d;
            EXPECT(proll(a, 4, 2, 0, &pol, &carry, 0, f, f, d, d, i32), MG_ERR_UNSUPPORTED);
            Walker g(2, 1, 1, 0, 0, 0);
            g.prm.substep_log = d;
            EXPECT(proll(g, 4, 2, 0, &pol, &carry, 0, f, f, d, d, i32), MG_ERR_BAD_CONFIG);
            mg_walker_policy p = pol;
            p.params_d = nullptr;
            EXPECT(proll(w, 4, 2, 0, &p, &carry, 0, f, f, d, d, i32), MG_ERR_NULL_POINTER);
            p = pol; p.policy_id_d = nullptr;
            EXPECT(proll(w, 4, 2, 0, &p, &carry, 0, f, f, d, d, i32), MG_ERR_NULL_POINTER);
            p = pol; p.n_policies = 0;
            EXPECT(proll(w, 4, 2, 0, &p, &carry, 0, f, f, d, d, i32), MG_ERR_BAD_SIZE);
            p = pol; p.hidden = 257;                        // one past the supported path
            EXPECT(proll(w, 4, 2, 0, &p, &carry, 0, f, f, d, d, i32), MG_ERR_BAD_SIZE);
            p = pol; p.hidden = rec ? 0 : -1;
            EXPECT(proll(w, 4, 2, 0, &p, &carry, 0, f, f, d, d, i32), MG_ERR_BAD_SIZE);
            p = pol; p.obs_dim = 11;
            EXPECT(proll(w, 4, 2, 0, &p, &carry, 0, f, f, d, d, i32), MG_ERR_BAD_CONFIG);
            p = pol; p.n_act = 2;
            EXPECT(proll(w, 4, 2, 0, &p, &carry, 0, f, f, d, d, i32), MG_ERR_BAD_CONFIG);
        }
        if (rec) {
            EXPECT(proll(w, 4, 2, 0, &pol, nullptr, 0, f, f, d, d, i32), MG_ERR_NULL_POINTER);
            for (int k = 0; k < 4; ++k) {
                mg_walker_rpolicy_carry c = carry;
                void **field[4] = {(void **)&c.h, (void **)&c.prev_action, (void **)&c.prev_reward, (void **)&c.prev_done};
                *field[k] = nullptr;
                EXPECT(proll(w, 4, 2, 0, &pol, &c, 0, f, f, d, d, i32), MG_ERR_NULL_POINTER);
            }
            EXPECT(proll(w, 4, 2, 0, &pol, &carry, 1, f, f, d, d, i32), MG_ERR_BAD_CONFIG);      // episodic without auto_reset
        }
    }
}

// ---- A1 ------------------------------------------------------------------------------------------------------------------------

static void a1() {
    double *d = fake<double>();
    int32_t *i32 = fake<int32_t>();
    uint8_t *u = fake<uint8_t>();
    mg_a1_actuator_config cfg;
    std::memset(&cfg, 0, sizeof(cfg));
    cfg.time_step = 0.002; cfg.action_repeat = 13; cfg.history_len = 100; cfg.mode = MG_A1_MODE_POSITION; cfg.max_angle_change = 0.2;
    mg_a1_actuator_state st;
    st.history = d; st.count = i32; st.head = i32; st.observed_torque = d; st.control_obs = d;
    // what every actuator entry point refuses about its descriptors, entry point by entry point
    typedef int (*Call)(const mg_a1_actuator_config *, int32_t, const mg_a1_actuator_state *);
    const Call calls[] = {
        [](const mg_a1_actuator_config *c, int32_t n, const mg_a1_actuator_state *s) {
            return mg_a1_apply_action(c, n, s, fake<double>(), nullptr, 1.0, fake<double>(), nullptr); },
        [](const mg_a1_actuator_config *c, int32_t n, const mg_a1_actuator_state *s) {
            return mg_a1_receive_observation(c, n, s, fake<double>(), fake<double>(), fake<double>(), fake<double>(), nullptr, nullptr); },
        [](const mg_a1_actuator_config *c, int32_t n, const mg_a1_actuator_state *s) {
            return mg_a1_receive_and_apply(c, n, s, fake<double>(), fake<double>(), fake<double>(), fake<double>(), fake<double>(), nullptr, 1.0,
                                           fake<double>(), nullptr); },
        [](const mg_a1_actuator_config *c, int32_t n, const mg_a1_actuator_state *s) { return mg_a1_receive_log(c, n, s, fake<double>(), 13, nullptr); },
        [](const mg_a1_actuator_config *c, int32_t n, const mg_a1_actuator_state *s) {
            return mg_a1_sensors(c, n, s, fake<double>(), nullptr, nullptr, nullptr, nullptr, nullptr); },
        [](const mg_a1_actuator_config *c, int32_t n, const mg_a1_actuator_state *s) {
            return mg_a1_info(c, n, s, fake<double>(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr); },
    };
    for (Call call : calls) {
        EXPECT(call(nullptr, 4, &st), MG_ERR_NULL_POINTER);
        EXPECT(call(&cfg, 4, nullptr), MG_ERR_NULL_POINTER);
        EXPECT(call(&cfg, 0, &st), MG_ERR_BAD_SIZE);
        for (int k = 0; k < 5; ++k) {
            mg_a1_actuator_config c = cfg;
            switch (k) {
            case 0: c.time_step = 0.0; break;
            case 1: c.action_repeat = 0; break;
            case 2: c.history_len = 1; break;
            case 3: c.mode = 0; break;
            default: c.mode = 4; break;                   // PWM
            }
            EXPECT(call(&c, 4, &st), MG_ERR_BAD_CONFIG);
            mg_a1_actuator_state s = st;
            void **field[5] = {(void **)&s.history, (void **)&s.count, (void **)&s.head, (void **)&s.observed_torque, (void **)&s.control_obs};
            *field[k] = nullptr;
            EXPECT(call(&cfg, 4, &s), MG_ERR_NULL_POINTER);
        }
    }
    EXPECT(mg_a1_apply_action(&cfg, 4, &st, nullptr, nullptr, 1.0, d, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_a1_apply_action(&cfg, 4, &st, d, nullptr, 1.0, nullptr, nullptr), MG_ERR_NULL_POINTER);
    for (int k = 0; k < 4; ++k) {
        const double *a[4] = {d, d, d, d};
        a[k] = nullptr;
        EXPECT(mg_a1_receive_observation(&cfg, 4, &st, a[0], a[1], a[2], a[3], nullptr, nullptr), MG_ERR_NULL_POINTER);
        EXPECT(mg_a1_receive_and_apply(&cfg, 4, &st, a[0], a[1], a[2], a[3], d, nullptr, 1.0, d, nullptr), MG_ERR_NULL_POINTER);
    }
    EXPECT(mg_a1_receive_and_apply(&cfg, 4, &st, d, d, d, d, nullptr, nullptr, 1.0, d, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_a1_receive_and_apply(&cfg, 4, &st, d, d, d, d, d, nullptr, 1.0, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_a1_receive_log(&cfg, 4, &st, nullptr, 13, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_a1_receive_log(&cfg, 4, &st, d, 0, nullptr), MG_ERR_BAD_SIZE);
    // the trajectory generator
    mg_a1_etg_config etg;
    std::memset(&etg, 0, sizeof(etg));
    etg.enabled = 1; etg.H = 20; etg.T = 0.5; etg.T2_ratio = 0.5; etg.sigma_sq = 0.04; etg.amp = 0.2; etg.etg_weight = 1.0;
    EXPECT(mg_a1_etg_action(nullptr, 4, d, d, d, d, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_a1_etg_action(&etg, 0, d, d, d, d, nullptr, nullptr), MG_ERR_BAD_SIZE);
    EXPECT(mg_a1_etg_action(&etg, 4, nullptr, d, d, d, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_a1_etg_action(&etg, 4, d, d, d, nullptr, nullptr, nullptr), MG_ERR_NULL_POINTER);
    {
        mg_a1_etg_config c = etg;
        c.H = MG_A1_ETG_MAX_H + 1;
        EXPECT(mg_a1_etg_action(&c, 4, d, d, d, d, nullptr, nullptr), MG_ERR_BAD_CONFIG);
        c = etg; c.sigma_sq = 0.0;
        EXPECT(mg_a1_etg_action(&c, 4, d, d, d, d, nullptr, nullptr), MG_ERR_BAD_CONFIG);
        c = etg; c.action_space = 4;
        EXPECT(mg_a1_etg_action(&c, 4, d, d, d, d, nullptr, nullptr), MG_ERR_BAD_CONFIG);
        c = etg; c.action_space = -1;
        EXPECT(mg_a1_etg_action(&c, 4, d, d, d, d, nullptr, nullptr), MG_ERR_BAD_CONFIG);
    }
    // reward shaping
    mg_a1_reward_config rc;
    std::memset(&rc, 0, sizeof(rc));
    rc.n_segments = 1;
    mg_a1_reward_state rs;
    rs.last_base = rs.last_base10 = rs.last_foot = rs.vd2 = d; rs.steps = i32;
    auto rstep = [&](const mg_a1_reward_config *c, int n, const mg_a1_reward_state *s, int null_at) {
        const void *a[9] = {d, d, d, d, d, d, i32, d, u};
        if (null_at >= 0) a[null_at] = nullptr;
        return mg_a1_reward_step(c, n, s, (const double *)a[0], (const double *)a[1], (const double *)a[2], (const double *)a[3], (const double *)a[4],
                                 (const double *)a[5], (const int32_t *)a[6], nullptr, nullptr, (double *)a[7], (uint8_t *)a[8], nullptr);
    };
    auto rreset = [&](const mg_a1_reward_config *c, int n, const mg_a1_reward_state *s, int null_at) {
        const double *a[3] = {d, d, d};
        if (null_at >= 0) a[null_at] = nullptr;
        return mg_a1_reward_reset(c, n, s, a[0], a[1], a[2], nullptr, nullptr);
    };
    for (int k = 0; k < 9; ++k) EXPECT(rstep(&rc, 4, &rs, k), MG_ERR_NULL_POINTER);
    for (int k = 0; k < 3; ++k) EXPECT(rreset(&rc, 4, &rs, k), MG_ERR_NULL_POINTER);
    for (int step = 0; step < 2; ++step) {
        auto call = [&](const mg_a1_reward_config *c, int n, const mg_a1_reward_state *s) { return step ? rstep(c, n, s, -1) : rreset(c, n, s, -1); };
        EXPECT(call(nullptr, 4, &rs), MG_ERR_NULL_POINTER);
        EXPECT(call(&rc, 4, nullptr), MG_ERR_NULL_POINTER);
        EXPECT(call(&rc, 0, &rs), MG_ERR_BAD_SIZE);
        mg_a1_reward_config c = rc;
        c.n_segments = MG_A1_MAX_SEGMENTS + 1;
        EXPECT(call(&c, 4, &rs), MG_ERR_BAD_SIZE);
        c.n_segments = -1;
        EXPECT(call(&c, 4, &rs), MG_ERR_BAD_SIZE);
        for (int k = 0; k < 5; ++k) {
            mg_a1_reward_state s = rs;
            void **field[5] = {(void **)&s.last_base, (void **)&s.last_base10, (void **)&s.last_foot, (void **)&s.vd2, (void **)&s.steps};
            *field[k] = nullptr;
            EXPECT(call(&rc, 4, &s), MG_ERR_NULL_POINTER);
        }
    }
    // the sensor stack
    mg_a1_sensor_config sc;
    std::memset(&sc, 0, sizeof(sc));
    sc.normal = 1; sc.disp_dt = 0.026; sc.motor_dt = 0.026;
    mg_a1_sensor_state ss;
    std::memset(&ss, 0, sizeof(ss));
    ss.base_last = ss.base_cur = ss.yaw = ss.first_rpy = ss.last_angle = d; ss.first = i32;
    auto observe = [&](const mg_a1_sensor_config *c, int n, const mg_a1_sensor_state *s, int null_at) {
        double *a[6] = {d, d, d, d, d, d};
        if (null_at >= 0) a[null_at] = nullptr;
        return mg_a1_observation(c, n, s, a[0], a[1], a[2], a[3], a[4], nullptr, a[5], nullptr);
    };
    EXPECT(observe(nullptr, 4, &ss, -1), MG_ERR_NULL_POINTER);
    EXPECT(observe(&sc, 4, nullptr, -1), MG_ERR_NULL_POINTER);
    EXPECT(observe(&sc, 0, &ss, -1), MG_ERR_BAD_SIZE);
    for (int k = 0; k < 6; ++k) {
        EXPECT(observe(&sc, 4, &ss, k), MG_ERR_NULL_POINTER);
        mg_a1_sensor_state s = ss;
        void **field[6] = {(void **)&s.base_last, (void **)&s.base_cur, (void **)&s.yaw, (void **)&s.first_rpy, (void **)&s.last_angle, (void **)&s.first};
        *field[k] = nullptr;
        EXPECT(observe(&sc, 4, &s, -1), MG_ERR_NULL_POINTER);
    }
    {
        mg_a1_sensor_config c = sc;
        c.disp_dt = 0.0;
        EXPECT(observe(&c, 4, &ss, -1), MG_ERR_BAD_CONFIG);
        c = sc; c.motor_dt = NAN;
        EXPECT(observe(&c, 4, &ss, -1), MG_ERR_BAD_CONFIG);
    }
    const int all = MG_A1_EXTRA_ETG | MG_A1_EXTRA_ETG_OBS | MG_A1_EXTRA_YAW;
    EXPECT(mg_a1_observation_extras(0, all, 1, 20, d, d, d, nullptr, d, nullptr), MG_ERR_BAD_SIZE);
    EXPECT(mg_a1_observation_extras(4, 8, 1, 20, d, d, d, nullptr, d, nullptr), MG_ERR_BAD_CONFIG);
    EXPECT(mg_a1_observation_extras(4, all, 1, 0, d, d, d, nullptr, d, nullptr), MG_ERR_BAD_SIZE);
    EXPECT(mg_a1_observation_extras(4, all, 1, MG_A1_ETG_MAX_H + 1, d, d, d, nullptr, d, nullptr), MG_ERR_BAD_SIZE);
    EXPECT(mg_a1_observation_extras(4, all, 1, 20, nullptr, d, d, nullptr, d, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_a1_observation_extras(4, all, 1, 20, d, nullptr, d, nullptr, d, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_a1_observation_extras(4, all, 1, 20, d, d, nullptr, nullptr, d, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_a1_observation_extras(4, all, 1, 20, d, d, d, nullptr, nullptr, nullptr), MG_ERR_NULL_POINTER);
    // the action filter
    mg_a1_filter_config fc;
    std::memset(&fc, 0, sizeof(fc));
    fc.hist_len = 2;
    EXPECT(mg_a1_action_filter(nullptr, 4, d, d, d, d, nullptr, 0, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_a1_action_filter(&fc, 0, d, d, d, d, nullptr, 0, nullptr), MG_ERR_BAD_SIZE);
    EXPECT(mg_a1_action_filter(&fc, 4, nullptr, d, d, d, nullptr, 0, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_a1_action_filter(&fc, 4, d, nullptr, d, d, nullptr, 0, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_a1_action_filter(&fc, 4, d, d, nullptr, d, nullptr, 0, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_a1_action_filter(&fc, 4, d, d, d, nullptr, nullptr, 0, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_a1_action_filter(&fc, 4, nullptr, d, nullptr, nullptr, nullptr, 1, nullptr), MG_ERR_NULL_POINTER);
    for (int h : {0, MG_A1_FILTER_MAX_HIST + 1}) {
        mg_a1_filter_config c = fc;
        c.hist_len = h;
        EXPECT(mg_a1_action_filter(&c, 4, d, d, d, d, nullptr, 0, nullptr), MG_ERR_BAD_CONFIG);
    }
}

// ---- MetaLM --------------------------------------------------------------------------------------------------------------------

static void metalm() {
    int32_t *i32 = fake<int32_t>();
    uint32_t *u32 = fake<uint32_t>();
    mg_metalm_params p;
    p.V = 64; p.n = 10; p.L = 4096; p.l = 3.0; p.e = 0.1; p.mask_ratio = 0.3;
    auto gen = [&](const mg_metalm_params *q, int batch, const uint32_t *seeds, uint32_t *mt, int cap, int32_t *feat, int32_t *lab, int32_t *ovf) {
        return mg_metalm_generate(q, batch, 1u, seeds, mt, cap, feat, lab, ovf, nullptr);
    };
    EXPECT(gen(nullptr, 4, nullptr, nullptr, 64, i32, i32, i32), MG_ERR_NULL_POINTER);
    EXPECT(gen(&p, 4, nullptr, nullptr, 64, nullptr, i32, i32), MG_ERR_NULL_POINTER);
    EXPECT(gen(&p, 4, nullptr, nullptr, 64, i32, nullptr, i32), MG_ERR_NULL_POINTER);
    EXPECT(gen(&p, 4, nullptr, nullptr, 64, i32, i32, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(gen(&p, 0, nullptr, nullptr, 64, i32, i32, i32), MG_ERR_BAD_SIZE);
    EXPECT(gen(&p, 4, nullptr, nullptr, 3 * p.n - 1, i32, i32, i32), MG_ERR_BAD_SIZE);
    EXPECT(gen(&p, 4, nullptr, nullptr, (160 * 1024 - 2496) / 8 - p.n + 1, i32, i32, i32), MG_ERR_UNSUPPORTED);      // one token past 160 KiB of LDS
    EXPECT(gen(&p, 4, u32, u32, 64, i32, i32, i32), MG_ERR_BAD_CONFIG);                      // seeded and chained at once
    for (int k = 0; k < 10; ++k) {                      // the reference's asserts
        mg_metalm_params q = p;
        switch (k) {
        case 0: q.n = 1; break;
        case 1: q.V = 1; break;
        case 2: q.l = 1.0; break;
        case 3: q.l = INFINITY; break;
        case 4: q.e = 0.0; break;
        case 5: q.e = 1.0; break;
        case 6: q.L = 1; break;
        case 7: q.V = INT32_MAX; break;
        case 8: q.l = NAN; break;
        default: q.mask_ratio = NAN; break;
        }
        EXPECT(gen(&q, 4, nullptr, nullptr, 64, i32, i32, i32), MG_ERR_BAD_CONFIG);
    }
}

// ---- bandits -------------------------------------------------------------------------------------------------------------------

static void bandits() {
    int32_t *i32 = fake<int32_t>();
    float *f = fake<float>();
    double *d = fake<double>();
    uint8_t *u = fake<uint8_t>();
    mg_bandits_config cfg;
    std::memset(&cfg, 0, sizeof(cfg));
    cfg.arms = 10; cfg.max_steps = 100; cfg.distribution = MG_BANDITS_CLASSICAL; cfg.mean = 0.5; cfg.dev = 0.1;
    mg_bandits_state st;
    st.mt = fake<uint32_t>(); st.has_gauss = i32; st.gauss = d; st.gains = d; st.steps = i32; st.over = u;
    const mg_bandits_config bad[] = {[&] { auto c = cfg; c.arms = 1; return c; }(), [&] { auto c = cfg; c.max_steps = 1; return c; }(),
                                     [&] { auto c = cfg; c.distribution = 4; return c; }(), [&] { auto c = cfg; c.distribution = -1; return c; }()};
    auto state_without = [&](int k) {
        mg_bandits_state s = st;
        void **field[6] = {(void **)&s.mt, (void **)&s.has_gauss, (void **)&s.gauss, (void **)&s.gains, (void **)&s.steps, (void **)&s.over};
        *field[k] = nullptr;
        return s;
    };
    EXPECT(mg_bandits_seed(4, 1u, nullptr, nullptr, nullptr), MG_ERR_NULL_POINTER);
    for (int k = 0; k < 3; ++k) {                       // seeding touches only the stream record
        const mg_bandits_state s = state_without(k);
        EXPECT(mg_bandits_seed(4, 1u, nullptr, &s, nullptr), MG_ERR_NULL_POINTER);
    }
    EXPECT(mg_bandits_seed(0, 1u, nullptr, &st, nullptr), MG_ERR_BAD_SIZE);
    // what every other entry point refuses about the config and the state
    typedef int (*Call)(const mg_bandits_config *, int32_t, const mg_bandits_state *);
    static const mg_maze_policy_carry carry = {fake<float>(), fake<int32_t>(), fake<float>(), fake<uint8_t>()};
    static const mg_bandits_learner_carry lcarry = {fake<int32_t>(), fake<int32_t>()};
    static mg_bandits_policy pol;
    pol.params = f; pol.eps_threshold = nullptr; pol.n_policies = 2; pol.hidden = 8; pol.arms = 10;
    static mg_bandits_learner lrn;
    std::memset(&lrn, 0, sizeof(lrn));
    lrn.kind = MG_BANDITS_LEARNER_UCB; lrn.n_learners = 2; lrn.arms = 10; lrn.params = f;
    const Call calls[] = {
        [](const mg_bandits_config *c, int32_t n, const mg_bandits_state *s) { return mg_bandits_sample_task(c, n, s, nullptr, fake<double>(), nullptr); },
        [](const mg_bandits_config *c, int32_t n, const mg_bandits_state *s) { return mg_bandits_reset(c, n, s, nullptr, nullptr); },
        [](const mg_bandits_config *c, int32_t n, const mg_bandits_state *s) {
            return mg_bandits_step(c, n, s, 3, fake<int32_t>(), fake<float>(), fake<uint8_t>(), fake<int32_t>(), fake<double>(), fake<uint8_t>(), nullptr); },
        [](const mg_bandits_config *c, int32_t n, const mg_bandits_state *s) {
            return mg_bandits_policy_rollout(c, n, s, 3, &pol, fake<int32_t>(), &carry, 1u, 0u, 0, fake<double>(), fake<double>(), fake<int32_t>(),
                                             fake<int32_t>(), fake<double>(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr); },
        [](const mg_bandits_config *c, int32_t n, const mg_bandits_state *s) {
            return mg_bandits_learner_rollout(c, n, s, 3, &lrn, fake<int32_t>(), &lcarry, 1u, 0u, 0, fake<double>(), fake<double>(), fake<int32_t>(),
                                              fake<int32_t>(), fake<double>(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr); },
    };
    for (Call call : calls) {
        EXPECT(call(nullptr, 4, &st), MG_ERR_NULL_POINTER);
        EXPECT(call(&cfg, 4, nullptr), MG_ERR_NULL_POINTER);
        EXPECT(call(&cfg, 0, &st), MG_ERR_BAD_SIZE);
        for (int k = 0; k < 6; ++k) {
            const mg_bandits_state s = state_without(k);
            EXPECT(call(&cfg, 4, &s), MG_ERR_NULL_POINTER);
        }
        for (const mg_bandits_config &c : bad) EXPECT(call(&c, 4, &st), MG_ERR_BAD_CONFIG);
    }
    {
        mg_bandits_config c = cfg;
        c.distribution = MG_BANDITS_NONE;
        EXPECT(mg_bandits_sample_task(&c, 4, &st, nullptr, d, nullptr), MG_ERR_BAD_CONFIG);
        EXPECT(mg_bandits_sample_task(&cfg, 4, &st, nullptr, nullptr, nullptr), MG_ERR_NULL_POINTER);
    }
    for (int k = 0; k < 6; ++k) {                       // each output of the step
        const void *a[6] = {i32, f, u, i32, d, u};
        a[k] = nullptr;
        EXPECT(mg_bandits_step(&cfg, 4, &st, 3, (const int32_t *)a[0], (float *)a[1], (uint8_t *)a[2], (int32_t *)a[3], (double *)a[4], (uint8_t *)a[5],
                               nullptr), MG_ERR_NULL_POINTER);
    }
    EXPECT(mg_bandits_step(&cfg, 4, &st, 0, i32, f, u, i32, d, u, nullptr), MG_ERR_BAD_SIZE);
    // the recurrent policies and the learners
    for (int learner = 0; learner < 2; ++learner) {
        auto roll = [&](int steps, const void *p, const int32_t *ids, const void *c, double *rt, double *re, int32_t *el, int32_t *ep, double *rg) {
            return learner ? mg_bandits_learner_rollout(&cfg, 4, &st, steps, (const mg_bandits_learner *)p, ids, (const mg_bandits_learner_carry *)c, 1u,
                                                        0u, 0, rt, re, el, ep, rg, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)
                           : mg_bandits_policy_rollout(&cfg, 4, &st, steps, (const mg_bandits_policy *)p, ids, (const mg_bandits_policy_carry *)c, 1u, 0u,
                                                       0, rt, re, el, ep, rg, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
        };
        const void *p = learner ? (const void *)&lrn : (const void *)&pol, *c = learner ? (const void *)&lcarry : (const void *)&carry;
        EXPECT(roll(3, nullptr, i32, c, d, d, i32, i32, d), MG_ERR_NULL_POINTER);
        EXPECT(roll(3, p, nullptr, c, d, d, i32, i32, d), MG_ERR_NULL_POINTER);
        EXPECT(roll(3, p, i32, nullptr, d, d, i32, i32, d), MG_ERR_NULL_POINTER);
        EXPECT(roll(3, p, i32, c, nullptr, d, i32, i32, d), MG_ERR_NULL_POINTER);
        EXPECT(roll(3, p, i32, c, d, nullptr, i32, i32, d), MG_ERR_NULL_POINTER);
        EXPECT(roll(3, p, i32, c, d, d, nullptr, i32, d), MG_ERR_NULL_POINTER);
        EXPECT(roll(3, p, i32, c, d, d, i32, nullptr, d), MG_ERR_NULL_POINTER);
        EXPECT(roll(3, p, i32, c, d, d, i32, i32, nullptr), MG_ERR_NULL_POINTER);
        EXPECT(roll(0, p, i32, c, d, d, i32, i32, d), MG_ERR_BAD_SIZE);
    }
    auto proll = [&](const mg_bandits_policy *p, const mg_bandits_policy_carry *c) {
        return mg_bandits_policy_rollout(&cfg, 4, &st, 3, p, i32, c, 1u, 0u, 0, d, d, i32, i32, d, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                         nullptr, nullptr);
    };
    for (int k = 0; k < 4; ++k) {
        mg_bandits_policy_carry c = carry;
        void **field[4] = {(void **)&c.h, (void **)&c.prev_action, (void **)&c.prev_reward, (void **)&c.prev_done};
        *field[k] = nullptr;
        EXPECT(proll(&pol, &c), MG_ERR_NULL_POINTER);
    }
    {
        mg_bandits_policy p = pol;
        p.params = nullptr;
        EXPECT(proll(&p, &carry), MG_ERR_NULL_POINTER);
        p = pol; p.params = f + 1;
        EXPECT(proll(&p, &carry), MG_ERR_BAD_CONFIG);
        p = pol; p.n_policies = 0;
        EXPECT(proll(&p, &carry), MG_ERR_BAD_SIZE);
        p = pol; p.hidden = 0;
        EXPECT(proll(&p, &carry), MG_ERR_BAD_SIZE);
        p = pol; p.hidden = 65;                             // one past the supported path
        EXPECT(proll(&p, &carry), MG_ERR_BAD_SIZE);
        p = pol; p.arms = 65;                               // 65 arms
        EXPECT(proll(&p, &carry), MG_ERR_BAD_SIZE);
        p = pol; p.arms = 1;
        EXPECT(proll(&p, &carry), MG_ERR_BAD_SIZE);
        p = pol; p.arms = 11;                               // not the env's
        EXPECT(proll(&p, &carry), MG_ERR_BAD_CONFIG);
    }
    for (int scores = 0; scores < 2; ++scores) {
        auto call = [&](const mg_bandits_learner *l, const mg_bandits_learner_carry *c) {
            return scores ? mg_bandits_learner_scores(4, l, i32, c, 1u, 0u, f, nullptr, nullptr)
                          : mg_bandits_learner_rollout(&cfg, 4, &st, 3, l, i32, c, 1u, 0u, 0, d, d, i32, i32, d, nullptr, nullptr, nullptr, nullptr,
                                                       nullptr, nullptr, nullptr, nullptr);
        };
        mg_bandits_learner_carry c = lcarry;
        c.pulls = nullptr;
        EXPECT(call(&lrn, &c), MG_ERR_NULL_POINTER);
        c = lcarry; c.wins = nullptr;
        EXPECT(call(&lrn, &c), MG_ERR_NULL_POINTER);
        mg_bandits_learner l = lrn;
        l.kind = 4;
        EXPECT(call(&l, &lcarry), MG_ERR_BAD_CONFIG);
        l.kind = -1;
        EXPECT(call(&l, &lcarry), MG_ERR_BAD_CONFIG);
        l = lrn; l.params = nullptr;
        EXPECT(call(&l, &lcarry), MG_ERR_NULL_POINTER);
        l = lrn; l.n_learners = 0;
        EXPECT(call(&l, &lcarry), MG_ERR_BAD_SIZE);
        l = lrn; l.arms = 65;
        EXPECT(call(&l, &lcarry), MG_ERR_BAD_SIZE);
        l = lrn; l.arms = 1;
        EXPECT(call(&l, &lcarry), MG_ERR_BAD_SIZE);
        l = lrn; l.kind = MG_BANDITS_LEARNER_TABLE; l.table_cap = 8;
        EXPECT(call(&l, &lcarry), MG_ERR_NULL_POINTER);        // no table
        l.table = f; l.table_cap = 0;
        EXPECT(call(&l, &lcarry), MG_ERR_BAD_SIZE);
        l.table_cap = 1024;
        EXPECT(call(&l, &lcarry), MG_ERR_BAD_SIZE);
        l = lrn; l.kind = MG_BANDITS_LEARNER_THOMPSON; l.max_attempts = 0;
        EXPECT(call(&l, &lcarry), MG_ERR_BAD_SIZE);
        l.max_attempts = 65;
        EXPECT(call(&l, &lcarry), MG_ERR_BAD_SIZE);
        l.max_attempts = 8; l.eps_threshold = fake<uint32_t>();
        EXPECT(call(&l, &lcarry), MG_ERR_BAD_CONFIG);
        if (!scores) {
            l = lrn; l.arms = 11;                            // not the env's
            EXPECT(call(&l, &lcarry), MG_ERR_BAD_CONFIG);
        }
    }
    EXPECT(mg_bandits_learner_scores(4, nullptr, i32, &lcarry, 1u, 0u, f, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_bandits_learner_scores(4, &lrn, nullptr, &lcarry, 1u, 0u, f, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_bandits_learner_scores(4, &lrn, i32, nullptr, 1u, 0u, f, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_bandits_learner_scores(4, &lrn, i32, &lcarry, 1u, 0u, nullptr, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_bandits_learner_scores(0, &lrn, i32, &lcarry, 1u, 0u, f, nullptr, nullptr), MG_ERR_BAD_SIZE);
}

// the liftsim entry points that launch: the same configuration refusals as mg_liftsim_layout, and their own pointers
static void liftsim_launches() {
    int32_t *i32 = fake<int32_t>();
    float *f = fake<float>();
    double *d = fake<double>();
    static mg_liftsim_policy pol;
    std::memset(&pol, 0, sizeof(pol));
    pol.params = f; pol.n_policies = 2; pol.hidden = 8; pol.floors = 10; pol.elevators = 4;
    static mg_liftsim_rpolicy rpol;
    std::memset(&rpol, 0, sizeof(rpol));
    rpol.params = f; rpol.n_policies = 2; rpol.hidden = 8; rpol.floors = 10; rpol.elevators = 4;
    static const mg_liftsim_policy_state pst = {fake<float>(), fake<int32_t>(), fake<float>()};
    typedef int (*Call)(const mg_liftsim_config *, int32_t, void *);
    const Call calls[] = {
        [](const mg_liftsim_config *c, int32_t n, void *a) { return mg_liftsim_seed(c, n, a, 1u, nullptr, nullptr); },
        [](const mg_liftsim_config *c, int32_t n, void *a) { return mg_liftsim_reset(c, n, a, nullptr, nullptr); },
        [](const mg_liftsim_config *c, int32_t n, void *a) { return mg_liftsim_step(c, n, a, fake<int32_t>(), nullptr); },
        [](const mg_liftsim_config *c, int32_t n, void *a) { return mg_liftsim_statistics(c, n, a, nullptr); },
        [](const mg_liftsim_config *c, int32_t n, void *a) { return mg_liftsim_rule_policy(c, n, a, fake<int32_t>(), nullptr); },
        [](const mg_liftsim_config *c, int32_t n, void *a) {
            return mg_liftsim_rollout(c, n, a, MG_LIFTSIM_POLICY_RULE, nullptr, 3, fake<double>(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr); },
        [](const mg_liftsim_config *c, int32_t n, void *a) {
            return mg_liftsim_policy_rollout(c, n, a, 3, &pol, fake<int32_t>(), fake<double>(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr); },
        [](const mg_liftsim_config *c, int32_t n, void *a) {
            return mg_liftsim_rpolicy_rollout(c, n, a, 3, &rpol, fake<int32_t>(), &pst, fake<double>(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr); },
    };
    const mg_liftsim_config cfg = lift_config(10, 4);
    for (Call call : calls) {
        EXPECT(call(nullptr, 4, g_fake), MG_ERR_NULL_POINTER);
        EXPECT(call(&cfg, 4, nullptr), MG_ERR_NULL_POINTER);
        EXPECT(call(&cfg, 0, g_fake), MG_ERR_BAD_SIZE);
        for (int bad = 0; bad < 11; ++bad) {
            mg_liftsim_config b = cfg;
            switch (bad) {
            case 0: b.floors = 1; break;
            case 1: b.floors = MG_LIFTSIM_MAX_FLOORS + 1; break;
            case 2: b.elevators = 0; break;
            case 3: b.elevators = MG_LIFTSIM_MAX_ELEVATORS + 1; break;
            case 4: b.dt = 0.0; break;
            case 5: b.floor_height = -1.0; break;
            case 6: b.queue_capacity = 0; break;
            case 7: b.window = (1 << 20) + 1; break;
            case 8: b.generation_interval = 0.0; break;
            case 9: b.generator = MG_LIFTSIM_CUSTOM; b.table_len = 3; break;      // CUSTOM without its tables
            default: b.generator = 2; break;
            }
            EXPECT(call(&b, 4, g_fake), MG_ERR_BAD_CONFIG);
        }
    }
    EXPECT(mg_liftsim_rule_policy(&cfg, 4, g_fake, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_liftsim_rollout(&cfg, 4, g_fake, MG_LIFTSIM_POLICY_RULE, nullptr, 3, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_liftsim_rollout(&cfg, 4, g_fake, MG_LIFTSIM_POLICY_ACTIONS, nullptr, 3, d, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), MG_ERR_NULL_POINTER);
    EXPECT(mg_liftsim_rollout(&cfg, 4, g_fake, MG_LIFTSIM_POLICY_ACTIONS, i32, 0, d, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), MG_ERR_BAD_SIZE);
    EXPECT(mg_liftsim_rollout(&cfg, 4, g_fake, 2, i32, 3, d, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), MG_ERR_BAD_CONFIG);
    EXPECT(mg_liftsim_rollout(&cfg, 4, g_fake, MG_LIFTSIM_POLICY_ACTIONS, i32, 3, d, nullptr, nullptr, nullptr, nullptr, i32, nullptr), MG_ERR_BAD_CONFIG);
    for (int rec = 0; rec < 2; ++rec) {
        auto roll = [&](int steps, const mg_liftsim_policy *p, const int32_t *ids, const mg_liftsim_policy_state *s, double *ret) {
            mg_liftsim_rpolicy rp;                          // the same fields in the same order
            if (p) std::memcpy(&rp, p, sizeof(rp));
            return rec ? mg_liftsim_rpolicy_rollout(&cfg, 4, g_fake, steps, p ? &rp : nullptr, ids, s, ret, nullptr, nullptr, nullptr, nullptr,
                                                    nullptr, nullptr)
                       : mg_liftsim_policy_rollout(&cfg, 4, g_fake, steps, p, ids, ret, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
        };
        static_assert(sizeof(mg_liftsim_policy) == sizeof(mg_liftsim_rpolicy), "the two descriptors share one layout");
        EXPECT(roll(3, nullptr, i32, &pst, d), MG_ERR_NULL_POINTER);
        EXPECT(roll(3, &pol, nullptr, &pst, d), MG_ERR_NULL_POINTER);
        EXPECT(roll(3, &pol, i32, &pst, nullptr), MG_ERR_NULL_POINTER);
        EXPECT(roll(0, &pol, i32, &pst, d), MG_ERR_BAD_SIZE);
        mg_liftsim_policy p = pol;
        p.params = nullptr;
        EXPECT(roll(3, &p, i32, &pst, d), MG_ERR_NULL_POINTER);
        p = pol; p.params = f + 1;
        EXPECT(roll(3, &p, i32, &pst, d), MG_ERR_BAD_CONFIG);
        p = pol; p.n_policies = 0;
        EXPECT(roll(3, &p, i32, &pst, d), MG_ERR_BAD_SIZE);
        p = pol; p.hidden = 0;
        EXPECT(roll(3, &p, i32, &pst, d), MG_ERR_BAD_SIZE);
        p = pol; p.hidden = 65;                             // one past the supported path
        EXPECT(roll(3, &p, i32, &pst, d), MG_ERR_BAD_SIZE);
        p = pol; p.floors = 11;                             // not the building's
        EXPECT(roll(3, &p, i32, &pst, d), MG_ERR_BAD_CONFIG);
        p = pol; p.elevators = 3;
        EXPECT(roll(3, &p, i32, &pst, d), MG_ERR_BAD_CONFIG);
        if (rec) {
            EXPECT(roll(3, &pol, i32, nullptr, d), MG_ERR_NULL_POINTER);
            for (int k = 0; k < 3; ++k) {
                mg_liftsim_policy_state s = pst;
                void **field[3] = {(void **)&s.h, (void **)&s.prev_choice, (void **)&s.prev_reward};
                *field[k] = nullptr;
                EXPECT(roll(3, &pol, i32, &s, d), MG_ERR_NULL_POINTER);
            }
            mg_liftsim_policy_state s = pst;
            s.h = (float *)(g_fake + 2);                    // not 4-byte aligned
            EXPECT(roll(3, &pol, i32, &s, d), MG_ERR_BAD_CONFIG);
        }
    }
}

int main() {
    quadrotor();
    quadrotor_launches();
    param_counts();
    liftsim();
    liftsim_launches();
    maze();
    walker();
    walker_launches();
    a1();
    metalm();
    bandits();
    if (g_failed) {
        std::printf("%d of %d checks FAILED\n", g_failed, g_checks);
        return 1;
    }
    std::printf("%d checks passed\n", g_checks);
    return 0;
}
