// Pendulum-v1 per-env step (the equations of the header's K18P comment + TimeLimit), shared by K18P
// (xpa_pendulum_step, classic.hip) and K32's fused rollout step (rollout.hip) so both run the same arithmetic.
#pragma once
#include "xpa_common.h"

struct XpaPendulumEnv {
    double *state;  // [N, 2] f64 (th, thdot)
    float *obs;     // [N, ld_obs]: the next observation (cos th, sin th, thdot; of the reset state after a done)
    int64_t ld_obs;
    float *final_obs;  // [N, 3]: the step's own observation (before any reset)
    float *rew;
    uint8_t *term, *trunc;
    int *ep_step;
    uint32_t *ep_index;
    float *ep_score, *ep_last_score;
    int *ep_last_len;
    uint32_t seed;
    int max_episode_steps;
};

namespace pendulum {
constexpr double kMaxSpeed = 8.0, kMaxTorque = 2.0, kDt = 0.05;
constexpr double kSinGain = 15.0, kTorqueGain = 3.0;  // 3 g / (2 l), 3 / (m l^2) at g = 10, m = l = 1
constexpr double kPi = 3.141592653589793, kTwoPi = 2.0 * 3.141592653589793;
constexpr uint32_t kSaltPendulum = 0x9E2D0105u;

// th0 = (2 u - 1) pi, thdot0 = 2 u - 1 from the counter hash (f32-exact uniform, then f64)
__device__ __forceinline__ double reset_dim(uint32_t seed, uint32_t env, uint32_t ep, uint32_t d) {
#pragma clang fp contract(off)
    const double c = 2.0 * (double)xpa_u01(xpa_hash4(seed ^ kSaltPendulum, env, ep, d)) - 1.0;
    return d == 0 ? c * kPi : c;
}

// Python's float x % y for y > 0 (floor modulo: the result has y's sign)
__device__ __forceinline__ double floor_mod(double x, double y) {
#pragma clang fp contract(off)
    double m = fmod(x, y);
    if (m != 0.0) {
        if (m < 0.0) m = m + y;
    } else {
        m = 0.0;
    }
    return m;
}

// One env's mutable state, held in registers by the caller (K18P loads and stores it around one step; K32 keeps it
// for a whole launch of steps).
struct Local {
    double th, thdot;
    int ep_step;
    uint32_t ep_index;
    float ep_score;
};

__device__ __forceinline__ Local load(const XpaPendulumEnv &e, int64_t n) {
    const double *st = e.state + 2 * n;
    return Local{st[0], st[1], e.ep_step[n], e.ep_index[n], e.ep_score[n]};
}

__device__ __forceinline__ void store(const XpaPendulumEnv &e, int64_t n, const Local &s) {
    double *st = e.state + 2 * n;
    st[0] = s.th;
    st[1] = s.thdot;
    e.ep_step[n] = s.ep_step;
    e.ep_index[n] = s.ep_index;
    e.ep_score[n] = s.ep_score;
}

// One env's step with torque a (clamped to +-2 here) on the register state s: writes final_obs / obs / rew / term /
// trunc (and the finished episode's score / length); returns the reward, *te / *tr the flags (never terminated),
// obs_out[0..2] the next observation (of the reset state after a truncation).
__device__ __forceinline__ float step(const XpaPendulumEnv &e, int64_t n, float a, Local &s, bool *te_out,
                                      bool *tr_out, float *obs_out) {
#pragma clang fp contract(off)  // every product and sum rounded on its own (no fma), as the numpy checker does
    double th = s.th, thdot = s.thdot;
    const double u = fmin(fmax((double)a, -kMaxTorque), kMaxTorque);
    const double an = floor_mod(th + kPi, kTwoPi) - kPi;
    const double cost = an * an + 0.1 * (thdot * thdot) + 0.001 * (u * u);
    const double acc = kSinGain * sin(th) + kTorqueGain * u;
    thdot = fmin(fmax(thdot + acc * kDt, -kMaxSpeed), kMaxSpeed);
    th = th + thdot * kDt;
    const float r = (float)(-cost);
    const int steps = s.ep_step + 1;
    const bool tr = steps >= e.max_episode_steps;  // TimeLimit; the env itself never terminates
    const float score = s.ep_score + r;
    float *fo = e.final_obs + 3 * n;
    const float f0 = (float)cos(th), f1 = (float)sin(th), f2 = (float)thdot;
    fo[0] = f0;
    fo[1] = f1;
    fo[2] = f2;
    e.rew[n] = r;
    e.term[n] = 0;
    e.trunc[n] = tr ? 1 : 0;
    if (tr) {
        const uint32_t ep = s.ep_index + 1u;
        s.ep_index = ep;
        e.ep_last_score[n] = score;
        e.ep_last_len[n] = steps;
        s.ep_step = 0;
        s.ep_score = 0.f;
        th = reset_dim(e.seed, (uint32_t)n, ep, 0);
        thdot = reset_dim(e.seed, (uint32_t)n, ep, 1);
        obs_out[0] = (float)cos(th);
        obs_out[1] = (float)sin(th);
        obs_out[2] = (float)thdot;
    } else {
        s.ep_step = steps;
        s.ep_score = score;
        obs_out[0] = f0;
        obs_out[1] = f1;
        obs_out[2] = f2;
    }
    s.th = th;
    s.thdot = thdot;
    float *o = e.obs + n * e.ld_obs;
    o[0] = obs_out[0];
    o[1] = obs_out[1];
    o[2] = obs_out[2];
    *te_out = false;
    *tr_out = tr;
    return r;
}
}  // namespace pendulum
