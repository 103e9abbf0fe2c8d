// Acrobot-v1 per-env step (the equations of the header's K18A comment + TimeLimit), shared by K18A
// (xpa_acrobot_step, classic.hip) and K32's fused rollout step (rollout.hip) so both run the same arithmetic.
#pragma once
#include "xpa_common.h"

struct XpaAcrobotEnv {
    double *state;  // [N, 4] f64 (th1, th2, thdot1, thdot2)
    float *obs;     // [N, ld_obs]: the next observation (cos th1, sin th1, cos th2, sin th2, thdot1, thdot2; of the
                    // reset state after a done)
    int64_t ld_obs;
    float *final_obs;  // [N, 6]: the step's own observation (before any reset)
    float *rew;
    uint8_t *term, *trunc;
    int *ep_step;
    uint32_t *ep_index;
    float *ep_score, *ep_last_score;
    int *ep_last_len;
    uint32_t seed;
    int max_episode_steps;
};

namespace acrobot {
constexpr double kM1 = 1.0, kM2 = 1.0, kL1 = 1.0, kLc1 = 0.5, kLc2 = 0.5, kI1 = 1.0, kI2 = 1.0, kG = 9.8, kDt = 0.2;
constexpr double kPi = 3.141592653589793, kTwoPi = 2.0 * 3.141592653589793, kHalfPi = 3.141592653589793 / 2.0;
constexpr double kMaxVel1 = 4.0 * 3.141592653589793, kMaxVel2 = 9.0 * 3.141592653589793;
constexpr uint32_t kSaltAcrobot = 0xAC20B075u;

// every state dim starts at 0.2 u - 0.1 from the counter hash (f32-exact uniform, then f64)
__device__ __forceinline__ double reset_dim(uint32_t seed, uint32_t env, uint32_t ep, uint32_t d) {
#pragma clang fp contract(off)
    return 0.2 * (double)xpa_u01(xpa_hash4(seed ^ kSaltAcrobot, env, ep, d)) - 0.1;
}

// while x > pi: x -= 2 pi; while x < -pi: x += 2 pi.  One step moves an angle by a few hundred radians at the most
// (the velocities are clamped between steps); a value no subtraction of 2 pi would change is returned as it is, so
// that the loops end on any input.
__device__ __forceinline__ double wrap_pi(double x) {
#pragma clang fp contract(off)
    if (!(fabs(x) <= 1.0e6)) return x;
    while (x > kPi) x = x - kTwoPi;
    while (x < -kPi) x = x + kTwoPi;
    return x;
}

struct Vec4 {
    double th1, th2, v1, v2;
};

// The "book" derivative of (th1, th2, thdot1, thdot2) under torque a, in the header's operation order; the two
// cos(. - pi / 2) terms are formed as cosines.
__device__ __forceinline__ Vec4 deriv(const Vec4 &y, double a) {
#pragma clang fp contract(off)
    const double c2 = cos(y.th2), s2 = sin(y.th2);
    const double d1 =
        ((kM1 * (kLc1 * kLc1) + kM2 * (((kL1 * kL1) + (kLc2 * kLc2)) + ((2.0 * kL1) * kLc2) * c2)) + kI1) + kI2;
    const double d2 = kM2 * ((kLc2 * kLc2) + (kL1 * kLc2) * c2) + kI2;
    const double phi2 = ((kM2 * kLc2) * kG) * cos((y.th1 + y.th2) - kHalfPi);
    const double phi1 = (((((-kM2 * kL1) * kLc2) * (y.v2 * y.v2)) * s2 -
                          (((((2.0 * kM2) * kL1) * kLc2) * y.v2) * y.v1) * s2) +
                         ((kM1 * kLc1 + kM2 * kL1) * kG) * cos(y.th1 - kHalfPi)) +
                        phi2;
    const double dd2 = (((a + (d2 / d1) * phi1) - (((kM2 * kL1) * kLc2) * (y.v1 * y.v1)) * s2) - phi2) /
                       ((kM2 * (kLc2 * kLc2) + kI2) - (d2 * d2) / d1);
    const double dd1 = -((d2 * dd2 + phi1) / d1);
    return Vec4{y.v1, y.v2, dd1, dd2};
}

// One env's mutable state, held in registers by the caller (K18A loads and stores it around one step; K32 keeps it
// for a whole launch of steps).
struct Local {
    double th1, th2, v1, v2;
    int ep_step;
    uint32_t ep_index;
    float ep_score;
};

__device__ __forceinline__ Local load(const XpaAcrobotEnv &e, int64_t n) {
    const double *st = e.state + 4 * n;
    return Local{st[0], st[1], st[2], st[3], e.ep_step[n], e.ep_index[n], e.ep_score[n]};
}

__device__ __forceinline__ void store(const XpaAcrobotEnv &e, int64_t n, const Local &s) {
    double *st = e.state + 4 * n;
    st[0] = s.th1;
    st[1] = s.th2;
    st[2] = s.v1;
    st[3] = s.v2;
    e.ep_step[n] = s.ep_step;
    e.ep_index[n] = s.ep_index;
    e.ep_score[n] = s.ep_score;
}

__device__ __forceinline__ void obs_of(double th1, double th2, double v1, double v2, float *o) {
    o[0] = (float)cos(th1);
    o[1] = (float)sin(th1);
    o[2] = (float)cos(th2);
    o[3] = (float)sin(th2);
    o[4] = (float)v1;
    o[5] = (float)v2;
}

// One env's step with action a (0 / 1 / 2: torque -1 / 0 / +1) on the register state s: writes final_obs / obs / rew /
// term / trunc (and the finished episode's score / length); returns the reward, *te / *tr the flags, obs_out[0..5] the
// next observation (of the reset state after a done).
__device__ __forceinline__ float step(const XpaAcrobotEnv &e, int64_t n, int a, Local &s, bool *te_out, bool *tr_out,
                                      float *obs_out) {
#pragma clang fp contract(off)  // every product and sum rounded on its own (no fma), as the numpy checker does
    const double torque = (double)(a - 1);
    const Vec4 y{s.th1, s.th2, s.v1, s.v2};
    // classic RK4 over [0, dt]: acc = ((k1 + 2 k2) + 2 k3) + k4.  One loop body (not unrolled): the derivative's four
    // f64 sin / cos stay one copy of code.
    Vec4 yt = y, acc{0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
    for (int st = 0; st < 4; ++st) {
        const Vec4 k = deriv(yt, torque);
        if (st == 0) {
            acc = k;
        } else {
            const double w = st == 3 ? 1.0 : 2.0;
            acc = Vec4{acc.th1 + w * k.th1, acc.th2 + w * k.th2, acc.v1 + w * k.v1, acc.v2 + w * k.v2};
        }
        const double h = st < 2 ? kDt / 2.0 : kDt;
        yt = Vec4{y.th1 + h * k.th1, y.th2 + h * k.th2, y.v1 + h * k.v1, y.v2 + h * k.v2};
    }
    constexpr double h6 = kDt / 6.0;
    double th1 = wrap_pi(y.th1 + h6 * acc.th1);
    double th2 = wrap_pi(y.th2 + h6 * acc.th2);
    double v1 = fmin(fmax(y.v1 + h6 * acc.v1, -kMaxVel1), kMaxVel1);
    double v2 = fmin(fmax(y.v2 + h6 * acc.v2, -kMaxVel2), kMaxVel2);
    const bool te = (-cos(th1) - cos(th2 + th1)) > 1.0;
    const float r = te ? 0.0f : -1.0f;
    const int steps = s.ep_step + 1;
    const bool tr = steps >= e.max_episode_steps;  // gym TimeLimit: independent of terminated
    const float score = s.ep_score + r;
    float f[6];
    obs_of(th1, th2, v1, v2, f);
    float *fo = e.final_obs + 6 * n;
#pragma unroll
    for (int d = 0; d < 6; ++d) fo[d] = f[d];
    e.rew[n] = r;
    e.term[n] = te ? 1 : 0;
    e.trunc[n] = tr ? 1 : 0;
    if (te || tr) {
        const uint32_t ep = s.ep_index + 1u;
        s.ep_index = ep;
        e.ep_last_score[n] = score;
        e.ep_last_len[n] = steps;
        s.ep_step = 0;
        s.ep_score = 0.f;
        th1 = reset_dim(e.seed, (uint32_t)n, ep, 0);
        th2 = reset_dim(e.seed, (uint32_t)n, ep, 1);
        v1 = reset_dim(e.seed, (uint32_t)n, ep, 2);
        v2 = reset_dim(e.seed, (uint32_t)n, ep, 3);
        obs_of(th1, th2, v1, v2, obs_out);
    } else {
        s.ep_step = steps;
        s.ep_score = score;
#pragma unroll
        for (int d = 0; d < 6; ++d) obs_out[d] = f[d];
    }
    s.th1 = th1;
    s.th2 = th2;
    s.v1 = v1;
    s.v2 = v2;
    float *o = e.obs + n * e.ld_obs;
#pragma unroll
    for (int d = 0; d < 6; ++d) o[d] = obs_out[d];
    *te_out = te;
    *tr_out = tr;
    return r;
}
}  // namespace acrobot
