// MountainCar-v0 per-env step (the equations of the header's K18M comment + TimeLimit) behind the reference's frame
// stack of 4, shared by K18M (xpa_mountaincar_step, classic.hip) and K32's fused rollout step (rollout.hip) so both run
// the same arithmetic.
#pragma once
#include "xpa_common.h"

struct XpaMountainCarEnv {
    double *state;  // [N, 2] f64 (position, velocity)
    float *obs;     // [N, ld_obs]: the last four (position, velocity) frames, oldest first (the reset frame four times
                    // after a done).  The stack lives here: a step reads columns 2..7 and appends its own frame
    int64_t ld_obs;
    float *final_obs;  // [N, 8]: the stack with the step's own frame (before any reset)
    float *rew;
    uint8_t *term, *trunc;
    int *ep_step;
    uint32_t *ep_index;
    float *ep_score, *ep_last_score;
    int *ep_last_len;
    uint32_t seed;
    int max_episode_steps;
};

namespace mountaincar {
constexpr double kMinPos = -1.2, kMaxPos = 0.6, kMaxSpeed = 0.07, kGoalPos = 0.5, kGoalVel = 0.0;
constexpr double kForce = 0.001, kGravity = 0.0025;
constexpr int kStack = 4, kObs = 2 * kStack;
constexpr uint32_t kSaltMountainCar = 0x30CA2005u;

// position0 = 0.2 u - 0.6 from the counter hash (f32-exact uniform, then f64); velocity0 = 0
__device__ __forceinline__ double reset_pos(uint32_t seed, uint32_t env, uint32_t ep) {
#pragma clang fp contract(off)
    return 0.2 * (double)xpa_u01(xpa_hash4(seed ^ kSaltMountainCar, env, ep, 0u)) - 0.6;
}
__device__ __forceinline__ double reset_dim(uint32_t seed, uint32_t env, uint32_t ep, uint32_t d) {
    return d == 0 ? reset_pos(seed, env, ep) : 0.0;
}

// One env's mutable state, held in registers by the caller (K18M loads and stores it around one step; K32 keeps it
// for a whole launch of steps).  fr: the three newest frames of the observation row (its columns 2..7), read at load;
// every step writes the whole row back, so nothing but (position, velocity) is stored beside it.
struct Local {
    double pos, vel;
    float fr[kObs - 2];
    int ep_step;
    uint32_t ep_index;
    float ep_score;
};

__device__ __forceinline__ Local load(const XpaMountainCarEnv &e, int64_t n) {
    const double *st = e.state + 2 * n;
    const float *o = e.obs + n * e.ld_obs;
    Local s{st[0], st[1], {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, e.ep_step[n], e.ep_index[n], e.ep_score[n]};
#pragma unroll
    for (int d = 0; d < kObs - 2; ++d) s.fr[d] = o[2 + d];
    return s;
}

__device__ __forceinline__ void store(const XpaMountainCarEnv &e, int64_t n, const Local &s) {
    double *st = e.state + 2 * n;
    st[0] = s.pos;
    st[1] = s.vel;
    e.ep_step[n] = s.ep_step;
    e.ep_index[n] = s.ep_index;
    e.ep_score[n] = s.ep_score;
}

// One env's step with action a (0 / 1 / 2: push left / none / right) on the register state s: writes final_obs / obs /
// rew / term / trunc (and the finished episode's score / length); returns the reward, *te / *tr the flags,
// obs_out[0..7] the next observation (the reset stack after a done).
__device__ __forceinline__ float step(const XpaMountainCarEnv &e, int64_t n, int a, Local &s, bool *te_out,
                                      bool *tr_out, float *obs_out) {
#pragma clang fp contract(off)  // gym's Python arithmetic: every product and sum rounded on its own (no fma)
    double pos = s.pos, vel = s.vel;
    vel = vel + ((double)(a - 1) * kForce + cos(3.0 * pos) * (-kGravity));
    vel = fmin(fmax(vel, -kMaxSpeed), kMaxSpeed);
    pos = pos + vel;
    pos = fmin(fmax(pos, kMinPos), kMaxPos);
    if (pos == kMinPos && vel < 0.0) vel = 0.0;
    const bool te = pos >= kGoalPos && vel >= kGoalVel;
    const int steps = s.ep_step + 1;
    const bool tr = steps >= e.max_episode_steps;  // gym TimeLimit: independent of terminated
    const float score = s.ep_score + -1.0f;
    float f[kObs];
#pragma unroll
    for (int d = 0; d < kObs - 2; ++d) f[d] = s.fr[d];
    f[kObs - 2] = (float)pos;
    f[kObs - 1] = (float)vel;
    float *fo = e.final_obs + kObs * n;
#pragma unroll
    for (int d = 0; d < kObs; ++d) fo[d] = f[d];
    e.rew[n] = -1.0f;
    e.term[n] = te ? 1 : 0;
    e.trunc[n] = tr ? 1 : 0;
    if (te || tr) {
        const uint32_t ep = s.ep_index + 1u;
        s.ep_index = ep;
        e.ep_last_score[n] = score;
        e.ep_last_len[n] = steps;
        s.ep_step = 0;
        s.ep_score = 0.f;
        pos = reset_pos(e.seed, (uint32_t)n, ep);
        vel = 0.0;
#pragma unroll
        for (int k = 0; k < kStack; ++k) {
            obs_out[2 * k] = (float)pos;
            obs_out[2 * k + 1] = 0.f;
        }
    } else {
        s.ep_step = steps;
        s.ep_score = score;
#pragma unroll
        for (int d = 0; d < kObs; ++d) obs_out[d] = f[d];
    }
    s.pos = pos;
    s.vel = vel;
#pragma unroll
    for (int d = 0; d < kObs - 2; ++d) s.fr[d] = obs_out[2 + d];
    float *o = e.obs + n * e.ld_obs;
#pragma unroll
    for (int d = 0; d < kObs; ++d) o[d] = obs_out[d];
    *te_out = te;
    *tr_out = tr;
    return -1.0f;
}
}  // namespace mountaincar
