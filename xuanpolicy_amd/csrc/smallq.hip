// K34 — one PER-DQN learner step of a small MLP Q-network (the reference's perdqn/classic_control configs: D -> 128
// -> 128 -> A, batch 128), gfx950: a main launch of one workgroup per 32 batch rows and a finalize launch.
//
// Replaces everything PerDQN_Learner.update does around K19 for such a network (perdqn_learner.py:17-48): the eval
// forward on obs, the target forward on next, the TD target / loss / |TD| (K19's arithmetic, dqn.hip), autograd's
// backward, Adam.step() and, every sync_frequency updates, the hard target copy — some tens of launches for ~10 MFLOP.
//
// A workgroup (512 threads, 8 waves) owns 32 rows.  Activations are transposed, [feature][row] with row stride 36;
// every dense product is a set of 32 x 32 tiles on v_mfma_f32_32x32x2_f32 (sm_tile, one wave per tile).  The target
// network goes FIRST: its W0 / W1 / Wq are staged, its forward runs on the next rows and each row is reduced to
// y = rew + gamma (1 - term) max_a Qt; after that nothing of the target network is live and the same LDS regions take
// the eval network, so one 128 x 128 W1 image (16.5 k floats) and two activation planes are all that is ever resident
// (34 000 floats at 128 / 128; two images plus both networks' planes would not fit the 40 704-float budget).
// d loss / d Qe is one-hot per row, so the output layer's backward has no GEMM: dh1[row] = dq[row] Wq[act[row]][:]
// and gWq / gbq are per-action sums over the rows, on the VALU.  gW1 = dz1^T h0, dh0 = dz1 W1 and gW0 = dz0^T x stay
// on sm_tile; h1 is reused in place as dz1 and h0 as dz0.  Each workgroup writes its partial gradients at the flat
// gradient's offsets; the finalize sums them in workgroup order, steps Adam (K9's arithmetic, no clipping: the
// reference's learner has none) from the device schedule, writes the loss scalars and copies the updated eval
// parameters over the target ones when the call's sync_target flag is set.
#include "small_tile.h"

namespace {

constexpr int kSqThreads = 512;
constexpr int kSqWaves = kSqThreads / 64;
constexpr int kSqLds = 40704;   // floats, K30's budget
constexpr int kSqS = 36;        // row stride of the activation planes (32 rows + 4)
constexpr int kSqMaxGroups = 16;

// The LDS carve of one workgroup (offsets multiples of 4 floats)
struct SqLds {
    float *xT;     // [DP][S]   the rows' inputs (next, then obs)
    float *h0T;    // [H0][S]   -> dz0
    float *h1T;    // [H1][S]   -> dz1
    float *W0T;    // [DP][H0]
    float *W1i;    // [H0][H1 + 1] transposed in the forwards, then row-major [H1][H0] for dh0
    float *WqT;    // [H1][KP]
    float *b0s, *b1s, *bqs;   // [H0], [H1], [KP]
    float *rowf;   // [6][32]: action, reward, terminal, y, dq, (unused)
    float *q;      // [32][KP]
};

__device__ __forceinline__ SqLds sq_carve(float *lds, int DP, int H0, int H1, int KP) {
    SqLds L;
    L.xT = lds;
    L.h0T = L.xT + DP * kSqS;
    L.h1T = L.h0T + H0 * kSqS;
    L.W0T = L.h1T + H1 * kSqS;
    L.W1i = L.W0T + DP * H0;
    L.WqT = L.W1i + ((H0 * (H1 + 1) + 3) & ~3);
    L.b0s = L.WqT + H1 * KP;
    L.b1s = L.b0s + H0;
    L.bqs = L.b1s + H1;
    L.rowf = L.bqs + KP;
    L.q = L.rowf + 6 * 32;
    return L;
}

// One network's weights into the images (all threads; the caller's barrier follows).  W1 is walked in source order
// with 8 loads in flight and written with the odd row stride H1 + 1 (K30's stage_T: coalesced loads, conflict-free
// stores).
__device__ __forceinline__ void sq_stage_net(const SqLds &L, const float *W0, const float *b0, const float *W1,
                                             const float *b1, const float *Wq, const float *bq, int D, int DP, int H0,
                                             int H1, int A, int KP) {
    const int t = threadIdx.x, H1P = H1 + 1;
    for (int e0 = t; e0 < H1 * H0; e0 += 8 * kSqThreads) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = e0 + u * kSqThreads;
            v[u] = e < H1 * H0 ? W1[e] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = e0 + u * kSqThreads;
            if (e < H1 * H0) L.W1i[(e % H0) * H1P + e / H0] = v[u];
        }
    }
    for (int e = t; e < DP * H0; e += kSqThreads) {   // W0 [H0][D] -> W0T [DP][H0], rows D .. DP zero
        const int i = e / H0, j = e % H0;
        L.W0T[e] = i < D ? W0[j * D + i] : 0.f;
    }
    for (int e = t; e < H1 * KP; e += kSqThreads) {   // Wq [A][H1] -> WqT [H1][KP], columns A .. KP zero
        const int j = e / KP, a = e % KP;
        L.WqT[e] = a < A ? Wq[a * H1 + j] : 0.f;
    }
    for (int e = t; e < H0; e += kSqThreads) L.b0s[e] = b0[e];
    for (int e = t; e < H1; e += kSqThreads) L.b1s[e] = b1[e];
    for (int e = t; e < KP; e += kSqThreads) L.bqs[e] = e < A ? bq[e] : 0.f;
}

// The workgroup's B <= 32 rows of src [n_rows, ld] into xT (rows >= B and features >= D zero): thread (row, quarter)
__device__ __forceinline__ void sq_stage_rows(const SqLds &L, const float *src, int64_t ld, const int64_t *rows, int B,
                                              int D, int DP) {
    const int t = threadIdx.x;
    if (t < 128) {
        const int b = t & 31, c = t >> 5;
        const bool ok = b < B;
        const int64_t row = ok ? rows[b] : 0;
        for (int i = c; i < DP; i += 4) L.xT[i * kSqS + b] = ok && i < D ? src[row * ld + i] : 0.f;
    }
}

// x -> h0 -> h1 -> q over the staged images (the caller's barrier before; ends with one: q [32][KP] is complete)
template <int ACT>
__device__ __forceinline__ void sq_forward(const SqLds &L, int DP, int H0, int H1, int KP, float slope) {
    const int w = threadIdx.x >> 6, li = threadIdx.x & 31;
    for (int tl = w; tl < H0 / 32; tl += kSqWaves) {
        const int j0 = 32 * tl;
        const f32x16 acc = sm_tile(L.xT, 1, kSqS, 32, L.W0T + j0, H0, 1, 32, DP);
#pragma unroll
        for (int r = 0; r < 16; ++r)
            L.h0T[(j0 + li) * kSqS + sm_row(r)] = sm_act<ACT>(acc[r] + L.b0s[j0 + li], slope);
    }
    __syncthreads();
    for (int tl = w; tl < H1 / 32; tl += kSqWaves) {
        const int j0 = 32 * tl;
        const f32x16 acc = sm_tile(L.h0T, 1, kSqS, 32, L.W1i + j0, H1 + 1, 1, 32, H0);
#pragma unroll
        for (int r = 0; r < 16; ++r)
            L.h1T[(j0 + li) * kSqS + sm_row(r)] = sm_act<ACT>(acc[r] + L.b1s[j0 + li], slope);
    }
    __syncthreads();
    if (w == 0) {
        const f32x16 acc = sm_tile(L.h1T, 1, kSqS, 32, L.WqT, KP, 1, KP, H1);
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (li < KP) L.q[sm_row(r) * KP + li] = acc[r] + L.bqs[li];
    }
    __syncthreads();
}

// The row indices of the workgroup's rows, clamped into [0, n_rows) (s_rows), and the count of clamped ones
__device__ __forceinline__ int sq_row_indices(const int64_t *idx, int r0, int B, int64_t n_rows, int64_t *s_rows) {
    const int t = threadIdx.x;
    int bad = 0;
    if (t < 32) {
        int64_t row = 0;
        if (t < B) {
            row = idx ? idx[r0 + t] : (int64_t)(r0 + t);
            if (row < 0 || row >= n_rows) {
                bad = 1;
                row = row < 0 ? 0 : n_rows - 1;
            }
        }
        s_rows[t] = row;
    }
    return bad;
}

template <int ACT>
__global__ __launch_bounds__(kSqThreads, 1) void small_q_update_kernel(XpaSmallQArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[kSqLds];
    __shared__ int64_t s_rows[32];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, li = lane & 31;
    const int gi = blockIdx.x, r0 = 32 * gi, Btot = a.batch;
    const int B = min(32, Btot - r0);
    const int D = a.d_in, DP = (a.d_in + 3) & ~3, H0 = a.h0, H1 = a.h1, A = a.k, KP = (a.k + 3) & ~3;
    const float slope = a.slope;
    const SqLds L = sq_carve(lds, DP, H0, H1, KP);
    float *act_s = L.rowf, *rew_s = L.rowf + 32, *term_s = L.rowf + 64, *y_s = L.rowf + 96, *dq_s = L.rowf + 128;
    float *part = a.grad_part + (int64_t)gi * a.n;
    auto gp = [&](float *p) -> float * { return part + (p - a.grad); };
    // ---- gather: the row indices, then the target network's images with the next rows ----
    int bad = sq_row_indices(a.idx, r0, B, a.n_rows, s_rows);
    sq_stage_net(L, a.tW0, a.tb0, a.tW1, a.tb1, a.tWq, a.tbq, D, DP, H0, H1, A, KP);
    __syncthreads();   // s_rows
    sq_stage_rows(L, a.next, a.obs_ld, s_rows, B, D, DP);
    if (t >= 128 && t < 160) {   // the rows' action (clamped, counted), reward and terminal flag
        const int b = t - 128;
        const bool ok = b < B;
        const int64_t row = s_rows[b];
        int ai = ok ? (int)a.act[row] : 0;
        if (ai < 0 || ai >= A) {
            ++bad;
            ai = ai < 0 ? 0 : A - 1;
        }
        act_s[b] = (float)ai;
        rew_s[b] = ok ? a.rew[row] : 0.f;
        term_s[b] = ok ? a.term[row] : 0.f;
    }
    if (a.err && bad) atomicAdd(a.err, bad);
    __syncthreads();
    // ---- target pass: y = rew + (gamma (1 - term)) max_a Qt, K19's operation order ----
    sq_forward<ACT>(L, DP, H0, H1, KP, slope);
    if (t < 32) {
        const float *tq = L.q + t * KP;
        float m = tq[0];
        for (int k = 1; k < A; ++k) m = fmaxf(m, tq[k]);
        y_s[t] = __fadd_rn(rew_s[t], __fmul_rn(__fmul_rn(a.gamma, __fsub_rn(1.0f, term_s[t])), m));
    }
    __syncthreads();   // q and every image of the target network are dead from here
    // ---- eval pass ----
    sq_stage_net(L, a.W0, a.b0, a.W1, a.b1, a.Wq, a.bq, D, DP, H0, H1, A, KP);
    sq_stage_rows(L, a.obs, a.obs_ld, s_rows, B, D, DP);
    __syncthreads();
    sq_forward<ACT>(L, DP, H0, H1, KP, slope);
    // W1 row-major over its transposed image for dh0 (the forward was the image's last reader): loads issued now
    float w1v[4][8];
    const int nW1 = H1 * H0;
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = t + (s * 8 + u) * kSqThreads;
            w1v[s][u] = e < nW1 ? a.W1[e] : 0.f;
        }
    // TD error, |TD|, dq (K19) and the workgroup's loss sums (f64, wave 0 holds the 32 rows)
    if (w == 0) {
        double sq = 0.0, ps = 0.0;
        if (lane < 32) {
            float dq = 0.f;
            if (lane < B) {
                const float p = L.q[lane * KP + (int)act_s[lane]], y = y_s[lane];
                const float d = p - y;
                a.td_abs[r0 + lane] = fabsf(y - p);
                dq = (2.0f / (float)Btot) * d;
                sq = (double)d * (double)d;
                ps = (double)p;
            }
            dq_s[lane] = dq;
        }
        sq = xpa_wave_sum(sq);
        ps = xpa_wave_sum(ps);
        if (lane == 0) {
            a.loss_part[2 * gi] = sq;
            a.loss_part[2 * gi + 1] = ps;
        }
    }
    __syncthreads();
    // ---- backward ----
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = t + (s * 8 + u) * kSqThreads;
            if (e < nW1) L.W1i[e] = w1v[s][u];
        }
    // output layer: gWq [A][H1] and gbq [A] as per-action sums over the rows (dq is 0 on rows >= B)
    for (int e = t; e < A * H1; e += kSqThreads) {
        const int k = e / H1, j = e % H1;
        const float *h = L.h1T + j * kSqS;
        float s = 0.f;
        for (int b = 0; b < 32; b += 4) {
            const float4 v = *reinterpret_cast<const float4 *>(h + b);
            s += ((int)act_s[b] == k ? dq_s[b] : 0.f) * v.x;
            s += ((int)act_s[b + 1] == k ? dq_s[b + 1] : 0.f) * v.y;
            s += ((int)act_s[b + 2] == k ? dq_s[b + 2] : 0.f) * v.z;
            s += ((int)act_s[b + 3] == k ? dq_s[b + 3] : 0.f) * v.w;
        }
        gp(a.gWq)[e] = s;
    }
    if (t >= kSqThreads - A) {
        const int k = kSqThreads - 1 - t;
        float s = 0.f;
        for (int b = 0; b < 32; ++b) s += (int)act_s[b] == k ? dq_s[b] : 0.f;
        gp(a.gbq)[k] = s;
    }
    __syncthreads();
    // dz1 = dq Wq[act][:] act'(h1), in place over h1
    for (int e = t; e < H1 * 32; e += kSqThreads) {
        const int j = e >> 5, b = e & 31;
        float *p = L.h1T + j * kSqS + b;
        *p = dq_s[b] * L.WqT[j * KP + (int)act_s[b]] * sm_grad<ACT>(*p, slope);
    }
    __syncthreads();
    // gW1 [H1][H0] = dz1^T h0
    for (int tl = w; tl < (H1 / 32) * (H0 / 32); tl += kSqWaves) {
        const int j0 = 32 * (tl % (H1 / 32)), i0 = 32 * (tl / (H1 / 32));
        const f32x16 acc = sm_tile(L.h1T + j0 * kSqS, kSqS, 1, 32, L.h0T + i0 * kSqS, 1, kSqS, 32, 32);
        float *gW = gp(a.gW1);
#pragma unroll
        for (int r = 0; r < 16; ++r) gW[(j0 + sm_row(r)) * H0 + i0 + li] = acc[r];
    }
    __syncthreads();
    // dz0 = (dz1 W1) act'(h0), in place over h0
    for (int tl = w; tl < H0 / 32; tl += kSqWaves) {
        const int i0 = 32 * tl;
        const f32x16 acc = sm_tile(L.h1T, 1, kSqS, 32, L.W1i + i0, H0, 1, 32, H1);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float *p = L.h0T + (i0 + li) * kSqS + sm_row(r);
            *p = acc[r] * sm_grad<ACT>(*p, slope);
        }
    }
    __syncthreads();
    // gW0 [H0][D] = dz0^T x, and the hidden layers' bias gradients (row sums over the 32 rows, 16-B reads)
    for (int tl = w; tl < H0 / 32; tl += kSqWaves) {
        const int i0 = 32 * tl;
        const f32x16 acc = sm_tile(L.h0T + i0 * kSqS, kSqS, 1, 32, L.xT, 1, kSqS, DP, 32);
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (li < D) gp(a.gW0)[(i0 + sm_row(r)) * D + li] = acc[r];
    }
    for (int f = t; f < H0 + H1; f += kSqThreads) {
        const float *src = f < H0 ? L.h0T + f * kSqS : L.h1T + (f - H0) * kSqS;
        float *dst = f < H0 ? gp(a.gb0) + f : gp(a.gb1) + (f - H0);
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        for (int b = 0; b < 32; b += 4) {
            const float4 v = *reinterpret_cast<const float4 *>(src + b);
            s0 += v.x;
            s1 += v.y;
            s2 += v.z;
            s3 += v.w;
        }
        *dst = (s0 + s1) + (s2 + s3);
    }
}

// The second launch (one workgroup): loss scalars, the gradient as the sum of the workgroups' partials in workgroup
// order, Adam without clipping (K9's element arithmetic) at the schedule cursor, then the hard target update.
__global__ __launch_bounds__(kSqThreads, 1) void small_q_finalize_kernel(XpaSmallQArgs a) {
    __shared__ float s_step, s_inv;
    const int t = threadIdx.x, G = a.n_groups;
    if (t == 0) {
        double sq = 0.0, ps = 0.0;
        for (int g = 0; g < G; ++g) {
            sq += a.loss_part[2 * g];
            ps += a.loss_part[2 * g + 1];
        }
        a.scalars[0] = (float)(sq / (double)a.batch);   // Qloss
        a.scalars[1] = (float)(ps / (double)a.batch);   // predictQ mean
        int k = a.cursor[0];
        if (k >= a.n_sched) {
            a.cursor[2] = 1;
            k = a.n_sched - 1;
        }
        s_step = a.sched[2 * k];
        s_inv = a.sched[2 * k + 1];
    }
    __syncthreads();
    const float step_size = s_step, inv_bc2_sqrt = s_inv, b1 = a.beta1, b2 = a.beta2, eps = a.eps;
    const int64_t n4 = a.n / 4;
    const float4 *part4 = reinterpret_cast<const float4 *>(a.grad_part);
    float4 *p4 = reinterpret_cast<float4 *>(a.param), *g4 = reinterpret_cast<float4 *>(a.grad);
    float4 *m4 = reinterpret_cast<float4 *>(a.exp_avg), *v4 = reinterpret_cast<float4 *>(a.exp_avg_sq);
    for (int64_t i0 = t; i0 < n4; i0 += 2 * kSqThreads) {
        float4 Q[2][kSqMaxGroups], P[2], M[2], V[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int64_t i = i0 + u * kSqThreads < n4 ? i0 + u * kSqThreads : n4 - 1;
#pragma unroll
            for (int g = 0; g < kSqMaxGroups; ++g)
                if (g < G) Q[u][g] = part4[(int64_t)g * n4 + i];
            P[u] = p4[i];
            M[u] = m4[i];
            V[u] = v4[i];
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            float4 sg = Q[u][0];
#pragma unroll
            for (int g = 1; g < kSqMaxGroups; ++g)
                if (g < G) {
                    sg.x += Q[u][g].x;
                    sg.y += Q[u][g].y;
                    sg.z += Q[u][g].z;
                    sg.w += Q[u][g].w;
                }
            float *pp = &P[u].x, *gg = &sg.x, *mm = &M[u].x, *vv = &V[u].x;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float g = gg[c];
                float m = mm[c], v = vv[c];
                m = m + (1.0f - b1) * (g - m);
                v = b2 * v + (1.0f - b2) * g * g;
                const float denom = sqrtf(v) * inv_bc2_sqrt + eps;
                pp[c] = pp[c] - step_size * (m / denom);
                mm[c] = m;
                vv[c] = v;
            }
            if (i0 + u * kSqThreads < n4) {
                const int64_t i = i0 + u * kSqThreads;
                p4[i] = P[u];
                g4[i] = sg;
                m4[i] = M[u];
                v4[i] = V[u];
            }
        }
    }
    if (a.sync_target) {
        // the updated parameters, written by this workgroup, land before the copies read them (and the target spans'
        // own Adam stores, which leave them unchanged, before the copies' stores)
        xpa_drain();
        __syncthreads();
        const int D = a.d_in, H0 = a.h0, H1 = a.h1, A = a.k;
        for (int e = t; e < H1 * H0; e += kSqThreads) a.tW1[e] = a.W1[e];
        for (int e = t; e < H0 * D; e += kSqThreads) a.tW0[e] = a.W0[e];
        for (int e = t; e < A * H1; e += kSqThreads) a.tWq[e] = a.Wq[e];
        for (int e = t; e < H0; e += kSqThreads) a.tb0[e] = a.b0[e];
        for (int e = t; e < H1; e += kSqThreads) a.tb1[e] = a.b1[e];
        for (int e = t; e < A; e += kSqThreads) a.tbq[e] = a.bq[e];
    }
    if (t == 0) a.cursor[0] = a.cursor[0] + 1;
}

// The forward alone: the eval network on rows [n, ld], one workgroup per 32 rows
template <int ACT>
__global__ __launch_bounds__(kSqThreads, 1) void small_q_values_kernel(XpaSmallQArgs a, const float *__restrict__ rows,
                                                                       int64_t ld, int64_t n,
                                                                       float *__restrict__ q_out) {
    __shared__ __attribute__((aligned(16))) float lds[kSqLds];
    __shared__ int64_t s_rows[32];
    const int t = threadIdx.x;
    const int64_t r0 = 32 * (int64_t)blockIdx.x;
    const int B = (int)(n - r0 < 32 ? n - r0 : 32);
    const int D = a.d_in, DP = (a.d_in + 3) & ~3, H0 = a.h0, H1 = a.h1, A = a.k, KP = (a.k + 3) & ~3;
    const SqLds L = sq_carve(lds, DP, H0, H1, KP);
    if (t < 32) s_rows[t] = t < B ? r0 + t : 0;
    sq_stage_net(L, a.W0, a.b0, a.W1, a.b1, a.Wq, a.bq, D, DP, H0, H1, A, KP);
    __syncthreads();
    sq_stage_rows(L, rows, ld, s_rows, B, D, DP);
    __syncthreads();
    sq_forward<ACT>(L, DP, H0, H1, KP, a.slope);
    for (int e = t; e < B * A; e += kSqThreads) q_out[r0 * A + e] = L.q[(e / A) * KP + e % A];
}

bool sq_width_ok(int64_t h) { return h == 32 || h == 64 || h == 128; }

}  // namespace

XPA_API int64_t xpa_small_q_lds_floats(int64_t rows, int64_t d_in, int64_t h0, int64_t h1, int64_t k) {
    const int64_t S = ((rows + 31) & ~(int64_t)31) + 4, DP = (d_in + 3) & ~3, KP = (k + 3) & ~3;
    return DP * S + (h0 + h1) * S + DP * h0 + ((h0 * (h1 + 1) + 3) & ~(int64_t)3) + h1 * KP + h0 + h1 + KP + 6 * 32 +
           32 * KP;
}

XPA_API int xpa_small_q_ok(int64_t batch, int64_t d_in, int64_t h0, int64_t h1, int64_t k) {
    return batch >= 1 && batch <= 32 * kSqMaxGroups && d_in >= 1 && d_in <= 32 && sq_width_ok(h0) && sq_width_ok(h1) &&
           k >= 2 && k <= 16 && xpa_small_q_lds_floats(32, d_in, h0, h1, k) <= kSqLds;
}

XPA_API int xpa_small_q_update(const XpaSmallQArgs *args, xpa_stream_t stream) {
    if (!args) return (int)hipErrorInvalidValue;
    const XpaSmallQArgs &a = *args;
    if (!xpa_small_q_ok(a.batch, a.d_in, a.h0, a.h1, a.k) || a.act_code < 0 || a.act_code > 2 ||
        a.n_groups != (a.batch + 31) / 32 || a.n_sched < 1 || a.n < 4 || a.n % 4 || a.n_rows < 1 || a.obs_ld < a.d_in ||
        !a.obs || !a.next || !a.act || !a.rew || !a.term || !a.W0 || !a.b0 || !a.W1 || !a.b1 || !a.Wq || !a.bq ||
        !a.tW0 || !a.tb0 || !a.tW1 || !a.tb1 || !a.tWq || !a.tbq || !a.param || !a.grad || !a.exp_avg ||
        !a.exp_avg_sq || !a.sched || !a.cursor || !a.td_abs || !a.scalars || !a.grad_part || !a.loss_part ||
        ((uintptr_t)a.param | (uintptr_t)a.grad | (uintptr_t)a.exp_avg | (uintptr_t)a.exp_avg_sq |
         (uintptr_t)a.grad_part) % 16)
        return (int)hipErrorInvalidValue;
    // every gradient view inside the flat gradient: the partials mirror its offsets
    const struct { const float *p; int64_t len; } views[6] = {
        {a.gW0, (int64_t)a.h0 * a.d_in}, {a.gb0, a.h0}, {a.gW1, (int64_t)a.h1 * a.h0}, {a.gb1, a.h1},
        {a.gWq, (int64_t)a.k * a.h1}, {a.gbq, a.k}};
    for (const auto &v : views)
        if (!v.p || v.p < a.grad || v.p + v.len > a.grad + a.n) return (int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(a.n_groups), block(kSqThreads);
    if (a.act_code == 0) hipLaunchKernelGGL((small_q_update_kernel<0>), grid, block, 0, s, a);
    else if (a.act_code == 1) hipLaunchKernelGGL((small_q_update_kernel<1>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((small_q_update_kernel<2>), grid, block, 0, s, a);
    hipLaunchKernelGGL(small_q_finalize_kernel, dim3(1), block, 0, s, a);
    return xpa_launch_status();
}

XPA_API int xpa_small_q_values(const XpaSmallQArgs *args, const float *rows, int64_t ld, int64_t n, float *q_out,
                               xpa_stream_t stream) {
    if (!args) return (int)hipErrorInvalidValue;
    const XpaSmallQArgs &a = *args;
    if (!xpa_small_q_ok(1, a.d_in, a.h0, a.h1, a.k) || a.act_code < 0 || a.act_code > 2 || !a.W0 || !a.b0 || !a.W1 ||
        !a.b1 || !a.Wq || !a.bq || !rows || !q_out || n < 1 || n > 32 * (int64_t)65535 || ld < a.d_in)
        return (int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((n + 31) / 32)), block(kSqThreads);
    if (a.act_code == 0) hipLaunchKernelGGL((small_q_values_kernel<0>), grid, block, 0, s, a, rows, ld, n, q_out);
    else if (a.act_code == 1) hipLaunchKernelGGL((small_q_values_kernel<1>), grid, block, 0, s, a, rows, ld, n, q_out);
    else hipLaunchKernelGGL((small_q_values_kernel<2>), grid, block, 0, s, a, rows, ld, n, q_out);
    return xpa_launch_status();
}
