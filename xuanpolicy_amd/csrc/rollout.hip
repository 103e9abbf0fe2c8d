// Rollout-side kernels of the fused on-policy pipeline (gfx950):
//   K4 xpa_gather_minibatch  minibatch row gather + advantage moments (memory_tools.py:231-242)
//   K5 xpa_rms_*             RunningMeanStd + obs normalisation (statistic_tools.py:63-112, agent.py:104-116)
//   K3 xpa_rollout_sample    action sample + log-prob + buffer store (ppoclip_agent.py:50-57, memory_tools.py:196-204)
//   K7 xpa_synthbox_step     synthetic env step with auto-reset (gym_vec_env.py:201-212 contract)
//   K8 xpa_rollout_post      reward norm, return tracker, ret_rms, path closures (ppoclip_agent.py:68-101)
// All per-step kernels read the buffer column from a device cursor so a whole env step can be
// captured once in a hipGraph and replayed.
#include "acrobot_body.h"
#include "cartpole_body.h"
#include "mountaincar_body.h"
#include "pendulum_body.h"

#include <algorithm>
#include <vector>

namespace {

constexpr int kGatherRows = 64;  // rows per gather block == rows per adv partial (1024 blocks at B = 65 536)
constexpr int kRmsRows = 256;     // rows per RMS partial block
// threads per RMS partial block: 1024 for wide observations (r02: with 256, C4's 376 columns had one thread per column
// walking all 256 rows, 43.8 us per env step -> 17.9 us), 256 for narrow ones (C1 / C2: the reduction and the merge
// stay as short as before)
constexpr int kRmsWideDim = 64;
constexpr uint32_t kSaltAct = 0xAC7105EDu;
constexpr uint32_t kSaltReset = 0x5EED0000u;  // oracle/synth_env.py SALT_RESET

// ---------------------------------------------------------------------------------------------
// K4 gather
// ---------------------------------------------------------------------------------------------
template <typename V>
__global__ __launch_bounds__(256) void gather_rows_kernel(const int64_t *__restrict__ idx, int64_t batch,
                                                          int64_t n_rows, const V *__restrict__ src, int64_t row_vecs,
                                                          V *__restrict__ dst, const float *__restrict__ adv,
                                                          double *__restrict__ adv_partials, int *__restrict__ err,
                                                          int64_t out_vecs = -1) {
    __shared__ double s_red[4];
    __shared__ int64_t s_src[kGatherRows];
    const int64_t r0 = (int64_t)blockIdx.x * kGatherRows;
    const int64_t r1 = r0 + kGatherRows < batch ? r0 + kGatherRows : batch;
    const int nr = (int)(r1 - r0);
    if ((int)threadIdx.x < nr) {
        const int64_t sr = idx[r0 + threadIdx.x];
        s_src[threadIdx.x] = sr;
        if (err && (sr < 0 || sr >= n_rows)) atomicAdd(err, 1);  // the row is zero-filled, and counted
    }
    __syncthreads();
    // Consecutive lanes copy consecutive vectors of a row (32-bit index math; the row's source offset
    // comes from LDS), so each row is one contiguous burst.
    // out_vecs (r05): the output row pitch in vectors (-1: packed rows); the pitch's tail of each row is not written
    const uint32_t rv = (uint32_t)row_vecs;
    const uint32_t n = (uint32_t)nr * rv;
    const int64_t op = out_vecs < 0 ? row_vecs : out_vecs;
    V *out = dst + r0 * op;
    for (uint32_t e = threadIdx.x; e < n; e += 256) {
        const uint32_t r = e / rv;
        const uint32_t c = e - r * rv;
        const int64_t sr = s_src[r];
        out[(int64_t)r * op + c] = (sr >= 0 && sr < n_rows) ? src[sr * row_vecs + c] : V{};
    }
    if (adv_partials) {
        double s = 0.0, q = 0.0;
        const int64_t sr = (int)threadIdx.x < nr ? s_src[threadIdx.x] : -1;
        if (sr >= 0 && sr < n_rows) {
            const double a = (double)adv[sr];
            s = a;
            q = a * a;
        }
        s = xpa_block_sum(s, s_red, 4);
        q = xpa_block_sum(q, s_red, 4);
        if (threadIdx.x == 0) {
            adv_partials[2 * blockIdx.x] = s;
            adv_partials[2 * blockIdx.x + 1] = q;
        }
    }
}

// Wide rows (>= 4 KiB, e.g. 4x84x84 uint8 frames of the replay buffer): one block per (row, 16 KiB
// chunk), four independent 16-B non-temporal loads per thread in flight.
constexpr int kWideU = 4;
typedef unsigned int u4v __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void gather_wide_kernel(const int64_t *__restrict__ idx, int64_t n_rows,
                                                          const u4v *__restrict__ src, int64_t row_vecs,
                                                          int64_t chunks, u4v *__restrict__ dst, int *__restrict__ err) {
    const int64_t row = (int64_t)blockIdx.x / chunks, chunk = (int64_t)blockIdx.x - row * chunks;
    const int64_t sr = idx[row];
    const bool ok = sr >= 0 && sr < n_rows;
    if (err && !ok && chunk == 0 && threadIdx.x == 0) atomicAdd(err, 1);
    const int64_t c0 = chunk * 256 * kWideU + threadIdx.x;
    u4v v[kWideU];
#pragma unroll
    for (int u = 0; u < kWideU; ++u) {
        const int64_t c = c0 + u * 256;
        v[u] = (ok && c < row_vecs) ? __builtin_nontemporal_load(src + sr * row_vecs + c) : u4v{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int u = 0; u < kWideU; ++u) {
        const int64_t c = c0 + u * 256;
        if (c < row_vecs) __builtin_nontemporal_store(v[u], dst + row * row_vecs + c);
    }
}

// Column store: dst[(n * horizon + cursor->ptr) * row_vecs + c] = src[n * row_vecs + c] (raw uint8
// Atari observations into the rollout buffer, DummyOnPolicyBuffer_Atari.store, memory_tools.py:196-204).
__global__ __launch_bounds__(256) void store_column_kernel(const u4v *__restrict__ src, int64_t n, int64_t row_vecs,
                                                           u4v *__restrict__ dst, int64_t horizon,
                                                           const xpa_cursor_t *__restrict__ cur) {
    const int64_t t = cur->ptr;
    const int64_t total = n * row_vecs;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t r = e / row_vecs, c = e - r * row_vecs;
        __builtin_nontemporal_store(__builtin_nontemporal_load(src + e), dst + (r * horizon + t) * row_vecs + c);
    }
}

// Epoch permutation of [0, n) (the np.random.shuffle of ppoclip_agent.py:76-81): a 4-round Feistel
// network over 2h bits (2^(2h) >= n) keyed by a counter hash of (seed, counter), cycle-walked into
// [0, n) — a bijection computed independently per element, one launch, no sort.
constexpr uint32_t kSaltPerm = 0x9E2A0000u;
__device__ __forceinline__ uint32_t feistel(uint32_t x, int h, uint32_t seed, uint32_t counter) {
    const uint32_t mask = (1u << h) - 1u;
    uint32_t L = x >> h, R = x & mask;
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
        const uint32_t F = xpa_hash4(seed ^ kSaltPerm, counter, r, R) & mask;
        const uint32_t nl = R;
        R = L ^ F;
        L = nl;
    }
    return (L << h) | R;
}

__global__ __launch_bounds__(256) void permutation_kernel(int64_t n, int h, uint32_t seed, uint32_t counter,
                                                          int64_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t x = (uint32_t)i;
    do {
        x = feistel(x, h, seed, counter);
    } while ((int64_t)x >= n);
    out[i] = (int64_t)x;
}

// permutation_kernel over grid (blocks, P): row blockIdx.y of out [P, n] is agent blockIdx.y's permutation, keyed by
// its own (seed, counter) — element for element what permutation_kernel writes for that key
__global__ __launch_bounds__(256) void permutation_batch_kernel(int64_t n, int h, const uint32_t *__restrict__ seeds,
                                                                const uint32_t *__restrict__ counters,
                                                                int64_t *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t seed = seeds[blockIdx.y], counter = counters[blockIdx.y];
    uint32_t x = (uint32_t)i;
    do {
        x = feistel(x, h, seed, counter);
    } while ((int64_t)x >= n);
    out[(int64_t)blockIdx.y * n + i] = (int64_t)x;
}

// ---------------------------------------------------------------------------------------------
// K5 RunningMeanStd
// ---------------------------------------------------------------------------------------------
// Block g sums rows [g*kRmsRows, (g+1)*kRmsRows) of (x - shift) and (x - shift)^2 in f64 per column
// (shift = the running mean, so the one-pass variance does not cancel).  Threads cover a
// (row group x column) tile, all row loads of a thread are independent (no serial latency chain),
// and the row groups are combined through LDS in a fixed order.
__device__ void rms_merge_body(const double *part, int64_t np, int64_t n, int64_t dim, float *__restrict__ mean,
                               float *__restrict__ var, double *__restrict__ count);

// MERGE: the last block to finish (atomic ticket) also runs the merge below over all blocks' partials in
// block order (deterministic, = xpa_rms_merge) and resets the ticket: one launch per obs-RMS update.
template <bool MERGE, int kRmsThreads>
__global__ __launch_bounds__(kRmsThreads) void rms_partials_kernel(const float *__restrict__ x, int64_t n, int64_t dim,
                                                                   int64_t ld, const float *shift,  // may alias mean
                                                                   double *__restrict__ part, float *mean,
                                                                   float *__restrict__ var, double *__restrict__ count,
                                                                   unsigned int *__restrict__ ticket) {
    __shared__ double s_sum[kRmsThreads], s_sq[kRmsThreads];
    __shared__ bool s_last;
    const int64_t r0 = (int64_t)blockIdx.x * kRmsRows;
    const int64_t r1 = r0 + kRmsRows < n ? r0 + kRmsRows : n;
    const int64_t np = gridDim.x;
    for (int64_t c0 = 0; c0 < dim; c0 += 256) {
        const int dc = (int)(dim - c0 < 256 ? dim - c0 : 256);  // columns in this tile
        const int groups = kRmsThreads / dc;                    // row groups
        const int c = threadIdx.x % dc, gsub = threadIdx.x / dc;
        double s = 0.0, q = 0.0;
        if (gsub < groups) {
            const float sh = shift ? shift[c0 + c] : 0.f;
            // 16 rows' loads issued before their (in-order) accumulation: one memory round trip per 16 rows (the
            // unroll-4 loop waited once per 4 rows: ~5 serial HBM round trips per thread at C2's 17 columns)
            for (int64_t rb = r0 + gsub; rb < r1; rb += 16 * (int64_t)groups) {
                float xv[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) {
                    const int64_t r = rb + (int64_t)u * groups;
                    xv[u] = x[(r < r1 ? r : rb) * ld + c0 + c];
                }
#pragma unroll
                for (int u = 0; u < 16; ++u)
                    if (rb + (int64_t)u * groups < r1) {
                        const double v = (double)xv[u] - (double)sh;
                        s += v;
                        q += v * v;
                    }
            }
        }
        s_sum[threadIdx.x] = s;
        s_sq[threadIdx.x] = q;
        __syncthreads();
        if ((int)threadIdx.x < dc) {
            double ts = 0.0, tq = 0.0;
            for (int k = 0; k < groups; ++k) {
                ts += s_sum[k * dc + threadIdx.x];
                tq += s_sq[k * dc + threadIdx.x];
            }
            xpa_store_agent(part + (int64_t)blockIdx.x * dim + c0 + threadIdx.x, ts);  // sc1: handed to the
            xpa_store_agent(part + (np + blockIdx.x) * dim + c0 + threadIdx.x, tq);    // merging block
        }
        __syncthreads();
    }
    if (MERGE) {
        xpa_drain();
        __syncthreads();
        if (threadIdx.x == 0) s_last = xpa_ticket(ticket) == (unsigned)(np - 1);
        __syncthreads();
        if (!s_last) return;
        rms_merge_body(part, np, n, dim, mean, var, count);
        if (threadIdx.x == 0) *ticket = 0u;
    }
}

// r05, wide observations (dim > kRmsWideDim, C4's 376): the same partials from a 2-D grid — block (g, cb) takes row
// block g (kRmsRows rows) x columns 64 cb .. + 63, thread (group j, column c) sums rows j, j + 16, ... (16 loads in
// flight) and the 16 groups are added in order — so np x ceil(dim / 64) blocks share the chip (the 1-D form ran the
// 16 row blocks of a 4096-env step on 16 CUs: 21.5 us); the last of all the blocks merges (rms_merge_body, np = gridDim.x)
template <bool MERGE>
__global__ __launch_bounds__(1024) void rms_partials_cols_kernel(const float *__restrict__ x, int64_t n, int64_t dim,
                                                                  int64_t ld, const float *shift,
                                                                  double *__restrict__ part, float *mean,
                                                                  float *__restrict__ var, double *__restrict__ count,
                                                                  unsigned int *__restrict__ ticket) {
    __shared__ double s_sum[16][64], s_sq[16][64];
    __shared__ bool s_last;
    const int64_t r0 = (int64_t)blockIdx.x * kRmsRows;
    const int64_t r1 = r0 + kRmsRows < n ? r0 + kRmsRows : n;
    const int64_t np = gridDim.x;
    const int64_t c0 = (int64_t)blockIdx.y * 64;
    const int c = threadIdx.x & 63, j = threadIdx.x >> 6;
    double s = 0.0, q = 0.0;
    if (c0 + c < dim) {
        const float sh = shift ? shift[c0 + c] : 0.f;
        for (int64_t rb = r0 + j; rb < r1; rb += 16 * 16) {
            float xv[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int64_t r = rb + (int64_t)u * 16;
                xv[u] = x[(r < r1 ? r : rb) * ld + c0 + c];
            }
#pragma unroll
            for (int u = 0; u < 16; ++u)
                if (rb + (int64_t)u * 16 < r1) {
                    const double v = (double)xv[u] - (double)sh;
                    s += v;
                    q += v * v;
                }
        }
    }
    s_sum[j][c] = s;
    s_sq[j][c] = q;
    __syncthreads();
    if (threadIdx.x < 64 && c0 + threadIdx.x < dim) {
        double ts = s_sum[0][threadIdx.x], tq = s_sq[0][threadIdx.x];
#pragma unroll
        for (int k = 1; k < 16; ++k) {
            ts += s_sum[k][threadIdx.x];
            tq += s_sq[k][threadIdx.x];
        }
        xpa_store_agent(part + (int64_t)blockIdx.x * dim + c0 + threadIdx.x, ts);
        xpa_store_agent(part + (np + blockIdx.x) * dim + c0 + threadIdx.x, tq);
    }
    if (MERGE) {
        xpa_drain();
        __syncthreads();
        if (threadIdx.x == 0) s_last = xpa_ticket(ticket) == (unsigned)(gridDim.x * gridDim.y - 1);
        __syncthreads();
        if (!s_last) return;
        rms_merge_body(part, np, n, dim, mean, var, count);
        if (threadIdx.x == 0) *ticket = 0u;
    }
}

// Sum of the partials (fixed order) -> batch mean/var, then update_from_moments
// (statistic_tools.py:86-112) into mean/var (f32) and count (f64).  mean doubles as the shift the
// partials were taken around.
// Every (partial, column) sum / square is loaded by its own thread into LDS in one round trip (sc1 loads:
// the partials may come from other blocks of the same launch), then each column is summed over the
// partials in block order (deterministic).
constexpr int kMergeLds = 2048;  // doubles of LDS staging: np * dim <= 1024 (else per-column global loads)
// column d of the merge: s / q = the batch's sums of (x - mean[d]) and its square over n rows, c0 = the running count
__device__ __forceinline__ void rms_merge_col(double s, double q, double n, double c0, float *mean, float *var,
                                              int64_t d) {
    const double ms = s / n;
    const double m0 = (double)mean[d], v0 = (double)var[d];
    const double bm = m0 + ms;                        // batch mean
    const double bvar = fmax(q / n - ms * ms, 0.0);   // np.std(x, axis=0)**2 (ddof 0)
    const double tot = c0 + n;
    const double delta = bm - m0;
    const double new_mean = m0 + delta * n / tot;
    const double m2 = v0 * c0 + bvar * n + delta * delta * c0 * n / tot;
    mean[d] = (float)new_mean;
    var[d] = (float)(m2 / tot);
}

__device__ void rms_merge_body(const double *part, int64_t np, int64_t n, int64_t dim, float *__restrict__ mean,
                               float *__restrict__ var, double *__restrict__ count) {
    __shared__ double s_part[kMergeLds];
    const double c0 = *count;
    const bool staged = np * dim * 2 <= kMergeLds;
    if (staged)
        for (int64_t i = threadIdx.x; i < 2 * np * dim; i += blockDim.x) s_part[i] = xpa_load_agent(part + i);
    __syncthreads();
    for (int64_t d = threadIdx.x; d < dim; d += blockDim.x) {
        double s = 0.0, q = 0.0;
        for (int64_t p = 0; p < np; ++p) {
            s += staged ? s_part[p * dim + d] : xpa_load_agent(part + p * dim + d);
            q += staged ? s_part[(np + p) * dim + d] : xpa_load_agent(part + (np + p) * dim + d);
        }
        rms_merge_col(s, q, (double)n, c0, mean, var, d);
    }
    __syncthreads();
    if (threadIdx.x == 0) *count = c0 + (double)n;
}

__global__ __launch_bounds__(256) void rms_merge_kernel(const double *__restrict__ part, int64_t np, int64_t n,
                                                        int64_t dim, float *__restrict__ mean, float *__restrict__ var,
                                                        double *__restrict__ count) {
    rms_merge_body(part, np, n, dim, mean, var, count);
}

__global__ __launch_bounds__(256) void obs_normalize_kernel(const float *__restrict__ x, int64_t n, int64_t dim,
                                                            int64_t ldx, const float *__restrict__ mean,
                                                            const float *__restrict__ var, float clip_range,
                                                            float *__restrict__ out, int64_t ldo,
                                                            float *__restrict__ col_out, int64_t col_ld,
                                                            const xpa_cursor_t *__restrict__ cursor) {
    const int64_t total = n * dim;
    const int64_t coff = (col_out && cursor) ? (int64_t)cursor->ptr * dim : 0;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = e / dim, d = e % dim;
        const float sd = sqrtf(var[d]);
        float y = (x[r * ldx + d] - mean[d]) / (sd + 1e-8f);
        y = fminf(fmaxf(y, -clip_range), clip_range);
        out[r * ldo + d] = y;
        if (col_out) col_out[r * col_ld + coff + d] = y;
    }
}

// ---------------------------------------------------------------------------------------------
// K3 sample + log-prob + store
// ---------------------------------------------------------------------------------------------
// Returns the clipped action of the last dimension (K32 steps its one-torque env with it: A = 1).
__device__ __forceinline__ float gauss_sample_store_at(int64_t n, int A, int64_t T, int32_t t, uint32_t step,
                                                       const float *mu_row, const float *__restrict__ logstd, float v,
                                                       uint32_t seed, float act_clip, float *__restrict__ buf_act,
                                                       float *__restrict__ buf_logp, float *__restrict__ buf_val,
                                                       float *__restrict__ env_in, int64_t ld_env) {
    const int64_t cell = n * T + t;
    float logp = 0.f, clipped = 0.f;
    for (int a = 0; a < A; ++a) {
        const uint32_t h1 = xpa_hash4(seed ^ kSaltAct, step, (uint32_t)n, (uint32_t)(2 * a));
        const uint32_t h2 = xpa_hash4(seed ^ kSaltAct, step, (uint32_t)n, (uint32_t)(2 * a + 1));
        const float u1 = 1.0f - xpa_u01(h1);  // (0, 1]
        const float u2 = xpa_u01(h2);
        const float eps = sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
        const float sc = expf(logstd[a]);
        const float m = mu_row[a];
        const float x = m + sc * eps;
        const float diff = x - m;
        logp += -(diff * diff) / (2.0f * sc * sc) - logf(sc) - 0.91893853320467274178f;
        buf_act[cell * A + a] = x;
        clipped = fminf(fmaxf(x, -act_clip), act_clip);
        env_in[n * ld_env + a] = clipped;
    }
    buf_logp[cell] = logp;
    buf_val[cell] = v;
    return clipped;
}

__device__ __forceinline__ void gauss_sample_store(int64_t n, int A, int64_t T, const float *mu_row,
                                                   const float *__restrict__ logstd, float v,
                                                   const xpa_cursor_t *__restrict__ cur, uint32_t seed, float act_clip,
                                                   float *__restrict__ buf_act, float *__restrict__ buf_logp,
                                                   float *__restrict__ buf_val, float *__restrict__ env_in,
                                                   int64_t ld_env) {
    gauss_sample_store_at(n, A, T, cur->ptr, cur->step, mu_row, logstd, v, seed, act_clip, buf_act, buf_logp, buf_val,
                          env_in, ld_env);
}

// Returns the sampled action (K32 steps its env with it).
__device__ __forceinline__ int cat_sample_store_at(int64_t n, int K, int64_t T, int32_t t, uint32_t step,
                                                   const float *z, float v, uint32_t seed, float *__restrict__ buf_act,
                                                   float *__restrict__ buf_logp, float *__restrict__ buf_val,
                                                   float *__restrict__ env_in, int64_t ld_env) {
    const int64_t cell = n * T + t;
    float m = z[0];
    for (int k = 1; k < K; ++k) m = fmaxf(m, z[k]);
    float se = 0.f;
    for (int k = 0; k < K; ++k) se += expf(z[k] - m);
    const float lse = m + logf(se);
    const float u = xpa_u01(xpa_hash4(seed ^ kSaltAct, step, (uint32_t)n, 0u));
    int pick = K - 1;
    float cdf = 0.f;
    for (int k = 0; k < K; ++k) {
        cdf += expf(z[k] - lse);
        if (u < cdf) {
            pick = k;
            break;
        }
    }
    buf_act[cell] = (float)pick;
    buf_logp[cell] = z[pick] - lse;
    buf_val[cell] = v;
    for (int k = 0; k < K; ++k) env_in[n * ld_env + k] = (k == pick) ? 1.f : 0.f;
    return pick;
}

__device__ __forceinline__ void cat_sample_store(int64_t n, int K, int64_t T, const float *z, float v,
                                                 const xpa_cursor_t *__restrict__ cur, uint32_t seed,
                                                 float *__restrict__ buf_act, float *__restrict__ buf_logp,
                                                 float *__restrict__ buf_val, float *__restrict__ env_in,
                                                 int64_t ld_env) {
    cat_sample_store_at(n, K, T, cur->ptr, cur->step, z, v, seed, buf_act, buf_logp, buf_val, env_in, ld_env);
}

__global__ __launch_bounds__(256) void rollout_sample_gauss_kernel(
    int64_t n_envs, int A, int64_t T, const float *__restrict__ mu, const float *__restrict__ logstd,
    const float *__restrict__ v, const xpa_cursor_t *__restrict__ cur, uint32_t seed, float act_clip,
    float *__restrict__ buf_act, float *__restrict__ buf_logp, float *__restrict__ buf_val, float *__restrict__ env_in,
    int64_t ld_env) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_envs) return;
    gauss_sample_store(n, A, T, mu + n * A, logstd, v[n], cur, seed, act_clip, buf_act, buf_logp, buf_val, env_in,
                       ld_env);
}

__global__ __launch_bounds__(256) void rollout_sample_cat_kernel(
    int64_t n_envs, int K, int64_t T, const float *__restrict__ logits, const float *__restrict__ v,
    const xpa_cursor_t *__restrict__ cur, uint32_t seed, float *__restrict__ buf_act, float *__restrict__ buf_logp,
    float *__restrict__ buf_val, float *__restrict__ env_in, int64_t ld_env) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_envs) return;
    cat_sample_store(n, K, T, logits + n * K, v[n], cur, seed, buf_act, buf_logp, buf_val, env_in, ld_env);
}

// ---------------------------------------------------------------------------------------------
// K14 rollout policy head: hidden activation + output layers (one wave per env, lane l owns hidden
// columns [4l, 4l + 4), butterfly dot products) + the K3 sample/store above, or the value alone.
// ---------------------------------------------------------------------------------------------
// K7's per-env body, shared by the standalone env step and K14's fused form: one wave per env, lanes over
// the state dims; pre(d) = the env's pre-activation for state dim d (row d of [W | U] (s | a)).
struct SynthEnvArgs {
    int D;
    uint32_t seed;
    int max_steps;
    float noise, thresh, reset_scale;
    float *state;
    int64_t ld_state;
    float *final_obs, *rew;
    uint8_t *term, *trunc;
    int32_t *ep_step;
    uint32_t *ep_index;
    float *ep_score, *ep_last_score;
    int32_t *ep_last_len;
    const float *wt;  // fused form: [W | U]^T, [D + A, D] row-major
};

// What K14F's post tail needs from the step, in registers: reward and flags (every lane), and lane d's final observation
// (sv) and next state (sn) for d = lane < min(D, 64)
struct EnvRowOut {
    float r, sv, sn;
    bool te, tr;
};

// t, ep, score0: the env's ep_step / ep_index / ep_score (loaded by the caller, early in the fused form)
template <class PreFn>
__device__ __forceinline__ EnvRowOut synthbox_env_row(int64_t n, int lane, const SynthEnvArgs &e, PreFn pre, int t,
                                                      uint32_t ep, float score0) {
    const int D = e.D;
    EnvRowOut o{0.f, 0.f, 0.f, false, false};
    float sumsq = 0.f, s0 = 0.f;
    for (int d = lane; d < D; d += 64) {
        const uint32_t base = ((uint32_t)t * (uint32_t)D + (uint32_t)d) * 4u;
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc += xpa_u01(xpa_hash4(e.seed, (uint32_t)n, ep, base + (uint32_t)j));
        const float xi = (acc - 2.0f) * 1.7320508075688772f;
        const float sv = tanhf(pre(d) + e.noise * xi);
        e.final_obs[n * D + d] = sv;
        sumsq += sv * sv;
        if (d == 0) s0 = sv;
        if (d == lane) o.sv = sv;
    }
    sumsq = xpa_wave_sum(sumsq);
    s0 = __shfl(s0, 0, 64);
    const float r = -sumsq / (float)D;
    const bool te = s0 > e.thresh;
    const int t1 = t + 1;
    const bool tr = t1 >= e.max_steps;
    const bool done = te || tr;
    const float score = score0 + r;
    for (int d = lane; d < D; d += 64) {
        float sn;
        if (done) {
            const uint32_t h = xpa_hash4(e.seed ^ kSaltReset, (uint32_t)n, ep + 1u, (uint32_t)d);
            sn = (2.0f * xpa_u01(h) - 1.0f) * e.reset_scale;
        } else {
            sn = e.final_obs[n * D + d];
        }
        e.state[n * e.ld_state + d] = sn;
        if (d == lane) o.sn = sn;
    }
    o.r = r;
    o.te = te;
    o.tr = tr;
    if (lane == 0) {
        e.rew[n] = r;
        e.term[n] = te ? 1 : 0;
        e.trunc[n] = tr ? 1 : 0;
        if (done) {
            e.ep_last_score[n] = score;
            e.ep_last_len[n] = t1;
            e.ep_index[n] = ep + 1u;
            e.ep_step[n] = 0;
            e.ep_score[n] = 0.f;
        } else {
            e.ep_step[n] = t1;
            e.ep_score[n] = score;
        }
    }
    return o;
}

__device__ __forceinline__ float wave_allsum_f(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// obs_normalize_kernel's arithmetic on one element (K8's NORM form and K14F)
__device__ __forceinline__ float obs_norm1(float x, float m, float v, float clip) {
    const float sd = sqrtf(v);
    const float y = (x - m) / (sd + 1e-8f);
    return fminf(fmaxf(y, -clip), clip);
}

// ret_rms.update_from_moments (statistic_tools.py:86-112) from the summed (count, sum, sumsq) of the closed paths.
__device__ __forceinline__ void ret_rms_merge_local(double c, double s1, double s2, float &m, float &v, double &cnt) {
    if (c > 0.0) {
        const double bm = s1 / c;
        const double bvar = fmax(s2 / c - bm * bm, 0.0);
        const double c0 = cnt, m0 = (double)m, v0 = (double)v;
        const double tot = c0 + c;
        const double delta = bm - m0;
        m = (float)(m0 + delta * c / tot);
        v = (float)((v0 * c0 + bvar * c + delta * delta * c0 * c / tot) / tot);
        cnt = tot;
    }
}

__device__ __forceinline__ void ret_rms_merge(double c, double s1, double s2, float *ret_mean, float *ret_var,
                                              double *ret_count) {
    if (c > 0.0) {
        float m = *ret_mean, v = *ret_var;
        double cnt = *ret_count;
        ret_rms_merge_local(c, s1, s2, m, v, cnt);
        *ret_mean = m;
        *ret_var = v;
        *ret_count = cnt;
    }
}

// ---- K14F (r06): K8's deferred, normalised post step and the next step's obs_rms.update in K14E's launch ----------------
// An env step of the C2 rollout then takes three launches (normalise + trunk, K40R, K14F) instead of five (+ K8 + K5).
// Per env (one wave, lanes over the state dims) the tail does what post_env<true, true> does for it (reward
// normalisation, buffer column t, closures, kept truncation rows, boot_norm at the last step, the return tracker) from the
// step's results in registers (EnvRowOut) and forms the env's share of the ret_rms moments and of the next observation's
// sums around the running mean; the 4 envs of a block are added in wave order.  The block partials (P = 3 + 2D f64) are
// reduced in two ticketed levels, both in a fixed order (any arrival order gives the same bits): the last block of each
// group of kPostGrp blocks sums its group's partials (4 contiguous chunks, then the chunks in order), and the last group
// to finish sums the group partials in group order, merges obs_rms (rms_merge_col) and ret_rms (ret_rms_merge), advances
// the cursor and resets the tickets.  Every block reads the statistics and the cursor before its ticket, the final block
// writes them after every ticket was taken (K8's protocol).
constexpr int kPostGrp = 64;
// tickets 256 B apart: atomics on one line serialise, and 1024 blocks' tickets on the two lines of a packed [1 + 16]
// array cost ~10 us per launch (tools/k14f_probe.py, r06: drain + group tickets 9.6 us packed)
constexpr int kTicketStride = 64;
// diagnostics (tools/k14f_probe.py, xpa_k14f_probe): bit 1 = the tail ends after the block partial stores, bit 2 = after
// the group tickets, bit 4 = after the group sums (results then invalid: timing only); 0 in production
__device__ int g_k14f_probe = 0;
struct PostArgs {
    xpa_cursor_t *cur;
    float *ret_mean, *ret_var;
    double *ret_count;
    float *returns, *buf_rew, *buf_term;
    uint8_t *buf_closed;
    float *buf_boot;
    float gamma, rew_range, obs_clip;
    int mask_returns, use_rewnorm, atari_lifeloss, slot_from_next, n_slots;
    float *slot_obs;
    int32_t *slot_t, *overflow;
    float *obs_mean, *obs_var;
    double *obs_count;   // nullptr: no obs_rms update (P = 3)
    float *boot_norm;
    int64_t ld_norm;
    double *part;        // f64 [(blocks + groups) * P]
    unsigned *tickets;   // [(1 + groups) * kTicketStride] (ticket i at i * kTicketStride), zero between launches
};

__device__ __forceinline__ void k14f_tail(const PostArgs &pa, int D, const EnvRowOut &eo, bool valid, int64_t n,
                                          int64_t n_envs, int64_t T, int lane, int wave) {
    __shared__ double s_pp[4][3 + 2 * 64];
    __shared__ double s_ch[4][3 + 2 * 64];
    __shared__ bool s_last;
    const bool rms = pa.obs_count != nullptr;
    const int P = 3 + (rms ? 2 * D : 0);
    const int32_t t = pa.cur->ptr;
    double cnt = 0.0, sm = 0.0, sq = 0.0, rp = 0.0, rq = 0.0;
    if (valid) {   // wave-uniform
        const bool last = t == (int32_t)(T - 1);
        const int64_t cell = n * T + t;
        const bool done = eo.te || eo.tr;
        const bool close = last || (done && !(pa.atari_lifeloss && !eo.tr));
        const float m = lane < D ? pa.obs_mean[lane] : 0.f, v = lane < D ? pa.obs_var[lane] : 1.f;
        if (lane == 0) {
            const float rstd = fminf(fmaxf(sqrtf(*pa.ret_var), 0.1f), 100.0f);
            pa.buf_rew[cell] = pa.use_rewnorm ? fminf(fmaxf(eo.r / rstd, -pa.rew_range), pa.rew_range) : eo.r;
            pa.buf_term[cell] = eo.te ? 1.f : 0.f;
            pa.buf_closed[cell] = close ? 1 : 0;
            pa.buf_boot[cell] = 0.f;   // deferred: the bootstraps are written after the rollout
            const float R = pa.returns[n];
            float Rk = pa.mask_returns ? (eo.te ? 0.f : pa.gamma * R) + eo.r : pa.gamma * R + eo.r;
            if (done) {
                cnt = 1.0;
                sm = (double)Rk;
                sq = (double)Rk * (double)Rk;
                Rk = 0.f;
            }
            pa.returns[n] = Rk;
        }
        if (close && !eo.te && !last) {   // mid-buffer truncation: keep the normalised row for later
            int k = 0;
            if (lane == 0) {
                while (k < pa.n_slots && pa.slot_t[(int64_t)k * n_envs + n] >= 0) ++k;
                if (k == pa.n_slots) {   // contract broken: counted (the agent raises), the last slot is reused
                    atomicAdd(pa.overflow, 1);
                    k = pa.n_slots - 1;
                }
                pa.slot_t[(int64_t)k * n_envs + n] = t;
            }
            k = __shfl(k, 0, 64);
            if (lane < D)
                pa.slot_obs[((int64_t)k * n_envs + n) * D + lane] =
                    obs_norm1(pa.slot_from_next ? eo.sn : eo.sv, m, v, pa.obs_clip);
        }
        if (last && lane < D) pa.boot_norm[n * pa.ld_norm + lane] = obs_norm1(eo.sv, m, v, pa.obs_clip);
        if (rms && lane < D) {
            const double dv = (double)eo.sn - (double)m;
            rp = dv;
            rq = dv * dv;
        }
    }
    if (lane == 0) {
        s_pp[wave][0] = cnt;
        s_pp[wave][1] = sm;
        s_pp[wave][2] = sq;
    }
    if (rms && lane < D) {
        s_pp[wave][3 + lane] = rp;
        s_pp[wave][3 + D + lane] = rq;
    }
    __syncthreads();
    const int tid = threadIdx.x;
    const unsigned nblk = gridDim.x, G = (nblk + kPostGrp - 1) / kPostGrp;
    const int probe = g_k14f_probe;
    if (tid < P)
        xpa_store_agent(pa.part + (int64_t)blockIdx.x * P + tid, ((s_pp[0][tid] + s_pp[1][tid]) + s_pp[2][tid]) + s_pp[3][tid]);
    if (probe & 1) return;
    xpa_drain();
    __syncthreads();
    const unsigned g = blockIdx.x / kPostGrp, g0 = g * kPostGrp;
    const int gn = (int)min((unsigned)kPostGrp, nblk - g0);
    if (tid == 0) s_last = xpa_ticket(pa.tickets + kTicketStride * (1 + g)) == (unsigned)(gn - 1);
    __syncthreads();
    if (!s_last) return;
    if (probe & 2) {
        if (tid == 0) pa.tickets[kTicketStride * (1 + g)] = 0u;
        return;
    }
    // the group's partials: thread (chunk j, column i) sums a contiguous run of blocks in order, then the runs in order
    const int nch = min(4, 256 / P);
    const int i = tid % P, j = tid / P;
    if (j < nch) {
        const int per = (gn + nch - 1) / nch;
        const int lo = j * per, hi = min(gn, lo + per);
        double acc = 0.0;
        for (int b0 = lo; b0 < hi; b0 += 16) {
            double x[16];
#pragma unroll
            for (int u = 0; u < 16; ++u)
                x[u] = b0 + u < hi ? xpa_load_agent(pa.part + (int64_t)(g0 + b0 + u) * P + i) : 0.0;
#pragma unroll
            for (int u = 0; u < 16; ++u)
                if (b0 + u < hi) acc += x[u];
        }
        s_ch[j][i] = acc;
    }
    __syncthreads();
    if (tid < P) {
        double a = s_ch[0][tid];
        for (int jj = 1; jj < nch; ++jj) a += s_ch[jj][tid];
        xpa_store_agent(pa.part + (int64_t)(nblk + g) * P + tid, a);
    }
    if (tid == 0) pa.tickets[kTicketStride * (1 + g)] = 0u;   // every block of the group has taken its ticket
    if (probe & 4) return;
    xpa_drain();
    __syncthreads();
    if (tid == 0) s_last = xpa_ticket(pa.tickets) == G - 1;
    __syncthreads();
    if (!s_last) return;
    // the last group: the group partials in group order
    if (tid < P) {
        double a = 0.0;
        for (unsigned b0 = 0; b0 < G; b0 += 16) {
            double x[16];
#pragma unroll
            for (unsigned u = 0; u < 16; ++u)
                x[u] = b0 + u < G ? xpa_load_agent(pa.part + (int64_t)(nblk + b0 + u) * P + tid) : 0.0;
#pragma unroll
            for (unsigned u = 0; u < 16; ++u)
                if (b0 + u < G) a += x[u];
        }
        s_ch[0][tid] = a;
    }
    const double c0 = rms ? *pa.obs_count : 0.0;
    __syncthreads();
    if (rms && tid < D) rms_merge_col(s_ch[0][3 + tid], s_ch[0][3 + D + tid], (double)n_envs, c0, pa.obs_mean, pa.obs_var, tid);
    if (tid == 0) {
        if (rms) *pa.obs_count = c0 + (double)n_envs;
        ret_rms_merge(s_ch[0][0], s_ch[0][1], s_ch[0][2], pa.ret_mean, pa.ret_var, pa.ret_count);
        pa.cur->ptr = (int32_t)((t + 1) % T);
        pa.cur->step = pa.cur->step + 1u;
        pa.tickets[0] = 0u;
    }
}

// MODE: 0 Gaussian sample, 1 Categorical sample, 2 value only (v_out[n]).
constexpr int kRolloutKMax = 32;  // head width limit of K14 (lanes < K draw the Gaussian dimensions)
// ENV (Gaussian only): the SynthBox env step of the same env fused after the sample — pre = [W | U] (s | clip(a))
// from the state row and the lanes' clipped actions (fixed k order), then K7's body: no env GEMM and no K7
// launch.  Needs D <= 64 (one state dim per lane).
// r05: with n_envs % 64 == 0, K14E's block b (on XCD b % 8) takes the 8-env granule G = 8 (m >> 1) + (b & 7), m = b >> 3,
// half m & 1: granule G lies on XCD G % 8 — where the rollout trunk's 8-row tile G was written (thin_fwd_norm: block = tile)
// and K40R's XCD-mapped row tiles read and write it — so the z rows and the next step's observation rows stay in one
// XCD's L2 from producer to consumer.  Any env order gives the same per-env results.
__device__ __forceinline__ int64_t xcd_env(int64_t b, int wave, int64_t n_envs) {
    if ((n_envs & 63) != 0) return b * 4 + wave;
    const int64_t m = b >> 3, G = 8 * (m >> 1) + (b & 7);
    return 8 * G + 4 * (m & 1) + wave;
}

// POST (K14F, r06, with MODE 0 + ENV): k14f_tail after the env step; every wave of the block reaches it (waves past
// n_envs skip the env body only)
template <int MODE, int ACT, bool ENV = false, bool POST = false>
__global__ __launch_bounds__(256) void rollout_policy_head_kernel(
    int64_t n_envs, int K, int64_t T, const float *__restrict__ za, const float *__restrict__ zc, int64_t ld,
    float slope, const float *__restrict__ Wa, const float *__restrict__ ba, const float *__restrict__ Wc,
    const float *__restrict__ bc, const float *__restrict__ logstd, const xpa_cursor_t *cur,   // POST: also pa.cur
    uint32_t seed, float act_clip, float *__restrict__ buf_act, float *__restrict__ buf_logp,
    float *__restrict__ buf_val, float *__restrict__ env_in, int64_t ld_env, float *__restrict__ v_out,
    SynthEnvArgs env, PostArgs pa = PostArgs{}) {
    static_assert(!POST || (MODE == 0 && ENV), "K14F is the Gaussian env-fused form");
    __shared__ float s_head[4][kRolloutKMax];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n = ENV ? xcd_env(blockIdx.x, wave, n_envs) : (int64_t)blockIdx.x * 4 + wave;
    const bool valid = n < n_envs;
    if (!POST && !valid) return;  // wave-uniform
    EnvRowOut eo{0.f, 0.f, 0.f, false, false};
    if (valid) {
        // ENV: the env's state row, counters and the first kPreW rows of [W | U]^T are loaded first, so their
        // latency hides under the head arithmetic
        constexpr int kPreW = 24;
        float xs = 0.f, wreg[ENV ? kPreW : 1];
        int e_t = 0;
        uint32_t e_ep = 0u;
        float e_score = 0.f;
        int dl = 0;
        if constexpr (ENV) {
            dl = lane < env.D ? lane : 0;
            xs = lane < env.D ? env.state[n * env.ld_state + lane] : 0.f;
            e_t = env.ep_step[n];
            e_ep = env.ep_index[n];
            e_score = env.ep_score[n];
#pragma unroll
            for (int j = 0; j < kPreW; ++j) {  // unconditional loads (clamped row): no branch + wait per element
                const int jj = j < env.D + K ? j : env.D + K - 1;
                wreg[j] = env.wt[jj * env.D + dl];
            }
        }
        const float4 hc = xpa_act4<ACT>(*reinterpret_cast<const float4 *>(zc + n * ld + 4 * lane), slope);
        const float v = wave_allsum_f(xpa_dot4(hc, *reinterpret_cast<const float4 *>(Wc + 4 * lane))) + bc[0];
        if (MODE == 2) {
            if (lane == 0) v_out[n] = v;
            return;
        }
        const float4 h = xpa_act4<ACT>(*reinterpret_cast<const float4 *>(za + n * ld + 4 * lane), slope);
        float mine = 0.f;  // lane o keeps head[o]
        for (int o = 0; o < K; ++o) {
            const float p = wave_allsum_f(xpa_dot4(h, *reinterpret_cast<const float4 *>(Wa + o * 256 + 4 * lane))) + ba[o];
            if (lane == o) mine = p;
            if (MODE == 1 && lane == 0) s_head[wave][o] = p;
        }
        if (MODE == 1) {
            if (lane == 0) cat_sample_store(n, K, T, s_head[wave], v, cur, seed, buf_act, buf_logp, buf_val, env_in, ld_env);
            return;
        }
        // Gaussian: lane a draws dimension a (the K3 arithmetic); lane 0 adds the log-prob terms in
        // dimension order, so the sum is bitwise K3's sequential one.
        const int64_t cell = n * T + cur->ptr;
        float term_a = 0.f, xclip = 0.f;
        if (lane < K) {
            const int a = lane;
            const uint32_t step = cur->step;
            const uint32_t h1 = xpa_hash4(seed ^ kSaltAct, step, (uint32_t)n, (uint32_t)(2 * a));
            const uint32_t h2 = xpa_hash4(seed ^ kSaltAct, step, (uint32_t)n, (uint32_t)(2 * a + 1));
            const float u1 = 1.0f - xpa_u01(h1);
            const float u2 = xpa_u01(h2);
            const float eps = sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
            const float sc = expf(logstd[a]);
            const float x = mine + sc * eps;
            const float diff = x - mine;
            term_a = -(diff * diff) / (2.0f * sc * sc) - logf(sc) - 0.91893853320467274178f;
            buf_act[cell * K + a] = x;
            xclip = fminf(fmaxf(x, -act_clip), act_clip);
            env_in[n * ld_env + a] = xclip;
        }
        float logp = 0.f;
        for (int a = 0; a < K; ++a) logp += __shfl(term_a, a, 64);
        if (lane == 0) {
            buf_logp[cell] = logp;
            buf_val[cell] = v;
        }
        if constexpr (ENV) {
            // pre = [W | U] (s | clip(a)) for state dim `lane`: one fmaf chain over j < D + K in order
            const int D = env.D, J = D + K;
            float pre = 0.f;
#pragma unroll
            for (int j = 0; j < kPreW; ++j) {
                if (j < J) {  // uniform
                    const float v = __shfl(j < D ? xs : xclip, j < D ? j : j - D, 64);
                    if (lane < D) pre = fmaf(v, wreg[j], pre);
                }
            }
            for (int j = kPreW; j < J; ++j) {
                const float v = __shfl(j < D ? xs : xclip, j < D ? j : j - D, 64);
                const float w = env.wt[j * D + dl];
                if (lane < D) pre = fmaf(v, w, pre);
            }
            eo = synthbox_env_row(n, lane, env, [&](int) { return pre; }, e_t, e_ep, e_score);
        }
    }
    if constexpr (POST) k14f_tail(pa, env.D, eo, valid, n, n_envs, T, lane, wave);
}

// ---------------------------------------------------------------------------------------------
// K7 SynthBox env step (one wave per env, lanes over the state dims)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void synthbox_step_kernel(const float *__restrict__ pre, SynthEnvArgs e,
                                                            int64_t n_envs) {
    const int64_t n = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (n >= n_envs) return;  // wave-uniform
    synthbox_env_row(n, lane, e, [&](int d) { return pre[n * e.D + d]; }, e.ep_step[n], e.ep_index[n], e.ep_score[n]);
}

// ---------------------------------------------------------------------------------------------
// K8 post-step bookkeeping (single block)
// ---------------------------------------------------------------------------------------------
// One env per thread over ceil(n_envs / 256) blocks (the scattered column writes spread over the chip);
// each block writes its finished-return moments (count, sum, sum of squares; f64) to `partials`, and
// the last block to arrive (atomic ticket) merges them in block order into ret_rms, advances the
// cursor and resets the ticket to 0 (graph replays see a fresh ticket).
// DEFER: no v_boot; a mid-buffer truncation of env n copies its normalised final observation row
// (boot_obs) into the env's first free slot k < n_slots (slot_obs[k n_envs + n], slot_t[k n_envs + n] = t);
// with every slot taken it counts in *overflow (the agent sizes n_slots from the env's time limit so that
// this cannot happen: at most ceil((T - 1) / max_episode_steps) mid-buffer truncations per rollout);
// bootstraps are written afterwards by xpa_rollout_bootstrap_fixup.
constexpr int kPostThreads = 256;
// NORM (with DEFER): boot_obs holds the RAW final observations; the kernel normalises them with the obs
// running statistics (obs_normalize_kernel's exact arithmetic) where it keeps a truncation row, and at the
// rollout's last step writes every env's normalised final observation into boot_norm — the second
// normalise launch of each env step is folded in here.

// K8's per-env body (shared with K32): reward normalisation, buffer column t, closures / kept truncation rows,
// the return tracker (R in, the new running return out); (cnt, sum, sumsq) = the env's contribution to ret_rms's
// batch moments.
template <bool DEFER, bool NORM>
__device__ __forceinline__ float post_env(
    int64_t n, int64_t n_envs, int64_t T, int32_t t, bool last, float rstd, float r, bool te, bool tr, float vb,
    float R, float *__restrict__ buf_rew, float *__restrict__ buf_term,
    uint8_t *__restrict__ buf_closed, float *__restrict__ buf_boot, float gamma, int mask_returns, int use_rewnorm,
    float rew_range, int atari_lifeloss, const float *__restrict__ boot_obs, int64_t ld_boot, int64_t dim,
    float *__restrict__ slot_obs, int *__restrict__ slot_t, int n_slots, int *__restrict__ overflow,
    const float *__restrict__ obs_mean, const float *__restrict__ obs_var, float obs_clip,
    float *__restrict__ boot_norm, int64_t ld_norm, double &cnt, double &sum, double &sumsq,
    const float *__restrict__ slot_src = nullptr, int64_t ld_slot = 0) {
    const int64_t cell = n * T + t;
    buf_rew[cell] = use_rewnorm ? fminf(fmaxf(r / rstd, -rew_range), rew_range) : r;
    buf_term[cell] = te ? 1.f : 0.f;
    const bool done = te || tr;
    const bool close = last || (done && !(atari_lifeloss && !tr));
    buf_closed[cell] = close ? 1 : 0;
    buf_boot[cell] = close ? (te ? 0.f : vb) : 0.f;
    if (DEFER && close && !te && !last) {  // mid-buffer truncation: keep the row for later
        int k = 0;
        while (k < n_slots && slot_t[(int64_t)k * n_envs + n] >= 0) ++k;
        if (k == n_slots) {  // contract broken: counted (the agent raises), the last slot is reused
            atomicAdd(overflow, 1);
            k = n_slots - 1;
        }
        const int64_t sl = (int64_t)k * n_envs + n;
        slot_t[sl] = (int)t;
        // the row the bootstrap is formed from: the final observation (PPO), or with slot_src the env's next
        // (reset) observation — A2C's critic call sees obs[i] = reset_obs (a2c_agent.py:88-95)
        const float *src = slot_src ? slot_src + n * ld_slot : boot_obs + n * ld_boot;
        for (int64_t d = 0; d < dim; ++d)
            slot_obs[sl * dim + d] = NORM ? obs_norm1(src[d], obs_mean[d], obs_var[d], obs_clip) : src[d];
    }
    if (NORM && last)
        for (int64_t d = 0; d < dim; ++d)
            boot_norm[n * ld_norm + d] = obs_norm1(boot_obs[n * ld_boot + d], obs_mean[d], obs_var[d], obs_clip);
    float Rk = mask_returns ? (te ? 0.f : gamma * R) + r : gamma * R + r;
    if (done) {
        cnt = 1.0;
        sum = (double)Rk;
        sumsq = (double)Rk * (double)Rk;
        Rk = 0.f;
    }
    return Rk;  // the env's running return
}


// RMS (r05): the NEXT step's obs_rms.update folded in — each block also sums (x - mean) and its square over its envs'
// rows of the observation the env step just produced (f64; the block's 4 waves' sums in order), in
// rms_partials_kernel's partial layout, and the last block runs rms_merge_body after the ret_rms merge.  The next
// step then normalises with the merged statistics and needs no rms launch of its own (the reference updates obs_rms with
// the observation before acting on it: ppoclip_agent.py:62-63, statistic_tools.py:86-112).  obs_dim <= 64.
constexpr int kPostRmsMax = 64;
template <bool DEFER, bool NORM = false, bool RMS = false>
__global__ __launch_bounds__(kPostThreads) void rollout_post_kernel(
    int64_t n_envs, int64_t T, const float *__restrict__ rew, const uint8_t *__restrict__ term,
    const uint8_t *__restrict__ trunc, const float *__restrict__ v_boot, xpa_cursor_t *__restrict__ cur,
    float *__restrict__ ret_mean, float *__restrict__ ret_var, double *__restrict__ ret_count,
    float *__restrict__ returns, float *__restrict__ buf_rew, float *__restrict__ buf_term,
    uint8_t *__restrict__ buf_closed, float *__restrict__ buf_boot, float gamma, int mask_returns, int use_rewnorm,
    float rew_range, int atari_lifeloss, const float *__restrict__ boot_obs, int64_t ld_boot, int64_t dim,
    float *__restrict__ slot_obs, int *__restrict__ slot_t, int n_slots, int *__restrict__ overflow,
    double *__restrict__ partials,
    unsigned int *__restrict__ ticket, const float *__restrict__ obs_mean = nullptr,
    const float *__restrict__ obs_var = nullptr, float obs_clip = 0.f, float *__restrict__ boot_norm = nullptr,
    int64_t ld_norm = 0, const float *__restrict__ slot_src = nullptr, int64_t ld_slot = 0,
    const float *__restrict__ v_boot_mid = nullptr, const float *__restrict__ rms_x = nullptr, int64_t rms_ld = 0,
    int rms_dim = 0, double *__restrict__ rms_part = nullptr, float *rms_mean = nullptr,
    float *__restrict__ rms_var = nullptr, double *__restrict__ rms_count = nullptr) {
    __shared__ double s_red[kPostThreads / 64];
    __shared__ bool s_last;
    const int32_t t = cur->ptr;
    const float rstd = fminf(fmaxf(sqrtf(*ret_var), 0.1f), 100.0f);
    const bool last = (t == (int32_t)(T - 1));
    double cnt = 0.0, sum = 0.0, sumsq = 0.0;
    const int64_t n = (int64_t)blockIdx.x * kPostThreads + threadIdx.x;
    if (n < n_envs)
        returns[n] = post_env<DEFER, NORM>(n, n_envs, T, t, last, rstd, rew[n], term[n] != 0, trunc[n] != 0,
                              DEFER ? 0.f : (v_boot_mid && !last ? v_boot_mid[n] : v_boot[n]), returns[n], buf_rew, buf_term, buf_closed, buf_boot, gamma,
                              mask_returns, use_rewnorm, rew_range, atari_lifeloss, boot_obs, ld_boot, dim, slot_obs,
                              slot_t, n_slots, overflow, obs_mean, obs_var, obs_clip, boot_norm, ld_norm, cnt, sum,
                              sumsq, slot_src, ld_slot);
    constexpr int nw = kPostThreads / 64;
    if constexpr (RMS) {   // this block's partial of the next observation's moments around the running mean
        // 16 columns at a time: the block's rows staged in LDS, then thread (g, j) sums rows g, g + 16, ... of column j
        // in f64 (x - mean exact in f64) and the 16 row groups are added in order
        __shared__ float s_x[kPostThreads][17];
        __shared__ double s_p[16][16], s_q[16][16];
        const int j = threadIdx.x & 15, g = threadIdx.x >> 4;
        for (int c0 = 0; c0 < rms_dim; c0 += 16) {
            const int nc = rms_dim - c0 < 16 ? rms_dim - c0 : 16;
            const int64_t nr = n < n_envs ? n : 0;
            float v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = rms_x[nr * rms_ld + c0 + (u < nc ? u : 0)];
#pragma unroll
            for (int u = 0; u < 16; ++u) s_x[threadIdx.x][u] = v[u];
            __syncthreads();
            double sp = 0.0, sq = 0.0;
            if (j < nc) {
                const double mu = (double)rms_mean[c0 + j];
                for (int r = g; r < kPostThreads; r += 16) {
                    if ((int64_t)blockIdx.x * kPostThreads + r >= n_envs) break;
                    const double d = (double)s_x[r][j] - mu;
                    sp += d;
                    sq += d * d;
                }
            }
            s_p[g][j] = sp;
            s_q[g][j] = sq;
            __syncthreads();
            if ((int)threadIdx.x < nc) {
                double a = s_p[0][threadIdx.x], b = s_q[0][threadIdx.x];
#pragma unroll
                for (int w = 1; w < 16; ++w) {
                    a += s_p[w][threadIdx.x];
                    b += s_q[w][threadIdx.x];
                }
                xpa_store_agent(rms_part + (int64_t)blockIdx.x * rms_dim + c0 + threadIdx.x, a);
                xpa_store_agent(rms_part + ((int64_t)gridDim.x + blockIdx.x) * rms_dim + c0 + threadIdx.x, b);
            }
            __syncthreads();   // s_x / s_p reused by the next 16 columns
        }
    }
    cnt = xpa_block_sum(cnt, s_red, nw);
    sum = xpa_block_sum(sum, s_red, nw);
    sumsq = xpa_block_sum(sumsq, s_red, nw);
    if (RMS) {
        xpa_drain();        // every thread's rms partial stores complete before thread 0's ticket
        __syncthreads();
    }
    if (threadIdx.x == 0) {  // sc1 stores, drained before the ticket (no L2 write-back fence)
        xpa_store_agent(partials + 3 * blockIdx.x, cnt);
        xpa_store_agent(partials + 3 * blockIdx.x + 1, sum);
        xpa_store_agent(partials + 3 * blockIdx.x + 2, sumsq);
        xpa_drain();
        s_last = xpa_ticket(ticket) == gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last) return;
    if constexpr (RMS) {   // the next observation's obs_rms merge (all of the last block's threads), then ret_rms
        rms_merge_body(rms_part, gridDim.x, n_envs, rms_dim, rms_mean, rms_var, rms_count);
        __syncthreads();
    }
    // all of the last block's threads load the partials at once (one round trip), thread 0 sums them in
    // block order (deterministic)
    __shared__ double s_pp[3 * 1024];
    const bool staged = gridDim.x <= 1024;
    if (staged)
        for (unsigned i = threadIdx.x; i < 3 * gridDim.x; i += kPostThreads) s_pp[i] = xpa_load_agent(partials + i);
    __syncthreads();
    if (threadIdx.x != 0) return;
    double c = 0.0, s1 = 0.0, s2 = 0.0;
    for (unsigned g = 0; g < gridDim.x; ++g) {  // fixed order -> deterministic
        c += staged ? s_pp[3 * g] : xpa_load_agent(partials + 3 * g);
        s1 += staged ? s_pp[3 * g + 1] : xpa_load_agent(partials + 3 * g + 1);
        s2 += staged ? s_pp[3 * g + 2] : xpa_load_agent(partials + 3 * g + 2);
    }
    ret_rms_merge(c, s1, s2, ret_mean, ret_var, ret_count);
    cur->ptr = (int32_t)((t + 1) % T);
    cur->step = cur->step + 1u;
    *ticket = 0u;
}

// ---------------------------------------------------------------------------------------------
// K32 — `steps` device env steps of a small-MLP agent on a classic-control env (the E trait: observation width 1..8)
// in one launch (one workgroup):
// obs RMS (K5) -> normalise (obs_normalize) -> MLP forward -> K3 sample/store -> K18 env step -> K8 (deferred,
// NORM).  The RMS sums, the merge, the normalisation, the sampler, the env and the post step are the multi-kernel
// path's own code or arithmetic (one RMS partial block: rows summed per (row group, column) and the groups in
// order, as rms_partials_kernel<., 256> does for n <= 256); the weight rows the forward needs stay in VGPRs for
// the whole launch.  C1: 8 envs, ~10 launches x 128 steps per rollout -> one launch.
// ---------------------------------------------------------------------------------------------
constexpr int kRoThreads = 256;
constexpr int kRoLdsMax = 16384;  // floats of dynamic LDS (64 KiB: no attribute needed)

__host__ __device__ constexpr int ro_r4(int x) { return (x + 3) & ~3; }

struct RoLayout {
    int sy, sz, sbo, sh, total;
};
constexpr int kRoWide = 128;           // K32W's width: h0 == h1 == h2 == 128
constexpr int kRoWideQ = 32 + 4;       // K32W's h0 tile: floats per (row, k & 3) group (32 + a 16-B pad)
constexpr int kRoWideP = 4 * kRoWideQ;  // ... and per row
// sy: the normalised observations [N][D]; sz: the output layers' partial sums [wave][N][K + 1]; sbo: biases; sh
// (K32W only): h0 of one 16-env tile, element (row, k) at row kRoWideP + (k & 3) kRoWideQ + (k >> 2)
__host__ __device__ inline RoLayout ro_layout(int N, int D, int H0, int H1, int H2, int K) {
    RoLayout l;
    const int K1 = K + 1;
    (void)H1;
    (void)H2;
    l.sy = 0;
    l.sz = ro_r4(N * D);
    l.sbo = ro_r4(l.sz + 4 * N * K1);
    l.total = ro_r4(l.sbo + K1);
    l.sh = l.total;
    if (H0 == kRoWide) l.total += 16 * kRoWideP;
    return l;
}

// Sum over the wave's 64 lanes on DPP lane moves (no LDS round trip); the total lands in lane 63.  Lanes a move
// leaves out (row_mask) add 0.
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ float ro_dpp(float src) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, src), CTRL, ROW_MASK, 0xf,
                                                                 false));
}
__device__ __forceinline__ float ro_wave_sum63(float v) {
    v += ro_dpp<0xB1>(v);        // quad_perm [1, 0, 3, 2]
    v += ro_dpp<0x4E>(v);        // quad_perm [2, 3, 0, 1]
    v += ro_dpp<0x141>(v);       // row_half_mirror: sums of 8
    v += ro_dpp<0x140>(v);       // row_mirror: sums of 16
    v += ro_dpp<0x142, 0xA>(v);  // row_bcast:15 into rows 1, 3
    v += ro_dpp<0x143, 0xC>(v);  // row_bcast:31 into rows 2, 3
    return v;
}

// Sum over the 16 lanes of each DPP row (every lane gets its row's sum).
__device__ __forceinline__ float ro_row_sum16(float v) {
    v += ro_dpp<0xB1>(v);   // quad_perm [1, 0, 3, 2]
    v += ro_dpp<0x4E>(v);   // quad_perm [2, 3, 0, 1]
    v += ro_dpp<0x141>(v);  // row_half_mirror: sums of 8
    v += ro_dpp<0x140>(v);  // row_mirror: sums of 16
    return v;
}
typedef float ro_f32x4 __attribute__((ext_vector_type(4)));

// K8's f64 wave butterfly (xpa_wave_sum) when only lanes [0, n) hold values (the rest +0): the steps whose partner
// lanes are all empty add +0 and are skipped.
__device__ __forceinline__ double ro_wave_sum_first(double v, int n) {
    for (int o = 32; o > 0; o >>= 1)
        if (o < n) v += __shfl_xor(v, o, 64);
    return v;
}

template <int ACT>
__device__ __forceinline__ float ro_act(float z, float slope) {
    if (ACT == 1) return z > 0.f ? z : z * slope;
    if (ACT == 2) return tanhf(z);
    return z;
}

// The env / head pair of a K32 instantiation: the observation width D, the output units at most KO (the head's k
// + the value), the env's argument block, register state and step, and the sampler with what it takes beyond
// XpaSmallRolloutArgs (Head).  act_step: K3's sample + stores at (t, step) from the output layers' z[0 .. k] (z[k] the
// value), then the env's step with the sampled action; returns the reward.
struct RoCartPoleCat {
    static constexpr int D = 4, KO = 3;
    using Env = XpaCartPoleEnv;
    using Local = cartpole::Local;
    struct Head {};
    static __device__ __forceinline__ Env env(const XpaSmallRolloutArgs &a) {
        return Env{a.env_state,   a.env_obs,   a.ld_obs,     a.final_obs,  a.env_rew,
                   a.env_term,    a.env_trunc, a.ep_step,    a.ep_index,   a.ep_score,
                   a.ep_last_score, a.ep_last_len, a.env_seed, a.max_episode_steps,
                   cartpole::kThetaThreshold};
    }
    static __device__ __forceinline__ Local load(const Env &e, int n) { return cartpole::load(e, n); }
    static __device__ __forceinline__ void store(const Env &e, int n, const Local &s) { cartpole::store(e, n, s); }
    static __device__ __forceinline__ float act_step(const XpaSmallRolloutArgs &a, const Head &, const Env &e, int n,
                                                     int K, int T, int32_t t, uint32_t step, const float *z, Local &es,
                                                     bool *te, bool *tr, float *o) {
        const int pick = cat_sample_store_at(n, K, T, t, step, z, z[K], a.seed, a.buf_act, a.buf_logp, a.buf_val,
                                             a.act_in, a.ld_act);
        return cartpole::step(e, n, pick, es, te, tr, o);
    }
};

struct RoPendulumGauss {
    static constexpr int D = 3, KO = 2;
    using Env = XpaPendulumEnv;
    using Local = pendulum::Local;
    struct Head {
        const float *logstd;
        float act_clip;
    };
    static __device__ __forceinline__ Env env(const XpaSmallRolloutArgs &a) {
        return Env{a.env_state, a.env_obs,  a.ld_obs,   a.final_obs,     a.env_rew,     a.env_term,  a.env_trunc,
                   a.ep_step,   a.ep_index, a.ep_score, a.ep_last_score, a.ep_last_len, a.env_seed,
                   a.max_episode_steps};
    }
    static __device__ __forceinline__ Local load(const Env &e, int n) { return pendulum::load(e, n); }
    static __device__ __forceinline__ void store(const Env &e, int n, const Local &s) { pendulum::store(e, n, s); }
    static __device__ __forceinline__ float act_step(const XpaSmallRolloutArgs &a, const Head &hd, const Env &e, int n,
                                                     int K, int T, int32_t t, uint32_t step, const float *z, Local &es,
                                                     bool *te, bool *tr, float *o) {
        const float u = gauss_sample_store_at(n, K, T, t, step, z, hd.logstd, z[K], a.seed, hd.act_clip, a.buf_act,
                                              a.buf_logp, a.buf_val, a.act_in, a.ld_act);
        return pendulum::step(e, n, u, es, te, tr, o);  // K == 1: the one torque
    }
};

// Acrobot-v1 / MountainCar-v0 with a Categorical head of 3 actions: K3's categorical sampler, then the env's step
struct RoAcrobotCat {
    static constexpr int D = 6, KO = 4;
    using Env = XpaAcrobotEnv;
    using Local = acrobot::Local;
    struct Head {};
    static __device__ __forceinline__ Env env(const XpaSmallRolloutArgs &a) {
        return Env{a.env_state, a.env_obs,  a.ld_obs,   a.final_obs,     a.env_rew,     a.env_term,  a.env_trunc,
                   a.ep_step,   a.ep_index, a.ep_score, a.ep_last_score, a.ep_last_len, a.env_seed,
                   a.max_episode_steps};
    }
    static __device__ __forceinline__ Local load(const Env &e, int n) { return acrobot::load(e, n); }
    static __device__ __forceinline__ void store(const Env &e, int n, const Local &s) { acrobot::store(e, n, s); }
    static __device__ __forceinline__ float act_step(const XpaSmallRolloutArgs &a, const Head &, const Env &e, int n,
                                                     int K, int T, int32_t t, uint32_t step, const float *z, Local &es,
                                                     bool *te, bool *tr, float *o) {
        const int pick = cat_sample_store_at(n, K, T, t, step, z, z[K], a.seed, a.buf_act, a.buf_logp, a.buf_val,
                                             a.act_in, a.ld_act);
        return acrobot::step(e, n, pick, es, te, tr, o);
    }
};

struct RoMountainCarCat {
    static constexpr int D = 8, KO = 4;
    using Env = XpaMountainCarEnv;
    using Local = mountaincar::Local;
    struct Head {};
    static __device__ __forceinline__ Env env(const XpaSmallRolloutArgs &a) {
        return Env{a.env_state, a.env_obs,  a.ld_obs,   a.final_obs,     a.env_rew,     a.env_term,  a.env_trunc,
                   a.ep_step,   a.ep_index, a.ep_score, a.ep_last_score, a.ep_last_len, a.env_seed,
                   a.max_episode_steps};
    }
    static __device__ __forceinline__ Local load(const Env &e, int n) { return mountaincar::load(e, n); }
    static __device__ __forceinline__ void store(const Env &e, int n, const Local &s) { mountaincar::store(e, n, s); }
    static __device__ __forceinline__ float act_step(const XpaSmallRolloutArgs &a, const Head &, const Env &e, int n,
                                                     int K, int T, int32_t t, uint32_t step, const float *z, Local &es,
                                                     bool *te, bool *tr, float *o) {
        const int pick = cat_sample_store_at(n, K, T, t, step, z, z[K], a.seed, a.buf_act, a.buf_logp, a.buf_val,
                                             a.act_in, a.ld_act);
        return mountaincar::step(e, n, pick, es, te, tr, o);
    }
};

// ---- the episode log of the device evaluation (K32E, xpa_eval_post; layout: include/xuanpolicy_amd.h) ----------------
constexpr int kLogCount = 0, kLogTarget = 1, kLogDone = 2, kLogSteps = 3, kLogOverflow = 4, kLogHeader = 8;
// int32 index of the first entry: the header, then the snapshot padded to 16 B
__host__ __device__ constexpr int64_t eval_log_entries(int64_t snap_dim) {
    return kLogHeader + ((2 + 2 * snap_dim + 3) & ~3LL);
}

// entry i of the log: (step, env, score, length); past capacity nothing is written and the overflow word is set
__device__ __forceinline__ void eval_log_put(int32_t *log, int64_t ent0, int64_t capacity, int64_t i, int32_t step,
                                             int32_t env, float score, int32_t len) {
    if (i < capacity) {
        int32_t *e = log + ent0 + 4 * i;
        e[0] = step;
        e[1] = env;
        e[2] = __builtin_bit_cast(int32_t, score);
        e[3] = len;
    } else {
        log[kLogOverflow] = 1;
    }
}

// K32E's arguments beyond XpaSmallRolloutArgs (whose cursor / seed are then the evaluation's own)
struct RoEval {
    int32_t *log;
    int64_t capacity, ent0;
};
struct RoNoEval {};

// EVAL (K32E): the evaluation form — the same obs-RMS update, normalisation, forward, sampler and env step; no buffer
// column (the sampler's three stores go to [N] scratch columns: T = 1, t = 0), no post step, no ret_rms; each step's
// finished episodes are compacted into the log in env order and the step loop ends after the first step at which the
// log holds `target` episodes (the reference's test loop, ppoclip_agent.py:113-165).
// The body is one device function under two __global__ wrappers: small_rollout_kernel (one agent, the block and the
// head in the kernel arguments) and small_rollout_batch_kernel (one workgroup per agent, each with its own block read
// from device memory).
template <class E, int ACT, int H0, bool EVAL>
__device__ __forceinline__ void small_rollout_body(const XpaSmallRolloutArgs &args, const typename E::Head &head,
                                                   const std::conditional_t<EVAL, RoEval, RoNoEval> &eval) {
    // local copies: the fields become values read once at entry, as a kernel's by-value arguments are
    const XpaSmallRolloutArgs a = args;
    const typename E::Head hd = head;
    const std::conditional_t<EVAL, RoEval, RoNoEval> ev = eval;
    extern __shared__ float lds[];
    __shared__ double s_sum[kRoThreads], s_sq[kRoThreads];
    __shared__ double s_red[kRoThreads / 64];
    __shared__ float s_mean[ro_r4(E::D)], s_var[ro_r4(E::D)];
    __shared__ float s_obs[256 * E::D];  // the raw observations of the step
    __shared__ float s_rstd;
    constexpr int D = E::D, KO = E::KO;
    static_assert(D >= 1 && D <= 8, "K32's observation widths");
    const int tid = threadIdx.x;
    const int N = a.n_envs, H1 = a.h1, H2 = a.h2, K = a.k, K1 = a.k + 1, U = a.h1 + a.h2;
    const int T = a.horizon;
    [[maybe_unused]] int32_t e_count = 0, e_target = 0, e_steps = 0;
    if constexpr (EVAL) {
        // block-uniform: a launch queued behind the one that completed the log returns at once
        if (ev.log[kLogDone] != 0) return;
        e_count = ev.log[kLogCount];
        e_target = ev.log[kLogTarget];
        e_steps = ev.log[kLogSteps];
    }
    const RoLayout L = ro_layout(N, D, H0, H1, H2, K);
    float *sy = lds + L.sy, *sz = lds + L.sz, *sbo = lds + L.sbo;
    const typename E::Env env = E::env(a);
    if (tid < K1) sbo[tid] = tid < K ? a.ba[tid] : a.bc[0];
    // The forward on v_mfma_f32_16x16x4_f32: [16-row tile of envs] x [actor | critic hidden units], K = h0.  Wave w
    // owns the unit tiles w and w + 4 (16 units each) with their weight rows in VGPRs (B operand, loaded once per
    // launch); lane (q, i) forms the A operand itself — h0[row i][4 kk + q] of the representation layer, from the
    // normalised row in LDS — so h0 never goes through LDS; the output layers are per-lane partial dot products over
    // the lane's units, summed over the 16 lanes of a DPP row and then over the waves (LDS, fixed order).
    // WIDE (K32W, h0 = h1 = h2 = 128): that layout would take D x 32 + 2 x 32 registers for the first layer alone and
    // form every h0 element once per wave.  Here wave w owns the four unit tiles w, w + 4, w + 8, w + 12 (128
    // registers of weight rows); thread t keeps only row t & 127 of the representation layer, the 16-env tile's h0 is
    // formed once by the whole block into LDS (sh, stored so that a lane's A operands of four k-steps are one 16-B
    // read) and every wave takes its A operands from there.
    constexpr bool WIDE = H0 == kRoWide;
    const int wave = tid >> 6, lane = tid & 63;
    const int li = lane & 15, lq = lane >> 4;
    constexpr int KK = H0 / 4, J = WIDE ? 4 : 2, KW = WIDE ? 1 : KK;
    const int UT = U >> 4;   // unit tiles (4, 6 or 8; WIDE: 16)
    float w0k[KW][D];   // the representation layer's rows 4 kk + q: D x h0 / 4 registers per lane (WIDE: row t & 127)
    float b0k[KW];
#pragma unroll
    for (int kk = 0; kk < KW; ++kk) {
        const int k = WIDE ? (tid & (kRoWide - 1)) : 4 * kk + lq;
#pragma unroll
        for (int d = 0; d < D; ++d) w0k[kk][d] = a.W0[k * D + d];
        b0k[kk] = a.b0[k];
    }
    float bw[J][KK], b12[J], wo[J][KO];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int tile = wave + 4 * j;
        const bool tok = tile < UT;
        const int u = tok ? 16 * tile + li : 0;
        const bool actor = u < H1;
        const float *wr = actor ? a.W1 + u * H0 : a.W2 + (u - H1) * H0;
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) bw[j][kk] = tok ? wr[4 * kk + lq] : 0.f;
        b12[j] = tok ? (actor ? a.b1[u] : a.b2[u - H1]) : 0.f;
#pragma unroll
        for (int o = 0; o < KO; ++o)
            wo[j][o] = !tok || o >= K1 ? 0.f : (o < K ? (actor ? a.Wa[o * H1 + u] : 0.f) : (actor ? 0.f : a.Wc[u - H1]));
    }

    // state that lives across the steps of the launch: each env's state and running return (thread n),
    // the raw observations and obs statistics (LDS), the obs count (every thread), the return statistics (thread 0)
    typename E::Local es{};
    float R = 0.f;
    if (tid < N) {
        es = E::load(env, tid);
        if constexpr (!EVAL) R = a.returns[tid];
#pragma unroll
        for (int d = 0; d < D; ++d) s_obs[tid * D + d] = a.env_obs[tid * a.ld_obs + d];
    }
    if (tid < D) {
        s_mean[tid] = a.obs_mean[tid];
        s_var[tid] = a.obs_var[tid];
    }
    double ocount = *a.obs_count;
    float rmean = 0.f, rvar = 0.f;
    double rcount = 0.0;
    if (!EVAL && tid == 0) {
        rmean = *a.ret_mean;
        rvar = *a.ret_var;
        rcount = *a.ret_count;
        s_rstd = fminf(fmaxf(sqrtf(rvar), 0.1f), 100.0f);
    }
    int32_t t = EVAL ? 0 : a.cursor->ptr;
    uint32_t step = a.cursor->step;
    int64_t st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, st_prev = 0, st_t0 = 0;
#define XPA_RO_STAMP(i_)                                                    \
    do {                                                                    \
        if (a.stamps && tid == 0) {                                         \
            const int64_t now_ = (int64_t)__builtin_amdgcn_s_memtime();     \
            st_acc[i_] += now_ - st_prev;                                   \
            st_prev = now_;                                                 \
        }                                                                   \
    } while (0)
    __syncthreads();
    if (a.stamps && tid == 0) st_prev = st_t0 = (int64_t)__builtin_amdgcn_s_memtime();
    // rms_partials_kernel<., 256>'s row groups at dim D (64 at dim 4, 42 at 6, 32 at 8; at dim 3, 85: thread 255
    // belongs to no group; at 6, threads 252 .. 255)
    constexpr int kGroups = kRoThreads / D;
    for (int s = 0; s < a.steps; ++s) {
        const bool last = t == T - 1;
        // (a) obs_rms.update(obs): xpa_rms_update with one partial block
        if (a.use_obsnorm) {
            double ts = 0.0, tq = 0.0;
            if (N <= kGroups) {
                // one row per row group: the group-ordered sums are the row sums in row order (every group sum is
                // 0 + v or 0 + v * v, rounded once; the empty groups add +0)
                if (tid < D) {
#pragma clang fp contract(off)
                    const float sh = s_mean[tid];
                    for (int r = 0; r < N; ++r) {
                        const double v = (double)s_obs[r * D + tid] - (double)sh;
                        const double vv = v * v;
                        ts = ts + v;
                        tq = tq + vv;
                    }
                }
            } else {
                const int c = tid % D, gsub = tid / D;
                double sm = 0.0, q = 0.0;
                const float sh = s_mean[c];
                if (gsub < kGroups)
                    for (int r = gsub; r < N; r += kGroups) {
                        const double v = (double)s_obs[r * D + c] - (double)sh;
                        sm += v;
                        q += v * v;
                    }
                s_sum[tid] = sm;
                s_sq[tid] = q;
                __syncthreads();
                if (tid < D)
                    for (int k = 0; k < kGroups; ++k) {
                        ts += s_sum[k * D + tid];
                        tq += s_sq[k * D + tid];
                    }
            }
            if (tid < D) {
                double s1 = 0.0, q1 = 0.0;  // rms_merge_body over the one partial
                s1 += ts;
                q1 += tq;
                const double n = (double)N, c0 = ocount;
                const double ms = s1 / n;
                const double m0 = (double)s_mean[tid], v0 = (double)s_var[tid];
                const double bm = m0 + ms;
                const double bvar = fmax(q1 / n - ms * ms, 0.0);
                const double tot = c0 + n;
                const double delta = bm - m0;
                const double new_mean = m0 + delta * n / tot;
                const double m2 = v0 * c0 + bvar * n + delta * delta * c0 * n / tot;
                const float fm = (float)new_mean, fv = (float)(m2 / tot);
                a.obs_mean[tid] = fm;
                a.obs_var[tid] = fv;
                s_mean[tid] = fm;
                s_var[tid] = fv;
            }
            ocount = ocount + (double)N;
            if (tid == 0) *a.obs_count = ocount;
            __syncthreads();
        }
        XPA_RO_STAMP(0);
        // (b) normalise into the policy input and buffer column t (obs_normalize_kernel's arithmetic)
        for (int e = tid; e < N * D; e += kRoThreads) {
            const int r = e / D, d = e % D;
            const float y = obs_norm1(s_obs[e], s_mean[d], s_var[d], a.obs_clip);
            sy[e] = y;
            if constexpr (!EVAL) {
                a.obs_norm[r * a.ld_norm + d] = y;
                a.buf_obs[((int64_t)r * T + t) * D + d] = y;
            }
        }
        __syncthreads();
        XPA_RO_STAMP(1);
        // (c)-(e) the forward, one 16-row tile of envs at a time
        for (int r0 = 0; r0 < N; r0 += 16) {
            ro_f32x4 acc[J];
#pragma unroll
            for (int j = 0; j < J; ++j) acc[j] = ro_f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (WIDE) {
                float *sh = lds + L.sh;
                if (r0 > 0) __syncthreads();   // the previous tile's A operands are read
                // h0 of the tile: thread t forms unit t & 127 of the rows (t >> 7) + 2 i (rows past N: row N - 1's,
                // results unused)
                const int u = tid & (kRoWide - 1), rh = tid >> 7;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int row = rh + 2 * i;
                    const float *yr = sy + (r0 + row < N ? r0 + row : N - 1) * D;
                    float z = b0k[0];
#pragma unroll
                    for (int d = 0; d < D; ++d) z = fmaf(w0k[0][d], yr[d], z);   // ascending d
                    sh[row * kRoWideP + (u & 3) * kRoWideQ + (u >> 2)] = ro_act<ACT>(z, a.slope);
                }
                __syncthreads();
                // lane (q, i)'s A operand of k-step kk is h0[row i][4 kk + q] = sh[i][q][kk]
                const float *ap = sh + li * kRoWideP + lq * kRoWideQ;
#pragma unroll
                for (int k4 = 0; k4 < KK; k4 += 4) {
                    const float4 a4 = *reinterpret_cast<const float4 *>(ap + k4);
                    const float av[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
                    for (int c = 0; c < 4; ++c)
#pragma unroll
                        for (int j = 0; j < J; ++j)
                            acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[c], bw[j][k4 + c], acc[j], 0, 0, 0);
                }
            } else {
                const int ra = r0 + li < N ? r0 + li : N - 1;   // this lane's A row (rows past N: results unused)
                float y[D];   // the lane's normalised row (16-B LDS reads where the row pitch keeps them aligned)
                if constexpr (D % 4 == 0) {
#pragma unroll
                    for (int d = 0; d < D; d += 4) {
                        const float4 y4 = *reinterpret_cast<const float4 *>(sy + ra * D + d);
                        y[d] = y4.x;
                        y[d + 1] = y4.y;
                        y[d + 2] = y4.z;
                        y[d + 3] = y4.w;
                    }
                } else {
#pragma unroll
                    for (int d = 0; d < D; ++d) y[d] = sy[ra * D + d];
                }
                float av[KK];
#pragma unroll
                for (int kk = 0; kk < KK; ++kk) {
                    float z = b0k[kk];
#pragma unroll
                    for (int d = 0; d < D; ++d) z = fmaf(w0k[kk][d], y[d], z);   // ascending d
                    av[kk] = ro_act<ACT>(z, a.slope);
                }
#pragma unroll
                for (int kk = 0; kk < KK; ++kk)
#pragma unroll
                    for (int j = 0; j < J; ++j)
                        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[kk], bw[j][kk], acc[j], 0, 0, 0);
            }
            // D element r of lane (q, i): row r0 + 4 q + r, unit 16 tile + i
            float part[4][KO];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int o = 0; o < KO; ++o) {
                    float pv = 0.f;
#pragma unroll
                    for (int j = 0; j < J; ++j) pv = fmaf(wo[j][o], ro_act<ACT>(acc[j][r] + b12[j], a.slope), pv);
                    part[r][o] = ro_row_sum16(pv);
                }
            if (li == 0)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int m = r0 + 4 * lq + r;
                    if (m < N)
                        for (int o = 0; o < K1; ++o) sz[(wave * N + m) * K1 + o] = part[r][o];
                }
        }
        __syncthreads();
        XPA_RO_STAMP(4);
        // (f) sample + store, env step, post step (one thread per env)
        double cnt = 0.0, sum = 0.0, sumsq = 0.0;
        [[maybe_unused]] bool fin = false;
        if (tid < N) {
            float z[KO];
            for (int o = 0; o < K1; ++o) {
                float v = sbo[o];
                for (int w = 0; w < 4; ++w) v += sz[(w * N + tid) * K1 + o];
                z[o] = v;
            }
            bool te, tr;
            float o[D];
            const float r = E::act_step(a, hd, env, tid, K, T, t, step, z, es, &te, &tr, o);
#pragma unroll
            for (int d = 0; d < D; ++d) s_obs[tid * D + d] = o[d];
            if constexpr (EVAL) {
                fin = te || tr;
                (void)r;
            } else {
                R = post_env<true, true>(tid, N, T, t, last, s_rstd, r, te, tr, 0.f, R, a.buf_rew, a.buf_term,
                                         a.buf_closed, a.buf_boot, a.gamma, a.mask_returns, a.use_rewnorm,
                                         a.rew_range, 0, a.final_obs, D, D, a.slot_obs, a.slot_t, a.n_slots,
                                         a.overflow, s_mean, s_var, a.obs_clip, a.boot_norm, a.ld_boot, cnt, sum,
                                         sumsq, a.slot_reset_obs ? a.env_obs : nullptr, a.ld_obs);
                a.returns[tid] = R;
            }
        }
        XPA_RO_STAMP(5);
        if constexpr (EVAL) {
            // the step's finished episodes into the log in env order: lane offset from the wave's ballot, wave offset
            // from the four wave totals (every thread forms the same new count: the stop below is block-uniform)
            __shared__ int s_wtot[kRoThreads / 64];
            const unsigned long long m = __ballot(fin);
            if (lane == 0) s_wtot[wave] = __popcll(m);
            __syncthreads();
            int before = 0, total = 0;
            for (int w = 0; w < kRoThreads / 64; ++w) {
                if (w < wave) before += s_wtot[w];
                total += s_wtot[w];
            }
            if (fin) {
                const int64_t i = (int64_t)e_count + before + __popcll(m & ((1ull << lane) - 1ull));
                eval_log_put(ev.log, ev.ent0, ev.capacity, i, e_steps, tid, env.ep_last_score[tid],
                             env.ep_last_len[tid]);
            }
            e_count += total;
            e_steps += 1;
            step += 1u;
            __syncthreads();  // next observations and statistics visible to the next step; s_wtot free again
            if (e_count >= e_target) break;
            continue;
        }
        // (g) ret_rms over the closed paths: K8's block sums (all envs in wave 0 when N <= 64: the other waves'
        // sums are +0), then its merge
        if (N <= 64) {
            if (tid < 64) {
                const int np2 = N <= 1 ? 1 : 1 << (32 - __builtin_clz(N - 1));  // lanes [0, np2) may hold values
                cnt = 0.0 + ro_wave_sum_first(cnt, np2);
                sum = 0.0 + ro_wave_sum_first(sum, np2);
                sumsq = 0.0 + ro_wave_sum_first(sumsq, np2);
            }
        } else {
            cnt = xpa_block_sum(cnt, s_red, kRoThreads / 64);
            sum = xpa_block_sum(sum, s_red, kRoThreads / 64);
            sumsq = xpa_block_sum(sumsq, s_red, kRoThreads / 64);
        }
        if (tid == 0 && cnt > 0.0) {
            ret_rms_merge_local(cnt, sum, sumsq, rmean, rvar, rcount);
            *a.ret_mean = rmean;
            *a.ret_var = rvar;
            *a.ret_count = rcount;
            s_rstd = fminf(fmaxf(sqrtf(rvar), 0.1f), 100.0f);
        }
        XPA_RO_STAMP(6);
        t = (t + 1) % T;
        step += 1u;
        __syncthreads();  // next observations, statistics and rstd visible to the next step
        XPA_RO_STAMP(7);
    }
#undef XPA_RO_STAMP
    if (a.stamps && tid == 0) {
        for (int i = 0; i < 8; ++i) a.stamps[i] = st_acc[i];
        a.stamps[8] = (int64_t)__builtin_amdgcn_s_memtime() - st_t0;
    }
    if (tid < N) E::store(env, tid, es);
    if (tid == 0) {
        a.cursor->ptr = t;
        a.cursor->step = step;
        if constexpr (EVAL) {
            ev.log[kLogCount] = e_count;
            ev.log[kLogSteps] = e_steps;
            ev.log[kLogDone] = e_count >= e_target ? 1 : 0;
        }
    }
}

template <class E, int ACT, int H0, bool EVAL = false>
__global__ __launch_bounds__(kRoThreads) void small_rollout_kernel(XpaSmallRolloutArgs a, typename E::Head hd,
                                                                   std::conditional_t<EVAL, RoEval, RoNoEval> ev) {
    small_rollout_body<E, ACT, H0, EVAL>(a, hd, ev);
}

// The population form (xpa_small_rollout_batch): workgroup p is agent p.  Its block (and, for a Gaussian head, its
// logstd / act_clip) is a plain load at a wave-uniform address; from there on it is the training body, and no
// workgroup reads or waits on anything another one writes.
template <class E, int ACT, int H0>
__global__ __launch_bounds__(kRoThreads) void small_rollout_batch_kernel(
    const XpaSmallRolloutArgs *__restrict__ blocks, const XpaSmallRolloutHead *__restrict__ heads) {
    const XpaSmallRolloutArgs a = blocks[blockIdx.x];
    typename E::Head hd{};
    if constexpr (!std::is_empty_v<typename E::Head>) {
        const XpaSmallRolloutHead h = heads[blockIdx.x];
        hd = typename E::Head{h.logstd, h.act_clip};
    }
    small_rollout_body<E, ACT, H0, false>(a, hd, RoNoEval{});
}

// K32EB — the population form of the evaluation (xpa_small_eval_batch): workgroup p is agent p.  Its block, its head
// and its XpaSmallEval record (log, scratch, capacity, snap_dim) are plain loads at wave-uniform addresses; the local
// copy of the block takes the overrides small_eval_launch makes on the host (horizon 1, the sampler's three stores
// into scratch, no stamps), and from there on it is K32E's body.  The stop rule is block-uniform and per log, so
// members finish at different steps without coordination: a workgroup whose log has done set returns at once while
// its neighbours run on, and no workgroup reads or waits on anything another one writes.
template <class E, int ACT, int H0>
__global__ __launch_bounds__(kRoThreads) void small_eval_batch_kernel(
    const XpaSmallRolloutArgs *__restrict__ blocks, const XpaSmallRolloutHead *__restrict__ heads,
    const XpaSmallEval *__restrict__ evals) {
    XpaSmallRolloutArgs a = blocks[blockIdx.x];
    const XpaSmallEval e = evals[blockIdx.x];
    typename E::Head hd{};
    if constexpr (!std::is_empty_v<typename E::Head>) {
        const XpaSmallRolloutHead h = heads[blockIdx.x];
        hd = typename E::Head{h.logstd, h.act_clip};
    }
    a.horizon = 1;
    a.buf_act = e.scratch;
    a.buf_logp = e.scratch + a.n_envs;
    a.buf_val = e.scratch + 2 * a.n_envs;
    a.stamps = nullptr;
    small_rollout_body<E, ACT, H0, true>(a, hd, RoEval{e.log, e.capacity, eval_log_entries(e.snap_dim)});
}

// The device half of the env classes' reset() for P env sets in one launch (xpa_small_env_reset_batch): workgroup p
// is agent p, thread n env n.  ro_reset0: env n's episode-0 state from the env body's own reset draw (what its step
// draws after a done, at episode 0) and the observation the class forms from it.
// CartPole's draw is restated: cartpole::reset_dim carries no contraction pragma and compiles to one v_fma_f64, while
// reset() forms u * 0.1 - 0.05 in numpy, the product and the difference each rounded — the f64 state this must equal.
__device__ __forceinline__ void ro_reset0(const XpaCartPoleEnv &e, int n) {
#pragma clang fp contract(off)
    double *st = e.state + 4 * n;
    float *o = e.obs + n * e.ld_obs;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const double u = (double)xpa_u01(xpa_hash4(e.seed ^ cartpole::kSaltCartPole, (uint32_t)n, 0u, (uint32_t)d));
        const double v = u * 0.1 - 0.05;
        st[d] = v;
        o[d] = (float)v;
    }
}
__device__ __forceinline__ void ro_reset0(const XpaPendulumEnv &e, int n) {
    const double th = pendulum::reset_dim(e.seed, (uint32_t)n, 0u, 0u);
    const double thdot = pendulum::reset_dim(e.seed, (uint32_t)n, 0u, 1u);
    double *st = e.state + 2 * n;
    float *o = e.obs + n * e.ld_obs;
    st[0] = th;
    st[1] = thdot;
    o[0] = (float)cos(th);
    o[1] = (float)sin(th);
    o[2] = (float)thdot;
}
__device__ __forceinline__ void ro_reset0(const XpaAcrobotEnv &e, int n) {
    double s[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) s[d] = acrobot::reset_dim(e.seed, (uint32_t)n, 0u, (uint32_t)d);
    double *st = e.state + 4 * n;
#pragma unroll
    for (int d = 0; d < 4; ++d) st[d] = s[d];
    float f[6];
    acrobot::obs_of(s[0], s[1], s[2], s[3], f);
    float *o = e.obs + n * e.ld_obs;
#pragma unroll
    for (int d = 0; d < 6; ++d) o[d] = f[d];
}
__device__ __forceinline__ void ro_reset0(const XpaMountainCarEnv &e, int n) {
    const double pos = mountaincar::reset_pos(e.seed, (uint32_t)n, 0u);
    double *st = e.state + 2 * n;
    float *o = e.obs + n * e.ld_obs;
    st[0] = pos;
    st[1] = 0.0;
#pragma unroll
    for (int k = 0; k < mountaincar::kStack; ++k) {   // the reset frame four times
        o[2 * k] = (float)pos;
        o[2 * k + 1] = 0.f;
    }
}

// ZERO_ACT: the class's reset() zeroes its action input (every env's but CartPole's)
template <class E, bool ZERO_ACT>
__global__ __launch_bounds__(kRoThreads) void small_env_reset_batch_kernel(
    const XpaSmallRolloutArgs *__restrict__ blocks) {
    const XpaSmallRolloutArgs a = blocks[blockIdx.x];
    const typename E::Env env = E::env(a);
    for (int n = threadIdx.x; n < a.n_envs; n += kRoThreads) {
        ro_reset0(env, n);
        env.ep_step[n] = 0;
        env.ep_index[n] = 0u;
        env.ep_score[n] = 0.f;
        env.ep_last_score[n] = 0.f;
        env.ep_last_len[n] = 0;
        env.rew[n] = 0.f;
        env.term[n] = 0;
        env.trunc[n] = 0;
        if constexpr (ZERO_ACT)
            for (int j = 0; j < a.k; ++j) a.act_in[n * a.ld_act + j] = 0.f;
    }
}

// ---------------------------------------------------------------------------------------------
// K33 — the closing of a K32 / K32W rollout in one launch (one workgroup per agent): the critic over the deferred
// bootstrap rows, bootstrap_fixup_kernel's writes and the advantage scan (xpa_gae_scan's recurrence on the dense
// closure record).
// The critic pass is K32's forward restated (K32's own code is left as it is): the same weight registers, the same
// fmaf chain over ascending d, the same MFMA tiling with every unit tile (the actor's too: they add the exact +0
// terms they add in K32), the same per-lane fmaf over the lane's tiles, ro_row_sum16 and bc + wave 0 + .. + wave 3,
// so a row's value is bit for bit what K32 writes into buf_val for that normalised row.  Only the value output is
// formed (each output's sum is independent of the others).  The observation width is a run-time 1 .. 8 here (the
// kernel does not depend on the env): the first layer's chain is unrolled to 8 and steps d >= D are skipped, not
// added as zeros.  The rows go through LDS in passes of n_envs, so ro_layout(n_envs, ...) is the budget.
// Thread n then owns env n's bootstraps: it writes them into boot (the fixup), and after a barrier the four waves scan
// the rows with xpa_gae_scan's own dense forms, restated below over a wave index instead of a grid: a row is a segment
// of L lanes, 4 steps per lane in 16-B accesses (T % 4 == 0 and 16-B aligned tensors: every rollout buffer; the DPP
// form for T > 32), the same affine compositions in the same order, so adv / ret are what xpa_gae_scan gives on the
// same record.  (gae.hip's kernels are left as they are: moving their bodies into shared device functions changed
// their ISA.)  The problem is latency-bound (8 x 128 .. 10 x 256 elements per agent).
// ---------------------------------------------------------------------------------------------
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ float ro_dpp_mov(float old, float src) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old),
                                                                 __builtin_bit_cast(int, src), CTRL, ROW_MASK, 0xf,
                                                                 false));
}
// v of lane src of the wave (a ds_bpermute lane read)
__device__ __forceinline__ float ro_lane(float v, int src) {
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src << 2, __builtin_bit_cast(int, v)));
}
__device__ __forceinline__ int ro_lane(int v, int src) { return __builtin_amdgcn_ds_bpermute(src << 2, v); }
constexpr int kRoDppRowShr = 0x110, kRoDppWaveShr1 = 0x138, kRoDppRowBcast15 = 0x142, kRoDppRowBcast31 = 0x143;

// (LA, LB) <- (LA, LB) o the map CTRL brings in; disabled / out-of-row lanes bring the identity.  FUSED: LB + LA oB
// rounded once (fma) or twice — see the note on roundings below.
template <int CTRL, int ROW_MASK, bool FUSED>
__device__ __forceinline__ void ro_dpp_combine(float &LA, float &LB) {
#pragma clang fp contract(off)
    const float oA = ro_dpp_mov<CTRL, ROW_MASK>(1.f, LA);
    const float oB = ro_dpp_mov<CTRL, ROW_MASK>(0.f, LB);
    LB = FUSED ? fmaf(LA, oB, LB) : LB + LA * oB;
    LA = LA * oA;
}

struct RoScanArgs {
    const float *rew, *val, *term;
    const uint8_t *closed;
    const float *boot;
    int n_rows, T;
    float gamma, gl;
    int use_gae;
    float *adv, *ret;
};

// Roundings: the compiler is free to fuse x + a b into an fma, and xpa_gae_scan's compiled kernels fuse every one but
// two — in the DPP form, the segment scan's last combine and `first` (the two products become one packed multiply).
// The restatements below fix exactly those choices (contraction off, fmaf where gae.hip's kernels fuse), so that K33's
// adv / ret are xpa_gae_scan's to the last bit on the same record; tests/test_gpu_small_close.py compares them.
// Maintenance: the fused and non-fused spots are read off gae.hip's ISA as one compiler builds it.  If that test fails
// after a toolchain change with neither source changed, re-derive them from the new ISA of gae_scan_kernel<., ., 0>
// and gae_dpp_kernel<., 0> (v_fma / v_fmac against v_mul + v_add, v_pk_mul) and place fmaf accordingly; and any change
// to gae.hip's scan arithmetic has to be mirrored here.
// gae_scan_kernel<VEC, ., COMPACT = 0> (gae.hip) for the rows of wave index `wave`: lane sl of a row's L = 1 <<
// seg_log2 lanes owns VEC consecutive steps, chunks of L * VEC steps from the row's end with a register carry, the
// segmented scan on lane shuffles.  VEC = 4 takes T % 4 == 0 and 16-B aligned tensors.
template <int VEC>
__device__ __forceinline__ void ro_gae_scan_rows(const RoScanArgs &g, int wave, int seg_log2) {
#pragma clang fp contract(off)
    const int T = g.T;
    const int L = 1 << seg_log2;
    const int lane = threadIdx.x & 63;
    const int sl = lane & (L - 1);
    const int row = wave * (64 >> seg_log2) + (lane >> seg_log2);
    const bool row_ok = row < g.n_rows;
    const int64_t base = row_ok ? row * (int64_t)T : 0;
    const int C = L * VEC;
    const int nchunks = (T + C - 1) / C;
    float carry = 0.f, carry_v = 0.f;
    int carry_any = 0;
    for (int c = nchunks - 1; c >= 0; --c) {
        const int t0 = c * C + sl * VEC;
        float r[VEC], v[VEC], d[VEC], bt[VEC];
        int cl[VEC];
        const bool full = row_ok && (t0 + VEC <= T);
        if (VEC == 4 && full) {
            const float4 r4 = *reinterpret_cast<const float4 *>(g.rew + base + t0);
            const float4 v4 = *reinterpret_cast<const float4 *>(g.val + base + t0);
            const float4 d4 = *reinterpret_cast<const float4 *>(g.term + base + t0);
            const uint32_t c4 = *reinterpret_cast<const uint32_t *>(g.closed + base + t0);
            const float4 q4 = *reinterpret_cast<const float4 *>(g.boot + base + t0);
            bt[0] = q4.x; bt[1] = q4.y; bt[2] = q4.z; bt[3] = q4.w;
            r[0] = r4.x; r[1] = r4.y; r[2] = r4.z; r[3] = r4.w;
            v[0] = v4.x; v[1] = v4.y; v[2] = v4.z; v[3] = v4.w;
            d[0] = d4.x; d[1] = d4.y; d[2] = d4.z; d[3] = d4.w;
            cl[0] = c4 & 0xff; cl[1] = (c4 >> 8) & 0xff; cl[2] = (c4 >> 16) & 0xff; cl[3] = c4 >> 24;
        } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const int t = t0 + e;
                const bool ok = row_ok && t < T;
                r[e] = ok ? g.rew[base + t] : 0.f;
                v[e] = ok ? g.val[base + t] : 0.f;
                d[e] = ok ? g.term[base + t] : 0.f;
                cl[e] = ok ? (int)g.closed[base + t] : 0;
                bt[e] = cl[e] ? g.boot[base + t] : 0.f;
            }
        }
        // v_{t+1} of this lane's last element: the next lane's first v, or the later chunk's
        const int seg0 = lane & ~(L - 1);
        // (a lane whose partner would lie past the row's segment reads itself and does not use the value)
        float vn_lane = ro_lane(v[0], sl + 1 < L ? lane + 1 : lane);
        if (sl == L - 1) vn_lane = carry_v;
        float a[VEC], b[VEC], adv_direct[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const int t = t0 + e;
            const bool ok = row_ok && t < T;
            const float vnext = (e < VEC - 1) ? v[e + 1] : vn_lane;
            const float nv = cl[e] ? bt[e] : vnext;
            const float nd = 1.0f - d[e];
            if (g.use_gae) {
                b[e] = fmaf(g.gamma * nd, nv, r[e]) - v[e];
                a[e] = cl[e] ? 0.f : g.gl * nd;
            } else {
                b[e] = r[e] + (cl[e] ? g.gamma * bt[e] : 0.f);
                a[e] = cl[e] ? 0.f : g.gamma;
                adv_direct[e] = fmaf(g.gamma, nv, r[e]) - v[e];
            }
            if (!ok) { a[e] = 1.f; b[e] = 0.f; }
        }
        float LA = 1.f, LB = 0.f;   // the lane's own composition (last element first)
        int lany = 0;
#pragma unroll
        for (int e = VEC - 1; e >= 0; --e) {
            LB = fmaf(a[e], LB, b[e]);
            LA = a[e] * LA;
            lany |= cl[e];
        }
        for (int o = 1; o < L; o <<= 1) {   // segmented reverse inclusive scan across the row's lanes
            const int src = sl + o < L ? lane + o : lane;
            const float oA = ro_lane(LA, src);
            const float oB = ro_lane(LB, src);
            const int oany = ro_lane(lany, src);
            if (sl + o < L) {
                LB = fmaf(LA, oB, LB);
                LA = LA * oA;
                lany |= oany;
            }
        }
        const float first = fmaf(LA, carry, LB);
        const int any_first = lany | carry_any;
        float nxt = ro_lane(first, sl + 1 < L ? lane + 1 : lane);
        int nany = ro_lane(any_first, sl + 1 < L ? lane + 1 : lane);
        if (sl == L - 1) {
            nxt = carry;
            nany = carry_any;
        }
        float oa[VEC], orr[VEC];
        int wr[VEC];
#pragma unroll
        for (int e = VEC - 1; e >= 0; --e) {
            const float x = fmaf(a[e], nxt, b[e]);
            const int anyc = cl[e] | nany;
            if (g.use_gae) {
                oa[e] = x;
                orr[e] = x + v[e];
            } else {
                oa[e] = adv_direct[e];
                orr[e] = x;
            }
            wr[e] = anyc && row_ok && (t0 + e < T);
            nxt = x;
            nany = anyc;
        }
        if (VEC == 4 && full && wr[0] && wr[1] && wr[2] && wr[3]) {
            *reinterpret_cast<float4 *>(g.adv + base + t0) = make_float4(oa[0], oa[1], oa[2], oa[3]);
            *reinterpret_cast<float4 *>(g.ret + base + t0) = make_float4(orr[0], orr[1], orr[2], orr[3]);
        } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e)
                if (wr[e]) {
                    g.adv[base + t0 + e] = oa[e];
                    g.ret[base + t0 + e] = orr[e];
                }
        }
        carry = ro_lane(first, seg0);
        carry_v = ro_lane(v[0], seg0);
        carry_any = ro_lane(any_first, seg0);
    }
}

// gae_dpp_kernel<SEG_LOG2, COMPACT = 0> (gae.hip; T > 32, T % 4 == 0, 16-B aligned) for the rows of wave index `wave`:
// the lane order reversed inside a row segment (lane sl owns the 4 steps from c C + (L - 1 - sl) 4), so the reverse
// scan in time is a forward scan in lane order on DPP moves.
template <int SEG_LOG2>
__device__ __forceinline__ void ro_gae_dpp_rows(const RoScanArgs &g, int wave) {
#pragma clang fp contract(off)
    constexpr int L = 1 << SEG_LOG2;
    constexpr int C = 4 * L;
    const int T = g.T;
    const int lane = threadIdx.x & 63;
    const int sl = lane & (L - 1);
    const int seg_base = lane & ~(L - 1);
    const int row = wave * (64 / L) + (lane >> SEG_LOG2);
    const bool row_ok = row < g.n_rows;
    const int64_t base = row_ok ? row * (int64_t)T : 0;
    const int nchunks = (T + C - 1) / C;
    const uint64_t seg_mask = (L == 64) ? ~0ull : ((1ull << L) - 1ull);
    float carry = 0.f, carry_v = 0.f;
    bool carry_any = false;
    for (int c = nchunks - 1; c >= 0; --c) {
        const int t0 = c * C + (L - 1 - sl) * 4;
        const bool in = row_ok && t0 < T;   // T % 4 == 0: a lane's 4 steps are all in or all out
        float r[4] = {0.f, 0.f, 0.f, 0.f}, v[4] = {0.f, 0.f, 0.f, 0.f}, d[4] = {0.f, 0.f, 0.f, 0.f};
        float bt[4] = {0.f, 0.f, 0.f, 0.f};
        bool cl[4] = {false, false, false, false};
        if (in) {
            const float4 r4 = *reinterpret_cast<const float4 *>(g.rew + base + t0);
            const float4 v4 = *reinterpret_cast<const float4 *>(g.val + base + t0);
            const float4 d4 = *reinterpret_cast<const float4 *>(g.term + base + t0);
            const uint32_t c4 = *reinterpret_cast<const uint32_t *>(g.closed + base + t0);
            const float4 q4 = *reinterpret_cast<const float4 *>(g.boot + base + t0);
            r[0] = r4.x; r[1] = r4.y; r[2] = r4.z; r[3] = r4.w;
            v[0] = v4.x; v[1] = v4.y; v[2] = v4.z; v[3] = v4.w;
            d[0] = d4.x; d[1] = d4.y; d[2] = d4.z; d[3] = d4.w;
            bt[0] = q4.x; bt[1] = q4.y; bt[2] = q4.z; bt[3] = q4.w;
            cl[0] = (c4 & 0xff) != 0; cl[1] = ((c4 >> 8) & 0xff) != 0;
            cl[2] = ((c4 >> 16) & 0xff) != 0; cl[3] = (c4 >> 24) != 0;
        }
        // v_{t+1} of this lane's last step = v[0] of the lane below it (it owns the following steps)
        float vn = ro_dpp_mov<kRoDppWaveShr1>(0.f, v[0]);
        if (sl == 0) vn = carry_v;
        float a[4], b[4], adv_direct[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float vnext = (e < 3) ? v[e + 1] : vn;
            const float nv = cl[e] ? bt[e] : vnext;
            const float nd = 1.0f - d[e];
            if (g.use_gae) {
                b[e] = fmaf(g.gamma * nd, nv, r[e]) - v[e];
                a[e] = cl[e] ? 0.f : g.gl * nd;
            } else {
                b[e] = r[e] + (cl[e] ? g.gamma * bt[e] : 0.f);
                a[e] = cl[e] ? 0.f : g.gamma;
            }
            adv_direct[e] = fmaf(g.gamma, nv, r[e]) - v[e];
            if (!in) { a[e] = 1.f; b[e] = 0.f; }
        }
        float LA = 1.f, LB = 0.f;
        bool lany = false;
#pragma unroll
        for (int e = 3; e >= 0; --e) {
            LB = fmaf(a[e], LB, b[e]);
            LA = a[e] * LA;
            lany |= cl[e];
        }
        // inclusive scan in lane order inside the segment (lower lanes = later steps)
        ro_dpp_combine<kRoDppRowShr + 1, 0xf, true>(LA, LB);
        ro_dpp_combine<kRoDppRowShr + 2, 0xf, true>(LA, LB);
        ro_dpp_combine<kRoDppRowShr + 4, 0xf, true>(LA, LB);
        ro_dpp_combine<kRoDppRowShr + 8, 0xf, (L > 16)>(LA, LB);
        if (L >= 32) ro_dpp_combine<kRoDppRowBcast15, 0xa, (L > 32)>(LA, LB);
        if (L == 64) ro_dpp_combine<kRoDppRowBcast31, 0xc, false>(LA, LB);
        const float first = LB + LA * carry;   // A (or R) at this lane's first step (two roundings)
        const uint64_t segbits = (__ballot(lany) >> seg_base) & seg_mask;
        bool nany = carry_any || (segbits & ((1ull << sl) - 1ull)) != 0;
        float nxt = ro_dpp_mov<kRoDppWaveShr1>(0.f, first);
        if (sl == 0) nxt = carry;
        float oa[4], orr[4];
        bool wr[4];
#pragma unroll
        for (int e = 3; e >= 0; --e) {
            const float x = fmaf(a[e], nxt, b[e]);
            const bool anyc = cl[e] || nany;
            oa[e] = g.use_gae ? x : adv_direct[e];
            orr[e] = g.use_gae ? x + v[e] : x;
            wr[e] = anyc && in;
            nxt = x;
            nany = anyc;
        }
        if (wr[0] && wr[1] && wr[2] && wr[3]) {
            *reinterpret_cast<float4 *>(g.adv + base + t0) = make_float4(oa[0], oa[1], oa[2], oa[3]);
            *reinterpret_cast<float4 *>(g.ret + base + t0) = make_float4(orr[0], orr[1], orr[2], orr[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (wr[e]) {
                    g.adv[base + t0 + e] = oa[e];
                    g.ret[base + t0 + e] = orr[e];
                }
        }
        if (c > 0) {   // the earlier chunk continues from this chunk's first step (lane L - 1)
            carry = ro_lane(first, seg_base + L - 1);
            carry_v = ro_lane(v[0], seg_base + L - 1);
            carry_any = carry_any || segbits != 0;
        }
    }
}

template <int ACT, int H0>
__device__ __forceinline__ void small_close_body(const XpaSmallCloseArgs &args) {
    const XpaSmallCloseArgs a = args;
    extern __shared__ float lds[];
    constexpr int DM = 8;   // the widest observation
    const int tid = threadIdx.x;
    const int N = a.n_envs, D = a.d_in, H1 = a.h1, H2 = a.h2, U = a.h1 + a.h2, T = a.horizon, S = a.n_slots;
    const RoLayout L = ro_layout(N, D, H0, H1, H2, a.k);
    float *sy = lds + L.sy, *sz = lds + L.sz;   // sz: the value's partial sums [wave][N]
    constexpr bool WIDE = H0 == kRoWide;
    const int wave = tid >> 6, lane = tid & 63;
    const int li = lane & 15, lq = lane >> 4;
    constexpr int KK = H0 / 4, J = WIDE ? 4 : 2, KW = WIDE ? 1 : KK;
    const int UT = U >> 4;
    float w0k[KW][DM], b0k[KW];
#pragma unroll
    for (int kk = 0; kk < KW; ++kk) {
        const int k = WIDE ? (tid & (kRoWide - 1)) : 4 * kk + lq;
#pragma unroll
        for (int d = 0; d < DM; ++d) w0k[kk][d] = d < D ? a.W0[k * D + d] : 0.f;
        b0k[kk] = a.b0[k];
    }
    float bw[J][KK], b12[J], wc[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int tile = wave + 4 * j;
        const bool tok = tile < UT;
        const int u = tok ? 16 * tile + li : 0;
        const bool actor = u < H1;
        const float *wr = actor ? a.W1 + u * H0 : a.W2 + (u - H1) * H0;
#pragma unroll
        for (int kk = 0; kk < KK; ++kk) bw[j][kk] = tok ? wr[4 * kk + lq] : 0.f;
        b12[j] = tok ? (actor ? a.b1[u] : a.b2[u - H1]) : 0.f;
        wc[j] = tok && !actor ? a.Wc[u - H1] : 0.f;
    }
    const float bc = a.bc[0];
    const int64_t rbase = (int64_t)tid * T;   // thread n < N: env n's row
    for (int k = 0; k <= S; ++k) {
        if (k > 0) __syncthreads();   // the previous pass's rows and partial sums are read
        for (int e = tid; e < N * D; e += kRoThreads) {
            const int r = e / D, d = e % D;
            sy[e] = a.rows[((int64_t)k * N + r) * a.ld_rows + d];
        }
        __syncthreads();
        for (int r0 = 0; r0 < N; r0 += 16) {
            ro_f32x4 acc[J];
#pragma unroll
            for (int j = 0; j < J; ++j) acc[j] = ro_f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (WIDE) {
                float *sh = lds + L.sh;
                if (r0 > 0) __syncthreads();   // the previous tile's A operands are read
                const int u = tid & (kRoWide - 1), rh = tid >> 7;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int row = rh + 2 * i;
                    const float *yr = sy + (r0 + row < N ? r0 + row : N - 1) * D;
                    float z = b0k[0];
#pragma unroll
                    for (int d = 0; d < DM; ++d)
                        if (d < D) z = fmaf(w0k[0][d], yr[d], z);   // ascending d
                    sh[row * kRoWideP + (u & 3) * kRoWideQ + (u >> 2)] = ro_act<ACT>(z, a.slope);
                }
                __syncthreads();
                const float *ap = sh + li * kRoWideP + lq * kRoWideQ;
#pragma unroll
                for (int k4 = 0; k4 < KK; k4 += 4) {
                    const float4 a4 = *reinterpret_cast<const float4 *>(ap + k4);
                    const float av[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
                    for (int c = 0; c < 4; ++c)
#pragma unroll
                        for (int j = 0; j < J; ++j)
                            acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[c], bw[j][k4 + c], acc[j], 0, 0, 0);
                }
            } else {
                const int ra = r0 + li < N ? r0 + li : N - 1;   // this lane's A row (rows past N: results unused)
                float y[DM];
#pragma unroll
                for (int d = 0; d < DM; ++d) y[d] = d < D ? sy[ra * D + d] : 0.f;
                float av[KK];
#pragma unroll
                for (int kk = 0; kk < KK; ++kk) {
                    float z = b0k[kk];
#pragma unroll
                    for (int d = 0; d < DM; ++d)
                        if (d < D) z = fmaf(w0k[kk][d], y[d], z);   // ascending d
                    av[kk] = ro_act<ACT>(z, a.slope);
                }
#pragma unroll
                for (int kk = 0; kk < KK; ++kk)
#pragma unroll
                    for (int j = 0; j < J; ++j)
                        acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[kk], bw[j][kk], acc[j], 0, 0, 0);
            }
            // D element r of lane (q, i): row r0 + 4 q + r, unit 16 tile + i
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float pv = 0.f;
#pragma unroll
                for (int j = 0; j < J; ++j) pv = fmaf(wc[j], ro_act<ACT>(acc[j][r] + b12[j], a.slope), pv);
                pv = ro_row_sum16(pv);
                const int m = r0 + 4 * lq + r;
                if (li == 0 && m < N) sz[wave * N + m] = pv;
            }
        }
        __syncthreads();
        if (tid < N) {
            float v = bc;
            for (int w = 0; w < 4; ++w) v += sz[w * N + tid];
            const int64_t sl = (int64_t)k * N + tid;
            if (a.vboot_out) a.vboot_out[sl] = v;
            if (k < S) {   // bootstrap_fixup_kernel's writes
                const int t = a.slot_t[sl];
                if (t >= 0 && t < T) a.boot[rbase + t] = v;
                a.slot_t[sl] = -1;
            } else {
                a.boot[rbase + T - 1] = a.term[rbase + T - 1] != 0.f ? 0.f : v;
            }
        }
    }
    __syncthreads();   // the bootstraps in boot (global stores of this workgroup) are visible to its scan
    // the advantage scan: xpa_gae_scan's choice of form, the four waves over the wave indices
    const RoScanArgs g{a.rew, a.val, a.term, a.closed, a.boot, N, T, a.gamma, a.gamma * a.gae_lambda, a.use_gae,
                       a.adv, a.ret};
    const bool vec4 = T % 4 == 0 && ((((uintptr_t)a.rew | (uintptr_t)a.val | (uintptr_t)a.term | (uintptr_t)a.boot |
                                       (uintptr_t)a.adv | (uintptr_t)a.ret) & 15) == 0) &&
                      (((uintptr_t)a.closed & 3) == 0);
    const int per_lane = vec4 ? T / 4 : T;
    int seg_log2 = 0;
    while ((1 << seg_log2) < per_lane && seg_log2 < 6) ++seg_log2;
    const int rows_per_wave = 64 >> seg_log2;
    for (int w = wave; w * rows_per_wave < N; w += kRoThreads / 64) {
        if (!vec4) ro_gae_scan_rows<1>(g, w, seg_log2);
        else if (seg_log2 == 4) ro_gae_dpp_rows<4>(g, w);
        else if (seg_log2 == 5) ro_gae_dpp_rows<5>(g, w);
        else if (seg_log2 == 6) ro_gae_dpp_rows<6>(g, w);
        else ro_gae_scan_rows<4>(g, w, seg_log2);
    }
}

template <int ACT, int H0>
__global__ __launch_bounds__(kRoThreads) void small_close_kernel(XpaSmallCloseArgs a) {
    small_close_body<ACT, H0>(a);
}

// The population form (xpa_small_close_batch): workgroup p closes agent p's rollout from its own block
template <int ACT, int H0>
__global__ __launch_bounds__(kRoThreads) void small_close_batch_kernel(const XpaSmallCloseArgs *__restrict__ blocks) {
    const XpaSmallCloseArgs a = blocks[blockIdx.x];
    small_close_body<ACT, H0>(a);
}

// xpa_eval_post: one workgroup walks the envs in passes of kEvalThreads, so a step's entries land in env order (lane
// offset from the wave's ballot, wave offset from the pass's wave totals, pass offset carried along).
constexpr int kEvalThreads = 1024;
__global__ __launch_bounds__(kEvalThreads) void eval_post_kernel(
    int32_t *__restrict__ log, int64_t capacity, int64_t ent0, int64_t n_envs, const uint8_t *__restrict__ term,
    const uint8_t *__restrict__ trunc, const float *__restrict__ ep_last_score,
    const int32_t *__restrict__ ep_last_len, int atari_lifeloss, xpa_cursor_t *__restrict__ cur,
    const float *__restrict__ obs_mean, const float *__restrict__ obs_var, const double *__restrict__ obs_count,
    int64_t snap_dim) {
    __shared__ int s_wtot[kEvalThreads / 64];
    if (log[kLogDone] != 0) return;   // block-uniform
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int32_t step = log[kLogSteps];
    int64_t count = log[kLogCount];
    const int32_t target = log[kLogTarget];
    for (int64_t n0 = 0; n0 < n_envs; n0 += kEvalThreads) {
        const int64_t n = n0 + tid;
        bool fin = false;
        if (n < n_envs) {
            const bool te = term[n] != 0, tr = trunc[n] != 0;
            fin = (te || tr) && !(atari_lifeloss && !tr);   // a life loss: the game goes on
        }
        const unsigned long long m = __ballot(fin);
        if (lane == 0) s_wtot[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < kEvalThreads / 64; ++w) {
            if (w < wave) before += s_wtot[w];
            total += s_wtot[w];
        }
        if (fin)
            eval_log_put(log, ent0, capacity, count + before + __popcll(m & ((1ull << lane) - 1ull)), step, (int32_t)n,
                         ep_last_score[n], ep_last_len[n]);
        count += total;
        __syncthreads();   // s_wtot free for the next pass
    }
    const bool latch = count >= target;
    if (latch && obs_count) {   // the statistics as they stand after this step's update (the host restores them)
        float *snap = reinterpret_cast<float *>(log + kLogHeader);
        for (int64_t d = tid; d < snap_dim; d += kEvalThreads) {
            snap[2 + d] = obs_mean[d];
            snap[2 + snap_dim + d] = obs_var[d];
        }
        if (tid == 0) *reinterpret_cast<double *>(snap) = *obs_count;
    }
    if (tid == 0) {
        log[kLogCount] = (int32_t)count;
        log[kLogSteps] = step + 1;
        if (latch) log[kLogDone] = 1;
        cur->ptr = 0;
        cur->step = cur->step + 1u;
    }
}

}  // namespace

// ---- K4 --------------------------------------------------------------------------------------------
XPA_API int64_t xpa_gather_num_partials(int64_t batch) { return (batch + kGatherRows - 1) / kGatherRows; }

XPA_API int xpa_gather_minibatch(const int64_t *idx, int64_t batch, int64_t n_rows, const void *obs,
                                 int64_t obs_row_bytes, void *obs_out, const float *adv, double *adv_partials,
                                 int32_t *err, xpa_stream_t stream) {
    if (batch <= 0 || n_rows <= 0 || obs_row_bytes < 0 || !idx) return (int)hipErrorInvalidValue;
    if (obs_row_bytes > 0 && (!obs || !obs_out)) return (int)hipErrorInvalidValue;
    if (adv_partials && !adv) return (int)hipErrorInvalidValue;
    const int64_t blocks = xpa_gather_num_partials(batch);
    hipStream_t s = (hipStream_t)stream;
    const uintptr_t al = (uintptr_t)obs | (uintptr_t)obs_out;
    if (obs_row_bytes >= 4096 && obs_row_bytes % 16 == 0 && al % 16 == 0) {
        const int64_t rv = obs_row_bytes / 16, chunks = (rv + 256 * kWideU - 1) / (256 * kWideU);
        if (batch * chunks > 0x7fffffffLL) return (int)hipErrorInvalidValue;
        hipLaunchKernelGGL(gather_wide_kernel, dim3((unsigned)(batch * chunks)), dim3(256), 0, s, idx, n_rows,
                           (const u4v *)obs, rv, chunks, (u4v *)obs_out, err);
        if (adv_partials)  // the moments alone (no row copy)
            hipLaunchKernelGGL(gather_rows_kernel<uint4>, dim3((unsigned)blocks), dim3(256), 0, s, idx, batch, n_rows,
                               (const uint4 *)obs, (int64_t)0, (uint4 *)obs_out, adv, adv_partials,
                               (int *)nullptr);
    } else if (obs_row_bytes % 16 == 0 && al % 16 == 0)
        hipLaunchKernelGGL(gather_rows_kernel<uint4>, dim3((unsigned)blocks), dim3(256), 0, s, idx, batch,
                           n_rows, (const uint4 *)obs, obs_row_bytes / 16, (uint4 *)obs_out, adv, adv_partials, err);
    else if (obs_row_bytes % 4 == 0 && al % 4 == 0)
        hipLaunchKernelGGL(gather_rows_kernel<uint32_t>, dim3((unsigned)blocks), dim3(256), 0, s, idx, batch,
                           n_rows, (const uint32_t *)obs, obs_row_bytes / 4, (uint32_t *)obs_out, adv, adv_partials,
                           err);
    else
        hipLaunchKernelGGL(gather_rows_kernel<uint8_t>, dim3((unsigned)blocks), dim3(256), 0, s, idx, batch,
                           n_rows, (const uint8_t *)obs, obs_row_bytes, (uint8_t *)obs_out, adv, adv_partials, err);
    return xpa_launch_status();
}

// r05: K4 into rows of pitch out_row_bytes >= obs_row_bytes (the bytes past each row's obs_row_bytes untouched: the
// C4 trunk's zero-padded K40F operand, 376 -> 384 floats); 16-B vectors only
XPA_API int xpa_gather_minibatch_pitched(const int64_t *idx, int64_t batch, int64_t n_rows, const void *obs,
                                         int64_t obs_row_bytes, void *obs_out, int64_t out_row_bytes,
                                         const float *adv, double *adv_partials, int32_t *err, xpa_stream_t stream) {
    if (batch <= 0 || n_rows <= 0 || obs_row_bytes <= 0 || !idx || !obs || !obs_out || out_row_bytes < obs_row_bytes ||
        obs_row_bytes % 16 || out_row_bytes % 16 || (((uintptr_t)obs | (uintptr_t)obs_out) % 16) ||
        (adv_partials && !adv))
        return (int)hipErrorInvalidValue;
    const int64_t blocks = xpa_gather_num_partials(batch);
    if ((int64_t)kGatherRows * (obs_row_bytes / 16) > 0xffffffffLL) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(gather_rows_kernel<uint4>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, idx, batch,
                       n_rows, (const uint4 *)obs, obs_row_bytes / 16, (uint4 *)obs_out, adv, adv_partials, err,
                       out_row_bytes / 16);
    return xpa_launch_status();
}

// ---- K5 --------------------------------------------------------------------------------------------
XPA_API int64_t xpa_rms_num_partials(int64_t n) { return (n + kRmsRows - 1) / kRmsRows; }

XPA_API int xpa_rms_partials(const float *x, int64_t n, int64_t dim, int64_t ld, const float *shift,
                             double *partials, xpa_stream_t stream) {
    if (n <= 0 || dim <= 0 || ld < dim || !x || !partials) return (int)hipErrorInvalidValue;
    const int64_t np = xpa_rms_num_partials(n);
    if (dim > kRmsWideDim)
        hipLaunchKernelGGL((rms_partials_cols_kernel<false>), dim3((unsigned)np, (unsigned)((dim + 63) / 64)), dim3(1024),
                           0, (hipStream_t)stream, x, n, dim, ld, shift, partials, (float *)nullptr, (float *)nullptr,
                           (double *)nullptr, (unsigned int *)nullptr);
    else
        hipLaunchKernelGGL((rms_partials_kernel<false, 256>), dim3((unsigned)np), dim3(256), 0, (hipStream_t)stream, x,
                           n, dim, ld, shift, partials, (float *)nullptr, (float *)nullptr, (double *)nullptr,
                           (unsigned int *)nullptr);
    return xpa_launch_status();
}

XPA_API int xpa_rms_update(const float *x, int64_t n, int64_t dim, int64_t ld, float *mean, float *var,
                           double *count, double *partials, int32_t *ticket, xpa_stream_t stream) {
    if (n <= 0 || dim <= 0 || ld < dim || !x || !mean || !var || !count || !partials || !ticket)
        return (int)hipErrorInvalidValue;
    const int64_t np = xpa_rms_num_partials(n);
    if (dim > kRmsWideDim)
        hipLaunchKernelGGL((rms_partials_cols_kernel<true>), dim3((unsigned)np, (unsigned)((dim + 63) / 64)), dim3(1024),
                           0, (hipStream_t)stream, x, n, dim, ld, (const float *)mean, partials, mean, var, count,
                           (unsigned int *)ticket);
    else
        hipLaunchKernelGGL((rms_partials_kernel<true, 256>), dim3((unsigned)np), dim3(256), 0, (hipStream_t)stream, x,
                           n, dim, ld, (const float *)mean, partials, mean, var, count, (unsigned int *)ticket);
    return xpa_launch_status();
}

XPA_API int xpa_rms_merge(const double *partials, int64_t n_partials, int64_t n, int64_t dim, float *mean,
                          float *var, double *count, xpa_stream_t stream) {
    if (n <= 0 || dim <= 0 || n_partials <= 0 || !partials || !mean || !var || !count)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(rms_merge_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, n_partials, n, dim,
                       mean, var, count);
    return xpa_launch_status();
}

XPA_API int xpa_obs_normalize(const float *x, int64_t n, int64_t dim, int64_t ldx, const float *mean,
                              const float *var, float clip_range, float *out, int64_t ldo, float *col_out,
                              int64_t col_ld, const xpa_cursor_t *cursor, xpa_stream_t stream) {
    if (n <= 0 || dim <= 0 || ldx < dim || ldo < dim || !x || !mean || !var || !out) return (int)hipErrorInvalidValue;
    if (col_out && (!cursor || col_ld < dim)) return (int)hipErrorInvalidValue;
    const int64_t total = n * dim;
    int64_t blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(obs_normalize_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, n, dim, ldx,
                       mean, var, clip_range, out, ldo, col_out, col_ld, cursor);
    return xpa_launch_status();
}

// ---- K3 --------------------------------------------------------------------------------------------
XPA_API int xpa_rollout_sample(int dist, int64_t n_envs, int64_t act_dim, int64_t horizon, const float *head,
                               const float *logstd, const float *v, const xpa_cursor_t *cursor, uint32_t seed,
                               float act_clip, float *buf_act, float *buf_logp, float *buf_val, float *env_in,
                               int64_t ld_env, xpa_stream_t stream) {
    if (n_envs <= 0 || act_dim <= 0 || horizon <= 0 || !head || !v || !cursor || !buf_act || !buf_logp ||
        !buf_val || !env_in || ld_env < act_dim)
        return (int)hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((n_envs + 255) / 256);
    hipStream_t s = (hipStream_t)stream;
    if (dist == XPA_DIST_GAUSSIAN) {
        if (!logstd) return (int)hipErrorInvalidValue;
        hipLaunchKernelGGL(rollout_sample_gauss_kernel, dim3(blocks), dim3(256), 0, s, n_envs, (int)act_dim, horizon,
                           head, logstd, v, cursor, seed, act_clip, buf_act, buf_logp, buf_val, env_in, ld_env);
    } else if (dist == XPA_DIST_CATEGORICAL) {
        if (act_dim < 2) return (int)hipErrorInvalidValue;
        hipLaunchKernelGGL(rollout_sample_cat_kernel, dim3(blocks), dim3(256), 0, s, n_envs, (int)act_dim, horizon,
                           head, v, cursor, seed, buf_act, buf_logp, buf_val, env_in, ld_env);
    } else {
        return (int)hipErrorInvalidValue;
    }
    return xpa_launch_status();
}

// ---- K7 --------------------------------------------------------------------------------------------
XPA_API int xpa_synthbox_step(int64_t n_envs, int64_t obs_dim, const float *pre, uint32_t seed,
                              int32_t max_episode_steps, float noise, float term_thresh, float reset_scale,
                              float *state, int64_t ld_state, float *final_obs, float *rew, uint8_t *term,
                              uint8_t *trunc, int32_t *ep_step, uint32_t *ep_index, float *ep_score,
                              float *ep_last_score, int32_t *ep_last_len, xpa_stream_t stream) {
    if (n_envs <= 0 || obs_dim <= 0 || ld_state < obs_dim || !pre || !state || !final_obs || !rew || !term ||
        !trunc || !ep_step || !ep_index || !ep_score || !ep_last_score || !ep_last_len)
        return (int)hipErrorInvalidValue;
    SynthEnvArgs e{(int)obs_dim, seed, max_episode_steps, noise, term_thresh, reset_scale, state, ld_state, final_obs,
                   rew, term, trunc, ep_step, ep_index, ep_score, ep_last_score, ep_last_len, nullptr};
    const unsigned blocks = (unsigned)((n_envs + 3) / 4);
    hipLaunchKernelGGL(synthbox_step_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, pre, e, n_envs);
    return xpa_launch_status();
}

// ---- K8 --------------------------------------------------------------------------------------------
XPA_API int64_t xpa_rollout_post_num_blocks(int64_t n_envs) {
    return (n_envs + kPostThreads - 1) / kPostThreads;
}

XPA_API int xpa_rollout_post(int64_t n_envs, int64_t horizon, const float *rew, const uint8_t *term,
                             const uint8_t *trunc, const float *v_boot, const float *v_boot_mid,
                             xpa_cursor_t *cursor, float *ret_mean,
                             float *ret_var, double *ret_count, float *returns, float *buf_rew, float *buf_term,
                             uint8_t *buf_closed, float *buf_boot, float gamma, int mask_returns, int use_rewnorm,
                             float rew_range, int atari_lifeloss, double *partials, uint32_t *ticket,
                             xpa_stream_t stream) {
    if (n_envs <= 0 || horizon <= 0 || !rew || !term || !trunc || !v_boot || !cursor || !ret_mean || !ret_var ||
        !ret_count || !returns || !buf_rew || !buf_term || !buf_closed || !buf_boot || !partials || !ticket ||
        xpa_rollout_post_num_blocks(n_envs) > 0x7fffffff)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(rollout_post_kernel<false>, dim3((unsigned)xpa_rollout_post_num_blocks(n_envs)),
                       dim3(kPostThreads), 0, (hipStream_t)stream, n_envs, horizon, rew, term, trunc, v_boot, cursor,
                       ret_mean, ret_var, ret_count, returns, buf_rew, buf_term, buf_closed, buf_boot, gamma,
                       mask_returns, use_rewnorm, rew_range, atari_lifeloss, (const float *)nullptr, (int64_t)0,
                       (int64_t)0, (float *)nullptr, (int *)nullptr, 0, (int *)nullptr, partials, (unsigned *)ticket,
                       (const float *)nullptr, (const float *)nullptr, 0.f, (float *)nullptr, (int64_t)0,
                       (const float *)nullptr, (int64_t)0, v_boot_mid);
    return xpa_launch_status();
}

XPA_API int xpa_rollout_post_deferred(int64_t n_envs, int64_t horizon, const float *rew, const uint8_t *term,
                                      const uint8_t *trunc, const float *boot_obs, int64_t ld_boot, int64_t obs_dim,
                                      float *slot_obs, int32_t *slot_t, int64_t n_slots, int32_t *overflow,
                                      xpa_cursor_t *cursor, float *ret_mean, float *ret_var, double *ret_count,
                                      float *returns, float *buf_rew, float *buf_term, uint8_t *buf_closed,
                                      float *buf_boot, float gamma, int mask_returns, int use_rewnorm,
                                      float rew_range, int atari_lifeloss, double *partials, uint32_t *ticket,
                                      xpa_stream_t stream) {
    if (n_envs <= 0 || horizon <= 0 || obs_dim <= 0 || ld_boot < obs_dim || n_slots < 1 || n_slots > horizon ||
        !rew || !term || !trunc || !boot_obs ||
        !slot_obs || !slot_t || !overflow || !cursor || !ret_mean || !ret_var || !ret_count || !returns || !buf_rew ||
        !buf_term || !buf_closed || !buf_boot || !partials || !ticket || xpa_rollout_post_num_blocks(n_envs) > 0x7fffffff)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(rollout_post_kernel<true>, dim3((unsigned)xpa_rollout_post_num_blocks(n_envs)),
                       dim3(kPostThreads), 0, (hipStream_t)stream, n_envs, horizon, rew, term, trunc,
                       (const float *)nullptr, cursor, ret_mean, ret_var, ret_count, returns, buf_rew, buf_term,
                       buf_closed, buf_boot, gamma, mask_returns, use_rewnorm, rew_range, atari_lifeloss, boot_obs,
                       ld_boot, obs_dim, slot_obs, slot_t, (int)n_slots, overflow, partials, (unsigned *)ticket,
                       (const float *)nullptr, (const float *)nullptr, 0.f, (float *)nullptr, (int64_t)0);
    return xpa_launch_status();
}

XPA_API int xpa_rollout_post_deferred_norm(int64_t n_envs, int64_t horizon, const float *rew, const uint8_t *term,
                                           const uint8_t *trunc, const float *final_obs, int64_t ld_final,
                                           const float *slot_src, int64_t ld_slot, int64_t obs_dim, const float *obs_mean, const float *obs_var,
                                           float obs_clip, float *boot_norm, int64_t ld_norm, float *slot_obs,
                                           int32_t *slot_t, int64_t n_slots, int32_t *overflow,
                                           xpa_cursor_t *cursor, float *ret_mean,
                                           float *ret_var, double *ret_count, float *returns, float *buf_rew,
                                           float *buf_term, uint8_t *buf_closed, float *buf_boot, float gamma,
                                           int mask_returns, int use_rewnorm, float rew_range, int atari_lifeloss,
                                           double *partials, uint32_t *ticket, xpa_stream_t stream) {
    if (n_envs <= 0 || horizon <= 0 || obs_dim <= 0 || ld_final < obs_dim || ld_norm < obs_dim || n_slots < 1 ||
        n_slots > horizon || (slot_src && ld_slot < obs_dim) || !rew || !term ||
        !trunc || !final_obs || !obs_mean || !obs_var || !boot_norm || !slot_obs || !slot_t || !overflow || !cursor ||
        !ret_mean || !ret_var || !ret_count || !returns || !buf_rew || !buf_term || !buf_closed || !buf_boot ||
        !partials || !ticket || xpa_rollout_post_num_blocks(n_envs) > 0x7fffffff)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL((rollout_post_kernel<true, true>), dim3((unsigned)xpa_rollout_post_num_blocks(n_envs)),
                       dim3(kPostThreads), 0, (hipStream_t)stream, n_envs, horizon, rew, term, trunc,
                       (const float *)nullptr, cursor, ret_mean, ret_var, ret_count, returns, buf_rew, buf_term,
                       buf_closed, buf_boot, gamma, mask_returns, use_rewnorm, rew_range, atari_lifeloss, final_obs,
                       ld_final, obs_dim, slot_obs, slot_t, (int)n_slots, overflow, partials, (unsigned *)ticket,
                       obs_mean, obs_var, obs_clip, boot_norm, ld_norm, slot_src, ld_slot);
    return xpa_launch_status();
}

// r05: xpa_rollout_post_deferred_norm with the NEXT step's obs_rms.update folded in (rms_x [n_envs, rms_dim], row
// stride rms_ld: the observation the env step just produced; rms_part f64 [2 * xpa_rollout_post_num_blocks(n_envs),
// rms_dim]; obs_mean / obs_var / obs_count updated in place by the last block, after every block normalised with the
// old statistics).  obs_dim <= 64.
XPA_API int xpa_rollout_post_deferred_norm_rms(
    int64_t n_envs, int64_t horizon, const float *rew, const uint8_t *term, const uint8_t *trunc, const float *final_obs,
    int64_t ld_final, const float *slot_src, int64_t ld_slot, int64_t obs_dim, float *obs_mean, float *obs_var,
    double *obs_count, float obs_clip, float *boot_norm, int64_t ld_norm, float *slot_obs, int32_t *slot_t,
    int64_t n_slots, int32_t *overflow, xpa_cursor_t *cursor, float *ret_mean, float *ret_var, double *ret_count,
    float *returns, float *buf_rew, float *buf_term, uint8_t *buf_closed, float *buf_boot, float gamma,
    int mask_returns, int use_rewnorm, float rew_range, int atari_lifeloss, double *partials, uint32_t *ticket,
    const float *rms_x, int64_t rms_ld, double *rms_part, xpa_stream_t stream) {
    if (n_envs <= 0 || horizon <= 0 || obs_dim <= 0 || obs_dim > kPostRmsMax || ld_final < obs_dim ||
        ld_norm < obs_dim || n_slots < 1 || n_slots > horizon || (slot_src && ld_slot < obs_dim) || !rew || !term ||
        !trunc || !final_obs || !obs_mean || !obs_var || !obs_count || !boot_norm || !slot_obs || !slot_t ||
        !overflow || !cursor || !ret_mean || !ret_var || !ret_count || !returns || !buf_rew || !buf_term ||
        !buf_closed || !buf_boot || !partials || !ticket || !rms_x || rms_ld < obs_dim || !rms_part ||
        xpa_rollout_post_num_blocks(n_envs) > 0x7fffffff)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL((rollout_post_kernel<true, true, true>), dim3((unsigned)xpa_rollout_post_num_blocks(n_envs)),
                       dim3(kPostThreads), 0, (hipStream_t)stream, n_envs, horizon, rew, term, trunc,
                       (const float *)nullptr, cursor, ret_mean, ret_var, ret_count, returns, buf_rew, buf_term,
                       buf_closed, buf_boot, gamma, mask_returns, use_rewnorm, rew_range, atari_lifeloss, final_obs,
                       ld_final, obs_dim, slot_obs, slot_t, (int)n_slots, overflow, partials, (unsigned *)ticket,
                       obs_mean, obs_var, obs_clip, boot_norm, ld_norm, slot_src, ld_slot, (const float *)nullptr,
                       rms_x, rms_ld, (int)obs_dim, rms_part, obs_mean, obs_var, obs_count);
    return xpa_launch_status();
}

namespace {
// v = V([slot rows (n_slots x n_envs); last-step rows (n_envs)]): every used slot's bootstrap, then the last column's.
__global__ __launch_bounds__(256) void bootstrap_fixup_kernel(int64_t n_envs, int64_t T, int n_slots,
                                                              const float *__restrict__ v, int *__restrict__ slot_t,
                                                              const float *__restrict__ buf_term,
                                                              float *__restrict__ buf_boot) {
    const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= n_envs) return;
    for (int k = 0; k < n_slots; ++k) {
        const int64_t sl = (int64_t)k * n_envs + n;
        const int t = slot_t[sl];
        if (t >= 0 && t < T) buf_boot[n * T + t] = v[sl];
        slot_t[sl] = -1;
    }
    const int64_t last = n * T + T - 1;
    buf_boot[last] = buf_term[last] != 0.f ? 0.f : v[(int64_t)n_slots * n_envs + n];
}
}  // namespace

XPA_API int xpa_rollout_bootstrap_fixup(int64_t n_envs, int64_t horizon, const float *values, int32_t *slot_t,
                                        int64_t n_slots, const float *buf_term, float *buf_boot, xpa_stream_t stream) {
    if (n_envs <= 0 || horizon <= 0 || n_slots < 1 || n_slots > horizon || !values || !slot_t || !buf_term ||
        !buf_boot)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(bootstrap_fixup_kernel, dim3((unsigned)((n_envs + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, n_envs, horizon, (int)n_slots, values, slot_t, buf_term, buf_boot);
    return xpa_launch_status();
}

// ---- K14 -------------------------------------------------------------------------------------------
XPA_API int xpa_rollout_policy_head(int dist, int act, int64_t n_envs, int64_t act_dim, int64_t horizon,
                                    int64_t hidden, int64_t ld, const float *z_actor, const float *z_critic,
                                    float slope, const float *w_actor, const float *b_actor, const float *w_critic,
                                    const float *b_critic, const float *logstd, const xpa_cursor_t *cursor,
                                    uint32_t seed, float act_clip, float *buf_act, float *buf_logp, float *buf_val,
                                    float *env_in, int64_t ld_env, xpa_stream_t stream) {
    if (n_envs <= 0 || act_dim < 1 || act_dim > kRolloutKMax || horizon <= 0 || hidden != 256 || ld < 256 || ld % 4 ||
        act < 0 || act > 2 || !z_actor || !z_critic || !w_actor || !b_actor || !w_critic || !b_critic || !cursor ||
        !buf_act || !buf_logp || !buf_val || !env_in || ld_env < act_dim)
        return (int)hipErrorInvalidValue;
    if (((uintptr_t)z_actor | (uintptr_t)z_critic | (uintptr_t)w_actor | (uintptr_t)w_critic) % 16)
        return (int)hipErrorInvalidValue;
    if ((dist == XPA_DIST_GAUSSIAN && !logstd) || (dist == XPA_DIST_CATEGORICAL && act_dim < 2) ||
        (dist != XPA_DIST_GAUSSIAN && dist != XPA_DIST_CATEGORICAL))
        return (int)hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((n_envs + 3) / 4);
    hipStream_t s = (hipStream_t)stream;
#define XPA_K14(M_, A_)                                                                                          \
    hipLaunchKernelGGL((rollout_policy_head_kernel<M_, A_>), dim3(blocks), dim3(256), 0, s, n_envs, (int)act_dim, \
                       horizon, z_actor, z_critic, ld, slope, w_actor, b_actor, w_critic, b_critic, logstd, cursor,   \
                       seed, act_clip, buf_act, buf_logp, buf_val, env_in, ld_env, (float *)nullptr, SynthEnvArgs{})
    if (dist == XPA_DIST_GAUSSIAN) {
        if (act == 0) XPA_K14(0, 0);
        else if (act == 1) XPA_K14(0, 1);
        else XPA_K14(0, 2);
    } else {
        if (act == 0) XPA_K14(1, 0);
        else if (act == 1) XPA_K14(1, 1);
        else XPA_K14(1, 2);
    }
#undef XPA_K14
    return xpa_launch_status();
}

XPA_API int xpa_value_head(int act, int64_t n, int64_t hidden, int64_t ld, const float *z_critic, float slope,
                           const float *w_critic, const float *b_critic, float *v_out, xpa_stream_t stream) {
    if (n <= 0 || hidden != 256 || ld < 256 || ld % 4 || act < 0 || act > 2 || !z_critic || !w_critic ||
        !b_critic || !v_out || ((uintptr_t)z_critic | (uintptr_t)w_critic) % 16)
        return (int)hipErrorInvalidValue;
    const unsigned blocks = (unsigned)((n + 3) / 4);
    hipStream_t s = (hipStream_t)stream;
#define XPA_VH(A_)                                                                                                 \
    hipLaunchKernelGGL((rollout_policy_head_kernel<2, A_>), dim3(blocks), dim3(256), 0, s, n, 1, (int64_t)1,        \
                       z_critic, z_critic, ld, slope, w_critic, b_critic, w_critic, b_critic, (const float *)nullptr, \
                       (const xpa_cursor_t *)nullptr, 0u, 0.f, (float *)nullptr, (float *)nullptr, (float *)nullptr, \
                       (float *)nullptr, (int64_t)0, v_out, SynthEnvArgs{})
    if (act == 0) XPA_VH(0);
    else if (act == 1) XPA_VH(1);
    else XPA_VH(2);
#undef XPA_VH
    return xpa_launch_status();
}

XPA_API int xpa_store_column(const void *src, int64_t n, int64_t row_bytes, void *dst, int64_t horizon,
                             const xpa_cursor_t *cursor, xpa_stream_t stream) {
    if (n <= 0 || row_bytes <= 0 || row_bytes % 16 || horizon <= 0 || !src || !dst || !cursor ||
        ((uintptr_t)src | (uintptr_t)dst) % 16)
        return (int)hipErrorInvalidValue;
    const int64_t rv = row_bytes / 16;
    int64_t blocks = (n * rv + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(store_column_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       (const u4v *)src, n, rv, (u4v *)dst, horizon, cursor);
    return xpa_launch_status();
}

XPA_API int xpa_random_permutation(int64_t n, uint32_t seed, uint32_t counter, int64_t *out, xpa_stream_t stream) {
    if (n <= 0 || n > (1LL << 31) || !out) return (int)hipErrorInvalidValue;
    int h = 1;
    while ((1LL << (2 * h)) < n) ++h;
    hipLaunchKernelGGL(permutation_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, h,
                       seed, counter, out);
    return xpa_launch_status();
}

XPA_API int xpa_random_permutation_batch(int64_t n, int64_t n_agents, const uint32_t *seeds, const uint32_t *counters,
                                         int64_t *out, xpa_stream_t stream) {
    if (n <= 0 || n > (1LL << 31) || n_agents < 1 || n_agents > 65535 || !seeds || !counters || !out)
        return (int)hipErrorInvalidValue;
    int h = 1;
    while ((1LL << (2 * h)) < n) ++h;
    hipLaunchKernelGGL(permutation_batch_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)n_agents), dim3(256), 0,
                       (hipStream_t)stream, n, h, seeds, counters, out);
    return xpa_launch_status();
}

XPA_API int xpa_rollout_policy_head_synthbox(int act, int64_t n_envs, int64_t act_dim, int64_t horizon, int64_t hidden,
                                             int64_t ld, const float *z_actor, const float *z_critic, float slope,
                                             const float *w_actor, const float *b_actor, const float *w_critic,
                                             const float *b_critic, const float *logstd, const xpa_cursor_t *cursor,
                                             uint32_t seed, float act_clip, float *buf_act, float *buf_logp,
                                             float *buf_val, int64_t obs_dim, const float *wcat_t, uint32_t env_seed,
                                             int32_t max_episode_steps, float noise, float term_thresh,
                                             float reset_scale, float *state, int64_t ld_state, float *final_obs,
                                             float *rew, uint8_t *term, uint8_t *trunc, int32_t *ep_step,
                                             uint32_t *ep_index, float *ep_score, float *ep_last_score,
                                             int32_t *ep_last_len, xpa_stream_t stream) {
    if (n_envs <= 0 || act_dim < 1 || act_dim > kRolloutKMax || horizon <= 0 || hidden != 256 || ld < 256 || ld % 4 ||
        act < 0 || act > 2 || !z_actor || !z_critic || !w_actor || !b_actor || !w_critic || !b_critic || !cursor ||
        !logstd || !buf_act || !buf_logp || !buf_val)
        return (int)hipErrorInvalidValue;
    if (((uintptr_t)z_actor | (uintptr_t)z_critic | (uintptr_t)w_actor | (uintptr_t)w_critic) % 16)
        return (int)hipErrorInvalidValue;
    if (obs_dim < 1 || obs_dim > 64 || !wcat_t || !state || ld_state < obs_dim + act_dim || !final_obs || !rew ||
        !term || !trunc || !ep_step || !ep_index || !ep_score || !ep_last_score || !ep_last_len)
        return (int)hipErrorInvalidValue;
    SynthEnvArgs e{(int)obs_dim, env_seed, max_episode_steps, noise, term_thresh, reset_scale, state, ld_state,
                   final_obs, rew, term, trunc, ep_step, ep_index, ep_score, ep_last_score, ep_last_len, wcat_t};
    float *env_in = state + obs_dim;  // the action columns of the env's input rows (s | a)
    const unsigned blocks = (unsigned)((n_envs + 3) / 4);
    hipStream_t s = (hipStream_t)stream;
#define XPA_K14E(A_)                                                                                              \
    hipLaunchKernelGGL((rollout_policy_head_kernel<0, A_, true>), dim3(blocks), dim3(256), 0, s, n_envs,           \
                       (int)act_dim, horizon, z_actor, z_critic, ld, slope, w_actor, b_actor, w_critic, b_critic,     \
                       logstd, cursor, seed, act_clip, buf_act, buf_logp, buf_val, env_in, ld_state, (float *)nullptr, \
                       e)
    if (act == 0) XPA_K14E(0);
    else if (act == 1) XPA_K14E(1);
    else XPA_K14E(2);
#undef XPA_K14E
    return xpa_launch_status();
}

// ---- K14F (r06) ------------------------------------------------------------------------------------
XPA_API int xpa_k14f_probe(int bits) {
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_k14f_probe), &bits, sizeof(int));
}

// Workspace of xpa_rollout_step_synthbox: f64 partials (returned, in doubles) and *n_tickets int32 tickets (zeroed once
// by the caller; every launch leaves them zero).  rms: with the obs_rms update.
XPA_API int64_t xpa_rollout_step_workspace(int64_t n_envs, int64_t obs_dim, int rms, int64_t *n_tickets) {
    if (n_envs <= 0 || obs_dim < 1 || obs_dim > 64 || !n_tickets) return -1;
    const int64_t blocks = (n_envs + 3) / 4, groups = (blocks + kPostGrp - 1) / kPostGrp;
    *n_tickets = (1 + groups) * kTicketStride;
    return (blocks + groups) * (3 + (rms ? 2 * obs_dim : 0));
}

// xpa_rollout_policy_head_synthbox and K8's deferred + normalised post step (xpa_rollout_post_deferred_norm, with
// obs_count non-null also the next step's obs_rms.update: xpa_rollout_post_deferred_norm_rms) in ONE launch (K14F).
// The post arguments mean what they mean there; slot_from_next (A2C's boot_from_reset): kept truncation rows are the
// env's next observation instead of its final one; part / tickets: xpa_rollout_step_workspace.
XPA_API int xpa_rollout_step_synthbox(
    int act, int64_t n_envs, int64_t act_dim, int64_t horizon, int64_t hidden, int64_t ld, const float *z_actor,
    const float *z_critic, float slope, const float *w_actor, const float *b_actor, const float *w_critic,
    const float *b_critic, const float *logstd, xpa_cursor_t *cursor, uint32_t seed, float act_clip, float *buf_act,
    float *buf_logp, float *buf_val, int64_t obs_dim, const float *wcat_t, uint32_t env_seed, int32_t max_episode_steps,
    float noise, float term_thresh, float reset_scale, float *state, int64_t ld_state, float *final_obs, float *rew,
    uint8_t *term, uint8_t *trunc, int32_t *ep_step, uint32_t *ep_index, float *ep_score, float *ep_last_score,
    int32_t *ep_last_len, float *slot_obs, int32_t *slot_t, int64_t n_slots, int32_t *overflow, int slot_from_next,
    float *obs_mean, float *obs_var, double *obs_count, float obs_clip, float *boot_norm, int64_t ld_norm,
    float *ret_mean, float *ret_var, double *ret_count, float *returns, float *buf_rew, float *buf_term,
    uint8_t *buf_closed, float *buf_boot, float gamma, int mask_returns, int use_rewnorm, float rew_range,
    int atari_lifeloss, double *part, int32_t *tickets, xpa_stream_t stream) {
    if (n_envs <= 0 || act_dim < 1 || act_dim > kRolloutKMax || horizon <= 0 || hidden != 256 || ld < 256 || ld % 4 ||
        act < 0 || act > 2 || !z_actor || !z_critic || !w_actor || !b_actor || !w_critic || !b_critic || !cursor ||
        !logstd || !buf_act || !buf_logp || !buf_val)
        return (int)hipErrorInvalidValue;
    if (((uintptr_t)z_actor | (uintptr_t)z_critic | (uintptr_t)w_actor | (uintptr_t)w_critic) % 16)
        return (int)hipErrorInvalidValue;
    if (obs_dim < 1 || obs_dim > 64 || !wcat_t || !state || ld_state < obs_dim + act_dim || !final_obs || !rew ||
        !term || !trunc || !ep_step || !ep_index || !ep_score || !ep_last_score || !ep_last_len)
        return (int)hipErrorInvalidValue;
    if (n_slots < 1 || n_slots > horizon || !slot_obs || !slot_t || !overflow || !obs_mean || !obs_var || !boot_norm ||
        ld_norm < obs_dim || !ret_mean || !ret_var || !ret_count || !returns || !buf_rew || !buf_term || !buf_closed ||
        !buf_boot || !part || !tickets || (n_envs + 3) / 4 > 0x7fffffff)
        return (int)hipErrorInvalidValue;
    SynthEnvArgs e{(int)obs_dim, env_seed, max_episode_steps, noise, term_thresh, reset_scale, state, ld_state,
                   final_obs, rew, term, trunc, ep_step, ep_index, ep_score, ep_last_score, ep_last_len, wcat_t};
    PostArgs pa{cursor, ret_mean, ret_var, ret_count, returns, buf_rew, buf_term, buf_closed, buf_boot, gamma, rew_range,
                obs_clip, mask_returns, use_rewnorm, atari_lifeloss, slot_from_next, (int)n_slots, slot_obs, slot_t,
                overflow, obs_mean, obs_var, obs_count, boot_norm, ld_norm, part, (unsigned *)tickets};
    float *env_in = state + obs_dim;
    const unsigned blocks = (unsigned)((n_envs + 3) / 4);
    hipStream_t s = (hipStream_t)stream;
#define XPA_K14F(A_)                                                                                              \
    hipLaunchKernelGGL((rollout_policy_head_kernel<0, A_, true, true>), dim3(blocks), dim3(256), 0, s, n_envs,     \
                       (int)act_dim, horizon, z_actor, z_critic, ld, slope, w_actor, b_actor, w_critic, b_critic,     \
                       logstd, cursor, seed, act_clip, buf_act, buf_logp, buf_val, env_in, ld_state, (float *)nullptr, \
                       e, pa)
    if (act == 0) XPA_K14F(0);
    else if (act == 1) XPA_K14F(1);
    else XPA_K14F(2);
#undef XPA_K14F
    return xpa_launch_status();
}

// ---- K32 -------------------------------------------------------------------------------------------
XPA_API int64_t xpa_small_rollout_lds_floats(int64_t n_envs, int64_t d_in, int64_t h0, int64_t h1, int64_t h2,
                                             int64_t k) {
    const bool wide = h0 == kRoWide && h1 == kRoWide && h2 == kRoWide;   // K32W
    if (n_envs <= 0 || n_envs > 256 || d_in <= 0 || d_in > 32 || k <= 0 || k > 16 ||
        (!wide && (h0 <= 0 || h0 > 64 || h1 <= 0 || h1 > 64 || h2 <= 0 || h2 > 64)))
        return -1;
    return ro_layout((int)n_envs, (int)d_in, (int)h0, (int)h1, (int)h2, (int)k).total;
}

namespace {
// K32's widths (each of 32, 64) or K32W's (all 128)
bool ro_widths_ok(int64_t h0, int64_t h1, int64_t h2) {
    if (h0 == kRoWide) return h1 == kRoWide && h2 == kRoWide;
    return (h0 == 32 || h0 == 64) && (h1 == 32 || h1 == 64) && (h2 == 32 || h2 == 64);
}

// The one ladder over a checked block's (h0, act_code): launch(ACT, H0), both std::integral_constants, so that the
// callee names its instantiation with decltype(ACT)::value / decltype(H0)::value.  WIDE: the 128-wide column (K32W)
// exists for this kernel; without it h0 is 32 or 64 and no H0 = 128 instantiation is made (K32E).
template <bool WIDE, class F>
void ro_dispatch(int64_t h0, int act_code, F launch) {
    auto by_act = [&](auto H0) {
        if (act_code == 0) launch(std::integral_constant<int, 0>{}, H0);
        else if (act_code == 1) launch(std::integral_constant<int, 1>{}, H0);
        else launch(std::integral_constant<int, 2>{}, H0);
    };
    if constexpr (WIDE) {
        if (h0 == kRoWide) return by_act(std::integral_constant<int, kRoWide>{});
    }
    if (h0 == 64) by_act(std::integral_constant<int, 64>{});
    else by_act(std::integral_constant<int, 32>{});
}

// The checks and the launch shared by K32's entry points; E: the instantiation's env / head pair, k its head width.
// K32E's checks and launch: only what the evaluation form dereferences is required (the training-only pointers of
// XpaSmallRolloutArgs may be null); horizon 1 and the sampler's three stores into scratch [3 * n_envs]
// The predicate is shared by the single-agent launch and the population's (one agent's block and its log / scratch).
// wide: the widths admitted are K32W's (all 128: K32WE) and not K32's (each of 32, 64: K32E); nothing else differs.
template <class E>
bool ro_eval_args_ok_at(bool wide, const XpaSmallRolloutArgs *a0, int k, const int32_t *log, int64_t capacity,
                        int64_t snap_dim, const float *scratch) {
    if (!a0 || !log || capacity <= 0 || capacity > 0x7fffffff || snap_dim < 0 || !scratch || ((uintptr_t)log % 16))
        return false;
    const XpaSmallRolloutArgs &a = *a0;
    const bool widths = wide ? a.h0 == kRoWide && a.h1 == kRoWide && a.h2 == kRoWide
                             : (a.h0 == 32 || a.h0 == 64) && (a.h1 == 32 || a.h1 == 64) && (a.h2 == 32 || a.h2 == 64);
    if (a.n_envs <= 0 || a.n_envs > 256 || a.steps <= 0 || a.d_in != E::D || !widths || a.k != k || a.act_code < 0 ||
        a.act_code > 2 || a.max_episode_steps <= 0 || a.ld_obs < E::D || a.ld_act < k)
        return false;
    if (!a.W0 || !a.b0 || !a.W1 || !a.b1 || !a.W2 || !a.b2 || !a.Wa || !a.ba || !a.Wc || !a.bc || !a.obs_mean ||
        !a.obs_var || !a.obs_count || !a.act_in || !a.env_state || !a.env_obs || !a.final_obs || !a.env_rew ||
        !a.env_term || !a.env_trunc || !a.ep_step || !a.ep_index || !a.ep_score || !a.ep_last_score || !a.ep_last_len ||
        !a.cursor)
        return false;
    const int64_t lf = xpa_small_rollout_lds_floats(a.n_envs, a.d_in, a.h0, a.h1, a.h2, a.k);
    return lf >= 0 && lf <= kRoLdsMax;
}
template <class E>
bool ro_eval_args_ok(const XpaSmallRolloutArgs *a0, int k, const int32_t *log, int64_t capacity, int64_t snap_dim,
                     const float *scratch) {
    return ro_eval_args_ok_at<E>(false, a0, k, log, capacity, snap_dim, scratch);
}

// WIDE: K32WE (the all-128 widths and the ladder's 128-wide column) in place of K32E
template <class E, bool WIDE = false>
int small_eval_launch(const XpaSmallRolloutArgs *a0, int k, typename E::Head hd, int32_t *log, int64_t capacity,
                      int64_t snap_dim, float *scratch, xpa_stream_t stream) {
    if (!ro_eval_args_ok_at<E>(WIDE, a0, k, log, capacity, snap_dim, scratch)) return (int)hipErrorInvalidValue;
    XpaSmallRolloutArgs a = *a0;
    const int64_t lf = xpa_small_rollout_lds_floats(a.n_envs, a.d_in, a.h0, a.h1, a.h2, a.k);
    a.horizon = 1;
    a.buf_act = scratch;
    a.buf_logp = scratch + a.n_envs;
    a.buf_val = scratch + 2 * a.n_envs;
    a.stamps = nullptr;
    const RoEval ev{log, capacity, eval_log_entries(snap_dim)};
    const size_t bytes = (size_t)lf * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    ro_dispatch<WIDE>(a.h0, a.act_code, [&](auto ACT, auto H0) {
        hipLaunchKernelGGL((small_rollout_kernel<E, decltype(ACT)::value, decltype(H0)::value, true>), dim3(1),
                           dim3(kRoThreads), bytes, s, a, hd, ev);
    });
    return xpa_launch_status();
}

// The argument checks of K32's training form (one agent's block)
template <class E>
bool ro_train_args_ok(const XpaSmallRolloutArgs *a, int k) {
    if (!a || a->n_envs <= 0 || a->n_envs > 256 || a->horizon <= 0 || a->steps <= 0 || a->d_in != E::D ||
        !ro_widths_ok(a->h0, a->h1, a->h2) || a->k != k ||
        a->act_code < 0 || a->act_code > 2 || a->n_slots < 1 || a->n_slots > a->horizon || a->max_episode_steps <= 0 ||
        a->ld_norm < a->d_in || a->ld_obs < E::D || a->ld_act < k || a->ld_boot < a->d_in)
        return false;
    if (!a->W0 || !a->b0 || !a->W1 || !a->b1 || !a->W2 || !a->b2 || !a->Wa || !a->ba || !a->Wc || !a->bc ||
        !a->obs_mean || !a->obs_var || !a->obs_count || !a->obs_norm || !a->buf_obs || !a->buf_act || !a->buf_logp ||
        !a->buf_val || !a->buf_rew || !a->buf_term || !a->buf_closed || !a->buf_boot || !a->act_in || !a->env_state ||
        !a->env_obs || !a->final_obs || !a->env_rew || !a->env_term || !a->env_trunc || !a->ep_step || !a->ep_index ||
        !a->ep_score || !a->ep_last_score || !a->ep_last_len || !a->returns || !a->ret_mean || !a->ret_var ||
        !a->ret_count || !a->slot_obs || !a->slot_t || !a->overflow || !a->boot_norm || !a->cursor)
        return false;
    const int64_t lf = xpa_small_rollout_lds_floats(a->n_envs, a->d_in, a->h0, a->h1, a->h2, a->k);
    return lf >= 0 && lf <= kRoLdsMax;
}

template <class E>
int small_rollout_launch(const XpaSmallRolloutArgs *a, int k, typename E::Head hd, xpa_stream_t stream) {
    if (!ro_train_args_ok<E>(a, k)) return (int)hipErrorInvalidValue;
    const int64_t lf = xpa_small_rollout_lds_floats(a->n_envs, a->d_in, a->h0, a->h1, a->h2, a->k);
    const size_t bytes = (size_t)lf * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    ro_dispatch<true>(a->h0, a->act_code, [&](auto ACT, auto H0) {
        hipLaunchKernelGGL((small_rollout_kernel<E, decltype(ACT)::value, decltype(H0)::value>), dim3(1),
                           dim3(kRoThreads), bytes, s, *a, hd, RoNoEval{});
    });
    return xpa_launch_status();
}

// Every non-pointer field but seed / env_seed: what one instantiation, one LDS carve and one launch shape share
bool ro_same_shape(const XpaSmallRolloutArgs &x, const XpaSmallRolloutArgs &y) {
    return x.n_envs == y.n_envs && x.horizon == y.horizon && x.steps == y.steps && x.d_in == y.d_in && x.h0 == y.h0 &&
           x.h1 == y.h1 && x.h2 == y.h2 && x.k == y.k && x.act_code == y.act_code && x.use_obsnorm == y.use_obsnorm &&
           x.n_slots == y.n_slots && x.mask_returns == y.mask_returns && x.use_rewnorm == y.use_rewnorm &&
           x.max_episode_steps == y.max_episode_steps && x.slot_reset_obs == y.slot_reset_obs && x.slope == y.slope &&
           x.obs_clip == y.obs_clip && x.gamma == y.gamma && x.rew_range == y.rew_range && x.ld_norm == y.ld_norm &&
           x.ld_act == y.ld_act && x.ld_obs == y.ld_obs && x.ld_boot == y.ld_boot;
}

// xpa_small_rollout_batch for one env / head pair: every check on the host copies before any HIP call, the
// instantiation from block 0, one workgroup per agent
template <class E>
int small_rollout_batch_launch(int64_t n_agents, const XpaSmallRolloutArgs *host, const XpaSmallRolloutArgs *dev,
                               int k, const XpaSmallRolloutHead *host_heads, const XpaSmallRolloutHead *dev_heads,
                               xpa_stream_t stream) {
    constexpr bool kHead = !std::is_empty_v<typename E::Head>;
    if (n_agents < 1 || n_agents > 0x7fffffff || !host || !dev || (kHead && (!host_heads || !dev_heads)))
        return (int)hipErrorInvalidValue;
    for (int64_t p = 0; p < n_agents; ++p) {
        if (!ro_train_args_ok<E>(host + p, k) || !ro_same_shape(host[p], host[0])) return (int)hipErrorInvalidValue;
        if (kHead && (!host_heads[p].logstd || !(host_heads[p].act_clip > 0.f))) return (int)hipErrorInvalidValue;
    }
    const XpaSmallRolloutArgs *a = host;
    const int64_t lf = xpa_small_rollout_lds_floats(a->n_envs, a->d_in, a->h0, a->h1, a->h2, a->k);
    const size_t bytes = (size_t)lf * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    ro_dispatch<true>(a->h0, a->act_code, [&](auto ACT, auto H0) {
        hipLaunchKernelGGL((small_rollout_batch_kernel<E, decltype(ACT)::value, decltype(H0)::value>),
                           dim3((unsigned)n_agents), dim3(kRoThreads), bytes, s, dev, dev_heads);
    });
    return xpa_launch_status();
}

// The non-pointer fields the evaluation form reads (seed apart): one instantiation, one LDS carve, one step count
bool ro_eval_same_shape(const XpaSmallRolloutArgs &x, const XpaSmallRolloutArgs &y) {
    return x.n_envs == y.n_envs && x.steps == y.steps && x.d_in == y.d_in && x.h0 == y.h0 && x.h1 == y.h1 &&
           x.h2 == y.h2 && x.k == y.k && x.act_code == y.act_code && x.use_obsnorm == y.use_obsnorm &&
           x.max_episode_steps == y.max_episode_steps && x.slope == y.slope && x.obs_clip == y.obs_clip &&
           x.ld_obs == y.ld_obs && x.ld_act == y.ld_act;
}

// xpa_small_eval_batch for one env / head pair: every check on the host copies before any HIP call, the
// instantiation (K32E's widths only; WIDE: K32WEB, K32W's only) and the LDS size from block 0, one workgroup per agent
template <class E, bool WIDE = false>
int small_eval_batch_launch(int64_t n_agents, const XpaSmallRolloutArgs *host, const XpaSmallRolloutArgs *dev, int k,
                            const XpaSmallRolloutHead *host_heads, const XpaSmallRolloutHead *dev_heads,
                            const XpaSmallEval *host_evals, const XpaSmallEval *dev_evals, xpa_stream_t stream) {
    constexpr bool kHead = !std::is_empty_v<typename E::Head>;
    if (n_agents < 1 || n_agents > 0x7fffffff || !host || !dev || !host_evals || !dev_evals ||
        (host_heads != nullptr) != kHead || (dev_heads != nullptr) != kHead)
        return (int)hipErrorInvalidValue;
    std::vector<uintptr_t> logs, scratches;
    for (int64_t p = 0; p < n_agents; ++p) {
        const XpaSmallEval &e = host_evals[p];
        if (!ro_eval_args_ok_at<E>(WIDE, host + p, k, e.log, e.capacity, e.snap_dim, e.scratch) ||
            !ro_eval_same_shape(host[p], host[0]) || e.capacity != host_evals[0].capacity ||
            e.snap_dim != host_evals[0].snap_dim)
            return (int)hipErrorInvalidValue;
        if (kHead && (!host_heads[p].logstd || !(host_heads[p].act_clip > 0.f))) return (int)hipErrorInvalidValue;
        logs.push_back((uintptr_t)e.log);
        scratches.push_back((uintptr_t)e.scratch);
    }
    for (auto *v : {&logs, &scratches}) {   // no two members share a log or a scratch
        std::sort(v->begin(), v->end());
        if (std::adjacent_find(v->begin(), v->end()) != v->end()) return (int)hipErrorInvalidValue;
    }
    const XpaSmallRolloutArgs *a = host;
    const int64_t lf = xpa_small_rollout_lds_floats(a->n_envs, a->d_in, a->h0, a->h1, a->h2, a->k);
    const size_t bytes = (size_t)lf * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    ro_dispatch<WIDE>(a->h0, a->act_code, [&](auto ACT, auto H0) {
        hipLaunchKernelGGL((small_eval_batch_kernel<E, decltype(ACT)::value, decltype(H0)::value>),
                           dim3((unsigned)n_agents), dim3(kRoThreads), bytes, s, dev, dev_heads, dev_evals);
    });
    return xpa_launch_status();
}
}  // namespace

XPA_API int xpa_small_rollout_cartpole(const XpaSmallRolloutArgs *a, xpa_stream_t stream) {
    return small_rollout_launch<RoCartPoleCat>(a, 2, RoCartPoleCat::Head{}, stream);
}

XPA_API int xpa_small_rollout_pendulum(const XpaSmallRolloutArgs *a, const float *logstd, float act_clip,
                                       xpa_stream_t stream) {
    if (!logstd || !(act_clip > 0.f)) return (int)hipErrorInvalidValue;
    return small_rollout_launch<RoPendulumGauss>(a, 1, RoPendulumGauss::Head{logstd, act_clip}, stream);
}

XPA_API int xpa_small_rollout_acrobot(const XpaSmallRolloutArgs *a, xpa_stream_t stream) {
    return small_rollout_launch<RoAcrobotCat>(a, 3, RoAcrobotCat::Head{}, stream);
}

XPA_API int xpa_small_rollout_mountaincar(const XpaSmallRolloutArgs *a, xpa_stream_t stream) {
    return small_rollout_launch<RoMountainCarCat>(a, 3, RoMountainCarCat::Head{}, stream);
}

XPA_API int xpa_small_rollout_batch(int env, int64_t n_agents, const XpaSmallRolloutArgs *host_blocks,
                                    const XpaSmallRolloutArgs *dev_blocks, const XpaSmallRolloutHead *host_heads,
                                    const XpaSmallRolloutHead *dev_heads, xpa_stream_t stream) {
    switch (env) {
    case XPA_ENV_CARTPOLE:
        return small_rollout_batch_launch<RoCartPoleCat>(n_agents, host_blocks, dev_blocks, 2, host_heads, dev_heads,
                                                         stream);
    case XPA_ENV_PENDULUM:
        return small_rollout_batch_launch<RoPendulumGauss>(n_agents, host_blocks, dev_blocks, 1, host_heads, dev_heads,
                                                           stream);
    case XPA_ENV_ACROBOT:
        return small_rollout_batch_launch<RoAcrobotCat>(n_agents, host_blocks, dev_blocks, 3, host_heads, dev_heads,
                                                        stream);
    case XPA_ENV_MOUNTAINCAR:
        return small_rollout_batch_launch<RoMountainCarCat>(n_agents, host_blocks, dev_blocks, 3, host_heads,
                                                            dev_heads, stream);
    default:
        return (int)hipErrorInvalidValue;
    }
}

// ---- K33 -------------------------------------------------------------------------------------------
namespace {
// The argument checks of one agent's closing block (host only: no HIP call)
bool ro_close_args_ok(const XpaSmallCloseArgs *a) {
    if (!a || a->n_envs <= 0 || a->n_envs > 256 || a->horizon <= 0 || a->d_in < 1 || a->d_in > 8 ||
        !ro_widths_ok(a->h0, a->h1, a->h2) || a->k < 1 || a->k > 3 || a->act_code < 0 || a->act_code > 2 ||
        a->n_slots < 1 || a->n_slots > a->horizon || a->ld_rows < a->d_in)
        return false;
    if (!a->W0 || !a->b0 || !a->W1 || !a->b1 || !a->W2 || !a->b2 || !a->Wa || !a->ba || !a->Wc || !a->bc || !a->rows ||
        !a->slot_t || !a->rew || !a->val || !a->term || !a->closed || !a->boot || !a->adv || !a->ret)
        return false;
    const int64_t lf = xpa_small_rollout_lds_floats(a->n_envs, a->d_in, a->h0, a->h1, a->h2, a->k);
    return lf >= 0 && lf <= kRoLdsMax;
}

// Every non-pointer field: what one instantiation, one LDS carve and one set of scalars share
bool ro_close_same_shape(const XpaSmallCloseArgs &x, const XpaSmallCloseArgs &y) {
    return x.n_envs == y.n_envs && x.horizon == y.horizon && x.d_in == y.d_in && x.h0 == y.h0 && x.h1 == y.h1 &&
           x.h2 == y.h2 && x.k == y.k && x.act_code == y.act_code && x.n_slots == y.n_slots &&
           x.use_gae == y.use_gae && x.slope == y.slope && x.gamma == y.gamma && x.gae_lambda == y.gae_lambda &&
           x.ld_rows == y.ld_rows;
}

// one: the single agent's block (by value); else n_agents blocks in device memory.  a: the (first) host block, checked.
int small_close_launch(const XpaSmallCloseArgs *a, int64_t n_agents, const XpaSmallCloseArgs *dev, bool one,
                       xpa_stream_t stream) {
    const int64_t lf = xpa_small_rollout_lds_floats(a->n_envs, a->d_in, a->h0, a->h1, a->h2, a->k);
    const size_t bytes = (size_t)lf * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    ro_dispatch<true>(a->h0, a->act_code, [&](auto ACT, auto H0) {
        constexpr int A = decltype(ACT)::value, H = decltype(H0)::value;
        if (one)
            hipLaunchKernelGGL((small_close_kernel<A, H>), dim3(1), dim3(kRoThreads), bytes, s, *a);
        else
            hipLaunchKernelGGL((small_close_batch_kernel<A, H>), dim3((unsigned)n_agents), dim3(kRoThreads), bytes, s,
                               dev);
    });
    return xpa_launch_status();
}
}  // namespace

XPA_API int xpa_small_close(const XpaSmallCloseArgs *a, xpa_stream_t stream) {
    if (!ro_close_args_ok(a)) return (int)hipErrorInvalidValue;
    return small_close_launch(a, 1, nullptr, true, stream);
}

XPA_API int xpa_small_close_batch(int64_t n_agents, const XpaSmallCloseArgs *host_blocks,
                                  const XpaSmallCloseArgs *dev_blocks, xpa_stream_t stream) {
    if (n_agents < 1 || n_agents > 65535 || !host_blocks || !dev_blocks) return (int)hipErrorInvalidValue;
    for (int64_t p = 0; p < n_agents; ++p)
        if (!ro_close_args_ok(host_blocks + p) || !ro_close_same_shape(host_blocks[p], host_blocks[0]))
            return (int)hipErrorInvalidValue;
    return small_close_launch(host_blocks, n_agents, dev_blocks, false, stream);
}

// ---- device evaluation: K32E and the generic tier's per-step log writer ---------------------------------------------
XPA_API int64_t xpa_eval_log_ints(int64_t capacity, int64_t snap_dim) {
    if (capacity <= 0 || capacity > 0x7fffffff || snap_dim < 0) return -1;
    return eval_log_entries(snap_dim) + 4 * capacity;
}

XPA_API int xpa_small_eval_cartpole(const XpaSmallRolloutArgs *a, int32_t *log, int64_t capacity, int64_t snap_dim,
                                    float *scratch, xpa_stream_t stream) {
    return small_eval_launch<RoCartPoleCat>(a, 2, RoCartPoleCat::Head{}, log, capacity, snap_dim, scratch, stream);
}

XPA_API int xpa_small_eval_pendulum(const XpaSmallRolloutArgs *a, const float *logstd, float act_clip, int32_t *log,
                                    int64_t capacity, int64_t snap_dim, float *scratch, xpa_stream_t stream) {
    if (!logstd || !(act_clip > 0.f)) return (int)hipErrorInvalidValue;
    return small_eval_launch<RoPendulumGauss>(a, 1, RoPendulumGauss::Head{logstd, act_clip}, log, capacity, snap_dim,
                                              scratch, stream);
}

XPA_API int xpa_small_eval_acrobot(const XpaSmallRolloutArgs *a, int32_t *log, int64_t capacity, int64_t snap_dim,
                                   float *scratch, xpa_stream_t stream) {
    return small_eval_launch<RoAcrobotCat>(a, 3, RoAcrobotCat::Head{}, log, capacity, snap_dim, scratch, stream);
}

XPA_API int xpa_small_eval_mountaincar(const XpaSmallRolloutArgs *a, int32_t *log, int64_t capacity, int64_t snap_dim,
                                       float *scratch, xpa_stream_t stream) {
    return small_eval_launch<RoMountainCarCat>(a, 3, RoMountainCarCat::Head{}, log, capacity, snap_dim, scratch,
                                               stream);
}

XPA_API int xpa_small_eval_batch(int env, int64_t n_agents, const XpaSmallRolloutArgs *host_blocks,
                                 const XpaSmallRolloutArgs *dev_blocks, const XpaSmallRolloutHead *host_heads,
                                 const XpaSmallRolloutHead *dev_heads, const XpaSmallEval *host_evals,
                                 const XpaSmallEval *dev_evals, xpa_stream_t stream) {
    switch (env) {
    case XPA_ENV_CARTPOLE:
        return small_eval_batch_launch<RoCartPoleCat>(n_agents, host_blocks, dev_blocks, 2, host_heads, dev_heads,
                                                      host_evals, dev_evals, stream);
    case XPA_ENV_PENDULUM:
        return small_eval_batch_launch<RoPendulumGauss>(n_agents, host_blocks, dev_blocks, 1, host_heads, dev_heads,
                                                        host_evals, dev_evals, stream);
    case XPA_ENV_ACROBOT:
        return small_eval_batch_launch<RoAcrobotCat>(n_agents, host_blocks, dev_blocks, 3, host_heads, dev_heads,
                                                     host_evals, dev_evals, stream);
    case XPA_ENV_MOUNTAINCAR:
        return small_eval_batch_launch<RoMountainCarCat>(n_agents, host_blocks, dev_blocks, 3, host_heads, dev_heads,
                                                         host_evals, dev_evals, stream);
    default:
        return (int)hipErrorInvalidValue;
    }
}

// ---- K32WE / K32WEB and the batched test-env reset ------------------------------------------------------------------
namespace {
// f(E{}, k) for the env code's env / head pair and its head width; an unknown code is an error before any HIP call
template <class F>
int ro_by_env(int env, F f) {
    switch (env) {
    case XPA_ENV_CARTPOLE:
        return f(RoCartPoleCat{}, 2);
    case XPA_ENV_PENDULUM:
        return f(RoPendulumGauss{}, 1);
    case XPA_ENV_ACROBOT:
        return f(RoAcrobotCat{}, 3);
    case XPA_ENV_MOUNTAINCAR:
        return f(RoMountainCarCat{}, 3);
    default:
        return (int)hipErrorInvalidValue;
    }
}

// xpa_small_env_reset_batch for one env: the checks on the host copies, then one workgroup per agent
template <class E>
int small_env_reset_batch_launch(int64_t n_agents, const XpaSmallRolloutArgs *host, const XpaSmallRolloutArgs *dev,
                                 int k, xpa_stream_t stream) {
    if (n_agents < 1 || n_agents > 0x7fffffff || !host || !dev) return (int)hipErrorInvalidValue;
    std::vector<uintptr_t> states;
    for (int64_t p = 0; p < n_agents; ++p) {
        const XpaSmallRolloutArgs &a = host[p];
        if (a.n_envs < 1 || a.n_envs > 256 || a.n_envs != host[0].n_envs || a.d_in != E::D || a.k != k ||
            a.ld_obs < E::D || a.ld_act < k)
            return (int)hipErrorInvalidValue;
        if (!a.act_in || !a.env_state || !a.env_obs || !a.env_rew || !a.env_term || !a.env_trunc || !a.ep_step ||
            !a.ep_index || !a.ep_score || !a.ep_last_score || !a.ep_last_len)
            return (int)hipErrorInvalidValue;
        states.push_back((uintptr_t)a.env_state);
    }
    std::sort(states.begin(), states.end());   // no two members share an env set
    if (std::adjacent_find(states.begin(), states.end()) != states.end()) return (int)hipErrorInvalidValue;
    constexpr bool kZeroAct = !std::is_same_v<E, RoCartPoleCat>;
    hipLaunchKernelGGL((small_env_reset_batch_kernel<E, kZeroAct>), dim3((unsigned)n_agents), dim3(kRoThreads), 0,
                       (hipStream_t)stream, dev);
    return xpa_launch_status();
}
}  // namespace

XPA_API int xpa_small_eval_wide(int env, const XpaSmallRolloutArgs *a, const XpaSmallRolloutHead *head, int32_t *log,
                                int64_t capacity, int64_t snap_dim, float *scratch, xpa_stream_t stream) {
    return ro_by_env(env, [&](auto e, int k) {
        using E = decltype(e);
        typename E::Head hd{};
        if constexpr (std::is_empty_v<typename E::Head>) {
            if (head) return (int)hipErrorInvalidValue;
        } else {
            if (!head || !head->logstd || !(head->act_clip > 0.f)) return (int)hipErrorInvalidValue;
            hd = typename E::Head{head->logstd, head->act_clip};
        }
        return small_eval_launch<E, true>(a, k, hd, log, capacity, snap_dim, scratch, stream);
    });
}

XPA_API int xpa_small_eval_wide_batch(int env, int64_t n_agents, const XpaSmallRolloutArgs *host_blocks,
                                      const XpaSmallRolloutArgs *dev_blocks, const XpaSmallRolloutHead *host_heads,
                                      const XpaSmallRolloutHead *dev_heads, const XpaSmallEval *host_evals,
                                      const XpaSmallEval *dev_evals, xpa_stream_t stream) {
    return ro_by_env(env, [&](auto e, int k) {
        return small_eval_batch_launch<decltype(e), true>(n_agents, host_blocks, dev_blocks, k, host_heads, dev_heads,
                                                          host_evals, dev_evals, stream);
    });
}

XPA_API int xpa_small_env_reset_batch(int env, int64_t n_agents, const XpaSmallRolloutArgs *host_blocks,
                                      const XpaSmallRolloutArgs *dev_blocks, xpa_stream_t stream) {
    return ro_by_env(env, [&](auto e, int k) {
        return small_env_reset_batch_launch<decltype(e)>(n_agents, host_blocks, dev_blocks, k, stream);
    });
}

XPA_API int xpa_eval_post(int32_t *log, int64_t capacity, int64_t snap_dim, int64_t n_envs, const uint8_t *term,
                          const uint8_t *trunc, const float *ep_last_score, const int32_t *ep_last_len,
                          int atari_lifeloss, xpa_cursor_t *cursor, const float *obs_mean, const float *obs_var,
                          const double *obs_count, xpa_stream_t stream) {
    if (!log || ((uintptr_t)log % 16) || capacity <= 0 || capacity > 0x7fffffff || snap_dim < 0 || n_envs <= 0 ||
        n_envs > 0x7fffffff || !term || !trunc || !ep_last_score || !ep_last_len || !cursor)
        return (int)hipErrorInvalidValue;
    if ((obs_count != nullptr) != (obs_mean != nullptr) || (obs_count != nullptr) != (obs_var != nullptr))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(eval_post_kernel, dim3(1), dim3(kEvalThreads), 0, (hipStream_t)stream, log, capacity,
                       eval_log_entries(snap_dim), n_envs, term, trunc, ep_last_score, ep_last_len, atari_lifeloss,
                       cursor, obs_mean, obs_var, obs_count, snap_dim);
    return xpa_launch_status();
}
