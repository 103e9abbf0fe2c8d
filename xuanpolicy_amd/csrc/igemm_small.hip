// K28R — the conv forward of small batches on the bf16 matrix cores (the rollout's and the Q-learner's forwards of
// the later conv blocks of AC_CNN_Atari C3 / Basic_CNN C5: cnn_block xuance/torch/utils/layers.py:27-57,
// xuance/torch/representations/cnn.py:5-93), the row counts K28 (igemm.hip) leaves to the library: one 1024-thread
// block per CU that stages the whole f32 weight image before its first MFMA has nothing to overlap when a launch
// holds less than one 512-row step per CU.
//
//   y[m, n] = act(sum_{tap, c} x[pixel(m, tap), c] W[n, c, tap] + b[n])   over the output pixels m = (b, oy, ox)
//
// K28's pixel map, activation codes and NHWC output; K28B's arithmetic: both operands in the exact three-way bf16
// split (s3_split.h), six v_mfma_f32_32x32x16_bf16 products per 16-k step (xpa_mfma_s3), so the f32 GEMM's accuracy.
// What differs is where the work sits:
//   weights   split ONCE per weight version by xpa_conv_wsplit into three bf16 planes in HBM, in the B fragment's own
//             order: [tap][16-channel step j][plane][lane half h][n < 32 NT][8 channels 16 j + 8 h ..+7].  One tap of
//             all planes is one contiguous run of CIN / 16 x NT x 3 KiB (24 KiB at 64 -> 64 channels); a lane's
//             fragment is one 16-B LDS read, 16 consecutive lanes read 256 consecutive bytes.  The main kernel does
//             no split work on B.
//   B ring    two tap stages in LDS, filled by LDS-DMA (global_load_lds_dwordx4, the copies of K40's ring in
//             sgemm3.hip), 1 KiB pieces dealt round-robin to the block's 4 waves.  Tap t + 1 is requested right after
//             the one barrier of tap t, ahead of tap t's MFMAs.
//   rows      block = 256 threads = 4 waves (one per SIMD) = 4 x 32 rows x 32 NT columns, grid = ceil(rows / 128), not
//             persistent: at most 48 KiB of LDS per block, so three blocks share a CU and one block's staging, barrier
//             and epilogue overlap another's MFMAs.
//   A         as K28B: lane (h, i) owns row i of its wave's tile and channels 16 j + 8 h ..+7 of a step: two 16-B
//             range-checked buffer loads from the pixel's NHWC address (padding taps and ragged rows: an offset past
//             the record, zeros from the hardware, no select), split in registers, a register ring one step ahead.
// k order: taps ascending, then channel steps, xpa_mfma_s3's product order inside a step; no atomics, no grid-wide
// synchronisation: two launches give the same bits, and a row's value depends neither on the batch size nor on where
// the row falls in a tile.
//
// This file is compiled without the packed-f32 VALU forms (_lib.EXTRA_FLAGS).
#include "xpa_common.h"
#include "s3_split.h"

namespace {

typedef float f4v __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) char lds_char_t;

constexpr int kSmWaves = 4;                  // one per SIMD
constexpr int kSmRows = 32 * kSmWaves;       // rows per block
constexpr int kSmStages = 2;                 // tap stages of the B ring
constexpr int kSmPiece = 1024;               // bytes one wave's LDS-DMA instruction moves

// bytes of one tap of the three planes: [CIN / 16][3][2][32 nt][8] bf16
constexpr int64_t sm_tap_bytes(int64_t cin, int64_t nt) { return cin / 16 * nt * 3 * kSmPiece; }

bool sm_shape(int64_t cin, int64_t cout, int64_t k, int &nt) {
    if ((cin != 16 && cin != 32 && cin != 64) || cout < 1 || cout > 64 || k < 1 || k > 12) return false;
    nt = cout <= 32 ? 1 : 2;
    return true;
}

template <int ACT>
__device__ __forceinline__ float sm_act(float z, float slope) {   // K28's codes
    if (ACT == 1) return z > 0.f ? z : z * slope;
    if (ACT == 2) return tanhf(z);
    return z;
}

__device__ __forceinline__ void sm_glds16(const void *g, unsigned lds_wave_base) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(g), "s"(lds_wave_base)
                 : "memory", "m0");
}

// ---- W [out][in][k][k] (f32) -> the three planes --------------------------------------------------------------------
// one thread per (tap, step j, half h, column n < 32 nt): its 8 channels split, columns n >= out_c zero
__global__ __launch_bounds__(256) void conv_wsplit_kernel(const float *__restrict__ w, int cin, int cout, int k, int nt,
                                                          __bf16 *__restrict__ out) {
    const int coutp = 32 * nt, spt = cin / 16, taps = k * k;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= taps * spt * 2 * coutp) return;
    const int n = e % coutp, h = (e / coutp) & 1, j = (e / (2 * coutp)) % spt, tap = e / (2 * coutp * spt);
    xpa_bf16x8 ph, pm, pl;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float x = n < cout ? w[((int64_t)n * cin + 16 * j + 8 * h + c) * taps + tap] : 0.f;
        __bf16 a0, a1, a2;
        xpa_split3(x, a0, a1, a2);
        ph[c] = a0;
        pm[c] = a1;
        pl[c] = a2;
    }
    xpa_bf16x8 *o = reinterpret_cast<xpa_bf16x8 *>(out) + ((int64_t)(tap * spt + j) * 3 * 2 + h) * coutp + n;
    o[0] = ph;
    o[2 * coutp] = pm;
    o[4 * coutp] = pl;
}

struct SmArgs {
    const float *in;       // NHWC [B, IH, IW, CIN]
    int64_t in_bytes;      // < 2^31: the loads use 32-bit buffer offsets
    const char *planes;    // xpa_conv_wsplit's output
    const float *bias;     // [COUT] (nullable)
    float *out;            // NHWC [B, OH, OW, COUT]
    int64_t rows;          // B * OH * OW
    int IH, IW, OH, OW, COUT, K, S, P;
    float slope;
};

template <int CIN, int NT, int ACT>
__global__ __launch_bounds__(64 * kSmWaves) void conv_small_kernel(SmArgs a) {
    constexpr int SPT = CIN / 16;                        // 16-channel steps per tap
    constexpr int COUTP = 32 * NT;
    constexpr int STAGE = (int)sm_tap_bytes(CIN, NT);    // one tap of the three planes
    constexpr int PIECES = STAGE / kSmPiece;
    // ONE LDS array, the DMA's target (its address reaches the copies' asm, whose memory clobber orders the reads)
    __shared__ __attribute__((aligned(16))) char lds[kSmStages * STAGE];
    const unsigned base = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(lds_char_t *)lds);
    const int t = threadIdx.x, lane = t & 63, h = lane >> 5, i = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int taps = a.K * a.K;
    // this lane's row: output pixel (b, oy, ox) -> the top-left input pixel of its window
    const int64_t m = (int64_t)blockIdx.x * kSmRows + wave * 32 + i;
    const bool ok = m < a.rows;
    const int64_t mc = ok ? m : 0, ohw = (int64_t)a.OH * a.OW;
    const int64_t b = mc / ohw;
    const int rem = (int)(mc - b * ohw);
    const int oy = rem / a.OW, ox = rem - oy * a.OW;
    const int pbase = (int)(b * a.IH * a.IW), iy0 = oy * a.S - a.P, ix0 = ox * a.S - a.P;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(a.in), 0, (int)a.in_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rout = __builtin_amdgcn_make_buffer_rsrc(a.out, 0, (int)(a.rows * a.COUT * 4),
                                                                          0x00020000);
    // tap `tap` of the planes -> its ring stage: the wave's share of the 1 KiB pieces (piece p: lane l's 16 B)
    auto issue_tap = [&](int tap) {
        const char *src = a.planes + (int64_t)tap * STAGE + lane * 16;
        const unsigned st = base + (unsigned)((tap & (kSmStages - 1)) * STAGE);
#pragma unroll
        for (int u = 0; u < (PIECES + kSmWaves - 1) / kSmWaves; ++u) {
            const int p = wave + kSmWaves * u;
            if (p < PIECES) sm_glds16(src + p * kSmPiece, st + (unsigned)(p * kSmPiece));
        }
    };
    // the lane's 8 channels of step j of tap (ky, kx): a padding tap or a ragged row reads past the record (zeros)
    auto load_step = [&](f4v (&v)[2], int ky, int kx, int j) {
        const int iy = iy0 + ky, ix = ix0 + kx;
        const bool valid = ok && (unsigned)iy < (unsigned)a.IH && (unsigned)ix < (unsigned)a.IW;
        const int off = ((pbase + iy * a.IW + ix) * CIN + 16 * j + 8 * h) * 4;
#pragma unroll
        for (int q = 0; q < 2; ++q)
            v[q] = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rsrc, valid ? off + 16 * q : INT32_MIN,
                                                                                 0, 0));
    };
    float bn[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) bn[nt] = a.bias && 32 * nt + i < a.COUT ? a.bias[32 * nt + i] : 0.f;
    xpa_f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;
    issue_tap(0);
    f4v va[2], vb[2];
    load_step(va, 0, 0, 0);
    int ky = 0, kx = 0;   // the tap of the loop below
#pragma unroll 1
    for (int tap = 0; tap < taps; ++tap) {
        // the one barrier of a tap: this wave's pieces of tap `tap` (and its A step, requested one step ago) have
        // landed, then every wave's; and every wave is past tap - 1's MFMAs, whose stage tap + 1 refills
        // (va passes through the asm so the compiler counts it as landed: left to its own count, which misses the
        // DMAs, its wait for va after the requests below would drain all but three of tap + 1's pieces)
        asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" : "+v"(va[0]), "+v"(va[1])::"memory");
        const bool more = tap + 1 < taps;
        if (more) issue_tap(tap + 1);
        const char *sb = lds + (tap & (kSmStages - 1)) * STAGE;
        int nky = ky, nkx = kx + 1;
        if (nkx == a.K) {
            nkx = 0;
            ++nky;
        }
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
            // step + 1 requested before this step's MFMAs
            if (j + 1 < SPT) load_step(vb, ky, kx, j + 1);
            else if (more) load_step(vb, nky, nkx, 0);
            __builtin_amdgcn_sched_barrier(0);
            xpa_bf16x8 ah, am, al;
            xpa_split8(float4{va[0][0], va[0][1], va[0][2], va[0][3]}, float4{va[1][0], va[1][1], va[1][2], va[1][3]},
                       ah, am, al);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const xpa_bf16x8 *bp = reinterpret_cast<const xpa_bf16x8 *>(sb) + (j * 3 * 2 + h) * COUTP + 32 * nt + i;
                acc[nt] = xpa_mfma_s3(ah, am, al, bp[0], bp[2 * COUTP], bp[4 * COUTP], acc[nt]);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                va[q] = vb[q];
                asm volatile("" ::"v"(va[q]));
            }
        }
        ky = nky;
        kx = nkx;
    }
    // K28's epilogue (C/D map: row = (r & 3) + 8 (r >> 2) + 4 h of the wave's tile, column n = 32 nt + i): branch-free
    // buffer stores, ragged rows and padded columns past the record
    const int64_t m0 = (int64_t)blockIdx.x * kSmRows + wave * 32 + 4 * h;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int n = 32 * nt + i;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t mr = m0 + (r & 3) + 8 * (r >> 2);
            const int o = mr < a.rows && n < a.COUT ? (int)(mr * a.COUT + n) * 4 : INT32_MIN;
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, sm_act<ACT>(acc[nt][r] + bn[nt], a.slope)),
                                                  rout, o, 0, 0);
        }
    }
}

template <int ACT>
int sm_dispatch(const SmArgs &a, int cin, int nt, hipStream_t s) {
    const dim3 grid((unsigned)((a.rows + kSmRows - 1) / kSmRows)), block(64 * kSmWaves);
#define XPA_SM(C_, N_) hipLaunchKernelGGL((conv_small_kernel<C_, N_, ACT>), grid, block, 0, s, a)
    if (nt == 1) {
        if (cin == 16) XPA_SM(16, 1); else if (cin == 32) XPA_SM(32, 1); else XPA_SM(64, 1);
    } else {
        if (cin == 16) XPA_SM(16, 2); else if (cin == 32) XPA_SM(32, 2); else XPA_SM(64, 2);
    }
#undef XPA_SM
    return xpa_launch_status();
}

}  // namespace

XPA_API int xpa_conv_small_ok(int64_t in_c, int64_t out_c, int64_t kernel) {
    int nt;
    return sm_shape(in_c, out_c, kernel, nt) ? 1 : 0;
}

XPA_API int64_t xpa_conv_wsplit_bytes(int64_t in_c, int64_t out_c, int64_t kernel) {
    int nt;
    return sm_shape(in_c, out_c, kernel, nt) ? kernel * kernel * sm_tap_bytes(in_c, nt) : 0;
}

XPA_API int xpa_conv_wsplit(const float *w, int64_t in_c, int64_t out_c, int64_t kernel, void *planes,
                            xpa_stream_t stream) {
    int nt;
    if (!w || !planes || ((uintptr_t)planes % 16) || !sm_shape(in_c, out_c, kernel, nt)) return (int)hipErrorInvalidValue;
    const int64_t n = kernel * kernel * (in_c / 16) * 2 * 32 * nt;   // <= 144 x 4 x 128 threads
    hipLaunchKernelGGL(conv_wsplit_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w,
                       (int)in_c, (int)out_c, (int)kernel, nt, reinterpret_cast<__bf16 *>(planes));
    return xpa_launch_status();
}

XPA_API int xpa_conv_fwd_small(int act, const float *x, int64_t batch, int64_t in_h, int64_t in_w, int64_t in_c,
                               const void *planes, const float *bias, int64_t out_c, int64_t kernel, int64_t stride,
                               int64_t pad, float slope, float *y, xpa_stream_t stream) {
    int nt;
    if (batch <= 0 || in_h <= 0 || in_w <= 0 || stride < 1 || pad < 0 || act < 0 || act > 2 || !x || !planes || !y ||
        !sm_shape(in_c, out_c, kernel, nt) || ((uintptr_t)x % 16) || ((uintptr_t)planes % 16) || ((uintptr_t)y % 4))
        return (int)hipErrorInvalidValue;
    const int64_t OH = (in_h + 2 * pad - kernel) / stride + 1, OW = (in_w + 2 * pad - kernel) / stride + 1;
    // the input's and the output's buffer records and their 32-bit byte offsets: both under 2 GiB (as xpa_conv_fwd)
    if (in_h + 2 * pad < kernel || in_w + 2 * pad < kernel || OH < 1 || OW < 1 ||
        batch * in_h * in_w * in_c * 4 >= ((int64_t)1 << 31) || batch * OH * OW * out_c * 4 >= ((int64_t)1 << 31))
        return (int)hipErrorInvalidValue;
    SmArgs a{};
    a.in = x; a.in_bytes = batch * in_h * in_w * in_c * 4; a.planes = static_cast<const char *>(planes); a.bias = bias;
    a.out = y; a.rows = batch * OH * OW;
    a.IH = (int)in_h; a.IW = (int)in_w; a.OH = (int)OH; a.OW = (int)OW; a.COUT = (int)out_c;
    a.K = (int)kernel; a.S = (int)stride; a.P = (int)pad; a.slope = slope;
    hipStream_t s = (hipStream_t)stream;
    if (act == 0) return sm_dispatch<0>(a, (int)in_c, nt, s);
    if (act == 1) return sm_dispatch<1>(a, (int)in_c, nt, s);
    return sm_dispatch<2>(a, (int)in_c, nt, s);
}
