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
// K28R-D (xpa_conv_dgrad_small, below the forward) is the data gradient at the same row counts: the same ring, blocks
// and arithmetic over the conv's input pixels, from planes split transposed, stride 2 as one stride-1 map per residue
// class, the previous block's activation backward and bias partials in its epilogue.
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
// one thread per (tap, step j, half h, column n < 32 nt): its 8 channels split, columns n >= cout zero.  GEMM column n,
// GEMM channel c of a tap sit at w[(n sn + c sc) taps + tap]: the forward's planes sn = in_c, sc = 1 (n = out channel);
// the data gradient's transposed ones sn = 1, sc = in_c (n = the conv's input channel, c = its output channel)
__global__ __launch_bounds__(256) void conv_wsplit_kernel(const float *__restrict__ w, int cin, int cout, int sn, int sc,
                                                          int k, int nt, __bf16 *__restrict__ out) {
    const int coutp = 32 * nt, spt = cin / 16, taps = k * k;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= taps * spt * 2 * coutp) return;
    const int n = e % coutp, h = (e / coutp) & 1, j = (e / (2 * coutp)) % spt, tap = e / (2 * coutp * spt);
    xpa_bf16x8 ph, pm, pl;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float x = n < cout ? w[((int64_t)n * sn + (int64_t)(16 * j + 8 * h + c) * sc) * taps + tap] : 0.f;
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

// ---- K28R-D: the data gradient ---------------------------------------------------------------------------------------
//   dx[m, ci] = act_prev'(y_prev[m, ci]) sum_{tap, co} dz[pixel(m, tap), co] W[co, ci, tap]   over the INPUT pixels m
// the same implicit GEMM with k = the conv's output channels (CO), n = its input channels, the planes transposed
// (conv_wsplit_kernel with sn = 1, sc = in_c).  The ring, the A registers and the barrier are the forward's; new are
//   classes   input pixel (iy, ix) with ((iy + P) % S, (ix + P) % S) = (ry, rx) receives only the taps ky = ry + S ty,
//             kx = rx + S tx, from the dz pixel ((iy + P) / S - ty, (ix + P) / S - tx): a stride-1 map over the class's
//             pixel lattice.  A block's 128 rows are 128 consecutive pixels (b, cy, cx) of ONE class's lattice, the grid
//             the sum of the S^2 classes' tiles (blk0: each class's first block), and the block's ring streams only
//             its class's taps (ascending; a tap is one contiguous run of the planes, so a subset streams as the whole
//             set does).  No MFMA on a masked tap; a class without taps (kernel 1, stride 2) writes act'(y) 0.
//   epilogue  lane i knows its row's dx pixel; the C/D map's rows fetch theirs by one cross-lane read each.  y_prev by
//             range-checked buffer loads at the store's own offsets, the stores branch-free; the column sums of what
//             was stored: 16 registers, the lane halves (one cross-lane add), the 4 waves through LDS in wave order,
//             plain stores to bias_partial[block][in_c].
struct SdArgs {
    const float *dz;       // NHWC [B, OH, OW, CO]
    int64_t dz_bytes;      // < 2^31
    const char *planes;    // xpa_conv_wsplit_t's output
    const float *yprev;    // NHWC [B, IH, IW, CI] (ACT > 0)
    float *dx;             // NHWC [B, IH, IW, CI]
    float *bias_partial;   // [gridDim.x][CI] (nullable)
    int64_t dx_bytes;      // < 2^31
    int B, IH, IW, OH, OW, CI, K, S, P;
    int blk0[4];           // class c = ry S + rx: its first block (INT32_MAX: no such class)
    int chy[2], cwx[2];    // the lattice of residue r: rows iy = ((r - P) mod S) + S cy, cy < chy[r]; columns likewise
    float slope;
};

template <int ACT>
__device__ __forceinline__ float sm_grad(float d, float y, float slope) {   // K28's ig_grad: act' from the OUTPUT y
#pragma clang fp contract(off)
    if (ACT == 1) return y > 0.f ? d : d * slope;
    if (ACT == 2) return d * (1.0f - y * y);
    return d;
}

template <int CO, int NT, int ACT>
__global__ __launch_bounds__(64 * kSmWaves) void conv_small_dgrad_kernel(SdArgs a) {
    constexpr int SPT = CO / 16;                         // 16-channel steps per tap
    constexpr int CIP = 32 * NT;
    constexpr int STAGE = (int)sm_tap_bytes(CO, NT);     // one tap of the three planes
    constexpr int PIECES = STAGE / kSmPiece;
    __shared__ __attribute__((aligned(16))) char lds[kSmStages * STAGE];   // the ring, then the waves' column sums
    const unsigned base = __builtin_amdgcn_readfirstlane((unsigned)(uintptr_t)(lds_char_t *)lds);
    const int t = threadIdx.x, lane = t & 63, h = lane >> 5, i = lane & 31;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    // the block's class and its first block
    const int bid = blockIdx.x, sh = a.S - 1;
    int c = 0, b0 = 0;
#pragma unroll
    for (int q = 1; q < 4; ++q)
        if (bid >= a.blk0[q]) {
            c = q;
            b0 = a.blk0[q];
        }
    const int ry = c >> sh, rx = c & sh;
    const int chy = ry ? a.chy[1] : a.chy[0], cwx = rx ? a.cwx[1] : a.cwx[0];
    const int fy = (ry - a.P) & sh, fx = (rx - a.P) & sh;
    const int nty = a.K > ry ? (a.K - ry + sh) >> sh : 0, ntx = a.K > rx ? (a.K - rx + sh) >> sh : 0;
    const int taps = nty * ntx;
    // this lane's row: pixel (b, cy, cx) of the class's lattice -> the dx pixel and the dz pixel of tap (0, 0)
    const int64_t m = (int64_t)(bid - b0) * kSmRows + wave * 32 + i, hw = (int64_t)chy * cwx;
    const bool ok = m < a.B * hw;
    const int64_t mc = ok ? m : 0;
    const int b = (int)(mc / hw), rem = (int)(mc - b * hw);
    const int cy = rem / cwx, cx = rem - cy * cwx;
    const int iy = fy + (cy << sh), ix = fx + (cx << sh);
    const int pix = ok ? (b * a.IH + iy) * a.IW + ix : -1;
    const int pbase = b * a.OH * a.OW, qy = (iy + a.P) >> sh, qx = (ix + a.P) >> sh;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(a.dz), 0, (int)a.dz_bytes, 0x00020000);
    // local tap `lt` (global tap index `tap`) of the planes -> its ring stage
    auto issue_tap = [&](int lt, int tap) {
        const char *src = a.planes + (int64_t)tap * STAGE + lane * 16;
        const unsigned st = base + (unsigned)((lt & (kSmStages - 1)) * STAGE);
#pragma unroll
        for (int u = 0; u < (PIECES + kSmWaves - 1) / kSmWaves; ++u) {
            const int p = wave + kSmWaves * u;
            if (p < PIECES) sm_glds16(src + p * kSmPiece, st + (unsigned)(p * kSmPiece));
        }
    };
    auto tap_index = [&](int ty, int tx) { return (ry + (ty << sh)) * a.K + rx + (tx << sh); };
    // the lane's 8 channels of step j of the class's tap (ty, tx): outside the dz map, or a ragged row: zeros
    auto load_step = [&](f4v (&v)[2], int ty, int tx, int j) {
        const int oy = qy - ty, ox = qx - tx;
        const bool valid = ok && (unsigned)oy < (unsigned)a.OH && (unsigned)ox < (unsigned)a.OW;
        const int off = ((pbase + oy * a.OW + ox) * CO + 16 * j + 8 * h) * 4;
#pragma unroll
        for (int q = 0; q < 2; ++q)
            v[q] = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rsrc, valid ? off + 16 * q : INT32_MIN,
                                                                                 0, 0));
    };
    xpa_f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;
    f4v va[2] = {f4v{0.f, 0.f, 0.f, 0.f}, f4v{0.f, 0.f, 0.f, 0.f}}, vb[2];
    if (taps > 0) {
        issue_tap(0, tap_index(0, 0));
        load_step(va, 0, 0, 0);
    }
    int ty = 0, tx = 0;   // the tap of the loop below
#pragma unroll 1
    for (int lt = 0; lt < taps; ++lt) {
        // the one barrier of a tap, as the forward's (va through the asm for the reason given there)
        asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" : "+v"(va[0]), "+v"(va[1])::"memory");
        const bool more = lt + 1 < taps;
        int nty_ = ty, ntx_ = tx + 1;
        if (ntx_ == ntx) {
            ntx_ = 0;
            ++nty_;
        }
        if (more) issue_tap(lt + 1, tap_index(nty_, ntx_));
        const char *sb = lds + (lt & (kSmStages - 1)) * STAGE;
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
            if (j + 1 < SPT) load_step(vb, ty, tx, j + 1);
            else if (more) load_step(vb, nty_, ntx_, 0);
            __builtin_amdgcn_sched_barrier(0);
            xpa_bf16x8 ah, am, al;
            xpa_split8(float4{va[0][0], va[0][1], va[0][2], va[0][3]}, float4{va[1][0], va[1][1], va[1][2], va[1][3]},
                       ah, am, al);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const xpa_bf16x8 *bp = reinterpret_cast<const xpa_bf16x8 *>(sb) + (j * 3 * 2 + h) * CIP + 32 * nt + i;
                acc[nt] = xpa_mfma_s3(ah, am, al, bp[0], bp[2 * CIP], bp[4 * CIP], acc[nt]);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                va[q] = vb[q];
                asm volatile("" ::"v"(va[q]));
            }
        }
        ty = nty_;
        tx = ntx_;
    }
    // C/D map: row = (r & 3) + 8 (r >> 2) + 4 h of the wave's tile (its dx pixel from the lane that owns the row),
    // column n = 32 nt + i; ragged rows and padded columns past the records
    const __amdgpu_buffer_rsrc_t rout = __builtin_amdgcn_make_buffer_rsrc(a.dx, 0, (int)a.dx_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t ryp = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(ACT > 0 ? a.yprev : a.dx), 0, (int)a.dx_bytes, 0x00020000);
    int prow[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) prow[r] = __shfl(pix, 4 * h + (r & 3) + 8 * (r >> 2), 64);
    float bsum[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int n = 32 * nt + i;
        bsum[nt] = 0.f;
#pragma unroll
        for (int r0 = 0; r0 < 16; r0 += 8) {   // 8 y_prev loads in flight at a time
            int o[8];
            float yp[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                o[r] = prow[r0 + r] >= 0 && n < a.CI ? (prow[r0 + r] * a.CI + n) * 4 : INT32_MIN;
                if (ACT > 0) yp[r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ryp, o[r], 0, 0));
            }
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                float v = acc[nt][r0 + r];
                if (ACT > 0) v = sm_grad<ACT>(v, yp[r], a.slope);
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rout, o[r], 0, 0);
                bsum[nt] += o[r] != INT32_MIN ? v : 0.f;
            }
        }
    }
    if (a.bias_partial) {
        float *sB = reinterpret_cast<float *>(lds);
        __syncthreads();   // every wave done with the ring
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const float s = bsum[nt] + __shfl_xor(bsum[nt], 32, 64);
            if (h == 0) sB[wave * CIP + 32 * nt + i] = s;
        }
        __syncthreads();
        if (t < a.CI) {
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < kSmWaves; ++w) s += sB[w * CIP + t];
            a.bias_partial[(int64_t)bid * a.CI + t] = s;
        }
    }
}

bool sd_shape(int64_t in_c, int64_t out_c, int64_t k, int64_t stride, int &nt) {
    if ((out_c != 16 && out_c != 32 && out_c != 64) || in_c < 1 || in_c > 64 || k < 1 || k > 12 ||
        (stride != 1 && stride != 2))
        return false;
    nt = in_c <= 32 ? 1 : 2;
    return true;
}

// the lattice of residue r along an axis of n pixels (first pixel, count) and the classes' tiles: the grid
int64_t sd_classes(int64_t batch, int64_t in_h, int64_t in_w, int64_t stride, int64_t pad, SdArgs *a) {
    const int sh = (int)stride - 1;
    int chy[2] = {0, 0}, cwx[2] = {0, 0};
    for (int r = 0; r < stride; ++r) {
        const int f = (int)((r - pad) & sh);
        chy[r] = in_h > f ? (int)((in_h - f + sh) >> sh) : 0;
        cwx[r] = in_w > f ? (int)((in_w - f + sh) >> sh) : 0;
    }
    int64_t blocks = 0;
    for (int c = 0; c < 4; ++c) {
        const bool is = c < stride * stride;
        if (a) a->blk0[c] = is ? (int)blocks : INT32_MAX;
        if (is) blocks += (batch * chy[c >> sh] * cwx[c & sh] + kSmRows - 1) / kSmRows;
    }
    if (a)
        for (int r = 0; r < 2; ++r) {
            a->chy[r] = chy[r];
            a->cwx[r] = cwx[r];
        }
    return blocks;
}

template <int ACT>
int sd_dispatch(const SdArgs &a, int64_t blocks, int co, int nt, hipStream_t s) {
    const dim3 grid((unsigned)blocks), block(64 * kSmWaves);
#define XPA_SD(C_, N_) hipLaunchKernelGGL((conv_small_dgrad_kernel<C_, N_, ACT>), grid, block, 0, s, a)
    if (nt == 1) {
        if (co == 16) XPA_SD(16, 1); else if (co == 32) XPA_SD(32, 1); else XPA_SD(64, 1);
    } else {
        if (co == 16) XPA_SD(16, 2); else if (co == 32) XPA_SD(32, 2); else XPA_SD(64, 2);
    }
#undef XPA_SD
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
                       (int)in_c, (int)out_c, (int)in_c, 1, (int)kernel, nt, reinterpret_cast<__bf16 *>(planes));
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

XPA_API int xpa_conv_small_dgrad_ok(int64_t in_c, int64_t out_c, int64_t kernel, int64_t stride) {
    int nt;
    return sd_shape(in_c, out_c, kernel, stride, nt) ? 1 : 0;
}

XPA_API int64_t xpa_conv_wsplit_t_bytes(int64_t in_c, int64_t out_c, int64_t kernel) {
    int nt;
    return sd_shape(in_c, out_c, kernel, 1, nt) ? kernel * kernel * sm_tap_bytes(out_c, nt) : 0;
}

XPA_API int xpa_conv_wsplit_t(const float *w, int64_t in_c, int64_t out_c, int64_t kernel, void *planes,
                              xpa_stream_t stream) {
    int nt;
    if (!w || !planes || ((uintptr_t)planes % 16) || !sd_shape(in_c, out_c, kernel, 1, nt))
        return (int)hipErrorInvalidValue;
    const int64_t n = kernel * kernel * (out_c / 16) * 2 * 32 * nt;
    // GEMM k = out_c channels, GEMM columns = the in_c input channels: W'[n = ci][c = co][tap] = w[co][ci][tap]
    hipLaunchKernelGGL(conv_wsplit_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w,
                       (int)out_c, (int)in_c, 1, (int)in_c, (int)kernel, nt, reinterpret_cast<__bf16 *>(planes));
    return xpa_launch_status();
}

XPA_API int64_t xpa_conv_dgrad_small_num_partials(int64_t batch, int64_t in_h, int64_t in_w, int64_t stride) {
    if (batch <= 0 || in_h <= 0 || in_w <= 0 || (stride != 1 && stride != 2)) return 0;
    return sd_classes(batch, in_h, in_w, stride, 0, nullptr);   // the padding permutes the classes, not their sizes
}

XPA_API int xpa_conv_dgrad_small(const float *dz, int64_t batch, int64_t out_h, int64_t out_w, int64_t out_c,
                                 const void *planes, int64_t in_c, int64_t kernel, int64_t stride, int64_t pad,
                                 int64_t in_h, int64_t in_w, int act_prev, const float *y_prev, float slope, float *dx,
                                 float *bias_partial, xpa_stream_t stream) {
    int nt;
    if (batch <= 0 || in_h <= 0 || in_w <= 0 || pad < 0 || act_prev < -1 || act_prev > 2 || !dz || !planes || !dx ||
        !sd_shape(in_c, out_c, kernel, stride, nt) || ((uintptr_t)dz % 16) || ((uintptr_t)planes % 16) ||
        ((uintptr_t)dx % 4) || in_h + 2 * pad < kernel || in_w + 2 * pad < kernel ||
        out_h != (in_h + 2 * pad - kernel) / stride + 1 || out_w != (in_w + 2 * pad - kernel) / stride + 1 ||
        (act_prev >= 0 && !y_prev) ||
        batch * in_h * in_w * in_c * 4 >= ((int64_t)1 << 31) || batch * out_h * out_w * out_c * 4 >= ((int64_t)1 << 31))
        return (int)hipErrorInvalidValue;
    SdArgs a{};
    a.dz = dz; a.dz_bytes = batch * out_h * out_w * out_c * 4; a.planes = static_cast<const char *>(planes);
    a.yprev = y_prev; a.dx = dx; a.bias_partial = act_prev >= 0 ? bias_partial : nullptr;
    a.dx_bytes = batch * in_h * in_w * in_c * 4;
    a.B = (int)batch; a.IH = (int)in_h; a.IW = (int)in_w; a.OH = (int)out_h; a.OW = (int)out_w; a.CI = (int)in_c;
    a.K = (int)kernel; a.S = (int)stride; a.P = (int)pad; a.slope = slope;
    const int64_t blocks = sd_classes(batch, in_h, in_w, stride, pad, &a);
    hipStream_t s = (hipStream_t)stream;
    // act_prev -1 is the identity without partials
    if (act_prev <= 0) return sd_dispatch<0>(a, blocks, (int)out_c, nt, s);
    if (act_prev == 1) return sd_dispatch<1>(a, blocks, (int)out_c, nt, s);
    return sd_dispatch<2>(a, blocks, (int)out_c, nt, s);
}
