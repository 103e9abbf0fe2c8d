// K28R-W — the conv weight gradient of small batches on the bf16 matrix cores: the third direction of K28R / K28R-D
// (igemm_small.hip), the row counts below igemm_min_rows that K29 (igemm.hip, fp32 MFMA, a fixed 512-block grid) leaves
// to the library.
//
//   dW[co, ci, ky, kx] = sum_m dz[m, co] x[pixel(m, ky, kx), ci]        m = (b, oy, ox) over the output pixels,
//                                                                        pixel = (oy S - P + ky, ox S - P + kx)
//
// A GEMM with M = out_c, N = k k in_c (column n = tap in_c + ci), K = rows, and BOTH operands k-major in memory (NHWC
// keeps a pixel's channels together): K41V's situation (sgemm3.hip).  Its staging: float4 loads along the channels,
// xpa_split3, ds_write_b64 of bf16x4 into three k-major bf16 planes, MFMA fragments back by ds_read_b64_tr_b16; the
// arithmetic is xpa_mfma_s3's six v_mfma_f32_32x32x16_bf16 products per 16-k step.
//   implicit   a transposed read takes a per-lane address, so for a tile's tap (ky, kx) the fragment's k-row m reads the
//              LDS row of input pixel pixel(m, ky, kx) of the staged input slab.  x is split once per slab, not once per
//              tap; dz once; no im2col matrix anywhere.
//   slab       R output rows of one image (the whole image where it fits): the input rows they cover, staged ZERO-PADDED
//              as [(R - 1) S + k rows][PW = (OW - 1) S + k columns][in_c] (K29's slab: a padding tap reads a staged
//              zero, no bounds check in the loop), and the R OW dz rows up to a multiple of 16 (the ragged k-step's
//              rows zero).  Then pixel(m, tap) = base(m) + (ky PW + kx): base(m) from a table in LDS built once (a
//              slab's geometry never changes), the tap's offset a per-lane constant of the kernel.
//   pitch      a 16-lane group of a transposed read covers 4 k-rows x 32 B, two groups 64 B per row; the four rows are
//              4 consecutive output pixels = input pixels S apart.  The pixel pitch is the smallest >= 2 in_c B with
//              (S x pitch) mod 256 in {64, 192}, so the four rows fall in four different 16-bank quarters at stride 1
//              and at stride 2 (in_c 64: 192 / 160 B; 32: 64 / 96 B; 16: 32 B, 32-B windows); dz (consecutive rows)
//              likewise: 32 / 64 / 192 B.  A row wrap (ox = OW - 1 -> 0) breaks the pattern for that one read.
//   tiles      the [out_c x k k in_c] accumulator is cut into 32 x 32 tiles, co-tile major, and dealt T consecutive
//              tiles per wave (T <= 4; <= 36 tiles = 36 864 floats per block, the register file's 144 KiB of 512): a wave's
//              tiles share their dz fragments (re-read only where the co-tile changes) and read their own taps' x
//              fragments.  A 16-lane group's 16 columns lie in one tap (in_c >= 16), so in_c 16 packs two taps into a
//              tile.  Lanes past out_c (out_c 16) or past the last tap read one zero area kept in LDS.  More than 36
//              tiles (out_c 16 wastes half of each): column groups over blockIdx.y, each writing its own columns of
//              the same partial.
//   grid       persistent: G = min(slabs, CUs / column groups) blocks, block g takes slabs g, g + G, ...; LDS is double-
//              buffered: slab n + 1's global loads are issued into registers before slab n's MFMAs, split and written
//              to the other stage after them; one barrier per slab.  Each block writes its partial once, in the
//              weight's own [out_c][in_c][k][k] order, for xpa_colsum_finalize (f64, fixed order).  Every block has a
//              slab, so every partial is written.
// No atomics, no grid-wide synchronisation, fixed summation order (slabs ascending per block, 16-row steps ascending,
// xpa_mfma_s3's product order): two launches give the same bits.  Nothing is written outside the partials.
//
// Compiled with igemm_small.hip's flags (_lib.EXTRA_FLAGS).
#include "xpa_common.h"
#include "s3_split.h"

#include <atomic>

namespace {

typedef float f4v __attribute__((ext_vector_type(4)));
typedef __bf16 sw_bf16x4 __attribute__((ext_vector_type(4)));
typedef short sw_v4s __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) sw_v4s sw_lds_v4s;

constexpr int kSwUX = 6, kSwUA = 3;        // float4 staging units per thread and slab: input, dz
constexpr int kSwTileCap = 36;             // accumulator tiles per block
constexpr int kSwLds = 160 * 1024;
constexpr int kSwZero = 256;               // bytes of the zero area at the start of LDS
constexpr int kSwNoRow = 0x1fff;           // row field of a unit that never loads
constexpr int kSwNoLds = 0x3ffff;          // LDS field of a unit that never writes

struct SwArgs {
    const float *dz, *x;
    float *partial;
    int dz_bytes, x_bytes;
    int IH, IW, OH, OW, CI, CO, K, S, P;
    int lg_ci4, lg_co4;          // log2(in_c / 4), log2(out_c / 4)
    int R, nsl, nslabs;          // output rows per slab, slabs per image, slabs
    int PW, jpad;                // staged columns per input row; R OW rounded up to 16
    int pitch_x, pitch_a;        // bytes per pixel and plane
    int plane_x, plane_a;        // bytes per plane
    int stage;                   // 3 plane_x + 3 plane_a
    int xunits, aunits;          // float4s of one slab
    int ntl, tiles, per;         // n-tiles; tiles = co-tiles x ntl; tiles per column group
};

__device__ __forceinline__ xpa_bf16x8 sw_frag(const char *p0, const char *p1) {
    const sw_v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((sw_lds_v4s *)p0);
    const sw_v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((sw_lds_v4s *)p1);
    return __builtin_bit_cast(xpa_bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// the three planes of 4 consecutive channels (K41V's v_put)
__device__ __forceinline__ void sw_put(char *p, int plane, f4v v) {
    sw_bf16x4 h, m, l;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        __bf16 a0, a1, a2;
        xpa_split3(v[j], a0, a1, a2);
        h[j] = a0;
        m[j] = a1;
        l[j] = a2;
    }
    *reinterpret_cast<sw_bf16x4 *>(p) = h;
    *reinterpret_cast<sw_bf16x4 *>(p + plane) = m;
    *reinterpret_cast<sw_bf16x4 *>(p + 2 * plane) = l;
}

template <int T>
__global__ __launch_bounds__(T == 4 ? 512 : 768) void conv_wgrad_small_kernel(SwArgs a) {
    // [zero area][table: jpad ints][stage 0][stage 1]; a stage: x planes hi / mid / lo, dz planes hi / mid / lo
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int t = threadIdx.x, nthr = blockDim.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3, h = lane >> 5, i31 = lane & 31;
    int *tab = reinterpret_cast<int *>(lds + kSwZero);
    char *st0 = lds + kSwZero + 4 * a.jpad;
    const int taps = a.K * a.K;
    // ---- once: the zero area, the pixel table, the staging units, the wave's tiles -----------------------------------
    for (int e = t; e < kSwZero / 4; e += nthr) reinterpret_cast<int *>(lds)[e] = 0;
    for (int j = t; j < a.jpad; j += nthr) {   // output pixel j of a slab -> its tap-(0, 0) pixel of the staged input
        const int r = j / a.OW, ox = j - r * a.OW;
        tab[j] = r < a.R ? (r * a.S * a.PW + ox * a.S) * a.pitch_x : 0;
    }
    int xs[kSwUX], xm[kSwUX], as[kSwUA], am[kSwUA];   // source byte offset inside the slab; (row << 18) | LDS offset
#pragma unroll
    for (int i = 0; i < kSwUX; ++i) {
        const int u = t + nthr * i;
        const int c4 = u & ((1 << a.lg_ci4) - 1), pix = u >> a.lg_ci4;
        const int rr = pix / a.PW, ix = pix - rr * a.PW - a.P;
        const bool on = u < a.xunits, col = (unsigned)ix < (unsigned)a.IW;
        xs[i] = (int)(((unsigned)(rr * a.IW + ix) * a.CI + 4 * c4) * 4u);
        xm[i] = ((on && col ? rr : kSwNoRow) << 18) | (on ? pix * a.pitch_x + 8 * c4 : kSwNoLds);
    }
#pragma unroll
    for (int i = 0; i < kSwUA; ++i) {
        const int u = t + nthr * i;
        const int c4 = u & ((1 << a.lg_co4) - 1), j = u >> a.lg_co4;
        const bool on = u < a.aunits;
        as[i] = (int)(((unsigned)j * a.CO + 4 * c4) * 4u);
        am[i] = ((on ? j : kSwNoRow) << 18) | (on ? 3 * a.plane_x + j * a.pitch_a + 8 * c4 : kSwNoLds);
    }
    // tiles [first, first + ntw) of the block's column group, co-tile major: tile -> (ct, nt)
    const int grp0 = blockIdx.y * a.per, grp1 = min(a.tiles, grp0 + a.per);
    const int first = grp0 + wave * T;
    const int ntw = max(0, min(T, grp1 - first));
    int ct[T], boff[T];
    bool bok[T];
#pragma unroll
    for (int u = 0; u < T; ++u) {
        const int idx = first + u;
        ct[u] = __builtin_amdgcn_readfirstlane(idx / a.ntl);
        const int nt = idx - ct[u] * a.ntl;
        const int n0 = 32 * nt + 16 * (g & 1), tap = n0 / a.CI, ci0 = (n0 & (a.CI - 1)) + 4 * p;
        const int ky = tap / a.K, kx = tap - ky * a.K;
        bok[u] = tap < taps;
        boff[u] = (ky * a.PW + kx) * a.pitch_x + 2 * ci0;
    }
    const char *zaddr = lds + 8 * (lane & 15);
    const int acol = 2 * (16 * (g & 1) + 4 * p);
    xpa_f32x16 acc[T];
#pragma unroll
    for (int u = 0; u < T; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[u][r] = 0.f;

    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.x), 0, a.x_bytes,
                                                                        0x00020000);
    const __amdgpu_buffer_rsrc_t rz = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(a.dz), 0, a.dz_bytes,
                                                                        0x00020000);
    f4v vx[kSwUX], va[kSwUA];
    // slab n's float4s into registers: a padding pixel, a row outside the image, a dz row past the slab's last: an offset
    // past the record, zeros from the hardware
    auto load_slab = [&](int n) {
        const int b = n / a.nsl, oy0 = (n - b * a.nsl) * a.R;
        const int iys = oy0 * a.S - a.P, jn = min(a.R, a.OH - oy0) * a.OW;
        const unsigned xb = (unsigned)((b * a.IH + iys) * a.IW) * (unsigned)(a.CI * 4);   // (iys < 0: mod 2^32)
        const unsigned ab = (unsigned)((b * a.OH + oy0) * a.OW) * (unsigned)(a.CO * 4);
#pragma unroll
        for (int i = 0; i < kSwUX; ++i) {
            const bool ok = (unsigned)(iys + (xm[i] >> 18)) < (unsigned)a.IH;   // the row field is 13 bits: >> is exact
            // (the sum in unsigned: a unit that never loads may wrap)
            const int off = ok ? (int)((unsigned)xb + (unsigned)xs[i]) : INT32_MIN;
            vx[i] = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rx, off, 0, 0));
        }
#pragma unroll
        for (int i = 0; i < kSwUA; ++i) {
            const bool ok = (am[i] >> 18) < jn;
            const int off = ok ? (int)((unsigned)ab + (unsigned)as[i]) : INT32_MIN;
            va[i] = __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(rz, off, 0, 0));
        }
    };
    auto store_slab = [&](char *st) {
#pragma unroll
        for (int i = 0; i < kSwUX; ++i)
            if ((xm[i] & kSwNoLds) != kSwNoLds) sw_put(st + (xm[i] & kSwNoLds), a.plane_x, vx[i]);
#pragma unroll
        for (int i = 0; i < kSwUA; ++i)
            if ((am[i] & kSwNoLds) != kSwNoLds) sw_put(st + (am[i] & kSwNoLds), a.plane_a, va[i]);
    };
    int n = blockIdx.x;   // < nslabs: the grid holds no block without a slab
    load_slab(n);
    store_slab(st0);
    __syncthreads();
    int cur = 0;
#pragma unroll 1
    for (; n < a.nslabs; n += gridDim.x) {
        const bool more = n + (int)gridDim.x < a.nslabs;
        if (more) load_slab(n + gridDim.x);
        const char *sx = st0 + cur * a.stage, *sa = sx + 3 * a.plane_x;
        const int sl = n % a.nsl;
        const int steps = (min(a.R, a.OH - sl * a.R) * a.OW + 15) >> 4;
        if (ntw > 0) {
#pragma unroll 1
            for (int ks = 0; ks < steps; ++ks) {
                // lane 4q + p of a 16-lane group supplies k-rows 8h + q and 8h + 4 + q, channels 4p ..+3 of its 16
                const int j0 = 16 * ks + 8 * h + q;
                const int tb0 = tab[j0], tb1 = tab[j0 + 4];
                xpa_bf16x8 ah, amid, al;
#pragma unroll
                for (int u = 0; u < T; ++u) {
                    if (u < ntw) {
                        if (u == 0 || ct[u] != ct[u - 1]) {   // wave-uniform: the dz fragments of co-tile ct[u]
                            const bool aok = 32 * ct[u] + 16 * (g & 1) < a.CO;
                            const char *a0 = aok ? sa + j0 * a.pitch_a + 64 * ct[u] + acol : zaddr;
                            const char *a1 = aok ? a0 + 4 * a.pitch_a : zaddr;
                            const int pa = aok ? a.plane_a : 0;
                            ah = sw_frag(a0, a1);
                            amid = sw_frag(a0 + pa, a1 + pa);
                            al = sw_frag(a0 + 2 * pa, a1 + 2 * pa);
                        }
                        const char *b0 = bok[u] ? sx + tb0 + boff[u] : zaddr;
                        const char *b1 = bok[u] ? sx + tb1 + boff[u] : zaddr;
                        const int pb = bok[u] ? a.plane_x : 0;
                        const xpa_bf16x8 bh = sw_frag(b0, b1), bm = sw_frag(b0 + pb, b1 + pb),
                                         bl = sw_frag(b0 + 2 * pb, b1 + 2 * pb);
                        acc[u] = xpa_mfma_s3(ah, amid, al, bh, bm, bl, acc[u]);
                    }
                }
            }
        }
        cur ^= 1;
        if (more) store_slab(st0 + cur * a.stage);
        __syncthreads();   // slab n + 1 is whole, and every wave is past slab n: the next pass may refill its stage
    }
    // C/D map: row co = 32 ct + (r & 3) + 8 (r >> 2) + 4 h, column n = 32 nt + (lane & 31) = tap in_c + ci
    float *out = a.partial + (int64_t)blockIdx.x * a.CO * a.CI * taps;
#pragma unroll
    for (int u = 0; u < T; ++u) {
        if (u < ntw) {
            const int nn = 32 * (first + u - ct[u] * a.ntl) + i31, tap = nn / a.CI, ci = nn & (a.CI - 1);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = 32 * ct[u] + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (tap < taps && co < a.CO) out[(co * a.CI + ci) * taps + tap] = acc[u][r];
            }
        }
    }
}

int sw_lg(int64_t v) { return v == 4 ? 2 : v == 8 ? 3 : 4; }   // log2 of channels / 4

bool sw_shape(int64_t in_c, int64_t out_c, int64_t k, int64_t stride) {
    return (in_c == 16 || in_c == 32 || in_c == 64) && (out_c == 16 || out_c == 32 || out_c == 64) && k >= 1 &&
           (stride == 1 || stride == 2) && k * k * in_c * out_c <= 36864;
}

// the smallest pixel pitch >= bytes whose four rows `step` pixels apart fall in four 16-bank quarters
int sw_pitch(int bytes, int step) {
    if (bytes < 64) return bytes;   // 16 channels: 32-B windows, consecutive rows
    int pitch = bytes;
    while ((step * pitch) % 256 != 64 && (step * pitch) % 256 != 192) pitch += 32;
    return pitch;
}

// the current device and its CU count, asked on every call (two host-side lookups): num_partials and the launch agree
// as long as the same device is current for both
int sw_cus(int &dev) {
    int n = 0;
    dev = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) {
        (void)hipGetLastError();
        return 256;
    }
    return n;
}

// the part of the launch plan that the map alone decides: tiles per wave T, waves, column groups, the slab; false: not
// even a slab of one output row fits (two stages in LDS, kSwUX + kSwUA float4 units per thread).  No runtime call.
bool sw_slab(int64_t in_h, int64_t in_w, int64_t in_c, int64_t out_c, int64_t k, int64_t s, int64_t pad, SwArgs &a,
             int &T, int &waves, int &groups, int &lds_bytes) {
    const int64_t OH = (in_h + 2 * pad - k) / s + 1, OW = (in_w + 2 * pad - k) / s + 1;
    a.IH = (int)in_h; a.IW = (int)in_w; a.OH = (int)OH; a.OW = (int)OW; a.CI = (int)in_c; a.CO = (int)out_c;
    a.K = (int)k; a.S = (int)s; a.P = (int)pad;
    a.lg_ci4 = sw_lg(in_c / 4); a.lg_co4 = sw_lg(out_c / 4);
    a.ntl = (int)((k * k * in_c + 31) / 32);
    a.tiles = (int)((out_c + 31) / 32) * a.ntl;
    groups = (a.tiles + kSwTileCap - 1) / kSwTileCap;
    a.per = (a.tiles + groups - 1) / groups;
    // T tiles per wave: the least MFMA work on the busiest SIMD (waves go round the 4 SIMDs); ties: more waves
    int best = INT32_MAX;
    for (int t = 4; t >= 1; --t) {
        const int w = (a.per + t - 1) / t, cost = t * ((w + 3) / 4);
        if (w <= (t == 4 ? 8 : 12) && cost <= best) {
            best = cost;
            T = t;
            waves = w < 4 ? 4 : w;
        }
    }
    const int64_t nthr = 64 * waves;
    a.PW = (int)((OW - 1) * s + k);
    a.pitch_x = sw_pitch((int)in_c * 2, (int)s);
    a.pitch_a = sw_pitch((int)out_c * 2, 1);
    int64_t r = OH;
    for (; r >= 1; --r) {
        const int64_t xpix = ((r - 1) * s + k) * a.PW, jpad = (r * OW + 15) & ~(int64_t)15;
        const int64_t stage = 3 * (xpix * a.pitch_x + jpad * a.pitch_a);
        if (kSwZero + 4 * jpad + 2 * stage <= kSwLds && xpix * in_c / 4 <= kSwUX * nthr &&
            jpad * out_c / 4 <= kSwUA * nthr && (r - 1) * s + k < kSwNoRow && jpad < kSwNoRow)
            break;
    }
    if (r < 1 || in_h + pad >= kSwNoRow) return false;   // (a unit's "never" row must lie outside every image)
    a.nsl = (int)((OH + r - 1) / r);
    a.R = (int)((OH + a.nsl - 1) / a.nsl);
    const int64_t xpix = ((int64_t)(a.R - 1) * s + k) * a.PW;
    a.jpad = (int)((a.R * OW + 15) & ~(int64_t)15);
    a.plane_x = (int)(xpix * a.pitch_x); a.plane_a = a.jpad * a.pitch_a;
    a.stage = 3 * (a.plane_x + a.plane_a);
    a.xunits = (int)(xpix * in_c / 4); a.aunits = (int)(a.jpad * out_c / 4);
    lds_bytes = kSwZero + 4 * a.jpad + 2 * a.stage;
    return true;
}

bool sw_map_ok(int64_t in_h, int64_t in_w, int64_t in_c, int64_t out_c, int64_t k, int64_t s, int64_t pad) {
    return in_h > 0 && in_w > 0 && pad >= 0 && sw_shape(in_c, out_c, k, s) && in_h + 2 * pad >= k && in_w + 2 * pad >= k;
}

// the whole plan: + the slabs of this batch and the grid (partials x column groups) on the current device
bool sw_plan(int64_t batch, int64_t in_h, int64_t in_w, int64_t in_c, int64_t out_c, int64_t k, int64_t s, int64_t pad,
             SwArgs &a, int &T, int &waves, dim3 &grid, int &lds_bytes, int &dev) {
    int groups = 1;
    if (!sw_slab(in_h, in_w, in_c, out_c, k, s, pad, a, T, waves, groups, lds_bytes) ||
        batch * a.nsl >= ((int64_t)1 << 31))
        return false;
    a.nslabs = (int)(batch * a.nsl);
    const int slots = sw_cus(dev) / groups;
    grid = dim3((unsigned)(a.nslabs < slots ? a.nslabs : slots < 1 ? 1 : slots), (unsigned)groups);
    return true;
}

bool sw_args_ok(int64_t batch, int64_t in_h, int64_t in_w, int64_t in_c, int64_t out_c, int64_t k, int64_t s,
                int64_t pad) {
    return batch > 0 && sw_map_ok(in_h, in_w, in_c, out_c, k, s, pad) &&
           batch * in_h * in_w * in_c * 4 < ((int64_t)1 << 31) &&
           batch * ((in_h + 2 * pad - k) / s + 1) * ((in_w + 2 * pad - k) / s + 1) * out_c * 4 < ((int64_t)1 << 31);
}

template <int T>
int sw_launch(const SwArgs &a, dim3 grid, int waves, int lds_bytes, int dev, hipStream_t s) {
    // once per instance and device (bit dev of the mask; a device past 63 asks every time): the kernel's dynamic LDS
    // may exceed 64 KiB.  Two threads racing here both set the attribute, which is idempotent
    static std::atomic<uint64_t> sized{0};
    const uint64_t bit = dev >= 0 && dev < 64 ? (uint64_t)1 << dev : 0;
    if (!(sized.load(std::memory_order_relaxed) & bit)) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&conv_wgrad_small_kernel<T>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, kSwLds);
        if (e != hipSuccess) return (int)e;
        sized.fetch_or(bit, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL((conv_wgrad_small_kernel<T>), grid, dim3((unsigned)(64 * waves)), (size_t)lds_bytes, s, a);
    return xpa_launch_status();
}

}  // namespace

XPA_API int xpa_conv_small_wgrad_ok(int64_t in_c, int64_t out_c, int64_t kernel, int64_t stride) {
    return sw_shape(in_c, out_c, kernel, stride) ? 1 : 0;
}

XPA_API int xpa_conv_wgrad_small_fits(int64_t in_h, int64_t in_w, int64_t in_c, int64_t out_c, int64_t kernel,
                                      int64_t stride, int64_t pad) {
    SwArgs a{};
    int T = 0, waves = 0, groups = 0, lds_bytes = 0;
    return sw_map_ok(in_h, in_w, in_c, out_c, kernel, stride, pad) &&
                   sw_slab(in_h, in_w, in_c, out_c, kernel, stride, pad, a, T, waves, groups, lds_bytes) ? 1 : 0;
}

XPA_API int64_t xpa_conv_wgrad_small_num_partials(int64_t batch, int64_t in_h, int64_t in_w, int64_t in_c,
                                                  int64_t out_c, int64_t kernel, int64_t stride, int64_t pad) {
    SwArgs a{};
    int T = 0, waves = 0, lds_bytes = 0, dev = 0;
    dim3 grid;
    if (!sw_args_ok(batch, in_h, in_w, in_c, out_c, kernel, stride, pad) ||
        !sw_plan(batch, in_h, in_w, in_c, out_c, kernel, stride, pad, a, T, waves, grid, lds_bytes, dev))
        return 0;
    return grid.x;
}

XPA_API int xpa_conv_wgrad_small(const float *dz, const float *x, int64_t batch, int64_t in_h, int64_t in_w,
                                 int64_t in_c, int64_t out_c, int64_t kernel, int64_t stride, int64_t pad,
                                 int64_t out_h, int64_t out_w, float *partial, xpa_stream_t stream) {
    SwArgs a{};
    int T = 0, waves = 0, lds_bytes = 0, dev = 0;
    dim3 grid;
    if (!dz || !x || !partial || ((uintptr_t)dz % 16) || ((uintptr_t)x % 16) || ((uintptr_t)partial % 4) ||
        !sw_args_ok(batch, in_h, in_w, in_c, out_c, kernel, stride, pad) ||
        out_h != (in_h + 2 * pad - kernel) / stride + 1 || out_w != (in_w + 2 * pad - kernel) / stride + 1 ||
        !sw_plan(batch, in_h, in_w, in_c, out_c, kernel, stride, pad, a, T, waves, grid, lds_bytes, dev))
        return (int)hipErrorInvalidValue;
    a.dz = dz; a.x = x; a.partial = partial;
    a.x_bytes = (int)(batch * in_h * in_w * in_c * 4);
    a.dz_bytes = (int)(batch * out_h * out_w * out_c * 4);
    hipStream_t s = (hipStream_t)stream;
    if (T == 4) return sw_launch<4>(a, grid, waves, lds_bytes, dev, s);
    if (T == 3) return sw_launch<3>(a, grid, waves, lds_bytes, dev, s);
    if (T == 2) return sw_launch<2>(a, grid, waves, lds_bytes, dev, s);
    return sw_launch<1>(a, grid, waves, lds_bytes, dev, s);
}
