/*
 * rtc_denoise.hip -- an edge-avoiding a-trous wavelet filter over a frame's accumulator (Dammertz et al.
 * 2010), guided by the first-hit buffers, with the per-sample-count normalisation of rtc_resolve_async and the project's
 * quantiser folded in.  The statement (denoise_load, denoise_tap, denoise_pixel, denoise_store) is compiled once for the
 * host (rtc_denoise_host) and once for the device (rtc_denoise_pack, rtc_denoise_iter_tile, rtc_denoise_iter_direct); the
 * device's output equals the host's byte for byte.  No reference counterpart: the reference writes its frame as it accumulated it (main.c:296-305).
 * The render kernels (rtc_render.hip) are not involved, no scene is named and the launch planner takes no part: the
 * entries work on the current device, like rtc_select_pixels_async.
 */
#include <hip/hip_runtime.h>

#include <new>

#include "../../include/rtc.h"
#include "rtc_device.h"
#include "rtc_internal.h"
#include "rtc_hip_util.h"
#include "rtc_pass_util.h"

/* ---- the filter's shape (rtc_denoise_shape gives the tile; raytracingc_amd/_abi.py mirrors it as constants and
 * tests/test_denoise_abi.py compares the two) ---- */
constexpr int kDnBlock = 256;               /* threads of every kernel below: 4 waves */
constexpr int kDnTile = 32;                 /* a workgroup's image tile at steps 1 and 2: 32 x 32 pixels, 4 per thread */
constexpr int kDnRowsPerThread = kDnTile * kDnTile / kDnBlock;
constexpr int kDnMaxIterations = 6, kDnMaxSquarings = 8;
static_assert(kDnBlock % kDnTile == 0 && kDnRowsPerThread * kDnBlock == kDnTile * kDnTile, "a thread takes whole entries");

/* what a tap needs beside the two pixels: host floats, the same on both sides */
struct DnWeights {
    float depthScale, colorScale; /* colorScale: cs_k of the iteration, made on the host */
    int squarings, hasNormal, hasDepth;
};

/* ---- the statement.  f32 operation by operation (the translation unit is built with -ffp-contract=off); every
 * division is the correctly rounded one on both sides; subnormals are kept on both sides. ---- */
/* Load: pixel p's colour entry (rgb, pad), scaled as rtc_resolve_async scales it */
__host__ __device__ inline float4 denoise_load(const float *accum, const int *samples, const float *albedo, size_t p,
                                               float fspp, float albedoFloor)
{
    float L[3] = {accum[3 * p], accum[3 * p + 1], accum[3 * p + 2]};
    if (samples) {
        const float scale = rtc_sample_scale(fspp, samples[p]);
        for (int c = 0; c < 3; ++c)
            L[c] = L[c] * scale;
    }
    if (albedo)
        for (int c = 0; c < 3; ++c) {
            const float a = albedo[3 * p + c];
            L[c] = a > albedoFloor ? L[c] / a : L[c];
        }
    return make_float4(L[0], L[1], L[2], 0.f);
}

/* pixel p's guide entry (normal.xyz, depth); a guide that is not given is never looked at */
__host__ __device__ inline float4 denoise_guide(const float *normal, const float *depth, size_t p)
{
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    if (normal) {
        g.x = normal[3 * p];
        g.y = normal[3 * p + 1];
        g.z = normal[3 * p + 2];
    }
    if (depth)
        g.w = depth[p];
    return g;
}

__host__ __device__ inline float denoise_h(int i)
{
    return i == 0 ? 0.375f : (i == 1 || i == -1) ? 0.25f : 0.0625f;
}

/* One tap: centre colour c and guide g, tap colour q and guide gq, w = H[|i|] * H[|j|] on entry. */
__host__ __device__ inline void denoise_tap(float w, const float4 &c, const float4 &g, const float4 &q, const float4 &gq,
                                            const DnWeights &k, float sum[3], float &wsum)
{
    if (k.hasNormal) {
        float t = (g.x * gq.x + g.y * gq.y) + g.z * gq.z;
        t = t > 0.f ? t : 0.f;
        for (int r = 0; r < k.squarings; ++r)
            t = t * t;
        w = w * t;
    }
    if (k.hasDepth) {
        const float dz = (g.w - gq.w) * k.depthScale;
        w = w / (1.f + dz * dz);
    }
    const float e = (__builtin_fabsf(c.x - q.x) + __builtin_fabsf(c.y - q.y)) + __builtin_fabsf(c.z - q.z);
    w = w / (1.f + (e * e) * k.colorScale);
    if (!(w > 0.f)) /* a NaN or zero weight never enters */
        return;
    sum[0] = sum[0] + q.x * w;
    sum[1] = sum[1] + q.y * w;
    sum[2] = sum[2] + q.z * w;
    wsum = wsum + w;
}

/* One iteration at pixel (x, y) of a width x rows image with step s: the centre, then the other 24 taps in row-major
 * order, a tap outside the image skipped.  at.color(i, j) and at.guide(i, j) give the entries of the tap (i, j); they are
 * called only for taps inside the image. */
template <class At>
__host__ __device__ inline float4 denoise_pixel(int x, int y, int width, int rows, int s, const DnWeights &k, const At &at)
{
    const float4 c = at.color(0, 0), g = at.guide(0, 0);
    float sum[3] = {c.x * 0.140625f, c.y * 0.140625f, c.z * 0.140625f};
    float wsum = 0.140625f;
#pragma unroll
    for (int j = -2; j <= 2; ++j) {
        const int dy = j * s; /* (|dy| <= 64: no overflow; y + dy is never formed for a tap outside) */
        if (dy < -y || dy >= rows - y)
            continue;
#pragma unroll
        for (int i = -2; i <= 2; ++i) {
            const int dx = i * s;
            if ((i == 0 && j == 0) || dx < -x || dx >= width - x)
                continue;
            denoise_tap(denoise_h(i) * denoise_h(j), c, g, at.color(i, j), at.guide(i, j), k, sum, wsum);
        }
    }
    return make_float4(sum[0] / wsum, sum[1] / wsum, sum[2] / wsum, 0.f);
}

/* Store: the last iteration's colour of pixel p to dOut and, where given, quantised to colors' bytes 3 p .. 3 p + 2 */
__host__ __device__ inline void denoise_store(const float4 &v, const float *albedo, float albedoFloor, size_t p, float O[3])
{
    O[0] = v.x;
    O[1] = v.y;
    O[2] = v.z;
    if (albedo)
        for (int c = 0; c < 3; ++c) {
            const float a = albedo[3 * p + c];
            O[c] = a > albedoFloor ? O[c] * a : O[c];
        }
}

/* ---- kernels ------------------------------------------------------------------------------------------------------ */
/* Pack: the load step, one pixel a thread, into the scratch's 16-byte entries. */
__global__ __launch_bounds__(kDnBlock) void rtc_denoise_pack(const float *__restrict__ accum, const int *__restrict__ samples,
                                                              const float *__restrict__ normal,
                                                              const float *__restrict__ depth,
                                                              const float *__restrict__ albedo, unsigned n, float fspp,
                                                              float albedoFloor, float4 *__restrict__ color,
                                                              float4 *__restrict__ guide)
{
    const unsigned p = blockIdx.x * (unsigned)kDnBlock + threadIdx.x;
    if (p >= n)
        return;
    color[p] = denoise_load(accum, samples, albedo, p, fspp, albedoFloor);
    guide[p] = denoise_guide(normal, depth, p);
}

/* what an iteration leaves of pixel p: the next 16-byte colour entry, or (LAST) the store step */
template <bool LAST>
__device__ inline void denoise_write(const float4 &v, size_t p, float4 *__restrict__ colorOut,
                                     const float *__restrict__ albedo, float albedoFloor, float *__restrict__ out,
                                     unsigned char *__restrict__ colors)
{
    if (!LAST) {
        colorOut[p] = v;
        return;
    }
    float O[3];
    denoise_store(v, albedo, albedoFloor, p, O);
    out[3 * p] = O[0];
    out[3 * p + 1] = O[1];
    out[3 * p + 2] = O[2];
    if (colors) { /* bytes: any alignment */
        colors[3 * p] = rtcdev::float_to_u8(O[0]);
        colors[3 * p + 1] = rtcdev::float_to_u8(O[1]);
        colors[3 * p + 2] = rtcdev::float_to_u8(O[2]);
    }
}

/* the staged tile as denoise_pixel sees it from pixel (lx, ly) of the tile: step S in LDS entries */
template <int S>
struct DnTileAt {
    const float4 *color_, *guide_; /* the centre's entries in LDS */
    __device__ float4 color(int i, int j) const { return color_[j * S * (kDnTile + 4 * S) + i * S]; }
    __device__ float4 guide(int i, int j) const { return guide_[j * S * (kDnTile + 4 * S) + i * S]; }
};

/* An iteration with step S <= 2 out of LDS.  Workgroup b takes the image tile (b % tilesX, b / tilesX) of 32 x 32 pixels,
 * stages it with its halo of 2 S -- (32 + 4 S)^2 entries of colour and of guide, a dwordx4 load each; an entry outside
 * the image is neither loaded nor read -- and runs every pixel's 24 taps out of LDS in the statement's order, in
 * registers: thread t takes column t % 32 of rows t / 32 + 8 r.  LAST: the store step instead of the next colour image. */
template <bool LAST, int S>
__global__ __launch_bounds__(kDnBlock) void rtc_denoise_iter_tile(const float4 *__restrict__ colorIn,
                                                                   const float4 *__restrict__ guide, int width, int rows,
                                                                   unsigned tilesX, DnWeights k,
                                                                   float4 *__restrict__ colorOut,
                                                                   const float *__restrict__ albedo, float albedoFloor,
                                                                   float *__restrict__ out,
                                                                   unsigned char *__restrict__ colors)
{
    constexpr int kStage = kDnTile + 4 * S, kHalo = 2 * S;
    __shared__ float4 sColor[kStage * kStage];
    __shared__ float4 sGuide[kStage * kStage];
    const int x0 = (int)(blockIdx.x % tilesX) * kDnTile, y0 = (int)(blockIdx.x / tilesX) * kDnTile;
    const bool wantGuide = k.hasNormal || k.hasDepth;
    for (int e = threadIdx.x; e < kStage * kStage; e += kDnBlock) {
        const int x = x0 - kHalo + e % kStage, y = y0 - kHalo + e / kStage;
        if (x < 0 || x >= width || y < 0 || y >= rows)
            continue;
        const size_t q = (size_t)y * (size_t)width + (size_t)x;
        sColor[e] = colorIn[q];
        if (wantGuide)
            sGuide[e] = guide[q];
    }
    __syncthreads();
    const int lx = threadIdx.x % kDnTile, x = x0 + lx;
    if (x >= width)
        return;
#pragma unroll 1
    for (int r = 0; r < kDnRowsPerThread; ++r) {
        const int ly = threadIdx.x / kDnTile + r * (kDnBlock / kDnTile), y = y0 + ly;
        if (y >= rows)
            break;
        const int centre = (ly + kHalo) * kStage + lx + kHalo;
        const DnTileAt<S> at = {sColor + centre, sGuide + centre};
        const float4 v = denoise_pixel(x, y, width, rows, S, k, at);
        denoise_write<LAST>(v, (size_t)y * (size_t)width + (size_t)x, colorOut, albedo, albedoFloor, out, colors);
    }
}

/* the images in memory (the device's, or rtc_denoise_host's) as denoise_pixel sees them from pixel p */
struct DnGlobalAt {
    const float4 *color_, *guide_; /* the centre's entries */
    long long pitch;
    int s;
    __host__ __device__ float4 color(int i, int j) const { return color_[j * s * pitch + i * s]; }
    __host__ __device__ float4 guide(int i, int j) const { return guide_[j * s * pitch + i * s]; }
};

/* An iteration with step s >= 4, where a halo of 2 s would outweigh the tile: every tap is two dwordx4 loads from global
 * memory.  Workgroup b takes the 32 x 8 pixels at (32 (b % tilesX), 8 (b / tilesX)), a pixel a thread. */
constexpr int kDnDirectRows = kDnBlock / kDnTile;
template <bool LAST>
__global__ __launch_bounds__(kDnBlock) void rtc_denoise_iter_direct(const float4 *__restrict__ colorIn,
                                                                     const float4 *__restrict__ guide, int width, int rows,
                                                                     int s, unsigned tilesX, DnWeights k,
                                                                     float4 *__restrict__ colorOut,
                                                                     const float *__restrict__ albedo, float albedoFloor,
                                                                     float *__restrict__ out,
                                                                     unsigned char *__restrict__ colors)
{
    const int x = (int)(blockIdx.x % tilesX) * kDnTile + (int)(threadIdx.x % kDnTile);
    const int y = (int)(blockIdx.x / tilesX) * kDnDirectRows + (int)(threadIdx.x / kDnTile);
    if (x >= width || y >= rows)
        return;
    const size_t p = (size_t)y * (size_t)width + (size_t)x;
    const DnGlobalAt at = {colorIn + p, guide + p, width, s};
    const float4 v = denoise_pixel(x, y, width, rows, s, k, at);
    denoise_write<LAST>(v, p, colorOut, albedo, albedoFloor, out, colors);
}

/* ---- host side ---------------------------------------------------------------------------------------------------- */
/* the scratch: the guide entries, then one colour image, then (two or more iterations) the second */
static size_t denoise_images(int iterations)
{
    return iterations >= 2 ? 3 : 2;
}

/* the refusals the device entry and the host statement share */
static int refuse_denoise(const char *who, const float *accum, const int *samples, const RtcHitBuffers *guides,
                          const RtcDenoiseDesc *d, const float *out)
{
    if (!accum || !d || !out)
        return rtc_fail(RTC_EINVAL, "%s: null accumulator, desc or output", who);
    if (d->width <= 0 || d->rows <= 0)
        return rtc_fail(RTC_EINVAL, "%s: an image of %d x %d", who, d->width, d->rows);
    if ((long long)d->width * (long long)d->rows > 0x7fffffffLL)
        return rtc_fail(RTC_EINVAL, "%s: %d x %d pixels (at most 2147483647 in one call)", who, d->width, d->rows);
    if (d->iterations < 1 || d->iterations > kDnMaxIterations)
        return rtc_fail(RTC_EINVAL, "%s: iterations = %d (1 .. %d)", who, d->iterations, kDnMaxIterations);
    if (d->normalSquarings < 0 || d->normalSquarings > kDnMaxSquarings)
        return rtc_fail(RTC_EINVAL, "%s: normalSquarings = %d (0 .. %d)", who, d->normalSquarings, kDnMaxSquarings);
    if (d->flags & ~RTC_DN_DEMODULATE)
        return rtc_fail(RTC_EINVAL, "%s: unknown flag in 0x%x", who, (unsigned)d->flags);
    if ((d->flags & RTC_DN_DEMODULATE) && !(guides && guides->albedo))
        return rtc_fail(RTC_EINVAL, "%s: RTC_DN_DEMODULATE without an albedo buffer", who);
    if (samples && d->spp <= 0)
        return rtc_fail(RTC_EINVAL, "%s: samples given with spp = %d", who, d->spp);
    if (out == accum)
        return rtc_fail(RTC_EINVAL, "%s: the output is the accumulator", who);
    return 0;
}

/* iteration k's weights: cs_k = colorScale * (float)(1 << 2k), on the host */
static DnWeights denoise_weights(const RtcDenoiseDesc *d, const RtcHitBuffers *guides, int k)
{
    DnWeights w;
    w.depthScale = d->depthScale;
    w.colorScale = d->colorScale * (float)(1 << (2 * k));
    w.squarings = d->normalSquarings;
    w.hasNormal = guides && guides->normal;
    w.hasDepth = guides && guides->depth;
    return w;
}

/* what a run works on: the guides it uses (albedo: only when demodulating) and, in `base`'s 3 n entries, the guide entries
 * and the two colour images (image[1]: only with two or more iterations) */
struct DnBuffers {
    const float *normal, *depth, *albedo;
    float4 *guide, *image[2];
};
static DnBuffers denoise_buffers(const RtcHitBuffers *guides, const RtcDenoiseDesc *d, float4 *base, size_t n)
{
    return {guides ? guides->normal : nullptr, guides ? guides->depth : nullptr,
            (d->flags & RTC_DN_DEMODULATE) ? guides->albedo : nullptr, base, {base + n, base + 2 * n}};
}

extern "C" int rtc_denoise_shape(int *tileW, int *tileH)
{
    if (!tileW || !tileH)
        return rtc_fail(RTC_EINVAL, "rtc_denoise_shape: null argument");
    *tileW = kDnTile;
    *tileH = kDnTile;
    return 0;
}

extern "C" size_t rtc_denoise_scratch_bytes(size_t pixelCount, int iterations)
{
    return pixelCount * sizeof(float4) * denoise_images(iterations);
}

extern "C" int rtc_denoise_async(const float *dAccum, const int *dSamples, const RtcHitBuffers *guides,
                                 const RtcDenoiseDesc *d, float *dOut, void *dColors, void *dScratch, size_t scratchBytes,
                                 void *stream)
{
    const char *const who = "rtc_denoise_async";
    if (const int rc = refuse_denoise(who, dAccum, dSamples, guides, d, dOut))
        return rc;
    const size_t n = (size_t)d->width * (size_t)d->rows;
    if (const int rc = rtc_refuse_scratch(who, dScratch))
        return rc;
    if (scratchBytes < rtc_denoise_scratch_bytes(n, d->iterations))
        return rtc_fail(RTC_EINVAL, "%s: %zu bytes of scratch, %zu pixels and %d iterations need %zu "
                        "(rtc_denoise_scratch_bytes)", who, scratchBytes, n, d->iterations,
                        rtc_denoise_scratch_bytes(n, d->iterations));
    const hipStream_t st = (hipStream_t)stream;
    const DnBuffers b = denoise_buffers(guides, d, (float4 *)dScratch, n);
    const dim3 block(kDnBlock);
    hipLaunchKernelGGL(rtc_denoise_pack, dim3((unsigned)((n + kDnBlock - 1) / kDnBlock)), block, 0, st, dAccum, dSamples,
                       b.normal, b.depth, b.albedo, (unsigned)n, (float)d->spp, d->albedoFloor, b.image[0], b.guide);
    for (int k = 0; k < d->iterations; ++k) {
        const int s = 1 << k;
        const DnWeights w = denoise_weights(d, guides, k);
        const bool last = k + 1 == d->iterations;
        const float4 *const in = b.image[k & 1];
        float4 *const next = last ? (float4 *)nullptr : b.image[(k + 1) & 1];
        unsigned char *const col = (unsigned char *)dColors;
        const unsigned tilesX = (unsigned)((d->width + kDnTile - 1) / kDnTile);
        const int tileRows = s <= 2 ? kDnTile : kDnDirectRows;
        const dim3 grid(tilesX * (unsigned)((d->rows + tileRows - 1) / tileRows)); /* (<= n / 256 + width + rows: < 2^31) */
        if (s <= 2) {
            const auto tile = s == 1 ? (last ? rtc_denoise_iter_tile<true, 1> : rtc_denoise_iter_tile<false, 1>)
                                     : (last ? rtc_denoise_iter_tile<true, 2> : rtc_denoise_iter_tile<false, 2>);
            hipLaunchKernelGGL(tile, grid, block, 0, st, in, b.guide, d->width, d->rows, tilesX, w, next, b.albedo,
                               d->albedoFloor, dOut, col);
        } else
            hipLaunchKernelGGL(last ? rtc_denoise_iter_direct<true> : rtc_denoise_iter_direct<false>, grid, block, 0, st, in,
                               b.guide, d->width, d->rows, s, tilesX, w, next, b.albedo, d->albedoFloor, dOut, col);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int rtc_denoise_host(const float *accum, const int *samples, const RtcHitBuffers *guides,
                                const RtcDenoiseDesc *d, float *out, void *colors)
{
    const char *const who = "rtc_denoise_host";
    if (const int rc = refuse_denoise(who, accum, samples, guides, d, out))
        return rc;
    const size_t n = (size_t)d->width * (size_t)d->rows;
    float4 *const store = new (std::nothrow) float4[3 * n];
    if (!store)
        return rtc_fail(RTC_ENOMEM, "%s: %zu bytes of host memory", who, 3 * n * sizeof(float4));
    const DnBuffers b = denoise_buffers(guides, d, store, n);
    for (size_t p = 0; p < n; ++p) {
        b.image[0][p] = denoise_load(accum, samples, b.albedo, p, (float)d->spp, d->albedoFloor);
        b.guide[p] = denoise_guide(b.normal, b.depth, p);
    }
    int rc = 0;
    for (int k = 0; k < d->iterations; ++k) {
        const DnWeights w = denoise_weights(d, guides, k);
        const float4 *const in = b.image[k & 1];
        float4 *const next = b.image[(k + 1) & 1];
        for (int y = 0; y < d->rows; ++y)
            for (int x = 0; x < d->width; ++x) {
                const size_t p = (size_t)y * (size_t)d->width + (size_t)x;
                const DnGlobalAt at = {in + p, b.guide + p, d->width, 1 << k};
                next[p] = denoise_pixel(x, y, d->width, d->rows, 1 << k, w, at);
            }
    }
    const float4 *const last = b.image[d->iterations & 1];
    for (size_t p = 0; p < n && rc == 0; ++p) {
        float O[3];
        denoise_store(last[p], b.albedo, d->albedoFloor, p, O);
        out[3 * p] = O[0];
        out[3 * p + 1] = O[1];
        out[3 * p + 2] = O[2];
        if (colors)
            rc = rtc_quantize(O, 1, (Color *)colors + p); /* the host's floatToUint */
    }
    delete[] store;
    return rc;
}
