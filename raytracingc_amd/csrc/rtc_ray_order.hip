/*
 * rtc_ray_order.hip -- a coherent order for caller-supplied rays: the 30-bit coherence key
 * (rtc_ray_keys_host and the key kernel: one statement, compiled for the host and for the device), a stable LSD radix
 * sort of (key, index) pairs on the device (rtc_ray_order_async, rtc_ray_order) and the two permutation kernels that apply
 * an order to the buffers of a query (rtc_gather_async, rtc_scatter_async).  No reference counterpart: the reference traces
 * the rays of a pixel grid in raster order (main.c:81-104) and never meets an incoherent ray buffer.
 * The query kernels (rtc_render.hip) are not involved: an ordered query is order, gather, the existing query on the gathered
 * buffers, scatter.
 */
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "rtc_layout.h"
#include "rtc_internal.h"
#include "rtc_hip_util.h"
#include "rtc_pass_util.h"
#include "rtc_staged.h"

/* ---- the sort's shape (rtc_ray_order_shape gives B and G; raytracingc_amd/_abi.py mirrors them as constants and
 * tests/test_ray_order_abi.py compares the two) ---- */
constexpr int kOrderBlock = 256;         /* threads of every kernel below: 4 waves */
constexpr int kOrderWaves = kOrderBlock / 64;
constexpr int kOrderRounds = 16;         /* keys per lane */
constexpr int kOrderKeysPerWave = 64 * kOrderRounds;
constexpr int kOrderKeysPerGroup = kOrderWaves * kOrderKeysPerWave; /* B = 4096 keys per workgroup */
constexpr int kOrderDigitBits = 8;
constexpr int kOrderRadix = 1 << kOrderDigitBits;                    /* 256 digits = one per thread */
constexpr int kOrderKeyBits = 30;
constexpr int kOrderPasses = (kOrderKeyBits + kOrderDigitBits - 1) / kOrderDigitBits; /* 4: bits 0-7, 8-15, 16-23, 24-29 */
constexpr int kOrderScanGroups = kOrderBlock; /* G = 256: workgroup counts one scan workgroup takes per step of its loop */
static_assert(kOrderRadix == kOrderBlock, "one digit per thread");
static_assert(kOrderPasses % 2 == 0, "the passes alternate between two buffers and end in dOrder");

/* The key's box: lo and scale = 32 / (hi - lo) per axis, computed once on the host (0 for a flat or unbounded axis). */
struct RtcKeyBox {
    float lo[3], scale[3];
};

/* ---- the key: this one statement is compiled for the host (rtc_ray_keys_host) and for the device (rtc_rsort_keys) ------
 * f32 operation by operation (the translation unit is built with -ffp-contract=off; the divisions are the correctly
 * rounded IEEE ones on both sides). */
__host__ __device__ inline unsigned key_cell(float pos, float lo, float scale)
{
    const float t = (pos - lo) * scale;
    return !(t >= 0.f) ? 0u : t >= 31.f ? 31u : (unsigned)(int)t;
}
__host__ __device__ inline unsigned key_q(float p)
{
    const float v = p * 64.f;
    return !(p >= 0.f) ? 0u : v >= 63.f ? 63u : (unsigned)(int)v;
}
/* bit b of a 5-bit value to bit 3 b */
__host__ __device__ inline unsigned key_spread(unsigned c)
{
    return (c & 1u) | (c & 2u) << 2 | (c & 4u) << 4 | (c & 8u) << 6 | (c & 16u) << 8;
}
__host__ __device__ inline unsigned ray_key(const float r[6], const RtcKeyBox &b)
{
    const unsigned cx = key_cell(r[0], b.lo[0], b.scale[0]), cy = key_cell(r[1], b.lo[1], b.scale[1]),
                   cz = key_cell(r[2], b.lo[2], b.scale[2]);
    const unsigned cell = key_spread(cx) | key_spread(cy) << 1 | key_spread(cz) << 2;
    const float ax = __builtin_fabsf(r[3]), ay = __builtin_fabsf(r[4]), az = __builtin_fabsf(r[5]);
    const float L = (ax + ay) + az;
    const float px = ax / L, py = ay / L;
    const unsigned oct = (r[3] < 0.f ? 1u : 0u) | (r[4] < 0.f ? 2u : 0u) | (r[5] < 0.f ? 4u : 0u);
    return cell << 15 | oct << 12 | key_q(py) << 6 | key_q(px);
}

static RtcKeyBox key_box(const float lo[3], const float hi[3])
{
    RtcKeyBox b;
    for (int a = 0; a < 3; ++a) {
        const float q = 32.f / (hi[a] - lo[a]);
        b.lo[a] = lo[a];
        b.scale[a] = hi[a] > lo[a] && std::isfinite(q) ? q : 0.f;
    }
    return b;
}

/* ---- kernels ------------------------------------------------------------------------------------------------------ */
/* key(rays[i]) into the sort's first key buffer and, where asked for, into the caller's dKeys */
__global__ __launch_bounds__(kOrderBlock) void rtc_rsort_keys(const float *__restrict__ rays, unsigned n, RtcKeyBox box,
                                                               unsigned *__restrict__ keys,
                                                               unsigned *__restrict__ userKeys)
{
    const unsigned i = blockIdx.x * (unsigned)kOrderBlock + threadIdx.x;
    if (i >= n)
        return;
    const float *p = rays + (size_t)i * 6;
    const float r[6] = {p[0], p[1], p[2], p[3], p[4], p[5]};
    const unsigned k = ray_key(r, box);
    keys[i] = k;
    if (userKeys)
        userKeys[i] = k;
}

/* One round of a wave over 64 consecutive keys: the lane's rank among the keys of its digit that this wave has met so far,
 * in the wave's order (round, then lane).  `same` = the valid lanes with the lane's digit, from one ballot per digit bit;
 * the lanes below give the rank inside the round, and the first lane of the set advances the wave's running count of the
 * digit in LDS (cnt: this wave's kOrderRadix counters, touched by no other wave).  Every lane of the wave calls it. */
__device__ inline unsigned order_wave_rank(unsigned digit, bool valid, unsigned *cnt, int lane)
{
    unsigned long long same = __ballot(valid);
#pragma unroll
    for (int b = 0; b < kOrderDigitBits; ++b) {
        const bool bit = (digit >> b) & 1u;
        const unsigned long long v = __ballot(bit);
        same &= bit ? v : ~v;
    }
    const unsigned below = (unsigned)__popcll(same & ((1ull << lane) - 1ull));
    const int first = valid ? __ffsll((long long)same) - 1 : lane;
    unsigned old = 0;
    if (valid && lane == first) {
        old = cnt[digit];
        cnt[digit] = old + (unsigned)__popcll(same);
    }
    old = __shfl(old, first);
    /* the next round's first lanes read what this round's wrote: LDS operations of one wave complete in order */
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    return old + below;
}

/* Per-workgroup digit histogram of one pass: hist[digit * groups + workgroup] = the workgroup's keys of that digit.  Wave w
 * of workgroup g takes keys [g B + w * 1024, + 1024), 64 consecutive keys a round. */
__global__ __launch_bounds__(kOrderBlock) void rtc_rsort_hist(const unsigned *__restrict__ keys, unsigned n, int shift,
                                                               unsigned groups, unsigned *__restrict__ hist)
{
    __shared__ unsigned cnt[kOrderWaves][kOrderRadix];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int w = 0; w < kOrderWaves; ++w)
        cnt[w][t] = 0;
    __syncthreads();
    const unsigned base = blockIdx.x * (unsigned)kOrderKeysPerGroup + (unsigned)(wave * kOrderKeysPerWave);
    for (int r = 0; r < kOrderRounds; ++r) {
        const unsigned i = base + (unsigned)(r * 64 + lane);
        const bool valid = i < n;
        const unsigned digit = valid ? (keys[i] >> shift) & (unsigned)(kOrderRadix - 1) : 0u;
        (void)order_wave_rank(digit, valid, cnt[wave], lane);
    }
    __syncthreads();
    unsigned sum = 0;
#pragma unroll
    for (int w = 0; w < kOrderWaves; ++w)
        sum += cnt[w][t];
    hist[(size_t)t * groups + blockIdx.x] = sum;
}

/* The scan over (digit, workgroup): workgroup d turns row d of hist into its exclusive prefix in place, kOrderScanGroups
 * entries a step with the running sum carried, and leaves the digit's total in totals[d]. */
__global__ __launch_bounds__(kOrderBlock) void rtc_rsort_scan(unsigned *__restrict__ hist, unsigned groups,
                                                               unsigned *__restrict__ totals)
{
    __shared__ unsigned waveSum[kOrderWaves];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    unsigned *row = hist + (size_t)blockIdx.x * groups;
    unsigned carry = 0;
    for (unsigned c = 0; c < groups; c += (unsigned)kOrderScanGroups) {
        const unsigned g = c + (unsigned)t;
        const unsigned v = g < groups ? row[g] : 0u;
        unsigned total;
        const unsigned excl = rtc_block_scan<kOrderWaves>(v, waveSum, lane, wave, total);
        if (g < groups)
            row[g] = carry + excl;
        carry += total;
    }
    if (t == 0)
        totals[blockIdx.x] = carry;
}

/* The stable scatter of one pass.  A key's place = the digits below it (the scan of totals) + its digit's keys in earlier
 * workgroups (the scanned hist) + in earlier waves of its workgroup + its rank in its wave (order_wave_rank): ascending
 * input position inside every digit, so equal keys keep their order.  FIRST: the index is the position itself (no index
 * buffer yet).  LAST: the keys are not needed any more. */
template <bool FIRST, bool LAST>
__global__ __launch_bounds__(kOrderBlock) void rtc_rsort_scatter(const unsigned *__restrict__ keysIn,
                                                                  const unsigned *__restrict__ idxIn, unsigned n, int shift,
                                                                  unsigned groups, const unsigned *__restrict__ hist,
                                                                  const unsigned *__restrict__ totals,
                                                                  unsigned *__restrict__ keysOut,
                                                                  unsigned *__restrict__ idxOut)
{
    __shared__ unsigned cnt[kOrderWaves][kOrderRadix];
    __shared__ unsigned waveSum[kOrderWaves];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int w = 0; w < kOrderWaves; ++w)
        cnt[w][t] = 0;
    unsigned all; /* (the scan's barriers cover the zeroing) */
    const unsigned digitBase = rtc_block_scan<kOrderWaves>(totals[t], waveSum, lane, wave, all);
    const unsigned base = blockIdx.x * (unsigned)kOrderKeysPerGroup + (unsigned)(wave * kOrderKeysPerWave);
    unsigned key[kOrderRounds], rank[kOrderRounds];
#pragma unroll
    for (int r = 0; r < kOrderRounds; ++r) {
        const unsigned i = base + (unsigned)(r * 64 + lane);
        const bool valid = i < n;
        key[r] = valid ? keysIn[i] : 0u;
        rank[r] = order_wave_rank((key[r] >> shift) & (unsigned)(kOrderRadix - 1), valid, cnt[wave], lane);
    }
    __syncthreads();
    { /* thread t = digit t: the counts of the four waves become the waves' first places */
        unsigned at = digitBase + hist[(size_t)t * groups + blockIdx.x];
#pragma unroll
        for (int w = 0; w < kOrderWaves; ++w) {
            const unsigned c = cnt[w][t];
            cnt[w][t] = at;
            at += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kOrderRounds; ++r) {
        const unsigned i = base + (unsigned)(r * 64 + lane);
        if (i < n) {
            const unsigned pos = cnt[wave][(key[r] >> shift) & (unsigned)(kOrderRadix - 1)] + rank[r];
            if (pos < n) { /* (always: the places of a pass are a permutation of [0, n)) */
                if (!LAST)
                    keysOut[pos] = key[r];
                idxOut[pos] = FIRST ? i : idxIn[i];
            }
        }
    }
}

/* dst[i] = src[order[i]] (SCATTER: dst[order[i]] = src[i]) for elements of K dwords (K == 0: `words`, at run time):
 * consecutive lanes take consecutive dwords of the side that is read or written in order. */
template <int K, bool SCATTER>
__global__ __launch_bounds__(kOrderBlock) void rtc_permute_words(unsigned *__restrict__ dst,
                                                                  const unsigned *__restrict__ src,
                                                                  const unsigned *__restrict__ order, size_t total,
                                                                  unsigned words)
{
    const unsigned k = K ? (unsigned)K : words;
    const size_t g = blockIdx.x * (size_t)kOrderBlock + threadIdx.x;
    if (g >= total)
        return;
    const size_t e = g / k;
    const unsigned j = (unsigned)(g - e * k);
    const size_t o = (size_t)order[e] * k + j;
    if (SCATTER)
        dst[o] = src[g];
    else
        dst[g] = src[o];
}
/* the same for single bytes, at any alignment: byte loads and byte stores only */
template <bool SCATTER>
__global__ __launch_bounds__(kOrderBlock) void rtc_permute_bytes(unsigned char *__restrict__ dst,
                                                                  const unsigned char *__restrict__ src,
                                                                  const unsigned *__restrict__ order, unsigned n)
{
    const unsigned i = blockIdx.x * (unsigned)kOrderBlock + threadIdx.x;
    if (i >= n)
        return;
    if (SCATTER)
        dst[order[i]] = src[i];
    else
        dst[i] = src[order[i]];
}

/* ---- the sort's scratch: three arrays of n words (two key buffers, one index buffer; dOrder is the other index buffer),
 * the histogram of kOrderRadix x groups words and the kOrderRadix digit totals, each region a multiple of 256 bytes */
struct RtcOrderScratch {
    size_t groups, keys0, keys1, idx, hist, totals, words;
};
static RtcOrderScratch order_scratch(size_t n)
{
    RtcOrderScratch L;
    const size_t r = (n + 63) / 64 * 64;
    L.groups = (n + kOrderKeysPerGroup - 1) / kOrderKeysPerGroup;
    L.keys0 = 0, L.keys1 = r, L.idx = 2 * r, L.hist = 3 * r;
    L.totals = L.hist + (L.groups * kOrderRadix + 63) / 64 * 64;
    L.words = L.totals + kOrderRadix;
    return L;
}

static int refuse_order(const char *who, const void *s, const void *rays, const void *order, size_t n)
{
    if (!s)
        return rtc_fail(RTC_EINVAL, "%s: null scene", who);
    if (!rays || !order)
        return rtc_fail(RTC_EINVAL, "%s: null argument", who);
    if (n > (size_t)0x7fffffff)
        return rtc_fail(RTC_EINVAL, "%s: %zu rays (at most 2147483647 in one call)", who, n);
    return 0;
}

template <bool SCATTER>
static int permute(const char *who, void *dDst, const void *dSrc, const unsigned *dOrder, size_t n, size_t elemBytes, void *stream)
{
    if (!dDst || !dSrc || !dOrder)
        return rtc_fail(RTC_EINVAL, "%s: null pointer", who);
    if (n > (size_t)0x7fffffff)
        return rtc_fail(RTC_EINVAL, "%s: %zu elements (at most 2147483647 in one call)", who, n);
    if (elemBytes != 1 && (elemBytes == 0 || elemBytes % 4 != 0 || elemBytes > 64))
        return rtc_fail(RTC_EINVAL, "%s: elements of %zu bytes (1, or a multiple of 4 up to 64)", who, elemBytes);
    if (elemBytes != 1 && (((size_t)dDst | (size_t)dSrc) & 3) != 0)
        return rtc_fail(RTC_EINVAL, "%s: elements of %zu bytes need 4-byte aligned buffers", who, elemBytes);
    if (dDst == dSrc)
        return rtc_fail(RTC_EINVAL, "%s: the destination is the source", who);
    if (n == 0)
        return 0;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 block(kOrderBlock);
    if (elemBytes == 1) {
        hipLaunchKernelGGL(rtc_permute_bytes<SCATTER>, dim3((unsigned)((n + kOrderBlock - 1) / kOrderBlock)), block, 0, st,
                           (unsigned char *)dDst, (const unsigned char *)dSrc, dOrder, (unsigned)n);
    } else {
        const unsigned k = (unsigned)(elemBytes / 4);
        const size_t total = n * k; /* < 2^35: at most 2^27 workgroups */
        const dim3 grid((unsigned)((total + kOrderBlock - 1) / kOrderBlock));
        unsigned *d = (unsigned *)dDst;
        const unsigned *s = (const unsigned *)dSrc;
        switch (k) { /* the queries' sizes by name: 4 (prim, depth, seeds, limits), 12 (vectors), 24 (rays) */
        case 1: hipLaunchKernelGGL((rtc_permute_words<1, SCATTER>), grid, block, 0, st, d, s, dOrder, total, k); break;
        case 3: hipLaunchKernelGGL((rtc_permute_words<3, SCATTER>), grid, block, 0, st, d, s, dOrder, total, k); break;
        case 6: hipLaunchKernelGGL((rtc_permute_words<6, SCATTER>), grid, block, 0, st, d, s, dOrder, total, k); break;
        default: hipLaunchKernelGGL((rtc_permute_words<0, SCATTER>), grid, block, 0, st, d, s, dOrder, total, k); break;
        }
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int rtc_scene_bounds(const RtcDeviceScene *s, float lo[3], float hi[3])
{
    if (!s || !lo || !hi)
        return rtc_fail(RTC_EINVAL, "rtc_scene_bounds: null argument");
    memcpy(lo, s->boundsLo, sizeof s->boundsLo);
    memcpy(hi, s->boundsHi, sizeof s->boundsHi);
    return 0;
}

extern "C" int rtc_ray_keys_host(const Ray *rays, size_t n, const float lo[3], const float hi[3], unsigned *keys)
{
    if (!lo || !hi || (n && (!rays || !keys)))
        return rtc_fail(RTC_EINVAL, "rtc_ray_keys_host: null argument");
    const RtcKeyBox box = key_box(lo, hi);
    for (size_t i = 0; i < n; ++i) {
        const float r[6] = {rays[i].pos.x, rays[i].pos.y, rays[i].pos.z, rays[i].dir.x, rays[i].dir.y, rays[i].dir.z};
        keys[i] = ray_key(r, box);
    }
    return 0;
}

extern "C" int rtc_ray_order_shape(int *keysPerGroup, int *scanGroups)
{
    if (!keysPerGroup || !scanGroups)
        return rtc_fail(RTC_EINVAL, "rtc_ray_order_shape: null argument");
    *keysPerGroup = kOrderKeysPerGroup;
    *scanGroups = kOrderScanGroups;
    return 0;
}

extern "C" size_t rtc_ray_order_scratch_bytes(size_t n)
{
    return order_scratch(n).words * sizeof(unsigned);
}

extern "C" int rtc_ray_order_async(const RtcDeviceScene *s, const Ray *dRays, size_t n, const float *bounds,
                                   unsigned *dOrder, unsigned *dKeys, void *dScratch, size_t scratchBytes, void *stream)
{
    const char *const who = "rtc_ray_order_async";
    if (const int rc = refuse_order(who, s, dRays, dOrder, n))
        return rc;
    if (const int rc = rtc_refuse_scratch(who, dScratch))
        return rc;
    if (scratchBytes < rtc_ray_order_scratch_bytes(n))
        return rtc_fail(RTC_EINVAL, "%s: %zu bytes of scratch, %zu rays need %zu (rtc_ray_order_scratch_bytes)", who,
                        scratchBytes, n, rtc_ray_order_scratch_bytes(n));
    if (n == 0)
        return 0;
    const RtcKeyBox box = bounds ? key_box(bounds, bounds + 3) : key_box(s->boundsLo, s->boundsHi);
    RtcDeviceGuard guard(s->device);
    if (!guard.ok())
        return rtc_fail(RTC_ENODEV, "%s: cannot select the scene's device %d", who, s->device);
    const RtcOrderScratch L = order_scratch(n);
    unsigned *const w = (unsigned *)dScratch;
    unsigned *const keys[2] = {w + L.keys0, w + L.keys1};
    unsigned *const idx[2] = {dOrder, w + L.idx}; /* pass p reads idx[p & 1] (p > 0) and writes idx[(p + 1) & 1] */
    unsigned *const hist = w + L.hist, *const totals = w + L.totals;
    const hipStream_t st = (hipStream_t)stream;
    const dim3 block(kOrderBlock), groups((unsigned)L.groups);
    const unsigned un = (unsigned)n, ug = (unsigned)L.groups;
    hipLaunchKernelGGL(rtc_rsort_keys, dim3((unsigned)((n + kOrderBlock - 1) / kOrderBlock)), block, 0, st,
                       (const float *)dRays, un, box, keys[0], dKeys);
    for (int p = 0; p < kOrderPasses; ++p) {
        const int shift = p * kOrderDigitBits;
        const unsigned *kin = keys[p & 1], *iin = idx[p & 1];
        unsigned *kout = keys[(p + 1) & 1], *iout = idx[(p + 1) & 1];
        hipLaunchKernelGGL(rtc_rsort_hist, groups, block, 0, st, kin, un, shift, ug, hist);
        hipLaunchKernelGGL(rtc_rsort_scan, dim3(kOrderRadix), block, 0, st, hist, ug, totals);
        /* the first pass, the last, the ones between (in the order the kernels are emitted in) */
        static constexpr decltype(&rtc_rsort_scatter<true, false>) kScatter[3] = {
            rtc_rsort_scatter<true, false>, rtc_rsort_scatter<false, true>, rtc_rsort_scatter<false, false>};
        hipLaunchKernelGGL(kScatter[p == 0 ? 0 : p == kOrderPasses - 1 ? 1 : 2], groups, block, 0, st, kin, iin, un, shift,
                           ug, hist, totals, kout, iout);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int rtc_ray_order(const RtcDeviceScene *s, const Ray *rays, size_t n, const float *bounds, unsigned *order,
                             unsigned *keys)
{
    const char *const who = "rtc_ray_order";
    if (const int rc = refuse_order(who, s, rays, order, n))
        return rc;
    if (n == 0)
        return 0;
    const Staged items[4] = {{rays, nullptr, n * sizeof(Ray), true},
                             {nullptr, order, n * sizeof(unsigned), true},
                             {nullptr, keys, n * sizeof(unsigned), keys != nullptr},
                             {nullptr, nullptr, rtc_ray_order_scratch_bytes(n), true}};
    return staged_query(who, s, items, [&](void *const *dev) {
        return rtc_ray_order_async(s, (const Ray *)dev[0], n, bounds, (unsigned *)dev[1], (unsigned *)dev[2], dev[3],
                                   items[3].bytes, nullptr);
    });
}

extern "C" int rtc_gather_async(void *dDst, const void *dSrc, const unsigned *dOrder, size_t n, size_t elemBytes,
                                void *stream)
{
    return permute<false>("rtc_gather_async", dDst, dSrc, dOrder, n, elemBytes, stream);
}

extern "C" int rtc_scatter_async(void *dDst, const void *dSrc, const unsigned *dOrder, size_t n, size_t elemBytes,
                                 void *stream)
{
    return permute<true>("rtc_scatter_async", dDst, dSrc, dOrder, n, elemBytes, stream);
}
