/*
 * rtc_select.hip -- the device side of an adaptively sampled frame: the selection statement (select_pixel:
 * one statement, compiled for the host and for the device), the stable compaction that turns it into the next pixel
 * list of rtc_render_pixels_async (rtc_select_pixels_async: judge, scan, emit; rtc_select_pixels_host states the same
 * sequence semantics without a GPU) and the final normalise-and-quantise (rtc_resolve_async, rtc_resolve_host).  No
 * reference counterpart: the reference gives every pixel the same number of samples (main.c:98-99).
 * The render kernels (rtc_render.hip) are not involved, no scene is named and the launch planner takes no part: the
 * entries work on the current device, like rtc_gather_async.
 */
#include <hip/hip_runtime.h>

#include "../../include/rtc.h"
#include "rtc_device.h"
#include "rtc_internal.h"
#include "rtc_hip_util.h"
#include "rtc_pass_util.h"

/* ---- the select's shape (rtc_select_shape gives T and G; raytracingc_amd/_abi.py mirrors them as constants and
 * tests/test_select_abi.py compares the two) ---- */
constexpr int kSelBlock = 256;                          /* threads of every kernel below: 4 waves */
constexpr int kSelWaves = kSelBlock / 64;
constexpr int kSelRounds = 8;                           /* entries per lane: one ballot word per wave and round */
constexpr int kSelWordsPerWave = kSelRounds;
constexpr int kSelWordsPerTile = kSelWaves * kSelRounds; /* 32 */
constexpr int kSelTile = kSelBlock * kSelRounds;        /* T = 2048 entries per workgroup */
constexpr int kSelScanGroups = kSelBlock;               /* G = 256: tile counts the scan workgroup takes per step */
constexpr unsigned kSelSentinel = 0xFFFFFFFFu;
static_assert(kSelWordsPerTile <= 64, "one wave scans a tile's word counts");

/* ---- the selection: this one statement is compiled for the host (rtc_select_pixels_host) and for the device
 * (rtc_select_judge).  f32 operation by operation (the translation unit is built with -ffp-contract=off).  The comparison
 * is strict and false for any NaN. */
__host__ __device__ inline bool select_pixel(const float A[3], const float P[3], const RtcSelectDesc &s)
{
    const float ex = __builtin_fabsf(A[0] * s.wAccum - P[0] * s.wPrev);
    const float ey = __builtin_fabsf(A[1] * s.wAccum - P[1] * s.wPrev);
    const float ez = __builtin_fabsf(A[2] * s.wAccum - P[2] * s.wPrev);
    const float d = (ex + ey) + ez;
    const float l = ((A[0] + A[1]) + A[2]) * s.wLevel;
    return d * d > s.threshold * (l + s.floor);
}

/* ---- kernels ------------------------------------------------------------------------------------------------------ */
/* Judge.  Workgroup g takes entries [g T, (g + 1) T), wave w of it [g T + 512 w, + 512), 64 consecutive entries a round.
 * Entry i names pixel p = in[i] (LIST) or i; a valid one (i < n and p < pixels) is judged and stamped.  Each round's
 * predicate is one ballot word, stored at mask[i / 64] by lane 0 -- every word below ceil(n / 64) is written, the lanes
 * past n as zeros -- and the tile's number of selected entries goes to counts[g]. */
template <bool LIST>
__global__ __launch_bounds__(kSelBlock) void rtc_select_judge(const float *__restrict__ accum,
                                                                const float *__restrict__ prev, unsigned pixels,
                                                                const unsigned *__restrict__ in, unsigned n,
                                                                RtcSelectDesc sel, unsigned long long *__restrict__ mask,
                                                                unsigned *__restrict__ counts, int *__restrict__ samples)
{
    __shared__ unsigned waveCount[kSelWaves];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const unsigned base = blockIdx.x * (unsigned)kSelTile + (unsigned)(wave * 64 * kSelRounds);
    unsigned count = 0;
#pragma unroll
    for (int r = 0; r < kSelRounds; ++r) {
        const unsigned first = base + (unsigned)(r * 64); /* (wave-uniform) */
        if (first >= n)
            break;
        const unsigned i = first + (unsigned)lane;
        unsigned p = kSelSentinel;
        if (i < n)
            p = LIST ? in[i] : i;
        const bool ok = p < pixels; /* (i >= n: the sentinel, which is no pixel: pixels <= 0x7fffffff) */
        bool chosen = false;
        if (ok) {
            const float *a = accum + (size_t)p * 3, *q = prev + (size_t)p * 3;
            const float A[3] = {a[0], a[1], a[2]}, P[3] = {q[0], q[1], q[2]};
            chosen = select_pixel(A, P, sel);
            if (samples)
                samples[p] = sel.samplesDone;
        }
        const unsigned long long word = __ballot(chosen);
        if (lane == 0)
            mask[first >> 6] = word;
        count += (unsigned)__popcll(word);
    }
    if (lane == 0)
        waveCount[wave] = count;
    __syncthreads();
    if (t == 0) {
        unsigned sum = 0;
#pragma unroll
        for (int w = 0; w < kSelWaves; ++w)
            sum += waveCount[w];
        counts[blockIdx.x] = sum;
    }
}

/* Scan.  One workgroup turns counts[0, groups) into its exclusive prefix in place, kSelScanGroups counts a step with the
 * running sum carried (as rtc_rsort_scan does), and leaves the total in *total (the emit kernel's) and, where given, in
 * *userCount.  groups == 0: both become 0. */
__global__ __launch_bounds__(kSelBlock) void rtc_select_scan(unsigned *__restrict__ counts, unsigned groups,
                                                              unsigned *__restrict__ total,
                                                              unsigned long long *__restrict__ userCount)
{
    __shared__ unsigned waveSum[kSelWaves];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    unsigned carry = 0;
    for (unsigned c = 0; c < groups; c += (unsigned)kSelScanGroups) {
        const unsigned g = c + (unsigned)t;
        const unsigned v = g < groups ? counts[g] : 0u;
        unsigned sum;
        const unsigned excl = rtc_block_scan<kSelWaves>(v, waveSum, lane, wave, sum);
        if (g < groups)
            counts[g] = carry + excl;
        carry += sum;
    }
    if (t == 0) {
        *total = carry;
        if (userCount)
            *userCount = carry;
    }
}

/* Emit.  Workgroup g < groups re-reads its tile's ballot words, the tile's offset and the input entries: a selected entry's
 * place = the tile's offset + the selected entries of the tile's earlier words (a prefix over the 32 word counts, made by
 * wave 0 and handed on in LDS) + the selected lanes below it in its own word (mbcnt) -- ascending input position, so
 * the output is the input's subsequence.  A place >= capacity is not stored.  Every workgroup also writes its share of the
 * sentinel tail out[min(total, capacity), capacity): the grid holds at least ceil(capacity / T) workgroups. */
template <bool LIST>
__global__ __launch_bounds__(kSelBlock) void rtc_select_emit(const unsigned *__restrict__ in, unsigned n, unsigned groups,
                                                               const unsigned long long *__restrict__ mask,
                                                               const unsigned *__restrict__ offsets,
                                                               const unsigned *__restrict__ total,
                                                               unsigned *__restrict__ out, unsigned capacity)
{
    __shared__ unsigned long long tileWord[kSelWordsPerTile];
    __shared__ unsigned wordBase[kSelWordsPerTile];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const unsigned selected = *total;
    { /* the sentinel tail: places start + [b T, (b + 1) T) below capacity */
        const unsigned start = selected < capacity ? selected : capacity;
        const unsigned long long lo = (unsigned long long)start + (unsigned long long)blockIdx.x * kSelTile;
        const unsigned long long hi = lo + kSelTile < capacity ? lo + kSelTile : capacity;
        for (unsigned long long k = lo + (unsigned)t; k < hi; k += kSelBlock)
            out[k] = kSelSentinel;
    }
    if (blockIdx.x >= groups)
        return;
    const unsigned offset = offsets[blockIdx.x];
    if (offset >= capacity) /* (workgroup-uniform) every place of the tile is cut */
        return;
    const unsigned words = (n + 63u) >> 6;
    const unsigned firstWord = blockIdx.x * (unsigned)kSelWordsPerTile;
    if (wave == 0) {
        unsigned long long w = 0;
        if (lane < kSelWordsPerTile && firstWord + (unsigned)lane < words)
            w = mask[firstWord + (unsigned)lane];
        const unsigned c = (unsigned)__popcll(w);
        unsigned incl = c;
#pragma unroll
        for (int o = 1; o < kSelWordsPerTile; o <<= 1) {
            const unsigned u = __shfl_up(incl, o);
            if (lane >= o)
                incl += u;
        }
        if (lane < kSelWordsPerTile) {
            tileWord[lane] = w;
            wordBase[lane] = offset + incl - c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kSelRounds; ++r) {
        const int j = wave * kSelWordsPerWave + r;
        const unsigned long long w = tileWord[j];
        if (!((w >> lane) & 1ull))
            continue;
        const unsigned below = __builtin_amdgcn_mbcnt_hi((unsigned)(w >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)w, 0u));
        const unsigned place = wordBase[j] + below;
        if (place < capacity) {
            const unsigned i = (firstWord + (unsigned)j) * 64u + (unsigned)lane; /* (< n: only valid entries are set) */
            out[place] = LIST ? in[i] : i;
        }
    }
}

/* Resolve.  Byte k of the Color buffer is component k % 3 of pixel k / 3, from accumulator float k: thread g takes the
 * aligned dword g of the buffer (four floats in, one dword out); the bytes before the first aligned dword and after the
 * last are stored singly by the first threads.  head: the bytes before the first aligned dword (0 .. 3, at most `bytes`). */
__device__ inline unsigned resolve_byte(const float *__restrict__ accum, const int *__restrict__ samples, float fspp,
                                        size_t k)
{
    return (unsigned)rtcdev::float_to_u8(accum[k] * rtc_sample_scale(fspp, samples[k / 3]));
}
__global__ __launch_bounds__(kSelBlock) void rtc_resolve_colors(const float *__restrict__ accum,
                                                                 const int *__restrict__ samples, float fspp,
                                                                 unsigned char *__restrict__ colors, size_t bytes,
                                                                 unsigned head, size_t dwords)
{
    const size_t g = blockIdx.x * (size_t)kSelBlock + threadIdx.x;
    if (g < dwords) {
        const size_t k = head + 4 * g;
        const unsigned b0 = resolve_byte(accum, samples, fspp, k), b1 = resolve_byte(accum, samples, fspp, k + 1),
                       b2 = resolve_byte(accum, samples, fspp, k + 2), b3 = resolve_byte(accum, samples, fspp, k + 3);
        *(unsigned *)(colors + k) = b0 | b1 << 8 | b2 << 16 | b3 << 24;
    }
    if (g < head)
        colors[g] = (unsigned char)resolve_byte(accum, samples, fspp, g);
    const size_t tailAt = head + 4 * dwords;
    if (g < bytes - tailAt)
        colors[tailAt + g] = (unsigned char)resolve_byte(accum, samples, fspp, tailAt + g);
}

/* ---- the select's scratch: the ballot words (one u64 per 64 entries), the tile counts / offsets and the total, each
 * region a multiple of 16 bytes */
struct RtcSelectScratch {
    size_t groups, maskWords, counts, total, bytes; /* counts, total: byte offsets */
};
static RtcSelectScratch select_scratch(size_t n)
{
    RtcSelectScratch L;
    L.groups = (n + kSelTile - 1) / kSelTile;
    L.maskWords = (n + 63) / 64;
    L.counts = (L.maskWords * 8 + 15) / 16 * 16;
    L.total = L.counts + (L.groups * 4 + 15) / 16 * 16;
    L.bytes = L.total + 16;
    return L;
}

/* the refusals the device entry and the host statement share */
static int refuse_select(const char *who, const float *accum, const float *prev, size_t pixelCount, const unsigned *in,
                         size_t nIn, const RtcSelectDesc *sel, const unsigned *out, size_t capacity,
                         const unsigned long long *count, const int *samples)
{
    if (!accum || !prev || !sel)
        return rtc_fail(RTC_EINVAL, "%s: null accumulator, snapshot or desc", who);
    if (pixelCount > (size_t)0x7fffffff || nIn > (size_t)0x7fffffff || capacity > (size_t)0x7fffffff)
        return rtc_fail(RTC_EINVAL, "%s: %zu pixels, %zu entries, capacity %zu (each at most 2147483647)", who, pixelCount,
                        nIn, capacity);
    if (!in && nIn != 0)
        return rtc_fail(RTC_EINVAL, "%s: no input list, but %zu entries (without a list the input is every pixel: 0)", who,
                        nIn);
    if (!out && capacity != 0)
        return rtc_fail(RTC_EINVAL, "%s: no output list, but a capacity of %zu", who, capacity);
    if (!out && !count && !samples)
        return rtc_fail(RTC_EINVAL, "%s: no output: list, count and samples are all null", who);
    if (out && out == in)
        return rtc_fail(RTC_EINVAL, "%s: the output list is the input list", who);
    if (samples && sel->samplesDone < 0)
        return rtc_fail(RTC_EINVAL, "%s: samplesDone = %d to stamp", who, sel->samplesDone);
    return 0;
}

extern "C" int rtc_select_shape(int *entriesPerGroup, int *scanGroups)
{
    if (!entriesPerGroup || !scanGroups)
        return rtc_fail(RTC_EINVAL, "rtc_select_shape: null argument");
    *entriesPerGroup = kSelTile;
    *scanGroups = kSelScanGroups;
    return 0;
}

extern "C" size_t rtc_select_scratch_bytes(size_t nIn)
{
    return select_scratch(nIn).bytes;
}

extern "C" int rtc_select_pixels_async(const float *dAccum, const float *dPrev, size_t pixelCount, const unsigned *dIn,
                                       size_t nIn, const RtcSelectDesc *sel, unsigned *dOut, size_t capacity,
                                       unsigned long long *dCount, int *dSamples, void *dScratch, size_t scratchBytes,
                                       void *stream)
{
    const char *const who = "rtc_select_pixels_async";
    if (const int rc = refuse_select(who, dAccum, dPrev, pixelCount, dIn, nIn, sel, dOut, capacity, dCount, dSamples))
        return rc;
    const size_t n = dIn ? nIn : pixelCount; /* the input sequence's length */
    if (const int rc = rtc_refuse_scratch(who, dScratch))
        return rc;
    if (scratchBytes < rtc_select_scratch_bytes(n))
        return rtc_fail(RTC_EINVAL, "%s: %zu bytes of scratch, %zu entries need %zu (rtc_select_scratch_bytes)", who,
                        scratchBytes, n, rtc_select_scratch_bytes(n));
    const RtcSelectScratch L = select_scratch(n);
    unsigned long long *const mask = (unsigned long long *)dScratch;
    unsigned *const counts = (unsigned *)((char *)dScratch + L.counts);
    unsigned *const total = (unsigned *)((char *)dScratch + L.total);
    const hipStream_t st = (hipStream_t)stream;
    const dim3 block(kSelBlock);
    const unsigned un = (unsigned)n, ug = (unsigned)L.groups, up = (unsigned)pixelCount, cap = (unsigned)capacity;
    if (ug)
        hipLaunchKernelGGL(dIn ? rtc_select_judge<true> : rtc_select_judge<false>, dim3(ug), block, 0, st, dAccum, dPrev, up,
                           dIn, un, *sel, mask, counts, dSamples);
    if (dCount || cap)
        hipLaunchKernelGGL(rtc_select_scan, dim3(1), block, 0, st, counts, ug, total, dCount);
    if (cap) {
        const unsigned tailGroups = (cap + (unsigned)kSelTile - 1) / (unsigned)kSelTile;
        const dim3 grid(ug > tailGroups ? ug : tailGroups);
        hipLaunchKernelGGL(dIn ? rtc_select_emit<true> : rtc_select_emit<false>, grid, block, 0, st, dIn, un, ug, mask,
                           counts, total, dOut, cap);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int rtc_select_pixels_host(const float *accum, const float *prev, size_t pixelCount, const unsigned *in,
                                      size_t nIn, const RtcSelectDesc *sel, unsigned *out, size_t capacity,
                                      unsigned long long *count, int *samples)
{
    if (const int rc = refuse_select("rtc_select_pixels_host", accum, prev, pixelCount, in, nIn, sel, out, capacity, count,
                                     samples))
        return rc;
    const size_t n = in ? nIn : pixelCount;
    size_t selected = 0;
    for (size_t i = 0; i < n; ++i) {
        const size_t p = in ? in[i] : i;
        if (p >= pixelCount)
            continue;
        if (samples)
            samples[p] = sel->samplesDone;
        if (select_pixel(accum + 3 * p, prev + 3 * p, *sel)) {
            if (selected < capacity)
                out[selected] = (unsigned)p;
            ++selected;
        }
    }
    for (size_t k = selected; k < capacity; ++k)
        out[k] = kSelSentinel;
    if (count)
        *count = selected;
    return 0;
}

static int refuse_resolve(const char *who, const void *accum, const void *samples, size_t pixelCount, int spp,
                          const void *colors)
{
    if (!accum || !samples || !colors)
        return rtc_fail(RTC_EINVAL, "%s: null pointer", who);
    if (spp <= 0)
        return rtc_fail(RTC_EINVAL, "%s: spp = %d", who, spp);
    if (pixelCount > (size_t)0x7fffffff)
        return rtc_fail(RTC_EINVAL, "%s: %zu pixels (at most 2147483647 in one call)", who, pixelCount);
    return 0;
}

extern "C" int rtc_resolve_async(const float *dAccum, const int *dSamples, size_t pixelCount, int spp, void *dColors,
                                 void *stream)
{
    if (const int rc = refuse_resolve("rtc_resolve_async", dAccum, dSamples, pixelCount, spp, dColors))
        return rc;
    if (pixelCount == 0)
        return 0;
    const size_t bytes = 3 * pixelCount;
    size_t head = (size_t)(-(ptrdiff_t)(size_t)dColors) & 3;
    if (head > bytes)
        head = bytes;
    const size_t dwords = (bytes - head) / 4;
    const size_t threads = dwords > 3 ? dwords : 3; /* (the head and the tail: at most 3 bytes each) */
    hipLaunchKernelGGL(rtc_resolve_colors, dim3((unsigned)((threads + kSelBlock - 1) / kSelBlock)), dim3(kSelBlock), 0,
                       (hipStream_t)stream, dAccum, dSamples, (float)spp, (unsigned char *)dColors, bytes, (unsigned)head,
                       dwords);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int rtc_resolve_host(const float *accum, const int *samples, size_t pixelCount, int spp, void *colors)
{
    if (const int rc = refuse_resolve("rtc_resolve_host", accum, samples, pixelCount, spp, colors))
        return rc;
    const float fspp = (float)spp;
    for (size_t p = 0; p < pixelCount; ++p) {
        const float scale = rtc_sample_scale(fspp, samples[p]);
        const float v[3] = {accum[3 * p] * scale, accum[3 * p + 1] * scale, accum[3 * p + 2] * scale};
        if (const int rc = rtc_quantize(v, 1, (Color *)colors + p)) /* the host's floatToUint */
            return rc;
    }
    return 0;
}
