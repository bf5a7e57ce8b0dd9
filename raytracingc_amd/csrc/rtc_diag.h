/* rtc_diag.h -- the diagnostic build's buffers, its rtc_diag_* entry points and the stamp macros the kernels carry
 * (RTC_DIAG: librtc_diag.so; empty macros otherwise).
 * A section of rtc_render.hip's translation unit: included there once, after the headers above it in that file's
 * list (it uses their names, and rtcdev's through the file's using-directive). */
#pragma once

#ifdef RTC_DIAG
/* diagnostic build only (librtc_diag.so): per-wave {cycles, wave-loop iterations, start stamp, cycles inside
 * closest_hit} */
__device__ unsigned long long *g_rtc_diag = nullptr;
extern "C" int rtc_diag_set_buffer(void *dptr)
{
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_rtc_diag), &dptr, sizeof dptr));
    return 0;
}
/* heavy-kernel section cycles (s_memtime deltas summed over waves): 0 primary trace, 1 cluster tests,
 * 2 general filter loop, 3 general exact loop, 4 lane reduction, 5 hit shading, 6 sky (miss), 7 loop total */
constexpr int kDiagSects = 28;
__device__ unsigned long long g_rtc_sect[kDiagSects]; /* [8..12] window statistics (rtc_render_chain) */
/* rtc_render_chain's diagnostics, written with plain stores to per-wave-slot / per-item addresses (no same-address global
 * atomics: thousands of them queued at a kernel's end held up other waves' memory operations behind them in the L2
 * channels and made the tail look slow):
 *   g_rtc_wavelog[slot]: start, end, items, the end of items 1..5 (s_memrealtime, the 100 MHz constant clock);
 *   g_rtc_sectw[slot]: the wave's section cycles (s_rtc_sect) and window statistics, summed by rtc_diag_sections;
 *   g_rtc_itemlog[item]: (start, end), (windows | tile candidates << 16 | wave slot << 32), (bounce iterations |
 *     Box-Muller fallback lanes << 16 | triangle tests of the window lanes << 32, RTC_DIAG_COUNT builds only);
 *   g_rtc_itemsect[item]: the item's cycles in sections kItemSectIds (s_memtime deltas). */
constexpr int kWaveLog = 16384, kWaveLogCols = 8;
__device__ unsigned long long g_rtc_wavelog[kWaveLog][kWaveLogCols];
__device__ unsigned long long g_rtc_sectw[kWaveLog][kDiagSects];
constexpr int kItemLog = 1 << 18, kItemSectLog = 1 << 17, kItemSects = 16;
__device__ unsigned long long g_rtc_itemlog[kItemLog][4];
__device__ unsigned g_rtc_itemsect[kItemSectLog][kItemSects];
__device__ __forceinline__ int item_sect_id(int k) /* the sections of g_rtc_itemsect's columns */
{
    return k < 10 ? k : (k == 10 ? 14 : k + 4); /* columns 0..9: sections 0..9; 10: 14; 11..15: 15..19 */
}
template <typename T> static int diag_zero(const T &sym)
{
    void *p = nullptr;
    HIP_TRY(hipGetSymbolAddress(&p, HIP_SYMBOL(sym)));
    HIP_TRY(hipMemset(p, 0, sizeof(T)));
    return 0;
}
extern "C" int rtc_diag_itemlog(unsigned long long *out, int maxItems)
{
    const int n = std::min(maxItems, kItemLog);
    if (out && n > 0)
        HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rtc_itemlog), (size_t)n * 4 * sizeof(unsigned long long)));
    return n;
}
extern "C" int rtc_diag_itemsect(unsigned *out, int maxItems)
{
    const int n = std::min(maxItems, kItemSectLog);
    if (out && n > 0)
        HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rtc_itemsect), (size_t)n * kItemSects * sizeof(unsigned)));
    return n;
}
/* the wave records of the last launches (rows with a zero start: no wave); returns the slots copied */
extern "C" int rtc_diag_wavelog(unsigned long long *out, int maxWaves, int reset)
{
    const int n = std::min(maxWaves, kWaveLog);
    if (out && n > 0)
        HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rtc_wavelog), (size_t)n * kWaveLogCols * sizeof(unsigned long long)));
    if (reset && diag_zero(g_rtc_wavelog))
        return -1;
    return n;
}
#define CSTAMP(v) const unsigned long long v = __builtin_amdgcn_s_memtime()
/* per-block records of rtc_tile_cull (wave 0): {start, level 1 done, end, geometry, level-2 prefilter cycles, candidate
 * loop cycles, candidates, 0}, written with plain stores into the buffer rtc_diag_set_cull_buffer names (null: none) */
__device__ unsigned long long *g_rtc_cullwg = nullptr;
extern "C" int rtc_diag_set_cull_buffer(void *dptr)
{
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_rtc_cullwg), &dptr, sizeof dptr));
    return 0;
}
#define CREC(blk, a, b, c, geo, pre, loop, cand)                                                              \
    do {                                                                                                       \
        if (g_rtc_cullwg && threadIdx.x == 0) {                                                                \
            unsigned long long *r_ = g_rtc_cullwg + (size_t)(blk) * 8;                                         \
            r_[0] = (a), r_[1] = (b), r_[2] = (c), r_[3] = (geo), r_[4] = (pre), r_[5] = (loop), r_[6] = (cand); \
        }                                                                                                      \
    } while (0)
__shared__ unsigned long long s_rtc_sect[4][kDiagSects]; /* [wave][section]: 0..7, 13..27 (rtc_render_chain) */
#define DSECT_BEGIN(v) const unsigned long long v = __builtin_amdgcn_s_memtime()
#define DSECT_END(v, k)                                                                                        \
    do {                                                                                                       \
        const unsigned long long dsectNow = __builtin_amdgcn_s_memtime();                                      \
        if ((threadIdx.x & 63) == __builtin_amdgcn_readfirstlane(threadIdx.x & 63))                           \
            s_rtc_sect[threadIdx.x >> 6][k] += dsectNow - (v);                                                 \
    } while (0)
/* Uniform section marks: the cycles since the previous mark of the wave go to section k.  Placed at wave-uniform points
 * only, the marks tile the loop: every cycle between the kernel's first mark and its last lands in exactly one section
 * (the BEGIN/END pairs above nest inside them) */
#define DMARK_INIT(v) unsigned long long v = __builtin_amdgcn_s_memtime()
#define DMARK(v, k)                                                                                            \
    do {                                                                                                       \
        const unsigned long long dmarkNow = __builtin_amdgcn_s_memtime();                                      \
        if ((threadIdx.x & 63) == __builtin_amdgcn_readfirstlane(threadIdx.x & 63))                           \
            s_rtc_sect[threadIdx.x >> 6][k] += dmarkNow - (v);                                                 \
        (v) = dmarkNow;                                                                                        \
    } while (0)
extern "C" int rtc_diag_sections(unsigned long long *out, int reset)
{
    /* out: kDiagSects (28) counters */
    if (out) {
        HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rtc_sect), kDiagSects * sizeof(unsigned long long)));
        std::vector<unsigned long long> w((size_t)kWaveLog * kDiagSects);
        HIP_TRY(hipMemcpyFromSymbol(w.data(), HIP_SYMBOL(g_rtc_sectw), w.size() * sizeof(unsigned long long)));
        for (size_t i = 0; i < w.size(); ++i)
            out[i % kDiagSects] += w[i];
    }
    if (reset) {
        unsigned long long z[kDiagSects] = {0};
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_rtc_sect), z, sizeof z));
        if (diag_zero(g_rtc_sectw))
            return -1;
    }
    return 0;
}
#else
#define DSECT_BEGIN(v) (void)0
#define DSECT_END(v, k) (void)0
#define DMARK_INIT(v) (void)0
#define DMARK(v, k) (void)0
#define CSTAMP(v) (void)0
#define CREC(blk, a, b, c, geo, pre, loop, cand) (void)0
#endif
