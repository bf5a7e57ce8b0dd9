/*
 * rtc_render.hip -- the MI355X render path behind include/rtc.h.
 *
 * Replaces the reference's render region main.c:263-304: rowThread (main.c:81-104) fanned out over 12
 * pthreads, each pixel running accumulationCount x calcColor (raytracing.c:262-296) over a brute-force
 * calculateRayCollision (raytracing.c:216-240).
 *
 * Design:
 *  - one lane per pixel, a 256-thread workgroup = 16x16 pixels, each wave an 8x8 tile (coherent primary
 *    rays for the wave-uniform early-outs);
 *  - each lane runs its pixel's samples sequentially (the RNG state x + y*W advances across samples,
 *    main.c:95, so samples of one pixel cannot be split) as a segment state machine: every iteration of
 *    the wave loop is ONE closest-hit query for every live lane, so the triangle loop is always
 *    wave-uniform and triangles are read with scalar loads (SGPR operands, no LDS/VGPR traffic);
 *  - triangles are stored with the edges AB, AC precomputed (bit-exact: the same f32 subtraction);
 *  - quantisation (vec3ToColor) is fused; the float accumulator is written only when asked for.
 *
 * Here: the error API, the launch code (which kernel variant a launch runs, and the planned operations' execution), the
 * frame copy kernels and the list that fixes the order of the device code.  The render kernels are sections of this
 * translation unit, included below.
 */
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#ifdef RTC_DIAG
__device__ unsigned g_rtc_bmfall[65536]; /* Box-Muller exact fallbacks per wave slot (diagnostic builds) */
#endif

#include "../../include/rtc.h"
#include "rtc_layout.h"
#include "rtc_internal.h"
#include "rtc_hip_util.h"
#include "rtc_staged.h"

static_assert(sizeof(vec3) == 12, "vec3 layout");
static_assert(sizeof(Material) == 20, "Material layout");
static_assert(sizeof(Sphere) == 36, "Sphere layout");
static_assert(sizeof(Triangle) == 68, "Triangle layout");
static_assert(sizeof(Scene) == 56, "Scene layout");
static_assert(sizeof(Color) == 3, "Color layout");
static_assert(sizeof(Ray) == 24, "Ray layout");
static_assert(sizeof(RtcRenderDesc) == 36, "RtcRenderDesc layout (ctypes mirror: raytracingc_amd/_abi.py)");

using namespace rtcdev;

/* ---- errors ---------------------------------------------------------------------------------------- */
static thread_local char g_err[1024] = "";

extern "C" int rtc_fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

extern "C" void rtc_log(int level, const char *fmt, ...)
{
    const char *v = getenv("RTC_VERBOSE");
    if (!v || atoi(v) < level)
        return;
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
}

extern "C" const char *rtc_last_error(void) { return g_err; }
extern "C" const char *rtc_version(void) { return "rtc-mi355x 0.1 (gfx950)"; }


extern "C" int rtc_device_count(int *count)
{
    if (!count)
        return rtc_fail(RTC_EINVAL, "null count");
    *count = 0;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return rtc_fail(RTC_ENODEV, "no HIP device: %s", hipGetErrorString(e));
    *count = n;
    return 0;
}

/* ---- the kernels, by concern; in this order (each uses the ones before it) ------------------------------ */
#include "rtc_params.h"
#include "rtc_closest.h"
#include "rtc_diag.h"
#include "rtc_cull.h"
#include "rtc_lane.h"
#include "rtc_sky.h"
#include "rtc_chain.h"
#include "rtc_first_hit.h"
#include "rtc_trace_rays.h"
#include "rtc_trace_paths.h"
#include "rtc_occluded.h"
#include "rtc_render_pixels.h"

/* A kernel launch whose completion also records `stop` (null: a plain launch): the event is the dispatch's own
 * completion signal, so the stream gets no separate marker packet -- each marker on the launch stream cost ~5-7 us
 * before the next kernel (round 3: a hipEventRecord after the launch) */
template <typename... K, typename... A>
static hipError_t launch_stop(void (*k)(K...), dim3 g, dim3 b, size_t sh, hipStream_t st, hipEvent_t stop, A... args)
{
    if (stop) {
        hipExtLaunchKernelGGL(k, g, b, (std::uint32_t)sh, st, nullptr, stop, 0u, args...);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(k, g, b, sh, st, args...);
    return hipGetLastError();
}

/* ---- which instantiation of rtc_render_chain a launch runs ----------------------------------------------------
 * The template flags, in the template's order (their meaning: rtc_chain.h). */
struct ChainFlags {
    bool multi, count, hits, general, spheres, resume, draws;
    constexpr bool operator==(const ChainFlags &o) const
    {
        return multi == o.multi && count == o.count && hits == o.hits && general == o.general && spheres == o.spheres &&
               resume == o.resume && draws == o.draws;
    }
};

/* The launch's properties -> the flags.  `defer`: the launch may give items deferred sample slots, hoists the primary
 * segments or reads the primary filter records from global memory.  `hits`: the scene's bounces often hit again.  Only a
 * launch that is none of multi-chunk, counting, deferring, with spheres or a pass runs a kernel without the GENERAL code,
 * and only there does `hits` choose: both choices render the same frame, so only the static_asserts below and the
 * launch's report (rtc_scene_chain_report, which tests/test_gpu_chain_paths.py holds to the launch meant) notice a
 * wrong one.  `draws`: the launch uses the draw cache (rtcplan::Plan::draws, planned for launches without the GENERAL code
 * only); a GENERAL kernel never reads it. */
constexpr ChainFlags chain_flags(bool multi, bool count, bool defer, bool hits, bool spheres, bool resume,
                                 bool draws = false)
{
    const bool general = multi || count || defer || spheres || resume;
    return ChainFlags{multi, count, hits && !general, general, spheres, resume, draws && !general};
}

struct ChainVariant {
    ChainFlags flags;
    void (*kernel)(RenderParams);
};
#define CHAIN_ROW(...) ChainVariant{ChainFlags{__VA_ARGS__}, rtc_render_chain<__VA_ARGS__>}

/* the row of `table` with these flags; n: none */
template <int n> constexpr int chain_variant(const ChainVariant (&table)[n], ChainFlags f)
{
    for (int i = 0; i < n; ++i)
        if (table[i].flags == f)
            return i;
    return n;
}

/* `rule` for each of chain_flags' 128 inputs (`in`: one bit per parameter, below) and the flags it gives */
constexpr int kInMulti = 1, kInCount = 2, kInDefer = 4, kInHits = 8, kInSpheres = 16, kInResume = 32, kInDraws = 64;
template <typename Rule> constexpr bool every_chain_launch(Rule rule)
{
    for (int in = 0; in < 128; ++in)
        if (!rule(in, chain_flags(in & kInMulti, in & kInCount, in & kInDefer, in & kInHits, in & kInSpheres,
                                  in & kInResume, in & kInDraws)))
            return false;
    return true;
}
static_assert(every_chain_launch([](int in, ChainFlags f) { return f.general == ((in & ~(kInHits | kInDraws)) != 0); }),
              "GENERAL whenever the launch is multi-chunk, counting, deferring, with spheres or a pass");
static_assert(every_chain_launch([](int in, ChainFlags f) { return f.hits == ((in & ~kInDraws) == kInHits); }),
              "HITS only when none of them holds and the scene is hit-heavy");
static_assert(every_chain_launch([](int in, ChainFlags f) { return f.draws == (!!(in & kInDraws) && !f.general); }),
              "DRAWS only in the two kernels without GENERAL");
static_assert(every_chain_launch([](int in, ChainFlags f) {
                  return f.multi == !!(in & kInMulti) && f.count == !!(in & kInCount) &&
                         f.spheres == !!(in & kInSpheres) && f.resume == !!(in & kInResume);
              }),
              "MULTI, COUNT, SPHERES and RESUME are the launch's own");
static_assert(every_chain_launch([](int, ChainFlags f) { return !((f.hits || !f.general) && (f.spheres || f.resume)); }),
              "SPHERES and RESUME kernels are GENERAL ones without HITS");

#ifdef RTC_AB_NO_SLOTS
constexpr bool kAbNoSlots = true; /* timing experiment only (RTC_EXPERIMENT): deferred samples neither stored nor summed */
#else
constexpr bool kAbNoSlots = false;
#endif
/* One launch as its planned kernels see it */
struct Launch {
    const RtcDeviceScene *s;
    const rtcplan::Plan &pl;
    RenderParams P;
    int wgsPerCu;    /* the geometry kernel's workgroups per CU */
    size_t chainDyn; /* and its dynamic LDS */
    bool resume;     /* a pass (rtc_render_samples_async): the RESUME kernels */
    const RtcHitBuffers *hit = nullptr; /* a first-hit launch (rtc_render_first_hit_async): its buffers */
    DrawCache dc{};  /* a launch that uses the draw cache (pl.draws): the caching tile cull's and the fill's argument */
    dim3 grid() const { return dim3(pl.gridX, pl.gridY); } /* one 16x16 workgroup block each */
    /* every pointer into the scratch: a region the plan binds (rtcplan::Buf), in the launch's slot; unbound: null */
    template <typename T> T *region(int buf) const
    {
        return pl.binds(buf) ? (T *)(s->scratch + pl.slotOffset + pl.reg[buf].offset) : nullptr;
    }
};

/* `who`: the entry point, for the error texts.  `hit`: a first-hit launch (no Scene, its buffers in place of dColors; every
 * flag but RTC_F_NO_TILE_CULL refused). */
static int check_arguments(const char *who, const Scene *scene, const RtcCamera *cam, const RtcRenderDesc *d,
                           const void *dColors, const RtcHitBuffers *hit)
{
    if ((!scene && !hit) || !cam || !d || (!dColors && !hit))
        return rtc_fail(RTC_EINVAL, "%s: null argument", who);
    if (hit && !hit->prim && !hit->depth && !hit->normal && !hit->albedo)
        return rtc_fail(RTC_EINVAL, "%s: no buffer asked for (prim, depth, normal and albedo are all null)", who);
    const int geometry = rtcplan::geometry_error(*d);
    if (geometry == 1)
        return rtc_fail(RTC_EINVAL, "%s: bad geometry %dx%d rows %d+k*%d", who, d->width, d->height, d->rowStart,
                        d->rowStride);
    if (geometry)
        return rtc_fail(RTC_EINVAL, "frame too large");
    if (hit && (d->flags & ~RTC_F_NO_TILE_CULL))
        return rtc_fail(RTC_EINVAL, "%s: flags 0x%x (a first-hit launch takes RTC_F_NO_TILE_CULL and no other flag)", who,
                        d->flags);
    if (d->flags & (RTC_F_COOP4 | RTC_F_COOP8 | RTC_F_PIPE | RTC_F_SPEC))
        return rtc_fail(RTC_EINVAL, "%s: RTC_F_COOP4 / COOP8 / PIPE / SPEC name kernels that were "
                                    "removed (rtc_render_chain renders every geometry pixel)", who);
    return 0;
}

/* what the kernels read of the scene's shape, the launch's shape and the camera (the plan's buffers, the scene records
 * among them: bind_plan) */
static RenderParams render_params(const RtcDeviceScene *s, const Scene *scene, const RtcCamera &cam,
                                  const RtcRenderDesc &d, int rows, void *dColors, float *dAccum,
                                  unsigned long long *dSegments, const RtcSampleRange *range)
{
    RenderParams P;
    memset(&P, 0, sizeof P);
    P.triCount = s->triCount, P.triPadded = s->triPadded, P.maskWords = s->maskWords;
    P.sphereCount = d.trianglesOnly ? 0 : s->sphereCount;
    P.clusterCount = s->clusterCount;
    P.chunkCount = s->chunkCount, P.clusterCull = !(d.flags & RTC_F_NO_CLUSTER_CULL);
    P.colors = (unsigned char *)dColors, P.accum = dAccum;
    P.segments = dSegments, P.segSlots = s->segSlots;
    P.width = d.width, P.height = d.height;
    P.rows = rows, P.rowStart = d.rowStart, P.rowStride = d.rowStride;
    P.rowBandShift = d.rowBand > 1 ? __builtin_ctz((unsigned)d.rowBand) : 0;
    /* a pass renders range->count samples, each weighted by the frame's (float)(1. / accumulationCount) */
    P.spp = range ? range->count : d.spp, P.maxBounce = d.maxBounce;
    P.sampleFirst = range ? range->first : 0;
    P.hoist = (d.flags & RTC_F_HOIST_PRIMARY) ? 1 : 0;
    P.invSpp = d.spp > 0 ? (float)(1. / (double)d.spp) : 0.f;
    P.origin = v3(cam.origin), P.ex = v3(cam.ex), P.ey = v3(cam.ey), P.ez = v3(cam.ez), P.fov = cam.fov;
    if (scene) /* (a first-hit launch has none: its kernel evaluates no environment) */
        P.env = env_of(*scene);
    return P;
}

/* every slot of the scratch, or the sample slots (hipFree synchronises the device: no launch still reads the old ones) */
static int regrow(unsigned char *&buf, size_t &cap, size_t need)
{
    if (buf)
        HIP_TRY(hipFree(buf));
    buf = nullptr;
    cap = 0;
    HIP_TRY(hipMalloc(&buf, need));
    cap = need;
    return 0;
}

/* the second cull stream, the scratch and the sample slots the plan asks for */
static int grow_capacity(RtcDeviceScene *ms, const rtcplan::Plan &pl)
{
    if (pl.needCst2) { /* created on first use: whole frames keep three streams (one more costs them ~1 %) */
        int leastPrio = 0, greatestPrio = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&leastPrio, &greatestPrio));
        HIP_TRY(hipStreamCreateWithPriority(&ms->cst2, hipStreamNonBlocking, greatestPrio));
        ms->plan.cst2 = true;
    }
    if (const int rc = pl.scratchGrow ? regrow(ms->scratch, ms->plan.scratchCap, pl.scratchNeed) : 0)
        return rc;
    return pl.samplesGrow ? regrow(ms->samples, ms->plan.samplesCap, pl.samplesNeed) : 0;
}

/* the plan's buffers as RenderParams fields (the kernel arguments beside P: the run_ functions) */
static void bind_plan(Launch &L, int flags)
{
    const RtcDeviceScene *s = L.s;
    const rtcplan::Plan &pl = L.pl;
    RenderParams &P = L.P;
    const SceneRecords &g = s->gen[pl.gen]; /* the scene records of the generation the plan binds (kBufSceneGen) */
    P.tris = g.tris, P.mats = g.mats, P.spheres = g.spheres;
    P.clTris = g.clTris, P.clusters = g.clusters, P.chunks = g.chunks;
    P.primF = s->primF + (size_t)pl.half * s->primStride;
    P.primX = s->primX + (size_t)pl.half * s->primStride;
    P.blocksX = (int)pl.gridX;
    /* (read-only aliases of rtc_tile_cull's mask / pixMask arguments) */
    P.tileMask = L.region<unsigned long long>(rtcplan::kBufMask);
    P.pixMask = L.region<unsigned long long>(rtcplan::kBufPixMask);
    /* RTC_F_NO_REORDER: rtc_order_blocks still runs and writes the bound region; the render kernel takes raster order */
    P.order = (flags & RTC_F_NO_REORDER) ? nullptr : L.region<int>(rtcplan::kBufOrder);
    P.superMask = L.region<unsigned long long>(rtcplan::kBufSuperMask);
    P.superX = P.superMask ? (int)pl.superX : 0;
    P.geoList = L.region<unsigned>(rtcplan::kBufGeoList);
    P.pixItem = L.region<unsigned>(rtcplan::kBufPixItem);
    P.geoColor = L.region<unsigned>(rtcplan::kBufGeoColor);
    if (pl.binds(rtcplan::kBufGeoSet)) {
        P.geoCount = s->geoCounts + (size_t)pl.geoSet * kGeoSetInts;
        P.geoCountNext = s->geoCounts + (size_t)pl.geoSetNext * kGeoSetInts;
        P.geoCap = pl.geoCap;
        P.wideItems = pl.wideItems;
        P.cullPrio = pl.cullPrio;
    }
    if (pl.binds(rtcplan::kBufDrawTable) && pl.binds(rtcplan::kBufItemDraw)) { /* (rtc_draws_prepare has run) */
        const RtcDeviceScene::Draws &D = s->draws;
        L.dc.table = D.table, L.dc.ctr = D.ctr, L.dc.blockSeed = D.blockSeed, L.dc.pool = (float4 *)D.pool;
        L.dc.itemDraw = (unsigned *)(D.itemDraw + pl.itemDrawOffset);
        L.dc.capacity = (unsigned)D.capacity;
        L.dc.tablePixels = (unsigned)((size_t)P.width * (size_t)P.height);
        L.dc.parity = D.parity;
        /* the geometry kernel's two (in the deferred samples' places: a launch that uses the cache has no such slots) */
        P.drawPool = L.dc.pool;
        P.itemDraw = L.dc.itemDraw;
    }
    if (pl.binds(rtcplan::kBufSamples)) { /* (a pass: P.spp is its sample count, as the planner sized the slots) */
        P.sampleBuf = (SampleSlot *)s->samples;
        P.itemPix = (int *)(s->samples + (size_t)pl.sampleCap * (size_t)P.spp * sizeof(SampleSlot));
        P.sampleCap = pl.sampleCap;
    }
}

/* dynamic LDS of the geometry kernel: the clustered records (single-chunk scenes), then the primary filter records
 * when the block stays within its workgroups per CU */
/* whether a launch at wgsPerCu workgroups per CU stages the primary filter records (single-chunk scenes whose block stays
 * within its share of the CU's LDS) */
static bool chain_prim_f_staged(const RtcDeviceScene *s, int wgsPerCu)
{
    const size_t recLds = s->chunkCount <= 1 ? (size_t)soa_slots(s->clusterCount * kClusterSize) * sizeof(DevTri) : 0;
    const size_t pfLds = (size_t)s->triPadded * sizeof(DevPrimF);
    return s->chunkCount <= 1 && kChainStaticLds + recLds + pfLds <= kCuLds / (size_t)wgsPerCu;
}

/* rtcplan::Request::drawCache: the scene's part of "the launch runs a geometry kernel without the GENERAL code" -- the
 * cache is on, the scene is one chunk and its primary filter records are staged -- for whole frames (bit 0) and small
 * shares (bit 1), whose workgroups per CU differ */
static int draw_cache_eligible(const RtcDeviceScene *s)
{
    if (s->draws.blocks == 0 || s->triCount == 0)
        return 0;
    return (chain_prim_f_staged(s, s->chainWgsFull) ? 1 : 0) | (chain_prim_f_staged(s, RTC_CHAIN_WGS_SHARE) ? 2 : 0);
}

static void size_chain_lds(Launch &L)
{
    const RtcDeviceScene *s = L.s;
    L.wgsPerCu = L.pl.smallShare ? RTC_CHAIN_WGS_SHARE : s->chainWgsFull;
    const size_t recLds = s->chunkCount <= 1 ? (size_t)soa_slots(s->clusterCount * kClusterSize) * sizeof(DevTri) : 0;
    const size_t pfLds = (size_t)s->triPadded * sizeof(DevPrimF);
    L.P.chainPrimF = chain_prim_f_staged(s, L.wgsPerCu);
    const size_t floorLds = chain_lds_floor(L.wgsPerCu);
    L.chainDyn = std::max<size_t>(recLds + (L.P.chainPrimF ? pfLds : 0),
                                  floorLds > kChainStaticLds ? floorLds - kChainStaticLds : 0);
}

/* ---- one function per planned kernel, in rtcplan::Kernel's order (kPlanned): on stream `os`, completing `ev`.
 * A kernel family's variants stand in one table each, here; the order their device code is emitted in is the
 * instantiation list's, at the end of this file. */
static int run_prep(const Launch &L, hipStream_t os, hipEvent_t)
{
    const int n = L.s->triPadded;
    HIP_TRY(launch_stop(rtc_prep_primary, dim3((n + 8 + 63) / 64), dim3(64), 0, os, nullptr, L.P.tris,
                        const_cast<DevPrimF *>(L.P.primF), const_cast<DevPrimX *>(L.P.primX), n > 0 ? n + 8 : 0,
                        L.P.origin, L.pl.prepCounts ? L.P.geoCount : nullptr));
    return 0;
}

static int run_super_cull(const Launch &L, hipStream_t os, hipEvent_t)
{
    HIP_TRY(launch_stop(rtc_super_cull, dim3(L.pl.superX, L.pl.superY), dim3(64), 0, os, nullptr, L.P,
                        L.region<unsigned long long>(rtcplan::kBufSuperMask)));
    return 0;
}

static int run_tile_cull(const Launch &L, hipStream_t os, hipEvent_t ev)
{
    unsigned long long *const mask = L.region<unsigned long long>(rtcplan::kBufMask);
    unsigned long long *const pixMask = L.region<unsigned long long>(rtcplan::kBufPixMask);
    unsigned *const weight = L.region<unsigned>(rtcplan::kBufWeight);
    const size_t lds = (size_t)L.s->maskWords * sizeof(unsigned long long);
    const bool spheres = L.P.geoList && L.P.sphereCount > 0; /* the sphere split: sphere pixels are geometry pixels */
    static void (*const kCull[2])(RenderParams, unsigned long long *, unsigned *, unsigned long long *) = {
        rtc_tile_cull, rtc_tile_cull_sph<true>};
    if (L.pl.draws) {
        /* the draw cache: the caching cull, then the fill of the blocks it handed out -- two launches under the one planned
         * operation, whose completion event is the fill's: the sky pass forks and the next cull starts behind both.  The
         * fill's parity moves on once it is enqueued (a fill that was not leaves the mark where the next one reads it) */
        HIP_TRY(launch_stop(rtc_tile_cull_draws<true>, L.grid(), dim3(kBlock), lds, os, nullptr, L.P, mask, weight, pixMask,
                            L.dc));
        HIP_TRY(launch_stop(rtc_fill_draws<true>, dim3(kFillBlocks), dim3(256), 0, os, ev, L.dc));
        const_cast<RtcDeviceScene *>(L.s)->draws.parity ^= 1;
        return 0;
    }
    HIP_TRY(launch_stop(kCull[spheres], L.grid(), dim3(kBlock), lds, os, ev, L.P, mask, weight, pixMask));
    return 0;
}

static int run_sky(const Launch &L, hipStream_t os, hipEvent_t)
{
    const RenderParams &P = L.P;
    const bool wide = L.pl.smallShare && (size_t)P.width * (size_t)P.rows > 400000; /* four-wave workgroups */
    const bool general = P.geoColor || P.hoist || P.accum || P.segments;
    /* <kSkyWaves, GENERAL, RESUME>, by [wide][plain, general, a pass (which is GENERAL)] */
    static void (*const kSky[2][3])(RenderParams) = {
        {rtc_render_sky_rows<1, false>, rtc_render_sky_rows<1, true>, rtc_render_sky_rows<1, true, true>},
        {rtc_render_sky_rows<4, false>, rtc_render_sky_rows<4, true>, rtc_render_sky_rows<4, true, true>}};
    if (L.s->timing)
        HIP_TRY(hipEventRecord(L.s->evSky0, os));
    const dim3 grid((P.width + 63) / 64, wide ? (P.rows + 3) / 4 : P.rows);
    HIP_TRY(launch_stop(kSky[wide][L.resume ? 2 : general], grid, dim3(wide ? 256 : 64), 0, os, nullptr, P));
    if (L.s->timing)
        HIP_TRY(hipEventRecord(L.s->evSky1, os));
    return 0;
}

static int run_chain(const Launch &L, hipStream_t os, hipEvent_t ev)
{
    const RtcDeviceScene *s = L.s;
    const RenderParams &P = L.P;
    const dim3 cg((unsigned)(L.wgsPerCu * s->cuCount)), cb(kChainBlock);
    const bool multi = s->chunkCount > 1, count = P.segments != nullptr;
    const bool defer = P.sampleCap > 0 || P.hoist || !P.chainPrimF; /* (GENERAL) */
    const bool hits = s->chainWgsFull == RTC_CHAIN_WGS_HIT && RTC_CHAIN_WGS_HIT != RTC_CHAIN_WGS_FULL;
    /* <MULTI, COUNT, HITS, GENERAL, SPHERES, RESUME>: the two kernels without GENERAL; GENERAL for MULTI x COUNT, for
     * the sphere split and for a pass */
    static constexpr ChainVariant kChain[] = {
        CHAIN_ROW(false, false, false, false, false, false), CHAIN_ROW(false, false, true, false, false, false),
        CHAIN_ROW(false, false, false, true, false, false),  CHAIN_ROW(false, true, false, true, false, false),
        CHAIN_ROW(true, false, false, true, false, false),   CHAIN_ROW(true, true, false, true, false, false),
        CHAIN_ROW(false, false, false, true, true, false),   CHAIN_ROW(false, true, false, true, true, false),
        CHAIN_ROW(true, false, false, true, true, false),    CHAIN_ROW(true, true, false, true, true, false),
        CHAIN_ROW(false, false, false, true, false, true),   CHAIN_ROW(false, true, false, true, false, true),
        CHAIN_ROW(true, false, false, true, false, true),    CHAIN_ROW(true, true, false, true, false, true),
        CHAIN_ROW(false, false, false, true, true, true),    CHAIN_ROW(false, true, false, true, true, true),
        CHAIN_ROW(true, false, false, true, true, true),     CHAIN_ROW(true, true, false, true, true, true),
        /* the draw cache: the two kernels without GENERAL */
        CHAIN_ROW(false, false, false, false, false, false, true), CHAIN_ROW(false, false, true, false, false, false, true)};
    constexpr int kVariants = (int)(sizeof kChain / sizeof kChain[0]);
    static_assert(every_chain_launch([](int, ChainFlags f) { return chain_variant(kChain, f) < kVariants; }),
                  "every launch selects an instantiated kernel");
    const int variant =
        chain_variant(kChain, chain_flags(multi, count, defer, hits, P.sphereCount > 0, L.resume, L.pl.draws));
    if (kChain[variant].flags.draws != L.pl.draws) /* (the planner's conditions are chain_flags' and draw_cache_eligible's) */
        return rtc_fail(RTC_EINVAL, "rtc_render_chain: the launch was planned with the draw cache but runs a GENERAL kernel");
    { /* rtc_scene_chain_report: the row taken and size_chain_lds' choices (host stores only) */
        const ChainFlags &f = kChain[variant].flags;
        RtcChainReport &r = const_cast<RtcDeviceScene *>(s)->chainReport;
        r = RtcChainReport{f.multi,      f.count,    f.hits,          f.general,       f.spheres,     f.resume,
                           P.chainPrimF, L.wgsPerCu, (int)L.chainDyn, s->clusterCount, s->chunkCount, r.launches + 1};
    }
    if (s->timing)
        HIP_TRY(hipEventRecord(s->evHeavy0, os));
    HIP_TRY(launch_stop(kChain[variant].kernel, cg, cb, L.chainDyn, os, ev, P));
    if (s->timing) /* the chain kernel alone (rocprof's rtc_render_chain row) */
        HIP_TRY(hipEventRecord(s->evHeavy1, os));
    return 0;
}

static int run_accumulate(const Launch &L, hipStream_t os, hipEvent_t ev)
{
    const unsigned g = (unsigned)std::min<size_t>(((size_t)L.P.sampleCap + 255) / 256, 1024);
    if (L.resume)
        HIP_TRY(launch_stop(rtc_accumulate_samples_resume<true>, dim3(g), dim3(256), 0, os, ev, L.P));
    else if (!kAbNoSlots)
        HIP_TRY(launch_stop(rtc_accumulate_samples, dim3(g), dim3(256), 0, os, ev, L.P));
    else if (ev)
        HIP_TRY(hipEventRecord(ev, os));
    return 0;
}

static int run_order(const Launch &L, hipStream_t os, hipEvent_t)
{
    HIP_TRY(launch_stop(rtc_order_blocks, dim3(1), dim3(1024), 0, os, nullptr, L.region<unsigned>(rtcplan::kBufWeight),
                        (int)L.pl.blocks, L.region<int>(rtcplan::kBufOrder)));
    return 0;
}

static int run_render(const Launch &L, hipStream_t os, hipEvent_t)
{
    /* <SPHERES, DEBUG, RESUME>, by [spheres][debug][a pass] */
    static void (*const kRender[2][2][2])(RenderParams) = {
        {{rtc_render_kernel<false, false>, rtc_render_kernel<false, false, true>},
         {rtc_render_kernel<false, true>, rtc_render_kernel<false, true, true>}},
        {{rtc_render_kernel<true, false>, rtc_render_kernel<true, false, true>},
         {rtc_render_kernel<true, true>, rtc_render_kernel<true, true, true>}}};
    HIP_TRY(launch_stop(kRender[L.P.sphereCount > 0][L.pl.debug][L.resume], L.grid(), dim3(kBlock), 0, os, nullptr,
                        L.P));
    return 0;
}

static int run_reduce(const Launch &L, hipStream_t os, hipEvent_t)
{
    HIP_TRY(launch_stop(rtc_reduce_segments, dim3(1), dim3(kSegSlots), 0, os, nullptr, L.P.segSlots, L.P.segments));
    return 0;
}

static int run_first_hit(const Launch &L, hipStream_t os, hipEvent_t)
{
    /* <SPHERES> */
    static void (*const kFirstHit[2])(RenderParams, int *, float *, float *, float *) = {rtc_first_hit<false>,
                                                                                         rtc_first_hit<true>};
    const RtcHitBuffers &h = *L.hit;
    HIP_TRY(launch_stop(kFirstHit[L.P.sphereCount > 0], L.grid(), dim3(kBlock), 0, os, nullptr, L.P, h.prim, h.depth,
                        h.normal, h.albedo));
    return 0;
}

/* by rtcplan::Kernel (null: rtc_scene_update_async's refit kernel, which no launch plans) */
static int (*const kPlanned[])(const Launch &, hipStream_t, hipEvent_t) = {
    run_prep,  run_super_cull, run_tile_cull, run_sky, run_chain,    run_accumulate,
    run_order, run_render,     run_reduce,    nullptr, run_first_hit};
static_assert(sizeof kPlanned / sizeof kPlanned[0] == rtcplan::kKFirstHit + 1 && rtcplan::kKRefit == rtcplan::kKReduce + 1,
              "one function per planned kernel");

/* rtc_render_rows_async; with `items` (rtc_cull_items) the launch's preparation and culls alone: the kernels after the
 * tile cull are not enqueued (the plan's events are, so the ordering state stays true: a launch whose render kernels did
 * nothing), and `items` gets the launch's counter set and list regions.  With `hit` (rtc_render_first_hit_async) a
 * first-hit launch: no Scene, Color, accumulator or counters; the caller's hooks stay armed and the split launch's timing
 * and report as they were. */
static int render_rows(const RtcDeviceScene *s, const Scene *scene, const RtcCamera *cam, const RtcRenderDesc *d,
                       void *dColors, float *dAccum, unsigned long long *dSegments, void *stream, RtcCullItems *items,
                       const RtcSampleRange *range = nullptr, unsigned *dRngState = nullptr,
                       const RtcHitBuffers *hit = nullptr)
{
    const char *const who = hit ? "rtc_render_first_hit_async" : "rtc_render_rows_async";
    if (!s)
        return rtc_fail(RTC_EINVAL, "%s: null scene", who);
    RtcDeviceScene *const ms = const_cast<RtcDeviceScene *>(s);
    /* The hooks are one-shot: this launch takes the events armed before it and forgets them -- before any early
     * return, so a later launch never records an event its caller has since released (rtc_scene_set_geometry_event /
     * _frame_event); a launch that fails records neither.  (A first-hit launch is not a frame: it leaves them armed.) */
    const hipEvent_t geoEvent = hit ? nullptr : s->geoEvent, frameEvent = hit ? nullptr : s->frameEvent;
    if (!hit)
        ms->geoEvent = ms->frameEvent = nullptr;
    if (const int rc = check_arguments(who, scene, cam, d, dColors, hit))
        return rc;
    if (range) { /* rtc_render_samples_async: nothing is enqueued for a pass that is refused */
        if (!dAccum || !dRngState)
            return rtc_fail(RTC_EINVAL, "rtc_render_samples_async: the accumulator and the RNG-state buffer are required");
        if (range->first < 0 || range->count <= 0 || range->first > d->spp - range->count)
            return rtc_fail(RTC_EINVAL, "rtc_render_samples_async: samples [%d, %d + %d) are not within the frame's %d",
                            range->first, range->first, range->count, d->spp);
        if (d->flags & RTC_F_OVERLAP)
            return rtc_fail(RTC_EINVAL, "rtc_render_samples_async: RTC_F_OVERLAP (an unjoined sky pass would race the next "
                                        "pass's read of the accumulator)");
    }
    const int rows = rtc_rows_selected(d);
    /* the scene's buffers, scratch and kernels live on s->device; the caller's current device is restored */
    RtcDeviceGuard guard(s->device);
    if (!guard.ok())
        return rtc_fail(RTC_ENODEV, "%s: cannot select the scene's device %d", who, s->device);
    const hipStream_t st = (hipStream_t)stream;
    if (rows == 0) { /* nothing to render: the (empty) frame is complete once `stream` gets here */
        for (hipEvent_t ev : {geoEvent, frameEvent})
            if (ev)
                HIP_TRY(hipEventRecord(ev, st));
        /* rtc_scene_last_plan: the planner's empty launch (it reads no more of the request than this) */
        rtcplan::Request none{};
        none.firstHit = hit != nullptr;
        rtcplan::Plan empty;
        rtcplan::plan_launch(s->plan, none, empty);
        rtcplan::record_launch(empty, none, ms->lastPlan);
        return 0;
    }
    static thread_local rtcplan::Plan pl;
    Launch L{s, pl, render_params(s, scene, *cam, *d, rows, dColors, dAccum, dSegments, range), 0, 0, range != nullptr,
             hit};
    /* every ordering decision -- slot, streams, events, which kernels, which buffers -- comes from the planner
     * (rtc_plan.h); this function executes its operations */
    const RenderParams &P = L.P;
    const EnvParams &E = P.env;
    const float camKey[13] = {P.origin.x, P.origin.y, P.origin.z, P.ex.x, P.ex.y, P.ex.z, P.ey.x,
                              P.ey.y,     P.ey.z,     P.ez.x,     P.ez.y, P.ez.z, P.fov};
    const float envKey[14] = {E.sun.x,    E.sun.y,    E.sun.z,    E.horizon.x, E.horizon.y, E.horizon.z, E.zenith.x,
                              E.zenith.y, E.zenith.z, E.ground.x, E.ground.y,  E.ground.z,  E.focus,     E.intensity};
    rtcplan::Request rq = rtcplan::make_request(
        *d, rows, rtcplan::SceneShape{s->triPadded, s->maskWords, s->sphereCount, s->sphereSplitGate},
        (uint64_t)(uintptr_t)st, (uint64_t)(uintptr_t)dColors, (uint64_t)(uintptr_t)dAccum, dSegments != nullptr, camKey,
        envKey);
    rq.noMerge = !RTC_SKY_MERGE;
    if (range)
        rtcplan::set_sample_range(rq, range->first, range->count, (uint64_t)(uintptr_t)dRngState);
    if (hit) {
        const uint64_t ids[4] = {(uint64_t)(uintptr_t)hit->prim, (uint64_t)(uintptr_t)hit->depth,
                                 (uint64_t)(uintptr_t)hit->normal, (uint64_t)(uintptr_t)hit->albedo};
        rtcplan::set_first_hit(rq, ids);
    }
    if (!hit && !items) /* (the probes' launches enqueue no geometry kernel: nothing would fill or read a block) */
        rtcplan::set_draw_cache(rq, draw_cache_eligible(s));
    rtcplan::plan_launch(s->plan, rq, pl);
    /* the saved state claims only what has been enqueued: until every operation below is, a later launch sees none of
     * this launch's primary records or counter zeroing (it re-runs rtc_prep_primary) */
    ms->plan.prepValid[pl.half] = false;
    if (!hit) /* (a first-hit launch touches no counter set) */
        ms->plan.cullValid = false;
    if (const int rc = grow_capacity(ms, pl))
        return rc;
    if (pl.draws) /* the draw cache's memory: allocated, cleared for this frame size, the item-draw arrays large enough */
        if (const int rc = rtc_draws_prepare(ms, d->width, d->height, pl.drawReset, pl.itemDrawGrow ? pl.itemDrawNeed : 0))
            return rc;
    bind_plan(L, d->flags);
    if (range) /* (after bind_plan: the state pointer lies where an ordinary launch keeps geoColor, unbound in a pass) */
        L.P.rngState = dRngState;
    size_chain_lds(L);
    const hipStream_t streams[rtcplan::kStreams] = {st, s->cst, ms->cst2, s->side};
    hipEvent_t events[rtcplan::kEvents] = {}; /* (the caller's hooks may be unarmed: null) */
    events[rtcplan::kEvCullSync] = s->evCullSync, events[rtcplan::kEvFork] = s->evFork, events[rtcplan::kEvJoin] = s->evJoin;
    events[rtcplan::kEvFrame] = frameEvent, events[rtcplan::kEvGeometry] = geoEvent;
    for (int h = 0; h < kSkySlots; ++h)
        events[rtcplan::kEvSkyDone0 + h] = s->evSkyDone[h], events[rtcplan::kEvGeoDone0 + h] = s->evGeoDone[h];
    for (int i = 0; i < pl.nOps; ++i) {
        const rtcplan::Op &op = pl.ops[i];
        const hipStream_t os = streams[op.stream];
        const hipEvent_t ev = op.event >= 0 && op.event < rtcplan::kEvents ? events[op.event] : nullptr;
        if (op.kind == rtcplan::kOpRecord) {
            if (ev)
                HIP_TRY(hipEventRecord(ev, os));
        } else if (op.kind == rtcplan::kOpWait) {
            HIP_TRY(hipStreamWaitEvent(os, ev, 0));
        } else if (op.kernel < 0 || op.kernel > rtcplan::kKFirstHit || !kPlanned[op.kernel]) {
            return rtc_fail(RTC_EINVAL, "%s: unknown planned kernel %d", who, op.kernel);
        } else if (items && op.kernel > rtcplan::kKTileCull) {
            if (ev) /* (the skipped kernel's completion) */
                HIP_TRY(hipEventRecord(ev, os));
        } else if (const int rc = kPlanned[op.kernel](L, os, ev)) {
            return rc;
        }
    }
    if (!hit)
        ms->timed = pl.fused && s->timing;
    ms->plan = pl.after; /* every operation is enqueued */
    if (items) {
        if (!pl.chain)
            return rtc_fail(RTC_EINVAL, "rtc_cull_items: not a split launch");
        *items = RtcCullItems{P.geoCount, P.geoList,   P.pixMask, P.geoCap,    P.blocksX * 2,        pl.tiles, P.wideItems,
                              P.tileMask, P.maskWords, P.primF,   P.triPadded, pl.superCull ? 1 : 0};
    }
    rtcplan::record_launch(pl, rq, ms->lastPlan); /* (behind the last refusal: a call that fails leaves the record) */
    return 0;
}

extern "C" int rtc_render_rows_async(const RtcDeviceScene *s, const Scene *scene, const RtcCamera *cam,
                                     const RtcRenderDesc *d, void *dColors, float *dAccum,
                                     unsigned long long *dSegments, void *stream)
{
    return render_rows(s, scene, cam, d, dColors, dAccum, dSegments, stream, nullptr);
}

extern "C" int rtc_render_samples_async(const RtcDeviceScene *s, const Scene *scene, const RtcCamera *cam,
                                        const RtcRenderDesc *d, const RtcSampleRange *range, void *dColors,
                                        float *dAccum, unsigned int *dRngState, unsigned long long *dSegments,
                                        void *stream)
{
    if (!range)
        return rtc_fail(RTC_EINVAL, "rtc_render_samples_async: null sample range");
    return render_rows(s, scene, cam, d, dColors, dAccum, dSegments, stream, nullptr, range, dRngState);
}

extern "C" int rtc_render_first_hit_async(const RtcDeviceScene *s, const RtcCamera *cam, const RtcRenderDesc *d,
                                          const RtcHitBuffers *out, void *stream)
{
    if (!s)
        return rtc_fail(RTC_EINVAL, "rtc_render_first_hit_async: null scene");
    if (!out)
        return rtc_fail(RTC_EINVAL, "rtc_render_first_hit_async: null argument");
    return render_rows(s, nullptr, cam, d, nullptr, nullptr, nullptr, stream, nullptr, nullptr, nullptr, out);
}

/* ---- caller-supplied rays: closest hit, radiance, occlusion -------------------------------------- */
/* The three queries (and the pass over a list of pixels behind them, §3.17, which is a path query whose rays and seeds come
 * from a frame) share everything on the host but their arguments.  A query supplies: its args struct (whose record
 * part, `rays` and `n` carry these names), its <SPHERES, CULL> kernel table and kernel number, its own refusals, its
 * footprint rows (rtc_plan.h) and, for the host entry, the table of what is staged. */

static int no_refusal() { return 0; }

/* The refusals of a query's two entries, before any device call and before `s` is read, in the order every query keeps:
 * the scene, the entry's own arguments (nullArgument; noneAsked: the text when no output is asked for, else null), the
 * ray count, whatever else is the query's own (`own`), the flags (`allowed`: the query's own whitelist, `allowedNames` its
 * text).  `noun`: "a ray", "a path", "an occlusion". */
template <class Own>
static int refuse_query(const char *who, const char *noun, const RtcDeviceScene *s, bool nullArgument,
                        const char *noneAsked, size_t n, int flags, int allowed, const char *allowedNames, Own own)
{
    if (!s)
        return rtc_fail(RTC_EINVAL, "%s: null scene", who);
    if (nullArgument)
        return rtc_fail(RTC_EINVAL, "%s: null argument", who);
    if (noneAsked)
        return rtc_fail(RTC_EINVAL, "%s: %s", who, noneAsked);
    if (n > (size_t)0x7fffffff)
        return rtc_fail(RTC_EINVAL, "%s: %zu rays (at most 2147483647 in one call)", who, n);
    if (const int rc = own())
        return rc;
    if (flags & ~allowed)
        return rtc_fail(RTC_EINVAL, "%s: flags 0x%x (%s query takes %s and no other flag)", who, flags, noun, allowedNames);
    return 0;
}
/* the whitelist of a query that has one kernel */
static const char *const kCullFlagOnly = "RTC_F_NO_CLUSTER_CULL";

static void set_mats(OccludedArgs &, const DevMat *) {} /* (an occlusion query reads no material) */
template <class Args>
static void set_mats(Args &a, const DevMat *mats)
{
    a.mats = mats;
}

/* (a pixel pass has no ray buffer: its list is among its own fields) */
static void set_rays(RenderPixelsArgs &a, const Ray *, size_t n) { a.n = (unsigned)n; }
template <class Args>
static void set_rays(Args &a, const Ray *dRays, size_t n)
{
    a.rays = (const float *)dRays, a.n = (unsigned)n;
}

/* From a query's args, its own fields filled, to its kernel enqueued on `stream` (n > 0).  The planner names the generation
 * and the one operation (rtc_plan.h plan_query); the ordering state stays as it is (TracePlan::after == s->plan), and so do
 * the hooks, the timing events, the chain report and the draw cache.  `raysPerGroup`: how many rays a workgroup of the
 * table's kernels takes (kBlock: a lane each; kBlock / 64: a wave each, at most 2^29 workgroups for 2^31 - 1 rays).
 * `rows(plan, out, max)`: the query's footprint call (rtc_plan.h), recorded with the plan for rtc_scene_last_plan. */
template <class Args, class Rows>
static int enqueue_query(const char *who, const RtcDeviceScene *s, int kernel, void (*const (&table)[2][2])(Args), Args &a,
                         const Ray *dRays, size_t n, int trianglesOnly, int flags, void *stream, Rows rows,
                         size_t raysPerGroup = kBlock)
{
    RtcDeviceGuard guard(s->device);
    if (!guard.ok())
        return rtc_fail(RTC_ENODEV, "%s: cannot select the scene's device %d", who, s->device);
    rtcplan::TracePlan tp;
    rtcplan::plan_query(s->plan, kernel, tp);
    const SceneRecords &g = s->gen[tp.gen];
    a.tris = g.tris, a.spheres = g.spheres, a.clTris = g.clTris, a.clusters = g.clusters, a.chunks = g.chunks;
    set_mats(a, g.mats);
    a.triPadded = s->triPadded, a.sphereCount = trianglesOnly ? 0 : s->sphereCount;
    a.clusterCount = s->clusterCount, a.chunkCount = s->chunkCount;
    set_rays(a, dRays, n);
    for (int i = 0; i < tp.nOps; ++i) {
        const rtcplan::Op &op = tp.ops[i];
        if (op.kind != rtcplan::kOpKernel || op.kernel != kernel || op.stream != rtcplan::kStCaller)
            return rtc_fail(RTC_EINVAL, "%s: unknown planned operation %d", who, op.kind);
        hipLaunchKernelGGL(table[a.sphereCount > 0][!(flags & RTC_F_NO_CLUSTER_CULL)],
                           dim3((unsigned)((n + raysPerGroup - 1) / raysPerGroup)), dim3(kBlock), 0, (hipStream_t)stream,
                           a);
        HIP_TRY(hipGetLastError());
    }
    rtcplan::Footprint f[24];
    const int nf = std::min(rows(tp, f, 24), 24);
    rtcplan::record_query(tp, f, nf, const_cast<RtcDeviceScene *>(s)->lastPlan);
    return 0;
}

/* A path query -- rtc_trace_paths_async, rtc_render_pixels_async -- has two kernel families, by [RTC_F_WAVE_PER_RAY]: a
 * lane per ray, and a wave per ray (rtc_trace_paths.h): the same operation, buffers and ordering,
 * kBlock / 64 rays to a workgroup. */
#define PATH_TABLE(k) {{k<false, false>, k<false, true>}, {k<true, false>, k<true, true>}} /* <SPHERES, CULL> */
template <class Args, class Rows>
static int enqueue_path_query(const char *who, const RtcDeviceScene *s, int kernel, void (*const (&table)[2][2][2])(Args),
                              Args &a, const Ray *dRays, size_t n, int trianglesOnly, int flags, void *stream, Rows rows)
{
    const bool wave = (flags & RTC_F_WAVE_PER_RAY) != 0;
    return enqueue_query(who, s, kernel, table[wave], a, dRays, n, trianglesOnly, flags, stream, rows,
                         wave ? kBlock / 64 : kBlock);
}

/* ---- closest hit */
static int check_trace_rays(const char *who, const RtcDeviceScene *s, const void *rays, size_t n, int flags,
                            const void *const out[4], bool haveOut)
{
    return refuse_query(who, "a ray", s, !rays || !haveOut,
                        out[0] || out[1] || out[2] || out[3]
                            ? nullptr
                            : "no buffer asked for (prim, depth, normal and albedo are all null)",
                        n, flags, RTC_F_NO_CLUSTER_CULL, kCullFlagOnly, no_refusal);
}

extern "C" int rtc_trace_rays_async(const RtcDeviceScene *s, const Ray *dRays, size_t n, int trianglesOnly, int flags,
                                    const RtcHitBuffers *out, void *stream)
{
    const char *const who = "rtc_trace_rays_async";
    const void *const bufs[4] = {out ? out->prim : nullptr, out ? out->depth : nullptr, out ? out->normal : nullptr,
                                 out ? out->albedo : nullptr};
    if (const int rc = check_trace_rays(who, s, dRays, n, flags, bufs, out != nullptr))
        return rc;
    if (n == 0)
        return 0;
    TraceRaysArgs a{};
    a.prim = out->prim, a.depth = out->depth, a.normal = out->normal, a.albedo = out->albedo;
    /* <SPHERES, CULL> */
    static void (*const kTraceRays[2][2])(TraceRaysArgs) = {{rtc_trace_rays<false, false>, rtc_trace_rays<false, true>},
                                                            {rtc_trace_rays<true, false>, rtc_trace_rays<true, true>}};
    const uint64_t ids[4] = {(uint64_t)(uintptr_t)out->prim, (uint64_t)(uintptr_t)out->depth,
                             (uint64_t)(uintptr_t)out->normal, (uint64_t)(uintptr_t)out->albedo};
    return enqueue_query(who, s, rtcplan::kKTraceRays, kTraceRays, a, dRays, n, trianglesOnly, flags, stream,
                         [&](const rtcplan::TracePlan &t, rtcplan::Footprint *f, int max) {
                             return rtcplan::trace_footprint(t, (uint64_t)(uintptr_t)dRays, ids, f, max);
                         });
}

extern "C" int rtc_trace_rays(const RtcDeviceScene *s, const Ray *rays, size_t n, int trianglesOnly, int flags, int *prim,
                              float *depth, float *normal, float *albedo)
{
    const char *const who = "rtc_trace_rays";
    const void *const host[4] = {prim, depth, normal, albedo};
    if (const int rc = check_trace_rays(who, s, rays, n, flags, host, true))
        return rc;
    if (n == 0)
        return 0;
    const Staged items[5] = {{rays, nullptr, n * sizeof(Ray), true},
                             {nullptr, prim, n * sizeof(int), prim != nullptr},
                             {nullptr, depth, n * sizeof(float), depth != nullptr},
                             {nullptr, normal, n * 3 * sizeof(float), normal != nullptr},
                             {nullptr, albedo, n * 3 * sizeof(float), albedo != nullptr}};
    return staged_query(who, s, items, [&](void *const *dev) {
        const RtcHitBuffers out{(int *)dev[1], (float *)dev[2], (float *)dev[3], (float *)dev[4]};
        return rtc_trace_rays_async(s, (const Ray *)dev[0], n, trianglesOnly, flags, &out, nullptr);
    });
}

/* ---- radiance */
static int check_trace_paths(const char *who, const RtcDeviceScene *s, const Scene *scene, const void *rays,
                             const void *seeds, size_t n, const RtcPathDesc *d, const void *radiance)
{
    return refuse_query(who, "a path", s, !scene || !rays || !seeds || !d || !radiance, nullptr, n, d ? d->flags : 0,
                        RTC_F_NO_CLUSTER_CULL | RTC_F_WAVE_PER_RAY, "RTC_F_NO_CLUSTER_CULL, RTC_F_WAVE_PER_RAY", [&] {
        if (d->spp <= 0)
            return rtc_fail(RTC_EINVAL, "%s: spp %d", who, d->spp);
        if (d->sampleFirst < 0 || d->sampleCount <= 0 || d->sampleFirst > d->spp - d->sampleCount)
            return rtc_fail(RTC_EINVAL, "%s: samples [%d, %d + %d) of spp %d", who, d->sampleFirst, d->sampleFirst,
                            d->sampleCount, d->spp);
        return 0;
    });
}

extern "C" int rtc_trace_paths_async(const RtcDeviceScene *s, const Scene *scene, const Ray *dRays,
                                     const unsigned int *dSeeds, size_t n, const RtcPathDesc *d, float *dRadiance,
                                     unsigned int *dSeedsOut, unsigned long long *dSegments, void *stream)
{
    const char *const who = "rtc_trace_paths_async";
    if (const int rc = check_trace_paths(who, s, scene, dRays, dSeeds, n, d, dRadiance))
        return rc;
    if (n == 0)
        return 0;
    TracePathsArgs a{};
    a.env = env_of(*scene);
    a.invSpp = (float)(1. / d->spp); /* main.c:99 */
    a.sampleFirst = d->sampleFirst, a.sampleCount = d->sampleCount, a.maxBounce = d->maxBounce;
    a.seeds = dSeeds, a.radiance = dRadiance, a.seedsOut = dSeedsOut, a.segments = dSegments;
    static void (*const kTracePaths[2][2][2])(TracePathsArgs) = {PATH_TABLE(rtc_trace_paths),
                                                                 PATH_TABLE(rtc_trace_paths_wave)};
    return enqueue_path_query(who, s, rtcplan::kKTracePaths, kTracePaths, a, dRays, n, d->trianglesOnly, d->flags, stream,
                              [&](const rtcplan::TracePlan &t, rtcplan::Footprint *f, int max) {
                                  return rtcplan::paths_footprint(t, (uint64_t)(uintptr_t)dRays, (uint64_t)(uintptr_t)dSeeds,
                                                                  (uint64_t)(uintptr_t)dRadiance,
                                                                  (uint64_t)(uintptr_t)dSeedsOut, dSegments != nullptr,
                                                                  d->sampleFirst > 0, f, max);
                              });
}

extern "C" int rtc_trace_paths(const RtcDeviceScene *s, const Scene *scene, const Ray *rays, const unsigned int *seeds,
                               size_t n, const RtcPathDesc *d, float *radiance, unsigned int *seedsOut,
                               unsigned long long *segments)
{
    const char *const who = "rtc_trace_paths";
    if (const int rc = check_trace_paths(who, s, scene, rays, seeds, n, d, radiance))
        return rc;
    if (n == 0)
        return 0;
    /* the radiance goes in too when the call continues an accumulation, and the segment counter starts at the caller's
     * value */
    const Staged items[5] = {{rays, nullptr, n * sizeof(Ray), true},
                             {seeds, nullptr, n * sizeof(unsigned), true},
                             {d->sampleFirst > 0 ? radiance : nullptr, radiance, n * 3 * sizeof(float), true},
                             {nullptr, seedsOut, n * sizeof(unsigned), seedsOut != nullptr},
                             {segments, segments, sizeof(unsigned long long), segments != nullptr}};
    return staged_query(who, s, items, [&](void *const *dev) {
        return rtc_trace_paths_async(s, scene, (const Ray *)dev[0], (const unsigned *)dev[1], n, d, (float *)dev[2],
                                     (unsigned *)dev[3], (unsigned long long *)dev[4], nullptr);
    });
}

/* ---- occlusion within a distance limit */
static int check_occluded(const char *who, const RtcDeviceScene *s, const void *rays, size_t n, int flags,
                          const void *occluded, const void *count)
{
    return refuse_query(who, "an occlusion", s, !rays,
                        occluded || count ? nullptr : "no output asked for (occluded and count are both null)", n, flags,
                        RTC_F_NO_CLUSTER_CULL, kCullFlagOnly, no_refusal);
}

extern "C" int rtc_occluded_async(const RtcDeviceScene *s, const Ray *dRays, const float *dTMax, size_t n,
                                  int trianglesOnly, int flags, unsigned char *dOccluded, unsigned long long *dCount,
                                  void *stream)
{
    const char *const who = "rtc_occluded_async";
    if (const int rc = check_occluded(who, s, dRays, n, flags, dOccluded, dCount))
        return rc;
    if (n == 0)
        return 0;
    OccludedArgs a{};
    a.tMax = dTMax, a.occluded = dOccluded, a.count = dCount;
    /* <SPHERES, CULL> */
    static void (*const kOccluded[2][2])(OccludedArgs) = {{rtc_occluded<false, false>, rtc_occluded<false, true>},
                                                          {rtc_occluded<true, false>, rtc_occluded<true, true>}};
    return enqueue_query(who, s, rtcplan::kKOccluded, kOccluded, a, dRays, n, trianglesOnly, flags, stream,
                         [&](const rtcplan::TracePlan &t, rtcplan::Footprint *f, int max) {
                             return rtcplan::occluded_footprint(t, (uint64_t)(uintptr_t)dRays, (uint64_t)(uintptr_t)dTMax,
                                                                (uint64_t)(uintptr_t)dOccluded, dCount != nullptr, f, max);
                         });
}

extern "C" int rtc_occluded(const RtcDeviceScene *s, const Ray *rays, const float *tMax, size_t n, int trianglesOnly,
                            int flags, unsigned char *occluded, unsigned long long *count)
{
    const char *const who = "rtc_occluded";
    if (const int rc = check_occluded(who, s, rays, n, flags, occluded, count))
        return rc;
    if (n == 0)
        return 0;
    /* the counter starts at the caller's value */
    const Staged items[4] = {{rays, nullptr, n * sizeof(Ray), true},
                             {tMax, nullptr, n * sizeof(float), tMax != nullptr},
                             {nullptr, occluded, n, occluded != nullptr},
                             {count, count, sizeof(unsigned long long), count != nullptr}};
    return staged_query(who, s, items, [&](void *const *dev) {
        return rtc_occluded_async(s, (const Ray *)dev[0], (const float *)dev[1], n, trianglesOnly, flags,
                                  (unsigned char *)dev[2], (unsigned long long *)dev[3], nullptr);
    });
}

/* ---- a pass over a list of pixels of a progressive frame */
static int check_render_pixels(const char *who, const RtcDeviceScene *s, const Scene *scene, const RtcCamera *cam,
                               const RtcRenderDesc *d, const RtcSampleRange *range, const void *pixels, size_t n, int flags,
                               const void *accum, const void *rngState)
{
    return refuse_query(who, "a pixel", s, !scene || !cam || !d || !range || !pixels || !accum || !rngState, nullptr, n,
                        flags, RTC_F_NO_CLUSTER_CULL | RTC_F_WAVE_PER_RAY, "RTC_F_NO_CLUSTER_CULL, RTC_F_WAVE_PER_RAY", [&] {
        const int geometry = rtcplan::geometry_error(*d); /* (as check_arguments reports it) */
        if (geometry == 1)
            return rtc_fail(RTC_EINVAL, "%s: bad geometry %dx%d rows %d+k*%d", who, d->width, d->height, d->rowStart,
                            d->rowStride);
        if (geometry)
            return rtc_fail(RTC_EINVAL, "%s: frame too large", who);
        if (d->spp <= 0)
            return rtc_fail(RTC_EINVAL, "%s: spp %d", who, d->spp);
        if (range->first < 0 || range->count <= 0 || range->first > d->spp - range->count)
            return rtc_fail(RTC_EINVAL, "%s: samples [%d, %d + %d) are not within the frame's %d", who, range->first,
                            range->first, range->count, d->spp);
        /* of the frame's own flags: every other bit only chooses a route of the frame's launches and is ignored, so that a
         * caller passes the desc of its whole passes */
        if (d->flags & (RTC_F_DEBUG_BOUNCES | RTC_F_OVERLAP))
            return rtc_fail(RTC_EINVAL, "%s: desc flags 0x%x (RTC_F_DEBUG_BOUNCES: calcDebugColor is not offered for pixel "
                                        "lists; RTC_F_OVERLAP: a pass is never overlapped)", who, d->flags);
        if (d->flags & (RTC_F_COOP4 | RTC_F_COOP8 | RTC_F_PIPE | RTC_F_SPEC))
            return rtc_fail(RTC_EINVAL, "%s: desc flags RTC_F_COOP4 / COOP8 / PIPE / SPEC name kernels that were removed", who);
        return 0;
    });
}

extern "C" int rtc_render_pixels_async(const RtcDeviceScene *s, const Scene *scene, const RtcCamera *cam,
                                       const RtcRenderDesc *d, const RtcSampleRange *range, const unsigned int *dPixels,
                                       size_t n, int flags, void *dColors, float *dAccum, unsigned int *dRngState,
                                       unsigned long long *dSegments, void *stream)
{
    const char *const who = "rtc_render_pixels_async";
    if (const int rc = check_render_pixels(who, s, scene, cam, d, range, dPixels, n, flags, dAccum, dRngState))
        return rc;
    const int rows = rtc_rows_selected(d);
    if (n == 0 || rows == 0)
        return 0;
    RenderPixelsArgs a{};
    a.env = env_of(*scene);
    a.invSpp = (float)(1. / (double)d->spp); /* main.c:99 */
    a.sampleFirst = range->first, a.sampleCount = range->count, a.maxBounce = d->maxBounce;
    a.view.width = d->width, a.view.height = d->height, a.view.rows = rows;
    a.view.rowStart = d->rowStart, a.view.rowStride = d->rowStride;
    a.view.rowBandShift = d->rowBand > 1 ? __builtin_ctz((unsigned)d->rowBand) : 0;
    a.view.ex = v3(cam->ex), a.view.ey = v3(cam->ey), a.view.ez = v3(cam->ez), a.view.fov = cam->fov;
    a.origin = v3(cam->origin);
    a.pixelCount = (unsigned)((size_t)rows * (size_t)d->width); /* (geometry_error: at most 2^29) */
    a.pixels = dPixels;
    a.colors = (unsigned char *)dColors, a.accum = dAccum, a.rngState = dRngState, a.segments = dSegments;
    static void (*const kRenderPixels[2][2][2])(RenderPixelsArgs) = {PATH_TABLE(rtc_render_pixels),
                                                                     PATH_TABLE(rtc_render_pixels_wave)};
    return enqueue_path_query(who, s, rtcplan::kKRenderPixels, kRenderPixels, a, nullptr, n, d->trianglesOnly, flags, stream,
                              [&](const rtcplan::TracePlan &t, rtcplan::Footprint *f, int max) {
                                  return rtcplan::pixels_footprint(t, (uint64_t)(uintptr_t)dPixels,
                                                                   (uint64_t)(uintptr_t)dColors, (uint64_t)(uintptr_t)dAccum,
                                                                   (uint64_t)(uintptr_t)dRngState, dSegments != nullptr,
                                                                   range->first > 0, f, max);
                              });
}

extern "C" int rtc_render_pixels(const RtcDeviceScene *s, const Scene *scene, const RtcCamera *cam, const RtcRenderDesc *d,
                                 const RtcSampleRange *range, const unsigned int *pixels, size_t n, int flags, void *colors,
                                 float *accum, unsigned int *rngState, unsigned long long *segments)
{
    const char *const who = "rtc_render_pixels";
    if (const int rc = check_render_pixels(who, s, scene, cam, d, range, pixels, n, flags, accum, rngState))
        return rc;
    const size_t px = (size_t)rtc_rows_selected(d) * (size_t)d->width;
    if (n == 0 || px == 0)
        return 0;
    /* the list, the frame's three whole buffers and the counter's value.  The buffers go in as well as out, whatever the
     * range: the pixels that are not listed come back as they were */
    const Staged items[5] = {{pixels, nullptr, n * sizeof(unsigned), true},
                             {colors, colors, px * 3, colors != nullptr},
                             {accum, accum, px * 3 * sizeof(float), true},
                             {rngState, rngState, px * sizeof(unsigned), true},
                             {segments, segments, sizeof(unsigned long long), segments != nullptr}};
    return staged_query(who, s, items, [&](void *const *dev) {
        return rtc_render_pixels_async(s, scene, cam, d, range, (const unsigned *)dev[0], n, flags, dev[1], (float *)dev[2],
                                       (unsigned *)dev[3], (unsigned long long *)dev[4], nullptr);
    });
}

int rtc_cull_items(const RtcDeviceScene *s, const Scene *scene, const RtcCamera *cam, const RtcRenderDesc *d,
                   void *dColors, RtcCullItems *items)
{
    if (!items)
        return rtc_fail(RTC_EINVAL, "rtc_cull_items: null argument");
    return render_rows(s, scene, cam, d, dColors, nullptr, nullptr, nullptr, items);
}

/* ---- row de-interleave after a gather (bytes) ----------------------------------------------------- */
__global__ __launch_bounds__(256) void rtc_deinterleave_kernel(const unsigned char *__restrict__ in, int parts,
                                                                int rowsPerPart, int rowBytes, int height, int bandShift,
                                                                unsigned char *__restrict__ out)
{
    /* one block-row per output row y: band b = y / B of part b % parts, the part's band b / parts */
    const int y = blockIdx.y;
    if (y >= height)
        return;
    const int b = y >> bandShift, j = y & ((1 << bandShift) - 1);
    const int g = b % parts, k = ((b / parts) << bandShift) + j;
    const unsigned char *src = in + ((size_t)g * rowsPerPart + k) * (size_t)rowBytes;
    unsigned char *dst = out + (size_t)y * rowBytes;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < rowBytes; i += gridDim.x * blockDim.x)
        dst[i] = src[i];
}

extern "C" int rtc_deinterleave_bands_async(const void *dCompact, int parts, int rowsPerPart, int width, int height,
                                            int rowBand, void *dOut, void *stream)
{
    if (!dCompact || !dOut || parts <= 0 || width <= 0 || height <= 0 || rowBand < 0 || rowBand > 64 ||
        (rowBand & (rowBand - 1)) != 0)
        return rtc_fail(RTC_EINVAL, "rtc_deinterleave_bands_async: bad argument");
    const int B = rowBand > 1 ? rowBand : 1;
    /* every part holds its bands' rows: part 0's count is the largest */
    RtcRenderDesc d0{};
    d0.width = width, d0.height = height, d0.rowStart = 0, d0.rowStride = parts, d0.rowBand = B;
    if (rowsPerPart < rtc_rows_selected(&d0))
        return rtc_fail(RTC_EINVAL, "rtc_deinterleave_bands_async: %d rows per part, part 0 has %d", rowsPerPart,
                        rtc_rows_selected(&d0));
    const int rowBytes = width * 3;
    dim3 grid((rowBytes + 255) / 256 < 8 ? (rowBytes + 255) / 256 : 8, height);
    hipLaunchKernelGGL(rtc_deinterleave_kernel, grid, dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char *)dCompact, parts, rowsPerPart, rowBytes, height, __builtin_ctz((unsigned)B),
                       (unsigned char *)dOut);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int rtc_deinterleave_async(const void *dCompact, int parts, int rowsPerPart, int width, int height,
                                      void *dOut, void *stream)
{
    if (!dCompact || !dOut || parts <= 0 || width <= 0 || height <= 0 || rowsPerPart * parts < height)
        return rtc_fail(RTC_EINVAL, "rtc_deinterleave_async: bad argument");
    return rtc_deinterleave_bands_async(dCompact, parts, rowsPerPart, width, height, 1, dOut, stream);
}

/* A frame copy with a small footprint (rtc_copy_async): `blocks` workgroups stream 16-byte words (the byte tail
 * by the first lanes), e.g. from HBM into pinned host memory over PCIe, so a D2H of Color[] occupies a few CU
 * slots instead of one workgroup on every CU (the runtime's blit kernel) while the render kernels run. */
__global__ __launch_bounds__(256) void rtc_copy_kernel(const unsigned char *__restrict__ src,
                                                       unsigned char *__restrict__ dst, size_t bytes)
{
    const size_t n16 = bytes / 16;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    const uint4 *s16 = (const uint4 *)src;
    uint4 *d16 = (uint4 *)dst;
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    for (; i + 3 * stride < n16; i += 4 * stride) { /* four independent 16-byte loads in flight per lane */
        const uint4 a = s16[i], b = s16[i + stride], c = s16[i + 2 * stride], d = s16[i + 3 * stride];
        d16[i] = a;
        d16[i + stride] = b;
        d16[i + 2 * stride] = c;
        d16[i + 3 * stride] = d;
    }
    for (; i < n16; i += stride)
        d16[i] = s16[i];
    const size_t t = n16 * 16 + blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t < bytes)
        dst[t] = src[t];
}

extern "C" int rtc_copy_async(void *dst, const void *src, size_t bytes, int blocks, void *stream)
{
    if ((!dst || !src) && bytes)
        return rtc_fail(RTC_EINVAL, "rtc_copy_async: null pointer");
    if (bytes == 0)
        return 0;
    if ((((size_t)dst | (size_t)src) & 15) != 0)
        return rtc_fail(RTC_EINVAL, "rtc_copy_async: pointers must be 16-byte aligned");
    if (blocks <= 0)
        blocks = 32;
    hipLaunchKernelGGL(rtc_copy_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char *)src, (unsigned char *)dst, bytes);
    HIP_TRY(hipGetLastError());
    return 0;
}

/* ---- the instantiation list -------------------------------------------------------------------------------------
 * Every instantiation of the kernel templates, once.  The device code is emitted as the non-template kernels in source
 * order, then these in the order listed, whichever the host code above names first.  That order is kept from change to
 * change (the kernels then lie at the same offsets from one another in the code object: DESIGN §3.7 measured a frame
 * 0.3 % slower with new kernels between the old ones; tools/kernel_diff.py fails a change that moves one).  So new
 * instantiations are appended, and the list stays after the last kernel definition. */
template __global__ void rtc_render_sky_rows<4, true>(RenderParams);
template __global__ void rtc_render_sky_rows<4, false>(RenderParams);
template __global__ void rtc_render_sky_rows<1, true>(RenderParams);
template __global__ void rtc_render_sky_rows<1, false>(RenderParams);
template __global__ void rtc_render_chain<true, true, false, true>(RenderParams);
template __global__ void rtc_render_chain<true, false, false, true>(RenderParams);
template __global__ void rtc_render_chain<false, true, false, true>(RenderParams);
template __global__ void rtc_render_chain<false, false, false, true>(RenderParams);
template __global__ void rtc_render_chain<false, false, true, false>(RenderParams);
template __global__ void rtc_render_chain<false, false, false, false>(RenderParams);
template __global__ void rtc_render_kernel<true, true>(RenderParams);
template __global__ void rtc_render_kernel<true, false>(RenderParams);
template __global__ void rtc_render_kernel<false, true>(RenderParams);
template __global__ void rtc_render_kernel<false, false>(RenderParams);
/* the sphere split */
template __global__ void rtc_tile_cull_sph<true>(RenderParams, unsigned long long *, unsigned *, unsigned long long *);
template __global__ void rtc_render_chain<true, true, false, true, true>(RenderParams);
template __global__ void rtc_render_chain<true, false, false, true, true>(RenderParams);
template __global__ void rtc_render_chain<false, true, false, true, true>(RenderParams);
template __global__ void rtc_render_chain<false, false, false, true, true>(RenderParams);
/* a pass (RESUME) */
template __global__ void rtc_render_sky_rows<4, true, true>(RenderParams);
template __global__ void rtc_render_sky_rows<1, true, true>(RenderParams);
template __global__ void rtc_render_chain<false, false, false, true, false, true>(RenderParams);
template __global__ void rtc_render_chain<false, false, false, true, true, true>(RenderParams);
template __global__ void rtc_render_chain<false, true, false, true, false, true>(RenderParams);
template __global__ void rtc_render_chain<false, true, false, true, true, true>(RenderParams);
template __global__ void rtc_render_chain<true, false, false, true, false, true>(RenderParams);
template __global__ void rtc_render_chain<true, false, false, true, true, true>(RenderParams);
template __global__ void rtc_render_chain<true, true, false, true, false, true>(RenderParams);
template __global__ void rtc_render_chain<true, true, false, true, true, true>(RenderParams);
template __global__ void rtc_accumulate_samples_resume<true>(RenderParams);
template __global__ void rtc_render_kernel<false, false, true>(RenderParams);
template __global__ void rtc_render_kernel<false, true, true>(RenderParams);
template __global__ void rtc_render_kernel<true, false, true>(RenderParams);
template __global__ void rtc_render_kernel<true, true, true>(RenderParams);
/* the first-hit buffers */
template __global__ void rtc_first_hit<false>(RenderParams, int *, float *, float *, float *);
template __global__ void rtc_first_hit<true>(RenderParams, int *, float *, float *, float *);
/* caller-supplied rays */
template __global__ void rtc_trace_rays<false, true>(TraceRaysArgs);
template __global__ void rtc_trace_rays<true, true>(TraceRaysArgs);
template __global__ void rtc_trace_rays<false, false>(TraceRaysArgs);
template __global__ void rtc_trace_rays<true, false>(TraceRaysArgs);
/* the draw cache */
template __global__ void rtc_tile_cull_draws<true>(RenderParams, unsigned long long *, unsigned *, unsigned long long *,
                                                   DrawCache);
template __global__ void rtc_fill_draws<true>(DrawCache);
template __global__ void rtc_render_chain<false, false, false, false, false, false, true>(RenderParams);
template __global__ void rtc_render_chain<false, false, true, false, false, false, true>(RenderParams);
/* caller-supplied rays: radiance */
template __global__ void rtc_trace_paths<false, true>(TracePathsArgs);
template __global__ void rtc_trace_paths<true, true>(TracePathsArgs);
template __global__ void rtc_trace_paths<false, false>(TracePathsArgs);
template __global__ void rtc_trace_paths<true, false>(TracePathsArgs);
/* caller-supplied rays: occlusion */
template __global__ void rtc_occluded<false, true>(OccludedArgs);
template __global__ void rtc_occluded<true, true>(OccludedArgs);
template __global__ void rtc_occluded<false, false>(OccludedArgs);
template __global__ void rtc_occluded<true, false>(OccludedArgs);
/* caller-supplied rays: radiance, a wave per ray */
template __global__ void rtc_trace_paths_wave<false, true>(TracePathsArgs);
template __global__ void rtc_trace_paths_wave<true, true>(TracePathsArgs);
template __global__ void rtc_trace_paths_wave<false, false>(TracePathsArgs);
template __global__ void rtc_trace_paths_wave<true, false>(TracePathsArgs);
/* a pass over a list of pixels: a lane per pixel, a wave per pixel */
template __global__ void rtc_render_pixels<false, true>(RenderPixelsArgs);
template __global__ void rtc_render_pixels<true, true>(RenderPixelsArgs);
template __global__ void rtc_render_pixels<false, false>(RenderPixelsArgs);
template __global__ void rtc_render_pixels<true, false>(RenderPixelsArgs);
template __global__ void rtc_render_pixels_wave<false, true>(RenderPixelsArgs);
template __global__ void rtc_render_pixels_wave<true, true>(RenderPixelsArgs);
template __global__ void rtc_render_pixels_wave<false, false>(RenderPixelsArgs);
template __global__ void rtc_render_pixels_wave<true, false>(RenderPixelsArgs);
