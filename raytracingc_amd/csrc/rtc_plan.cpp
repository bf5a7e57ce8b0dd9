/*
 * rtc_plan.cpp -- the launch planner (rtc_plan.h): every ordering decision of rtc_render_rows_async, as data.
 * Pure host C++; the HIP executor is rtc_render_rows_async (rtc_render.hip), the CPU test tests/test_plan.py.
 */
#include "rtc_plan.h"
#include "rtc_regroup.h"

#include <algorithm>
#include <cstring>
#include <initializer_list>

namespace rtcplan {

void init(State &s)
{
    memset(&s, 0, sizeof s);
}

namespace {
size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct Emitter {
    Plan &p;
    void op(int kind, int stream, int event, int kernel)
    {
        if (p.nOps < (int)(sizeof p.ops / sizeof p.ops[0]))
            p.ops[p.nOps++] = Op{kind, stream, event, kernel};
    }
    void record(int st, int ev) { op(kOpRecord, st, ev, -1); }
    void wait(int st, int ev) { op(kOpWait, st, ev, -1); }
    void kernel(int st, int k, int stopEv = kEvNone) { op(kOpKernel, st, stopEv, k); }
};

/* The scratch slot: one row per region (Buf order), one loop for the offsets and the slot size.  An alignment is
 * budgeted in full in the slot size, so the slot always holds the aligned offsets. */
void layout_slot(Plan &p, size_t maskWords)
{
    /* one entry per pixel at worst: an item record per entry of the lists, a colour word per entry of geoColor */
    const size_t entries = (size_t)kGeoLists * p.geoCap, counters = (size_t)kGeoLists * kGeoCountStride * 4;
    const struct { size_t used, align, padAfter; } rows[kScratchRegions] = {
        /* kBufMask      */ {p.tiles * maskWords * 8, 1, 0},
        /* kBufPixMask   */ {p.tiles * 8, 1, 0},
        /* kBufWeight    */ {p.blocks * 4, 1, 0},
        /* kBufOrder     */ {(p.blocks + 4) * 4, 1, counters}, /* historical padding: the sub-list counters' old place */
        /* kBufGeoList   */ {entries * kItemRecordBytes, kItemRecordBytes, 0}, /* (written as whole 16-B records) */
        /* kBufSuperMask */ {(size_t)p.superX * p.superY * maskWords * 8, 8, 0},
        /* kBufPixItem   */ {p.tiles * 64 * 4, 256, 0},
        /* kBufGeoColor  */ {entries * 4, 1, p.tiles * 4},           /* historical padding: an int per tile, long unused */
    };
    size_t off = 0, budget = 0;
    for (int b = 0; b < kScratchRegions; ++b) {
        p.reg[b] = Region{align_up(off, rows[b].align), rows[b].used};
        off = p.reg[b].offset + rows[b].used + rows[b].padAfter;
        budget += rows[b].used + rows[b].padAfter + (rows[b].align > 1 ? rows[b].align : 0);
    }
    p.slotBytes = align_up(budget, 256);
}

uint64_t stream_id(int st, uint64_t caller)
{
    return st == kStCull0 ? kIdCull0 : st == kStCull1 ? kIdCull1 : caller;
}
} // namespace

bool sphere_split(int sphereCount, bool gateAllows, int flags)
{
    return sphereCount > 0 && sphereCount <= kSplitSpheresMax && (gateAllows || (flags & RTC_F_SPLIT_SPHERES)) &&
           !(flags & (RTC_F_NO_COOP | RTC_F_NO_REORDER | RTC_F_NO_TILE_CULL | RTC_F_DEBUG_BOUNCES));
}

Request make_request(const RtcRenderDesc &d, int rows, const SceneShape &sc, uint64_t stream, uint64_t colors,
                     uint64_t accum, bool segments, const float cam[13], const float env[14])
{
    Request r;
    memset(&r, 0, sizeof r); /* (the key is compared with memcmp) */
    r.stream = stream;
    r.flags = d.flags;
    r.width = d.width;
    r.rows = rows;
    r.rowStride = d.rowStride;
    r.spp = d.spp;
    r.sphereCount = d.trianglesOnly ? 0 : sc.sphereCount;
    r.sphereSplit = sphere_split(r.sphereCount, sc.splitGate, d.flags);
    r.triPadded = sc.triPadded;
    r.maskWords = sc.maskWords;
    r.segments = segments;
    r.key.colors = colors;
    r.key.accum = accum;
    memcpy(r.key.cam, cam, sizeof r.key.cam);
    memcpy(r.key.env, env, sizeof r.key.env);
    const int dims[9] = {d.width, d.height, rows, d.rowStart, d.rowStride, d.spp, d.maxBounce,
                         (d.flags & RTC_F_HOIST_PRIMARY) ? 1 : 0, d.rowBand > 1 ? __builtin_ctz((unsigned)d.rowBand) : 0};
    memcpy(r.key.dims, dims, sizeof dims);
    memcpy(r.origin, cam, sizeof r.origin);
    r.height = d.height;
    return r;
}

void set_draw_cache(Request &r, int eligible)
{
    r.drawCache = eligible & 3;
}

void set_sample_range(Request &r, int first, int count, uint64_t rngState)
{
    r.resume = true;
    r.sampleFirst = first;
    r.sampleCount = count;
    r.rngState = rngState;
    r.flags &= ~RTC_F_OVERLAP; /* (the entry point refuses it) */
}

void set_first_hit(Request &r, const uint64_t ids[4])
{
    r.firstHit = true;
    memcpy(r.hit, ids, sizeof r.hit);
    r.flags &= RTC_F_NO_TILE_CULL; /* (the entry point refuses every other flag) */
    r.segments = false;
    /* no Color, accumulator or sample decides what it writes: the key is the camera and the rows alone */
    r.key.colors = r.key.accum = 0;
}

int geometry_error(const RtcRenderDesc &d)
{
    if (d.width <= 0 || d.height <= 0 || d.rowStride <= 0 || d.rowStart < 0 || d.rowBand < 0 || d.rowBand > 64 ||
        (d.rowBand & (d.rowBand - 1)) != 0)
        return 1;
    return (long long)d.width * d.height > (1ll << 31) / 4 ? 2 : 0;
}

void plan_launch(const State &s, const Request &r, Plan &p)
{
    memset(&p, 0, sizeof p);
    p.after = s;
    State &n = p.after;
    Emitter E{p};
    if (r.rows <= 0) { /* nothing to render: the (empty) frame is complete once the caller's stream gets here */
        p.empty = true;
        if (!r.firstHit) { /* (a first-hit launch leaves the caller's hooks armed) */
            E.record(kStCaller, kEvGeometry);
            E.record(kStCaller, kEvFrame);
        }
        return;
    }
    const size_t px = (size_t)r.width * (size_t)r.rows;
    p.debug = (r.flags & RTC_F_DEBUG_BOUNCES) != 0;
    p.resume = r.resume;
    p.resumeRead = r.resume && r.sampleFirst > 0;
    /* the tile cull keeps a workgroup's prefilter survivors in LDS (maskWords u64, <= 48 KB) */
    p.cull = !(r.flags & RTC_F_NO_TILE_CULL) && r.maskWords <= kMaxCullMaskWords;
    /* the split launch (rtc_render_chain + the sky pass): every triangle-only scene, and the sphere scenes sphere_split
     * admits */
    p.fused = p.cull && !p.debug && (r.sphereCount == 0 || r.sphereSplit) &&
              !(r.flags & (RTC_F_NO_COOP | RTC_F_NO_REORDER)) && !r.firstHit;
    p.chain = p.fused;
    p.gridX = (unsigned)((r.width + 15) / 16);
    p.gridY = (unsigned)((r.rows + 15) / 16);
    p.blocks = (size_t)p.gridX * p.gridY;
    p.tiles = 4 * p.blocks;
    p.superX = (p.gridX + 3) / 4;
    p.superY = (p.gridY + 3) / 4;
    p.superCull = p.cull && px > kSuperCullPixels && r.maskWords > 0;
    p.geoCap = (int)((p.tiles + kGeoLists - 1) / kGeoLists * 64); /* sub-list l: the tiles t = l mod kGeoLists */
    p.wideItems = r.width > kItemCoordMax || r.rows > kItemCoordMax;
    /* RTC_F_OVERLAP: the sky pass is not joined into the caller's stream (a launch that counts segments joins: the
     * reduction reads the sky pass's counters) */
    p.overlap = (r.flags & RTC_F_OVERLAP) && p.fused && !r.segments && !r.resume;
    p.half = p.overlap ? s.flip : 0;
    p.gen = s.gen;
    if (p.overlap) /* (every return below adopts n: an overlapped launch always ends with its slot's sky-done record) */
        n.slotGens[p.half] |= (unsigned char)(1u << s.gen);
    /* small shares (row stride > 1, <= kInlineSumPixels) sum in-kernel and, pipelined, prepare, cull and run their
     * geometry kernel on one of the two cull streams by slot parity; so do whole pipelined frames of more pixels
     * (DESIGN §3); smaller whole frames keep the caller's stream (C1 256x256x1: cross-stream hops would be its period) */
    p.smallShare = r.rowStride > 1 && px <= kInlineSumPixels;
    p.chainOnCs = p.overlap && (p.smallShare || px > kInlineSumPixels);
    /* Round 6: a pipelined launch on the alternating streams runs its sky pass AFTER its geometry kernel
     * (which then writes each pixel's colour into a per-item word, not into Color) and the sky pass writes every pixel of
     * the frame in whole 64-B lines.  In the pipelined steady state this sky pass runs beside the next frame's geometry
     * kernel, as the previous one did beside this frame's.  Small shares only: whole 1080p frames took 19 % longer with it
     * (0.398 vs 0.336 ms: the sky pass no longer hides beside its own frame's geometry kernel), 1080p 1/4 shares 4 % less
     * (0.110 vs 0.115 ms), 1/8 shares and C3 fsuzane the same (profiles/r06_f_ab_merged_sky.log).  It does not save
     * bytes: the per-item words are as scattered as the Color triples were (1/4 share: geometry kernel WRITE_SIZE 452 ->
     * 601 KB, sky 1465 -> 1519 KB, profiles/r06_j_pmc_writes.log); the gain is the schedule. */
    p.merge = p.chainOnCs && p.smallShare && !r.noMerge;
    p.needCst2 = p.chainOnCs && !s.cst2;
    if (p.needCst2)
        n.cst2 = true;
    p.cs = p.chainOnCs ? ((p.half & 1) ? kStCull1 : kStCull0) : kStCaller;
    p.gs = p.chainOnCs ? p.cs : kStCaller;
    const uint64_t csId = stream_id(p.cs, r.stream);

    /* An unjoined sky pass of an earlier overlapped launch may still write Color rows and read its scratch slot.  A
     * launch that is not overlapped waits for every such pass; an overlapped one waits when a pending pass reads the slot
     * it rewrites (unless its culls move to a cull stream, which waits for that slot itself, below), or writes the same
     * Color or accumulator buffer with other rows, camera or environment.  One wait on the newest such pass covers every
     * earlier one (the side stream runs them in order); evSkyDone[h] also covers launch h's geometry kernel. */
    /* A first-hit launch writes no Color or accumulator row: it waits like an overlapped launch that keeps the caller's
     * stream, for the pass that reads its slot (0) and its primary records, and for no other. */
    const bool waitAll = !p.overlap && !r.firstHit;
    int waitSky = -1;
    for (int h = 0; h < kSlots; ++h)
        if (s.skyPending[h] &&
            (waitAll || (h == p.half && p.cs == kStCaller) ||
             (!r.firstHit &&
              (s.skyKey[h].colors == r.key.colors || (r.key.accum && s.skyKey[h].accum == r.key.accum)) &&
              memcmp(&s.skyKey[h], &r.key, sizeof r.key) != 0)) &&
            (waitSky < 0 || s.skySeq[h] > s.skySeq[waitSky]))
            waitSky = h;
    if (waitSky >= 0) {
        E.wait(kStCaller, kEvSkyDone0 + waitSky);
        const unsigned long long upTo = s.skySeq[waitSky];
        for (int h = 0; h < kSlots; ++h)
            if (s.skySeq[h] <= upTo)
                n.skyPending[h] = false;
    }

    /* the scratch: kSlots slots; slot h starts at h x (the allocation's slot size), not h x this launch's size --
     * launches of different sizes are in flight together (round 5 fix; the legacy layout is a test hook) */
    if (p.cull) {
        layout_slot(p, (size_t)r.maskWords);
        p.scratchNeed = kSlots * p.slotBytes;
        p.scratchGrow = p.scratchNeed > s.scratchCap;
        if (p.scratchGrow)
            n.scratchCap = p.scratchNeed;
        const size_t slotStride = r.legacySlotLayout ? p.slotBytes : n.scratchCap / kSlots;
        p.slotOffset = (size_t)p.half * slotStride;
    }
    if (p.chain) {
        p.geoSet = s.geoSeq % kGeoRing;
        p.geoSetNext = (s.geoSeq + 1) % kGeoRing;
        p.cullPrio = p.smallShare && px > 400000;
        /* deferred accumulation slots (joined whole frames; small shares and the alternating streams sum in-kernel) */
        if (r.spp > 0 && !(r.flags & RTC_F_CHAIN_INLINE) && !p.smallShare && !p.chainOnCs) {
            /* (a pass: slots for its own samples, [item][sampleCount]) */
            const size_t per = (size_t)(r.resume ? r.sampleCount : r.spp) * kSampleSlotBytes + sizeof(int);
            const size_t cap = std::min<size_t>(px, kSampleBufBudget / per);
            p.samplesNeed = cap * per + 256;
            p.samplesGrow = p.samplesNeed > s.samplesCap;
            if (p.samplesGrow)
                n.samplesCap = p.samplesNeed;
            p.sampleCap = (int)cap;
        }
        /* the draw cache: the launches whose geometry kernel has no GENERAL code (rtc_render.hip chain_flags: in-kernel
         * sums, no hoisting, counters, spheres or pass; the scene's part is Request::drawCache), unless the launch opts out.
         * The slot table is built for one frame size: another one clears it; the slots' item-draw arrays (one u32 per entry
         * of the lists) grow like the scratch, slot h at h x the allocation's slot size */
        p.draws = ((r.drawCache >> (p.smallShare ? 1 : 0)) & 1) && r.spp > 0 && p.sampleCap == 0 && !r.segments &&
                  !r.resume && r.sphereCount == 0 && !(r.flags & (RTC_F_HOIST_PRIMARY | RTC_F_NO_DRAW_CACHE));
        if (p.draws) {
            p.drawReset = s.drawWidth != r.width || s.drawHeight != r.height;
            n.drawWidth = r.width, n.drawHeight = r.height;
            const size_t slotItemDraw = align_up((size_t)kGeoLists * p.geoCap * 4, 256);
            p.itemDrawNeed = kSlots * slotItemDraw;
            p.itemDrawGrow = p.itemDrawNeed > s.itemDrawCap;
            if (p.itemDrawGrow)
                n.itemDrawCap = p.itemDrawNeed;
            p.itemDrawOffset = (size_t)p.half * (n.itemDrawCap / kSlots);
        }
    }
    /* what the launch binds: the executor hands its kernels these buffers and no other, and only these have footprints */
    const auto bind = [&p](bool on, std::initializer_list<int> bufs) { for (int b : bufs) p.bound |= (unsigned)on << b; };
    bind(true, {kBufPrim, kBufSceneGen});
    bind(!r.firstHit, {kBufColors});
    bind(r.firstHit, {kBufHit});
    bind(p.cull, {kBufMask, kBufPixMask, kBufWeight});
    bind(p.cull && !p.fused && !r.firstHit, {kBufOrder});
    bind(p.superCull, {kBufSuperMask});
    bind(p.chain, {kBufGeoList, kBufGeoSet, kBufGeoSetNext});
    bind(p.merge, {kBufPixItem, kBufGeoColor});
    bind(p.sampleCap > 0, {kBufSamples});
    bind(r.key.accum != 0, {kBufAccum});
    bind(r.segments, {kBufSegSlots, kBufCallerSegments});
    bind(r.resume, {kBufRngState});
    bind(p.draws, {kBufDrawTable, kBufItemDraw});

    if (p.cs != kStCaller) {
        /* the cull stream runs this launch's first kernels: after everything the caller enqueued before the launch and
         * after the sky wait above (an event at the caller stream's position), and after the slot's previous user ended
         * (its sky pass and its geometry kernel) */
        E.record(kStCaller, kEvCullSync);
        E.wait(p.cs, kEvCullSync);
        if (s.slotUsed[p.half]) {
            E.wait(p.cs, kEvSkyDone0 + p.half);
            E.wait(p.cs, kEvGeoDone0 + p.half);
        }
    }
    /* the previous split launch's tile cull zeroed this launch's counter set: when it ran on another stream (the null
     * stream included), wait for it -- kEvFork is its completion */
    const bool waitPrevCull = p.chain && s.cullValid && s.cullStream != csId;
    if (waitPrevCull)
        E.wait(p.cs, kEvFork);
    const bool prepCurrent = s.prepValid[p.half] && s.prepStream[p.half] == csId &&
                             memcmp(s.prepOrigin[p.half], r.origin, sizeof r.origin) == 0;
    const bool countsZeroed = !p.chain || (s.cullValid && (s.cullStream == csId || waitPrevCull));
    if (p.chain)
        n.cullValid = false;
    /* rtc_prep_primary: the primary records of this camera origin, and this launch's counter set zeroed; skipped for
     * frames of one camera position on one stream */
    if ((r.triPadded > 0 || p.chain) && !(prepCurrent && countsZeroed)) {
        p.prep = true;
        p.prepCounts = p.chain;
        E.kernel(p.cs, kKPrep);
        n.prepValid[p.half] = true;
        n.prepStream[p.half] = csId;
        memcpy(n.prepOrigin[p.half], r.origin, sizeof r.origin);
    }
    if (p.superCull)
        E.kernel(p.cs, kKSuperCull);
    if (r.firstHit) { /* joined by construction: every kernel on the caller's stream, no hook, no counter set */
        if (p.cull)
            E.kernel(kStCaller, kKTileCull);
        E.kernel(kStCaller, kKFirstHit);
        return;
    }
    if (!p.cull) {
        E.kernel(kStCaller, kKRender);
    } else {
        /* the split launch forks its sky pass at the tile cull's end: kEvFork is the cull's own completion */
        E.kernel(p.cs, kKTileCull, p.fused ? kEvFork : kEvNone);
        if (p.chain) { /* this cull zeroes the next counter set */
            n.geoSeq = s.geoSeq + 1;
            n.cullValid = true;
            n.cullStream = csId;
        }
        if (p.cs != kStCaller && !p.chainOnCs)
            E.wait(kStCaller, kEvFork);
        if (!p.fused) {
            E.kernel(kStCaller, kKOrder);
            E.kernel(kStCaller, kKRender);
        } else {
            /* the sky pixels on the side stream: concurrently with the geometry kernel, or (merge) after it */
            if (p.merge) {
                E.kernel(p.gs, kKChain, kEvGeoDone0 + p.half);
                E.record(p.gs, kEvGeometry);
                E.wait(kStSide, kEvGeoDone0 + p.half); /* (after the cull too: the geometry kernel follows it on gs) */
                E.kernel(kStSide, kKSky);
                n.skyPending[p.half] = true;
                n.skyKey[p.half] = r.key;
                n.skySeq[p.half] = ++n.skyCount;
                E.record(kStSide, kEvSkyDone0 + p.half);
                E.record(kStSide, kEvFrame);
                n.slotUsed[p.half] = true;
                n.flip = (s.flip + 1) % kSlots;
                return;
            }
            if (p.resume) {
                /* a pass: every pixel kernel on the caller's stream, the sky pass first (set_sample_range) */
                E.kernel(kStCaller, kKSky);
                E.kernel(kStCaller, kKChain);
                if (p.sampleCap > 0)
                    E.kernel(kStCaller, kKAccum);
                E.record(kStCaller, kEvGeometry);
                if (r.segments)
                    E.kernel(kStCaller, kKReduce);
                E.record(kStCaller, kEvFrame);
                return;
            }
            E.wait(kStSide, kEvFork);
            E.kernel(kStSide, kKSky);
            E.record(kStSide, kEvJoin);
            if (p.overlap) {
                n.skyPending[p.half] = true;
                n.skyKey[p.half] = r.key;
                n.skySeq[p.half] = ++n.skyCount;
            }
            /* kEvGeoDone[half]: the completion of the geometry stream's last kernel (the in-order sums, or the
             * geometry kernel when it sums in-kernel) */
            const bool accum = p.sampleCap > 0;
            E.kernel(p.gs, kKChain, p.overlap && !accum ? kEvGeoDone0 + p.half : kEvNone);
            if (accum)
                E.kernel(p.gs, kKAccum, p.overlap ? kEvGeoDone0 + p.half : kEvNone);
            E.record(p.gs, kEvGeometry);
            if (p.overlap) {
                /* no join: the frame is complete once the side stream has passed both passes; kEvSkyDone[half] marks
                 * that point, so a later launch that waits for this one waits for its geometry kernel too */
                E.wait(kStSide, kEvGeoDone0 + p.half);
                E.record(kStSide, kEvSkyDone0 + p.half);
                E.record(kStSide, kEvFrame);
                n.slotUsed[p.half] = true;
                n.flip = (s.flip + 1) % kSlots;
                return;
            }
            E.wait(kStCaller, kEvJoin);
            if (r.segments)
                E.kernel(kStCaller, kKReduce);
            E.record(kStCaller, kEvFrame);
            return;
        }
    }
    E.record(kStCaller, kEvGeometry);
    if (r.segments)
        E.kernel(kStCaller, kKReduce);
    E.record(kStCaller, kEvFrame);
}

namespace {
/* Every access of every kernel: a row counts when the launch binds its buffer and its predicate holds */
enum When : int { kAlways, kIfMerge, kIfNotMerge, kIfPrepCounts, kIfResumeRead };
struct Touch {
    int kernel, buf, access, when;
};
const Touch kTouches[] = {
    {kKPrep, kBufPrim, kWrite, kAlways},          {kKPrep, kBufGeoSet, kWrite, kIfPrepCounts},
    {kKSuperCull, kBufPrim, kRead, kAlways},      {kKSuperCull, kBufSuperMask, kWrite, kAlways},
    {kKTileCull, kBufPrim, kRead, kAlways},       {kKTileCull, kBufSuperMask, kRead, kAlways},
    {kKTileCull, kBufMask, kWrite, kAlways},      {kKTileCull, kBufPixMask, kWrite, kAlways},
    {kKTileCull, kBufWeight, kWrite, kAlways},    {kKTileCull, kBufGeoList, kWrite, kAlways},
    {kKTileCull, kBufPixItem, kWrite, kAlways},   {kKTileCull, kBufGeoSet, kAtomic, kAlways},
    {kKTileCull, kBufGeoSetNext, kWrite, kAlways},
    {kKSky, kBufPixMask, kRead, kAlways},         {kKSky, kBufPixItem, kRead, kAlways},
    {kKSky, kBufGeoColor, kRead, kAlways},        {kKSky, kBufGeoSet, kRead, kIfMerge}, /* the counts: an entry's item */
    {kKSky, kBufColors, kKeyedWrite, kAlways},    {kKSky, kBufAccum, kKeyedWrite, kAlways},
    {kKSky, kBufSegSlots, kAtomic, kAlways},
    {kKChain, kBufPrim, kRead, kAlways},          {kKChain, kBufMask, kRead, kAlways},
    {kKChain, kBufGeoList, kRead, kAlways},       {kKChain, kBufGeoSet, kRead, kAlways},
    {kKChain, kBufSamples, kWrite, kAlways},      {kKChain, kBufGeoColor, kWrite, kAlways}, /* (merge) or else Color: */
    {kKChain, kBufColors, kKeyedWrite, kIfNotMerge}, {kKChain, kBufAccum, kKeyedWrite, kAlways},
    {kKChain, kBufSegSlots, kAtomic, kAlways},
    {kKAccum, kBufGeoSet, kRead, kAlways},        {kKAccum, kBufSamples, kRead, kAlways},
    {kKAccum, kBufColors, kKeyedWrite, kAlways},  {kKAccum, kBufAccum, kKeyedWrite, kAlways},
    {kKOrder, kBufWeight, kRead, kAlways},        {kKOrder, kBufOrder, kWrite, kAlways},
    {kKRender, kBufPrim, kRead, kAlways},         {kKRender, kBufMask, kRead, kAlways},
    {kKRender, kBufOrder, kRead, kAlways},        {kKRender, kBufColors, kKeyedWrite, kAlways},
    {kKRender, kBufAccum, kKeyedWrite, kAlways},  {kKRender, kBufSegSlots, kAtomic, kAlways},
    {kKReduce, kBufSegSlots, kWrite, kAlways},    {kKReduce, kBufCallerSegments, kWrite, kAlways},
    /* a pass (the state buffer is bound in a pass only): every pixel kernel is declared to write the states
     * and, past the frame's first pass, to read them and the accumulator -- a superset (the accumulate pass touches no
     * state, the sky pass writes it in the first pass only) */
    {kKSky, kBufRngState, kKeyedWrite, kAlways},   {kKChain, kBufRngState, kKeyedWrite, kAlways},
    {kKAccum, kBufRngState, kKeyedWrite, kAlways}, {kKRender, kBufRngState, kKeyedWrite, kAlways},
    {kKSky, kBufRngState, kRead, kIfResumeRead},   {kKChain, kBufRngState, kRead, kIfResumeRead},
    {kKAccum, kBufRngState, kRead, kIfResumeRead}, {kKRender, kBufRngState, kRead, kIfResumeRead},
    {kKSky, kBufAccum, kRead, kIfResumeRead},      {kKChain, kBufAccum, kRead, kIfResumeRead},
    {kKAccum, kBufAccum, kRead, kIfResumeRead},    {kKRender, kBufAccum, kRead, kIfResumeRead},
    /* the scene records of the bound generation (triangles, materials, spheres, clustered records, balls): every kernel
     * that gets them (a superset: the culls read the spheres of a sphere launch only, and today's sky pass, whose
     * pixels' primary rays hit nothing, reads none) */
    {kKPrep, kBufSceneGen, kRead, kAlways},        {kKSuperCull, kBufSceneGen, kRead, kAlways},
    {kKTileCull, kBufSceneGen, kRead, kAlways},    {kKSky, kBufSceneGen, kRead, kAlways},
    {kKChain, kBufSceneGen, kRead, kAlways},       {kKRender, kBufSceneGen, kRead, kAlways},
    /* rtc_first_hit: the tile's candidate words (none with RTC_F_NO_TILE_CULL: unbound), the slot's primary
     * records, the scene records, and the caller's buffers */
    {kKFirstHit, kBufMask, kRead, kAlways},        {kKFirstHit, kBufPrim, kRead, kAlways},
    {kKFirstHit, kBufSceneGen, kRead, kAlways},    {kKFirstHit, kBufHit, kWrite, kAlways},
    /* the draw cache (rtc_plan.h Buf: the pool's blocks are append-only and in no row) */
    {kKTileCull, kBufDrawTable, kWrite, kAlways},  {kKTileCull, kBufItemDraw, kWrite, kAlways},
    {kKChain, kBufItemDraw, kRead, kAlways},
};
} // namespace

int kernel_footprint(const Plan &p, const Request &r, int kernel, Footprint *out, int max)
{
    /* the resources outside the slot, in Buf order: their kind and identity, one unit each */
    const struct { int res; unsigned long long id; } outside[kBufs - kScratchRegions] = {
        {kResPrim, (unsigned long long)p.half}, {kResGeoSet, p.geoSet}, {kResGeoSet, p.geoSetNext}, {kResSamples, 0},
        {kResSegSlots, 0}, {kResColors, r.key.colors}, {kResAccum, r.key.accum}, {kResCallerSegments, 0},
        {kResRngState, r.rngState}, {kResSceneGen, (unsigned long long)p.gen}, {kResHit, 0},
        {kResDrawTable, 0}, {kResItemDraw, (unsigned long long)p.half}};
    int k = 0;
    for (const Touch &t : kTouches) {
        const bool when = t.when == kAlways || (t.when == kIfResumeRead ? p.resumeRead
                                                : t.when == kIfPrepCounts ? p.prepCounts
                                                                          : p.merge == (t.when == kIfMerge));
        if (t.kernel != kernel || !p.binds(t.buf) || !when)
            continue;
        if (t.buf == kBufHit) { /* one row per buffer asked for, its identity the caller's */
            for (const uint64_t id : r.hit)
                if (id) {
                    if (k < max)
                        out[k] = Footprint{kResHit, t.access, id, 0, 1};
                    ++k;
                }
            continue;
        }
        if (k < max && t.buf < kScratchRegions)
            out[k] = Footprint{kResScratch, t.access, 0, p.slotOffset + p.reg[t.buf].offset,
                               p.slotOffset + p.reg[t.buf].offset + p.reg[t.buf].size};
        else if (k < max)
            out[k] = Footprint{outside[t.buf - kScratchRegions].res, t.access, outside[t.buf - kScratchRegions].id, 0, 1};
        ++k;
    }
    return k;
}

void plan_update(const State &s, int fault, UpdatePlan &u)
{
    memset(&u, 0, sizeof u);
    u.after = s;
    State &n = u.after;
    const int other = s.gen ^ 1;
    u.reads = s.gen;
    u.writes = fault == 3 ? s.gen : other;
    for (int h = 0; h < kSlots; ++h)
        if (s.slotGens[h] >> other & 1) {
            if (fault != 1)
                u.ops[u.nOps++] = Op{kOpWait, kStCaller, kEvSkyDone0 + h, -1};
            n.slotGens[h] = 0; /* the caller's stream is now past every launch of the slot */
        }
    u.ops[u.nOps++] = Op{kOpKernel, kStCaller, kEvNone, kKRefit};
    n.gen = u.writes;
    if (fault != 2)
        for (int h = 0; h < kSlots; ++h)
            n.prepValid[h] = false;
}

int update_footprint(const UpdatePlan &u, Footprint *out, int max)
{
    const Footprint f[2] = {{kResSceneGen, kWrite, (unsigned long long)u.writes, 0, 1},
                            {kResSceneGen, kRead, (unsigned long long)u.reads, 0, 1}};
    for (int k = 0; k < 2 && k < max; ++k)
        out[k] = f[k];
    return 2;
}

void plan_regroup(const State &s, int levels, RegroupPlan &g)
{
    memset(&g, 0, sizeof g);
    UpdatePlan u;
    plan_update(s, 0, u);
    g.reads = u.reads, g.writes = u.writes;
    g.levels = levels < 0 ? 0 : levels > kRegroupMaxLevels ? kRegroupMaxLevels : levels;
    for (int i = 0; i + 1 < u.nOps; ++i) /* the update's waits */
        g.ops[g.nOps++] = u.ops[i];
    g.ops[g.nOps++] = Op{kOpKernel, kStCaller, kEvNone, kKRegroupCentroids};
    for (int l = 0; l < g.levels; ++l)
        g.ops[g.nOps++] = Op{kOpKernel, kStCaller, kEvNone, kKRegroupLevel};
    g.ops[g.nOps++] = Op{kOpKernel, kStCaller, kEvNone, kKRegroupIndex};
    g.ops[g.nOps++] = u.ops[u.nOps - 1]; /* the refit */
    g.after = u.after;
}

int regroup_footprint(const RegroupPlan &g, int kernel, uint64_t scratch, Footprint *out, int max)
{
    const Footprint sr{kResRegroupScratch, kRead, scratch, 0, 1}, sw{kResRegroupScratch, kWrite, scratch, 0, 1};
    const Footprint mr{kResMembership, kRead, 0, 0, 1}, mw{kResMembership, kWrite, 0, 0, 1};
    Footprint f[3];
    int k = 0;
    if (kernel == kKRegroupCentroids) {
        f[k++] = sw;
    } else if (kernel == kKRegroupLevel) {
        f[k++] = sr, f[k++] = sw;
    } else if (kernel == kKRegroupIndex) {
        f[k++] = sr, f[k++] = mw;
    } else if (kernel == kKRefit) {
        UpdatePlan u{};
        u.reads = g.reads, u.writes = g.writes;
        k = update_footprint(u, f, 2);
        f[k++] = mr;
    }
    for (int j = 0; j < k && j < max; ++j)
        out[j] = f[j];
    return k;
}

void plan_query(const State &s, int kernel, TracePlan &t)
{
    memset(&t, 0, sizeof t);
    t.after = s; /* nothing the planner keeps changes */
    t.gen = s.gen;
    t.ops[t.nOps++] = Op{kOpKernel, kStCaller, kEvNone, kernel};
}

int query_footprint(const TracePlan &t, std::initializer_list<QueryRow> rows, Footprint *out, int max)
{
    int k = 0;
    const auto row = [&](const QueryRow &r) {
        if (!r.present)
            return;
        if (k < max)
            out[k] = Footprint{r.res, r.access, r.id, 0, 1};
        ++k;
    };
    row({kResSceneGen, kRead, (unsigned long long)t.gen, true});
    for (const QueryRow &r : rows)
        row(r);
    return k;
}

int trace_footprint(const TracePlan &t, uint64_t rays, const uint64_t hit[4], Footprint *out, int max)
{
    return query_footprint(t,
                           {{kResRays, kRead, rays, true},
                            {kResHit, kWrite, hit[0], hit[0] != 0},
                            {kResHit, kWrite, hit[1], hit[1] != 0},
                            {kResHit, kWrite, hit[2], hit[2] != 0},
                            {kResHit, kWrite, hit[3], hit[3] != 0}},
                           out, max);
}

int paths_footprint(const TracePlan &t, uint64_t rays, uint64_t seeds, uint64_t radiance, uint64_t seedsOut, bool segments,
                    bool readRadiance, Footprint *out, int max)
{
    return query_footprint(t,
                           {{kResRays, kRead, rays, true},
                            {kResSeeds, kRead, seeds, true},
                            {kResRadiance, kRead, radiance, readRadiance},
                            {kResRadiance, kWrite, radiance, true},
                            {kResSeeds, kWrite, seedsOut, seedsOut != 0},
                            {kResCallerSegments, kAtomic, 0, segments}},
                           out, max);
}

int occluded_footprint(const TracePlan &t, uint64_t rays, uint64_t tMax, uint64_t occluded, bool count, Footprint *out,
                       int max)
{
    return query_footprint(t,
                           {{kResRays, kRead, rays, true},
                            {kResTMax, kRead, tMax, tMax != 0},
                            {kResOccluded, kWrite, occluded, occluded != 0},
                            {kResCallerSegments, kAtomic, 0, count}},
                           out, max);
}

int pixels_footprint(const TracePlan &t, uint64_t pixels, uint64_t colors, uint64_t accum, uint64_t rngState, bool segments,
                     bool readState, Footprint *out, int max)
{
    return query_footprint(t,
                           {{kResPixelList, kRead, pixels, true},
                            {kResAccum, kRead, accum, readState},
                            {kResRngState, kRead, rngState, readState},
                            {kResAccum, kWrite, accum, true},
                            {kResRngState, kWrite, rngState, true},
                            {kResColors, kWrite, colors, colors != 0},
                            {kResCallerSegments, kAtomic, 0, segments}},
                           out, max);
}

} // namespace rtcplan

/* ---- the CPU test hook (include/rtc.h rtc_plan_sim_*) ---------------------------------------------------------- */
struct RtcPlanSim {
    rtcplan::State st;
    rtcplan::SceneShape shape; /* rtc_plan_sim_set_spheres: 0 spheres by default */
    int legacy;
    rtcplan::Plan last; /* rtc_plan_sim_regions */
    bool ranged;        /* rtc_plan_sim_set_sample_range: the next launch is a pass */
    int first, count;
    unsigned long long rngBuffer;
    int updateFault; /* rtc_plan_sim_set_update_fault */
    bool hitNext;    /* rtc_plan_sim_set_first_hit: the next launch is a first-hit launch */
    uint64_t hit[4];
    bool drawCache;  /* rtc_plan_sim_set_draw_cache: the scene has a draw cache and may use it in every launch shape */
};

namespace {
/* What every rtc_plan_sim_* hook hands back.  ops: 4 ints each (kind, stream, event, kernel), at most maxOps of them.  fp:
 * 6 u64 per row, at most maxFp rows, none when fp is null -- per kernel op written, its footprint entries (op index, res,
 * access, id, lo, hi: `footprint` fills at most `max` Footprints and returns how many there are), then the hook's trailer
 * (~0 and its five values).  Returns nOps | (rows, the trailer included) << 8, whatever fitted. */
template <class FootprintOf>
int serialise(const rtcplan::Op *o, int nOps, int *ops, int maxOps, unsigned long long *fp, int maxFp,
              const unsigned long long (&trailer)[5], FootprintOf footprint)
{
    int nf = 0;
    for (int i = 0; i < nOps && i < maxOps; ++i) {
        ops[4 * i] = o[i].kind, ops[4 * i + 1] = o[i].stream, ops[4 * i + 2] = o[i].event, ops[4 * i + 3] = o[i].kernel;
        if (o[i].kind != rtcplan::kOpKernel)
            continue;
        rtcplan::Footprint f[24];
        const int k = std::min(footprint(o[i], f, 24), 24);
        for (int j = 0; j < k; ++j, ++nf)
            if (fp && nf < maxFp) {
                unsigned long long *q = fp + 6 * (size_t)nf;
                q[0] = (unsigned long long)i, q[1] = (unsigned long long)f[j].res, q[2] = (unsigned long long)f[j].access;
                q[3] = f[j].id, q[4] = f[j].lo, q[5] = f[j].hi;
            }
    }
    if (fp && nf < maxFp) {
        unsigned long long *q = fp + 6 * (size_t)nf;
        q[0] = ~0ull;
        std::copy(trailer, trailer + 5, q + 1);
    }
    return nOps | ((nf + 1) << 8);
}

/* The encoding of each kind of plan, once: what its rtc_plan_sim_* hook hands back and what the executor records for
 * rtc_scene_last_plan (rtc_plan.h Recorded). */
/* a launch.  The trailer: the regrowth (hipFree + hipMalloc of the scratch or the sample slots: the device is synchronised
 * first; so it is before the draw cache is cleared or its item-draw arrays regrown) and the plan's shape */
int encode_launch(const rtcplan::Plan &p, const rtcplan::Request &r, int *ops, int maxOps, unsigned long long *fp, int maxFp)
{
    return serialise(p.ops, p.nOps, ops, maxOps, fp, maxFp,
                     {p.scratchGrow || p.samplesGrow || p.drawReset || p.itemDrawGrow, (unsigned long long)p.half,
                      p.chainOnCs, p.overlap, p.slotOffset},
                     [&](const rtcplan::Op &o, rtcplan::Footprint *f, int max) {
                         return rtcplan::kernel_footprint(p, r, o.kernel, f, max);
                     });
}
/* an update.  The trailer: (~0, nothing regrown, the generation written, -, -, -) */
int encode_update(const rtcplan::UpdatePlan &u, int *ops, int maxOps, unsigned long long *fp, int maxFp)
{
    return serialise(u.ops, u.nOps, ops, maxOps, fp, maxFp, {0, (unsigned long long)u.writes, 0, 0, 0},
                     [&](const rtcplan::Op &, rtcplan::Footprint *f, int max) {
                         return rtcplan::update_footprint(u, f, max);
                     });
}
/* a regroup.  The trailer: (~0, nothing regrown, the generation written, the levels, -, -) */
int encode_regroup(const rtcplan::RegroupPlan &g, uint64_t scratch, int *ops, int maxOps, unsigned long long *fp, int maxFp)
{
    return serialise(g.ops, g.nOps, ops, maxOps, fp, maxFp,
                     {0, (unsigned long long)g.writes, (unsigned long long)g.levels, 0, 0},
                     [&](const rtcplan::Op &o, rtcplan::Footprint *f, int max) {
                         return rtcplan::regroup_footprint(g, o.kernel, scratch, f, max);
                     });
}
/* a query, its one kernel's rows given.  The trailer: (~0, nothing regrown, the generation read, -, -, -) */
int encode_query(const rtcplan::TracePlan &t, const rtcplan::Footprint *rows, int n, int *ops, int maxOps,
                 unsigned long long *fp, int maxFp)
{
    return serialise(t.ops, t.nOps, ops, maxOps, fp, maxFp, {0, (unsigned long long)t.gen, 0, 0, 0},
                     [&](const rtcplan::Op &, rtcplan::Footprint *f, int max) {
                         std::copy(rows, rows + std::min(n, max), f);
                         return n;
                     });
}

/* a query, once its hook has refused what its entry point refuses: planned, the state adopted, and handed back */
template <class FootprintOf>
int sim_query(RtcPlanSim *s, int kernel, int *ops, int maxOps, unsigned long long *fp, int maxFp, FootprintOf footprint)
{
    rtcplan::TracePlan t;
    rtcplan::plan_query(s->st, kernel, t);
    s->st = t.after;
    rtcplan::Footprint rows[24];
    const int n = std::min(footprint(t, rows, 24), 24);
    return encode_query(t, rows, n, ops, maxOps, fp, maxFp);
}
} // namespace

namespace rtcplan {
/* A Recorded holds every operation any plan can have; its rows suffice for every plan there is (a launch has some 60),
 * and a plan that ever had more is not recorded in part: serialise counts what there is, not what fitted, so such a
 * record is void (encoded 0) and rtc_scene_last_plan never reads past what was stored. */
static_assert(sizeof Plan{}.ops / sizeof(Op) <= kRecordedOps && sizeof UpdatePlan{}.ops / sizeof(Op) <= kRecordedOps &&
                  sizeof RegroupPlan{}.ops / sizeof(Op) <= kRecordedOps && sizeof TracePlan{}.ops / sizeof(Op) <= kRecordedOps,
              "a Recorded holds the operations of every kind of plan");
static_assert(kRecordedOps <= 0xff, "nOps | rows << 8");
static int stored(int encoded)
{
    return (encoded & 0xff) <= kRecordedOps && (encoded >> 8) <= kRecordedRows ? encoded : 0;
}
void record_launch(const Plan &p, const Request &r, Recorded &out)
{
    out.encoded = stored(encode_launch(p, r, out.ops, kRecordedOps, out.fp, kRecordedRows));
}
void record_update(const UpdatePlan &u, Recorded &out)
{
    out.encoded = stored(encode_update(u, out.ops, kRecordedOps, out.fp, kRecordedRows));
}
void record_regroup(const RegroupPlan &g, uint64_t scratch, Recorded &out)
{
    out.encoded = stored(encode_regroup(g, scratch, out.ops, kRecordedOps, out.fp, kRecordedRows));
}
void record_query(const TracePlan &t, const Footprint *rows, int n, Recorded &out)
{
    out.encoded = stored(encode_query(t, rows, n, out.ops, kRecordedOps, out.fp, kRecordedRows));
}
} // namespace rtcplan

extern "C" int rtc_plan_sim_create(int triCount, int legacySlotLayout, RtcPlanSim **out)
{
    if (!out || triCount < 0)
        return RTC_EINVAL;
    RtcPlanSim *s = new RtcPlanSim();
    rtcplan::init(s->st);
    s->shape.triPadded = (triCount + 7) / 8 * 8;
    s->shape.maskWords = (s->shape.triPadded + 63) / 64;
    s->legacy = legacySlotLayout;
    *out = s;
    return 0;
}

extern "C" int rtc_plan_sim_set_spheres(RtcPlanSim *s, int sphereCount, int gateAllows)
{
    if (!s || sphereCount < 0)
        return RTC_EINVAL;
    s->shape.sphereCount = sphereCount;
    s->shape.splitGate = gateAllows != 0;
    return 0;
}

extern "C" int rtc_plan_sim_set_draw_cache(RtcPlanSim *s, int on)
{
    if (!s)
        return RTC_EINVAL;
    s->drawCache = on != 0;
    return 0;
}

extern "C" int rtc_plan_sim_set_sample_range(RtcPlanSim *s, int first, int count, unsigned long long rngBuffer)
{
    if (!s)
        return RTC_EINVAL;
    s->ranged = true;
    s->first = first, s->count = count, s->rngBuffer = rngBuffer;
    return 0;
}

extern "C" int rtc_plan_sim_set_first_hit(RtcPlanSim *s, unsigned long long prim, unsigned long long depth,
                                          unsigned long long normal, unsigned long long albedo)
{
    if (!s)
        return RTC_EINVAL;
    s->hitNext = true;
    s->hit[0] = prim, s->hit[1] = depth, s->hit[2] = normal, s->hit[3] = albedo;
    return 0;
}

extern "C" int rtc_plan_sim_release(RtcPlanSim *s)
{
    delete s;
    return 0;
}

extern "C" int rtc_plan_sim_launch(RtcPlanSim *s, const RtcRenderDesc *d, unsigned long long stream,
                                   unsigned long long colors, unsigned long long accum, int segments, const float cam[13],
                                   const float env[14], int *ops, int maxOps, unsigned long long *fp, int maxFp)
{
    if (!s || !d || !cam || !env)
        return RTC_EINVAL;
    rtcplan::Request r = rtcplan::make_request(*d, rtc_rows_selected(d), s->shape, stream, colors, accum, segments != 0,
                                               cam, env);
    r.legacySlotLayout = s->legacy != 0;
    if (s->hitNext) { /* a first-hit launch, refused as rtc_render_first_hit_async refuses it; consumed either way */
        s->hitNext = false;
        s->ranged = false;
        if (!(s->hit[0] | s->hit[1] | s->hit[2] | s->hit[3]) || (d->flags & ~RTC_F_NO_TILE_CULL) ||
            rtcplan::geometry_error(*d))
            return RTC_EINVAL;
        rtcplan::set_first_hit(r, s->hit);
    }
    if (s->ranged) { /* a pass, refused as rtc_render_samples_async refuses it; the range is consumed either way */
        s->ranged = false;
        if (s->first < 0 || s->count <= 0 || s->first > d->spp - s->count || (d->flags & RTC_F_OVERLAP) || !accum ||
            !s->rngBuffer)
            return RTC_EINVAL;
        rtcplan::set_sample_range(r, s->first, s->count, s->rngBuffer);
    }
    if (s->drawCache)
        rtcplan::set_draw_cache(r, 3);
    rtcplan::Plan &p = s->last;
    rtcplan::plan_launch(s->st, r, p);
    s->st = p.after;
    return encode_launch(p, r, ops, maxOps, fp, maxFp);
}

extern "C" int rtc_plan_sim_set_update_fault(RtcPlanSim *s, int mode)
{
    if (!s || mode < 0 || mode > 3)
        return RTC_EINVAL;
    s->updateFault = mode;
    return 0;
}

extern "C" int rtc_plan_sim_update(RtcPlanSim *s, unsigned long long stream, int *ops, int maxOps, unsigned long long *fp,
                                   int maxFp)
{
    if (!s || !ops)
        return RTC_EINVAL;
    (void)stream; /* (the caller's stream is stream 0 of the ops, whichever it is) */
    rtcplan::UpdatePlan u;
    rtcplan::plan_update(s->st, s->updateFault, u);
    s->st = u.after;
    return encode_update(u, ops, maxOps, fp, maxFp);
}

extern "C" int rtc_plan_sim_regroup(RtcPlanSim *s, unsigned long long stream, unsigned long long scratch, int *ops,
                                    int maxOps, unsigned long long *fp, int maxFp)
{
    /* refused as rtc_scene_regroup_async refuses it, as far as the planner sees it: no scratch, a misaligned one, a scene
     * without triangles or of more than the regroup takes */
    if (!s || !ops || !scratch || scratch % 16 || s->shape.triPadded <= 0 || s->shape.triPadded > kRegroupMaxTris)
        return RTC_EINVAL;
    (void)stream; /* (the caller's stream is stream 0 of the ops, whichever it is) */
    rtcplan::RegroupPlan g;
    rtcplan::plan_regroup(s->st, regroup_levels(s->shape.triPadded), g);
    s->st = g.after;
    return encode_regroup(g, scratch, ops, maxOps, fp, maxFp);
}

extern "C" int rtc_plan_sim_trace_rays(RtcPlanSim *s, unsigned long long stream, unsigned long long rays,
                                       const unsigned long long hit[4], int flags, int *ops, int maxOps,
                                       unsigned long long *fp, int maxFp)
{
    /* refused as rtc_trace_rays_async refuses it */
    if (!s || !ops || !rays || !hit || !(hit[0] | hit[1] | hit[2] | hit[3]) || (flags & ~RTC_F_NO_CLUSTER_CULL))
        return RTC_EINVAL;
    (void)stream; /* (the caller's stream is stream 0 of the ops, whichever it is) */
    const uint64_t ids[4] = {hit[0], hit[1], hit[2], hit[3]};
    return sim_query(s, rtcplan::kKTraceRays, ops, maxOps, fp, maxFp,
                     [&](const rtcplan::TracePlan &t, rtcplan::Footprint *f, int max) {
                         return rtcplan::trace_footprint(t, rays, ids, f, max);
                     });
}

extern "C" int rtc_plan_sim_trace_paths(RtcPlanSim *s, unsigned long long stream, unsigned long long rays,
                                        unsigned long long seeds, unsigned long long radiance,
                                        unsigned long long seedsOut, unsigned long long segments, int sampleFirst,
                                        int flags, int *ops, int maxOps, unsigned long long *fp, int maxFp)
{
    /* refused as rtc_trace_paths_async refuses it.  RTC_F_WAVE_PER_RAY changes the kernel alone: the same operation, the
     * same footprint */
    if (!s || !ops || !rays || !seeds || !radiance || sampleFirst < 0 ||
        (flags & ~(RTC_F_NO_CLUSTER_CULL | RTC_F_WAVE_PER_RAY)))
        return RTC_EINVAL;
    (void)stream; /* (the caller's stream is stream 0 of the ops, whichever it is) */
    return sim_query(s, rtcplan::kKTracePaths, ops, maxOps, fp, maxFp,
                     [&](const rtcplan::TracePlan &t, rtcplan::Footprint *f, int max) {
                         return rtcplan::paths_footprint(t, rays, seeds, radiance, seedsOut, segments != 0, sampleFirst > 0,
                                                         f, max);
                     });
}

extern "C" int rtc_plan_sim_occluded(RtcPlanSim *s, unsigned long long stream, unsigned long long rays,
                                     unsigned long long tMax, unsigned long long occluded, unsigned long long count,
                                     int flags, int *ops, int maxOps, unsigned long long *fp, int maxFp)
{
    /* refused as rtc_occluded_async refuses it */
    if (!s || !ops || !rays || !(occluded | count) || (flags & ~RTC_F_NO_CLUSTER_CULL))
        return RTC_EINVAL;
    (void)stream; /* (the caller's stream is stream 0 of the ops, whichever it is) */
    return sim_query(s, rtcplan::kKOccluded, ops, maxOps, fp, maxFp,
                     [&](const rtcplan::TracePlan &t, rtcplan::Footprint *f, int max) {
                         return rtcplan::occluded_footprint(t, rays, tMax, occluded, count != 0, f, max);
                     });
}

extern "C" int rtc_plan_sim_render_pixels(RtcPlanSim *s, unsigned long long stream, unsigned long long pixels,
                                          unsigned long long colors, unsigned long long accum, unsigned long long rng,
                                          unsigned long long segments, int first, int flags, int *ops, int maxOps,
                                          unsigned long long *fp, int maxFp)
{
    /* refused as rtc_render_pixels_async refuses it, as far as the planner sees it.  RTC_F_WAVE_PER_RAY changes the kernel
     * alone: the same operation, the same footprint */
    if (!s || !ops || !pixels || !accum || !rng || first < 0 || (flags & ~(RTC_F_NO_CLUSTER_CULL | RTC_F_WAVE_PER_RAY)))
        return RTC_EINVAL;
    (void)stream; /* (the caller's stream is stream 0 of the ops, whichever it is) */
    return sim_query(s, rtcplan::kKRenderPixels, ops, maxOps, fp, maxFp,
                     [&](const rtcplan::TracePlan &t, rtcplan::Footprint *f, int max) {
                         return rtcplan::pixels_footprint(t, pixels, colors, accum, rng, segments != 0, first > 0, f, max);
                     });
}

extern "C" int rtc_plan_sim_regions(const RtcPlanSim *s, unsigned long long *out, int maxRows)
{
    if (!s || !out || maxRows < 2 + rtcplan::kScratchRegions)
        return RTC_EINVAL;
    const rtcplan::Plan &p = s->last;
    unsigned long long *q = out;
    *q++ = p.slotOffset, *q++ = p.slotBytes, *q++ = p.scratchNeed;
    *q++ = p.after.scratchCap, *q++ = p.samplesNeed, *q++ = p.bound;
    for (int b = 0; b < rtcplan::kScratchRegions; ++b)
        if (p.binds(b))
            *q++ = (unsigned long long)b, *q++ = p.slotOffset + p.reg[b].offset, *q++ = p.reg[b].size;
    return (int)((q - out) / 3);
}
