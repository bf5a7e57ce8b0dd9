/*
 * rtc_plan.h -- the launch planner of rtc_render_rows_async (pure host code: no HIP, no device memory).
 *
 * One call of rtc_render_rows_async is the reference's render region (main.c:263-304) as a short sequence of kernels on
 * up to four streams: the caller's, two cull streams and the scene's side stream.  Pipelined
 * launches (RTC_F_OVERLAP) are in flight together, so every buffer two of them may touch at once needs either its own
 * copy (a scratch slot, a counter set) or an event between them.  rtc_plan_launch decides all of it from the scene's
 * ordering state and the launch's shape -- the scratch slot, the streams, every event record and wait, which kernels
 * run and which event each one completes -- as a list of operations; the HIP side only executes that list
 * (rtc_render.hip).  The same function drives the CPU test of the ordering (tests/test_plan.py through rtc_plan_sim_*),
 * which checks that every two kernels that may run together touch disjoint memory.
 *
 * A launch's buffers are described once, by the Buf enumeration: one table (rtc_plan.cpp layout_slot) gives every scratch
 * region its used size, alignment and padding, and one loop over it the offsets and the slot size; plan_launch records
 * which buffers the launch binds (Plan::bound); the executor takes every scratch pointer from those bound regions and
 * nothing else; and kernel_footprint evaluates one static list of (kernel, buffer, access) rows (kTouches) against
 * them, so the ordering test sees the regions the executor binds.  A new buffer is a name in Buf, a row in layout_slot's
 * table if it lies in the slot, its condition in plan_launch's bindings and its rows in kTouches.
 */
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>

#include "../../include/rtc.h"

namespace rtcplan {

constexpr int kSlots = 8;     /* scratch slots the pipelined launches cycle through (kSkySlots) */
constexpr int kGeoRing = 16;  /* geometry-pixel counter sets (one per split launch, a ring) */
constexpr int kGeoLists = 16; /* sub-lists per counter set */
constexpr int kGeoCountStride = 32;
/* a geometry pixel's item record in kBufGeoList: dword 0 = x | launch row << 16 (a launch of more than kItemCoordMax
 * columns or launch rows, Plan::wideItems: tile * 64 + bit), dwords 1-3 = the bits of its primary direction */
constexpr size_t kItemRecordBytes = 16;
constexpr int kItemCoordMax = 65535;
constexpr size_t kInlineSumPixels = 600000; /* small shares, and the alternating cull streams' limit for whole frames */
constexpr size_t kSuperCullPixels = 400000; /* launches of more pixels run rtc_super_cull */
/* the tile cull keeps a workgroup's prefilter survivors in LDS (maskWords u64, <= 48 KB: 393,216 triangles); larger
 * scenes render without it, and without the geometry kernel whose occupancy bounce_hit_share chooses */
constexpr int kMaxCullMaskWords = 6144;
constexpr size_t kSampleBufBudget = (size_t)2 << 30;
constexpr size_t kSampleSlotBytes = 12;
/* Sphere scenes through the split launch: at most kSplitSpheresMax spheres (the per-lane sphere loop of
 * more is the one-lane-per-pixel kernel's own work, and the cull's per-pixel sphere tests would dominate), and only scenes
 * whose bounce rays mostly escape -- the upload's probe hitShareAll at most kSplitMaxHitShare (a closed scene traces ~10
 * segments per sample, and a chain window spends one lane per state index: nine lanes in ten would be discarded).
 * kSplitMaxHitShare: see DESIGN §3.7 for the scenes it separates. */
constexpr int kSplitSpheresMax = 32;
constexpr double kSplitMaxHitShare = 0.5;

/* streams of a plan: the caller's, the scene's two cull streams and its side stream */
enum Stream : int { kStCaller = 0, kStCull0 = 1, kStCull1 = 2, kStSide = 3, kStreams = 4 };
/* events: the scene's own, per slot where they describe one slot's launch, and the caller's two hooks */
enum Event : int {
    kEvNone = -1,
    kEvCullSync = 0,
    kEvFork = 1,
    kEvJoin = 2,
    kEvSkyDone0 = 3,            /* + slot */
    kEvGeoDone0 = 3 + kSlots,   /* + slot */
    kEvFrame = 3 + 2 * kSlots,  /* the caller's frame event (rtc_scene_set_frame_event) */
    kEvGeometry = 4 + 2 * kSlots, /* the caller's geometry event */
    kEvents = 5 + 2 * kSlots
};
enum Kernel : int { kKPrep, kKSuperCull, kKTileCull, kKSky, kKChain, kKAccum, kKOrder, kKRender, kKReduce,
                    kKRefit /* rtc_scene_update_async's kernel (plan_update); never part of a launch */,
                    kKFirstHit /* rtc_render_first_hit_async's kernel (set_first_hit); of no other launch */,
                    kKTraceRays /* rtc_trace_rays_async's kernel (plan_query); never part of a launch */,
                    kKTracePaths /* rtc_trace_paths_async's kernel (plan_query); never part of a launch */,
                    kKOccluded /* rtc_occluded_async's kernel (plan_query); never part of a launch */,
                    /* rtc_scene_regroup_async's kernels before its refit (plan_regroup); never part of a launch */
                    kKRegroupCentroids, kKRegroupLevel, kKRegroupIndex,
                    kKRenderPixels /* rtc_render_pixels_async's kernel (plan_query); never part of a launch */ };
static_assert(kKRefit == 9 && kKFirstHit == 10 && kKTraceRays == 11 && kKTracePaths == 12 && kKOccluded == 13 &&
                  kKRegroupCentroids == 14 && kKRegroupLevel == 15 && kKRegroupIndex == 16 && kKRenderPixels == 17,
              "the kernels' numbers are the test hooks' encoding");
enum OpKind : int { kOpKernel = 0, kOpRecord = 1, kOpWait = 2 };
struct Op {
    int kind;   /* OpKind */
    int stream; /* Stream */
    int event;  /* record / wait: the event; kernel: the event its completion records (kEvNone: none) */
    int kernel; /* kernel ops: Kernel */
};

/* a stream's identity for the ordering state: the caller's hipStream_t value (0 = the null stream, a stream like any
 * other), or one of the scene's own */
constexpr uint64_t kIdCull0 = ~0ull - 1, kIdCull1 = ~0ull - 2;

/* what a pending (unjoined) sky pass writes: its Color / accumulator buffers and everything that decides their values */
struct Key {
    uint64_t colors, accum;
    float cam[13], env[14];
    int dims[9];
};

/* the per-scene ordering state (RtcDeviceScene::plan) */
struct State {
    int flip;                         /* the next overlapped launch's slot */
    bool slotUsed[kSlots];            /* an overlapped launch used the slot (its events are armed) */
    bool skyPending[kSlots];          /* that launch's sky pass has not been waited for by a later launch */
    Key skyKey[kSlots];
    unsigned long long skySeq[kSlots], skyCount;
    unsigned long long geoSeq;        /* split launches so far: the counter set is geoSeq % kGeoRing */
    bool cullValid;                   /* the last split launch's tile cull zeroed the next counter set ... */
    uint64_t cullStream;              /* ... on this stream (its completion: kEvFork) */
    bool prepValid[kSlots];           /* the slot's primary records are for prepOrigin, written on prepStream */
    uint64_t prepStream[kSlots];
    float prepOrigin[kSlots][3];
    size_t scratchCap, samplesCap;    /* bytes allocated (kSlots slots of scratch; the deferred sample slots) */
    bool cst2;                        /* the second cull stream exists */
    /* the scene records' two generations: launches bind generation `gen`; rtc_scene_update_async writes the
     * other one and makes it current.  slotGens[h] bit g: an overlapped launch of slot h read generation g, and no update
     * has waited for the slot's sky-done event since (that event covers every earlier launch of the slot: each one starts
     * after its predecessor ended).  Joined launches need no entry: they are complete at the caller's stream, which an
     * update follows -- the scene serves one stream at a time, and a caller that changes streams orders them (rtc.h). */
    int gen;
    unsigned char slotGens[kSlots];
    /* the draw cache: the frame size its slot table is built for (0 x 0: none yet) and the bytes allocated
     * for the slots' item-draw arrays */
    int drawWidth, drawHeight;
    size_t itemDrawCap;
};
void init(State &s);

/* the launch as the planner needs it */
struct Request {
    uint64_t stream; /* the caller's stream identity */
    int flags;       /* RTC_F_* */
    int width, rows, rowStride;
    int spp;
    int sphereCount; /* spheres the launch renders (0 with trianglesOnly) */
    bool sphereSplit; /* a launch with spheres may take the split launch (sphere_split) */
    int triPadded, maskWords;
    bool segments;   /* the caller asked for segment counters (a joined, counting launch) */
    Key key;
    float origin[3];
    bool legacySlotLayout; /* test hook: round 5's broken layout (slot h at h x this launch's slot size) */
    bool noMerge;          /* the sky pass beside the geometry kernel even where it could follow it (A/B) */
    /* a pass of rtc_render_samples_async (set_sample_range): samples [sampleFirst, sampleFirst + sampleCount)
     * of the frame's spp, from and into the caller's accumulator and RNG-state buffer */
    bool resume;
    int sampleFirst, sampleCount;
    uint64_t rngState;
    /* a first-hit launch (set_first_hit): the identities of the caller's prim, depth, normal and albedo
     * buffers, 0 where one is not asked for */
    bool firstHit;
    uint64_t hit[4];
    /* the scene's draw cache (set_draw_cache; 0: off or the scene cannot use it): bit 0, whole frames would run the chain
     * kernel without its GENERAL code as far as the scene decides it (one chunk, the primary filter records staged at the
     * whole frames' workgroups per CU); bit 1, small shares would.  The launch's own conditions are plan_launch's. */
    int drawCache;
    int height; /* the frame's (the slot table is indexed by x + y * width over the whole frame) */
};

/* the scene's shape as the planner needs it (RtcDeviceScene; rtc_plan_sim_create / _set_spheres) */
struct SceneShape {
    int triPadded, maskWords, sphereCount;
    bool splitGate; /* sphere_split's gate */
};
/* The one constructor of a Request (the executor's and the test hook's): rows = rtc_rows_selected(d); the key is the
 * camera cam[13] = origin, ex, ey, ez, fov, the environment env[14] = sun, horizon, zenith, ground, focus, intensity and
 * nine dims of the launch; legacySlotLayout and noMerge are left clear */
Request make_request(const RtcRenderDesc &d, int rows, const SceneShape &sc, uint64_t stream, uint64_t colors,
                     uint64_t accum, bool segments, const float cam[13], const float env[14]);

/* Makes r a pass: samples [first, first + count) of r.spp (the caller has checked the range), the RNG-state buffer's
 * identity.  A pass is never overlapped: its sky pass is joined, and runs on the caller's stream before the geometry
 * kernel -- both read and rewrite the accumulator (disjoint pixels, which the footprints do not tell apart) -- and it
 * never takes the alternating cull streams. */
void set_sample_range(Request &r, int first, int count, uint64_t rngState);

/* Makes r a first-hit launch (rtc_render_first_hit_async; the caller has checked that one identity is not 0 and that the
 * flags are RTC_F_NO_TILE_CULL at most).  It is never overlapped and keeps to the caller's stream (never the alternating
 * cull streams): rtc_prep_primary where slot 0's records are stale, rtc_super_cull above kSuperCullPixels, the triangle
 * tile cull, then rtc_first_hit -- no sky, chain, accumulate, order, render or reduce kernel, no Color or accumulator
 * buffer, no counter set, list or sample slot, and with RTC_F_NO_TILE_CULL no scratch at all.  It waits for an overlapped
 * launch still in flight in slot 0 and for no other; it records neither of the caller's two hooks. */
void set_first_hit(Request &r, const uint64_t ids[4]);

/* The scene's draw cache as the launch may use it (Request::drawCache) */
void set_draw_cache(Request &r, int eligible);

/* The geometry every launch's entry point checks (rtc_render_rows_async's check_arguments, the first-hit test hook):
 * 0 fine, 1 bad geometry (sizes, row selection, band), 2 a frame of more than 2^29 pixels */
int geometry_error(const RtcRenderDesc &d);

/* The launch-scoped buffers: the regions of one scratch slot, in slot order, then the resources outside it */
enum Buf : int {
    kBufMask,      /* per tile: maskWords u64 of candidate triangles */
    kBufPixMask,   /* per tile: its pixels with a candidate */
    kBufWeight,    /* per workgroup block: its weight (rtc_order_blocks) */
    kBufOrder,     /* launch slot -> workgroup block (one-lane-per-pixel kernel) */
    kBufGeoList,   /* kGeoLists sub-lists of geoCap geometry pixels' item records (kItemRecordBytes each) */
    kBufSuperMask, /* per superblock: maskWords u64 of survivors (rtc_super_cull) */
    kBufPixItem,   /* per pixel (tile * 64 + bit) of the geometry pixels: its item (merged sky pass) */
    kBufGeoColor,  /* per item: its Color bytes (merged sky pass) */
    kScratchRegions,
    kBufPrim = kScratchRegions, /* the slot's primary records */
    kBufGeoSet, kBufGeoSetNext, /* this split launch's counter set and the next one's */
    kBufSamples,                /* the deferred sample slots */
    kBufSegSlots,
    kBufColors, kBufAccum, kBufCallerSegments, /* the caller's */
    kBufRngState,               /* the caller's per-pixel RNG states (a pass, Request::resume) */
    kBufSceneGen,               /* the scene records of the bound generation (Plan::gen) */
    kBufHit,                    /* the caller's first-hit buffers (Request::hit: one footprint row per buffer asked for) */
    /* The draw cache (Plan::draws).  kBufDrawTable: the slot table (seed -> block) with the pool counter and the blocks'
     * seeds -- written by the tile cull (its lanes allocate; the fill kernel issued under the same operation moves the
     * fill mark) and touched by no other kernel; culls are ordered among themselves by kEvFork.  kBufItemDraw: the slot's
     * array of one block number per item, written by the tile cull beside the item record and read by the geometry
     * kernel.  The pool's blocks are in neither: they are append-only -- a block is written once, by the fill kernel of the
     * launch whose cull allocated it, which completes (the cull operation's event) before any geometry kernel that can
     * name the block starts; later culls and fills never touch an allocated block or a non-zero table entry. */
    kBufDrawTable, kBufItemDraw,
    kBufs
};
struct Region {
    size_t offset, size; /* inside the slot; size: the bytes in use (padding and alignment gaps belong to no region) */
};

struct Plan {
    bool empty;          /* no rows: only the caller's hooks are recorded */
    bool cull, fused, chain, overlap, smallShare, chainOnCs, superCull, debug;
    bool resume;         /* a pass (Request::resume): joined, one stream, the sky pass before the geometry kernel */
    bool resumeRead;     /* ... that starts from the stored accumulator and states (sampleFirst > 0) */
    bool merge;          /* the sky pass follows the geometry kernel and writes every pixel's Color in whole lines */
    int half;            /* the scratch slot */
    int gen;             /* the generation of scene records the launch's kernels read */
    int cs, gs;          /* the culls' stream and the geometry kernel's (Stream) */
    unsigned gridX, gridY, superX, superY;
    size_t blocks, tiles;
    int geoCap;
    bool wideItems;      /* more than kItemCoordMax columns or launch rows: the records keep tile * 64 + bit */
    size_t slotBytes;    /* bytes per slot (halfBytes: what this launch needs) */
    size_t slotOffset;   /* where slot `half` starts */
    Region reg[kScratchRegions];
    unsigned bound;      /* bit b: the launch binds Buf b (an unbound buffer: a null pointer, no footprint row) */
    bool binds(int b) const { return (bound >> b & 1u) != 0; }
    size_t scratchNeed;  /* kSlots x slotBytes: grow the scratch to it first (hipFree synchronises the device) */
    bool scratchGrow, samplesGrow, needCst2;
    size_t samplesNeed;
    int sampleCap;       /* items with a deferred slot (0: every geometry pixel sums in-kernel) */
    unsigned long long geoSet, geoSetNext; /* counter sets (ring indices) */
    bool prep, prepCounts; /* rtc_prep_primary runs, and zeroes the counter set too */
    bool cullPrio;
    /* the draw cache: the launch's tile cull allocates and fills blocks and its geometry kernel reads them; the cache is
     * cleared first (another frame size, or none yet), the item-draw arrays regrown first -- both behind a device
     * synchronisation; the bytes of all kSlots arrays and where this launch's starts */
    bool draws, drawReset, itemDrawGrow;
    size_t itemDrawNeed, itemDrawOffset;
    int nOps;
    Op ops[40];
    State after;         /* the ordering state once every operation is enqueued */
};

/* Whether a launch that renders sphereCount > 0 spheres may take the split launch: few enough spheres, the scene's gate
 * (or RTC_F_SPLIT_SPHERES), and none of the flags that select the one-lane-per-pixel kernel */
bool sphere_split(int sphereCount, bool gateAllows, int flags);

/* Plan one launch; `s` is not modified (the executor adopts plan.after once every operation is enqueued). */
void plan_launch(const State &s, const Request &r, Plan &p);

/* The memory one kernel of a plan touches, for the ordering test: resource kinds and byte ranges */
enum Res : int { kResScratch = 0, kResPrim = 1, kResGeoSet = 2, kResSamples = 3, kResSegSlots = 4, kResColors = 5,
                 kResAccum = 6, kResCallerSegments = 7, kResRngState = 8, kResSceneGen = 9 /* id: the generation */,
                 kResHit = 10 /* id: the caller's buffer */, kResRays = 11 /* id: the caller's ray buffer */,
                 kResDrawTable = 12, kResItemDraw = 13 /* id: the slot */,
                 kResSeeds = 14 /* id: the caller's seed buffer */, kResRadiance = 15 /* id: the caller's buffer */,
                 kResTMax = 16 /* id: the caller's limit buffer */, kResOccluded = 17 /* id: the caller's byte buffer */,
                 kResMembership = 18 /* the scene's cluster membership (clIndex) */,
                 kResRegroupScratch = 19 /* id: the caller's regroup scratch */,
                 kResPixelList = 20 /* id: the caller's list of pixels (rtc_render_pixels_async) */,
                 kResDrawPool = 21 /* the draw cache's blocks: append-only (Buf), so in no footprint row; rtc_scene_spans
                                      lists them under this number */ };
enum Access : int { kRead = 0, kWrite = 1, kAtomic = 2, kKeyedWrite = 3 /* writes values the key determines */ };
struct Footprint {
    int res, access;
    unsigned long long id; /* slot / set / buffer identity */
    unsigned long long lo, hi; /* byte range (scratch) or [0, 1) */
};
int kernel_footprint(const Plan &p, const Request &r, int kernel, Footprint *out, int max);

/* One rtc_scene_update_async: the refit kernel on the caller's stream writes the generation no launch
 * binds, after a wait for the sky-done event of every slot whose overlapped launches read that generation (the event
 * covers the slot's geometry kernel too); the written generation becomes current and every slot's primary records become
 * stale (they are derived from the triangles, not only from the camera origin).  Launches planned afterwards follow the
 * update: those on the caller's stream by stream order, those on a cull stream through kEvCullSync.
 * `fault`, a test hook like Request::legacySlotLayout (0: none): 1 drops the waits, 2 keeps the primary records valid,
 * 3 writes the current generation. */
struct UpdatePlan {
    int reads, writes; /* generations: the one a partial update copies from, the one the kernel writes */
    int nOps;
    Op ops[kSlots + 1];
    State after;
};
void plan_update(const State &s, int fault, UpdatePlan &u);
/* the refit kernel's footprint: the generation it writes and the one it may copy from */
int update_footprint(const UpdatePlan &u, Footprint *out, int max);

/* One rtc_scene_regroup_async: an update whose refit is preceded, on the caller's stream, by the kernels
 * that decide the membership anew -- the centroids, one kernel per level of the median split (`levels` of them:
 * regroup_levels of the scene's triangle count) and the one that writes the membership.  The waits, the generation
 * written and the state afterwards are plan_update's own (the plan is made from one); the membership is read by refits
 * alone, and refits are ordered on the caller's stream -- a scene serves one stream at a time --, so it needs no event and
 * no second copy: launches in flight read the records of their generation, never the membership. */
constexpr int kRegroupMaxLevels = 32;
struct RegroupPlan {
    int reads, writes; /* generations, as UpdatePlan's */
    int levels;
    int nOps;
    Op ops[kSlots + 3 + kRegroupMaxLevels];
    State after;
};
void plan_regroup(const State &s, int levels, RegroupPlan &g);
/* One regroup kernel's footprint.  The centroids: the scratch written (id: the caller's buffer).  A level: the scratch
 * read and written.  The index kernel: the scratch read, the membership written.  The refit: update_footprint's two rows,
 * then the membership read. */
int regroup_footprint(const RegroupPlan &g, int kernel, uint64_t scratch, Footprint *out, int max);

/* One query for caller-supplied rays -- rtc_trace_rays_async (kKTraceRays), rtc_trace_paths_async
 * (kKTracePaths, §3.12) or rtc_occluded_async (kKOccluded, §3.13) -- or one pass over a list of a frame's pixels
 * (rtc_render_pixels_async, kKRenderPixels, §3.17): one kernel on the caller's stream that reads the current
 * generation of the scene records and the caller's buffers and writes the caller's buffers.  It uses no scratch slot,
 * primary record, counter set, stream or event of the scene's, so it waits for nothing and arms nothing: stream order
 * alone places it after the update that wrote its generation and before the one that will rewrite it (an update writes
 * the generation no launch binds, on the caller's stream).  `after` equals the state it was planned from. */
struct TracePlan {
    int gen; /* the generation the kernel reads */
    int nOps;
    Op ops[1];
    State after;
};
void plan_query(const State &s, int kernel, TracePlan &t);
/* A query kernel's footprint: the generation read, then the query's own rows in the order given, those that are present
 * (a buffer not asked for has no row); every row is one unit, [0, 1) */
struct QueryRow {
    int res, access;
    unsigned long long id;
    bool present;
};
int query_footprint(const TracePlan &t, std::initializer_list<QueryRow> rows, Footprint *out, int max);

/* rtc_trace_rays_async: the generation read, the rays read (id: the buffer), one write per hit buffer asked for
 * (hit[k] == 0: not asked for), in that order */
int trace_footprint(const TracePlan &t, uint64_t rays, const uint64_t hit[4], Footprint *out, int max);
/* rtc_trace_paths_async, in this order: the generation read, the rays read, the seeds read (ids: the buffers), the
 * radiance read only when the call continues an accumulation (readRadiance: sampleFirst > 0), the radiance written, the
 * seeds written (id: the out buffer; 0: not asked for) and the caller's segment counter added to atomically (when asked
 * for; id 0 as in a launch's footprint) */
int paths_footprint(const TracePlan &t, uint64_t rays, uint64_t seeds, uint64_t radiance, uint64_t seedsOut, bool segments,
                    bool readRadiance, Footprint *out, int max);
/* rtc_occluded_async, in this order: the generation read, the rays read, the limits read (ids: the buffers; tMax 0: none
 * given), the bytes written (id: the buffer; 0: not asked for) and the caller's counter added to atomically (when asked
 * for; resource 7 with id 0, as in a launch's footprint) */
int occluded_footprint(const TracePlan &t, uint64_t rays, uint64_t tMax, uint64_t occluded, bool count, Footprint *out,
                       int max);
/* rtc_render_pixels_async, in this order: the generation read, the list read (id: the buffer), the accumulator and the RNG
 * states read only when the pass continues a frame (readState: first > 0), both written, the Color written (id: the
 * buffer; 0: not asked for) and the caller's segment counter added to atomically (when asked for; id 0 as in a launch's
 * footprint).  The accumulator, the states and the Color carry the resources a launch's footprint gives them. */
int pixels_footprint(const TracePlan &t, uint64_t pixels, uint64_t colors, uint64_t accum, uint64_t rngState, bool segments,
                     bool readState, Footprint *out, int max);

/* What a scene's most recent enqueue planned (RtcDeviceScene::lastPlan, rtc_scene_last_plan), kept as the rtc_plan_sim_*
 * hooks hand a plan back: 4 ints per operation, 6 u64 per footprint row, the hook's trailing ~0 record, and
 * encoded = nOps | rows << 8 (0: nothing enqueued yet).  Each record_* is the one encoding its rtc_plan_sim_* hook returns
 * too, filled from the plan the executor ran when every operation of it is enqueued: host stores, no device work. */
constexpr int kRecordedOps = 48, kRecordedRows = 256;
struct Recorded {
    int encoded;
    int ops[4 * kRecordedOps];
    unsigned long long fp[6 * kRecordedRows];
};
void record_launch(const Plan &p, const Request &r, Recorded &out);
void record_update(const UpdatePlan &u, Recorded &out);
void record_regroup(const RegroupPlan &g, uint64_t scratch, Recorded &out);
/* a query: `rows` is what its *_footprint call returned for `t` (n of them) */
void record_query(const TracePlan &t, const Footprint *rows, int n, Recorded &out);

} // namespace rtcplan
