/*
 * rtc_layout.h -- the device scene as librtc.so's translation units share it: the HBM records the kernels read
 * (triangles with precomputed edges, materials, per-launch primary records, triangle clusters), the bounce-ray cluster
 * test, and the per-scene host state (RtcDeviceScene: buffers, streams, the launch-ordering state).
 * Reference layout it replaces: Triangle / Sphere / Material (raytracing.h:7-69) and the arrays main.c:229-243 builds.
 */
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "../../include/rtc.h"
#include "rtc_device.h"
#include "rtc_plan.h"

using namespace rtcdev;

/* ---- device scene layout ------------------------------------------------------------------------- */
/* 64 B per triangle, read wave-uniformly by s_load_dwordx16: A, AB, AC, N (the reference's stored normal). */
struct __attribute__((aligned(64))) DevTri {
    float ax, ay, az, abx, aby, abz, acx, acy, acz, nx, ny, nz, pad0, pad1, pad2, pad3;
};
/* material, read only for the winning triangle */
struct __attribute__((aligned(32))) DevMat {
    float r, g, b, emission, smoothness, pad0, pad1, pad2;
};
struct __attribute__((aligned(16))) DevSphere {
    float cx, cy, cz, radius, r, g, b, emission, smoothness, pad0, pad1, pad2;
};
/* Per-launch records for primary rays (bounce 0): every primary ray starts at the camera origin O, so all
 * the quantities rayTriangle derives from the ray are LINEAR in its direction d:
 *   nd = d.N,  det = AB.(d x AC) = d.Gd,  uu = s0.(d x AC) = d.Gu,  vv = d.q0
 * with s0 = O - A, q0 = s0 x AB, Gd = AC x AB, Gu = AC x s0 (raytracing.c:189-206).
 * DevPrimF drives an exact-safe FILTER: FMA dot products against these vectors plus per-triangle error
 * bounds (rtc_prep_primary derives them in double) reject a lane only when the reference's own float
 * arithmetic provably rejects it.  Surviving lanes run the reference arithmetic with DevPrimX (AB, AC, s0,
 * q0 and dot(AC, q0) computed once per launch with the reference's f32 ops: bit-exact).
 *
 * Orientation folding: a hit needs dst = dot(AC, q0) * invDet >= EPSILON > 0, so sign(det) must equal the
 * sign of dAC0 = dot(AC, q0) -- a per-triangle constant for primary rays.  The filter vectors are stored
 * pre-multiplied by sigma = sign(dAC0) (exact negation), which turns the per-lane sign normalisation into
 * nothing: a lane is a candidate iff  sigma*det~ >= c  and  min(sigma*u~, sigma*v~, sigma*w~) >= -m. */
struct __attribute__((aligned(64))) DevPrimF { /* 64 B: one s_load_dwordx16 */
    float nx, ny, nz, mnd;      /* N and the nd margin (-inf: the triangle can never be hit, skip it) */
    float gdx, gdy, gdz, c;     /* sigma*Gd and the det threshold c = EPSILON - ed, rounded down */
    float gux, guy, guz, negm;  /* sigma*Gu and -m (the combined edge margin, negated) */
    float q0x, q0y, q0z, pad0;  /* sigma*q0 */
};
struct __attribute__((aligned(64))) DevPrimX {
    float abx, aby, abz, acx, acy, acz, s0x, s0y, s0z, q0x, q0y, q0z, dac0, pad[3];
};

/* The pixel -> primary ray map and the primary filter's per-pixel verdict, shared by the render kernels (rtc_render.hip,
 * where the proofs are) and the filter's soundness probe (rtc_probe_primary_cull).  P is any record with the launch's
 * width, height, rowStart, rowStride, rowBandShift, ex, ey, ez and fov: RenderParams, or the probe's PrimaryView. */
struct PrimaryView {
    int width, height, rows, rowStart, rowStride, rowBandShift;
    V3 ex, ey, ez;
    float fov;
};

template <typename PT> __device__ __forceinline__ V3 primary_dir(const PT &P, int x, int y)
{
    /* integer halves, then int->float, f32 divide */
    const float dx = (float)(x - P.width / 2) / (float)(P.height / 2);
    const float dy = (float)(y - P.height / 2) / (float)(P.height / 2);
    return normalized(add(add(mul(P.ex, dx), mul(P.ey, dy)), mul(P.ez, P.fov)));
}

/* Launch row r -> image row y: y = rowStart + k*rowStride (main.c:84's interleave), or bands of 2^rowBandShift rows
 * (rtc.h rowBand): y = rowStart + (r / B)*rowStride*B + r % B */
template <typename PT> __device__ __forceinline__ int launch_row_y(const PT &P, int r)
{
    const int sh = P.rowBandShift;
    return P.rowStart + ((r >> sh) * P.rowStride << sh) + (r & ((1 << sh) - 1));
}

__device__ __forceinline__ float fdot(V3 d, float x, float y, float z) { return fmaf(d.z, z, fmaf(d.y, y, d.x * x)); }

__device__ __forceinline__ bool prim_backfacing(V3 dir, const DevPrimF &F)
{
    return fdot(dir, F.nx, F.ny, F.nz) > F.mnd;
}

__device__ __forceinline__ bool prim_pass(V3 dir, const DevPrimF &F)
{
    const float dt = fdot(dir, F.gdx, F.gdy, F.gdz);
    const float ut = fdot(dir, F.gux, F.guy, F.guz);
    const float vt = fdot(dir, F.q0x, F.q0y, F.q0z);
    const float wt = (dt - ut) - vt;
    return (dt >= F.c) & (fminf(fminf(ut, vt), wt) >= F.negm);
}

/* The tile prefilter (its derivation: rtc_cull.h, "Tile prefilter"): the cone of a pixel rectangle and the test that no
 * pixel of it can pass the filter for a record.  P: as for primary_dir, with the launch's `rows`. */
struct TileCone {
    double c[4][3];
    double vmin, vmax, eDir;
    double ivmin, ivmax; /* 1 / vmin, 1 / vmax (cone_range multiplies and widens instead of dividing) */
    bool ok;
};

/* the cone of the pixel rectangle [x0, x1] x [r0, r1] (launch rows) */
template <typename PT> __device__ TileCone rect_cone(const PT &P, int x0, int x1, int r0, int r1)
{
    TileCone K;
    x1 = min(x1, P.width - 1);
    r1 = min(r1, P.rows - 1);
    const int y0 = launch_row_y(P, r0), y1 = launch_row_y(P, r1); /* (y is increasing in the launch row) */
    /* the same f32 expressions as primary_dir */
    const float dxs[2] = {(float)(x0 - P.width / 2) / (float)(P.height / 2),
                          (float)(x1 - P.width / 2) / (float)(P.height / 2)};
    const float dys[2] = {(float)(y0 - P.height / 2) / (float)(P.height / 2),
                          (float)(y1 - P.height / 2) / (float)(P.height / 2)};
    const double ezl = sqrt((double)P.ez.x * P.ez.x + (double)P.ez.y * P.ez.y + (double)P.ez.z * P.ez.z);
    double vmin = 1e300, vmax = 0.0;
    bool finite = ezl > 0.0 && ezl < 1e300;
    for (int k = 0; k < 4; ++k) {
        const double dx = dxs[k & 1], dy = dys[k >> 1];
        const double v[3] = {(double)P.ex.x * dx + (double)P.ey.x * dy + (double)P.ez.x * P.fov,
                             (double)P.ex.y * dx + (double)P.ey.y * dy + (double)P.ez.y * P.fov,
                             (double)P.ex.z * dx + (double)P.ey.z * dy + (double)P.ez.z * P.fov};
        for (int i = 0; i < 3; ++i) {
            K.c[k][i] = v[i];
            finite = finite && (v[i] - v[i] == 0.0);
        }
        vmax = fmax(vmax, sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]));
        vmin = fmin(vmin, (v[0] * P.ez.x + v[1] * P.ez.y + v[2] * P.ez.z) / ezl);
    }
    const double u = 5.9604644775390625e-08;
    const double S = fmax(fabs((double)dxs[0]), fabs((double)dxs[1])) + fmax(fabs((double)dys[0]), fabs((double)dys[1])) +
                     fabs((double)P.fov);
    K.vmin = vmin * (1.0 - 1e-12);
    K.vmax = vmax * (1.0 + 1e-12);
    K.eDir = 16.0 * u * S / K.vmin + 4.0 * u;
    K.ivmin = 1.0 / K.vmin;
    K.ivmax = 1.0 / K.vmax;
    /* basis components <= 1 (normalized f32 vectors) is assumed by the error bound */
    const bool unitBasis = fabs(P.ex.x) <= 1.0001f && fabs(P.ex.y) <= 1.0001f && fabs(P.ex.z) <= 1.0001f &&
                           fabs(P.ey.x) <= 1.0001f && fabs(P.ey.y) <= 1.0001f && fabs(P.ey.z) <= 1.0001f &&
                           fabs(P.ez.x) <= 1.0001f && fabs(P.ez.y) <= 1.0001f && fabs(P.ez.z) <= 1.0001f;
    K.ok = finite && unitBasis && K.vmin > 1e-6 && K.eDir < 1e-3 && S - S == 0.0;
    return K;
}

template <typename PT> __device__ TileCone tile_cone(const PT &P, int tx, int ty)
{
    return rect_cone(P, tx * 8, tx * 8 + 7, ty * 8, ty * 8 + 7);
}

/* [LB, UB] of g.v/|v| over the tile (see TileCone) */
__device__ __forceinline__ void cone_range(const TileCone &K, double gx, double gy, double gz, double &lb, double &ub)
{
    double mx = -1e300, mn = 1e300;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double a = gx * K.c[k][0] + gy * K.c[k][1] + gz * K.c[k][2];
        mx = fmax(mx, a);
        mn = fmin(mn, a);
    }
    /* mx / vmin (or / vmax) as a product with the rounded reciprocal: two double roundings, < 2^-51 relative, so
     * widening by 2^-50 of the magnitude keeps ub above (lb below) the exact quotient -- the bound only loosens */
    ub = mx * (mx >= 0.0 ? K.ivmin : K.ivmax);
    lb = mn * (mn >= 0.0 ? K.ivmax : K.ivmin);
    ub += fabs(ub) * 0x1p-50;
    lb -= fabs(lb) * 0x1p-50;
}

/* true: no pixel of the tile can pass prim_backfacing / prim_pass for F */
__device__ bool tile_prunes(const TileCone &K, const DevPrimF &F)
{
    const double u = 5.9604644775390625e-08;
    const double e = K.eDir + 3.01 * u;
    auto n1 = [](double a, double b, double c) { return fabs(a) + fabs(b) + fabs(c); };
    double lb, ub;
    /* every pixel back-facing: nd > mnd */
    cone_range(K, F.nx, F.ny, F.nz, lb, ub);
    if (lb - n1(F.nx, F.ny, F.nz) * e > (double)F.mnd)
        return true;
    const double nd = n1(F.gdx, F.gdy, F.gdz), nu = n1(F.gux, F.guy, F.guz), nv = n1(F.q0x, F.q0y, F.q0z);
    cone_range(K, F.gdx, F.gdy, F.gdz, lb, ub);
    if (ub + nd * e < (double)F.c)
        return true;
    cone_range(K, F.gux, F.guy, F.guz, lb, ub);
    if (ub + nu * e < (double)F.negm)
        return true;
    cone_range(K, F.q0x, F.q0y, F.q0z, lb, ub);
    if (ub + nv * e < (double)F.negm)
        return true;
    /* wt = (dt - ut) - vt: the three slacks plus two f32 subtractions */
    cone_range(K, (double)F.gdx - F.gux - F.q0x, (double)F.gdy - F.guy - F.q0y, (double)F.gdz - F.guz - F.q0z, lb,
               ub);
    if (ub + (nd + nu + nv) * (e + 2.01 * u * 1.0001) < (double)F.negm)
        return true;
    return false;
}

/* ---- triangle clusters for bounce rays (rtc_render_chain) -----------------------------------------------
 * The triangles are grouped into clusters of kClusterSize (spatial median splits, rtc_build_clusters); a
 * bounce ray skips a whole cluster when its half-line provably passes farther from the cluster's bounding
 * ball than any point rayTriangle could report.  Bound (SURVEY Appendix A arithmetic, unit roundoff
 * u = 2^-24): for a reported hit (|det| >= EPSILON, u, v in the triangle, dst >= EPSILON) the exact point
 * pos + dst*dir lies within
 *     eps = rho * (alpha + beta * S) + gamma * (S + E)
 * of the triangle, where rho >= |dir|, S >= |pos - A|, E = the cluster's longest AB / AC edge, and
 *     beta = F k 45 u E^2 / EPSILON,  alpha = F k 32 u E^3 / EPSILON,  k = 1 / (1 - 8 u E^2 rhoMax / EPSILON)
 * (forward error of the f32 cross / dot products over the Cramer solution, divided by |det| >= EPSILON;
 * safety factor F = 4; gamma covers the f32 evaluation of the cull test itself).  Clusters with
 * 8 u E^2 rhoMax / EPSILON >= 1/2, and rays with |dir|_1 > rhoMax, are never culled. */
constexpr int kClusterSize = 8;
constexpr int kChunkClusters = 32; /* clusters per chunk (one 32-bit cull mask per lane in rtc_render_chain) */
constexpr float kClusterRhoMax = 4.f;
constexpr float kClusterGamma = 2e-5f;
struct __attribute__((aligned(32))) DevCluster {
    float cx, cy, cz, r;          /* bounding ball (every vertex A, A+AB, A+AC of the cluster inside) */
    float alpha, beta, gammaE, e; /* the eps terms above: alpha, beta, gamma*E (or +inf: never cull), E */
};

/* The scene's own events only order its streams on one device (the caller's frame / geometry events keep their
 * flags): no system-scope fence when they are recorded (1/8 share 0.100 -> 0.094 ms, round 3) */
constexpr unsigned kOrderEventFlags = hipEventDisableTiming | hipEventDisableSystemFence;
/* An unjoined sky pass (RTC_F_OVERLAP) writes its launch's Color (and accumulator) rows: what it writes where */
constexpr int kSkySlots = 8;
#ifndef RTC_CHAIN_WGS_FULL
#define RTC_CHAIN_WGS_FULL 3
#endif
/* Small shares of more pixels (the 1080p 1/4 share, 518 k px) run the tile cull at issue priority 3 as well: the next
 * share's cull then competes on equal terms with this share's geometry kernel (1/4 share 0.1205 -> 0.1170 ms; the 1/8
 * share measured no better that way, profiles/r05_cpq_ab_cull_priority.log) */
constexpr size_t kCullPrioMinPixels = 400000;
/* Wave priority of the geometry kernel (s_setprio): its waves are issued before the sky pass's on a shared SIMD.  A row
 * share's chain kernel runs ~3 pixels per wave; as its waves retire, sky waves fill their slots and the remaining chain
 * waves -- the share's critical path -- got a sixth of the issue: a wave's third and fourth pixels took 2-7x its first
 * (tools/wave_spread.py).  Round 5: 1080p 1/8 share 0.0757 -> 0.0697 ms, whole frames unchanged (the sky pass still
 * fills the chain kernel's idle slots); the tile cull at priority 3 too within noise of it
 * (profiles/r05_pr_ab_wave_priority.log) */
#ifndef RTC_CHAIN_PRIO
#define RTC_CHAIN_PRIO 3
#endif
#ifndef RTC_CHAIN_WGS_HIT
#define RTC_CHAIN_WGS_HIT 4 /* whole frames of scenes whose bounce-hit share (bounce_hit_share) exceeds kWgsHitShare */
#endif
constexpr double kWgsHitShare = 0.15;

/* rtc_render_chain's geometry-pixel sub-lists: kGeoLists counters, kGeoCountStride ints (one 128-B line) apart; a ring
 * of kGeoRing counter sets of kGeoSetInts ints (see RtcDeviceScene::geoCounts) */
constexpr int kGeoLists = 16, kGeoCountStride = 32;
constexpr int kItemRecDwords = 4; /* a geometry pixel's item record (item_record, rtc_params.h) */
constexpr int kGeoRing = 16, kGeoSetInts = kGeoLists * kGeoCountStride;
static_assert(kGeoSetInts >= kGeoLists * kGeoCountStride, "a counter set holds every sub-list counter");
static_assert(kSkySlots == rtcplan::kSlots && kGeoRing == rtcplan::kGeoRing && kGeoLists == rtcplan::kGeoLists &&
                  kGeoCountStride == rtcplan::kGeoCountStride && kItemRecDwords * 4 == rtcplan::kItemRecordBytes,
              "the planner's slot and counter-set layout is the device's");
/* The draw cache's blocks and counter words (rtc_params.h DrawCache) */
constexpr int kDrawEntries = 64; /* entries (float4) per block: one window's lanes */
constexpr size_t kDrawBlockBytes = kDrawEntries * 16;
enum DrawCtr : int {
    kDcTaken = 0,    /* blocks handed out (may pass the capacity by requests that were not granted: readers clamp) */
    kDcFilled0 = 1,  /* the fill mark, alternating between two words by the fill's parity: a fill reads its own ... */
    kDcFilled1 = 2,  /* ... and writes the next fill's, so no workgroup reads the word another one writes */
    kDcUncachedAcc = 3, /* this launch's items without a block so far (the fill moves it to kDcUncached and zeroes it) */
    kDcFresh = 4, kDcUncached = 5, /* the last launch's fresh and uncached items (rtc_scene_draw_cache_stats) */
    kDcWords = 8
};
/* One generation of the scene records: everything a launch reads of the scene's geometry.  A scene keeps two
 * (DESIGN §3.9): launches read the current one, rtc_scene_update_async writes the other and makes it current. */
struct SceneRecords {
    DevTri *tris;       /* triPadded + 8 records in reference order (the padding records stay zero) */
    DevMat *mats;
    DevSphere *spheres;
    DevTri *clTris;     /* clusterCount * kClusterSize records in cluster order, pad0 = reference index (int) */
    DevCluster *clusters;
    DevCluster *chunks; /* chunkCount balls over kChunkClusters consecutive clusters */
};
/* The six arrays of a SceneRecords, named once: whatever allocates, copies, frees, sizes or reports them walks this table
 * (the Python side's RECORD_ARRAYS has the same names in the same order). */
enum SceneArrayId : int { kArrTris, kArrMats, kArrSpheres, kArrClTris, kArrClusters, kArrChunks, kSceneArrayCount };
struct SceneArray {
    const char *name;
    size_t elem; /* bytes per record */
    size_t at;   /* where the array's pointer lives in a SceneRecords */
};
constexpr SceneArray kSceneArrays[kSceneArrayCount] = {
    {"tris", sizeof(DevTri), offsetof(SceneRecords, tris)},
    {"mats", sizeof(DevMat), offsetof(SceneRecords, mats)},
    {"spheres", sizeof(DevSphere), offsetof(SceneRecords, spheres)},
    {"clTris", sizeof(DevTri), offsetof(SceneRecords, clTris)},
    {"clusters", sizeof(DevCluster), offsetof(SceneRecords, clusters)},
    {"chunks", sizeof(DevCluster), offsetof(SceneRecords, chunks)},
};
static_assert(sizeof(SceneRecords) == kSceneArrayCount * sizeof(void *), "every pointer of a SceneRecords is in the table");
inline void *&scene_array(SceneRecords &g, int k)
{
    return *reinterpret_cast<void **>(reinterpret_cast<unsigned char *>(&g) + kSceneArrays[k].at);
}
inline void *scene_array(const SceneRecords &g, int k) { return scene_array(const_cast<SceneRecords &>(g), k); }
struct RtcDeviceScene {
    int device;
    int cuCount; /* compute units of the device (the persistent chain kernel's workgroups are a multiple of it) */
    int triCount, triPadded, sphereCount; /* triPadded: multiple of kUnroll, zero (never-hit) records */
    int clusterCount;   /* ceil(triCount / kClusterSize) */
    int chunkCount;
    /* the box of the upload's triangle vertices and sphere extents (centre -+ r), kept on the host for the ray order's key
     * (rtc_scene_bounds); an update does not move it: the key only affects speed.  An empty scene: zeros. */
    float boundsLo[3], boundsHi[3];
    SceneRecords gen[2]; /* by generation; a launch binds gen[Plan::gen] */
    /* the generation a launch enqueued now would read (probes, rtc_cull_items) */
    const SceneRecords &current() const { return gen[plan.gen]; }
    /* clustered record -> reference index (-1: padding), clusterCount * kClusterSize ints: the cluster membership, decided
     * at upload and again by every rtc_scene_regroup_async.  One copy serves both generations: only refits
     * read it (rtc_refit) and only a regroup's index kernel writes it, all of them on the caller's stream, and a scene serves
     * one stream at a time (rtc.h), so stream order alone puts every read after the write it means and before the next.
     * Launches in flight read the records of their generation, never this. */
    int *clIndex;
    size_t recBytes[kSceneArrayCount]; /* bytes of each array of kSceneArrays (each generation) */
    /* per-launch primary records, one copy per scratch slot (primStride records each), written by rtc_prep_primary:
     * an overlapped launch's preparation (on the cull stream) may run while the previous frame's geometry kernel still
     * reads its own copy */
    DevPrimF *primF;
    DevPrimX *primX;
    size_t primStride;
    /* per-launch scratch: kSkySlots slots, each the regions of rtcplan::Buf (candidate bit-sets, pixel masks, weights,
     * dispatch order, geometry-pixel sub-lists, superblock survivors, the merged sky pass's items and colours) at the
     * offsets of the planner's region table; a launch's kernels get the regions its plan binds (Plan::bound) and no
     * other pointer into it; grown on demand (plan.scratchCap bytes) */
    unsigned char *scratch;
    /* rtc_render_chain's sub-list counters: a ring of kGeoRing sets, set q % kGeoRing for the q-th split launch;
     * each launch's tile cull zeroes the next launch's set */
    int *geoCounts;
    double hitShare;  /* bounce_hit_share at upload */
    int chainWgsFull; /* rtc_render_chain workgroups per CU for whole frames */
    double hitShareAll;   /* the same probe with the spheres as origins and targets too (== hitShare without spheres) */
    bool sphereSplitGate; /* launches with spheres may take the split launch (rtcplan::sphere_split's gate) */
    /* every ordering decision's state: slots, pending sky passes, counter sets, prep records (rtc_plan.h) */
    rtcplan::State plan;
    /* streams: overlapped launches prepare, cull and run their geometry kernel on `cst` or `cst2` (high priority, by
     * slot parity); the sky pass runs on `side` (low priority) */
    hipStream_t cst;
    hipStream_t cst2; /* the second cull stream (odd slots; created on first use) */
    hipStream_t side;
    /* the scene's ordering events (rtcplan::Event): the caller stream's position when the culls move to a cull stream,
     * the tile cull's completion (the sky pass forks there), the sky pass's end, and per slot the end of its launch's
     * sky pass (after its geometry kernel) and of its geometry kernel */
    hipEvent_t evCullSync, evFork, evJoin;
    hipEvent_t evSkyDone[kSkySlots], evGeoDone[kSkySlots];
    hipEvent_t frameEvent; /* caller's (rtc_scene_set_frame_event) or null */
    /* caller's event (rtc_scene_set_geometry_event): recorded on the caller's stream once a launch's
     * geometry-pixel kernels are enqueued (before the join with the sky pass); null: none */
    hipEvent_t geoEvent;
    /* rtc_render_chain's deferred accumulation: the accumulated samples' radiance per geometry pixel (grown on demand,
     * <= kSampleBufBudget bytes: plan.samplesCap) */
    unsigned char *samples;
    int maskWords;     /* ceil(triPadded / 64) */
    unsigned long long *segSlots; /* per-launch partial segment counters */
    /* timing events around the split launch's two kernels (rtc_scene_kernel_times) */
    hipEvent_t evHeavy0, evHeavy1, evSky0, evSky1;
    bool timing; /* record them (rtc_scene_set_timing; off by default: each record costs the launch a few us) */
    bool timed;  /* the last launch was a split launch that recorded them */
    RtcChainReport chainReport; /* what the last geometry-kernel launch chose (run_chain; rtc_scene_chain_report) */
    /* what the last enqueue planned -- a launch, a pass, a first-hit launch, an update, a regroup, a query, a pixel pass --
     * recorded once every operation of its plan is enqueued (host stores only; rtc_scene_last_plan) */
    rtcplan::Recorded lastPlan;
    /* The draw cache (rtc_params.h DrawCache), allocated at the first launch that uses it and freed with the
     * scene.  The pool's blocks are append-only -- written once by the fill behind the cull that allocated them, before
     * any geometry kernel that can name them; never touched again -- which is why launches in flight may read them while
     * a later launch's cull and fill run.  Cleared (table, counters) behind a device synchronisation when the frame size
     * changes (plan.drawWidth x plan.drawHeight: what the table is built for). */
    struct Draws {
        long long blocks;        /* the capacity asked for (rtc_scene_set_draw_cache; < 0: the default; 0: off) */
        unsigned *table;         /* tablePixels entries */
        size_t tablePixels;
        unsigned *ctr;           /* DrawCtr words */
        unsigned *blockSeed;     /* capacity entries */
        void *pool;              /* capacity blocks of 1 KB */
        size_t capacity;         /* blocks allocated (0: not yet) */
        unsigned char *itemDraw; /* kSkySlots arrays (plan.itemDrawCap bytes) */
        int parity;              /* the next fill's (DrawCtr kDcFilled0 / 1) */
    } draws;
};
constexpr long long kDrawCacheDefaultBytes = 1ll << 30; /* of 1-KB blocks, at most the frame's pixel count */

/* A split launch's geometry-pixel lists once its culls have run, for rtc_probe_item_records: the launch's preparation,
 * superblock and tile culls on the null stream and none of its render kernels (rtc_render.hip); device pointers into the
 * launch's counter set and scratch slot, valid until the scene's next launch */
struct RtcCullItems {
    const int *geoCount;      /* sub-list l's entries: geoCount[l * kGeoCountStride] (clamp to geoCap) */
    const unsigned *geoList;  /* sub-list l's records from l * geoCap * kItemRecDwords */
    const unsigned long long *pixMask;
    int geoCap, tilesX;
    size_t tiles;
    int wide;                 /* the records keep tile * 64 + bit (RenderParams::wideItems) */
    /* for rtc_probe_primary_cull: the tiles' candidate bit-sets (maskWords u64 per tile; a split launch leaves the words
     * of a workgroup without a survivor unwritten: its tiles' pixMask is 0), the launch's primary filter records, and
     * whether rtc_super_cull (level 0) ran */
    const unsigned long long *tileMask;
    int maskWords;
    const DevPrimF *primF;
    int triPadded;
    int level0;
};
int rtc_cull_items(const RtcDeviceScene *s, const Scene *scene, const RtcCamera *cam, const RtcRenderDesc *d,
                   void *dColors, RtcCullItems *items);
/* The draw cache's memory for a launch that uses it (rtc_scene.hip; the scene's device is current): the first such launch
 * allocates; `reset` (another frame size, or none yet) clears the table and the counters and `growBytes` > 0 regrows the
 * slots' item-draw arrays to that size, each behind a device synchronisation -- no launch in flight reads what goes. */
int rtc_draws_prepare(RtcDeviceScene *s, int width, int height, bool reset, size_t growBytes);
/* everything of it freed (the caller has synchronised); the scene's capacity setting stays */
void rtc_draws_free(RtcDeviceScene *s);

/* True when the bounce ray (pos, dir) provably cannot hit any triangle of cluster K (see DevCluster): the
 * half-line's distance to the ball centre exceeds T >= r + eps.  rho = |dir|_1 >= |dir| bounds the eps terms;
 * dd = dir.dir.  With w = centre - pos and b = w.dir, the half-line's closest point to the centre is interior
 * when b > 0, at distance |w x dir| / |dir|, else the origin, at |w|.  |w x dir|^2 is evaluated by Lagrange's
 * identity w2 dd - b^2 (FMA dots, each within 3u relative; the cancellation is covered by an explicit margin of
 * 25u w2 dd >= the evaluation error) and compared with T^2 dd: the 1.00001 factor on T covers dd's own error.
 * The f32 evaluation of w, S and T is covered by the gamma terms (rtc_build_clusters).  NaN never culls.
 * cluster_terms: the per-(origin, cluster) values, culled_by: the per-direction test (the chain kernel tabulates
 * the first for a pixel's primary hit point, where every first bounce starts). */
struct ClusterTerms {
    V3 w;
    float w2, A, B; /* T = (A + rho B) * 1.00001 */
};
__device__ __forceinline__ ClusterTerms cluster_terms(V3 pos, const DevCluster &K)
{
    ClusterTerms t;
    t.w = sub(V3{K.cx, K.cy, K.cz}, pos);
    const float S = fabsf(t.w.x) + fabsf(t.w.y) + fabsf(t.w.z) + K.r; /* >= |pos - A| for every vertex A */
    t.w2 = fmaf(t.w.z, t.w.z, fmaf(t.w.y, t.w.y, t.w.x * t.w.x));
    t.A = (K.r + kClusterGamma * S) + K.gammaE;
    t.B = fmaf(K.beta, S, K.alpha);
    return t;
}
__device__ __forceinline__ bool culled_by(const ClusterTerms &t, V3 dir, float rho, float dd)
{
    const float T = fmaf(rho, t.B, t.A) * 1.00001f;
    const float T2 = T * T;
    const float b = fmaf(t.w.z, dir.z, fmaf(t.w.y, dir.y, t.w.x * dir.x));
    const float wd = t.w2 * dd;
    const float x2 = fmaf(-b, b, wd);
    return b > 0.f ? (x2 - 1.5e-6f * wd > T2 * dd) : (t.w2 > T2);
}
__device__ __forceinline__ float dir_dd(V3 dir) { return fmaf(dir.z, dir.z, fmaf(dir.y, dir.y, dir.x * dir.x)); }
__device__ __forceinline__ bool cluster_culled(V3 pos, V3 dir, float rho, float dd, const DevCluster &K)
{
    return culled_by(cluster_terms(pos, K), dir, rho, dd);
}

__host__ __device__ static inline V3 v3(vec3 v) { return V3{v.x, v.y, v.z}; }

#ifndef RTC_SUN_VANISH
#define RTC_SUN_VANISH 1 /* (A/B switch, round 6) */
#endif
/* What the kernels read of a Scene's environment, built on the host (the powf tables are attached by each workgroup,
 * PowTablesLds): the one construction of a launch's (render_params) and of the sun-skip probe's (rtc_probe_sun_vanish), so
 * that the probe tests the limit and the gating the sky kernel runs with. */
static inline EnvParams env_of(const Scene &s)
{
    EnvParams e{};
    e.sun = v3(s.normalizedSunDirection);
    e.horizon = v3(s.skyColorHorizon);
    e.zenith = v3(s.skyColorZenith);
    e.ground = v3(s.groundColor);
    e.focus = s.sunFocus;
    e.intensity = s.sunIntensity;
    e.sunSkip = env_sun_skippable(e.focus, e.intensity);
    const float col[9] = {e.ground.x, e.ground.y, e.ground.z, e.horizon.x, e.horizon.y, e.horizon.z,
                          e.zenith.x, e.zenith.y, e.zenith.z};
    e.vanishLim = RTC_SUN_VANISH && e.sunSkip ? env_vanish_limit(e.focus, e.intensity, col) : -__builtin_inf();
    return e;
}

/* the tile cull's cap on a scene's mask words: the planner's (rtc_plan.h) */
constexpr int kMaxCullMaskWords = rtcplan::kMaxCullMaskWords;
