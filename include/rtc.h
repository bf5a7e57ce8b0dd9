/*
 * rtc.h -- C ABI of the MI355X-native render path (librtc.so).
 *
 * This is the drop-in boundary for the reference's render seam, main.c:263-304 (the pthread fan-out of
 * rowThread, main.c:81-104, over calcColor raytracing.c:262-296).  The reference has no plugin or FFI API;
 * its only "interface" for this path is that seam plus the scene-build / output functions either side
 * of it, so the entry points below are what a maintainer binds in place of that region.
 *
 * Plain C: plain pointers and sizes, no torch or HIP types.  All structs keep the reference's byte
 * layouts (raytracing.h:7-69, moremath.h:10-13) so host arrays produced by the reference's own loaders
 * pass through unconverted.
 *
 * Error convention: 0 = OK; a negative value is either -(hipError_t) (|v| < 10000) or one of the RTC_E*
 * codes below; a positive value is an RCCL ncclResult_t (rtc_render_multi).  Nothing here calls exit();
 * rtc_last_error() returns a message for the calling thread.  Entry points that select a device restore
 * the caller's current device before returning.
 */
#ifndef RTC_H
#define RTC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- reference types (identical layouts; sizes are static_assert-ed in the implementation) ------------ */
typedef unsigned char uint8;                                                   /* moremath.h:6 */
typedef struct vec3 { float x, y, z; } vec3;                                   /* moremath.h:10-13, 12 B */
typedef struct Scene {                                                         /* raytracing.h:7-11, 56 B */
    vec3 normalizedSunDirection, skyColorHorizon, skyColorZenith, groundColor;
    float sunFocus, sunIntensity;
} Scene;
typedef struct Color { uint8 r, g, b; } Color;                                 /* raytracing.h:15-18, 3 B */
typedef struct Material { vec3 color; float emissionStrength; float smoothness; } Material; /* :25-30, 20 B */
typedef struct Sphere { vec3 pos; float r; Material mat; } Sphere;             /* raytracing.h:34-39, 36 B */
typedef struct Triangle { vec3 posA, posB, posC, normal; Material mat; } Triangle; /* :41-45, 68 B */
typedef struct Ray { vec3 pos; vec3 dir; } Ray;                                /* raytracing.h:64-68, 24 B */

/* ---- render description ---------------------------------------------------------------------------- */
/* Camera: origin plus the basis main.c:252-255 computes, and fov (main.c:116). */
typedef struct RtcCamera { vec3 origin, ex, ey, ez; float fov; } RtcCamera;   /* 52 B */

/* Which pixels and how.  width/height/maxBounce = main.c:10-12; spp = accumulationCount (scene.h:26);
 * trianglesOnly = main.c:113,241.  Rows rendered: y = rowStart + k*rowStride for k = 0..ceil(..)-1, the
 * reference's row interleave (main.c:84) lifted to devices/ranks.  rowStride = 1, rowStart = 0 renders the
 * whole frame.  rowBand = B > 1 (a power of two, at most 64; 0 or 1: single rows) interleaves bands of B rows
 * instead: launch row r is image row y = rowStart + (r / B)*rowStride*B + r % B -- rank g of G renders the bands
 * b = g, g + G, ... with rowStart = g*B, rowStride = G (north_star's row-tile split: with B = 8 a rank's 8x8 pixel
 * tiles are 8 adjacent image rows, not 8 rows G apart).  The launch writes its rows compactly in that order.  The
 * frame does not depend on the partition (the seed is the absolute pixel index, main.c:95). */
typedef struct RtcRenderDesc {
    int width, height;
    int spp;
    int maxBounce;
    int trianglesOnly;
    int rowStart, rowStride;
    int flags;                 /* RTC_F_* */
    int rowBand;               /* rows per interleaved band (0 or 1: single rows) */
} RtcRenderDesc;

#define RTC_F_HOIST_PRIMARY 0x1  /* bit-exact: trace each pixel's primary ray once; default off */
#define RTC_F_DEBUG_BOUNCES 0x2  /* calcDebugColor (raytracing.c:242-260) instead of calcColor: bounce-count grey */
#define RTC_F_NO_TILE_CULL  0x4  /* primary segments test every triangle (brute force, as calculateRayCollision
                                    does) instead of the 8x8 tile's candidate list; same output bit for bit */
#define RTC_F_NO_REORDER    0x8  /* dispatch workgroups in raster order instead of heaviest first (for A/B
                                    timing; the frame is identical) */
#define RTC_F_NO_COOP       0x10 /* pixels that see geometry are rendered like the rest, one lane per pixel
                                    (rtc_render_kernel), instead of by the split launch's rtc_render_chain
                                    (A/B timing; the frame is identical) */
#define RTC_F_NO_CLUSTER_CULL 0x20 /* bounce rays test every triangle instead of only the clusters their
                                      half-line may reach (A/B timing; identical frame); rtc_trace_rays_async: every
                                      record in reference order, no ball test (identical buffers) */
/* The split launch renders the pixels that see geometry with rtc_render_chain (state-indexed samples: lanes
 * evaluate the samples that start at consecutive RNG offsets, then the chain of the reference's samples is walked
 * in order).  0x40, 0x80, 0x100 and 0x200 selected older kernels for A/B timing; they were removed and these flags
 * are now RTC_EINVAL. */
#define RTC_F_COOP4         0x40 /* removed: RTC_EINVAL */
#define RTC_F_COOP8         0x80 /* removed: RTC_EINVAL */
#define RTC_F_PIPE          0x200 /* removed: RTC_EINVAL */
#define RTC_F_SPEC          0x100 /* removed: RTC_EINVAL */
#define RTC_F_CHAIN_INLINE  0x400 /* rtc_render_chain adds each pixel's samples itself instead of deferring the
                                     in-order sum to a separate pass (identical frame; the default for a small share
                                     of a row-partitioned frame, rowStride > 1 and width * rows <= 600,000, and for
                                     the overlapped launches on the alternating streams, RTC_F_OVERLAP) */
#define RTC_F_HOST_ROWS     0x1000 /* rtc_render_multi only: no gather -- every device copies its rows straight into
                                      their places of the host frame (rtc_copy_rows_d2h_dma, its own PCIe link);
                                      without it the parts are gathered to device 0 over RCCL, re-interleaved there
                                      and copied once.  Same frame bit for bit. */
#define RTC_F_SPLIT_SPHERES 0x2000 /* a launch that renders spheres takes the split launch (tile cull with sphere coverage,
                                      sky pass, rtc_render_chain with spheres) even where the scene's gate keeps it on
                                      the one-lane-per-pixel kernel (rtc_scene_sphere_split == 0); A/B timing and tests,
                                      like RTC_F_NO_COOP.  Never more than 32 spheres, and not with RTC_F_NO_COOP,
                                      RTC_F_NO_REORDER, RTC_F_NO_TILE_CULL or RTC_F_DEBUG_BOUNCES.  Same frame bit for
                                      bit. */
#define RTC_F_NO_DRAW_CACHE 0x4000 /* the launch neither reads nor fills the scene's draw cache (rtc_scene_set_draw_cache):
                                      rtc_render_chain computes every hit draw as before the cache.  A/B timing and
                                      tests.  Same frame bit for bit. */
#define RTC_F_WAVE_PER_RAY  0x20000 /* rtc_trace_paths_async / rtc_trace_paths, and rtc_render_pixels_async / rtc_render_pixels
                                       (a wave per listed pixel), only (every other entry: RTC_EINVAL): one
                                       wave per ray, the ray's samples on the wave's lanes at RNG offsets 7 draws apart
                                       (lane j starts 7 j draws after the ray's state), instead of one
                                       lane per ray.  Same radiance, seeds and segment count bit for bit; for few rays
                                       with many samples.  The choice is the caller's. */
#define RTC_F_OVERLAP       0x800 /* frame pipelining (device-resident split only): the launch does not make
                                     `stream` wait for its sky pass, so the next launches on the same scene render
                                     (scratch in 8 slots) while this one's sky pass still runs.  A later overlapped
                                     launch waits for it only when it would rewrite its scratch slot (8 launches
                                     later) or writes the same Color / accumulator buffer with other rows, camera or
                                     environment; a later launch that is not overlapped waits for it before its
                                     first kernel.  Every overlapped launch but a row-stride-1 frame of at most
                                     600 k pixels prepares, culls and runs its geometry kernel on one of two scene
                                     streams (alternating), unordered against the previous launch's geometry
                                     kernel, and sums each pixel's samples in-kernel: such a launch starts after
                                     everything enqueued on `stream` before it, but `stream` is not made to wait for
                                     its kernels.  Every overlapped launch's frame is complete when the scene's frame
                                     event (rtc_scene_set_frame_event) fires -- consume it there, not at `stream`;
                                     with segment counters requested the launch joins as usual.  Same frame bit for
                                     bit. */

typedef struct RtcStats {
    double renderMs;             /* device time of the render launch (slowest device), HIP events */
    double totalMs;              /* wall time of the whole call incl. scene upload, allocations, readback */
    unsigned long long segments; /* closest-hit queries traced (calculateRayCollision calls) */
    unsigned long long samples;  /* camera samples = pixels * spp */
    unsigned long long triTests; /* ray-triangle tests evaluated (segments x triangles the segment visits) */
    unsigned long long clusterTests; /* ray-cluster bounding-ball tests (cooperative path, bounce rays) */
    unsigned long long discardedTests; /* ray-triangle tests of speculative samples not accumulated */
    double frameMs;              /* SURVEY.md §8(d) frame time: first render kernel launch after the scene upload
                                    until Color[W*H] is in (pinned) host memory -- render, RCCL gather and
                                    re-interleave (multi), D2H; HIP events on device 0 */
} RtcStats;

/* ---- error codes ----------------------------------------------------------------------------------- */
#define RTC_OK 0
#define RTC_EINVAL (-10001)
#define RTC_ENODEV (-10002)
#define RTC_EIO (-10003)
#define RTC_ENOMEM (-10004)
#define RTC_EFORMAT (-10005)
#define RTC_ETIMEDOUT (-10006) /* an SDMA copy did not complete in time and may still run (rtc_dma_pending) */
#define RTC_EBUSY (-10007)     /* a range a timed-out copy may still write (rtc_host_unregister) */

const char *rtc_last_error(void);
const char *rtc_version(void);
int rtc_device_count(int *count);

/* ---- scene build (host; restates objloader.c:340-551 + raytracing.c:19-147) ------------------------ */
/* loadOBJTriangles (raytracing.c:100-147): OBJ/MTL -> Triangle[] with the x,y negation.  On failure
 * returns RTC_EIO (the reference exits 42, raytracing.c:106-110; the CLI driver keeps that). *outTris is
 * malloc'd; free with rtc_free. */
int rtc_load_obj(const char *path, Triangle **outTris, int *outCount);
/* parseTriangleFile (raytracing.c:76-98) incl. cleanFile (:47-74).  Writes "<path>.parsed" beside the
 * input exactly like the reference.  Missing file -> RTC_EIO with count 0 (the reference silently keeps 0). */
int rtc_parse_triangle_file(const char *path, Triangle **outTris, int *outCount);
void rtc_free(void *p);
/* The default scene's sphere list (scene.h:17-19) and sky/sun (main.c:14,21-28), sun normalised as main.c:247. */
int rtc_default_spheres(const Sphere **outSpheres, int *outCount);
int rtc_default_scene(Scene *outScene);
int rtc_scene_set_sun(Scene *scene, vec3 sunDirection);
/* main.c:252-255 */
int rtc_camera_basis(vec3 origin, vec3 lookingAt, float fov, RtcCamera *outCam);
/* 24-bit BMP, byte-identical to stbi_write_bmp (stbi_image_write.h:492-529) */
int rtc_write_bmp(const char *path, int width, int height, const Color *image);
/* vec3ToColor / floatToUint (raytracing.c:11-15, moremath.c:25-30) on a host float3 buffer */
int rtc_quantize(const float *accum, size_t pixels, Color *out);

/* ---- render: host buffers (the seam main.c:263-304) ------------------------------------------------ */
/* Uploads the scene to HBM, renders the rows selected by d (normally the full frame) on `device`
 * (-1 = current), writes Color rows (row-major, y = 0 top; a partial row set is written compactly in
 * row order) and optionally the pre-quantisation float3 accumulator.  Inputs are borrowed for the call. */
int rtc_render(const Triangle *tris, int triCount, const Sphere *spheres, int sphereCount,
               const Scene *scene, const RtcCamera *cam, const RtcRenderDesc *d, int device,
               Color *outImage, float *outAccum, RtcStats *stats);

/* Single-process multi-GPU variant of rtc_render (replaces the 12-pthread fan-out main.c:285-302): devices
 * 0..numDevices-1 each render the rows y = g + k*numDevices (the reference's row interleave, main.c:84,
 * lifted to GPUs) -- or, with d->rowBand = B > 1, the bands of B rows b = g + k*numDevices -- into a compact part,
 * concurrently; one RCCL communicator clique (ncclCommInitAll) gathers
 * the parts to device 0 over xGMI (ncclGather, grouped), device 0 re-interleaves them and one D2H brings the
 * frame to the host.  Output is bit-identical to numDevices = 1 (the seed is the absolute pixel index,
 * main.c:95).  RCCL errors are returned as positive ncclResult_t values.  stats->renderMs = slowest
 * device's render launch; stats->frameMs = render + gather + re-interleave + D2H. */
int rtc_render_multi(const Triangle *tris, int triCount, const Sphere *spheres, int sphereCount,
                     const Scene *scene, const RtcCamera *cam, const RtcRenderDesc *d, int numDevices,
                     Color *outImage, float *outAccum, RtcStats *stats);
/* What the calling thread's last rtc_render_multi ran on: *path 0 (no call yet), 1 (RCCL gather) or 2 (RTC_F_HOST_ROWS,
 * no communicator); *devices its numDevices; commRanks[g] (up to maxComms) the rank count communicator g reports itself
 * (ncclCommCount; -1 if not reported).  Returns the number of communicators.  No reference counterpart: it shows that
 * RCCL saw the whole clique (main.c:285-302's fan-out lifted to GPUs). */
int rtc_last_multi_info(int *path, int *devices, int *commRanks, int maxComms);

/* ---- render: device-resident (used by the multi-GPU host and bench) -------------------------------- */
typedef struct RtcDeviceScene RtcDeviceScene;
int rtc_scene_upload(const Triangle *tris, int triCount, const Sphere *spheres, int sphereCount,
                     int device, RtcDeviceScene **out);
int rtc_scene_release(RtcDeviceScene *s);
/* Replace the resident scene's triangles and / or spheres (positions, normals, materials) without a new upload: one short
 * kernel on `stream` (a refit), no host work, no synchronisation (no reference counterpart: main.c:229-243 builds its
 * arrays once).  dTris / dSpheres are DEVICE pointers on the scene's device in the reference's own layouts (68 / 36 bytes
 * per primitive); a null pointer leaves that kind unchanged, and its count is then 0; a count given equals the upload's --
 * the number of primitives is fixed at upload, and an update keeps the grouping of the triangles into clusters (the
 * upload's, or the last rtc_scene_regroup_async's).  The kernel rewrites what
 * the upload derived from the primitives: the packed triangles (A, AB = B - A, AC = C - A in f32, the normal), the
 * materials, the spheres, the triangles in cluster order with their aligned-normal flags, and every cluster's and chunk's
 * bounding ball and cull margins, byte for byte what an upload of the new primitives with the old grouping would hold.
 * The culling is exact for any ball that contains its vertices and carries its margins, so the frames are the new
 * geometry's bit for bit, however far it moved; geometry that drifts far from the upload's clusters is only culled worse
 * (larger, overlapping balls) and is a reason to regroup (rtc_scene_regroup_async below) -- an update never regroups.
 * Ordering: asynchronous on `stream`, under rtc_render_rows_async's contract (a scene serves one stream at a time; a
 * caller that changes streams orders them).  Every launch enqueued on the scene after the call renders the new geometry,
 * every launch enqueued before it the old one, overlapped launches (RTC_F_OVERLAP) whose kernels or sky pass are still in
 * flight included: the scene keeps two generations of its records, the update writes the one no launch in flight reads
 * (it waits only for launches from before the previous update) and later launches read that one.  The source buffers
 * may be reused once `stream` has passed the call.
 * The scheduling hints of the upload (rtc_scene_chain_wgs, the sphere split's gate rtc_scene_sphere_split) keep their
 * values: they never change a frame.  An animation that turns an open sphere scene into a closed one keeps the route the
 * upload chose; RTC_F_SPLIT_SPHERES and RTC_F_NO_COOP select a route per launch as before.
 * RTC_EINVAL, with nothing enqueued: a null scene; both pointers null; a count that differs from the upload's (or is not
 * 0 beside a null pointer); a pointer for a kind the scene was uploaded without.
 * rtc_scene_update takes HOST arrays: it stages them on the device, waits for the device, runs the update, waits for it
 * and restores the caller's current device (synchronous; the same refusals). */
int rtc_scene_update_async(RtcDeviceScene *s, const Triangle *dTris, int triCount, const Sphere *dSpheres,
                           int sphereCount, void *stream);
int rtc_scene_update(RtcDeviceScene *s, const Triangle *tris, int triCount, const Sphere *spheres, int sphereCount);
/* rtc_scene_update_async with the grouping of the triangles into clusters decided anew from dTris, on the device: a few
 * short kernels on `stream` before the refit -- the centroids, one kernel per level of the upload's median split, the
 * membership --, no host work, no host read of device memory, no allocation, no synchronisation (no
 * reference counterpart).  Once `stream` has passed the call the six record arrays of the current generation are, byte for
 * byte, those of a fresh rtc_scene_upload of dTris (rtc_scene_records_host(dTris, n, NULL, spheres, ..)), and a later
 * rtc_scene_update_async(tris2) refits THAT grouping (rtc_scene_records_host(dTris, n, tris2, ..)).  The frames are the
 * new geometry's bit for bit either way; the regroup restores the culling a drifted grouping lost.
 * dTris is required, with the upload's count; dSpheres is as in an update (nullable: the spheres are kept).  dScratch:
 * rtc_scene_regroup_scratch_bytes(s) bytes of device memory on the scene's device, 16-byte aligned, the caller's; it holds
 * the centroids and two index buffers and may be reused, like the source arrays, once `stream` has passed the call.
 * Ordering, generations and waits are exactly an update's.  The upload's hints (rtc_scene_chain_wgs, the sphere split's
 * gate, rtc_scene_bounds, the HITS choice) keep their values; the draw cache, the caller's hooks and the chain report are
 * untouched.
 * The work is quadratic in the triangle count (a stable sort as a rank count: deterministic, no atomics), so it is offered
 * up to rtc_scene_regroup_max_tris() triangles -- the largest power of two at which it was measured faster than the
 * upload it replaces; above it, upload again.
 * RTC_EINVAL, with nothing enqueued: whatever rtc_scene_update_async refuses; a null dTris; a null dScratch, one that is
 * not 16-byte aligned or holds fewer than rtc_scene_regroup_scratch_bytes(s) bytes; more triangles than
 * rtc_scene_regroup_max_tris().
 * rtc_scene_regroup takes HOST arrays, staged like rtc_scene_update's, with a scratch of its own (synchronous; the same
 * refusals; a null scene is refused before any device call).  rtc_scene_regroup_scratch_bytes: a multiple of 16; 0 for a
 * null scene. */
size_t rtc_scene_regroup_scratch_bytes(const RtcDeviceScene *s);
int rtc_scene_regroup_max_tris(void);
int rtc_scene_regroup_async(RtcDeviceScene *s, const Triangle *dTris, int triCount, const Sphere *dSpheres,
                            int sphereCount, void *dScratch, size_t scratchBytes, void *stream);
int rtc_scene_regroup(RtcDeviceScene *s, const Triangle *tris, int triCount, const Sphere *spheres, int sphereCount);
/* The membership a regroup leaves, on the host and without a GPU: idx[k] = the index in tris of clustered record k
 * (triCount ints).  It runs the device's formulation -- level by level, every element to its rank (rtc_regroup.h) -- in
 * plain C++, and equals the membership of rtc_scene_upload (rtc_scene_records_host's clTris, dword 12) for every input,
 * NaN, infinities and zeros of either sign included.  Quadratic: meant for tests. */
int rtc_regroup_membership_host(const Triangle *tris, int triCount, int *idx);
/* Number of rows d selects (ceil((height - rowStart) / rowStride) for single rows; with bands, the full bands' rows
 * plus the last band's rows inside the frame), 0 if none. */
int rtc_rows_selected(const RtcRenderDesc *d);
/* Asynchronous on `stream` (a hipStream_t, NULL = default stream).  dColors: device buffer of
 * rows_selected*width*3 bytes; dAccum: nullable device float buffer rows_selected*width*3; dSegments:
 * nullable device u64[RTC_SEGMENT_COUNTERS] the kernel atomically adds to: [0] calculateRayCollision calls
 * (the reference's segment count), [1] closest-hit queries actually traced (smaller with
 * RTC_F_HOIST_PRIMARY), [2] ray-triangle tests of the accumulated samples, [3] ray-cluster bounding-ball
 * tests, [4] ray-triangle tests of speculatively evaluated samples that were not accumulated (state-indexed
 * window lanes off the chain, mispredicted speculative samples); [2] + [4] = every test evaluated.
 * A scene handle serves one stream at a time: its per-launch scratch (primary-ray records, tile candidate
 * lists) is rewritten by every launch. */
#define RTC_SEGMENT_COUNTERS 5
/* Per-kernel timing of the split launch: with rtc_scene_set_timing(s, 1) every later launch on s records HIP
 * events around its two kernels (off by default: the records cost each launch a few microseconds), and
 * rtc_scene_kernel_times returns the device times (ms) of the last launch: out[0] the geometry-pixel kernel
 * (rtc_render_chain by default, without the rtc_accumulate_samples pass that follows it), out[1] the sky
 * kernel (concurrent, on the scene's side stream); -1 when that launch recorded none.  Waits for that launch
 * to finish. */
int rtc_scene_set_timing(RtcDeviceScene *s, int enable);
/* Pipelining hooks.  Both are ONE-SHOT: the event is armed for the next launch on s that renders rows
 * (rtc_render_rows_async with rows_selected > 0), which records it and forgets it, so no later launch can record
 * an event its caller has released.  Arm again before every launch that should record one; NULL disarms.
 * Geometry event: recorded on the launch's stream once the geometry-pixel kernels are enqueued, before the join
 * with the sky pass; a caller can start the previous frame's D2H there, so that the copy overlaps the sky pass
 * instead of the next frame's persistent geometry kernel (whose workgroups then all start at once). */
int rtc_scene_set_geometry_event(RtcDeviceScene *s, void *event);
/* Frame event: recorded once the whole frame -- the geometry pixels and the sky pass -- is written: on the launch's
 * stream after the join, or with RTC_F_OVERLAP (no join) on the scene's side stream after both passes.  Consumers
 * of the frame (a D2H, a gather) wait for it.  The event must stay valid until that launch has been enqueued
 * (rtc_render_rows_async returned). */
int rtc_scene_set_frame_event(RtcDeviceScene *s, void *event);
int rtc_scene_kernel_times(const RtcDeviceScene *s, float out[2]);
/* Scheduling hints chosen at upload (no reference counterpart; they never change a frame):
 * rtc_bounce_hit_share estimates (host only, fixed-seed probe) the share of diffuse bounce rays from the triangles that
 * hit the scene again; rtc_scene_chain_wgs reports the geometry kernel's workgroups per CU for whole frames that the
 * scene got from it (4 above 0.15, else 3; small row shares run 3). */
int rtc_bounce_hit_share(const Triangle *tris, int triCount, float *share);
int rtc_scene_chain_wgs(const RtcDeviceScene *s);
/* What the scene's last geometry-kernel launch (rtc_render_chain, the split launch's kernel for the pixels that see
 * geometry) chose, recorded on the host when the launch was enqueued -- read-only, no device work, no reference
 * counterpart: every choice renders the same frame, so only this report tells a test which code path a launch ran.
 * multi .. resume: the kernel's template flags (MULTI: more than one chunk of 32 clusters; COUNT: segment counters; HITS: the
 * hit-heavy scenes' instantiation; GENERAL: deferred slots, hoisted primaries or unstaged primary filter records, and every
 * MULTI / COUNT / SPHERES / RESUME launch; SPHERES; RESUME: a pass).  chainPrimF: the primary filter records are staged in
 * LDS.  wgsPerCu: the launch's workgroups per CU (rtc_scene_chain_wgs for whole frames, 3 for small row shares).
 * chainDyn: its dynamic LDS in bytes.  clusterCount, chunkCount: the scene's.  launches: how many geometry-kernel launches
 * the scene has enqueued so far (0: none yet, every other field 0; a launch without the split launch leaves the report as
 * it was). */
typedef struct RtcChainReport {
    int multi, count, hits, general, spheres, resume;
    int chainPrimF, wgsPerCu, chainDyn, clusterCount, chunkCount, launches;
} RtcChainReport;
int rtc_scene_chain_report(const RtcDeviceScene *s, RtcChainReport *out);
/* What the scene's most recent enqueue planned -- a launch, a pass, a first-hit launch, an update, a regroup, one of the
 * queries for caller-supplied rays or a pass over a list of pixels -- recorded on the host, from the plan the call
 * executed, when its last operation was enqueued (a call that is refused or fails leaves the record as it was); read-only,
 * no device work, no reference counterpart.  The encoding is the planner hooks' (rtc_plan_sim_launch, _update, _regroup,
 * _trace_rays, _trace_paths, _occluded, _render_pixels, below): 4 ints per operation into ops, 6 u64 per footprint row into
 * footprint, the hook's trailing ~0 record last, and the return value nOps | rows << 8 -- the caller's buffers carry their
 * device addresses as identities.  0 before anything was enqueued; RTC_EINVAL for a null argument or when maxOps or
 * maxFootprint is less than the plan has (48 operations and 256 rows always suffice).  tests/test_gpu_footprints.py holds
 * every byte a call changes in the scene's memory to the write rows of this record. */
int rtc_scene_last_plan(const RtcDeviceScene *s, int *ops, int maxOps, unsigned long long *footprint, int maxFootprint);
/* Every device allocation the scene owns, as spans: res and id in the footprint rows' numbering, part where one (res, id)
 * is several arrays, base the device address, bytes the size (0 with base 0: not allocated yet).  In this order: the
 * scratch (res 0: all slots, footprint rows give byte ranges inside it); each slot's primary records (res 1, id the slot,
 * parts 0 and 1: the filter and the exact records); each counter set (res 2, id the set); the deferred sample slots (res
 * 3); the segment-counter slots (res 4); each array of each generation of the scene records (res 9, id the generation,
 * part the array: tris, mats, spheres, clTris, clusters, chunks); the draw cache's slot table, counter words and block
 * seeds (res 12, parts 0-2); each slot's item-draw array (res 13, id the slot); the cluster membership (res 18); the draw
 * cache's pool of 1-KB blocks (res 21, which no footprint row names: a block is written once, by the launch whose tile cull
 * took it -- the first counter word, part 1 of res 12, is the number of blocks taken).  Returns the number of spans (60);
 * RTC_EINVAL for a null argument or max less than that.  Read-only host state: no device work; a launch that regrows or
 * first allocates a buffer changes its span. */
typedef struct RtcSpan {
    unsigned long long res, id, part, base, bytes;
} RtcSpan;
int rtc_scene_spans(const RtcDeviceScene *s, RtcSpan *out, int max);
/* The draw cache (no reference counterpart; it never changes a frame).  A sample's m-th hit draws RandomDiretion's six
 * values and the roulette's one from the pixel's seed x + y * width (main.c:95) advanced by 7 (j + m) draws: a function of
 * the frame's width and the pixel alone, whatever the camera, scene, materials or environment.  The scene keeps, per pixel
 * that has seen geometry, the 64 entries D_j = (RandomDiretion from the seed advanced 7 j draws, the roulette value that
 * follows), j = 0..63, in a 1-KB block of device memory, filled once by the launch that first meets the pixel (the tile
 * cull allocates, a fill kernel behind it computes) and read by rtc_render_chain's first window of every later launch in
 * place of its Box-Muller.  Only the launches that run the chain kernel without its GENERAL code use it (in-kernel sums,
 * single chunk, no counters, spheres, passes or hoisting); every sample still traces its rays and evaluates the
 * environment.  Blocks are never evicted: when the pool is full, new pixels are computed as before.  A launch whose width
 * or height differs from the cached frame's clears the cache behind a device synchronisation.
 * rtc_scene_set_draw_cache: the pool's capacity in blocks (0 disables; < 0 the default: RTC_DRAW_CACHE_BLOCKS at upload,
 * else 1 GiB of blocks, in either case at most the frame's pixel count); when anything is cached it synchronises the
 * device and drops it.  (rtc_render and rtc_render_multi, whose scenes render one frame, run without the cache.)
 * rtc_scene_draw_cache_reset: synchronises and clears.  rtc_scene_draw_cache_stats: synchronises; out = blocks in use,
 * capacity (0 before the first cached launch), the last cached launch's fresh items, its uncached items.
 * rtc_probe_draw_cache: synchronises; the 64 entries (256 floats) of the pixel with this seed into out and its block in
 * *block, or *block = -1 when it has none. */
int rtc_scene_set_draw_cache(RtcDeviceScene *s, long long blocks);
int rtc_scene_draw_cache_reset(RtcDeviceScene *s);
int rtc_scene_draw_cache_stats(const RtcDeviceScene *s, unsigned long long out[4]);
int rtc_probe_draw_cache(const RtcDeviceScene *s, unsigned int seed, float *out, int *block);
/* Sphere scenes (calculateRayCollision's sphere loop, raytracing.c:219-228).  A launch that renders spheres takes the split
 * launch -- the pixels whose primary ray hits nothing go to the sky pass, the others to rtc_render_chain, which tests the
 * spheres first and lets a triangle win only when strictly closer -- when all of these hold: at most 32 spheres; the
 * scene's gate allows it or the launch carries RTC_F_SPLIT_SPHERES; none of RTC_F_NO_COOP, RTC_F_NO_REORDER,
 * RTC_F_NO_TILE_CULL, RTC_F_DEBUG_BOUNCES.  Every other sphere launch runs the one-lane-per-pixel kernel.  The gate is
 * decided at upload: rtc_bounce_hit_share_all is rtc_bounce_hit_share's probe with ray origins on triangles and spheres
 * (area-weighted, a sphere's area 4 pi r^2) tested against both, and the gate allows the split launch when that share is
 * at most 0.5 (open scenes: most bounce rays escape; a closed box traces ~10 segments per sample, which the chain kernel's
 * windows of one lane per RNG state index would mostly discard) and the scene has at least one triangle (spheres alone
 * render faster one lane per pixel).  Measured at 1920x1080x64: an open scene 12.9 -> 6.5 ms per frame through the split
 * launch, the reference's default box 40.8 -> 451 ms (gated off).  rtc_scene_sphere_split returns the upload's decision,
 * 1 or 0 (0 for a scene without spheres, without triangles or with more than 32 spheres).  The frame is the same bit for
 * bit on either route. */
int rtc_bounce_hit_share_all(const Triangle *tris, int triCount, const Sphere *spheres, int sphereCount, float *share);
int rtc_scene_sphere_split(const RtcDeviceScene *s);
int rtc_render_rows_async(const RtcDeviceScene *s, const Scene *scene, const RtcCamera *cam,
                          const RtcRenderDesc *d, void *dColors, float *dAccum,
                          unsigned long long *dSegments, void *stream);
/* Progressive rendering: a frame's samples in resumable passes (main.c:95-100 with the accumulationCount loop cut into
 * ranges).  The launch evaluates samples range->first .. range->first + range->count - 1 of every selected pixel, in order;
 * d->spp stays the frame's accumulationCount and every sample is weighted (float)(1. / d->spp) (main.c:99).  A pixel's
 * whole resume state is 16 bytes, both buffers required, read and written: dAccum (as rtc_render_rows_async's) and
 * dRngState, one unsigned per pixel at launchRow * width + x (compact in launch-row order like dAccum).  With first == 0
 * neither is read: the pixel starts from the seed x + y * width and +0.  With first > 0 it starts from the stored state
 * and sum.  After the launch dAccum is the reference's accumulatedColor after first + count iterations of main.c:98-99,
 * dRngState its rngState at that point (a pixel whose primary ray misses draws nothing: its state stays the seed, which
 * the first pass writes), dColors vec3ToColor of that sum -- a partial frame is darker by done / spp; scaling a preview
 * is the caller's business.  Passes [0, a), [a, b), .., [z, spp) leave the sum, the Color and the state of one launch of
 * spp samples, bit for bit, and dSegments counter [0] adds up to that launch's ([1], the queries traced, counts one primary
 * trace per pass with RTC_F_HOIST_PRIMARY).  The caller keeps the scene, the camera, d and the three buffers the same
 * across the passes of a frame and orders the passes on one stream (each pass is complete at `stream`, like a launch
 * without RTC_F_OVERLAP; other launches on the scene may come between them).  RTC_EINVAL, with nothing enqueued: a null
 * range, dAccum or dRngState; first < 0, count <= 0 or first + count > d->spp; RTC_F_OVERLAP (an unjoined sky pass would
 * race the next pass's read of the accumulator; pipelining passes is not offered).  rtc_render, rtc_render_multi,
 * rtc_frame_loop and the CLI render whole frames only. */
typedef struct RtcSampleRange { int first, count; } RtcSampleRange;   /* samples [first, first+count) of d->spp */
int rtc_render_samples_async(const RtcDeviceScene *s, const Scene *scene, const RtcCamera *cam,
                             const RtcRenderDesc *d, const RtcSampleRange *range,
                             void *dColors, float *dAccum, unsigned int *dRngState,
                             unsigned long long *dSegments, void *stream);
/* First-hit buffers: what every selected pixel's primary ray (main.c:88-94) sees, i.e. the result of
 * calculateRayCollision(ray, d->trianglesOnly) (raytracing.c:216-240), for picking, depth compositing and denoiser guides.
 * No Scene, no RNG, no samples: d->spp and d->maxBounce are ignored.  Each buffer is a DEVICE pointer on the scene's device
 * or null (at least one is not); pixel (launch row r, x) lies at r * width + x, compact in launch-row order like dAccum,
 * and the row selection (rowStart, rowStride, rowBand) means what it means for rtc_render_rows_async -- the values do not
 * depend on the partition.
 *   prim:   the winner: triangle index t >= 0, -2 - i for sphere i, -1 for a miss; ties keep the first in the reference's
 *           order (spheres before triangles, ascending index, strict `<`)
 *   depth:  closest.dst; 999999.f on a miss (the reference's initial value)
 *   normal: a triangle's stored normal bit for bit; a sphere's normalized(hitPoint - centre), hitPoint = pos + dir * dst
 *           (raytracing.c:181-182); +0, +0, +0 on a miss
 *   albedo: closest.mat.color bit for bit; +0, +0, +0 on a miss
 * Every value is the reference's bit for bit (the primary query of the render kernels: the tile cull's candidates, then the
 * reference's arithmetic).  d->flags may carry RTC_F_NO_TILE_CULL (every record tested for every pixel; the same buffers,
 * for A/B timing and tests).  Any number of spheres and a scene without triangles are accepted.
 * Asynchronous on `stream` and complete at `stream` (joined, like a pass), under rtc_render_rows_async's rule that a scene
 * serves one stream at a time.  It may come between pipelined RTC_F_OVERLAP launches, between the passes of a progressive
 * frame and after rtc_scene_update_async (it reads the generation current when it is enqueued).  It neither records nor
 * forgets the one-shot geometry and frame events, leaves rtc_scene_chain_report and rtc_scene_kernel_times as they were and
 * restores the caller's current device.  rows_selected == 0: returns 0, nothing enqueued.
 * RTC_EINVAL, with nothing enqueued: a null scene, camera, desc or `out`; all four pointers null; bad geometry (as
 * rtc_render_rows_async); a flag other than RTC_F_NO_TILE_CULL. */
typedef struct RtcHitBuffers {
    int *prim;     /* 4 B / pixel */
    float *depth;  /* 4 B / pixel */
    float *normal; /* 12 B / pixel */
    float *albedo; /* 12 B / pixel */
} RtcHitBuffers;
int rtc_render_first_hit_async(const RtcDeviceScene *s, const RtcCamera *cam, const RtcRenderDesc *d,
                               const RtcHitBuffers *out, void *stream);
/* Closest hits of caller-supplied rays: element i of each buffer of `out` is
 * calculateRayCollision(dRays[i], trianglesOnly) (raytracing.c:216-240) against the resident scene, in RtcHitBuffers'
 * encoding (above; hitPoint = pos + dir * dst of ray i), every value the reference's bit for bit.  dRays: n Rays (24 B:
 * pos, dir) in DEVICE memory on the scene's device; it must not alias an output buffer.  The direction is used as given:
 * it is not normalised (the reference does not), dst is in units of dir, and the EPSILON tests on det and dst see the
 * caller's scale; zero, NaN and infinite components get what the reference's arithmetic gives (a zero direction can hit a
 * sphere).  Any number of spheres and a scene without triangles are accepted; trianglesOnly != 0 skips the spheres.
 * flags: 0 -- the cluster hierarchy (bounding balls over 8 triangles and over 32 clusters, exact for every ray; a ray of
 * |dir|_1 > 4 tests every cluster) -- or RTC_F_NO_CLUSTER_CULL: every record in reference order, the same buffers.
 * Asynchronous on `stream` and complete at `stream`, under the rule that a scene serves one stream at a time.  It reads the
 * generation of scene records current when it is enqueued (after rtc_scene_update_async on that stream: the new
 * geometry), may come between RTC_F_OVERLAP launches and between passes, uses no scratch, primary record, counter set,
 * stream or event of the scene's -- it waits for nothing, and nothing waits for it, beyond stream order -- leaves the
 * one-shot frame and geometry events, rtc_scene_chain_report and rtc_scene_kernel_times as they were and restores the
 * caller's current device.  n == 0: returns 0, nothing enqueued.
 * RTC_EINVAL, with nothing enqueued, checked before any device call: a null scene, dRays or `out`; all four pointers
 * null; n > 0x7fffffff; a flag other than RTC_F_NO_CLUSTER_CULL. */
int rtc_trace_rays_async(const RtcDeviceScene *s, const Ray *dRays, size_t n, int trianglesOnly, int flags,
                         const RtcHitBuffers *out, void *stream);
/* The same for HOST arrays, synchronous: stages the rays, waits for the device, runs the query on the null stream and
 * copies back the arrays asked for (null: not wanted; at least one): prim[n], depth[n], normal[3 n], albedo[3 n].  The
 * same refusals; RTC_ENODEV without a GPU. */
int rtc_trace_rays(const RtcDeviceScene *s, const Ray *rays, size_t n, int trianglesOnly, int flags, int *prim,
                   float *depth, float *normal, float *albedo);
/* Radiance along caller-supplied rays: for ray i, main.c:95-100 with the ray given instead of derived
 * from a pixel -- rngState = dSeeds[i]; acc = +0 when sampleFirst == 0, otherwise dRadiance[3 i ..]; sampleCount times
 * acc = acc + calcColor(dRays[i], trianglesOnly, maxBounce, *scene) * (float)(1. / spp) (raytracing.c:262-296); then
 * dRadiance[3 i ..] = acc and, where dSeedsOut is not null, dSeedsOut[i] = rngState.  Every float is the reference's bit
 * for bit (where the reference gives a NaN: a NaN).  The direction is used as given, as rtc_trace_rays_async uses it: not
 * normalised, dst in units of dir, the EPSILON tests at the caller's scale; bounce directions come out of the reference's
 * own lerp.  dSegments, where not null, is one device u64 to which the launch atomically adds its number of
 * calculateRayCollision calls.
 * The samples of one ray form one RNG chain.  By default the kernel is one lane per ray and runs them one after the
 * other.  With RTC_F_WAVE_PER_RAY it is one wave per ray: a hit draws exactly 7 values and a miss none, so every sample
 * starts at the seed advanced by a multiple of 7 draws; 64 lanes evaluate the candidates at 64 consecutive such offsets
 * and the wave adds, in the reference's order, those the chain really reaches.  The outputs are the same
 * bit for bit; only the kernel differs, and a frame's passes may mix calls with and without the flag.  It is meant for
 * few rays with many samples (DESIGN §3.14 has the measurements); no choice is made for the caller.
 * `scene` and `d` are host pointers, borrowed for the call.  dRays (n Rays), dSeeds (n) and dRadiance (3 n floats) are
 * required DEVICE pointers on the scene's device; dSeedsOut (n) may be null and may be dSeeds (in place); dRays aliases
 * no output.  With sampleFirst > 0 the caller passes the previous call's dSeedsOut as dSeeds and the same dRadiance:
 * calls over [0, a), [a, b), .., [z, spp) leave the radiance, the seeds and the segment count of one call of spp samples,
 * bit for bit.
 * d->flags: 0 (the cluster hierarchy), RTC_F_NO_CLUSTER_CULL (every record in reference order, the same values),
 * RTC_F_WAVE_PER_RAY (above), or both.
 * Asynchronous on `stream` and complete there, under rtc_trace_rays_async's rules word for word: it reads the generation
 * current when it is enqueued, may come between RTC_F_OVERLAP launches, between passes and after an update, uses no
 * scratch, primary record, counter set, stream or event of the scene's, leaves the one-shot events,
 * rtc_scene_chain_report, rtc_scene_kernel_times and the draw cache as they were and restores the caller's current
 * device.  n == 0: returns 0, nothing enqueued.
 * RTC_EINVAL, with nothing enqueued, checked before any device call and before `s` is read: a null s, scene, dRays,
 * dSeeds, d or dRadiance; n > 0x7fffffff; spp <= 0; sampleFirst < 0, sampleCount <= 0 or sampleFirst + sampleCount > spp;
 * a flag other than RTC_F_NO_CLUSTER_CULL and RTC_F_WAVE_PER_RAY (RTC_F_DEBUG_BOUNCES included: calcDebugColor is not
 * offered for caller rays). */
typedef struct RtcPathDesc {
    int spp;            /* the weight's accumulationCount: every sample is weighted (float)(1. / spp) (main.c:99) */
    int maxBounce;      /* calcColor's maxBounce; <= 0: no segment is traced, a sample is +0 and draws nothing */
    int trianglesOnly;
    int flags;          /* 0, RTC_F_NO_CLUSTER_CULL, RTC_F_WAVE_PER_RAY or both */
    int sampleFirst, sampleCount; /* this call evaluates samples [sampleFirst, sampleFirst + sampleCount) of spp */
} RtcPathDesc;
int rtc_trace_paths_async(const RtcDeviceScene *s, const Scene *scene, const Ray *dRays, const unsigned int *dSeeds,
                          size_t n, const RtcPathDesc *d, float *dRadiance, unsigned int *dSeedsOut,
                          unsigned long long *dSegments, void *stream);
/* The same for HOST arrays, synchronous, built like rtc_trace_rays: stages the rays and seeds (and, with sampleFirst > 0,
 * the radiance; and the segment counter's value), waits for the device, runs the query on the null stream and copies
 * back radiance[3 n], seedsOut[n] and *segments (the last two nullable).  The same refusals; RTC_ENODEV without a GPU. */
int rtc_trace_paths(const RtcDeviceScene *s, const Scene *scene, const Ray *rays, const unsigned int *seeds, size_t n,
                    const RtcPathDesc *d, float *radiance, unsigned int *seedsOut, unsigned long long *segments);
/* Occlusion queries for caller-supplied rays, with a distance limit: "is anything in the way within tMax?"
 * For ray i with L = dTMax[i] (a float in units of dir, like dst; dTMax == NULL: no limit, L = +inf),
 *     occluded[i] = 1  iff  closest.didHit && closest.dst < L,  closest = calculateRayCollision(dRays[i], trianglesOnly)
 * (raytracing.c:216-240), i.e. iff some primitive's raySphere / rayTriangle (:162-214) reports a hit with dst < L and
 * dst < 999999.f; otherwise 0.  The byte is exactly 0 or 1.  The comparison is strict, in f32, on the reference's own dst
 * bit for bit: L == closest.dst is not occluded, nextafterf(closest.dst, +inf) is.  A NaN L never compares true: NaN, +-0,
 * negative and -inf limits give 0, and so does every L <= EPSILON (both reference tests report nothing below EPSILON;
 * such a ray tests nothing).  L = +inf, and any L >= 999999.f, ask "does calculateRayCollision hit at all".
 * The direction is used as given, exactly as rtc_trace_rays_async uses it: it is not normalised, dst and tMax are in
 * units of dir, the EPSILON tests see the caller's scale, and zero, NaN and infinite components get what the reference's
 * arithmetic gives.  Line of sight from a to b is therefore pos = a, dir = b - a, tMax = 1 (such a ray with |dir|_1 > 4
 * is never ball-culled: it tests every cluster, like a ray query's).  rayTriangle is one-sided -- dot(dir, normal) >= 0
 * is no hit (raytracing.c:189) -- and occlusion inherits that: a triangle seen from behind does not occlude.
 * dRays: n Rays in DEVICE memory on the scene's device; dTMax: n floats there, or null.  dOccluded: n bytes there at ANY
 * byte alignment, or null; the kernel writes exactly bytes [0, n), with byte stores only.  dCount: one device u64, or null;
 * the launch atomically adds its number of occluded rays to it (one atomic per wave of 64 rays that has any), so a caller
 * gets a visible fraction without moving n bytes.  At least one of the two is not null; the inputs alias no output.
 * flags: 0 -- the cluster hierarchy with rtc_trace_rays_async's exact-safe half-line test per bounding ball (a ray of
 * |dir|_1 > 4 tests every cluster); a wave of 64 rays stops as soon as each of its rays has found a hit;
 * RTC_F_NO_CLUSTER_CULL -- every record in reference order, no ball test.  The same bytes and count under either.
 * Asynchronous on `stream` and complete there, under rtc_trace_rays_async's rules word for word: it reads the generation
 * current when it is enqueued, may come between RTC_F_OVERLAP launches, between passes and after an update, uses no
 * scratch, primary record, counter set, stream or event of the scene's, leaves the one-shot events,
 * rtc_scene_chain_report, rtc_scene_kernel_times and the draw cache as they were and restores the caller's current
 * device.  n == 0: returns 0, nothing enqueued.
 * RTC_EINVAL, with nothing enqueued, checked before any device call and before `s` is read: a null s or dRays; dOccluded
 * and dCount both null; n > 0x7fffffff; a flag other than RTC_F_NO_CLUSTER_CULL. */
int rtc_occluded_async(const RtcDeviceScene *s, const Ray *dRays, const float *dTMax /* nullable */, size_t n,
                       int trianglesOnly, int flags, unsigned char *dOccluded /* nullable */,
                       unsigned long long *dCount /* nullable */, void *stream);
/* The same for HOST arrays, synchronous, built like rtc_trace_rays: stages the rays and limits (tMax nullable: none) and
 * the counter's value, waits for the device, runs the query on the null stream and copies back occluded[n] and *count
 * (each nullable, not both; *count += the occluded rays).  The same refusals; RTC_ENODEV without a GPU. */
int rtc_occluded(const RtcDeviceScene *s, const Ray *rays, const float *tMax, size_t n, int trianglesOnly, int flags,
                 unsigned char *occluded, unsigned long long *count);
/* A pass over a list of pixels of a progressive frame: rtc_render_samples_async for the listed pixels
 * alone, in the frame's own buffers, in place.  d, range, dColors, dAccum and dRngState mean what they mean there: the
 * frame's desc (d->spp gives the weight (float)(1. / spp)) and the frame's three buffers, compact in launch-row order.
 * dPixels[k] is a compact pixel index p = launchRow * width + x: the index of the pixel's rngState; its accumulator lies
 * at 3 p and its Color at bytes 3 p .. 3 p + 2.  For every listed p < rows_selected * width: x = p % width, the launch
 * row r = p / width, the image row y as a launch selects it (rowStart, rowStride, rowBand), the ray {cam->origin, the
 * direction of main.c:88-94 for (x, y)}.  With range->first == 0 neither buffer is read: the pixel starts from the seed
 * x + y * width and +0; otherwise from dRngState[p] and dAccum[3 p ..].  Then range->count times acc = acc +
 * calcColor(ray, trianglesOnly, maxBounce, *scene) * (float)(1. / spp); then dAccum[3 p ..] and dRngState[p] are stored
 * and, where dColors is not null, vec3ToColor(acc) at dColors[3 p .. 3 p + 2], with byte stores only (a pixel whose primary
 * ray misses draws nothing: its state stays its seed, which a first == 0 pass writes).  dSegments, where not null, is ONE
 * device u64 (rtc_trace_paths_async's, not a launch's counter array) to which the launch atomically adds its number of
 * calculateRayCollision calls.
 * The contract: after whole passes over [0, a) and a pixel pass over [a, b) with list L, every p in L holds the
 * accumulator, the RNG state and the Color of whole passes over [0, b), bit for bit, and every p not in L holds, byte for
 * byte, what it held before.  Pixel passes chain like whole passes and may alternate with them.
 * An index >= rows_selected * width is skipped: its lane or wave loads and stores nothing (a stale list is never an
 * out-of-bounds access).  Duplicates are the caller's error: the values at a duplicated pixel are unspecified, nothing
 * else is affected.
 * flags (the entry's own): 0, RTC_F_NO_CLUSTER_CULL, RTC_F_WAVE_PER_RAY -- here one wave per listed pixel -- or both; the
 * same words under each.  Of d->flags, RTC_F_DEBUG_BOUNCES and RTC_F_OVERLAP are refused (calcDebugColor is not offered
 * for pixel lists) and so are the removed kernels' flags; the remaining bits only choose routes of frame launches and are
 * ignored, so a caller passes the desc it passes to its whole passes.
 * Asynchronous on `stream` and complete there, under rtc_trace_paths_async's rules: it reads the generation current when
 * it is enqueued, uses no scratch, primary record, counter set, stream or event of the scene's, leaves the one-shot
 * events, rtc_scene_chain_report, rtc_scene_kernel_times and the draw cache as they were and restores the caller's current
 * device.  It waits for nothing beyond stream order: whole passes are joined, so they and other pixel passes on `stream`
 * are complete before it; the frame's buffers must not be the target of an RTC_F_OVERLAP launch still in flight.
 * n == 0 or rows_selected == 0: returns 0, nothing enqueued.
 * RTC_EINVAL, with nothing enqueued, checked before any device call and before `s` is read: a null s, scene, cam, d,
 * range, dPixels, dAccum or dRngState; n > 0x7fffffff; bad geometry (as rtc_render_rows_async); d->spp <= 0; first < 0,
 * count <= 0 or first + count > spp; the d->flags named above; any other bit in flags. */
int rtc_render_pixels_async(const RtcDeviceScene *s, const Scene *scene, const RtcCamera *cam, const RtcRenderDesc *d,
                            const RtcSampleRange *range, const unsigned int *dPixels, size_t n, int flags,
                            void *dColors /* nullable */, float *dAccum, unsigned int *dRngState,
                            unsigned long long *dSegments /* nullable, ONE u64 */, void *stream);
/* The same for HOST arrays, synchronous, built like rtc_trace_paths: stages the list, the frame's three whole buffers
 * (colors nullable; each goes in as well as out, so the pixels that are not listed come back as they were) and the
 * counter's value, waits for the device, runs the pass on the null stream and copies the buffers and *segments back.  The
 * same refusals; RTC_ENODEV without a GPU. */
int rtc_render_pixels(const RtcDeviceScene *s, const Scene *scene, const RtcCamera *cam, const RtcRenderDesc *d,
                      const RtcSampleRange *range, const unsigned int *pixels, size_t n, int flags, void *colors,
                      float *accum, unsigned int *rngState, unsigned long long *segments);
/* A coherent order for caller-supplied rays.  The three queries above put 64 consecutive rays of the
 * caller's buffer in one wave, so their speed depends on the order the rays are stored in; these entries sort rays by a
 * 30-bit coherence key on the device and apply the order.  No query kernel and no value changes: an ordered query is
 * rtc_ray_order_async, rtc_gather_async of its inputs, the query on the gathered buffers, rtc_scatter_async of its
 * outputs -- a ray's result depends on the ray (and its seed) alone, so every output is the same bit for bit.
 * The key, all arithmetic f32, operation by operation, no contraction; bounds lo[3], hi[3] (the caller's, or the scene's:
 * the box of the upload's triangle vertices and sphere extents centre -+ r, rtc_scene_bounds; a refit does not move it):
 *   per axis a: scale_a = 32.f / (hi_a - lo_a) when hi_a > lo_a and the quotient is finite, else 0.f (host, once);
 *               t = (pos_a - lo_a) * scale_a;  c_a = !(t >= 0) ? 0 : t >= 31.f ? 31 : (int)t
 *   cell (15 bits, Morton): bit b of c_x, c_y, c_z at bits 3 b, 3 b + 1, 3 b + 2
 *   ax, ay, az = fabsf(dir.*);  L = (ax + ay) + az;  px = ax / L, py = ay / L (correctly rounded)
 *   q(p) = !(p >= 0) ? 0 : p * 64.f >= 63.f ? 63 : (int)(p * 64.f)
 *   oct = (dir.x < 0) | (dir.y < 0) << 1 | (dir.z < 0) << 2          (-0 and NaN: not negative)
 *   key = cell << 15 | oct << 12 | q(py) << 6 | q(px)                  (< 2^30)
 * rtc_ray_keys_host states it on the host (no GPU); the device's keys are the same bits.
 * rtc_ray_order_async: dOrder[0, n) becomes the permutation of [0, n) that sorts dRays by key, STABLE (equal keys keep
 * ascending index) -- a function of the rays and bounds alone; dKeys (nullable) receives key(dRays[i]) at i.  bounds: 6
 * HOST floats lo, hi, or NULL for the scene's.  dScratch: rtc_ray_order_scratch_bytes(n) bytes of device memory, 16-byte
 * aligned; all temporary storage.  An LSD radix sort of (key, index) pairs over the 30 bits, 8 bits a pass, without atomics.
 * Asynchronous on `stream`, complete there: no allocation, no synchronisation, no host read of device memory; nothing is
 * written outside dOrder[0, n), dKeys[0, n) and the scratch's stated size; the rays are only read.  It reads nothing of
 * the scene on the device (only its device number and bounds on the host), takes no part in the launch planner, leaves
 * the scene's ordering state, hooks, chain report and draw cache alone and restores the caller's current device.
 * n == 0: returns 0, nothing enqueued.  RTC_EINVAL, checked before any device call and before `s` is read: a null s,
 * dRays, dOrder or dScratch; n > 0x7fffffff; scratchBytes too small; dScratch not 16-byte aligned. */
int rtc_scene_bounds(const RtcDeviceScene *s, float lo[3], float hi[3]);
size_t rtc_ray_order_scratch_bytes(size_t n); /* a multiple of 16, monotone in n */
/* The sort's shape (host only): the keys a sort workgroup takes (B) and the workgroup counts one scan workgroup takes per
 * step of its loop (G) -- n = B +- 1, 2 B + 1 and G B + 1 are the sizes at which the sort takes another path. */
int rtc_ray_order_shape(int *keysPerGroup, int *scanGroups);
int rtc_ray_order_async(const RtcDeviceScene *s, const Ray *dRays, size_t n, const float *bounds,
                        unsigned *dOrder, unsigned *dKeys, void *dScratch, size_t scratchBytes, void *stream);
/* The same for HOST arrays, synchronous, staged like rtc_trace_rays (keys nullable).  RTC_ENODEV without a GPU. */
int rtc_ray_order(const RtcDeviceScene *s, const Ray *rays, size_t n, const float *bounds, unsigned *order,
                  unsigned *keys);
int rtc_ray_keys_host(const Ray *rays, size_t n, const float lo[3], const float hi[3], unsigned *keys);
/* Apply an order on the current device (like rtc_copy_async), asynchronously on `stream`: n elements of elemBytes each,
 * gather dst[i] = src[order[i]], scatter dst[order[i]] = src[i]; dOrder holds values below n (a permutation, for a scatter
 * that leaves no element unwritten).  elemBytes is 1 -- byte loads and stores, any alignment, as rtc_occluded_async's byte
 * buffer -- or a multiple of 4 up to 64 -- dword copies, consecutive lanes on consecutive dwords; 4-byte aligned buffers.
 * dst must not alias src.  RTC_EINVAL: another elemBytes, a null pointer, n > 0x7fffffff, dDst == dSrc, a misaligned
 * dword buffer.  n == 0: returns 0, nothing enqueued. */
int rtc_gather_async(void *dDst, const void *dSrc, const unsigned *dOrder, size_t n, size_t elemBytes, void *stream);
int rtc_scatter_async(void *dDst, const void *dSrc, const unsigned *dOrder, size_t n, size_t elemBytes, void *stream);
/* The next pixel list of an adaptively sampled frame, made on the device: the producer of the list that
 * rtc_render_pixels_async takes, the per-pixel sample counts, and the final normalise-and-quantise.  The entries work on
 * the current device (like rtc_gather_async): they name no scene and take no part in the launch planner.
 * The selection, for pixel p with A = dAccum[3 p ..] and P = dPrev[3 p ..] (a snapshot of the accumulator at an earlier
 * sample count, which the caller makes with a device-to-device copy), all arithmetic f32, operation by operation, no
 * contraction:
 *   e_c = fabsf(A_c * wAccum - P_c * wPrev)   for c = x, y, z
 *   d   = (e_x + e_y) + e_z
 *   l   = ((A_x + A_y) + A_z) * wLevel
 *   selected(p) = d * d > threshold * (l + floor)
 * The comparison is strict (equality is not selected) and false for any NaN; infinities, an overflowing d * d and a
 * negative l + floor get what the arithmetic gives.  The weights are the caller's: with wAccum = spp / (done - before),
 * wPrev = wAccum + spp / before and wLevel = spp / done the statement compares the mean of the samples since the snapshot
 * with the mean before it, a squared relative-error test without a division or a square root.  samplesDone is what the
 * call stamps into dSamples. */
typedef struct RtcSelectDesc {
    float wAccum, wPrev, wLevel; /* host weights, the caller's */
    float floor, threshold;
    int samplesDone;
} RtcSelectDesc;
/* rtc_select_pixels_async.  The input sequence is dIn[0, nIn), or 0 .. pixelCount - 1 with dIn == NULL (nIn must then be
 * 0).  An entry >= pixelCount is invalid: nothing is loaded for it, it is not selected and not stamped -- the sentinel tail
 * of an earlier output is this case, and invalid entries may stand anywhere.  The selected valid entries go to
 * dOut[0, min(count, capacity)) IN INPUT ORDER: the output is a subsequence of the input (stable; ascending when the input
 * is; duplicates judged and listed once each); dOut[k] = 0xFFFFFFFF for min(count, capacity) <= k < capacity, which
 * rtc_render_pixels_async skips; *dCount = count, a store: the number selected BEFORE the cut at capacity, so the caller
 * sees an overflow.  Where dSamples is given, dSamples[p] = sel->samplesDone for every valid entry p, selected or not (the
 * select visits exactly the pixels the pass before it rendered).  dOut == NULL goes with capacity == 0: a call that only
 * stamps and counts.  nIn == 0 with a list: dOut[0, capacity) becomes sentinels and *dCount = 0 -- enqueued work, not a
 * no-op, because the next pass reads the list.
 * dScratch: rtc_select_scratch_bytes(n) bytes of device memory, 16-byte aligned, n the input sequence's length (nIn, or
 * pixelCount without a list); all temporary storage.  Three kernels -- judge (one ballot word per 64 entries and a count
 * per tile of T entries), scan (one workgroup, G tile counts a step), emit -- without atomics and without one workgroup
 * waiting for another, so the result is a function of the inputs alone.
 * Asynchronous on `stream`, complete there: no allocation, no synchronisation, no host read of device memory; nothing is
 * written outside dOut[0, capacity), the 8 bytes of dCount, dSamples at valid entries and the scratch's stated size; the
 * accumulator, the snapshot and the input are only read.  The frame's buffers must not be the target of an RTC_F_OVERLAP
 * launch still in flight (rtc_render_pixels_async's rule).
 * RTC_EINVAL, checked before any device call: a null dAccum, dPrev or sel; pixelCount, nIn or capacity > 0x7fffffff;
 * dIn == NULL with nIn != 0; dOut == NULL with capacity != 0; dOut, dCount and dSamples all null; dOut == dIn; dSamples
 * given with samplesDone < 0; dScratch null, not 16-byte aligned or scratchBytes too small. */
size_t rtc_select_scratch_bytes(size_t nIn); /* a multiple of 16, monotone in nIn */
/* The select's shape (host only): the entries a workgroup takes (T) and the tile counts the scan workgroup takes per step
 * of its loop (G) -- n = T +- 1, 2 T + 1 and G T + 1 are the sizes at which the select takes another path. */
int rtc_select_shape(int *entriesPerGroup, int *scanGroups);
int rtc_select_pixels_async(const float *dAccum, const float *dPrev, size_t pixelCount,
                            const unsigned *dIn /* nullable */, size_t nIn, const RtcSelectDesc *sel,
                            unsigned *dOut /* nullable */, size_t capacity, unsigned long long *dCount /* nullable */,
                            int *dSamples /* nullable */, void *dScratch, size_t scratchBytes, void *stream);
/* The same statement and the same sequence semantics for HOST arrays in plain C++, without a GPU and without scratch: what
 * the device's output, count and samples are compared with, byte for byte.  The same refusals (but the scratch's). */
int rtc_select_pixels_host(const float *accum, const float *prev, size_t pixelCount, const unsigned *in, size_t nIn,
                           const RtcSelectDesc *sel, unsigned *out, size_t capacity, unsigned long long *count,
                           int *samples);
/* The displayable frame of an adaptive render: every sample is weighted 1 / spp, so a pixel that stopped at s samples is
 * spp / s too dark.  Per pixel p: s = dSamples[p]; scale = s > 0 ? (float)spp / (float)s : 0.f (the correctly rounded
 * f32 division); dColors[3 p + c] = floatToUint(dAccum[3 p + c] * scale) (moremath.c:25-30; NaN gives 0, as
 * rtc_quantize).  Exactly 3 * pixelCount bytes are written, at any byte alignment of dColors: whole dwords where aligned,
 * single bytes at a ragged head or tail.  Asynchronous on `stream`, on the current device.  pixelCount == 0: returns 0,
 * nothing enqueued.  RTC_EINVAL: a null pointer, spp <= 0, pixelCount > 0x7fffffff. */
int rtc_resolve_async(const float *dAccum, const int *dSamples, size_t pixelCount, int spp, void *dColors, void *stream);
/* The same for HOST arrays, without a GPU (rtc_quantize of the scaled accumulator). */
int rtc_resolve_host(const float *accum, const int *samples, size_t pixelCount, int spp, void *colors);
/* Denoise a frame on the device: an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) over the
 * accumulator, guided by the first-hit buffers (rtc_render_first_hit_async), with rtc_resolve_async's per-sample-count
 * normalisation and the quantiser folded in.  The entries work on the current device (like rtc_select_pixels_async): they
 * name no scene and take no part in the launch planner.  The image is rows * width pixels, pixel (x, y) at p = y * width
 * + x, compact in launch-row order like dAccum.  All arithmetic is f32, operation by operation, no contraction; every
 * division is the correctly rounded one; the device keeps subnormals, the host does too.
 * Load.  For pixel p with A = dAccum[3 p ..]:
 *   L_c = A_c                      without dSamples
 *   L_c = A_c * scale              with dSamples: s = dSamples[p]; scale = s > 0 ? (float)spp / (float)s : 0.f, exactly
 *                                  as in rtc_resolve_async
 *   L_c = albedo_c > albedoFloor ? L_c / albedo_c : L_c      then, with RTC_DN_DEMODULATE; the test is per component and
 *                                  false for NaN
 * Iteration k = 0 .. iterations - 1.  Step s = 1 << k, input image C (C = L for k = 0).  The 1-D taps are
 * H[0] = 0.375f, H[1] = 0.25f, H[2] = 0.0625f.  For the pixel at (x, y) with centre colour c, normal n and depth z:
 *   sum_c = c_c * 0.140625f;  wsum = 0.140625f        (the centre tap is never edge-tested)
 *   the other 24 taps in row-major order: j = -2 .. 2 outer, i = -2 .. 2 inner, skipping (0, 0)
 *     qx = x + i s, qy = y + j s; a tap outside [0, width) x [0, rows) is skipped
 *     w = H[|i|] * H[|j|]
 *     normal weight, when guides->normal is given:
 *       t = (n.x nq.x + n.y nq.y) + n.z nq.z;  t = t > 0 ? t : 0.f;  then normalSquarings times t = t * t;  w = w * t
 *     depth weight, when guides->depth is given:
 *       dz = (z - zq) * depthScale;  w = w / (1.f + dz * dz)
 *     colour weight, always:
 *       e = (|c.x - q.x| + |c.y - q.y|) + |c.z - q.z|;  w = w / (1.f + (e * e) * cs_k)
 *       cs_k = colorScale * (float)(1 << 2k), computed on the host
 *     if (!(w > 0)) continue;     (a NaN or zero weight never enters, so a NaN neighbour cannot spread; a pixel's own NaN
 *                                  stays)
 *     sum_c = sum_c + q_c * w;  wsum = wsum + w
 *   C'_c = sum_c / wsum
 * Store.  After the last iteration: O_c = albedo_c > albedoFloor ? C'_c * albedo_c : C'_c with RTC_DN_DEMODULATE, else
 * O_c = C'_c; dOut[3 p + c] = O_c; where dColors is given, byte 3 p + c of it = floatToUint(O_c) (moremath.c:25-30; NaN
 * gives 0, as rtc_quantize), at any byte alignment of dColors, exactly 3 * width * rows bytes, as rtc_resolve_async.
 * Miss pixels.  A first-hit miss has the normal +0, +0, +0 and the depth 999999.f: wherever normals are given it gives
 * and takes the weight 0 (t = 0), so it comes out as c * w0 / w0 with w0 = 0.140625f, its own colour up to that rounding.
 * guides: nullable, and each member nullable (no weight of that kind); prim is ignored.  dSamples: nullable.
 * dScratch: rtc_denoise_scratch_bytes(width * rows, iterations) bytes of device memory, 16-byte aligned; all temporary
 * storage: a pack pass performs the load step into 16-byte entries (colour rgb + pad; normal.xyz + depth), so that every
 * tap is two 16-byte loads, and the intermediate images alternate between two such colour images.  An iteration is one
 * kernel: at steps 1 and 2 a workgroup stages a tileW x tileH tile of the image plus a halo of 2 s in LDS and takes the
 * taps from there, from step 4 on every tap is loaded from global memory; either way a pixel's taps are summed in the
 * order above, in registers.  No atomics: the result is a function of the inputs alone.
 * Asynchronous on `stream`, complete there: no allocation, no synchronisation, no host read of device memory; nothing is
 * written outside dOut[0, 3 n), the 3 n bytes of dColors (n = width * rows) and the scratch's stated size; the
 * accumulator, the samples and the guides are only read.
 * RTC_EINVAL, checked before any device call: a null dAccum, d or dOut; width or rows <= 0; width * rows > 0x7fffffff;
 * iterations outside 1 .. 6; normalSquarings outside 0 .. 8; a flag other than RTC_DN_DEMODULATE; RTC_DN_DEMODULATE
 * without guides->albedo; dSamples given with spp <= 0; dOut == dAccum; dScratch null, not 16-byte aligned or
 * scratchBytes too small. */
#define RTC_DN_DEMODULATE 0x1
typedef struct RtcDenoiseDesc {
    int width, rows;        /* the image: rows * width pixels, compact launch-row order, like dAccum */
    int iterations;         /* 1 .. 6: iteration k = 0.. uses step s = 1 << k */
    int flags;              /* 0 or RTC_DN_DEMODULATE (needs guides->albedo) */
    int spp;                /* with dSamples: the frame's spp, as rtc_resolve_async; otherwise ignored */
    int normalSquarings;    /* 0 .. 8: the normal weight is max(0, n.nq) ^ (2 ^ normalSquarings) */
    float depthScale, colorScale, albedoFloor; /* host floats, the caller's */
} RtcDenoiseDesc;
size_t rtc_denoise_scratch_bytes(size_t pixelCount, int iterations); /* a multiple of 16, monotone in both */
/* The filter's shape (host only): the image tile a workgroup stages at steps 1 and 2 -- width or rows = tile +- 1 and
 * 2 tile + 1 are the sizes at which the kernels take another path (from step 4 on a workgroup takes tileW x 8 pixels). */
int rtc_denoise_shape(int *tileW, int *tileH);
int rtc_denoise_async(const float *dAccum, const int *dSamples /* nullable */, const RtcHitBuffers *guides /* nullable */,
                      const RtcDenoiseDesc *d, float *dOut, void *dColors /* nullable */, void *dScratch,
                      size_t scratchBytes, void *stream);
/* The same statement for HOST arrays in plain C++, without a GPU and without scratch: what the device's dOut and dColors
 * are compared with, byte for byte.  The same refusals (but the scratch's); RTC_ENOMEM when its own images do not fit. */
int rtc_denoise_host(const float *accum, const int *samples, const RtcHitBuffers *guides, const RtcDenoiseDesc *d,
                     float *out, void *colors);
/* Copy `bytes` (16-byte aligned pointers) on `stream` with `blocks` workgroups (<= 0: 32): e.g. Color[] from HBM
 * into pinned host memory with a small CU footprint while render kernels run (the runtime's D2H blit kernel
 * takes one workgroup on every CU).  Asynchronous. */
int rtc_copy_async(void *dst, const void *src, size_t bytes, int blocks, void *stream);
/* Copy `bytes` of device memory into page-locked host memory (hipHostMalloc) with the SDMA copy engines (HSA
 * runtime), blocking until done; the caller orders it after the frame (e.g. a host thread that waits for the
 * frame's event first).  Unlike the runtime's D2H blit kernel it does not slow render kernels running at the
 * same time (~0.01 vs ~0.1 ms per 1080p frame). */
int rtc_copy_d2h_dma(void *hostDst, const void *devSrc, size_t bytes);
/* Copy-engine timeouts (rtc_copy_d2h_dma, rtc_copy_rows_d2h_dma, rtc_frame_loop): a copy that has not completed after
 * 20 s (RTC_DMA_TIMEOUT_MS overrides) returns RTC_ETIMEDOUT, but the engine may still read its source and write its
 * destination.  The library keeps such a copy listed (its completion signal is neither reused nor destroyed) until the
 * signal shows it ended.  After RTC_ETIMEDOUT the caller must not free, reuse or unregister either buffer while
 * rtc_dma_pending over it is > 0; rtc_host_unregister refuses such a range with RTC_EBUSY.
 * rtc_dma_pending: the number of listed copies whose source or destination overlaps [p, p + bytes) (p = NULL: all),
 * reaping those that have ended. */
int rtc_dma_pending(const void *p, size_t bytes);
/* Test hook of that bookkeeping (no copy engine involved): list (pending != 0) or drop a simulated in-flight copy
 * into [p, p + bytes). */
int rtc_dma_debug_inflight(void *p, size_t bytes, int pending);
/* Copy `rows` rows of `rowBytes` from device memory (row pitch srcPitch) into page-locked host memory (row pitch
 * hostPitch) with the SDMA engines, blocking until done: one SDMA sub-window copy (all pointers, pitches and rowBytes
 * multiples of 4), else one linear copy per row.  A rank's compact rows y = r + k*G (rtc_render_rows_async with
 * rowStart r, rowStride G) land in their places of the interleaved host frame with hostDst = frame + r*W*3 and
 * hostPitch = G*W*3 -- every GPU writes its own rows over its own PCIe link, as the reference's threads write their
 * rows into the shared image (main.c:84, :285-302).  The host memory is hipHostMalloc'd or registered
 * (rtc_host_register, e.g. a shared-memory frame all ranks map); the copy runs through the CPU agent nearest the
 * source GPU. */
int rtc_copy_rows_d2h_dma(void *hostDst, size_t hostPitch, const void *devSrc, size_t srcPitch, size_t rowBytes,
                          int rows);
/* Page-lock (hsa_amd_memory_lock, every agent) / release an existing host range so the copies above can target it. */
int rtc_host_register(void *p, size_t bytes);
int rtc_host_unregister(void *p);

/* Test hooks of the launch planner (rtc_plan.h; no GPU involved): the ordering decisions rtc_render_rows_async would take
 * for a sequence of launches on a scene of triCount triangles, without any device.  rtc_plan_sim_launch plans one launch
 * (d; the caller's stream identity `stream`, 0 = the null stream; Color / accumulator buffer identities; segment counters
 * asked for or not; the camera cam[13] = origin, ex, ey, ez, fov and environment env[14] = sun, horizon, zenith, ground,
 * focus, intensity that decide the pixel values) and writes its operations as 4 ints each (kind 0 kernel / 1 record /
 * 2 wait, stream 0 caller / 1, 2 cull streams / 3 side stream, event, kernel) and each kernel's memory footprint as 6 u64
 * each (op index, resource, access, id, byte range), then one u64 record (~0, scratch regrown, slot, alternating streams,
 * overlapped, slot offset).  Returns nOps | (footprint records << 8).  legacySlotLayout: round 5's broken scratch
 * layout (slot h at h x the launch's own slot size), for the test that must catch it. */
typedef struct RtcPlanSim RtcPlanSim;
int rtc_plan_sim_create(int triCount, int legacySlotLayout, RtcPlanSim **out);
int rtc_plan_sim_launch(RtcPlanSim *sim, const RtcRenderDesc *d, unsigned long long stream, unsigned long long colors,
                        unsigned long long accum, int segments, const float cam[13], const float env[14], int *ops,
                        int maxOps, unsigned long long *footprint, int maxFootprint);
/* The simulated scene's spheres (0 by default) and whether its upload gate would allow the split launch for them; a
 * launch with d->trianglesOnly renders none. */
int rtc_plan_sim_set_spheres(RtcPlanSim *sim, int sphereCount, int gateAllows);
/* The simulated scene's draw cache (off by default): on, the launches that would use it declare the slot table with its
 * pool counter (footprint resource 12) and their slot's item-draw array (resource 13, id = the slot), and a launch that
 * clears the cache or regrows the item-draw array reports it in the `scratch regrown` field (the device is synchronised). */
int rtc_plan_sim_set_draw_cache(RtcPlanSim *sim, int on);
/* Makes the next rtc_plan_sim_launch (only) a pass of rtc_render_samples_async: samples [first, first + count) of its
 * d->spp, the RNG-state buffer's identity (footprint resource 8).  That launch returns RTC_EINVAL where the entry point
 * would (a bad range, RTC_F_OVERLAP, no accumulator or state buffer). */
int rtc_plan_sim_set_sample_range(RtcPlanSim *sim, int first, int count, unsigned long long rngBuffer);
/* Makes the next rtc_plan_sim_launch (only) a first-hit launch (rtc_render_first_hit_async): the four buffers' identities
 * (footprint resource 10, one write record per identity that is not 0; 0: the buffer is not asked for).  That launch's
 * colors / accum / segments arguments are ignored; its kernel is kernel 10; it returns RTC_EINVAL where the entry point
 * would (every identity 0, a flag other than RTC_F_NO_TILE_CULL, bad geometry). */
int rtc_plan_sim_set_first_hit(RtcPlanSim *sim, unsigned long long prim, unsigned long long depth,
                               unsigned long long normal, unsigned long long albedo);
/* Plans one rtc_scene_update_async on the caller's stream `stream`, in rtc_plan_sim_launch's encodings: the waits, then the
 * refit kernel (kernel 9) with two footprint records -- it writes one generation of the scene records (resource 9, id = the
 * generation) and may read the other -- then one u64 record (~0, 0, the generation written, 0, 0, 0).  Launches planned
 * afterwards read that generation (their kernels' footprints name it).  rtc_plan_sim_set_update_fault breaks later updates
 * on purpose, for the test that must catch it: mode 1 drops the update's waits, 2 keeps the slots' primary records valid,
 * 3 writes the generation the launches in flight read; 0 mends it. */
int rtc_plan_sim_update(RtcPlanSim *sim, unsigned long long stream, int *ops, int maxOps, unsigned long long *footprint,
                        int maxFootprint);
int rtc_plan_sim_set_update_fault(RtcPlanSim *sim, int mode);
/* Plans one rtc_scene_regroup_async on the caller's stream `stream`, in rtc_plan_sim_update's encodings: an update's waits,
 * then on stream 0, without events, the centroid kernel (kernel 14: writes the caller's scratch, resource 19, id =
 * `scratch`), one level kernel per level of the scene's triangle count (kernel 15: reads and writes the scratch), the index
 * kernel (kernel 16: reads the scratch, writes the membership, resource 18, id 0) and the refit (kernel 9: an update's two
 * records, then a read of the membership); then one u64 record (~0, 0, the generation written, the levels, 0, 0).
 * rtc_plan_sim_update's output is unchanged: its refit names no membership.  RTC_EINVAL where the entry point would, as far
 * as the planner sees it: a `scratch` of 0 or not a multiple of 16, a scene of no triangles or of more than
 * rtc_scene_regroup_max_tris(). */
int rtc_plan_sim_regroup(RtcPlanSim *sim, unsigned long long stream, unsigned long long scratch, int *ops, int maxOps,
                         unsigned long long *footprint, int maxFootprint);
/* Plans one rtc_trace_rays_async on the caller's stream `stream`, in rtc_plan_sim_update's encodings: one kernel op (kernel
 * 11, stream 0, no event) with its footprint records -- it reads the current generation (resource 9, id = the generation)
 * and the ray buffer (resource 11, id = `rays`) and writes each hit buffer asked for (resource 10, id = hit[k]; 0: not
 * asked for), in that order -- then one u64 record (~0, 0, the generation read, 0, 0, 0).  The planner's state is left as
 * it was.  RTC_EINVAL where the entry point refuses: `rays` 0, every hit identity 0, a flag other than
 * RTC_F_NO_CLUSTER_CULL. */
int rtc_plan_sim_trace_rays(RtcPlanSim *sim, unsigned long long stream, unsigned long long rays,
                            const unsigned long long hit[4], int flags, int *ops, int maxOps,
                            unsigned long long *footprint, int maxFootprint);
/* Plans one rtc_trace_paths_async on the caller's stream `stream`, in rtc_plan_sim_trace_rays's encodings: one kernel op
 * (kernel 12, stream 0, no event) with its footprint records -- it reads the current generation (resource 9), the ray
 * buffer (resource 11, id = `rays`), the seeds (resource 14, id = `seeds`) and, with sampleFirst > 0, the radiance
 * (resource 15, id = `radiance`), writes the radiance and, where asked for (an identity that is not 0), the seeds
 * (resource 14, id = `seedsOut`) and the caller's segment counter (resource 7, an atomic add), in that order -- then one
 * u64 record (~0, 0, the generation read, 0, 0, 0).  The planner's state is left as it was.  RTC_EINVAL where the entry
 * point refuses: `rays`, `seeds` or `radiance` 0, sampleFirst < 0, a flag other than RTC_F_NO_CLUSTER_CULL and
 * RTC_F_WAVE_PER_RAY (which plans the same operation and the same records: only the kernel behind the number
 * differs). */
int rtc_plan_sim_trace_paths(RtcPlanSim *sim, unsigned long long stream, unsigned long long rays,
                             unsigned long long seeds, unsigned long long radiance, unsigned long long seedsOut,
                             unsigned long long segments, int sampleFirst, int flags, int *ops, int maxOps,
                             unsigned long long *footprint, int maxFootprint);
/* Plans one rtc_occluded_async on the caller's stream `stream`, in rtc_plan_sim_trace_rays's encodings: one kernel op
 * (kernel 13, stream 0, no event) with its footprint records -- it reads the current generation (resource 9), the ray
 * buffer (resource 11, id = `rays`) and, where given (an identity that is not 0), the limits (resource 16, id = `tMax`),
 * writes the bytes (resource 17, id = `occluded`) and adds to the caller's counter (resource 7, an atomic add) where asked
 * for, in that order -- then one u64 record (~0, 0, the generation read, 0, 0, 0).  The planner's state is left as it
 * was.  RTC_EINVAL where the entry point refuses: `rays` 0, `occluded` and `count` both 0, a flag other than
 * RTC_F_NO_CLUSTER_CULL. */
int rtc_plan_sim_occluded(RtcPlanSim *sim, unsigned long long stream, unsigned long long rays, unsigned long long tMax,
                          unsigned long long occluded, unsigned long long count, int flags, int *ops, int maxOps,
                          unsigned long long *footprint, int maxFootprint);
/* Plans one rtc_render_pixels_async on the caller's stream `stream`, in rtc_plan_sim_trace_paths's encodings: one kernel op
 * (kernel 17, stream 0, no event) with its footprint records -- it reads the current generation (resource 9) and the list
 * (resource 20, id = `pixels`) and, with first > 0, the accumulator (resource 6, id = `accum`) and the RNG states
 * (resource 8, id = `rng`), writes the accumulator and the states and, where asked for (an identity that is not 0), the
 * Color (resource 5, id = `colors`) and adds to the caller's segment counter (resource 7, an atomic add), in that order --
 * then one u64 record (~0, 0, the generation read, 0, 0, 0).  The planner's state is left as it was.  RTC_EINVAL where the
 * entry point refuses, as far as the planner sees it: `pixels`, `accum` or `rng` 0, first < 0, a flag other than
 * RTC_F_NO_CLUSTER_CULL and RTC_F_WAVE_PER_RAY (which plans the same operation and the same records). */
int rtc_plan_sim_render_pixels(RtcPlanSim *sim, unsigned long long stream, unsigned long long pixels,
                               unsigned long long colors, unsigned long long accum, unsigned long long rng,
                               unsigned long long segments, int first, int flags, int *ops, int maxOps,
                               unsigned long long *footprint, int maxFootprint);
/* The last planned launch's scratch, as rows of 3 u64: (slot offset, slot bytes, scratch bytes the launch needs), (scratch
 * bytes allocated once it is enqueued, sample-slot bytes it needs, bit mask of the buffers it binds: rtc_plan.h Buf),
 * then one row per scratch region it binds (region index, byte offset in the scratch, bytes in use).  Returns the
 * number of rows (at most 10: maxRows must hold them). */
int rtc_plan_sim_regions(const RtcPlanSim *sim, unsigned long long *rows, int maxRows);
int rtc_plan_sim_release(RtcPlanSim *sim);

/* Pipelined frames on one device, driven from native code (the per-frame host cost is the launch enqueue alone).
 * Frame k renders d's rows with RTC_F_OVERLAP into devRows[k % nbuf] (device buffers of rows_selected*width*3 bytes)
 * on `stream`; a copy thread waits for the frame's event and moves the rows into hostRows[k % nbuf] (page-locked,
 * pitch hostPitch between consecutive rows, or between consecutive bands of d->rowBand rows, each band's rows
 * adjacent) with rtc_copy_rows_d2h_dma; buffer b is rendered into again once its copy has finished.
 * Returns when the last frame's rows are in host memory.  Uses the scene's frame event hook itself. */
typedef struct RtcLoopStats {
    double wallMs;       /* first enqueue .. the last frame's rows in host memory (host clock) */
    int frames;
    double enqueueMs;    /* host time spent in rtc_render_rows_async, summed over the frames */
    double copyMsMedian; /* one frame's SDMA copy as the copy thread timed it: median and maximum */
    double copyMsMax;
} RtcLoopStats;
int rtc_frame_loop(RtcDeviceScene *s, const Scene *scene, const RtcCamera *cam, const RtcRenderDesc *d,
                   void *const *devRows, void *const *hostRows, size_t hostPitch, int nbuf, int frames, void *stream,
                   RtcLoopStats *stats);
/* The same loop with a moving camera: frame k renders with cams[k % ncams] (e.g. an orbit; every camera change
 * re-derives the per-launch primary records, and an unjoined sky pass of another camera is waited for before the
 * next launch writes its buffer).  rtc_frame_loop is this with ncams = 1.  On an error (e.g. RTC_ETIMEDOUT from a
 * copy) the loop stops enqueueing, waits for the copies it started and returns the first error; no buffer is
 * rendered into again after its copy failed. */
int rtc_frame_loop_cameras(RtcDeviceScene *s, const Scene *scene, const RtcCamera *cams, int ncams,
                           const RtcRenderDesc *d, void *const *devRows, void *const *hostRows, size_t hostPitch,
                           int nbuf, int frames, void *stream, RtcLoopStats *stats);

/* Re-assemble a row-interleaved gather: dCompact holds `parts` blocks of rowsPerPart*width*3 bytes, block
 * g holding rows y = g + k*parts; dOut receives the height*width*3 frame.  Asynchronous on `stream`. */
int rtc_deinterleave_async(const void *dCompact, int parts, int rowsPerPart, int width, int height,
                           void *dOut, void *stream);
/* The same for parts of interleaved bands of rowBand rows (RtcRenderDesc.rowBand; 0 or 1: single rows): block g holds
 * the bands b = g, g + parts, ... (rows b*rowBand .. b*rowBand + rowBand - 1), each band's rows in order. */
int rtc_deinterleave_bands_async(const void *dCompact, int parts, int rowsPerPart, int width, int height, int rowBand,
                                 void *dOut, void *stream);

/* ---- device probes: run single reference functions on the GPU for known-answer tests --------------- */
/* Each copies inputs to the current device, runs one kernel of the same device code the renderer uses,
 * and copies results back (synchronous). */
int rtc_probe_ray_triangle(const Ray *rays, const Triangle *tris, size_t n, int *didHit, float *dst);   /* raytracing.c:186 */
int rtc_probe_ray_sphere(const Ray *rays, const Sphere *spheres, size_t n, int *didHit, float *dst,
                         vec3 *normal);                                                                 /* raytracing.c:162 */
int rtc_probe_environment(const Ray *rays, const Scene *scenes, size_t n, vec3 *out);                  /* raytracing.c:151 */
int rtc_probe_random(const unsigned int *seeds, size_t n, int draws, float *uniform, float *normal,
                     vec3 *direction);                                                                  /* moremath.c:89-108 */
/* The sky kernel's per-pixel sun skip (no reference counterpart; raytracing.c:155-158 is what it must reproduce), for one
 * scene on every ray, with the limit and the gating a launch of that scene computes on the host: vanish[i] = 1 where the
 * sun term is proved below half an ulp of every colour component, out[i] = getEnvironmentLight evaluated with that skip
 * (equal to rtc_probe_environment's value for every ray), and sum[i] = the sky kernel's pixel sum of spp camera-ray misses
 * (main.c:97-99: from +0, spp times sum + (0 + environment) * (1 / spp)). */
int rtc_probe_sun_vanish(const Ray *rays, const Scene *scene, size_t n, int spp, int *vanish, vec3 *out, vec3 *sum);
/* The bound the skip compares focus * log2(x) with in a launch of the scene (host only; -inf: the scene's colours or sun
 * admit no skip). */
int rtc_env_vanish_limit(const Scene *scene, double *limit);
/* Soundness probe of the bounce-ray cluster culling (no reference counterpart; raytracing.c:186-214 is the
 * per-triangle test it must never contradict): clusters `tris` as rtc_scene_upload does and, for every ray and
 * every cluster ball (8 triangles) and chunk ball (32 clusters, scenes of more than one chunk), counts [0] hits
 * inside balls the ray was culled from (0 when sound), [1] balls culled, [2] ball tests, [3] hits, [4] float
 * bits of the largest hit-point excess over a ball's radius, [5] hits on triangles the first-bounce reach mask
 * calls unreachable from the ray's origin (0 when sound), [6] (ray, triangle) pairs it calls so. */
int rtc_probe_cluster_bound(const Triangle *tris, int triCount, const Ray *rays, size_t n,
                            unsigned long long counts[7]);
/* The split launch's item records (no reference counterpart; main.c:88-94 is the ray each must carry): uploads the
 * scene to the current device, runs the preparation and the culls of the launch `d` as rtc_render_rows_async would (no
 * render kernel) and copies back counts[16] = the entries of the 16 geometry-pixel sub-lists, info[4] = {entries a
 * sub-list can hold, 8x8 tiles per launch row, tiles, 1 when the launch has more than 65,535 columns or launch rows},
 * records = the sub-lists' records one after the other, 4 dwords each: x | launch row << 16 (tile * 64 + bit in such a wide
 * launch) and the float bits of the pixel's primary direction, and pixMask = per tile its pixels with a primary candidate
 * (bit = (row % 8) * 8 + x % 8).  RTC_EINVAL when the launch is not a split launch or an output is too small. */
int rtc_probe_item_records(const Triangle *tris, int triCount, const Sphere *spheres, int sphereCount, const Scene *scene,
                           const RtcCamera *cam, const RtcRenderDesc *d, int counts[16], int info[4],
                           unsigned int *records, size_t maxRecords, unsigned long long *pixMask, size_t maxTiles);
/* Soundness probe of the primary cull (no reference counterpart; a test decides hits with rayTriangle on the CPU): uploads
 * the triangles, runs the preparation and the culls of the launch `d` as rtc_render_rows_async would (no render kernel) and
 * copies back kept[(launch row * width + x) * triCount + t] = 1 when the primary filter keeps triangle t for that pixel
 * (evaluated by the render kernels' own functions on the launch's records and the pixel's primary direction, for every
 * triangle whatever the tile prefilter said), tileBits = per 8x8 tile its candidate bit-set (info[2] words of 64
 * triangles; tile = (row / 8) * info[1] + x / 8), pixMask as rtc_probe_item_records, and info[4] = {tiles, tiles per
 * launch row, words per tile, 1 when the superblock level of the tile cull ran}.  Optional (null: not wanted): primF =
 * the launch's filter records, 16 floats per triangle {N, mnd, sigma Gd, c, sigma Gu, -m, sigma q0, 0}; cones and pruned
 * (both or neither, maxTiles tiles) = per tile the prefilter's {eDir, vmin, vmax, 1 when the cone is usable} and
 * pruned[tile * triCount + t] = 1 when the tile's own prefilter prunes triangle t.  RTC_EINVAL when the launch is not a
 * split launch or an output is too small. */
int rtc_probe_primary_cull(const Triangle *tris, int triCount, const Scene *scene, const RtcCamera *cam,
                           const RtcRenderDesc *d, unsigned char *kept, size_t maxKept, unsigned long long *tileBits,
                           size_t maxWords, unsigned long long *pixMask, size_t maxTiles, int info[4], float *primF,
                           double *cones, unsigned char *pruned);
/* The scene records (no reference counterpart; main.c:229-243 builds the arrays they replace), for the tests of
 * rtc_scene_update_async.  Both write up to six arrays -- triangles (64 B each, reference order), materials (32 B), spheres
 * (48 B), the triangles in cluster order (64 B; dword 12 = the reference index, -1 for padding, dword 13 = the
 * aligned-normal flag), the cluster balls and the chunk balls (32 B: centre, radius, alpha, beta, gamma E, E) -- into the
 * buffers given (null: not wanted); bytes[6] holds each buffer's capacity on entry and each array's size on return
 * (RTC_EINVAL when a buffer is too small; call with null buffers first for the sizes).
 * rtc_scene_records_host runs without a GPU: it clusters `tris` as rtc_scene_upload does and returns the upload's records,
 * or with newTris (triCount of them) the records a refit of that membership to newTris must produce -- the host statement
 * the device kernel is compared with byte for byte.  rtc_probe_scene_records synchronises the device and copies back the
 * records a launch enqueued now would read (the current generation). */
int rtc_scene_records_host(const Triangle *tris, int triCount, const Triangle *newTris, const Sphere *spheres,
                           int sphereCount, void *outTris, void *outMats, void *outSpheres, void *outClTris,
                           void *outClusters, void *outChunks, size_t bytes[6]);
int rtc_probe_scene_records(const RtcDeviceScene *s, void *outTris, void *outMats, void *outSpheres, void *outClTris,
                            void *outClusters, void *outChunks, size_t bytes[6]);

#ifdef __cplusplus
}
#endif
#endif /* RTC_H */
