/* rtc_trace_rays.h -- rtc_trace_rays: the closest hit of caller-supplied rays against the resident scene
 * (rtc_trace_rays_async): calculateRayCollision(ray, trianglesOnly) (raytracing.c:216-240) for n arbitrary
 * Rays, into rtc_first_hit's four buffers -- and trace_closest, the closest-hit walk of every query kernel that follows
 * (rtc_trace_paths.h, rtc_render_pixels.h).
 * A section of rtc_render.hip's translation unit: included there once, after the headers above it in that file's
 * list (it uses their names, and rtcdev's through the file's using-directive). */
#pragma once

/* The kernel's own arguments (not RenderParams: no launch geometry, camera, scratch or primary record is involved): the
 * bound generation's records and their counts, the rays, and the four outputs (each nullable). */
struct TraceRaysArgs {
    const DevTri *__restrict__ tris;         /* reference order, triPadded + 8 records */
    const DevMat *__restrict__ mats;
    const DevSphere *__restrict__ spheres;
    const DevTri *__restrict__ clTris;       /* cluster order, pad0 = reference index (-1: padding, a zero record) */
    const DevCluster *__restrict__ clusters;
    const DevCluster *__restrict__ chunks;
    int triPadded, sphereCount, clusterCount, chunkCount;
    const float *__restrict__ rays;          /* n Rays: pos.xyz, dir.xyz (24 B, 4-byte aligned) */
    unsigned n;                              /* <= 0x7fffffff */
    int *__restrict__ prim;
    float *__restrict__ depth;
    float *__restrict__ normal;
    float *__restrict__ albedo;
};

/* The closest hit of one ray per lane (calculateRayCollision(ray, trianglesOnly), raytracing.c:216-240), wave-wide, for
 * every query kernel of this unit: `A` is any argument struct with TraceRaysArgs' record fields.  `live` is this lane's bit
 * of the participating lanes: a lane that is not live runs through the wave-uniform loops with whatever ray it holds, keeps
 * no ball in the ballots and gets a result its caller discards.  Call it from wave-uniform control flow.
 * Spheres first, per lane, in index order with strict `<`, as closest_hit does (A.sphereCount: 0 with trianglesOnly).
 * !CULL: closest_general over the records in reference order -- general_test, strict `<`, ascending index.
 * CULL: the cluster hierarchy, with wave-uniform loops over the chunks (scenes of more than one) and a chunk's clusters.
 * Each lane evaluates cluster_culled for its own ray -- only with rho = |dir|_1 <= kClusterRhoMax, the premise of the
 * bound (rtc_layout.h; a NaN rho compares false: never culled) -- and a ballot skips a ball no live lane keeps.  A kept
 * cluster's 8 records are scalar loads, tested by every lane with general_filter / general_exact: a lane whose own ball
 * test culled the cluster tests records that cannot hit it, which is cheaper than a branch around them.  Clusters are
 * not visited in index order, so equal distances keep the lowest reference index (general_exact's rule; a sphere's index
 * is below every triangle's): the result does not depend on the order, nor on the other lanes' rays.
 * The direction is used as given (not normalised: the reference does not).
 * (rtc_occluded's walk is another one: any hit within a distance limit.) */
template <bool SPHERES, bool CULL, class Args>
__device__ __forceinline__ Closest trace_closest(const Args &A, V3 pos, V3 dir, bool live)
{
    Closest c{999999.f, -1}; /* HitInfo closest = {0, 999999} */
    if (SPHERES) {
        for (int k = 0; k < A.sphereCount; ++k) {
            const DevSphere sp = A.spheres[k];
            float d;
            if (ray_sphere(pos, dir, V3{sp.cx, sp.cy, sp.cz}, sp.radius, d) && d < c.dst) {
                c.dst = d;
                c.idx = k;
            }
        }
    }
    const int base = SPHERES ? A.sphereCount : 0;
    if (!CULL) {
        RenderParams P{}; /* (closest_general reads the records and their padded count, nothing else) */
        P.tris = A.tris;
        P.triPadded = A.triPadded;
        closest_general(P, pos, dir, c, base);
    } else {
        const float rho = fabsf(dir.x) + fabsf(dir.y) + fabsf(dir.z), dd = dir_dd(dir);
        const bool cull = live && rho <= kClusterRhoMax; /* this lane may cull: it has a ray, within the bound's premise */
        for (int h = 0; h < A.chunkCount; ++h) {
            const int c0 = h * kChunkClusters, nCl = min(kChunkClusters, A.clusterCount - c0);
            if (A.chunkCount > 1) {
                const DevCluster H = KLOAD(A.chunks, h);
                if (!__ballot(live && !(cull && cluster_culled(pos, dir, rho, dd, H))))
                    continue;
            }
            for (int k = 0; k < nCl; ++k) {
                const DevCluster K = KLOAD(A.clusters, c0 + k);
                if (!__ballot(live && !(cull && cluster_culled(pos, dir, rho, dd, K))))
                    continue;
                const DevTri *rec = A.clTris + (size_t)(c0 + k) * kClusterSize;
#pragma unroll 4
                for (int j = 0; j < kClusterSize; ++j) {
                    const DevTri R = KLOAD(rec, j);
                    if (general_filter(pos, dir, R))
                        general_exact(pos, dir, R, base + __float_as_int(R.pad0), c);
                }
            }
        }
    }
    return c;
}

/* One lane per ray, a wave 64 consecutive rays; lanes past n load and store nothing but stay in trace_closest's wave-wide
 * operations (their ray is pos = dir = 0: whatever it is tested against is discarded).
 * Loads and stores: plain per-lane accesses.  A lane's six ray dwords lie at a 24-B stride (the compiler merges them into
 * one dwordx4 and one dwordx2 load; the wave's 1,536 B are 12 adjacent lines, read once from L2 and again from the vector
 * L1), and store_hit's stores are rtc_first_hit's (a dword each for prim and depth, a dwordx3 at a 12-B stride for normal
 * and albedo).  No staging through LDS: at ~120 record tests per ray the 56 B a ray moves are not what the kernel waits
 * for (DESIGN §3.11 has the measurement). */
template <bool SPHERES, bool CULL>
__global__ __launch_bounds__(kBlock) void rtc_trace_rays(TraceRaysArgs A)
{
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = i < (size_t)A.n;
    V3 pos{0.f, 0.f, 0.f}, dir{0.f, 0.f, 0.f};
    if (live) {
        const float *r = A.rays + 6 * i;
        pos = V3{r[0], r[1], r[2]};
        dir = V3{r[3], r[4], r[5]};
    }
    const Closest c = trace_closest<SPHERES, CULL>(A, pos, dir, live);
    if (live)
        store_hit<SPHERES>(A, pos, dir, c.idx, c.dst, i, A.prim, A.depth, A.normal, A.albedo);
}
