/* rtc_occluded.h -- rtc_occluded: "is anything in the way within tMax?" for caller-supplied rays against the resident
 * scene (rtc_occluded_async): per ray, whether calculateRayCollision(ray, trianglesOnly)
 * (raytracing.c:216-240) records a hit with dst < tMax -- one byte per ray and / or one count per launch.
 * A section of rtc_render.hip's translation unit: included there once, after rtc_trace_rays.h (it uses the names of the
 * headers above it in that file's list, and rtcdev's through the file's using-directive). */
#pragma once

/* The kernel's own arguments: the bound generation's records and their counts, the rays, the limits (nullable: none) and
 * the two outputs (each nullable, not both). */
struct OccludedArgs {
    const DevTri *__restrict__ tris;         /* reference order, triPadded + 8 records */
    const DevSphere *__restrict__ spheres;
    const DevTri *__restrict__ clTris;       /* cluster order */
    const DevCluster *__restrict__ clusters;
    const DevCluster *__restrict__ chunks;
    int triPadded, sphereCount, clusterCount, chunkCount;
    const float *__restrict__ rays;          /* n Rays: pos.xyz, dir.xyz (24 B, 4-byte aligned) */
    const float *__restrict__ tMax;          /* n limits in units of dir; null: +inf for every ray */
    unsigned n;                              /* <= 0x7fffffff */
    unsigned char *__restrict__ occluded;    /* n bytes at any alignment: 0 or 1 */
    unsigned long long *__restrict__ count;  /* += the launch's occluded rays, one atomic per wave that has any */
};

/* The any-hit form of rayTriangle for one record: general_filter's exact-safe rejection, then the reference's arithmetic
 * (general_exact's, statement for statement) with the any-hit acceptance `dst < lim` in place of the closest-hit one.
 * Strict: a hit at dst == lim is none (seeding general_exact with Closest{lim, -1} would accept it: its tie rule compares
 * the indices unsigned).  lim <= 999999.f, so the reference's own `dst < closest.dst` against the initial 999999 is
 * part of it.  NaN anywhere compares false: no hit, as in the reference. */
__device__ __forceinline__ bool general_any(V3 pos, V3 dir, const DevTri &R, float lim)
{
    if (!general_filter(pos, dir, R))
        return false;
    const V3 AB{R.abx, R.aby, R.abz}, AC{R.acx, R.acy, R.acz};
    const V3 h = cross(dir, AC);
    const float det = dot(AB, h);
    const V3 s = sub(pos, V3{R.ax, R.ay, R.az});
    const float invDet = rcp_cr(det); /* IEEE 1.f / det */
    const float u = dot(s, h) * invDet;
    const V3 q = cross(s, AB);
    const float v = dot(dir, q) * invDet;
    const float dst = dot(AC, q) * invDet;
    return !(u < 0.f || u > 1.f) && !(v < 0.f || u + v > 1.f) && !(dst < kEps) && dst < lim;
}

/* One lane per ray, a wave 64 consecutive rays, like rtc_trace_rays.  `want`: the lane has a ray whose limit can be met
 * (i < n and L > EPSILON: both reference tests report nothing below EPSILON; a NaN L compares false).  `seeking`: want,
 * and no hit with dst < L so far.  A lane is answered 1 iff it wanted and stopped seeking.  Lanes that never seek stay in
 * the wave-wide operations with pos = dir = 0.
 * Early exit: the sphere loop, every chunk, every cluster and every batch of !CULL records is entered only while some lane
 * of the wave still seeks (and, for a ball, keeps it); once none does the wave leaves all loops.  The ball test is
 * rtc_trace_rays' cluster_culled alone: a distance-limit ("reach") term beside it was built, measured and deleted
 * (it did not pay on incoherent rays).
 * Lanes that no longer seek, or whose own test culled the ball, still run a kept cluster's record tests (cheaper than a
 * branch).  That cannot set a flag wrongly: general_any fires only on what the reference's own arithmetic reports as a hit
 * of this ray with dst < L, which makes the answer 1 whichever ball it was found in; and the flag only ever goes from
 * seeking to found.  The culls have one duty: never to drop a ball that holds such a hit for a lane that seeks.
 * The answer of a lane does not depend on the other lanes: they decide only which balls are visited beyond the lane's own.
 * Stores: one byte per live lane (global_store_byte: any alignment, exactly bytes [0, n)); one 64-bit atomic add per wave
 * with an occluded ray.  No LDS. */
template <bool SPHERES, bool CULL>
__global__ __launch_bounds__(kBlock) void rtc_occluded(OccludedArgs A)
{
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = i < (size_t)A.n;
    V3 pos{0.f, 0.f, 0.f}, dir{0.f, 0.f, 0.f};
    float L = 0.f;
    if (live) {
        const float *r = A.rays + 6 * i;
        pos = V3{r[0], r[1], r[2]};
        dir = V3{r[3], r[4], r[5]};
        L = A.tMax ? A.tMax[i] : __builtin_inff();
    }
    const bool want = live && L > kEps;
    const float lim = L < 999999.f ? L : 999999.f; /* dst < lim <=> dst < L && dst < 999999.f (closest.dst's start) */
    bool seeking = want;
    if (SPHERES) {
        for (int k = 0; k < A.sphereCount && __ballot(seeking); ++k) {
            const DevSphere sp = A.spheres[k];
            float d;
            if (ray_sphere(pos, dir, V3{sp.cx, sp.cy, sp.cz}, sp.radius, d) && d < lim)
                seeking = false;
        }
    }
    if (!CULL) {
        /* every record in reference order, kClusterSize at a time (the array is padded to a multiple of 8 with zero
         * records, which the filter rejects) */
        for (int t0 = 0; t0 < A.triPadded && __ballot(seeking); t0 += kClusterSize) {
#pragma unroll 4
            for (int j = 0; j < kClusterSize; ++j) {
                const DevTri R = KLOAD(A.tris, t0 + j);
                if (general_any(pos, dir, R, lim))
                    seeking = false;
            }
        }
    } else {
        const float rho = fabsf(dir.x) + fabsf(dir.y) + fabsf(dir.z), dd = dir_dd(dir);
        const bool cull = live && rho <= kClusterRhoMax; /* this lane may cull: it has a ray, within the bound's premise */
        for (int h = 0; h < A.chunkCount && __ballot(seeking); ++h) {
            const int c0 = h * kChunkClusters, nCl = min(kChunkClusters, A.clusterCount - c0);
            if (A.chunkCount > 1) {
                const DevCluster H = KLOAD(A.chunks, h);
                if (!__ballot(seeking && !(cull && cluster_culled(pos, dir, rho, dd, H))))
                    continue;
            }
            for (int k = 0; k < nCl; ++k) {
                const DevCluster K = KLOAD(A.clusters, c0 + k);
                if (!__ballot(seeking && !(cull && cluster_culled(pos, dir, rho, dd, K))))
                    continue;
                const DevTri *rec = A.clTris + (size_t)(c0 + k) * kClusterSize;
#pragma unroll 4
                for (int j = 0; j < kClusterSize; ++j) {
                    const DevTri R = KLOAD(rec, j);
                    if (general_any(pos, dir, R, lim))
                        seeking = false;
                }
                if (!__ballot(seeking))
                    break;
            }
        }
    }
    const bool occ = want && !seeking;
    if (live && A.occluded)
        A.occluded[i] = occ ? 1 : 0;
    const unsigned long long found = __ballot(occ);
    if (A.count && found && (threadIdx.x & 63) == 0)
        atomicAdd(A.count, (unsigned long long)__popcll(found));
}
