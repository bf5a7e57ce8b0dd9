/*
 * rtc_probe.hip -- the reference's single functions on the device for known-answer tests (include/rtc.h rtc_probe_*):
 * rayTriangle (raytracing.c:186-214), raySphere (:162-184), getEnvironmentLight (:151-160), the RNG
 * (moremath.c:89-108), the soundness probe of the bounce-ray cluster culling (rtc_layout.h cluster_culled), the split
 * launch's item records, and the soundness probe of the primary cull (the primary filter and the tile prefilter).
 */
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "rtc_layout.h"
#include "rtc_internal.h"
#include "rtc_hip_util.h"

/* ---- probes: single reference functions on the device, for known-answer tests ---------------------- */
__global__ void probe_tri_kernel(const Ray *rays, const Triangle *tris, size_t n, int *didHit, float *dst)
{
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const Ray R = rays[i];
    const Triangle T = tris[i];
    const V3 A = v3(T.posA);
    float d = 0.f;
    bool h = ray_triangle(v3(R.pos), v3(R.dir), A, sub(v3(T.posB), A), sub(v3(T.posC), A), v3(T.normal), d);
    didHit[i] = h ? 1 : 0;
    dst[i] = h ? d : 0.f;
}

__global__ void probe_sphere_kernel(const Ray *rays, const Sphere *sph, size_t n, int *didHit, float *dst,
                                    vec3 *normal)
{
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const Ray R = rays[i];
    const Sphere S = sph[i];
    float d = 0.f;
    bool h = ray_sphere(v3(R.pos), v3(R.dir), v3(S.pos), S.r, d);
    didHit[i] = h ? 1 : 0;
    dst[i] = h ? d : 0.f;
    V3 nrm{0.f, 0.f, 0.f};
    if (h)
        nrm = normalized(sub(add(v3(R.pos), mul(v3(R.dir), d)), v3(S.pos)));
    normal[i] = vec3{nrm.x, nrm.y, nrm.z};
}

__global__ void probe_env_kernel(const Ray *rays, const Scene *scenes, size_t n, vec3 *out)
{
    __shared__ PowTablesLds sPow; /* the environment reads its powf tables from LDS, as in the render kernels */
    sPow.fill(threadIdx.x);
    __syncthreads();
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    Scene s = scenes[i];
    EnvParams e{};
    sPow.attach(e);
    e.sun = v3(s.normalizedSunDirection);
    e.horizon = v3(s.skyColorHorizon);
    e.zenith = v3(s.skyColorZenith);
    e.ground = v3(s.groundColor);
    e.focus = s.sunFocus;
    e.intensity = s.sunIntensity;
    e.sunSkip = env_sun_skippable(e.focus, e.intensity);
    V3 c = environment(v3(rays[i].dir), e);
    out[i] = vec3{c.x, c.y, c.z};
}

/* the sky kernel's per-pixel sun skip (rtc_device.h sun_vanishes) with the environment a launch would carry (env_of, built
 * on the host: its limit and gating, one scene for every lane as in a launch, so the wave-uniform branches of
 * environment_t are a render's): the flag, the environment evaluated with it, and the sky kernel's pixel sum of spp samples
 * of environment_miss_term (rtc_render_sky_rows: acc = acc + m * (1 / spp) from +0) */
__global__ void probe_vanish_kernel(const Ray *rays, EnvParams env, size_t n, int spp, float invSpp, int *vanish,
                                    vec3 *out, vec3 *sum)
{
    __shared__ PowTablesLds sPow;
    sPow.fill(threadIdx.x);
    __syncthreads();
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    EnvParams e = env;
    sPow.attach(e);
    const V3 d = v3(rays[i].dir);
    const bool v = sun_vanishes(d, e);
    vanish[i] = v ? 1 : 0;
    const V3 c = environment_t<false>(d, e, v);
    out[i] = vec3{c.x, c.y, c.z};
    V3 acc{0.f, 0.f, 0.f};
    for (int s = 0; s < spp; ++s)
        acc = add(acc, mul(environment_miss_term(d, e, v), invSpp));
    sum[i] = vec3{acc.x, acc.y, acc.z};
}

__global__ void probe_random_kernel(const unsigned *seeds, size_t n, int draws, float *uni, float *nrm, vec3 *dirs)
{
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    unsigned s = seeds[i];
    for (int k = 0; k < draws; ++k)
        uni[i * draws + k] = random_value(s);
    s = seeds[i];
    for (int k = 0; k < draws; ++k)
        nrm[i * draws + k] = random_normal(s);
    s = seeds[i];
    for (int k = 0; k < draws; ++k) {
        V3 d = random_direction(s);
        dirs[i * draws + k] = vec3{d.x, d.y, d.z};
    }
}

/* Cluster culling soundness (DevCluster): every (ray, cluster) pair is culled or not by cluster_culled, and
 * every triangle of the cluster is tested with the reference's rayTriangle arithmetic.  counts: [0] hits in
 * culled clusters (must stay 0), [1] clusters culled, [2] cluster tests, [3] hits, [4] float bits of the
 * largest (distance from the ball centre to the reported hit point) - r over all hits; with reach, [5] hits on
 * records judged unreachable from the ray's origin (aligned_normal; must stay 0), [6] (ray, record) pairs judged
 * so. */
__global__ void probe_cluster_kernel(const DevTri *clTris, const DevCluster *cl, int clusterCount, int per,
                                     int recCount, bool reach, const Ray *rays, size_t n,
                                     unsigned long long *counts)
{
    size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    const V3 pos = v3(rays[i].pos), dir = v3(rays[i].dir);
    const float rho = fabsf(dir.x) + fabsf(dir.y) + fabsf(dir.z);
    unsigned viol = 0, culled = 0, hits = 0, unreachHits = 0, unreach = 0;
    float excess = 0.f;
    for (int k = 0; k < clusterCount; ++k) {
        const DevCluster K = cl[k];
        const bool cut = rho <= kClusterRhoMax && cluster_culled(pos, dir, rho, dir_dd(dir), K);
        culled += cut;
        for (int j = 0; j < per && k * per + j < recCount; ++j) {
            const DevTri R = clTris[k * per + j];
            if (__float_as_int(R.pad0) < 0)
                continue;
            /* rtc_render_chain's first-bounce reach mask: not hittable from pos in any direction */
            const V3 q = cross(sub(pos, V3{R.ax, R.ay, R.az}), V3{R.abx, R.aby, R.abz});
            const bool cannot = reach && rho <= kClusterRhoMax && __float_as_int(R.pad1) != 0 &&
                                !(dot(V3{R.acx, R.acy, R.acz}, q) > 0.f);
            unreach += cannot;
            float dst;
            if (ray_triangle(pos, dir, V3{R.ax, R.ay, R.az}, V3{R.abx, R.aby, R.abz}, V3{R.acx, R.acy, R.acz},
                             V3{R.nx, R.ny, R.nz}, dst)) {
                hits++;
                viol += cut;
                unreachHits += cannot;
                const V3 h = add(pos, mul(dir, dst));
                const V3 w = sub(h, V3{K.cx, K.cy, K.cz});
                excess = fmaxf(excess, (float)__builtin_sqrt((double)dot(w, w)) - K.r);
            }
        }
    }
    atomicAdd(&counts[0], (unsigned long long)viol);
    atomicAdd(&counts[1], (unsigned long long)culled);
    atomicAdd(&counts[2], (unsigned long long)clusterCount);
    atomicAdd(&counts[3], (unsigned long long)hits);
    atomicMax(&counts[4], (unsigned long long)__float_as_uint(excess));
    if (reach) {
        atomicAdd(&counts[5], (unsigned long long)unreachHits);
        atomicAdd(&counts[6], (unsigned long long)unreach);
    }
}

namespace {
struct Scratch {
    std::vector<void *> ptrs;
    ~Scratch()
    {
        for (void *p : ptrs)
            (void)hipFree(p);
    }
    hipError_t alloc(void **p, size_t bytes)
    {
        hipError_t e = hipMalloc(p, bytes ? bytes : 16);
        if (e == hipSuccess)
            ptrs.push_back(*p);
        return e;
    }
};
int probe_prelude()
{
    int n = 0;
    return rtc_device_count(&n);
}
} // namespace

#define ALLOC_IN(dptr, hptr, bytes)                                                                    \
    HIP_TRY(sc.alloc((void **)&dptr, bytes));                                                          \
    HIP_TRY(hipMemcpy(dptr, hptr, bytes, hipMemcpyHostToDevice))
#define ALLOC_OUT(dptr, bytes) HIP_TRY(sc.alloc((void **)&dptr, bytes))

static unsigned probe_blocks(size_t n) { return (unsigned)((n + 255) / 256 > 0 ? (n + 255) / 256 : 1); }

extern "C" int rtc_probe_ray_triangle(const Ray *rays, const Triangle *tris, size_t n, int *didHit, float *dst)
{
    if (int rc = probe_prelude())
        return rc;
    if (n == 0)
        return 0;
    Scratch sc;
    Ray *dr;
    Triangle *dt;
    int *dh;
    float *dd;
    ALLOC_IN(dr, rays, n * sizeof(Ray));
    ALLOC_IN(dt, tris, n * sizeof(Triangle));
    ALLOC_OUT(dh, n * sizeof(int));
    ALLOC_OUT(dd, n * sizeof(float));
    hipLaunchKernelGGL(probe_tri_kernel, dim3(probe_blocks(n)), dim3(256), 0, nullptr, dr, dt, n, dh, dd);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(didHit, dh, n * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(dst, dd, n * sizeof(float), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int rtc_probe_ray_sphere(const Ray *rays, const Sphere *spheres, size_t n, int *didHit, float *dst,
                                    vec3 *normal)
{
    if (int rc = probe_prelude())
        return rc;
    if (n == 0)
        return 0;
    Scratch sc;
    Ray *dr;
    Sphere *ds;
    int *dh;
    float *dd;
    vec3 *dn;
    ALLOC_IN(dr, rays, n * sizeof(Ray));
    ALLOC_IN(ds, spheres, n * sizeof(Sphere));
    ALLOC_OUT(dh, n * sizeof(int));
    ALLOC_OUT(dd, n * sizeof(float));
    ALLOC_OUT(dn, n * sizeof(vec3));
    hipLaunchKernelGGL(probe_sphere_kernel, dim3(probe_blocks(n)), dim3(256), 0, nullptr, dr, ds, n, dh, dd, dn);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(didHit, dh, n * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(dst, dd, n * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(normal, dn, n * sizeof(vec3), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int rtc_probe_environment(const Ray *rays, const Scene *scenes, size_t n, vec3 *out)
{
    if (int rc = probe_prelude())
        return rc;
    if (n == 0)
        return 0;
    Scratch sc;
    Ray *dr;
    Scene *ds;
    vec3 *dout;
    ALLOC_IN(dr, rays, n * sizeof(Ray));
    ALLOC_IN(ds, scenes, n * sizeof(Scene));
    ALLOC_OUT(dout, n * sizeof(vec3));
    hipLaunchKernelGGL(probe_env_kernel, dim3(probe_blocks(n)), dim3(256), 0, nullptr, dr, ds, n, dout);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, dout, n * sizeof(vec3), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int rtc_probe_sun_vanish(const Ray *rays, const Scene *scene, size_t n, int spp, int *vanish, vec3 *out,
                                    vec3 *sum)
{
    if (!scene || spp < 0 || (n > 0 && (!rays || !vanish || !out || !sum)))
        return rtc_fail(RTC_EINVAL, "rtc_probe_sun_vanish: bad argument");
    if (int rc = probe_prelude())
        return rc;
    if (n == 0)
        return 0;
    Scratch sc;
    Ray *dr;
    int *dv;
    vec3 *dout, *dsum;
    ALLOC_IN(dr, rays, n * sizeof(Ray));
    ALLOC_OUT(dv, n * sizeof(int));
    ALLOC_OUT(dout, n * sizeof(vec3));
    ALLOC_OUT(dsum, n * sizeof(vec3));
    const float invSpp = spp > 0 ? (float)(1. / (double)spp) : 0.f; /* as a launch's (render_params) */
    hipLaunchKernelGGL(probe_vanish_kernel, dim3(probe_blocks(n)), dim3(256), 0, nullptr, dr, env_of(*scene), n, spp,
                       invSpp, dv, dout, dsum);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(vanish, dv, n * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out, dout, n * sizeof(vec3), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(sum, dsum, n * sizeof(vec3), hipMemcpyDeviceToHost));
    return 0;
}

/* the limit sun_vanishes compares with in a launch of this scene (host code: no device needed) */
extern "C" int rtc_env_vanish_limit(const Scene *scene, double *limit)
{
    if (!scene || !limit)
        return RTC_EINVAL;
    *limit = env_of(*scene).vanishLim;
    return 0;
}

extern "C" int rtc_probe_random(const unsigned int *seeds, size_t n, int draws, float *uniform, float *normal,
                                vec3 *direction)
{
    if (int rc = probe_prelude())
        return rc;
    if (n == 0 || draws <= 0)
        return 0;
    Scratch sc;
    unsigned *dsd;
    float *du, *dn;
    vec3 *dd;
    const size_t m = n * (size_t)draws;
    ALLOC_IN(dsd, seeds, n * sizeof(unsigned));
    ALLOC_OUT(du, m * sizeof(float));
    ALLOC_OUT(dn, m * sizeof(float));
    ALLOC_OUT(dd, m * sizeof(vec3));
    hipLaunchKernelGGL(probe_random_kernel, dim3(probe_blocks(n)), dim3(256), 0, nullptr, dsd, n, draws, du, dn, dd);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(uniform, du, m * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(normal, dn, m * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(direction, dd, m * sizeof(vec3), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int rtc_probe_cluster_bound(const Triangle *tris, int triCount, const Ray *rays, size_t n,
                                       unsigned long long counts[7])
{
    if (!counts || triCount < 0 || (triCount > 0 && !tris) || (n > 0 && !rays))
        return rtc_fail(RTC_EINVAL, "rtc_probe_cluster_bound: bad argument");
    memset(counts, 0, 7 * sizeof(unsigned long long));
    if (int rc = probe_prelude())
        return rc;
    if (n == 0 || triCount == 0)
        return 0;
    RtcDeviceScene *s = nullptr;
    if (int rc = rtc_scene_upload(tris, triCount, nullptr, 0, -1, &s))
        return rc;
    Scratch sc;
    Ray *dr = nullptr;
    unsigned long long *dc = nullptr;
    int rc = 0;
    hipError_t e = sc.alloc((void **)&dr, n * sizeof(Ray));
    if (e == hipSuccess)
        e = hipMemcpy(dr, rays, n * sizeof(Ray), hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = sc.alloc((void **)&dc, 7 * sizeof(unsigned long long));
    if (e == hipSuccess)
        e = hipMemset(dc, 0, 7 * sizeof(unsigned long long));
    if (e == hipSuccess) {
        /* the clusters, then the chunks (balls over kChunkClusters clusters, rtc_render_chain's first level) */
        const SceneRecords &g = s->current();
        hipLaunchKernelGGL(probe_cluster_kernel, dim3(probe_blocks(n)), dim3(256), 0, nullptr, g.clTris, g.clusters,
                           s->clusterCount, kClusterSize, s->clusterCount * kClusterSize, true, dr, n, dc);
        e = hipGetLastError();
        if (e == hipSuccess && s->chunkCount > 1) {
            hipLaunchKernelGGL(probe_cluster_kernel, dim3(probe_blocks(n)), dim3(256), 0, nullptr, g.clTris, g.chunks,
                               s->chunkCount, kClusterSize * kChunkClusters, s->clusterCount * kClusterSize, false, dr, n,
                               dc);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess)
        e = hipMemcpy(counts, dc, 7 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    if (e != hipSuccess)
        rc = rtc_fail(-(int)e, "rtc_probe_cluster_bound: %s", hipGetErrorString(e));
    rtc_scene_release(s);
    return rc;
}

/* The split launch's item records (rtc_params.h item_record): uploads the scene, runs the preparation and culls of the
 * launch `d` (rtc_cull_items) and copies back the sub-lists' counts, the records (the sub-lists one after the other) and
 * the tiles' pixel masks */
extern "C" int rtc_probe_item_records(const Triangle *tris, int triCount, const Sphere *spheres, int sphereCount,
                                      const Scene *scene, const RtcCamera *cam, const RtcRenderDesc *d, int counts[16],
                                      int info[4], unsigned *records, size_t maxRecords, unsigned long long *pixMask,
                                      size_t maxTiles)
{
    static_assert(kGeoLists == 16, "counts[16]: one per sub-list");
    if (!scene || !cam || !d || !counts || !info || !records || !pixMask || triCount < 0 || sphereCount < 0)
        return rtc_fail(RTC_EINVAL, "rtc_probe_item_records: bad argument");
    if (int rc = probe_prelude())
        return rc;
    RtcDeviceScene *s = nullptr;
    if (int rc = rtc_scene_upload(tris, triCount, spheres, sphereCount, -1, &s))
        return rc;
    Scratch sc;
    int rc = 0;
    const auto run = [&]() -> int {
        unsigned char *dColors = nullptr; /* (the launch's key; no kernel of the probe's writes it) */
        HIP_TRY(sc.alloc((void **)&dColors, (size_t)d->width * (size_t)(rtc_rows_selected(d) > 0 ? rtc_rows_selected(d) : 1) * 3));
        RtcCullItems it{};
        if (const int r = rtc_cull_items(s, scene, cam, d, dColors, &it))
            return r;
        HIP_TRY(hipDeviceSynchronize());
        int raw[kGeoSetInts];
        HIP_TRY(hipMemcpy(raw, it.geoCount, sizeof raw, hipMemcpyDeviceToHost));
        size_t total = 0;
        for (int l = 0; l < kGeoLists; ++l) {
            counts[l] = raw[l * kGeoCountStride] < it.geoCap ? raw[l * kGeoCountStride] : it.geoCap;
            total += (size_t)counts[l];
        }
        info[0] = it.geoCap, info[1] = it.tilesX, info[2] = (int)it.tiles, info[3] = it.wide;
        if (total > maxRecords || it.tiles > maxTiles)
            return rtc_fail(RTC_EINVAL, "rtc_probe_item_records: %zu records, %zu tiles: the outputs are smaller", total,
                            it.tiles);
        size_t at = 0;
        for (int l = 0; l < kGeoLists; ++l) {
            HIP_TRY(hipMemcpy(records + at * kItemRecDwords, it.geoList + (size_t)l * it.geoCap * kItemRecDwords,
                              (size_t)counts[l] * kItemRecDwords * 4, hipMemcpyDeviceToHost));
            at += (size_t)counts[l];
        }
        HIP_TRY(hipMemcpy(pixMask, it.pixMask, it.tiles * 8, hipMemcpyDeviceToHost));
        return 0;
    };
    rc = run();
    rtc_scene_release(s);
    return rc;
}

/* The primary filter's verdict for every (pixel of the launch, triangle): !prim_backfacing && prim_pass (rtc_layout.h, the
 * render kernels' own functions) on the launch's DevPrimF records and the pixel's primary_dir.  One thread per pixel
 * (launch row r, column x: pixel r * width + x); kept[pixel * triCount + t]. */
__global__ void probe_primary_kernel(PrimaryView V, int rows, const DevPrimF *primF, int triCount, unsigned char *kept)
{
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= (size_t)rows * (size_t)V.width)
        return;
    const int x = (int)(i % (size_t)V.width), r = (int)(i / (size_t)V.width);
    const V3 dir = primary_dir(V, x, launch_row_y(V, r));
    for (int t = 0; t < triCount; ++t) {
        const DevPrimF F = primF[t];
        kept[i * (size_t)triCount + t] = !prim_backfacing(dir, F) && prim_pass(dir, F) ? 1 : 0;
    }
}

/* The tile prefilter per 8x8 tile (level 2 of rtc_tile_cull: tile_cone / tile_prunes, rtc_layout.h): one thread per tile;
 * cones[tile * 4 ..] = {eDir, vmin, vmax, ok}, pruned[tile * triCount + t] = the cone is usable and prunes record t */
__global__ void probe_cone_kernel(PrimaryView V, int tilesX, int tiles, const DevPrimF *primF, int triCount, double *cones,
                                  unsigned char *pruned)
{
    const int tile = blockIdx.x * blockDim.x + threadIdx.x;
    if (tile >= tiles)
        return;
    const TileCone K = tile_cone(V, tile % tilesX, tile / tilesX);
    cones[tile * 4 + 0] = K.eDir, cones[tile * 4 + 1] = K.vmin, cones[tile * 4 + 2] = K.vmax, cones[tile * 4 + 3] = K.ok ? 1.0 : 0.0;
    for (int t = 0; t < triCount; ++t)
        pruned[(size_t)tile * (size_t)triCount + t] = K.ok && tile_prunes(K, primF[t]) ? 1 : 0;
}

/* Soundness probe of the primary cull (include/rtc.h): the launch's own preparation and culls (rtc_cull_items), then the
 * per-pixel verdicts by probe_primary_kernel; the tiles' bit-sets and pixel masks are the launch's */
extern "C" int rtc_probe_primary_cull(const Triangle *tris, int triCount, const Scene *scene, const RtcCamera *cam,
                                      const RtcRenderDesc *d, unsigned char *kept, size_t maxKept,
                                      unsigned long long *tileBits, size_t maxWords, unsigned long long *pixMask,
                                      size_t maxTiles, int info[4], float *primF, double *cones, unsigned char *pruned)
{
    if (!tris || triCount <= 0 || !scene || !cam || !d || !kept || !tileBits || !pixMask || !info)
        return rtc_fail(RTC_EINVAL, "rtc_probe_primary_cull: bad argument");
    if (int rc = probe_prelude())
        return rc;
    RtcDeviceScene *s = nullptr;
    if (int rc = rtc_scene_upload(tris, triCount, nullptr, 0, -1, &s))
        return rc;
    Scratch sc;
    const auto run = [&]() -> int {
        const int rows = rtc_rows_selected(d);
        if (rows <= 0)
            return rtc_fail(RTC_EINVAL, "rtc_probe_primary_cull: the launch has no rows");
        unsigned char *dColors = nullptr; /* (the launch's key; no kernel of the probe's writes it) */
        HIP_TRY(sc.alloc((void **)&dColors, (size_t)d->width * (size_t)rows * 3));
        RtcCullItems it{};
        if (const int r = rtc_cull_items(s, scene, cam, d, dColors, &it))
            return r;
        HIP_TRY(hipDeviceSynchronize());
        const size_t pixels = (size_t)rows * (size_t)d->width, words = it.tiles * (size_t)it.maskWords;
        info[0] = (int)it.tiles, info[1] = it.tilesX, info[2] = it.maskWords, info[3] = it.level0;
        if (pixels * (size_t)triCount > maxKept || words > maxWords || it.tiles > maxTiles || triCount > it.triPadded)
            return rtc_fail(RTC_EINVAL, "rtc_probe_primary_cull: %zu verdicts, %zu words, %zu tiles: the outputs are smaller",
                            pixels * (size_t)triCount, words, it.tiles);
        unsigned char *dk = nullptr;
        HIP_TRY(sc.alloc((void **)&dk, pixels * (size_t)triCount));
        PrimaryView V{};
        V.width = d->width, V.height = d->height, V.rows = rows, V.rowStart = d->rowStart, V.rowStride = d->rowStride;
        V.rowBandShift = d->rowBand > 1 ? __builtin_ctz((unsigned)d->rowBand) : 0; /* as render_params */
        V.ex = v3(cam->ex), V.ey = v3(cam->ey), V.ez = v3(cam->ez), V.fov = cam->fov;
        hipLaunchKernelGGL(probe_primary_kernel, dim3(probe_blocks(pixels)), dim3(256), 0, nullptr, V, rows, it.primF,
                           triCount, dk);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(kept, dk, pixels * (size_t)triCount, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(pixMask, it.pixMask, it.tiles * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(tileBits, it.tileMask, words * 8, hipMemcpyDeviceToHost));
        if (primF) /* the launch's filter records, 16 floats each (DevPrimF) */
            HIP_TRY(hipMemcpy(primF, it.primF, (size_t)triCount * sizeof(DevPrimF), hipMemcpyDeviceToHost));
        if (cones && pruned) { /* (sized by the caller from info's tiles: maxTiles tiles) */
            double *dc = nullptr;
            unsigned char *dp = nullptr;
            HIP_TRY(sc.alloc((void **)&dc, it.tiles * 4 * sizeof(double)));
            HIP_TRY(sc.alloc((void **)&dp, it.tiles * (size_t)triCount));
            hipLaunchKernelGGL(probe_cone_kernel, dim3(probe_blocks(it.tiles)), dim3(256), 0, nullptr, V, it.tilesX,
                               (int)it.tiles, it.primF, triCount, dc, dp);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpy(cones, dc, it.tiles * 4 * sizeof(double), hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(pruned, dp, it.tiles * (size_t)triCount, hipMemcpyDeviceToHost));
        }
        /* a split launch writes no words for the tiles of a workgroup without a survivor (rtc_tile_cull): their lists
         * are empty, which their pixMask says */
        for (size_t t = 0; t < it.tiles; ++t)
            if (pixMask[t] == 0ull)
                memset(tileBits + t * (size_t)it.maskWords, 0, (size_t)it.maskWords * 8);
        return 0;
    };
    const int rc = run();
    rtc_scene_release(s);
    return rc;
}
