/*
 * rtc_scene.hip -- the scene on the device (rtc_scene_upload / rtc_scene_release, include/rtc.h): the reference's
 * Triangle[] (objloader.c / main.c:229-243) packed into the HBM records of rtc_layout.h, grouped into clusters and chunks
 * for the bounce rays' culling, the scheduling hint bounce_hit_share, the scene's streams and ordering events, and the
 * per-scene hooks (frame / geometry events, kernel timing); and the same records rewritten in place for new primitives
 * by a kernel (rtc_scene_update_async, rtc_refit), after the clusters were decided anew on the device where
 * asked (rtc_scene_regroup_async, the rtc_regroup_* kernels).  The records' arithmetic (packing, aligned
 * normals, balls and margins) is rtc_records.h's and the membership's is rtc_regroup.h's, each stated once: here are the
 * host's loops and the device's kernels over them, and the six record arrays are walked by rtc_layout.h's table.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rtc_layout.h"
#include "rtc_internal.h"
#include "rtc_hip_util.h"
#include "rtc_records.h"
#include "rtc_regroup.h"
#include "rtc_staged.h"

/* The share of diffuse bounce rays that hit the scene again, estimated at upload (host, a fixed-seed probe): rays from
 * area-weighted random points of the triangles, in directions normal + a random unit vector (the reference's diffuse
 * lobe, raytracing.c:276-279, without the specular part), tested against every triangle in double precision with the
 * reference's backface rule.  Only a scheduling hint (rtc_render_chain's workgroups per CU): it never changes a
 * frame.  Measured shares: fsuzane 0.21, rsuzanne 0.11, ultracomplex 0.019, complex 0.016, cube 0.
 * With spheres (ns > 0: hitShareAll, the sphere split's gate, rtcplan::kSplitMaxHitShare) the origins are drawn from the
 * triangles and the spheres together, area-weighted (a sphere's area is 4 pi r^2; a sphere's bounce rays leave along its
 * outward normal, raytracing.c:182), and every ray is tested against the spheres too (raySphere, raytracing.c:162-184, in
 * double).  Without spheres the draws and tests are the triangle-only probe's, value for value. */
static double bounce_hit_share(const Triangle *t, int n, const Sphere *sp = nullptr, int ns = 0)
{
    if (n < 0)
        n = 0;
    if (ns < 0 || !sp)
        ns = 0;
    if (n + ns <= 0)
        return 0.0;
    struct D3 { double x, y, z; };
    const auto sub3 = [](D3 a, D3 b) { return D3{a.x - b.x, a.y - b.y, a.z - b.z}; };
    const auto dot3 = [](D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; };
    const auto cross3 = [](D3 a, D3 b) { return D3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; };
    const auto d3 = [](vec3 v) { return D3{v.x, v.y, v.z}; };
    const int prims = n + ns;
    std::vector<double> cdf((size_t)prims);
    double total = 0.0;
    for (int i = 0; i < n; ++i) {
        const D3 c = cross3(sub3(d3(t[i].posB), d3(t[i].posA)), sub3(d3(t[i].posC), d3(t[i].posA)));
        total += 0.5 * std::sqrt(dot3(c, c));
        cdf[(size_t)i] = total;
    }
    for (int i = 0; i < ns; ++i) {
        const double r = sp[i].r;
        if (r == r && std::isfinite(r))
            total += 4.0 * 3.14159265358979323846 * r * r;
        cdf[(size_t)(n + i)] = total;
    }
    if (!(total > 0.0) || !std::isfinite(total))
        return 0.0;
    unsigned long long st = 0x9E3779B97F4A7C15ull;
    const auto uni = [&]() { /* xorshift64*, [0, 1) */
        st ^= st >> 12;
        st ^= st << 25;
        st ^= st >> 27;
        return (double)((st * 0x2545F4914F6CDD1Dull) >> 11) * (1.0 / 9007199254740992.0);
    };
    const auto unit = [&](D3 &q) { /* a uniform random unit vector (rejection from the cube) */
        double ql = 0.0;
        do {
            q = D3{2 * uni() - 1, 2 * uni() - 1, 2 * uni() - 1};
            ql = dot3(q, q);
        } while (ql > 1.0 || ql < 1e-12);
        ql = std::sqrt(ql);
        q = D3{q.x / ql, q.y / ql, q.z / ql};
    };
    /* rays x n ray-triangle tests: ~4 M up to 62.5 k triangles, 64 n beyond (a 1 M-triangle scene: 64 M tests, a few
     * tenths of a second of upload; scenes past the tile cull's limit skip the probe, rtc_scene_upload) */
    const int rays = (int)std::min<long long>(2048, std::max<long long>(64, 4000000LL / prims));
    int hits = 0;
    for (int r = 0; r < rays; ++r) {
        const int i = std::min((int)(std::lower_bound(cdf.begin(), cdf.end(), uni() * total) - cdf.begin()), prims - 1);
        D3 nn{0, 0, 0}, O{0, 0, 0}; /* the origin's unit normal, and the point of the surface */
        if (i < n) {
            const Triangle &T = t[i];
            double u = uni(), w = uni();
            if (u + w > 1.0) {
                u = 1.0 - u;
                w = 1.0 - w;
            }
            const D3 A = d3(T.posA), AB = sub3(d3(T.posB), A), AC = sub3(d3(T.posC), A);
            nn = d3(T.normal);
            const double nl = std::sqrt(dot3(nn, nn));
            if (!(nl > 0.0))
                continue;
            nn = D3{nn.x / nl, nn.y / nl, nn.z / nl};
            O = D3{A.x + u * AB.x + w * AC.x, A.y + u * AB.y + w * AC.y, A.z + u * AB.z + w * AC.z};
        } else { /* a uniform point of the sphere; its normal points outwards */
            const Sphere &S = sp[i - n];
            unit(nn);
            O = D3{S.pos.x + S.r * nn.x, S.pos.y + S.r * nn.y, S.pos.z + S.r * nn.z};
        }
        D3 q{0, 0, 0};
        unit(q);
        D3 dir{nn.x + q.x, nn.y + q.y, nn.z + q.z};
        const double dl = std::sqrt(dot3(dir, dir));
        if (!(dl > 1e-9))
            continue;
        dir = D3{dir.x / dl, dir.y / dl, dir.z / dl};
        const D3 P{O.x + 1e-4 * nn.x, O.y + 1e-4 * nn.y, O.z + 1e-4 * nn.z};
        bool hit = false;
        for (int j = 0; j < ns && !hit; ++j) { /* raySphere's tests (raytracing.c:162-184), in double */
            const D3 off = sub3(P, d3(sp[j].pos));
            const double b = dot3(off, dir), cc = dot3(off, off) - (double)sp[j].r * (double)sp[j].r;
            double delta = b * b - cc;
            if (!(delta >= 0.0))
                continue;
            delta = std::sqrt(delta);
            double dst = -b - delta;
            if (dst < 1e-3)
                dst = -b + delta;
            hit = dst >= 1e-3;
        }
        for (int j = 0; j < n && !hit; ++j) { /* rayTriangle's tests (raytracing.c:186-214), in double */
            if (dot3(dir, d3(t[j].normal)) >= 0.0)
                continue;
            const D3 a = d3(t[j].posA), ab = sub3(d3(t[j].posB), a), ac = sub3(d3(t[j].posC), a);
            const D3 h = cross3(dir, ac);
            const double det = dot3(ab, h);
            if (std::fabs(det) < 1e-12)
                continue;
            const D3 sv = sub3(P, a);
            const double uu = dot3(sv, h) / det;
            if (uu < 0.0 || uu > 1.0)
                continue;
            const D3 qv = cross3(sv, ab);
            const double vv = dot3(dir, qv) / det;
            if (vv < 0.0 || uu + vv > 1.0 || dot3(ac, qv) / det < 1e-3)
                continue;
            hit = true;
        }
        hits += hit ? 1 : 0;
    }
    return (double)hits / (double)rays;
}

static void pack_scene(const Triangle *tris, int triCount, const Sphere *sph, int sphCount, std::vector<DevTri> &dt,
                       std::vector<DevMat> &dm, std::vector<DevSphere> &ds)
{
    const size_t padded = ((size_t)(triCount > 0 ? triCount : 0) + 7) / 8 * 8 + 8;
    /* zero records are never hit: N = 0 makes dot(dir, N) >= 0 (or NaN, and then det is NaN too) */
    dt.assign(padded, DevTri{});
    dm.assign(padded, DevMat{});
    for (int i = 0; i < triCount; ++i) {
        const float *p = reinterpret_cast<const float *>(tris + i);
        dt[i] = pack_tri(p);
        dm[i] = pack_mat(p);
    }
    ds.resize(sphCount > 0 ? sphCount : 1);
    for (int i = 0; i < sphCount; ++i)
        ds[i] = pack_sphere(reinterpret_cast<const float *>(sph + i));
}

/* Clusters of kClusterSize triangles: recursive splits of the centroids along their longest extent, each
 * split at a multiple of kClusterSize so that every leaf but the last is full (ceil(n / 8) clusters).  The definition of
 * the membership; its centroid, extent, axis, key and split point are rtc_regroup.h's, which the device's levels share. */
static_assert(kRegroupLeaf == kClusterSize, "a leaf of the split is a cluster");
static void split_clusters(const std::vector<DevTri> &dt, std::vector<int> &idx, size_t lo, size_t hi)
{
    if (hi - lo <= (size_t)kClusterSize)
        return;
    const auto centroid = [&](int i, int a) {
        const float *f = &dt[i].ax; /* ax, ay, az, abx, aby, abz, acx, acy, acz */
        return regroup_centroid(f[a], f[3 + a], f[6 + a]);
    };
    RegroupExtent e[3] = {regroup_extent_init(), regroup_extent_init(), regroup_extent_init()};
    for (size_t k = lo; k < hi; ++k)
        for (int a = 0; a < 3; ++a)
            regroup_extent_take(e[a], centroid(idx[k], a));
    const int axis = regroup_axis(e);
    std::stable_sort(idx.begin() + lo, idx.begin() + hi,
                     [&](int p, int q) { return regroup_key(centroid(p, axis)) < regroup_key(centroid(q, axis)); });
    const size_t mid = (size_t)regroup_mid((int)lo, (int)hi);
    split_clusters(dt, idx, lo, mid);
    split_clusters(dt, idx, mid, hi);
}

/* Bounding ball and cull margins (DevCluster) of the records ct[first, first + count) whose index (pad0) is >= 0, taken
 * in sequence (rtc_records.h: the order decides the sign of a zero centre). */
static DevCluster ball_of(const std::vector<DevTri> &ct, size_t first, size_t count)
{
    const auto real = [](const DevTri &r) {
        int i;
        memcpy(&i, &r.pad0, sizeof i);
        return i >= 0;
    };
    BallAcc b;
    acc_init(b);
    for (size_t j = first; j < first + count; ++j)
        if (real(ct[j]))
            acc_record(b, ct[j]);
    float c[3];
    ball_centre(b, c);
    double R = 0.0;
    for (size_t j = first; j < first + count; ++j)
        if (real(ct[j]))
            R = std::max(R, rec_radius(ct[j], c));
    return ball_finish(b, c, R);
}

/* The cluster membership: idx[k] = the reference index of clustered record k (idx holds triCount entries; the last
 * cluster's missing records are padding).  Decided at upload; an update keeps it (rtc_scene_update_async), a regroup
 * decides it again on the device by regroup_membership's formulation (rtc_scene_regroup_async). */
static void rtc_cluster_membership(const std::vector<DevTri> &dt, int triCount, std::vector<int> &idx)
{
    idx.resize(triCount > 0 ? triCount : 0);
    for (int i = 0; i < triCount; ++i)
        idx[i] = i;
    split_clusters(dt, idx, 0, (size_t)triCount);
}

/* The same membership by the level-by-level rank count the device runs (rtc_regroup.h), in plain C++ and in
 * the kernels' own structure: per level, every sorting segment by its path -- the axis from its extents, each element to
 * its rank --, then every position no segment of the level sorts copied across.  rtc_cluster_membership stays the
 * definition; tests/test_regroup_host.py holds the two equal. */
static void regroup_membership(const std::vector<DevTri> &dt, int n, std::vector<int> &idx)
{
    std::vector<double> cent[3];
    for (int a = 0; a < 3; ++a)
        cent[a].resize((size_t)(n > 0 ? n : 0));
    std::vector<int> buf[2];
    buf[0].resize(cent[0].size()), buf[1].resize(cent[0].size());
    for (int i = 0; i < n; ++i) { /* rtc_regroup_centroids */
        const DevTri &t = dt[i];
        cent[0][i] = regroup_centroid(t.ax, t.abx, t.acx);
        cent[1][i] = regroup_centroid(t.ay, t.aby, t.acy);
        cent[2][i] = regroup_centroid(t.az, t.abz, t.acz);
        buf[0][i] = i;
    }
    const int levels = regroup_levels(n);
    for (int level = 0; level < levels; ++level) { /* rtc_regroup_level */
        const std::vector<int> &in = buf[level & 1];
        std::vector<int> &out = buf[(level & 1) ^ 1];
        for (unsigned path = 0; path < 1u << level; ++path) {
            int lo, hi;
            if (!regroup_segment_of_path(n, level, path, lo, hi))
                continue;
            RegroupExtent e[3] = {regroup_extent_init(), regroup_extent_init(), regroup_extent_init()};
            for (int q = lo; q < hi; ++q)
                for (int a = 0; a < 3; ++a)
                    regroup_extent_take(e[a], cent[a][in[q]]);
            const std::vector<double> &c = cent[regroup_axis(e)];
            for (int p = lo; p < hi; ++p) {
                const double kp = regroup_key(c[in[p]]);
                int rank = 0;
                for (int q = lo; q < hi; ++q)
                    rank += regroup_rank(regroup_key(c[in[q]]), q, kp, p);
                out[lo + rank] = in[p];
            }
        }
        for (int p = 0; p < n; ++p) {
            int lo, hi;
            if (!regroup_segment_of_position(n, level, p, lo, hi))
                out[p] = in[p];
        }
    }
    idx = buf[levels & 1];
}

extern "C" int rtc_regroup_membership_host(const Triangle *tris, int triCount, int *idx)
{
    if (triCount < 0 || (triCount > 0 && (!tris || !idx)))
        return rtc_fail(RTC_EINVAL, "rtc_regroup_membership_host: bad argument");
    std::vector<DevTri> dt;
    std::vector<DevMat> dm;
    std::vector<DevSphere> ds;
    pack_scene(tris, triCount, nullptr, 0, dt, dm, ds);
    std::vector<int> m;
    regroup_membership(dt, triCount, m);
    std::copy(m.begin(), m.end(), idx);
    return 0;
}

/* The one host statement of the clustered records for a membership `idx` (rtc_cluster_membership): upload builds them
 * from the membership it has just decided, a refit (rtc_scene_records_host with new triangles; on the device rtc_refit,
 * from the same functions of rtc_records.h) from the upload's membership and the new packed records dt. */
static void rtc_cluster_records(const std::vector<DevTri> &dt, int triCount, const std::vector<int> &idx,
                                std::vector<DevTri> &ct, std::vector<DevCluster> &cl, std::vector<DevCluster> &ch)
{
    const int nc = (triCount + kClusterSize - 1) / kClusterSize;
    ct.assign((size_t)nc * kClusterSize, DevTri{});
    cl.assign((size_t)(nc > 0 ? nc : 1), DevCluster{});
    for (int c = 0; c < nc; ++c) {
        const int n = std::min(kClusterSize, triCount - c * kClusterSize);
        for (int j = 0; j < kClusterSize; ++j) {
            DevTri &r = ct[(size_t)c * kClusterSize + j];
            if (j >= n) { /* zero record: never hit; index -1 */
                const int none = -1;
                memcpy(&r.pad0, &none, sizeof none);
                continue;
            }
            const int i = idx[(size_t)c * kClusterSize + j];
            r = dt[i];
            memcpy(&r.pad0, &i, sizeof i);
            const int al = aligned_normal(r) ? 1 : 0;
            memcpy(&r.pad1, &al, sizeof al);
        }
        cl[c] = ball_of(ct, (size_t)c * kClusterSize, kClusterSize);
    }
    const int nch = (nc + kChunkClusters - 1) / kChunkClusters;
    ch.assign((size_t)(nch > 0 ? nch : 1), DevCluster{});
    for (int h = 0; h < nch; ++h) {
        const size_t c0 = (size_t)h * kChunkClusters, c1 = std::min<size_t>((size_t)nc, c0 + kChunkClusters);
        ch[h] = ball_of(ct, c0 * kClusterSize, (c1 - c0) * kClusterSize);
    }
}

/* Every record of a scene on the host: dt / dm / ds in reference order (pack_scene); ct: the records in cluster order
 * (pad0 = reference index, -1 for padding), cl: one ball per cluster of kClusterSize, ch: one ball per chunk of
 * kChunkClusters consecutive clusters (a subtree of the median split: the chain kernel's first culling level for scenes
 * of more than one chunk); idx: the membership.  With `refit` the membership in R.idx is kept (an update) and only the
 * records are rebuilt; without it the membership is decided from these triangles (an upload). */
struct HostRecords {
    std::vector<DevTri> dt, ct;
    std::vector<DevMat> dm;
    std::vector<DevSphere> ds;
    std::vector<DevCluster> cl, ch;
    std::vector<int> idx;
    /* the six record arrays in kSceneArrays' order: where each lies and its bytes */
    void arrays(const void *data[kSceneArrayCount], size_t bytes[kSceneArrayCount]) const
    {
        const void *const d[kSceneArrayCount] = {dt.data(), dm.data(), ds.data(), ct.data(), cl.data(), ch.data()};
        const size_t n[kSceneArrayCount] = {dt.size(), dm.size(), ds.size(), ct.size(), cl.size(), ch.size()};
        for (int k = 0; k < kSceneArrayCount; ++k)
            data[k] = d[k], bytes[k] = n[k] * kSceneArrays[k].elem;
    }
};
static void host_records(const Triangle *tris, int triCount, const Sphere *spheres, int sphereCount, bool refit,
                         HostRecords &R)
{
    pack_scene(tris, triCount, spheres, sphereCount, R.dt, R.dm, R.ds);
    if (!refit)
        rtc_cluster_membership(R.dt, triCount, R.idx);
    rtc_cluster_records(R.dt, triCount, R.idx, R.ct, R.cl, R.ch);
    if (R.ct.empty())
        R.ct.assign(1, DevTri{});
}

/* ---- the refit on the device (rtc_scene_update_async) ---------------------------------------------------------------
 * rtc_refit writes one generation of scene records from the caller's Triangle[] / Sphere[] in device memory: what
 * pack_scene and rtc_cluster_records produce for the upload's membership (clIndex), byte for byte.  One workgroup per
 * chunk, one lane per clustered record: the lane packs its triangle (tris / mats in reference order, clTris in cluster
 * order with the aligned-normal flag), its cluster's ball comes from reductions over the aligned group of 8 lanes, the
 * chunk's from those through LDS.  The packing, the aligned-normal flag and the ball are rtc_records.h's functions, the ones
 * the host's loops run; the partial extents merged here hold no NaN and the merges keep the lower lane's and the lower
 * cluster's value where two are equal, the one the host's sequence keeps.  A kind of primitive the caller leaves out is
 * copied from the current generation. */
struct RefitArgs {
    const Triangle *srcTris;  /* null: copy the triangles' records of `from` */
    const Sphere *srcSpheres; /* null: copy from's spheres */
    SceneRecords from, to;
    const int *clIndex;
    int clusterCount, sphereCount;
    size_t n16[kSceneArrayCount]; /* 16-byte words of each array (rtc_layout.h kSceneArrays) */
};

__device__ __forceinline__ BallAcc acc_shfl_xor(const BallAcc &b, int mask)
{
    BallAcc o;
    for (int a = 0; a < 3; ++a) {
        o.lo[a] = __shfl_xor(b.lo[a], mask, kClusterSize);
        o.hi[a] = __shfl_xor(b.hi[a], mask, kClusterSize);
    }
    o.E = __shfl_xor(b.E, mask, kClusterSize);
    o.finite = __shfl_xor(b.finite, mask, kClusterSize);
    o.n = __shfl_xor(b.n, mask, kClusterSize);
    return o;
}

__device__ __forceinline__ void copy16(void *dst, const void *src, size_t n16, size_t first, size_t stride)
{
    for (size_t k = first; k < n16; k += stride)
        ((uint4 *)dst)[k] = ((const uint4 *)src)[k];
}

constexpr int kRefitBlock = kChunkClusters * kClusterSize; /* one lane per clustered record of a chunk */
static_assert(kRefitBlock == 256 && kClusterSize == 8, "rtc_refit: a workgroup per chunk, 8-lane cluster reductions");

__global__ __launch_bounds__(kRefitBlock) void rtc_refit(RefitArgs a)
{
    const int tid = (int)threadIdx.x, h = (int)blockIdx.x;
    const size_t gt = (size_t)h * kRefitBlock + tid, gstride = (size_t)gridDim.x * kRefitBlock;
    if (a.srcSpheres) { /* pack_scene's sphere loop */
        for (size_t i = gt; i < (size_t)a.sphereCount; i += gstride)
            a.to.spheres[i] = pack_sphere(reinterpret_cast<const float *>(a.srcSpheres) + 9 * i);
    } else {
        copy16(a.to.spheres, a.from.spheres, a.n16[kArrSpheres], gt, gstride);
    }
    if (!a.srcTris) { /* (the same for every lane of the grid) */
        copy16(a.to.tris, a.from.tris, a.n16[kArrTris], gt, gstride);
        copy16(a.to.mats, a.from.mats, a.n16[kArrMats], gt, gstride);
        copy16(a.to.clTris, a.from.clTris, a.n16[kArrClTris], gt, gstride);
        copy16(a.to.clusters, a.from.clusters, a.n16[kArrClusters], gt, gstride);
        copy16(a.to.chunks, a.from.chunks, a.n16[kArrChunks], gt, gstride);
        return;
    }
    __shared__ BallAcc sAcc[kChunkClusters];
    __shared__ double sR[kChunkClusters];
    const size_t slot = gt, slots = (size_t)a.clusterCount * kClusterSize;
    const bool valid = slot < slots;
    const int i = valid ? a.clIndex[slot] : -1;
    DevTri r{};
    if (i >= 0) {
        const float *p = reinterpret_cast<const float *>(a.srcTris) + 17 * (size_t)i;
        r = pack_tri(p);
        a.to.tris[i] = r;
        a.to.mats[i] = pack_mat(p);
        r.pad0 = __int_as_float(i);
        r.pad1 = __int_as_float(aligned_normal(r) ? 1 : 0);
    } else {
        r.pad0 = __int_as_float(-1); /* zero record: never hit */
    }
    if (valid)
        a.to.clTris[slot] = r;
    /* the cluster: the aligned group of 8 lanes */
    BallAcc b;
    acc_init(b);
    if (i >= 0)
        acc_record(b, r);
    for (int m = 1; m < kClusterSize; m <<= 1)
        acc_merge(b, acc_shfl_xor(b, m));
    float c[3];
    ball_centre(b, c);
    double R = i >= 0 ? rec_radius(r, c) : 0.0;
    for (int m = 1; m < kClusterSize; m <<= 1) {
        const double o = __shfl_xor(R, m, kClusterSize);
        R = R < o ? o : R;
    }
    const int cl = tid / kClusterSize;
    if (tid % kClusterSize == 0) {
        if (slot < slots)
            a.to.clusters[slot / kClusterSize] = ball_finish(b, c, R);
        sAcc[cl] = b;
    }
    __syncthreads();
    /* the chunk: its clusters' extents (a cluster past the scene's last one is empty), then the radius about its centre */
    BallAcc cb = sAcc[0];
#pragma unroll 1 /* (unrolled, the 32 extents are all loaded first: 500 registers) */
    for (int k = 1; k < kChunkClusters; ++k)
        acc_merge(cb, sAcc[k]);
    float cc[3];
    ball_centre(cb, cc);
    double Rc = i >= 0 ? rec_radius(r, cc) : 0.0;
    for (int m = 1; m < kClusterSize; m <<= 1) {
        const double o = __shfl_xor(Rc, m, kClusterSize);
        Rc = Rc < o ? o : Rc;
    }
    if (tid % kClusterSize == 0)
        sR[cl] = Rc;
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < kChunkClusters; ++k)
            Rc = Rc < sR[k] ? sR[k] : Rc;
        a.to.chunks[h] = ball_finish(cb, cc, Rc);
    }
}

/* ---- the regroup on the device (rtc_scene_regroup_async) ------------------------------------------------
 * The membership of a fresh upload of the caller's triangles, decided on the device before the refit: rtc_regroup.h's
 * levels, operation for operation (-ffp-contract=off; IEEE divide).  The caller's scratch holds the centroids, one array
 * of n doubles per axis, and two index buffers the levels alternate between.  Every position of a level's output is
 * written exactly once: a sorting segment's ranks are a permutation of its positions, and the others are copied. */
struct RegroupScratch {
    double *cent; /* [3][n] */
    int *idx[2];  /* position -> reference index, before and after a level */
};
static size_t regroup_round16(size_t b)
{
    return (b + 15) / 16 * 16;
}
static size_t regroup_scratch_bytes(int n)
{
    return regroup_round16(3 * sizeof(double) * (size_t)n) + 2 * regroup_round16(sizeof(int) * (size_t)n);
}
static RegroupScratch regroup_scratch(void *base, int n)
{
    unsigned char *p = static_cast<unsigned char *>(base);
    RegroupScratch r;
    r.cent = reinterpret_cast<double *>(p);
    p += regroup_round16(3 * sizeof(double) * (size_t)n);
    r.idx[0] = reinterpret_cast<int *>(p);
    r.idx[1] = reinterpret_cast<int *>(p + regroup_round16(sizeof(int) * (size_t)n));
    return r;
}

constexpr int kRegroupBlock = 256;
__global__ __launch_bounds__(kRegroupBlock) void rtc_regroup_centroids(const Triangle *tris, double *cent, int *idx, int n)
{
    const int i = (int)(blockIdx.x * kRegroupBlock + threadIdx.x);
    if (i >= n)
        return;
    const float *p = reinterpret_cast<const float *>(tris) + 17 * (size_t)i;
    for (int a = 0; a < 3; ++a)
        cent[(size_t)a * n + i] = regroup_centroid(p[a], pack_edge(p, 1, a), pack_edge(p, 2, a));
    idx[i] = i;
}

/* One level.  Workgroup (x, y): the positions [lo + 64 x, lo + 64 x + 64) of the segment reached by path y; its four waves
 * each count a quarter of every tile of kRegroupBlock keys streamed through LDS (the reads of sKey are broadcasts), and
 * the quarters are summed through LDS: ranks are sums of integers, any order.  The segment's extents are reduced by every
 * workgroup of the segment for itself, lanes first, then waves (regroup_extent_merge: any order).  Before that the whole
 * grid copies the positions this level does not sort. */
constexpr int kRegroupLanes = 64, kRegroupSlices = kRegroupBlock / kRegroupLanes;
__global__ __launch_bounds__(kRegroupBlock) void rtc_regroup_level(const double *cent, const int *in, int *out, int n,
                                                                    int level)
{
    const int tid = (int)threadIdx.x, px = tid % kRegroupLanes, slice = tid / kRegroupLanes;
    {
        const size_t g = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kRegroupBlock + tid;
        const size_t stride = (size_t)gridDim.x * gridDim.y * kRegroupBlock;
        for (size_t p = g; p < (size_t)n; p += stride) {
            int l, h;
            if (!regroup_segment_of_position(n, level, (int)p, l, h))
                out[p] = in[p];
        }
    }
    int lo, hi;
    if (!regroup_segment_of_path(n, level, blockIdx.y, lo, hi) || lo + (int)blockIdx.x * kRegroupLanes >= hi)
        return; /* (the same for every lane of the workgroup) */
    __shared__ RegroupExtent sExt[kRegroupSlices][3];
    __shared__ double sKey[kRegroupBlock];
    __shared__ int sRank[kRegroupSlices][kRegroupLanes];
    RegroupExtent e[3] = {regroup_extent_init(), regroup_extent_init(), regroup_extent_init()};
    for (int q = lo + tid; q < hi; q += kRegroupBlock) {
        const int i = in[q];
        for (int a = 0; a < 3; ++a)
            regroup_extent_take(e[a], cent[(size_t)a * n + i]);
    }
    for (int m = 1; m < kRegroupLanes; m <<= 1)
        for (int a = 0; a < 3; ++a) {
            const RegroupExtent o{__shfl_xor(e[a].mn, m, kRegroupLanes), __shfl_xor(e[a].mx, m, kRegroupLanes)};
            regroup_extent_merge(e[a], o);
        }
    if (px == 0)
        for (int a = 0; a < 3; ++a)
            sExt[slice][a] = e[a];
    __syncthreads();
    for (int a = 0; a < 3; ++a) {
        e[a] = sExt[0][a];
        for (int w = 1; w < kRegroupSlices; ++w)
            regroup_extent_merge(e[a], sExt[w][a]);
    }
    const double *key = cent + (size_t)regroup_axis(e) * n;
    const int p = lo + (int)blockIdx.x * kRegroupLanes + px;
    const bool mine = p < hi;
    const int ip = mine ? in[p] : 0;
    const double kp = mine ? regroup_key(key[ip]) : 0.0;
    int rank = 0;
    for (int base = lo; base < hi; base += kRegroupBlock) {
        const int q = base + tid;
        __syncthreads(); /* the tile before is counted */
        sKey[tid] = q < hi ? regroup_key(key[in[q]]) : 0.0;
        __syncthreads();
        const int j0 = slice * kRegroupLanes, j1 = min(j0 + kRegroupLanes, hi - base);
        if (mine)
            for (int j = j0; j < j1; ++j)
                rank += regroup_rank(sKey[j], base + j, kp, p);
    }
    sRank[slice][px] = rank;
    __syncthreads();
    if (slice == 0 && mine) {
        for (int w = 1; w < kRegroupSlices; ++w)
            rank += sRank[w][px];
        out[lo + rank] = ip;
    }
}

/* the membership as rtc_refit reads it: one int per clustered record, -1 for the last cluster's padding */
__global__ __launch_bounds__(kRegroupBlock) void rtc_regroup_index(const int *idx, int *clIndex, int n, int slots)
{
    const int k = (int)(blockIdx.x * kRegroupBlock + threadIdx.x);
    if (k < slots)
        clIndex[k] = k < n ? idx[k] : -1;
}

extern "C" int rtc_bounce_hit_share(const Triangle *tris, int triCount, float *share)
{
    if (!share || triCount < 0 || (triCount > 0 && !tris))
        return rtc_fail(RTC_EINVAL, "rtc_bounce_hit_share: bad argument");
    *share = (float)bounce_hit_share(tris, triCount);
    return 0;
}

extern "C" int rtc_bounce_hit_share_all(const Triangle *tris, int triCount, const Sphere *spheres, int sphereCount,
                                        float *share)
{
    if (!share || triCount < 0 || sphereCount < 0 || (triCount > 0 && !tris) || (sphereCount > 0 && !spheres))
        return rtc_fail(RTC_EINVAL, "rtc_bounce_hit_share_all: bad argument");
    *share = (float)bounce_hit_share(tris, triCount, spheres, sphereCount);
    return 0;
}

extern "C" int rtc_scene_sphere_split(const RtcDeviceScene *s)
{
    if (!s)
        return rtc_fail(RTC_EINVAL, "rtc_scene_sphere_split: null scene");
    return s->sphereSplitGate ? 1 : 0;
}

extern "C" int rtc_scene_chain_wgs(const RtcDeviceScene *s)
{
    if (!s)
        return rtc_fail(RTC_EINVAL, "rtc_scene_chain_wgs: null scene");
    return s->chainWgsFull;
}

extern "C" int rtc_scene_chain_report(const RtcDeviceScene *s, RtcChainReport *out)
{
    if (!s || !out)
        return rtc_fail(RTC_EINVAL, "rtc_scene_chain_report: null argument");
    *out = s->chainReport;
    return 0;
}

extern "C" int rtc_scene_last_plan(const RtcDeviceScene *s, int *ops, int maxOps, unsigned long long *footprint,
                                   int maxFootprint)
{
    if (!s || !ops || !footprint)
        return rtc_fail(RTC_EINVAL, "rtc_scene_last_plan: null argument");
    const rtcplan::Recorded &r = s->lastPlan;
    const int nOps = r.encoded & 0xff, rows = r.encoded >> 8;
    if (maxOps < nOps || maxFootprint < rows)
        return rtc_fail(RTC_EINVAL, "rtc_scene_last_plan: room for %d operations and %d rows, the plan has %d and %d",
                        maxOps, maxFootprint, nOps, rows);
    std::copy(r.ops, r.ops + 4 * nOps, ops);
    std::copy(r.fp, r.fp + 6 * (size_t)rows, footprint);
    return r.encoded;
}

/* Every device allocation of a scene, by the planner's resource numbers (rtc_plan.h Res).  The allocations are those of
 * rtc_scene_upload_with_share (the two generations' arrays, clIndex, primF, primX, segSlots, geoCounts), of
 * rtc_render.hip's grow_capacity (scratch, samples) and of draws_prepare above (table, ctr, blockSeed, pool, itemDraw):
 * a new hipMalloc in one of them needs its span here (tests/test_footprints.py counts them). */
extern "C" int rtc_scene_spans(const RtcDeviceScene *s, RtcSpan *out, int max)
{
    if (!s || !out)
        return rtc_fail(RTC_EINVAL, "rtc_scene_spans: null argument");
    int n = 0;
    const auto span = [&](int res, unsigned long long id, int part, const void *base, size_t bytes) {
        if (n < max)
            out[n] = RtcSpan{(unsigned long long)res, id, (unsigned long long)part,
                             (unsigned long long)(uintptr_t)(base && bytes ? base : nullptr), base ? bytes : 0};
        ++n;
    };
    span(rtcplan::kResScratch, 0, 0, s->scratch, s->plan.scratchCap);
    for (int h = 0; h < kSkySlots; ++h) {
        span(rtcplan::kResPrim, h, 0, s->primF + (size_t)h * s->primStride, s->primStride * sizeof(DevPrimF));
        span(rtcplan::kResPrim, h, 1, s->primX + (size_t)h * s->primStride, s->primStride * sizeof(DevPrimX));
    }
    for (int q = 0; q < kGeoRing; ++q)
        span(rtcplan::kResGeoSet, q, 0, s->geoCounts + (size_t)q * kGeoSetInts, kGeoSetInts * sizeof(int));
    span(rtcplan::kResSamples, 0, 0, s->samples, s->plan.samplesCap);
    span(rtcplan::kResSegSlots, 0, 0, s->segSlots, 256 * 16 * sizeof(unsigned long long));
    for (int g = 0; g < 2; ++g)
        for (int k = 0; k < kSceneArrayCount; ++k)
            span(rtcplan::kResSceneGen, g, k, scene_array(s->gen[g], k), s->recBytes[k]);
    const RtcDeviceScene::Draws &D = s->draws;
    span(rtcplan::kResDrawTable, 0, 0, D.table, D.tablePixels * sizeof(unsigned));
    span(rtcplan::kResDrawTable, 0, 1, D.ctr, kDcWords * sizeof(unsigned));
    span(rtcplan::kResDrawTable, 0, 2, D.blockSeed, D.capacity * sizeof(unsigned));
    for (int h = 0; h < kSkySlots; ++h)
        span(rtcplan::kResItemDraw, h, 0, D.itemDraw ? D.itemDraw + (size_t)h * (s->plan.itemDrawCap / kSkySlots) : nullptr,
             s->plan.itemDrawCap / kSkySlots);
    span(rtcplan::kResMembership, 0, 0, s->clIndex, (size_t)s->clusterCount * kClusterSize * sizeof(int));
    span(rtcplan::kResDrawPool, 0, 0, D.pool, D.capacity * kDrawBlockBytes);
    if (n > max)
        return rtc_fail(RTC_EINVAL, "rtc_scene_spans: room for %d spans, the scene has %d", max, n);
    return n;
}

/* ---- the draw cache's memory (rtc_layout.h RtcDeviceScene::Draws; the kernels: rtc_cull.h, rtc_chain.h) -------------- */
void rtc_draws_free(RtcDeviceScene *s)
{
    RtcDeviceScene::Draws &D = s->draws;
    for (void *p : {(void *)D.table, (void *)D.ctr, (void *)D.blockSeed, D.pool, (void *)D.itemDraw})
        if (p)
            (void)hipFree(p);
    const long long blocks = D.blocks;
    D = RtcDeviceScene::Draws{};
    D.blocks = blocks;
    /* the next launch that uses the cache plans a cleared table and new item-draw arrays */
    s->plan.drawWidth = s->plan.drawHeight = 0;
    s->plan.itemDrawCap = 0;
}

static int draws_prepare(RtcDeviceScene *s, int width, int height, bool reset, size_t growBytes)
{
    RtcDeviceScene::Draws &D = s->draws;
    const size_t pixels = (size_t)width * (size_t)height;
    if (reset || growBytes || !D.capacity)
        HIP_TRY(hipDeviceSynchronize());
    if (!D.capacity)
        reset = true;
    if (reset) {
        /* the pool: allocated at the first launch that uses the cache and never grown under launches in flight (that would
         * need a hipFree); a cleared cache for a larger frame, behind the synchronisation above, gets the larger pool */
        const long long want = D.blocks < 0 ? kDrawCacheDefaultBytes / (long long)kDrawBlockBytes : D.blocks;
        const size_t cap = std::min<size_t>((size_t)want, pixels);
        if (cap == 0 || cap >= 0xffffffffull)
            return rtc_fail(RTC_EINVAL, "draw cache: %zu blocks", cap);
        if (cap > D.capacity) {
            for (void *p : {(void *)D.blockSeed, D.pool})
                if (p)
                    HIP_TRY(hipFree(p));
            D.blockSeed = nullptr, D.pool = nullptr, D.capacity = 0;
            HIP_TRY(hipMalloc(&D.blockSeed, cap * sizeof(unsigned)));
            HIP_TRY(hipMalloc(&D.pool, cap * kDrawBlockBytes));
            D.capacity = cap;
        }
        if (!D.ctr)
            HIP_TRY(hipMalloc(&D.ctr, kDcWords * sizeof(unsigned)));
        if (pixels > D.tablePixels) {
            if (D.table)
                HIP_TRY(hipFree(D.table));
            D.table = nullptr, D.tablePixels = 0;
            HIP_TRY(hipMalloc(&D.table, pixels * sizeof(unsigned)));
            D.tablePixels = pixels;
        }
        HIP_TRY(hipMemset(D.table, 0, pixels * sizeof(unsigned)));
        HIP_TRY(hipMemset(D.ctr, 0, kDcWords * sizeof(unsigned)));
        D.parity = 0;
    }
    if (growBytes) {
        if (D.itemDraw)
            HIP_TRY(hipFree(D.itemDraw));
        D.itemDraw = nullptr;
        HIP_TRY(hipMalloc(&D.itemDraw, growBytes));
    }
    if (reset) /* (the scene's streams do not wait for the null stream's memsets) */
        HIP_TRY(hipDeviceSynchronize());
    return 0;
}

int rtc_draws_prepare(RtcDeviceScene *s, int width, int height, bool reset, size_t growBytes)
{
    const int rc = draws_prepare(s, width, height, reset, growBytes);
    if (rc) { /* nothing half-built stays behind */
        (void)hipDeviceSynchronize();
        rtc_draws_free(s);
    }
    return rc;
}

extern "C" int rtc_scene_set_draw_cache(RtcDeviceScene *s, long long blocks)
{
    if (!s)
        return rtc_fail(RTC_EINVAL, "rtc_scene_set_draw_cache: null scene");
    RtcDeviceGuard guard(s->device);
    if (!guard.ok())
        return rtc_fail(RTC_ENODEV, "rtc_scene_set_draw_cache: cannot select the scene's device %d", s->device);
    const RtcDeviceScene::Draws &D = s->draws;
    if (D.table || D.ctr || D.blockSeed || D.pool || D.itemDraw) { /* (nothing to drop before the first cached launch) */
        HIP_TRY(hipDeviceSynchronize());
        rtc_draws_free(s);
    }
    s->draws.blocks = blocks < 0 ? -1 : blocks;
    return 0;
}

extern "C" int rtc_scene_draw_cache_reset(RtcDeviceScene *s)
{
    if (!s)
        return rtc_fail(RTC_EINVAL, "rtc_scene_draw_cache_reset: null scene");
    RtcDeviceGuard guard(s->device);
    if (!guard.ok())
        return rtc_fail(RTC_ENODEV, "rtc_scene_draw_cache_reset: cannot select the scene's device %d", s->device);
    HIP_TRY(hipDeviceSynchronize());
    /* the next launch that uses the cache clears it (plan_launch: no frame size yet) */
    s->plan.drawWidth = s->plan.drawHeight = 0;
    return 0;
}

extern "C" int rtc_scene_draw_cache_stats(const RtcDeviceScene *s, unsigned long long out[4])
{
    if (!s || !out)
        return rtc_fail(RTC_EINVAL, "rtc_scene_draw_cache_stats: null argument");
    out[0] = out[1] = out[2] = out[3] = 0;
    RtcDeviceGuard guard(s->device);
    if (!guard.ok())
        return rtc_fail(RTC_ENODEV, "rtc_scene_draw_cache_stats: cannot select the scene's device %d", s->device);
    const RtcDeviceScene::Draws &D = s->draws;
    if (!D.capacity)
        return 0;
    HIP_TRY(hipDeviceSynchronize());
    unsigned c[kDcWords];
    HIP_TRY(hipMemcpy(c, D.ctr, sizeof c, hipMemcpyDeviceToHost));
    out[0] = std::min<unsigned long long>(c[kDcTaken], D.capacity);
    out[1] = D.capacity;
    out[2] = c[kDcFresh];
    out[3] = c[kDcUncached];
    return 0;
}

extern "C" int rtc_probe_draw_cache(const RtcDeviceScene *s, unsigned int seed, float *out, int *block)
{
    if (!s || !out || !block)
        return rtc_fail(RTC_EINVAL, "rtc_probe_draw_cache: null argument");
    *block = -1;
    RtcDeviceGuard guard(s->device);
    if (!guard.ok())
        return rtc_fail(RTC_ENODEV, "rtc_probe_draw_cache: cannot select the scene's device %d", s->device);
    const RtcDeviceScene::Draws &D = s->draws;
    if (!D.capacity || (size_t)seed >= (size_t)s->plan.drawWidth * (size_t)s->plan.drawHeight)
        return 0;
    HIP_TRY(hipDeviceSynchronize());
    unsigned k = 0;
    HIP_TRY(hipMemcpy(&k, D.table + seed, sizeof k, hipMemcpyDeviceToHost));
    if (k == 0 || k > D.capacity)
        return 0;
    HIP_TRY(hipMemcpy(out, (const unsigned char *)D.pool + (size_t)(k - 1) * kDrawBlockBytes, kDrawBlockBytes,
                      hipMemcpyDeviceToHost));
    *block = (int)(k - 1);
    return 0;
}

extern "C" int rtc_scene_upload(const Triangle *tris, int triCount, const Sphere *spheres, int sphereCount, int device,
                                RtcDeviceScene **out)
{
    return rtc_scene_upload_with_share(tris, triCount, spheres, sphereCount, device, -1.f, -1.f, out);
}


extern "C" float rtc_upload_hit_share(const Triangle *tris, int triCount)
{
    const int maskWords = ((triCount + 7) / 8 * 8 + 63) / 64;
    return triCount > 0 && tris && maskWords <= kMaxCullMaskWords ? (float)bounce_hit_share(tris, triCount) : 0.f;
}

extern "C" float rtc_upload_hit_share_all(const Triangle *tris, int triCount, const Sphere *spheres, int sphereCount,
                                          float hitShare)
{
    /* only launches the sphere split could take read it: without spheres it is the triangles' share, and with more
     * spheres than the split admits (or triangles than the tile cull does) the probe is skipped */
    const int maskWords = ((triCount + 7) / 8 * 8 + 63) / 64;
    if (sphereCount <= 0 || !spheres)
        return hitShare;
    if (sphereCount > rtcplan::kSplitSpheresMax || maskWords > kMaxCullMaskWords || (triCount > 0 && !tris))
        return 1.f;
    return (float)bounce_hit_share(tris, triCount, spheres, sphereCount);
}

/* The box of the triangles' vertices and the spheres' extents centre -+ r, in f32 (a NaN coordinate takes no part); zeros
 * for a scene without primitives.  The default bounds of the ray order's key. */
static void scene_bounds(const Triangle *tris, int triCount, const Sphere *spheres, int sphereCount, float lo[3], float hi[3])
{
    for (int a = 0; a < 3; ++a)
        lo[a] = INFINITY, hi[a] = -INFINITY;
    const auto take = [&](const float l[3], const float h[3]) {
        for (int a = 0; a < 3; ++a) {
            lo[a] = l[a] < lo[a] ? l[a] : lo[a];
            hi[a] = h[a] > hi[a] ? h[a] : hi[a];
        }
    };
    for (int i = 0; i < triCount; ++i)
        for (const vec3 *v : {&tris[i].posA, &tris[i].posB, &tris[i].posC}) {
            const float p[3] = {v->x, v->y, v->z};
            take(p, p);
        }
    for (int i = 0; i < sphereCount; ++i) {
        const Sphere &sp = spheres[i];
        const float l[3] = {sp.pos.x - sp.r, sp.pos.y - sp.r, sp.pos.z - sp.r};
        const float h[3] = {sp.pos.x + sp.r, sp.pos.y + sp.r, sp.pos.z + sp.r};
        take(l, h);
    }
    for (int a = 0; a < 3; ++a)
        if (!(lo[a] <= hi[a]))
            lo[a] = hi[a] = 0.f;
}

extern "C" int rtc_scene_upload_with_share(const Triangle *tris, int triCount, const Sphere *spheres, int sphereCount,
                                           int device, float hitShare, float hitShareAll, RtcDeviceScene **out)
{
    if (!out || triCount < 0 || sphereCount < 0 || (triCount > 0 && !tris) || (sphereCount > 0 && !spheres))
        return rtc_fail(RTC_EINVAL, "rtc_scene_upload: bad argument");
    *out = nullptr;
    int n = 0;
    int rc = rtc_device_count(&n);
    if (rc)
        return rc;
    if (device < 0)
        HIP_TRY(hipGetDevice(&device));
    if (device >= n)
        return rtc_fail(RTC_EINVAL, "device %d out of range (%d devices)", device, n);
    RtcDeviceGuard guard(device);
    if (!guard.ok())
        return rtc_fail(RTC_ENODEV, "rtc_scene_upload: cannot select device %d", device);
    HostRecords R;
    host_records(tris, triCount, spheres, sphereCount, false, R);
    const std::vector<DevTri> &dt = R.dt;
    RtcDeviceScene *s = new RtcDeviceScene();
    s->device = device;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0)
        cus = 256; /* MI355X */
    s->cuCount = cus;
    s->triCount = triCount;
    s->triPadded = (triCount + 7) / 8 * 8; /* whole pairs of batches; arrays hold 8 more records for prefetch */
    s->sphereCount = sphereCount;
    s->maskWords = (s->triPadded + 63) / 64;
    scene_bounds(tris, triCount, spheres, sphereCount, s->boundsLo, s->boundsHi);
    s->clusterCount = (triCount + kClusterSize - 1) / kClusterSize;
    s->chunkCount = (s->clusterCount + kChunkClusters - 1) / kChunkClusters;
    { /* the draw cache's capacity in blocks: RTC_DRAW_CACHE_BLOCKS (0: off), else the default (rtc_scene_set_draw_cache) */
        const char *v = getenv("RTC_DRAW_CACHE_BLOCKS");
        char *end = nullptr;
        const long long b = v && *v ? strtoll(v, &end, 10) : -1;
        s->draws.blocks = v && *v && end && *end == '\0' && b >= 0 ? b : -1;
    }
    /* whole frames of scenes whose bounce rays often hit again (fsuzane) run 4 chain workgroups per CU: their frame is
     * nearly all geometry kernel, which then has the registers the co-resident sky waves would use (round 5, 1080p x64:
     * fsuzane 1.25 -> 1.16 ms per frame; ultracomplex 0.348 -> 0.379, complex 4K 1.22 -> 1.34, so 3 stays the default,
     * profiles/r05_w4_ab_chain_wgs.log) */
    s->hitShare = hitShare >= 0.f ? (double)hitShare : (double)rtc_upload_hit_share(tris, triCount);
    s->chainWgsFull = s->hitShare > kWgsHitShare ? RTC_CHAIN_WGS_HIT : RTC_CHAIN_WGS_FULL;
    /* sphere scenes whose bounce rays mostly escape render through the split launch (rtcplan::sphere_split) */
    s->hitShareAll = hitShareAll >= 0.f
                         ? (double)hitShareAll
                         : (double)rtc_upload_hit_share_all(tris, triCount, spheres, sphereCount, (float)s->hitShare);
    /* (a scene of spheres alone stays on the pixel kernel: no threshold on the share separates it from the open scenes
     * with triangles -- both measure 0.001 -- and without triangle work a wave per pixel loses to a lane per pixel,
     * 3.06 vs 2.74 ms per 1080p x64 frame) */
    s->sphereSplitGate = sphereCount > 0 && sphereCount <= rtcplan::kSplitSpheresMax && triCount > 0 &&
                         s->hitShareAll <= rtcplan::kSplitMaxHitShare;
    /* two generations of the records (rtc_scene_update_async writes the one no launch binds); the upload's are
     * generation 0, generation 1 starts zeroed (its padding records stay zero: an update writes the real ones) */
    const void *host[kSceneArrayCount];
    R.arrays(host, s->recBytes);
    hipError_t e = hipSuccess;
    for (int g = 0; g < 2; ++g)
        for (int k = 0; k < kSceneArrayCount; ++k) {
            void *&dev = scene_array(s->gen[g], k);
            const size_t bytes = s->recBytes[k];
            if (e == hipSuccess)
                e = hipMalloc(&dev, bytes);
            if (e == hipSuccess)
                e = g == 0 ? hipMemcpy(dev, host[k], bytes, hipMemcpyHostToDevice) : hipMemset(dev, 0, bytes);
        }
    /* the membership, one int per clustered record (-1: the last cluster's padding) */
    std::vector<int> clIndex(R.ct.size(), -1);
    std::copy(R.idx.begin(), R.idx.end(), clIndex.begin());
    if (e == hipSuccess)
        e = hipMalloc(&s->clIndex, clIndex.size() * sizeof(int));
    if (e == hipSuccess)
        e = hipMemcpy(s->clIndex, clIndex.data(), clIndex.size() * sizeof(int), hipMemcpyHostToDevice);
    s->primStride = dt.size();
    if (e == hipSuccess)
        e = hipMalloc(&s->primF, kSkySlots * dt.size() * sizeof(DevPrimF));
    if (e == hipSuccess)
        e = hipMalloc(&s->primX, kSkySlots * dt.size() * sizeof(DevPrimX));
    if (e == hipSuccess)
        e = hipMalloc(&s->segSlots, 256 * 16 * sizeof(unsigned long long));
    if (e == hipSuccess) /* kept zero between launches by rtc_reduce_segments */
        e = hipMemset(s->segSlots, 0, 256 * 16 * sizeof(unsigned long long));
    if (e == hipSuccess)
        e = hipMalloc(&s->geoCounts, kGeoRing * kGeoSetInts * sizeof(int));
    if (e == hipSuccess)
        e = hipMemset(s->geoCounts, 0, kGeoRing * kGeoSetInts * sizeof(int));
    int leastPrio = 0, greatestPrio = 0;
    if (e == hipSuccess)
        e = hipDeviceGetStreamPriorityRange(&leastPrio, &greatestPrio);
    if (e == hipSuccess) /* the sky tiles yield to the heavy tiles */
        e = hipStreamCreateWithPriority(&s->side, hipStreamNonBlocking, leastPrio);
    if (e == hipSuccess) /* the next frame's cull goes first wherever a CU frees up */
        e = hipStreamCreateWithPriority(&s->cst, hipStreamNonBlocking, greatestPrio);
    if (e == hipSuccess)
        e = hipEventCreateWithFlags(&s->evCullSync, kOrderEventFlags);
    if (e == hipSuccess)
        e = hipEventCreateWithFlags(&s->evFork, kOrderEventFlags);
    if (e == hipSuccess)
        e = hipEventCreateWithFlags(&s->evJoin, kOrderEventFlags);
    for (int h = 0; h < kSkySlots; ++h)
        if (e == hipSuccess)
            e = hipEventCreateWithFlags(&s->evSkyDone[h], kOrderEventFlags);
    for (int h = 0; h < kSkySlots; ++h)
        if (e == hipSuccess)
            e = hipEventCreateWithFlags(&s->evGeoDone[h], kOrderEventFlags);
    for (hipEvent_t *ev : {&s->evHeavy0, &s->evHeavy1, &s->evSky0, &s->evSky1})
        if (e == hipSuccess)
            e = hipEventCreate(ev);
    if (e != hipSuccess) {
        rtc_scene_release(s);
        return rtc_fail(-(int)e, "scene upload failed: %s", hipGetErrorString(e));
    }
    *out = s;
    return 0;
}

extern "C" int rtc_scene_release(RtcDeviceScene *s)
{
    if (!s)
        return 0;
    int cur = -1;
    (void)hipGetDevice(&cur);
    (void)hipSetDevice(s->device);
    if (s->side) /* an unjoined sky pass (RTC_F_OVERLAP) may still read the scratch */
        (void)hipStreamSynchronize(s->side);
    if (s->cst)
        (void)hipStreamSynchronize(s->cst);
    if (s->cst2)
        (void)hipStreamSynchronize(s->cst2);
    for (const SceneRecords &g : s->gen)
        for (int k = 0; k < kSceneArrayCount; ++k)
            if (void *p = scene_array(g, k))
                (void)hipFree(p);
    if (s->clIndex)
        (void)hipFree(s->clIndex);
    if (s->primF)
        (void)hipFree(s->primF);
    if (s->primX)
        (void)hipFree(s->primX);
    if (s->scratch)
        (void)hipFree(s->scratch);
    if (s->samples)
        (void)hipFree(s->samples);
    if (s->segSlots)
        (void)hipFree(s->segSlots);
    if (s->geoCounts)
        (void)hipFree(s->geoCounts);
    rtc_draws_free(s);
    if (s->evFork)
        (void)hipEventDestroy(s->evFork);
    if (s->evJoin)
        (void)hipEventDestroy(s->evJoin);
    for (hipEvent_t ev : {s->evHeavy0, s->evHeavy1, s->evSky0, s->evSky1, s->evCullSync})
        if (ev)
            (void)hipEventDestroy(ev);
    for (hipEvent_t ev : s->evSkyDone)
        if (ev)
            (void)hipEventDestroy(ev);
    for (hipEvent_t ev : s->evGeoDone)
        if (ev)
            (void)hipEventDestroy(ev);
    if (s->side)
        (void)hipStreamDestroy(s->side);
    if (s->cst)
        (void)hipStreamDestroy(s->cst);
    if (s->cst2)
        (void)hipStreamDestroy(s->cst2);
    if (cur >= 0)
        (void)hipSetDevice(cur);
    delete s;
    return 0;
}

/* what rtc_scene_update_async and rtc_scene_regroup_async refuse alike (0: fine) */
static int update_arguments(const char *who, const RtcDeviceScene *s, const Triangle *dTris, int triCount,
                            const Sphere *dSpheres, int sphereCount)
{
    if (!s)
        return rtc_fail(RTC_EINVAL, "%s: null scene", who);
    if (!dTris && !dSpheres)
        return rtc_fail(RTC_EINVAL, "%s: neither triangles nor spheres", who);
    if (triCount != (dTris ? s->triCount : 0) || sphereCount != (dSpheres ? s->sphereCount : 0))
        return rtc_fail(RTC_EINVAL, "%s: %d triangles / %d spheres for a scene uploaded with %d / %d "
                                    "(a kind left out: a null pointer and 0)",
                        who, triCount, sphereCount, s->triCount, s->sphereCount);
    if ((dTris && s->triCount == 0) || (dSpheres && s->sphereCount == 0))
        return rtc_fail(RTC_EINVAL, "%s: the scene was uploaded without that kind of primitive", who);
    return 0;
}

/* the planned wait of an update or a regroup: the sky-done event of a slot (false: not one) */
static bool update_wait(const RtcDeviceScene *s, const rtcplan::Op &op, hipStream_t st, hipError_t &e)
{
    const int slot = op.event - rtcplan::kEvSkyDone0;
    if (op.kind != rtcplan::kOpWait || slot < 0 || slot >= kSkySlots)
        return false;
    e = hipStreamWaitEvent(st, s->evSkyDone[slot], 0);
    return true;
}

static hipError_t launch_refit(const RtcDeviceScene *s, const Triangle *dTris, const Sphere *dSpheres, int reads, int writes,
                               hipStream_t st)
{
    RefitArgs a{};
    a.srcTris = dTris, a.srcSpheres = dSpheres;
    a.from = s->gen[reads], a.to = s->gen[writes];
    a.clIndex = s->clIndex;
    a.clusterCount = s->clusterCount, a.sphereCount = s->sphereCount;
    for (int k = 0; k < kSceneArrayCount; ++k)
        a.n16[k] = s->recBytes[k] / 16;
    hipLaunchKernelGGL(rtc_refit, dim3((unsigned)std::max(s->chunkCount, 1)), dim3(kRefitBlock), 0, st, a);
    return hipGetLastError();
}

extern "C" int rtc_scene_update_async(RtcDeviceScene *s, const Triangle *dTris, int triCount, const Sphere *dSpheres,
                                      int sphereCount, void *stream)
{
    if (const int rc = update_arguments("rtc_scene_update_async", s, dTris, triCount, dSpheres, sphereCount))
        return rc;
    RtcDeviceGuard guard(s->device);
    if (!guard.ok())
        return rtc_fail(RTC_ENODEV, "rtc_scene_update_async: cannot select the scene's device %d", s->device);
    /* the planner decides which launches the kernel waits for and which generation it writes (rtc_plan.h plan_update);
     * this function executes its operations */
    rtcplan::UpdatePlan up;
    rtcplan::plan_update(s->plan, 0, up);
    const hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i < up.nOps; ++i) {
        const rtcplan::Op &op = up.ops[i];
        if (op.stream != rtcplan::kStCaller)
            return rtc_fail(RTC_EINVAL, "rtc_scene_update_async: an operation off the caller's stream");
        hipError_t e = hipSuccess;
        if (update_wait(s, op, st, e)) {
            HIP_TRY(e);
        } else if (op.kind == rtcplan::kOpKernel && op.kernel == rtcplan::kKRefit) {
            HIP_TRY(launch_refit(s, dTris, dSpheres, up.reads, up.writes, st));
        } else {
            return rtc_fail(RTC_EINVAL, "rtc_scene_update_async: unknown planned operation %d", op.kind);
        }
    }
    s->plan = up.after; /* every operation is enqueued */
    rtcplan::record_update(up, s->lastPlan);
    return 0;
}

extern "C" int rtc_scene_regroup_max_tris(void)
{
    return kRegroupMaxTris;
}

extern "C" size_t rtc_scene_regroup_scratch_bytes(const RtcDeviceScene *s)
{
    return s ? regroup_scratch_bytes(s->triCount) : 0;
}

extern "C" int rtc_scene_regroup_async(RtcDeviceScene *s, const Triangle *dTris, int triCount, const Sphere *dSpheres,
                                       int sphereCount, void *dScratch, size_t scratchBytes, void *stream)
{
    const char *const who = "rtc_scene_regroup_async";
    if (const int rc = update_arguments(who, s, dTris, triCount, dSpheres, sphereCount))
        return rc;
    if (!dTris)
        return rtc_fail(RTC_EINVAL, "%s: no triangles (the membership is decided from them)", who);
    if (triCount > kRegroupMaxTris)
        return rtc_fail(RTC_EINVAL, "%s: %d triangles, a regroup takes at most %d (rtc_scene_regroup_max_tris): upload again",
                        who, triCount, kRegroupMaxTris);
    if (!dScratch || (uintptr_t)dScratch % 16 || scratchBytes < regroup_scratch_bytes(triCount))
        return rtc_fail(RTC_EINVAL, "%s: the scratch must be %zu bytes of device memory, 16-byte aligned "
                                    "(rtc_scene_regroup_scratch_bytes)", who, regroup_scratch_bytes(triCount));
    RtcDeviceGuard guard(s->device);
    if (!guard.ok())
        return rtc_fail(RTC_ENODEV, "%s: cannot select the scene's device %d", who, s->device);
    /* the planner's operations (rtc_plan.h plan_regroup: an update's waits and generation, the membership's kernels, the
     * refit), executed in order; the level kernels take their levels in the order planned */
    const int n = triCount;
    rtcplan::RegroupPlan gp;
    rtcplan::plan_regroup(s->plan, regroup_levels(n), gp);
    const RegroupScratch sc = regroup_scratch(dScratch, n);
    const hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((n + kRegroupBlock - 1) / kRegroupBlock);
    int level = 0;
    for (int i = 0; i < gp.nOps; ++i) {
        const rtcplan::Op &op = gp.ops[i];
        if (op.stream != rtcplan::kStCaller)
            return rtc_fail(RTC_EINVAL, "%s: an operation off the caller's stream", who);
        hipError_t e = hipSuccess;
        if (update_wait(s, op, st, e)) {
            HIP_TRY(e);
        } else if (op.kind != rtcplan::kOpKernel) {
            return rtc_fail(RTC_EINVAL, "%s: unknown planned operation %d", who, op.kind);
        } else if (op.kernel == rtcplan::kKRegroupCentroids) {
            hipLaunchKernelGGL(rtc_regroup_centroids, dim3(blocks), dim3(kRegroupBlock), 0, st, dTris, sc.cent, sc.idx[0], n);
            HIP_TRY(hipGetLastError());
        } else if (op.kernel == rtcplan::kKRegroupLevel && level < gp.levels) {
            const unsigned tiles = (unsigned)((regroup_level_width(n, level) + kRegroupLanes - 1) / kRegroupLanes);
            hipLaunchKernelGGL(rtc_regroup_level, dim3(tiles, 1u << level), dim3(kRegroupBlock), 0, st, sc.cent,
                               sc.idx[level & 1], sc.idx[(level & 1) ^ 1], n, level);
            HIP_TRY(hipGetLastError());
            ++level;
        } else if (op.kernel == rtcplan::kKRegroupIndex) {
            const int slots = s->clusterCount * kClusterSize;
            hipLaunchKernelGGL(rtc_regroup_index, dim3((unsigned)((slots + kRegroupBlock - 1) / kRegroupBlock)),
                               dim3(kRegroupBlock), 0, st, sc.idx[gp.levels & 1], s->clIndex, n, slots);
            HIP_TRY(hipGetLastError());
        } else if (op.kernel == rtcplan::kKRefit) {
            HIP_TRY(launch_refit(s, dTris, dSpheres, gp.reads, gp.writes, st));
        } else {
            return rtc_fail(RTC_EINVAL, "%s: unknown planned kernel %d", who, op.kernel);
        }
    }
    s->plan = gp.after; /* every operation is enqueued */
    rtcplan::record_regroup(gp, (uint64_t)(uintptr_t)dScratch, s->lastPlan);
    return 0;
}

extern "C" int rtc_scene_regroup(RtcDeviceScene *s, const Triangle *tris, int triCount, const Sphere *spheres,
                                 int sphereCount)
{
    if (!s)
        return rtc_fail(RTC_EINVAL, "rtc_scene_regroup: null scene");
    if (!tris || triCount <= 0)
        return rtc_fail(RTC_EINVAL, "rtc_scene_regroup: no triangles (the membership is decided from them)");
    /* staged as rtc_scene_update stages, the scratch with them; the other arguments are checked by the asynchronous call */
    const bool sph = spheres && sphereCount > 0;
    const size_t scratch = regroup_scratch_bytes(triCount);
    const Staged items[3] = {{tris, nullptr, (size_t)triCount * sizeof(Triangle), true},
                             {spheres, nullptr, sph ? (size_t)sphereCount * sizeof(Sphere) : 0, sph},
                             {nullptr, nullptr, scratch, true}};
    return staged_query("rtc_scene_regroup", s, items, [&](void *const dev[3]) {
        return rtc_scene_regroup_async(s, static_cast<const Triangle *>(dev[0]), triCount,
                                       spheres ? static_cast<const Sphere *>(dev[1]) : nullptr, sphereCount, dev[2], scratch,
                                       nullptr);
    });
}

extern "C" int rtc_scene_update(RtcDeviceScene *s, const Triangle *tris, int triCount, const Sphere *spheres,
                                int sphereCount)
{
    if (!s)
        return rtc_fail(RTC_EINVAL, "rtc_scene_update: null scene");
    /* staged through two device buffers (a kind left out, or given with no count: a null pointer and the caller's count);
     * the arguments are checked by the asynchronous call */
    const bool tri = tris && triCount > 0, sph = spheres && sphereCount > 0;
    const Staged items[2] = {{tris, nullptr, tri ? (size_t)triCount * sizeof(Triangle) : 0, tri},
                             {spheres, nullptr, sph ? (size_t)sphereCount * sizeof(Sphere) : 0, sph}};
    return staged_query("rtc_scene_update", s, items, [&](void *const dev[2]) {
        return rtc_scene_update_async(s, static_cast<const Triangle *>(dev[0]), triCount,
                                      static_cast<const Sphere *>(dev[1]), sphereCount, nullptr);
    });
}

/* copies `bytes` of `src` (host or device) into out when the caller gave a buffer, and reports the size */
static int give_records(void *const out[], size_t cap[], const void *const src[], const size_t bytes[], bool device)
{
    for (int k = 0; k < kSceneArrayCount; ++k) {
        if (out[k] && cap[k] < bytes[k])
            return rtc_fail(RTC_EINVAL, "scene records: buffer %d holds %zu bytes of %zu", k, cap[k], bytes[k]);
        if (out[k] && device)
            HIP_TRY(hipMemcpy(out[k], src[k], bytes[k], hipMemcpyDeviceToHost));
        else if (out[k])
            memcpy(out[k], src[k], bytes[k]);
        cap[k] = bytes[k];
    }
    return 0;
}

extern "C" int rtc_scene_records_host(const Triangle *tris, int triCount, const Triangle *newTris, const Sphere *spheres,
                                      int sphereCount, void *outTris, void *outMats, void *outSpheres, void *outClTris,
                                      void *outClusters, void *outChunks, size_t bytes[6])
{
    if (!bytes || triCount < 0 || sphereCount < 0 || (triCount > 0 && !tris) || (sphereCount > 0 && !spheres))
        return rtc_fail(RTC_EINVAL, "rtc_scene_records_host: bad argument");
    HostRecords R;
    host_records(tris, triCount, spheres, sphereCount, false, R);
    if (newTris)
        host_records(newTris, triCount, spheres, sphereCount, true, R);
    void *const out[kSceneArrayCount] = {outTris, outMats, outSpheres, outClTris, outClusters, outChunks};
    const void *src[kSceneArrayCount];
    size_t have[kSceneArrayCount];
    R.arrays(src, have);
    return give_records(out, bytes, src, have, false);
}

extern "C" int rtc_probe_scene_records(const RtcDeviceScene *s, void *outTris, void *outMats, void *outSpheres,
                                       void *outClTris, void *outClusters, void *outChunks, size_t bytes[6])
{
    if (!s || !bytes)
        return rtc_fail(RTC_EINVAL, "rtc_probe_scene_records: null argument");
    RtcDeviceGuard guard(s->device);
    if (!guard.ok())
        return rtc_fail(RTC_ENODEV, "rtc_probe_scene_records: cannot select the scene's device %d", s->device);
    HIP_TRY(hipDeviceSynchronize()); /* the scene's streams and the caller's: every update enqueued so far has run */
    const SceneRecords &g = s->current();
    void *const out[kSceneArrayCount] = {outTris, outMats, outSpheres, outClTris, outClusters, outChunks};
    const void *src[kSceneArrayCount];
    for (int k = 0; k < kSceneArrayCount; ++k)
        src[k] = scene_array(g, k);
    return give_records(out, bytes, src, s->recBytes, true);
}

extern "C" int rtc_rows_selected(const RtcRenderDesc *d)
{
    if (!d || d->rowStride <= 0 || d->rowStart < 0 || d->rowStart >= d->height || d->height <= 0 || d->rowBand < 0)
        return 0;
    /* bands of B rows (rowBand, rtc.h): the full bands' rows, plus the last band's rows inside the frame */
    const long long B = d->rowBand > 1 ? d->rowBand : 1, step = (long long)d->rowStride * B;
    const long long nb = (d->height - d->rowStart + step - 1) / step, last = d->rowStart + (nb - 1) * step;
    return (int)((nb - 1) * B + std::min<long long>(B, d->height - last));
}

extern "C" int rtc_scene_set_geometry_event(RtcDeviceScene *s, void *event)
{
    if (!s)
        return rtc_fail(RTC_EINVAL, "rtc_scene_set_geometry_event: null scene");
    s->geoEvent = (hipEvent_t)event;
    return 0;
}

extern "C" int rtc_scene_set_frame_event(RtcDeviceScene *s, void *event)
{
    if (!s)
        return rtc_fail(RTC_EINVAL, "rtc_scene_set_frame_event: null scene");
    s->frameEvent = (hipEvent_t)event;
    return 0;
}

extern "C" int rtc_scene_set_timing(RtcDeviceScene *s, int enable)
{
    if (!s)
        return rtc_fail(RTC_EINVAL, "rtc_scene_set_timing: null scene");
    s->timing = enable != 0;
    return 0;
}

extern "C" int rtc_scene_kernel_times(const RtcDeviceScene *s, float out[2])
{
    if (!s || !out)
        return rtc_fail(RTC_EINVAL, "rtc_scene_kernel_times: null argument");
    out[0] = out[1] = -1.f;
    if (!s->timed)
        return 0;
    RtcDeviceGuard guard(s->device);
    HIP_TRY(hipEventSynchronize(s->evHeavy1));
    HIP_TRY(hipEventSynchronize(s->evSky1));
    HIP_TRY(hipEventElapsedTime(&out[0], s->evHeavy0, s->evHeavy1));
    HIP_TRY(hipEventElapsedTime(&out[1], s->evSky0, s->evSky1));
    return 0;
}
