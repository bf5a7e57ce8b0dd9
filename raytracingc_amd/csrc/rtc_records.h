/* rtc_records.h -- the arithmetic of the scene records, stated once for the host and the device: a
 * Triangle / Sphere packed into DevTri / DevMat / DevSphere, the aligned-normal flag of a clustered record, and the
 * bounding ball and cull margins (DevCluster) of a cluster or a chunk.  The upload's host build (rtc_scene.hip pack_scene,
 * ball_of, rtc_cluster_records) and the device refit (rtc_refit) are both built from these functions, so a resident scene
 * after an update or a regroup holds what a fresh upload builds, byte for byte, by construction and not by two
 * restatements agreeing.  All double arithmetic: -ffp-contract=off on both sides, IEEE divide.  The functions have the
 * shape the kernel needs (one record at a time, partial results merged); the host loops over them. */
#pragma once
#include <cmath>

#include "rtc_layout.h"

#define RTC_REC_HD __host__ __device__ __forceinline__

/* The primitives that are spelled differently per side.  Both sides are correctly rounded IEEE operations (the square
 * root) or exact ones (the classification, the absolute value), so both give the same bits. */
#if defined(__HIP_DEVICE_COMPILE__)
RTC_REC_HD double rec_sqrt(double x) { return __dsqrt_rn(x); }
RTC_REC_HD bool rec_isfinite(double x) { return isfinite(x); }
RTC_REC_HD double rec_fabs(double x) { return fabs(x); }
#else
RTC_REC_HD double rec_sqrt(double x) { return std::sqrt(x); }
RTC_REC_HD bool rec_isfinite(double x) { return std::isfinite(x); }
RTC_REC_HD double rec_fabs(double x) { return std::fabs(x); }
#endif

/* ---- packing: p is a Triangle as 17 floats (posA, posB, posC, normal, mat) or a Sphere as 9 (pos, r, mat) ------------- */
static_assert(sizeof(Triangle) == 17 * sizeof(float) && sizeof(Sphere) == 9 * sizeof(float), "the packers read floats");

/* The edges AB (v = 1) and AC (v = 2) along axis a: raytracing.c:191-192 minus(posB, posA), minus(posC, posA), the same
 * f32 operation */
RTC_REC_HD float pack_edge(const float *p, int v, int a)
{
    return p[3 * v + a] - p[a];
}

RTC_REC_HD DevTri pack_tri(const float *p)
{
    DevTri r{};
    r.ax = p[0], r.ay = p[1], r.az = p[2];
    r.abx = pack_edge(p, 1, 0), r.aby = pack_edge(p, 1, 1), r.abz = pack_edge(p, 1, 2);
    r.acx = pack_edge(p, 2, 0), r.acy = pack_edge(p, 2, 1), r.acz = pack_edge(p, 2, 2);
    r.nx = p[9], r.ny = p[10], r.nz = p[11];
    return r;
}

RTC_REC_HD DevMat pack_mat(const float *p)
{
    return DevMat{p[12], p[13], p[14], p[15], p[16], 0.f, 0.f, 0.f};
}

RTC_REC_HD DevSphere pack_sphere(const float *p)
{
    return DevSphere{p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], 0.f, 0.f, 0.f};
}

/* ---- the aligned-normal flag ------------------------------------------------------------------------------------------
 * A triangle whose stored normal N points along its geometric normal G' = AB x AC closely enough that, for every
 * ray of |dir|_1 <= kClusterRhoMax, rayTriangle's backface test (dot(dir, N) < 0, raytracing.c:189) forces
 * det = dot(AB, dir x AC) > -EPSILON (raytracing.c:195): then a hit needs det >= EPSILON, and since
 * dst = dot(AC, q) / det (q = (pos - A) x AB, raytracing.c:202-206) must be >= EPSILON, dot(AC, q) > 0.  For a
 * ray origin where the reference's own f32 dot(AC, q) is <= 0 (pos on or behind the plane), the triangle cannot
 * be hit from there in any direction (rtc_render_chain's first bounces).  Bound: with N = a G'/|G'| + e (e
 * orthogonal), fl(dot(dir, N)) < 0 gives dir.G'/|G'| < rho (3.01u |N|_inf + |e|) / a, and |det + dir.G'| <=
 * 5.1u |AB|_1 |AC|_1 rho; aligned when rho times their sum, with a factor 2, stays below EPSILON. */
RTC_REC_HD bool aligned_normal(const DevTri &r)
{
    const double u = 0x1p-24;
    const double AB[3] = {r.abx, r.aby, r.abz}, AC[3] = {r.acx, r.acy, r.acz}, N[3] = {r.nx, r.ny, r.nz};
    const double G[3] = {AB[1] * AC[2] - AB[2] * AC[1], AB[2] * AC[0] - AB[0] * AC[2], AB[0] * AC[1] - AB[1] * AC[0]};
    const double g = rec_sqrt(G[0] * G[0] + G[1] * G[1] + G[2] * G[2]);
    if (!(g > 0.0) || !rec_isfinite(g))
        return false;
    const double a = (N[0] * G[0] + N[1] * G[1] + N[2] * G[2]) / g;
    if (!(a > 0.0))
        return false;
    const double e[3] = {N[0] - a * G[0] / g, N[1] - a * G[1] / g, N[2] - a * G[2] / g};
    const double en = rec_sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]) + 1e-12 * (rec_fabs(N[0]) + rec_fabs(N[1]) + rec_fabs(N[2]));
    const double m12 = rec_fabs(N[1]) < rec_fabs(N[2]) ? rec_fabs(N[2]) : rec_fabs(N[1]);
    const double ninf = rec_fabs(N[0]) < m12 ? m12 : rec_fabs(N[0]);
    const double n1 = rec_fabs(AB[0]) + rec_fabs(AB[1]) + rec_fabs(AB[2]), c1 = rec_fabs(AC[0]) + rec_fabs(AC[1]) + rec_fabs(AC[2]);
    const double K = g * (3.01 * u * ninf + en) / a + 5.1 * u * n1 * c1;
    return rec_isfinite(K) && 2.0 * kClusterRhoMax * K < 0.001;
}

/* ---- the ball ---------------------------------------------------------------------------------------------------------
 * Bounding ball and cull margins (DevCluster) of a set of records: the ball holds every vertex A, A + AB, A + AC; E is the
 * longest AB / AC edge.  First the extent of the vertices (BallAcc: acc_init, acc_record per record, acc_merge of partial
 * results), then the centre (ball_centre), then the radius about the rounded (float) centre (the largest rec_radius), then
 * ball_finish.  The min / max steps keep the accumulator unless the candidate is strictly smaller (larger): they skip a
 * NaN, and among equal zeros the first one offered stays, so the order decides the sign of a zero centre: the host offers
 * the records in sequence (chunks too: over their records, never merged), and the device's merges keep the lower lane's
 * and the lower cluster's value in the lane that writes, which is the same one. */
struct BallAcc {
    double lo[3], hi[3], E;
    int finite, n;
};

RTC_REC_HD void acc_init(BallAcc &b)
{
    for (int a = 0; a < 3; ++a)
        b.lo[a] = 1e300, b.hi[a] = -1e300;
    b.E = 0.0;
    b.finite = 1;
    b.n = 0;
}

RTC_REC_HD void acc_record(BallAcc &b, const DevTri &r)
{
    ++b.n;
    const double A[3] = {r.ax, r.ay, r.az}, B[3] = {r.abx, r.aby, r.abz}, C[3] = {r.acx, r.acy, r.acz};
    for (int a = 0; a < 3; ++a) {
        const double v[3] = {A[a], A[a] + B[a], A[a] + C[a]};
        for (int w = 0; w < 3; ++w) {
            const double x = v[w];
            b.finite = b.finite && rec_isfinite(x);
            b.lo[a] = x < b.lo[a] ? x : b.lo[a];
            b.hi[a] = b.hi[a] < x ? x : b.hi[a];
        }
    }
    const double sb = rec_sqrt(B[0] * B[0] + B[1] * B[1] + B[2] * B[2]);
    const double sc = rec_sqrt(C[0] * C[0] + C[1] * C[1] + C[2] * C[2]);
    const double m = sb < sc ? sc : sb;
    b.E = b.E < m ? m : b.E;
}

/* two partial results (neither holds a NaN: acc_record never stores one) */
RTC_REC_HD void acc_merge(BallAcc &b, const BallAcc &o)
{
    for (int a = 0; a < 3; ++a) {
        b.lo[a] = o.lo[a] < b.lo[a] ? o.lo[a] : b.lo[a];
        b.hi[a] = b.hi[a] < o.hi[a] ? o.hi[a] : b.hi[a];
    }
    b.E = b.E < o.E ? o.E : b.E;
    b.finite = b.finite && o.finite;
    b.n += o.n;
}

RTC_REC_HD void ball_centre(const BallAcc &b, float c[3])
{
    for (int a = 0; a < 3; ++a)
        c[a] = b.n ? (float)((b.lo[a] + b.hi[a]) / 2) : 0.f;
}

/* the largest distance of one record's vertices from the (float) centre */
RTC_REC_HD double rec_radius(const DevTri &r, const float c[3])
{
    const double A[3] = {r.ax, r.ay, r.az}, B[3] = {r.abx, r.aby, r.abz}, C[3] = {r.acx, r.acy, r.acz};
    const double K[3] = {c[0], c[1], c[2]};
    double R = 0.0;
    for (int w = 0; w < 3; ++w) {
        double d2 = 0.0;
        for (int a = 0; a < 3; ++a) {
            const double x = A[a] + (w == 1 ? B[a] : w == 2 ? C[a] : 0.0) - K[a];
            d2 += x * x;
        }
        const double s = rec_sqrt(d2);
        R = R < s ? s : R;
    }
    return R;
}

RTC_REC_HD float next_up(float x) /* nextafter(x, +inf) for x >= 0, +inf or NaN: a bit increment */
{
    if (!(x < INFINITY))
        return x;
    return __builtin_bit_cast(float, x == 0.f ? 1u : __builtin_bit_cast(unsigned, x) + 1u);
}

/* the record from the reduced extent, the centre and the radius about it; |det| >= 0.001f > eps for every reported hit */
RTC_REC_HD DevCluster ball_finish(const BallAcc &b, const float c[3], double R)
{
    const double u = 0x1p-24, eps = 0.001, E = b.E;
    DevCluster k{};
    k.cx = c[0], k.cy = c[1], k.cz = c[2];
    const double F = 4.0, edRatio = 8.0 * u * E * E * kClusterRhoMax / eps;
    k.r = next_up((float)(R * (1.0 + 1e-9)));
    k.e = (float)E;
    if (!b.finite || b.n == 0 || !(edRatio < 0.5) || !(k.r < 1e18f)) {
        k.alpha = INFINITY; /* never culled */
        k.beta = k.gammaE = 0.f;
        return k;
    }
    const double kk = 1.0 / (1.0 - edRatio);
    k.alpha = next_up((float)(F * kk * 32.0 * u * E * E * E / eps));
    k.beta = next_up((float)(F * kk * 45.0 * u * E * E / eps));
    k.gammaE = next_up((float)(kClusterGamma * E));
    return k;
}
