/* rtc_closest.h -- the primary filter's records (rtc_prep_primary) and the closest-hit queries of the one-lane-per-pixel
 * kernel: calculateRayCollision over the primary and the general records.
 * A section of rtc_render.hip's translation unit: included there once, after the headers above it in that file's
 * list (it uses their names, and rtcdev's through the file's using-directive). */
#pragma once

/* Error bounds for the primary filter (u = 2^-24, |d_i| <= 1 + 2^-22 for a normalized float direction).
 * Reference det: h = cross(d, AC) then a 3-term dot -> |det_e - d.(AC x AB)| <= 5.001 u |AB|_1 |AC|_1.
 * Filter det: FMA dot with Gd rounded to float -> <= 4.004 u |AB|_1 |AC|_1.  Same with s0 for uu; vv uses q0
 * (exact) on both sides (<= 6.002 u |q0|_1); nd uses N on both sides (<= 6.002 u |N|_1).  For u+v > 1 the
 * filter forms w~ = (det~ - u~) - v~ (two more roundings, <= 2.0001 u (|det~| + |u~| + |v~|)) and the
 * reference rejects once sigma*(det - uu - vv) < -2^-21 |det| (three roundings), so that edge carries the
 * three bounds above, the subtraction error and 2^-21 |AB|_1 |AC|_1 (>= |det|).  Every bound is taken 4x and rounded up; the sign tests also carry 2^-60
 * so a product that could round to -0 is never treated as negative. */
__global__ __launch_bounds__(64) void rtc_prep_primary(const DevTri *__restrict__ tris, DevPrimF *__restrict__ pf,
                                                        DevPrimX *__restrict__ px, int triCount, V3 origin,
                                                        int *__restrict__ geoCount)
{
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (geoCount && blockIdx.x == 0 && threadIdx.x < kGeoLists) /* the launch's geometry sub-lists start empty */
        geoCount[threadIdx.x * kGeoCountStride] = 0;
    if (t >= triCount)
        return;
    const DevTri T = tris[t];
    const V3 AB{T.abx, T.aby, T.abz}, AC{T.acx, T.acy, T.acz}, N{T.nx, T.ny, T.nz};
    const V3 s0 = sub(origin, V3{T.ax, T.ay, T.az}); /* raytracing.c:198 */
    const V3 q0 = cross(s0, AB);                      /* :202 */
    const float dac0 = dot(AC, q0);                   /* :206 numerator */
    DevPrimX x;
    x.abx = AB.x, x.aby = AB.y, x.abz = AB.z;
    x.acx = AC.x, x.acy = AC.y, x.acz = AC.z;
    x.s0x = s0.x, x.s0y = s0.y, x.s0z = s0.z;
    x.q0x = q0.x, x.q0y = q0.y, x.q0z = q0.z;
    x.dac0 = dac0;
    x.pad[0] = x.pad[1] = x.pad[2] = 0.f;
    px[t] = x;

    /* exact-math direction vectors, in double, then rounded to float */
    const double abx = AB.x, aby = AB.y, abz = AB.z, acx = AC.x, acy = AC.y, acz = AC.z;
    const double sx = s0.x, sy = s0.y, sz = s0.z;
    const double gdx = acy * abz - acz * aby, gdy = acz * abx - acx * abz, gdz = acx * aby - acy * abx;
    const double gux = acy * sz - acz * sy, guy = acz * sx - acx * sz, guz = acx * sy - acy * sx;
    auto n1 = [](double a, double b, double c) { return fabs(a) + fabs(b) + fabs(c); };
    const double u = 5.9604644775390625e-08; /* 2^-24 */
    const double nAB = n1(abx, aby, abz), nAC = n1(acx, acy, acz), nS = n1(sx, sy, sz);
    const double nQ = n1(q0.x, q0.y, q0.z), nN = n1(N.x, N.y, N.z);
    const double eD = 9.006 * u * nAB * nAC;
    const double eU = 9.006 * u * nS * nAC;
    const double eV = 6.002 * u * nQ;
    const double eW = eD + eU + eV + 2.0002 * u * (nAB * nAC + nS * nAC + nQ) + 4.8e-7 * nAB * nAC;
    const double tiny = 8.673617379884035e-19; /* 2^-60 */
    const double m = fmax(fmax(eU, eV), eW) * 4.0 + tiny;
    const double ed = eD * 4.0;
    const double mnd = 6.002 * u * nN * 4.0;
    /* gigantic or non-finite geometry: disable the filter for this triangle (zero vectors and infinite
     * margins: every finite direction is a candidate and the exact path decides) */
    const bool sane = ed < 2.5e-4 && nAB * nAC < 1e30 && nS * nAC < 1e30 && nQ < 1e30 && m < 1e30 && mnd < 1e30;
    /* dAC0 == 0 (or NaN): dst is 0 or NaN for every ray, which the reference never records */
    const bool never = !(dac0 < 0.f || dac0 > 0.f);
    const float sg = dac0 < 0.f ? -1.f : 1.f;
    DevPrimF f;
    f.nx = N.x, f.ny = N.y, f.nz = N.z;
    f.gdx = sane ? sg * (float)gdx : 0.f, f.gdy = sane ? sg * (float)gdy : 0.f, f.gdz = sane ? sg * (float)gdz : 0.f;
    f.gux = sane ? sg * (float)gux : 0.f, f.guy = sane ? sg * (float)guy : 0.f, f.guz = sane ? sg * (float)guz : 0.f;
    f.q0x = sane ? sg * q0.x : 0.f, f.q0y = sane ? sg * q0.y : 0.f, f.q0z = sane ? sg * q0.z : 0.f;
    f.pad0 = 0.f;
    /* margins rounded outwards to float: sigma*det >= 0.001f (float EPSILON compare, raytracing.c:195) and
     * |det~ - det| <= ed give sigma*det~ >= 0.001f - ed >= c */
    f.mnd = never ? -__builtin_inff() : (sane ? __double2float_ru(mnd) : __builtin_inff());
    f.c = sane ? __double2float_rd((double)0.001f - ed) : -__builtin_inff();
    f.negm = sane ? -__double2float_ru(m) : -__builtin_inff();
    pf[t] = f;
}

struct Closest {
    float dst;
    int idx; /* -1 none; 0..S-1 sphere; S.. triangle (S + t) */
};

/* Exact-safe rejection filter.  With r = rcp(det) (<= 1 ulp) the approximations ua = uu*r, va = vv*r,
 * da = dd*r are within 2^-21 relative of the reference's u, v, dst (raytracing.c:197-207, invDet = 1/det
 * rounded), so each failed comparison below implies the corresponding reference rejection:
 *   ua < -2^-60 => u < 0;  va < -2^-60 => v < 0;  ua+va > 1+1e-5 (ua, va >= -2^-60) => u+v > 1 or u > 1;
 *   da < 0.00099 => dst < EPSILON.
 * The 2^-60 floor keeps the sign tests away from products that could round to -0 (no rejection in the
 * reference).  Every comparison is written so that NaN keeps the lane a candidate: the exact path then
 * decides as the reference does. */
constexpr float kTiny = 8.67361738e-19f; /* 2^-60 */




/* Primary segments (every live lane at bounce 0, pos == camera origin).
 * Filter (per lane, 13 VALU for a front-facing record, 4 for a back-facing one): FMA dot products of the
 * direction with the orientation-folded DevPrimF vectors (sigma = sign(dAC0), see DevPrimF); reject when the
 * bounds prove the reference rejects:
 *   nd > mnd                        => dot(dir, N) > 0                          (raytracing.c:189)
 *   sigma*det~ < c = EPSILON - ed   => |det| < EPSILON or sign(det) != sigma (then dst < 0)   (:195, :206)
 *   min(sigma*u~, sigma*v~, sigma*w~) < -m => u < 0, v < 0 or u+v > 1       (:200-204)
 * The exact reference arithmetic runs only for lanes the filter keeps (NaN directions are never kept:
 * their det is NaN, so the reference cannot record a hit either).  Records are scalar-loaded in batches.
 * prim_backfacing / prim_pass (rtc_layout.h) are THE filter: the render kernel and rtc_tile_cull both use them, and
 * rtc_probe_primary_cull returns their verdicts for tests/test_gpu_primary_cull.py. */

/* One primary record (see closest_primary). */
__device__ __forceinline__ void primary_test(const RenderParams &P, V3 dir, const DevPrimF &F, int t, int base,
                                             Closest &c)
{
    if (!prim_backfacing(dir, F)) {
        if (prim_pass(dir, F)) {
            /* the reference's arithmetic (raytracing.c:189-208) */
            const DevPrimX X = P.primX[t];
            if (!(dot(dir, V3{F.nx, F.ny, F.nz}) >= 0.f)) {
                const V3 h = cross(dir, V3{X.acx, X.acy, X.acz});
                const float det = dot(V3{X.abx, X.aby, X.abz}, h);
                if (!(-kEps < det && det < kEps)) {
                    const float invDet = rcp_cr(det); /* IEEE 1.f / det */
                    const float u = dot(V3{X.s0x, X.s0y, X.s0z}, h) * invDet;
                    const float v = dot(dir, V3{X.q0x, X.q0y, X.q0z}) * invDet;
                    const float dst = X.dac0 * invDet;
                    if (!(u < 0.f || u > 1.f) && !(v < 0.f || u + v > 1.f) && !(dst < kEps) && dst < c.dst) {
                        c.dst = dst;
                        c.idx = base + t;
                    }
                }
            }
        }
    }
}

/* Brute force over every record (RTC_F_NO_TILE_CULL).  Records are scalar-loaded in two alternating
 * batches of kUnroll: the next batch is in flight while the current one is tested (the arrays carry 8 spare
 * records so the last prefetch stays in bounds). */
__device__ __forceinline__ void closest_primary(const RenderParams &P, V3 dir, Closest &c, int base)
{
    const DevPrimF *rec = P.primF;
    DevPrimF A[kUnroll], B[kUnroll];
#pragma unroll
    for (int k = 0; k < kUnroll; ++k)
        A[k] = rec[k];
    for (int t0 = 0; t0 < P.triPadded; t0 += 2 * kUnroll, rec += 2 * kUnroll) {
#pragma unroll
        for (int k = 0; k < kUnroll; ++k)
            B[k] = rec[kUnroll + k];
#pragma unroll
        for (int k = 0; k < kUnroll; ++k)
            primary_test(P, dir, A[k], t0 + k, base, c);
#pragma unroll
        for (int k = 0; k < kUnroll; ++k)
            A[k] = rec[2 * kUnroll + k];
#pragma unroll
        for (int k = 0; k < kUnroll; ++k)
            primary_test(P, dir, B[k], t0 + kUnroll + k, base, c);
    }
}

/* Only the tile's candidates (rtc_tile_cull), in ascending index order, so ties keep the lowest index as
 * calculateRayCollision's strict `<` does (raytracing.c:231).  `mask` is wave-uniform: the bit-set words
 * and the records are scalar loads. */
__device__ __forceinline__ void closest_primary_listed(const RenderParams &P, V3 dir, Closest &c, int base,
                                                       const unsigned long long *__restrict__ mask)
{
    for (int w = 0; w < P.maskWords; ++w) {
        unsigned long long m = mask[w];
        while (m) {
            const int t = w * 64 + __builtin_ctzll(m);
            m &= m - 1;
            primary_test(P, dir, P.primF[t], t, base, c);
        }
    }
}

/* General segments (any origin): rayTriangle (raytracing.c:186-214) with AB, AC precomputed.
 * general_filter: the exact-safe rejection (backface, |det| < EPSILON, u out of range by the rcp estimate);
 * general_exact: the reference's arithmetic for a record the filter keeps (recomputes the same values). */
__device__ __forceinline__ bool general_filter(V3 pos, V3 dir, const DevTri &R)
{
    const float nd = dot(dir, V3{R.nx, R.ny, R.nz});
    const V3 AB{R.abx, R.aby, R.abz}, AC{R.acx, R.acy, R.acz};
    const V3 h = cross(dir, AC);
    const float det = dot(AB, h);
    const V3 s = sub(pos, V3{R.ax, R.ay, R.az});
    const float uu = dot(s, h);
    const float ua = uu * __builtin_amdgcn_rcpf(det);
    const bool detOk = !(-kEps < det && det < kEps);
    return (int)!(nd >= 0.f) & (int)detOk & (int)!(ua < -kTiny) & (int)!(ua > 1.000001f);
}

__device__ __forceinline__ void general_exact(V3 pos, V3 dir, const DevTri &R, int idx, Closest &c)
{
    const V3 AB{R.abx, R.aby, R.abz}, AC{R.acx, R.acy, R.acz};
    const V3 h = cross(dir, AC);
    const float det = dot(AB, h);
    const V3 s = sub(pos, V3{R.ax, R.ay, R.az});
    const float invDet = rcp_cr(det); /* IEEE 1.f / det */
    const float u = dot(s, h) * invDet;
    const V3 q = cross(s, AB);
    const float v = dot(dir, q) * invDet;
    const float dst = dot(AC, q) * invDet;
    /* records may be visited out of index order (clusters): equal distances keep the lowest index, as the
     * reference's strict `<` over ascending indices does (raytracing.c:231) */
    if (!(u < 0.f || u > 1.f) && !(v < 0.f || u + v > 1.f) && !(dst < kEps) &&
        (dst < c.dst || (dst == c.dst && (unsigned)idx < (unsigned)c.idx))) {
        c.dst = dst;
        c.idx = idx;
    }
}

__device__ __forceinline__ void general_test(V3 pos, V3 dir, const DevTri &R, int idx, Closest &c)
{
    const float nd = dot(dir, V3{R.nx, R.ny, R.nz});
    if (!(nd >= 0.f)) {
        const V3 AB{R.abx, R.aby, R.abz}, AC{R.acx, R.acy, R.acz};
        const V3 h = cross(dir, AC);
        const float det = dot(AB, h);
        const V3 s = sub(pos, V3{R.ax, R.ay, R.az});
        const float uu = dot(s, h);
        const float r = __builtin_amdgcn_rcpf(det);
        const float ua = uu * r;
        const bool detOk = !(-kEps < det && det < kEps);
        if (detOk & !(ua < -kTiny) & !(ua > 1.000001f)) {
            const float invDet = rcp_cr(det); /* IEEE 1.f / det */
            const float u = uu * invDet;
            const V3 q = cross(s, AB);
            const float v = dot(dir, q) * invDet;
            const float dst = dot(AC, q) * invDet;
            if (!(u < 0.f || u > 1.f) && !(v < 0.f || u + v > 1.f) && !(dst < kEps) && dst < c.dst) {
                c.dst = dst;
                c.idx = idx;
            }
        }
    }
}

/* Scenes up to kLdsTris triangles keep their general-path records in LDS (one copy per workgroup, loaded at
 * kernel start): the general loop then reads them as broadcast ds_read_b128 instead of scalar loads that
 * compete for the scalar cache with the primary records. */
constexpr int kLdsTris = 256;

__device__ __forceinline__ void closest_general_lds(const DevTri *__restrict__ lds, int Tp, V3 pos, V3 dir,
                                                    Closest &c, int base)
{
    for (int t0 = 0; t0 < Tp; t0 += 2) {
        const DevTri R0 = lds[t0], R1 = lds[t0 + 1];
        general_test(pos, dir, R0, base + t0, c);
        general_test(pos, dir, R1, base + t0 + 1, c);
    }
}

__device__ __forceinline__ void closest_general(const RenderParams &P, V3 pos, V3 dir, Closest &c, int base)
{
    const int Tp = P.triPadded;
    /* two alternating scalar-load batches, as closest_primary: the next records are in flight while the
     * current ones are tested (the arrays carry 8 spare records) */
    const DevTri *rec = P.tris;
    DevTri A[kUnroll], B[kUnroll];
#pragma unroll
    for (int k = 0; k < kUnroll; ++k)
        A[k] = rec[k];
    for (int t0 = 0; t0 < Tp; t0 += 2 * kUnroll, rec += 2 * kUnroll) {
#pragma unroll
        for (int k = 0; k < kUnroll; ++k)
            B[k] = rec[kUnroll + k];
#pragma unroll
        for (int k = 0; k < kUnroll; ++k)
            general_test(pos, dir, A[k], base + t0 + k, c);
#pragma unroll
        for (int k = 0; k < kUnroll; ++k)
            A[k] = rec[2 * kUnroll + k];
#pragma unroll
        for (int k = 0; k < kUnroll; ++k)
            general_test(pos, dir, B[k], base + t0 + kUnroll + k, c);
    }
}

/* calculateRayCollision (raytracing.c:216-240): spheres first (only if !trianglesOnly), then triangles
 * in index order; a candidate replaces the current one only if strictly closer (ties keep the lower
 * index).  The loop trip counts are kernel arguments, so the triangle index is wave-uniform and its
 * record is fetched with scalar loads.  `primaryWave` (wave-uniform) = every live lane is at bounce 0;
 * `mask` (wave-uniform, nullable) = the tile's primary candidates. */
template <bool SPHERES>
__device__ __forceinline__ Closest closest_hit(const RenderParams &P, V3 pos, V3 dir, bool primaryWave,
                                               const unsigned long long *mask, const DevTri *lds)
{
    Closest c{999999.f, -1};
    if (SPHERES) {
        for (int i = 0; i < P.sphereCount; ++i) {
            const DevSphere sp = P.spheres[i];
            float d;
            if (ray_sphere(pos, dir, V3{sp.cx, sp.cy, sp.cz}, sp.radius, d) && d < c.dst) {
                c.dst = d;
                c.idx = i;
            }
        }
    }
    const int base = SPHERES ? P.sphereCount : 0;
    if (primaryWave) {
        if (mask)
            closest_primary_listed(P, dir, c, base, mask);
        else
            closest_primary(P, dir, c, base);
    } else if (lds) {
        closest_general_lds(lds, P.triPadded, pos, dir, c, base);
    } else {
        closest_general(P, pos, dir, c, base);
    }
    return c;
}
