/* rtc_first_hit.h -- rtc_first_hit: the closest hit of every pixel's primary ray as buffers (rtc_render_first_hit_async,
 * DESIGN §3.10): calculateRayCollision (raytracing.c:216-240) on the ray of main.c:88-94, once per pixel, no samples.
 * A section of rtc_render.hip's translation unit: included there once, after the headers above it in that file's
 * list (it uses their names, and rtcdev's through the file's using-directive). */
#pragma once

/* A closest-hit query's result (a Closest's idx and dst: idx < sphereCount a sphere, else sphereCount + triangle; -1 a
 * miss) as the four buffers' values at element o, each buffer nullable -- the one statement of the encoding described
 * below, shared by rtc_first_hit and rtc_trace_rays (rtc_trace_rays.h).  P: the kernel's arguments, of which tris, mats,
 * spheres and sphereCount are read (RenderParams, TraceRaysArgs); (pos, dir): the ray the query traced, for a sphere's
 * normal.  (idx and dst are passed apart and in this order: rtc_first_hit then compiles to the code it had before the
 * function was taken out of it, instruction for instruction -- tools/kernel_diff.py.) */
template <bool SPHERES, typename PT>
__device__ __forceinline__ void store_hit(const PT &P, V3 pos, V3 dir, const int idx, const float dst, size_t o,
                                          int *__restrict__ prim, float *__restrict__ depth, float *__restrict__ normal,
                                          float *__restrict__ albedo)
{
    int winner = -1;
    V3 n{0.f, 0.f, 0.f}, color{0.f, 0.f, 0.f};
    if (idx >= 0) {
        if (SPHERES && idx < P.sphereCount) {
            const DevSphere sp = P.spheres[idx];
            const V3 hitPoint = add(pos, mul(dir, dst));            /* raytracing.c:181 */
            n = normalized(sub(hitPoint, V3{sp.cx, sp.cy, sp.cz})); /* :182 */
            color = V3{sp.r, sp.g, sp.b};
            winner = -2 - idx;
        } else {
            winner = idx - (SPHERES ? P.sphereCount : 0);
            const DevTri T = P.tris[winner];
            const DevMat M = P.mats[winner];
            n = V3{T.nx, T.ny, T.nz};
            color = V3{M.r, M.g, M.b};
        }
    }
    if (prim)
        prim[o] = winner;
    if (depth)
        depth[o] = dst;
    if (normal) {
        normal[3 * o] = n.x;
        normal[3 * o + 1] = n.y;
        normal[3 * o + 2] = n.z;
    }
    if (albedo) {
        albedo[3 * o] = color.x;
        albedo[3 * o + 1] = color.y;
        albedo[3 * o + 2] = color.z;
    }
}

/* One lane per pixel, the one-lane-per-pixel kernel's geometry in raster order (block_xy with P.order null, pixel_ray,
 * wave_tile): a wave is an 8x8 tile, its candidate words (rtc_tile_cull; P.tileMask null: every record, closest_primary)
 * are wave-uniform and the records scalar loads.  The query is closest_hit's primary one -- spheres first, then the
 * tile's triangles in ascending index, strict `<` -- so the winner and its distance are the render kernels' own, and
 * the exactness argument is rtc_closest.h's.  Spheres are tested per lane whatever the tile's words say: the words
 * come from the triangle cull alone.  A tile without a candidate word and without spheres tests nothing.
 * The four outputs are separate arguments, each nullable; pixel (launch row r, x) lies at r * width + x, as in dAccum.
 *   prim:   triangle t >= 0, sphere i as -2 - i, a miss -1 (the CPU oracle's `winner`)
 *   depth:  closest.dst; 999999.f on a miss
 *   normal: the triangle's stored normal, or normalized(hitPoint - centre) (raytracing.c:181-182); +0 on a miss
 *   albedo: closest.mat.color; +0 on a miss
 * Stores: plain per-lane dword stores (a wave's eight pixels of a row are 32 B of prim / depth and 96 B of a float3
 * array, adjacent); the kernel's time is the candidate tests' (DESIGN §3.10). */
template <bool SPHERES>
__global__ __launch_bounds__(kBlock) void rtc_first_hit(RenderParams P, int *__restrict__ prim, float *__restrict__ depth,
                                                        float *__restrict__ normal, float *__restrict__ albedo)
{
    int bx, by;
    block_xy(P, bx, by);
    const PixelRay px = pixel_ray(P, bx, by);
    const unsigned long long *tmask = nullptr;
    bool work = SPHERES || P.triPadded > 0; /* (wave-uniform) */
    if (P.tileMask) {
        tmask = P.tileMask + (size_t)wave_tile(bx, by) * P.maskWords;
        unsigned long long any = 0ull;
        for (int w = 0; w < P.maskWords; ++w)
            any |= tmask[w];
        work = SPHERES || any != 0ull;
    }
    Closest c{999999.f, -1}; /* HitInfo closest = {0, 999999} */
    if (work && px.valid)
        c = closest_hit<SPHERES>(P, P.origin, px.dir, true, tmask, nullptr);
    if (!px.valid)
        return;
    store_hit<SPHERES>(P, P.origin, px.dir, c.idx, c.dst, (size_t)px.r * (size_t)P.width + (size_t)px.x, prim, depth,
                       normal, albedo);
}
