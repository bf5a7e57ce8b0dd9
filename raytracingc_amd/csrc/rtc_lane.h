/* rtc_lane.h -- rtc_render_kernel: one lane per pixel (the launches that are not split, and the debug colours).
 * A section of rtc_render.hip's translation unit: included there once, after the headers above it in that file's
 * list (it uses their names, and rtcdev's through the file's using-directive). */
#pragma once

/* RESUME (a pass of rtc_render_samples_async): the lane's RNG state and accumulator are loaded before the
 * sample loop when the pass is not the frame's first, and stored after it; P.spp is the pass's sample count. */
template <bool SPHERES, bool DEBUG, bool RESUME = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(1))) void rtc_render_kernel(
    RenderParams P)
{
#ifdef RTC_DIAG
    const unsigned long long diagT0 = __builtin_amdgcn_s_memtime();
    unsigned diagIters = 0;
    unsigned long long diagTrace = 0;
#endif
    const int lane = threadIdx.x & 63;
    int bx, by;
    block_xy(P, bx, by);
    const PixelRay px = pixel_ray(P, bx, by);
    const int x = px.x, r = px.r, y = px.y;
    const bool valid = px.valid;
    const V3 pdir = px.dir;
    unsigned rng = (unsigned)(x + y * P.width); /* main.c:95 */

    /* general-path records in LDS (small scenes) and the powf tables */
    __shared__ DevTri sTris[kLdsTris];
    __shared__ PowTablesLds sPow;
    const bool useLds = P.triPadded <= kLdsTris;
    if (useLds) {
        for (int i = threadIdx.x; i < P.triPadded; i += kBlock)
            sTris[i] = P.tris[i];
    }
    sPow.fill(threadIdx.x);
    __syncthreads();
    sPow.attach(P.env);
    const DevTri *lds = useLds ? sTris : nullptr;

    /* this wave's primary candidates (rtc_tile_cull) */
    const unsigned long long *tmask = nullptr;
    unsigned listLen = (unsigned)P.triCount;
    if (P.tileMask) {
        tmask = P.tileMask + (size_t)wave_tile(bx, by) * P.maskWords;
        listLen = 0;
        for (int w = 0; w < P.maskWords; ++w)
            listLen += (unsigned)__popcll(tmask[w]);
    }

    V3 acc{0.f, 0.f, 0.f};
    if constexpr (RESUME) {
        if (valid && P.sampleFirst > 0) { /* the reference's rngState and accumulatedColor after sampleFirst samples */
            const size_t o = (size_t)r * (size_t)P.width + (size_t)x;
            rng = P.rngState[o];
            acc = V3{P.accum[3 * o], P.accum[3 * o + 1], P.accum[3 * o + 2]};
        }
    }
    bool alive = valid && P.spp > 0 && P.maxBounce > 0;
    if (DEBUG && valid && !(P.maxBounce > 0)) {
        /* calcDebugColor with no bounce loop returns lerp(BLACK, WHITE, 0 / (float)maxBounce) */
        const float t = 0.f / (float)P.maxBounce;
        const V3 g = lerp(V3{0.f, 0.f, 0.f}, V3{1.f, 1.f, 1.f}, t);
        for (int i = 0; i < P.spp; ++i)
            acc = add(acc, mul(g, P.invSpp));
    }
    int sample = 0, bounce = 0;
    V3 pos = P.origin, dir = pdir, rayColor{1.f, 1.f, 1.f}, light{0.f, 0.f, 0.f};
    unsigned segCalls = 0, segTraced = 0;
    unsigned long long segTests = 0;

    /* Sky tile (wave-uniform): no triangle is a primary candidate anywhere in this 8x8 tile and there are
     * no spheres, so calculateRayCollision over the tile's (empty) candidate list misses for every primary
     * ray here, and every sample of calcColor is that one miss: light = 0 + env(dir) * (1,1,1)
     * (raytracing.c:268-293), acc += light * (float)(1/spp) (main.c:99).  Same operations as the state
     * machine below, without its per-segment bookkeeping; the sample loop is unrolled for ILP. */
    const bool skyTile = !DEBUG && !SPHERES && P.tileMask && listLen == 0;
    if (skyTile) {
        if (alive) {
#pragma unroll 2
            for (int s = 0; s < P.spp; ++s) {
                const V3 l = add(V3{0.f, 0.f, 0.f}, mulv(environment(pdir, P.env), V3{1.f, 1.f, 1.f}));
                acc = add(acc, mul(l, P.invSpp));
            }
            segCalls = (unsigned)P.spp;
            segTraced = P.hoist ? 1u : (unsigned)P.spp;
        }
        alive = false;
    }

    /* bit-exact primary-hit hoisting: the primary ray consumes no RNG, so its closest hit
     * is a function of the pixel; trace it once instead of once per sample. */
    Closest primary{999999.f, -1};
    if (P.hoist && alive) {
        primary = closest_hit<SPHERES>(P, pos, dir, true, tmask, lds);
        segTraced++;
        segTests += listLen;
    }

    while (__any(alive)) {
#ifdef RTC_DIAG
        diagIters++;
#endif
        /* wave-uniform: every live lane that traces this iteration is at bounce 0 (origin = camera) */
        const bool needTrace = alive && !(P.hoist && bounce == 0);
        const bool primaryWave = __all(!needTrace || bounce == 0);
        if (alive) {
            Closest c;
            segCalls++;
            if (!needTrace) {
                c = primary;
            } else {
#ifdef RTC_DIAG
                const unsigned long long dt0 = __builtin_amdgcn_s_memtime();
#endif
                c = closest_hit<SPHERES>(P, pos, dir, primaryWave, tmask, lds);
#ifdef RTC_DIAG
                diagTrace += __builtin_amdgcn_s_memtime() - dt0;
#endif
                segTraced++;
                segTests += primaryWave ? listLen : (unsigned)P.triCount;
            }
            bool endSample;
            if (c.idx >= 0) {
                /* closest.hitPoint = ray.pos + ray.dir * closest.dst (raytracing.c:238) */
                const V3 hitPoint = add(pos, mul(dir, c.dst));
                V3 normal, color;
                float emission, smoothness;
                if (SPHERES && c.idx < P.sphereCount) {
                    const DevSphere sp = P.spheres[c.idx];
                    normal = normalized(sub(hitPoint, V3{sp.cx, sp.cy, sp.cz})); /* raytracing.c:182 */
                    color = V3{sp.r, sp.g, sp.b};
                    emission = sp.emission;
                    smoothness = sp.smoothness;
                } else {
                    const int t = c.idx - (SPHERES ? P.sphereCount : 0);
                    const DevTri T = P.tris[t];
                    const DevMat M = P.mats[t];
                    normal = V3{T.nx, T.ny, T.nz};
                    color = V3{M.r, M.g, M.b};
                    emission = M.emission;
                    smoothness = M.smoothness;
                }
                /* calcColor hit branch, raytracing.c:274-287 (calcDebugColor :251-254 shares the first part) */
                const V3 diffuseDir = normalized(add(normal, random_direction(rng)));
                const V3 specularDir = reflect(dir, normal);
                dir = lerp(diffuseDir, specularDir, smoothness);
                pos = hitPoint;
                if (DEBUG) {
                    bounce++;
                    endSample = bounce >= P.maxBounce;
                    if (endSample)
                        light = lerp(V3{0.f, 0.f, 0.f}, V3{1.f, 1.f, 1.f}, (float)bounce / (float)P.maxBounce);
                } else {
                const V3 emitted = mul(color, emission);
                light = add(light, mulv(emitted, rayColor));
                rayColor = mulv(rayColor, color);
                const float p = fmax_ref(fmax_ref(rayColor.x, rayColor.y), rayColor.z);
                endSample = p < random_value(rng);
                if (!endSample) {
                    rayColor = mul(rayColor, rcp_cr(p)); /* (float)(1.0 / p) */
                    bounce++;
                    endSample = bounce >= P.maxBounce;
                }
                }
            } else if (DEBUG) {
                /* calcDebugColor: first miss ends the sample with lerp(BLACK, WHITE, i / (float)maxBounce) */
                light = lerp(V3{0.f, 0.f, 0.f}, V3{1.f, 1.f, 1.f}, (float)bounce / (float)P.maxBounce);
                endSample = true;
            } else {
                /* miss branch, raytracing.c:291 */
                light = add(light, mulv(environment(dir, P.env), rayColor));
                endSample = true;
            }
            if (endSample) {
                /* main.c:99: acc = acc + calcColor(...) * (float)(1./spp) */
                acc = add(acc, mul(light, P.invSpp));
                sample++;
                if (sample >= P.spp) {
                    alive = false;
                } else {
                    pos = P.origin;
                    dir = pdir;
                    rayColor = V3{1.f, 1.f, 1.f};
                    light = V3{0.f, 0.f, 0.f};
                    bounce = 0;
                }
            }
        }
    }

    if (valid) {
        const size_t o = (size_t)r * (size_t)P.width + (size_t)x;
        /* vec3ToColor (raytracing.c:11-15) fused */
        P.colors[3 * o] = float_to_u8(acc.x);
        P.colors[3 * o + 1] = float_to_u8(acc.y);
        P.colors[3 * o + 2] = float_to_u8(acc.z);
        if (P.accum) {
            P.accum[3 * o] = acc.x;
            P.accum[3 * o + 1] = acc.y;
            P.accum[3 * o + 2] = acc.z;
        }
        if constexpr (RESUME)
            P.rngState[o] = rng; /* a pixel without a hit drew nothing: its seed */
    }
#ifdef RTC_DIAG
    if (g_rtc_diag && lane == 0) {
        const int wave = threadIdx.x >> 6;
        const size_t w = ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (kBlock / 64) + wave;
        g_rtc_diag[4 * w] = __builtin_amdgcn_s_memtime() - diagT0;
        g_rtc_diag[4 * w + 1] = diagIters;
        g_rtc_diag[4 * w + 2] = diagT0;
        g_rtc_diag[4 * w + 3] = diagTrace;
    }
#endif
    flush_counters(P, segCalls, segTraced, segTests, lane);
}
