/* rtc_render_pixels.h -- rtc_render_pixels: a pass over a list of pixels of a progressive frame (rtc_render_pixels_async,
 * DESIGN §3.17): main.c:88-100 for the listed pixels alone -- per pixel, the camera ray of main.c:88-94, the state of
 * main.c:95 or the frame's stored one, sampleCount times acc = acc + calcColor(ray, trianglesOnly, maxBounce, scene) *
 * (float)(1. / spp), and the pixel's 16 bytes of state and 3 bytes of Color stored where a whole pass keeps them.
 * A section of rtc_render.hip's translation unit: included there once, after rtc_trace_paths.h (it uses rtc_trace_rays.h's
 * trace_closest and the names of the headers above it in that file's list, and rtcdev's through the file's
 * using-directive).
 * The two kernels are rtc_trace_paths and rtc_trace_paths_wave with another head (the pixel index, the derived ray and
 * seed, the state load) and another tail (the state store, the three Color bytes).  Between the two their statements are
 * rtc_trace_paths.h's own, again: the shared bodies that were built measured slower (that file's comment). */
#pragma once

/* The kernel's own arguments: the record part of TracePathsArgs (the bound generation's records and their counts), the
 * environment, the sample range, the frame's pixel -> ray map with the camera origin, the frame's pixel count, the list
 * and the frame's three buffers with the caller's counter. */
struct RenderPixelsArgs {
    const DevTri *__restrict__ tris;         /* reference order, triPadded + 8 records */
    const DevMat *__restrict__ mats;
    const DevSphere *__restrict__ spheres;
    const DevTri *__restrict__ clTris;       /* cluster order, pad0 = reference index (-1: padding, a zero record) */
    const DevCluster *__restrict__ clusters;
    const DevCluster *__restrict__ chunks;
    int triPadded, sphereCount, clusterCount, chunkCount;
    EnvParams env;                           /* env_of(*scene); the kernel points its tables at the LDS copies */
    float invSpp;                            /* (float)(1. / spp), main.c:99 */
    int sampleFirst, sampleCount, maxBounce;
    PrimaryView view;                        /* the frame's: launch_row_y and primary_dir read it */
    V3 origin;                               /* cam->origin: every listed pixel's ray starts there */
    unsigned pixelCount;                     /* rows * width: an index at or past it is skipped */
    const unsigned *__restrict__ pixels;     /* n compact indices p = launchRow * width + x */
    unsigned n;                              /* <= 0x7fffffff */
    unsigned char *colors;                   /* 3 pixelCount bytes, nullable: bytes 3 p .. 3 p + 2 of a listed pixel */
    float *accum;                            /* 3 pixelCount; read when sampleFirst > 0, written */
    unsigned *rngState;                      /* pixelCount; read when sampleFirst > 0, written */
    unsigned long long *segments;            /* one u64, nullable: += calculateRayCollision calls */
};

/* A listed pixel's camera ray direction and seed (main.c:88-95): x = p % width, launch row r = p / width, image row
 * y = launch_row_y(r) */
__device__ __forceinline__ V3 listed_pixel_dir(const RenderPixelsArgs &A, unsigned p, unsigned &seed)
{
    const int x = (int)(p % (unsigned)A.view.width), r = (int)(p / (unsigned)A.view.width);
    const int y = launch_row_y(A.view, r);
    seed = (unsigned)(x + y * A.view.width); /* main.c:95 */
    return primary_dir(A.view, x, y);
}

/* the tail: the pixel's state where a whole pass keeps it and, where asked for, vec3ToColor (raytracing.c:11-15) of the sum
 * as three byte stores -- the neighbouring pixels' bytes share the Color's dwords and are not this launch's to touch */
__device__ __forceinline__ void store_listed_pixel(const RenderPixelsArgs &A, unsigned p, V3 acc, unsigned rng)
{
    const size_t o = (size_t)p;
    A.accum[3 * o] = acc.x;
    A.accum[3 * o + 1] = acc.y;
    A.accum[3 * o + 2] = acc.z;
    A.rngState[o] = rng; /* a pixel without a hit drew nothing: its seed */
    if (A.colors) {
        A.colors[3 * o] = float_to_u8(acc.x);
        A.colors[3 * o + 1] = float_to_u8(acc.y);
        A.colors[3 * o + 2] = float_to_u8(acc.z);
    }
}

/* One lane per listed pixel, a wave 64 consecutive entries of the list: rtc_trace_paths with the ray and the state taken
 * from the frame.  A lane past n, or whose index is not a pixel of the frame (p >= pixelCount: a stale list), loads and
 * stores nothing, is never alive and stays in the wave-wide operations.
 * A lane's result depends on its pixel's ray and state and on the scene alone: trace_closest's does not depend on the
 * other lanes' rays, and everything else is per lane -- which is why a listed pixel holds what a whole pass leaves there.
 * The only LDS is the powf tables (PowTablesLds).  The segment count is reduced over the wave and added once per wave. */
template <bool SPHERES, bool CULL>
__global__ __launch_bounds__(kBlock) void rtc_render_pixels(RenderPixelsArgs A)
{
    __shared__ PowTablesLds sPow;
    sPow.fill(threadIdx.x);
    __syncthreads();
    sPow.attach(A.env);

    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    unsigned p = 0;
    bool live = i < (size_t)A.n;
    if (live) {
        p = A.pixels[i];
        live = p < A.pixelCount;
    }
    const V3 pos0 = A.origin;
    V3 dir0{0.f, 0.f, 0.f}, acc{0.f, 0.f, 0.f};
    unsigned rng = 0;
    if (live) {
        dir0 = listed_pixel_dir(A, p, rng);
        if (A.sampleFirst > 0) { /* the reference's rngState and accumulatedColor after sampleFirst samples */
            rng = A.rngState[p];
            acc = V3{A.accum[3 * (size_t)p], A.accum[3 * (size_t)p + 1], A.accum[3 * (size_t)p + 2]};
        }
    }
    bool alive = live && A.maxBounce > 0;
    if (live && !alive) /* calcColor without a bounce loop returns +0: acc + 0 * invSpp, the same after one sample or many */
        acc = add(acc, mul(V3{0.f, 0.f, 0.f}, A.invSpp));
    int sample = 0, bounce = 0;
    V3 pos = pos0, dir = dir0, rayColor{1.f, 1.f, 1.f}, light{0.f, 0.f, 0.f};
    unsigned long long segCalls = 0;

    while (__any(alive)) {
        const Closest c = trace_closest<SPHERES, CULL>(A, pos, dir, alive);
        if (alive) {
            segCalls++;
            bool endSample;
            if (c.idx >= 0) {
                /* closest.hitPoint = ray.pos + ray.dir * closest.dst (raytracing.c:238) */
                const V3 hitPoint = add(pos, mul(dir, c.dst));
                V3 normal, color;
                float emission, smoothness;
                if (SPHERES && c.idx < A.sphereCount) {
                    const DevSphere sp = A.spheres[c.idx];
                    normal = normalized(sub(hitPoint, V3{sp.cx, sp.cy, sp.cz})); /* raytracing.c:182 */
                    color = V3{sp.r, sp.g, sp.b};
                    emission = sp.emission;
                    smoothness = sp.smoothness;
                } else {
                    const int t = c.idx - (SPHERES ? A.sphereCount : 0);
                    const DevTri R = A.tris[t];
                    const DevMat M = A.mats[t];
                    normal = V3{R.nx, R.ny, R.nz};
                    color = V3{M.r, M.g, M.b};
                    emission = M.emission;
                    smoothness = M.smoothness;
                }
                /* calcColor hit branch, raytracing.c:274-287 */
                const V3 diffuseDir = normalized(add(normal, random_direction(rng)));
                const V3 specularDir = reflect(dir, normal);
                dir = lerp(diffuseDir, specularDir, smoothness);
                pos = hitPoint;
                const V3 emitted = mul(color, emission);
                light = add(light, mulv(emitted, rayColor));
                rayColor = mulv(rayColor, color);
                const float q = fmax_ref(fmax_ref(rayColor.x, rayColor.y), rayColor.z);
                endSample = q < random_value(rng);
                if (!endSample) {
                    rayColor = mul(rayColor, rcp_cr(q)); /* (float)(1.0 / p) */
                    bounce++;
                    endSample = bounce >= A.maxBounce;
                }
            } else {
                /* miss branch, raytracing.c:291 */
                light = add(light, mulv(environment(dir, A.env), rayColor));
                endSample = true;
            }
            if (endSample) {
                /* main.c:99: acc = acc + calcColor(...) * (float)(1./spp) */
                acc = add(acc, mul(light, A.invSpp));
                sample++;
                if (sample >= A.sampleCount) {
                    alive = false;
                } else {
                    pos = pos0;
                    dir = dir0;
                    rayColor = V3{1.f, 1.f, 1.f};
                    light = V3{0.f, 0.f, 0.f};
                    bounce = 0;
                }
            }
        }
    }

    if (live)
        store_listed_pixel(A, p, acc, rng);
    if (A.segments) {
        for (int off = 32; off > 0; off >>= 1)
            segCalls += __shfl_xor(segCalls, off);
        if ((threadIdx.x & 63) == 0 && segCalls)
            atomicAdd(A.segments, segCalls);
    }
}

/* RTC_F_WAVE_PER_RAY: one wave per listed pixel, the pixel's samples on the wave's lanes -- rtc_trace_paths_wave (its
 * description and the argument for the walk: rtc_trace_paths.h) with the ray and the state taken from the
 * frame.  Lane j evaluates the candidate that starts 7 j draws after the pixel's state; the walk follows the reference's
 * chain in order.  Every wave-uniform value (p, S, acc, left, calls, k) is computed by all lanes alike; lane 0 stores.  A
 * wave past n, or whose index is not a pixel of the frame, takes part in the table fill and its barrier and leaves: it
 * loads and stores nothing. */
template <bool SPHERES, bool CULL>
__global__ __launch_bounds__(kBlock) void rtc_render_pixels_wave(RenderPixelsArgs A)
{
    __shared__ PowTablesLds sPow;
    sPow.fill(threadIdx.x);
    __syncthreads();
    sPow.attach(A.env);

    const size_t i = (size_t)blockIdx.x * (kBlock / 64) + (size_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (i >= (size_t)A.n)
        return;
    const unsigned p = (unsigned)__builtin_amdgcn_readfirstlane((int)A.pixels[i]);
    if (p >= A.pixelCount)
        return;
    const unsigned lane = threadIdx.x & 63u;
    unsigned S;
    const V3 pos0 = A.origin, dir0 = listed_pixel_dir(A, p, S);
    V3 acc{0.f, 0.f, 0.f};
    if (A.sampleFirst > 0) { /* the reference's rngState and accumulatedColor after sampleFirst samples */
        S = A.rngState[p];
        acc = V3{A.accum[3 * (size_t)p], A.accum[3 * (size_t)p + 1], A.accum[3 * (size_t)p + 2]};
    }
    int left = A.sampleCount;
    unsigned long long calls = 0;

    if (A.maxBounce <= 0) { /* calcColor without a bounce loop returns +0: acc + 0 * invSpp, as the lane kernel has it */
        acc = add(acc, mul(V3{0.f, 0.f, 0.f}, A.invSpp));
        left = 0;
    }
    /* every sample's first segment is the camera ray: traced once, counted per sample */
    Closest first{999999.f, -1};
    if (left > 0)
        first = trace_closest<SPHERES, CULL>(A, pos0, dir0, true);
    const RngJump laneJump = rng_jump_by(7u * lane); /* s -> the state 7 lane draws later */

    while (left > 0) {
        /* lane j > 0 can start one of the `left` samples only if j <= (left - 1) * maxBounce: a sample makes at most
         * maxBounce hits */
        bool alive = lane == 0 || (unsigned long long)lane <= (unsigned long long)(left - 1) * (unsigned long long)A.maxBounce;
        unsigned rng = S * laneJump.a + laneJump.c;
        int bounce = 0;
        unsigned hits = 0, segCalls = 0;
        V3 pos = pos0, dir = dir0, rayColor{1.f, 1.f, 1.f}, light{0.f, 0.f, 0.f};
        Closest c = first;
        for (;;) {
            if (alive) {
                segCalls++;
                bool endSample;
                if (c.idx >= 0) {
                    /* closest.hitPoint = ray.pos + ray.dir * closest.dst (raytracing.c:238) */
                    const V3 hitPoint = add(pos, mul(dir, c.dst));
                    V3 normal, color;
                    float emission, smoothness;
                    if (SPHERES && c.idx < A.sphereCount) {
                        const DevSphere sp = A.spheres[c.idx];
                        normal = normalized(sub(hitPoint, V3{sp.cx, sp.cy, sp.cz})); /* raytracing.c:182 */
                        color = V3{sp.r, sp.g, sp.b};
                        emission = sp.emission;
                        smoothness = sp.smoothness;
                    } else {
                        const int t = c.idx - (SPHERES ? A.sphereCount : 0);
                        const DevTri R = A.tris[t];
                        const DevMat M = A.mats[t];
                        normal = V3{R.nx, R.ny, R.nz};
                        color = V3{M.r, M.g, M.b};
                        emission = M.emission;
                        smoothness = M.smoothness;
                    }
                    /* calcColor hit branch, raytracing.c:274-287 */
                    hits++;
                    const V3 diffuseDir = normalized(add(normal, random_direction(rng)));
                    const V3 specularDir = reflect(dir, normal);
                    dir = lerp(diffuseDir, specularDir, smoothness);
                    pos = hitPoint;
                    const V3 emitted = mul(color, emission);
                    light = add(light, mulv(emitted, rayColor));
                    rayColor = mulv(rayColor, color);
                    const float q = fmax_ref(fmax_ref(rayColor.x, rayColor.y), rayColor.z);
                    endSample = q < random_value(rng);
                    if (!endSample) {
                        rayColor = mul(rayColor, rcp_cr(q)); /* (float)(1.0 / p) */
                        bounce++;
                        endSample = bounce >= A.maxBounce;
                    }
                } else {
                    /* miss branch, raytracing.c:291 */
                    light = add(light, mulv(environment(dir, A.env), rayColor));
                    endSample = true;
                }
                if (endSample)
                    alive = false;
            }
            if (!__any(alive))
                break;
            c = trace_closest<SPHERES, CULL>(A, pos, dir, alive);
        }

        /* the walk, in the reference's order */
        unsigned k = 0;
        while (left > 0 && k < 64u) {
            const V3 lk{__shfl(light.x, (int)k), __shfl(light.y, (int)k), __shfl(light.z, (int)k)};
            const unsigned hk = __shfl(hits, (int)k), ck = __shfl(segCalls, (int)k);
            /* main.c:99: acc = acc + calcColor(...) * (float)(1./spp) */
            const V3 term = mul(lk, A.invSpp);
            acc = add(acc, term);
            calls += ck;
            --left;
            if (hk == 0) {
                /* the sample drew nothing: every remaining sample starts from the same state and is this sample again.  Its
                 * adds one by one; once one leaves acc's bits as they were, so does every later one */
                calls += (unsigned long long)left * ck;
                for (; left > 0; --left) {
                    const V3 was = acc;
                    acc = add(acc, term);
                    if (__float_as_uint(acc.x) == __float_as_uint(was.x) && __float_as_uint(acc.y) == __float_as_uint(was.y) &&
                        __float_as_uint(acc.z) == __float_as_uint(was.z))
                        break;
                }
                left = 0;
            } else {
                k += hk;
            }
        }
        /* k may pass 64 (maxBounce 65, 100): the next window's lane 0 starts a real sample; 7 k mod 2^32 is the LCG's own
         * period */
        S = rng_advance(S, 7u * k);
    }

    if (lane == 0) {
        store_listed_pixel(A, p, acc, S);
        if (A.segments && calls)
            atomicAdd(A.segments, calls);
    }
}
