/* rtc_trace_paths.h -- rtc_trace_paths: the radiance along caller-supplied rays against the resident scene
 * (rtc_trace_paths_async): main.c:95-100 with the ray given instead of derived from a pixel -- per ray,
 * sampleCount times acc = acc + calcColor(ray, trianglesOnly, maxBounce, scene) * (float)(1. / spp) (raytracing.c:262-296)
 * on one RNG chain that starts at the caller's seed.
 * A section of rtc_render.hip's translation unit: included there once, after rtc_trace_rays.h (it uses that file's
 * trace_closest, the names of the headers above it in that file's list, and rtcdev's through the file's
 * using-directive). */
#pragma once

/* The kernel's own arguments: the record part of TraceRaysArgs (the bound generation's records and their counts), the
 * environment, the sample range and the five buffers. */
struct TracePathsArgs {
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
    const float *__restrict__ rays;          /* n Rays: pos.xyz, dir.xyz (24 B, 4-byte aligned) */
    unsigned n;                              /* <= 0x7fffffff */
    const unsigned *seeds;                   /* n; may be seedsOut (in place): not restrict */
    float *radiance;                         /* 3 n; read when sampleFirst > 0, written */
    unsigned *seedsOut;                      /* n; nullable */
    unsigned long long *segments;            /* one u64, nullable: += calculateRayCollision calls */
};

/* One lane per ray, a wave 64 consecutive rays; lanes past n load and store nothing, are never alive and stay in the
 * wave-wide operations.  rtc_lane.h's state machine without the camera, the tile masks, hoisting and DEBUG: while any
 * lane of the wave is alive every alive lane traces one segment -- trace_closest, the wave-wide part: the lanes that are
 * not alive run through it with a stale ray whose result is discarded -- and then takes the hit branch (raytracing.c:
 * 274-287, rtc_lane.h's arithmetic) or the miss branch (:291, environment).  At a sample's end acc = acc + light *
 * invSpp (main.c:99) and the lane restarts from its own ray, or dies after sampleCount samples.  The samples of one ray
 * are sequential (one RNG chain); a lane whose ray is done idles until the wave's last ray ends.
 * A lane's result depends on its ray and seed alone: trace_closest's does not depend on the other lanes' rays, and
 * everything else is per lane.
 * The only LDS is the powf tables (PowTablesLds).  The seed is read before the loop and written after it, so seedsOut
 * may be seeds.  The segment count is reduced over the wave and added once per wave. */
template <bool SPHERES, bool CULL>
__global__ __launch_bounds__(kBlock) void rtc_trace_paths(TracePathsArgs A)
{
    __shared__ PowTablesLds sPow;
    sPow.fill(threadIdx.x);
    __syncthreads();
    sPow.attach(A.env);

    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = i < (size_t)A.n;
    V3 pos0{0.f, 0.f, 0.f}, dir0{0.f, 0.f, 0.f}, acc{0.f, 0.f, 0.f};
    unsigned rng = 0;
    if (live) {
        const float *r = A.rays + 6 * i;
        pos0 = V3{r[0], r[1], r[2]};
        dir0 = V3{r[3], r[4], r[5]};
        rng = A.seeds[i];
        if (A.sampleFirst > 0) /* the accumulator after sampleFirst samples */
            acc = V3{A.radiance[3 * i], A.radiance[3 * i + 1], A.radiance[3 * i + 2]};
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
                    const DevTri T = A.tris[t];
                    const DevMat M = A.mats[t];
                    normal = V3{T.nx, T.ny, T.nz};
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
                const float p = fmax_ref(fmax_ref(rayColor.x, rayColor.y), rayColor.z);
                endSample = p < random_value(rng);
                if (!endSample) {
                    rayColor = mul(rayColor, rcp_cr(p)); /* (float)(1.0 / p) */
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

    if (live) {
        A.radiance[3 * i] = acc.x;
        A.radiance[3 * i + 1] = acc.y;
        A.radiance[3 * i + 2] = acc.z;
        if (A.seedsOut)
            A.seedsOut[i] = rng; /* a ray without a hit drew nothing: its seed */
    }
    if (A.segments) {
        for (int off = 32; off > 0; off >>= 1)
            segCalls += __shfl_xor(segCalls, off);
        if ((threadIdx.x & 63) == 0 && segCalls)
            atomicAdd(A.segments, segCalls);
    }
}

/* RTC_F_WAVE_PER_RAY: one wave per ray, the ray's samples on the wave's lanes.  A hit draws exactly 7 values
 * (RandomDiretion's six and the roulette's one, raytracing.c:274, 285) and a miss none, so every sample of a ray starts at
 * the seed advanced by a multiple of 7 draws.  In a window lane j evaluates the whole calcColor that starts at S advanced
 * by 7 j draws -- a candidate: a real sample only if an earlier real sample ends exactly there.  The walk then follows the
 * reference's chain in order: sample 0 is lane 0's, it made h hits, so the next sample is lane h's, and so on; the
 * accumulator takes the walked lights one f32 multiply and add at a time (main.c:99), as the lane kernel's does.  A lane's
 * result depends on the ray and on the state it starts from alone (trace_closest's does not depend on the other lanes'
 * rays), so a walked lane holds what the sequential chain computes there.
 * Every wave-uniform value (S, acc, left, calls, k) is computed by all lanes alike; lane 0 stores.  A wave past n takes part
 * in the table fill and its barrier and leaves.
 * The hit and miss statements are rtc_trace_paths' own, and rtc_render_pixels.h has both kernels' bodies again: one
 * calcColor step and one body per kind, called from all four, were built and measured -- the same
 * instructions in another register allocation, 0.5 to 1.3 % slower on three of this file's legs in both alternations, one
 * VGPR more in one pixel kernel -- so a change to the bounce step or the window loop is made in each of them. */
template <bool SPHERES, bool CULL>
__global__ __launch_bounds__(kBlock) void rtc_trace_paths_wave(TracePathsArgs A)
{
    __shared__ PowTablesLds sPow;
    sPow.fill(threadIdx.x);
    __syncthreads();
    sPow.attach(A.env);

    const size_t i = (size_t)blockIdx.x * (kBlock / 64) + (size_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (i >= (size_t)A.n)
        return;
    const unsigned lane = threadIdx.x & 63u;
    const float *r = A.rays + 6 * i;
    const V3 pos0{r[0], r[1], r[2]}, dir0{r[3], r[4], r[5]};
    unsigned S = A.seeds[i];
    V3 acc{0.f, 0.f, 0.f};
    if (A.sampleFirst > 0) /* the accumulator after sampleFirst samples */
        acc = V3{A.radiance[3 * i], A.radiance[3 * i + 1], A.radiance[3 * i + 2]};
    int left = A.sampleCount;
    unsigned long long calls = 0;

    if (A.maxBounce <= 0) { /* calcColor without a bounce loop returns +0: acc + 0 * invSpp, as the lane kernel has it */
        acc = add(acc, mul(V3{0.f, 0.f, 0.f}, A.invSpp));
        left = 0;
    }
    /* every sample's first segment is the ray as given: traced once, counted per sample */
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
                        const DevTri T = A.tris[t];
                        const DevMat M = A.mats[t];
                        normal = V3{T.nx, T.ny, T.nz};
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
                    const float p = fmax_ref(fmax_ref(rayColor.x, rayColor.y), rayColor.z);
                    endSample = p < random_value(rng);
                    if (!endSample) {
                        rayColor = mul(rayColor, rcp_cr(p)); /* (float)(1.0 / p) */
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
        A.radiance[3 * i] = acc.x;
        A.radiance[3 * i + 1] = acc.y;
        A.radiance[3 * i + 2] = acc.z;
        if (A.seedsOut)
            A.seedsOut[i] = S;
        if (A.segments && calls)
            atomicAdd(A.segments, calls);
    }
}
