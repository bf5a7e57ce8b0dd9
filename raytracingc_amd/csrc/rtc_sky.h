/* rtc_sky.h -- rtc_render_sky_rows: the sky pass of a split launch.
 * A section of rtc_render.hip's translation unit: included there once, after the headers above it in that file's
 * list (it uses their names, and rtcdev's through the file's using-directive). */
#pragma once

/* LDS writes of this wave visible to its other lanes (the wave is the only user of the region) */
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

/* The sky pass (rtc_render_sky_rows): every pixel whose primary ray provably misses, few registers, so many waves per SIMD
 * hide the latency of the environment's double-precision chains.  <= 64 VGPRs: two sky waves fit where one chain wave
 * retires (frame -1.5 %, round 4). */
#ifndef RTC_SKY_WAVES
#define RTC_SKY_WAVES 8
#endif
/* Sky pixels by row strips (round 5): each wave takes 64 consecutive pixels of one launch row (workgroups of
 * kSkyWaves waves: kSkyWaves consecutive rows), so a strip of Color is 192 B = three whole 64-B lines when the row starts
 * on a line (every BASELINE width: 1920 * 3 and 3840 * 3 are multiples of 64), written by twelve 16-B stores staged in
 * LDS.  The 8x8-tile waves wrote 24-B tile rows that straddle lines shared with the neighbouring tiles' waves, so every
 * line was written back partially two or three times (sky WRITE_SIZE 12.0 MB per 1080p launch for 6.0 MB of Color,
 * VERDICT r04 #5).  A strip holding geometry pixels (rtc_render_chain writes those, maybe concurrently) or cut by the frame
 * edge writes its sky pixels' bytes only.  Same pixels, same per-sample environment loop, same values.  kSkyWaves waves per
 * workgroup: 1, or 4 for small shares of more than 400 k pixels (one-wave workgroups fill the registers and wave slots
 * the co-resident chain workgroups leave free at a finer grain -- whole frames -1 %, the 1080p 1/8 share -2 % -- but
 * the 1/4 share took 3.5 % longer with them, profiles/r04_zd_ab_sky_wg.log). */
/* GENERAL (round 6): the launch may merge (P.geoColor), hoist, write the accumulator or count segments; the pipelined
 * faithful whole frames run an instantiation without that code (56 VGPRs and no SGPR spill instead of 59 and 8; since
 * round 11's specialised sample loops 62 and none instead of 59 and 28). */
/* RESUME (a pass of rtc_render_samples_async; GENERAL): the sum starts from the stored accumulator when the
 * pass is not the frame's first; the first pass writes the pixel's state, its seed x + y * width (a sky pixel draws
 * nothing, so later passes leave it).  The shortcuts and a sum that does not start at +0: the sun-term skip (sun_vanishes)
 * concerns e + sv alone, whatever it is added to; environment_miss_term needs a sum that is not -0, and the stored sum is
 * +0 plus such terms, which in round-to-nearest is never -0; the hoisted term is one value added P.spp times either way.
 * A pass never merges (geoColor's place holds rngState). */
/* The faithful sample loop with its path decided once per strip (round 11, RTC_SKY_PATHS; 0 builds the loop that calls
 * environment_miss_term, which decides every sample): a pixel's direction, the launch's environment and the strip's live
 * lanes are the same in every sample, so env_classify's wave-wide tests are made once before the loop, under its exec
 * mask, and the loop is one of environment_miss_body's instantiations behind one wave-uniform switch -- no ballot and no
 * choice of path per sample, and the unrolled copies interleave (RTC_SKY_UNROLL samples per iteration: DESIGN §3.3).  Every sample still runs the reference's arithmetic (both powf
 * cores from the tables, the lerps, the adds by zero beside a computed sun term, the sequential sum): sky_keep_per_sample
 * keeps the table reads, and with them all that follows from them, inside the loop now that no branch does, and the
 * path without a sky powf keeps its lerps there by an opaque +0 (environment_miss_body). */
#ifndef RTC_SKY_PATHS
#define RTC_SKY_PATHS 1
#endif
#ifndef RTC_SKY_UNROLL
#define RTC_SKY_UNROLL 2
#endif
/* a fence against the lane itself (no instruction): loads after it are not moved before it, so a loop's loads stay in it
 * (not an empty asm statement: device asm is convergent, and a loop with a convergent call is not unrolled) */
__device__ __forceinline__ void sky_keep_per_sample() { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "singlethread"); }

template <int SKY, int SUN, int UNROLL>
__device__ __forceinline__ V3 sky_samples(V3 acc, V3 dir, const EnvParams &env, int spp, float invSpp)
{
#pragma unroll UNROLL
    for (int s = 0; s < spp; ++s) {
        sky_keep_per_sample();
        /* raytracing.c:291 with rayColor (1, 1, 1): 0 + environment (environment_miss_term: acc starts at +0) */
        const V3 l = environment_miss_body<SKY, SUN>(dir, env);
        acc = add(acc, mul(l, invSpp)); /* main.c:99 */
    }
    return acc;
}
template <int UNROLL, int I = 0>
__device__ __forceinline__ V3 sky_samples_on(EnvPath p, V3 acc, V3 dir, const EnvParams &env, int spp, float invSpp)
{
    if constexpr (I + 1 < kEnvSkyPaths * kEnvSunPaths) {
        if (p.sky * kEnvSunPaths + p.sun != I) /* (wave-uniform) */
            return sky_samples_on<UNROLL, I + 1>(p, acc, dir, env, spp, invSpp);
    }
    /* (the path without a sky powf holds an asm statement, and a loop with one is not unrolled; its body is short) */
    return sky_samples<I / kEnvSunPaths, I % kEnvSunPaths, I / kEnvSunPaths == kSkyPowNone ? 1 : UNROLL>(acc, dir, env, spp,
                                                                                                        invSpp);
}

template <int kSkyWaves, bool GENERAL, bool RESUME = false>
__global__ __launch_bounds__(kSkyWaves * 64) __attribute__((amdgpu_waves_per_eu(RTC_SKY_WAVES))) void rtc_render_sky_rows(
    RenderParams P)
{
    static_assert(kSkyWaves == 4 || kSkyWaves == 1, "one or four row strips per workgroup");
    __shared__ PowTablesLds sPow;
    __shared__ __attribute__((aligned(16))) unsigned char sStrip[kSkyWaves][192];
    sPow.fill(threadIdx.x);
    __syncthreads();
    sPow.attach(P.env);
    const int lane = threadIdx.x & 63, lw = threadIdx.x >> 6;
    unsigned segCalls = 0, segTraced = 0;
    const int r = (int)blockIdx.y * kSkyWaves + __builtin_amdgcn_readfirstlane(lw); /* launch row (wave-uniform) */
    const int x = (int)blockIdx.x * 64 + lane;
    const bool inFrame = r < P.rows && x < P.width;
    /* the pixel's tile: pixels with a primary candidate are rtc_render_chain's (pixMask bit (row % 8) * 8 + x % 8) */
    bool geo = false;
    int t = 0;
    if (inFrame) {
        t = (r >> 3) * (P.blocksX * 2) + (x >> 3);
        geo = ((P.pixMask[t] >> (((r & 7) << 3) | (x & 7))) & 1ull) != 0ull;
    }
    const bool valid = inFrame && !geo; /* a sky pixel: this kernel renders it */
    /* merged (P.geoColor): the geometry kernel has finished; its pixels' bytes are written here too, so every strip is
     * whole lines.  Their words are requested now and used after the sky loop. */
    const bool merged = GENERAL && !RESUME && P.geoColor != nullptr; /* (uniform) */
    const bool writes = merged ? inFrame : valid;
    const unsigned long long mine = __ballot(writes);
    if (mine == 0ull)
        return;
    unsigned gw = 0;
    if (merged) {
        /* the geometry kernel's items are the sub-lists concatenated: entry pos of sub-list l is item (entries of the
         * sub-lists before l) + pos -- the exclusive prefix of the launch's counts, lane l holding sub-list l's */
        const int cnt = lane < kGeoLists ? min(P.geoCount[lane * kGeoCountStride], P.geoCap) : 0;
        int incl = cnt;
#pragma unroll
        for (int d = 1; d < kGeoLists; d <<= 1) {
            const int v = __shfl_up(incl, d);
            if (lane >= d)
                incl += v;
        }
        const unsigned e = geo ? P.pixItem[(size_t)t * 64 + (((r & 7) << 3) | (x & 7))] : 0u;
        const int excl = __shfl(incl - cnt, (int)(e % kGeoLists));
        if (geo)
            gw = P.geoColor[excl + (int)(e / kGeoLists)];
    }
    const int y = launch_row_y(P, r);
    const V3 dir = primary_dir(P, x, y);
    V3 acc{0.f, 0.f, 0.f};
    if constexpr (RESUME) {
        if (valid && P.sampleFirst > 0) {
            const size_t o = 3 * ((size_t)r * (size_t)P.width + (size_t)x);
            acc = V3{P.accum[o], P.accum[o + 1], P.accum[o + 2]};
        }
    }
    if (valid && P.spp > 0 && P.maxBounce > 0) {
        /* hoisted mode evaluates the primary ray's miss once (a function of the pixel, like its closest hit), faithful
         * mode every sample */
        if (GENERAL && P.hoist) {
            const V3 l = add(V3{0.f, 0.f, 0.f}, mulv(environment(dir, P.env), V3{1.f, 1.f, 1.f}));
            for (int s = 0; s < P.spp; ++s)
                acc = add(acc, mul(l, P.invSpp));
        } else {
            /* the sun term provably below half an ulp of every colour component for this pixel (sun_vanishes, a
             * function of the pixel's direction and the launch's environment) */
            const bool vanish = sun_vanishes(dir, P.env);
#if RTC_SKY_PATHS && !defined(RTC_AB_CHEAP_ENV_SKY)
            /* (the GENERAL kernels one sample per iteration: two took them to scratch) */
            acc = sky_samples_on<GENERAL ? 1 : RTC_SKY_UNROLL>(env_classify(dir, P.env, vanish), acc, dir, P.env, P.spp,
                                                               P.invSpp);
#else
#pragma unroll 2
            for (int s = 0; s < P.spp; ++s) {
#if defined(RTC_AB_CHEAP_ENV_SKY) && defined(RTC_EXPERIMENT) /* timing experiment only (the environment's cost) */
                const V3 l = lerp(P.env.horizon, P.env.zenith, fmaxf(dir.y + (float)s * 1e-9f, 0.f));
#else
                /* raytracing.c:291 with rayColor (1, 1, 1): 0 + environment (environment_miss_term: acc starts at +0) */
                const V3 l = environment_miss_term(dir, P.env, vanish);
#endif
                acc = add(acc, mul(l, P.invSpp)); /* main.c:99 */
            }
#endif
        }
        segCalls = (unsigned)P.spp;
        segTraced = P.hoist ? 1u : (unsigned)P.spp;
    }
    /* vec3ToColor (raytracing.c:11-15, main.c:101); a geometry pixel's bytes as the geometry kernel quantised them */
    const unsigned char c0 = valid ? float_to_u8(acc.x) : (unsigned char)(gw & 0xffu);
    const unsigned char c1 = valid ? float_to_u8(acc.y) : (unsigned char)((gw >> 8) & 0xffu);
    const unsigned char c2 = valid ? float_to_u8(acc.z) : (unsigned char)((gw >> 16) & 0xffu);
    unsigned char *const rowp = P.colors + 3 * ((size_t)r * (size_t)P.width + (size_t)blockIdx.x * 64);
    const bool whole = mine == ~0ull && ((uintptr_t)rowp & 15u) == 0u; /* wave-uniform */
    if (whole) {
        unsigned char *st = sStrip[lw];
        st[3 * lane] = c0;
        st[3 * lane + 1] = c1;
        st[3 * lane + 2] = c2;
        wave_lds_sync();
        if (lane < 12)
            ((uint4 *)rowp)[lane] = ((const uint4 *)st)[lane];
    } else if (writes) {
        rowp[3 * lane] = c0;
        rowp[3 * lane + 1] = c1;
        rowp[3 * lane + 2] = c2;
    }
    if (GENERAL && valid && P.accum) {
        const size_t o = 3 * ((size_t)r * (size_t)P.width + (size_t)x);
        P.accum[o] = acc.x;
        P.accum[o + 1] = acc.y;
        P.accum[o + 2] = acc.z;
    }
    if constexpr (RESUME) {
        if (valid && P.sampleFirst == 0)
            P.rngState[(size_t)r * (size_t)P.width + (size_t)x] = (unsigned)(x + y * P.width); /* main.c:95 */
    }
    if (GENERAL)
        flush_counters(P, segCalls, segTraced, 0ull, lane);
}
