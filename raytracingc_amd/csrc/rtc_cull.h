/* rtc_cull.h -- the kernels around the render kernels: the superblock and tile culls (candidate lists, geometry-pixel
 * items), the workgroup launch order, and the segment counters with their reduction.
 * A section of rtc_render.hip's translation unit: included there once, after the headers above it in that file's
 * list (it uses their names, and rtcdev's through the file's using-directive). */
#pragma once

/* Tile candidate lists for primary segments.  A pixel's primary ray is the same ray for every sample
 * (main.c:88-94: no jitter), so the primary filter's verdict for (pixel, triangle) is the same for
 * every sample.  One pass over the launch's pixels records, per 8x8 tile (= one wave of the render kernel),
 * the set of triangles the filter keeps for at least one pixel of the tile; the render kernel's primary
 * segments then visit only that set, in index order.  A triangle left out fails the filter for every pixel
 * of the tile, so the reference's rayTriangle rejects it for every primary ray there: the closest hit is
 * unchanged, bit for bit.  The filter is the render kernel's own (prim_backfacing / prim_pass, same records,
 * same pixel_ray). */
/* Tile prefilter.  The per-pixel filter values nd, dt, ut, vt, wt are (FMA) dot products of the pixel's f32
 * direction d with per-triangle vectors g.  Over an 8x8 tile, d = v / |v| with v = ex dx + ey dy + ez fov
 * affine in the pixel's (dx, dy), which lie in the rectangle spanned by the tile's extreme pixels (dx, dy
 * are monotone in x, y).  So g.v takes its extremes at the rectangle's corners, |v| lies in [vmin, vmax]
 * (vmax: |v| is convex, a corner; vmin: v.ez/|ez| is affine, its smallest corner value, when positive), and
 * g.d (exact direction) lies in [LB, UB] with UB = Amax / vmin or Amax / vmax by the sign of the corner
 * maximum Amax (LB likewise).  The computed value differs from g.d(exact) by at most
 *   |g|_1 (eDir + 3.01 u),  eDir = 16 u S / vmin + 4 u  (u = 2^-24, S = max|dx| + max|dy| + |fov|)
 * (f32 v: 3 roundings per component, <= 3 u S each; normalisation <= 2 u; the FMA dot <= 3 u |g|_1; the
 * constants carry ~1.5x).  A triangle is left out of the tile when one filter condition fails for every
 * point of that range -- then it fails for every pixel, exactly as the per-pixel filter would decide.
 * Computed in double per (tile, triangle); a tile whose bounds are not finite or whose vmin <= 0 is never
 * pruned. */
/* (TileCone, rect_cone, tile_cone, cone_range and tile_prunes: rtc_layout.h, shared with the primary cull's probe) */

/* Level 0 of the tile cull: the same prefilter over a superblock of kSuperBlocks x kSuperBlocks workgroup blocks (64 x 64
 * pixels of the launch's rows), one wave each.  A triangle it prunes fails the filter for every pixel of the superblock,
 * so rtc_tile_cull's level 1 tests only its survivors, and a block whose superblock keeps none (the sky of a frame)
 * skips its own double-precision cone.  Same candidate lists bit for bit (each level only removes triangles the
 * per-pixel filter rejects for every pixel of the rectangle). */
constexpr int kSuperBlocks = 4;
/* (launches of more than rtcplan::kSuperCullPixels pixels run level 0) */
__global__ __launch_bounds__(64) void rtc_super_cull(RenderParams P, unsigned long long *__restrict__ superMask)
{
    const int sx = blockIdx.x, sy = blockIdx.y, lane = threadIdx.x;
    const int x0 = sx * kSuperBlocks * kTileW, r0 = sy * kSuperBlocks * kTileH;
    const TileCone K = rect_cone(P, x0, x0 + kSuperBlocks * kTileW - 1, r0, r0 + kSuperBlocks * kTileH - 1);
    unsigned long long *out = superMask + (size_t)(sy * P.superX + sx) * P.maskWords;
    for (int w = 0; w < P.maskWords; ++w) {
        const int ti = w * 64 + lane;
        const bool maybe = ti < P.triPadded && (!K.ok || !tile_prunes(K, P.primF[ti]));
        const unsigned long long m = __ballot(maybe);
        if (lane == 0)
            out[w] = m;
    }
}

/* Outputs: pixMask (every tile: its pixels with a candidate) and, for the split launch (P.geoList), the candidate words
 * of the workgroups with a surviving triangle and the geometry-pixel lists: rtc_render_chain reads the words of the
 * tiles its items lie in, the sky pass pixMask alone.  Round 6: a split launch no longer writes the zero words of the
 * workgroups without a survivor (most of a sky-heavy frame), a per-tile pixel count or the workgroup weights (only
 * rtc_order_blocks reads those, before the one-lane-per-pixel kernel): WRITE_SIZE per 1080p launch 2.13 -> 0.88 MB, the
 * frame unchanged (profiles/r06_j_pmc_writes.log, r06_i_ab_cull_trim_xcd_runs_prefetch.log). */
/* SPH (the sphere split): the launch renders P.sphereCount > 0 spheres through the split launch, so a pixel
 * is a geometry pixel also when its primary ray records a sphere hit -- the reference's own predicate on the pixel's
 * primary_dir: raySphere hits with dst < 999999 (calculateRayCollision's initial closest distance, raytracing.c:218-228)
 * for some sphere.  It is exact, not a bound: the sky pass then renders exactly the pixels whose primary ray hits
 * neither a sphere nor a triangle candidate.  A NaN direction (height-1 frames) gives dst = NaN, and NaN < 999999 is
 * false, as in the reference.  The workgroup and superblock shortcuts that skip triangle-free pixels do not skip a
 * workgroup with a sphere pixel; the tile's triangle mask words are the triangle-only launch's.  A template, not a
 * uniform branch: rtc_tile_cull (without spheres) is the kernel every other launch ran before, instruction for
 * instruction. */
/* DRAWS (the draw cache, rtc_params.h DrawCache): the lane that appends a pixel's item record looks up the pixel's block
 * in the slot table (by its seed x + y * width, frame coordinates); a pixel without one takes a block while the pool has
 * room -- one atomic per tile with such pixels -- and enters it in the table with its seed in blockSeed, for the fill kernel
 * behind this one; the item's block + 1 (0: none, the geometry kernel computes its draws) goes to itemDraw beside the
 * record.  A template like SPH: the other launches' kernels stay what they were. */
template <bool SPH, bool DRAWS = false>
__device__ __forceinline__ void tile_cull_body(const RenderParams &P, unsigned long long *__restrict__ mask,
                                               unsigned *__restrict__ weight, unsigned long long *__restrict__ pixMask,
                                               const DrawCache &C = DrawCache{})
{
    const bool split = P.geoList != nullptr; /* (uniform) */
    if (KARG(cullPrio)) /* (RenderParams::cullPrio) */
        __builtin_amdgcn_s_setprio(3);
    __shared__ unsigned wgWeight, wgAny;
    extern __shared__ unsigned long long sBlockCand[]; /* maskWords: the block's 16x16 prefilter survivors */
    CSTAMP(c0);
    if (threadIdx.x == 0) {
        wgWeight = 0;
        wgAny = 0;
    }
    const int bx = blockIdx.x, by = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (P.geoCountNext && bx == 0 && by == 0 && threadIdx.x < kGeoLists) /* the next split launch's sub-lists */
        P.geoCountNext[threadIdx.x * kGeoCountStride] = 0;
    /* level 1: the prefilter over the workgroup's 16x16 pixels (a superset of each tile's direction range, so
     * a triangle it prunes fails for every pixel of the four tiles); the waves share the mask words */
    __syncthreads();
    /* the superblock's survivors (level 0, rtc_super_cull; all ones without it): wave-uniform scalar loads */
    const unsigned long long *sup =
        P.superMask ? P.superMask + (size_t)((by / kSuperBlocks) * P.superX + bx / kSuperBlocks) * P.maskWords : nullptr;
    bool supAny = !sup;
    for (int w = 0; sup && w < P.maskWords && !supAny; ++w)
        supAny = KCONST(sup)[w] != 0ull;
    if (wave < P.maskWords && supAny) { /* wave-uniform: only the waves with mask words need the block's cone */
        const TileCone KB = rect_cone(P, bx * kTileW, bx * kTileW + kTileW - 1, by * kTileH, by * kTileH + kTileH - 1);
        for (int w = wave; w < P.maskWords; w += kBlock / 64) {
            const int ti = w * 64 + lane;
            const unsigned long long sw = sup ? KCONST(sup)[w] : ~0ull;
            const bool maybe = ((sw >> lane) & 1ull) && ti < P.triPadded &&
                               (!KB.ok || !tile_prunes(KB, P.primF[ti]));
            const unsigned long long m = __ballot(maybe);
            if (lane == 0) {
                sBlockCand[w] = m;
                if (m)
                    wgAny = 1; /* benign race: every writer stores 1 */
            }
        }
    }
    bool sphHit = false; /* SPH: this lane's primary ray records a sphere hit */
    if (SPH) {
        const PixelRay ps = pixel_ray(P, bx, by);
        if (ps.valid) {
            for (int i = 0; i < P.sphereCount; ++i) { /* wave-uniform: the records are scalar loads */
                const DevSphere sp = KLOAD(P.spheres, i);
                float d;
                if (ray_sphere(P.origin, ps.dir, V3{sp.cx, sp.cy, sp.cz}, sp.radius, d) && d < 999999.f)
                    sphHit = true;
            }
        }
        /* a superblock that keeps no triangle ran no level-1 pass: the block's survivors are none (level 2 reads them
         * when a sphere pixel keeps the workgroup) */
        if (!supAny)
            for (int w = threadIdx.x; w < P.maskWords; w += kBlock)
                sBlockCand[w] = 0ull;
        if (__ballot(sphHit) != 0ull && lane == 0)
            wgAny = 1; /* (the same benign race) */
    }
    __syncthreads();
    CSTAMP(c1);
    const int tile = wave_tile(bx, by);
    unsigned long long *out = mask + (size_t)tile * P.maskWords;
    if (!wgAny) { /* workgroup-uniform: no triangle survives for any of its pixels (most of a sky-heavy frame) */
        for (int w = lane; !split && w < P.maskWords; w += 64)
            out[w] = 0ull;
        if (lane == 0)
            pixMask[tile] = 0ull;
        if (threadIdx.x == 0 && !split)
            weight[blockIdx.y * gridDim.x + blockIdx.x] = 0u;
        CSTAMP(c9);
        CREC(blockIdx.y * gridDim.x + blockIdx.x, c0, c1, c9, 0, 0, 0, 0);
        return;
    }
#ifdef RTC_DIAG
    unsigned long long dPre = 0, dLoop = 0, dCand = 0;
#endif
    const PixelRay px = pixel_ray(P, bx, by);
    bool anyCand = SPH && sphHit;
    /* level 2: the tile's own prefilter on the block's survivors, then the per-pixel filter */
    const TileCone K = tile_cone(P, tile % (int)(gridDim.x * 2), tile / (int)(gridDim.x * 2));
    for (int w = 0; w < P.maskWords; ++w) {
        /* lane l: may triangle 64w + l pass for some pixel of the tile? */
        const int ti = w * 64 + lane;
        const unsigned long long bc = sBlockCand[w];
        CSTAMP(c2);
        const bool maybe = ((bc >> lane) & 1ull) && (!K.ok || !tile_prunes(K, P.primF[ti]));
        unsigned long long todo = bc ? __ballot(maybe) : 0ull;
        unsigned long long bits = 0;
        CSTAMP(c3);
#ifdef RTC_DIAG
        dPre += c3 - c2;
        dCand += (unsigned long long)__popcll(todo);
#endif
        while (todo) {
            const int j = __builtin_ctzll(todo);
            todo &= todo - 1;
            const DevPrimF F = KLOAD(P.primF, w * 64 + j);
            const bool keep = (int)px.valid & (int)!prim_backfacing(px.dir, F) & (int)prim_pass(px.dir, F);
            anyCand |= keep;
            if (__ballot(keep))
                bits |= 1ull << j;
        }
        CSTAMP(c4);
#ifdef RTC_DIAG
        dLoop += c4 - c3;
#endif
        if (lane == 0)
            out[w] = bits;
    }
    /* the tile's pixels with at least one candidate (they do the bounce work); a tile has a non-empty candidate list
     * exactly when one of them is set */
    const unsigned long long b = __ballot(anyCand);
    if (lane == 0)
        pixMask[tile] = b;
    if (P.geoList && b) {
        unsigned blk = 0; /* DRAWS: this lane's pixel's block + 1 */
        if constexpr (DRAWS) {
            const bool geo = (b >> lane) & 1ull;
            const unsigned seed = (unsigned)(px.x + px.y * P.width); /* main.c:95 */
            const bool inTable = geo && seed < C.tablePixels;
            if (inTable)
                blk = C.table[seed];
            const unsigned long long want = __ballot(inTable && blk == 0u);
            if (want) { /* (uniform) pixels new to the cache: nothing of this in the steady state */
                const unsigned n = (unsigned)__popcll(want);
                unsigned base = C.capacity;
                if (lane == 0 && __atomic_load_n(&C.ctr[kDcTaken], __ATOMIC_RELAXED) < C.capacity)
                    base = atomicAdd(&C.ctr[kDcTaken], n);
                base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
                const unsigned k = base + (unsigned)__popcll(want & ((1ull << lane) - 1ull));
                if (((want >> lane) & 1ull) && k < C.capacity) { /* granted: the table entry, the fill's input */
                    blk = k + 1u;
                    C.table[seed] = blk;
                    C.blockSeed[k] = seed;
                }
            }
            const unsigned long long none = __ballot(geo && blk == 0u);
            if (none && lane == 0)
                atomicAdd(&C.ctr[kDcUncachedAcc], (unsigned)__popcll(none));
        }
        /* this tile's geometry pixels, appended to sub-list tile % kGeoLists (rtc_render_chain's work) */
        const auto append = [&](unsigned long long gb, int l) {
            int base = 0;
            if (lane == 0)
                base = atomicAdd(&P.geoCount[l * kGeoCountStride], __popcll(gb));
            base = __builtin_amdgcn_readfirstlane(base);
            /* a sub-list holds every geometry pixel of its tiles (geoCap = 64 x its tiles) when its counter started at
             * 0; a stale counter must not write past it (the readers clamp the counts to geoCap too) */
            if (((gb >> lane) & 1ull) && base + __popcll(gb) <= P.geoCap) {
                const int pos = base + __popcll(gb & ((1ull << lane) - 1ull));
                ((uint4 *)P.geoList)[(size_t)l * P.geoCap + pos] = item_record(P, px, tile, lane);
                if constexpr (DRAWS)
                    C.itemDraw[(size_t)l * P.geoCap + pos] = blk;
                if (P.pixItem) /* the pixel's entry: pos of sub-list l (the sky pass turns it into its item) */
                    P.pixItem[(size_t)tile * 64 + lane] = (unsigned)(pos * kGeoLists + l);
            }
        };
        append(b, tile % kGeoLists);
    }
    if (!split) { /* the one-lane-per-pixel kernel's workgroup order (rtc_order_blocks) */
        if (lane == 0 && b)
            atomicAdd(&wgWeight, (unsigned)__popcll(b));
        __syncthreads();
        if (threadIdx.x == 0)
            weight[blockIdx.y * gridDim.x + blockIdx.x] = wgWeight;
    }
    CSTAMP(c6);
#ifdef RTC_DIAG
    CREC(blockIdx.y * gridDim.x + blockIdx.x, c0, c1, c6, 1, dPre, dLoop, dCand);
#endif
}

/* The kernel of every launch but the sphere split's; rtc_tile_cull_sph<true> is the sphere split's (the same body with SPH).
 * That one is a template so that its code is emitted where rtc_render.hip's instantiation list names it, after the
 * kernels of the launches without spheres, and not here among the non-template kernels. */
__global__ __launch_bounds__(kBlock) void rtc_tile_cull(RenderParams P, unsigned long long *__restrict__ mask,
                                                       unsigned *__restrict__ weight,
                                                       unsigned long long *__restrict__ pixMask)
{
    tile_cull_body<false>(P, mask, weight, pixMask);
}
template <bool SPH>
__global__ __launch_bounds__(kBlock) void rtc_tile_cull_sph(RenderParams P, unsigned long long *__restrict__ mask,
                                                           unsigned *__restrict__ weight,
                                                           unsigned long long *__restrict__ pixMask)
{
    tile_cull_body<SPH>(P, mask, weight, pixMask);
}

/* The tile cull of a launch that uses the draw cache (tile_cull_body<.., DRAWS>), and the fill kernel the executor issues
 * behind it under the same planned operation (its completion is the operation's event).  Templates for the same reason as
 * rtc_tile_cull_sph: their code is emitted where the instantiation list names them. */
template <bool DRAWS>
__global__ __launch_bounds__(kBlock) void rtc_tile_cull_draws(RenderParams P, unsigned long long *__restrict__ mask,
                                                             unsigned *__restrict__ weight,
                                                             unsigned long long *__restrict__ pixMask, DrawCache C)
{
    tile_cull_body<false, DRAWS>(P, mask, weight, pixMask, C);
}
/* The blocks the cull before it handed out, [fill mark, taken): a wave per block, lane j computes entry j -- the seed
 * advanced by 7 j draws, RandomDiretion and the roulette value, by the geometry kernel's own functions (random_direction
 * with its exact fallback, random_value) -- all 64 entries whatever the launch's spp.  Dense, full-lane, independent work.
 * In the steady state nothing is fresh: every workgroup reads the two counters and ends.  Workgroup 0 moves the fill mark
 * (into the other parity's word, which no workgroup of this launch reads) and publishes the launch's statistics. */
constexpr int kFillBlocks = 512; /* workgroups of 4 waves */
template <bool DRAWS>
__global__ __launch_bounds__(256) void rtc_fill_draws(DrawCache C)
{
    const unsigned hi = min(C.ctr[kDcTaken], C.capacity);
    const unsigned lo = min(C.ctr[C.parity ? kDcFilled1 : kDcFilled0], hi);
    const int lane = threadIdx.x & 63;
    const RngJump laneJump = rng_jump_by(7u * (unsigned)lane);
    for (unsigned k = lo + blockIdx.x * 4u + (threadIdx.x >> 6); k < hi; k += gridDim.x * 4u) {
        unsigned s = C.blockSeed[k] * laneJump.a + laneJump.c;
        const V3 rd = random_direction(s);
        C.pool[(size_t)k * kDrawEntries + lane] = make_float4(rd.x, rd.y, rd.z, random_value(s));
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        C.ctr[C.parity ? kDcFilled0 : kDcFilled1] = hi;
        C.ctr[kDcFresh] = hi - lo;
        C.ctr[kDcUncached] = C.ctr[kDcUncachedAcc];
        C.ctr[kDcUncachedAcc] = 0u;
    }
}

/* Launch order of the render kernel's workgroups: a counting sort of the weights, heaviest bucket first
 * (order inside a bucket is arbitrary; the frame does not depend on it -- every pixel is seeded by its own
 * index, main.c:95).  One workgroup; n is at most a few ten thousand. */
constexpr int kOrderBuckets = 17; /* weight / 16: 0 (sky only) .. 16 (all 256 pixels see geometry) */
__global__ __launch_bounds__(1024) void rtc_order_blocks(const unsigned *__restrict__ weight, int n,
                                                          int *__restrict__ order)
{
    __shared__ int cnt[kOrderBuckets];
    if (threadIdx.x < kOrderBuckets)
        cnt[threadIdx.x] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x)
        atomicAdd(&cnt[min(kOrderBuckets - 1, (int)((weight[i] + 15) / 16))], 1);
    __syncthreads();
    if (threadIdx.x == 0) {
        int off = 0;
        for (int b = kOrderBuckets - 1; b >= 0; --b) {
            const int c = cnt[b];
            cnt[b] = off;
            off += c;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x)
        order[atomicAdd(&cnt[min(kOrderBuckets - 1, (int)((weight[i] + 15) / 16))], 1)] = i;
}

/* Segment counters.  One atomic per wave into the caller's three counters serialises in L2 (tens of
 * thousands of same-address atomics per frame cost milliseconds), so waves add into kSegSlots slots, each
 * in its own 128-B line, and rtc_reduce_segments folds the slots into the caller's counters at the end. */
constexpr int kSegSlots = 256, kSegSlotStride = 16; /* u64 */
static_assert(kSegSlots * kSegSlotStride == 256 * 16, "rtc_scene_upload allocates 256 x 16 u64");

/* counters (rtc.h RTC_SEGMENT_COUNTERS): [0] calculateRayCollision calls, [1] traced, [2] ray-triangle tests of
 * the accumulated samples, [3] ray-cluster tests, [4] ray-triangle tests of speculative samples that were
 * evaluated but not accumulated (rtc_render_chain window lanes off the chain) */
__device__ __forceinline__ void flush_counters(const RenderParams &P, unsigned segCalls, unsigned segTraced,
                                               unsigned long long segTests, int lane, unsigned segClusters = 0,
                                               unsigned long long segSpec = 0)
{
    if (!P.segments)
        return;
    unsigned long long a = segCalls, b = segTraced, n = segTests, k = segClusters, q = segSpec;
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_xor(a, off);
        b += __shfl_xor(b, off);
        n += __shfl_xor(n, off);
        k += __shfl_xor(k, off);
        q += __shfl_xor(q, off);
    }
    if (lane == 0 && (a | b | n | k | q)) {
        const unsigned slot = (blockIdx.x * 7u + blockIdx.y * 131u + (threadIdx.x >> 6)) % kSegSlots;
        unsigned long long *c = P.segSlots + (size_t)slot * kSegSlotStride;
        atomicAdd(&c[0], a);
        atomicAdd(&c[1], b);
        atomicAdd(&c[2], n);
        if (k)
            atomicAdd(&c[3], k);
        if (q)
            atomicAdd(&c[4], q);
    }
}

__global__ __launch_bounds__(kSegSlots) void rtc_reduce_segments(unsigned long long *__restrict__ slots,
                                                                 unsigned long long *__restrict__ out)
{
    __shared__ unsigned long long part[RTC_SEGMENT_COUNTERS][kSegSlots / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
#pragma unroll
    for (int k = 0; k < RTC_SEGMENT_COUNTERS; ++k) {
        unsigned long long v = slots[(size_t)t * kSegSlotStride + k];
        slots[(size_t)t * kSegSlotStride + k] = 0; /* zero again for the next launch */
        for (int off = 32; off > 0; off >>= 1)
            v += __shfl_xor(v, off);
        if (lane == 0)
            part[k][w] = v;
    }
    __syncthreads();
    if (t < RTC_SEGMENT_COUNTERS) {
        unsigned long long v = 0;
        for (int i = 0; i < kSegSlots / 64; ++i)
            v += part[t][i];
        out[t] += v; /* stream-ordered after every render kernel of the launch: no atomic needed */
    }
}
