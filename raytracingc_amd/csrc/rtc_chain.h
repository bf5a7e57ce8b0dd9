/* rtc_chain.h -- rtc_render_chain: one wave per geometry pixel of a split launch, with its helpers, and the kernels
 * that sum its deferred samples (rtc_accumulate_samples, and a pass's rtc_accumulate_samples_resume).
 * A section of rtc_render.hip's translation unit: included there once, after the headers above it in that file's
 * list (it uses their names, and rtcdev's through the file's using-directive). */
#pragma once

/* ---- state-indexed samples (rtc_render_chain, the default for pixels that see geometry) --------------------
 * A pixel's samples are chained only through its RNG state (main.c:95-100), and in the OBJ scenes every sample
 * whose primary ray hits draws exactly 7 values per hit (RandomDiretion's six, moremath.c:104-108, and the
 * roulette draw, raytracing.c:285) and none on a miss.  So a sample is a pure function of the draw offset it
 * starts at: write S_j for the sample started from the seed advanced by 7 j draws (rng_advance; the LCG step
 * is affine) and h_j for its number of hits.  The reference's k-th sample is S_{j_k} with
 *     j_0 = 0,   j_{k+1} = j_k + h_{j_k}
 * (h >= 1 when the primary ray hits; when it misses every sample is S_0 and h = 0).  The kernel evaluates
 * S_j for a window of consecutive j -- one lane per j, 64 at a time -- and then walks the chain through the
 * window, adding the members' radiance in sample order (main.c:99, sequential f32 adds).  Every accumulated
 * value is one of the reference's samples, computed by the reference's operations from its exact start state,
 * so the frame is bit-identical; no prediction is involved.  ~97 % of the geometry pixels of the BASELINE frame
 * have no sample with a second hit (sum h = spp), so one window of 64 covers them; the others take a second
 * window.  The lanes of a wave share the pixel's primary ray: the primary trace is wave-uniform (scalar-loaded
 * candidate records), the shading at the primary hit runs in lockstep, and only the bounce segments diverge.
 * Work: one wave per geometry pixel, from the tile cull's sub-lists (see the kernel). */
static_assert(sizeof(SampleSlot) == rtcplan::kSampleSlotBytes, "the planner sizes the deferred sample slots");
/* Shares (row stride > 1) of up to rtcplan::kInlineSumPixels pixels are "small": they sum in-kernel and,
 * pipelined, prepare, cull and run their geometry kernel on the two cull streams.  Round 4 raised it
 * from 400 k to 600 k pixels so that the 1080p 1/4 share (518 k) is one: 0.137 -> 0.117 ms per pipelined share; the
 * 1/2 share and the 4K 1/8 share (1.04 M) measured no better that way (tools/scale_probe.py, profiles/r04_y_*) */
#ifndef RTC_SKY_MERGE
#define RTC_SKY_MERGE 1 /* (A/B switch, round 6) */
#endif
constexpr int kChainBlock = 256; /* threads per chain workgroup (two-wave workgroups were slower everywhere, r04_ze) */
/* Persistent chain workgroups per CU (each 4 waves of 128 VGPRs: 4 fill every SIMD's registers).  A whole frame runs 3,
 * so that a quarter of every SIMD's registers holds two sky waves (<= 64 VGPRs) from the start: the sky pass then runs
 * in the chain kernel's idle issue slots instead of waiting for its tail, and the launch stream's small kernels are no
 * longer starved by that tail (round 4: frame 0.372 -> 0.351 ms; 4 per CU: 0.370 vs 0.340 ms on the alternating streams,
 * though fsuzane, whose frame is nearly all geometry kernel, takes 1.12 vs 1.22 ms with 4).  Small shares run 3 too since
 * consecutive shares overlap on the alternating streams (4 before).  Round 5: whole frames of scenes whose bounce rays
 * often hit again run 4 (RTC_CHAIN_WGS_HIT, chosen at upload by bounce_hit_share).  Workers = per-CU count x CUs:
 * exactly the resident capacity, no second round.  (RTC_CHAIN_WGS_FULL / _HIT are defined with kSkySlots.) */
#ifndef RTC_CHAIN_WGS_SHARE
#define RTC_CHAIN_WGS_SHARE 3 /* 1/4 share 0.116 -> 0.113 ms, 1/8 share 0.075 -> 0.074 ms (round 4, r04_za) */
#endif
#ifndef RTC_CHAIN_WAVES
#define RTC_CHAIN_WAVES 4
#endif

/* The bounce segments of a wave's lanes (calculateRayCollision, raytracing.c:216-240), as a dense list of
 * (lane, cluster) pairs.  Each live lane culls the clusters its half-line cannot reach (DevCluster bound) and
 * enters the rest into the wave's pair list (cluster-major); the list is then processed 64 pairs at a time,
 * every lane taking one pair: the owner's ray from LDS, the cluster's 8 records from LDS (staged once per
 * workgroup), the exact-safe filter and the reference arithmetic for survivors.  A pair's closest hit goes
 * to its owner with an LDS atomic minimum on (dst bits << 32 | index): dst >= EPSILON > 0, so the float bits
 * order like the values and the key order is the lexicographic (dst, index) order -- the lowest index among
 * equal distances, as the reference's strict `<` over ascending indices keeps (raytracing.c:231).  Only
 * candidates with dst < 999999 (the reference's initial closest distance, raytracing.c:218) enter.
 * Compared with a wave-uniform loop over the union of the lanes' clusters (every lane masked through every
 * cluster some lane needs), each ray-triangle test here occupies one lane-slot instead of up to 64. */
typedef float f2 __attribute__((ext_vector_type(2)));
/* A sample's m-th hit draws the 7 values at state index j + m (RandomDiretion's six, the roulette's one): exactly
 * what S_{j+m}'s first hit draws.  So the window's active lanes enter the draws of their own state index, computed
 * at the primary hit, in a per-wave LDS table, and a later hit of lane l in bounce iteration i reads entry l + i
 * instead of running Box-Muller again; only lanes with l + i past the window's active lanes compute theirs (the
 * state advanced by 7 i draws).  The values are the same function of the same state, so the frame is unchanged;
 * what goes is most of the divergent Box-Muller passes of the bounce iterations with a hit (scenes whose rays hit
 * several times: fsuzane 2.00 -> 1.93 ms per frame, 1.77 with the dense culls below). */
constexpr int kChainPairs = 1024;
struct ChainWaveLds {
    float4 cl[kChunkClusters][2]; /* first bounces: the clusters' origin terms (ClusterTerms) */
    unsigned long long key[64];   /* closest hit per lane, (dst bits << 32) | index */
    /* lane | cluster << 6 (or lane | record << 6), cluster-major; a full list is run through the passes and
     * refilled.  Its size keeps a block (4 waves + the staged records of one chunk) within 40 KB of LDS: four
     * blocks per CU, the 4 waves per SIMD that 128 VGPRs allow */
    unsigned short pair[kChainPairs];
    float4 draw[64]; /* the window's hit draws by state index jn + i: RandomDirection's vector, the roulette value */
};
constexpr unsigned long long kNoHitKey = ((unsigned long long)0x497423F0u << 32) | 0xFFFFFFFFull; /* 999999.f */
static_assert(kChunkClusters <= 32, "cluster masks are 32-bit");
static_assert(kChainPairs >= 64 * kClusterSize, "one cluster's pairs of a full wave fit the list");
/* The in-kernel sums' staging (rtc_render_chain, flush()): component c of a window's staged sample i at
 * stage[c * kStageRow + i] in the pair list's space; lane c < 3 then reads its row four samples at a time (ds_read_b128).
 * The row length is padded: the generic loop reads one quad ahead (at most quad 16 = dwords 64..67 of a row), the rows
 * start 16-byte aligned, and they start 4 banks apart -- ds_read_b128 banks by (dword address) mod 64, and lanes 0..2
 * are in one of its 16-lane groups, so the three lanes' quads (same quad index, three rows) must not share a bank.
 * The staging lanes write consecutive dwords of a row (ds_write_b32: 32 lanes per group, banks mod 32): no conflict. */
constexpr int kStageRow = 68;
constexpr bool stage_rows_disjoint(int row)
{
    for (int a = 0; a < 3; ++a)
        for (int b = a + 1; b < 3; ++b) {
            const int d = ((b - a) * row) % 64; /* row b's quad starts d banks after row a's; each covers 4 banks */
            if (d < 4 || d > 60)
                return false;
        }
    return true;
}
static_assert(kStageRow >= 64 + 4, "the quad read ahead of a full window stays inside the row");
static_assert(kStageRow % 4 == 0 && offsetof(ChainWaveLds, pair) % 16 == 0 && alignof(ChainWaveLds) >= 16,
              "the rows start 16-byte aligned (ds_read_b128)");
static_assert(stage_rows_disjoint(kStageRow), "the three summing lanes' ds_read_b128 hit disjoint banks");
constexpr int kStageLaneStride = 1; /* dwords between the entries two neighbouring staging lanes write */
static_assert(kStageLaneStride % 2 == 1, "a 32-lane group's staging writes fall on 32 distinct banks");
static_assert(kChainPairs * sizeof(unsigned short) >= 3 * kStageRow * sizeof(float), "a window's staged samples fit the list");
/* rtc_render_chain's static LDS (powf tables, the waves' ChainWaveLds, the work counter) and the block budget
 * that keeps 4 blocks (16 waves) per CU */
constexpr size_t kChainStaticLds = sizeof(PowTablesLds) +
                                   (kChainBlock / 64) * sizeof(ChainWaveLds) + 64 +
                                   kChunkClusters * sizeof(DevCluster) /* sCl (the dense culls) */;
constexpr size_t kCuLds = 160 * 1024; /* gfx950 LDS per CU */
/* the block LDS that keeps the chain workgroups per CU at most n: above kCuLds / (n + 1) */
constexpr size_t chain_lds_floor(int n) { return n >= 4 ? 0 : kCuLds / (size_t)(n + 1) + 256; }

/* The pair passes: entry i of W.pair (i < n) is a (lane, cluster) pair -- the cluster's 8 records; the owner's ray
 * by ds_bpermute from the owner lane (every lane takes part), the exact-safe filter, the reference arithmetic for
 * survivors, an atomic lexicographic minimum into the owner's key. */
/* The clustered records staged in LDS structure-of-arrays: 16-B quarter k of record i at q[k * n + i], n = the
 * staged record count.  Lanes reading different records then hit different banks in ds_read_b128's 16-lane
 * groups (64-B records at lane-varying indices put four lanes of a group on each bank); one record is still four
 * ds_read_b128.  (Round 5 tried a slot skipped after every cluster, for pair passes whose lanes read record j of
 * different clusters: conflict cycles 3.8 M -> 5.0 M per 1080p launch -- the pair list is cluster-major, so a pass's
 * lanes mostly share a cluster, while the reach table's consecutive records then straddled the skipped slots.) */
__host__ __device__ constexpr int soa_slots(int n) { return n; }
__device__ __forceinline__ DevTri rec_soa(const float4 *__restrict__ q, int n, int i)
{
    DevTri t;
    float4 *v = (float4 *)&t;
    v[0] = q[i];
    v[1] = q[n + i];
    v[2] = q[2 * n + i];
    v[3] = q[3 * n + i];
    return t;
}
__device__ __forceinline__ float bperm_f(int srcLane, float v)
{
    return __int_as_float(__builtin_amdgcn_ds_bpermute(srcLane << 2, __float_as_int(v)));
}
template <bool MULTI>
__device__ __forceinline__ void chain_pair_passes(const RenderParams &P, int n, int c0, const float4 *__restrict__ sRec,
                                                  ChainWaveLds &W, int lane, V3 pos, V3 dir)
{
    for (int b = 0; b < n; b += 64) {
        const int i = b + lane;
        const unsigned pr = i < n ? W.pair[i] : (unsigned)lane;
        const int o = (int)(pr & 63u);
        const V3 rpos{bperm_f(o, pos.x), bperm_f(o, pos.y), bperm_f(o, pos.z)};
        const V3 rdir{bperm_f(o, dir.x), bperm_f(o, dir.y), bperm_f(o, dir.z)};
        if (i < n) {
            Closest c{999999.f, -1};
            const int r0 = (c0 + (int)(pr >> 6)) * kClusterSize, nRec = P.clusterCount * kClusterSize;
            auto rec = [&](int j) -> DevTri { return MULTI ? P.clTris[r0 + j] : rec_soa(sRec, nRec, r0 + j); };
            unsigned surv = 0;
#pragma unroll 4 /* (round 5: 4 vs 2, fsuzane -1 %, headline within noise; same registers) */
            for (int j = 0; j < kClusterSize; ++j)
                surv |= (unsigned)general_filter(rpos, rdir, rec(j)) << j;
            while (surv) {
                const int j = __builtin_ctz(surv);
                surv &= surv - 1;
                const DevTri R = rec(j);
                general_exact(rpos, rdir, R, __float_as_int(R.pad0), c);
            }
            if (c.idx >= 0 && c.dst < 999999.f)
                atomicMin(&W.key[o], ((unsigned long long)__float_as_uint(c.dst) << 32) | (unsigned)c.idx);
        }
    }
}
/* The first-bounce pairs as (lane, live cluster j) -- one entry per cluster a lane keeps, the pass
 * looping over that cluster's records reachable from p0 (W.cl[j][1]: z = cluster index, w = reach bits); one
 * atomic per entry instead of one per record */
__device__ __forceinline__ void chain_pair_passes_cl(int n, const float4 *__restrict__ sRec, int nRec, ChainWaveLds &W,
                                                     int lane, V3 pos, V3 dir)
{
    for (int b = 0; b < n; b += 64) {
        const int i = b + lane;
        const unsigned pr = i < n ? W.pair[i] : (unsigned)lane;
        const int o = (int)(pr & 63u);
        const V3 rpos{bperm_f(o, pos.x), bperm_f(o, pos.y), bperm_f(o, pos.z)};
        const V3 rdir{bperm_f(o, dir.x), bperm_f(o, dir.y), bperm_f(o, dir.z)};
        if (i < n) {
            const float4 kb = W.cl[pr >> 6][1];
            const int r0 = __float_as_int(kb.z) * kClusterSize;
            Closest c{999999.f, -1};
            for (unsigned r = (unsigned)__float_as_int(kb.w); r; r &= r - 1) {
                const DevTri T = rec_soa(sRec, nRec, r0 + __builtin_ctz(r));
                if (general_filter(rpos, rdir, T))
                    general_exact(rpos, rdir, T, __float_as_int(T.pad0), c);
            }
            if (c.idx >= 0 && c.dst < 999999.f)
                atomicMin(&W.key[o], ((unsigned long long)__float_as_uint(c.dst) << 32) | (unsigned)c.idx);
        }
    }
}

/* Dense cluster culls (single-chunk scenes, bounce segments after the first): with a live lanes and nCl clusters, the
 * per-lane loop issues nCl culls for the wave however few lanes are live; instead the wave takes the a * nCl (live
 * lane, cluster) culls 64 at a time -- cluster-major, so the pairs kept come out in the per-lane loop's order -- the
 * owner's ray by ds_bpermute, the cluster from LDS.  Taken while a <= kDenseCullMax (fsuzane 1.93 -> 1.77 ms per
 * frame with 16, 1.80 with 32; the headline frame, whose later bounces are rare, within noise). */
constexpr int kDenseCullMax = 16;
static_assert(kDenseCullMax * kChunkClusters <= kChainPairs, "a dense cull's pairs fit the list");
static_assert(sizeof(ChainWaveLds::cl) >= 64 * sizeof(int), "the dense cull's owner lanes fit W.cl");

template <bool MULTI, bool COUNT, bool HITS>
__device__ __forceinline__ Closest chain_trace_pairs(const RenderParams &P, bool alive, bool firstBounce, V3 pos,
                                                     V3 dir, const float4 *__restrict__ sRec, ChainWaveLds &W,
                                                     int lane, unsigned &tests, const DevCluster *__restrict__ sCl)
{
    W.key[lane] = kNoHitKey;
    const float rho = fabsf(dir.x) + fabsf(dir.y) + fabsf(dir.z), dd = dir_dd(dir);
    const bool rhoOk = P.clusterCull && rho <= kClusterRhoMax;
    tests = 0;
    /* A pixel's first bounces all start at its primary hit point p0 (lane 0's pos; single-chunk scenes):
     *  - the clusters' origin terms, once, one lane per cluster, into LDS, compacted to the clusters with a
     *    record reachable from p0 (below), so the per-lane cull loop is branch-free over those only;
     *  - the records that can be hit from p0 at all, one lane per record: the reference's own f32
     *    dot(AC, (p0 - A) x AB) > 0, or a stored normal not aligned with the geometric one (aligned_normal:
     *    with an aligned normal and that dot <= 0, rayTriangle rejects every direction from p0).
     * The records that cannot be hit are not tested; the rest are tested as (lane, record) pairs.  The argument
     * holds for |dir|_1 <= kClusterRhoMax: a wave with a live ray beyond that takes the per-cluster path. */
    const bool table = !MULTI && firstBounce && P.clusterCull && !__ballot(alive && !rhoOk);
    unsigned long long reach[kChunkClusters * kClusterSize / 64];
    unsigned long long live = 0; /* clusters with a record reachable from p0 (their terms compacted in W.cl) */
    DSECT_BEGIN(dtab);
    if (table) {
        const V3 p0{__int_as_float(__builtin_amdgcn_readlane(__float_as_int(pos.x), 0)),
                    __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pos.y), 0)),
                    __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pos.z), 0))};
#pragma unroll
        for (int q = 0; q < kChunkClusters * kClusterSize / 64; ++q) {
            const int i = q * 64 + lane;
            bool can = false;
            if (i < P.clusterCount * kClusterSize) {
                const DevTri R = rec_soa(sRec, P.clusterCount * kClusterSize, i);
                if (__float_as_int(R.pad0) >= 0) {
                    const V3 sv = sub(p0, V3{R.ax, R.ay, R.az});               /* raytracing.c:198 */
                    const V3 qv = cross(sv, V3{R.abx, R.aby, R.abz});          /* :202 */
                    const float dac = dot(V3{R.acx, R.acy, R.acz}, qv);        /* :206 numerator */
                    can = dac > 0.f || __float_as_int(R.pad1) == 0;
                }
            }
            reach[q] = __ballot(can);
        }
        /* lane k < clusterCount: cluster k's reachable records r8; the clusters with any enter W.cl compacted, in
         * cluster order, with (k, r8) in the second vector */
        unsigned r8l = 0;
        if (lane < P.clusterCount) {
            const unsigned long long rw = lane < 8 ? reach[0] : lane < 16 ? reach[1] : lane < 24 ? reach[2] : reach[3];
            r8l = (unsigned)(rw >> ((lane & 7) * 8)) & 0xffu;
        }
        live = __ballot(r8l != 0u);
        if (r8l) {
            const int pos = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(live >> 32),
                                                           __builtin_amdgcn_mbcnt_lo((unsigned)live, 0u));
            /* (the workgroup's LDS copy of the clusters: a global load here was a round trip on every window) */
            const ClusterTerms t = cluster_terms(p0, sCl[lane]);
            W.cl[pos][0] = make_float4(t.w.x, t.w.y, t.w.z, t.w2);
            W.cl[pos][1] = make_float4(t.A, t.B, __int_as_float(lane), __int_as_float((int)r8l));
        }
        wave_lds_sync();
    }
    DSECT_END(dtab, 14);
    /* scenes of more than kChunkClusters clusters: chunk by chunk (a chunk's ball culls its clusters for a lane
     * at once); the records come from global memory when they are not staged in LDS (sRec null) */
    const int nChunks = MULTI ? P.chunkCount : 1;
    for (int h = 0; h < nChunks; ++h) {
        const int c0 = h * kChunkClusters, nCl = MULTI ? min(kChunkClusters, P.clusterCount - c0) : P.clusterCount;
        bool in = alive;
        if (MULTI) {
            if (alive)
                in = !(rhoOk && cluster_culled(pos, dir, rho, dd, P.chunks[h]));
            if (!__ballot(in))
                continue;
        }
        unsigned cm = 0;
        int n = 0;
        DSECT_BEGIN(dc3);
        const unsigned long long inM = __ballot(in);
        const int nIn = (int)__popcll(inM);
        const bool dense = !MULTI && !table && nIn <= kDenseCullMax;
        if (dense) {
            int *own = (int *)&W.cl[0][0]; /* W.cl is free outside the first bounce's table mode */
            int *kept = own + 64;          /* COUNT: per owner lane, clusters kept (+ 1 << 16 for the scene's last) */
            if (in)
                own[__builtin_amdgcn_mbcnt_hi((unsigned)(inM >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)inM, 0u))] = lane;
            if (COUNT)
                kept[lane] = 0;
            wave_lds_sync();
            const int tot = nIn * nCl;
            const unsigned magic = nIn > 1 ? (unsigned)((0x100000000ull + (unsigned)nIn - 1u) / (unsigned)nIn) : 0u;
            for (int b = 0; b < tot; b += 64) {
                const int e = b + lane;
                const int k = nIn > 1 ? (int)__umulhi((unsigned)e, magic) : e; /* e / nIn, exact for e < 2^16 */
                const bool valid = e < tot;
                const int o = own[valid ? e - k * nIn : 0];
                const V3 rp{bperm_f(o, pos.x), bperm_f(o, pos.y), bperm_f(o, pos.z)};
                const V3 rd{bperm_f(o, dir.x), bperm_f(o, dir.y), bperm_f(o, dir.z)};
                bool keep = false;
                if (valid) {
                    const float rr = fabsf(rd.x) + fabsf(rd.y) + fabsf(rd.z);
                    keep = !(P.clusterCull && rr <= kClusterRhoMax && cluster_culled(rp, rd, rr, dir_dd(rd), sCl[k]));
                }
                const unsigned long long m = __ballot(keep);
                if (keep)
                    W.pair[n + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32),
                                                              __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u))] =
                        (unsigned short)(o | (k << 6));
                if (COUNT && keep)
                    atomicAdd(&kept[o], 1 + (k == P.clusterCount - 1 ? 1 << 16 : 0));
                n += (int)__popcll(m);
            }
            if (COUNT) {
                wave_lds_sync();
                const int kc = kept[lane];
                tests = (unsigned)(kc & 0xffff) * kClusterSize -
                        (unsigned)(kc >> 16) * (unsigned)(P.clusterCount * kClusterSize - P.triCount);
            }
        }
        /* table mode: bit j of cm = the j-th live cluster kept (branch-free body over the compacted terms) */
        const int nLive = __popcll(live);
        /* (round 6) table mode with every lane's pairs fitting the list: the cull and the pair list in one pass over the
         * live clusters -- each cluster's ballot of the lanes keeping it appends their entries at once, in the same
         * cluster-major, lane-ascending order as the separate build below (frame -0.7 %, profiles/r06_p_ab_fused_pairs.log) */
        const bool fused = table && nLive * 64 <= kChainPairs; /* (uniform) */
        /* the same for the per-lane culls of later bounces (more than kDenseCullMax live lanes), in the HITS instantiation
         * only: fsuzane -1 to -2 %, while in the one instantiation of round 6's first try the headline's geometry kernel --
         * which never takes that path -- took 0.8-1.4 % longer from the code it adds (profiles/r06_t / r06_u / r06_v) */
        const bool fusedG = HITS && !firstBounce && !table && !dense && nCl * 64 <= kChainPairs; /* (uniform) */
        if (fusedG) {
            for (int k = 0; k < nCl; ++k) {
                const bool kept = in && !(rhoOk && cluster_culled(pos, dir, rho, dd, P.clusters[c0 + k]));
                cm |= (unsigned)kept << k;
                const unsigned long long m = __ballot(kept);
                if (kept)
                    W.pair[n + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32),
                                                              __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u))] =
                        (unsigned short)(lane | (k << 6));
                n += (int)__popcll(m);
            }
            if (in) /* triangles in the clusters kept (only the scene's last cluster has zero records) */
                tests += (unsigned)__popc(cm) * kClusterSize -
                         (c0 + nCl == P.clusterCount ? ((cm >> (nCl - 1)) & 1u) : 0u) *
                             (unsigned)(P.clusterCount * kClusterSize - P.triCount);
        } else if (fused) {
#pragma unroll 4
            for (int j = 0; j < nLive; ++j) {
                const float4 a = W.cl[j][0], b = W.cl[j][1];
                const ClusterTerms t{V3{a.x, a.y, a.z}, a.w, b.x, b.y};
                const bool kept = in && !(rhoOk && culled_by(t, dir, rho, dd));
                tests += kept ? (unsigned)__popc((unsigned)__float_as_int(b.w)) : 0u;
                const unsigned long long m = __ballot(kept);
                if (kept)
                    W.pair[n + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32),
                                                              __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u))] =
                        (unsigned short)(lane | (j << 6));
                n += (int)__popcll(m);
            }
        } else if (dense) {
        } else if (in && table) {
            /* (round 6: each live cluster's terms by v_readlane from the lane that computed them instead of these LDS
             * reads -- six VALU readlanes per cluster: chain kernel +3 %, frame +2.4 %, profiles/r06_c_ab_*) */
#pragma unroll 4
            for (int j = 0; j < nLive; ++j) {
                const float4 a = W.cl[j][0], b = W.cl[j][1];
                const ClusterTerms t{V3{a.x, a.y, a.z}, a.w, b.x, b.y};
                const bool kept = !(rhoOk && culled_by(t, dir, rho, dd));
                cm |= (unsigned)kept << j;
                tests += kept ? (unsigned)__popc((unsigned)__float_as_int(b.w)) : 0u;
            }
        } else if (in) {
            for (int k = 0; k < nCl; ++k)
                cm |= (unsigned)!(rhoOk && cluster_culled(pos, dir, rho, dd, P.clusters[c0 + k])) << k;
            /* triangles in the clusters kept (only the scene's last cluster has zero records) */
            tests += (unsigned)__popc(cm) * kClusterSize -
                     (c0 + nCl == P.clusterCount ? ((cm >> (nCl - 1)) & 1u) : 0u) *
                         (unsigned)(P.clusterCount * kClusterSize - P.triCount);
        }
        DSECT_END(dc3, 3);
        DSECT_BEGIN(dc4);
        constexpr int kCap = kChainPairs;
        if (dense || fused || fusedG) {
        } else if (table) {
            /* (lane, live cluster) entries, one per cluster a lane keeps; the list is flushed through the passes
             * whenever the next cluster would overflow it */
            for (int j = 0; j < nLive; ++j) {
                const unsigned long long m = __ballot((cm >> j) & 1u);
                if (!m)
                    continue;
                if (n + (int)__popcll(m) > kCap) {
                    wave_lds_sync();
                    chain_pair_passes_cl(n, sRec, P.clusterCount * kClusterSize, W, lane, pos, dir);
                    wave_lds_sync();
                    n = 0;
                }
                if ((cm >> j) & 1u)
                    W.pair[n + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32),
                                                              __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u))] =
                        (unsigned short)(lane | (j << 6));
                n += (int)__popcll(m);
            }
        } else {
            for (int k = 0; k < nCl; ++k) {
                const unsigned long long m = __ballot((cm >> k) & 1u);
                if (!m)
                    continue;
                if (n + (int)__popcll(m) > kCap) {
                    wave_lds_sync();
                    chain_pair_passes<MULTI>(P, n, c0, sRec, W, lane, pos, dir);
                    wave_lds_sync();
                    n = 0;
                }
                if ((cm >> k) & 1u)
                    W.pair[n + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32),
                                                              __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u))] =
                        (unsigned short)(lane | (k << 6));
                n += (int)__popcll(m);
            }
        }
        wave_lds_sync();
        DSECT_END(dc4, 4);
        DSECT_BEGIN(dc5);
        if (table)
            chain_pair_passes_cl(n, sRec, P.clusterCount * kClusterSize, W, lane, pos, dir);
        else
            chain_pair_passes<MULTI>(P, n, c0, sRec, W, lane, pos, dir);
        wave_lds_sync(); /* the pair list is rewritten by the next chunk */
        DSECT_END(dc5, 5);
    }
    const unsigned long long key = W.key[lane];
    Closest c{999999.f, -1};
    if (key != kNoHitKey) {
        c.dst = __uint_as_float((unsigned)(key >> 32));
        c.idx = (int)(unsigned)key;
    }
    return c;
}

/* The deferred half of rtc_render_chain's walk: for each geometry pixel with a slot, its accumulated samples'
 * radiance in sample order (main.c:97-100: acc = acc + calcColor(...) * (1/spp), sequential f32 adds from 0), then
 * vec3ToColor (raytracing.c:11-15).  One lane per pixel.  (Summing a wave's own pixels at the end of
 * rtc_render_chain instead, without this launch, measured 0.477 vs 0.430 ms per frame: the waves' serial tails hold
 * their CUs while the sky pass waits for them.) */
__global__ __launch_bounds__(256) void rtc_accumulate_samples(RenderParams P)
{
    int items = 0;
    for (int l = 0; l < kGeoLists; ++l)
        items += min(P.geoCount[l * kGeoCountStride], P.geoCap);
    items = min(items, P.sampleCap);
    for (int it = blockIdx.x * 256 + threadIdx.x; it < items; it += gridDim.x * 256) {
        const SampleSlot *slot = P.sampleBuf + (size_t)it * (size_t)P.spp;
        f2 accxy{0.f, 0.f};
        float accz = 0.f;
        if (P.maxBounce > 0) {
#pragma unroll 8
            for (int k = 0; k < P.spp; ++k) {
                const SampleSlot v = slot[k];
                accxy = accxy + f2{v.x, v.y};
                accz = accz + v.z;
            }
        }
        const size_t o = (size_t)P.itemPix[it];
        P.colors[3 * o] = float_to_u8(accxy.x);
        P.colors[3 * o + 1] = float_to_u8(accxy.y);
        P.colors[3 * o + 2] = float_to_u8(accz);
        if (P.accum) {
            P.accum[3 * o] = accxy.x;
            P.accum[3 * o + 1] = accxy.y;
            P.accum[3 * o + 2] = accz;
        }
    }
}

/* Primary segments over the tile's candidates (rtc_render_chain) with the filter records staged in LDS (null: from
 * global memory): the filter's record is an LDS read instead of a dependent scalar load per candidate; DevPrimX
 * (survivors only) stays global.  Same operations as closest_primary_listed. */
__device__ __forceinline__ void closest_primary_listed_lds(const RenderParams &P, V3 dir, Closest &c, const unsigned long long *__restrict__ mask,
                                                           unsigned long long m0, unsigned long long m1,
                                                           const DevPrimF *__restrict__ sF, bool staged)
{
    /* m0, m1: the tile's first two mask words, already read (the chain kernel prefetches them one item ahead) */
    const int maskWords = KARG(maskWords);
    const DevPrimF *const primF = KARG(primF);
    const DevPrimX *const primX = KARG(primX);
    for (int w = 0; w < maskWords; ++w) {
        unsigned long long m = w == 0 ? m0 : w == 1 ? m1 : KCONST(mask)[w];
        while (m) {
            const int t = w * 64 + __builtin_ctzll(m);
            m &= m - 1;
            /* two loads of known address space (LDS, or a scalar load): a pointer that may be either would be
             * read with flat loads, whose wait also covers the wave's pending slot stores.  (Requesting the next
             * candidate's record before testing this one, round 6: 1080p shares 2-3 % longer, the frame unchanged,
             * profiles/r06_i_ab_cull_trim_xcd_runs_prefetch.log.) */
            const DevPrimF F = staged ? sF[t] : KLOAD(primF, t);
            if (!prim_backfacing(dir, F) && prim_pass(dir, F) && !(dot(dir, V3{F.nx, F.ny, F.nz}) >= 0.f)) {
                /* the reference's arithmetic (raytracing.c:189-208) */
                const DevPrimX X = KLOAD(primX, t);
                const V3 h = cross(dir, V3{X.acx, X.acy, X.acz});
                const float det = dot(V3{X.abx, X.aby, X.abz}, h);
                if (!(-kEps < det && det < kEps)) {
                    const float invDet = rcp_cr(det); /* IEEE 1.f / det */
                    const float u = dot(V3{X.s0x, X.s0y, X.s0z}, h) * invDet;
                    const float v = dot(dir, V3{X.q0x, X.q0y, X.q0z}) * invDet;
                    const float dst = X.dac0 * invDet;
                    if (!(u < 0.f || u > 1.f) && !(v < 0.f || u + v > 1.f) && !(dst < kEps) && dst < c.dst) {
                        c.dst = dst;
                        c.idx = t;
                    }
                }
            }
        }
    }
}

/* rtc_render_chain<SPHERES>: calculateRayCollision's sphere loop (raytracing.c:219-228) before the triangles
 * -- the spheres in index order, each replacing the closest so far only when strictly closer, from 999999; the exact
 * ray_sphere.  The loop is wave-uniform and the records are scalar loads.  A sphere's index in a Closest is
 * kChainSphereBase + i (triangle indices stay their own: the tile cull admits fewer than 2^19 triangles), so the triangle
 * traces that follow -- which replace only when strictly closer, or are compared afterwards -- keep the reference's order:
 * spheres first, then triangles by index. */
constexpr int kChainSphereBase = 1 << 30;
__device__ __forceinline__ void closest_spheres(const RenderParams &P, V3 pos, V3 dir, Closest &c)
{
    const DevSphere *const spheres = KARG(spheres);
    const int n = KARG(sphereCount);
    for (int i = 0; i < n; ++i) {
        const DevSphere sp = KLOAD(spheres, i);
        float d;
        if (ray_sphere(pos, dir, V3{sp.cx, sp.cy, sp.cz}, sp.radius, d) && d < c.dst) {
            c.dst = d;
            c.idx = kChainSphereBase + i;
        }
    }
}

/* rtc_render_chain's dynamic LDS: the clustered records (MULTI: none), then, when the block's budget allows
 * (P.chainPrimF), the primary filter records.  (Staging the primary exact records and the shading records as well
 * measured no faster.) */
struct ChainStage {
    float4 *rec; /* structure-of-arrays (rec_soa) */
    DevPrimF *primF;
};
template <bool MULTI>
__device__ __forceinline__ ChainStage chain_stage(const RenderParams &P, unsigned char *sDyn)
{
    ChainStage S{nullptr, nullptr};
    if (!MULTI)
        S.rec = (float4 *)sDyn;
    if (P.chainPrimF)
        S.primF = (DevPrimF *)(sDyn + (MULTI ? 0 : (size_t)soa_slots(P.clusterCount * kClusterSize) * sizeof(DevTri)));
    const int nRec = P.clusterCount * kClusterSize, slots = soa_slots(nRec);
    for (int i = threadIdx.x; S.rec && i < nRec; i += kChainBlock) {
        const float4 *g = (const float4 *)(P.clTris + i);
        for (int k = 0; k < 4; ++k)
            S.rec[k * slots + i] = g[k];
    }
    for (int i = threadIdx.x; S.primF && i < P.triPadded; i += kChainBlock)
        S.primF[i] = P.primF[i];
    return S;
}

/* COUNT: the launch asks for segment counters (instrumentation, untimed); without it the counters are compiled out */
/* MULTI: more than one chunk of clusters (chunk-level culling, records from global).  GENERAL (round 6): the launch may give
 * items deferred sample slots (P.sampleCap > 0: joined whole frames), hoist the primary segments (P.hoist) or read the
 * primary filter records from global memory (!P.chainPrimF: too large to stage); without it every item sums in-kernel
 * and traces its primary ray per sample over the staged records, and none of the other code is in the kernel -- the pipelined faithful launches' instantiation, whose registers and schedule are then its own
 * (without the slot code: frame -0.8 %, chain -1.4 %, 1/8 share -2 %, profiles/r06_w_ab_defer_specialisation.log).
 * Counting launches always take GENERAL.  HITS: the fast instantiation of scenes whose bounces often hit again (the
 * upload's bounce_hit_share above kWgsHitShare, e.g. C3 fsuzane), with the later bounces' one-pass cull and pair build
 * (chain_trace_pairs); the other scenes' instantiation does not carry that code.  SPHERES (GENERAL launches only): the
 * launch renders P.sphereCount > 0 spheres (closest_spheres before the primary trace and before every bounce trace, the
 * sphere's normal and material at a sphere hit); a hit draws the same 7 values on a sphere as on a triangle
 * (RandomDiretion and the roulette), so the state-indexed chain, the draw table and the walk are unchanged.  Without it
 * none of that code is in the kernel. */
/* RESUME (GENERAL launches only; DESIGN §3.8, a pass of rtc_render_samples_async): P.spp is the pass's sample count.  When the
 * pass is not the frame's first, the item's seed is the pixel's stored state -- the reference's rngState after the samples
 * so far, so the chain S_j of the remaining samples is indexed from it exactly as the whole frame's is from x + y * width --
 * and an item that sums in-kernel starts from the stored accumulator (a deferred item's sum: rtc_accumulate_samples_resume).
 * At the item's end one lane stores the state 7 jn draws on: jn is the chain's position after the pass's last sample, the
 * hits so far (a primary miss or maxBounce == 0 leaves jn = 0, the state where it was). */
/* DRAWS (the two kernels without the GENERAL code only; the draw cache, rtc_params.h DrawCache): an item's block number comes
 * with its record through the one-item-ahead prefetch (P.itemDraw, lanes 4..7 of the record load).  For an item with a block,
 * lane l requests entry l of the block (one global_load_dwordx4) at the item's start, as soon as the block is known, and the
 * primary hit of the item's first window (jn == 0) takes that value -- the same function of (seed, l) that it would compute
 * -- in place of Box-Muller, and enters it in W.draw as before.  Windows with jn > 0, lanes past the window's active ones
 * and items without a block compute, on wave-uniform branches.  (The seed is the pixel index there: no RESUME.) */
template <bool MULTI, bool COUNT, bool HITS, bool GENERAL, bool SPHERES = false, bool RESUME = false, bool DRAWS = false>
__global__ __launch_bounds__(kChainBlock) __attribute__((amdgpu_waves_per_eu(RTC_CHAIN_WAVES))) void rtc_render_chain(
    RenderParams P)
{
    if (RTC_CHAIN_PRIO > 0)
        __builtin_amdgcn_s_setprio(RTC_CHAIN_PRIO);
    DSECT_BEGIN(dtot);
    DMARK_INIT(dcur);
#ifdef RTC_DIAG
    const unsigned long long dWaveT0 = __builtin_amdgcn_s_memrealtime();
    unsigned dWaveItems = 0;
    unsigned long long dItemEnd[5] = {0, 0, 0, 0, 0};
#endif
    extern __shared__ __attribute__((aligned(64))) unsigned char sDyn[];
    __shared__ PowTablesLds sPow;
    __shared__ ChainWaveLds sWave[kChainBlock / 64];
    __shared__ int sWork; /* the workgroup's next item (see below) */
    __shared__ DevCluster sCl[kChunkClusters]; /* single-chunk scenes: the clusters, for the dense culls */
    if (!MULTI && threadIdx.x < P.clusterCount && threadIdx.x < kChunkClusters)
        sCl[threadIdx.x] = P.clusters[threadIdx.x];
    if (threadIdx.x == 0)
        sWork = 0;
    sPow.fill(threadIdx.x);
    const ChainStage S = chain_stage<MULTI>(P, sDyn);
    const float4 *sRec = S.rec;
    /* the staged primary filter records: always the LDS address (never null), used when P.chainPrimF */
    const DevPrimF *sPF = (const DevPrimF *)(sDyn + (MULTI ? 0 : (size_t)soa_slots(P.clusterCount * kClusterSize) * sizeof(DevTri)));
    const bool pfStaged = !GENERAL || P.chainPrimF != 0; /* (the fast instantiation runs only with the records staged) */
#ifdef RTC_DIAG
    if ((threadIdx.x & 63) < kDiagSects)
        s_rtc_sect[threadIdx.x >> 6][threadIdx.x & 63] = 0;
    static_assert(kChainBlock / 64 <= 4, "s_rtc_sect holds four waves");
#endif
    __syncthreads();
    sPow.attach(P.env);
    const int lane = threadIdx.x & 63;
    ChainWaveLds &W = sWave[threadIdx.x >> 6];
    const RngJump laneJump = rng_jump_by(7u * (unsigned)lane); /* s -> the state 7 lane draws later */
    /* the geometry pixels: kGeoLists sub-lists from rtc_tile_cull, taken as one concatenated index space
     * (l: the sub-list of item `it`, base: its first item).  Workgroup b owns the items b + k * gridDim.x; its
     * waves take the next k from an LDS counter, so a wave that drew cheap pixels takes more of them (a global
     * counter would serialise ~80 k same-address atomics across the XCDs; per-XCD returning counters, round 3,
     * shortened the kernel 4 % but made every workgroup retire at its end, so the sky pass no longer filled the
     * tail: frame 0.396 -> 0.42 ms). */
    int nextIt = 0;
    /* (Global item counters instead, round 5: the kernel 6 % shorter, the frame 3-4 % longer -- the sky pass no longer
     * fills its tail -- and small shares 17-28 % longer.  Items grouped by XCD, round 6 -- XCD group b % 8 taking the
     * (b % 8)-th eighth of the list, so that a tile's neighbouring pixels share an L2: frame 0.333 -> 0.358 ms, 1/8 share
     * 0.068 -> 0.079 ms, profiles/r06_c_ab_xcd_items_readlane_cull.log.) */
    /* (Runs of G / 8 consecutive items per XCD in every round of G = gridDim.x items, round 6 -- a tile's pixels under
     * one L2, so that their Color bytes merge before write-back: 1080p 1/4 and 1/8 shares 2-3 % longer, fsuzane +1 %,
     * profiles/r06_i_ab_cull_trim_xcd_runs_prefetch.log.) */
    const auto next_item = [&]() { return (int)blockIdx.x + atomicAdd(&sWork, 1) * (int)gridDim.x; };
    if (lane == 0)
        nextIt = next_item();
    /* (the launch constants below that are used once per item, window or escaped bounce are re-read from the kernarg
     * segment where they are used: KARG) */
#ifdef RTC_DIAG_COUNT /* diagnostic variant: the test counters on in every launch (rtc_diag_itemlog's tests) */
    constexpr bool counting = true;
#else
    constexpr bool counting = COUNT;
#endif
    unsigned segCalls = 0, segTraced = 0, segClusters = 0;
    unsigned long long segTests = 0, segSpec = 0;
#ifdef RTC_DIAG
    unsigned long long dIters = 0, dAlive = 0, dAct = 0, dWindows = 0, dUsed = 0, dIters2 = 0, dAlive2 = 0;
#endif
    /* the sub-lists' inclusive prefix counts, lane l < kGeoLists holding sub-list l's, loaded once per wave: an
     * item's sub-list is then a ballot, not a chain of dependent count loads as a wave's items pass the sub-lists */
    int incl = lane < kGeoLists ? min(P.geoCount[lane * kGeoCountStride], P.geoCap) : 0;
#pragma unroll
    for (int d = 1; d < kGeoLists; d <<= 1) {
        const int v = __shfl_up(incl, d);
        if (lane >= d)
            incl += v;
    }
    const int nItems = __builtin_amdgcn_readlane(incl, kGeoLists - 1);
    /* Prefetch (round 5): an item's record and its tile's first two mask words were written by the tile cull on
     * other XCDs, so their first reads miss this XCD's L2; read as scalar loads at the item's start they were a chain
     * of dependent misses on the critical path of every item (round-4 stamps: item setup 17 % of the waves' lifetime).
     * Here they are VECTOR loads issued one item ahead: the next item's record (lane j: dword j & 3 of it, so the
     * address differs by lane and the load is a vector one) at this item's start, its tile's mask dwords (lane j < 4:
     * dword j) at this item's first bounce iteration, once the record is back.  Vector loads return in order and are
     * waited for by vmcnt, so a scalar wait never completes them early.  Each lives in one register that is consumed
     * before it is reloaded (a loop-carried copy of an in-flight load would wait for it at the copy), and neither is in
     * flight at a loop preheader that flushes vmcnt (after the bounce loop, the walk's did). */
    const auto entry_of = [&](int it2) -> size_t {
        const int l = (int)__popcll(__ballot(lane < kGeoLists && incl <= it2));
        const int base = l ? __builtin_amdgcn_readlane(incl, l - 1) : 0;
        return (size_t)l * KARG(geoCap) + (size_t)(it2 - base);
    };
    static_assert(!DRAWS || (!GENERAL && !RESUME && !SPHERES && !MULTI && !COUNT), "the draw cache: the kernels without GENERAL");
    const auto record_dwords = [&](int it2) -> unsigned {
        if constexpr (DRAWS) { /* lanes 4..7 of every eight: the item's block + 1 (P.itemDraw), by the same load */
            const size_t e = entry_of(it2);
            const unsigned *const rec = KARG(geoList) + e * (size_t)kItemRecDwords + (size_t)(lane & (kItemRecDwords - 1));
            const unsigned *const blk = KARG(itemDraw) + e;
            return gload((lane & kItemRecDwords) ? blk : rec, 0);
        }
        return gload(KARG(geoList), entry_of(it2) * (size_t)kItemRecDwords + (size_t)(lane & (kItemRecDwords - 1)));
    };
    /* the tile of a record (its dword 0, item_record) */
    const auto record_tile = [&](unsigned d0) -> int {
        return KARG(wideItems) ? (int)(d0 >> 6) : (int)(d0 >> 19) * (KARG(blocksX) * 2) + (int)((d0 & 0xffffu) >> 3);
    };
    const auto mask_dwords = [&](unsigned d0) -> unsigned {
        const unsigned *mw = (const unsigned *)(KARG(tileMask) + (size_t)record_tile(d0) * P.maskWords);
        return lane < 2 * P.maskWords && lane < 4 ? gload(mw, (size_t)lane) : 0u;
    };
    int it = __builtin_amdgcn_readfirstlane(nextIt);
    unsigned vc = 0, vm = 0; /* the current item's record and mask dwords (vector registers) */
    if (it < nItems) {
        vc = record_dwords(it);
        vm = mask_dwords((unsigned)__builtin_amdgcn_readfirstlane((int)vc));
    }
    if (lane == 0)
        nextIt = next_item();
    DMARK(dcur, 19); /* prologue: staging, tables, the first item */
    for (;;) {
        if (it >= nItems)
            break;
#ifdef RTC_DIAG
        const unsigned long long dItemT0 = __builtin_amdgcn_s_memrealtime();
        unsigned dItemWindows = 0;
        const unsigned long long dItemIters0 = dIters;
        const unsigned dBm0 = __atomic_load_n(&g_rtc_bmfall[(blockIdx.x * (kChainBlock / 64) + (threadIdx.x >> 6)) & 65535u],
                                              __ATOMIC_RELAXED);
        const unsigned long long dSect = lane < kItemSects ? s_rtc_sect[threadIdx.x >> 6][item_sect_id(lane)] : 0ull;
        unsigned long long dItemTests = 0;
#endif
        const unsigned d0 = (unsigned)__builtin_amdgcn_readfirstlane((int)vc);
        /* the pixel's primary direction (main.c:88-94), as the tile cull's lane formed it (item_record) */
        const V3 pdir{__uint_as_float((unsigned)__builtin_amdgcn_readlane((int)vc, 1)),
                      __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)vc, 2)),
                      __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)vc, 3))};
        const unsigned long long m0 = (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)vm, 0) |
                                      (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)vm, 1) << 32;
        const unsigned long long m1 = (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)vm, 2) |
                                      (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)vm, 3) << 32;
        /* DRAWS: the item's cached draws, entry `lane` of its block, requested here and consumed at the primary hit of the
         * item's first window (four registers live across the primary trace, which is scalar work) */
        float4 cachedDraw = make_float4(0.f, 0.f, 0.f, 0.f);
        unsigned drawBlock = 0;
        if constexpr (DRAWS) {
            drawBlock = (unsigned)__builtin_amdgcn_readlane((int)vc, kItemRecDwords);
            if (drawBlock) /* (uniform) */
                cachedDraw = gload4(KARG(drawPool), (size_t)(drawBlock - 1u) * kDrawEntries + (size_t)lane);
        }
        /* the next item: its number (the LDS counter read at this item's previous start), its entry, and the counter for
         * the one after */
        const int itNext = __builtin_amdgcn_readfirstlane(nextIt);
        if (itNext < nItems)
            vc = record_dwords(itNext);
        /* the next item's mask dwords requested (none needed past the end) */
        bool maskNext = itNext >= nItems;
        if (lane == 0)
            nextIt = next_item();
        const int tile = record_tile(d0);
        int x = (int)(d0 & 0xffffu), r = (int)(d0 >> 16);
        if (KARG(wideItems)) { /* (uniform; launches of more than 65,535 columns or launch rows) */
            const int tilesX = KARG(blocksX) * 2, bit = (int)(d0 & 63u);
            x = (tile % tilesX) * 8 + (bit & 7), r = (tile / tilesX) * 8 + (bit >> 3);
        }
        const int sh = KARG(rowBandShift); /* launch_row_y */
        const int y = KARG(rowStart) + ((r >> sh) * KARG(rowStride) << sh) + (r & ((1 << sh) - 1));
        const unsigned long long *mask = KARG(tileMask) + (size_t)tile * P.maskWords;
        unsigned L = 0;
        if (counting)
            for (int w = 0; w < P.maskWords; ++w)
                L += (unsigned)__popcll(mask[w]);
        unsigned seedOf = (unsigned)(x + y * KARG(width)); /* main.c:95 */
        if constexpr (RESUME) {
            if (KARG(sampleFirst) > 0) /* (uniform; every lane loads the pixel's dword) */
                seedOf = (unsigned)__builtin_amdgcn_readfirstlane(
                    (int)gload(KARG(rngState), (size_t)r * (size_t)KARG(width) + (size_t)x));
        }
        const unsigned seed = seedOf;
        const bool deferred = GENERAL && it < P.sampleCap; /* wave-uniform */
        Closest prim{999999.f, -1};
        if (GENERAL && P.hoist && P.spp > 0 && P.maxBounce > 0) {
            if constexpr (SPHERES)
                closest_spheres(P, KARG(origin), pdir, prim);
            closest_primary_listed_lds(P, pdir, prim, mask, m0, m1, sPF, pfStaged);
            if (counting && lane == 0) {
                segTraced++;
                segTests += L;
            }
        }
        DMARK(dcur, 15); /* item setup */
        /* in-kernel sums (items without a deferred slot): the pixel's accumulator (main.c:97), component c in lane c */
        float acc = 0.f;
        if constexpr (RESUME) {
            if (KARG(sampleFirst) > 0 && !deferred && lane < 3)
                acc = __uint_as_float(gload(KARG(accum), 3 * ((size_t)r * (size_t)KARG(width) + (size_t)x) + (size_t)lane));
        }
        int k = 0;       /* samples accumulated */
        unsigned jn = 0; /* state index (in units of 7 draws) of sample k */
        while (k < P.spp && P.maxBounce > 0) {
            /* window: the state indices the remaining samples likely span (the pixel's hits per sample so far, a
             * margin; the first window assumes one hit per sample) */
            const int need = P.spp - k;
            const int est = k > 0 ? (int)(((unsigned long long)need * jn + (unsigned)k - 1u) / (unsigned)k) : need;
            const int nAct = min(64, est + (est >> 3) + 1);
            const bool act = lane < nAct;
            /* the lane's start state: the seed advanced by 7 (jn + lane) draws = the wave-uniform state at jn,
             * then this lane's fixed jump by 7 lane draws (both affine LCG compositions, rng_advance) */
            const unsigned s0 = (unsigned)__builtin_amdgcn_readfirstlane((int)rng_advance(seed, 7u * jn));
            unsigned rng = s0 * laneJump.a + laneJump.c;
            DMARK(dcur, 0); /* window setup */
            /* ---- S_{jn + lane}: one calcColor (raytracing.c:262-296) ---- */
            V3 pos = KARG(origin), dir = pdir, rayColor{1.f, 1.f, 1.f}, light{0.f, 0.f, 0.f};
            int bounce = 0;
            unsigned hits = 0, calls = 0, tests = 0, clTests = 0;
            bool alive = act;
            for (int iter = 0; __any(alive); ++iter) {
                const bool first = iter == 0, bounce1 = iter == 1; /* wave-uniform */
#ifdef RTC_DIAG
                dIters++;
                dAlive += (unsigned long long)__popcll(__ballot(alive));
                if (iter >= 2) {
                    dIters2++;
                    dAlive2 += (unsigned long long)__popcll(__ballot(alive));
                }
#endif
                Closest c{999999.f, -1};
                if (first) { /* every live lane: the pixel's primary ray (bounce 0) */
                    if (alive) {
                        if (GENERAL && P.hoist) {
                            c = prim;
                        } else {
                            if constexpr (SPHERES)
                                closest_spheres(P, pos, dir, c);
                            closest_primary_listed_lds(P, dir, c, mask, m0, m1, sPF, pfStaged);
                            if (counting)
                                tests += L;
                        }
                    }
                    DMARK(dcur, 1); /* primary trace */
                } else { /* bounce segments of the live lanes (the whole wave takes part) */
                    if (!maskNext) { /* the next item's mask dwords (see the prefetch above) */
                        vm = mask_dwords((unsigned)__builtin_amdgcn_readfirstlane((int)vc));
                        maskNext = true;
                    }
                    unsigned t = 0;
                    if constexpr (SPHERES) {
                        /* the spheres first, every lane (a retired lane's result is not used); then the wave's triangle
                         * trace, whose hit replaces the sphere's only when strictly closer (raytracing.c:231).  A scene
                         * without triangles (no cluster) has no triangle trace */
                        Closest cs{999999.f, -1};
                        closest_spheres(P, pos, dir, cs);
                        if (P.clusterCount > 0) /* (uniform) */
                            c = chain_trace_pairs<MULTI, COUNT, HITS>(P, alive, bounce1, pos, dir, sRec, W, lane, t, sCl);
                        else
                            wave_lds_sync(); /* (the draw table's entries, as chain_trace_pairs' syncs order them) */
                        if (!(c.idx >= 0 && c.dst < cs.dst))
                            c = cs;
                    } else {
                        c = chain_trace_pairs<MULTI, COUNT, HITS>(P, alive, bounce1, pos, dir, sRec, W, lane, t, sCl);
                    }
                    if (counting && alive) {
                        tests += t;
                        clTests += (unsigned)P.clusterCount;
                    }
                    DMARK(dcur, bounce1 ? 17 : 20); /* bounce trace: the first bounce (17), later ones (20); 14 table, 3
                                                     * cull, 4 pair build, 5 pair passes inside */
                }
                /* the state advance of this iteration's hits (7 draws per earlier hit), for lanes past the draw table */
                RngJump J{1u, 0u};
                if (!first && __ballot(alive && c.idx >= 0 && lane + iter >= nAct))
                    J = rng_jump_by(7u * (unsigned)iter); /* wave-uniform */
                if (alive) {
                    if (counting)
                        calls++;
                    bool endSample;
                    if (c.idx >= 0) {
                        DSECT_BEGIN(dc2);
                        hits++;
                        /* calcColor hit branch, raytracing.c:272-287 */
                        const V3 hitPoint = add(pos, mul(dir, c.dst)); /* raytracing.c:238 */
                        V3 normal{0.f, 0.f, 0.f}, color{0.f, 0.f, 0.f};
                        float emission = 0.f, smoothness = 0.f;
                        bool onSphere = false;
                        if constexpr (SPHERES) {
                            /* a sphere hit: normal = normalized(hitPoint - centre) (raytracing.c:182), the sphere's
                             * material; at the primary hit the winner is the same in every lane (scalar loads) */
                            DevSphere sp;
                            if (first) {
                                const int u = __builtin_amdgcn_readfirstlane(c.idx);
                                onSphere = u >= kChainSphereBase; /* (uniform) */
                                if (onSphere)
                                    sp = KLOAD(KARG(spheres), u - kChainSphereBase);
                            } else {
                                onSphere = c.idx >= kChainSphereBase;
                                if (onSphere)
                                    sp = P.spheres[c.idx - kChainSphereBase];
                            }
                            if (onSphere) {
                                normal = normalized(sub(hitPoint, V3{sp.cx, sp.cy, sp.cz}));
                                color = V3{sp.r, sp.g, sp.b};
                                emission = sp.emission;
                                smoothness = sp.smoothness;
                            }
                        }
                        if (!onSphere) {
                            DevTri T;
                            DevMat M;
                            if (first) { /* the pixel's primary hit: the same triangle in every lane */
                                const int u = __builtin_amdgcn_readfirstlane(c.idx);
                                T = KLOAD(KARG(tris), u);
                                M = KLOAD(KARG(mats), u);
                            } else {
                                T = P.tris[c.idx]; /* (kernel-argument pointers: global loads, not flat) */
                                M = P.mats[c.idx];
                            }
                            normal = V3{T.nx, T.ny, T.nz};
                            color = V3{M.r, M.g, M.b};
                            emission = M.emission;
                            smoothness = M.smoothness;
                        }
                        /* the hit draws (see ChainWaveLds::draw): the primary hit computes the lane's own and enters
                         * them in the table (every active lane hits there: one primary ray per wave); a later hit
                         * reads entry lane + iter, or computes it when that is past the window's active lanes */
                        float4 D;
                        if (first || lane + iter >= nAct) {
                            if (DRAWS && first && drawBlock != 0u && jn == 0u) { /* (uniform) the cached entry `lane` */
                                D = cachedDraw;
                            } else {
                                unsigned s = first ? rng : rng * J.a + J.c;
                                const V3 rd = random_direction(s);
                                D = make_float4(rd.x, rd.y, rd.z, random_value(s));
                            }
                            if (first)
                                W.draw[lane] = D; /* read in later iterations, after chain_trace_pairs' LDS syncs */
                        } else {
                            D = W.draw[lane + iter];
                        }
                        const V3 diffuseDir = normalized(add(normal, V3{D.x, D.y, D.z}));
                        const V3 specularDir = reflect(dir, normal);
                        dir = lerp(diffuseDir, specularDir, smoothness);
                        pos = hitPoint;
                        const V3 emitted = mul(color, emission);
                        light = add(light, mulv(emitted, rayColor));
                        rayColor = mulv(rayColor, color);
                        const float p = fmax_ref(fmax_ref(rayColor.x, rayColor.y), rayColor.z);
                        endSample = p < D.w;
                        if (!endSample) {
                            rayColor = mul(rayColor, rcp_cr(p)); /* (float)(1.0 / p) */
                            bounce++;
                            endSample = bounce >= P.maxBounce;
                        }
                        DSECT_END(dc2, 2);
                    } else {
                        DSECT_BEGIN(dc6);
                        EnvParams env = KARG(env); /* the launch's sky and sun, the powf tables in LDS */
                        sPow.attach(env);
                        light = add(light, mulv(environment(dir, env), rayColor)); /* raytracing.c:291 */
                        endSample = true;
                        DSECT_END(dc6, 6);
                    }
                    if (endSample)
                        alive = false;
                }
                DMARK(dcur, iter < 2 ? 16 : 21); /* shading (2 hit, 6 environment inside); 21: after later bounces */
            }
            (void)bounce;
            /* ---- walk the chain through the window, accumulating in sample order (main.c:99) ---- */
            const V3 t = mul(light, KARG(invSpp)); /* calcColor(...) * (float)(1./spp), main.c:99 */
            const unsigned long long ones = __ballot(act && hits == 1u);
            unsigned mult = 0; /* how many accumulated samples this lane's S_j is */
            int p = 0;
            SampleSlot *slot = P.sampleBuf + (size_t)it * (size_t)P.spp;
            /* in-kernel sums: the window's samples are staged in sample order in LDS -- the pair list's space, free
             * until the next window's bounces; component c of staged sample i at stage[c kStageRow + i] (kStageRow, above:
             * its padding and the banks) -- and lane c then adds its row in order, main.c:99's sequential f32 adds.  The
             * row comes into registers four samples per ds_read_b128, ahead of the adds, so that the dependent adds issue
             * back to back instead of each batch of eight waiting for its own LDS round trip (until round 14:
             * stage[3 i + c], dword reads threaded between the 64 adds of a full window).  The last quad of a count that is no multiple of four is
             * read whole and only its staged entries are added: the other dwords are whatever the pair list left there.
             * Both syncs stay: the first orders the staging writes before the reads; the second the reads before the
             * space's next writer, another lane -- the next window's pair build, or a staging run after a mid-window flush */
            float *const stage = (float *)W.pair;
            int staged = 0;
            /* full: the call may see a full window (the flush at the window's end; a flush mid-window follows a lane
             * that was not staged, so fewer than 64 are) */
            auto flush = [&](const bool full) {
                DSECT_BEGIN(df0);
                wave_lds_sync();
                DSECT_END(df0, 25);
                DSECT_BEGIN(df1);
                if (full && staged == 64) { /* (uniform) every window of a frame of one-hit pixels: no loop */
                    if (lane < 3) {
                        const float4 *row = (const float4 *)(stage + lane * kStageRow);
                        /* groups of kGroup quads, the next group requested before this one's adds: the kernels without
                         * the GENERAL code hold the whole row (64 registers, all 16 reads ahead of the first add), the
                         * GENERAL ones, which have no registers to spare, two groups of four quads at a time */
                        constexpr int kGroup = GENERAL ? 4 : 16;
                        float4 v[16];
#pragma unroll
                        for (int g = 0; g < kGroup; ++g)
                            v[g] = row[g];
#pragma unroll
                        for (int g0 = 0; g0 < 16; g0 += kGroup) {
#pragma unroll
                            for (int g = g0 + kGroup; g < 16 && g < g0 + 2 * kGroup; ++g)
                                v[g] = row[g];
#pragma unroll
                            for (int g = g0; g < g0 + kGroup; ++g) {
                                acc = acc + v[g].x;
                                acc = acc + v[g].y;
                                acc = acc + v[g].z;
                                acc = acc + v[g].w;
                            }
                        }
                    }
                } else if (lane < 3) {
                    /* every other count: whole quads with the next one requested before this one's adds (the quad after
                     * the last whole one lies inside the padded row), then the 1..3 staged entries of the last quad */
                    const float4 *row = (const float4 *)(stage + lane * kStageRow);
                    float4 v = row[0];
                    int i = 0;
                    for (; i + 4 <= staged; i += 4) {
                        const float4 nx = row[(i >> 2) + 1];
                        acc = acc + v.x;
                        acc = acc + v.y;
                        acc = acc + v.z;
                        acc = acc + v.w;
                        v = nx;
                    }
                    if (i < staged)
                        acc = acc + v.x;
                    if (i + 1 < staged)
                        acc = acc + v.y;
                    if (i + 2 < staged)
                        acc = acc + v.z;
                }
                DSECT_END(df1, 26);
                DSECT_BEGIN(df2);
                wave_lds_sync();
                DSECT_END(df2, 27);
                staged = 0;
            };
            DSECT_BEGIN(dwalk);
            while (k < P.spp && p < nAct) {
                const unsigned long long win = (nAct >= 64 ? ~0ull : ((1ull << nAct) - 1ull)) & (~0ull << p);
                const unsigned long long notOne = ~ones & win;
                const int q = notOne ? __builtin_ctzll(notOne) : nAct;
                const int take = min(q - p, P.spp - k);
                /* a run of one-hit samples: j advances by 1 */
                if (deferred) {
#ifndef RTC_AB_NO_SLOTS /* timing experiment only (the deferred slots' cost): nothing stored, no sum pass */
                    if (lane >= p && lane < p + take)
                        slot[k + lane - p] = SampleSlot{t.x, t.y, t.z};
#endif
                } else {
                    if (lane >= p && lane < p + take) {
                        const int i = (staged + lane - p) * kStageLaneStride;
                        stage[i] = t.x;
                        stage[kStageRow + i] = t.y;
                        stage[2 * kStageRow + i] = t.z;
                    }
                    staged += take;
                }
                mult += (lane >= p && lane < p + take) ? 1u : 0u;
                k += take;
                p += take;
                if (k >= P.spp || p != q || q >= nAct)
                    break;
                /* lane q: a sample with h != 1 (two or more hits, or none when the primary ray misses) */
                const int hq = __builtin_amdgcn_readlane((int)hits, q);
                const float qx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t.x), q));
                const float qy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t.y), q));
                const float qz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t.z), q));
                const int m = hq == 0 ? P.spp - k : 1; /* a primary miss: every remaining sample is this one */
                if (deferred) {
                    for (int kk = k + lane; kk < k + m; kk += 64)
                        slot[kk] = SampleSlot{qx, qy, qz};
                } else if (m == 1) {
                    if (lane == q) {
                        stage[staged] = t.x;
                        stage[kStageRow + staged] = t.y;
                        stage[2 * kStageRow + staged] = t.z;
                    }
                    ++staged;
                } else { /* the staged samples first, then this one m times */
                    flush(false);
                    const float v = lane == 0 ? qx : (lane == 1 ? qy : qz);
                    for (int b = 0; b < m; ++b)
                        acc = acc + v;
                }
                mult += lane == q ? (unsigned)m : 0u;
                k += m;
                if (hq == 0)
                    break;
                p = q + hq;
            }
            DSECT_END(dwalk, 24); /* 24 the walk and its staging; 25 sync, 26 reads and adds, 27 sync inside flush() */
            if (!deferred)
                flush(true);
            jn += (unsigned)p;
#ifdef RTC_DIAG
            {
                unsigned long long tw = act ? tests : 0u;
                for (int o = 32; o > 0; o >>= 1)
                    tw += __shfl_xor(tw, o);
                dItemTests += tw;
            }
            dItemWindows++;
            dWindows++;
            dAct += (unsigned)nAct;
            dUsed += (unsigned long long)__popcll(__ballot(mult > 0));
#endif
            /* counters: committed samples (with multiplicity) and the tests of the discarded ones */
            if (counting) {
                segCalls += mult * calls;
                segTraced += mult * (P.hoist ? calls - 1u : calls);
                segTests += (unsigned long long)mult * tests;
                segClusters += mult * clTests;
                if (act && mult == 0)
                    segSpec += tests;
            }
            DMARK(dcur, 7); /* walk and sums */
        }
        if constexpr (RESUME) {
            if (lane == 0)
                P.rngState[(size_t)r * (size_t)KARG(width) + (size_t)x] = rng_advance(seed, 7u * jn);
        }
        if (deferred) {
            if (lane == 0)
                P.itemPix[it] = r * KARG(width) + x;
        } else if (!RESUME && P.geoColor) { /* merged sky pass: the pixel's three bytes as one word of its item */
            const unsigned b = float_to_u8(acc);
            const unsigned w = (unsigned)__builtin_amdgcn_readlane((int)b, 0) |
                               (unsigned)__builtin_amdgcn_readlane((int)b, 1) << 8 |
                               (unsigned)__builtin_amdgcn_readlane((int)b, 2) << 16;
            if (lane == 0)
                P.geoColor[it] = w;
            if (lane < 3 && P.accum)
                P.accum[3 * ((size_t)r * (size_t)KARG(width) + (size_t)x) + (size_t)lane] = acc;
        } else if (lane < 3) {
            const size_t o = 3 * ((size_t)r * (size_t)KARG(width) + (size_t)x) + (size_t)lane;
            P.colors[o] = float_to_u8(acc);
            if (P.accum)
                P.accum[o] = acc;
        }
        if (!maskNext) /* (an item without a bounce iteration) */
            vm = mask_dwords((unsigned)__builtin_amdgcn_readfirstlane((int)vc));
#ifdef RTC_DIAG
        if (lane == 0 && it < kItemLog) {
            g_rtc_itemlog[it][0] = dItemT0;
            g_rtc_itemlog[it][1] = __builtin_amdgcn_s_memrealtime();
            g_rtc_itemlog[it][2] = (unsigned long long)dItemWindows |
                                   (unsigned long long)(__popcll(m0) + __popcll(m1)) << 16 |
                                   (unsigned long long)(blockIdx.x * (kChainBlock / 64) + (threadIdx.x >> 6)) << 32;
            const unsigned dBm1 = __atomic_load_n(
                &g_rtc_bmfall[(blockIdx.x * (kChainBlock / 64) + (threadIdx.x >> 6)) & 65535u], __ATOMIC_RELAXED);
            g_rtc_itemlog[it][3] = (dIters - dItemIters0) | (unsigned long long)(dBm1 - dBm0) << 16 | dItemTests << 32;
        }
        if (it < kItemSectLog && lane < kItemSects)
            g_rtc_itemsect[it][lane] = (unsigned)(s_rtc_sect[threadIdx.x >> 6][item_sect_id(lane)] - dSect);
#endif
        it = itNext;
#ifdef RTC_DIAG
        if (dWaveItems < 5)
            dItemEnd[dWaveItems] = __builtin_amdgcn_s_memrealtime();
        dWaveItems++;
#endif
        DMARK(dcur, 18); /* item tail: the pixel's colour */
    }
    DMARK(dcur, 15);
#ifdef RTC_DIAG
    DSECT_END(dtot, 13);
    {
        /* per-slot plain stores (see g_rtc_sectw): lanes 0..7, 13..21 the sections, 8..12 and 22, 23 the window statistics */
        const unsigned slotW = (blockIdx.x * (kChainBlock / 64) + (threadIdx.x >> 6)) % (unsigned)kWaveLog;
        unsigned long long v = lane < kDiagSects ? s_rtc_sect[threadIdx.x >> 6][lane] : 0ull;
        v = lane == 8 ? dIters : lane == 9 ? dAlive : lane == 10 ? dAct : lane == 11 ? dWindows : lane == 12 ? dUsed : v;
        v = lane == 22 ? dIters2 : lane == 23 ? dAlive2 : v;
        if (lane < kDiagSects)
            g_rtc_sectw[slotW][lane] = v;
    }
#endif
    if (counting)
        flush_counters(P, segCalls, segTraced, segTests, lane, segClusters, segSpec);
#ifdef RTC_DIAG
    if (lane == 0) {
        const unsigned w = (blockIdx.x * (kChainBlock / 64) + (threadIdx.x >> 6)) % (unsigned)kWaveLog;
        g_rtc_wavelog[w][0] = dWaveT0;
        g_rtc_wavelog[w][1] = __builtin_amdgcn_s_memrealtime();
        g_rtc_wavelog[w][2] = dWaveItems;
        for (int q = 0; q < 5; ++q)
            g_rtc_wavelog[w][3 + q] = dItemEnd[q];
    }
#endif
}

/* rtc_accumulate_samples for a pass: the pixel's sum goes on from the stored accumulator when the pass is not the frame's
 * first (main.c:97-100 after sampleFirst iterations), over the pass's P.spp deferred samples in sample order.  Stays a
 * template, instantiated with true alone: as a plain kernel it would be emitted among the non-template kernels. */
template <bool RESUME>
__global__ __launch_bounds__(256) void rtc_accumulate_samples_resume(RenderParams P)
{
    int items = 0;
    for (int l = 0; l < kGeoLists; ++l)
        items += min(P.geoCount[l * kGeoCountStride], P.geoCap);
    items = min(items, P.sampleCap);
    for (int it = blockIdx.x * 256 + threadIdx.x; it < items; it += gridDim.x * 256) {
        const SampleSlot *slot = P.sampleBuf + (size_t)it * (size_t)P.spp;
        const size_t o = (size_t)P.itemPix[it];
        f2 accxy{0.f, 0.f};
        float accz = 0.f;
        if (RESUME && P.sampleFirst > 0) {
            accxy = f2{P.accum[3 * o], P.accum[3 * o + 1]};
            accz = P.accum[3 * o + 2];
        }
        if (P.maxBounce > 0) {
#pragma unroll 8
            for (int k = 0; k < P.spp; ++k) {
                const SampleSlot v = slot[k];
                accxy = accxy + f2{v.x, v.y};
                accz = accz + v.z;
            }
        }
        P.colors[3 * o] = float_to_u8(accxy.x);
        P.colors[3 * o + 1] = float_to_u8(accxy.y);
        P.colors[3 * o + 2] = float_to_u8(accz);
        P.accum[3 * o] = accxy.x;
        P.accum[3 * o + 1] = accxy.y;
        P.accum[3 * o + 2] = accz;
    }
}
