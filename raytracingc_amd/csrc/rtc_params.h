/* rtc_params.h -- what every render kernel is launched with: RenderParams, the scalar-load accessors for it and for
 * read-only data (KCONST / KLOAD / KARG), and the pixel a lane or wave renders (PixelRay, item records, block order).
 * A section of rtc_render.hip's translation unit: included there once, after the headers above it in that file's
 * list (it uses their names, and rtcdev's through the file's using-directive). */
#pragma once

/* ---- device scene layout: rtc_layout.h; upload: rtc_scene.hip; probes: rtc_probe.hip ---------------------- */
constexpr int kUnroll = 2; /* records per scalar-load batch; arrays are padded to a multiple of 8 */
static_assert(8 % (2 * kUnroll) == 0 || kUnroll == 1, "padding assumes two batches divide 8");

/* ---- the render kernel ---------------------------------------------------------------------------- */
/* one deferred sample: radiance * (1/spp), 12 B (stored and read as 3 dwords) */
struct SampleSlot {
    float x, y, z;
};

struct RenderParams {
    const DevTri *__restrict__ tris;
    const DevMat *__restrict__ mats;
    const DevSphere *__restrict__ spheres;
    const DevPrimF *__restrict__ primF;
    const DevPrimX *__restrict__ primX;
    const DevTri *__restrict__ clTris;         /* cluster order (rtc_build_clusters) */
    const DevCluster *__restrict__ clusters;
    const DevCluster *__restrict__ chunks;
    int chunkCount;
    int clusterCount, clusterCull;
    /* rtc_render_samples_async: the first sample of the pass; > 0: the pixel kernels start from rngState and
     * accum.  (In the 4 bytes of padding the struct had here: no other field moves, so every kernel of the launches without
     * a sample range reads its arguments where it did.)  A pass carries spp = its sample count and invSpp = 1 / the
     * frame's accumulationCount. */
    int sampleFirst;
    const unsigned long long *__restrict__ tileMask; /* null: primary segments test every triangle */
    const unsigned long long *__restrict__ pixMask;  /* per 8x8 tile: pixels with a primary candidate (bit i =
                                                       pixel i, row-major); the others see only the sky */
    const int *__restrict__ order; /* null: identity; else launch slot -> workgroup (heavy first) */
    /* rtc_super_cull's survivors (maskWords u64 per superblock of kSuperBlocks x kSuperBlocks workgroup blocks,
     * superX per row of superblocks); null: rtc_tile_cull tests every triangle at level 1 */
    const unsigned long long *__restrict__ superMask;
    int superX;
    /* rtc_render_chain's work: kGeoLists sub-lists of geometry pixels, one item record (kItemRecDwords dwords, see
     * item_record) each, filled by rtc_tile_cull (tile t appends to sub-list t % kGeoLists, one atomic per tile with
     * geometry, spread over kGeoLists counters in separate cache lines); geoCount[l * 32] = entries of sub-list l,
     * zeroed by the previous split launch's rtc_tile_cull on the same stream, or by rtc_prep_primary */
    int *__restrict__ geoCount;
    int *__restrict__ geoCountNext; /* the next split launch's counters, zeroed by this launch's rtc_tile_cull */
    unsigned *__restrict__ geoList;
    int geoCap; /* entries (records) per sub-list */
    int cullPrio; /* rtc_tile_cull's waves at issue priority 3 (kCullPrioMinPixels) */
    int blocksX; /* 16x16 blocks per row of the launch */
    int wideItems; /* the launch has more than 65,535 columns or launch rows: see item_record */
    /* merged sky pass (rtcplan::Plan::merge; null: none): rtc_tile_cull writes each geometry pixel's item (pixItem[tile * 64
     * + bit]), rtc_render_chain each item's Color bytes (geoColor[item], bytes 0-2), and the sky pass -- after it -- every
     * pixel's Color in whole lines */
    unsigned *__restrict__ pixItem;
    /* rngState (passes only, the RESUME instantiations): one state per pixel at launch row * width + x.  It shares
     * geoColor's place -- a pass never merges its sky pass (rtcplan), and only RESUME kernels, which have no merged path,
     * run in it -- so that the struct keeps its size and layout. */
    union {
        unsigned *__restrict__ geoColor;
        unsigned *__restrict__ rngState;
    };
    /* The draw cache's two pointers for the geometry kernel (the DRAWS instantiations) share the deferred samples' places
     * -- a launch that uses the cache sums in-kernel (sampleCap == 0: no kernel of it reads sampleBuf or itemPix), and the
     * DRAWS kernels have no deferred path -- so that the struct keeps its size and layout, as with rngState.  drawPool: the
     * pool's blocks (float4[64] each); itemDraw: per entry of the launch's lists, 0 or the item's block + 1. */
    union {
        SampleSlot *__restrict__ sampleBuf; /* rtc_render_chain, deferred accumulation: [item][spp] radiance * (1/spp) */
        const float4 *__restrict__ drawPool;
    };
    union {
        int *__restrict__ itemPix;      /* [item] the pixel's offset in the launch's Color rows */
        const unsigned *__restrict__ itemDraw;
    };
    int sampleCap;                  /* items with a slot in sampleBuf; items beyond it accumulate in-kernel */
    int chainPrimF;                 /* rtc_render_chain stages DevPrimF[triPadded] in LDS */
    unsigned char *__restrict__ colors;
    float *__restrict__ accum;
    unsigned long long *__restrict__ segments; /* [0] calculateRayCollision calls, [1] traced, [2] tri tests */
    unsigned long long *__restrict__ segSlots; /* kSegSlots x kSegSlotStride partial counters (flush_counters) */
    int triCount, triPadded, sphereCount, maskWords;
    int width, height, rows, rowStart, rowStride;
    int rowBandShift; /* log2 of the rows per band (rtc.h rowBand): 0 = single rows */
    int spp, maxBounce;
    int hoist;
    float invSpp; /* (float)(1. / accumulationCount), main.c:99 */
    V3 origin, ex, ey, ez;
    float fov;
    EnvParams env;
};

/* Data a kernel only reads (written by earlier kernels of the launch) at a wave-uniform address, read through
 * the constant address space so that the compiler issues scalar loads: they return on lgkmcnt,
 * so waiting for one does not also wait for the wave's earlier sample-slot stores to be acknowledged, as a
 * vector load's vmcnt wait does on gfx9 (loads and stores share vmcnt). */
template <typename T> __device__ __forceinline__ const __attribute__((address_space(4))) T *kconst(const T *p)
{
    return (const __attribute__((address_space(4))) T *)p;
}
/* a record of T (a multiple of 4 bytes) from a wave-uniform address, dword by dword through kconst */
template <typename T> __device__ __forceinline__ T kload(const T *p, int i)
{
    static_assert(sizeof(T) % 4 == 0, "dword records");
    T v;
    const __attribute__((address_space(4))) unsigned *q = kconst((const unsigned *)(p + i));
#pragma unroll
    for (int k = 0; k < (int)(sizeof(T) / 4); ++k)
        ((unsigned *)&v)[k] = q[k];
    return v;
}
#define KCONST(p) kconst(p)
#define KLOAD(p, i) kload(p, i)

/* A RenderParams field of the launch, re-read from the kernarg segment where it is used (KARG; values, and pointers
 * read through KCONST / KLOAD / gload only -- a pointer loaded this way has no known address space, so a plain vector
 * access through it would be a flat one, whose wait covers lgkmcnt too): the kernel's one
 * argument is RenderParams at offset 0 of that segment.  The segment pointer is laundered through an empty asm at every
 * use, so the scalar load is neither hoisted out of the loops nor merged with another use: the field occupies no SGPR
 * between uses.  rtc_render_chain keeps ~60 SGPRs of launch constants (camera, environment, dimensions, pointers)
 * otherwise, and spilled 155 SGPRs to VGPR lanes (v_writelane / v_readlane in its loops).  For fields
 * read once per item, window or escaped bounce: a scalar-cache hit against a register that would have been spilled. */
/* a dword of global memory by a global (not flat) vector load: a flat load's wait would also cover the LDS and scalar
 * loads (lgkmcnt) */
template <typename T> __device__ __forceinline__ unsigned gload(const T *p, size_t i)
{
    static_assert(sizeof(T) == 4, "dwords");
    return ((const __attribute__((address_space(1))) unsigned *)p)[i];
}
/* 16 bytes likewise (global_load_dwordx4) */
__device__ __forceinline__ float4 gload4(const float4 *p, size_t i)
{
    typedef float v4 __attribute__((ext_vector_type(4)));
    const v4 v = ((const __attribute__((address_space(1))) v4 *)p)[i];
    return make_float4(v.x, v.y, v.z, v.w);
}
template <typename T> __device__ __forceinline__ T karg_at(size_t off)
{
    const __attribute__((address_space(4))) char *base =
        (const __attribute__((address_space(4))) char *)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(base));
    static_assert(sizeof(T) % 4 == 0, "dword fields");
    T v;
    const __attribute__((address_space(4))) unsigned *q = (const __attribute__((address_space(4))) unsigned *)(base + off);
#pragma unroll
    for (int k = 0; k < (int)(sizeof(T) / 4); ++k)
        ((unsigned *)&v)[k] = q[k];
    return v;
}
/* Contract: KARG(field) names `P`, which must be the calling kernel's one RenderParams argument -- every
 * kernel that uses KARG, directly or through a helper, is declared `kernel(RenderParams P, ...)` with P first, at
 * kernarg offset 0 (rtc_tile_cull, rtc_render_chain), and a helper that uses it takes `const RenderParams &P`.
 * karg_field refuses any other `P` at compile time. */
template <typename PT, typename T> __device__ __forceinline__ T karg_field(size_t off)
{
    static_assert(std::is_same<typename std::decay<PT>::type, RenderParams>::value,
                  "KARG reads the kernel's RenderParams argument: P must be it");
    return karg_at<T>(off);
}
#define KARG(field) karg_field<decltype(P), decltype(RenderParams::field)>(offsetof(RenderParams, field))

static_assert(offsetof(RenderParams, tileMask) == 80 && offsetof(RenderParams, sampleFirst) == 76 &&
                  offsetof(RenderParams, env) == 344 && sizeof(RenderParams) == 432,
              "RenderParams keeps the layout the kernels of ordinary launches were compiled against");

constexpr int kTileW = 16, kTileH = 16, kBlock = 256;

/* ---- the draw cache ------------------------------------------------------------------------------------
 * Per pixel that has seen geometry, the 64 hit draws D_j = (RandomDiretion from the seed advanced 7 j draws, the roulette
 * value that follows): what rtc_render_chain's first window enters in ChainWaveLds::draw, a function of the seed
 * x + y * width alone.  The argument of the caching tile cull and of the fill kernel behind it (rtc_cull.h).
 * The blocks are APPEND-ONLY: a block is written once, by the fill of the launch whose cull allocated it, before any
 * geometry kernel that can name it starts (the cull operation's completion event is the fill's); later culls and fills
 * never touch an allocated block or a non-zero table entry.  So a geometry kernel may read blocks while a later launch's
 * cull and fill run. */
/* (kDrawEntries and the counter words, DrawCtr: rtc_layout.h, shared with the host code that allocates and reads them) */
struct DrawCache {
    unsigned *__restrict__ table;     /* [tablePixels] by seed: 0 none, k + 1 block k */
    unsigned *__restrict__ ctr;       /* DrawCtr */
    unsigned *__restrict__ blockSeed; /* [capacity] block k's seed (the fill's input) */
    float4 *__restrict__ pool;        /* [capacity][kDrawEntries] */
    unsigned *__restrict__ itemDraw;  /* the launch slot's: per entry of the lists, 0 or block + 1 */
    unsigned capacity, tablePixels;
    int parity;
};


/* The pixel a lane renders and its primary ray (rowThread, main.c:88-94).  A 256-thread workgroup covers
 * 16x16 pixels of the launch's rows; wave w of it the 8x8 tile (w & 1, w >> 1). */
struct PixelRay {
    int x, r, y;
    bool valid;
    V3 dir;
};

/* (primary_dir and launch_row_y: rtc_layout.h, shared with the primary filter's probe) */
__device__ __forceinline__ PixelRay pixel_ray(const RenderParams &P, int bx, int by)
{
    PixelRay px;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    px.x = bx * kTileW + (wave & 1) * 8 + (lane & 7);
    px.r = by * kTileH + (wave >> 1) * 8 + (lane >> 3);
    px.valid = px.x < P.width && px.r < P.rows;
    px.y = launch_row_y(P, px.r);
    px.dir = primary_dir(P, px.x, px.y);
    return px;
}

/* A geometry pixel's item record, rtc_tile_cull -> rtc_render_chain (private to the two: the list has no other reader).
 * Dword 0: x | launch row << 16; a launch with more than 65,535 columns or launch rows (P.wideItems) keeps tile * 64 + bit
 * there instead, which the chain kernel decodes by a divide.  Dwords 1-3: the bits of the pixel's primary direction
 * (main.c:88-94, formed once per pixel as in the reference), which the cull's lane holds already: the chain kernel's
 * wave does not rebuild it for 64 lanes from the camera. */
__device__ __forceinline__ uint4 item_record(const RenderParams &P, const PixelRay &px, int tile, int bit)
{
    const unsigned d0 = P.wideItems ? (unsigned)(tile * 64 + bit) : (unsigned)px.x | (unsigned)px.r << 16;
    return uint4{d0, __float_as_uint(px.dir.x), __float_as_uint(px.dir.y), __float_as_uint(px.dir.z)};
}

/* This wave's 8x8 tile in the launch (made provably wave-uniform, so tile data is scalar-loaded). */
__device__ __forceinline__ int wave_tile(int bx, int by)
{
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    return (by * 2 + (wave >> 1)) * (gridDim.x * 2) + bx * 2 + (wave & 1);
}

/* The workgroup this launch slot renders.  Workgroups are dispatched in launch-slot order; with P.order
 * (rtc_order_blocks) the ones whose pixels see geometry -- the long-running ones -- go first, so the many
 * short sky-only workgroups fill in behind them instead of leaving them as a tail. */
__device__ __forceinline__ void block_xy(const RenderParams &P, int &bx, int &by)
{
    if (P.order) {
        const int id = P.order[blockIdx.y * gridDim.x + blockIdx.x];
        bx = id % (int)gridDim.x;
        by = id / (int)gridDim.x;
    } else {
        bx = blockIdx.x;
        by = blockIdx.y;
    }
}
