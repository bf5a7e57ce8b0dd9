/* rtc_pass_util.h -- what the device passes outside the launch planner share (rtc_ray_order.hip, rtc_select.hip,
 * rtc_denoise.hip): the workgroup scan, the per-pixel sample scale and the refusal of a scratch pointer. */
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/rtc.h"
#include "rtc_internal.h"

/* The workgroup's exclusive prefix of one value per thread, and the workgroup's sum in `total`, for a workgroup of WAVES
 * waves; waveSum: WAVES LDS words.  Two barriers; every thread of the workgroup calls it. */
template <int WAVES>
__device__ inline unsigned rtc_block_scan(unsigned v, unsigned *waveSum, int lane, int wave, unsigned &total)
{
    unsigned incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned u = __shfl_up(incl, o);
        if (lane >= o)
            incl += u;
    }
    if (lane == 63)
        waveSum[wave] = incl;
    __syncthreads();
    unsigned pre = 0, sum = 0;
#pragma unroll
    for (int u = 0; u < WAVES; ++u) {
        const unsigned w = waveSum[u];
        pre += u < wave ? w : 0u;
        sum += w;
    }
    __syncthreads();
    total = sum;
    return pre + incl - v;
}

/* What a pixel's sum of s samples of a frame of fspp is multiplied with: this one statement is the resolve's and the
 * denoise's, compiled for the host and for the device (the correctly rounded f32 division on both sides). */
__host__ __device__ inline float rtc_sample_scale(float fspp, int s)
{
    return s > 0 ? fspp / (float)s : 0.f;
}

/* A device entry's scratch pointer: null, then alignment; the size follows in the entry, in its own quantities. */
inline int rtc_refuse_scratch(const char *who, const void *dScratch)
{
    if (!dScratch)
        return rtc_fail(RTC_EINVAL, "%s: null scratch", who);
    if (((size_t)dScratch & 15) != 0)
        return rtc_fail(RTC_EINVAL, "%s: the scratch must be 16-byte aligned", who);
    return 0;
}
