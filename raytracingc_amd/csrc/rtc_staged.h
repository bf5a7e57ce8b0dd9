/* rtc_staged.h -- the host path of the entries that take HOST arrays (rtc_trace_rays, rtc_trace_paths, rtc_occluded,
 * rtc_ray_order, rtc_scene_update, rtc_scene_regroup): staged through device buffers around the asynchronous entry, stated
 * once (C++ only). */
#pragma once
#include <hip/hip_runtime.h>

#include "rtc_layout.h"
#include "rtc_internal.h"
#include "rtc_hip_util.h"

/* One buffer of a host entry: `bytes` of device memory when wanted (else the query gets a null pointer), filled from `in`
 * first (null: left as allocated) and copied to `out` afterwards (null: an input) */
struct Staged {
    const void *in;
    void *out;
    size_t bytes;
    bool want;
};

/* A host entry (a non-null scene, nothing refused): staged through device buffers on the null stream.  `call` gets the
 * device pointers in the items' order (null for an item not wanted) and issues the asynchronous entry. */
template <int N, class Call>
static int staged_query(const char *who, const RtcDeviceScene *s, const Staged (&items)[N], Call call)
{
    int devices = 0;
    if (const int rc = rtc_device_count(&devices)) /* (RTC_ENODEV before the handle is read) */
        return rc;
    RtcDeviceGuard guard(s->device);
    if (!guard.ok())
        return rtc_fail(RTC_ENODEV, "%s: cannot select the scene's device %d", who, s->device);
    void *dev[N] = {};
    hipError_t e = hipSuccess;
    for (int k = 0; k < N; ++k) {
        if (e == hipSuccess && items[k].want)
            e = hipMalloc(&dev[k], items[k].bytes);
        if (e == hipSuccess && items[k].want && items[k].in)
            e = hipMemcpy(dev[k], items[k].in, items[k].bytes, hipMemcpyHostToDevice);
    }
    /* a host caller names no stream: every launch enqueued so far, on whichever stream, ends before the query */
    if (e == hipSuccess)
        e = hipDeviceSynchronize();
    int rc = e == hipSuccess ? call(dev) : rtc_fail(-(int)e, "%s: staging failed: %s", who, hipGetErrorString(e));
    if (rc == 0 && (e = hipStreamSynchronize(nullptr)) != hipSuccess)
        rc = rtc_fail(-(int)e, "%s: %s", who, hipGetErrorString(e));
    for (int k = 0; k < N; ++k)
        if (rc == 0 && dev[k] && items[k].out &&
            (e = hipMemcpy(items[k].out, dev[k], items[k].bytes, hipMemcpyDeviceToHost)) != hipSuccess)
            rc = rtc_fail(-(int)e, "%s: %s", who, hipGetErrorString(e));
    for (void *p : dev)
        if (p)
            (void)hipFree(p);
    return rc;
}
