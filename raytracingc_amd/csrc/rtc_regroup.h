/* rtc_regroup.h -- the cluster membership as a sequence of levels, stated once for the host and the device.
 *
 * split_clusters (rtc_scene.hip) is a recursion: a segment [lo, hi) of more than kRegroupLeaf positions takes the axis of
 * its centroids' longest extent, is stable-sorted by the centroid along it, and splits at lo + (leaves + 1) / 2 * 8 with
 * leaves = (hi - lo + 7) / 8.  The split points depend on the triangle count alone, so the recursion's d-th generation of
 * calls is a fixed set of disjoint segments -- a level -- and a level needs, per segment, one axis and one stable sort.
 * A stable sort by a strict weak order has one result: the element at position p of the segment goes to
 *     lo + #{q in [lo, hi) : key_q < key_p} + #{q in [lo, p) : key_q == key_p},
 * q over the segment's positions before the sort (regroup_rank).  The keys hold no NaN (regroup_key), so `<` on doubles is
 * a strict weak order and `==` is its equivalence, +0 and -0 together; the count needs no sort primitive, no atomics and
 * is the same whatever the order of evaluation.  split_clusters takes its centroid, extent, axis, key and split point from
 * these functions; rtc_regroup_membership_host runs the levels in plain C++ and the regroup kernels on the device
 * (rtc_scene.hip).
 * Pure functions of their arguments; no HIP needed to compile them. */
#pragma once

#if defined(__HIPCC__)
#define RTC_REGROUP_HD __host__ __device__ inline
#else
#define RTC_REGROUP_HD inline
#endif
#define RTC_REGROUP_HDC RTC_REGROUP_HD constexpr

/* rtc_scene_regroup_max_tris: the rank count is quadratic, so the regroup is offered only up to the largest power of two
 * at which it was measured faster than the upload it replaces (DESIGN §3.16 has the times at every size tried).  At this
 * value the measured regroup was still the faster one; it is also the most the level kernel's grid can address (one
 * grid row per segment of a level, kRegroupMaxPaths of them at most). */
constexpr int kRegroupMaxTris = 524288;
constexpr int kRegroupMaxPaths = 65535; /* gridDim.y */
constexpr int kRegroupLeaf = 8; /* kClusterSize: a segment of at most this many positions is left as it is */

/* split_clusters' centroid along one axis from the PACKED f32 values a, ab = b - a, ac = c - a (pack_scene, rtc_refit):
 * double arithmetic, IEEE divide, no contraction */
RTC_REGROUP_HD double regroup_centroid(float a, float ab, float ac)
{
    return (double)a + ((double)ab + (double)ac) / 3.0;
}

/* The extent of a segment's centroids along one axis: split_clusters' mn = 1e300, mx = -1e300, a NaN skipped with c == c,
 * std::min / std::max with the accumulator first.  The order of the reduction does not matter: `take` keeps the
 * accumulator unless the candidate is strictly smaller (larger), so any order -- and any tree of `merge`s of partial
 * extents -- ends at the least (greatest) value offered, 1e300 (-1e300) included, which is unique up to the sign of a
 * zero; and regroup_axis sees the bounds only through mx - mn compared with `>`, where x - (+0) and x - (-0) are the same
 * number for x != 0 and zeros of either sign compare equal. */
struct RegroupExtent {
    double mn, mx;
};
RTC_REGROUP_HD RegroupExtent regroup_extent_init()
{
    return RegroupExtent{1e300, -1e300};
}
RTC_REGROUP_HD void regroup_extent_take(RegroupExtent &e, double c)
{
    if (c == c) {
        e.mn = c < e.mn ? c : e.mn; /* std::min(mn, c) */
        e.mx = e.mx < c ? c : e.mx; /* std::max(mx, c) */
    }
}
RTC_REGROUP_HD void regroup_extent_merge(RegroupExtent &e, const RegroupExtent &o)
{
    e.mn = o.mn < e.mn ? o.mn : e.mn;
    e.mx = e.mx < o.mx ? o.mx : e.mx;
}
/* split_clusters' axis: 0 unless a later axis is strictly longer (an extent of NaN, inf - inf, never wins and never loses) */
RTC_REGROUP_HD int regroup_axis(const RegroupExtent e[3])
{
    int axis = 0;
    for (int a = 1; a < 3; ++a)
        if (e[a].mx - e[a].mn > e[axis].mx - e[axis].mn)
            axis = a;
    return axis;
}

/* the sort key of a centroid: NaN sorts as 1e300 */
RTC_REGROUP_HD double regroup_key(double c)
{
    return c == c ? c : 1e300;
}

/* one element's contribution to the rank of the element (key kp, position p): q's key kq */
RTC_REGROUP_HD int regroup_rank(double kq, int q, double kp, int p)
{
    return (kq < kp ? 1 : 0) + (kq == kp && q < p ? 1 : 0);
}

/* split_clusters' split point of [lo, hi), hi - lo > kRegroupLeaf */
RTC_REGROUP_HDC int regroup_mid(int lo, int hi)
{
    const int leaves = (hi - lo + kRegroupLeaf - 1) / kRegroupLeaf;
    return lo + (leaves + 1) / 2 * kRegroupLeaf;
}

/* levels of n positions: the depth of the recursion's deepest sorting call (0: nothing is sorted).  The left half is never
 * the smaller one, so the leftmost path is the deepest. */
RTC_REGROUP_HDC int regroup_levels(int n)
{
    int levels = 0;
    for (int hi = n; hi > kRegroupLeaf; hi = regroup_mid(0, hi))
        ++levels;
    return levels;
}
static_assert(regroup_levels(8) == 0 && regroup_levels(9) == 1 && regroup_levels(24) == 2 && regroup_levels(3868) == 9,
              "ceil(log2(ceil(n / 8))) levels");
static_assert(regroup_levels(kRegroupMaxTris) >= 1 && 1 << (regroup_levels(kRegroupMaxTris) - 1) <= kRegroupMaxPaths,
              "the deepest level's segments are one grid row each");

/* The segment of level `level` reached from [0, n) by the turns `path` (bit level - 1 first: 0 left, 1 right), as the
 * recursion reaches it.  False when the path ends in a leaf before that level, or when the segment is a leaf itself:
 * nothing is sorted there. */
RTC_REGROUP_HD bool regroup_segment_of_path(int n, int level, unsigned path, int &lo, int &hi)
{
    lo = 0, hi = n;
    for (int d = level - 1; d >= 0; --d) {
        if (hi - lo <= kRegroupLeaf)
            return false;
        const int mid = regroup_mid(lo, hi);
        if (path >> d & 1u)
            lo = mid;
        else
            hi = mid;
    }
    return hi - lo > kRegroupLeaf;
}

/* The same segment found from a position in it: the segment of `level` that holds position p (0 <= p < n).  False as
 * above; then [lo, hi) is the leaf that holds p. */
RTC_REGROUP_HD bool regroup_segment_of_position(int n, int level, int p, int &lo, int &hi)
{
    lo = 0, hi = n;
    for (int d = 0; d < level; ++d) {
        if (hi - lo <= kRegroupLeaf)
            return false;
        const int mid = regroup_mid(lo, hi);
        if (p >= mid)
            lo = mid;
        else
            hi = mid;
    }
    return hi - lo > kRegroupLeaf;
}

/* the largest segment of a level: the leftmost one */
RTC_REGROUP_HD int regroup_level_width(int n, int level)
{
    int hi = n;
    for (int d = 0; d < level && hi > kRegroupLeaf; ++d)
        hi = regroup_mid(0, hi);
    return hi;
}
