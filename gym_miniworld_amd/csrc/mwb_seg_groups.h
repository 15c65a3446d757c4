// mwb_seg_groups.h - bounding boxes of an env's collision segments, taken eight at a time.
//
// Plain C++ without any HIP type, so that the same function runs in reset_kernel (the one writer of d.segs) and in a host
// program (tests/test_seg_groups_host.py builds one around this header).
//
// The circle-vs-segment tests of a step read an env's segments in groups of MWB_SEG_GROUP - the unit step_kernel's loop loads.
// d.seg_box holds one float32 box {min_x, min_z, max_x, max_z} per group, [ceil(S_max / 8)][4][N], transposed like d.segs.  A
// reader skips a group when the point lies outside the box grown by radius + 1e-9, computed in float64 from the float32 bounds
// (mwb_seg_box_near).  Every bound is rounded OUTWARDS, so the grown box contains the grown float64 box of every member
// segment: the group test can only skip what step_kernel's per-segment reject skips, and that reject is exact (a segment whose
// grown bounding box excludes the point is farther away than the radius).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MWB_SEG_HD __host__ __device__
#define MWB_SEG_UNROLL _Pragma("unroll")
#else
#define MWB_SEG_HD
#define MWB_SEG_UNROLL
#endif

#define MWB_SEG_GROUP 8

struct MwbSegBox { float min_x, min_z, max_x, max_z; };

MWB_SEG_HD static inline int mwb_seg_groups(int n_segs) { return (n_segs + MWB_SEG_GROUP - 1) / MWB_SEG_GROUP; }

// the largest float32 <= v / the smallest float32 >= v (v finite); -inf / +inf should a conversion ever fail to give one
MWB_SEG_HD static inline float mwb_f32_below(double v) {
    float f = (float)v;
    if ((double)f > v) f = nextafterf(f, -INFINITY);
    return (double)f <= v ? f : -INFINITY;
}
MWB_SEG_HD static inline float mwb_f32_above(double v) {
    float f = (float)v;
    if ((double)f < v) f = nextafterf(f, INFINITY);
    return (double)f >= v ? f : INFINITY;
}

// segs: n (1 .. MWB_SEG_GROUP) segments of 4 float64 each (a.x a.z b.x b.z), the segments of the group that exist.  A NaN or
// infinite coordinate anywhere gives the box every point passes; so does n < 1.
MWB_SEG_HD static inline MwbSegBox mwb_seg_group_box(const double *segs, int n) {
    const MwbSegBox all = {-INFINITY, -INFINITY, INFINITY, INFINITY};
    if (n < 1) return all;
    if (n > MWB_SEG_GROUP) n = MWB_SEG_GROUP;
    double mnx = INFINITY, mnz = INFINITY, mxx = -INFINITY, mxz = -INFINITY;
    MWB_SEG_UNROLL
    for (int i = 0; i < MWB_SEG_GROUP; i++) {   // (constant trip count: a caller's register array stays in registers)
        if (i >= n) break;
        const double ax = segs[i * 4 + 0], az = segs[i * 4 + 1], bx = segs[i * 4 + 2], bz = segs[i * 4 + 3];
        if (!(fabs(ax) <= 1.7976931348623157e308 && fabs(az) <= 1.7976931348623157e308 &&
              fabs(bx) <= 1.7976931348623157e308 && fabs(bz) <= 1.7976931348623157e308)) return all;   // NaN fails every comparison
        mnx = ax < mnx ? ax : mnx; mnx = bx < mnx ? bx : mnx; mxx = ax > mxx ? ax : mxx; mxx = bx > mxx ? bx : mxx;
        mnz = az < mnz ? az : mnz; mnz = bz < mnz ? bz : mnz; mxz = az > mxz ? az : mxz; mxz = bz > mxz ? bz : mxz;
    }
    const MwbSegBox b = {mwb_f32_below(mnx), mwb_f32_below(mnz), mwb_f32_above(mxx), mwb_f32_above(mxz)};
    return b;
}

// may a circle of `guard` (radius + 1e-9) around (px, pz) touch a segment of the group?  false only where the per-segment
// bounding-box reject would turn every member down
MWB_SEG_HD static inline bool mwb_seg_box_near(float min_x, float min_z, float max_x, float max_z, double px, double pz, double guard) {
    return px >= (double)min_x - guard && px <= (double)max_x + guard && pz >= (double)min_z - guard && pz <= (double)max_z + guard;
}
