// Host program around gym_miniworld_amd/csrc/mwb_seg_groups.h for tests/test_seg_groups_host.py.
//   seg_groups_host            random and directed groups: every bound of the float32 box lies outside or on the float64 bound of
//                              every member segment, and the group test passes wherever a member's own bounding-box test does;
//                              prints "checked <groups> <points>" and exits 0, or says what failed and exits 1
//   seg_groups_host box N v..  the box of the N segments given as 4 N float64 values (hex floats welcome), four %a values
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "mwb_seg_groups.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() {   // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}
static double uniform() { return (double)(next_u64() >> 11) / 9007199254740992.0; }

// a finite coordinate: most of them the size of a world's, some huge, tiny, denormal, zero of either sign, float32-exact
static double coord() {
    const unsigned k = (unsigned)(next_u64() % 16);
    const double sign = (next_u64() & 1) ? -1.0 : 1.0;
    if (k < 9) return (uniform() - 0.3) * 80.0;
    if (k == 9) return sign * std::ldexp(uniform() + 0.5, (int)(next_u64() % 250) - 125);     // any float32 exponent
    if (k == 10) return sign * std::ldexp(uniform() + 0.5, -127 - (int)(next_u64() % 30));    // float32 denormal range and below
    if (k == 11) return sign * std::ldexp(uniform() + 0.5, -1040 - (int)(next_u64() % 30));   // float64 denormals
    if (k == 12) return sign * 0.0;
    if (k == 13) return (double)(float)((uniform() - 0.5) * 100.0);                            // exact in float32
    if (k == 14) return sign * std::ldexp(uniform() + 0.5, 128 + (int)(next_u64() % 800));    // finite, beyond float32
    return sign * 1e30;
}

static int failures = 0;
static void fail(const char *what, const double *s, int n, const MwbSegBox &b) {
    if (failures++ < 10) {
        std::printf("FAIL %s: n=%d box %a %a %a %a\n", what, n, b.min_x, b.min_z, b.max_x, b.max_z);
        for (int i = 0; i < n; i++) std::printf("  seg %d: %a %a %a %a\n", i, s[i * 4], s[i * 4 + 1], s[i * 4 + 2], s[i * 4 + 3]);
    }
}

// every bound outside or on every member's float64 bound; tight: one float32 step inwards is inside some member
static void check_box(const double *s, int n) {
    const MwbSegBox b = mwb_seg_group_box(s, n);
    double mnx = INFINITY, mnz = INFINITY, mxx = -INFINITY, mxz = -INFINITY;
    for (int i = 0; i < n; i++) {
        const double x0 = std::fmin(s[i * 4], s[i * 4 + 2]), x1 = std::fmax(s[i * 4], s[i * 4 + 2]);
        const double z0 = std::fmin(s[i * 4 + 1], s[i * 4 + 3]), z1 = std::fmax(s[i * 4 + 1], s[i * 4 + 3]);
        if (!((double)b.min_x <= x0 && (double)b.max_x >= x1 && (double)b.min_z <= z0 && (double)b.max_z >= z1)) fail("bound inside a member", s, n, b);
        mnx = std::fmin(mnx, x0); mxx = std::fmax(mxx, x1); mnz = std::fmin(mnz, z0); mxz = std::fmax(mxz, z1);
    }
    // no looser than one float32 step (where the bound is finite: a coordinate beyond float32 rounds out to infinity)
    if (std::isfinite(b.min_x) && !((double)std::nextafterf(b.min_x, INFINITY) > mnx)) fail("min_x loose", s, n, b);
    if (std::isfinite(b.min_z) && !((double)std::nextafterf(b.min_z, INFINITY) > mnz)) fail("min_z loose", s, n, b);
    if (std::isfinite(b.max_x) && !((double)std::nextafterf(b.max_x, -INFINITY) < mxx)) fail("max_x loose", s, n, b);
    if (std::isfinite(b.max_z) && !((double)std::nextafterf(b.max_z, -INFINITY) < mxz)) fail("max_z loose", s, n, b);
}

// step_kernel's per-segment reject, as written there
static bool seg_nearby(const double *q, double px, double pz, double guard) {
    return px >= std::fmin(q[0], q[2]) - guard && px <= std::fmax(q[0], q[2]) + guard &&
           pz >= std::fmin(q[1], q[3]) - guard && pz <= std::fmax(q[1], q[3]) + guard;
}

static long long points = 0;
static void check_points(const double *s, int n) {
    const MwbSegBox b = mwb_seg_group_box(s, n);
    const double guards[3] = {0.4 + 1e-9, 0.11 + 1e-9, 0.48 + 1e-9};
    for (int t = 0; t < 6; t++) {
        const double guard = guards[t % 3];
        const double *q = s + (next_u64() % (unsigned)n) * 4;
        // a point on the edge of a member's grown box, and a few ulps either side of it
        double px = (next_u64() & 1) ? std::fmin(q[0], q[2]) - guard : std::fmax(q[0], q[2]) + guard;
        double pz = (next_u64() & 1) ? std::fmin(q[1], q[3]) - guard : std::fmax(q[1], q[3]) + guard;
        for (int k = (int)(next_u64() % 4); k > 0; k--) px = std::nextafter(px, (next_u64() & 1) ? INFINITY : -INFINITY);
        for (int k = (int)(next_u64() % 4); k > 0; k--) pz = std::nextafter(pz, (next_u64() & 1) ? INFINITY : -INFINITY);
        if (t >= 4) { px = coord(); pz = coord(); }
        bool any = false;
        for (int i = 0; i < n; i++) any = any || seg_nearby(s + i * 4, px, pz, guard);
        points++;
        if (any && !mwb_seg_box_near(b.min_x, b.min_z, b.max_x, b.max_z, px, pz, guard)) fail("group test turns down a point a member accepts", s, n, b);
    }
}

static bool all_pass(const MwbSegBox &b) { return b.min_x == -INFINITY && b.min_z == -INFINITY && b.max_x == INFINITY && b.max_z == INFINITY; }

static void directed() {
    const double inf = INFINITY, nan = std::numeric_limits<double>::quiet_NaN();
    {   // not representable in float32: the box must open by one float32 step, not round to nearest
        const double s[4] = {0.1, -0.1, 16777217.0, 1.0 / 3.0};
        const MwbSegBox b = mwb_seg_group_box(s, 1);
        check_box(s, 1);
        if (!(b.min_x == std::nextafterf(0.1f, -INFINITY) && (double)b.min_x < 0.1 && b.max_x == 16777218.0f)) fail("0.1 / 2^24 + 1", s, 1, b);
        if (!((double)b.min_z < -0.1 && (double)b.max_z > 1.0 / 3.0)) fail("-0.1 / 1/3", s, 1, b);
    }
    {   // float32-exact values stay as they are
        const double s[4] = {1.5, -2.25, 1.5, 1024.0};
        const MwbSegBox b = mwb_seg_group_box(s, 1);
        if (!(b.min_x == 1.5f && b.max_x == 1.5f && b.min_z == -2.25f && b.max_z == 1024.0f)) fail("exact values moved", s, 1, b);
    }
    {   // zeros of either sign: a bound that compares equal to zero
        const double s[8] = {-0.0, 0.0, 0.0, -0.0, 0.0, -0.0, -0.0, 0.0};
        const MwbSegBox b = mwb_seg_group_box(s, 2);
        check_box(s, 2);
        if (!(b.min_x == 0.0f && b.max_x == 0.0f && b.min_z == 0.0f && b.max_z == 0.0f)) fail("negative zero", s, 2, b);
    }
    {   // float64 and float32 denormals
        const double s[8] = {4.9e-324, -4.9e-324, 1e-310, -1e-310, 1e-40, -1e-40, 1.4e-45, -3e-45};
        const MwbSegBox b = mwb_seg_group_box(s, 2);
        check_box(s, 2);
        if (!(b.min_x == 0.0f && (double)b.max_x >= 1e-40 && (double)b.max_x < 1.1e-40 && (double)b.min_z <= -1e-40)) fail("denormals", s, 2, b);
    }
    {   // 1e30 (a float32 value's neighbour) and a finite value beyond float32
        const double s[8] = {1e30, -1e30, -1e30, 1e30, 1e300, -1e300, 0.0, 0.0};
        const MwbSegBox b1 = mwb_seg_group_box(s, 1), b2 = mwb_seg_group_box(s, 2);
        check_box(s, 1); check_box(s, 2);
        if (!std::isfinite(b1.min_x) || !std::isfinite(b1.max_z)) fail("1e30 left float32", s, 1, b1);
        if (!(b2.max_x == INFINITY && b2.min_z == -INFINITY)) fail("1e300 must round out to infinity", s, 2, b2);
    }
    for (int n = 1; n <= 8; n++) {   // a partial group covers the segments that exist, and none behind them
        double s[32];
        for (int i = 0; i < 8; i++) { s[i * 4] = i; s[i * 4 + 1] = -i; s[i * 4 + 2] = i + 0.5; s[i * 4 + 3] = -i - 0.5; }
        const MwbSegBox b = mwb_seg_group_box(s, n);
        check_box(s, n);
        if (!(b.min_x == 0.0f && b.max_x == (float)(n - 1 + 0.5) && b.max_z == 0.0f && b.min_z == (float)(-(n - 1) - 0.5))) fail("partial group", s, n, b);
    }
    for (int n = 1; n <= 8; n++)   // NaN or inf in any coordinate of any member: every point passes
        for (int at = 0; at < n * 4; at++)
            for (int k = 0; k < 3; k++) {
                double s[32];
                for (int i = 0; i < 32; i++) s[i] = i * 0.25;
                s[at] = k == 0 ? nan : (k == 1 ? inf : -inf);
                const MwbSegBox b = mwb_seg_group_box(s, n);
                if (!all_pass(b)) fail("NaN / inf must give the all-pass box", s, n, b);
                if (!mwb_seg_box_near(b.min_x, b.min_z, b.max_x, b.max_z, 1e300, -1e300, 0.4)) fail("all-pass box turns a point down", s, n, b);
            }
    {   // ... but not behind the group's end
        double s[32];
        for (int i = 0; i < 32; i++) s[i] = i;
        s[12] = nan;
        if (all_pass(mwb_seg_group_box(s, 3))) fail("a segment behind the end was read", s, 3, mwb_seg_group_box(s, 3));
    }
    if (mwb_seg_groups(0) != 0 || mwb_seg_groups(1) != 1 || mwb_seg_groups(8) != 1 || mwb_seg_groups(9) != 2 || mwb_seg_groups(256) != 32) { std::printf("FAIL mwb_seg_groups\n"); failures++; }
}

int main(int argc, char **argv) {
    if (argc >= 3 && !std::strcmp(argv[1], "box")) {
        const int n = std::atoi(argv[2]);
        if (n < 1 || n > MWB_SEG_GROUP || argc != 3 + 4 * n) return 2;
        double s[MWB_SEG_GROUP * 4];
        for (int i = 0; i < 4 * n; i++) s[i] = std::strtod(argv[3 + i], nullptr);
        const MwbSegBox b = mwb_seg_group_box(s, n);
        std::printf("%a %a %a %a\n", b.min_x, b.min_z, b.max_x, b.max_z);
        return 0;
    }
    directed();
    const long long groups = argc >= 2 ? std::atoll(argv[1]) : 1200000;
    for (long long g = 0; g < groups; g++) {
        double s[MWB_SEG_GROUP * 4];
        const int n = 1 + (int)(next_u64() % MWB_SEG_GROUP);
        for (int i = 0; i < n * 4; i++) s[i] = coord();
        if (next_u64() % 4 == 0)   // axis-aligned walls, as the worlds have them
            for (int i = 0; i < n; i++) { const int a = (int)(next_u64() & 1); s[i * 4 + 2 + a] = s[i * 4 + a]; }
        check_box(s, n);
        check_points(s, n);
    }
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("checked %lld %lld\n", groups, points);
    return 0;
}
