// mwb_rollout_window_map.h - the windowed gather: which pixel of a stored frame an output pixel of mwb_rollout_gather_window
// shows, and which offset pair a row draws (mwb_rollout_window_offsets).
//
// Plain C++ without any HIP type, so that the same functions run in the kernels (mwb_rollout_window.hip), in the host API and in
// a host program (tests/test_rollout_window_host.py builds one around this header).
//
// The reference is the trainer's image augmentation of a minibatch (RAD / DrQ "random shift", random crop, random translate): one
// draw per stacked observation, shared by all of its frames.  A window is (out_w, out_h, border, dx_lo, dx_hi, dy_lo, dy_hi); a
// row has one offset pair (dx, dy), clamped to [dx_lo, dx_hi] x [dy_lo, dy_hi] before anything else is computed from it.  With F
// the plain stacked observation [nstack * C][W][H] of the row, the windowed row is [nstack * C][out_w][out_h]:
//
//   out[p][x][y] = F[p][sx][sy]                                with sx = x + dx, sy = y + dy, if 0 <= sx < W and 0 <= sy < H
//                = F[p][clamp(sx, 0, W-1)][clamp(sy, 0, H-1)]  otherwise, border 0 (edge replication)
//                = 0                                           otherwise, border 1 (zeros)
//
//   shift(pad)          out W x H, border 0, dx, dy in -pad .. pad           (replicate-pad by pad, crop back)
//   crop(w, h)          out w x h, border 0 (never used), dx in 0 .. W - w, dy in 0 .. H - h
//   center_crop(w, h)   the same with dx = (W - w) / 2, dy = (H - h) / 2 only
//   translate(w, h)     out w x h >= W x H, border 1, dx in -(w - W) .. 0, dy in -(h - H) .. 0   (the frame on a black canvas)
//
// The draw follows the level sampler's recipe (mwb_levels_map.h), keyed by the row's gather index t * N + e, not by its place in
// the minibatch: a transition gets the same draw wherever a permutation puts it, and a new one when `call` changes.
#pragma once
#include <stdint.h>
#include "mwb_levels_map.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MWB_WINDOW_HD __host__ __device__
#else
#define MWB_WINDOW_HD
#endif

#define MWB_WINDOW_MAX_OUT 1024        // out_w, out_h
#define MWB_WINDOW_MAX_OFFSET 32767    // |every bound of the two ranges|
#define MWB_WINDOW_BORDER_EDGE 0
#define MWB_WINDOW_BORDER_ZERO 1

// what is wrong with a window: 0 = nothing, otherwise the number of the limit it breaks (mwb_window_limit_text names it)
MWB_WINDOW_HD static inline int mwb_window_check(int out_w, int out_h, int border, int dx_lo, int dx_hi, int dy_lo, int dy_hi) {
    if (out_w < 1 || out_w > MWB_WINDOW_MAX_OUT || out_h < 1 || out_h > MWB_WINDOW_MAX_OUT) return 1;
    if ((out_w * out_h) % 4) return 2;
    if (dx_lo > dx_hi || dy_lo > dy_hi) return 3;
    if (dx_lo < -MWB_WINDOW_MAX_OFFSET || dx_hi > MWB_WINDOW_MAX_OFFSET || dy_lo < -MWB_WINDOW_MAX_OFFSET || dy_hi > MWB_WINDOW_MAX_OFFSET) return 4;
    if (border != MWB_WINDOW_BORDER_EDGE && border != MWB_WINDOW_BORDER_ZERO) return 5;
    return 0;
}

static inline const char *mwb_window_limit_text(int limit) {
    switch (limit) {
    case 1: return "out_w and out_h must lie in 1 .. 1024";
    case 2: return "out_w * out_h must be a multiple of 4";
    case 3: return "an offset range has lo > hi";
    case 4: return "the offset bounds must lie in -32767 .. 32767";
    case 5: return "border must be 0 (edge replication) or 1 (zeros)";
    default: return "";
    }
}

// ------------------------------------------------------------------------------------------------ the window rule
MWB_WINDOW_HD static inline int mwb_window_clamp(int v, int lo, int hi) {   // lo <= hi; a maximum, then a minimum
    const int a = v > lo ? v : lo;
    return a < hi ? a : hi;
}

// The rule is separable.  One axis of it: output coordinate v (an x or a y) of a row whose CLAMPED offset on that axis is d, over
// n source pixels -> the source coordinate, always inside 0 .. n - 1 (the only coordinates an address is formed from);
// *inside = v + d lay inside already.  v < 1024 and |d| <= 32767: the sum fits an int
MWB_WINDOW_HD static inline int mwb_window_axis(int v, int d, int n, int *inside) {
    const int u = v + d, s = mwb_window_clamp(u, 0, n - 1);
    *inside = u == s;
    return s;
}

// output pixel (x, y) of a row whose CLAMPED offsets are (dx, dy), over a W x H frame: 1 = it shows F[*sx][*sy], 0 = it is zero
MWB_WINDOW_HD static inline int mwb_window_source(int x, int y, int dx, int dy, int W, int H, int border, int *sx, int *sy) {
    int in_x, in_y;
    *sx = mwb_window_axis(x, dx, W, &in_x);
    *sy = mwb_window_axis(y, dy, H, &in_y);
    return border == MWB_WINDOW_BORDER_EDGE || (in_x && in_y);
}

// n / d for n < 2^20, 1 <= d <= 1024 as one multiplication: magic = 2^32 / d + 1, so magic * d = 2^32 + e with 0 < e <= d and
// n * e < 2^30: the quotient is exact.  (The kernel splits a pixel number into column and place in the column with it.)
MWB_WINDOW_HD static inline uint64_t mwb_window_div_magic(uint32_t d) { return (1ULL << 32) / d + 1; }
MWB_WINDOW_HD static inline uint32_t mwb_window_div(uint32_t n, uint64_t magic) { return (uint32_t)(((uint64_t)n * magic) >> 32); }

// ------------------------------------------------------------------------------------------------ the draw
MWB_WINDOW_HD static inline uint64_t mwb_window_key(uint64_t seed, uint64_t call) { return mwb_levels_mix(seed + MWB_LEVELS_GOLD * (call + 1)); }

// the offsets of gather index `index` under `key`: uniform over [dx_lo, dx_hi] x [dy_lo, dy_hi] (ranges of at most 65535 values)
MWB_WINDOW_HD static inline void mwb_window_draw(uint64_t key, int64_t index, int dx_lo, int dx_hi, int dy_lo, int dy_hi, int *dx, int *dy) {
    const uint64_t h = mwb_levels_mix(key + MWB_LEVELS_GOLD * ((uint64_t)index + 1));
    *dx = dx_lo + (int)(((h >> 32) * (uint64_t)(dx_hi - dx_lo + 1)) >> 32);
    *dy = dy_lo + (int)(((h & 0xffffffffULL) * (uint64_t)(dy_hi - dy_lo + 1)) >> 32);
}
