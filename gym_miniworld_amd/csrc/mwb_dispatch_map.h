// mwb_dispatch_map.h - which workgroup of a step's bulk render launch does what.
//
// Plain C++ without any HIP type, so that the same function runs in render_body (MODE 2) and in a host program
// (tests/test_dispatch_map_host.py builds one around this header).
//
// prep_kernel(mode 2) leaves two lists: render_list[0 .. R), the envs this launch renders, in the order of the cost map in use
// (dearest first), and reuse_list[0 .. C), the envs whose last frame is copied.  Regenerated envs are in neither (R + C <= N).
// The launch has grid = N + split_envs blocks whatever R and C are - the host knows neither.  With S = min(split_envs, R):
//   blocks [0, R - S)            render render_list[b] whole
//   blocks [R - S, R + S)        render the last S entries - the cheapest frames - as two half-frame workgroups each
//   blocks [R + S, R + S + C)    copy reuse_list[b - (R + S)], one env each (R + S + C <= N + split_envs: there are enough blocks)
//   every block behind them exits
// So the launch starts every rendering workgroup before any that only copies or exits, and its last units are halves.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MWB_DISPATCH_HD __host__ __device__
#else
#define MWB_DISPATCH_HD
#endif

enum { MWB_ROLE_EXIT = 0, MWB_ROLE_RENDER = 1, MWB_ROLE_COPY = 2 };

struct MwbDispatch {
    int32_t role;    // MWB_ROLE_*
    int32_t index;   // RENDER: entry of render_list; COPY: entry of reuse_list
    int32_t part;    // RENDER: -1 the whole frame, 0 / 1 one half of it
};

MWB_DISPATCH_HD static inline MwbDispatch mwb_dispatch_map(int32_t b, int32_t R, int32_t C, int32_t split_envs, int32_t grid) {
    MwbDispatch m = {MWB_ROLE_EXIT, 0, -1};
    if (b < 0 || b >= grid || R < 0 || C < 0) return m;
    const int32_t S = split_envs < 0 ? 0 : (split_envs < R ? split_envs : R);
    const int32_t whole = R - S;
    if (b < whole) { m.role = MWB_ROLE_RENDER; m.index = b; return m; }
    const int32_t h = b - whole;   // >= 0
    if (h < 2 * S) { m.role = MWB_ROLE_RENDER; m.index = whole + (h >> 1); m.part = h & 1; return m; }
    if (h - 2 * S < C) { m.role = MWB_ROLE_COPY; m.index = h - 2 * S; }
    return m;
}
