// mwb_terminal_map.h - which compact row the terminal observation of an ended env gets, and where the history of its stacked
// observation lies in the fused frame stack: the arithmetic of mwb_terminal_enable's pass (mwb_terminal.hip).
//
// Plain C++ without any HIP type, so that the same functions run in the kernels, in the host API and in a host program
// (tests/test_terminal_host.py builds one around this header), as mwb_rollout_map.h.
//
// The reference's VecEnv worker resets a finished env inside step (vec_env/subproc_vec_env.py:10-13) and returns the reset
// frame; the frame step() rendered at `done` (miniworld.py:708-711 raise it by the clock, the task rules on top) is lost.  The
// terminal pass renders that frame before the reset and hands it out in compact rows:
//
//   rank of env e    the number of envs e' < e that ended in the same step: ascending env index, so that the rows do not depend on
//                    the order in which the step kernels' atomicAdd filled reset_list
//   row of rank r    r while r < capacity, otherwise none (-1): the env ended, its terminal frame is rendered, but no stacked row
//                    is written for it; it is counted in `dropped`
//   count            all ended envs of the step, possibly more than capacity
//
// The fused stack keeps per env K planes, of which the window [stk_pos, stk_pos + C) (C = nstack * cpf) is the stacked
// observation of the pass; its newest frame group is the last one.  When a step advances the window by one frame (or slides it
// back to plane 0: the history is copied to the front first) the planes [stk_pos, stk_pos + C - cpf) are the nstack - 1 frame
// groups before the step's frame - the history of the terminal observation, zeros included where the episode was shorter.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MWB_TERMINAL_HD __host__ __device__
#else
#define MWB_TERMINAL_HD
#endif

#define MWB_TERMINAL_TILE 1024   // envs terminal_rank_kernel's one workgroup ranks per turn

// rank among the step's ended envs -> compact row, or -1 for an env that gets none
MWB_TERMINAL_HD static inline int mwb_terminal_row(int rank, int capacity) { return rank < capacity ? rank : -1; }

// the rank of an ended env: ended envs in the tiles before its tile, in the waves of its tile before its wave, in the lanes of its
// wave below its lane
MWB_TERMINAL_HD static inline int mwb_terminal_rank(int tiles_before, int waves_before, int lanes_below) { return tiles_before + waves_before + lanes_below; }

// rows written by a step in which `count` envs ended, and the envs that got none
MWB_TERMINAL_HD static inline int mwb_terminal_rows(int count, int capacity) { return count < capacity ? count : capacity; }
MWB_TERMINAL_HD static inline int mwb_terminal_dropped_of(int count, int capacity) { return count > capacity ? count - capacity : 0; }

// first plane of history group g (0 = oldest, g < nstack - 1) of the window that starts at plane stk_pos; cpf planes per frame
MWB_TERMINAL_HD static inline int mwb_terminal_history_plane(int stk_pos, int g, int cpf) { return stk_pos + g * cpf; }
// planes of the whole history (one contiguous run of the env's planes) and the plane of the row that takes the terminal frame
MWB_TERMINAL_HD static inline int mwb_terminal_history_planes(int nstack, int cpf) { return (nstack - 1) * cpf; }
// the window position of the pass after the one at `from` (K planes per env): one frame on, or back to 0 when the next window
// would pass the end - the rule of the fused stack's advance, restated for the tests of the arithmetic above
MWB_TERMINAL_HD static inline int mwb_terminal_next_pos(int from, int nstack, int cpf, int K) {
    const int pos = from + cpf;
    return pos + nstack * cpf > K ? 0 : pos;
}

// the whole ranking, serially: what terminal_rank_kernel computes with ballots and a prefix over its waves.  row_of [N], row_env
// [capacity] (-1 behind the rows written).  Returns count; *dropped receives the envs without a row.
static inline int mwb_terminal_rank_serial(const uint8_t *reset_set, int N, int capacity, int32_t *row_of, int32_t *row_env, int *dropped) {
    int count = 0;
    for (int t0 = 0; t0 < N; t0 += MWB_TERMINAL_TILE) {   // tile by tile, wave by wave, as the kernel does
        int in_tile = 0;
        for (int w0 = t0; w0 < N && w0 < t0 + MWB_TERMINAL_TILE; w0 += 64) {
            int in_wave = 0;
            for (int e = w0; e < N && e < w0 + 64; e++) {
                const int ended = reset_set[e] != 0;
                const int row = ended ? mwb_terminal_row(mwb_terminal_rank(count, in_tile, in_wave), capacity) : -1;
                row_of[e] = row;
                if (row >= 0) row_env[row] = e;
                in_wave += ended;
            }
            in_tile += in_wave;
        }
        count += in_tile;
    }
    for (int r = mwb_terminal_rows(count, capacity); r < capacity; r++) row_env[r] = -1;
    *dropped = mwb_terminal_dropped_of(count, capacity);
    return count;
}
