// mwb_rollout_map.h - where the frames of a rollout live: the ring arithmetic of mwb_rollout_push / mwb_rollout_gather /
// mwb_rollout_after_update and the rule that says which frames of a stacked observation are zeros.
//
// Plain C++ without any HIP type, so that the same functions run in the kernels (mwb_rollout.hip), in the host API and in a host
// program (tests/test_rollout_host.py builds one around this header).
//
// The reference is RolloutStorage.obs (pytorch-a2c-ppo-acktr/storage.py:12,55,75,121), a [T + 1][N] array of the stacked
// observations VecPyTorchFrameStack (envs.py:135-165) returned.  Row t of it is, per env, the last nstack frames with everything
// before the episode's first frame zeroed.  The rollout keeps every frame ONCE, in a time-major ring of R slots, and one byte per
// (t, env): age = how many frames before frame t belong to the observation (0 at an episode's first frame, nstack - 1 at most).
//
//   logical time t of the current window (0 .. T)          slot (base + t) mod R
//   the frame j steps before it (j = 0 .. nstack - 1)      slot (base + t - j + R) mod R   - also for t - j < 0: the last frames
//                                                          of the window before, which after_update left where they were
//   after_update                                           base = (base + T) mod R: time T becomes time 0, no frame moves
//
// R = T + nstack is the smallest ring that works.  A window's times 0 .. T need the slots base - (nstack - 1) .. base + T, that
// is T + nstack of them, while its own pushes (t = 1 .. T) are being written: R >= T + nstack.  With R = T + nstack the pushes of
// the NEXT window (base' = base + T) land on base' + 1 .. base' + T = base' - (nstack - 1) - 1 - (T - 1) .. base' - nstack (mod R):
// the last of them nstack slots behind its time 0, one slot clear of the nstack - 1 history slots base' - (nstack - 1) .. base' - 1.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MWB_ROLLOUT_HD __host__ __device__
#else
#define MWB_ROLLOUT_HD
#endif

MWB_ROLLOUT_HD static inline int mwb_rollout_ring_slots(int num_steps, int nstack) { return num_steps + nstack; }

// slot of the frame j steps before logical time t; base in [0, R), t in [0, T], j in [0, nstack): the sum lies in (0, 3 R), never
// negative, and fits an int (mwb_rollout_enable bounds num_steps by 2^24)
MWB_ROLLOUT_HD static inline int mwb_rollout_slot(int base, int t, int j, int R) { return (base + t - j + R) % R; }

// age[t][e] from age[t - 1][e]: `fresh` = frame t is the first of an episode (the env was done, or the caller's fresh list names it)
MWB_ROLLOUT_HD static inline uint8_t mwb_rollout_age(int fresh, int prev_age, int nstack) {
    return (uint8_t)(fresh ? 0 : (prev_age + 1 < nstack - 1 ? prev_age + 1 : nstack - 1));
}

// frame group k (0 = oldest) of the stacked observation at time t of an env whose age there is `age`: the slot to read, or -1 for zeros
MWB_ROLLOUT_HD static inline int mwb_rollout_source(int base, int t, int k, int nstack, int R, int age) {
    const int j = nstack - 1 - k;
    return j <= age ? mwb_rollout_slot(base, t, j, R) : -1;
}

MWB_ROLLOUT_HD static inline int mwb_rollout_next_base(int base, int num_steps, int R) { return (base + num_steps) % R; }

// a gather index names (t, env) = (index / N, index % N) with t in 0 .. cursor
MWB_ROLLOUT_HD static inline int mwb_rollout_index_ok(int64_t index, int cursor, int N) { return index >= 0 && index < ((int64_t)cursor + 1) * N; }
