// mwb_repeat_fold.h - how mwb_step_repeat folds the outputs of its sub-steps into one transition per env.
//
// Plain C++ without any HIP type, so that the same rule runs in repeat_fold_kernel (mwb_repeat.hip) and in a host program
// (tests/test_repeat_fold_host.py builds one around this header).
//
// The reference is the frame-skip loop a trainer puts around env.step inside the worker of vec_env/subproc_vec_env.py:5-33,
// under the worker's auto-reset:
//     total = 0.0
//     for _ in range(n): obs, r, done, info = env.step(a); total += r; taken += 1
//                        if done: break
// One call of mwb_repeat_fold per env after every sub-step's step kernel, sub = 0 .. repeat - 1, with what that kernel left in
// the env's output slots.  While an env is frozen the step kernels do not touch it, so those slots still hold the values of its
// last sub-step and the rule ignores them.
//   sum     float64 sum of the sub-steps' rewards in sub-step order, starting from 0.0
//   taken   sub-steps the env took (0 for an env the caller's skip mask names: it takes the 'dummy' path once)
//   same    every sub-step so far left the env's frame as it was (the AND of the step kernel's frame_same)
//   frozen  the env takes no further sub-step in this call: it is done, masked, or has reached its count
// Sub-step 0 initialises all four: nothing carries over from one call to the next.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MWB_FOLD_HD __host__ __device__
#else
#define MWB_FOLD_HD
#endif

struct MwbFoldEnv {
    double sum;
    int32_t taken;
    uint8_t same, frozen;
};

// sub-steps env i may take: counts[i] clamped to [1, repeat] (on the device, so that the host never has to look at counts)
MWB_FOLD_HD static inline int32_t mwb_repeat_count(int32_t raw, int32_t repeat) { return raw < 1 ? 1 : (raw > repeat ? repeat : raw); }

// masked: the caller's skip mask names the env (only looked at in sub-step 0; such an env is frozen from then on).
// reward64 / done / frame_same: the env's output slots after sub-step `sub`; count: mwb_repeat_count of the env.
MWB_FOLD_HD static inline void mwb_repeat_fold(MwbFoldEnv &s, int sub, int masked, double reward64, int done, int frame_same, int32_t count) {
    if (sub == 0) { s.sum = 0.0; s.taken = 0; s.same = 1; s.frozen = 0; }
    if (s.frozen) return;
    s.sum += reward64;
    s.same = (uint8_t)(s.same && frame_same);
    if (sub == 0 && masked) { s.frozen = 1; return; }   // reward -99 once, not a sub-step
    s.taken += 1;
    s.frozen = (uint8_t)(done || s.taken >= count);
}

// what the call leaves in frame_same[e] after its last sub-step: the env's last frame stands only if no sub-step changed anything
// it depends on and the env is not being regenerated
MWB_FOLD_HD static inline int mwb_repeat_frame_same(const MwbFoldEnv &s, int reset_set) { return s.same && !reset_set; }
