// mwb_repeat.hip - the kernel of mwb_step_repeat: k sub-steps of MiniWorldEnv.step per call, one render.
//
// A call launches the step kernel k times.  After each launch repeat_fold_kernel (one thread per env, every access a coalesced
// row) folds that sub-step's outputs into the call's per-env scratch by the rule of mwb_repeat_fold.h and decides which envs are
// frozen: from the next launch on the step kernels leave those completely untouched (MwbDev::frozen), so their done, ep_steps,
// feature, goal_pos, reset_set, reset_list entry and render override stay those of their last sub-step.  After the last
// sub-step the same kernel writes the summed reward and the call's frame_same; the rest of the pass (regeneration, prep, render)
// then runs as it does after a single mwb_step.  No LDS, no atomics; 14 bytes of scratch per env.
#include "mwb_internal.h"
#include "mwb_repeat_fold.h"

#define FOLD_THREADS 256

__global__ void __launch_bounds__(FOLD_THREADS) repeat_fold_kernel(MwbDev d, int sub, int last, int repeat, const uint8_t *__restrict__ skip,
                                                                   const int32_t *__restrict__ counts, double *__restrict__ sum,
                                                                   int32_t *__restrict__ taken, uint8_t *__restrict__ same,
                                                                   uint8_t *__restrict__ frozen) {
    const int e = blockIdx.x * FOLD_THREADS + threadIdx.x;
    if (e >= d.N) return;
    MwbFoldEnv s;
    s.sum = sum[e]; s.taken = taken[e]; s.same = same[e]; s.frozen = sub ? frozen[e] : 0;
    if (!s.frozen) {   // a frozen env's slots were not rewritten by this sub-step: nothing to fold
        const int masked = sub == 0 && skip && skip[e];
        const int32_t count = mwb_repeat_count(counts ? counts[e] : repeat, repeat);
        mwb_repeat_fold(s, sub, masked, d.reward64[e], d.done[e], d.frame_same ? d.frame_same[e] : 0, count);
        sum[e] = s.sum; taken[e] = s.taken; same[e] = s.same; frozen[e] = s.frozen;
    }
    if (last) {
        d.reward64[e] = s.sum; d.reward[e] = (float)s.sum;
        if (d.frame_same) d.frame_same[e] = (uint8_t)mwb_repeat_frame_same(s, d.reset_set[e]);
    }
}

void mwb_launch_repeat_fold(const MwbDev &d, int sub, int last, int repeat, const uint8_t *skip, const int32_t *counts, double *sum,
                            int32_t *taken, uint8_t *same, uint8_t *frozen, hipStream_t s) {
    hipLaunchKernelGGL(repeat_fold_kernel, dim3((d.N + FOLD_THREADS - 1) / FOLD_THREADS), dim3(FOLD_THREADS), 0, s, d, sub, last, repeat, skip,
                       counts, sum, taken, same, frozen);
}
