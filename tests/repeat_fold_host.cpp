// Host program around gym_miniworld_amd/csrc/mwb_repeat_fold.h (tests/test_repeat_fold_host.py): plays one mwb_step_repeat call
// on the CPU.  The sub-steps' results come from stdin; the program keeps the per-env output slots as the step kernels do (an
// env that is frozen is not touched, a masked env takes the skip path in sub-step 0) and folds them exactly as
// repeat_fold_kernel does, one mwb_repeat_fold per env and sub-step.
//   stdin:  repeat n_envs auto_reset
//           per env: masked count frame_same_of_the_skip_path, then `repeat` triples  reward(hex bits of the double) done frame_same
//   stdout: per env: sum(hex bits) reward(hex bits of the float) taken frame_same done last_sub_step_applied(-1 none)
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mwb_repeat_fold.h"

int main() {
    int repeat, n, auto_reset;
    if (scanf("%d %d %d", &repeat, &n, &auto_reset) != 3) return 2;
    for (int e = 0; e < n; e++) {
        int masked, count, skip_same;
        if (scanf("%d %d %d", &masked, &count, &skip_same) != 3) return 2;
        std::vector<double> r(repeat);
        std::vector<int> dn(repeat), fs(repeat);
        for (int j = 0; j < repeat; j++) {
            uint64_t bits;
            if (scanf("%" SCNx64 " %d %d", &bits, &dn[j], &fs[j]) != 3) return 2;
            memcpy(&r[j], &bits, 8);
        }
        // the env's output slots: junk until a step kernel writes them
        double reward64 = 12345.0;
        int done = 1, frame_same = 1, reset_set = 1, applied = -1;
        MwbFoldEnv s;
        memset(&s, 0x5a, sizeof(s));   // nothing carries over from the call before: sub-step 0 must initialise all of it
        for (int sub = 0; sub < repeat; sub++) {
            const bool frozen = sub > 0 && s.frozen;   // what the step kernel of sub-step `sub` sees (null pointer in sub-step 0)
            if (!frozen) {
                if (sub == 0 && masked) { reward64 = -99.0; done = 0; reset_set = 0; frame_same = skip_same; }
                else { reward64 = r[sub]; done = dn[sub]; frame_same = fs[sub] && !(done && auto_reset); reset_set = done && auto_reset; applied = sub; }
            }
            mwb_repeat_fold(s, sub, sub == 0 && masked, reward64, done, frame_same, mwb_repeat_count(count, repeat));
        }
        const float rf = (float)s.sum;
        uint64_t sb; uint32_t fb;
        memcpy(&sb, &s.sum, 8); memcpy(&fb, &rf, 4);
        printf("%" PRIx64 " %x %d %d %d %d\n", sb, fb, (int)s.taken, mwb_repeat_frame_same(s, reset_set), done, applied);
    }
    return 0;
}
