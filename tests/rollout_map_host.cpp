// Host program around gym_miniworld_amd/csrc/mwb_rollout_map.h (tests/test_rollout_host.py): plays the pushes and after_updates of
// a rollout exactly as the API and the kernels do - base and cursor as mwb_api.hip keeps them, the age rows as rollout_push_kernel
// and rollout_after_update_kernel write them - and prints where every frame of every stacked observation is read from.
//
// stdin:  T nstack E W, then W * T lines of E flags: fresh[e] of push t = 1 .. T of window w = 0 .. W - 1
// stdout: P w t slot          the push of logical time t of window w writes this slot (t = 0: the reset push, window 0 only)
//         G w t e age         age[t][e] as that push (or the after_update that opened window w, t = 0) left it
//         M w c t e k slot    with the cursor at c: frame group k of (t, e) is read from this slot, -1 = zeros; after every push
//                             and every after_update, for all t <= c
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "mwb_rollout_map.h"

int main() {
    int T, nstack, E, W;
    if (scanf("%d %d %d %d", &T, &nstack, &E, &W) != 4 || T < 1 || nstack < 1 || E < 1 || W < 1) return 2;
    const int R = mwb_rollout_ring_slots(T, nstack);
    std::vector<uint8_t> age((size_t)(T + 1) * E, 0);
    int base = 0, cursor = -1;
    auto dump = [&](int w) {
        for (int t = 0; t <= cursor; t++)
            for (int e = 0; e < E; e++)
                for (int k = 0; k < nstack; k++)
                    printf("M %d %d %d %d %d %d\n", w, cursor, t, e, k, mwb_rollout_source(base, t, k, nstack, R, age[(size_t)t * E + e]));
    };
    // the reset push
    cursor = 0;
    printf("P 0 0 %d\n", mwb_rollout_slot(base, 0, 0, R));
    for (int e = 0; e < E; e++) { age[e] = 0; printf("G 0 0 %d 0\n", e); }
    dump(0);
    for (int w = 0; w < W; w++) {
        if (w > 0) {   // after_update: row T becomes row 0, base moves T slots on
            for (int e = 0; e < E; e++) { age[e] = age[(size_t)T * E + e]; printf("G %d 0 %d %d\n", w, e, age[e]); }
            base = mwb_rollout_next_base(base, T, R);
            cursor = 0;
            dump(w);
        }
        for (int t = 1; t <= T; t++) {
            if (cursor >= T) return 3;
            cursor = t;
            printf("P %d %d %d\n", w, t, mwb_rollout_slot(base, t, 0, R));
            for (int e = 0; e < E; e++) {
                int fresh;
                if (scanf("%d", &fresh) != 1) return 2;
                age[(size_t)t * E + e] = mwb_rollout_age(fresh, age[(size_t)(t - 1) * E + e], nstack);
                printf("G %d %d %d %d\n", w, t, e, age[(size_t)t * E + e]);
            }
            dump(w);
        }
    }
    if (!mwb_rollout_index_ok(0, 0, E) || mwb_rollout_index_ok(-1, T, E) || mwb_rollout_index_ok((int64_t)(T + 1) * E, T, E) ||
        !mwb_rollout_index_ok((int64_t)(T + 1) * E - 1, T, E) || mwb_rollout_index_ok((int64_t)1 << 40, T, E))
        return 4;
    return 0;
}
