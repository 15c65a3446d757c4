// Host program around gym_miniworld_amd/csrc/mwb_terminal_map.h (tests/test_terminal_host.py): ranks the ended envs of one step as
// terminal_rank_kernel does - tile by tile, wave by wave, through the header's own functions - and walks the fused stack's window
// over a run of passes, printing where the history groups of a terminal observation lie.
//
// stdin:  N capacity, then N flags (reset_set); then nstack cpf K passes
// stdout: C count dropped     ended envs of the step, envs without a row
//         R e row             row_of[e], only for envs with a flag or a row (the others must be -1: checked here, exit 5)
//         E r env             row_env[r] for r < capacity
//         W p pos             the window's first plane in pass p (pass 0: a reset, plane 0; then one step each)
//         H p g plane         first plane of history group g of a terminal observation rendered in pass p
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "mwb_terminal_map.h"

int main() {
    int N, capacity;
    if (scanf("%d %d", &N, &capacity) != 2 || N < 1 || capacity < 1 || capacity > N) return 2;
    std::vector<uint8_t> set((size_t)N);
    for (int e = 0; e < N; e++) {
        int f;
        if (scanf("%d", &f) != 1) return 2;
        set[e] = (uint8_t)f;
    }
    std::vector<int32_t> row_of((size_t)N, -7), row_env((size_t)capacity, -7);
    int dropped = -1;
    const int count = mwb_terminal_rank_serial(set.data(), N, capacity, row_of.data(), row_env.data(), &dropped);
    printf("C %d %d\n", count, dropped);
    for (int e = 0; e < N; e++) {
        if (!set[e] && row_of[e] != -1) return 5;
        if (set[e] || row_of[e] >= 0) printf("R %d %d\n", e, row_of[e]);
    }
    for (int r = 0; r < capacity; r++) printf("E %d %d\n", r, row_env[r]);
    if (mwb_terminal_rows(count, capacity) + dropped != count) return 6;

    int nstack, cpf, K, passes;
    if (scanf("%d %d %d %d", &nstack, &cpf, &K, &passes) != 4 || nstack < 1 || cpf < 1 || K < nstack * cpf || passes < 1) return 2;
    int pos = 0;
    for (int p = 0; p < passes; p++) {
        if (p) pos = mwb_terminal_next_pos(pos, nstack, cpf, K);
        if (pos < 0 || pos + nstack * cpf > K) return 7;   // the window lies inside the env's planes
        printf("W %d %d\n", p, pos);
        for (int g = 0; g < nstack - 1; g++) printf("H %d %d %d\n", p, g, mwb_terminal_history_plane(pos, g, cpf));
        if (mwb_terminal_history_plane(pos, 0, cpf) + mwb_terminal_history_planes(nstack, cpf) != pos + (nstack - 1) * cpf) return 8;
    }
    return 0;
}
