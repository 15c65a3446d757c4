// Host program around gym_miniworld_amd/csrc/mwb_dispatch_map.h (tests/test_dispatch_map_host.py builds and runs it).
//   dispatch_map_host                 every N <= 12, split_envs in [0, N + 2], R + C <= N, grid = N + split_envs: checks the cover of
//                                     both lists, prints "checked <launches> launches" and exits 0, or prints the first violations
//                                     and exits 1
//   dispatch_map_host N split R C     prints "role index part" of every block of that launch
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "mwb_dispatch_map.h"

static int g_bad = 0;
static void bad(const char *what, int N, int split, int R, int C, int b) {
    if (g_bad++ < 20) printf("VIOLATION %s: N %d split %d R %d C %d block or entry %d\n", what, N, split, R, C, b);
}

// one launch: every entry of render_list by exactly one whole block or by each of its two halves exactly once, every entry of
// reuse_list by exactly one copy, no index out of range, and no work for the blocks behind
static void check_launch(int N, int split, int R, int C) {
    const int grid = N + split;
    std::vector<int> whole(R, 0), half0(R, 0), half1(R, 0), copied(C, 0);
    const int S = split < R ? split : R;
    int last_busy = -1;
    for (int b = 0; b < grid; b++) {
        const MwbDispatch m = mwb_dispatch_map(b, R, C, split, grid);
        if (m.role == MWB_ROLE_RENDER) {
            last_busy = b;
            if (m.index < 0 || m.index >= R) { bad("render index out of range", N, split, R, C, b); continue; }
            if (m.part == -1) whole[m.index]++;
            else if (m.part == 0) half0[m.index]++;
            else if (m.part == 1) half1[m.index]++;
            else bad("part out of range", N, split, R, C, b);
            if ((m.part >= 0) != (m.index >= R - S)) bad("halves are the last min(split, R) entries, and only they", N, split, R, C, b);
        } else if (m.role == MWB_ROLE_COPY) {
            last_busy = b;
            if (m.index < 0 || m.index >= C) { bad("copy index out of range", N, split, R, C, b); continue; }
            copied[m.index]++;
        } else if (m.role != MWB_ROLE_EXIT) bad("unknown role", N, split, R, C, b);
    }
    for (int i = 0; i < R; i++) {
        const bool as_whole = whole[i] == 1 && half0[i] == 0 && half1[i] == 0, as_halves = whole[i] == 0 && half0[i] == 1 && half1[i] == 1;
        if (!as_whole && !as_halves) bad("render entry not covered exactly once", N, split, R, C, i);
    }
    for (int j = 0; j < C; j++) if (copied[j] != 1) bad("reuse entry not copied exactly once", N, split, R, C, j);
    // the work is a prefix of the grid: R - S whole frames, 2 S halves, C copies; everything behind exits
    if (last_busy != R + S + C - 1) bad("blocks beyond the work must exit", N, split, R, C, last_busy);
    // a block number outside the grid has no work
    if (mwb_dispatch_map(-1, R, C, split, grid).role != MWB_ROLE_EXIT || mwb_dispatch_map(grid, R, C, split, grid).role != MWB_ROLE_EXIT)
        bad("block outside the grid", N, split, R, C, grid);
}

int main(int argc, char **argv) {
    if (argc >= 5) {
        const int N = atoi(argv[1]), split = atoi(argv[2]), R = atoi(argv[3]), C = atoi(argv[4]);
        for (int b = 0; b < N + split; b++) {
            const MwbDispatch m = mwb_dispatch_map(b, R, C, split, N + split);
            printf("%d %d %d\n", m.role, m.index, m.part);
        }
        return 0;
    }
    long launches = 0;
    for (int N = 0; N <= 12; N++)
        for (int split = 0; split <= N + 2; split++)
            for (int R = 0; R <= N; R++)
                for (int C = 0; R + C <= N; C++) { check_launch(N, split, R, C); launches++; }
    if (g_bad) { printf("%d violations\n", g_bad); return 1; }
    printf("checked %ld launches\n", launches);
    return 0;
}
