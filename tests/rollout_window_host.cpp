// Host program around gym_miniworld_amd/csrc/mwb_rollout_window_map.h (tests/test_rollout_window_host.py builds and drives it):
// the functions the windowed gather's kernels and the host API share, called with what stdin says, one command per line:
//
//   K seed call                                                  -> key in hex
//   D seed call dx_lo dx_hi dy_lo dy_hi index                    -> "dx dy"
//   C out_w out_h border dx_lo dx_hi dy_lo dy_hi                 -> the number of the limit the window breaks (0: none)
//   W W H out_w out_h border dx_lo dx_hi dy_lo dy_hi dx dy       -> "O dx dy" (the clamped pair), then per output pixel, x-major,
//                                                                   "sx sy" (the source pixel) or "zero"
//   M d                                                          -> mismatches of n / d by the magic multiplication over n < 2^20
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include "mwb_rollout_window_map.h"

int main() {
    char cmd[8];
    while (scanf("%7s", cmd) == 1) {
        if (!strcmp(cmd, "K")) {
            uint64_t seed, call;
            if (scanf("%" SCNu64 " %" SCNu64, &seed, &call) != 2) return 2;
            printf("%016" PRIx64 "\n", mwb_window_key(seed, call));
        } else if (!strcmp(cmd, "D")) {
            uint64_t seed, call;
            int r[4];
            int64_t index;
            if (scanf("%" SCNu64 " %" SCNu64 " %d %d %d %d %" SCNd64, &seed, &call, &r[0], &r[1], &r[2], &r[3], &index) != 7) return 2;
            int dx, dy;
            mwb_window_draw(mwb_window_key(seed, call), index, r[0], r[1], r[2], r[3], &dx, &dy);
            printf("%d %d\n", dx, dy);
        } else if (!strcmp(cmd, "C")) {
            int w[7];
            for (int i = 0; i < 7; i++)
                if (scanf("%d", &w[i]) != 1) return 2;
            const int limit = mwb_window_check(w[0], w[1], w[2], w[3], w[4], w[5], w[6]);
            printf("%d %s\n", limit, mwb_window_limit_text(limit));
        } else if (!strcmp(cmd, "W")) {
            int W, H, w[7], odx, ody;
            if (scanf("%d %d", &W, &H) != 2) return 2;
            for (int i = 0; i < 7; i++)
                if (scanf("%d", &w[i]) != 1) return 2;
            if (scanf("%d %d", &odx, &ody) != 2) return 2;
            if (mwb_window_check(w[0], w[1], w[2], w[3], w[4], w[5], w[6])) return 3;
            const int dx = mwb_window_clamp(odx, w[3], w[4]), dy = mwb_window_clamp(ody, w[5], w[6]);
            printf("O %d %d\n", dx, dy);
            for (int x = 0; x < w[0]; x++)
                for (int y = 0; y < w[1]; y++) {
                    int sx = -1, sy = -1;
                    const int shown = mwb_window_source(x, y, dx, dy, W, H, w[2], &sx, &sy);
                    if (sx < 0 || sx >= W || sy < 0 || sy >= H) return 4;   // the coordinates an address is formed from
                    if (shown) printf("%d %d\n", sx, sy);
                    else printf("zero\n");
                }
        } else if (!strcmp(cmd, "M")) {
            unsigned d;
            if (scanf("%u", &d) != 1 || d < 1 || d > MWB_WINDOW_MAX_OUT) return 2;
            const uint64_t magic = mwb_window_div_magic(d);
            long bad = 0;
            for (uint32_t n = 0; n < (1u << 20); n++) bad += mwb_window_div(n, magic) != n / d;
            printf("%ld\n", bad);
        } else {
            return 1;
        }
    }
    return 0;
}
