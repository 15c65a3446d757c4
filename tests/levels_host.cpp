// Host program around gym_miniworld_amd/csrc/mwb_levels_map.h (tests/test_levels_host.py): the functions levels_assign_kernel and
// mwb_seed share - SHA-512 of a decimal seed, the MT19937 key, init_by_array over a row accessor, the three level rules - answer
// one request per input line.
//
// stdin lines                                   stdout lines
//   D seed                                        128 hex digits of sha512(str(seed)), then key0 key1 key_length
//   R key0 key1 key_length                        the 625 words init_by_array leaves for that key (624 state words, the position)
//   Q seed                                        the 625 words of the row of that seed
//   C mode g n L stride sampler_seed request      level rejected
//   M x L                                         x mod L by mwb_levels_mod
//   S i start_level                               the seed of level i of a set without a table
//   U sampler_seed L kind                         L counts of 65536 UNIFORM draws: kind 0 = g 0 .. 4095 x n 0 .. 15, 1 = env 5's
//                                                 stream n 0 .. 65535, 2 = episode 3 of envs g 0 .. 65535
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "mwb_levels_map.h"

static void print_row(uint32_t key0, uint32_t key1, int n, const uint32_t *base) {
    std::vector<uint32_t> mt(625, 0xDEADBEEFu);   // exactly 625 words: a write past the row is AddressSanitizer's to find
    MwbLevelsPlainRow row = {mt.data()};
    mwb_levels_init_by_array(row, base, key0, key1, n);
    for (int i = 0; i < 625; i++) printf("%u%c", mt[i], i == 624 ? '\n' : ' ');
}

int main() {
    uint32_t base[624];
    mwb_levels_mt_base(base);
    char line[256];
    while (fgets(line, sizeof(line), stdin)) {
        uint64_t a, b, c, d, e, f;
        int64_t req;
        unsigned k0, k1;
        int n, mode;
        if (sscanf(line, "D %" SCNu64, &a) == 1) {
            uint64_t dig[8];
            uint32_t key[2];
            mwb_levels_sha512_decimal(a, dig);
            n = mwb_levels_seed_key(a, key);
            for (int i = 0; i < 8; i++) printf("%016" PRIx64, dig[i]);
            printf(" %u %u %d\n", key[0], key[1], n);
        } else if (sscanf(line, "R %u %u %d", &k0, &k1, &n) == 3) {
            if (n != 1 && n != 2) return 3;
            print_row(k0, k1, n, base);
        } else if (sscanf(line, "Q %" SCNu64, &a) == 1) {
            uint32_t key[2];
            n = mwb_levels_seed_key(a, key);
            print_row(key[0], key[1], n, base);
        } else if (sscanf(line, "C %d %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNd64, &mode, &a, &b, &c, &d, &e, &req) == 7) {
            if (c < 1 || c > (uint64_t)MWB_LEVELS_MAX) return 3;
            int rejected = -1;
            const int32_t i = mwb_levels_choose(mode, a, b, c, d, e, (int32_t)req, &rejected);
            if (i < 0 || (uint64_t)i >= c) return 4;   // a level of the set, whatever the request was
            printf("%d %d\n", i, rejected);
        } else if (sscanf(line, "M %" SCNu64 " %" SCNu64, &a, &b) == 2) {
            if (b < 1 || b > (uint64_t)MWB_LEVELS_MAX) return 3;
            printf("%u\n", mwb_levels_mod(a, (uint32_t)b));
        } else if (sscanf(line, "S %" SCNu64 " %" SCNu64, &a, &f) == 2) {
            printf("%" PRIu64 "\n", mwb_levels_seed_of((int32_t)a, f, nullptr));
        } else if (sscanf(line, "U %" SCNu64 " %" SCNu64 " %d", &a, &b, &mode) == 3) {
            if (b < 1 || b > 100000 || mode < 0 || mode > 2) return 3;
            std::vector<unsigned> counts((size_t)b, 0u);
            for (uint64_t k = 0; k < 65536; k++) {
                const uint64_t g = mode == 0 ? k >> 4 : mode == 1 ? 5 : k, ep = mode == 0 ? k & 15 : mode == 1 ? k : 3;
                counts[(size_t)mwb_levels_uniform(a, g, ep, b)]++;
            }
            for (uint64_t i = 0; i < b; i++) printf("%u%c", counts[(size_t)i], i + 1 == b ? '\n' : ' ');
        } else if (line[0] != '\n') {
            return 2;
        }
    }
    return 0;
}
