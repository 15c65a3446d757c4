// Host program around gym_miniworld_amd/csrc/mwb_copy_check.h (tests/test_copy_envs_host.py): runs the three passes of
// mwb_copy_envs' pair validation exactly as copy_validate_kernel does, on the CPU.
//   copy_check_host n_dst n_src same_handle dst0 src0 dst1 src1 ...
// prints one verdict per pair (0 copy, 1 identity, 2 rejected) and, last, 1 if the scratch arrays are all zero again.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mwb_copy_check.h"

int main(int argc, char **argv) {
    if (argc < 4 || (argc - 4) % 2) return 2;
    const int32_t n_dst = (int32_t)atoll(argv[1]), n_src = (int32_t)atoll(argv[2]);
    const int same = atoi(argv[3]);
    const int count = (argc - 4) / 2;
    std::vector<int32_t> dst(count), src(count);
    for (int i = 0; i < count; i++) { dst[i] = (int32_t)atoll(argv[4 + 2 * i]); src[i] = (int32_t)atoll(argv[5 + 2 * i]); }
    // exactly n entries, heap-allocated: an index that slips past the range check is caught by a sanitizer build of this program
    std::vector<int32_t> pairs_at((size_t)n_dst, 0);
    std::vector<uint8_t> mark((size_t)(same ? n_src : 0), 0);
    for (int i = 0; i < count; i++) {
        if (mwb_copy_counts_dst(dst[i], n_dst)) pairs_at.at(dst[i])++;
        if (mwb_copy_marks_src(dst[i], src[i], n_src, same)) mark.at(src[i]) = 1;
    }
    for (int i = 0; i < count; i++) {
        const bool in = mwb_copy_index_ok(dst[i], n_dst);
        printf("%d ", mwb_copy_verdict(dst[i], src[i], n_dst, n_src, same, in ? pairs_at.at(dst[i]) : 0, in && same ? mark.at(dst[i]) : 0));
    }
    for (int i = 0; i < count; i++) {
        if (mwb_copy_counts_dst(dst[i], n_dst)) pairs_at.at(dst[i]) = 0;
        if (mwb_copy_marks_src(dst[i], src[i], n_src, same)) mark.at(src[i]) = 0;
    }
    int clean = 1;
    for (int32_t v : pairs_at) clean &= v == 0;
    for (uint8_t v : mark) clean &= v == 0;
    printf("%d\n", clean);
    return 0;
}
