// mwb_copy_check.h - which (destination, source) pairs of an mwb_copy_envs call are carried out.
//
// Plain C++ without any HIP type, so that the same functions run in copy_validate_kernel (the only device code that reads an
// index nobody has checked yet) and in a host program (tests/test_copy_envs_host.py builds one around this header).
//
// The rules (include/miniworld_batch.h at mwb_copy_envs).  A pair (dst, src) is rejected when
//   - dst is outside [0, n_dst) or src is outside [0, n_src),
//   - more than one pair of the call names dst as its destination,
//   - both handles are the same one and dst is also the source of some pair;
// except that on one handle dst == src is valid and copies nothing (an identity pair: neither rejected nor carried out).
// They are evaluated in two passes over the index lists, around two per-env scratch arrays of the handles that are all zero
// between calls:
//   pass 1  every pair counts itself at its destination (mwb_copy_counts_dst) and marks its source (mwb_copy_marks_src)
//   pass 2  mwb_copy_verdict(pair, the count at its destination, the mark at its destination)
//   pass 3  the same walk puts the scratch back to zero (every entry pass 1 touched belongs to an index that is in range)
// Counting and marking are deliberately conservative: a pair that is itself rejected (say for its source index) still counts at
// its destination and still marks its source, so what a call does never depends on the order of its pairs.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MWB_COPY_HD __host__ __device__
#else
#define MWB_COPY_HD
#endif

enum { MWB_PAIR_COPY = 0, MWB_PAIR_IDENTITY = 1, MWB_PAIR_REJECTED = 2 };

MWB_COPY_HD static inline int mwb_copy_index_ok(int32_t idx, int32_t n) { return idx >= 0 && idx < n; }

// pass 1: does the pair add one to its destination's pair count / set its source's mark?  (the caller indexes the scratch
// arrays only where these say yes: they imply that the index is in range)
MWB_COPY_HD static inline int mwb_copy_counts_dst(int32_t dst, int32_t n_dst) { return mwb_copy_index_ok(dst, n_dst); }
MWB_COPY_HD static inline int mwb_copy_marks_src(int32_t dst, int32_t src, int32_t n_src, int same_handle) {
    return same_handle && mwb_copy_index_ok(src, n_src) && dst != src;
}

// pass 2: dst_pairs = pairs counted at dst, dst_is_src = the mark at dst (both only read when dst is in range; pass 0 otherwise)
MWB_COPY_HD static inline int mwb_copy_verdict(int32_t dst, int32_t src, int32_t n_dst, int32_t n_src, int same_handle,
                                               int32_t dst_pairs, int dst_is_src) {
    if (!mwb_copy_index_ok(dst, n_dst) || !mwb_copy_index_ok(src, n_src)) return MWB_PAIR_REJECTED;
    if (dst_pairs != 1) return MWB_PAIR_REJECTED;
    if (same_handle && dst == src) return MWB_PAIR_IDENTITY;
    if (same_handle && dst_is_src) return MWB_PAIR_REJECTED;
    return MWB_PAIR_COPY;
}
