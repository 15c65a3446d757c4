// mwb_copy.hip - the kernels of mwb_copy_envs: env dst_idx[i] of one handle becomes a twin of env src_idx[i] of another (or of
// the same) handle, without leaving the device.
//
//   copy_validate_kernel  the only code that reads the caller's index lists.  Three launches (the passes of mwb_copy_check.h)
//                         leave one int2 {dst, src} per pair, dst = -1 where the pair is not carried out; everything below
//                         reads these and nothing else, so no index reaches an address computation unchecked.
//   copy_envs_kernel      the per-env arrays of MwbDev through the descriptor table (mwb_for_each_copied_array, mwb_internal.h).
//                         <false>: pieces of up to 32 bytes, lane = pair, one workgroup per chunk of rows of one array - with
//                         consecutive destination (and source) indices, the common arange list, a wave moves one contiguous
//                         run of 64 pieces.  <true>: large env-major rows (the MT19937 state, the room table), one workgroup
//                         per pair and array, 16 bytes per lane where both addresses allow it, dwords otherwise (an rng row
//                         is 2500 bytes: only 4-byte aligned).  Whole rows, not their live part.
//   copy_list_kernel      the accepted destinations onto / off the handle's reset_set + reset_list (the existing mode-1
//                         prep and render launches then draw exactly these), or their frame_cached flags down.
//   copy_seg_box_kernel   the group boxes of the copied collision segments (d.seg_box, mwb_seg_groups.h), rebuilt from the
//                         destination's segments - derived data, not on the list of copied arrays.
//   copy_stack_kernel     the visible window of the frame stack, a workgroup per pair and 32 KB of it.
// No scratch, no LDS; a pair that is not carried out costs its lane one 8-byte load.
#include "mwb_internal.h"
#include "mwb_copy_check.h"
#include "mwb_seg_groups.h"

#define COPY_THREADS 256

// phase 0: count / mark, 1: verdicts, 2: scratch back to zero
__global__ void __launch_bounds__(COPY_THREADS) copy_validate_kernel(int phase, const int32_t *__restrict__ dst_idx, const int32_t *__restrict__ src_idx,
                                                                     int count, int n_dst, int n_src, int same_handle, int32_t *__restrict__ dst_pairs,
                                                                     uint8_t *__restrict__ src_mark, int2 *__restrict__ pairs,
                                                                     unsigned long long *__restrict__ rejected) {
    for (size_t i = (size_t)blockIdx.x * COPY_THREADS + threadIdx.x; i < (size_t)count; i += (size_t)gridDim.x * COPY_THREADS) {
        const int32_t dst = dst_idx[i], src = src_idx[i];
        if (phase == 0) {
            if (mwb_copy_counts_dst(dst, n_dst)) atomicAdd(dst_pairs + dst, 1);
            if (mwb_copy_marks_src(dst, src, n_src, same_handle)) src_mark[src] = 1;
        } else if (phase == 1) {
            const bool in = mwb_copy_index_ok(dst, n_dst);
            const int v = mwb_copy_verdict(dst, src, n_dst, n_src, same_handle, in ? dst_pairs[dst] : 0, in && same_handle ? src_mark[dst] : 0);
            pairs[i] = v == MWB_PAIR_COPY ? make_int2(dst, src) : make_int2(-1, -1);
            if (v == MWB_PAIR_REJECTED) atomicAdd(rejected, 1ull);
        } else {
            if (mwb_copy_counts_dst(dst, n_dst)) dst_pairs[dst] = 0;
            if (mwb_copy_marks_src(dst, src, n_src, same_handle)) src_mark[src] = 0;
        }
    }
}

// `bytes` (a multiple of 4) from src to dst by the whole workgroup
__device__ __forceinline__ void copy_run(char *dst, const char *src, size_t bytes) {
    if ((((uintptr_t)dst | (uintptr_t)src | bytes) & 15) == 0) {   // block-uniform
        const uint4 *s = (const uint4 *)src;
        uint4 *d = (uint4 *)dst;
        for (size_t i = threadIdx.x; i < bytes / 16; i += COPY_THREADS) d[i] = s[i];
    } else {
        const uint32_t *s = (const uint32_t *)src;
        uint32_t *d = (uint32_t *)dst;
        for (size_t i = threadIdx.x; i < bytes / 4; i += COPY_THREADS) d[i] = s[i];
    }
}

// table: n_small descriptors of small pieces (first_chunk ascending), then the large ones.
// LARGE = false: grid (row chunks of all small arrays, blocks over the pairs); true: grid (pairs, large arrays)
template <bool LARGE>
__global__ void __launch_bounds__(COPY_THREADS) copy_envs_kernel(const MwbCopyDesc *__restrict__ table, int n_small, const int2 *__restrict__ pairs, int count) {
    if (LARGE) {
        const int2 p = pairs[blockIdx.x];   // block-uniform
        if (p.x < 0) return;
        const MwbCopyDesc t = table[n_small + blockIdx.y];
        copy_run(t.dst + (size_t)p.x * t.elem, t.src + (size_t)p.y * t.elem, t.elem);
        return;
    }
    int k = 0;   // the array this workgroup's row chunk belongs to (a few dozen descriptors: a scalar scan)
    while (k + 1 < n_small && table[k + 1].first_chunk <= blockIdx.x) k++;
    const MwbCopyDesc t = table[k];
    const uint32_t r0 = (blockIdx.x - t.first_chunk) * MWB_COPY_ROW_CHUNK;
    const uint32_t r1 = r0 + MWB_COPY_ROW_CHUNK < t.rows ? r0 + MWB_COPY_ROW_CHUNK : t.rows;
    const bool wide = (t.elem & 7) == 0;   // every base is a hipMalloc pointer and every stride a multiple of elem: 8-byte aligned pieces
    for (size_t i = (size_t)blockIdx.y * COPY_THREADS + threadIdx.x; i < (size_t)count; i += (size_t)gridDim.y * COPY_THREADS) {
        const int2 p = pairs[i];
        if (p.x < 0) continue;
        for (uint32_t r = r0; r < r1; r++) {
            const char *s = t.src + r * t.src_stride + (size_t)p.y * t.elem;
            char *d = t.dst + r * t.dst_stride + (size_t)p.x * t.elem;
            if (wide) for (uint32_t b = 0; b < t.elem; b += 8) *(uint64_t *)(d + b) = *(const uint64_t *)(s + b);
            else for (uint32_t b = 0; b < t.elem; b += 4) *(uint32_t *)(d + b) = *(const uint32_t *)(s + b);
        }
    }
}

__global__ void __launch_bounds__(COPY_THREADS) copy_list_kernel(MwbDev d, const int2 *__restrict__ pairs, int count, int what) {
    if (what == 1 && blockIdx.x == 0 && threadIdx.x == 0) d.reset_count[0] = 0;   // the list has been rendered: consumed
    for (size_t i = (size_t)blockIdx.x * COPY_THREADS + threadIdx.x; i < (size_t)count; i += (size_t)gridDim.x * COPY_THREADS) {
        const int dst = pairs[i].x;
        if (dst < 0) continue;
        if (what == 0) {
            d.reset_set[dst] = 1;
            const int at = atomicAdd(d.reset_count, 1);   // every destination is named once (validated) and the list is empty between
            if (at < d.N) d.reset_list[at] = dst;         // passes: at most N entries
        } else if (what == 1) {
            d.reset_set[dst] = 0;   // left set, a later mwb_render would zero the env's fused-stack history
        } else if (d.frame_cached) {
            d.frame_cached[dst] = 0;
        }
    }
}

// one lane per (pair, segment group): after copy_envs_kernel the destination's n_segs and segs are its source's
__global__ void __launch_bounds__(COPY_THREADS) copy_seg_box_kernel(MwbDev d, const int2 *__restrict__ pairs, int count) {
    const size_t G = (size_t)mwb_seg_groups(d.S_max), N = (size_t)d.N;
    for (size_t i = (size_t)blockIdx.x * COPY_THREADS + threadIdx.x; i < (size_t)count * G; i += (size_t)gridDim.x * COPY_THREADS) {
        const int dst = pairs[i / G].x, g = (int)(i % G);
        if (dst < 0) continue;
        const int ns = d.n_segs[dst] < d.S_max ? d.n_segs[dst] : d.S_max, n = ns - g * MWB_SEG_GROUP < MWB_SEG_GROUP ? ns - g * MWB_SEG_GROUP : MWB_SEG_GROUP;
        if (n < 1) continue;   // no reader looks at a group past the env's segments
        double q[MWB_SEG_GROUP * 4];
#pragma unroll
        for (int k = 0; k < MWB_SEG_GROUP * 4; k++) q[k] = d.segs[((size_t)g * MWB_SEG_GROUP * 4 + (k < n * 4 ? k : 0)) * N + dst];
        const MwbSegBox b = mwb_seg_group_box(q, n);
        float *o = d.seg_box + (size_t)g * 4 * N + dst;
        o[0] = b.min_x; o[N] = b.min_z; o[2 * N] = b.max_x; o[3 * N] = b.max_z;
        if (d.seg_rows) {   // and the env-major twin of the group
            double *r = d.seg_rows + ((size_t)dst * d.S_max + (size_t)g * MWB_SEG_GROUP) * 4;
#pragma unroll
            for (int k = 0; k < MWB_SEG_GROUP * 4; k++) if (k < n * 4) r[k] = q[k];
        }
    }
}

#define COPY_STACK_RUN 32768   // bytes of one env's window a workgroup moves
__global__ void __launch_bounds__(COPY_THREADS) copy_stack_kernel(char *dst, size_t env_bytes_dst, size_t off_dst, const char *src,
                                                                  size_t env_bytes_src, size_t off_src, size_t window_bytes, const int2 *__restrict__ pairs) {
    const int2 p = pairs[blockIdx.x];   // block-uniform
    if (p.x < 0) return;
    const size_t b0 = (size_t)blockIdx.y * COPY_STACK_RUN, n = window_bytes - b0 < COPY_STACK_RUN ? window_bytes - b0 : COPY_STACK_RUN;
    copy_run(dst + (size_t)p.x * env_bytes_dst + off_dst + b0, src + (size_t)p.y * env_bytes_src + off_src + b0, n);
}

// ====================================================================================== launch
static inline unsigned pair_blocks(int count) {
    const long long b = ((long long)count + COPY_THREADS - 1) / COPY_THREADS;
    return (unsigned)(b < 1 ? 1 : b > 4096 ? 4096 : b);   // the kernels stride over longer lists
}

void mwb_launch_copy_validate(const int32_t *dst_idx, const int32_t *src_idx, int count, int n_dst, int n_src, int same_handle,
                              int32_t *dst_pairs, uint8_t *src_mark, int2 *pairs, unsigned long long *rejected, hipStream_t s) {
    for (int phase = 0; phase < 3; phase++)
        hipLaunchKernelGGL(copy_validate_kernel, dim3(pair_blocks(count)), dim3(COPY_THREADS), 0, s, phase, dst_idx, src_idx, count, n_dst, n_src,
                           same_handle, dst_pairs, src_mark, pairs, rejected);
}

void mwb_launch_copy_envs(const MwbCopyDesc *table, int n_small, int small_chunks, int n_large, const int2 *pairs, int count, hipStream_t s) {
    if (n_small > 0 && small_chunks > 0)
        hipLaunchKernelGGL(copy_envs_kernel<false>, dim3((unsigned)small_chunks, pair_blocks(count)), dim3(COPY_THREADS), 0, s, table, n_small, pairs, count);
    if (n_large > 0)
        hipLaunchKernelGGL(copy_envs_kernel<true>, dim3((unsigned)count, (unsigned)n_large), dim3(COPY_THREADS), 0, s, table, n_small, pairs, count);
}

void mwb_launch_copy_list(const MwbDev &d, const int2 *pairs, int count, int what, hipStream_t s) {
    hipLaunchKernelGGL(copy_list_kernel, dim3(pair_blocks(count)), dim3(COPY_THREADS), 0, s, d, pairs, count, what);
}

void mwb_launch_copy_seg_box(const MwbDev &d, const int2 *pairs, int count, hipStream_t s) {
    const long long b = ((long long)count * mwb_seg_groups(d.S_max) + COPY_THREADS - 1) / COPY_THREADS;
    hipLaunchKernelGGL(copy_seg_box_kernel, dim3((unsigned)(b < 1 ? 1 : b > 4096 ? 4096 : b)), dim3(COPY_THREADS), 0, s, d, pairs, count);
}

void mwb_launch_copy_stack(char *dst, size_t env_bytes_dst, size_t off_dst, const char *src, size_t env_bytes_src, size_t off_src,
                           size_t window_bytes, const int2 *pairs, int count, hipStream_t s) {
    const unsigned runs = (unsigned)((window_bytes + COPY_STACK_RUN - 1) / COPY_STACK_RUN);
    hipLaunchKernelGGL(copy_stack_kernel, dim3((unsigned)count, runs), dim3(COPY_THREADS), 0, s, dst, env_bytes_dst, off_dst, src, env_bytes_src,
                       off_src, window_bytes, pairs);
}
