// mwb_levels.hip - the kernels of level sets (mwb_levels_enable): before an env is regenerated it gets the generator stream of a
// chosen level seed, on the device, in the pass that regenerates it.  A level is Procgen's (`num_levels` / `start_level`); the
// episode that follows equals the first episode of a reference env after `env.seed(level_seed); env.reset()`.  Which level, which
// seed, the SHA-512 and the MT19937 init_by_array behind it: mwb_levels_map.h - the same functions mwb_seed runs on the host.
//
//   levels_assign_kernel   the hot path.  One lane per env of the regenerated-env list; wave w takes list entries 64 w .. 64 w + 63
//                          and grid-strides over reset_count[0] as reset_kernel does.  Per lane: tally the level the env leaves
//                          (step passes only), choose the next one, the bookkeeping, one SHA-512 block, then the 624 + 623
//                          dependent steps of init_by_array - a serial chain of about five integer operations each, kept in
//                          registers; the only parallelism is the envs.  The constant table's word i is the same address for
//                          every lane (a uniform load), each new word is stored straight to the env's row, and the third loop
//                          reads the lane's own row MWB_LEVELS_AHEAD words ahead of the chain.  No LDS, no scratch.  Runs beside
//                          the bulk render on the side stream, ahead of reset_kernel: the same raised wave priority.
//   levels_restart_kernel  episode_no = 0, optionally the tallies = 0, mode and sampler seed (device memory).
//   levels_copy_kernel     index of the validated pairs of a mwb_copy_envs.
#include "mwb_internal.h"
#include "mwb_levels_map.h"

#define LEVELS_THREADS 256
#define LEVELS_MAX_BLOCKS 1024   // waves of levels_assign_kernel, as mwb_launch_reset's blocks in a step; more envs are grid-strided

struct LevelsDevRow {
    uint32_t *__restrict__ mt;
    __device__ __forceinline__ uint32_t get(int i) const { return mt[i]; }
    __device__ __forceinline__ void set(int i, uint32_t v) { mt[i] = v; }
};

__global__ void __launch_bounds__(64) levels_assign_kernel(MwbLevels v, const uint32_t *__restrict__ base, const int32_t *__restrict__ reset_list, const int32_t *__restrict__ reset_count,
                                                           uint32_t *__restrict__ rng, const uint8_t *__restrict__ done,
                                                           const double *__restrict__ reward64, const int32_t *__restrict__ ep_steps, int tally) {
    __builtin_amdgcn_s_setprio(3);   // a latency-bound wave beside the bulk render (see reset_kernel)
    const int count = reset_count[0] < v.N ? reset_count[0] : v.N;
    const int mode = (int)v.params[0];
    const uint64_t sampler_seed = v.params[1];
    const uint64_t L = (uint64_t)v.L;
    for (int li = blockIdx.x * 64 + threadIdx.x; li < count; li += gridDim.x * 64) {
        const int e = reset_list[li];
        if ((unsigned)e >= (unsigned)v.N) continue;   // (the list holds env indices; nothing is addressed from anything else)
        const int32_t old = v.index[e];
        // the level the env leaves: only an episode a step ended counts, and only where its level is known
        if (tally && v.tallies && done[e] && old >= 0 && (uint64_t)old < L) {
            // (the plane offsets are formed per lane: as wave-uniform addresses they are hoisted out of the loop and, held in
            // scalar registers across the SHA-512 rounds, spill)
            uint64_t plane = L;
            asm volatile("" : "+v"(plane));
            atomicAdd(&v.tallies[old], 1ull);
            atomicAdd(&v.tallies[plane + old], (unsigned long long)ep_steps[e]);
            if (reward64[e] > 0.0) atomicAdd(&v.tallies[2 * plane + old], 1ull);
        }
        const int64_t n = v.episode_no[e];
        const int32_t request = mode == MWB_LEVELS_MODE_TABLE ? v.next_level[e] : -1;
        int rejected;
        const int32_t i = mwb_levels_choose(mode, (uint64_t)(v.env_offset + e), (uint64_t)n, L, (uint64_t)v.env_stride, sampler_seed, request, &rejected);
        if (rejected) atomicAdd(v.rejected, 1ull);
        if (mode == MWB_LEVELS_MODE_TABLE) v.next_level[e] = -1;   // consumed either way
        v.prev_index[e] = old; v.index[e] = i; v.episode_no[e] = n + 1;
        uint32_t key[2];
        const int key_length = mwb_levels_seed_key(mwb_levels_seed_of(i, v.start_level, v.seeds), key);
        LevelsDevRow row = {rng + (size_t)e * MWB_MT_WORDS};
        mwb_levels_init_by_array(row, base, key[0], key[1], key_length);
    }
}

__global__ void __launch_bounds__(LEVELS_THREADS) levels_restart_kernel(MwbLevels v, int mode, uint64_t sampler_seed, int clear_tally) {
    const size_t first = (size_t)blockIdx.x * LEVELS_THREADS + threadIdx.x, step = (size_t)gridDim.x * LEVELS_THREADS;
    if (first == 0) { v.params[0] = (uint64_t)mode; v.params[1] = sampler_seed; }
    for (size_t e = first; e < (size_t)v.N; e += step) v.episode_no[e] = 0;
    if (clear_tally && v.tallies)
        for (size_t k = first; k < 3 * (size_t)v.L; k += step) v.tallies[k] = 0;
}

__global__ void __launch_bounds__(LEVELS_THREADS) levels_copy_kernel(int32_t *__restrict__ dst_index, const int32_t *src_index, const int2 *__restrict__ pairs,
                                                                     int count) {
    const int k = blockIdx.x * LEVELS_THREADS + threadIdx.x;
    if (k >= count) return;
    const int2 p = pairs[k];   // validated by copy_validate_kernel: .x = -1 where the pair was not carried out
    if (p.x < 0) return;
    dst_index[p.x] = src_index ? src_index[p.y] : -1;
}

void mwb_launch_levels_assign(const MwbLevels &v, const int32_t *reset_list, const int32_t *reset_count, uint32_t *rng, const uint8_t *done,
                              const double *reward64, const int32_t *ep_steps, int tally, hipStream_t s) {
    const int waves = (v.N + 63) / 64;
    hipLaunchKernelGGL(levels_assign_kernel, dim3(waves < LEVELS_MAX_BLOCKS ? waves : LEVELS_MAX_BLOCKS), dim3(64), 0, s, v, v.base, reset_list, reset_count, rng,
                       done, reward64, ep_steps, tally);
}

void mwb_launch_levels_restart(const MwbLevels &v, int mode, uint64_t sampler_seed, int clear_tally, hipStream_t s) {
    size_t items = (size_t)v.N;
    if (clear_tally && v.tallies && 3 * (size_t)v.L > items) items = 3 * (size_t)v.L;
    size_t blocks = (items + LEVELS_THREADS - 1) / LEVELS_THREADS;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(levels_restart_kernel, dim3((unsigned)blocks), dim3(LEVELS_THREADS), 0, s, v, mode, sampler_seed, clear_tally);
}

void mwb_launch_levels_copy(int32_t *dst_index, const int32_t *src_index, const int2 *pairs, int count, hipStream_t s) {
    hipLaunchKernelGGL(levels_copy_kernel, dim3((count + LEVELS_THREADS - 1) / LEVELS_THREADS), dim3(LEVELS_THREADS), 0, s, dst_index, src_index, pairs, count);
}
