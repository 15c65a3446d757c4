// mwb_monitor.hip - the kernels of the episode monitor (mwb_monitor_update / mwb_monitor_clear / mwb_monitor_quota): what the
// trainer's loop over the envs after every step keeps (pytorch-a2c-ppo-acktr/main.py:167-169) - per-env running returns and
// lengths, the log of the last `capacity` episodes, the per-env evaluation table.  Where a record of the log lives:
// mwb_monitor_map.h.
//
// One update is three launches; no workgroup ever waits for another (no flags, no look-back: the launches are the barriers):
//   monitor_accumulate_kernel   one lane per env, every access a coalesced [N] row.  Adds the step to the running episode; an env
//                               that is done writes last_*, its cell of the table and bumps finished (or counts as dropped when
//                               its episode's start was not seen); then retired.  The wave's loggable finishing lanes are a ballot:
//                               lane 0 stores it, with the wave's dropped / not-retired counts beside it.
//   monitor_scan_kernel         ONE workgroup: exclusive sum of the ballots' population counts over the waves, SCAN_THREADS waves
//                               per turn of a loop (70 001 envs are 1094 waves), carried from turn to turn; then the counters:
//                               the slot of rank 0 and the count c of this pass for the next launch, total += c, dropped,
//                               remaining.  LDS: the wave totals of the scan and of the two small sums, 48 bytes.
//   monitor_log_kernel          one lane per env: a lane whose bit is set in its wave's ballot has rank = the wave's base + the
//                               ballot bits below it, and stores its record (from last_*) in the slot of that rank, unless the
//                               pass finished more episodes than the ring holds and the rank is not among the last `capacity`.
//   monitor_clear_kernel, monitor_quota_kernel   one lane per env.
// No scratch; plain vector stores only; every offset into the table is size_t.
#include "mwb_internal.h"
#include "mwb_monitor_map.h"

#define MONITOR_THREADS 256   // a multiple of the wave: global wave index = env >> 6
#define SCAN_THREADS 256
#define MON_WAVE 64

static_assert(MONITOR_THREADS % MON_WAVE == 0 && SCAN_THREADS % MON_WAVE == 0, "whole waves");

__global__ void __launch_bounds__(MONITOR_THREADS) monitor_accumulate_kernel(MwbMonitor m, const uint8_t *__restrict__ skip, const double *__restrict__ reward,
                                                                            const uint8_t *__restrict__ done, const int32_t *__restrict__ taken) {
    const size_t e = (size_t)blockIdx.x * MONITOR_THREADS + threadIdx.x;
    const bool in = e < (size_t)m.N;   // (no early return: every lane of the wave takes part in the ballots)
    const bool live = in && !(skip && skip[e] != 0);
    bool loggable = false, dropped = false;
    int32_t fin = in ? m.finished[e] : 0;
    if (live) {
        double ret = m.run_return[e] + reward[e];   // one float64 add per step, from 0.0: the order Python's sum takes
        int32_t len = m.run_len[e] + (taken ? taken[e] : 1);
        int32_t calls = m.run_calls[e] + 1;
        if (done[e] != 0) {
            if (m.partial[e] != 0) {   // the start of this episode was not seen (mwb_monitor_clear with partial): not logged
                dropped = true;
                m.partial[e] = 0;
            } else {
                loggable = true;
                m.last_return[e] = ret; m.last_len[e] = len; m.last_calls[e] = calls;
                if (fin < m.Q) {
                    const size_t cell = (size_t)fin * (size_t)m.N + e;
                    m.tab_return[cell] = ret; m.tab_len[cell] = len;
                }
                m.finished[e] = ++fin;
            }
            ret = 0.0; len = 0; calls = 0;
        }
        m.run_return[e] = ret; m.run_len[e] = len; m.run_calls[e] = calls;
    }
    const uint32_t quota = m.counts32[MWB_MON_QUOTA];
    const bool retired = in && quota > 0 && (uint32_t)fin >= quota;
    if (in) { m.retired[e] = retired ? 1 : 0; m.logged[e] = loggable ? 1 : 0; }
    const unsigned long long b_log = __ballot(loggable), b_drop = __ballot(dropped), b_stay = __ballot(in && !retired);
    if ((threadIdx.x & (MON_WAVE - 1)) == 0) {   // the wave's first env is always inside: grids cover ceil(N / 64) waves exactly ...
        const size_t w = e / MON_WAVE;
        if (w < (size_t)m.n_waves) {         // ... up to the last workgroup's tail
            m.wave_ballot[w] = b_log;
            m.wave_aux[w] = (uint32_t)__popcll(b_drop) | ((uint32_t)__popcll(b_stay) << 8);
        }
    }
}

__global__ void __launch_bounds__(SCAN_THREADS) monitor_scan_kernel(MwbMonitor m) {
    __shared__ uint32_t wave_total[SCAN_THREADS / MON_WAVE];
    const uint32_t lane = threadIdx.x & (MON_WAVE - 1), wave = threadIdx.x / MON_WAVE;
    uint32_t carry = 0, drop = 0, stay = 0;   // carry: loggable episodes in the waves of earlier turns (the same in every thread)
    for (uint32_t w0 = 0; w0 < (uint32_t)m.n_waves; w0 += SCAN_THREADS) {
        const uint32_t w = w0 + threadIdx.x;
        const bool in = w < (uint32_t)m.n_waves;
        const uint32_t cnt = in ? (uint32_t)__popcll(m.wave_ballot[w]) : 0u;
        if (in) { const uint32_t a = m.wave_aux[w]; drop += a & 255u; stay += a >> 8; }
        uint32_t inc = cnt;   // inclusive sum inside the wave
        for (uint32_t ofs = 1; ofs < MON_WAVE; ofs <<= 1) { const uint32_t v = __shfl_up(inc, ofs); if (lane >= ofs) inc += v; }
        if (lane == MON_WAVE - 1) wave_total[wave] = inc;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t k = 0; k < SCAN_THREADS / MON_WAVE; k++) { const uint32_t t = wave_total[k]; if (k < wave) before += t; all += t; }
        if (in) m.wave_base[w] = carry + before + inc - cnt;
        carry += all;
        __syncthreads();   // wave_total is rewritten by the next turn
    }
    // the two small sums: inside the wave, then over the waves
    for (uint32_t ofs = MON_WAVE / 2; ofs > 0; ofs >>= 1) { drop += __shfl_down(drop, ofs); stay += __shfl_down(stay, ofs); }
    __shared__ uint32_t part[2][SCAN_THREADS / MON_WAVE];
    if (lane == 0) { part[0][wave] = drop; part[1][wave] = stay; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t d = 0, s = 0;
#pragma unroll
        for (uint32_t k = 0; k < SCAN_THREADS / MON_WAVE; k++) { d += part[0][k]; s += part[1][k]; }
        const unsigned long long total = m.counts64[MWB_MON_TOTAL];
        m.counts32[MWB_MON_BASE] = mwb_monitor_base(total, (uint32_t)m.capacity);
        m.counts32[MWB_MON_COUNT] = carry;
        m.counts64[MWB_MON_TOTAL] = total + carry;
        m.counts64[MWB_MON_DROPPED] += d;
        m.counts32[MWB_MON_REMAINING] = s;
    }
}

__global__ void __launch_bounds__(MONITOR_THREADS) monitor_log_kernel(MwbMonitor m) {
    const size_t e = (size_t)blockIdx.x * MONITOR_THREADS + threadIdx.x;
    if (e >= (size_t)m.N) return;
    const uint32_t lane = threadIdx.x & (MON_WAVE - 1);
    const size_t w = e / MON_WAVE;
    const unsigned long long ballot = m.wave_ballot[w];
    if (!((ballot >> lane) & 1ull)) return;
    const uint32_t rank = m.wave_base[w] + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
    const uint32_t cap = (uint32_t)m.capacity;
    if (!mwb_monitor_written(rank, m.counts32[MWB_MON_COUNT], cap)) return;
    const uint32_t slot = mwb_monitor_slot_from(m.counts32[MWB_MON_BASE], rank, cap);   // < capacity
    m.log_return[slot] = m.last_return[e]; m.log_len[slot] = m.last_len[e]; m.log_calls[slot] = m.last_calls[e];
    m.log_env[slot] = (int32_t)e;
}

__global__ void __launch_bounds__(MONITOR_THREADS) monitor_clear_kernel(MwbMonitor m, const uint8_t *__restrict__ mask, int partial) {
    const size_t e = (size_t)blockIdx.x * MONITOR_THREADS + threadIdx.x;
    if (e >= (size_t)m.N || (mask && mask[e] == 0)) return;
    m.run_return[e] = 0.0; m.run_len[e] = 0; m.run_calls[e] = 0;
    m.partial[e] = partial ? 1 : 0;
}

__global__ void __launch_bounds__(MONITOR_THREADS) monitor_quota_kernel(MwbMonitor m, int quota) {
    const size_t e = (size_t)blockIdx.x * MONITOR_THREADS + threadIdx.x;
    if (e >= (size_t)m.N) return;
    m.finished[e] = 0; m.retired[e] = 0;
    for (int j = 0; j < m.Q; j++) {   // unwritten cells: NaN / -1
        const size_t cell = (size_t)j * (size_t)m.N + e;
        m.tab_return[cell] = __longlong_as_double(0x7ff8000000000000LL); m.tab_len[cell] = -1;
    }
    if (e == 0) { m.counts32[MWB_MON_QUOTA] = (uint32_t)quota; m.counts32[MWB_MON_REMAINING] = (uint32_t)m.N; }
}

// ====================================================================================== launch
static inline unsigned env_blocks(int N) { return (unsigned)(((size_t)N + MONITOR_THREADS - 1) / MONITOR_THREADS); }

void mwb_launch_monitor_update(const MwbMonitor &m, const uint8_t *skip, const double *reward, const uint8_t *done, const int32_t *taken, hipStream_t s) {
    hipLaunchKernelGGL(monitor_accumulate_kernel, dim3(env_blocks(m.N)), dim3(MONITOR_THREADS), 0, s, m, skip, reward, done, taken);
    hipLaunchKernelGGL(monitor_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, m);
    hipLaunchKernelGGL(monitor_log_kernel, dim3(env_blocks(m.N)), dim3(MONITOR_THREADS), 0, s, m);
}

void mwb_launch_monitor_clear(const MwbMonitor &m, const uint8_t *mask, int partial, hipStream_t s) {
    hipLaunchKernelGGL(monitor_clear_kernel, dim3(env_blocks(m.N)), dim3(MONITOR_THREADS), 0, s, m, mask, partial);
}

void mwb_launch_monitor_quota(const MwbMonitor &m, int quota, hipStream_t s) {
    hipLaunchKernelGGL(monitor_quota_kernel, dim3(env_blocks(m.N)), dim3(MONITOR_THREADS), 0, s, m, quota);
}
