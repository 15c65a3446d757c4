// mwb_rollout_learner.hip - the kernels of the rollout's learner half (mwb_rollout_learner_enable): the columns a trainer's
// RolloutStorage keeps beside the observations (actions, log-probs, value predictions, the sub-steps every transition took) and
// what it computes from them (pytorch-a2c-ppo-acktr/storage.py:57-61, 82-105, 124-128).  The arithmetic: mwb_returns_scan.h.
//
//   rollout_taken_kernel        one thread per env: the row of `taken` that belongs to the push just made (the repeat's taken
//                               buffer, or 1).  A launch of its own, so that rollout_push_kernel is what it was.
//   rollout_insert_kernel       one thread per env: the row copies of mwb_rollout_insert.
//   rollout_returns_kernel      one lane per env, 64-thread workgroups (8192 envs are 128 waves: one per workgroup spreads them
//                               over 128 CUs instead of stacking four to a CU).  The loop over t runs backwards and is sequential
//                               per lane - the contract is bit equality with the reference's loop, a parallel scan would
//                               re-associate the sums.  Every access is a coalesced [N] row.  The loads of a step (reward, value,
//                               mask, taken) do not depend on the chain: the loop handles RETURNS_UNROLL steps at a time and has
//                               the loads of the NEXT group in flight while it runs the seven dependent operations per step of
//                               this one.  The table rows G[k], L[k] are no memory access: lane i of the wave keeps G[i] and L[i]
//                               in a register and a step reads row k with a cross-lane read (k = 64 is a wave-uniform scalar) -
//                               so every lane of the wave stays active, a lane past N works on env N - 1 and stores nothing.
//   rollout_gather_cols_kernel  one lane per row of a minibatch: six gathers, coalesced stores; an index outside [0, T * N) is
//                               written as zeros and counted, no address is formed from it.
// No LDS is allocated, no scratch; every offset is 64-bit.
#include "mwb_internal.h"
#include "mwb_returns_scan.h"
#include "mwb_rollout_map.h"

#define LEARNER_THREADS 256
#define RETURNS_THREADS 64   // one wave: the cross-lane table read below spans the workgroup
#define RETURNS_UNROLL 4

__global__ void __launch_bounds__(LEARNER_THREADS) rollout_taken_kernel(int32_t *__restrict__ row, const int32_t *__restrict__ taken, int N) {
    const int e = blockIdx.x * LEARNER_THREADS + threadIdx.x;
    if (e >= N) return;
    row[e] = taken ? taken[e] : 1;
}

__global__ void __launch_bounds__(LEARNER_THREADS) rollout_insert_kernel(MwbLearner l, int N, int row, const int64_t *__restrict__ action,
                                                                        const int32_t *__restrict__ action_i32, const float *__restrict__ log_prob,
                                                                        const float *__restrict__ value) {
    const int e = blockIdx.x * LEARNER_THREADS + threadIdx.x;
    if (e >= N) return;
    const size_t at = (size_t)row * N + e;
    if (action) l.action[at] = action[e];
    if (action_i32) l.action[at] = (int64_t)action_i32[e];
    if (log_prob) l.log_prob[at] = log_prob[e];
    if (value) l.value[at] = value[e];
}

// what one step reads: none of it depends on the step after it
struct ScanStep {
    float r, v, m;   // reward[t], value[t] (PSI: the two components of feature[t]); mask[t + 1]
    int32_t k;       // taken[t]
};

template <int MODE>
__device__ __forceinline__ ScanStep scan_load(const MwbRollout &r, const MwbLearner &l, const float *__restrict__ reward, size_t N, size_t e, int t) {
    const size_t at = (size_t)t * N + e;
    ScanStep s;
    if (MODE == MWB_SCAN_PSI) {
        const float2 f = ((const float2 *)r.feature)[at];
        s.r = f.x; s.v = f.y;
    } else {
        s.r = reward[at]; s.v = l.value[at];
    }
    s.m = r.mask[at + N];
    s.k = l.taken[at];
    return s;
}

// c0, c1: what the chain carries from step t + 1 (GAE: gae, value[t + 1]; DISCOUNTED: ret[t + 1]; PSI: the two components)
template <int MODE>
__device__ __forceinline__ void scan_step(const MwbLearner &l, const ScanStep &s, float Gk, float Lk, size_t at, bool live, float &c0, float &c1) {
    if (MODE == MWB_SCAN_GAE) {
        const float ret = mwb_returns_gae_step(Gk, Lk, s.r, s.v, c1, s.m, &c0);
        c1 = s.v;
        if (live) { l.ret[at] = ret; l.adv[at] = mwb_returns_advantage(ret, s.v); }
    } else if (MODE == MWB_SCAN_DISCOUNTED) {
        c0 = mwb_returns_discounted_step(Gk, c0, s.m, s.r);
        if (live) { l.ret[at] = c0; l.adv[at] = mwb_returns_advantage(c0, s.v); }
    } else {
        c0 = mwb_returns_discounted_step(Gk, c0, s.m, s.r);
        c1 = mwb_returns_discounted_step(Gk, c1, s.m, s.v);
        if (live) ((float2 *)l.psi_ret)[at] = make_float2(c0, c1);
    }
}

// next: next_value [N] (GAE, DISCOUNTED) or next_psi [N][2] (PSI); reward: the stored rewards or the caller's [T][N]
template <int MODE>
__global__ void __launch_bounds__(RETURNS_THREADS) rollout_returns_kernel(MwbRollout r, MwbLearner l, MwbReturnsTables tab, const float *__restrict__ next,
                                                                         const float *__restrict__ reward) {
    const int lane = threadIdx.x;
    const size_t N = (size_t)r.N;
    const size_t e_raw = (size_t)blockIdx.x * RETURNS_THREADS + lane;
    const bool live = e_raw < N;
    const size_t e = live ? e_raw : N - 1;   // a lane past the end reads env N - 1 along and stores nothing: the wave stays whole
    const int T = r.T;
    // rows 0 .. 63 of the tables, one per lane; row 64 is the same scalar in every lane
    const float Glane = tab.G[lane], Llane = tab.L[lane];
    const float G64 = tab.G[MWB_RETURNS_MAX_K], L64 = tab.L[MWB_RETURNS_MAX_K];
    auto rowG = [&](int32_t taken) { const int k = mwb_returns_k(taken); const float g = __shfl(Glane, k & 63); return k == MWB_RETURNS_MAX_K ? G64 : g; };
    auto rowL = [&](int32_t taken) { const int k = mwb_returns_k(taken); const float g = __shfl(Llane, k & 63); return k == MWB_RETURNS_MAX_K ? L64 : g; };

    float c0, c1;
    const size_t top = (size_t)T * N + e;
    if (MODE == MWB_SCAN_PSI) {
        const float2 np = ((const float2 *)next)[e];
        c0 = np.x; c1 = np.y;
        if (live) ((float2 *)l.psi_ret)[top] = np;
    } else {
        const float nv = next[e];
        c0 = MODE == MWB_SCAN_GAE ? 0.0f : nv;
        c1 = nv;
        if (live) { l.value[top] = nv; l.ret[top] = nv; }
    }

    int t = T - 1;
    // the steps that do not fill a group, one at a time
    for (; (t + 1) % RETURNS_UNROLL != 0; t--) {
        const ScanStep s = scan_load<MODE>(r, l, reward, N, e, t);
        scan_step<MODE>(l, s, rowG(s.k), MODE == MWB_SCAN_GAE ? rowL(s.k) : 0.0f, (size_t)t * N + e, live, c0, c1);
    }
    if (t < 0) return;
    // groups of four steps t .. t - 3 in named registers: the next group's loads are issued before this group's chain runs
    static_assert(RETURNS_UNROLL == 4, "four named registers per group below");
    ScanStep a0 = scan_load<MODE>(r, l, reward, N, e, t), a1 = scan_load<MODE>(r, l, reward, N, e, t - 1);
    ScanStep a2 = scan_load<MODE>(r, l, reward, N, e, t - 2), a3 = scan_load<MODE>(r, l, reward, N, e, t - 3);
    for (; t >= 0; t -= RETURNS_UNROLL) {
        ScanStep b0 = a0, b1 = a1, b2 = a2, b3 = a3;
        if (t >= RETURNS_UNROLL) {   // wave-uniform
            b0 = scan_load<MODE>(r, l, reward, N, e, t - 4); b1 = scan_load<MODE>(r, l, reward, N, e, t - 5);
            b2 = scan_load<MODE>(r, l, reward, N, e, t - 6); b3 = scan_load<MODE>(r, l, reward, N, e, t - 7);
        }
        const float g0 = rowG(a0.k), g1 = rowG(a1.k), g2 = rowG(a2.k), g3 = rowG(a3.k);
        float l0 = 0.0f, l1 = 0.0f, l2 = 0.0f, l3 = 0.0f;
        if (MODE == MWB_SCAN_GAE) { l0 = rowL(a0.k); l1 = rowL(a1.k); l2 = rowL(a2.k); l3 = rowL(a3.k); }
        const size_t at = (size_t)t * N + e;
        scan_step<MODE>(l, a0, g0, l0, at, live, c0, c1);
        scan_step<MODE>(l, a1, g1, l1, at - N, live, c0, c1);
        scan_step<MODE>(l, a2, g2, l2, at - 2 * N, live, c0, c1);
        scan_step<MODE>(l, a3, g3, l3, at - 3 * N, live, c0, c1);
        a0 = b0; a1 = b1; a2 = b2; a3 = b3;
    }
}

// out_f32: [5][count] = return, value, old log-prob, advantage, mask of the rows; the indices are those of the [:-1] views
__global__ void __launch_bounds__(LEARNER_THREADS) rollout_gather_cols_kernel(MwbRollout r, MwbLearner l, const int64_t *__restrict__ index,
                                                                             const float *__restrict__ adv_src, float *__restrict__ out_f32,
                                                                             int64_t *__restrict__ out_action, uint32_t count) {
    const uint32_t row = blockIdx.x * LEARNER_THREADS + threadIdx.x;
    if (row >= count) return;
    const int64_t idx = index[row];
    float ret = 0.0f, value = 0.0f, log_prob = 0.0f, adv = 0.0f, mask = 0.0f;
    int64_t action = 0;
    if (mwb_rollout_index_ok(idx, r.T - 1, r.N)) {   // [0, T * N)
        const size_t at = (size_t)idx;
        ret = l.ret[at]; value = l.value[at]; log_prob = l.log_prob[at]; adv = adv_src[at]; mask = r.mask[at];
        action = l.action[at];
    } else {
        atomicAdd(r.rejected, 1ull);   // (the compiler folds a wave's adds into one)
    }
    const size_t n = count;
    out_f32[row] = ret; out_f32[n + row] = value; out_f32[2 * n + row] = log_prob; out_f32[3 * n + row] = adv; out_f32[4 * n + row] = mask;
    out_action[row] = action;
}

// ====================================================================================== launch
static inline unsigned env_blocks(int N, int threads) { return (unsigned)(((size_t)N + threads - 1) / threads); }

void mwb_launch_rollout_taken(const MwbRollout &r, const MwbLearner &l, int t, const int32_t *taken, hipStream_t s) {
    hipLaunchKernelGGL(rollout_taken_kernel, dim3(env_blocks(r.N, LEARNER_THREADS)), dim3(LEARNER_THREADS), 0, s, l.taken + (size_t)(t - 1) * r.N, taken, r.N);
}

void mwb_launch_rollout_insert(const MwbRollout &r, const MwbLearner &l, int row, const int64_t *action, const int32_t *action_i32,
                               const float *log_prob, const float *value, hipStream_t s) {
    hipLaunchKernelGGL(rollout_insert_kernel, dim3(env_blocks(r.N, LEARNER_THREADS)), dim3(LEARNER_THREADS), 0, s, l, r.N, row, action, action_i32, log_prob, value);
}

void mwb_launch_rollout_returns(const MwbRollout &r, const MwbLearner &l, int mode, const MwbReturnsTables &tab, const float *next,
                                const float *reward, hipStream_t s) {
    const dim3 grid(env_blocks(r.N, RETURNS_THREADS)), block(RETURNS_THREADS);
    if (mode == MWB_SCAN_GAE) hipLaunchKernelGGL((rollout_returns_kernel<MWB_SCAN_GAE>), grid, block, 0, s, r, l, tab, next, reward);
    else if (mode == MWB_SCAN_DISCOUNTED) hipLaunchKernelGGL((rollout_returns_kernel<MWB_SCAN_DISCOUNTED>), grid, block, 0, s, r, l, tab, next, reward);
    else hipLaunchKernelGGL((rollout_returns_kernel<MWB_SCAN_PSI>), grid, block, 0, s, r, l, tab, next, reward);
}

// count > 0
void mwb_launch_rollout_gather_cols(const MwbRollout &r, const MwbLearner &l, const int64_t *index, int count, const float *adv_src,
                                    float *out_f32, int64_t *out_action, hipStream_t s) {
    hipLaunchKernelGGL(rollout_gather_cols_kernel, dim3(env_blocks(count, LEARNER_THREADS)), dim3(LEARNER_THREADS), 0, s, r, l, index, adv_src, out_f32,
                       out_action, (uint32_t)count);
}
