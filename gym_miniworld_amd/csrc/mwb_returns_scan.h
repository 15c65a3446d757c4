// mwb_returns_scan.h - the arithmetic of mwb_rollout_returns: the discount tables and the per-step recurrences of the three
// backward loops of RolloutStorage (pytorch-a2c-ppo-acktr/storage.py:82-105), extended by the sub-steps a transition took.
//
// Plain C++ without any HIP type, so that the same functions run in the kernel (mwb_rollout_learner.hip), in the host API (the
// tables) and in a host program (tests/test_returns_host.py builds one around this header).
//
// The contract is bit equality with torch's eager float32 arithmetic in the reference's operation order: every line below is ONE
// float32 operation, rounded to nearest, and the translation units that include this header are built with -ffp-contract=off (no
// fused multiply-add may join two lines).  Python hands torch gamma and gamma * tau as float64 scalars, which torch rounds to
// float32 once before it multiplies a float32 tensor by them: that is G[1] and L[1].  A transition that took k sub-steps is
// discounted by gamma^k: G[k] = (float)(gamma^k), the power formed in float64 by repeated multiplication (no pow: the table must
// be the same on every host), and L[k] likewise from the one float64 product gamma * tau.  k = 0 (a skipped env, a pass that is
// not a step) discounts by exactly 1.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MWB_RETURNS_HD __host__ __device__
#else
#define MWB_RETURNS_HD
#endif

#define MWB_RETURNS_MAX_K 64   // = MWB_MAX_REPEAT (mwb_api.hip asserts it)

// the `mode` of mwb_rollout_returns (include/miniworld_batch.h: MWB_RETURNS_*)
enum { MWB_SCAN_DISCOUNTED = 0, MWB_SCAN_GAE = 1, MWB_SCAN_PSI = 2 };

struct MwbReturnsTables {
    float G[MWB_RETURNS_MAX_K + 1];   // (float)(gamma^k)
    float L[MWB_RETURNS_MAX_K + 1];   // (float)((gamma * tau)^k)
};

// host: Gd[0] = 1, Gd[k] = Gd[k-1] * gamma in float64, G[k] = (float)Gd[k]; L from the single float64 product gamma * tau
static inline void mwb_returns_tables(double gamma, double tau, MwbReturnsTables *out) {
    const double gl = gamma * tau;
    double gd = 1.0, ld = 1.0;
    for (int k = 0; k <= MWB_RETURNS_MAX_K; k++) {
        out->G[k] = (float)gd;
        out->L[k] = (float)ld;
        gd = gd * gamma;
        ld = ld * gl;
    }
}

// taken[t][e] -> the table row: clamped to 0 .. MWB_RETURNS_MAX_K, no address is formed from anything else
MWB_RETURNS_HD static inline int mwb_returns_k(int32_t taken) { return taken < 0 ? 0 : (taken > MWB_RETURNS_MAX_K ? MWB_RETURNS_MAX_K : taken); }

// storage.py:87-89 - delta = rewards[t] + gamma * value_preds[t+1] * masks[t+1] - value_preds[t];
//                    gae = delta + gamma * tau * masks[t+1] * gae;  returns[t] = gae + value_preds[t]
// Gk, Lk: the table rows of the transition's k.  *gae: carried from step t + 1 (+0.0f at t = T - 1).  Returns returns[t].
MWB_RETURNS_HD static inline float mwb_returns_gae_step(float Gk, float Lk, float reward_t, float value_t, float value_t1, float mask_t1, float *gae) {
    float a = Gk * value_t1;
    a = a * mask_t1;
    float d = reward_t + a;
    d = d - value_t;
    float b = Lk * mask_t1;
    b = b * *gae;
    *gae = d + b;
    return *gae + value_t;
}

// storage.py:98-99 (and 94-95 with the estimated rewards, 104-105 per feature component):
//                    returns[t] = returns[t+1] * gamma * masks[t+1] + rewards[t]
MWB_RETURNS_HD static inline float mwb_returns_discounted_step(float Gk, float ret_t1, float mask_t1, float reward_t) {
    float a = ret_t1 * Gk;
    a = a * mask_t1;
    return a + reward_t;
}

// ppo.py:33 - advantages = returns[:-1] - value_preds[:-1]
MWB_RETURNS_HD static inline float mwb_returns_advantage(float ret_t, float value_t) { return ret_t - value_t; }
