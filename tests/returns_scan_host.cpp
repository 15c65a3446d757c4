// Host program around gym_miniworld_amd/csrc/mwb_returns_scan.h (tests/test_returns_host.py builds and runs it): the backward
// scans of mwb_rollout_returns, one env after the other, with the header's tables and step functions - the kernel's arithmetic
// without the kernel.
//
// stdin (binary, native endianness):  int32 mode, T, N; float64 gamma, tau; then float32 reward [T][N], value [T+1][N],
//                                     mask [T+1][N]; int32 taken [T][N]; float32 feature [T+1][N][2], next [N][2] (next_value in
//                                     the first N entries for the GAE and discounted modes)
// stdout (binary):                    float32 ret [T+1][N], adv [T][N], value [T+1][N], psi_ret [T+1][N][2], G [65], L [65]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mwb_returns_scan.h"

template <typename V>
static void get(std::vector<V> &v, size_t n) {
    v.resize(n);
    if (n && fread(v.data(), sizeof(V), n, stdin) != n) { fprintf(stderr, "short input\n"); exit(2); }
}
template <typename V>
static void put(const V *p, size_t n) {
    if (n && fwrite(p, sizeof(V), n, stdout) != n) { fprintf(stderr, "short output\n"); exit(3); }
}

int main() {
    std::vector<int32_t> head;
    std::vector<double> disc;
    get(head, 3); get(disc, 2);
    const int mode = head[0], T = head[1], N = head[2];
    if (T < 1 || N < 1 || mode < 0 || mode > 2) { fprintf(stderr, "bad header\n"); return 2; }
    const size_t n = (size_t)N, tn = (size_t)T * n, t1n = tn + n;
    std::vector<float> reward, value, mask, feature, next;
    std::vector<int32_t> taken;
    get(reward, tn); get(value, t1n); get(mask, t1n); get(taken, tn); get(feature, 2 * t1n); get(next, 2 * n);
    std::vector<float> ret(t1n, 0.0f), adv(tn, 0.0f), psi(2 * t1n, 0.0f);
    MwbReturnsTables tab;
    mwb_returns_tables(disc[0], disc[1], &tab);
    for (size_t e = 0; e < n; e++) {
        const size_t top = tn + e;
        float c0, c1;
        if (mode == MWB_SCAN_PSI) {
            c0 = psi[2 * top] = next[2 * e]; c1 = psi[2 * top + 1] = next[2 * e + 1];
        } else {
            value[top] = ret[top] = next[e];
            c0 = mode == MWB_SCAN_GAE ? 0.0f : next[e];
            c1 = next[e];
        }
        for (int t = T - 1; t >= 0; t--) {
            const size_t at = (size_t)t * n + e;
            const int k = mwb_returns_k(taken[at]);
            if (mode == MWB_SCAN_GAE) {
                ret[at] = mwb_returns_gae_step(tab.G[k], tab.L[k], reward[at], value[at], c1, mask[at + n], &c0);
                c1 = value[at];
                adv[at] = mwb_returns_advantage(ret[at], value[at]);
            } else if (mode == MWB_SCAN_DISCOUNTED) {
                ret[at] = c0 = mwb_returns_discounted_step(tab.G[k], c0, mask[at + n], reward[at]);
                adv[at] = mwb_returns_advantage(ret[at], value[at]);
            } else {
                psi[2 * at] = c0 = mwb_returns_discounted_step(tab.G[k], c0, mask[at + n], feature[2 * at]);
                psi[2 * at + 1] = c1 = mwb_returns_discounted_step(tab.G[k], c1, mask[at + n], feature[2 * at + 1]);
            }
        }
    }
    put(ret.data(), t1n); put(adv.data(), tn); put(value.data(), t1n); put(psi.data(), 2 * t1n);
    put(tab.G, MWB_RETURNS_MAX_K + 1); put(tab.L, MWB_RETURNS_MAX_K + 1);
    return 0;
}
