"""NumPy float32 restatement of the rollout's returns scan (mwb_rollout_returns): test infrastructure, like stack_ref.py.

Written from the rules the scan is specified by, one float32 operation per line (NumPy rounds every float32 operation to nearest,
once: there is no fused multiply-add in it):

  tables   Gd[0] = 1, Gd[k] = Gd[k-1] * gamma in float64, G[k] = float32(Gd[k]); L[k] the same from the single float64 product
           gamma * tau; k = 0 .. 64.  A transition that took k sub-steps uses row k, k clamped to 0 .. 64.
  GAE      value[T] = ret[T] = next_value, gae = +0; for t = T-1 .. 0:
           a = G[k] * value[t+1]; a = a * mask[t+1]; d = reward[t] + a; d = d - value[t];
           b = L[k] * mask[t+1]; b = b * gae; gae = d + b; ret[t] = gae + value[t]
  plain    value[T] = ret[T] = next_value; ret[t] = ((ret[t+1] * G[k]) * mask[t+1]) + reward[t]
  psi      psi[T] = next_psi; psi[t] = ((psi[t+1] * G[k]) * mask[t+1]) + feature[t], per component
  adv      adv[t] = ret[t] - value[t] (GAE and plain)

Arrays are time-major: reward, taken [T, N]; value, mask [T+1, N]; feature [T+1, N, 2]."""
import numpy as np

MAX_K = 64
F = np.float32


def tables(gamma, tau):
    """-> (G, L), float32 [65]"""
    gamma, gl = float(gamma), float(gamma) * float(tau)
    G, L = np.empty(MAX_K + 1, F), np.empty(MAX_K + 1, F)
    gd = ld = 1.0
    for k in range(MAX_K + 1):
        G[k], L[k] = F(gd), F(ld)
        gd, ld = gd * gamma, ld * gl
    return G, L


def _rows(table, taken_t):
    return table[np.clip(taken_t, 0, MAX_K)]


def gae(reward, value, mask, taken, next_value, gamma, tau):
    """-> (ret [T+1, N], adv [T, N], value [T+1, N] with row T = next_value)"""
    G, L = tables(gamma, tau)
    T = reward.shape[0]
    value = value.astype(F).copy()
    value[T] = next_value
    ret, adv = np.zeros_like(value), np.zeros_like(reward, dtype=F)
    ret[T] = next_value
    acc = np.zeros(reward.shape[1], F)
    for t in range(T - 1, -1, -1):
        a = _rows(G, taken[t]) * value[t + 1]
        a = a * mask[t + 1]
        d = reward[t] + a
        d = d - value[t]
        b = _rows(L, taken[t]) * mask[t + 1]
        b = b * acc
        acc = d + b
        ret[t] = acc + value[t]
        adv[t] = ret[t] - value[t]
    return ret, adv, value


def discounted(reward, value, mask, taken, next_value, gamma):
    """-> (ret, adv, value) as gae()"""
    G, _ = tables(gamma, 1.0)
    T = reward.shape[0]
    value = value.astype(F).copy()
    value[T] = next_value
    ret, adv = np.zeros_like(value), np.zeros_like(reward, dtype=F)
    ret[T] = next_value
    for t in range(T - 1, -1, -1):
        a = ret[t + 1] * _rows(G, taken[t])
        a = a * mask[t + 1]
        ret[t] = a + reward[t]
        adv[t] = ret[t] - value[t]
    return ret, adv, value


def psi(feature, mask, taken, next_psi, gamma):
    """-> psi_ret [T+1, N, 2]"""
    G, _ = tables(gamma, 1.0)
    T = taken.shape[0]
    out = np.zeros_like(feature, dtype=F)
    out[T] = next_psi
    for t in range(T - 1, -1, -1):
        a = out[t + 1] * _rows(G, taken[t])[:, None]
        a = a * mask[t + 1][:, None]
        out[t] = a + feature[t]
    return out


def magnitudes(rng, shape, zeros=0.1):
    """float32 of either sign with magnitude in [2^-10, 2^10], or exactly 0 (a fraction `zeros` of them).  Every product with a
    table row (>= 0.9^64 > 2^-10 for the discounts used here) and every sum of at most a few dozen such terms then lies far inside
    the normal range - a difference that cancels is either exactly 0 or no smaller than an ulp of its operands, about 2^-34 - so no
    intermediate of the scan can be subnormal and a flush-to-zero setting of the host or the device cannot matter."""
    x = np.exp2(rng.uniform(-10.0, 10.0, shape)) * rng.choice([-1.0, 1.0], shape)
    x = np.where(rng.random(shape) < zeros, 0.0, x)
    return x.astype(F)


def random_case(T, N, seed):
    """the columns of a rollout of T steps and N envs: masks of 0 / 1 with zeros forced into the last row and (T >= 1) row 1,
    taken in 0 .. 64 with both ends forced in, and an alternative reward array for the override"""
    rng = np.random.default_rng(seed)
    c = {
        "reward": magnitudes(rng, (T, N)), "reward_override": magnitudes(rng, (T, N)), "value": magnitudes(rng, (T + 1, N)),
        "mask": (rng.random((T + 1, N)) < 0.7).astype(F), "taken": rng.integers(0, MAX_K + 1, (T, N)).astype(np.int32),
        "feature": magnitudes(rng, (T + 1, N, 2)), "next_value": magnitudes(rng, (N,)), "next_psi": magnitudes(rng, (N, 2)),
    }
    c["mask"][T, ::2] = 0.0
    c["mask"][T, 1::2] = 1.0
    c["mask"][1, ::3] = 0.0
    c["taken"][0, 0] = 0
    c["taken"][T - 1, N - 1] = MAX_K
    if T * N > 2:
        c["taken"][T - 1, 0] = MAX_K
        c["taken"][0, N - 1] = 0
    return c
