"""Checking a per-env buffer of any size as a whole, on the device it lives on, without a reference of the same size.

Envs are made periodic with period P: env i gets the seed of env i % P (periodic_seeds through BatchedMiniWorld.seed(array)) and,
at every step, the action of env i % P (periodic_actions).  The envs of one residue class are then the same world, and every
per-env buffer x must satisfy x[i] == x[i - P] for all i >= P (assert_periodic: every env, every byte, no tolerance).  The first P
envs are compared with an independent reference - the oracle, tests/stack_ref.py - by the caller; induction over i does the rest.

What this catches: an env that was not written, written twice, written from another env's state, or written at a wrong address - as
long as the wrong address does not belong to an env of the same residue class.  An offset truncated to 32 (31) bits lands
2^32 (2^31) bytes early; with P prime and a per-env byte count that does not divide 2^31 that is never a whole number of periods,
which is why the callers use P = 13 and frames of 576, 14 400, 147 456, ... bytes."""
import numpy as np

P_DEFAULT = 13
CHUNK_ELEMS = 1 << 28   # elements compared at a time: the boolean temporary of one comparison is 256 MB


def periodic_seeds(n, P=P_DEFAULT, base=0):
    """seeds[i] = base + (i % P), uint64 [n]"""
    return (np.uint64(base) + (np.arange(n, dtype=np.uint64) % np.uint64(P))).astype(np.uint64)


def periodic_actions(a_P, n):
    """[P] actions -> [n]: env i gets a_P[i % P].  NumPy in, NumPy out; a torch tensor in, a torch tensor (same device) out"""
    P = len(a_P)
    if isinstance(a_P, np.ndarray):
        return a_P[np.arange(n) % P]
    import torch
    return a_P[torch.arange(n, device=a_P.device) % P]


def assert_periodic(x, P=P_DEFAULT, what=""):
    """x: torch tensor [N, ...] (any device, any strides): x[i] == x[i - P] for every i in [P, N), element for element.  Raises
    AssertionError naming the first env that differs, the first differing element in it and that element's byte offset in a
    contiguous buffer of x's shape."""
    N = x.shape[0]
    assert N > P, (what, "needs more than one period", N, P)
    per_env = 1
    for s in x.shape[1:]:
        per_env *= int(s)
    step = max(1, CHUNK_ELEMS // max(per_env, 1))
    for lo in range(P, N, step):
        hi = min(N, lo + step)
        ne = x[lo:hi] != x[lo - P:hi - P]
        if bool(ne.any()):
            ne = ne.reshape(hi - lo, -1)
            k = int(ne.any(dim=1).nonzero()[0])
            j = int(ne[k].nonzero()[0])
            env = lo + k
            n_bad = int(ne.any(dim=1).sum())
            raise AssertionError("%s: env %d differs from env %d at element %d (byte offset %d of the buffer, %d bytes per env); "
                                 "got %r, env %d has %r; %d envs of [%d, %d) differ from their predecessors"
                                 % (what, env, env - P, j, (env * per_env + j) * x.element_size(), per_env * x.element_size(),
                                    x[env].reshape(-1)[j].item(), env - P, x[env - P].reshape(-1)[j].item(), n_bad, lo, hi))
        del ne
