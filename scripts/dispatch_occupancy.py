#!/usr/bin/env python3
"""Occupancy curve and drain of the bulk render launch, and how many blocks of the half-frame tail do any rendering, from the
per-workgroup s_memrealtime stamps (MWB_DEBUG bit 4), at steady state.

    python scripts/dispatch_occupancy.py [workload] [warm-up steps] [measured steps] [old-map]     (on the GPU box, from the repo root)

After every measured step the stamps are read back and compared with the step before: a block whose stamps changed has
rendered in this step (a block that copies a reused frame, finds a regenerated env or has nothing to do writes none).  Per step:
the launch's span, the drain (from the first moment fewer than 90 % of the 1280 workgroup slots are busy, after the launch has
filled, to its end), the slot-time idle in it as a share of slots x span.  With `old-map` as the fourth argument - for a library from
before the work lists, whose last 2 x split_envs blocks are the halves of the split_envs cheapest envs of the whole
order - also the number of rendering blocks among those: what is missing there was reused, or regenerated.  (With the work lists
the halves are blocks [R - S, R + S) and all of them render; the grid's last blocks copy or exit.)"""
import ctypes
import os
import sys

import numpy as np

os.environ["MWB_DEBUG"] = str(int(os.environ.get("MWB_DEBUG", "0")) | 16)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from gym_miniworld_amd.batch import BatchedMiniWorld  # noqa: E402

SLOTS = 1280   # 256 CUs x 5 workgroups


def main():
    wl = sys.argv[1] if len(sys.argv) > 1 else "maze8192"
    warm = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 50
    old_map = len(sys.argv) > 4 and sys.argv[4] == "old-map"
    spec = bench.WORKLOADS[wl]
    env_id, n, depth, dr = spec[:4]
    n_actions = spec[5] if len(spec) > 5 else 3
    env = BatchedMiniWorld(env_id, num_envs=n, seed=1, domain_rand=dr, want_depth=depth)
    acts = bench.make_actions(warm + steps, 0, n, env.device, n_actions)
    env.reset()
    cap = 2 * n + 4096
    buf = np.zeros(cap * 2, np.uint64)

    def stamps():
        torch.cuda.synchronize()
        k = env.L.mwb_debug_wg_times(env.h, buf.ctypes.data_as(ctypes.c_void_p), cap)
        return buf[:2 * k].reshape(k, 2).astype(np.int64).copy()

    for t in range(warm):
        env.step(acts[t])
    prev = stamps()
    grid = len(prev)
    split = grid - n
    env.frame_reuse_stats()
    rows, curve = [], None
    for t in range(warm, warm + steps):
        env.step(acts[t])
        ts = stamps()
        reused, rendered = env.frame_reuse_stats()
        live = np.nonzero((ts != prev).any(axis=1))[0]
        prev = ts
        t0 = ts[live, 0].min()
        start, end = (ts[live, 0] - t0) / 100.0, (ts[live, 1] - t0) / 100.0   # microseconds
        span = end.max()
        # slots busy against time, exactly: +1 at every start, -1 at every end
        ev_t = np.concatenate([start, end])
        ev_d = np.concatenate([np.ones(len(start)), -np.ones(len(end))])
        o = np.argsort(ev_t, kind="stable")
        ev_t, busy = ev_t[o], np.cumsum(ev_d[o])
        full = np.nonzero(busy >= 0.9 * SLOTS)[0]
        if len(full):
            i_drain = full[-1] + 1          # the first event after which the launch never gets back to 90 %
            t_drain = ev_t[min(i_drain, len(ev_t) - 1)]
            seg = np.diff(np.append(ev_t[i_drain:], span))
            lost = float(np.sum((SLOTS - busy[i_drain:]) * seg))
        else:
            t_drain, lost = 0.0, float("nan")
        tail_blocks = int(np.sum(live >= n - split)) if split and old_map else 0
        rows.append((span, span - t_drain, lost / (SLOTS * span), len(live), tail_blocks, reused, rendered,
                     float(np.sum(end - start)) / (SLOTS * span)))
        if t == warm + steps - 1:
            g = np.linspace(0, span, 41)
            curve = [int(np.sum((start <= x) & (end > x))) for x in g]
            dur = end - start
            print("%s last step: %d rendering workgroups, duration mean %.1f us  p5 %.1f  p50 %.1f  p95 %.1f  max %.1f"
                  % (wl, len(live), dur.mean(), *np.percentile(dur, [5, 50, 95]), dur.max()))
            if split and old_map:
                hd = dur[live >= n - split]
                if len(hd):
                    print("  of them in the last 2 x %d blocks: %d, duration p5 %.1f  p50 %.1f  p95 %.1f us" % (split, len(hd), *np.percentile(hd, [5, 50, 95])))
            print("  slots busy over time (40 bins of %.1f us):" % (span / 40), " ".join("%d" % a for a in curve))
    r = np.array(rows, dtype=np.float64)
    med = np.median(r, axis=0)
    print("%s, N %d, split_envs %d, grid %d, %d steps after %d:" % (wl, n, split, grid, steps, warm))
    print("  launch span (first start to last end)  median %.1f us  (min %.1f  max %.1f)" % (med[0], r[:, 0].min(), r[:, 0].max()))
    print("  drain (below 90 %% of %d slots to the end) median %.1f us  (min %.1f  max %.1f)" % (SLOTS, med[1], r[:, 1].min(), r[:, 1].max()))
    print("  idle slot-time in the drain / (slots x span)  median %.4f  (min %.4f  max %.4f)" % (med[2], r[:, 2].min(), r[:, 2].max()))
    print("  busy slot-time over the whole launch / (slots x span)  median %.4f" % med[7])
    print("  rendering workgroups per step  median %d;  frames reused / rendered per step  median %d / %d" % (med[3], med[5], med[6]))
    if split and old_map:
        print("  rendering blocks among the last 2 x %d  median %d  (min %d  max %d): %.1f %% of the tail's blocks do not render"
              % (split, med[4], r[:, 4].min(), r[:, 4].max(), 100.0 * (1.0 - med[4] / (2.0 * split))))
    env.close()


if __name__ == "__main__":
    main()
