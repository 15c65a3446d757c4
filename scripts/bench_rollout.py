"""Rollout storage against the trainer's own lines (pytorch-a2c-ppo-acktr/storage.py:55,121), Maze at 8192 envs, nstack 4.

    python scripts/bench_rollout.py [--envs 8192] [--steps 16] [--batch 8192] [--reps 20] [--e2e-steps 300] [--out result.json]

One process, the two sides of every pair alternated, device events around every timed call, warm-up first:
  (a) gather      ro.gather(idx), B random rows           vs  storage_obs[:-1].view(-1, 12, 80, 60)[idx] on a materialised float32
                                                               [T + 1, N, 12, 80, 60] tensor with the same contents
  (b) push        ro.push() after a step                  vs  storage_obs[t + 1].copy_(stack)
  (c) end to end  envs.step with rollout_steps=T          vs  envs.step followed by storage_obs[t + 1].copy_(obs); env-steps/s
T = 16 keeps the baseline tensor at 32 GB (PPO's 128 would need 243 GB).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

COPY_TBPS = 6.29   # measured float4 copy rate of the MI355X's HBM


def timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(ms):
    ms = np.asarray(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()), "n": int(ms.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--e2e-steps", type=int, default=300)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from gym_miniworld_amd.batch import BatchedMiniWorld
    from gym_miniworld_amd.vec_env import make_vec_envs
    from stack_ref import FrameStackRef
    N, T, B, nstack = args.envs, args.steps, args.batch, 4
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    act = lambda: torch.from_numpy(np.where(rng.random(N) < 0.6, 2, rng.integers(0, 2, N))).to(dev)   # noqa: E731
    res = {"envs": N, "num_steps": T, "nstack": nstack, "batch": B, "device": torch.cuda.get_device_name(0)}

    # ---- (a) + (b): one batch, the rollout and the reference's storage side by side
    b = BatchedMiniWorld("MiniWorld-Maze-v0", num_envs=N, seed=1, layout="CWH")
    ro = b.rollout_enable(num_steps=T, nstack=nstack)
    ref = FrameStackRef(N, nstack, (3, b.W, b.H), device=dev)
    storage_obs = torch.zeros(T + 1, N, 3 * nstack, b.W, b.H, device=dev)
    b.reset()
    ro.push(after_reset=True)
    storage_obs[0].copy_(ref.reset(b.obs))
    push_ms, copy_ms = [], []
    for t in range(T):
        b.step(act())
        stack = ref.step(b.obs, b.done)
        for k in range(2):   # alternate which side goes first
            if (t + k) % 2 == 0:
                push_ms.append(timed(torch, ro.push)[0])
            else:
                copy_ms.append(timed(torch, lambda: storage_obs[t + 1].copy_(stack))[0])
    res["push"] = {"rollout": stats(push_ms[2:]), "baseline_copy": stats(copy_ms[2:]), "rollout_bytes_per_step": 2 * N * b.W * b.H * 3,
                   "baseline_bytes_per_step": 2 * N * 12 * b.W * b.H * 4}
    res["rollout_nbytes"], res["baseline_nbytes"] = ro.nbytes, storage_obs.numel() * 4
    flat = storage_obs[:-1].view(-1, 3 * nstack, b.W, b.H)
    g_ms, i_ms = [], []
    same = True
    for r in range(args.reps + 3):
        idx = torch.from_numpy(rng.integers(0, T * N, B)).to(dev)
        first = r % 2 == 0
        for side in ((0, 1) if first else (1, 0)):
            if side == 0:
                ms, x = timed(torch, lambda: ro.gather(idx))
                g_ms.append(ms)
            else:
                ms, y = timed(torch, lambda: flat[idx])
                i_ms.append(ms)
        same = same and torch.equal(x, y)
        del x, y
    g, i = stats(g_ms[3:]), stats(i_ms[3:])
    row = 12 * b.W * b.H
    res["gather"] = {"rollout": g, "baseline_index": i, "equal": bool(same), "rollout_bytes_per_row": row * 5, "baseline_bytes_per_row": row * 8,
                     "rollout_tb_per_s": B * row * 5 / (g["median_ms"] * 1e-3) / 1e12, "baseline_tb_per_s": B * row * 8 / (i["median_ms"] * 1e-3) / 1e12,
                     "copy_rate_tb_per_s": COPY_TBPS, "not_slower_than_baseline": bool(g["median_ms"] <= i["median_ms"])}
    b.close()
    del ro, ref, flat, b

    # ---- (c): env-steps/s through the VecEnv view, blocks of 100 steps alternated
    ea = make_vec_envs("MiniWorld-Maze-v0", seed=1, num_processes=N, device="cuda:0", rollout_steps=T)
    eb = make_vec_envs("MiniWorld-Maze-v0", seed=1, num_processes=N, device="cuda:0")
    storage_obs[0].copy_(eb.reset())
    ea.reset()
    acts = [torch.from_numpy(rng.integers(0, 3, (N, 1))).to(dev) for _ in range(16)]
    cursor = {"a": 0, "b": 0}

    def run_a(n):
        for s in range(n):
            if ea.rollout.full:
                ea.rollout.after_update()
            ea.step(acts[s % 16])

    def run_b(n):
        for s in range(n):
            if cursor["b"] == T:
                storage_obs[0].copy_(storage_obs[T])   # RolloutStorage.after_update
                cursor["b"] = 0
            obs, _, _, _ = eb.step(acts[s % 16])
            storage_obs[cursor["b"] + 1].copy_(obs)
            cursor["b"] += 1

    run_a(20), run_b(20)
    block, wall = 100, {"a": 0.0, "b": 0.0}
    for _ in range(max(1, args.e2e_steps // block)):
        for name, fn in (("a", run_a), ("b", run_b)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(block)
            torch.cuda.synchronize()
            wall[name] += time.perf_counter() - t0
    steps = max(1, args.e2e_steps // block) * block
    res["end_to_end"] = {"steps": steps, "rollout_env_steps_per_s": steps * N / wall["a"], "baseline_env_steps_per_s": steps * N / wall["b"]}
    ea.close()
    eb.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
