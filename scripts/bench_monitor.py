"""The episode monitor against the trainer's own loop (pytorch-a2c-ppo-acktr/main.py:167-169), Maze at 8192 envs through
make_vec_envs(..., frame_stack=4).

    python scripts/bench_monitor.py [--envs 8192] [--steps 300] [--runs 5] [--warmup 30] [--out result.json]

Three legs, one process, alternated run by run, warm-up first; per run `steps` steps, the figures are medians over the runs:
  (a) envs.step without a monitor                        what the library did before the monitor: the yardstick
  (b) envs.step with monitor=100                         the update's three launches and one more small copy inside every step
  (c) (a) plus the reference's loop on the host          for idx, eps_done in enumerate(done): ... with the return summed per
                                                         episode (the sum itself is one NumPy add per step: only the loop over
                                                         `done` and the appends are interpreted, the cheapest honest form of it)
device_ms: HIP events around everything a step enqueues (step_async), median over the steps of a run; wall_ms: wall clock of the
whole run (step + step_wait + the leg's host work) per step.  update_ms: HIP events around a block of back-to-back
monitor.update() calls, per call - the three launches alone.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time
from collections import deque

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--env-id", default="MiniWorld-Maze-v0")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from gym_miniworld_amd.vec_env import make_vec_envs
    N, dev = args.envs, torch.device("cuda:0")
    rng = np.random.default_rng(0)
    acts = [torch.from_numpy(np.where(rng.random(N) < 0.6, 2, rng.integers(0, 2, N)).reshape(N, 1)).to(dev) for _ in range(16)]
    legs = {"a_plain": make_vec_envs(args.env_id, seed=1, num_processes=N, device="cuda:0"),
            "b_monitor": make_vec_envs(args.env_id, seed=1, num_processes=N, device="cuda:0", monitor=100),
            "c_host_loop": make_vec_envs(args.env_id, seed=1, num_processes=N, device="cuda:0")}
    episode_rewards, running = deque(maxlen=100), np.zeros(N)
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]

    def run(name, n, timed):
        envs = legs[name]
        for s in range(n):
            if timed:
                events[s][0].record()
            envs.step_async(acts[s % 16])
            if timed:
                events[s][1].record()
            _, reward, done, _ = envs.step_wait()
            if name == "c_host_loop":
                np.add(running, reward.numpy()[:, 0], out=running)
                for idx, eps_done in enumerate(done):
                    if eps_done:
                        episode_rewards.append(running[idx])
                        running[idx] = 0.0

    for name, envs in legs.items():
        envs.reset()
        run(name, args.warmup, False)
    device_ms, wall_ms = {k: [] for k in legs}, {k: [] for k in legs}
    for r in range(args.runs):
        order = list(legs)[r % 3:] + list(legs)[:r % 3]   # every leg takes every place in the order
        for name in order:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(name, args.steps, True)
            torch.cuda.synchronize()
            wall_ms[name].append((time.perf_counter() - t0) * 1e3 / args.steps)
            device_ms[name].append(float(np.median([a.elapsed_time(b) for a, b in events])))
    res = {"envs": N, "env_id": args.env_id, "steps": args.steps, "runs": args.runs, "frame_stack": 4, "device": torch.cuda.get_device_name(0)}
    for name in legs:
        res[name] = {"device_ms": float(np.median(device_ms[name])), "wall_ms": float(np.median(wall_ms[name])),
                     "device_ms_runs": device_ms[name], "wall_ms_runs": wall_ms[name],
                     "env_steps_per_s": N / (float(np.median(wall_ms[name])) * 1e-3)}
    # the update alone: back-to-back calls, events around the block
    mon = legs["b_monitor"].monitor
    for _ in range(20):
        mon.update()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    per = []
    for _ in range(args.runs):
        a.record()
        for _ in range(200):
            mon.update()
        b.record()
        b.synchronize()
        per.append(a.elapsed_time(b) / 200)
    res["update_ms"] = float(np.median(per))
    base = res["a_plain"]
    res["monitor_over_plain"] = {"device": res["b_monitor"]["device_ms"] / base["device_ms"], "wall": res["b_monitor"]["wall_ms"] / base["wall_ms"]}
    res["host_loop_over_plain"] = {"wall": res["c_host_loop"]["wall_ms"] / base["wall_ms"]}
    res["host_loop_over_monitor"] = {"wall": res["c_host_loop"]["wall_ms"] / res["b_monitor"]["wall_ms"]}
    res["monitor_total"], res["host_loop_total"] = mon.read()[0], len(episode_rewards)
    for envs in legs.values():
        envs.close()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
