"""What terminal observations (MiniWorldVecEnv(terminal_obs=K)) cost a step: Maze at 8192 envs through
make_vec_envs(..., frame_stack=4), 300 steps after warm-up.

    python scripts/bench_terminal.py [--parent-lib libmwbatch_parent.so] [--envs 8192] [--steps 300] [--warmup 50] [--runs 2] [--out result.json]

Legs, each run in a fresh child process (a process loads one library), alternated run by run:
  (a) parent     the parent commit's library (--parent-lib, loaded through MWB_LIB; skipped without it), feature off
  (b) off        this library, feature off: must lie within the run-to-run spread of (a)
  (c) on_1024    terminal_obs=1024
  (d) on_n       terminal_obs=N
device_ms: HIP events around everything a step enqueues (step_async), median over the steps of a run; wall_ms: wall clock of the
run per step (step_async + step_wait).  spread: the largest difference between two runs of one leg.  ended: envs that ended per
step (mean, max) - what the side chain has to render twice with the feature on.  `--leg NAME` runs one leg in this process and
prints its JSON line (also the form to put behind `rocprofv3 --kernel-trace --stats --` for the terminal launches' own times).
Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEGS = {"parent": 0, "off": 0, "on_1024": 1024, "on_n": -1}


def run_leg(args):
    import torch
    from gym_miniworld_amd.vec_env import make_vec_envs
    N, dev = args.envs, torch.device("cuda:0")
    cap = LEGS[args.leg]
    kw = {"terminal_obs": min(N, cap) if cap > 0 else N} if cap else {}
    envs = make_vec_envs(args.env_id, seed=1, num_processes=N, device="cuda:0", **kw)
    rng = np.random.default_rng(0)
    acts = [torch.from_numpy(np.where(rng.random(N) < 0.6, 2, rng.integers(0, 2, N)).reshape(N, 1)).to(dev) for _ in range(16)]
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    envs.reset()
    for s in range(args.warmup):
        envs.step(acts[s % 16])
    ended = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(args.steps):
        events[s][0].record()
        envs.step_async(acts[s % 16])
        events[s][1].record()
        done = envs.step_wait()[2]
        ended.append(int(done.sum()))
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / args.steps
    res = {"leg": args.leg, "device_ms": float(np.median([a.elapsed_time(b) for a, b in events])), "wall_ms": wall,
           "ended_mean": float(np.mean(ended)), "ended_max": int(np.max(ended)), "device": torch.cuda.get_device_name(0)}
    if cap:
        res["dropped"] = envs.terminal.dropped()
    envs.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--env-id", default="MiniWorld-Maze-v0")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--leg", default=None, choices=sorted(LEGS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.leg:
        return run_leg(args)
    legs = [leg for leg in LEGS if leg != "parent" or args.parent_lib]
    runs = {leg: [] for leg in legs}
    for r in range(args.runs):
        for leg in legs[r % len(legs):] + legs[:r % len(legs)]:   # every leg takes another place in the order each run
            env = dict(os.environ)
            if leg == "parent":
                env["MWB_LIB"] = os.path.abspath(args.parent_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--envs", str(args.envs), "--steps", str(args.steps),
                   "--warmup", str(args.warmup), "--env-id", args.env_id]
            out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                raise SystemExit("leg %s failed (%d): %s" % (leg, out.returncode, out.stderr[-2000:]))
            runs[leg].append(json.loads(out.stdout.strip().split("\n")[-1]))
    res = {"envs": args.envs, "env_id": args.env_id, "steps": args.steps, "warmup": args.warmup, "runs": args.runs, "frame_stack": 4,
           "device": runs[legs[0]][0]["device"]}
    for leg in legs:
        d, w = [x["device_ms"] for x in runs[leg]], [x["wall_ms"] for x in runs[leg]]
        res[leg] = {"device_ms": float(np.median(d)), "wall_ms": float(np.median(w)), "device_ms_runs": d, "wall_ms_runs": w,
                    "device_spread": max(d) - min(d), "wall_spread": max(w) - min(w),
                    "ended_mean": runs[leg][0]["ended_mean"], "ended_max": runs[leg][0]["ended_max"]}
        if "dropped" in runs[leg][0]:
            res[leg]["dropped"] = runs[leg][0]["dropped"]
    if "parent" in res:
        res["off_minus_parent"] = {"device_ms": res["off"]["device_ms"] - res["parent"]["device_ms"], "wall_ms": res["off"]["wall_ms"] - res["parent"]["wall_ms"],
                                   "parent_device_spread": res["parent"]["device_spread"], "parent_wall_spread": res["parent"]["wall_spread"]}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
