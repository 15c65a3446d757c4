"""What level sets (MiniWorldVecEnv(num_levels=L)) cost a step, through make_vec_envs(..., frame_stack=4) at 8192 envs.

    python scripts/bench_levels.py [--parent-lib libmwbatch_parent.so] [--envs 8192] [--runs 3] [--workloads maze20,maze300,oneroom,timeout]
                                   [--out profiles/levels_bench.json]

Workloads:
  maze20    MiniWorld-Maze-v0, the 20-step protocol (5 warm-up steps)          few envs end per step
  maze300   MiniWorld-Maze-v0, the 300-step protocol (50 warm-up steps)
  oneroom   MiniWorld-OneRoomS6Fast-v0, 300 steps                              many envs end per step
  timeout   MiniWorld-Maze-v0 with max_episode_steps = 24: the steps at which every env times out together, timed alone
Legs, each run in a fresh child process (a process loads one library), alternated run by run so that every pair of
configurations is compared inside one call:
  parent    the parent commit's library (--parent-lib, loaded through MWB_LIB; skipped without it)
  off       this library without level sets: nothing more is launched, the difference to `parent` must lie inside the spread of
            the parent's own runs
  on        num_levels = 200, level_mode "uniform", tallies on
device_ms: HIP events around everything a step enqueues (step_async), median over the timed steps of a run (timeout: over the
mass time-out steps only); wall_ms: wall clock per step (step_async + step_wait).  spread: the largest difference between two runs of
one leg.  ended: envs regenerated per step (mean, max).  `--leg NAME --workload NAME` runs one leg in this process and prints its
JSON line - also the form to put behind `rocprofv3 --kernel-trace --stats --` for levels_assign_kernel's own time.  Prints one JSON
line."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEGS = ("parent", "off", "on")
# workload -> (env id, timed steps, warm-up steps, max_episode_steps or None)
WORKLOADS = {"maze20": ("MiniWorld-Maze-v0", 20, 5, None), "maze300": ("MiniWorld-Maze-v0", 300, 50, None),
             "oneroom": ("MiniWorld-OneRoomS6Fast-v0", 300, 50, None), "timeout": ("MiniWorld-Maze-v0", 120, 24, 24)}
NUM_LEVELS = 200


def run_leg(args):
    import torch
    from gym_miniworld_amd.vec_env import make_vec_envs
    env_id, steps, warmup, mes = WORKLOADS[args.workload]
    N, dev = args.envs, torch.device("cuda:0")
    kw = dict(num_levels=NUM_LEVELS, level_mode="uniform") if args.leg == "on" else {}
    if mes:
        kw["max_episode_steps"] = mes
    envs = make_vec_envs(env_id, seed=1, num_processes=N, device="cuda:0", **kw)
    rng = np.random.default_rng(0)
    acts = [torch.from_numpy(np.where(rng.random(N) < 0.6, 2, rng.integers(0, 2, N)).reshape(N, 1)).to(dev) for _ in range(16)]
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    envs.reset()
    for s in range(warmup):
        envs.step(acts[s % 16])
    ended = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for s in range(steps):
        events[s][0].record()
        envs.step_async(acts[s % 16])
        events[s][1].record()
        done = envs.step_wait()[2]
        ended.append(int(done.sum()))
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / steps
    ms = np.array([a.elapsed_time(b) for a, b in events])
    ended = np.array(ended)
    if mes:   # only the steps at which (nearly) every env timed out
        mass = ended > N // 2
        assert mass.any(), "no mass time-out inside the timed steps"
        ms, n_mass = ms[mass], int(mass.sum())
    res = {"leg": args.leg, "workload": args.workload, "device_ms": float(np.median(ms)), "wall_ms": wall,
           "ended_mean": float(ended.mean()), "ended_max": int(ended.max()), "device": torch.cuda.get_device_name(0)}
    if mes:
        res["mass_steps"] = n_mass
    if args.leg == "on":
        res["episodes_tallied"] = int(envs.levels.episodes.sum())
    envs.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--workloads", default="maze20,maze300,oneroom,timeout")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--leg", default=None, choices=LEGS)
    ap.add_argument("--workload", default="maze300", choices=sorted(WORKLOADS))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.leg:
        return run_leg(args)
    legs = [leg for leg in LEGS if leg != "parent" or args.parent_lib]
    res = {"envs": args.envs, "runs": args.runs, "frame_stack": 4, "num_levels": NUM_LEVELS, "workloads": {}}
    for wl in args.workloads.split(","):
        runs = {leg: [] for leg in legs}
        for r in range(args.runs):
            for leg in legs[r % len(legs):] + legs[:r % len(legs)]:   # every leg takes another place in the order each run
                env = dict(os.environ)
                if leg == "parent":
                    env["MWB_LIB"] = os.path.abspath(args.parent_lib)
                cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--workload", wl, "--envs", str(args.envs)]
                out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
                if out.returncode != 0:
                    raise SystemExit("leg %s of %s failed (%d): %s" % (leg, wl, out.returncode, out.stderr[-2000:]))
                runs[leg].append(json.loads(out.stdout.strip().split("\n")[-1]))
                print("# %s %s run %d: %s" % (wl, leg, r, out.stdout.strip().split("\n")[-1]), file=sys.stderr, flush=True)
        env_id, steps, warmup, mes = WORKLOADS[wl]
        w = {"env_id": env_id, "steps": steps, "warmup": warmup, "max_episode_steps": mes, "device": runs[legs[0]][0]["device"]}
        for leg in legs:
            d, t = [x["device_ms"] for x in runs[leg]], [x["wall_ms"] for x in runs[leg]]
            w[leg] = {"device_ms": float(np.median(d)), "wall_ms": float(np.median(t)), "device_ms_runs": d, "wall_ms_runs": t,
                      "device_spread": max(d) - min(d), "wall_spread": max(t) - min(t),
                      "ended_mean": runs[leg][0]["ended_mean"], "ended_max": runs[leg][0]["ended_max"]}
        w["on_minus_off"] = {"device_ms": w["on"]["device_ms"] - w["off"]["device_ms"], "wall_ms": w["on"]["wall_ms"] - w["off"]["wall_ms"],
                             "off_device_spread": w["off"]["device_spread"], "off_wall_spread": w["off"]["wall_spread"]}
        if "parent" in w:
            w["off_minus_parent"] = {"device_ms": w["off"]["device_ms"] - w["parent"]["device_ms"], "wall_ms": w["off"]["wall_ms"] - w["parent"]["wall_ms"],
                                     "parent_device_spread": w["parent"]["device_spread"], "parent_wall_spread": w["parent"]["wall_spread"]}
        res["workloads"][wl] = w
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
