"""The float32 4-frame stack make_vec_envs returns, in RGB and in grey (greyscale=True): MiniWorld-Maze-v0, 8192 envs, one process.
Both handles live in one process for the whole run (they share HBM and caches); the two variants are run alternately, REPEATS times STEPS steps each after a warm-up; prints env-steps/s per repeat, the medians
and the spread, and one JSON line.  usage: ab_grey_stack.py [--envs N] [--steps K] [--repeats R] [--json out.json]"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gym_miniworld_amd import make_vec_envs
from bench import make_actions

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=8192)
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--warmup", type=int, default=40)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--json", default=None)
args = ap.parse_args()
n = args.envs
envs = {"rgb": make_vec_envs("MiniWorld-Maze-v0", 1, n, device="cuda:0"),
        "grey": make_vec_envs("MiniWorld-Maze-v0", 1, n, device="cuda:0", greyscale=True)}
acts = make_actions(args.warmup + args.steps, 0, n, torch.device("cuda:0")).to(torch.int64).unsqueeze(2)   # LongTensor [T, N, 1]
for name, e in envs.items():
    obs = e.reset()
    cpf = 1 if name == "grey" else 3   # channel planes a step adds to the stack's window
    print(name, "observation", tuple(obs.shape), obs.dtype, "%.1f MB of new stack planes per step" % (cpf * n * obs.shape[2] * obs.shape[3] * 4 / 1e6))
    for t in range(args.warmup):
        e.step(acts[t])
rates = {k: [] for k in envs}
for rep in range(args.repeats):
    for name, e in envs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(args.warmup, args.warmup + args.steps):
            e.step(acts[t])
        torch.cuda.synchronize()
        rates[name].append(n * args.steps / (time.perf_counter() - t0))
        print("repeat %d %-4s %.3f M env-steps/s" % (rep, name, rates[name][-1] / 1e6))
res = {"workload": "MiniWorld-Maze-v0 x %d, make_vec_envs float32 4-frame stack, %d steps x %d repeats, alternating; both handles alive in one process (they share HBM and caches)" % (n, args.steps, args.repeats)}
for name, r in rates.items():
    res[name] = {"env_steps_per_s": [round(x) for x in r], "median": round(statistics.median(r)), "min": round(min(r)), "max": round(max(r))}
    print("%-4s median %.3f M  spread %.3f .. %.3f M" % (name, statistics.median(r) / 1e6, min(r) / 1e6, max(r) / 1e6))
res["grey_over_rgb"] = round(res["grey"]["median"] / res["rgb"]["median"], 4)
print(json.dumps(res))
if args.json:
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1)
for e in envs.values():
    e.close()
