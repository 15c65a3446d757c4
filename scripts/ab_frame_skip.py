"""Action repeat (frame_skip=k, mwb_step_repeat) against the plain step: make_vec_envs("MiniWorld-Maze-v0", 8192) with frame_skip 1, 2, 4
and 8 and the pickupobjs8192 workload at 1 and 4, one process.  All handles live in one process for the whole run (they share HBM
and caches); the variants are run alternately, REPEATS times CALLS calls each after a warm-up; prints calls/s and env-steps/s
(N * the sub-steps actually taken, info['taken'] - not N * k * calls) per repeat, the medians and the spread, the cost of one
further sub-step per call (t_k - t_1) / (k - 1) beside the step time mwb_timing_read reports, and one JSON line.
--root DIR imports the package (and bench.py's action stream) from another checkout - e.g. the parent commit's, for its plain-step
leg: that tree has no frame_skip argument, so only skip 1 can run there (--maze-skips 1 --pickup-skips "").
usage: ab_frame_skip.py [--envs N] [--calls K] [--repeats R] [--maze-skips 1,2,4,8] [--pickup-skips 1,4] [--root DIR] [--json out.json]"""
import argparse, json, os, statistics, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=8192)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--warmup", type=int, default=30)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--maze-skips", default="1,2,4,8")
ap.add_argument("--pickup-skips", default="1,4")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--json", default=None)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import torch
import gym_miniworld_amd
from gym_miniworld_amd import make_vec_envs
from bench import make_actions

n = args.envs
dev = torch.device("cuda:0")
ints = lambda s: [int(v) for v in s.split(",") if v.strip()]   # noqa: E731
variants = {}   # name -> (env, k, actions [T, N, 1])
T = args.warmup + args.calls
for task, env_id, skips, n_act in (("maze", "MiniWorld-Maze-v0", ints(args.maze_skips), 3), ("pickupobjs", "MiniWorld-PickupObjs-v0", ints(args.pickup_skips), 5)):
    acts = make_actions(T, 0, n, dev, n_act).to(torch.int64).unsqueeze(2) if skips else None   # LongTensor [T, N, 1], one action per call
    for k in skips:
        kw = {"frame_skip": k} if k > 1 else {}   # (a tree from before the feature has no such argument)
        variants["%s_skip%d" % (task, k)] = (make_vec_envs(env_id, 1, n, device="cuda:0", **kw), k, acts)
print("package:", os.path.dirname(gym_miniworld_amd.__file__), " variants:", ", ".join(variants))


def run(e, acts, t0, t1):
    taken = 0
    for t in range(t0, t1):
        _, _, _, infos = e.step(acts[t])
        tk = getattr(infos, "taken", None)
        taken += n if tk is None else int(tk.sum())
    return taken


for name, (e, k, acts) in variants.items():
    e.reset()
    run(e, acts, 0, args.warmup)
secs = {v: [] for v in variants}
steps = {v: [] for v in variants}
for rep in range(args.repeats):
    for name, (e, k, acts) in variants.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        taken = run(e, acts, args.warmup, T)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        secs[name].append(dt / args.calls)
        steps[name].append(taken / dt)
        print("repeat %d %-16s %8.1f calls/s  %.3f M env-steps/s  (%.2f sub-steps per env and call)" % (rep, name, args.calls / dt, taken / dt / 1e6, taken / (n * args.calls)))
# per-kernel times of a call (events every pass: outside the timed repeats).  "step" spans a call's step and fold launches
kernel_ms = {}
for name, (e, k, acts) in variants.items():
    e.batch.timing_enable(True)
    run(e, acts, args.warmup, args.warmup + min(args.calls, 60))
    torch.cuda.synchronize()
    tm = e.batch.timing_read()
    e.batch.timing_enable(False)
    kernel_ms[name] = {key: round(tm[key], 5) for key in ("step", "reset", "prep", "render")}
res = {"workload": "make_vec_envs float32 4-frame stack x %d envs, %d calls x %d repeats, alternating; all handles alive in one process" % (n, args.calls, args.repeats),
       "package": os.path.dirname(gym_miniworld_amd.__file__)}
for name, (e, k, acts) in variants.items():
    ms = [s * 1e3 for s in secs[name]]
    res[name] = {"frame_skip": k, "ms_per_call": [round(x, 4) for x in ms], "ms_per_call_median": round(statistics.median(ms), 4),
                 "calls_per_s_median": round(1e3 / statistics.median(ms), 1), "calls_per_s_min": round(1e3 / max(ms), 1), "calls_per_s_max": round(1e3 / min(ms), 1),
                 "env_steps_per_s": [round(x) for x in steps[name]], "env_steps_per_s_median": round(statistics.median(steps[name])),
                 "env_steps_per_s_min": round(min(steps[name])), "env_steps_per_s_max": round(max(steps[name])), "kernel_ms": kernel_ms[name]}
    print("%-16s median %8.1f calls/s  %.3f M env-steps/s  spread %.3f .. %.3f M   kernels %s" % (
        name, 1e3 / statistics.median(ms), statistics.median(steps[name]) / 1e6, min(steps[name]) / 1e6, max(steps[name]) / 1e6, kernel_ms[name]))
for task in ("maze", "pickupobjs"):
    base = res.get(task + "_skip1")
    for name, (e, k, acts) in variants.items():
        if base and name.startswith(task) and k > 1:
            res[name]["ms_per_further_sub_step"] = round((res[name]["ms_per_call_median"] - base["ms_per_call_median"]) / (k - 1), 5)
            res[name]["env_steps_over_skip1"] = round(res[name]["env_steps_per_s_median"] / base["env_steps_per_s_median"], 3)
            print("%-16s %.4f ms per further sub-step and call (step kernel of a plain call: %.4f ms), %.2fx the env-steps/s of skip 1" % (
                name, res[name]["ms_per_further_sub_step"], base["kernel_ms"]["step"], res[name]["env_steps_over_skip1"]))
print(json.dumps(res))
if args.json:
    with open(args.json, "w") as f:
        json.dump(res, f, indent=1)
for e, _, _ in variants.values():
    e.close()
