"""Cost of mwb_copy_envs on one MI355X: Maze-v0, 8192 envs, device events, all legs of a comparison in one process, alternating.

    python scripts/bench_copy_envs.py [--envs 8192] [--reps 200] [--parent DIR] [--out profiles/copy_envs.txt]

  (i)   the state-only copy of every env between two handles against one hipMemcpyAsync device-to-device of the same number of
        bytes (the descriptor table's total, mwb_copy_env_bytes): the plain copy is the floor, the ratio is reported
  (ii)  the rendering copy of every env against mwb_render on the same handle (expected: render + (i))
  (iii) with --parent DIR (a checkout of the parent commit, built): `python bench.py` of this tree and of DIR, alternating, three
        times each, one fresh process per run - the step path is untouched, so the two sets of three should overlap
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def summary(ms):
    ms = sorted(ms)
    return {"median_ms": statistics.median(ms), "min_ms": ms[0], "p90_ms": ms[int(0.9 * (len(ms) - 1))], "n": len(ms)}


def copy_legs(n, reps, warmup, lines):
    import torch
    from gym_miniworld_amd.batch import BatchedMiniWorld
    a = BatchedMiniWorld("MiniWorld-Maze-v0", num_envs=n, seed=1)
    b = BatchedMiniWorld("MiniWorld-Maze-v0", num_envs=n, seed=100000)
    a.reset(); b.reset()
    acts = torch.randint(0, 3, (8, n), dtype=torch.int32, device=a.device)
    for t in range(8):
        a.step(acts[t]); b.step(acts[t])
    idx = torch.arange(n, dtype=torch.int32, device=a.device)
    env_bytes = int(a.L.mwb_copy_env_bytes(b.h, a.h))
    total = env_bytes * n
    lines.append("Maze-v0, %d envs: %d bytes of state per env (descriptor table), %.1f MB per copy of every env" % (n, env_bytes, total / 1e6))
    src_buf = torch.empty(total, dtype=torch.uint8, device=a.device).random_(0, 255)
    dst_buf = torch.empty_like(src_buf)
    stream = ctypes.c_void_p(torch.cuda.current_stream(a.device).cuda_stream)
    hip = a.L   # the HIP runtime libmwbatch.so is linked against (dlsym looks through a library's dependencies): torch's own
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]

    def plain():
        assert hip.hipMemcpyAsync(dst_buf.data_ptr(), src_buf.data_ptr(), total, 3, stream) == 0   # hipMemcpyDeviceToDevice

    legs = {"state_copy": lambda: b.copy_envs(idx, idx, src=a, render=False), "memcpy_d2d": plain,
            "render_copy": lambda: b.copy_envs(idx, idx, src=a, render=True), "mwb_render": lambda: b.render()}
    events = {k: [] for k in legs}
    for r in range(warmup + reps):
        for k, fn in legs.items():   # alternating: every leg once per repetition
            ev = timed(torch, fn)
            if r >= warmup:
                events[k].append(ev)
    torch.cuda.synchronize()
    res = {k: summary([e0.elapsed_time(e1) for e0, e1 in v]) for k, v in events.items()}
    assert b.copy_rejected() == 0
    for k in ("state_copy", "memcpy_d2d", "render_copy", "mwb_render"):
        lines.append("%-12s median %.4f ms  min %.4f  p90 %.4f  (n = %d)" % (k, res[k]["median_ms"], res[k]["min_ms"], res[k]["p90_ms"], res[k]["n"]))
    gbs = lambda k: 2 * total / (res[k]["median_ms"] * 1e-3) / 1e9   # noqa: E731  read + write
    lines.append("(i)  state copy / plain copy = %.2f   (%.0f GB/s against %.0f GB/s, read + write)" %
                 (res["state_copy"]["median_ms"] / res["memcpy_d2d"]["median_ms"], gbs("state_copy"), gbs("memcpy_d2d")))
    lines.append("(ii) rendering copy %.4f ms = mwb_render %.4f ms + %.4f ms   (state copy alone: %.4f ms)" %
                 (res["render_copy"]["median_ms"], res["mwb_render"]["median_ms"], res["render_copy"]["median_ms"] - res["mwb_render"]["median_ms"],
                  res["state_copy"]["median_ms"]))
    a.close(); b.close()
    return res


def bench_legs(parent, steps, warmup, lines):
    vals = {"this": [], "parent": []}
    for r in range(3):
        for name, root in (("this", ROOT), ("parent", parent)):
            out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                                 cwd=root, capture_output=True, text=True, timeout=600, check=True).stdout
            vals[name].append(json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])["value"])
    for name in ("this", "parent"):
        lines.append("(iii) bench.py %-6s env-steps/s: %s" % (name, "  ".join("%.0f" % v for v in vals[name])))
    lo, hi = min(vals["parent"]), max(vals["parent"])
    inside = [lo <= v <= hi for v in vals["this"]]
    lines.append("(iii) parent's spread %.0f .. %.0f; this commit's runs inside it: %d of 3; medians %.0f (this) / %.0f (parent) = %.4f" %
                 (lo, hi, sum(inside), statistics.median(vals["this"]), statistics.median(vals["parent"]),
                  statistics.median(vals["this"]) / statistics.median(vals["parent"])))
    return vals


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: adds leg (iii)")
    ap.add_argument("--bench-steps", type=int, default=300)
    ap.add_argument("--bench-warmup", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    if args.parent:   # first, before this process opens the GPU: the benchmark runs have the device to themselves
        bench_legs(os.path.abspath(args.parent), args.bench_steps, args.bench_warmup, lines)
    copy_legs(args.envs, args.reps, args.warmup, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
