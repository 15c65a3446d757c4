"""The windowed gather against the plain gather and against the augmentation a trainer writes in torch today, Maze at 8192 envs,
T = 16, nstack 4, 8192 rows of float32.

    python scripts/bench_rollout_augment.py [--envs 8192] [--steps 16] [--batch 8192] [--reps 20] [--timeout 600] [--out result.json]

Four lines, alternated in one process (the order rotates every repetition), device events around every timed call, warm-up first,
medians reported:
  1. plain        ro.gather(idx)                                   mwb_rollout_gather, unchanged
  2. shift(4)     ro.gather(idx, augment=Augment.shift(4))         draw + windowed gather, one pass
  3. crop(64,48)  ro.gather(idx, augment=Augment.crop(64, 48))
  4. torch        torch_shift(ro, idx, 4) below: the plain gather, F.pad(mode="replicate"), a per-row advanced-index crop
Algorithmic bytes (what the route has to move: every stored byte read once, every output byte written once, and for line 4 the
reads and writes of its two extra passes) and GB/s are reported for each line, and the peak extra device memory
(torch.cuda.max_memory_allocated above the state before the call, minus the result itself).  The measurement runs in a child
process under a time limit; the parent never opens the GPU.  Prints one JSON line."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_shift(ro, idx, pad, dx=None, dy=None):
    """what a user writes today (RAD / DrQ random shift on a gathered minibatch): three passes over the float32 tensor"""
    import torch
    import torch.nn.functional as F
    x = ro.gather(idx)                                               # [B, 12, W, H] float32
    B, C, W, H = x.shape
    x = F.pad(x, (pad, pad, pad, pad), mode="replicate")             # [B, 12, W + 2 pad, H + 2 pad]
    dev = x.device
    dx = torch.randint(0, 2 * pad + 1, (B,), device=dev) if dx is None else dx
    dy = torch.randint(0, 2 * pad + 1, (B,), device=dev) if dy is None else dy
    ix = (dx[:, None] + torch.arange(W, device=dev))[:, None, :, None]
    iy = (dy[:, None] + torch.arange(H, device=dev))[:, None, None, :]
    return x[torch.arange(B, device=dev)[:, None, None, None], torch.arange(C, device=dev)[None, :, None, None], ix, iy]


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


def measure(args):
    import torch
    from gym_miniworld_amd import _lib
    from gym_miniworld_amd.batch import Augment, BatchedMiniWorld
    N, T, B, nstack, pad = args.envs, args.steps, args.batch, 4, 4
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    b = BatchedMiniWorld("MiniWorld-Maze-v0", num_envs=N, seed=1, layout="CWH")
    ro = b.rollout_enable(num_steps=T, nstack=nstack)
    b.reset()
    ro.push(after_reset=True)
    for _ in range(T):
        b.step(torch.from_numpy(np.where(rng.random(N) < 0.6, 2, rng.integers(0, 2, N))).to(dev))
        ro.push()
    W, H, P = b.W, b.H, 3 * nstack
    shift, crop = Augment.shift(pad), Augment.crop(64, 48)
    lines = {
        "plain": lambda idx: ro.gather(idx),
        "shift4": lambda idx: ro.gather(idx, augment=shift),
        "crop64x48": lambda idx: ro.gather(idx, augment=crop),
        "torch_shift4": lambda idx: torch_shift(ro, idx, pad),
    }
    row, crop_row, pad_row = P * W * H, P * 64 * 48, P * (W + 2 * pad) * (H + 2 * pad)
    bytes_per_row = {"plain": 5 * row, "shift4": 5 * row, "crop64x48": 5 * crop_row,
                     "torch_shift4": 5 * row + 4 * row + 4 * pad_row + 4 * row + 4 * row}   # gather; pad: read + write; crop: read + write
    out_bytes_per_row = {"plain": 4 * row, "shift4": 4 * row, "crop64x48": 4 * crop_row, "torch_shift4": 4 * row}

    # the two routes to shift(4) agree where they use the same offsets
    idx = torch.from_numpy(rng.integers(0, T * N, min(B, 512))).to(dev)
    got, offs = ro.gather(idx, augment=Augment.shift(pad, seed=3), return_offsets=True)
    same = bool(torch.equal(got, torch_shift(ro, idx, pad, offs[:, 0].long() + pad, offs[:, 1].long() + pad)))
    del got, offs

    names = list(lines)
    ms = {n: [] for n in names}
    peak = {n: 0 for n in names}
    for r in range(args.reps + 3):
        idx = torch.from_numpy(rng.integers(0, T * N, B)).to(dev)
        for k in range(len(names)):
            name = names[(r + k) % len(names)]   # the order rotates
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            t, out = timed(torch, lambda: lines[name](idx))
            peak[name] = max(peak[name], torch.cuda.max_memory_allocated() - before - out.numel() * out.element_size())
            ms[name].append(t)
            del out
    res = {"envs": N, "num_steps": T, "nstack": nstack, "batch": B, "frame": [W, H], "device": torch.cuda.get_device_name(0),
           "library": os.path.basename(_lib.LIB_PATH), "torch_route_equals_windowed_gather": same, "lines": {}}
    for n in names:
        s = stats(ms[n][3:])   # three warm-up repetitions
        s.update({"algorithmic_bytes": B * bytes_per_row[n], "result_bytes": B * out_bytes_per_row[n], "peak_extra_bytes": int(peak[n]),
                  "algorithmic_gb_per_s": B * bytes_per_row[n] / (s["median_ms"] * 1e-3) / 1e9})
        res["lines"][n] = s
    plain = res["lines"]["plain"]["median_ms"]
    res["shift4_over_plain"] = res["lines"]["shift4"]["median_ms"] / plain
    res["torch_shift4_over_shift4"] = res["lines"]["torch_shift4"]["median_ms"] / res["lines"]["shift4"]["median_ms"]
    b.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=600, help="seconds the measuring process may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(measure(args)))
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
    try:
        run = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.timeout)
    except subprocess.TimeoutExpired:
        print("bench_rollout_augment: the measuring process ran into its time limit of %d s" % args.timeout, file=sys.stderr)
        return 124
    if run.returncode != 0:
        print("bench_rollout_augment: the measuring process ended with status %d" % run.returncode, file=sys.stderr)
        return run.returncode if run.returncode > 0 else 1
    res = json.loads([ln for ln in run.stdout.split("\n") if ln.startswith("RESULT ")][-1][len("RESULT "):])
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
