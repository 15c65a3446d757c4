"""The rollout's returns scan and column gather against the trainer's own lines (pytorch-a2c-ppo-acktr/storage.py:82-105,124-128).

    python scripts/bench_rollout_returns.py [--envs 8192] [--steps 16 128] [--batch 8192] [--reps 30] [--out result.json]

One process, the two sides of every pair alternated, device events around every timed call, warm-up first.  Per T:
  (i)   ro.compute_returns / compute_psi_returns, one kernel each (GAE, discounted, psi)
  (ii)  the reference's backward loops restated on device tensors holding the same columns: T iterations of eager elementwise ops
  (iii) ro.minibatch's column kernel (mwb_rollout_gather_cols) for B rows  vs  the six separate tensor[idx] of the generator
The yardstick is (ii) and the six torch calls.  taken is 1 everywhere, so that both sides compute the same numbers ("equal" says
whether they are bit-equal).  The frames are 10 x 6 pixels: the columns are what is timed, and the ring stays small at T = 128.
Bytes are those the algorithm needs: per (step, env) the GAE and discounted scans read reward, value, mask, taken and write return
and advantage (24 B), psi reads feature, mask, taken and writes two components (24 B).  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

COPY_TBPS = 6.29   # measured float4 copy rate of the MI355X's HBM
TORCH_OPS_PER_STEP = {"gae": 9, "discounted": 4, "psi": 5}   # eager elementwise ops (one launch each) per iteration of the loops below
SCAN_BYTES = 24    # per (step, env), every mode


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


def torch_gae(rewards, value_preds, masks, returns, next_value, gamma, tau):
    value_preds[-1] = next_value
    gae = 0
    for step in reversed(range(rewards.size(0))):
        delta = rewards[step] + gamma * value_preds[step + 1] * masks[step + 1] - value_preds[step]
        gae = delta + gamma * tau * masks[step + 1] * gae
        returns[step] = gae + value_preds[step]


def torch_discounted(rewards, masks, returns, next_value, gamma):
    returns[-1] = next_value
    for step in reversed(range(rewards.size(0))):
        returns[step] = returns[step + 1] * gamma * masks[step + 1] + rewards[step]


def torch_psi(features, masks, psi_returns, next_psi, gamma):
    psi_returns[-1] = next_psi
    for step in reversed(range(features.size(0) - 1)):
        psi_returns[step] = psi_returns[step + 1] * gamma * masks[step + 1].repeat(1, psi_returns.shape[-1]) + features[step]


def one_size(torch, args, T, res):
    import returns_ref as R
    from gym_miniworld_amd.batch import BatchedMiniWorld
    N, B, gamma, tau = args.envs, args.batch, 0.99, 0.95
    dev = torch.device("cuda:0")
    b = BatchedMiniWorld("MiniWorld-Hallway-v0", num_envs=N, seed=1, layout="CWH", obs_width=10, obs_height=6)
    ro = b.rollout_enable(num_steps=T, nstack=1, learner=True)
    b.reset()
    ro.push(after_reset=True)
    for _ in range(T):
        b.step(torch.full((N,), 2, dtype=torch.int32))
        ro.push()
    c = R.random_case(T, N, seed=T)
    for view, key in ((ro.rewards, "reward"), (ro.masks, "mask"), (ro.value_preds, "value"), (ro.features, "feature")):
        view.copy_(torch.from_numpy(c[key]).to(dev))
    ro.taken.fill_(1)
    ro.action_log_probs.copy_(torch.from_numpy(c["reward_override"]).to(dev))
    nv, npsi = torch.from_numpy(c["next_value"]).to(dev), torch.from_numpy(c["next_psi"]).to(dev)
    # the reference's storage, [T (+ 1), N, 1] as it keeps them, with the same contents
    rewards, masks, value_preds = ro.rewards.clone().unsqueeze(2), ro.masks.clone().unsqueeze(2), ro.value_preds.clone().unsqueeze(2)
    features, returns, psi_returns = ro.features.clone(), torch.zeros(T + 1, N, 1, device=dev), torch.zeros(T + 1, N, 2, device=dev)
    sides = {
        "gae": (lambda: ro.compute_returns(nv, True, gamma, tau), lambda: torch_gae(rewards, value_preds, masks, returns, nv.unsqueeze(1), gamma, tau),
                lambda: torch.equal(ro.returns[:-1], returns[:-1, :, 0])),
        "discounted": (lambda: ro.compute_returns(nv, False, gamma, tau), lambda: torch_discounted(rewards, masks, returns, nv.unsqueeze(1), gamma),
                       lambda: torch.equal(ro.returns, returns[:, :, 0])),
        "psi": (lambda: ro.compute_psi_returns(npsi, gamma), lambda: torch_psi(features, masks, psi_returns, npsi, gamma),
                lambda: torch.equal(ro.psi_returns, psi_returns)),
    }
    out = {}
    for mode, (ours, theirs, equal) in sides.items():
        k_ms, t_ms = [], []
        for r in range(args.reps + 3):
            for side in ((0, 1) if r % 2 == 0 else (1, 0)):   # alternate which side goes first
                (k_ms if side == 0 else t_ms).append(timed(torch, ours if side == 0 else theirs)[0])
        k, t = stats(k_ms[3:]), stats(t_ms[3:])
        bytes_ = SCAN_BYTES * T * N
        out[mode] = {"kernel": k, "torch_loop": t, "equal": bool(equal()), "kernel_launches": 1, "torch_eager_ops": TORCH_OPS_PER_STEP[mode] * T,
                     "algorithmic_bytes": bytes_, "kernel_gb_per_s": bytes_ / (k["median_ms"] * 1e-3) / 1e9, "copy_rate_gb_per_s": COPY_TBPS * 1e3,
                     "speedup_median": t["median_ms"] / k["median_ms"]}
    # ---- (iii) the small columns of one minibatch
    ro.compute_returns(nv, True, gamma, tau)
    adv = ro.advantages.clone()
    rng = np.random.default_rng(T)
    flat = {"actions": ro.actions.view(-1, 1), "returns": ro.returns[:-1].view(-1, 1), "masks": ro.masks[:-1].view(-1, 1),
            "log_probs": ro.action_log_probs.view(-1, 1), "adv": adv.view(-1, 1), "values": ro.value_preds[:-1].view(-1, 1)}
    cols, act = torch.empty(5, B, device=dev), torch.empty(B, dtype=torch.int64, device=dev)
    ptr = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
    g_ms, i_ms, same = [], [], True
    for r in range(args.reps + 3):
        idx = torch.from_numpy(rng.integers(0, T * N, B)).to(dev)
        for side in ((0, 1) if r % 2 == 0 else (1, 0)):
            if side == 0:
                g_ms.append(timed(torch, lambda: b.L.mwb_rollout_gather_cols(b.h, ptr(idx), B, ptr(adv), ptr(cols), ptr(act), b._stream()))[0])
            else:
                ms, six = timed(torch, lambda: [v[idx] for v in flat.values()])
                i_ms.append(ms)
        same = same and torch.equal(act, six[0][:, 0]) and all(torch.equal(cols[j], six[k][:, 0]) for j, k in ((0, 1), (4, 2), (2, 3), (3, 4), (1, 5)))
    g, i = stats(g_ms[3:]), stats(i_ms[3:])
    out["gather_cols"] = {"kernel": g, "torch_six_index_calls": i, "equal": bool(same), "rows": B, "kernel_launches": 1, "torch_eager_ops": 6,
                          "algorithmic_bytes": 64 * B, "kernel_gb_per_s": 64 * B / (g["median_ms"] * 1e-3) / 1e9, "speedup_median": i["median_ms"] / g["median_ms"]}
    res["T%d" % T] = out
    b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--steps", type=int, nargs="+", default=[16, 128])
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    res = {"envs": args.envs, "batch": args.batch, "device": torch.cuda.get_device_name(0)}
    for T in args.steps:
        one_size(torch, args, T, res)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
