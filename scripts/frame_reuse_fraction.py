"""Share of a workload's frames that the step passes take from the last-frame cache instead of rendering them, over the
timed window of a default bench.py run (the same seeds, action stream, warm-up and step count).

    python scripts/frame_reuse_fraction.py [workload ...]        (on the GPU box, from the repo root)"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import torch
    import bench
    from gym_miniworld_amd.batch import BatchedMiniWorld
    steps, warmup = 300, 50
    for wl in sys.argv[1:] or ["maze8192"]:
        spec = bench.WORKLOADS[wl]
        env_id, n, depth, dr = spec[:4]
        n_actions = spec[5] if len(spec) > 5 else 3
        env = BatchedMiniWorld(env_id, num_envs=n, seed=1, domain_rand=dr, want_depth=depth)
        actions = bench.make_actions(steps + warmup, 0, n, torch.device("cuda", 0), n_actions)
        env.reset()
        for t in range(warmup):
            env.step(actions[t])
        env.frame_reuse_stats()
        for t in range(warmup, warmup + steps):
            env.step(actions[t])
        reused, rendered = env.frame_reuse_stats()
        print(json.dumps({"workload": wl, "steps": steps, "warmup": warmup, "frames_reused": reused, "frames_rendered": rendered,
                          "reuse_fraction": reused / max(1, reused + rendered)}))
        env.close()


if __name__ == "__main__":
    main()
