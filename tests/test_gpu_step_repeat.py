"""GPU: action repeat on the device (mwb_step_repeat / BatchedMiniWorld.step_repeat / MiniWorldVecEnv(frame_skip=k)).

The reference is the frame-skip loop a trainer wraps around env.step inside the VecEnv worker, driven on the CPU oracle:
    total = 0.0
    for _ in range(n_i): obs, r, done, info = env.step(a); total += r
                         if done: break
reward64, done, ep_steps and taken are exact at every call; the whole state (RNG position and key sum included) bit for bit every
5 calls; frames within +-1 and depth within 1e-4 m every 5 calls and at every call where an env finished (its frame is the new
episode's first).  Batches of 70 envs: two blocks of the step kernels, the second partial.  Every test asserts the paths it is
there for were reached."""
import math

import numpy as np
import pytest

from test_gpu_ents import assert_state_equal as assert_ents_state_equal
from test_gpu_ents import policy_action as collect_action
from test_gpu_frame_reuse import assert_twins_equal, forward_heavy_actions, make_twins, pose, scribble
from test_gpu_parity import assert_state_equal, obs_diff
from test_gpu_putnext import assert_putnext_state_equal, fetch_action
from test_gpu_sim2real import assert_rink_state_equal, params_of, push_action
from test_gpu_tmaze import assert_tmaze_state_equal, seek_action

pytestmark = pytest.mark.gpu

N = 70


def repeat_on_oracle(envs, acts, k, counts=None, auto_reset=True):
    """the wrapper loop on every oracle env.  Per env: (total, taken, done, state after the last sub-step - read before the
    auto-reset -, the sub-step (0-based) at which the entity list last changed or -1)"""
    out = []
    for i, e in enumerate(envs):
        n_i = k if counts is None else min(max(int(counts[i]), 1), k)
        total, taken, done, changed_at = 0.0, 0, False, -1
        for j in range(n_i):
            before = list(e.state().order)
            _, r, done, _ = e.step(int(acts[i]))
            total += r
            taken += 1
            if list(e.state().order) != before:
                changed_at = j
            if done:
                break
        s = e.state()
        out.append((total, taken, done, s, changed_at))
        if done and auto_reset:
            e.reset(render=False)
    return out


def check_frames(b, envs, which, step_frame, tag, depth):
    obs = b.obs.cpu().numpy()
    dep = b.depth.cpu().numpy()[..., 0] if depth else None
    for i in which:
        if depth:
            ref, refd = envs[i].render_obs(depth=True, step_frame=step_frame(i))
            assert np.abs(dep[i] - refd).max() <= 1e-4, (tag, i, "depth", float(np.abs(dep[i] - refd).max()))
        else:
            ref = envs[i].render_obs(step_frame=step_frame(i))
        d = obs_diff(obs[i], ref)
        assert d.max() <= 1, (tag, i, int(d.max()), int((d > 1).sum()))


def drive(b, envs, k, calls, policy, state_check, depth=False, ents=False, counts_fn=None, per_call=None, frame_envs=None, pick_cap=10 ** 9):
    """`calls` repeat calls of the batch `b` beside the oracle envs; returns what was reached.  frame_envs: the envs whose frames
    the periodic check compares (default all); pick_cap: how many frames after a pick-up in the last / in an earlier sub-step are
    compared (the oracle takes a third of a second for a frame with a ball in it)"""
    import torch
    seen = dict(rule_early=0, timeout_early=0, done_last=0, done=0, full=0, last_pick=0, early_pick=0, positive=0, negative=0, short_count=0)
    for t in range(calls):
        sts = [e.state() for e in envs]
        acts = np.array([policy(i, s) for i, s in enumerate(sts)], dtype=np.int32)
        counts = None if counts_fn is None else counts_fn(t)
        b.step_repeat(torch.from_numpy(acts), k, counts=None if counts is None else torch.from_numpy(counts))
        rew, done, eps, taken = b.reward64.cpu().numpy(), b.done.cpu().numpy(), b.ep_steps.cpu().numpy(), b.taken.cpu().numpy()
        res = repeat_on_oracle(envs, acts, k, counts)
        frames = set(range(len(envs)) if frame_envs is None else frame_envs) if t % 5 == 4 else set()
        fresh = set()
        for i, (total, n_taken, d, s, changed_at) in enumerate(res):
            tag = (t, i, int(acts[i]), total, rew[i], n_taken, taken[i], d, done[i])
            assert total == rew[i] and np.float64(total).tobytes() == rew[i].tobytes(), tag
            assert d == bool(done[i]) and s.step_count == eps[i] and n_taken == taken[i], tag
            n_i = k if counts is None else min(max(int(counts[i]), 1), k)
            timed_out = d and s.step_count >= s.max_episode_steps
            seen["done"] += d
            seen["rule_early"] += d and not timed_out and n_taken < n_i
            seen["timeout_early"] += timed_out and n_taken < n_i
            seen["done_last"] += d and n_taken == n_i and n_i > 1
            seen["full"] += (not d) and n_taken == k
            seen["short_count"] += (not d) and n_taken < k
            seen["positive"] += total > 0
            seen["negative"] += total < 0
            if d:
                frames.add(i)
                fresh.add(i)
            elif ents and changed_at >= 0:
                kind = "last_pick" if changed_at == n_taken - 1 else "early_pick"
                if seen[kind] < pick_cap:
                    frames.add(i)
                seen[kind] += 1
        if per_call is not None:
            per_call(t, res, sts)
        if frames:   # a finished env shows the first frame of its new episode, everybody else the last sub-step's own frame
            check_frames(b, envs, sorted(frames), lambda i: ents and i not in fresh, ("call", t), depth)
        if t % 5 == 4 or t == calls - 1:
            state_check(b.get_state(), envs, "call %d" % t)
    b.check()
    return seen


def parity_state(st, envs, tag):
    assert_state_equal(st, [e.state() for e in envs], tag=tag)


# ------------------------------------------------------------------------------------------- 1. against the oracle
def test_hallway_time_limit_between_sub_steps(oracle_mod):
    """k = 4, max_episode_steps = 10: every episode ends by the time limit in the call's second sub-step"""
    from gym_miniworld_amd.batch import BatchedMiniWorld
    b = BatchedMiniWorld("MiniWorld-Hallway-v0", num_envs=N, seed=600, max_episode_steps=10)
    envs = [oracle_mod.OracleEnv("Hallway", seed=600 + i, max_episode_steps=10) for i in range(N)]
    b.reset()
    for e in envs:
        e.reset(render=False)
    rng = np.random.default_rng(2)
    seen = drive(b, envs, 4, 30, lambda i, s: int(forward_heavy_actions(rng, 1)[0]), parity_state)
    assert seen["timeout_early"] >= N and seen["full"] > N, seen   # 10 is no multiple of 4
    b.close()


def test_maze_domain_rand_depth(oracle_mod):
    from gym_miniworld_amd.batch import BatchedMiniWorld
    b = BatchedMiniWorld("MiniWorld-MazeS3-v0", num_envs=N, seed=610, domain_rand=True, want_depth=True)
    envs = [oracle_mod.OracleEnv("Maze", seed=610 + i, domain_rand=True, task_args=[3, 3, 3]) for i in range(N)]
    b.reset()
    for e in envs:
        e.reset(render=False)
    rng = np.random.default_rng(3)

    def seek_box(i, s):   # towards the box as the crow flies (walls permitting), some noise: a 3 x 3 maze is small enough to get there
        if rng.random() < 0.25:
            return int(rng.integers(0, 3))
        want = math.atan2(-(s.box_pos[2] - s.agent_pos[2]), s.box_pos[0] - s.agent_pos[0])
        diff = (want - s.agent_dir + math.pi) % (2 * math.pi) - math.pi
        return 2 if abs(diff) < math.radians(20) else (0 if diff > 0 else 1)
    seen = drive(b, envs, 3, 35, seek_box, parity_state, depth=True)
    assert seen["done"] > 0 and seen["full"] > 0, seen
    b.close()


def test_simtorealpush_rng_follows_the_pushes(oracle_mod):
    from gym_miniworld_amd.batch import BatchedMiniWorld
    b = BatchedMiniWorld("MiniWorld-SimToRealPush-v0", num_envs=N, seed=620)
    envs = [oracle_mod.OracleEnv("SimToRealPush", seed=620 + i, domain_rand=True, params=params_of("SimToRealPush")) for i in range(N)]
    b.reset()
    for e in envs:
        e.reset(render=False)
    rng = np.random.default_rng(4)
    pushes = [0]

    def per_call(t, res, sts):
        pushes[0] += sum(1 for (_, _, d, s, _), s0 in zip(res, sts) if not d and (s.box_pos[0], s.box2_pos[0]) != (s0.box_pos[0], s0.box2_pos[0]))

    def policy(i, s):
        return push_action(s, rng) if i % 4 else int(rng.integers(0, 4))
    seen = drive(b, envs, 2, 40, policy, lambda st, ev, tag: assert_rink_state_equal(st, [e.state() for e in ev], tag=tag), per_call=per_call)
    assert pushes[0] > 10 and seen["full"] > 0, (pushes, seen)   # a push draws from the env's RNG: the positions checked above depend on it
    b.close()


def test_tmaze_twobox_penalty_feature_and_goal_pos_of_the_last_sub_step(oracle_mod):
    from gym_miniworld_amd.batch import BatchedMiniWorld
    args = [1, 0, 0, 9000000000000]
    b = BatchedMiniWorld("MiniWorld-TMazeTwoBoxDynamicFeaturesDebug-v0", num_envs=N, seed=630)
    envs = [oracle_mod.OracleEnv("TMazeTwoBox", seed=630 + i, task_args=args) for i in range(N)]
    b.reset()
    for e in envs:
        e.reset(render=False)
    # start the agents in the arms, a metre or two from a box, so that boxes are reached within the test's 35 calls
    for i, e in enumerate(envs):
        s = e.state()
        tgt = s.box2_pos if i % 2 else s.box_pos
        off = 0.9 + 0.035 * i
        z = tgt[2] - off if tgt[2] > 0 else tgt[2] + off
        e.set_agent(tgt[0], z, 0.0)
    b.set_agent(0, pos_xz=np.array([[e.state().agent_pos[0], e.state().agent_pos[2]] for e in envs]), dir=np.zeros(N))
    rng = np.random.default_rng(5)
    near_feature = [0]

    def policy(i, s):
        tgt = s.box2_pos if i % 2 else s.box_pos
        return seek_action(s, (tgt[0], tgt[2]), rng)

    def per_call(t, res, sts):
        feat, gpos = b.feature.cpu().numpy(), b.goal_pos.cpu().numpy()
        for i, (_, _, d, s, _) in enumerate(res):
            assert list(s.feature) == list(feat[i]), (t, i, list(s.feature), feat[i])   # info of the last sub-step taken
            gb = s.box2_pos if s.goal_idx == 1 else s.box_pos
            assert list(gb) == list(gpos[i]), (t, i)
            near_feature[0] += bool(s.feature[0] or s.feature[1])
    seen = drive(b, envs, 3, 35, policy, lambda st, ev, tag: assert_tmaze_state_equal(st, [e.state() for e in ev], True, tag=tag), per_call=per_call)
    assert seen["positive"] > 0 and seen["negative"] > 0 and near_feature[0] > 0, (seen, near_feature)
    assert seen["rule_early"] > 0 and seen["done_last"] > 0, seen   # done by the task rule before the last sub-step, and at it
    b.close()


def test_putnext_carrying_between_sub_steps(oracle_mod):
    from gym_miniworld_amd.batch import BatchedMiniWorld
    b = BatchedMiniWorld("MiniWorld-PutNext-v0", num_envs=N, seed=640)
    envs = [oracle_mod.OracleEnv("PutNext", seed=640 + i) for i in range(N)]
    b.reset()
    for e in envs:
        e.reset(render=False)
    rng = np.random.default_rng(6)
    carried = [0]

    def per_call(t, res, sts):
        carried[0] += sum(1 for r in res if r[3].carrying >= 0)
    seen = drive(b, envs, 2, 40, lambda i, s: fetch_action(s, rng), assert_putnext_state_equal, per_call=per_call)
    assert carried[0] > 20 and seen["full"] > 0, (carried, seen)
    b.close()


# ------------------------------------------------------------------------------------------- 2. entity tasks
@pytest.mark.parametrize("env_id,task,args", [("MiniWorld-PickupObjs-v0", "PickupObjs", [12, 5, 0, 0]), ("MiniWorld-CollectHealth-v0", "CollectHealth", [16, 0, 0, 0])])
def test_entity_tasks_show_the_last_sub_steps_override_only(oracle_mod, env_id, task, args):
    """k = 3: the frame after a call whose LAST sub-step picked something up still shows the entity (the reference renders before
    the task rule removes / respawns it); after a call where an EARLIER sub-step did, it does not.  One action per call: a
    pick-up succeeds in the first sub-step or in none, so the envs get per-env counts 1 .. 3 - with count 1 the first sub-step
    is the last"""
    from gym_miniworld_amd.batch import BatchedMiniWorld
    b = BatchedMiniWorld(env_id, num_envs=N, seed=650, want_depth=True)
    envs = [oracle_mod.OracleEnv(task, seed=650 + i, task_args=args) for i in range(N)]
    b.reset()
    for e in envs:
        e.reset(render=False)
    rng = np.random.default_rng(7)
    health_ok = [0]
    crng = np.random.default_rng(70)

    def per_call(t, res, sts):
        if not b.has_health:
            return
        health = b.feature.cpu().numpy()[:, 0]
        for i, (total, taken, d, s, _) in enumerate(res):
            assert health[i] == s.health, (t, i)   # info['health'] of the last sub-step
            if not d:
                assert total == 2 * taken, (t, i, total, taken)
                health_ok[0] += 1
    seen = drive(b, envs, 3, 36, lambda i, s: collect_action(s, b, rng, b.n_actions), lambda st, ev, tag: assert_ents_state_equal(b, st, ev, tag),
                 depth=True, ents=True, per_call=per_call, frame_envs=(3, 37, N - 1), pick_cap=5, counts_fn=lambda t: crng.integers(1, 4, N).astype(np.int32))
    assert seen["last_pick"] >= 5 and seen["early_pick"] >= 5, seen
    assert seen["full"] > 0 and seen["short_count"] > 0 and (health_ok[0] > 0 or not b.has_health)
    b.close()


# ------------------------------------------------------------------------------------------- 3. repeat = 1 is mwb_step
def test_repeat_1_is_step_bit_for_bit():
    import torch
    from gym_miniworld_amd.batch import BatchedMiniWorld
    a = BatchedMiniWorld("MiniWorld-Maze-v0", num_envs=N, seed=660, want_depth=True)
    b = BatchedMiniWorld("MiniWorld-Maze-v0", num_envs=N, seed=660, want_depth=True)
    a.reset(); b.reset()
    a.frame_reuse_stats(); b.frame_reuse_stats()
    rng = np.random.default_rng(8)
    reused = 0
    for t in range(40):
        acts = torch.from_numpy(forward_heavy_actions(rng, N))
        scribble(a, b)
        a.step(acts)
        b.step_repeat(acts, 1)
        assert torch.equal(a.obs, b.obs) and torch.equal(a.depth, b.depth) and torch.equal(a.pack, b.pack), t
        sa, sb = a.get_state(rng_state=True), b.get_state(rng_state=True)
        assert all(np.array_equal(sa[key], sb[key]) for key in sa), t
        fa, fb = a.frame_reuse_stats(), b.frame_reuse_stats()
        assert fa == fb and sum(fa) == N, (t, fa, fb)
        reused += fa[0]
        assert np.array_equal(b.taken.cpu().numpy(), np.ones(N, np.int32))
    assert reused > 0
    a.close(); b.close()


# ------------------------------------------------------------------------------------------- 4. k sub-steps are k steps
def test_one_repeat_call_equals_k_steps():
    import torch
    from gym_miniworld_amd.batch import BatchedMiniWorld
    n, k = 1000, 4
    rng = np.random.default_rng(9)
    a = BatchedMiniWorld("MiniWorld-Maze-v0", num_envs=n, seed=671)
    b = BatchedMiniWorld("MiniWorld-Maze-v0", num_envs=n, seed=671)
    a.reset(); b.reset()
    compared = 0
    for call in range(3):
        acts = torch.from_numpy(forward_heavy_actions(rng, n))
        a.step_repeat(acts, k)
        total = np.zeros(n)   # 0.0 + r0 + r1 + ...: the sequential float64 sum
        finished = np.zeros(n, bool)
        for j in range(k):
            b.step(acts)
            total = total + b.reward64.cpu().numpy()
            finished |= b.done.cpu().numpy() != 0
        keep = ~finished
        assert np.array_equal(a.done.cpu().numpy() != 0, finished), call
        assert np.array_equal(a.taken.cpu().numpy()[keep], np.full(int(keep.sum()), k, np.int32))
        assert a.reward64.cpu().numpy()[keep].tobytes() == total[keep].tobytes(), call
        assert torch.equal(a.obs[torch.from_numpy(keep)], b.obs[torch.from_numpy(keep)]), call
        sa, sb = a.get_state(rng_state=True), b.get_state(rng_state=True)
        for key in sa:
            assert np.array_equal(sa[key][keep], sb[key][keep]), (call, key)
        compared += int(keep.sum())
        if finished.any():   # a twin that finished mid-call has taken steps of its next episode: put the pair in step again
            idx = np.nonzero(finished)[0].astype(np.int32)
            b.copy_envs(idx, idx, src=a)
    assert compared > 2 * n
    a.close(); b.close()


# ------------------------------------------------------------------------------------------- 5. frame reuse under repeat
@pytest.mark.parametrize("env_id", ["MiniWorld-Maze-v0", "MiniWorld-PickupObjs-v0"])
def test_frame_reuse_needs_every_sub_step_unchanged(env_id):
    import torch
    k = 3
    a, b = make_twins(env_id, N, seed=680, want_depth=True)
    a.reset(); b.reset()
    a.frame_reuse_stats(); b.frame_reuse_stats()
    rng = np.random.default_rng(10)
    st = a.get_state()
    prev, prev_ents = pose(st), (st["boxes_pos"].copy(), st["task_i"].copy() if a.ent_task else None)
    total = moved_then_blocked = 0
    for t in range(40):
        acts = forward_heavy_actions(rng, N, p_forward=0.75)
        scribble(a, b)
        a.step_repeat(torch.from_numpy(acts), k); b.step_repeat(torch.from_numpy(acts), k)
        assert_twins_equal(a, b, (env_id, t))
        assert torch.equal(a.taken, b.taken)
        st = a.get_state()
        cur, cur_ents = pose(st), (st["boxes_pos"].copy(), st["task_i"].copy() if a.ent_task else None)
        done = a.done.cpu().numpy() != 0
        same_ents = (cur_ents[0] == prev_ents[0]).all(axis=(1, 2)) & (True if cur_ents[1] is None else cur_ents[1] == prev_ents[1])
        unchanged = (cur == prev).all(axis=1) & same_ents & ~done   # over the whole call, episode not regenerated
        # forward moves that covered less ground than k free sub-steps: moved first, then ran into something (no domain
        # randomisation: a free step is 0.15 m; once blocked with the same heading an agent stays blocked)
        dist = np.linalg.norm(cur.view(np.float64)[:, [0, 2]] - prev.view(np.float64)[:, [0, 2]], axis=1)
        partial = (acts == 2) & ~done & (dist > 0.1) & (dist < 0.15 * (k - 0.5))
        moved_then_blocked += int(partial.sum())
        assert not (partial & unchanged).any()
        reused, rendered = a.frame_reuse_stats()
        assert reused == int(unchanged.sum()) and reused + rendered == N, (env_id, t, reused, rendered, int(unchanged.sum()))
        assert b.frame_reuse_stats() == (0, N)
        total += reused
        prev, prev_ents = cur, cur_ents
    # those envs were rendered: the count of reused frames equals the count of envs unchanged over the whole call at every call,
    # and their frames equal the twin's, which renders everything
    assert total > 0 and moved_then_blocked > 0, (total, moved_then_blocked)
    a.close(); b.close()


# ------------------------------------------------------------------------------------------- 6. masks and counts
def test_skip_mask_takes_the_skip_path_once():
    import torch
    from gym_miniworld_amd.batch import BatchedMiniWorld
    b = BatchedMiniWorld("MiniWorld-OneRoom-v0", num_envs=N, seed=690)
    b.reset()
    b.step_repeat(torch.full((N,), 2, dtype=torch.int32), 2)
    before, obs0 = b.get_state(rng_state=True), b.obs.clone()
    mask = np.zeros(N, np.uint8)
    mask[::3] = 1
    m = mask.astype(bool)
    scribble(b)
    b.step_repeat(torch.full((N,), 2, dtype=torch.int32), 4, skip_mask=torch.from_numpy(mask))
    after = b.get_state(rng_state=True)
    assert np.array_equal(b.reward64.cpu().numpy()[m], np.full(int(m.sum()), -99.0)) and np.all(b.reward.cpu().numpy()[m] == -99.0)
    assert np.all(b.done.cpu().numpy()[m] == 0) and np.all(b.taken.cpu().numpy()[m] == 0)
    for key in before:
        assert np.array_equal(before[key][m], after[key][m]), key
    went = ~m & (b.done.cpu().numpy() == 0)   # the others took their four sub-steps (unless the box ended their episode)
    assert went.sum() > N // 2 and np.all(b.taken.cpu().numpy()[went] == 4)
    assert np.array_equal(after["step_count"][went], before["step_count"][went] + 4)
    assert torch.equal(b.obs[torch.from_numpy(m)], obs0[torch.from_numpy(m)])   # the frame on record, rewritten into the scribbled buffer
    assert np.array_equal(b.ep_steps.cpu().numpy()[m], before["step_count"][m])
    b.close()


def test_counts_per_env_against_the_oracle_and_clamped(oracle_mod):
    import torch
    from gym_miniworld_amd.batch import BatchedMiniWorld
    k = 4
    b = BatchedMiniWorld("MiniWorld-Hallway-v0", num_envs=N, seed=700, max_episode_steps=10)
    envs = [oracle_mod.OracleEnv("Hallway", seed=700 + i, max_episode_steps=10) for i in range(N)]
    b.reset()
    for e in envs:
        e.reset(render=False)
    rng = np.random.default_rng(11)
    crng = np.random.default_rng(12)

    def counts_fn(t):   # 1 .. k, and every fifth call values that must be clamped: 0, negative, k + 5
        c = crng.integers(1, k + 1, N).astype(np.int32)
        if t % 5 == 2:
            c[0::4], c[1::4], c[2::4] = 0, k + 5, -3
        return c
    seen = drive(b, envs, k, 20, lambda i, s: int(forward_heavy_actions(rng, 1)[0]), parity_state, counts_fn=counts_fn)
    assert seen["short_count"] > 0 and seen["full"] > 0 and seen["timeout_early"] > 0, seen
    b.close()
    # counts all equal to c: the same bits as repeat = c
    for c in (1, 3):
        x = BatchedMiniWorld("MiniWorld-Maze-v0", num_envs=N, seed=701, want_depth=True)
        y = BatchedMiniWorld("MiniWorld-Maze-v0", num_envs=N, seed=701, want_depth=True)
        x.reset(); y.reset()
        for t in range(6):
            acts = torch.from_numpy(forward_heavy_actions(rng, N))
            x.step_repeat(acts, k, counts=torch.full((N,), c, dtype=torch.int32))
            y.step_repeat(acts, c)
            assert torch.equal(x.obs, y.obs) and torch.equal(x.depth, y.depth) and torch.equal(x.pack, y.pack) and torch.equal(x.taken, y.taken), (c, t)
        sx, sy = x.get_state(rng_state=True), y.get_state(rng_state=True)
        assert all(np.array_equal(sx[key], sy[key]) for key in sx), c
        assert x.frame_reuse_stats() == y.frame_reuse_stats()
        x.close(); y.close()


def test_no_auto_reset_a_finished_env_stops(oracle_mod):
    import torch
    from gym_miniworld_amd.batch import BatchedMiniWorld
    k = 4
    b = BatchedMiniWorld("MiniWorld-Hallway-v0", num_envs=N, seed=710, max_episode_steps=6, auto_reset=False)
    envs = [oracle_mod.OracleEnv("Hallway", seed=710 + i, max_episode_steps=6) for i in range(N)]
    b.reset()
    for e in envs:
        e.reset(render=False)
    rng = np.random.default_rng(13)
    for t in range(2):
        acts = forward_heavy_actions(rng, N)
        b.step_repeat(torch.from_numpy(acts), k)
        res = repeat_on_oracle(envs, acts, k, auto_reset=False)
        rew, done, taken = b.reward64.cpu().numpy(), b.done.cpu().numpy(), b.taken.cpu().numpy()
        for i, (total, n_taken, d, s, _) in enumerate(res):
            assert total == rew[i] and d == bool(done[i]) and n_taken == taken[i], (t, i)
        parity_state(b.get_state(), envs, "no auto-reset, call %d" % t)   # nobody was regenerated: step_count 4, then 6
        check_frames(b, envs, range(0, N, 3), lambda i: False, ("no auto-reset", t), False)   # the last sub-step's frame
    assert (done != 0).all() and (taken == 2).all() and (b.get_state()["step_count"] == 6).all()
    b.close()


# ------------------------------------------------------------------------------------------- 7. VecEnv
@pytest.mark.parametrize("to_float,grey", [(True, False), (False, False), (True, True)])
def test_vecenv_frame_skip_with_frame_stack(to_float, grey):
    import torch
    from gym_miniworld_amd.vec_env import MiniWorldVecEnv
    from stack_ref import FrameStackRef
    kw = dict(seed=720, to_float=to_float, greyscale=grey, max_episode_steps=6, frame_skip=4)
    v = MiniWorldVecEnv("MiniWorld-OneRoom-v0", N, frame_stack=4, **kw)
    plain = MiniWorldVecEnv("MiniWorld-OneRoom-v0", N, frame_stack=0, **kw)
    c = 1 if grey else 3
    assert v.observation_space.shape == (4 * c, 80, 60) and v.frame_skip == 4
    ref = FrameStackRef(N, 4, (c, 80, 60), dtype=torch.float32 if to_float else torch.uint8)
    assert torch.equal(v.reset().cpu(), ref.reset(plain.reset().cpu()))
    g = torch.Generator().manual_seed(2)
    prev = np.zeros(N, np.int64)   # steps into the episode before the call
    seen_short = seen_full = 0
    for t in range(8):
        a = torch.randint(0, 3, (N, 1), generator=g)
        st, rew, done, infos = v.step(a)
        ob, rew2, done2, infos2 = plain.step(a)
        assert np.array_equal(done, done2) and torch.equal(rew, rew2) and np.array_equal(infos.taken, infos2.taken), t
        assert torch.equal(st.cpu(), ref.step(ob.cpu(), done)), t   # the window moves once per call and is zeroed on done
        eps = v.batch.ep_steps.cpu().numpy()
        assert np.array_equal(infos.taken, eps - prev) and np.array_equal(v.batch.taken.cpu().numpy(), infos.taken), t
        assert (infos.taken[~done] == 4).all() and infos[0]["taken"] == infos.taken[0] and infos[N - 1]["taken"] == infos.taken[N - 1]
        seen_short += int((done & (eps == 6) & (infos.taken == 2)).sum())   # the time limit, in the second sub-step of a call
        seen_full += int((~done).sum())
        prev = np.where(done, 0, eps)
        if t == 3:   # copy_envs between two calls: env 1 becomes env 0's twin in both views, window included
            v.copy_envs([1], [0])
            plain.copy_envs([1], [0])
            ref.stacked[1] = ref.stacked[0]
            prev[1] = prev[0]
    assert seen_short > N and seen_full > N
    v.close(); plain.close()


def test_vecenv_copy_then_repeat_keeps_twins_in_step():
    import torch
    from gym_miniworld_amd.vec_env import MiniWorldVecEnv
    v = MiniWorldVecEnv("MiniWorld-Maze-v0", N, seed=730, frame_stack=4, frame_skip=3)
    v.reset()
    g = torch.Generator().manual_seed(3)
    for t in range(3):
        v.step(torch.randint(0, 3, (N, 1), generator=g))
    v.copy_envs(np.arange(35, 70), np.arange(0, 35))
    for t in range(4):
        a = torch.randint(0, 3, (35, 1), generator=g)
        st, rew, done, infos = v.step(torch.cat([a, a]))
        assert torch.equal(st[:35], st[35:]) and torch.equal(rew[:35], rew[35:]) and np.array_equal(infos.taken[:35], infos.taken[35:]), t
    v.close()


def test_vecenv_graph_replay_with_frame_skip_equals_eager():
    import torch
    from gym_miniworld_amd.vec_env import MiniWorldVecEnv
    a = MiniWorldVecEnv("MiniWorld-FourRooms-v0", N, seed=740, to_float=False, graph=True, frame_skip=2, max_episode_steps=9)
    b = MiniWorldVecEnv("MiniWorld-FourRooms-v0", N, seed=740, to_float=False, graph=False, frame_skip=2, max_episode_steps=9)
    assert torch.equal(a.reset(), b.reset())
    g = torch.Generator().manual_seed(1)
    short = 0
    for t in range(12):
        act = torch.randint(0, 3, (N, 1), generator=g)
        oa, ra, da, ia = a.step(act)
        ob, rb, db, ib = b.step(act)
        assert torch.equal(oa, ob) and torch.equal(ra, rb) and np.array_equal(da, db) and np.array_equal(ia.taken, ib.taken), t
        short += int((ia.taken == 1).sum())
    assert a._graph is not None and b._graph is None and short >= N   # 9 steps: the time limit ends an episode after one sub-step
    a.close(); b.close()


def test_gym_view_frame_skip(oracle_mod):
    from gym_miniworld_amd.env import make
    env = make("MiniWorld-Hallway-v0", seed=750, frame_skip=3, max_episode_steps=7)
    e = oracle_mod.OracleEnv("Hallway", seed=750, max_episode_steps=7)
    env.reset()
    e.reset(render=False)
    for want in (3, 3, 1):
        obs, r, done, info = env.step(2)
        (total, taken, d, s, _), = repeat_on_oracle([e], [2], 3, auto_reset=False)
        assert info["taken"] == taken == want and r == total and done == d and env.step_count == s.step_count
        assert obs_diff(obs, e.render_obs()).max() <= 1
    assert done
    env.close()


# ------------------------------------------------------------------------------------------- 8. refusals
def test_repeat_out_of_range_is_refused_and_changes_nothing():
    import ctypes
    import torch
    from gym_miniworld_amd import _lib
    from gym_miniworld_amd.batch import BatchedMiniWorld
    b = BatchedMiniWorld("MiniWorld-OneRoom-v0", num_envs=N, seed=760, want_depth=True)
    b.reset()
    acts = torch.full((N,), 2, dtype=torch.int32, device=b.device)
    b.step_repeat(acts, 2)
    before, obs0, pack0, taken0 = b.get_state(rng_state=True), b.obs.clone(), b.pack.clone(), b.taken.clone()
    b.frame_reuse_stats()
    for rep in (0, -1, _lib.MAX_REPEAT + 1):
        with pytest.raises(ValueError):
            b.step_repeat(acts, rep)
        rc = b.L.mwb_step_repeat(b.h, ctypes.c_void_p(acts.data_ptr()), None, None, rep, None, b._stream())   # the ABI itself
        assert rc == -1 and b"repeat" in b.L.mwb_last_error()
    assert b.L.mwb_step_repeat(b.h, None, None, None, 2, None, b._stream()) == -1                 # no actions at all
    p = ctypes.c_void_p(acts.data_ptr())
    assert b.L.mwb_step_repeat(b.h, p, p, None, 2, None, b._stream()) == -1                        # both kinds
    after = b.get_state(rng_state=True)
    assert all(np.array_equal(before[key], after[key]) for key in before)
    assert torch.equal(b.obs, obs0) and torch.equal(b.pack, pack0) and torch.equal(b.taken, taken0) and b.frame_reuse_stats() == (0, 0)
    b.step_repeat(acts, _lib.MAX_REPEAT)   # the largest value is served
    assert int(b.taken.max()) == _lib.MAX_REPEAT or bool(b.done.any())
    b.close()
