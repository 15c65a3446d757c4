"""GPU: terminal observations and the cause of an episode's end (mwb_terminal_enable / BatchedMiniWorld.terminal_enable /
MiniWorldVecEnv(terminal_obs=K)).

The reference for the frames is the CPU oracle stepped WITHOUT auto-reset, reset by the test at `done` (as repeat_on_oracle in
test_gpu_step_repeat.py does): its frame at `done` is what the VecEnv worker overwrites (vec_env/subproc_vec_env.py:10-13).  The
reference for the cause is the oracle's step counter (miniworld.py:708-711) and, in the box tasks, its reward: a task rule that ends
the episode there pays a reward that is not zero.  Frames within the project's +-1 per channel; everything else bit for bit."""
import numpy as np
import pytest

from test_gpu_parity import obs_diff

pytestmark = pytest.mark.gpu

CLOCK, TASK = 1, 2


def make(env_id, n, seed=900, **kw):
    from gym_miniworld_amd.batch import BatchedMiniWorld
    return BatchedMiniWorld(env_id, num_envs=n, seed=seed, **kw)


def hwc(frame, layout):
    """a frame of the batch as [H, W, 3] (TransposeImage is obs.transpose(2, 1, 0), envs.py:106-107)"""
    return frame if layout == "HWC" else frame.transpose(2, 1, 0)


# ------------------------------------------------------------------------------- 1. frames against the oracle, and the twin
@pytest.mark.parametrize("env_id,task,targs,W,H,layout", [
    ("MiniWorld-Hallway-v0", "Hallway", None, 80, 60, "HWC"),
    ("MiniWorld-Hallway-v0", "Hallway", None, 80, 60, "CWH"),
    ("MiniWorld-Hallway-v0", "Hallway", None, 9, 7, "HWC"),      # W*H % 16 != 0, a frame of 189 bytes
    ("MiniWorld-TMazeTwoBoxDynamic-v0", "TMazeTwoBox", [0, 0, 0, 100], 80, 60, "HWC"),
    ("MiniWorld-TMazeTwoBoxDynamic-v0", "TMazeTwoBox", [0, 0, 0, 100], 9, 7, "CWH"),
])
def test_terminal_frames_against_the_oracle_and_the_twin(oracle_mod, env_id, task, targs, W, H, layout):
    """Random actions over three time-limit cycles: at every done frames[e] is the oracle's frame at done, obs[e] the reset
    frame, cause what the oracle's counter and reward say; a no_auto_reset twin shows, at each env's first done, an observation
    bit-equal to frames[e]; rows (no stack: single uint8 frames) are the frames of the ranked envs"""
    import torch
    n, mes, seed = 7, 6, 900
    kw = dict(max_episode_steps=mes, obs_width=W, obs_height=H, layout=layout)
    b = make(env_id, n, seed, **kw)
    term = b.terminal_enable()
    twin = make(env_id, n, seed, auto_reset=False, **kw)
    envs = [oracle_mod.OracleEnv(task, seed=seed + i, task_args=targs, max_episode_steps=mes, obs_width=W, obs_height=H) for i in range(n)]
    b.reset()
    twin.reset()
    for e in envs:
        e.reset(render=False)
    assert int(term.count[0]) == 0 and (term.row_of == -1).all() and (term.cause == 0).all()
    rng = np.random.default_rng(11)
    first_done = np.zeros(n, bool)
    seen = dict(done=0, clock=0, task=0, twin=0)
    for t in range(3 * mes + 1):
        a = rng.choice(3, size=n, p=[0.25, 0.25, 0.5]).astype(np.int32)
        b.step(torch.from_numpy(a))
        twin.step(torch.from_numpy(a))
        done, cause = b.done.cpu().numpy().astype(bool), term.cause.cpu().numpy()
        frames, obs, tobs = term.frames.cpu().numpy(), b.obs.cpu().numpy(), twin.obs.cpu().numpy()
        row_of, row_env, count = term.row_of.cpu().numpy(), term.row_env.cpu().numpy(), int(term.count[0])
        rows = term.rows.cpu().numpy()
        assert count == done.sum() and (row_env[:count] == np.flatnonzero(done)).all() and (row_env[count:] == -1).all(), (t, count)
        for i, e in enumerate(envs):
            _, r, d, _ = e.step(int(a[i]))
            assert d == done[i], (t, i)
            want = (CLOCK if e.state().step_count >= mes else 0) | (TASK if d and r != 0 else 0) if d else 0
            assert cause[i] == want, (t, i, cause[i], want, r)
            if not first_done[i]:   # up to the first done the twin is the same env
                if d:
                    assert np.array_equal(tobs[i], frames[i]), (t, i, "twin")
                    seen["twin"] += 1
                else:
                    assert np.array_equal(tobs[i], obs[i]), (t, i, "twin before done")
            if not d:
                assert row_of[i] == -1
                continue
            first_done[i] = True
            seen["done"] += 1
            seen["clock"] += bool(want & CLOCK)
            seen["task"] += bool(want & TASK)
            diff = obs_diff(hwc(frames[i], layout), e.render_obs())
            assert diff.max() <= 1, (t, i, "terminal frame", int(diff.max()), int((diff > 1).sum()))
            assert np.array_equal(rows[row_of[i]], frames[i]), (t, i, "row")
            e.reset(render=False)
            diff = obs_diff(hwc(obs[i], layout), e.render_obs())
            assert diff.max() <= 1, (t, i, "reset frame", int(diff.max()))
    assert seen["clock"] >= n and seen["done"] >= 3 * n and seen["twin"] == n, seen
    assert term.dropped() == 0
    b.check()
    b.close()
    twin.close()


def test_pickupobjs_last_pick_up_is_still_in_the_terminal_frame(oracle_mod):
    """a pick-up on the episode's last step: the rule removes the object after the reference has rendered the frame
    (pickupobjs.py:56-69), so the terminal frame shows it; reward 1 and not the last object - the clock alone ended the episode"""
    import torch
    n, mes, seed = 5, 6, 910
    b = make("MiniWorld-PickupObjs-v0", n, seed, max_episode_steps=mes)
    term = b.terminal_enable()
    envs = [oracle_mod.OracleEnv("PickupObjs", seed=seed + i, task_args=[12, 5, 0, 0], max_episode_steps=mes) for i in range(n)]
    b.reset()
    for e in envs:
        e.reset(render=False)
    b.set_state(0, carrying=np.zeros(n, np.int32), step_count=np.full(n, mes - 1, np.int32))
    for e in envs:
        e.set_carrying(0)
        e.set_step_count(mes - 1)
    a = np.zeros(n, np.int32)   # turn: the carried object follows, then the rule collects it
    b.step(torch.from_numpy(a))
    rew, done = b.reward64.cpu().numpy(), b.done.cpu().numpy()
    frames, cause = term.frames.cpu().numpy(), term.cause.cpu().numpy()
    for i, e in enumerate(envs):
        _, r, d, _ = e.step(0)
        assert r == rew[i] == 1.0 and d and done[i], (i, r, rew[i], d)
        assert cause[i] == CLOCK, (i, cause[i])
        diff = obs_diff(frames[i], e.render_obs(step_frame=True))
        assert diff.max() <= 1, (i, int(diff.max()), int((diff > 1).sum()))
    assert any(obs_diff(e.render_obs(step_frame=True), e.render_obs(step_frame=False)).max() > 1 for e in envs)   # the object is in view somewhere
    b.check()
    b.close()


# ------------------------------------------------------------------------------------------------- 2. nothing else moves
@pytest.mark.parametrize("stack", [None, "float32"])
def test_the_feature_changes_nothing_else(stack):
    import torch
    n, mes = 7, 6
    pair = []
    for on in (True, False):
        b = make("MiniWorld-Hallway-v0", n, 920, max_episode_steps=mes, layout="CWH")
        st = b.stack_enable(4, stack, fused=True) if stack else None
        if on:
            b.terminal_enable(3)
        b.reset()
        pair.append((b, st))
    rng = np.random.default_rng(3)
    (x, _), (y, _) = pair
    reused = 0
    for t in range(3 * mes + 2):
        a = torch.from_numpy(rng.choice(3, size=n, p=[0.2, 0.2, 0.6]).astype(np.int32))
        mask = None
        if t == 4:   # a skip-masked step as well
            mask = torch.tensor([0, 1, 0, 0, 1, 0, 0], dtype=torch.uint8)
        for b, _ in pair:
            b.step(a, skip_mask=mask)
        for name in ("obs", "reward64", "done", "ep_steps", "reward"):
            assert torch.equal(getattr(x, name), getattr(y, name)), (t, name)
        if stack:
            assert torch.equal(x.stack_update(), y.stack_update()), (t, "stack")
        sx, sy = x.get_state(rng_state=True), y.get_state(rng_state=True)
        for k in sx:
            assert np.array_equal(sx[k], sy[k]), (t, k)
        fx, fy = x.frame_reuse_stats(), y.frame_reuse_stats()
        assert fx == fy, (t, fx, fy)
        reused += fx[0]
        if mask is not None:
            assert (x.terminal.cause.cpu().numpy()[[1, 4]] == 0).all()
    assert x.terminal.dropped() > 0   # mass time-outs of 7 envs into 3 rows
    x.close()
    y.close()


# --------------------------------------------------------------------------------------------------------- 3. cause, directed
def place_at_box(b, envs, which, dist):
    """the agents of envs `which` at `dist` metres from their box (along +x), in the batch and in the oracle (None: batch only)"""
    st = b.get_state()
    for i in which:
        x, z = st["box_pos"][i][0] + dist, st["box_pos"][i][2]
        if dist > 5:   # "far": the end of the corridor (x in -1 .. 11, hallway.py) that is at least 5 m from the box
            x = 0.0 if st["box_pos"][i][0] > 5 else 10.0
        b.set_agent(i, pos_xz=np.array([[x, z]]), dir=np.array([st["agent_dir"][i]]))
        if envs is not None:
            envs[i].set_agent(float(x), float(z), float(st["agent_dir"][i]))


def test_cause_of_the_box_tasks_directed(oracle_mod):
    """Hallway, a turn in place: far from the box at max - 1 -> 1; next to the box early -> 2; next to the box at max - 1 -> 3; a
    skip-masked env -> 0; an env that goes on -> 0.  The oracle confirms the rewards and dones the byte is read beside."""
    import torch
    n, mes, seed = 6, 20, 930
    b = make("MiniWorld-Hallway-v0", n, seed, max_episode_steps=mes)
    term = b.terminal_enable()
    envs = [oracle_mod.OracleEnv("Hallway", seed=seed + i, max_episode_steps=mes) for i in range(n)]
    b.reset()
    for e in envs:
        e.reset(render=False)
    place_at_box(b, envs, [0, 1, 5], 30.0)   # far
    place_at_box(b, envs, [2, 3, 4], 0.7)    # inside near()'s threshold: 0.4 + the box's radius + 1.1 * 0.15 > 0.7
    for i in (0, 3, 4):
        b.set_agent(i, step_count=np.array([mes - 1], np.int32))
        envs[i].set_step_count(mes - 1)
    mask = torch.tensor([0, 0, 0, 0, 1, 0], dtype=torch.uint8)
    b.step(torch.zeros(n, dtype=torch.int32), skip_mask=mask)
    rew, done, cause = b.reward64.cpu().numpy(), b.done.cpu().numpy(), term.cause.cpu().numpy()
    for i, e in enumerate(envs):
        if i == 4:
            continue
        _, r, d, _ = e.step(0)
        assert r == rew[i] and d == bool(done[i]), (i, r, rew[i], d, done[i])
    assert cause.tolist() == [CLOCK, 0, TASK, CLOCK | TASK, 0, 0], cause.tolist()
    assert rew[0] == 0 and rew[2] > 0 and rew[3] > 0 and rew[4] == -99.0 and done.tolist() == [1, 0, 1, 1, 0, 0]
    assert term.truncated.tolist() == [True, False, False, False, False, False]
    assert term.terminated.tolist() == [False, False, True, True, False, False]
    assert term.row_of.tolist() == [0, -1, 1, 2, -1, -1] and int(term.count[0]) == 3
    b.reset(torch.tensor([1, 0, 0, 0, 0, 0], dtype=torch.uint8))   # a pass that is no step: nothing terminal is left
    assert int(term.count[0]) == 0 and (term.row_of == -1).all() and (term.cause == 0).all() and (term.row_env == -1).all()
    b.close()


def test_cause_of_the_entity_tasks_directed(oracle_mod):
    """Sidewalk's street ends the episode with reward 0 early -> 2; CollectHealth's death -> 2"""
    import torch
    n, seed = 3, 940
    b = make("MiniWorld-Sidewalk-v0", n, seed)
    term = b.terminal_enable()
    envs = [oracle_mod.OracleEnv("Sidewalk", seed=seed + i) for i in range(n)]
    b.reset()
    for e in envs:
        e.reset(render=False)
    st = b.get_state()
    for i in (0, 2):   # onto the street (0, 6) x (-80, 80), sidewalk.py:74-87
        b.set_agent(i, pos_xz=np.array([[3.0, st["agent_pos"][i][2]]]))
        envs[i].set_agent(3.0, float(st["agent_pos"][i][2]), float(st["agent_dir"][i]))
    b.step(torch.zeros(n, dtype=torch.int32))
    rew, done, cause = b.reward64.cpu().numpy(), b.done.cpu().numpy(), term.cause.cpu().numpy()
    for i, e in enumerate(envs):
        _, r, d, _ = e.step(0)
        assert r == rew[i] and d == bool(done[i]), (i, r, rew[i], d, done[i])
    assert done.tolist() == [1, 0, 1] and rew.tolist() == [0.0, 0.0, 0.0] and cause.tolist() == [TASK, 0, TASK], (done, rew, cause)
    diff = obs_diff(term.frames.cpu().numpy()[2], envs[2].render_obs(step_frame=True))
    assert diff.max() <= 1, int(diff.max())
    b.close()

    b = make("MiniWorld-CollectHealth-v0", n, seed)
    term = b.terminal_enable()
    b.reset()
    b.set_state(0, task_f=np.array([2.0, 50.0, 1.0]))   # health falls by 2 a step (collecthealth.py:51-77)
    b.step(torch.zeros(n, dtype=torch.int32))
    assert b.done.tolist() == [1, 0, 1] and b.reward64.tolist() == [-100.0, 2.0, -100.0]
    assert term.cause.tolist() == [TASK, 0, TASK]
    b.close()


def test_step_repeat_keeps_the_sub_steps_cause_and_frame(oracle_mod):
    """k = 4 with max_episode_steps = 6: the second call ends every env at its sub-step 2 - taken = 2, the clock's cause, and the
    frame of that sub-step (the later launches leave a frozen env alone)"""
    import torch
    n, mes, seed = 7, 6, 950
    b = make("MiniWorld-Hallway-v0", n, seed, max_episode_steps=mes)
    term = b.terminal_enable()
    envs = [oracle_mod.OracleEnv("Hallway", seed=seed + i, max_episode_steps=mes) for i in range(n)]
    b.reset()
    for e in envs:
        e.reset(render=False)
    place_at_box(b, envs, range(n), 30.0)   # nobody reaches the box
    a = np.array([0, 1, 0, 1, 0, 1, 0], np.int32)
    for call in range(2):
        b.step_repeat(torch.from_numpy(a), 4)
        if call == 0:
            assert (term.cause == 0).all() and int(term.count[0]) == 0
            for i, e in enumerate(envs):
                for _ in range(4):
                    e.step(int(a[i]))
    assert b.taken.tolist() == [2] * n and b.done.tolist() == [1] * n and term.cause.tolist() == [CLOCK] * n
    frames = term.frames.cpu().numpy()
    for i, e in enumerate(envs):
        for _ in range(2):
            _, _, d, _ = e.step(int(a[i]))
        assert d
        diff = obs_diff(frames[i], e.render_obs())
        assert diff.max() <= 1, (i, int(diff.max()))
    b.close()


# ------------------------------------------------------------------------------------------------------- 4. stacked rows
@pytest.mark.parametrize("dtype,grey,W,H", [("float32", False, 80, 60), ("uint8", False, 80, 60), ("float32", True, 80, 60),
                                            ("float32", False, 10, 6), ("float32", True, 10, 6)])   # 10 x 6: W*H % 16 != 0, 4-byte units
def test_stacked_rows_are_the_previous_observation_and_the_terminal_frame(dtype, grey, W, H):
    """rows[row_of[e]] == cat(prev_obs[e, cpf:], frame_e) bit for bit: episodes of every length from 1 step (two zero groups and
    the reset frame) upwards, over a run that passes the fused window's slide (8 slack frames: every 9th step) several times"""
    import torch
    n, mes, nstack = 7, 5, 4
    cpf = 1 if grey else 3
    b = make("MiniWorld-Hallway-v0", n, 960, max_episode_steps=mes, layout="CWH", greyscale=grey, obs_width=W, obs_height=H)
    b.stack_enable(nstack, dtype, fused=True, grey=grey)
    term = b.terminal_enable(n)
    assert tuple(term.rows.shape) == (n, nstack * cpf, W, H) and term.rows.dtype == getattr(torch, dtype)
    b.reset()
    b.set_agent(0, step_count=np.array([0, 4, 3, 2, 1, 0, 4], np.int32))   # the first episodes end after 5, 1, 2, 3, 4, 5, 1 steps
    prev = b.stack_update(after_reset=True).clone()
    rng = np.random.default_rng(8)
    checked, zero_groups, slides, last_first = 0, set(), 0, 0
    for t in range(30):
        b.step(torch.from_numpy(rng.choice(3, size=n, p=[0.3, 0.3, 0.4]).astype(np.int32)))
        obs = b.stack_update()
        first = obs.storage_offset() // (W * H) % (nstack * cpf + cpf * 8)
        slides += first < last_first
        last_first = first
        done, row_of = b.done.cpu().numpy(), term.row_of.cpu().numpy()
        for e in np.flatnonzero(done):
            frame = term.grey[e] if grey else term.frames[e].to(getattr(torch, dtype))
            want = torch.cat([prev[e, cpf:], frame])
            got = term.rows[int(row_of[e])]
            assert got.dtype == want.dtype and torch.equal(got, want), (t, int(e))
            zero_groups.add(sum(int((want[g * cpf:(g + 1) * cpf] == 0).all()) for g in range(nstack - 1)))
            checked += 1
            # the observation returned for the env is the new episode's: history zeroed, as before
            assert (obs[e, :(nstack - 1) * cpf] == 0).all()
        prev = obs.clone()
    assert checked >= 5 * n and zero_groups == {0, 1, 2} and slides >= 2, (checked, zero_groups, slides)
    b.close()


def test_non_fused_stacks_and_late_calls_are_refused():
    from gym_miniworld_amd._lib import MwbError
    b = make("MiniWorld-Hallway-v0", 3, layout="CWH")
    b.stack_enable(4, "float32", fused=False)
    with pytest.raises(ValueError, match="not the fused one"):
        b.terminal_enable()
    assert b.L.mwb_terminal_enable(b.h, 3, 0) == -1 and b"MWB_STACK_FUSED" in b.L.mwb_last_error()
    b.close()
    b = make("MiniWorld-Hallway-v0", 3, layout="CWH")
    b.terminal_enable(2)
    with pytest.raises(ValueError, match="after terminal_enable"):
        b.stack_enable(4, "float32", fused=False)
    assert b.L.mwb_stack_enable(b.h, 4, 1) != 0 and b"fused frame stack only" in b.L.mwb_last_error()
    with pytest.raises(ValueError, match="already enabled"):
        b.terminal_enable(2)
    b.close()
    b = make("MiniWorld-Hallway-v0", 3)
    b.reset()
    with pytest.raises(MwbError, match="before the first"):
        b.terminal_enable()
    b.close()
    b = make("MiniWorld-Hallway-v0", 3, auto_reset=False)
    with pytest.raises(ValueError, match="auto_reset=False"):
        b.terminal_enable()
    assert b.L.mwb_terminal_enable(b.h, 3, 0) == -1 and b"no_auto_reset" in b.L.mwb_last_error()
    assert b.L.mwb_terminal_enable(b.h, 4, 0) == -1
    b.close()


# ---------------------------------------------------------------------------------------------------- 5. mass time-out
@pytest.mark.parametrize("capacity", [1030, 100])
def test_mass_time_out(capacity):
    """N = 1030 (past one tile of the ranking kernel), 8 x 6 frames, max_episode_steps = 3: every env ends at step 3"""
    import torch
    n = 1030
    b = make("MiniWorld-Hallway-v0", n, 970, max_episode_steps=3, obs_width=8, obs_height=6)
    ref = make("MiniWorld-Hallway-v0", n, 970, max_episode_steps=3, obs_width=8, obs_height=6, auto_reset=False)
    term = b.terminal_enable(capacity)
    b.reset()
    ref.reset()
    box = b.get_state()["box_pos"]   # every agent to the end of the corridor that is 5 m or more from its box: only the clock ends episodes
    pos = np.stack([np.where(box[:, 0] > 5, 0.0, 10.0), box[:, 2]], axis=1)
    b.set_agent(0, pos_xz=pos)
    ref.set_agent(0, pos_xz=pos)
    a = torch.zeros(n, dtype=torch.int32)
    for t in range(3):
        b.step(a)
        ref.step(a)
        if t < 2:
            assert int(term.count[0]) == 0 and (term.row_of == -1).all()
    assert int(term.count[0]) == n and (b.done == 1).all() and (term.cause == CLOCK).all()
    ar = torch.arange(n, dtype=torch.int32, device=b.device)
    assert torch.equal(term.row_env, ar[:capacity])
    assert torch.equal(term.row_of[:capacity], ar[:capacity]) and (term.row_of[capacity:] == -1).all()
    assert torch.equal(term.frames, ref.obs)                     # complete for all N, whatever the capacity
    assert torch.equal(term.rows, term.frames[:capacity])
    assert term.dropped() == n - capacity and term.dropped() == 0
    b.close()
    ref.close()


# ------------------------------------------------------------------------------------------------------------- 6. VecEnv
def test_vec_env_infos_rollout_and_monitor():
    import torch
    from gym_miniworld_amd.vec_env import MiniWorldVecEnv, make_vec_envs
    with pytest.raises(ValueError, match="graph=True"):
        MiniWorldVecEnv("MiniWorld-Hallway-v0", 4, terminal_obs=4, graph=True)
    with pytest.raises(ValueError, match="outside 1"):
        MiniWorldVecEnv("MiniWorld-Hallway-v0", 4, terminal_obs=5)
    n, mes = 5, 4
    envs = make_vec_envs("MiniWorld-Hallway-v0", 980, n, device="cuda:0", max_episode_steps=mes, terminal_obs=3, rollout_steps=8, monitor=10)
    plain = make_vec_envs("MiniWorld-Hallway-v0", 980, n, device="cuda:0", max_episode_steps=mes, rollout_steps=8, monitor=10)
    obs, pobs = envs.reset(), plain.reset()
    assert torch.equal(obs, pobs)
    prev = obs.clone()
    for t in range(mes):
        a = torch.full((n, 1), t % 3, dtype=torch.int64, device=envs.device)
        obs, rew, done, infos = envs.step(a)
        pobs, prew, pdone, pinfos = plain.step(a)
        assert torch.equal(obs, pobs) and torch.equal(rew, prew) and (done == pdone).all()
        assert torch.equal(envs.rollout.rewards, plain.rollout.rewards)
        if t < mes - 1:
            assert not done.any() and not infos.truncated.any() and (infos.terminal_row == -1).all()
            assert all("TimeLimit.truncated" not in infos[i] and "terminal_observation" not in infos[i] for i in range(n))
            prev = obs.clone()
    assert done.all() and infos.truncated.all() and not infos.terminated.any()
    assert infos.terminal_row.tolist() == [0, 1, 2, -1, -1]
    for i in range(n):
        info = infos[i]
        assert info["TimeLimit.truncated"] is True and "episode" in info and info["feature"].tolist() == [0, 0]
        if i < 3:
            tob = info["terminal_observation"]
            assert tob.shape == obs.shape[1:] and tob.dtype == obs.dtype and tob.device == obs.device
            assert torch.equal(tob, envs.terminal.rows[i])
            assert torch.equal(tob, torch.cat([prev[i, 3:], envs.terminal.frames[i].float()]))
        else:
            assert "terminal_observation" not in info
    assert envs.terminal.dropped() == 2
    assert envs.monitor.read()[0] == plain.monitor.read()[0] == n
    envs.close()
    plain.close()


# ---------------------------------------------------------------------------------------------------------- 7. bootstrap
@pytest.mark.parametrize("frame_skip", [1, 4])
def test_bootstrap_truncated(frame_skip):
    """rewards[t] after bootstrap_truncated == rewards + G[k] * v in torch float32 at the clock-only rows, untouched elsewhere:
    an env that reached the box on its last step (cause 3), an env whose row was dropped, an env that goes on.  With
    frame_skip = 4 env 0 ends at sub-step 2 of the last call (k = 2), the others at sub-step 4 (k = 4)"""
    import torch
    n, mes, gamma, cap = 7, 8, 0.97, 5
    b = make("MiniWorld-Hallway-v0", n, 990, max_episode_steps=mes, layout="CWH")
    term = b.terminal_enable(cap)
    ro = b.rollout_enable(8, nstack=1, learner=True)
    with pytest.raises(ValueError, match="finite"):
        ro.bootstrap_truncated(torch.zeros(cap, device=b.device), float("nan"))
    b.reset()
    ro.push(after_reset=True)
    st = b.get_state()
    place_at_box(b, None, range(n), 30.0)   # nobody reaches a box
    start = np.zeros(n, np.int32)
    start[4] = -3                      # env 4 is in the middle of its episode when the others end
    start[0] = 2 if frame_skip == 4 else 0
    b.set_agent(0, step_count=start)
    a = torch.zeros(n, dtype=torch.int32)
    calls = mes // frame_skip
    for c in range(calls):
        if c == calls - 1:             # env 2 stands next to its box on its last step: the rule AND the clock
            b.set_agent(2, pos_xz=np.array([[st["box_pos"][2][0] + 0.7, st["box_pos"][2][2]]]), step_count=np.array([mes - 1], np.int32))
        if frame_skip == 1:
            b.step(a)
        else:
            b.step_repeat(a, frame_skip)
        ro.push()
    t = ro.step - 1
    cause, row_of, taken = term.cause.cpu(), term.row_of.cpu(), ro.taken[t].cpu()
    assert cause.tolist() == [CLOCK, CLOCK, CLOCK | TASK, CLOCK, 0, CLOCK, CLOCK] and row_of.tolist() == [0, 1, 2, 3, -1, 4, -1], (cause, row_of)
    assert taken.tolist() == ([1] * n if frame_skip == 1 else [2, 4, 1, 4, 4, 4, 4]), taken.tolist()
    before, earlier = ro.rewards[t].clone(), ro.rewards[:t].clone()
    v = torch.linspace(0.5, 2.5, cap, device=b.device)
    ro.bootstrap_truncated(v, gamma)
    want = before.clone()
    for e in (0, 1, 3, 5):             # the clock-only rows
        g = 1.0
        for _ in range(int(taken[e])):
            g = g * gamma                                               # float64, by repeated multiplication (mwb_returns_scan.h)
        G = torch.tensor(g, dtype=torch.float32, device=b.device)       # rounded to float32 once
        want[e] = before[e] + G * v[int(row_of[e])]
        assert want[e] != before[e]
    assert torch.equal(ro.rewards[t], want), (ro.rewards[t].tolist(), want.tolist())
    assert torch.equal(ro.rewards[:t], earlier) and term.dropped() == 1
    b.close()
