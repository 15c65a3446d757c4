"""GPU: the texel fetch (one 16-byte footprint entry per bilinear tap, gym_miniworld_amd/csrc/mwb_texture_host.h) on textures
whose pyramids are nothing like the shipped 512 x 512 images: every slot of OneRoom overridden by seeded noise of 8 x 8, 16 x 4 and
3 x 5 texels.  At 80 x 60 these frames live on the clamped top levels (l1 == l0), on levels one texel wide or high and on every wrap
case of a 2 x 2 level; a 320 x 240 view from half a metre in front of a wall is magnified down to level 0 and its border wrap.
The same images go to the oracle (its own mip chain, its own plain wrapped fetch); frames within +-1, depth within 1e-4 m as in
tests/test_gpu_parity.py."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SETS = [(8, 8), (16, 4), (3, 5)]   # (w, h)


def set_oracle_texture(O, tid, w, h, levels):
    flat = np.concatenate([lv.reshape(-1) for lv in levels]).astype(np.uint8)
    assert O.lib().mwo_set_texture(tid, w, h, len(levels), flat.ctypes.data_as(ctypes.c_void_p)) == 0


def test_small_awkward_textures_match_oracle(oracle_mod):
    import torch
    from gym_miniworld_amd import _lib
    from gym_miniworld_amd.batch import BatchedMiniWorld
    O = oracle_mod
    n, seed = 8, 11
    acts = np.random.default_rng(5).integers(0, 3, (6, n)).astype(np.int32)
    reset_frames = []
    try:
        for (w, h) in SETS:
            b = BatchedMiniWorld("MiniWorld-OneRoom-v0", num_envs=n, seed=seed, domain_rand=False, want_depth=True)
            envs = [O.OracleEnv("OneRoom", seed=seed + i) for i in range(n)]            # (loads the oracle's real textures)
            big = [O.OracleEnv("OneRoom", seed=seed + i, obs_width=320, obs_height=240) for i in range(2)]
            n_tex = b.L.mwb_num_textures(b.h)   # the slots this task uploads: floor, ceiling and wall families of the box tasks
            assert 0 < n_tex <= O.N_TEX_BASE
            rng = np.random.default_rng(100 * w + h)
            for tid in range(n_tex):
                img = np.ascontiguousarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
                _lib.check(b.L.mwb_set_texture(b.h, tid, w, h, img.ctypes.data_as(ctypes.c_void_p)))
                set_oracle_texture(O, tid, w, h, O.build_mip_chain(img))

            def check(tag):
                obs, dep = b.obs.cpu().numpy(), b.depth.cpu().numpy()[..., 0]
                for i, e in enumerate(envs):
                    ref, refd = e.render_obs(depth=True)
                    d = np.abs(obs[i].astype(np.int16) - ref.astype(np.int16))
                    print("texel fetch %dx%d %s env %d: max |d| %d, pixels off by 1: %d, depth err %.2e"
                          % (w, h, tag, i, int(d.max()), int((d == 1).sum()), float(np.abs(dep[i] - refd).max())))
                    assert d.max() <= 1, (w, h, tag, i, int(d.max()), int((d > 1).sum()))
                    assert np.abs(dep[i] - refd).max() <= 1e-4, (w, h, tag, i)

            reset_frames.append(b.reset().cpu().numpy().copy())
            for e in envs + big:
                e.reset(render=False)
            check("reset")
            # magnified: envs 0 and 1 stand 0.5 m in front of a wall (facing it, and along it), rendered at 320 x 240
            st = b.get_state()
            pos0, dir0 = np.array(st["agent_pos"])[:2, [0, 2]].astype(np.float64), np.array(st["agent_dir"])[:2].astype(np.float64)
            pos1, dir1 = np.array([[0.5, 5.0], [5.0, 9.5]]), np.array([np.pi, 0.3])
            b.set_agent(0, pos_xz=pos1, dir=dir1)
            img, dep = b.render_view(320, 240, depth=True)
            img, dep = img.cpu().numpy(), dep.cpu().numpy()[..., 0]
            for i, e in enumerate(big):
                e.set_agent(pos1[i, 0], pos1[i, 1], dir1[i])
                ref, refd = e.render_obs(depth=True)
                d = np.abs(img[i].astype(np.int16) - ref.astype(np.int16))
                print("texel fetch %dx%d view env %d: max |d| %d, pixels off by 1: %d" % (w, h, i, int(d.max()), int((d == 1).sum())))
                assert d.max() <= 1, (w, h, "view", i, int(d.max()), int((d > 1).sum()))
                assert np.abs(dep[i] - refd).max() <= 1e-4, (w, h, "view", i)
            b.set_agent(0, pos_xz=pos0, dir=dir0)
            for t in range(len(acts)):
                b.step(torch.from_numpy(acts[t]))
                done = b.done.cpu().numpy()
                for i, e in enumerate(envs):
                    _, _, dn, _ = e.step(int(acts[t, i]))
                    assert dn == bool(done[i])
                    if dn:
                        e.reset(render=False)
                if t in (1, 5):
                    check("t=%d" % t)
            b.close()
        # the frames show the textures: another set, another image (an untextured image would pass everything above)
        for k in range(1, len(SETS)):
            assert (reset_frames[0] != reset_frames[k]).mean() > 0.25, k
    finally:
        for tid, (w, h, levels) in O._tex_cache.items():
            set_oracle_texture(O, tid, w, h, levels)
