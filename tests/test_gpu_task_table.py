"""GPU: the library as built resolves tasks and lists its per-env arrays as the host programs of tests/test_task_table_host.py
and tests/test_env_arrays_host.py do.  Creation only: the handles are unseeded and never reset or rendered, as archive() builds
its sibling.  (A copy between handles of different N and every task stepped against the oracle are run by the suite already.)"""
import pytest

import host_tables as HT

pytestmark = pytest.mark.gpu


def test_handles_hold_what_the_host_tables_say():
    from gym_miniworld_amd import ENV_SPECS, _lib
    from gym_miniworld_amd.batch import BatchedMiniWorld
    ids = {}
    for env_id, spec in ENV_SPECS.items():   # the first registered id of each task
        ids.setdefault(spec[0], env_id)
    assert set(ids) == set(_lib.TASK_IDS) == set(HT.COPIED)
    for task, env_id in ids.items():
        _, args, steps, _, _ = ENV_SPECS[env_id]
        want = HT.resolve(_lib.TASK_IDS[task], args, steps)
        per_env = sum(c.rows * c.elem for c in HT.arrays(_lib.TASK_IDS[task], args)[1])
        b =BatchedMiniWorld(env_id, num_envs=3, _assets=False)
        try:
            assert (b.n_boxes, b.max_episode_steps) == (want.n_boxes, want.max_episode_steps), env_id
            assert b.agent_radius == want.agent_radius, env_id
            assert int(b.L.mwb_copy_env_bytes(b.h, b.h)) == per_env == HT.COPIED[task][2], env_id
        finally:
            b.close()
