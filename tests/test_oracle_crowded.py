"""CPU: the rows of tests/crowded_rows.py are as crowded as they claim - counted by the oracle itself (OracleEnv.place_stats: every
iteration of place_entity's loop, in resets and in steps), with the env counts, seeds and step scripts of
tests/test_gpu_crowded_worlds.py, every route of that file included.  A later change of seeds that turns that file into a test of
easy worlds fails here; one that leads into a world the reference never finishes fails here too, at the time limit below.

The band of a row, at domain_rand 0 and at 1: mean per reset, largest single placement and largest single reset at least half of
the figures recorded in crowded_rows.py, and at least one placement of 78 or more attempts (a whole block of the generator).
The 78-attempt condition is NOT met by the two rows named in crowded_rows.NO_TWIST_IN_ONE_PLACEMENT, where no seed reaches it;
for them a reset of 40 attempts stands in."""
import threading

import pytest

import crowded_rows as CR

LIMIT_S = 60   # the slowest script takes 3 s


def limited(fn, *args, **kw):
    """fn(*args) on a thread (the oracle's calls release the interpreter lock): place_entity of the reference has no way out of an
    impossible world, and a test that met one must fail, not hang"""
    out = []
    t = threading.Thread(target=lambda: out.append(fn(*args, **kw)), daemon=True)
    t.start()
    t.join(LIMIT_S)
    assert not t.is_alive() and out, "the oracle did not return within %d s: a world without a valid placement" % LIMIT_S
    return out[0]


def reset_stats(O, name, dr):
    envs = CR.make_oracles(O, name, dr=dr)
    for e in envs:
        for _ in range(CR.RESETS):
            e.reset(render=False)
    st = [e.place_stats() for e in envs]
    mean = sum(s["attempts"] for s in st) / sum(s["resets"] for s in st)
    return mean, max(s["max_placement"] for s in st), max(s["max_reset"] for s in st)


@pytest.mark.parametrize("dr", [0, 1])
@pytest.mark.parametrize("name", list(CR.CROWDED))
def test_resets_are_as_crowded_as_recorded(oracle_mod, name, dr):
    mean, mp, mr = limited(reset_stats, oracle_mod, name, dr)
    want_mean, want_mp, want_mr = (CR.CROWDED_DR1[name] if dr else CR.CROWDED[name][3])
    print("%s dr%d: mean per reset %.1f, largest placement %d, largest reset %d" % (name, dr, mean, mp, mr))
    assert 2 * mp >= want_mp and 2 * mr >= want_mr and 2 * mean >= want_mean, (name, dr, mean, mp, mr)
    if name not in CR.NO_TWIST_IN_ONE_PLACEMENT:
        assert mp >= 78, (name, dr, mp)
    else:
        assert mr >= 40, (name, dr, mr)   # 19 / 21 placements among up to 20 others


def test_counter_counts_and_clears(oracle_mod):
    """one env: the counts add up, `clear` zeroes them, and a default row needs next to nothing"""
    e = oracle_mod.OracleEnv("CollectHealth", seed=CR.SEED, task_args=[4, 0, 0, 0])
    e.reset(render=False)
    s = e.place_stats()
    assert s["resets"] == 1 and s["attempts"] == s["max_reset"] >= 19 and s["step_placements"] == 0 and 1 <= s["max_placement"] <= s["attempts"]
    e.reset(render=False)
    s2 = e.place_stats(clear=True)
    assert s2["resets"] == 2 and s2["attempts"] > s["attempts"] and s2["max_reset"] >= s["max_reset"]
    assert not any(e.place_stats().values())
    d = oracle_mod.OracleEnv("OneRoom", seed=CR.SEED)
    d.reset(render=False)
    assert d.place_stats()["attempts"] <= 6


def summary(envs):
    st = [e.place_stats() for e in envs]
    return (min(s["resets"] for s in st), max(s["max_placement"] for s in st), sum(s["step_placements"] for s in st),
            max(s["max_step_placement"] for s in st))


@pytest.mark.parametrize("name", list(CR.ROLLOUTS))
def test_rollouts_regenerate_and_respawn_in_crowded_worlds(oracle_mod, name):
    """the GPU rollouts' own scripts: every env regenerates its world several times; the CollectHealth rows respawn kits through
    two or more attempts (size 4: twenty or more)"""
    resets, mp, respawns, step_mp = summary(limited(CR.play_oracles, oracle_mod, name))
    print("%s: resets per env >= %d, largest placement %d, respawns %d, largest respawn %d" % (name, resets, mp, respawns, step_mp))
    assert resets >= 4, (name, resets)
    if name not in CR.NO_TWIST_IN_ONE_PLACEMENT:
        assert mp >= 78, (name, mp)
    if name.startswith("CollectHealth"):
        assert respawns >= 1 and step_mp >= (20 if name == "CollectHealth-4" else 2), (name, respawns, step_mp)


@pytest.mark.parametrize("name", CR.ROUTE_ROWS)
def test_other_routes_regenerate_crowded_worlds(oracle_mod, name):
    """step_repeat, the 60-step prefix that runs with MWB_NO_OVERLAP=1, and the first worlds of the level seeds"""
    resets, mp, _, _ = summary(limited(CR.play_repeat_oracles, oracle_mod, name))
    print("%s step_repeat: resets per env >= %d, largest placement %d" % (name, resets, mp))
    assert resets >= 4 and mp >= 78, (name, resets, mp)
    resets, mp, _, _ = summary(limited(CR.play_oracles, oracle_mod, name, steps=CR.NO_OVERLAP_STEPS))
    print("%s first %d steps: resets per env >= %d, largest placement %d" % (name, CR.NO_OVERLAP_STEPS, resets, mp))
    assert resets >= 3 and mp >= 78, (name, resets, mp)
    worlds = [e.place_stats()["max_placement"] for e in limited(CR.play_level_oracles, oracle_mod, name)]
    print("%s level worlds: largest placement of each %s" % (name, worlds))
    assert sum(w >= 78 for w in worlds) >= 2, (name, worlds)
