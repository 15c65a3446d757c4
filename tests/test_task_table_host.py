"""CPU: the library's task table and its resolver (gym_miniworld_amd/csrc/mwb_task_table.h), built into a small host program
(tests/task_table_host.cpp, a plain C++ compiler, no HIP).  mwb_create calls mwb_resolve_task once and copies its facts into the
handle; on a machine without a GPU mwb_create never gets that far, so the argument checks are reached here.  The same program
ties the C table to Python's (gym_miniworld_amd/tasks.py, _lib.TASK_IDS) and both to the oracle."""
import pytest

import host_tables as HT
from gym_miniworld_amd import ENV_SPECS, _lib
from gym_miniworld_amd.tasks import TASKS, task_facts

T = _lib.TASK_IDS
INT32_MAX = 2 ** 31 - 1

# with default arguments, as the library resolved them before the table existed:
# task: (n_boxes, R_max, S_max, max_episode_steps, n_tex, no_ceiling, agent_radius)
DEFAULTS = {
    "Hallway": (1, 1, 4, 250, 7, 0, 0.4), "OneRoom": (1, 1, 4, 180, 7, 0, 0.4), "FourRooms": (1, 8, 32, 250, 7, 0, 0.4),
    "Maze": (1, 127, 256, 1536, 7, 0, 0.4), "TMaze": (1, 2, 8, 280, 7, 0, 0.4), "TMazeTwoBox": (2, 2, 8, 280, 7, 0, 0.4),
    "SimToRealGoTo": (1, 1, 4, 100, 17, 1, 0.11), "SimToRealPush": (2, 1, 4, 150, 17, 1, 0.11), "PutNext": (6, 1, 4, 250, 7, 0, 0.4),
    "YMaze": (1, 6, 24, 280, 7, 0, 0.4), "PickupObjs": (5, 1, 4, 400, 25, 1, 0.4), "RoomObjs": (3, 1, 4, INT32_MAX, 25, 1, 1.5),
    "CollectHealth": (18, 1, 4, 1000, 25, 0, 0.4), "ThreeRooms": (6, 8, 24, 400, 25, 0, 0.4), "Sign": (7, 8, 24, 20, 97, 0, 0.4),
    "Sidewalk": (7, 8, 24, 150, 25, 1, 0.4), "WallGap": (2, 8, 24, 300, 25, 1, 0.4),
}
DEFAULT_ARGS = {"Hallway": [12, 0, 0, 0], "OneRoom": [10, 0, 0, 0], "Maze": [8, 8, 3, 0], "TMazeTwoBox": [0, 0, 0, 100], "PutNext": [12, 0, 0, 0],
                "PickupObjs": [12, 5, 0, 0], "RoomObjs": [10, 0, 0, 0], "CollectHealth": [16, 0, 0, 0], "Sign": [10, 0, 0, 0]}


def frame_words_for(n):   # MWB_FRAME_WORDS_FOR (csrc/mwb_internal.h): 36 fixed words, 34 per box, rounded up to 4
    return (36 + 34 * n + 3) & ~3


def test_default_facts():
    assert set(DEFAULTS) == set(T)
    for task, want in DEFAULTS.items():
        f = HT.resolve(T[task])
        assert (f.n_boxes, f.R_max, f.S_max, f.max_episode_steps, f.n_tex, f.no_ceiling, f.agent_radius) == want, task
        assert f.task_args == DEFAULT_ARGS.get(task, [0, 0, 0, 0]), task
        assert f.poly == (task == "YMaze") and f.room_words == (52 if task == "YMaze" else 24), task
        assert f.ent_task == (T[task] >= _lib.ENT_TASK_FIRST), task
        assert f.frame_words == frame_words_for(20 if f.ent_task else f.n_boxes), task


def test_argument_dependent_facts():
    f = HT.resolve(T["Maze"], [2, 2, 3])
    assert (f.R_max, f.S_max, f.max_episode_steps) == (7, 16, 96)
    f = HT.resolve(T["Maze"], [1, 1, 3])
    assert (f.R_max, f.S_max, f.max_episode_steps) == (1, 8, 24)   # S_max is raised to 8
    for n in (1, 20):
        f = HT.resolve(T["PickupObjs"], [12, n])
        assert f.n_boxes == n and f.task_args[:2] == [12, n]
        assert f.frame_words == frame_words_for(20)
    for task in T:   # an explicit limit overrides every default
        assert HT.resolve(T[task], [], 77).max_episode_steps == 77, task
    assert HT.resolve(T["Maze"], [2, 2, 3], 300).max_episode_steps == 300
    assert HT.resolve(T["PutNext"]).frame_words == frame_words_for(6)
    assert HT.resolve(T["TMazeTwoBox"]).frame_words == frame_words_for(2)
    # arguments that are given stay as given; accepted edges of the checks below
    assert HT.resolve(T["TMaze"], [1, 10, -6, 9e15]).task_args == [1, 10, -6, 9e15]
    assert HT.resolve(T["Maze"], [64, 64, 3]).R_max == 2 * 4096 - 1
    assert HT.resolve(T["Sign"], [10, 2, 1]).n_tex == 97
    assert HT.resolve(T["Hallway"], [2]).task_args[0] == 2


REJECTED = [
    ("Hallway", [1], "Hallway: length >= 2"), ("OneRoom", [1], "OneRoom: size >= 2"), ("PutNext", [1], "PutNext: size >= 2"),
    ("PickupObjs", [1], "size >= 2"), ("RoomObjs", [1], "size >= 2"), ("CollectHealth", [1], "size >= 2"),
    ("PickupObjs", [12, 21], "PickupObjs: num_objs must be 1 .. 20"), ("PickupObjs", [12, -1], "PickupObjs: num_objs must be 1 .. 20"),
    ("PickupObjs", [12, 2.5], "PickupObjs: num_objs must be 1 .. 20"),
    ("TMaze", [0, 0, 0, -1], "TMaze: bad sub_task_length"), ("TMaze", [0, 0, 0, 1e16], "TMaze: bad sub_task_length"),
    ("TMazeTwoBox", [0, 0, 0, -1], "TMaze: bad sub_task_length"), ("TMazeTwoBox", [0, 0, 0, 1e16], "TMaze: bad sub_task_length"),
    ("Maze", [-1, 8, 3], "Maze: bad num_rows / num_cols"), ("Maze", [65, 64, 3], "Maze: bad num_rows / num_cols"),
    ("Sign", [9, 0, 0], "Sign: size must be 10, color_index 0..2, goal 0..1"), ("Sign", [10, 3, 0], "Sign: size must be 10, color_index 0..2, goal 0..1"),
    ("Sign", [10, 1.5, 0], "Sign: size must be 10, color_index 0..2, goal 0..1"), ("Sign", [10, 0, 2], "Sign: size must be 10, color_index 0..2, goal 0..1"),
]


def test_rejections_keep_their_codes_and_messages():
    for task, args, msg in REJECTED:
        assert HT.resolve(T[task], args) == (HT.MWB_EINVAL, msg), (task, args)
    for bad in (-1, len(T)):
        assert HT.resolve(bad) == (HT.MWB_EINVAL, "mwb_create: unknown task")


def test_c_rows_and_python_tables_name_the_same_tasks():
    rows = HT.rows()
    assert [r[0] for r in rows] == list(range(len(rows)))
    assert {name: i for i, name, _ in rows} == T and [name for _, name, _ in rows] == sorted(T, key=T.get)
    assert set(TASKS) == set(T)
    ent_first = min(i for i, _, _ in rows if HT.resolve(i).ent_task)
    assert ent_first == _lib.ENT_TASK_FIRST and all(HT.resolve(i).ent_task == (i >= ent_first) for i, _, _ in rows)
    for _, name, geoms in rows:   # the geometries upload_meshes waits for are the ones Python registers
        assert len(set(geoms)) == len(geoms)
        assert {_lib.MESH_GEOMS[g] for g in geoms} == {g for g, _ in TASKS[name].meshes}, name


def test_every_env_id_agrees_with_the_oracle(oracle_mod):
    for env_id, (task, args, steps, params, _) in sorted(ENV_SPECS.items()):
        c = HT.resolve(T[task], args, steps)
        p = task_facts(task, args, steps)
        env = oracle_mod.OracleEnv(task, seed=1, task_args=args, max_episode_steps=steps, params=params().to_table() if params else None,
                                   textures=False)
        env.reset(render=False)   # (the oracle's agent gets its radius when a world is generated)
        o = env.state()
        assert c.max_episode_steps == p.max_episode_steps == o.max_episode_steps, env_id
        assert c.agent_radius == p.agent_radius == o.agent_radius, env_id
        assert c.n_boxes == o.n_boxes, env_id


def test_python_facts_without_a_handle():
    assert task_facts("Maze").max_episode_steps == 1536 and task_facts("Maze", [3, 3, 3]).max_episode_steps == 216
    assert task_facts("Maze", [3, 3, 3], 300).max_episode_steps == 300
    assert [task_facts(t).n_actions for t in sorted(T, key=T.get)] == [3, 3, 3, 3, 3, 3, 3, 4, 8, 3, 5, 8, 8, 3, 4, 3, 3]
    assert [t for t in T if task_facts(t).has_goal_pos] == ["TMaze", "TMazeTwoBox", "YMaze"]
    assert [t for t in T if task_facts(t).has_health] == ["CollectHealth"]
    assert task_facts("TMazeTwoBox", [1, 0, 0, 100000]).has_features and not task_facts("TMazeTwoBox", [0, 0, 0, 100]).has_features
    assert not task_facts("TMaze", [1, 10, -6, 0]).has_features
    with pytest.raises(KeyError):
        task_facts("NoSuchTask")
