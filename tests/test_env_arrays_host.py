"""CPU: the one list of per-env device arrays (mwb_for_each_env_array, gym_miniworld_amd/csrc/mwb_internal.h) from which
mwb_create allocates, mwb_copy_envs builds its descriptors and mwb_copy_env_bytes sums.  tests/env_arrays_host.cpp walks it for
two MwbDev filled from the task resolver, with no device: what a copy moves per task must stay what it was, and both users must
see every array's shape alike."""
import host_tables as HT
from gym_miniworld_amd import _lib

T = _lib.TASK_IDS


def test_copied_arrays_and_bytes_per_env():
    assert set(HT.COPIED) == set(T)
    for task, (args, n_arrays, n_bytes) in HT.COPIED.items():
        arr, cop = HT.arrays(T[task], args)
        assert len(cop) == n_arrays == sum(a.copied for a in arr), task
        assert sum(c.rows * c.elem for c in cop) == n_bytes, task
        # the descriptors are the copied arrays of the list, in its order
        assert [(c.rows, c.elem) for c in cop] == [(a.rows, a.per * a.type_size) for a in arr if a.copied], task


def test_shapes_that_hang_on_the_task():
    f = HT.resolve(T["Maze"], [3, 2, 3])
    by = {a.name: a for a in HT.arrays(T["Maze"], [3, 2, 3])[0]}
    assert (by["rooms"].minor, by["rooms"].per, by["rooms"].type_size) == (0, f.R_max * 24, 4)
    assert (by["segs"].minor, by["segs"].rows, by["segs"].per, by["segs"].type_size) == (1, f.S_max * 4, 1, 8)
    assert (by["rng"].minor, by["rng"].per, by["rng"].type_size) == (0, 625, 4)
    assert (by["frame"].per, by["frame"].copied) == (f.frame_words, 0)
    by = {a.name: a for a in HT.arrays(T["PutNext"])[0]}
    assert (by["box_color"].minor, by["box_color"].rows, by["box_color"].per) == (1, 6, 3) and by["box_x"].rows == 6
    assert "ent_meta" not in by
    by = {a.name: a for a in HT.arrays(T["CollectHealth"])[0]}
    assert by["ent_meta"].rows == 18 and by["ent_order"].per == 24 and by["text_tex"].per == 8 and by["ovr_pose"].per == 4
    assert {a.name: a for a in HT.arrays(T["YMaze"])[0]}["rooms"].per == 6 * 52


def test_arrays_that_hang_on_the_handle():
    names = lambda **kw: [a.name for a in HT.arrays(T["OneRoom"], **kw)[0]]   # noqa: E731
    base = names(want_depth=0, frame_reuse=0)
    assert not {"depth", "frame_cache", "depth_cache", "frame_cached", "frame_same"} & set(base)
    assert set(names(want_depth=1, frame_reuse=0)) - set(base) == {"depth"}
    assert set(names(want_depth=0, frame_reuse=1)) - set(base) == {"frame_cache", "frame_cached", "frame_same"}
    assert set(names(want_depth=1, frame_reuse=1)) - set(base) == {"depth", "frame_cache", "depth_cache", "frame_cached", "frame_same"}
    assert len(set(base)) == len(base)
    # none of them is state: a copy moves the same bytes whatever the handle keeps besides
    assert HT.arrays(T["OneRoom"], want_depth=1, frame_reuse=1)[1] == HT.arrays(T["OneRoom"], want_depth=0, frame_reuse=0)[1]


def test_handles_of_unequal_size():
    for task in ("FourRooms", "PutNext", "Sign"):
        arr, cop = HT.arrays(T[task], n_src=3, n_dst=5, want_depth=1, frame_reuse=1)
        for a in arr:   # what mwb_create asks for: N x rows x per elements, or N x count
            assert a.rows >= 1 and a.per >= 1 and (a.minor or a.rows == 1), a
            assert (a.elems_src, a.elems_dst) == (3 * a.rows * a.per, 5 * a.rows * a.per), a
        for a, c in zip([a for a in arr if a.copied], cop):
            elem = a.per * a.type_size
            assert (c.rows, c.elem) == (a.rows, elem), a
            assert (c.src_stride, c.dst_stride) == ((elem * 3, elem * 5) if a.minor else (0, 0)), a
        assert any(a.minor for a in arr if a.copied) and any(not a.minor for a in arr if a.copied)
