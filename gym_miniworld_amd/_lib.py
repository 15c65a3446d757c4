"""ctypes binding of the C ABI in include/miniworld_batch.h (libmwbatch.so, built in-tree by
`python -m gym_miniworld_amd.build` / __graft_entry__.build()).

There is deliberately no fallback: if the HIP library is missing or no GPU is present, loading or
mwb_create fails loudly.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MWB_LIB") or os.path.join(HERE, "libmwbatch.so")   # MWB_LIB: kernel A/B experiments only

NPARAM = 13
STACK_SLIDING = 16   # MWB_STACK_SLIDING
STACK_FUSED = 32     # MWB_STACK_FUSED
STACK_GREY = 64      # MWB_STACK_GREY
STACK_SLACK_FRAMES = 8   # MWB_STACK_SLACK_FRAMES
ROOM_WORDS = 24
POLY_ROOM_WORDS = 52   # MWB_TASK_YMAZE (include/miniworld_batch.h)
ABI_VERSION = 5
MT_WORDS = 625

TASK_IDS = {"Hallway": 0, "OneRoom": 1, "FourRooms": 2, "Maze": 3, "TMaze": 4, "TMazeTwoBox": 5,
            "SimToRealGoTo": 6, "SimToRealPush": 7, "PutNext": 8, "YMaze": 9,
            "PickupObjs": 10, "RoomObjs": 11, "CollectHealth": 12, "ThreeRooms": 13, "Sign": 14, "Sidewalk": 15, "WallGap": 16}
ENT_TASK_FIRST = 10      # MWB_TASK_PICKUPOBJS: the tasks with a general entity list
MAX_ENTS = 20            # MWB_MAX_ENTS
MESH_GEOMS = ["ball", "key", "medkit", "duckie", "building", "cone"]   # MWB_MESH_*
TEX_MESH0, TEX_CHAR0 = 21, 25
LAYOUT_HWC, LAYOUT_CWH = 0, 1
COPY_NO_RENDER = 1   # MWB_COPY_NO_RENDER
MAX_REPEAT = 64      # MWB_MAX_REPEAT
ROLLOUT_GREY = 1     # MWB_ROLLOUT_GREY
RETURNS_DISCOUNTED, RETURNS_GAE, RETURNS_PSI = 0, 1, 2   # MWB_RETURNS_*
MONITOR_MAX_CAPACITY, MONITOR_MAX_QUOTA = 65536, 64      # csrc/mwb_monitor_map.h
END_CLOCK, END_TASK = 1, 2   # MWB_END_*: the bits of the terminal pass's `cause`
TERMINAL_FLOAT = 1           # MWB_TERMINAL_FLOAT
LEVELS_SEQUENTIAL, LEVELS_UNIFORM, LEVELS_TABLE = 0, 1, 2   # MWB_LEVELS_*: how a level set hands out levels
LEVELS_TALLY = 1             # MWB_LEVELS_TALLY
LEVELS_MAX, LEVELS_MAX_TABLE, LEVELS_MAX_TALLY = 2 ** 31 - 1, 2 ** 24, 2 ** 22   # csrc/mwb_levels_map.h
WINDOW_MAX_OUT, WINDOW_MAX_OFFSET = 1024, 32767   # csrc/mwb_rollout_window_map.h
WINDOW_BORDER_EDGE, WINDOW_BORDER_ZERO = 0, 1


class MwbConfig(ctypes.Structure):
    _fields_ = [
        ("abi_version", ctypes.c_int32), ("task", ctypes.c_int32), ("num_envs", ctypes.c_int32),
        ("obs_width", ctypes.c_int32), ("obs_height", ctypes.c_int32), ("want_depth", ctypes.c_int32),
        ("layout", ctypes.c_int32), ("domain_rand", ctypes.c_int32), ("max_episode_steps", ctypes.c_int32),
        ("device", ctypes.c_int32), ("task_args", ctypes.c_double * 4),
        ("use_default_params", ctypes.c_int32), ("no_auto_reset", ctypes.c_int32),
        ("params", (ctypes.c_double * 9) * NPARAM),
    ]


class MwbOutputs(ctypes.Structure):
    _fields_ = [
        ("obs", ctypes.c_void_p), ("depth", ctypes.c_void_p), ("reward", ctypes.c_void_p),
        ("reward64", ctypes.c_void_p), ("done", ctypes.c_void_p), ("ep_steps", ctypes.c_void_p),
        ("obs_bytes", ctypes.c_size_t), ("depth_bytes", ctypes.c_size_t),
        ("stack", ctypes.c_void_p), ("stack_bytes", ctypes.c_size_t),
        ("feature", ctypes.c_void_p), ("goal_pos", ctypes.c_void_p),
        ("pack", ctypes.c_void_p), ("pack_bytes", ctypes.c_size_t),
    ]


# The fields of struct mwb_state in its order, each once (csrc/mwb_state_fields.h is the library's list; tests/test_state_fields_host.py
# holds the two together): name, dtype, shape after [count] ("B" = mwb_num_boxes(h) slots, "B+1" = the entity list with the
# agent), writable through mwb_set_state, exists for the entity-list tasks only.  MwbState, BatchedMiniWorld.get_state and
# set_state are derived from it.
STATE_FIELDS = [
    ("agent_pos", "f8", (3,), True, False), ("agent_dir", "f8", (), True, False),
    ("box_pos", "f8", ("B", 3), True, False), ("box_dir", "f8", ("B",), True, False), ("box_color", "f8", ("B", 3), True, False),
    ("box_size", "f8", ("B",), True, False),
    ("cam", "f8", (4,), True, False), ("sky_color", "f8", (3,), True, False), ("light_pos", "f8", (3,), True, False),
    ("light_color", "f8", (3,), True, False), ("light_ambient", "f8", (3,), True, False),
    ("step_count", "i4", (), True, False), ("rng_pos", "i4", (), False, False), ("rng_keysum", "u4", (), False, False),
    ("n_rooms", "i4", (), False, False), ("n_segs", "i4", (), False, False),
    ("goal_idx", "i4", (), True, False), ("episode_count", "i8", (), True, False), ("task_step_count", "i8", (), True, False),
    ("goal_dist", "f8", (), True, False), ("rng_state", "u4", (MT_WORDS,), True, False), ("carrying", "i4", (), True, False),
    ("ent_meta", "i4", ("B",), True, True), ("ent_radius", "f8", ("B",), False, True), ("ent_height", "f8", ("B",), False, True),
    ("ent_scale", "f8", ("B",), False, True), ("ent_order", "i4", ("B+1",), True, True),
    ("task_f", "f8", (), True, True), ("task_i", "i4", (), True, True), ("text_tex", "i4", (8,), False, True),
]


class MwbState(ctypes.Structure):
    _fields_ = [(f[0], ctypes.c_void_p) for f in STATE_FIELDS]


class MwbRolloutInfo(ctypes.Structure):   # struct mwb_rollout_info
    _fields_ = [
        ("reward", ctypes.c_void_p), ("mask", ctypes.c_void_p), ("feature", ctypes.c_void_p), ("age", ctypes.c_void_p),
        ("ring", ctypes.c_void_p),
        ("reward_bytes", ctypes.c_size_t), ("mask_bytes", ctypes.c_size_t), ("feature_bytes", ctypes.c_size_t),
        ("age_bytes", ctypes.c_size_t), ("ring_bytes", ctypes.c_size_t),
        ("num_steps", ctypes.c_int32), ("nstack", ctypes.c_int32), ("grey", ctypes.c_int32), ("cursor", ctypes.c_int32),
        ("base", ctypes.c_int32), ("pad", ctypes.c_int32),
    ]


class MwbRolloutWindow(ctypes.Structure):   # struct mwb_rollout_window
    _fields_ = [(n, ctypes.c_int32) for n in ("out_w", "out_h", "border", "dx_lo", "dx_hi", "dy_lo", "dy_hi", "pad")]


class MwbRolloutLearnerInfo(ctypes.Structure):   # struct mwb_rollout_learner_info
    _fields_ = [(n, ctypes.c_void_p) for n in ("action", "log_prob", "value", "taken", "ret", "adv", "psi_ret")] + \
               [(n + "_bytes", ctypes.c_size_t) for n in ("action", "log_prob", "value", "taken", "ret", "adv", "psi_ret")]


class MwbMonitorInfo(ctypes.Structure):   # struct mwb_monitor_info
    _fields_ = [(n, ctypes.c_void_p) for n in (
        "run_return", "last_return", "run_len", "run_calls", "last_len", "last_calls", "finished", "partial", "retired", "logged",
        "log_return", "log_len", "log_calls", "log_env", "tab_return", "tab_len", "counts", "host_pack")] + \
        [("host_pack_bytes", ctypes.c_size_t)] + [(n, ctypes.c_int32) for n in ("num_envs", "capacity", "quota_max", "pad")]


class MwbTerminalInfo(ctypes.Structure):   # struct mwb_terminal_info
    _fields_ = [(n, ctypes.c_void_p) for n in ("cause", "frames", "grey", "row_of", "row_env", "count", "rows")] + \
               [(n, ctypes.c_size_t) for n in ("frames_bytes", "grey_bytes", "rows_bytes")] + \
               [(n, ctypes.c_int32) for n in ("capacity", "rows_float", "planes", "nstack")]


class MwbLevelsInfo(ctypes.Structure):   # struct mwb_levels_info
    _fields_ = [(n, ctypes.c_void_p) for n in ("index", "prev_index", "next_level", "episode_no", "tallies", "level_seeds")] + \
               [("num_levels", ctypes.c_int64), ("start_level", ctypes.c_uint64), ("sampler_seed", ctypes.c_uint64),
                ("env_offset", ctypes.c_int64), ("env_stride", ctypes.c_int64), ("mode", ctypes.c_int32), ("flags", ctypes.c_uint32)]


class MwbMonitorCounts(ctypes.Structure):   # struct mwb_monitor_counts, as it lies on the device
    _fields_ = [("total", ctypes.c_ulonglong), ("dropped", ctypes.c_ulonglong), ("remaining", ctypes.c_uint32), ("quota", ctypes.c_uint32),
                ("last_base", ctypes.c_uint32), ("last_count", ctypes.c_uint32)]


EXPORTS = [
    "mwb_create", "mwb_destroy", "mwb_last_error", "mwb_abi_version", "mwb_set_texture", "mwb_seed", "mwb_reset",
    "mwb_step", "mwb_render", "mwb_get_outputs", "mwb_get_state", "mwb_set_agent", "mwb_intersect",
    "mwb_get_geometry", "mwb_timing_enable", "mwb_timing_read", "mwb_stack_enable", "mwb_stack_update", "mwb_stack_window", "mwb_check", "mwb_seed_key",
    "mwb_set_task_state", "mwb_set_domain_rand", "mwb_num_textures", "mwb_debug_wg_times", "mwb_set_state", "mwb_num_boxes", "mwb_room_words", "mwb_step_i64", "mwb_render_top_view", "mwb_visible_ents",
    "mwb_set_mesh", "mwb_set_mesh_dims", "mwb_render_view", "mwb_debug_counters", "mwb_frame_reuse_stats",
    "mwb_grey_enable", "mwb_grey_output", "mwb_grey_convert",
    "mwb_copy_envs", "mwb_copy_rejected", "mwb_copy_env_bytes",
    "mwb_step_repeat", "mwb_repeat_taken",
    "mwb_rollout_enable", "mwb_rollout_push", "mwb_rollout_gather", "mwb_rollout_after_update", "mwb_rollout_info", "mwb_rollout_rejected",
    "mwb_rollout_learner_enable", "mwb_rollout_learner_info", "mwb_rollout_insert", "mwb_rollout_returns", "mwb_rollout_gather_cols",
    "mwb_bulk_variant",
    "mwb_monitor_enable", "mwb_monitor_update", "mwb_monitor_clear", "mwb_monitor_quota", "mwb_monitor_info", "mwb_monitor_read",
    "mwb_terminal_enable", "mwb_terminal_info", "mwb_terminal_dropped", "mwb_rollout_bootstrap",
    "mwb_levels_enable", "mwb_levels_restart", "mwb_levels_info", "mwb_levels_rejected",
    "mwb_rollout_window_offsets", "mwb_rollout_gather_window",
]

_lib = None


class MwbError(RuntimeError):
    pass


def load():
    """Load libmwbatch.so; raises MwbError if it has not been built (no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MwbError("HIP extension %s is missing - run `python -m gym_miniworld_amd.build` "
                       "(hipcc --offload-arch=gfx950); there is no CPU fallback" % LIB_PATH)
    # PyTorch-ROCm wheels bundle their own libamdhip64; import torch first so that this library binds to
    # the SAME HIP runtime (two runtimes in one process do not see each other's devices or streams)
    import torch  # noqa: F401
    L = ctypes.CDLL(LIB_PATH)
    vp, i32 = ctypes.c_void_p, ctypes.c_int
    L.mwb_last_error.restype = ctypes.c_char_p
    L.mwb_create.argtypes = [ctypes.POINTER(MwbConfig), ctypes.POINTER(vp)]
    L.mwb_destroy.argtypes = [vp]
    L.mwb_set_texture.argtypes = [vp, i32, i32, i32, vp]
    L.mwb_set_mesh.argtypes = [vp, i32, i32, vp, vp, vp, i32, vp, vp, i32, i32, vp, vp]
    L.mwb_set_mesh_dims.argtypes = [vp, i32, ctypes.c_double, ctypes.c_double, ctypes.c_double, i32]
    L.mwb_seed.argtypes = [vp, vp]
    L.mwb_reset.argtypes = [vp, vp, vp]
    L.mwb_step.argtypes = [vp, vp, vp, vp]
    L.mwb_step_i64.argtypes = [vp, vp, vp, vp]
    L.mwb_step_repeat.argtypes = [vp, vp, vp, vp, i32, vp, vp]
    L.mwb_repeat_taken.argtypes = [vp, ctypes.POINTER(vp)]
    L.mwb_render.argtypes = [vp, vp]
    L.mwb_render_top_view.argtypes = [vp, vp, i32, i32, vp]
    L.mwb_visible_ents.argtypes = [vp, vp, vp]
    L.mwb_render_view.argtypes = [vp, vp, vp, i32, i32, vp]
    L.mwb_get_outputs.argtypes = [vp, ctypes.POINTER(MwbOutputs)]
    L.mwb_get_state.argtypes = [vp, i32, i32, ctypes.POINTER(MwbState)]
    L.mwb_set_state.argtypes = [vp, i32, i32, ctypes.POINTER(MwbState)]
    L.mwb_num_boxes.argtypes = [vp]
    L.mwb_room_words.argtypes = [vp]
    L.mwb_set_agent.argtypes = [vp, i32, i32, vp, vp, vp]
    L.mwb_set_task_state.argtypes = [vp, i32, i32, vp, vp, vp]
    L.mwb_set_domain_rand.argtypes = [vp, i32]
    L.mwb_num_textures.argtypes = [vp]
    L.mwb_debug_wg_times.argtypes = [vp, vp, i32]
    L.mwb_debug_counters.argtypes = [vp, vp, i32]
    L.mwb_frame_reuse_stats.argtypes = [vp, vp]
    L.mwb_intersect.argtypes = [vp, i32, i32, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.POINTER(i32)]
    L.mwb_get_geometry.argtypes = [vp, i32, vp, i32, vp, i32, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.mwb_timing_enable.argtypes = [vp, i32]
    L.mwb_stack_enable.argtypes = [vp, i32, i32]
    L.mwb_check.argtypes = [vp]
    L.mwb_seed_key.argtypes = [ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32)]
    L.mwb_stack_update.argtypes = [vp, i32, vp]
    L.mwb_stack_window.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.mwb_grey_enable.argtypes = [vp]
    L.mwb_grey_output.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t)]
    L.mwb_grey_convert.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp]
    L.mwb_copy_envs.argtypes = [vp, vp, vp, vp, i32, ctypes.c_uint, vp]
    L.mwb_copy_rejected.argtypes = [vp, ctypes.POINTER(ctypes.c_ulonglong)]
    L.mwb_copy_env_bytes.argtypes = [vp, vp]
    L.mwb_copy_env_bytes.restype = ctypes.c_longlong
    L.mwb_rollout_enable.argtypes = [vp, i32, i32, ctypes.c_uint]
    L.mwb_rollout_push.argtypes = [vp, i32, vp, vp]
    L.mwb_rollout_gather.argtypes = [vp, vp, i32, vp, i32, vp]
    L.mwb_rollout_after_update.argtypes = [vp, vp]
    L.mwb_rollout_info.argtypes = [vp, ctypes.POINTER(MwbRolloutInfo)]
    L.mwb_rollout_rejected.argtypes = [vp, ctypes.POINTER(ctypes.c_ulonglong)]
    L.mwb_rollout_learner_enable.argtypes = [vp]
    L.mwb_rollout_learner_info.argtypes = [vp, ctypes.POINTER(MwbRolloutLearnerInfo)]
    L.mwb_rollout_insert.argtypes = [vp, vp, vp, vp, vp, vp]
    L.mwb_rollout_returns.argtypes = [vp, i32, ctypes.c_double, ctypes.c_double, vp, vp, vp, vp]
    L.mwb_rollout_gather_cols.argtypes = [vp, vp, i32, vp, vp, vp, vp]
    L.mwb_monitor_enable.argtypes = [vp, i32, i32]
    L.mwb_monitor_update.argtypes = [vp, vp, vp, vp, vp, vp]
    L.mwb_monitor_clear.argtypes = [vp, vp, i32, vp]
    L.mwb_monitor_quota.argtypes = [vp, i32, vp]
    L.mwb_monitor_info.argtypes = [vp, ctypes.POINTER(MwbMonitorInfo)]
    L.mwb_monitor_read.argtypes = [vp, ctypes.POINTER(MwbMonitorCounts)]
    if hasattr(L, "mwb_terminal_enable"):   # (as mwb_bulk_variant below: an older library through MWB_LIB, scripts/bench_terminal.py's leg (a))
        L.mwb_terminal_enable.argtypes = [vp, i32, ctypes.c_uint]
        L.mwb_terminal_info.argtypes = [vp, ctypes.POINTER(MwbTerminalInfo)]
        L.mwb_terminal_dropped.argtypes = [vp, ctypes.POINTER(ctypes.c_ulonglong)]
        L.mwb_rollout_bootstrap.argtypes = [vp, vp, ctypes.c_double, vp]
    if hasattr(L, "mwb_levels_enable"):   # (an older library through MWB_LIB, scripts/bench_levels.py's parent leg)
        L.mwb_levels_enable.argtypes = [vp, ctypes.c_int64, ctypes.c_uint64, vp, i32, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, ctypes.c_uint]
        L.mwb_levels_restart.argtypes = [vp, i32, ctypes.c_uint64, i32, vp]
        L.mwb_levels_info.argtypes = [vp, ctypes.POINTER(MwbLevelsInfo)]
        L.mwb_levels_rejected.argtypes = [vp, ctypes.POINTER(ctypes.c_ulonglong)]
    if hasattr(L, "mwb_rollout_gather_window"):   # (an older library through MWB_LIB)
        L.mwb_rollout_window_offsets.argtypes = [vp, ctypes.POINTER(MwbRolloutWindow), ctypes.c_uint64, ctypes.c_uint64, vp, i32, vp, vp]
        L.mwb_rollout_gather_window.argtypes = [vp, vp, i32, ctypes.POINTER(MwbRolloutWindow), vp, vp, i32, vp]
    if hasattr(L, "mwb_bulk_variant"):   # (an older library loaded through MWB_LIB for a kernel A/B has none; build() checks EXPORTS)
        L.mwb_bulk_variant.argtypes = [vp]
    L.mwb_timing_read.argtypes = [vp] +[ctypes.POINTER(ctypes.c_double)] * 4 + [ctypes.POINTER(i32)]
    if L.mwb_abi_version() != ABI_VERSION:
        raise MwbError("libmwbatch.so ABI version mismatch")
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise MwbError("libmwbatch error %d: %s" % (rc, load().mwb_last_error().decode("utf8", "replace")))
