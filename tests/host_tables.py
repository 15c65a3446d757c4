"""The two host programs around the library's task table (csrc/mwb_task_table.h) and per-env array list (csrc/mwb_internal.h),
built on first use, and the figures the tests that run them share."""
import collections
import functools
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "gym_miniworld_amd", "csrc")
MWB_EINVAL = -1

Facts = collections.namedtuple("Facts", "n_boxes R_max S_max max_episode_steps n_tex no_ceiling poly room_words frame_words ent_task "
                                        "agent_radius task_args")
Array = collections.namedtuple("Array", "name minor rows per type_size elems_src elems_dst copied")
Copy = collections.namedtuple("Copy", "rows elem src_stride dst_stride")

# bytes of state mwb_copy_envs moves per env and the arrays it moves them in, measured on the commit before the array list
# existed (its mwb_for_each_env_array): task -> (task_args, copied arrays, bytes per env)
COPIED = {
    "Hallway": ([], 27, 3020), "OneRoom": ([], 27, 3020), "SimToRealGoTo": ([], 27, 3020), "FourRooms": ([], 27, 4588),
    "Maze": ([8, 8, 3], 27, 23180), "TMaze": ([], 27, 3244), "TMazeTwoBox": ([], 27, 3308), "SimToRealPush": ([], 27, 3084),
    "PutNext": ([], 27, 3340), "YMaze": ([], 27, 4812), "PickupObjs": ([12, 5], 38, 3524), "RoomObjs": ([], 38, 3340),
    "CollectHealth": ([], 38, 4720), "ThreeRooms": ([], 38, 4928), "Sign": ([], 38, 5020), "Sidewalk": ([], 38, 5020),
    "WallGap": ([], 38, 4560),
}


@functools.lru_cache(None)
def _exe(name, hip_headers):
    out = os.path.join(HERE, "_build")
    os.makedirs(out, exist_ok=True)
    exe, src = os.path.join(out, name), os.path.join(HERE, name + ".cpp")
    deps = [src, os.path.join(CSRC, "mwb_task_table.h"), os.path.join(CSRC, "mwb_internal.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in deps):
        flags = ["-D__HIP_PLATFORM_AMD__", "-I", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")] if hip_headers else []
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", CSRC] + flags + ["-o", exe, src])
    return exe


def _run(exe, *args):
    return subprocess.run([exe] + [repr(float(a)) if isinstance(a, float) else str(a) for a in args], check=True, capture_output=True,
                          text=True).stdout.splitlines()


def rows():
    """The C table's rows in order: [(task id, name, [mesh geometry ids])]"""
    out = []
    for ln in _run(_exe("task_table_host", False), "rows"):
        f = ln.split()
        assert len(f) == 3 + int(f[2])
        out.append((int(f[0]), f[1], [int(g) for g in f[3:]]))
    return out


def resolve(task_id, task_args=(), max_episode_steps=0):
    """mwb_resolve_task -> Facts, or (return code, message) where it refuses"""
    ta = [float(a) for a in (list(task_args) + [0, 0, 0, 0])[:4]]
    rc, rest = _run(_exe("task_table_host", False), "resolve", task_id, *ta, int(max_episode_steps))[0].split(" | ", 1)
    if int(rc):
        return int(rc), rest
    f = rest.split()
    return Facts(*[int(v) for v in f[:10]], float(f[10]), [float(v) for v in f[11:15]])


def arrays(task_id, task_args=(), n_src=3, n_dst=3, want_depth=0, frame_reuse=1):
    """The per-env array list for two handles of that task: ([Array ...] as mwb_create allocates, [Copy ...] as mwb_copy_envs moves)"""
    ta = [float(a) for a in (list(task_args) + [0, 0, 0, 0])[:4]]
    arr, cop = [], []
    for ln in _run(_exe("env_arrays_host", True), task_id, *ta, n_src, n_dst, want_depth, frame_reuse):
        f = ln.split()
        if f[0] == "array":
            arr.append(Array(f[1], *[int(v) for v in f[2:]]))
        else:
            cop.append(Copy(*[int(v) for v in f[1:]]))
    return arr, cop
