"""What a task is, as Python needs it: one row per task name.  The library's own table (csrc/mwb_task_table.h) holds what the
kernels need - capacities, textures, default arguments, the argument checks; max_episode_steps and agent_radius stand in both,
and tests/test_task_table_host.py holds the two tables together.  A new task is one new row here."""
from collections import namedtuple

# max_steps: the class default, None where it follows from the arguments (Maze)
# n_actions: action_space - Discrete(move_forward + 1) in the navigation tasks (e.g. hallway.py:23), Discrete(move_back + 1) in
#            SimToRealPush (simtorealpush.py:37), the base class' Discrete(len(Actions)) = 8 where the task does not narrow it
#            (PutNext: miniworld.py:470)
# goal_pos:  info['goal_pos'] is produced (tmaze.py:66,206, ymaze.py:92);  health: info['health'] arrives in feature[:, 0]
# meshes:    (geometry, height) pairs the task builds: Ball(size) / Key 0.35 / BigKey 0.6 (entity.py:410-434, sign.py:9-20), MeshEnt(...)
Task = namedtuple("Task", "max_steps agent_radius n_actions goal_pos health meshes", defaults=(0.4, 3, False, False, ()))

TASKS = {
    "Hallway": Task(250),                                  # hallway.py:18
    "OneRoom": Task(180),                                  # oneroom.py:14
    "FourRooms": Task(250),                                # fourrooms.py:15
    "Maze": Task(None),                                    # maze.py:27: num_rows * num_cols * 24
    "TMaze": Task(280, goal_pos=True),                     # tmaze.py:20
    "TMazeTwoBox": Task(280, goal_pos=True),               # tmaze.py:142
    "SimToRealGoTo": Task(100, agent_radius=0.11),         # simtorealgoto.py:30,50
    "SimToRealPush": Task(150, agent_radius=0.11, n_actions=4),   # simtorealpush.py:29
    "PutNext": Task(250, n_actions=8),                     # putnext.py:16
    "YMaze": Task(280, goal_pos=True),                     # ymaze.py:21
    "PickupObjs": Task(400, n_actions=5, meshes=(("ball", 0.9), ("key", 0.35))),                  # pickupobjs.py:19
    "RoomObjs": Task(2 ** 31 - 1, agent_radius=1.5, n_actions=8, meshes=(("ball", 0.9), ("key", 0.35))),   # roomobjs.py:19 (math.inf), :36
    "CollectHealth": Task(1000, n_actions=8, health=True, meshes=(("medkit", 0.40),)),            # collecthealth.py:24
    "ThreeRooms": Task(400, meshes=(("duckie", 0.25), ("key", 0.35), ("ball", 0.6))),             # threerooms.py:14
    "Sign": Task(20, n_actions=4, meshes=(("key", 0.6),)),                                        # sign.py:41
    "Sidewalk": Task(150, meshes=(("building", 30), ("cone", 0.75))),                             # sidewalk.py:15
    "WallGap": Task(300, meshes=(("building", 30),)),                                             # wallgap.py:14
}

TaskFacts = namedtuple("TaskFacts", "max_episode_steps agent_radius n_actions has_health has_features has_goal_pos meshes")


def task_facts(task, task_args=None, max_episode_steps=None):
    """The facts BatchedMiniWorld publishes about `task` with these arguments (0 / missing = the class default), without a handle."""
    row = TASKS[task]
    ta = list(task_args or []) + [0, 0, 0, 0]
    steps = max_episode_steps or row.max_steps or int(ta[0] or 8) * int(ta[1] or 8) * 24
    return TaskFacts(int(steps), row.agent_radius, row.n_actions, row.health,
                     task == "TMazeTwoBox" and ta[0] != 0,   # the *Features* classes produce info['feature'] (tmaze.py:311-318)
                     row.goal_pos, row.meshes)
