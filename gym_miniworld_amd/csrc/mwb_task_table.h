// mwb_task_table.h - what a task IS, as the library needs it: one row per MWB_TASK_* and the one function that turns an
// mwb_config into the facts mwb_create copies into MwbDev.  Host only, nothing of HIP: tests/task_table_host.cpp builds it with a
// plain C++ compiler.  A new task is one new row (and, where its facts hang on its arguments, one line in mwb_resolve_task);
// what only Python needs of a task (action count, info fields, mesh heights) is the table in gym_miniworld_amd/tasks.py, and
// tests/test_task_table_host.py holds the two together.
#pragma once
#include <string>

#include "../../include/miniworld_batch.h"

#define MWB_TASK_MAX_MESHES 3

struct MwbTaskRow {
    int task;                // MWB_TASK_*: the row's own index (checked below)
    const char *name;        // the task's name in Python (_lib.TASK_IDS)
    double args[4];          // the class defaults a 0 in mwb_config.task_args stands for
    int n_boxes;             // boxes, or entity slots in the entity tasks; 0: PickupObjs' num_objs
    int R_max, S_max;        // capacity of an env's room table / collision segment list; 0: from Maze's rows x cols
    int max_episode_steps;   // the class default; 0: Maze's rows x cols x 24 (maze.py:27)
    int n_tex;               // leading texture slots the task can draw
    int no_ceiling;          // its rooms have no ceiling
    int poly;                // its rooms are general convex polygons
    double agent_radius;
    int n_meshes, meshes[MWB_TASK_MAX_MESHES];   // the geometries (MWB_MESH_*) its entities use
    const char *size_msg;    // the message when task_args[0] (a room's size / length) is below 2; null: no such argument
};

#define MWB_TEX_ROOMS 7   // the plain navigation tasks' textures
#define MWB_TEX_RINK 17   // + the sim-to-real rinks' choices
inline constexpr MwbTaskRow MWB_TASK_TABLE[] = {
    //                                                    args          boxes  R   S  steps         n_tex          noceil poly radius meshes
    {MWB_TASK_HALLWAY, "Hallway",             {12, 0, 0, 0},   1, 1,  4,  250, MWB_TEX_ROOMS, 0, 0, 0.4, 0, {}, "Hallway: length >= 2"},   // hallway.py:18
    {MWB_TASK_ONEROOM, "OneRoom",             {10, 0, 0, 0},   1, 1,  4,  180, MWB_TEX_ROOMS, 0, 0, 0.4, 0, {}, "OneRoom: size >= 2"},     // oneroom.py:14
    {MWB_TASK_FOURROOMS, "FourRooms",         {0, 0, 0, 0},    1, 8, 32,  250, MWB_TEX_ROOMS, 0, 0, 0.4, 0, {}, nullptr},                  // fourrooms.py:15
    {MWB_TASK_MAZE, "Maze",                   {8, 8, 3, 0},    1, 0,  0,    0, MWB_TEX_ROOMS, 0, 0, 0.4, 0, {}, nullptr},                  // maze.py:27
    {MWB_TASK_TMAZE, "TMaze",                 {0, 0, 0, 0},    1, 2,  8,  280, MWB_TEX_ROOMS, 0, 0, 0.4, 0, {}, nullptr},                  // tmaze.py:20
    {MWB_TASK_TMAZE_TWOBOX, "TMazeTwoBox",    {0, 0, 0, 100},  2, 2,  8,  280, MWB_TEX_ROOMS, 0, 0, 0.4, 0, {}, nullptr},                  // tmaze.py:142; box 0 red, box 1 blue
    {MWB_TASK_SIM2REAL_GOTO, "SimToRealGoTo", {0, 0, 0, 0},    1, 1,  4,  100, MWB_TEX_RINK, 1, 0, 0.11, 0, {}, nullptr},                  // simtorealgoto.py:30, radius :50
    {MWB_TASK_SIM2REAL_PUSH, "SimToRealPush", {0, 0, 0, 0},    2, 1,  4,  150, MWB_TEX_RINK, 1, 0, 0.11, 0, {}, nullptr},                  // simtorealpush.py:29; red, yellow
    {MWB_TASK_PUTNEXT, "PutNext",             {12, 0, 0, 0},   6, 1,  4,  250, MWB_TEX_ROOMS, 0, 0, 0.4, 0, {}, "PutNext: size >= 2"},     // putnext.py:16; COLOR_NAMES order
    // corridor, hub, two arms, two connectors (the third pair of portals meets directly)
    {MWB_TASK_YMAZE, "YMaze",                 {0, 0, 0, 0},    1, 6, 24,  280, MWB_TEX_ROOMS, 0, 1, 0.4, 0, {}, nullptr},                  // ymaze.py:21
    // ---- the entity tasks: every row from here on has a general entity list (n_boxes = its slots)
    {MWB_TASK_PICKUPOBJS, "PickupObjs",       {12, 5, 0, 0},   0, 1,  4,  400, MWB_TEX_CHAR0, 1, 0, 0.4, 2, {MWB_MESH_BALL, MWB_MESH_KEY}, "size >= 2"},   // pickupobjs.py:19
    {MWB_TASK_ROOMOBJS, "RoomObjs",           {10, 0, 0, 0},   3, 1,  4,  2147483647, MWB_TEX_CHAR0, 1, 0, 1.5, 2, {MWB_MESH_BALL, MWB_MESH_KEY}, "size >= 2"},   // roomobjs.py:19: math.inf, radius :36
    {MWB_TASK_COLLECTHEALTH, "CollectHealth", {16, 0, 0, 0},  18, 1,  4, 1000, MWB_TEX_CHAR0, 0, 0, 0.4, 1, {MWB_MESH_MEDKIT}, "size >= 2"},   // collecthealth.py:24
    {MWB_TASK_THREEROOMS, "ThreeRooms",       {0, 0, 0, 0},    6, 8, 24,  400, MWB_TEX_CHAR0, 0, 0, 0.4, 3, {MWB_MESH_DUCKIE, MWB_MESH_KEY, MWB_MESH_BALL}, nullptr},   // threerooms.py:14
    {MWB_TASK_SIGN, "Sign",                   {10, 0, 0, 0},   7, 8, 24,   20, MWB_NUM_TEXTURES, 0, 0, 0.4, 1, {MWB_MESH_KEY}, nullptr},   // sign.py:41; + the characters of its words
    {MWB_TASK_SIDEWALK, "Sidewalk",           {0, 0, 0, 0},    7, 8, 24,  150, MWB_TEX_CHAR0, 1, 0, 0.4, 2, {MWB_MESH_BUILDING, MWB_MESH_CONE}, nullptr},   // sidewalk.py:15
    {MWB_TASK_WALLGAP, "WallGap",             {0, 0, 0, 0},    2, 8, 24,  300, MWB_TEX_CHAR0, 1, 0, 0.4, 1, {MWB_MESH_BUILDING}, nullptr},   // wallgap.py:14
};   // agent_radius 0.4: entity.py:451
static_assert(sizeof(MWB_TASK_TABLE) / sizeof(MWB_TASK_TABLE[0]) == MWB_NUM_TASKS, "one row per MWB_TASK_*");
constexpr bool mwb_task_rows_in_enum_order() {
    for (int i = 0; i < MWB_NUM_TASKS; i++)
        if (MWB_TASK_TABLE[i].task != i) return false;
    return true;
}
static_assert(mwb_task_rows_in_enum_order(), "row i describes task i");

// words of an env's frame constants with n box / entity blocks.  mwb_internal.h lays them out (MWB_FRAME_WORDS_FOR, which the
// kernels use); restated because this header stays free of HIP, and mwb_api.hip asserts that the two agree
constexpr int mwb_task_frame_words(int n) { return (36 + 34 * n + 3) & ~3; }

// a task with its arguments applied: what mwb_create copies into MwbDev
struct MwbTaskFacts {
    double task_args[4];   // defaults filled in
    int ent_task;          // the task has a general entity list
    int n_boxes, R_max, S_max, max_episode_steps, n_tex, no_ceiling, poly;
    int room_words;        // f32 words per room: MWB_ROOM_WORDS or MWB_POLY_ROOM_WORDS
    int frame_words;       // the entity render kernels are compiled for every slot: MWB_MAX_ENTS blocks there
    double agent_radius;
};

// Fills *out from cfg's task, task_args and max_episode_steps; MWB_OK, or MWB_EINVAL with *err set and *out unspecified.
static inline int mwb_resolve_task(const mwb_config &cfg, MwbTaskFacts *out, std::string *err) {
    auto bad = [&](const char *msg) { *err = msg; return (int)MWB_EINVAL; };
    if (cfg.task < 0 || cfg.task >= MWB_NUM_TASKS) return bad("mwb_create: unknown task");
    const MwbTaskRow &row = MWB_TASK_TABLE[cfg.task];
    MwbTaskFacts &t = *out;
    double *a = t.task_args;
    for (int i = 0; i < 4; i++) a[i] = cfg.task_args[i] != 0 ? cfg.task_args[i] : row.args[i];
    t.ent_task = cfg.task >= MWB_TASK_PICKUPOBJS ? 1 : 0;
    t.n_boxes = row.n_boxes; t.R_max = row.R_max; t.S_max = row.S_max; t.max_episode_steps = row.max_episode_steps;
    t.n_tex = row.n_tex; t.no_ceiling = row.no_ceiling; t.poly = row.poly; t.agent_radius = row.agent_radius;
    switch (cfg.task) {
    case MWB_TASK_PICKUPOBJS:
        if (!(a[1] >= 1 && a[1] <= MWB_MAX_ENTS) || a[1] != (double)(int)a[1]) return bad("PickupObjs: num_objs must be 1 .. 20");
        t.n_boxes = (int)a[1];
        break;
    case MWB_TASK_TMAZE: case MWB_TASK_TMAZE_TWOBOX:
        if (a[3] < 0 || a[3] > 9e15) return bad("TMaze: bad sub_task_length");
        break;
    case MWB_TASK_SIGN:   // the objects sit at fixed coordinates (sign.py:91-102): only the default room fits them
        if (a[0] != 10 || a[1] < 0 || a[1] > 2 || a[2] < 0 || a[2] > 1 || a[1] != (double)(int)a[1] || a[2] != (double)(int)a[2])
            return bad("Sign: size must be 10, color_index 0..2, goal 0..1");
        break;
    case MWB_TASK_MAZE: {
        if (!(a[0] > -1 && a[0] < 4097 && a[1] > -1 && a[1] < 4097)) return bad("Maze: bad num_rows / num_cols");   // (no cast overflows below)
        const int rows = (int)a[0], cols = (int)a[1];
        if (rows < 1 || cols < 1 || rows * cols > 4096) return bad("Maze: bad num_rows / num_cols");
        t.R_max = 2 * rows * cols - 1;
        t.S_max = 4 * rows * cols < 8 ? 8 : 4 * rows * cols;
        t.max_episode_steps = rows * cols * 24;
        break;
    }
    }
    if (row.size_msg && !(a[0] >= 2)) return bad(row.size_msg);
    if (cfg.max_episode_steps > 0) t.max_episode_steps = cfg.max_episode_steps;
    t.room_words = t.poly ? MWB_POLY_ROOM_WORDS : MWB_ROOM_WORDS;
    t.frame_words = mwb_task_frame_words(t.ent_task ? MWB_MAX_ENTS : t.n_boxes);
    return MWB_OK;
}
