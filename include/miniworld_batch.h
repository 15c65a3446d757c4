/* miniworld_batch.h - C ABI of the MI355X-native batched MiniWorld stepper + renderer.
 *
 * The reference (mjsargent/gym-miniworld) is pure Python and has no FFI for this path; its
 * boundary is two Python protocols.  Each entry point below names the reference
 * interface it replaces (file:line under the reference root); the Python binding a maintainer
 * would add is shown in INTEGRATION.md and implemented in gym_miniworld_amd/batch.py.
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success or a negative
 * MWB_E* code, with a message retrievable through mwb_last_error(); no exception crosses the
 * ABI.  One handle owns the state of `num_envs` environments on one GPU; a handle is not
 * thread-safe.  Device work is enqueued on the caller's HIP stream (void* = hipStream_t) and is
 * asynchronous unless stated; outputs are library-owned device buffers that stay valid and are
 * overwritten by the next mwb_step / mwb_reset / mwb_render on the same handle.
 */
#ifndef MINIWORLD_BATCH_H
#define MINIWORLD_BATCH_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MWB_ABI_VERSION 5

enum { MWB_OK = 0, MWB_EINVAL = -1, MWB_EHIP = -2, MWB_ENOMEM = -3, MWB_ESTATE = -4 };

/* tasks: the reference env classes registered as MiniWorld-<Class>-v0 (envs/__init__.py:43-49) */
enum { MWB_TASK_HALLWAY = 0,   /* envs/hallway.py   task_args = {length}                    */
       MWB_TASK_ONEROOM = 1,   /* envs/oneroom.py   task_args = {size}                      */
       MWB_TASK_FOURROOMS = 2, /* envs/fourrooms.py task_args = {}                          */
       MWB_TASK_MAZE = 3,      /* envs/maze.py      task_args = {num_rows,num_cols,room_size} */
       /* the T-maze family, envs/tmaze.py:
        * TMaze (7-74: goal_pos None -> random arm), TMazeLeft / TMazeRight (69-75: goal_pos given),
        * TMazeDynamic (77-106: the goal alternates between (10,0,-6) and (10,0,6) every sub_task_length-th
        * reset).  task_args = {goal_pos given (0/1), goal x, goal z, sub_task_length (> 0: TMazeDynamic)} */
       MWB_TASK_TMAZE = 4,
       /* TMazeTwoBoxDynamic (108-217) and its *Features* copies (220-650): a red box at (10,0,-6), a blue box
        * at (10,0,6); reaching the goal box ends the episode with +_reward(), the other with -_reward(), and
        * goal / penalty swap by the class' rule.  task_args = {rule, -, -, sub_task_length}: rule 0 = every
        * sub_task_length-th reset (TMazeTwoBoxDynamic.reset 210-217); rule 1 = at every reset once more than
        * sub_task_length steps have been taken - the counter is never cleared, as in the reference - and
        * info['feature'] = [near(blue), near(red)] is produced (*Features*.step 299-320, reset 322-330) */
       MWB_TASK_TMAZE_TWOBOX = 5,
       /* the sim-to-real rinks, envs/simtorealgoto.py and envs/simtorealpush.py: one square room of random size
        * without ceiling (low walls, sky above), random wall / floor texture families, a robot of radius 0.11
        * and per-episode box sizes; pass their `sim_params` table (params.py sim_to_real_params) and
        * domain_rand = 1 (the classes force it).  GoTo: reach the red box (Discrete(3)).  Push: drive the red box
        * to the yellow one - a forward move first shoves any box it would touch (simtorealpush.py:109-125, with an
        * RNG draw for the box's new heading), move_back is allowed (Discrete(4)), reward 1 when the boxes are
        * within goal_dist = 1.5 (size1 + size2).  task_args = {} */
       MWB_TASK_SIM2REAL_GOTO = 6,
       MWB_TASK_SIM2REAL_PUSH = 7,
       /* envs/putnext.py: one size x size room with six boxes - COLOR_NAMES order (entity.py:18): blue, green,
        * grey, purple, red, yellow - of sizes drawn per episode; the full MiniWorldEnv action set Discrete(8) incl. pickup (4)
        * and drop (5) with the carry physics of miniworld.py:594-606,622-631,645-654,682-702 (toggle 6 and done 7 do
        * nothing); reward + done once the red box is next to the yellow one and nothing is carried.  task_args = {size} */
       MWB_TASK_PUTNEXT = 8,
       /* envs/ymaze.py:8-103 (YMaze, YMazeLeft, YMazeRight): a corridor, a triangular hub and two arms rotated by -+120
        * degrees - rooms are convex polygons with 3 or 4 arbitrary edges (the polygon room table below); reward + done
        * near the box, info['goal_pos'] = box position; Discrete(3).  task_args = {goal given (0 = random arm), goal x, goal z} */
       MWB_TASK_YMAZE = 9,
       /* ---- tasks with a general entity list: mesh entities (MeshEnt / Key / Ball, entity.py:100-146,410-434),
        * image and text frames (entity.py:148-360), entities that leave the list or re-enter it at its end.  Meshes must be
        * registered with mwb_set_mesh / mwb_set_mesh_dims before the first reset. */
       /* envs/pickupobjs.py: num_objs objects (Ball 0.9, Box 0.9 or Key of a random colour each) in a size x size yard without
        * ceiling; Discrete(5); picking an object up removes it (after the step's frame was rendered) for reward 1; done when
        * all are gone.  task_args = {size, num_objs} */
       MWB_TASK_PICKUPOBJS = 10,
       /* envs/roomobjs.py: a box, a ball and a key of random colours, agent radius 1.5, no reward, no time limit
        * (max_episode_steps = INT32_MAX); the base class' Discrete(8).  task_args = {size} */
       MWB_TASK_ROOMOBJS = 11,
       /* envs/collecthealth.py: 18 medkits; health -= 2 per step, a pickup respawns the kit at a random place (it moves to the
        * END of the entity list) and restores health to 100; reward 2 per step alive, -100 and done at health <= 0;
        * info['health'] is delivered in mwb_outputs.feature[0].  task_args = {size} */
       MWB_TASK_COLLECTHEALTH = 12,
       /* envs/threerooms.py: three rooms, two boxes, the Mila logo as an ImageFrame, a duckie, a key, a ball; no reward */
       MWB_TASK_THREEROOMS = 13,
       /* envs/sign.py: three rooms in a U, (blue, red, green) x (box, big key) at fixed places, a TextFrame naming a colour;
        * Discrete(4) where action 3 moves back AND ends the episode; touching an object ends it with +1 (the named colour and the
        * goal's shape) or -1.  task_args = {size, color_index, goal}; pass Sign's parameter table (forward_step 0.7, turn_step 45) */
       MWB_TASK_SIGN = 14,
       /* envs/sidewalk.py: a sidewalk beside a long street (no ceilings), a far building and five cones (static meshes), a red
        * box; stepping into the street ends the episode with reward 0 */
       MWB_TASK_SIDEWALK = 15,
       /* envs/wallgap.py: two yards (no ceilings) joined by a gap in a wall, a red box, the far building */
       MWB_TASK_WALLGAP = 16,
       MWB_NUM_TASKS };

/* entity kinds and mesh geometries of the general entity list */
enum { MWB_ENT_BOX = 0, MWB_ENT_MESH = 1, MWB_ENT_IMAGE = 2, MWB_ENT_TEXT = 3 };
enum { MWB_MESH_BALL = 0, MWB_MESH_KEY, MWB_MESH_MEDKIT, MWB_MESH_DUCKIE, MWB_MESH_BUILDING, MWB_MESH_CONE, MWB_NUM_MESHES };
/* mwb_state.ent_meta word: kind | geometry << 4 | static << 8 | alive << 9 | radius is a float32 scalar << 10 | (colour index + 1) << 12 */
#define MWB_META_KIND(m) ((m) & 15)
#define MWB_META_GEOM(m) (((m) >> 4) & 15)
#define MWB_META_STATIC(m) (((m) >> 8) & 1)
#define MWB_META_ALIVE(m) (((m) >> 9) & 1)
#define MWB_META_RADF32(m) (((m) >> 10) & 1)
#define MWB_MAX_ENTS 20   /* entity slots besides the agent (CollectHealth: 18) */

/* observation layouts */
enum { MWB_LAYOUT_HWC = 0,  /* [N,H,W,3]  MiniWorldEnv.observation_space, miniworld.py:473-478 */
       MWB_LAYOUT_CWH = 1 }; /* [N,3,W,H]  after TransposeImage, pytorch-a2c-ppo-acktr/envs.py:96-107 */

/* domain parameters in the order of the reference table params.py:110-123 */
enum { MWB_P_SKY_COLOR = 0, MWB_P_LIGHT_POS, MWB_P_LIGHT_COLOR, MWB_P_LIGHT_AMBIENT, MWB_P_OBJ_COLOR_BIAS,
       MWB_P_FORWARD_STEP, MWB_P_FORWARD_DRIFT, MWB_P_TURN_STEP, MWB_P_BOT_RADIUS, MWB_P_CAM_PITCH,
       MWB_P_CAM_FOV_Y, MWB_P_CAM_HEIGHT, MWB_P_CAM_FWD_DISP, MWB_NPARAM };

/* Constructor arguments: MiniWorldEnv.__init__ kwargs (miniworld.py:456-465) + the task class'
 * own kwargs + batch size / device. */
typedef struct mwb_config {
    int32_t abi_version;       /* MWB_ABI_VERSION */
    int32_t task;              /* MWB_TASK_* */
    int32_t num_envs;          /* environments owned by this handle (this GPU's shard) */
    int32_t obs_width;         /* 80  (miniworld.py:459) */
    int32_t obs_height;        /* 60  (miniworld.py:460) */
    int32_t want_depth;        /* also produce render_depth() maps (miniworld.py:1207-1220) */
    int32_t layout;            /* MWB_LAYOUT_* of the observation batch */
    int32_t domain_rand;       /* miniworld.py:464 */
    int32_t max_episode_steps; /* <= 0: the task's default (hallway.py:18, oneroom.py:14, ...) */
    int32_t device;            /* HIP device ordinal */
    double task_args[4];       /* see MWB_TASK_*; 0 = the class default */
    int32_t use_default_params; /* 1: params.py:110-123 DEFAULT_PARAMS; 0: `params` below */
    int32_t no_auto_reset;     /* 0: a finished env is reset inside mwb_step (VecEnv worker, subproc_vec_env.py:10-13);
                                  1: plain Gym semantics, the caller resets (miniworld.py:658-716) */
    double params[MWB_NPARAM][9]; /* default[3], min[3], max[3] per parameter (DomainParams.set) */
} mwb_config;

typedef struct mwb_handle mwb_handle;

/* library-owned device buffers produced by mwb_reset / mwb_step / mwb_render */
typedef struct mwb_outputs {
    uint8_t *obs;       /* u8, layout per config: [N,H,W,3] or [N,3,W,H]                         */
    float *depth;       /* f32 [N,H,W] metres (get_depth_map, opengl.py:336-371) or NULL         */
    float *reward;      /* f32 [N]  (VecPyTorch.step_wait casts to float32, envs.py:129)          */
    double *reward64;   /* f64 [N]  the reference's Python float, for bit-exact checks            */
    uint8_t *done;      /* u8  [N]                                                                */
    int32_t *ep_steps;  /* i32 [N]  step_count of the transition just taken (before auto-reset)   */
    size_t obs_bytes, depth_bytes;
    void *stack;        /* frame stack [N, nstack*3, W, H], f32 or u8 (mwb_stack_enable), or NULL              */
    size_t stack_bytes;
    float *feature;     /* f32 [N][2] info['feature'] of the transition (tmaze.py:311-318); zeros for other tasks */
    double *goal_pos;   /* f64 [N][3] info['goal_pos'] of the transition, T-maze family (tmaze.py:66,206); else zeros */
    /* reward64, goal_pos, reward, feature, ep_steps and done live in ONE allocation [pack, pack + pack_bytes) so that a
     * host-side consumer (the VecEnv contract returns numpy dones, CPU rewards and info dicts every step,
     * vec_env/subproc_vec_env.py:69-75) fetches them with a single device-to-host copy; each pointer above = pack + offset.  Order inside the allocation: done,
     * reward, feature, goal_pos, ep_steps, reward64 - a consumer that needs only the first few copies that prefix */
    void *pack;
    size_t pack_bytes;
} mwb_outputs;

/* host-side snapshot of the simulator state of a contiguous env range, for tests / debugging / checkpoints;
 * every pointer may be NULL to skip that field. B = mwb_num_boxes(h); boxes in the order of the reference's
 * entity list (hallway.py:31 one red box; tmaze.py:166-169 red, blue; simtorealpush.py:88-99 red, yellow). */
typedef struct mwb_state {
    double *agent_pos;  /* [count][3] Entity.pos (entity.py:22-24), y = 0 */
    double *agent_dir;  /* [count]    Entity.dir                          */
    double *box_pos;    /* [count][B][3]  y > 0 while the box is carried (miniworld.py:603-604) */
    double *box_dir;    /* [count][B]    */
    double *box_color;  /* [count][B][3] Box.color_vec (entity.py:381-383)   */
    double *box_size;   /* [count][B] Box.size[0] (entity.py:366-378): 0.8 unless the task draws it per episode */
    double *cam;        /* [count][4] cam_height, cam_fwd_disp, cam_pitch, cam_fov_y (entity.py:486-492) */
    double *sky_color, *light_pos, *light_color, *light_ambient; /* [count][3] (miniworld.py:561-566) */
    int32_t *step_count;    /* [count] miniworld.py:539,663 */
    int32_t *rng_pos;       /* [count] MT19937 position (RandomState.get_state()[2]); read-only */
    uint32_t *rng_keysum;   /* [count] sum of the 624 key words mod 2^32; read-only */
    int32_t *n_rooms;       /* [count] read-only */
    int32_t *n_segs;        /* [count] read-only */
    int32_t *goal_idx;      /* [count] current_goal (tmaze.py:91) / goal_box_idx (tmaze.py:135) */
    int64_t *episode_count; /* [count] tmaze.py:80,130 (1 after construction: MiniWorldEnv.__init__ resets once) */
    int64_t *task_step_count; /* [count] tmaze.py:240 */
    double *goal_dist;      /* [count] simtorealpush.py:84 */
    uint32_t *rng_state;    /* [count][625] RandomState.get_state(): the 624 key words, then the position */
    int32_t *carrying;      /* [count] agent.carrying as an index into the boxes, or -1 (miniworld.py:682-702) */
    /* general entity list (tasks >= MWB_TASK_PICKUPOBJS; B = mwb_num_boxes(h) slots = the episode's first list, agent excluded) */
    int32_t *ent_meta;      /* [count][B] see MWB_META_*; read-only */
    double *ent_radius;     /* [count][B] Entity.radius (a float32 value for meshes under NumPy >= 2); read-only */
    double *ent_height;     /* [count][B] Entity.height; read-only */
    double *ent_scale;      /* [count][B] MeshEnt.scale (0 for other kinds); read-only */
    int32_t *ent_order;     /* [count][B + 1] self.entities now, as slots: -2 = the agent, -1 = past the end (entities removed) */
    double *task_f;         /* [count] CollectHealth.health */
    int32_t *task_i;        /* [count] PickupObjs.num_picked_up */
    int32_t *text_tex;      /* [count][8] texture slot per character of the task's TextFrame (-1 = none / space); read-only */
} mwb_state;

/* ---- lifetime ---------------------------------------------------------------------------- */
/* replaces: gym.make('MiniWorld-<Class>-v0') x N + SubprocVecEnv.__init__
 * (envs/__init__.py:43-49, pytorch-a2c-ppo-acktr/envs.py:57-63, vec_env/subproc_vec_env.py:36-56) */
int mwb_create(const mwb_config *cfg, mwb_handle **out);
/* replaces: SubprocVecEnv.close (vec_env/subproc_vec_env.py:87-97).  Frees everything the handle allocated, the buffers of
 * every mwb_*_enable below included.  Each of those functions either succeeds or leaves the handle as it was: what it had
 * allocated before a failure (MWB_ENOMEM, MWB_EHIP) is freed again, and the call can be repeated. */
int mwb_destroy(mwb_handle *h);
const char *mwb_last_error(void);
int mwb_abi_version(void);

/* ---- assets ------------------------------------------------------------------------------ */
/* replaces: Texture.load (opengl.py:71-108): upload RGB8 pixels (row 0 = TOP of the image, tightly
 * packed) for texture slot `tex_id` (0 floor_tiles_bw_1, 1-4 concrete_1..4, 5 concrete_tiles_1,
 * 6 brick_wall_1; the sim-to-real rinks also use 7-10 cardboard_1..4, 11-12 wood_1..2, 13 wood_planks_1,
 * 14 drywall_1, 15 stucco_1, 16 ceiling_tiles_1); the library builds the mip chain.  Every slot the task can
 * draw must be set before the first render. Synchronous. */
/* entity tasks: 17 asphalt_1, 18 slime_1, 19 cinder_blocks_1, 20 logo_mila_1, 21-24 the images of the textured meshes (medkit,
 * duckie, building, cone), 25 + 9 c + v: variant v + 1 of chars/ch_0x<ord>_*.png for the c-th character of "BLUERDGN" (Sign) */
#define MWB_NUM_TEXTURES 97
#define MWB_TEX_MESH0 21
#define MWB_TEX_CHAR0 25
int mwb_num_textures(mwb_handle *h);   /* how many leading slots the handle's task uses (7, 17, 25 or 97) */
/* replaces: ObjMesh.get / ObjMesh.__init__ (objmesh.py:16-216) for one mesh geometry, shared by all envs of the handle: the
 * triangle soup as the reference hands it to OpenGL - verts / norms float32 [n_tris][3][3], texcs [n_tris][3][2], in draw order -
 * its extents (ObjMesh.min_coords / max_coords), the texture slot of its image (-1 none) and a threaded bounding-volume
 * hierarchy over the triangles for the render kernel: nodes float32 [n_orders][n_nodes][8] = lo.xyz, skip (int bits) | hi.xyz,
 * first | count << 24 (int bits) in depth-first order (an inner node's first child follows it; `skip` = next node when the box
 * is missed or the leaf is done); perm int32 [n_tris] = triangle indices in leaf order.  n_orders is 1, or 8: eight threadings
 * of the same tree over the same leaves, threading k for rays whose direction (in the mesh's frame) has component a negative
 * iff bit a of k is set - the child nearer along the split axis first.  Host pointers; synchronous.
 * The vertex colour is the material's Kd, which the entity carries (ball_<c> / key_<c> share their geometry). */
int mwb_set_mesh(mwb_handle *h, int geom, int n_tris, const float *verts, const float *norms, const float *texcs, int tex_slot,
                 const float *min_coords, const float *max_coords, int n_nodes, int n_orders, const float *nodes, const int32_t *perm);
/* replaces: MeshEnt.__init__'s arithmetic (entity.py:118-127) - `scale = height / sy`, `radius = sqrt(sx^2 + sz^2) * scale` -
 * evaluated by the host with the reference's expressions, because their scalar type follows the installed NumPy (float32 under
 * NumPy >= 2, where sums with Python floats are then float32 too): one call per (geometry, height) the task builds. */
int mwb_set_mesh_dims(mwb_handle *h, int geom, double height, double scale, double radius, int is_float32);
/* debugging aid (MWB_DEBUG bit 4 at mwb_create): start / end s_memrealtime ticks (100 MHz) of every workgroup of the
 * last bulk render launch, [2 * n] u64; returns n or a negative code */
int mwb_debug_wg_times(mwb_handle *h, unsigned long long *out, int max_wgs);
/* debugging aid (MWB_EXP bit 2 at mwb_create): counters of the entity render kernel's mesh walks since the last reset - sample rays
 * entering the walk, walks started, node visits, triangle tests, wave loop iterations, wave calls (out8: 8 x u64) */
int mwb_debug_counters(mwb_handle *h, unsigned long long *out8, int reset);
int mwb_set_texture(mwb_handle *h, int tex_id, int width, int height, const uint8_t *rgb);

/* ---- simulation -------------------------------------------------------------------------- */
/* replaces: env.seed(seed + rank) per worker (envs.py:35-36, miniworld.py:528-530, random.py:9-10).
 * seeds: host array [num_envs]. Synchronous (host-side key hashing + upload). */
int mwb_seed(mwb_handle *h, const uint64_t *seeds);
/* the seed -> MT19937 init_by_array key of gym<=0.21's seeding.np_random (hash_seed: first 8 bytes of
 * sha512(str(seed)) as little-endian 32-bit limbs), host-only helper; returns the key length (1 or 2) */
int mwb_seed_key(uint64_t seed, uint32_t key[2]);
/* replaces: VecEnv.reset (vec_env/subproc_vec_env.py:77-80 -> MiniWorldEnv.reset miniworld.py:532-592)
 * mask: device u8[num_envs] or NULL; NULL or mask[i]!=0 resets env i. Renders the first observation. */
int mwb_reset(mwb_handle *h, const uint8_t *mask_dev, void *stream);
/* replaces: VecEnv.step_async+step_wait (vec_env/subproc_vec_env.py:58-75, worker 5-14,26-31 ->
 * MiniWorldEnv.step miniworld.py:658-716 + task rule e.g. envs/maze.py:106-113), including the
 * worker's auto-reset and the fork's `mask` ('dummy') semantics.
 * actions: device i32[num_envs], MiniWorldEnv.Actions values 0..7 (miniworld.py:437-454: turn_left, turn_right, move_forward,
 * move_back, pickup, drop, toggle, done - every task executes all of them as the base class does; any other value does
 * nothing but count a step, as the reference's if-chain does); skip_mask: device u8[num_envs] or NULL (mask[i]!=0 -> env i is not
 * stepped, reward -99, done 0, observation re-rendered). */
int mwb_step(mwb_handle *h, const int32_t *actions_dev, const uint8_t *skip_mask_dev, void *stream);
/* the same with the LongTensor the reference's policy produces (VecPyTorch.step_async, envs.py:121-125): int64 actions [N] in
 * device memory are read in place (no conversion pass); a value outside int32 is an unknown action (never aliased) */
int mwb_step_i64(mwb_handle *h, const int64_t *actions_dev, const uint8_t *skip_mask_dev, void *stream);
/* Action repeat ("frame skip").  replaces: the loop a trainer wraps around env.step inside the worker of
 * vec_env/subproc_vec_env.py:5-33, under the worker's auto-reset:
 *     total = 0.0
 *     for _ in range(n_i): obs, r, done, info = env.step(a); total += r
 *                          if done: break
 * In one call env i takes at most n_i sub-steps of MiniWorldEnv.step with its one action and only the frame after the last of
 * them is rendered.  n_i = repeat, or counts[i] clamped to [1, repeat] on the device when counts (device i32[num_envs]) is not
 * NULL.  An env stops at the sub-step that sets done (task rule or time limit, as mwb_step decides them).  Outputs: reward64 =
 * the float64 sum of the sub-steps' rewards in order, starting from 0.0; reward = that sum as float; done, ep_steps, feature and
 * goal_pos = those of the last sub-step taken; obs / depth / grey / the fused frame stack's newest planes = the last sub-step's
 * own frame (entity tasks: with that sub-step's render override and no earlier one), or, for a finished env under auto-reset,
 * the first frame of the new episode - it is regenerated once, after its last sub-step.  With no_auto_reset the env just stops.
 * An env named by skip_mask takes the skip path once (reward -99, done 0, no sub-step).  The frame stack and the dispatch order
 * move once per call.  An env's last frame is reused only if every sub-step of the call left it unchanged.
 * Exactly one of actions (i32) and actions_i64 (read in place as mwb_step_i64 reads them) is not NULL.  repeat lies in
 * 1 .. MWB_MAX_REPEAT (it bounds the kernel launches of a call: two per sub-step): MWB_EINVAL otherwise, and nothing changes.
 * repeat == 1 with counts == NULL leaves every output, the state and the frame-reuse counters exactly as mwb_step does.
 * Capturable into a HIP graph as mwb_step is (repeat is a host constant of the capture). */
#define MWB_MAX_REPEAT 64
int mwb_step_repeat(mwb_handle *h, const int32_t *actions_dev, const int64_t *actions_i64_dev, const uint8_t *skip_mask_dev, int repeat,
                    const int32_t *counts_dev, void *stream);
/* replaces: the `taken` a frame-skip wrapper would count in the loop above (a learner discounts by gamma ** taken).
 * *dev: library-owned device i32[num_envs], the sub-steps every env took in the last mwb_step_repeat (0 for an env its skip
 * mask named; zeros before the first call); the pointer is fixed for the handle's lifetime. */
int mwb_repeat_taken(mwb_handle *h, int32_t **dev);
/* replaces: MiniWorldEnv.render_obs / render_depth (miniworld.py:1160-1220) for the whole batch */
int mwb_render(mwb_handle *h, void *stream);
/* Last-frame reuse.  A step that leaves an env exactly as it was - a move that a wall or an entity blocks, nothing carried; an env
 * the skip mask leaves out - would render the frame of the step before once more.  The handle keeps every env's last frame in a
 * private cache (N x W*H*3 bytes, + N x W*H*4 with depth) and the step's bulk pass copies it into the outputs instead; the
 * outputs stay the caller's to overwrite, every step rewrites them in full.  mwb_reset and mwb_render always render.  The
 * environment variable MWB_NO_FRAME_REUSE=1 at mwb_create turns it off (no cache is allocated); it is off as well for frames
 * rendered in tiles.  out: frames the step passes reused / rendered since the last call.  Synchronous. */
int mwb_frame_reuse_stats(mwb_handle *h, unsigned long long out[2]);
/* Which kernel the bulk render launch of mwb_step runs for this handle now: 1 = render_fixed_kernel, compiled for 80 x 60
 * observations with the layout and "has depth" as constants (box tasks, no MWB_DEBUG / MWB_EXP bit set, no grey output, the
 * side stream in use), 0 = the generic render kernel (every other handle, and mwb_reset / mwb_render / the side stream always).
 * Both produce the same bytes.  The environment variable MWB_NO_FIXED=1 at mwb_create keeps the generic kernel.  NULL: 0. */
int mwb_bulk_variant(mwb_handle *h);
int mwb_get_outputs(mwb_handle *h, mwb_outputs *out);

/* ---- learner-side layout fusion ---------------------------------------- */
/* replaces: VecPyTorchFrameStack + VecPyTorch's .float() (pytorch-a2c-ppo-acktr/envs.py:117-165): a
 * library-owned channel-first stack [N, nstack*3, W, H] (needs MWB_LAYOUT_CWH), dtype 0 = u8, 1 = f32
 * (values 0..255).  mwb_stack_update(after_reset != 0) implements reset(): zero, newest obs in the last 3
 * channels (envs.py:158-162); after_reset == 0 implements step_wait(): shift by 3 channels, zero the envs
 * whose `done` is set, append the newest obs (envs.py:149-156) - one pass over the stack. */
int mwb_stack_enable(mwb_handle *h, int nstack, int dtype);
/* dtype | MWB_STACK_SLIDING: the stack as a sliding window over nstack*3 + 3*MWB_STACK_SLACK_FRAMES planes per env - a step
 * writes the new frame only (the history planes stay in place) and the window moves three planes on; once every
 * MWB_STACK_SLACK_FRAMES + 1 steps the history is copied back to the front.  The current view is planes
 * [first_plane, first_plane + nstack*3) of each env's planes_per_env (mwb_stack_window, valid after each mwb_stack_update):
 * same values as the shifting stack at ~1/4 of its HBM traffic.  The window position lives on the host, so a captured graph
 * of mwb_stack_update must not be replayed with this flag. */
#define MWB_STACK_SLIDING 16
#define MWB_STACK_SLACK_FRAMES 8
/* dtype | MWB_STACK_FUSED (implies the sliding window): mwb_reset / mwb_step move the window themselves and the render
 * kernels write each new frame straight into its newest three planes (u8 -> f32 on the way out of LDS), zeroing the history of
 * the envs they regenerate: mwb_stack_update becomes a no-op and the observation never takes a second trip through HBM.
 * Read the window with mwb_stack_window after every mwb_reset / mwb_step.  Must be enabled before the first mwb_reset /
 * mwb_step / mwb_render (MWB_ESTATE otherwise: the window would lack the frame already rendered).  A PARTIAL mwb_reset(mask)
 * is a step for the window: it moves three planes on, the masked envs get a zeroed history and their first frame, the others
 * get their re-rendered current frame appended once more (VecPyTorchFrameStack has no partial reset to compare with).
 * A view of an earlier window position is guaranteed only until the next pass: the history planes of an env that ends are
 * zeroed in place; for envs that keep running it stays intact for MWB_STACK_SLACK_FRAMES + 1 - nstack further steps. */
#define MWB_STACK_FUSED 32
/* dtype | MWB_STACK_GREY: the stack of GreyscaleWrapper's frames (below) - nstack planes per env instead of nstack*3, [N, nstack,
 * W, H], each step's grey frame in the newest ONE plane.  Needs mwb_grey_enable first (MWB_ESTATE otherwise) and dtype 1
 * (MWB_EINVAL with u8: the reference defines no uint8 grey).  Combines with the shifting stack, MWB_STACK_SLIDING and
 * MWB_STACK_FUSED: in the sliding forms the window moves one plane per step over nstack + MWB_STACK_SLACK_FRAMES planes
 * (mwb_stack_window reports them); the partial-reset rule and the history guarantee above hold with "three planes" read as "one
 * plane".  The non-fused forms take their frames from the grey buffer in mwb_stack_update; the fused one is written by the render kernels,
 * together with the grey buffer. */
#define MWB_STACK_GREY 64
int mwb_stack_window(mwb_handle *h, int *first_plane, int *planes_per_env);
int mwb_stack_update(mwb_handle *h, int after_reset, void *stream);

/* ---- greyscale observations ------------------------------------------------------------------ */
/* replaces: GreyscaleWrapper (gym_miniworld/wrappers.py:29-45) followed by VecPyTorch's .float() (pytorch-a2c-ppo-acktr/
 * envs.py:119,128): grey = float32((0.30 R + 0.59 G) + 0.11 B), the sum in float64 as NumPy evaluates it, rounded once - bit for
 * bit the reference's values.  Allocates a library-owned float32 buffer, [N][H][W] for MWB_LAYOUT_HWC handles (read it as
 * [N,H,W,1], the wrapper's observation_space) and [N][W][H] for MWB_LAYOUT_CWH ones ([N,1,W,H], after TransposeImage); every
 * mwb_reset / mwb_step / mwb_render from then on fills it in the pass that writes `obs`: the render kernel's copy-out writes each
 * frame twice, as RGB bytes and as grey, from the same LDS frame (handles with grey run the render_grey_kernel instantiations,
 * handles without it the kernels they always ran).  obs, depth and every other output are what they are without it.  Must be called before the first mwb_reset / mwb_step / mwb_render (MWB_ESTATE
 * otherwise: the buffer would lack the frame already rendered); MWB_EINVAL when W*H is no multiple of 4 or observations are
 * rendered in tiles (large frames, MWB_TILE: convert those with mwb_grey_convert); MWB_ESTATE when already enabled.  There is
 * no uint8 grey: the reference defines none. */
int mwb_grey_enable(mwb_handle *h);
/* the buffer mwb_grey_enable allocated and its size in bytes (either pointer may be NULL); MWB_ESTATE before mwb_grey_enable.
 * replaces: reading the observation GreyscaleWrapper.observation returned (wrappers.py:38-45) */
int mwb_grey_output(mwb_handle *h, float **grey, size_t *bytes);
/* replaces: GreyscaleWrapper.observation (wrappers.py:38-45) + .float() applied to ANY frames: n_frames RGB frames of width x
 * height in device memory - MWB_LAYOUT_HWC: interleaved [n][height][width][3], MWB_LAYOUT_CWH: three planes [n][3][width][height]
 * - to float32 [n][height][width] / [n][width][height], with the conversion the render kernels use; e.g. mwb_render_view's
 * output, or the observations of a handle whose frames are rendered in tiles.  Any size up to 4096 x 4096; enqueued on `stream`. */
int mwb_grey_convert(mwb_handle *h, const uint8_t *rgb_dev, float *grey_dev, int n_frames, int width, int height, int layout,
                     void *stream);

/* ---- copying environments on the device: clone, snapshot, restore ------------------------------ */
/* replaces: copy.deepcopy(env), or assigning a saved env's attributes (agent, entities, rooms, rand) to another env, on the
 * reference's Python objects.
 * For each i < count, env dst_idx[i] of `dst` becomes a TWIN of env src_idx[i] of `src`: stepped with the same actions the two
 * agree bit for bit at every later step - reward, done, ep_steps, the whole mwb_get_state (MT19937 words and entity order
 * included), mwb_get_geometry, obs, depth and grey - through episode ends and auto-resets.  Everything a later kernel reads of an env
 * is copied, the world (room table, collision segments) included; the outputs of the destination's last transition (reward,
 * done, ep_steps, feature, goal_pos) are not: the next step rewrites them.  Both index arrays are int32 in DEVICE memory, so
 * a selection computed on the device needs no synchronisation; all work is enqueued on `stream`.  dst == src clones inside one
 * handle; a second handle of the same configuration serves as an archive (there is no other object type).
 *
 * The two handles' mwb_config must be equal except for num_envs and domain_rand, on one device: MWB_EINVAL otherwise, the
 * message names the first differing field.  That both were given the same textures and meshes is the caller's duty.
 * MWB_ESTATE: the source has never been reset (nor received a copy); or a rendering copy into a destination that lacks
 * what mwb_render needs (seed, textures, meshes).  count == 0 is a no-op, count < 0 or a null argument MWB_EINVAL.  A slot of an
 * archive that never received a copy holds no world: copying FROM it is the caller's error (it yields an empty env).
 *
 * Pairs are validated on the device before anything is copied (csrc/mwb_copy_check.h).  A pair is REJECTED - skipped entirely and
 * counted - when an index is outside [0, num_envs) of its handle, when its destination is named by more than one pair, or when,
 * on one handle, its destination is also some pair's source; except that dst_idx[i] == src_idx[i] on one handle is valid and does
 * nothing.  mwb_copy_rejected returns the number of pairs rejected on `dst` since it was last called and clears it (synchronous).
 *
 * Observations.  Without MWB_COPY_NO_RENDER the accepted destinations are prepared and rendered on `stream` as mwb_render
 * renders them (the current state): when the call's work completes, obs, depth, grey and the last-frame cache of every destination
 * env hold what mwb_render would write for it, and every other env's outputs are untouched.  With MWB_COPY_NO_RENDER only state
 * moves: the destination's frames are stale until the caller renders (their cached last frames are dropped), and the
 * destination needs nothing beyond mwb_create - an archive never uploads a texture.
 *
 * Frame stack.  The window does not move in a copy.  (1) No stack on the destination: nothing is done.  (2) Both handles have a
 * stack of equal nstack, dtype and grey flag (the form - shifting, sliding, fused - may differ): the destination env's visible
 * window, planes [first_plane, first_plane + nstack * 3 or nstack), becomes a byte copy of the source env's, after the render.
 * PRECONDITION: the source's stack is current - for the non-fused forms mwb_stack_update has been called after the source's last
 * pass.  (3) The destination's stack is fused and the source has none or another one: the destination env gets what a
 * regenerated env gets, a zeroed history and its frame in the newest planes; MWB_EINVAL under MWB_COPY_NO_RENDER.  (4) The
 * destination's stack is not fused and the source has none or another one: MWB_EINVAL.
 *
 * Rollout storage (mwb_rollout_enable, below).  A copy touches no rollout, of either handle: the caller restarts the destinations'
 * history by naming them in the `fresh_dev` of its next mwb_rollout_push. */
#define MWB_COPY_NO_RENDER 1
int mwb_copy_envs(mwb_handle *dst, const int32_t *dst_idx_dev, mwb_handle *src, const int32_t *src_idx_dev,
                  int count, unsigned flags, void *stream);
int mwb_copy_rejected(mwb_handle *dst, unsigned long long *pairs);   /* synchronous; reads and clears */
/* bytes of per-env state one accepted pair of a copy from src into dst moves (for measurements); negative code on mismatch */
long long mwb_copy_env_bytes(mwb_handle *dst, mwb_handle *src);

/* ---- rollout storage on the device: frame ring and stacked-minibatch gather ------------------------ */
/* replaces: the observation half of RolloutStorage (pytorch-a2c-ppo-acktr/storage.py:12,55,75,121) together with its masks,
 * rewards and features rows - a [num_steps + 1][N] array of STACKED float32 observations, written with
 * obs[step + 1].copy_(obs) and read with obs[:-1].view(-1, ...)[indices].  The rollout keeps every single frame once, in the
 * format the handle renders it (uint8 RGB, or the float32 grey frame), in a time-major ring of R = num_steps + nstack slots
 * [R][N][C][W][H] (C = 3, or 1 for grey), plus one byte of "age" per (step, env): how many earlier frames belong to the stacked
 * observation VecPyTorchFrameStack (envs.py:135-165) held there.  mwb_rollout_gather rebuilds any stacked row from them, bit for
 * bit.  Logical time t lives in slot (base + t) mod R, the frame j steps before it in slot (base + t - j + R) mod R - for
 * t - j < 0 these are the last frames of the window before (csrc/mwb_rollout_map.h has the arithmetic and why R is the smallest
 * ring that works).  base and the cursor live on the host, as the sliding frame stack's window position does: a captured graph
 * of these calls must not be replayed.
 *
 * mwb_rollout_enable (replaces RolloutStorage.__init__, storage.py:10-25): num_steps >= 1, nstack in 1 .. 16, flags 0 or
 * MWB_ROLLOUT_GREY (the ring of the grey frames).  MWB_EINVAL: the handle is not MWB_LAYOUT_CWH, or W*H is no multiple of 4 (the
 * frame stack's own rules), or a bad argument.  MWB_ESTATE: already enabled, or MWB_ROLLOUT_GREY without mwb_grey_enable.  May be
 * called at any time: it reads only the output buffers (handles whose frames are rendered in tiles included).  Allocates the ring,
 * age u8 [T + 1][N], reward f32 [T][N], mask f32 [T + 1][N], feature f32 [T + 1][N][2] (T = num_steps); mwb_destroy frees them.
 * mwb_copy_envs does not touch a rollout: the caller restarts the destinations' history with `fresh_dev`, below. */
#define MWB_ROLLOUT_GREY 1
int mwb_rollout_enable(mwb_handle *h, int num_steps, int nstack, unsigned flags);
/* replaces: rollouts.obs[0].copy_(obs) after envs.reset() (after_reset != 0) and RolloutStorage.insert (storage.py:52-66,
 * after_reset == 0): records the handle's current outputs as one logical time step, enqueued on `stream` after the pass that
 * produced them.
 * after_reset != 0: the cursor becomes 0, frame(0) = obs (or grey), age[0] = 0, mask[0] = 1, feature[0] = 0 for every env
 *   (VecPyTorchFrameStack.reset, envs.py:158-162; the initial masks / features of RolloutStorage).
 * after_reset == 0: the cursor becomes t = cursor + 1, frame(t) = obs; with fresh[e] = fresh_dev ? fresh_dev[e] != 0 : done[e]:
 *   age[t][e] = fresh ? 0 : min(age[t-1][e] + 1, nstack - 1), mask[t][e] = fresh ? 0 : 1, feature[t][e] = feature[e] (the
 *   features[step + 1] convention, storage.py:67), reward[t-1][e] = reward[e], or 0 when fresh_dev is given.
 * fresh_dev (device u8[num_envs] or NULL) is for passes that are not steps - a partial mwb_reset(mask), where the caller passes
 * its mask, or the destinations of an mwb_copy_envs: the named envs start a new history, the others get their current frame
 * appended once more (the rule stated above for the fused stack's partial reset).  A skipped env (reward -99, done 0) is simply an
 * env that is not done; mwb_step_repeat is one frame per call.
 * MWB_ESTATE, and nothing changes: no after_reset push has been made yet, or the cursor is already num_steps (call
 * mwb_rollout_after_update). */
int mwb_rollout_push(mwb_handle *h, int after_reset, const uint8_t *fresh_dev, void *stream);
/* replaces: obs.view(-1, *obs.size()[2:])[indices] of the minibatch generators (storage.py:121) and obs[step] of the acting loop.
 * index_dev: device i64[count], index_dev[i] = t * N + e with t in 0 .. cursor - the flat index of that view, t = num_steps (the
 * bootstrap observation) allowed; any order, repeats allowed; read on the device, no synchronisation.  Row i of out_dev (device
 * memory, 16-byte aligned) is [nstack * C][W][H], contiguous: float32 for dtype 1 (uint8 -> float32 is exact, grey frames are
 * copied bitwise), uint8 for dtype 0 (MWB_EINVAL for a grey ring: the reference defines no uint8 grey).  Frame group k (0 =
 * oldest) is frame t - j with j = nstack - 1 - k if j <= age[t][e], zeros otherwise.  A row whose index is negative or
 * >= (cursor + 1) * N is written as zeros and counted (mwb_rollout_rejected); nothing is read or written outside the ring and
 * the `count` rows.  count == 0 is a no-op.  MWB_ESTATE before the first push. */
int mwb_rollout_gather(mwb_handle *h, const int64_t *index_dev, int count, void *out_dev, int dtype, void *stream);
/* replaces: RolloutStorage.after_update (storage.py:69-73): row num_steps of age, mask and feature becomes row 0, base moves
 * num_steps slots on and the cursor becomes 0 - no frame moves.  MWB_ESTATE before the first push. */
int mwb_rollout_after_update(mwb_handle *h, void *stream);
/* the rollout's device arrays (fixed for the handle's lifetime) and its position.  The struct has a tag only, no typedef: the
 * function below bears the same name, so the type is always written `struct mwb_rollout_info` */
struct mwb_rollout_info {
    float *reward, *mask, *feature;   /* f32 [T][N], [T+1][N], [T+1][N][2] */
    uint8_t *age;                     /* u8 [T+1][N] */
    void *ring;                       /* [R][N][C][W][H], u8 or (grey) f32 */
    size_t reward_bytes, mask_bytes, feature_bytes, age_bytes, ring_bytes;
    int32_t num_steps, nstack, grey;
    int32_t cursor;                   /* the last logical time pushed; -1 before the first after_reset push */
    int32_t base;                     /* ring slot of logical time 0 */
    int32_t pad;
};
int mwb_rollout_info(mwb_handle *h, struct mwb_rollout_info *out);   /* MWB_ESTATE before mwb_rollout_enable */
int mwb_rollout_rejected(mwb_handle *h, unsigned long long *rows);   /* synchronous; reads and clears */

/* ---- rollout storage: the windowed gather - per-row random shift, crop and translate ---------------- */
/* replaces: obs_batch = obs[:-1].view(-1, ...)[indices] (storage.py:121) FOLLOWED BY the trainer's image augmentation of that
 * minibatch (RAD / DrQ random shift with edge replication, random crop, random translate; DrAC / UCB-DrAC), which today costs a
 * second pass over the float32 tensor.  A window is applied while the row is rebuilt from its single uint8 frames: one pass, no
 * temporary.  Each row has one offset pair (dx, dy), shared by all of its planes (every frame group, every channel) and clamped
 * on the device to [dx_lo, dx_hi] x [dy_lo, dy_hi] before anything is computed from it.  With F the row mwb_rollout_gather would
 * write, [nstack * C][W][H], the windowed row is [nstack * C][out_w][out_h] (csrc/mwb_rollout_window_map.h has the rule as code):
 *   out[p][x][y] = F[p][sx][sy] with sx = x + dx, sy = y + dy where 0 <= sx < W and 0 <= sy < H; elsewhere
 *                  F[p][clamp(sx, 0, W-1)][clamp(sy, 0, H-1)] for border 0 (edge replication), 0 for border 1 (zeros).
 * A zero frame group stays zero under either border.  The named augmentations are settings of this rule:
 *   random shift by pad    out W x H, border 0, dx and dy in -pad .. pad
 *   random crop w x h      out w x h <= W x H, dx in 0 .. W - w, dy in 0 .. H - h   (centre crop: both ranges one value)
 *   random translate       out w x h >= W x H, border 1, dx in -(w - W) .. 0, dy in -(h - H) .. 0
 * MWB_EINVAL for a window outside the limits: 1 <= out_w, out_h <= 1024; out_w * out_h a multiple of 4 (the frame stack's own
 * rule); lo <= hi; every bound in -32767 .. 32767; border 0 or 1.  The struct has a tag only, as mwb_rollout_info. */
struct mwb_rollout_window { int32_t out_w, out_h, border, dx_lo, dx_hi, dy_lo, dy_hi, pad; };
/* replaces: the augmentation's own random draw (torch.randint of the pad / crop positions).  offsets_dev[i] = the draw of
 * index_dev[i] under (seed, call): device int32 [count][2] = (dx, dy), 8-byte aligned.  With mix = splitmix64's finaliser and
 * G = 0x9E3779B97F4A7C15 (the level sampler's recipe, uint64 arithmetic):
 *   key = mix(seed + G * (call + 1)), h = mix(key + G * ((uint64)index + 1)),
 *   dx = dx_lo + (((h >> 32) * (dx_hi - dx_lo + 1)) >> 32), dy = dy_lo + (((h & 0xffffffff) * (dy_hi - dy_lo + 1)) >> 32).
 * The draw is keyed by the index, not by the row's place in the minibatch: a transition gets the same draw wherever a permutation
 * puts it, and a new one when `call` changes.  Any int64 index is hashed; validity is the gather's business.  Needs no rollout.
 * count == 0 is a no-op.  MWB_EINVAL: a null handle or argument, a window outside the limits, count < 0, offsets_dev misaligned. */
int mwb_rollout_window_offsets(mwb_handle *h, const struct mwb_rollout_window *w, uint64_t seed, uint64_t call,
                               const int64_t *index_dev, int count, int32_t *offsets_dev, void *stream);
/* replaces: obs_batch of storage.py:121 followed by the trainer's augmentation (above).  mwb_rollout_gather with the window
 * applied on the way: row i of out_dev is [nstack * C][out_w][out_h].  offsets_dev: device int32 [count][2], 8-byte aligned, read
 * on the device and clamped to the window's ranges there - the caller's own (UCB-DrAC, a sampler of its own) or
 * mwb_rollout_window_offsets'.  dtype, out_dev's alignment, the index rule, zeros + mwb_rollout_rejected for rows out of range
 * (no address is formed from such an index, nor from an unclamped offset), count == 0: all as mwb_rollout_gather.
 * MWB_EINVAL: a null handle or argument, a window outside the limits, a bad dtype (uint8 from a grey ring included), count < 0, a
 * misaligned out_dev / offsets_dev.  MWB_ESTATE: before mwb_rollout_enable, or before the first push. */
int mwb_rollout_gather_window(mwb_handle *h, const int64_t *index_dev, int count, const struct mwb_rollout_window *w,
                              const int32_t *offsets_dev, void *out_dev, int dtype, void *stream);

/* ---- rollout storage, the learner half: small columns, returns / GAE scan, minibatch columns -------- */
/* replaces: the rest of RolloutStorage (storage.py:15-18,32-34): actions, action_log_probs, value_preds, returns, psi_returns -
 * and what no reference array holds: `taken`, the sub-steps every transition took (mwb_step_repeat), by which the scans below
 * discount.  Opt-in: a handle that never calls this launches exactly what it launched before.  Call after mwb_rollout_enable;
 * MWB_ESTATE before it, or when already enabled.  Allocates, with T = num_steps (mwb_destroy frees them):
 *   action i64 [T][N], log_prob f32 [T][N], value f32 [T+1][N], taken i32 [T][N], ret f32 [T+1][N], adv f32 [T][N],
 *   psi_ret f32 [T+1][N][2] - all zeros, except taken, which starts as 1.
 * From then on mwb_rollout_push(after_reset == 0) to time t also writes taken[t-1][e], in a small launch of its own: the taken
 * buffer of the mwb_step_repeat if that was the last pass on the handle (0 for an env its skip mask named), 1 after mwb_step /
 * mwb_step_i64, and 1 when fresh_dev is given (a pass that is not a step).  The handle remembers the kind of the last pass on
 * the host. */
int mwb_rollout_learner_enable(mwb_handle *h);
/* replaces: the columns of RolloutStorage.insert (storage.py:57-61) - actions[step], action_log_probs[step], value_preds[step]
 * of the transition that led to the last push: row cursor - 1 of action, log_prob and value.  Device arrays of num_envs
 * entries; every pointer may be NULL (that column keeps what it holds; storage.py:58-61 skip None the same way), at most one of
 * action_dev (i64) and action_i32_dev (widened) may be given: MWB_EINVAL otherwise.  MWB_ESTATE when the cursor is less than 1
 * (nothing pushed since the reset push or since after_update).  Nothing changes on an error. */
int mwb_rollout_insert(mwb_handle *h, const int64_t *action_dev, const int32_t *action_i32_dev, const float *log_prob_dev,
                       const float *value_dev, void *stream);
/* replaces: RolloutStorage.compute_returns (storage.py:82-99; MWB_RETURNS_GAE = use_gae, MWB_RETURNS_DISCOUNTED otherwise) and
 * compute_psi_returns (storage.py:101-105; MWB_RETURNS_PSI), the num_steps-long Python loops over tiny tensors: one kernel, one
 * lane per env, sequential over t.  The results are bit-equal to torch's eager float32 arithmetic in the reference's operation
 * order (csrc/mwb_returns_scan.h states every operation), with one extension: the transition t -> t+1 is discounted by
 * G[k] = (float)(gamma^k) - and L[k] = (float)((gamma * tau)^k) for the GAE trace - with k = taken[t][e] clamped to
 * 0 .. MWB_MAX_REPEAT, the powers formed in float64 by repeated multiplication.  With taken == 1 everywhere that is the reference.
 *   GAE:        value[T] = ret[T] = next_value; gae = 0; for t = T-1 .. 0:
 *               delta = reward[t] + G[k] * value[t+1] * mask[t+1] - value[t]; gae = delta + L[k] * mask[t+1] * gae;
 *               ret[t] = gae + value[t]
 *   DISCOUNTED: value[T] = ret[T] = next_value; ret[t] = ret[t+1] * G[k] * mask[t+1] + reward[t]
 *   PSI:        psi_ret[T] = next_psi; psi_ret[t] = psi_ret[t+1] * G[k] * mask[t+1] + feature[t], per component
 * GAE and DISCOUNTED also write adv[t] = ret[t] - value[t] (ppo.py:33; normalising them stays with the caller).
 * next_value_dev: f32 [N] (GAE, DISCOUNTED); next_psi_dev: f32 [N][2] (PSI); the one the mode does not use is ignored.
 * reward_override_dev: f32 [T][N] or NULL, read instead of the stored rewards (the sf=True branch's estimated_rewards,
 * storage.py:92-95); ignored by PSI.  tau is used by GAE only.  MWB_ESTATE unless the cursor is at num_steps; MWB_EINVAL for an
 * unknown mode or when the mode's `next` array is NULL.  Nothing changes on an error. */
#define MWB_RETURNS_DISCOUNTED 0
#define MWB_RETURNS_GAE 1
#define MWB_RETURNS_PSI 2
int mwb_rollout_returns(mwb_handle *h, int mode, double gamma, double tau, const float *next_value_dev, const float *next_psi_dev,
                        const float *reward_override_dev, void *stream);
/* replaces: the six small `tensor.view(-1, 1)[indices]` of a minibatch (storage.py:124-128, ppo.py:41-43): one kernel.
 * index_dev: device i64[count], the flat indices of the [:-1] views: idx = t * N + e with t in 0 .. T-1.  out_f32_dev: f32
 * [5][count] = return, value prediction, old log-prob, advantage, mask of the rows; out_action_dev: i64 [count].  adv_src_dev:
 * f32 [T*N], the caller's (normalised, ppo.py:34) advantages, or NULL for the stored adv.  A row whose index lies outside
 * [0, T*N) is written as zeros and counted in mwb_rollout_rejected; no address is formed from it.  count == 0 is a no-op. */
int mwb_rollout_gather_cols(mwb_handle *h, const int64_t *index_dev, int count, const float *adv_src_dev, float *out_f32_dev,
                            int64_t *out_action_dev, void *stream);
/* the learner half's device arrays (fixed for the handle's lifetime); MWB_ESTATE before mwb_rollout_learner_enable */
struct mwb_rollout_learner_info {
    int64_t *action;                  /* i64 [T][N] */
    float *log_prob, *value;          /* f32 [T][N], [T+1][N] */
    int32_t *taken;                   /* i32 [T][N] */
    float *ret, *adv, *psi_ret;       /* f32 [T+1][N], [T][N], [T+1][N][2] */
    size_t action_bytes, log_prob_bytes, value_bytes, taken_bytes, ret_bytes, adv_bytes, psi_ret_bytes;
};
int mwb_rollout_learner_info(mwb_handle *h, struct mwb_rollout_learner_info *out);

/* ---- episode monitor on the device: returns, lengths, the log of the last episodes, evaluation quotas ---------- */
/* replaces: the trainer's record of its own progress - `episode_rewards = deque(maxlen=100)` filled by a Python loop over every
 * env after every step (pytorch-a2c-ppo-acktr/main.py:141,167-169), which appends the LAST step's reward of a finished env (its own
 * comment: "works only for environments with sparse rewards") - and the bench.Monitor wrapper envs.py:45 comments out, whose
 * info['episode'] the evaluation loop waits for (main.py:248-262).  The monitor keeps, per env, the float64 sum of the rewards of
 * the running episode (one add per update, from 0.0: the order Python's sum takes), its length in env steps (sub-steps under
 * mwb_step_repeat) and in step calls; the episode that ended most recently; a ring of the last `capacity` episodes in the order
 * that loop appends them (pass by pass, increasing env index inside a pass; csrc/mwb_monitor_map.h has the arithmetic); and, for
 * evaluation, a table of every env's first quota_max episodes with a per-env quota after which an env is `retired` - the mask a
 * caller hands to the next step as its skip mask, so that "K episodes per env" replaces the biased "first K episodes to finish".
 * Opt-in: a handle that never calls mwb_monitor_enable launches exactly what it launched before.  Everything, the counters and
 * the quota included, lives on the device: an update can be captured into a graph together with the step.
 *
 * mwb_monitor_enable (replaces deque(maxlen=capacity), main.py:141): capacity in 1 .. 65536, quota_max in 0 .. 64, MWB_EINVAL
 * otherwise and for a handle created with no_auto_reset (a finished env stops there; what a later step means for an episode is
 * undefined).  MWB_ESTATE: already enabled.  All accumulators and counters start at zero, the table as NaN / -1, quota 0,
 * remaining = num_envs.  mwb_destroy frees it. */
int mwb_monitor_enable(mwb_handle *h, int capacity, int quota_max);
/* replaces: one turn of the loop main.py:167-169, with the return summed per episode.  With reward64_dev / done_dev / taken_dev
 * NULL it reads the handle's own reward64 and done outputs and, for the sub-steps of the call, the buffer of mwb_repeat_taken if
 * the last pass on the handle was an mwb_step_repeat, else 1 (the rule of the rollout's `taken` column, remembered on the host the
 * same way).  A non-NULL array (device f64 / u8 / i32 [num_envs]) stands in for that output: for a wrapper that shapes rewards.
 * skip_mask_dev (u8 [num_envs] or NULL): the skip mask the step was given.  For every env with skip_mask[e] == 0, in this order:
 * run_return += reward; run_len += taken; run_calls += 1; if done: with `partial` set the episode is counted in `dropped`, else
 * last_* are written, the episode is appended to the log, cell [finished[e]][e] of the table is written if finished[e] < quota_max
 * and finished[e] grows by one; then the three accumulators are zeroed and `partial` is cleared.  A skipped env is left untouched
 * (its reward of -99 enters no return).  After the pass retired[e] = quota > 0 && finished[e] >= quota and `remaining` counts the
 * envs with retired == 0.  Three small launches on `stream`; nothing is read back.  MWB_ESTATE before mwb_monitor_enable. */
int mwb_monitor_update(mwb_handle *h, const uint8_t *skip_mask_dev, const double *reward64_dev, const uint8_t *done_dev,
                       const int32_t *taken_dev, void *stream);
/* replaces: nothing the reference has (its envs are never reset or copied mid-episode).  Zeroes the accumulators of the envs
 * mask_dev (u8 [num_envs], NULL = all) names.  partial == 0: they start a fresh episode (after an mwb_reset).  partial != 0:
 * they are now in the middle of an episode whose start the monitor did not see (the destinations of an mwb_copy_envs): that
 * episode is dropped, not logged, when it ends. */
int mwb_monitor_clear(mwb_handle *h, const uint8_t *mask_dev, int partial, void *stream);
/* replaces: `while len(eval_episode_rewards) < 10` (main.py:248): sets the per-env quota, 0 .. quota_max (MWB_EINVAL otherwise),
 * 0 = none, nobody retires.  Zeroes finished and retired, sets remaining = num_envs and refills the table with NaN / -1; the
 * running accumulators and the log are not touched. */
int mwb_monitor_quota(mwb_handle *h, int quota, void *stream);
/* the monitor's device arrays (fixed for the handle's lifetime), for zero-copy views.  `host_pack` is one contiguous piece of
 * host_pack_bytes that holds what a host-side consumer wants after every step - last_return | last_len | last_calls | counts |
 * logged | retired, in this order - so that one copy delivers it.  counts: struct mwb_monitor_counts as it lies on the device. */
struct mwb_monitor_info {
    double *run_return, *last_return;                                /* f64 [N] */
    int32_t *run_len, *run_calls, *last_len, *last_calls, *finished; /* i32 [N] */
    uint8_t *partial, *retired;                                      /* u8 [N] */
    uint8_t *logged;                  /* u8 [N]: the last update appended an episode of env e (its last_* are that episode) */
    double *log_return;               /* f64 [capacity] */
    int32_t *log_len, *log_calls, *log_env;   /* i32 [capacity] */
    double *tab_return;               /* f64 [quota_max][N]; NULL when quota_max == 0 */
    int32_t *tab_len;                 /* i32 [quota_max][N] */
    void *counts;
    void *host_pack;
    size_t host_pack_bytes;
    int32_t num_envs, capacity, quota_max, pad;
};
int mwb_monitor_info(mwb_handle *h, struct mwb_monitor_info *out);   /* MWB_ESTATE before mwb_monitor_enable */
/* total: episodes ever appended to the log (ring slot = total % capacity); dropped: episodes that ended with `partial` set;
 * remaining: envs not retired; quota: as mwb_monitor_quota set it */
struct mwb_monitor_counts {
    unsigned long long total, dropped;
    uint32_t remaining, quota;
    uint32_t last_base, last_count;   /* of the last update: the slot of its first episode and how many it finished */
};
int mwb_monitor_read(mwb_handle *h, struct mwb_monitor_counts *out);   /* synchronous */

/* ---- terminal observations and the cause of an episode's end ---------------------------------------- */
/* replaces: what the reference's VecEnv worker throws away when it resets a finished env inside step
 * (vec_env/subproc_vec_env.py:10-13: `if done: ob = env.reset()` overwrites the frame step() rendered at `done`), and what a
 * modern VecEnv reports instead: info["terminal_observation"] and info["TimeLimit.truncated"].  MiniWorldEnv.step ends an episode
 * for two reasons that `done` merges (miniworld.py:708-711: `if self.step_count >= self.max_episode_steps: done = True`, and the
 * task's own rule on top); the reward cannot tell them apart.
 *
 * Opt-in: a handle that never calls mwb_terminal_enable launches exactly what it launched before.  On an enabled handle every
 * mwb_step / mwb_step_i64 / mwb_step_repeat
 *   - writes cause[e] = MWB_END_CLOCK | MWB_END_TASK bits where the step kernels write done[e]: 0 = the episode goes on (also for
 *     a skip-masked env); under mwb_step_repeat the byte of the env's last sub-step;
 *   - BEFORE it regenerates the envs that ended, renders their terminal frame - the step's own frame, as the observation of a
 *     no_auto_reset handle shows it (PickupObjs: the object picked up last is still drawn) - into frames[e] (and grey[e] on a
 *     handle with mwb_grey_enable), ranks them in ascending env index (row_of[e] = rank or -1, row_env[r] = env, count[0] = how
 *     many ended, possibly more than `capacity`) and writes for each of the first `capacity` of them one compact row: the
 *     stacked observation the policy would have seen had the env not been reset - the nstack - 1 history groups of the fused
 *     stack's window followed by the terminal frame - or, without a stack, the single frame.
 * Ended envs beyond `capacity` get no row (row_of = -1) and are counted; their frames[e] is still written.  All of it is ordered
 * before the step returns control of its outputs and stays valid until the handle's next pass.  mwb_reset, mwb_render and
 * mwb_copy_envs into the handle launch no terminal pass: after them count = 0, row_of = -1 and cause = 0 everywhere.
 * Terminal depth maps are not produced.
 *
 * mwb_terminal_enable: the handle auto-resets, 1 <= capacity <= num_envs, flags 0 or MWB_TERMINAL_FLOAT (stack-less handles: rows
 * are float32 instead of uint8; with a stack the rows take the stack's dtype), called before the first pass and AFTER
 * mwb_grey_enable / mwb_stack_enable where the handle uses them (it lays the rows out for the handle as it finds it; either call
 * is refused afterwards).  A handle with a frame stack must have the fused one (MWB_STACK_FUSED): a non-fused stack is refused
 * here, and mwb_stack_enable of one is refused after this call.  A grey fused stack gives grey rows.  MWB_EINVAL / MWB_ESTATE
 * otherwise, and nothing changes. */
#define MWB_END_CLOCK 1   /* step_count >= max_episode_steps */
#define MWB_END_TASK 2    /* a task rule raised done */
#define MWB_TERMINAL_FLOAT 1
int mwb_terminal_enable(mwb_handle *h, int capacity, unsigned flags);
/* the device arrays (fixed for the handle's lifetime).  Tag only, as struct mwb_rollout_info */
struct mwb_terminal_info {
    uint8_t *cause;                   /* u8 [N] */
    uint8_t *frames;                  /* u8 [N][W*H*3] in the handle's layout, env-indexed */
    float *grey;                      /* f32 [N][W*H] or NULL */
    int32_t *row_of, *row_env, *count;   /* i32 [N], [capacity], [1] */
    void *rows;                       /* [capacity][row_elems], u8 or f32 */
    size_t frames_bytes, grey_bytes, rows_bytes;
    int32_t capacity, rows_float, planes, nstack;   /* planes per row: C * nstack (3 or 1 per frame) */
};
int mwb_terminal_info(mwb_handle *h, struct mwb_terminal_info *out);   /* MWB_ESTATE before mwb_terminal_enable */
int mwb_terminal_dropped(mwb_handle *h, unsigned long long *envs);     /* synchronous; reads and clears */
/* The standard time-limit bootstrap on the rollout storage: for every terminal row r of the last step whose env e = row_env[r]
 * ended by the clock alone (cause[e] == MWB_END_CLOCK), reward[t][e] += G[k] * value_rows_dev[r] at t = cursor - 1, the transition
 * pushed last: one float32 multiply, then one float32 add.  G[k] = (float)(gamma^k) is the table of mwb_rollout_returns, k =
 * taken[t][e] with the learner half, 1 without.  value_rows_dev: f32 [capacity], V(rows[r]).  Envs without a row are skipped (they
 * are counted in mwb_terminal_dropped).  MWB_ESTATE unless both mwb_terminal_enable and mwb_rollout_enable were called and the
 * cursor is at least 1. */
int mwb_rollout_bootstrap(mwb_handle *h, const float *value_rows_dev, double gamma, void *stream);

/* ---- level sets: every episode's world from a level seed chosen on the device -------------------------- */
/* replaces: Procgen's `num_levels` / `start_level` (a finite, named set of worlds to train on, unseen ones to test on), and in
 * the reference `env.seed(s); env.reset()` per episode (miniworld.py seed(): `self.rand = RandGen(seed)`), which for a batch is
 * mwb_seed on the host: one SHA-512 and one init_by_array per env, 2500 bytes copied per env, and a full reset.
 *
 * Opt-in: a handle that never calls mwb_levels_enable launches exactly what it launched before.  On an enabled handle EVERY
 * regeneration of an env - the auto-reset inside mwb_step / mwb_step_i64 / mwb_step_repeat, mwb_reset(mask), mwb_reset(NULL) -
 * first overwrites the env's generator row rng[e][0..624] with exactly what mwb_seed writes for the seed of a chosen level
 * (SHA-512 of the decimal string, first 8 bytes, high limb dropped when zero; init_by_array; position 624).  The episode that
 * follows therefore equals the first episode of a reference env on which `env.seed(level_seed); env.reset()` ran, its
 * domain-randomisation draws at every step included.  The T-maze family's episode_count / task_step_count / goal_idx carry on
 * across it, as they do across env.seed() in the reference.
 *
 * A set has L = num_levels levels, 1 <= L <= 2^31 - 1.  Level i has the seed level_seeds_host[i] where a table was given
 * (L <= 2^24; copied to the device), start_level + i in uint64 arithmetic otherwise.  Per env the device keeps index (i32, the
 * level it is in, -1 before its first assignment), prev_index (i32, the level of its previous episode or -1), episode_no (i64,
 * assignments since enable or restart) and next_level (i32, a request, -1 = none).  The level of an assignment depends only on
 * (g, n, request), g = env_offset + e, n = episode_no[e], never on the order of the regenerated envs:
 *   MWB_LEVELS_SEQUENTIAL  i = (g + n * env_stride) mod L; with L = q * env_stride, q episodes per env visit every level once
 *   MWB_LEVELS_UNIFORM     a = mix(sampler_seed + GOLD * (g + 1)), h = mix(a + GOLD * (n + 1)), i = (h * L) >> 64, with
 *                          GOLD = 0x9E3779B97F4A7C15 and mix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27;
 *                          z *= 0x94D049BB133111EB; z ^= z >> 31
 *   MWB_LEVELS_TABLE       next_level[e] where 0 <= next_level[e] < L, the UNIFORM level otherwise; a value other than -1 that is
 *                          out of range is counted (mwb_levels_rejected) and no address is formed from it; the entry is consumed
 *                          either way (set to -1).  The caller refills next_level whenever it likes.
 * mode and sampler_seed live in device memory: mwb_levels_restart sets them, zeroes episode_no and (clear_tally) the tallies in
 * a small kernel on `stream`; index and prev_index stay.
 *
 * MWB_LEVELS_TALLY (L <= 2^22): u64 tallies[3][L] - episodes, env steps and successes (float64 reward > 0 on the ending
 * transition: the sparse-reward tasks' success; it means little for PickupObjs and CollectHealth) of the level an env LEAVES,
 * added with integer atomics in step passes only and only where index[e] >= 0.  mwb_reset abandons episodes and tallies nothing.
 *
 * mwb_copy_envs gives a destination its source's index where both handles have level sets (episode_no, prev_index and
 * next_level stay the destination's own: twins agree until the episode ends, then follow their own (g, n)); a destination
 * filled from a handle without level sets gets index -1, unknown, and is not tallied when it ends.
 *
 * mwb_levels_enable: once per handle; MWB_EINVAL for num_levels outside 1 .. 2^31 - 1, a table with more than 2^24 levels,
 * env_stride < 1, env_offset < 0, an unknown mode or flag, MWB_LEVELS_TALLY beyond 2^22 levels.  It marks the handle seeded:
 * mwb_seed is no longer required. */
#define MWB_LEVELS_SEQUENTIAL 0
#define MWB_LEVELS_UNIFORM    1
#define MWB_LEVELS_TABLE      2
#define MWB_LEVELS_TALLY      1u
int mwb_levels_enable(mwb_handle *h, int64_t num_levels, uint64_t start_level, const uint64_t *level_seeds_host /* or NULL */,
                      int mode, uint64_t sampler_seed, int64_t env_offset, int64_t env_stride, unsigned flags);
int mwb_levels_restart(mwb_handle *h, int mode, uint64_t sampler_seed, int clear_tally, void *stream);
/* the device arrays (fixed for the handle's lifetime) and the parameters.  Tag only, as struct mwb_rollout_info */
struct mwb_levels_info {
    int32_t *index, *prev_index, *next_level;   /* i32 [N] each; prev_index == index + N (one copy mirrors both) */
    int64_t *episode_no;                        /* i64 [N] */
    unsigned long long *tallies;                /* u64 [3][L]: episodes, env steps, successes; NULL without MWB_LEVELS_TALLY */
    const uint64_t *level_seeds;                /* u64 [L] on the device, NULL without a table */
    int64_t num_levels;
    uint64_t start_level, sampler_seed;         /* sampler_seed and mode: as enable / restart set them last */
    int64_t env_offset, env_stride;
    int32_t mode;
    uint32_t flags;
};
int mwb_levels_info(mwb_handle *h, struct mwb_levels_info *out);      /* MWB_ESTATE before mwb_levels_enable */
int mwb_levels_rejected(mwb_handle *h, unsigned long long *entries);   /* synchronous; reads and clears */

/* World generation cannot fail for the four tasks with sane arguments; if it ever does (a portal outside
 * its wall, more than one portal on an edge, a placement that finds no free spot in 100000 draws - the
 * reference would assert or spin) the kernel flags it. Synchronous: returns MWB_ESTATE if any env of the
 * handle hit such a condition since creation. */
int mwb_check(mwb_handle *h);

/* ---- introspection (tests, Gym single-env view) ------------------------------------------- */
int mwb_num_boxes(mwb_handle *h);   /* B: boxes per env of the handle's task */
int mwb_get_state(mwb_handle *h, int first_env, int count, mwb_state *out);          /* synchronous */
/* replaces: assigning env.agent.pos / env.box.pos / env.rand.np_random.set_state(...) etc. on the reference's
 * Python objects - overwrite the state of an env range with every non-NULL, non-read-only field of `in`
 * (test hook: inject oracle / reference states; also restores a snapshot taken with mwb_get_state). Synchronous.
 * MWB_EINVAL for non-finite values, box_size <= 0, carrying / goal_idx / MT19937 position out of range. */
int mwb_set_state(mwb_handle *h, int first_env, int count, const mwb_state *in);
/* overwrite pose / step counter of env range (NULL = leave); used to inject oracle states */
int mwb_set_agent(mwb_handle *h, int first_env, int count, const double *pos_xz, const double *dir,
                  const int32_t *step_count);
/* replaces: assigning `env.domain_rand = flag` after construction, as the reference's own smoke test does
 * for every env (run_tests.py:64-66; read at reset miniworld.py:558 and at every step miniworld.py:665);
 * takes effect from the next mwb_reset / mwb_step. Synchronous. */
int mwb_set_domain_rand(mwb_handle *h, int domain_rand);
/* overwrite the goal-alternation state of the T-maze family for an env range (NULL = leave); test hook */
int mwb_set_task_state(mwb_handle *h, int first_env, int count, const int64_t *episode_count,
                       const int64_t *task_step_count, const int32_t *goal_idx);
/* replaces: MiniWorldEnv.intersect(ent, pos, radius) (miniworld.py:933-959) for one env. `ent` = position of the
 * querying entity in the entity list (0 .. B-1 the boxes, B the agent) - it is skipped, as `ent2 is ent` is - or -1
 * to skip nobody.  result: 0 none, 1 wall (walls are tested first), 2 + k = the first entity k in list order within
 * radius + its radius. Synchronous. */
int mwb_intersect(mwb_handle *h, int env, int ent, double x, double z, double radius, int *result);
/* geometry of one env as the kernels see it: n_rooms x mwb_room_words(h) f32 words and n_segs x 4 f64.
 * Rectangle tasks: MWB_ROOM_WORDS words per room (min_x max_x min_z max_z, height, textures, neighbours, 4 x side).
 * MWB_TASK_YMAZE: MWB_POLY_ROOM_WORDS words per room - height, textures, n_edges | culled << 8, pad, then 4 edges of
 * 12 words: p.x p.z dir.x dir.z | n.x n.z portal_lo portal_hi | portal_max_y neighbour(int bits, -1 none) 0 0
 * (Room.outline / edge_dirs / edge_norms / portals, miniworld.py:75-218, as float32). */
#define MWB_ROOM_WORDS 24
#define MWB_POLY_ROOM_WORDS 52
int mwb_room_words(mwb_handle *h);
int mwb_get_geometry(mwb_handle *h, int env, float *rooms, int max_rooms, double *segs, int max_segs,
                     int *n_rooms, int *n_segs);

/* replaces: MiniWorldEnv.render_top_view(frame_buffer) (miniworld.py:1087-1158; `render(view='top')` 1317-1335) for the whole
 * batch: the floorplan from straight above, extents + 1 m widened to the frame's aspect, floors, box tops and the agent's
 * triangle.  out_dev: uint8 [N][height][width][3] in device memory, any frame size; enqueued on `stream`.  A display /
 * debugging view, not part of the step pipeline.
 * Entity tasks (MWB_TASK_PICKUPOBJS and later): the CURRENT entity list (as mwb_render draws it: an entity that left the list is not
 * drawn, a carried one is at its carry pose) in the reference's draw order - rooms, static entities, the others in list order, the
 * agent - the highest up-facing surface winning: box tops, the up-facing triangles of meshes (Gouraud-shaded, textured ones
 * modulated), the black top strip of image / text frames.  The agent's triangle is lit with the normal of the last glNormal3f issued
 * before it, vertex arrays changing nothing: (0, -1, 0) if the list holds a box or a frame, else the inward normal of the last wall
 * side of the last room (frozen).  Pinned to the reference's captured map-view streams within +-1 at >= 99.5 %
 * of the pixels (tests/test_gpu_top_view_ents.py); the agent's shade in the meshes-only case is parity unpinned against real
 * OpenGL.  Changes no later observation, reward or done. */
int mwb_render_top_view(mwb_handle *h, uint8_t *out_dev, int width, int height, void *stream);

/* replaces: MiniWorldEnv.render_obs(frame_buffer) / render_depth(frame_buffer) with ANOTHER frame buffer than the observation's
 * (miniworld.py:1160-1220) - in particular render(mode='rgb_array', view='agent'), which draws the agent's view into the
 * 800 x 600 `vis_fb` (miniworld.py:505,1317-1335): the current state of every env at width x height, same render spec as the
 * observation (8 samples per pixel; the reference asks for 16 in vis_fb - not modelled).  out_dev: uint8
 * [N][height][width][3], depth_dev: float32 [N][height][width] metres or NULL; device memory, enqueued on `stream`.  The view is
 * rendered in tiles (one workgroup each), so its size is not bound by LDS.  Not part of the step pipeline. */
int mwb_render_view(mwb_handle *h, uint8_t *out_dev, float *depth_dev, int width, int height, void *stream);

/* replaces: MiniWorldEnv.get_visible_ents() (miniworld.py:1222-1315) for the whole batch: per env a bit mask over the boxes in
 * entity-list order, bit b set iff box b's 0.2 m query cube passes its occlusion query (any of the 8 x W x H samples of the
 * observation frame nearer than the rooms and than the cubes of the boxes before it).  mask_dev: uint32 [N] in device memory;
 * enqueued on `stream`.  The reference never calls the function and holds no output of it (parity unpinned). */
int mwb_visible_ents(mwb_handle *h, uint32_t *mask_dev, void *stream);

/* ---- timing hooks used by bench.py -------------------------------------------------------- */
/* average device time (ms) of each kernel of the step pipeline since the last call (HIP events
 * recorded on the stream the kernels were launched on); names: "step","reset","prep","render".
 * enable: 0 off, 1 every pass, n > 1 every n-th pass (the seven events of a pass cost ~20 us of stream time). */
int mwb_timing_enable(mwb_handle *h, int enable);
int mwb_timing_read(mwb_handle *h, double *ms_step, double *ms_reset, double *ms_prep, double *ms_render,
                    int *n_samples);

#ifdef __cplusplus
}
#endif
#endif
