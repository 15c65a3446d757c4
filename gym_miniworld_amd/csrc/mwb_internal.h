// mwb_internal.h - data layout shared by the host API (mwb_api.hip) and the kernels (mwb_kernels.hip).
//
// HBM layout (one handle = one GPU's shard of N environments), structure-of-arrays:
//   sim  : per-env f64 pose / episode parameters (arrays of N), i32 counters, u8 flags
//   rng  : per-env MT19937 state, N x 625 u32 (624 key words + position), env-major
//   rooms: per-env room table, N x R_max x MWB_ROOM_WORDS (24) f32 words (render kernel stages it in LDS)
//   segs : collision segments, S_max x 4 x N f64 (a.x a.z b.x b.z; segment-major, env-minor so that
//          one-env-per-lane reads coalesce), reference order per env
//   frame: per-env render constants (camera basis, lit colours, box frames), N x frame_words f32
//   tex  : RGBA8 mip pyramids of the 7 textures, shared by all envs (L2 / Infinity Cache resident)
//   out  : obs u8 [N,H,W,3] or [N,3,W,H], depth f32 [N,H,W], reward f32/f64 [N], done u8 [N]
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/miniworld_batch.h"
#include "mwb_seg_groups.h"

#define MWB_MT_WORDS 625   // 624 key words + pos
#define MWB_MAX_TEX MWB_NUM_TEXTURES
#define MWB_MAX_LEVELS 12
#define MWB_MAX_BOXES 6   // box-only tasks (templated step / render kernels); entity tasks: MWB_MAX_ENTS slots
#define MWB_RESET_MAX_BLOCKS 4096   // largest grid reset_kernel is launched with
#define MWB_ENT_AGENT 255 // the agent's entry in an env's entity order list
#define MWB_ORDER_STRIDE 24   // bytes per env of d.ent_order (MWB_MAX_ENTS + 1 entries, padded)
// frame constants: 36 fixed words, then one block of FC_BOX_STRIDE words per box; d.frame_words = that, rounded up to 4

// room table: 24 f32 words (96 B) per room; ints stored as bit patterns
//   0-3  min_x max_x min_z max_z
//   4    wall height          5  textures wall | floor << 8 | ceil << 16, bits 24-27: wall-u runs backwards on side s
//   6    neighbour room behind the portal of side 0 | side 1 << 16 (0xFFFF = no portal)     7  sides 2 | 3 << 16
//   8+4s lo hi max_y u_org of side s (0:+x east, 1:-z north, 2:-x west, 3:+z south): portal extent along the
//        side's axis and in y (min_y is 0 in every supported task - enforced by reset_kernel), origin of
//        the wall texture's u coordinate
#define RW_MINX 0
#define RW_MAXX 1
#define RW_MINZ 2
#define RW_MAXZ 3
#define RW_HEIGHT 4
#define RW_TEX 5
#define RW_NBR01 6
#define RW_NBR23 7
#define RW_SIDE0 8
#define RW_SIDE_WORDS 4
#define RS_LO 0
#define RS_HI 1
#define RS_MAXY 2
#define RS_UORG 3
#define RW_NO_NBR 0xFFFFu

// polygon room table (MWB_TASK_YMAZE): MWB_POLY_ROOM_WORDS = 52 f32 words per room
//   0 wall height   1 textures (as RW_TEX, no flip bits)   2 n_edges | culled << 8   3 pad
//   4 + 12 k, edge k (a missing 4th edge has n = (0, 0): never an exit, never excludes the eye):
//     p.x p.z dir.x dir.z | n.x n.z lo hi | max_y nbr 0 0   nbr: room behind the portal as int bits, -1 none; a portal into a
//     "culled" connector (reversed winding, nothing of it is drawn) points on to the room behind the connector
#define PW_HEIGHT 0
#define PW_TEX 1
#define PW_FLAGS 2
#define PW_EDGE0 4
#define PW_EDGE_WORDS 12

// frame-constant word offsets
#define FC_EYE 0
#define FC_F 3
#define FC_S 6
#define FC_U 9
#define FC_TW 12
#define FC_TH 13
#define FC_SKY 14
#define FC_LIT_FLOOR 17
#define FC_LIT_CEIL 20
#define FC_LIT_WALL 23   // 4 x 3
#define FC_LIGHT_DIR 23  // polygon rooms (d.poly): the light itself instead of the four axis-aligned wall colours -
#define FC_LIGHT_AMB 26  //   a wall's colour is computed from its edge normal when it is shaded
#define FC_LIGHT_DIF 29
#define FC_BOX_IN_VIEW 35      // != 0 if some box's footprint-inflated sphere can meet the view cone
// per-box block of FC_BOX_STRIDE words starting at FC_LIT_BOX; box b at + b * FC_BOX_STRIDE
#define FC_BOX_STRIDE 34
#define FC_LIT_BOX 36    // 6 x 3
#define FC_BOX_POS 54
#define FC_BOX_C 57
#define FC_BOX_S 58
#define FC_BOX_HX 59
#define FC_BOX_HZ 60
#define FC_BOX_SY 61
#define FC_BOX_LO 62     // ray origin in box-local axes (3)
#define FC_CULL_OC 65    // box bounding-sphere centre minus eye (3)
#define FC_CULL_CC 68    // |oc|^2 - R^2
#define FC_CULL_CC_PIXEL 69   // same with R grown by a pixel footprint
#define MWB_FRAME_WORDS_FOR(n_boxes) ((36 + FC_BOX_STRIDE * (n_boxes) + 3) & ~3)
// Entity tasks: the same FC_BOX_STRIDE-word block per entity slot, read by kind.  FC_BOX_HX >= 0: a box (as above); -1: a mesh;
// -2: an image / text frame; an entity that has left the list has FC_CULL_CC = FC_CULL_CC_PIXEL = +inf (no ray ever passes its gate).
//   mesh  (offsets from the block's start = FC_LIT_BOX - 36): 0-2 light direction in the mesh's frame / scale, 3-5 Kd,
//         6-8 0.2 Kd + ambient Kd, 9-11 diffuse, 12 1 / scale, 13 geometry (int), 14 texture slot (int, -1 none), 15-17 + FC_BOX_SY: gate box;
//         FC_BOX_POS, FC_BOX_C, FC_BOX_S as for a box; FC_BOX_LO = the eye in the mesh's frame (rotated, / scale)
//   frame: 0-2 lit colour of the front, 3 depth, 4 half height, 5 half width, 6 character width, 7 characters (int),
//         8-15 texture slot per character (int, -1 = blank); FC_BOX_POS, C, S; FC_BOX_LO = the eye in the frame's axes
#define FE_MESH_LL 0
#define FE_MESH_KD 3
#define FE_MESH_AMB 6
#define FE_MESH_DIF 9
#define FE_MESH_INVS 12
#define FE_MESH_GEOM 13
#define FE_MESH_TEX 14
#define FE_MESH_BPAD 15   // gate box (below) grown by a pixel's footprint at the mesh's far side, in mesh units
#define FE_MESH_BHX 16    // a conservative box of the mesh in its own frame, for the interior-pixel gate: |x| <= BHX, |z| <= BHZ,
#define FE_MESH_BHZ 17    //   0 <= y <= FC_BOX_SY (objmesh.py re-centres every mesh: base at y = 0, x and z about the middle)
#define FE_FRAME_LIT 0
#define FE_FRAME_SX 3
#define FE_FRAME_HY 4
#define FE_FRAME_HZ 5
#define FE_FRAME_CW 6
#define FE_FRAME_NCH 7
#define FE_FRAME_TEX 8

// one mesh geometry in HBM (shared by all envs; L2 resident): BVH nodes (2 float4 each), triangle records in LEAF order
// (3 float4: v0.xyz e1.x | e1.yz e2.xy | e2.z, original index (int bits), 0, 0) and shading records by ORIGINAL index
// (4 float4: n0.xyz n1.x | n1.yz n2.xy | n2.z tc0.st tc1.s | tc1.t tc2.st 0)
struct MwbMeshDesc {
    int n_tris, n_nodes, tex_id;
    int n_orders;   // threadings of the hierarchy stored one after the other at node_off: 1, or 8 = one per sign pattern of the ray direction
    uint32_t node_off, tri_off, shade_off, tri2_off;   // float4 offsets into d.mesh_data; tri2 = the triangle records by ORIGINAL index (shading)
    float min_c[4], max_c[4];
};
struct MwbMeshDims { int geom, is_f32; double height, scale, radius; };
#define MWB_MAX_MESH_DIMS 16

struct MwbTexDesc {
    int w, h, n_levels;
    float sc_s, sc_t;                     // TEX_DENSITY / size (miniworld.py:17,30-31,58-63) as f32
    int pad[3];
    uint32_t level_off[MWB_MAX_LEVELS];   // first entry of the level's footprint table, in 16-byte entries of the shared texel buffer
};

struct MwbParam { double def[3], lo[3], hi[3]; };

// everything a kernel needs, passed by value
struct MwbDev {
    int N, task, W, H, want_depth, layout, domain_rand, max_episode_steps;
    int R_max, S_max, auto_reset;
    int n_boxes;       // 1; 2 for MWB_TASK_TMAZE_TWOBOX (box 0 red, box 1 blue) and SIM2REAL_PUSH (red, yellow); 6 for PUTNEXT (COLOR_NAMES order)
    int frame_words;   // MWB_FRAME_WORDS_FOR(n_boxes)
    int n_tex;         // leading texture slots the task can draw (7, or MWB_NUM_TEXTURES for the sim-to-real rinks)
    int split_envs;    // the last split_envs envs of a bulk render launch are rendered by two half-frame workgroups each
    int act_stride;    // int32 words between consecutive envs' actions: 1, or 2 when the caller hands over int64 actions
    int poly;          // rooms are general convex polygons (YMaze): polygon room table, POLY render kernels
    int room_words;    // f32 words per room of d.rooms: MWB_ROOM_WORDS or MWB_POLY_ROOM_WORDS
    int no_ceiling;    // the task's rooms have no ceiling (sim-to-real rinks): selects the NOCEIL render kernels
    double agent_radius;   // entity.py:451 (0.4), 0.11 in the sim-to-real rinks
    int debug_flags;   // MWB_DEBUG env var at mwb_create: bit0 = resolve every pixel with the full 8-sample path
    double task_args[4];
    MwbParam params[MWB_NPARAM];
    // sim state (f64 SoA)
    double *agent_x, *agent_z, *agent_dir;
    double *box_x, *box_z, *box_dir;   // [n_boxes][N]
    double *box_y;          // [n_boxes][N] 0 on the floor, the carry height while carried (miniworld.py:603-604)
    int32_t *carrying;      // [N] agent.carrying as a box index, or -1 (miniworld.py:682-702)
    double *box_color;      // [n_boxes][N][3]
    double *box_size;       // [n_boxes][N] Box edge length (0.8 unless the task draws it per episode)
    double *goal_dist;      // [N] SimToRealPush
    int64_t *episode_count, *task_step_count;   // [N] goal-alternation counters of the T-maze family (envs/tmaze.py)
    int32_t *goal_idx;      // [N]
    double *cam;            // [N][4] height, fwd_disp, pitch, fov_y
    double *sky_color, *light_pos, *light_color, *light_ambient;   // [N][3]
    int32_t *step_count, *n_rooms, *n_segs;
    double *seg_stage;   // reset_kernel's staging of an env's collision segments, MWB_RESET_MAX_BLOCKS x S_max x 4 (one row set per block)
    int32_t *n_rrooms;   // records in the env's room table: n_rooms, + 1 where a room with two openings on one wall was cut in two (reset_kernel)
    int32_t *error_flag;    // [1] set by reset_kernel when world generation hits a condition the reference asserts on
    uint8_t *reset_set;     // which envs are (re)generated in the current pass (set by step / mark_reset)
    int32_t *reset_list;    // [N] the same envs as a compact list (order arbitrary) ...
    int32_t *reset_count;   // [1] ... and its length; zeroed by clear_list_kernel at the end of every pass
    uint32_t *rng;          // [N][625]
    float *rooms;           // [N][R_max][room_words]
    double *segs;           // [S_max][4][N]
    float *frame;           // [N][frame_words]
    void *stk;              // fused frame stack (MWB_STACK_FUSED) or null: base of [N][stk_K][W][H] planes, f32 (stk_float) or u8;
    int stk_float, stk_C, stk_K, stk_pos;   // the window the frame being rendered belongs to starts at plane stk_pos
    int stk_cpf;            // channel planes per frame of that stack: 3, or 1 for a grey stack (MWB_STACK_GREY) fed from the grey frame
    double *world_ext;      // [N][4] min_x max_x min_z max_z of the floorplan (miniworld.py:576-579), written by reset_kernel
    const uint32_t *texels;
    const MwbTexDesc *tex_desc;   // [MWB_MAX_TEX] in device memory
    // outputs
    uint8_t *obs;
    float *depth, *reward;
    double *reward64;
    uint8_t *done;
    int32_t *ep_steps;
    float *grey;            // greyscale observations (mwb_grey_enable) or null: f32 [N][H][W] (HWC handles) / [N][W][H] (CWH), written with obs
    uint32_t *cost;         // [2N] s_memrealtime ticks (10 ns) the last bulk render spent on env e: whole frame at [2e], or the halves
    uint8_t *bucket;        // [N] scratch of order_kernel
    // blockIdx -> env maps of the bulk render, envs by decreasing measured frame cost (slow frames first), double-buffered
    // ON THE DEVICE so that a captured hipGraph keeps the whole mechanism: order_state[0] selects the map in use,
    // order_kernel fills the other one and raises order_state[1]; the next step_kernel flips the selection.
    int32_t *order_bufs[2]; // [N] each
    int32_t *order_state;   // [2] {map in use, the other map is complete}
    unsigned long long *wg_ts;   // [2 * (N + split_envs)] start / end s_memrealtime of every bulk render workgroup, or null (MWB_DEBUG bit 4)
    float *feature;         // [N][2]
    double *goal_pos;       // [N][3]
    // ---- entity tasks (task >= MWB_TASK_PICKUPOBJS): the general entity list.  Slot arrays are [n_boxes][N] like the box arrays
    // (box_x/y/z/dir = position and heading of any entity, box_size = Box edge / MeshEnt height, box_color = Box colour / mesh Kd)
    int ent_task;           // 1 for those tasks: step_ents_kernel, kind-aware prep, the ENT render kernels
    int step_pass;          // the frame being prepared is a step's own (an entity the task rule removed / respawned is still drawn)
    int32_t *ent_meta;      // [n_boxes][N] MWB_META_* word
    double *ent_radius, *ent_height, *ent_scale;   // [n_boxes][N]
    uint8_t *ent_order;     // [N][MWB_ORDER_STRIDE] self.entities as slots (MWB_ENT_AGENT = the agent), n_order entries
    int32_t *n_order;       // [N]
    double *task_f;         // [N] CollectHealth.health
    int32_t *task_i;        // [N] PickupObjs.num_picked_up
    int32_t *text_tex;      // [N][8] texture slot per character of the TextFrame
    int32_t *ovr_slot;      // [N] slot whose pose the step's frame takes from ovr_pose (-1 none): the entity as the frame saw it
    double *ovr_pose;       // [N][4] x y z dir
    const MwbMeshDesc *mesh_desc;   // [MWB_NUM_MESHES] in device memory
    const float4 *mesh_data;
    MwbMeshDims mesh_dims[MWB_MAX_MESH_DIMS];
    int n_mesh_dims;
    // ---- last-frame reuse (null / 0 when it is off: MWB_NO_FRAME_REUSE, or frames rendered in tiles).  A step that leaves an env's
    // pose, entities and episode as they were (a blocked move) would render the frame it rendered the step before: the bulk
    // pass copies that frame from a private cache instead (the outputs are the caller's to scribble on, so they cannot be it).
    uint8_t *frame_cache;   // [N][W*H*3] the last frame every env's workgroup(s) produced, in the handle's layout
    float *depth_cache;     // [N][W*H] its depth map (want_depth)
    uint8_t *frame_cached;  // [N] frame_cache[e] shows env e's current state: set by render_env's copy-out, cleared by the host's setters
    uint8_t *frame_same;    // [N] written by the step kernels every step: this step changed nothing env e's frame depends on AND
                            //     frame_cached[e] was set - the bulk pass of the same step copies instead of rendering
    int reuse_pass;         // the render launch belongs to a step (honours frame_same); 0: mwb_render / mwb_reset render everything
    unsigned long long *reuse_stats;   // [2] frames reused / rendered by step passes since mwb_frame_reuse_stats last read them
    int tile_w, tile_h;   // entity tasks: every frame is rendered as tiles of this size, one workgroup each (0: whole frames)
    unsigned long long *dbg_counters;   // [8] or null: walk_meshes counters (MWB_EXP bit 2)
    int exp_flags;   // MWB_EXP env var at mwb_create: bit 0 = meshes are never hit, bit 1 = flat grey mesh shading (timing experiments)
    // ---- work lists of a step's bulk render launch (mwb_dispatch_map.h), rebuilt by prep_kernel(mode 2) ahead of every such launch from
    // the order map in use, reset_set and frame_same: dispatch scratch like order_bufs, nothing carries over from step to step
    int32_t *render_list;   // [N] the envs the launch renders, dearest first; the first list_counts[0] entries are valid
    int32_t *reuse_list;    // [N] the envs whose last frame it copies; list_counts[1] entries
    int32_t *list_counts;   // [2]
    // ---- mwb_step_repeat (last on purpose: no other member's offset moves).  Null except in the launches of sub-steps 2..k of
    // such a call, where the step kernels leave env e untouched when frozen[e] is set (mwb_repeat_fold.h, repeat_fold_kernel)
    const uint8_t *frozen;  // [N]
    // ---- bounding boxes of the collision segments in groups of MWB_SEG_GROUP (mwb_seg_groups.h), written by reset_kernel beside
    // d.segs and read ahead of them by every circle-vs-walls loop: a group whose box excludes the point is not loaded
    float *seg_box;         // [ceil(S_max / MWB_SEG_GROUP)][4][N] min_x min_z max_x max_z, float32 rounded outwards; transposed like segs
    int no_seg_cull;        // MWB_NO_SEG_CULL=1 at mwb_create: every group passes (A/B and the tests of the cull itself)
    // worlds step_kernel culls (mwb_step_culls): the segments once more, env-major, so that the few groups an env does load are
    // 256 contiguous bytes each - out of the transposed block a single lane's group is 32 lines, 4 KB of traffic.  Null otherwise
    double *seg_rows;       // [N][S_max][4]
    // ---- mwb_terminal_enable (last on purpose, as frozen was).  Null otherwise.  Why the step ended env e's episode: MWB_END_CLOCK |
    // MWB_END_TASK, 0 where it goes on (and for a skip-masked env); written by the step kernels where they write done.  An output
    // of a pass, not state: not in the array list below, never copied
    uint8_t *end_cause;     // [N]
};
// step_kernel culls by group where a wave (it has STEP_PARTS = 8) would otherwise walk a chain of batches: more than 64 segments
MWB_SEG_HD static inline bool mwb_step_culls(int S_max) { return mwb_seg_groups(S_max) > 8; }

// ---- the per-env device arrays of MwbDev, each written down ONCE: mwb_create allocates from this list, mwb_copy_envs builds its
// descriptor table from it and mwb_copy_env_bytes sums it.  A new array is one new line here (and its member above), no second
// edit elsewhere; the line says whether a copied env needs it, so that an array which carries state from one pass to the next
// cannot be left out of the copy unnoticed - a copied env would be no twin of its source.
// Shapes: env-minor [rows][N][per] (agent_x [N], box_x [B][N], box_color [B][N][3], segs [S_max * 4][N]: one-env-per-lane reads
// coalesce) or env-major [N][count] (rng [N][625], rooms [N][R_max * words], cam [N][4]).
// Not per-env arrays, allocated by explicit lines in mwb_create: seg_stage (one row set per block of reset_kernel, scratch of one
// launch), error_flag, reset_count, order_state, list_counts, reuse_stats, wg_ts, dbg_counters, the texture and mesh descriptors,
// and the small outputs reward / reward64 / done / ep_steps / feature / goal_pos, which are parts of one allocation (`pack`).
struct MwbEnvArray {
    const char *name;
    bool minor;               // env-minor [rows][N][per]; otherwise env-major [N][per], rows == 1
    uint32_t rows;
    size_t per;
    const char *not_copied;   // null: state a later kernel reads, mwb_copy_envs copies it; otherwise why a copied env does without
};
static inline size_t mwb_env_array_elems(const MwbEnvArray &a, size_t N) { return N * a.rows * a.per; }   // what mwb_create allocates

// f(s.member, d.member, MwbEnvArray) for every array that exists in handles of s's configuration; s and d differ in N at most
// (mwb_create passes its one MwbDev twice).  frame_reuse: the handle keeps the last-frame cache.
template <class Dev, class F>
static inline void mwb_for_each_env_array(Dev &s, Dev &d, bool frame_reuse, F &&f) {
#define MWB_MINOR(p, rows, per, when, why) if (when) f(s.p, d.p, MwbEnvArray{#p, true, (uint32_t)(rows), (size_t)(per), why})
#define MWB_MAJOR(p, count, when, why) if (when) f(s.p, d.p, MwbEnvArray{#p, false, 1u, (size_t)(count), why})
    const char *const COPIED = nullptr;
    const char *const OUTPUT = "an output of the last transition or render: the next one rewrites it";
    const char *const DISPATCH = "dispatch scratch: a heuristic or a work list rebuilt before every launch";
    const char *const CACHE = "the copy pass and the render it runs maintain the cached frames and their flags";
    const int B = s.n_boxes;
    const bool always = true, ent = s.ent_task != 0, depth = s.want_depth != 0;
    const size_t pixels = (size_t)s.W * s.H;
    MWB_MINOR(agent_x, 1, 1, always, COPIED); MWB_MINOR(agent_z, 1, 1, always, COPIED); MWB_MINOR(agent_dir, 1, 1, always, COPIED);
    MWB_MINOR(box_x, B, 1, always, COPIED); MWB_MINOR(box_z, B, 1, always, COPIED); MWB_MINOR(box_dir, B, 1, always, COPIED);
    MWB_MINOR(box_y, B, 1, always, COPIED); MWB_MINOR(box_color, B, 3, always, COPIED); MWB_MINOR(box_size, B, 1, always, COPIED);
    MWB_MINOR(carrying, 1, 1, always, COPIED); MWB_MINOR(goal_dist, 1, 1, always, COPIED);
    MWB_MINOR(episode_count, 1, 1, always, COPIED); MWB_MINOR(task_step_count, 1, 1, always, COPIED); MWB_MINOR(goal_idx, 1, 1, always, COPIED);
    MWB_MAJOR(cam, 4, always, COPIED); MWB_MAJOR(sky_color, 3, always, COPIED); MWB_MAJOR(light_pos, 3, always, COPIED);
    MWB_MAJOR(light_color, 3, always, COPIED); MWB_MAJOR(light_ambient, 3, always, COPIED);
    MWB_MINOR(step_count, 1, 1, always, COPIED); MWB_MINOR(n_rooms, 1, 1, always, COPIED); MWB_MINOR(n_segs, 1, 1, always, COPIED);
    MWB_MINOR(n_rrooms, 1, 1, always, COPIED);
    MWB_MAJOR(world_ext, 4, always, COPIED);
    MWB_MAJOR(rng, MWB_MT_WORDS, always, COPIED);
    MWB_MAJOR(rooms, (size_t)s.R_max * s.room_words, always, COPIED);
    MWB_MINOR(segs, s.S_max * 4, 1, always, COPIED);
    MWB_MINOR(seg_box, mwb_seg_groups(s.S_max) * 4, 1, always, "derived from segs: copy_seg_box_kernel rebuilds it from the copied segments");
    MWB_MAJOR(seg_rows, (size_t)s.S_max * 4, mwb_step_culls(s.S_max), "derived from segs: copy_seg_box_kernel rebuilds it from the copied segments");
    MWB_MINOR(ent_meta, B, 1, ent, COPIED); MWB_MINOR(ent_radius, B, 1, ent, COPIED); MWB_MINOR(ent_height, B, 1, ent, COPIED);
    MWB_MINOR(ent_scale, B, 1, ent, COPIED);
    MWB_MAJOR(ent_order, MWB_ORDER_STRIDE, ent, COPIED); MWB_MINOR(n_order, 1, 1, ent, COPIED);
    MWB_MINOR(task_f, 1, 1, ent, COPIED); MWB_MINOR(task_i, 1, 1, ent, COPIED); MWB_MAJOR(text_tex, 8, ent, COPIED);
    MWB_MINOR(ovr_slot, 1, 1, ent, COPIED); MWB_MAJOR(ovr_pose, 4, ent, COPIED);
    MWB_MAJOR(frame, s.frame_words, always, "prep_kernel rebuilds it before every render");
    MWB_MINOR(reset_set, 1, 1, always, "the copy pass sets and clears it around the render it runs");
    MWB_MINOR(reset_list, 1, 1, always, "the copy pass sets and clears it around the render it runs");
    MWB_MAJOR(obs, pixels * 3, always, OUTPUT); MWB_MAJOR(depth, pixels, depth, OUTPUT);
    MWB_MAJOR(cost, 2, always, DISPATCH); MWB_MINOR(bucket, 1, 1, always, DISPATCH);
    MWB_MINOR(order_bufs[0], 1, 1, always, DISPATCH); MWB_MINOR(order_bufs[1], 1, 1, always, DISPATCH);
    MWB_MINOR(render_list, 1, 1, always, DISPATCH); MWB_MINOR(reuse_list, 1, 1, always, DISPATCH);
    MWB_MAJOR(frame_cache, pixels * 3, frame_reuse, CACHE); MWB_MAJOR(depth_cache, pixels, frame_reuse && depth, CACHE);
    MWB_MINOR(frame_cached, 1, 1, frame_reuse, CACHE); MWB_MINOR(frame_same, 1, 1, frame_reuse, CACHE);
#undef MWB_MINOR
#undef MWB_MAJOR
}

// ---- mwb_copy_envs.  One descriptor per copied array: env e of the array is `rows` pieces of `elem` bytes, piece r at
// base + r * row_stride + e * elem.  An env-major block is one row of many bytes; an env-minor array is many rows N * elem
// apart - N differs between two handles, so both strides travel.
struct MwbCopyDesc {
    const char *src;
    char *dst;
    uint32_t rows, elem;
    uint64_t src_stride, dst_stride;
    uint32_t first_chunk;   // small rows (elem <= MWB_COPY_SMALL_ELEM): index of the array's first row chunk in copy_envs_kernel's grid
    uint32_t pad;
};
#define MWB_COPY_SMALL_ELEM 32   // pieces up to this size are copied one per lane (lane = pair); larger ones by a workgroup per pair
#define MWB_COPY_ROW_CHUNK 8     // rows of one small array a workgroup of copy_envs_kernel takes

// f(src base, dst base, rows, elem bytes, src row stride, dst row stride) for every array of the list that a copy moves
template <class F>
static inline void mwb_for_each_copied_array(const MwbDev &s, const MwbDev &d, F &&f) {
    mwb_for_each_env_array(s, d, false, [&](auto *sp, auto *dp, const MwbEnvArray &a) {   // (no array behind frame_reuse is copied)
        if (a.not_copied) return;
        const uint64_t elem = sizeof(*sp) * a.per;
        f((const char *)sp, (char *)dp, a.rows, (uint32_t)elem, a.minor ? elem * (uint64_t)s.N : 0, a.minor ? elem * (uint64_t)d.N : 0);
    });
}

// launch wrappers implemented in mwb_copy.hip (mwb_copy_envs).  `pairs`: per pair of the call {dst, src} as copy_validate_kernel
// left them - dst = -1 for a pair that is not carried out (rejected, or an identity pair)
void mwb_launch_copy_validate(const int32_t *dst_idx, const int32_t *src_idx, int count, int n_dst, int n_src, int same_handle,
                              int32_t *dst_pairs, uint8_t *src_mark, int2 *pairs, unsigned long long *rejected, hipStream_t s);
void mwb_launch_copy_envs(const MwbCopyDesc *table, int n_small, int small_chunks, int n_large, const int2 *pairs, int count, hipStream_t s);
// what: 0 = put the destinations on d's reset_set / reset_list (before the list render), 1 = take them off again and empty the
// list (after it), 2 = no render: their cached frames no longer show their state
void mwb_launch_copy_list(const MwbDev &d, const int2 *pairs, int count, int what, hipStream_t s);
// the destinations' segment group boxes (d.seg_box) from the segments mwb_launch_copy_envs has just copied
void mwb_launch_copy_seg_box(const MwbDev &d, const int2 *pairs, int count, hipStream_t s);
// the visible window of the frame stack: env_bytes_* = bytes between consecutive envs, off_* = byte offset of the window's first plane
void mwb_launch_copy_stack(char *dst, size_t env_bytes_dst, size_t off_dst, const char *src, size_t env_bytes_src, size_t off_src,
                           size_t window_bytes, const int2 *pairs, int count, hipStream_t s);

// launch wrapper implemented in mwb_repeat.hip (mwb_step_repeat): folds sub-step `sub` of a call into the handle's scratch
void mwb_launch_repeat_fold(const MwbDev &d, int sub, int last, int repeat, const uint8_t *skip, const int32_t *counts, double *sum,
                            int32_t *taken, uint8_t *same, uint8_t *frozen, hipStream_t s);

// ---- the rollout storage (mwb_rollout_enable; mwb_rollout_map.h says where a frame lives).  Passed by value to the kernels of
// mwb_rollout.hip; base and cursor are the host's (a captured graph of these launches must not be replayed).
struct MwbRollout {
    int N, T, nstack, R;    // envs, num_steps, frames per stacked observation, ring slots = T + nstack
    int grey;               // the ring holds the float32 grey frames (1 plane) instead of the uint8 RGB ones (3 planes)
    int base, cursor;       // slot of logical time 0; the last time pushed (-1: none since mwb_rollout_enable)
    size_t frame_bytes;     // one env's frame in a slot: W*H*3, or W*H*4 for grey
    char *ring;             // [R][N][frame_bytes]
    uint8_t *age;           // [T + 1][N]
    float *reward, *mask, *feature;   // [T][N], [T + 1][N], [T + 1][N][2]
    unsigned long long *rejected;     // [1] rows of gathers whose index was out of range since mwb_rollout_rejected last read it
};
// launch wrappers implemented in mwb_rollout.hip.  push: time t (> 0, or 0 with after_reset) from the handle's done / reward /
// feature outputs; gather: count > 0 rows, out 16-byte aligned, out_float = 1 for a grey ring
void mwb_launch_rollout_push(const MwbRollout &r, int t, int after_reset, const uint8_t *fresh_dev, const uint8_t *done, const float *reward,
                             const float *feature, hipStream_t s);
void mwb_launch_rollout_after_update(const MwbRollout &r, hipStream_t s);
void mwb_launch_rollout_gather(const MwbRollout &r, const int64_t *index, int count, void *out, int out_float, hipStream_t s);

// ---- the windowed gather (mwb_rollout_gather_window; mwb_rollout_window_map.h has the rule): a checked window over W x H frames,
// passed by value to the kernels of mwb_rollout_window.hip
struct MwbWindow {
    int W, H;                             // the stored frame
    int out_w, out_h, border;             // the output plane; 0 = edge replication, 1 = zeros
    int dx_lo, dx_hi, dy_lo, dy_hi;       // the ranges a row's offsets are clamped to
};
// launch wrappers implemented in mwb_rollout_window.hip.  offsets: int32 [count][2], 8-byte aligned; key = mwb_window_key(seed,
// call); gather: count > 0 rows, out 16-byte aligned, out_float = 1 for a grey ring
void mwb_launch_rollout_window_offsets(const MwbWindow &w, uint64_t key, const int64_t *index, int count, int32_t *offsets, hipStream_t s);
void mwb_launch_rollout_window(const MwbRollout &r, const MwbWindow &w, const int64_t *index, int count, const int32_t *offsets, void *out,
                               int out_float, hipStream_t s);

// ---- the rollout's learner half (mwb_rollout_learner_enable): the small columns of RolloutStorage and what is computed from them
struct MwbLearner {
    int64_t *action;                 // [T][N]
    float *log_prob, *value;         // [T][N], [T + 1][N]
    int32_t *taken;                  // [T][N] sub-steps of the transition t -> t + 1
    float *ret, *adv, *psi_ret;      // [T + 1][N], [T][N], [T + 1][N][2]
};
struct MwbReturnsTables;   // mwb_returns_scan.h
// launch wrappers implemented in mwb_rollout_learner.hip.  taken: the row of the push to time t (> 0), `taken` = NULL writes 1;
// returns: mode = MWB_RETURNS_*, next = next_value or next_psi, reward = the rows to use; gather_cols: count > 0
void mwb_launch_rollout_taken(const MwbRollout &r, const MwbLearner &l, int t, const int32_t *taken, hipStream_t s);
void mwb_launch_rollout_insert(const MwbRollout &r, const MwbLearner &l, int row, const int64_t *action, const int32_t *action_i32,
                               const float *log_prob, const float *value, hipStream_t s);
void mwb_launch_rollout_returns(const MwbRollout &r, const MwbLearner &l, int mode, const MwbReturnsTables &tab, const float *next,
                                const float *reward, hipStream_t s);
void mwb_launch_rollout_gather_cols(const MwbRollout &r, const MwbLearner &l, const int64_t *index, int count, const float *adv_src,
                                    float *out_f32, int64_t *out_action, hipStream_t s);

// ---- the episode monitor (mwb_monitor_enable; mwb_monitor_map.h says where a record of the log lives).  Passed by value to the
// kernels of mwb_monitor.hip.  Nothing of it lives on the host: the counters, the quota and the scan's scratch are device memory,
// so a captured graph of an update can be replayed.
#define MWB_MON_TOTAL 0       // counts64[]: episodes ever appended to the log
#define MWB_MON_DROPPED 1     //             episodes that ended with `partial` set
#define MWB_MON_REMAINING 0   // counts32[]: envs not retired
#define MWB_MON_QUOTA 1       //             the per-env quota (0 = none)
#define MWB_MON_BASE 2        //             slot of rank 0 of the last pass
#define MWB_MON_COUNT 3       //             loggable episodes of the last pass
struct MwbMonitor {
    int N, capacity, Q, n_waves;   // envs, log records, rows of the table, ceil(N / 64)
    double *run_return, *last_return;
    int32_t *run_len, *run_calls, *last_len, *last_calls, *finished;
    uint8_t *partial, *retired, *logged;   // logged: the last update appended an episode of env e
    double *log_return;
    int32_t *log_len, *log_calls, *log_env;
    double *tab_return;                    // [Q][N]
    int32_t *tab_len;                      // [Q][N]
    unsigned long long *counts64;          // [2] MWB_MON_TOTAL, MWB_MON_DROPPED
    uint32_t *counts32;                    // [4] MWB_MON_REMAINING .. MWB_MON_COUNT
    unsigned long long *wave_ballot;       // [n_waves] the loggable finishing lanes of wave w in the last pass
    uint32_t *wave_base;                   // [n_waves] loggable episodes of the last pass in waves before w
    uint32_t *wave_aux;                    // [n_waves] dropped episodes | envs not retired << 8 of wave w in the last pass
};
// launch wrappers implemented in mwb_monitor.hip.  update: the three launches of one pass; reward / done as given, taken = NULL
// counts 1 per call.  clear: mask = NULL names every env.  quota: validated by the API (0 .. Q)
void mwb_launch_monitor_update(const MwbMonitor &m, const uint8_t *skip, const double *reward, const uint8_t *done, const int32_t *taken, hipStream_t s);
void mwb_launch_monitor_clear(const MwbMonitor &m, const uint8_t *mask, int partial, hipStream_t s);
void mwb_launch_monitor_quota(const MwbMonitor &m, int quota, hipStream_t s);

// ---- terminal observations (mwb_terminal_enable; mwb_terminal_map.h says which row an ended env gets and where its history
// lies in the fused stack).  Passed by value to the kernels of mwb_terminal.hip.  Terminal depth maps are not produced.
struct MwbTerminal {
    int N, capacity;
    int nstack, cpf;          // frames per row and planes per frame: 1 / 3 without a stack, else the fused stack's
    int rows_float, grey;     // rows are float32 (else uint8); the newest group comes from `grey` (a grey stack) instead of `frames`
    size_t plane;             // W * H
    uint8_t *frames;          // [N][plane * 3] the terminal frames, in the handle's layout
    float *grey_frames;       // [N][plane] or null
    float *frame_consts;      // [N][frame_words] the terminal render's own frame constants
    uint8_t *cause;           // [N] = MwbDev::end_cause
    int32_t *row_of, *row_env, *count;   // [N], [capacity], [1]
    unsigned long long *dropped;         // [1] ended envs without a row since mwb_terminal_dropped last read it
    char *rows;               // [capacity][nstack * cpf * plane] u8 or f32
};
// launch wrappers implemented in mwb_terminal.hip.  rank: row_of / row_env / count / dropped from reset_set; stack: the rows of the
// envs rank listed - stk = the fused stack's base (null: no stack), stk_K planes per env, window at stk_pos; clear: count = 0,
// row_of = row_env = -1, cause = 0; bootstrap: reward_t / taken_t = row t of the rollout's columns (taken_t null: k = 1)
void mwb_launch_terminal_rank(const MwbTerminal &t, const uint8_t *reset_set, hipStream_t s);
void mwb_launch_terminal_stack(const MwbTerminal &t, const void *stk, int stk_K, int stk_pos, hipStream_t s);
void mwb_launch_terminal_clear(const MwbTerminal &t, hipStream_t s);
void mwb_launch_terminal_bootstrap(const MwbTerminal &t, const MwbReturnsTables &tab, float *reward_t, const int32_t *taken_t, const float *value_rows,
                                   hipStream_t s);

// ---- level sets (mwb_levels_enable; mwb_levels_map.h says which level an env takes and what its generator row becomes).  Passed
// by value to the kernels of mwb_levels.hip; every buffer is the handle's own allocation.  MwbDev knows nothing of it: the kernels
// take the arrays of MwbDev they touch as plain pointers.
struct MwbLevels {
    int N;
    int64_t L;                       // levels of the set, 1 .. 2^31 - 1
    uint64_t start_level;            // level i has the seed start_level + i ...
    const uint64_t *seeds;           // ... unless a table was given: [L], else null
    int64_t env_offset, env_stride;  // g = env_offset + e; SEQUENTIAL's stride
    const uint32_t *base;            // [624] init_genrand(19650218), built once on the host
    uint64_t *params;                // [2] mode, sampler_seed: device memory, so that a pass depends on no host state
    int32_t *index, *prev_index, *next_level;   // [N] each
    int64_t *episode_no;             // [N]
    unsigned long long *rejected;    // [1] TABLE requests out of range since mwb_levels_rejected last read it
    unsigned long long *tallies;     // [3][L] episodes, env steps, successes per level, or null
};
// launch wrappers implemented in mwb_levels.hip.  assign: every env of reset_list gets its level and its generator row (tally != 0:
// the level it leaves is tallied first, from done / reward64 / ep_steps); restart: episode_no = 0, optionally the tallies, mode
// and sampler seed; copy: index of the validated pairs {dst, src} (src_index null: the destinations' index becomes -1)
void mwb_launch_levels_assign(const MwbLevels &v, const int32_t *reset_list, const int32_t *reset_count, uint32_t *rng, const uint8_t *done,
                              const double *reward64, const int32_t *ep_steps, int tally, hipStream_t s);
void mwb_launch_levels_restart(const MwbLevels &v, int mode, uint64_t sampler_seed, int clear_tally, hipStream_t s);
void mwb_launch_levels_copy(int32_t *dst_index, const int32_t *src_index, const int2 *pairs, int count, hipStream_t s);

// launch wrappers implemented in mwb_kernels.hip
void mwb_launch_step(const MwbDev &d, const int32_t *actions, const uint8_t *skip_mask, hipStream_t s);   // entity tasks: step_ents_kernel
void mwb_launch_clear_list(const MwbDev &d, hipStream_t s);
void mwb_launch_order(const MwbDev &d, hipStream_t s);   // envs by decreasing measured frame cost -> the map not in use
void mwb_launch_mark_reset(const MwbDev &d, const uint8_t *mask, hipStream_t s);
void mwb_view_tile(int *w, int *h);   // the tile mwb_render_view (and large observations) are rendered in
void mwb_launch_reset(const MwbDev &d, int max_blocks, hipStream_t s);   // grid-strides over reset_list
// mode 0: every env; 1: only envs with reset_set; 2: only envs without (lets reset overlap the bulk render)
void mwb_launch_prep(const MwbDev &d, int mode, hipStream_t s);
// fixed: a step's bulk launch (mode 2) may take render_fixed_kernel where mwb_bulk_fixed_ok(d) holds and no grey output is on
void mwb_launch_render(const MwbDev &d, int mode, hipStream_t s, bool fixed = false);
bool mwb_bulk_fixed_ok(const MwbDev &d);   // default observation size, no MWB_DEBUG / MWB_EXP bit, a box task, whole frames
// cpf: channel planes per frame - 3 (fed from d.obs), or 1 (a grey stack, f32 only: fed from d.grey)
void mwb_launch_stack(const MwbDev &d, void *stack, int nstack, int dtype, int after_reset, hipStream_t s, int cpf = 3);
void mwb_launch_stack_slide(const MwbDev &d, void *stack, int nstack, int planes, int dtype, int pos, int from, int mode, hipStream_t s, int cpf = 3);
// RGB frames in device memory -> float32 grey, n_frames x plane pixels (mwb_grey_convert)
void mwb_launch_grey_convert(const uint8_t *rgb, float *grey, int n_frames, int plane, int layout, hipStream_t s);
void mwb_launch_intersect(const MwbDev &d, int env, int ent, double x, double z, double radius, int *result_dev, hipStream_t s);
void mwb_launch_visible(const MwbDev &d, uint32_t *mask_out, hipStream_t s);   // get_visible_ents for every env
int mwb_launch_render_view(const MwbDev &d, hipStream_t s);   // the agent's view at d.W x d.H in tiles; 0 ok, -1 LDS, -2 HIP
void mwb_launch_top_view(const MwbDev &d, uint8_t *out, int W, int H, hipStream_t s);   // render_top_view for every env, [N][H][W][3]
void mwb_launch_top_view_ents(const MwbDev &d, uint8_t *out, int W, int H, hipStream_t s);   // the same for the entity tasks (tiles)
int mwb_prepare_kernels(const MwbDev &d);   // 0 ok, -1 world too large for LDS, -2 HIP error, -3 frame too large for the pixel queue
size_t mwb_reset_lds_bytes(const MwbDev &d);
size_t mwb_render_lds_bytes(const MwbDev &d);
