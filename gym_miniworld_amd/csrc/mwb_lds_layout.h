// mwb_lds_layout.h - where every region of a workgroup's dynamic LDS lives, for render_env and reset_kernel (mwb_kernels.hip).
//
// reset_kernel takes its pointers from ResetLds.  render_env keeps a pointer chain of its own (the reason is stated there): it steps
// through the same regions in the same order as render_lds() below, and both step by the same RL_*_BYTES size expressions, but
// that the two chains agree in ORDER is not checked by anything.  Every launch's byte count is a layout's `total`.
// Plain integers in, byte offsets out - the header compiles for the device, for the host side of hipcc and with a plain C++
// compiler (tests/test_lds_layout.py checks the layouts' order, alignment and pinned totals - not render_env's chain).
//
// Two invariants hold for both layouts:
//   * Sizing tile >= actual tile.  A tiled launch is sized by the host for (tile_w, tile_h); a workgroup at the frame's right or lower
//     edge lays out for its actual (tw, th) <= (tile_w, tile_h).  Every region's size grows with W and H or does not depend on
//     them, so the smaller layout ends at or before the sizing one's `total`.
//   * Regions a variant does not use get addresses but no bytes.  The entity regions (render: mesh queues, mleft, mdesc, batch
//     scratch; reset: the slot arrays) lie behind everything else; `total` covers them only when `ent` is set.  Box-task
//     instantiations compute these addresses and never dereference them.
#pragma once
#include <stddef.h>

#include "../../include/miniworld_batch.h"   // MWB_MAX_ENTS, MWB_NUM_MESHES

#if defined(__HIPCC__)
#define MWB_LDS_FN __host__ __device__ static inline
#else
#define MWB_LDS_FN static inline
#endif

#define WAVE 64
#define RENDER_THREADS 256
#define TILE_CX 16   // corner grid of one wave pass: 16 x 4 corners; marching down a strip it classifies 15 x 4 pixels
#define TILE_CY 4
#define QUEUE_CAP 128   // entries per wave of the 8-sample and the interior pixel queues
#define ITEM_RES_BYTES(W) ((((W) + TILE_CX - 2) / (TILE_CX - 1)) * 4 * 16)   // n_strips x 4 quarters x uint4
#define MQ_CAP 320     // mesh-pixel queue entries per wave: batches wait for the end of the frame, where all waves share them
#define MB_HALF 4      // pixels_mesh: samples per round
#define MB_TASKS 320   //   (ray, mesh) pairs per round
// one wave's mesh batch scratch: slots [MB_HALF][WAVE] u64, pairs [MB_TASKS] u16, pixel coordinates [WAVE] u32, counter (padded to 16 B)
enum { MB_SLOTS_OFF = 0, MB_PAIRS_OFF = MB_SLOTS_OFF + MB_HALF * WAVE * 8, MB_PIX_OFF = MB_PAIRS_OFF + MB_TASKS * 2,
       MB_COUNT_OFF = MB_PIX_OFF + WAVE * 4, MB_WAVE_BYTES = MB_COUNT_OFF + 16 };
#define MWB_TEX_LDS_BYTES 80   // sizeof(TexLds): a static_assert beside the struct holds the two together
#define MWB_WROOM_BYTES 272    // sizeof(WRoom): likewise

MWB_LDS_FN size_t mwb_lds_align16(size_t b) { return (b + 15) & ~(size_t)15; }

// bytes of render_env's regions: the steps of render_lds() here and of render_env's pointer chain
#define RL_WAVES (RENDER_THREADS / WAVE)
#define RL_ROOMS_BYTES(R_max, room_words) (((size_t)(R_max) * (room_words) * 4 + 15) & ~(size_t)15)
#define RL_FC_BYTES(frame_words) ((size_t)(frame_words) * 4)
#define RL_TEX_BYTES(n_tex) ((size_t)MWB_TEX_LDS_BYTES * (n_tex))
#define RL_SYNC_BYTES (16 + 2 * RL_WAVES * sizeof(int))   // eye room, work-item counter; two leftover counts per wave
#define RL_QUEUE_BYTES (RL_WAVES * QUEUE_CAP * sizeof(unsigned short))
#define RL_IKEYS_BYTES (RL_WAVES * QUEUE_CAP * sizeof(unsigned))
#define RL_BEHIND_FB(fb, W, H) (((fb) + (size_t)(W) * (H) * 3 + 15) & ~(size_t)15)   // first aligned byte behind the W x H x 3 frame at offset fb
#define RL_MQUEUE_BYTES (RL_WAVES * MQ_CAP * sizeof(unsigned short))
#define RL_MLEFT_BYTES 16
#define RL_MDESC_BYTES (16 * MWB_NUM_MESHES)

// render_env.  Regions in address order; 16-byte aligned: rooms, item_res, fb, mqueues, mdesc (float4 / uint4 accesses).
struct RenderLds {
    size_t rooms;      // [R_max][room_words] f32
    size_t fc;         // [frame_words] f32 frame constants
    size_t tex;        // [n_tex] TexLds
    size_t sync;       // eye room, work-item counter (16 B), then two leftover counts per wave
    size_t queues;     // [waves][QUEUE_CAP] u16 8-sample pixels
    size_t ikeys;      // [waves][QUEUE_CAP] u32 interior pixels' surface keys
    size_t ipix;       // [waves][QUEUE_CAP] u16 interior pixels
    size_t item_res;   // per work item: uniform rows + their key (uint4)
    size_t fb;         // [W * H * 3] the frame, assembled here and stored in 16-byte pieces
    // entity tasks only
    size_t mqueues;    // [waves][MQ_CAP] u16 pixels a mesh may cover
    size_t mleft;      // their leftover counts (16 B)
    size_t mdesc;      // [MWB_NUM_MESHES] uint4
    size_t mb;         // [waves][MB_WAVE_BYTES] batch scratch, one wave's laid out by MB_*_OFF
    size_t total;      // bytes the launch asks for
};
MWB_LDS_FN RenderLds render_lds(int R_max, int room_words, int frame_words, int n_tex, bool ent, int W, int H) {
    RenderLds L;
    size_t off = RL_ROOMS_BYTES(R_max, room_words);
    L.rooms = 0;
    L.fc = off; off += RL_FC_BYTES(frame_words);
    L.tex = off; off += RL_TEX_BYTES(n_tex);
    L.sync = off; off += RL_SYNC_BYTES;
    L.queues = off; off += RL_QUEUE_BYTES;
    L.ikeys = off; off += RL_IKEYS_BYTES;
    L.ipix = off; off += RL_QUEUE_BYTES;
    L.item_res = off; off += (size_t)ITEM_RES_BYTES(W);
    L.fb = off; off = RL_BEHIND_FB(off, W, H);
    L.mqueues = off;
    L.mleft = L.mqueues + RL_MQUEUE_BYTES;
    L.mdesc = L.mleft + RL_MLEFT_BYTES;
    L.mb = L.mdesc + RL_MDESC_BYTES;
    L.total = mwb_lds_align16(ent ? L.mb + (size_t)RL_WAVES * MB_WAVE_BYTES : off);
    return L;
}
// what a render launch asks for: `total`, and on whole-frame box-task launches only MWB_DEBUG bits 8+ in units of 128 B (occupancy experiments)
MWB_LDS_FN size_t render_lds_launch_bytes(const RenderLds &L, bool tiled, bool ent, int debug_flags) {
    return L.total + (tiled || ent ? 0 : (size_t)(debug_flags >> 8) * 128);
}

// Queued pixels are packed as (py << shift) | px in 16 bits, shift = mwb_coord_bits(W): the kernel packs with it, the host refuses
// (or tiles) a frame that does not fit with mwb_pixel_queue_fits.
MWB_LDS_FN int mwb_coord_bits(int n) { return 32 - __builtin_clz((unsigned)(n > 1 ? n - 1 : 1)); }
static inline bool mwb_pixel_queue_fits(int W, int H) { return ((size_t)H << mwb_coord_bits(W)) <= 65536; }

// reset_kernel (one wave per env).  Behind the generator's state one region with two tenants, never both: Maze's depth-first
// search, or the entity tasks' slot arrays ([MWB_MAX_ENTS] each; e_text: the TextFrame's 8 character textures).
struct ResetLds {
    size_t rooms;      // [R_max] WRoom
    size_t cdf;        // [R_max] f64
    size_t seg_off;    // [R_max rounded up to 4] i32
    size_t key;        // [624] u32 MT19937 key
    size_t dfs;        // Maze: [cells + 1][3] i32 frames, then [cells] u8 visited flags; cells = rows x cols = (R_max + 1) / 2
    size_t e_x, e_y, e_z, e_dir, e_size, e_rad, e_hgt, e_scale, e_bias /* [3][..] */;   // f64
    size_t e_meta, e_f32, e_col, e_text;                                                // i32
    size_t total;
};
MWB_LDS_FN ResetLds reset_lds(int R_max, bool ent, bool maze) {
    const size_t E = MWB_MAX_ENTS, cells = (size_t)(R_max + 1) / 2;
    ResetLds L;
    L.rooms = 0;
    L.cdf = (size_t)R_max * MWB_WROOM_BYTES;
    L.seg_off = L.cdf + (size_t)R_max * 8;
    L.key = L.seg_off + (size_t)((R_max + 3) & ~3) * 4;
    const size_t overlay = L.key + 624 * 4;
    L.dfs = overlay;
    L.e_x = overlay; L.e_y = L.e_x + E * 8; L.e_z = L.e_y + E * 8; L.e_dir = L.e_z + E * 8; L.e_size = L.e_dir + E * 8;
    L.e_rad = L.e_size + E * 8; L.e_hgt = L.e_rad + E * 8; L.e_scale = L.e_hgt + E * 8; L.e_bias = L.e_scale + E * 8;
    L.e_meta = L.e_bias + 3 * E * 8; L.e_f32 = L.e_meta + E * 4; L.e_col = L.e_f32 + E * 4; L.e_text = L.e_col + E * 4;
    size_t end = overlay;
    if (maze) end = L.dfs + (cells + 1) * 12 + cells + 4;   // + 4: slack the size has always had; kept so that Maze's LDS size stays what the profiles were taken at
    if (ent) end = L.e_text + 8 * 4;
    L.total = mwb_lds_align16(end);
    return L;
}
