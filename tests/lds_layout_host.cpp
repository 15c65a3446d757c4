// Host build of gym_miniworld_amd/csrc/mwb_lds_layout.h for tests/test_lds_layout.py: the layouts' fields as arrays of longs, in
// the order of the structs, and the constants the test sizes the regions with.
#include "../gym_miniworld_amd/csrc/mwb_lds_layout.h"

extern "C" {
int lds_render(int R_max, int room_words, int frame_words, int n_tex, int ent, int W, int H, long *out) {
    const RenderLds L = render_lds(R_max, room_words, frame_words, n_tex, ent != 0, W, H);
    const size_t f[] = {L.rooms, L.fc, L.tex, L.sync, L.queues, L.ikeys, L.ipix, L.item_res, L.fb, L.mqueues, L.mleft, L.mdesc, L.mb, L.total};
    const int n = (int)(sizeof(f) / sizeof(f[0]));
    for (int i = 0; i < n; i++) out[i] = (long)f[i];
    return n;
}
int lds_reset(int R_max, int ent, int maze, long *out) {
    const ResetLds L = reset_lds(R_max, ent != 0, maze != 0);
    const size_t f[] = {L.rooms, L.cdf, L.seg_off, L.key, L.dfs, L.e_x, L.e_y, L.e_z, L.e_dir, L.e_size, L.e_rad, L.e_hgt, L.e_scale,
                        L.e_bias, L.e_meta, L.e_f32, L.e_col, L.e_text, L.total};
    const int n = (int)(sizeof(f) / sizeof(f[0]));
    for (int i = 0; i < n; i++) out[i] = (long)f[i];
    return n;
}
long lds_launch_bytes(int R_max, int room_words, int frame_words, int n_tex, int ent, int W, int H, int tiled, int debug_flags) {
    return (long)render_lds_launch_bytes(render_lds(R_max, room_words, frame_words, n_tex, ent != 0, W, H), tiled != 0, ent != 0, debug_flags);
}
int lds_pixel_queue_fits(int W, int H) { return mwb_pixel_queue_fits(W, H) ? 1 : 0; }
int lds_coord_bits(int n) { return mwb_coord_bits(n); }
// waves, QUEUE_CAP, MQ_CAP, MB_HALF, MB_TASKS, MB_WAVE_BYTES and the four offsets inside it, texture descriptor bytes, WRoom bytes, entity slots, meshes, strip width
int lds_constants(long *out) {
    const long c[] = {RENDER_THREADS / WAVE, QUEUE_CAP, MQ_CAP, MB_HALF, MB_TASKS, MB_WAVE_BYTES, MB_SLOTS_OFF, MB_PAIRS_OFF, MB_PIX_OFF, MB_COUNT_OFF, MWB_TEX_LDS_BYTES, MWB_WROOM_BYTES,
                      MWB_MAX_ENTS, MWB_NUM_MESHES, TILE_CX - 1};
    const int n = (int)(sizeof(c) / sizeof(c[0]));
    for (int i = 0; i < n; i++) out[i] = c[i];
    return n;
}
}
