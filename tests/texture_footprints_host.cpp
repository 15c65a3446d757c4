// Host build of gym_miniworld_amd/csrc/mwb_texture_host.h for tests/test_texture_footprints.py: one pyramid at a time, its
// plain levels and its footprint tables handed out as they are.
#include "../gym_miniworld_amd/csrc/mwb_texture_host.h"

static std::vector<std::vector<uint32_t>> g_levels;
static std::vector<uint32_t> g_all;
static uint32_t g_off[64];

extern "C" {
// base_entries: entries already in the buffer (another texture's), so that offsets are checked away from zero
int fp_build(const uint8_t *rgb, int w, int h, int base_entries) {
    build_mips(rgb, w, h, g_levels);
    g_all.assign((size_t)base_entries * 4, 0xDEADBEEFu);
    if (g_levels.size() > 64) return -1;
    append_pyramid_footprints(g_levels, w, h, g_off, g_all);
    return (int)g_levels.size();
}
long fp_level_texels(int l) { return (long)g_levels[l].size(); }
void fp_level_copy(int l, uint32_t *out) { for (size_t i = 0; i < g_levels[l].size(); i++) out[i] = g_levels[l][i]; }
long fp_level_off(int l) { return (long)g_off[l]; }
long fp_total_words() { return (long)g_all.size(); }
void fp_table_copy(uint32_t *out) { for (size_t i = 0; i < g_all.size(); i++) out[i] = g_all[i]; }
long fp_pyramid_entries(int w, int h) { return (long)pyramid_footprint_entries(w, h); }
long fp_entries(int w, int h) { return (long)footprint_entries(w, h); }
}
