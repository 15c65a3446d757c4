"""The LDS layouts of render_env and reset_kernel (gym_miniworld_amd/csrc/mwb_lds_layout.h), built for the host.  Every launch's
byte count is a layout's `total`, and reset_kernel takes its pointers from ResetLds, so for those a mistake can only be in the
header: a region that overlaps its neighbour or sits at an address its vector accesses cannot use, a `total` that ends before
the last region does (an out-of-bounds LDS access) or that grew (31 968 B is what lets five Maze workgroups share a CU).
NOT covered: render_env walks the regions of RenderLds with a pointer chain of its own.  It steps by the header's RL_*_BYTES
sizes and MB_*_OFF offsets, so a size cannot drift, but a region added, dropped or reordered in one chain only passes this
test.  The sizes the regions need are stated here once more, on purpose: from what the kernels store in them."""
import ctypes
import math

import pytest

from lds_host import build_lds_host, frame_words

RENDER_FIELDS = ["rooms", "fc", "tex", "sync", "queues", "ikeys", "ipix", "item_res", "fb", "mqueues", "mleft", "mdesc", "mb", "total"]
RESET_FIELDS = ["rooms", "cdf", "seg_off", "key", "dfs", "e_x", "e_y", "e_z", "e_dir", "e_size", "e_rad", "e_hgt", "e_scale",
                "e_bias", "e_meta", "e_f32", "e_col", "e_text", "total"]
CONSTANTS = ["waves", "queue_cap", "mq_cap", "mb_half", "mb_tasks", "mb_wave_bytes", "mb_slots", "mb_pairs", "mb_pix", "mb_count", "tex_bytes", "wroom_bytes", "max_ents", "num_meshes", "strip_w"]


# name: R_max, room words, frame words, textures, entity task, W, H (the frame, or the tile a launch is sized for), pinned total
RENDER = {
    "maze8x8": (127, 24, frame_words(1), 7, 0, 80, 60, 31968),            # DESIGN.md's figure: five workgroups per CU
    "ymaze": (6, 52, frame_words(1), 7, 0, 80, 60, 21024),
    "hallway_view_tile": (1, 24, frame_words(1), 7, 0, 75, 60, 18912),
    "tmaze_two_box": (2, 24, frame_words(2), 7, 0, 80, 60, 20096),
    "putnext_six_box": (1, 24, frame_words(6), 7, 0, 80, 60, 20544),
    "sim2real_17_textures": (1, 24, frame_words(1), 17, 0, 80, 60, 20672),
    "pickupobjs": (1, 24, frame_words(20), 25, 1, 80, 60, 38400),
    "pickupobjs_tile_40x30": (1, 24, frame_words(20), 25, 1, 40, 30, 27408),
}
# name: R_max, entity task, Maze, pinned total
RESET = {"maze8x8": (127, 0, 1, 39424), "fourrooms": (8, 0, 0, 4768), "pickupobjs": (1, 1, 0, 4832)}


@pytest.fixture(scope="module")
def host():
    return build_lds_host()   # tests/lds_host.py: shared with test_gpu_frame_sizes.py


@pytest.fixture(scope="module")
def K(host):
    buf = (ctypes.c_long * 32)()
    assert host.lds_constants(buf) == len(CONSTANTS)
    return dict(zip(CONSTANTS, buf))


def render(host, R_max, room_words, fw, n_tex, ent, W, H):
    buf = (ctypes.c_long * 32)()
    assert host.lds_render(R_max, room_words, fw, n_tex, ent, W, H, buf) == len(RENDER_FIELDS)
    return dict(zip(RENDER_FIELDS, buf))


def reset(host, R_max, ent, maze):
    buf = (ctypes.c_long * 32)()
    assert host.lds_reset(R_max, ent, maze, buf) == len(RESET_FIELDS)
    return dict(zip(RESET_FIELDS, buf))


def render_regions(K, L, R_max, room_words, fw, n_tex, ent, W, H):
    """(name, first byte, bytes the kernel touches, alignment its accesses need), in address order; the entity regions only for an entity task"""
    wv = K["waves"]
    regs = [("rooms", L["rooms"], R_max * room_words * 4, 16),                      # staged as float4
            ("fc", L["fc"], fw * 4, 4),
            ("tex", L["tex"], n_tex * K["tex_bytes"], 4),
            ("sync", L["sync"], 16 + 2 * wv * 4, 4),
            ("queues", L["queues"], wv * K["queue_cap"] * 2, 2),
            ("ikeys", L["ikeys"], wv * K["queue_cap"] * 4, 4),
            ("ipix", L["ipix"], wv * K["queue_cap"] * 2, 2),
            ("item_res", L["item_res"], -(-W // K["strip_w"]) * 4 * 16, 16),        # uint4 per (strip, quarter)
            ("fb", L["fb"], W * H * 3, 16)]                                         # leaves as uint4
    if ent:
        regs += [("mqueues", L["mqueues"], wv * K["mq_cap"] * 2, 2),
                 ("mleft", L["mleft"], wv * 4, 4),
                 ("mdesc", L["mdesc"], K["num_meshes"] * 16, 16),                   # uint4 per mesh
                 ("mb", L["mb"], wv * K["mb_wave_bytes"], 8)]                       # every wave's slots are 64-bit words
    return regs


def check_regions(regs, total):
    end = 0
    for name, off, size, align in regs:
        assert off >= end, (name, "overlaps the region before it")
        assert off % align == 0, (name, off, align)
        end = off + size
    assert end <= total, (regs[-1][0], end, total)
    assert total % 16 == 0


@pytest.mark.parametrize("name", sorted(RENDER))
def test_render_regions_are_ordered_aligned_and_inside_total(host, K, name):
    cfg = RENDER[name][:7]
    L = render(host, *cfg)
    check_regions(render_regions(K, L, *cfg), L["total"])
    if not cfg[4]:   # a box task gets no bytes for the entity regions: total ends with the frame, rounded up
        assert L["total"] == (L["fb"] + cfg[5] * cfg[6] * 3 + 15) // 16 * 16
    # one wave's batch scratch: [MB_HALF][64] u64 slots, [MB_TASKS] u16 pairs, [64] u32 pixel coordinates, the counter
    wave = [("mb_slots", K["mb_slots"], K["mb_half"] * 64 * 8, 8), ("mb_pairs", K["mb_pairs"], K["mb_tasks"] * 2, 2),
            ("mb_pix", K["mb_pix"], 64 * 4, 4), ("mb_count", K["mb_count"], 4, 4)]
    assert K["mb_wave_bytes"] % 16 == 0
    check_regions(wave, K["mb_wave_bytes"])


@pytest.mark.parametrize("name", sorted(RENDER))
def test_render_totals_are_pinned(host, name):
    assert render(host, *RENDER[name][:7])["total"] == RENDER[name][7]


def test_debug_padding_only_on_whole_frame_box_task_launches(host):
    """MWB_DEBUG bits 8+ ask for units of 128 B on top of the layout; bits 0-7 are other switches"""
    maze, ents = RENDER["maze8x8"][:7], RENDER["pickupobjs"][:7]
    assert host.lds_launch_bytes(*maze, 0, 0) == host.lds_launch_bytes(*maze, 0, 255) == 31968
    assert host.lds_launch_bytes(*maze, 0, (2 << 8) | 1) == 32224   # Maze with 256 B of padding
    assert host.lds_launch_bytes(*maze, 1, 2 << 8) == 31968         # a tiled launch gets none
    assert host.lds_launch_bytes(*ents, 0, 2 << 8) == 38400         # nor does an entity task
    assert host.lds_launch_bytes(*RENDER["pickupobjs_tile_40x30"][:7], 1, 2 << 8) == 27408


@pytest.mark.parametrize("name,tile", [("hallway_view_tile", (75, 60)), ("pickupobjs_tile_40x30", (40, 30)), ("maze8x8", (75, 60))])
def test_a_smaller_tile_ends_inside_the_sizing_tile(host, K, name, tile):
    """the host sizes a tiled launch for (tile_w, tile_h); the workgroups at the right and lower edge lay out for less"""
    cfg = RENDER[name][:5]
    total = render(host, *cfg, *tile)["total"]
    for tw in range(1, tile[0] + 1):
        for th in range(1, tile[1] + 1):
            regs = render_regions(K, render(host, *cfg, tw, th), *cfg, tw, th)
            assert regs[-1][1] + regs[-1][2] <= total, (tw, th)


@pytest.mark.parametrize("name", sorted(RESET))
def test_reset_regions_are_ordered_aligned_and_inside_total(host, K, name):
    R_max, ent, maze, _ = RESET[name]
    L = reset(host, R_max, ent, maze)
    E, cells = K["max_ents"], (R_max + 1) // 2
    common = [("rooms", L["rooms"], R_max * K["wroom_bytes"], 16), ("cdf", L["cdf"], R_max * 8, 8), ("seg_off", L["seg_off"], R_max * 4, 4),
              ("key", L["key"], 624 * 4, 4)]
    # behind the key, two tenants of one region (an overlay on purpose): Maze's search, the entity tasks' slot arrays
    dfs = [("dfs", L["dfs"], (cells + 1) * 3 * 4 + cells, 4)]   # [cells + 1] frames of 3 ints, then a flag per cell
    ents = [(n, L[n], E * 8, 8) for n in ("e_x", "e_y", "e_z", "e_dir", "e_size", "e_rad", "e_hgt", "e_scale")] + [("e_bias", L["e_bias"], 3 * E * 8, 8)] + \
           [(n, L[n], E * 4, 4) for n in ("e_meta", "e_f32", "e_col")] + [("e_text", L["e_text"], 8 * 4, 4)]
    assert L["dfs"] == L["e_x"] == L["key"] + 624 * 4
    check_regions(common + (dfs if maze else ents if ent else []), L["total"])
    # whoever is not a tenant is still laid out in order and aligned - and simply gets no bytes
    check_regions(common + dfs, 1 << 62)
    check_regions(common + ents, 1 << 62)


@pytest.mark.parametrize("name", sorted(RESET))
def test_reset_totals_are_pinned(host, name):
    R_max, ent, maze, total = RESET[name]
    assert reset(host, R_max, ent, maze)["total"] == total


def test_pixel_queue_predicate(host):
    """a queued pixel is (py << ceil(log2 W)) | px in 16 bits"""
    assert host.lds_pixel_queue_fits(256, 256) == 1   # the limit case: 256 << 8 == 65536
    assert host.lds_pixel_queue_fits(257, 256) == 0
    assert host.lds_pixel_queue_fits(80, 60) == 1     # a whole frame per workgroup
    assert host.lds_pixel_queue_fits(320, 240) == 0   # rendered in tiles
    # W = 1 packs with one bit, as the kernel does
    assert host.lds_coord_bits(1) == 1 and host.lds_pixel_queue_fits(1, 32768) == 1 and host.lds_pixel_queue_fits(1, 32769) == 0
    for W in list(range(2, 300)) + [511, 512, 513, 800, 4096]:
        bits = math.ceil(math.log2(W))
        assert host.lds_coord_bits(W) == bits, W
        for H in (1, 59, 60, 65536 >> bits, (65536 >> bits) + 1, 600):
            assert host.lds_pixel_queue_fits(W, H) == int((H << bits) <= 65536), (W, H)
