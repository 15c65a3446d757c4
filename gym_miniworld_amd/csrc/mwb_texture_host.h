// Host side of the texture pyramids (plain C++, no HIP): the mip chain and the bilinear footprint tables the
// kernels fetch from.  Included by mwb_api.hip and by tests/texture_footprints_host.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

// Mip chain: level k+1 has dims max(1, n/2); each texel is the equal-weight mean (round half up) of
// the source texels it covers - 2x2 for even sizes (DESIGN.md render spec; restates
// glGenerateMipmap of opengl.py:98-99, whose filter GL leaves to the driver).
static inline void build_mips(const uint8_t *rgb, int w, int h, std::vector<std::vector<uint32_t>> &levels) {
    levels.clear();
    std::vector<uint32_t> cur((size_t)w * h);
    for (int y = 0; y < h; y++)   // flip: texture row 0 = bottom image row (pyglet upload order, opengl.py:85-96)
        for (int x = 0; x < w; x++) {
            const uint8_t *p = rgb + ((size_t)(h - 1 - y) * w + x) * 3;
            cur[(size_t)y * w + x] = p[0] | (p[1] << 8) | (p[2] << 16) | 0xFF000000u;
        }
    levels.push_back(cur);
    int sw = w, sh = h;
    while (sw > 1 || sh > 1) {
        int dw = sw > 1 ? sw / 2 : 1, dh = sh > 1 ? sh / 2 : 1;
        std::vector<uint32_t> nxt((size_t)dw * dh);
        const std::vector<uint32_t> &src = levels.back();
        for (int j = 0; j < dh; j++) {
            int j0 = (int)(((long long)j * sh) / dh), j1 = (int)((((long long)(j + 1) * sh) + dh - 1) / dh);
            for (int i = 0; i < dw; i++) {
                int i0 = (int)(((long long)i * sw) / dw), i1 = (int)((((long long)(i + 1) * sw) + dw - 1) / dw);
                uint32_t sum[4] = {0, 0, 0, 0};
                for (int y = j0; y < j1; y++)
                    for (int x = i0; x < i1; x++) {
                        uint32_t t = src[(size_t)y * sw + x];
                        sum[0] += t & 255u; sum[1] += (t >> 8) & 255u; sum[2] += (t >> 16) & 255u; sum[3] += t >> 24;
                    }
                uint32_t cnt = (uint32_t)((j1 - j0) * (i1 - i0));
                uint32_t o = 0;
                for (int c = 0; c < 4; c++) o |= ((sum[c] + cnt / 2) / cnt) << (8 * c);
                nxt[(size_t)j * dw + i] = o;
            }
        }
        levels.push_back(nxt);
        sw = dw; sh = dh;
    }
}

// Footprint table of one level (w x h texels, row-major): (w+1) x (h+1) entries of four texels (16 bytes).  Entry (I, J)
// serves the bilinear footprint whose lower-left texel is (i0, j0) = (I-1, J-1), i0 in [-1, w-1], j0 in [-1, h-1], with
// GL_REPEAT wrap already applied:  { L[j0][i0], L[j0][i0+1], L[j0+1][i0], L[j0+1][i0+1] }, indices mod h / mod w.
static inline size_t footprint_entries(int w, int h) { return (size_t)(w + 1) * (size_t)(h + 1); }

static inline void append_footprints(const uint32_t *L, int w, int h, std::vector<uint32_t> &out) {
    size_t o = out.size();
    out.resize(o + 4 * footprint_entries(w, h));
    for (int J = 0; J <= h; J++) {
        const int j0 = (J - 1 + h) % h, j1 = J % h;
        const uint32_t *r0 = L + (size_t)j0 * w, *r1 = L + (size_t)j1 * w;
        for (int I = 0; I <= w; I++) {
            const int i0 = (I - 1 + w) % w, i1 = I % w;
            out[o++] = r0[i0]; out[o++] = r0[i1]; out[o++] = r1[i0]; out[o++] = r1[i1];
        }
    }
}

// entries of the whole pyramid of a w x h texture (level l is max(1, w >> l) x max(1, h >> l))
static inline size_t pyramid_footprint_entries(int w, int h) {
    size_t n = 0;
    for (;;) {
        n += footprint_entries(w, h);
        if (w == 1 && h == 1) return n;
        w = w > 1 ? w / 2 : 1; h = h > 1 ? h / 2 : 1;
    }
}

// Appends the tables of every level of one pyramid to `all` (4 words per entry); level_off[l] = the level's first entry,
// counted in 16-byte entries from the start of `all`.
static inline void append_pyramid_footprints(const std::vector<std::vector<uint32_t>> &levels, int w, int h, uint32_t *level_off,
                                             std::vector<uint32_t> &all) {
    for (size_t l = 0; l < levels.size(); l++) {
        level_off[l] = (uint32_t)(all.size() / 4);
        append_footprints(levels[l].data(), w, h, all);
        w = w > 1 ? w / 2 : 1; h = h > 1 ? h / 2 : 1;
    }
}
