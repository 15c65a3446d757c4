// mwb_rollout_window.hip - the kernels of the windowed gather (mwb_rollout_window_offsets / mwb_rollout_gather_window): the
// stacked minibatch of mwb_rollout_gather with a per-row shift, crop or translate applied while the row is rebuilt from its single
// frames.  Which source pixel an output pixel shows and which offsets a row draws: mwb_rollout_window_map.h; where a frame lives:
// mwb_rollout_map.h.
//
//   rollout_window_offsets_kernel   one lane per row: a coalesced read of the index, two hashes, one 8-byte store of (dx, dy).
//   rollout_window_kernel           the hot path.  A work item is (row of the output, frame group, chunk of WINDOW_CHUNK quads); a
//                                   quad is four consecutive output pixels of one plane ([out_w][out_h], out_h contiguous;
//                                   out_w * out_h % 4 == 0, so no quad crosses a plane).  Index, validity, age, slot and the
//                                   clamped (dx, dy) are workgroup-uniform.  After a shift the source of an aligned output quad
//                                   starts at any byte of a 60-byte column, so the plain kernel's 16-byte loads do not carry
//                                   over: every lane reads its four source pixels one by one through the vector cache, at
//                                   coordinates clamped into the frame (edge replication is the clamp itself), all sixteen
//                                   loads of an item in flight before its first store; a zero border is a select at the store,
//                                   from a mask computed beside the loads (ZERO instantiations only).  The address arithmetic is
//                                   what the kernel costs, so out_h % 4 == 0 - every quad inside one column, a launch-uniform
//                                   fact - takes a path that clamps and multiplies once per quad, not once per pixel.  The
//                                   stores are the plain kernel's: a float4 per lane, 1 KB per wave instruction in one piece
//                                   (uint8 output: a dword per lane).  Grey frames move as float32 bit patterns.
// No LDS, no scratch; the only atomic is one add per rejected row.  Every offset into the ring and the output is 64-bit; inside
// one frame (at most 4 MiB) offsets are 32-bit.
#include "mwb_internal.h"
#include "mwb_rollout_map.h"
#include "mwb_rollout_window_map.h"

#define WINDOW_THREADS 256
#define WINDOW_UNROLL 4
#define WINDOW_CHUNK (WINDOW_THREADS * WINDOW_UNROLL)   // quads of one work item
#define WINDOW_MAX_BLOCKS 2048                          // 8 workgroups per CU; longer lists are grid-strided

__global__ void __launch_bounds__(WINDOW_THREADS) rollout_window_offsets_kernel(MwbWindow w, uint64_t key, const int64_t *__restrict__ index,
                                                                               int2 *__restrict__ offsets, uint32_t count) {
    const uint32_t i = blockIdx.x * WINDOW_THREADS + threadIdx.x;
    if (i >= count) return;
    int dx, dy;
    mwb_window_draw(key, index[i], w.dx_lo, w.dx_hi, w.dy_lo, w.dy_hi, &dx, &dy);
    offsets[i] = make_int2(dx, dy);
}

// what a row's work items share: the frame, the window, the row's clamped offsets
struct WindowRow {
    const uint8_t *src;     // the stored frame of this frame group
    int W, H, out_h, dx, dy;
    uint32_t plane_px;      // out_w * out_h
    uint64_t magic;         // mwb_window_div_magic(out_h)
};

// the four source pixels of quad q: byte values (RGB) or float32 bit patterns (grey), loaded at clamped coordinates and not touched
// here, so that nothing waits for them; ZERO: bit j of `zeros` = pixel j lies outside the frame.  COLUMN: out_h % 4 == 0
template <bool GREY, bool ZERO, bool COLUMN>
__device__ __forceinline__ void window_load_quad(const WindowRow &r, uint32_t q, uint4 &v, uint32_t &zeros) {
    const uint32_t p = q * 4;
    const uint32_t c = GREY ? 0u : (uint32_t)(p >= r.plane_px) + (uint32_t)(p >= 2 * r.plane_px);   // the plane (RGB: three of them)
    const uint32_t i = p - c * r.plane_px;
    const uint32_t x = mwb_window_div(i, r.magic), y = i - __umul24(x, (uint32_t)r.out_h);   // x, out_h <= 1024
    const uint32_t plane_off = __umul24(c, (uint32_t)(r.W * r.H));   // W * H <= 2^20
    auto load = [&](uint32_t off) -> uint32_t { return GREY ? ((const uint32_t *)r.src)[off] : (uint32_t)r.src[off]; };
    if (COLUMN) {   // one column: one clamp and one multiplication for the quad
        int in_x, in0, in1, in2, in3;
        const uint32_t col = plane_off + __umul24((uint32_t)mwb_window_axis((int)x, r.dx, r.W, &in_x), (uint32_t)r.H);
        v.x = load(col + (uint32_t)mwb_window_axis((int)y, r.dy, r.H, &in0));
        v.y = load(col + (uint32_t)mwb_window_axis((int)y + 1, r.dy, r.H, &in1));
        v.z = load(col + (uint32_t)mwb_window_axis((int)y + 2, r.dy, r.H, &in2));
        v.w = load(col + (uint32_t)mwb_window_axis((int)y + 3, r.dy, r.H, &in3));
        if (ZERO) zeros = in_x ? (uint32_t)(!in0) | ((uint32_t)(!in1) << 1) | ((uint32_t)(!in2) << 2) | ((uint32_t)(!in3) << 3) : 15u;
    } else {        // the next pixel of the quad may be the first of the next column
        uint32_t px = x, py = y, bit = 1u;
        zeros = 0u;
        auto pixel = [&]() -> uint32_t {
            int in_x, in_y;
            const uint32_t sx = (uint32_t)mwb_window_axis((int)px, r.dx, r.W, &in_x), sy = (uint32_t)mwb_window_axis((int)py, r.dy, r.H, &in_y);
            if (ZERO) { zeros |= (in_x && in_y) ? 0u : bit; bit <<= 1; }
            if (++py == (uint32_t)r.out_h) { py = 0; px++; }
            return load(plane_off + __umul24(sx, (uint32_t)r.H) + sy);
        };
        v.x = pixel(); v.y = pixel(); v.z = pixel(); v.w = pixel();
    }
}

template <bool OUT_FLOAT, bool GREY>
__device__ __forceinline__ void window_store_quad(char *dst, uint32_t q, uint4 v, uint32_t zeros) {
    if (zeros & 1u) v.x = 0u;
    if (zeros & 2u) v.y = 0u;
    if (zeros & 4u) v.z = 0u;
    if (zeros & 8u) v.w = 0u;
    if (GREY) *(uint4 *)(dst + (size_t)q * 16) = v;
    else if (OUT_FLOAT) *(float4 *)(dst + (size_t)q * 16) = make_float4((float)v.x, (float)v.y, (float)v.z, (float)v.w);   // exact: 0 .. 255
    else *(uint32_t *)(dst + (size_t)q * 4) = v.x | (v.y << 8) | (v.z << 16) | (v.w << 24);
}

// the rows of one workgroup
template <bool OUT_FLOAT, bool GREY, bool ZERO, bool COLUMN>
__device__ __forceinline__ void window_rows(const MwbRollout &r, const MwbWindow &w, uint64_t magic, const int64_t *__restrict__ index,
                                            const int2 *__restrict__ offsets, char *__restrict__ out, uint32_t quads, uint32_t chunks, uint32_t count) {
    constexpr int OUT_BYTES = (OUT_FLOAT || GREY) ? 16 : 4;   // of one quad
    const uint32_t k = blockIdx.x / chunks, chunk = blockIdx.x - k * chunks;
    const uint32_t q0 = chunk * WINDOW_CHUNK + threadIdx.x;
    const uint32_t q1 = q0 + WINDOW_THREADS, q2 = q0 + 2 * WINDOW_THREADS, q3 = q0 + 3 * WINDOW_THREADS;
    WindowRow wr;
    wr.W = w.W; wr.H = w.H; wr.out_h = w.out_h; wr.plane_px = (uint32_t)(w.out_w * w.out_h); wr.magic = magic;
    const bool small = ((int64_t)r.cursor + 1) * r.N <= 0x7fffffffLL;   // every valid index fits 32 bits: no 64-bit division
    for (uint32_t row = blockIdx.y; row < count; row += gridDim.y) {   // index, age, slot and the offsets are workgroup-uniform
        const int64_t idx = index[row];
        int slot = -1;
        size_t e = 0;
        if (mwb_rollout_index_ok(idx, r.cursor, r.N)) {
            const int t = small ? (int)((uint32_t)idx / (uint32_t)r.N) : (int)(idx / r.N);
            e = (size_t)(idx - (int64_t)t * r.N);
            slot = mwb_rollout_source(r.base, t, (int)k, r.nstack, r.R, r.age[(size_t)idx]);
        } else if (blockIdx.x == 0 && threadIdx.x == 0) {
            atomicAdd(r.rejected, 1ull);   // once per rejected row; its groups are written as zeros
        }
        char *dst = out + ((size_t)row * r.nstack + k) * ((size_t)quads * OUT_BYTES);
        if (slot < 0) {   // a zero group under either border: no load
            const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
            if (q0 < quads) window_store_quad<OUT_FLOAT, GREY>(dst, q0, zero, 0u);
            if (q1 < quads) window_store_quad<OUT_FLOAT, GREY>(dst, q1, zero, 0u);
            if (q2 < quads) window_store_quad<OUT_FLOAT, GREY>(dst, q2, zero, 0u);
            if (q3 < quads) window_store_quad<OUT_FLOAT, GREY>(dst, q3, zero, 0u);
            continue;
        }
        const int2 o = offsets[row];   // clamped before anything is computed from it
        wr.dx = mwb_window_clamp(o.x, w.dx_lo, w.dx_hi);
        wr.dy = mwb_window_clamp(o.y, w.dy_lo, w.dy_hi);
        wr.src = (const uint8_t *)(r.ring + ((size_t)slot * r.N + e) * r.frame_bytes);
        // all loads of the item in flight before the first store; named registers (an array here is promoted to LDS).  The loads
        // stand in one block without a branch - a quad past the end reads the last quad again and is not stored: under
        // `if (q < quads)` the compiler pulls each quad's conversions up behind its loads and waits for them there
        static_assert(WINDOW_UNROLL == 4, "four named registers below");
        uint4 v0, v1, v2, v3;
        uint32_t z0 = 0u, z1 = 0u, z2 = 0u, z3 = 0u;
        window_load_quad<GREY, ZERO, COLUMN>(wr, min(q0, quads - 1), v0, z0);
        window_load_quad<GREY, ZERO, COLUMN>(wr, min(q1, quads - 1), v1, z1);
        window_load_quad<GREY, ZERO, COLUMN>(wr, min(q2, quads - 1), v2, z2);
        window_load_quad<GREY, ZERO, COLUMN>(wr, min(q3, quads - 1), v3, z3);
        if (q0 < quads) window_store_quad<OUT_FLOAT, GREY>(dst, q0, v0, ZERO ? z0 : 0u);
        if (q1 < quads) window_store_quad<OUT_FLOAT, GREY>(dst, q1, v1, ZERO ? z1 : 0u);
        if (q2 < quads) window_store_quad<OUT_FLOAT, GREY>(dst, q2, v2, ZERO ? z2 : 0u);
        if (q3 < quads) window_store_quad<OUT_FLOAT, GREY>(dst, q3, v3, ZERO ? z3 : 0u);
    }
}

// quads: quads of one frame group of the output (C * out_w * out_h / 4); chunks = ceil(quads / WINDOW_CHUNK).  Grid: x = (frame
// group, chunk) of a row, nstack * chunks of them; y strides over the rows (x * y capped at about WINDOW_MAX_BLOCKS workgroups).
// ZERO: the window's border is zeros (edge replication needs nothing beyond the clamp)
template <bool OUT_FLOAT, bool GREY, bool ZERO>
__global__ void __launch_bounds__(WINDOW_THREADS) rollout_window_kernel(MwbRollout r, MwbWindow w, uint64_t magic, const int64_t *__restrict__ index,
                                                                       const int2 *__restrict__ offsets, char *__restrict__ out, uint32_t quads,
                                                                       uint32_t chunks, uint32_t count) {
    if ((w.out_h & 3) == 0) window_rows<OUT_FLOAT, GREY, ZERO, true>(r, w, magic, index, offsets, out, quads, chunks, count);
    else window_rows<OUT_FLOAT, GREY, ZERO, false>(r, w, magic, index, offsets, out, quads, chunks, count);
}

// ====================================================================================== launch
void mwb_launch_rollout_window_offsets(const MwbWindow &w, uint64_t key, const int64_t *index, int count, int32_t *offsets, hipStream_t s) {
    const unsigned blocks = (unsigned)(((int64_t)count + WINDOW_THREADS - 1) / WINDOW_THREADS);
    hipLaunchKernelGGL(rollout_window_offsets_kernel, dim3(blocks), dim3(WINDOW_THREADS), 0, s, w, key, index, (int2 *)offsets, (uint32_t)count);
}

template <bool OUT_FLOAT, bool GREY, bool ZERO>
static void launch_window(const MwbRollout &r, const MwbWindow &w, const int64_t *index, int count, const int32_t *offsets, char *out, hipStream_t s) {
    const uint32_t quads = (uint32_t)((GREY ? 1 : 3) * w.out_w * w.out_h / 4), chunks = (quads + WINDOW_CHUNK - 1) / WINDOW_CHUNK;
    const unsigned per_row = (unsigned)r.nstack * chunks;   // at most 16 x 768 (a 1024 x 1024 RGB output)
    unsigned rows = WINDOW_MAX_BLOCKS / per_row;
    rows = rows < 1 ? 1 : (rows > (unsigned)count ? (unsigned)count : rows);
    hipLaunchKernelGGL((rollout_window_kernel<OUT_FLOAT, GREY, ZERO>), dim3(per_row, rows), dim3(WINDOW_THREADS), 0, s, r, w,
                       mwb_window_div_magic((uint32_t)w.out_h), index, (const int2 *)offsets, out, quads, chunks, (uint32_t)count);
}

template <bool OUT_FLOAT, bool GREY>
static void launch_window_border(const MwbRollout &r, const MwbWindow &w, const int64_t *index, int count, const int32_t *offsets, char *out, hipStream_t s) {
    if (w.border == MWB_WINDOW_BORDER_ZERO) launch_window<OUT_FLOAT, GREY, true>(r, w, index, count, offsets, out, s);
    else launch_window<OUT_FLOAT, GREY, false>(r, w, index, count, offsets, out, s);
}

// count > 0; out is 16-byte, offsets 8-byte aligned; the window has passed mwb_window_check; a grey ring is gathered as float32 only
void mwb_launch_rollout_window(const MwbRollout &r, const MwbWindow &w, const int64_t *index, int count, const int32_t *offsets, void *out,
                               int out_float, hipStream_t s) {
    char *o = (char *)out;
    if (r.grey) launch_window_border<true, true>(r, w, index, count, offsets, o, s);
    else if (out_float) launch_window_border<true, false>(r, w, index, count, offsets, o, s);
    else launch_window_border<false, false>(r, w, index, count, offsets, o, s);
}
