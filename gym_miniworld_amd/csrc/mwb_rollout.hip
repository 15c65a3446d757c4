// mwb_rollout.hip - the kernels of the rollout storage (mwb_rollout_push / mwb_rollout_gather / mwb_rollout_after_update): the
// observation half of RolloutStorage (pytorch-a2c-ppo-acktr/storage.py) with every frame stored once.  Where a frame lives and
// which frames of a stacked observation are zeros: mwb_rollout_map.h.
//
//   rollout_push_kernel          one thread per env, every access a coalesced row: age, mask, feature of the new time step and
//                                the reward of the transition into it.  The frames themselves are one contiguous slab per slot
//                                (N x frame bytes): the host enqueues a device-to-device copy for them, no kernel.
//   rollout_gather_kernel        the hot path: (step, env) indices -> stacked observations.  A work item is (row of the output,
//                                frame group, chunk of GATHER_CHUNK units); its index, age and slot are workgroup-uniform, the
//                                body is a plain stream - every lane issues GATHER_UNROLL loads before its first store.
//                                WIDE: units of 16 bytes of the stored frame (uint8 -> float32: one 16-byte load of 16 pixels,
//                                four float4 stores, the dwords traded inside the wave first so that every store instruction
//                                writes one contiguous KB); otherwise units of 4 bytes, for frames whose W*H is no multiple of
//                                16.  Grey frames are float32 already and are copied bitwise (W*H % 4 == 0: always WIDE).
//   rollout_after_update_kernel  row T of age, mask and feature becomes row 0.
// No LDS is allocated, no scratch; the only atomic is one add per rejected row of a gather.  Every offset into the ring and the output is
// 64-bit: the ring passes 4 GiB at ordinary sizes.
#include "mwb_internal.h"
#include "mwb_rollout_map.h"

#define ROLLOUT_THREADS 256
#define GATHER_UNROLL 4
#define GATHER_CHUNK (ROLLOUT_THREADS * GATHER_UNROLL)   // units of one work item
#define GATHER_MAX_BLOCKS 2048                           // 8 workgroups per CU; longer lists are grid-strided

__global__ void __launch_bounds__(ROLLOUT_THREADS) rollout_push_kernel(MwbRollout r, int t, int after_reset, const uint8_t *__restrict__ fresh_dev,
                                                                      const uint8_t *__restrict__ done, const float *__restrict__ reward,
                                                                      const float *__restrict__ feature) {
    const int e = blockIdx.x * ROLLOUT_THREADS + threadIdx.x;
    if (e >= r.N) return;
    const size_t N = (size_t)r.N, at = (size_t)t * N + e;
    if (after_reset) {   // VecPyTorchFrameStack.reset; RolloutStorage's initial masks / features
        r.age[e] = 0; r.mask[e] = 1.0f;
        ((float2 *)r.feature)[e] = make_float2(0.0f, 0.0f);
        return;
    }
    const int fresh = fresh_dev ? fresh_dev[e] != 0 : done[e] != 0;
    r.age[at] = mwb_rollout_age(fresh, r.age[at - N], r.nstack);
    r.mask[at] = fresh ? 0.0f : 1.0f;
    ((float2 *)r.feature)[at] = ((const float2 *)feature)[e];
    r.reward[at - N] = fresh_dev ? 0.0f : reward[e];   // a pass that is not a step has no reward
}

__global__ void __launch_bounds__(ROLLOUT_THREADS) rollout_after_update_kernel(MwbRollout r) {
    const int e = blockIdx.x * ROLLOUT_THREADS + threadIdx.x;
    if (e >= r.N) return;
    const size_t last = (size_t)r.T * r.N + e;
    r.age[e] = r.age[last]; r.mask[e] = r.mask[last];
    ((float2 *)r.feature)[e] = ((const float2 *)r.feature)[last];
}

__device__ __forceinline__ float4 bytes_to_float4(uint32_t x) {   // exact: every value 0 .. 255 is a float32
    return make_float4((float)(x & 255u), (float)((x >> 8) & 255u), (float)((x >> 16) & 255u), (float)(x >> 24));
}

// one unit of the stored frame -> its place in the output row
template <bool OUT_FLOAT, bool GREY, bool WIDE>
struct GatherUnit;
template <bool OUT_FLOAT, bool GREY>
struct GatherUnit<OUT_FLOAT, GREY, true> {
    typedef uint4 in_t;
    static constexpr bool TRANSPOSED = OUT_FLOAT && !GREY;   // 16 pixels -> 64 bytes: stored by the wave as a whole (the kernel's body)
    static constexpr int OUT_BYTES = TRANSPOSED ? 64 : 16;
    static __device__ __forceinline__ void store(char *dst, const uint4 &v) { *(uint4 *)dst = v; }   // the copies: uint8 -> uint8, grey
    static __device__ __forceinline__ void zero(char *dst) {
        uint4 *d = (uint4 *)dst;
#pragma unroll
        for (int q = 0; q < OUT_BYTES / 16; q++) d[q] = make_uint4(0u, 0u, 0u, 0u);
    }
};
template <bool OUT_FLOAT>
struct GatherUnit<OUT_FLOAT, false, false> {
    typedef uint32_t in_t;
    static constexpr bool TRANSPOSED = false;
    static constexpr int OUT_BYTES = OUT_FLOAT ? 16 : 4;
    static __device__ __forceinline__ void store(char *dst, const uint32_t &v) {
        if (OUT_FLOAT) *(float4 *)dst = bytes_to_float4(v);
        else *(uint32_t *)dst = v;
    }
    static __device__ __forceinline__ void zero(char *dst) {
        if (OUT_FLOAT) *(uint4 *)dst = make_uint4(0u, 0u, 0u, 0u);
        else *(uint32_t *)dst = 0u;
    }
};

// units: units of one stored frame; chunks = ceil(units / GATHER_CHUNK).  Grid: x = (frame group, chunk) of a row, nstack * chunks
// of them; y strides over the rows (x * y capped at about GATHER_MAX_BLOCKS workgroups)
template <bool OUT_FLOAT, bool GREY, bool WIDE>
__global__ void __launch_bounds__(ROLLOUT_THREADS) rollout_gather_kernel(MwbRollout r, const int64_t *__restrict__ index, char *__restrict__ out,
                                                                        uint32_t units, uint32_t chunks, uint32_t count) {
    typedef GatherUnit<OUT_FLOAT, GREY, WIDE> U;
    typedef typename U::in_t in_t;
    const uint32_t k = blockIdx.x / chunks, chunk = blockIdx.x - k * chunks;
    const uint32_t u0 = chunk * GATHER_CHUNK + threadIdx.x;
    const bool small = ((int64_t)r.cursor + 1) * r.N <= 0x7fffffffLL;   // every valid index fits 32 bits: no 64-bit division
    for (uint32_t row = blockIdx.y; row < count; row += gridDim.y) {   // index, age and slot are workgroup-uniform
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
        char *dst = out + ((size_t)row * r.nstack + k) * ((size_t)units * U::OUT_BYTES);
        if (slot < 0) {
#pragma unroll
            for (int u = 0; u < GATHER_UNROLL; u++) {
                const uint32_t unit = u0 + u * ROLLOUT_THREADS;
                if (unit < units) U::zero(dst + (size_t)unit * U::OUT_BYTES);
            }
            continue;
        }
        const in_t *src = (const in_t *)(r.ring + ((size_t)slot * r.N + e) * r.frame_bytes);
        // all loads of the item in flight before the first store; named registers (an array here is promoted to LDS)
        static_assert(GATHER_UNROLL == 4, "four named registers below");
        const uint32_t u1 = u0 + ROLLOUT_THREADS, u2 = u0 + 2 * ROLLOUT_THREADS, u3 = u0 + 3 * ROLLOUT_THREADS;
        in_t v0 = {}, v1 = {}, v2 = {}, v3 = {};
        if (u0 < units) v0 = src[u0];
        if (u1 < units) v1 = src[u1];
        if (u2 < units) v2 = src[u2];
        if (u3 < units) v3 = src[u3];
        if constexpr (U::TRANSPOSED) {
            // uint8 -> float32.  A wave has loaded 1024 consecutive pixels, 16 per lane; stored as they lie, each of a lane's four
            // float4 stores would put 16 bytes every 64 (a quarter of every line per instruction: measured 3.4 TB/s).  The wave
            // trades dwords instead: store s of lane L takes pixels 256 s + 4 L .. + 3 = dword L & 3 of lane 16 s + (L >> 2), so
            // that every store instruction writes 1 KB in one piece (5.4 TB/s).  Cross-lane reads only, no LDS is allocated; the
            // control flow up to here is wave-uniform, so every lane takes part.
            const uint32_t lane = threadIdx.x & 63u, sel = lane & 3u;
            auto put = [&](const uint4 &v, uint32_t unit) {
                const uint32_t wave_unit0 = unit - lane;
#pragma unroll
                for (uint32_t s = 0; s < 4; s++) {
                    const uint32_t from = 16u * s + (lane >> 2);
                    const uint32_t a = __shfl(v.x, from), b = __shfl(v.y, from), c = __shfl(v.z, from), d = __shfl(v.w, from);
                    const uint32_t w = sel == 0 ? a : sel == 1 ? b : sel == 2 ? c : d;
                    if (wave_unit0 + from < units) *(float4 *)(dst + (size_t)wave_unit0 * 64 + 1024u * s + 16u * lane) = bytes_to_float4(w);
                }
            };
            put(v0, u0); put(v1, u1); put(v2, u2); put(v3, u3);
        } else {
            if (u0 < units) U::store(dst + (size_t)u0 * U::OUT_BYTES, v0);
            if (u1 < units) U::store(dst + (size_t)u1 * U::OUT_BYTES, v1);
            if (u2 < units) U::store(dst + (size_t)u2 * U::OUT_BYTES, v2);
            if (u3 < units) U::store(dst + (size_t)u3 * U::OUT_BYTES, v3);
        }
    }
}

// ====================================================================================== launch
static inline unsigned env_blocks(int N) { return (unsigned)((N + ROLLOUT_THREADS - 1) / ROLLOUT_THREADS); }

void mwb_launch_rollout_push(const MwbRollout &r, int t, int after_reset, const uint8_t *fresh_dev, const uint8_t *done, const float *reward,
                             const float *feature, hipStream_t s) {
    hipLaunchKernelGGL(rollout_push_kernel, dim3(env_blocks(r.N)), dim3(ROLLOUT_THREADS), 0, s, r, t, after_reset, fresh_dev, done, reward, feature);
}

void mwb_launch_rollout_after_update(const MwbRollout &r, hipStream_t s) {
    hipLaunchKernelGGL(rollout_after_update_kernel, dim3(env_blocks(r.N)), dim3(ROLLOUT_THREADS), 0, s, r);
}

template <bool OUT_FLOAT, bool GREY, bool WIDE>
static void launch_gather(const MwbRollout &r, const int64_t *index, int count, char *out, hipStream_t s) {
    const uint32_t units = (uint32_t)(r.frame_bytes / (WIDE ? 16 : 4)), chunks = (units + GATHER_CHUNK - 1) / GATHER_CHUNK;
    const unsigned per_row = (unsigned)r.nstack * chunks;   // at most 16 x 768 (a 1024 x 1024 frame in 4-byte units)
    unsigned rows = GATHER_MAX_BLOCKS / per_row;
    rows = rows < 1 ? 1 : (rows > (unsigned)count ? (unsigned)count : rows);
    hipLaunchKernelGGL((rollout_gather_kernel<OUT_FLOAT, GREY, WIDE>), dim3(per_row, rows), dim3(ROLLOUT_THREADS), 0, s, r, index, out, units, chunks,
                       (uint32_t)count);
}

// count > 0; out is 16-byte aligned; a grey ring is gathered as float32 only (the API has checked all three)
void mwb_launch_rollout_gather(const MwbRollout &r, const int64_t *index, int count, void *out, int out_float, hipStream_t s) {
    char *o = (char *)out;
    const bool wide = r.frame_bytes % 16 == 0;
    if (r.grey) launch_gather<true, true, true>(r, index, count, o, s);
    else if (out_float && wide) launch_gather<true, false, true>(r, index, count, o, s);
    else if (out_float) launch_gather<true, false, false>(r, index, count, o, s);
    else if (wide) launch_gather<false, false, true>(r, index, count, o, s);
    else launch_gather<false, false, false>(r, index, count, o, s);
}
