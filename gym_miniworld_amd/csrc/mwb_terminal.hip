// mwb_terminal.hip - the kernels of the terminal pass (mwb_terminal_enable): what the reference's VecEnv worker throws away when it
// resets a finished env inside step (vec_env/subproc_vec_env.py:10-13: the frame step() rendered at `done`, miniworld.py:708-711 and
// the task rules, is overwritten by the reset frame).  The terminal frames themselves come from the existing prep and render
// kernels (mode 1, through a redirected copy of MwbDev: mwb_api.hip); here is what surrounds them.  Which row an ended env gets
// and where its history lies in the fused stack: mwb_terminal_map.h.  Terminal depth maps are not produced.
//
//   terminal_rank_kernel     one workgroup: an exclusive scan over reset_set in tiles of MWB_TERMINAL_TILE envs (ballots inside a
//                            wave, the 16 wave counts of a tile through LDS) -> row_of, row_env, count, dropped.  Ascending env
//                            index: the rows do not depend on the order the step kernels' atomicAdd gave reset_list.
//   terminal_stack_kernel    the hot path, a pure stream: for every row r < min(count, capacity) the nstack - 1 history groups of
//                            env row_env[r] out of its fused-stack window (one contiguous run of planes, copied bitwise) and
//                            behind them the terminal frame (uint8 -> float32 for a float RGB stack, bitwise otherwise).  count is
//                            device memory: the grid is fixed, rows are strided over gridDim.y, and everything a workgroup decides
//                            - its segment, its row's env - is workgroup-uniform.  UNIT = bytes a lane moves per access: 16 where
//                            W*H % 16 == 0 (a float conversion then loads 16 pixels and trades dwords inside the wave so that every
//                            float4 store instruction writes one contiguous KB, as rollout_gather_kernel does), 4 otherwise, 1 for
//                            a stack-less handle whose frame is no multiple of 4 bytes.  No LDS, no scratch, 64-bit offsets.
//   terminal_clear_kernel    count = 0, row_of = row_env = -1, cause = 0: after a pass that is not a step.
//   terminal_bootstrap_kernel  reward[t][e] += G[k] * V(row) for the rows that ended by the clock alone.
#include "mwb_internal.h"
#include "mwb_returns_scan.h"
#include "mwb_terminal_map.h"

#define TERM_THREADS 256
#define TERM_UNROLL 4
#define TERM_CHUNK (TERM_THREADS * TERM_UNROLL)   // units of one work item
#define TERM_MAX_BLOCKS 2048                      // 8 workgroups per CU; more rows are grid-strided
static_assert(MWB_TERMINAL_TILE == 1024 && MWB_TERMINAL_TILE % 64 == 0, "terminal_rank_kernel: one lane per env of a tile, 16 waves");

__global__ void __launch_bounds__(MWB_TERMINAL_TILE) terminal_rank_kernel(MwbTerminal t, const uint8_t *__restrict__ reset_set) {
    constexpr int NW = MWB_TERMINAL_TILE / 64;
    __shared__ int wave_count[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    int count = 0;   // ended envs in the tiles before this one: every thread keeps the same sum
    for (int t0 = 0; t0 < t.N; t0 += MWB_TERMINAL_TILE) {   // block-uniform trip count: barriers inside
        const int e = t0 + tid;
        const bool ended = e < t.N && reset_set[e] != 0;
        const unsigned long long m = __ballot(ended);
        if (lane == 0) wave_count[wave] = __popcll(m);
        __syncthreads();
        int waves_before = 0, in_tile = 0;
#pragma unroll
        for (int w = 0; w < NW; w++) { const int c = wave_count[w]; waves_before += w < wave ? c : 0; in_tile += c; }
        if (e < t.N) {
            const int row = ended ? mwb_terminal_row(mwb_terminal_rank(count, waves_before, __popcll(m & below)), t.capacity) : -1;
            t.row_of[e] = row;
            if (row >= 0) t.row_env[row] = e;
        }
        count += in_tile;
        __syncthreads();   // wave_count is rewritten by the next tile
    }
    for (int r = mwb_terminal_rows(count, t.capacity) + tid; r < t.capacity; r += MWB_TERMINAL_TILE) t.row_env[r] = -1;
    if (tid == 0) {
        t.count[0] = count;
        const int dropped = mwb_terminal_dropped_of(count, t.capacity);
        if (dropped) atomicAdd(t.dropped, (unsigned long long)dropped);
    }
}

__global__ void __launch_bounds__(TERM_THREADS) terminal_clear_kernel(MwbTerminal t) {
    const int i = blockIdx.x * TERM_THREADS + threadIdx.x;
    if (i == 0) t.count[0] = 0;
    if (i < t.N) { t.row_of[i] = -1; t.cause[i] = 0; }
    if (i < t.capacity) t.row_env[i] = -1;
}

__global__ void __launch_bounds__(TERM_THREADS) terminal_bootstrap_kernel(MwbTerminal t, MwbReturnsTables tab, float *__restrict__ reward_t,
                                                                         const int32_t *__restrict__ taken_t, const float *__restrict__ value_rows) {
    const int r = blockIdx.x * TERM_THREADS + threadIdx.x;
    if (r >= mwb_terminal_rows(t.count[0], t.capacity)) return;
    const int e = t.row_env[r];
    if (t.cause[e] != MWB_END_CLOCK) return;   // ended by a task rule (alone or together with the clock): a true terminal state
    const float Gk = tab.G[taken_t ? mwb_returns_k(taken_t[e]) : 1];
    const float b = Gk * value_rows[r];   // one float32 multiply, then one float32 add (-ffp-contract=off)
    reward_t[e] = reward_t[e] + b;
}

__device__ __forceinline__ float4 term_bytes_to_float4(uint32_t x) {   // exact: every value 0 .. 255 is a float32
    return make_float4((float)(x & 255u), (float)((x >> 8) & 255u), (float)((x >> 16) & 255u), (float)(x >> 24));
}

template <int UNIT> struct TermIn;
template <> struct TermIn<16> { typedef uint4 type; };
template <> struct TermIn<4> { typedef uint32_t type; };
template <> struct TermIn<1> { typedef uint8_t type; };

// hist_units / new_units: UNIT-byte units of the history run (as stored: the row's element type) and of the newest group's SOURCE;
// hist_chunks = ceil(hist_units / TERM_CHUNK).  Grid: x = the chunks of the history run, then those of the newest group; y strides
// over the rows.  stk_env_bytes / stk_off_bytes: bytes between consecutive envs of the stack and of the window's first plane.
template <bool OUT_FLOAT, bool GREY, int UNIT>
__global__ void __launch_bounds__(TERM_THREADS) terminal_stack_kernel(MwbTerminal t, const char *__restrict__ stk, size_t stk_env_bytes, size_t stk_off_bytes,
                                                                     uint32_t hist_units, uint32_t hist_chunks, uint32_t new_units) {
    typedef typename TermIn<UNIT>::type in_t;
    constexpr bool CONVERT = OUT_FLOAT && !GREY;   // the newest group is uint8 RGB and the row float32
    const bool newest = blockIdx.x >= hist_chunks;   // workgroup-uniform
    const uint32_t chunk = newest ? blockIdx.x - hist_chunks : blockIdx.x;
    const uint32_t units = newest ? new_units : hist_units;
    const uint32_t u0 = chunk * TERM_CHUNK + threadIdx.x, u1 = u0 + TERM_THREADS, u2 = u0 + 2 * TERM_THREADS, u3 = u0 + 3 * TERM_THREADS;
    static_assert(TERM_UNROLL == 4, "four named registers below");
    const size_t hist_bytes = (size_t)hist_units * UNIT;
    const size_t row_bytes = (size_t)t.nstack * t.cpf * t.plane * (OUT_FLOAT ? 4 : 1);
    const uint32_t rows = (uint32_t)mwb_terminal_rows(t.count[0], t.capacity);
    for (uint32_t row = blockIdx.y; row < rows; row += gridDim.y) {   // the row's env is workgroup-uniform
        const size_t e = (size_t)t.row_env[row];
        char *dst = t.rows + (size_t)row * row_bytes + (newest ? hist_bytes : 0);
        const char *srcb;
        if (!newest) srcb = stk + e * stk_env_bytes + stk_off_bytes;
        else if (GREY) srcb = (const char *)(t.grey_frames + e * t.plane);
        else srcb = (const char *)(t.frames + e * t.plane * 3);
        const in_t *src = (const in_t *)srcb;
        // all loads of the item in flight before the first store; named registers (an array here is promoted to LDS)
        in_t v0 = {}, v1 = {}, v2 = {}, v3 = {};
        if (u0 < units) v0 = src[u0];
        if (u1 < units) v1 = src[u1];
        if (u2 < units) v2 = src[u2];
        if (u3 < units) v3 = src[u3];
        if (!CONVERT || !newest) {   // bitwise: the history (stored in the row's type), a uint8 or a grey frame
            in_t *o = (in_t *)dst;
            if (u0 < units) o[u0] = v0;
            if (u1 < units) o[u1] = v1;
            if (u2 < units) o[u2] = v2;
            if (u3 < units) o[u3] = v3;
        } else if constexpr (CONVERT && UNIT == 16) {
            // uint8 -> float32, 16 pixels a lane.  Stored as they lie, each of a lane's four float4 stores would put 16 bytes every
            // 64; the wave trades dwords instead: store s of lane L takes dword L & 3 of lane 16 s + (L >> 2), so that every store
            // instruction writes 1 KB in one piece (rollout_gather_kernel).  Cross-lane reads only; the control flow
            // up to here is wave-uniform, so every lane takes part.
            const uint32_t lane = threadIdx.x & 63u, sel = lane & 3u;
            auto put = [&](const uint4 &v, uint32_t unit) {
                const uint32_t wave_unit0 = unit - lane;
#pragma unroll
                for (uint32_t s = 0; s < 4; s++) {
                    const uint32_t from = 16u * s + (lane >> 2);
                    const uint32_t a = __shfl(v.x, from), b = __shfl(v.y, from), c = __shfl(v.z, from), d = __shfl(v.w, from);
                    const uint32_t w = sel == 0 ? a : sel == 1 ? b : sel == 2 ? c : d;
                    if (wave_unit0 + from < units) *(float4 *)(dst + (size_t)wave_unit0 * 64 + 1024u * s + 16u * lane) = term_bytes_to_float4(w);
                }
            };
            put(v0, u0); put(v1, u1); put(v2, u2); put(v3, u3);
        } else if constexpr (CONVERT && UNIT == 4) {
            float4 *o = (float4 *)dst;
            if (u0 < units) o[u0] = term_bytes_to_float4(v0);
            if (u1 < units) o[u1] = term_bytes_to_float4(v1);
            if (u2 < units) o[u2] = term_bytes_to_float4(v2);
            if (u3 < units) o[u3] = term_bytes_to_float4(v3);
        } else if constexpr (CONVERT) {
            float *o = (float *)dst;
            if (u0 < units) o[u0] = (float)v0;
            if (u1 < units) o[u1] = (float)v1;
            if (u2 < units) o[u2] = (float)v2;
            if (u3 < units) o[u3] = (float)v3;
        }
    }
}

// ====================================================================================== launch
void mwb_launch_terminal_rank(const MwbTerminal &t, const uint8_t *reset_set, hipStream_t s) {
    hipLaunchKernelGGL(terminal_rank_kernel, dim3(1), dim3(MWB_TERMINAL_TILE), 0, s, t, reset_set);
}

void mwb_launch_terminal_clear(const MwbTerminal &t, hipStream_t s) {
    const int n = t.N > t.capacity ? t.N : t.capacity;
    hipLaunchKernelGGL(terminal_clear_kernel, dim3((n + TERM_THREADS - 1) / TERM_THREADS), dim3(TERM_THREADS), 0, s, t);
}

void mwb_launch_terminal_bootstrap(const MwbTerminal &t, const MwbReturnsTables &tab, float *reward_t, const int32_t *taken_t, const float *value_rows,
                                   hipStream_t s) {
    hipLaunchKernelGGL(terminal_bootstrap_kernel, dim3((t.capacity + TERM_THREADS - 1) / TERM_THREADS), dim3(TERM_THREADS), 0, s, t, tab, reward_t, taken_t,
                       value_rows);
}

template <bool OUT_FLOAT, bool GREY, int UNIT>
static void launch_stack(const MwbTerminal &t, const char *stk, size_t stk_env_bytes, size_t stk_off_bytes, hipStream_t s) {
    const size_t elem = OUT_FLOAT ? 4 : 1;
    const size_t hist_bytes = (size_t)mwb_terminal_history_planes(t.nstack, t.cpf) * t.plane * elem;
    const size_t new_bytes = GREY ? t.plane * 4 : t.plane * 3;   // of the source frame
    const uint32_t hist_units = (uint32_t)(hist_bytes / UNIT), new_units = (uint32_t)(new_bytes / UNIT);
    const uint32_t hist_chunks = (hist_units + TERM_CHUNK - 1) / TERM_CHUNK, new_chunks = (new_units + TERM_CHUNK - 1) / TERM_CHUNK;
    const unsigned per_row = hist_chunks + new_chunks;
    unsigned rows = TERM_MAX_BLOCKS / per_row;
    rows = rows < 1 ? 1 : (rows > (unsigned)t.capacity ? (unsigned)t.capacity : rows);
    hipLaunchKernelGGL((terminal_stack_kernel<OUT_FLOAT, GREY, UNIT>), dim3(per_row, rows), dim3(TERM_THREADS), 0, s, t, stk, stk_env_bytes, stk_off_bytes,
                       hist_units, hist_chunks, new_units);
}

// The API has checked: a stack is fused (W*H % 4 == 0, a uint8 one W*H % 16 == 0), a grey one float32; without a stack nstack = 1
void mwb_launch_terminal_stack(const MwbTerminal &t, const void *stk, int stk_K, int stk_pos, hipStream_t s) {
    const size_t elem = t.rows_float ? 4 : 1;
    const size_t env_bytes = (size_t)stk_K * t.plane * elem, off_bytes = (size_t)mwb_terminal_history_plane(stk_pos, 0, t.cpf) * t.plane * elem;
    const char *k = (const char *)stk;
    const bool wide = t.plane % 16 == 0, quad = (t.plane * 3) % 4 == 0 && (t.nstack == 1 || t.plane % 4 == 0);
    if (t.grey) {   // float32 throughout: 16-byte units where the plane allows, else 4
        if (wide) launch_stack<true, true, 16>(t, k, env_bytes, off_bytes, s); else launch_stack<true, true, 4>(t, k, env_bytes, off_bytes, s);
    } else if (t.rows_float) {
        if (wide) launch_stack<true, false, 16>(t, k, env_bytes, off_bytes, s);
        else if (quad) launch_stack<true, false, 4>(t, k, env_bytes, off_bytes, s);
        else launch_stack<true, false, 1>(t, k, env_bytes, off_bytes, s);
    } else {
        if (wide) launch_stack<false, false, 16>(t, k, env_bytes, off_bytes, s);
        else if (quad) launch_stack<false, false, 4>(t, k, env_bytes, off_bytes, s);
        else launch_stack<false, false, 1>(t, k, env_bytes, off_bytes, s);
    }
}
