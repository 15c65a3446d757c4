// mwb_api.hip - host side of the C ABI declared in include/miniworld_batch.h.
//
// Owns the HBM-resident state of one shard of environments, hashes seeds to MT19937 states,
// builds the texture mip pyramids, and enqueues the step / reset / prep / render kernels on the
// caller's stream.  No torch types, no oracle code; fails loudly (negative status + message)
// rather than falling back to any CPU path.
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <type_traits>
#include <vector>

#include "mwb_internal.h"
#include "mwb_alloc_list.h"
#include "mwb_state_fields.h"
#include "mwb_lds_layout.h"
#include "mwb_rollout_map.h"
#include "mwb_rollout_window_map.h"
#include "mwb_monitor_map.h"
#include "mwb_levels_map.h"
#include "mwb_returns_scan.h"
#include "mwb_task_table.h"
#include "mwb_texture_host.h"

static_assert(mwb_task_frame_words(1) == MWB_FRAME_WORDS_FOR(1) && mwb_task_frame_words(MWB_MAX_ENTS) == MWB_FRAME_WORDS_FOR(MWB_MAX_ENTS),
              "mwb_task_table.h restates the frame constants' size");

static_assert(MWB_LEVELS_SEQUENTIAL == MWB_LEVELS_MODE_SEQUENTIAL && MWB_LEVELS_UNIFORM == MWB_LEVELS_MODE_UNIFORM && MWB_LEVELS_TABLE == MWB_LEVELS_MODE_TABLE,
              "mwb_levels_map.h restates the level modes");

static thread_local std::string g_err;
static int set_err(int code, const std::string &msg) { g_err = msg; return code; }
#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess)                                                               \
            return set_err(MWB_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e));    \
    } while (0)

// Every entry point runs on the handle's device and puts the caller's current device back on the way out
// (torch.cuda.current_device() reads the runtime's current device: a handle on cuda:1 must not move it).
struct DevGuard {
    int prev = -1;
    hipError_t err;
    explicit DevGuard(int dev) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) err = hipSetDevice(dev); else if (err == hipSuccess) prev = -1;
    }
    ~DevGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};
#define USE_DEVICE(dev)                                                                             \
    DevGuard _dev_guard(dev);                                                                        \
    if (_dev_guard.err != hipSuccess)                                                                \
        return set_err(MWB_EHIP, std::string("hipSetDevice: ") + hipGetErrorString(_dev_guard.err))

// The opening of an entry point that needs a feature: MWB_EINVAL unless `ok` (the handle and the pointers that must not be null;
// missing = "handle" or "argument"), MWB_ESTATE until the feature's enable function has run
#define NEED(ok, missing, on, enable)                                                                       \
    do {                                                                                                    \
        if (!(ok)) return set_err(MWB_EINVAL, std::string(__func__) + ": null " missing);                    \
        if (!(on)) return set_err(MWB_ESTATE, std::string(__func__) + ": call " #enable " first");           \
    } while (0)

struct mwb_handle {
    mwb_config cfg = {};
    MwbDev dev = {};
    MwbAllocList mem;   // every device allocation of the handle (dev_alloc); mwb_destroy frees from here and nowhere else
    std::vector<std::vector<uint32_t>> tex_levels[MWB_MAX_TEX];   // host mip chains (RGBA8 packed)
    int tex_w[MWB_MAX_TEX] = {}, tex_h[MWB_MAX_TEX] = {};
    uint32_t *texels_dev = nullptr;   // replaced by every upload_textures
    MwbTexDesc *tex_desc_dev = nullptr;
    bool seeded = false, textures_dirty = false, have_textures = false;
    bool have_obs = false;   // some pass has rendered an observation since creation
    int *scratch_int_dev = nullptr;
    // timing: five events per pipeline pass, drawn from a pool and only read back in
    // mwb_timing_read, so that enabling it adds no host synchronisation to the timed region
    bool timing = false, timing_now = false;   // enabled at all / recording the current pass
    int timing_period = 1, timing_tick = 0;   // record every timing_period-th pass (the events themselves cost ~20 us per pass)
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    hipEvent_t *ev = nullptr;   // the current pass' events: 0-4 on the caller's stream, 5-6 around reset_kernel
    // mwb_step overlaps world generation of the finished envs with the bulk render on a side stream
    bool overlap_reset = true;
    void *pack = nullptr;          // done | reward | feature | goal_pos | ep_steps | reward64 in one allocation
    size_t pack_bytes = 0;
    void *stack = nullptr;
    int stack_n = 0, stack_dtype = 0;
    int stack_fused = 0;               // the render kernels write the frames into the window themselves (MWB_STACK_FUSED)
    int stack_planes = 0, stack_pos = 0;   // sliding-window stack: planes per env (0 = the classic shifting stack), the window's first plane
    int stack_cpf = 3;                 // channel planes per frame: 3, or 1 (MWB_STACK_GREY: fed from the grey frame)
    size_t grey_bytes = 0;             // the grey buffer h->dev.grey (mwb_grey_enable), 0 while it is off
    size_t stack_bytes = 0;
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // entity tasks: mesh geometries (host copies until the first pass uploads them in one allocation)
    struct HostMesh { bool set = false; int n_tris = 0, n_nodes = 0, n_orders = 1, tex_id = -1; float min_c[3], max_c[3]; std::vector<float> nodes, tris, tris2, shade; };
    HostMesh meshes[MWB_NUM_MESHES];
    bool meshes_dirty = false;
    float4 *mesh_data_dev = nullptr;   // replaced by every upload_meshes
    MwbMeshDesc *mesh_desc_dev = nullptr;
    float *view_frame = nullptr;   // frame constants of mwb_render_view's size (lazily allocated)
    bool bulk_fixed = false;     // a step's bulk launch takes render_fixed_kernel (mwb_bulk_fixed_ok at creation and not MWB_NO_FIXED=1); grey output still overrides
    bool frame_reuse = false;    // the last-frame cache exists and step passes copy from it (off: MWB_NO_FRAME_REUSE=1, or frames rendered in tiles)
    // ---- mwb_copy_envs (all of its scratch lives here, none in MwbDev); allocated by the first copy that needs it
    unsigned long long serial = 0;      // unique per mwb_create: the key of another handle's cached descriptor table
    bool have_world = false;            // mwb_reset has generated worlds (or a copy has delivered some): the handle can be a source
    int32_t *copy_dst_pairs = nullptr;  // [N] pairs of the current call that name env e as their destination; zero between calls
    uint8_t *copy_src_mark = nullptr;   // [N] env e is the source of a pair of the current call (dst == src calls); zero between calls
    int2 *copy_pairs = nullptr;         // [copy_pairs_cap] {dst, src} per pair as validated, dst = -1: not carried out
    size_t copy_pairs_cap = 0;
    unsigned long long *copy_rejected = nullptr;  // [1] pairs rejected since mwb_copy_rejected last read it
    // descriptor tables for copies INTO this handle, one per source handle (by serial; 0 = free), MWB_COPY_TABLE_DESCS entries each
    MwbCopyDesc *copy_tables = nullptr;
    struct CopyTable { unsigned long long src = 0; int n_small = 0, small_chunks = 0, n_large = 0; } copy_table[4];
    int copy_table_next = 0;            // the slot the next new source takes (round robin)
    // ---- mwb_step_repeat: the per-env scratch of repeat_fold_kernel (mwb_repeat_fold.h); not part of an env's state, never copied
    double *rep_sum = nullptr;          // [N] float64 sum of the call's sub-step rewards
    int32_t *rep_taken = nullptr;       // [N] sub-steps taken in the last call (mwb_repeat_taken)
    uint8_t *rep_same = nullptr, *rep_frozen = nullptr;   // [N] each: every sub-step so far left the frame standing / the env takes no further sub-step
    // ---- the rollout storage (mwb_rollout_enable)
    bool rollout_on = false;
    MwbRollout rollout = {};
    size_t rollout_ring_bytes = 0;
    // ---- its learner half (mwb_rollout_learner_enable)
    bool learner_on = false;
    MwbLearner learner = {};
    bool last_pass_repeat = false;      // the last pass on the handle was an mwb_step_repeat: a push records its `taken` buffer
    // ---- the episode monitor (mwb_monitor_enable): one allocation, carved into the arrays of `monitor`
    bool monitor_on = false;
    MwbMonitor monitor = {};
    void *monitor_pack = nullptr;       // last_return | last_len | last_calls | counts | logged | retired, contiguous
    size_t monitor_pack_bytes = 0;
    // ---- terminal observations (mwb_terminal_enable); dev.end_cause is terminal.cause
    bool terminal_on = false;
    MwbTerminal terminal = {};
    size_t terminal_rows_bytes = 0;
    // ---- level sets (mwb_levels_enable); mode and sampler seed as the host set them last
    bool levels_on = false;
    MwbLevels levels = {};
    int levels_mode = 0;
    uint64_t levels_sampler_seed = 0;
    unsigned levels_flags = 0;
};
#define MWB_COPY_TABLE_DESCS 64
static unsigned long long g_next_serial = 1;

extern "C" const char *mwb_last_error(void) { return g_err.c_str(); }
extern "C" int mwb_abi_version(void) { return MWB_ABI_VERSION; }

// ------------------------------------------------------------------------------------ seeds
// The seed -> MT19937 state mapping of gym<=0.21 (gym/utils/seeding.py hash_seed, an un-vendored dependency of reference
// random.py:10): key = little-endian 32-bit limbs of the first 8 bytes of sha512(str(seed)), then numpy's RandomState.seed(list) ==
// init_by_array.  "Parity unpinned": gym is not available to check against.  The arithmetic is mwb_levels_map.h's - the functions
// levels_assign_kernel runs on the device; there is no second copy here.
extern "C" int mwb_seed_key(uint64_t seed, uint32_t key[2]) { return mwb_levels_seed_key(seed, key); }

// ------------------------------------------------------------------------------------ helpers
// n zeroed elements, owned by the handle's allocation list (mwb_alloc_list.h).  The caller holds the device guard.
template <typename T>
static int dev_alloc(mwb_handle *h, T **p, size_t n) {
    void *q = nullptr;
    size_t bytes = (n ? n : 1) * sizeof(T);
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) return set_err(MWB_ENOMEM, std::string("hipMalloc failed: ") + hipGetErrorString(e));
    e = hipMemset(q, 0, bytes);
    if (e != hipSuccess) { (void)hipFree(q); return set_err(MWB_EHIP, std::string("hipMemset failed: ") + hipGetErrorString(e)); }
    h->mem.add(q);
    *p = (T *)q;
    return MWB_OK;
}
static void dev_free(void *p) { (void)hipFree(p); }
// A buffer that is replaced during the handle's life: the old one goes (hipFree waits for the kernels still reading it)
template <typename T>
static int dev_realloc(mwb_handle *h, T **p, size_t n) {
    h->mem.release(*p, dev_free);
    *p = nullptr;
    return dev_alloc(h, p, n);
}
// What a feature allocates while it is being enabled: freed again unless the enable reaches keep().  Declared after the device
// guard, so that it frees on the handle's device.  A refused or failed enable leaves the handle as it was.
struct AllocScope {
    mwb_handle *h;
    size_t mark;
    explicit AllocScope(mwb_handle *handle) : h(handle), mark(handle->mem.mark()) {}
    ~AllocScope() { if (h) h->mem.release_to(mark, dev_free); }
    void keep() { h = nullptr; }
};

static void default_params(double p[MWB_NPARAM][9]) {   // params.py:110-123
    static const double T[MWB_NPARAM][9] = {
        {0.25, 0.82, 1, 0.1, 0.1, 0.1, 1.0, 1.0, 1.0},       {0, 2.5, 0, -40, 2.5, -40, 40, 5, 40},
        {0.7, 0.7, 0.7, 0.45, 0.45, 0.45, 0.8, 0.8, 0.8},    {0.45, 0.45, 0.45, 0.35, 0.35, 0.35, 0.55, 0.55, 0.55},
        {0, 0, 0, -0.2, -0.2, -0.2, 0.2, 0.2, 0.2},          {0.15, 0, 0, 0.12, 0, 0, 0.17, 0, 0},
        {0, 0, 0, -0.05, 0, 0, 0.05, 0, 0},                  {15, 0, 0, 10, 0, 0, 20, 0, 0},
        {0.4, 0, 0, 0.38, 0, 0, 0.42, 0, 0},                 {0, 0, 0, -5, 0, 0, 5, 0, 0},
        {60, 0, 0, 55, 0, 0, 65, 0, 0},                      {1.5, 0, 0, 1.45, 0, 0, 1.55, 0, 0},
        {0, 0, 0, -0.05, 0, 0, 0.10, 0, 0}};
    memcpy(p, T, sizeof(T));
}

extern "C" int mwb_create(const mwb_config *cfg, mwb_handle **out) {
    if (!cfg || !out) return set_err(MWB_EINVAL, "mwb_create: null argument");
    if (cfg->abi_version != MWB_ABI_VERSION) return set_err(MWB_EINVAL, "mwb_create: abi_version mismatch");
    if (cfg->num_envs <= 0) return set_err(MWB_EINVAL, "mwb_create: num_envs must be > 0");
    if (cfg->task < 0 || cfg->task >= MWB_NUM_TASKS) return set_err(MWB_EINVAL, "mwb_create: unknown task");
    if (cfg->obs_width <= 0 || cfg->obs_height <= 0 || cfg->obs_width > 1024 || cfg->obs_height > 1024)
        return set_err(MWB_EINVAL, "mwb_create: bad observation size");
    if (cfg->layout != MWB_LAYOUT_HWC && cfg->layout != MWB_LAYOUT_CWH) return set_err(MWB_EINVAL, "mwb_create: bad layout");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return set_err(MWB_EHIP, "mwb_create: no HIP device available (this library has no CPU path)");
    if (cfg->device < 0 || cfg->device >= ndev) return set_err(MWB_EINVAL, "mwb_create: bad device ordinal");
    USE_DEVICE(cfg->device);

    MwbTaskFacts t;
    {
        std::string why;
        if (int rc = mwb_resolve_task(*cfg, &t, &why)) return set_err(rc, why);
    }

    mwb_handle *h = new mwb_handle();
    h->cfg = *cfg;
    h->serial = g_next_serial++;
    MwbDev &d = h->dev;
    d.N = cfg->num_envs; d.task = cfg->task; d.W = cfg->obs_width; d.H = cfg->obs_height;
    d.want_depth = cfg->want_depth ? 1 : 0; d.layout = cfg->layout; d.domain_rand = cfg->domain_rand ? 1 : 0;
    d.auto_reset = cfg->no_auto_reset ? 0 : 1;
    // the task (mwb_task_table.h)
    d.ent_task = t.ent_task; d.n_boxes = t.n_boxes; d.R_max = t.R_max; d.S_max = t.S_max; d.max_episode_steps = t.max_episode_steps;
    d.n_tex = t.n_tex; d.no_ceiling = t.no_ceiling; d.poly = t.poly; d.room_words = t.room_words; d.frame_words = t.frame_words;
    d.agent_radius = t.agent_radius;
    memcpy(d.task_args, t.task_args, sizeof(d.task_args));
    double P[MWB_NPARAM][9];
    if (cfg->use_default_params) default_params(P); else memcpy(P, cfg->params, sizeof(P));
    for (int i = 0; i < MWB_NPARAM; i++)
        for (int k = 0; k < 3; k++) { d.params[i].def[k] = P[i][k]; d.params[i].lo[k] = P[i][3 + k]; d.params[i].hi[k] = P[i][6 + k]; }
    d.stk_cpf = 3;
    // the environment's knobs
    { const char *dbg = getenv("MWB_DEBUG"); d.debug_flags = dbg ? atoi(dbg) : 0; }
    { const char *ex = getenv("MWB_EXP"); d.exp_flags = ex ? atoi(ex) : 0; }
    { const char *no = getenv("MWB_NO_SEG_CULL"); d.no_seg_cull = no && atoi(no); }
    { const char *no = getenv("MWB_NO_OVERLAP"); h->overlap_reset = !(no && atoi(no)); }
    {   // the last ~0.6 round of resident workgroups (5 per CU x 256 CUs = 1280) of a bulk render launch drains in
        // half-frame units: measured best between 640 and 960 envs (+4 % at 8192 Maze envs); MWB_SPLIT overrides
        const char *sp = getenv("MWB_SPLIT");
        int split = sp ? atoi(sp) : 768;
        d.split_envs = split < 0 ? 0 : (split > cfg->num_envs ? cfg->num_envs : split);
    }
    if (d.ent_task) {   // MWB_TILE=WxH (0x0: whole frames): the tile a workgroup renders in the entity tasks
        int tw_ = 0, th_ = 0;   // default: whole frames (tiles cost 1.3 - 2.7x more in total: measured, scripts/ab_mesh_phases.py)
        const char *tl = getenv("MWB_TILE");
        if (tl && sscanf(tl, "%dx%d", &tw_, &th_) != 2) { tw_ = 0; th_ = 0; }
        if (tw_ > 0 && th_ > 0) { d.tile_w = tw_ < d.W ? tw_ : d.W; d.tile_h = th_ < d.H ? th_ : d.H; }
    }
    // an observation that does not fit one workgroup's LDS (or its 16-bit pixel queue) is rendered in tiles, like mwb_render_view's frames
    if (d.tile_w == 0 && (mwb_render_lds_bytes(d) > 160 * 1024 || !mwb_pixel_queue_fits(d.W, d.H))) {
        int tw = 0, th = 0;
        mwb_view_tile(&tw, &th);
        d.tile_w = tw < d.W ? tw : d.W; d.tile_h = th < d.H ? th : d.H;
    }
    // last-frame reuse: N x (W*H*3 [+ W*H*4 with depth]) bytes of cache and two flags per env; MWB_NO_FRAME_REUSE=1 turns it off
    { const char *no = getenv("MWB_NO_FRAME_REUSE"); h->frame_reuse = !(no && atoi(no)) && d.tile_w == 0; }
    // the step's bulk launch with the frame's shape compiled in (render_fixed_kernel); MWB_NO_FIXED=1 keeps the generic kernel
    { const char *no = getenv("MWB_NO_FIXED"); h->bulk_fixed = !(no && atoi(no)) && mwb_bulk_fixed_ok(d); }

    // device memory: the per-env arrays from their list (mwb_internal.h), then what is not per env
    const size_t N = (size_t)d.N;
    int rc = MWB_OK;
    mwb_for_each_env_array(d, d, h->frame_reuse, [&](auto *&, auto *&p, const MwbEnvArray &a) {
        if (rc == MWB_OK) rc = dev_alloc(h, &p, mwb_env_array_elems(a, N));
    });
#define A(ptr, n) if (rc == MWB_OK) rc = dev_alloc(h, &(ptr), (size_t)(n))
    A(d.seg_stage, (size_t)MWB_RESET_MAX_BLOCKS * d.S_max * 4);
    A(d.reset_count, 1); A(d.error_flag, 1); A(d.order_state, 2); A(d.list_counts, 2); A(d.reuse_stats, 2);
    if (d.debug_flags & 16) { A(d.wg_ts, 2 * (N + (size_t)d.split_envs)); }
    if (d.exp_flags & 4) { A(d.dbg_counters, 8); }
    {   // the small per-step outputs share one allocation (one D2H copy for a host-side consumer); 16-byte aligned parts
        auto up = [](size_t b) { return (b + 15) & ~(size_t)15; };
        // ordered by how often a host-side consumer needs them, so that it can copy a PREFIX: done | reward (what every step of a
        // VecEnv returns) | feature | goal_pos (the T-/Y-maze infos) | ep_steps | reward64
        const size_t o_done = 0, o_rew = o_done + up(N), o_feat = o_rew + up(N * 4), o_goal = o_feat + up(N * 8),
                     o_eps = o_goal + up(N * 24), o_r64 = o_eps + up(N * 4), total = o_r64 + up(N * 8);
        uint8_t *pack = nullptr;
        A(pack, total);
        if (rc == MWB_OK) {
            h->pack = pack; h->pack_bytes = total;
            d.reward64 = (double *)(pack + o_r64); d.goal_pos = (double *)(pack + o_goal); d.reward = (float *)(pack + o_rew);
            d.feature = (float *)(pack + o_feat); d.ep_steps = (int32_t *)(pack + o_eps); d.done = pack + o_done;
        }
    }
    A(h->tex_desc_dev, MWB_MAX_TEX);
    if (d.ent_task) { A(h->mesh_desc_dev, MWB_NUM_MESHES); }
    A(h->scratch_int_dev, 4);
    A(h->rep_sum, N); A(h->rep_taken, N); A(h->rep_same, N); A(h->rep_frozen, N);
#undef A
    d.tex_desc = h->tex_desc_dev; d.mesh_desc = h->mesh_desc_dev;
    if (rc == MWB_OK) {   // no cost known yet: identity order
        std::vector<int32_t> ident(N);
        for (size_t i = 0; i < N; i++) ident[i] = (int32_t)i;
        for (int k = 0; k < 2 && rc == MWB_OK; k++)
            if (hipMemcpy(d.order_bufs[k], ident.data(), N * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) rc = set_err(MWB_EHIP, "mwb_create: hipMemcpy failed");
    }
    // MiniWorldEnv.__init__ ends with self.reset() (miniworld.py:523): the episode counters of TMazeDynamic /
    // TMazeTwoBoxDynamic (tmaze.py:80,130) have seen one reset when the caller gets the env
    if (rc == MWB_OK && ((d.task == MWB_TASK_TMAZE && d.task_args[3] > 0) || (d.task == MWB_TASK_TMAZE_TWOBOX && d.task_args[0] == 0))) {
        std::vector<int64_t> ones(N, 1);
        if (hipMemcpy(d.episode_count, ones.data(), N * sizeof(int64_t), hipMemcpyHostToDevice) != hipSuccess) rc = set_err(MWB_EHIP, "mwb_create: hipMemcpy failed");
    }
    if (rc == MWB_OK && hipMemset(d.carrying, 0xFF, N * sizeof(int32_t)) != hipSuccess) rc = set_err(MWB_EHIP, "mwb_create: hipMemset failed");   // -1: nothing carried
    if (rc != MWB_OK) { mwb_destroy(h); return rc; }

    int prio_lo = 0, prio_hi = 0;
    hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);   // numerically lowest = highest priority
    if (hipStreamCreateWithPriority(&h->side, hipStreamNonBlocking, prio_hi) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) != hipSuccess) {
        mwb_destroy(h);
        return set_err(MWB_EHIP, "mwb_create: could not create the side stream / events");
    }
    if (int prc = mwb_prepare_kernels(d)) {
        mwb_destroy(h);
        return set_err(prc == -2 ? MWB_EHIP : MWB_EINVAL,
                       prc == -1 ? "mwb_create: world + observation too large for the 160 KB LDS staging buffers (room table + W*H*3 frame)"
                       : prc == -3 ? "mwb_create: observation too large for the 16-bit pixel queue (H << ceil(log2 W) must not exceed 65536)"
                                   : "mwb_create: hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
    }
    *out = h;
    return MWB_OK;
}

extern "C" int mwb_destroy(mwb_handle *h) {
    if (!h) return MWB_OK;
    DevGuard _dev_guard(h->cfg.device);
    hipDeviceSynchronize();
    h->mem.release_to(0, dev_free);
    for (hipEvent_t e : h->ev_pool) hipEventDestroy(e);
    if (h->ev_fork) hipEventDestroy(h->ev_fork);
    if (h->ev_join) hipEventDestroy(h->ev_join);
    if (h->side) hipStreamDestroy(h->side);
    delete h;
    return MWB_OK;
}

// ------------------------------------------------------------------------------------ textures
// build_mips and the footprint tables: mwb_texture_host.h

extern "C" int mwb_set_texture(mwb_handle *h, int tex_id, int width, int height, const uint8_t *rgb) {
    if (!h || !rgb) return set_err(MWB_EINVAL, "mwb_set_texture: null argument");
    if (tex_id < 0 || tex_id >= MWB_MAX_TEX || width <= 0 || height <= 0 || width > 4096 || height > 4096)
        return set_err(MWB_EINVAL, "mwb_set_texture: bad texture id or size");
    build_mips(rgb, width, height, h->tex_levels[tex_id]);
    if ((int)h->tex_levels[tex_id].size() > MWB_MAX_LEVELS) return set_err(MWB_EINVAL, "mwb_set_texture: too many mip levels");
    h->tex_w[tex_id] = width; h->tex_h[tex_id] = height;
    h->textures_dirty = true;
    return MWB_OK;
}

static int upload_textures(mwb_handle *h) {
    USE_DEVICE(h->cfg.device);
    const int n_tex = h->dev.n_tex;
    for (int i = 0; i < n_tex; i++)
        if (h->tex_w[i] == 0)
            return set_err(MWB_ESTATE, "render requested before the task's " + std::to_string(n_tex) + " textures were set (mwb_set_texture)");
    // one footprint table per mip level: (w+1) x (h+1) entries of the four wrapped texels of a bilinear tap (mwb_texture_host.h).
    // The kernels address entries with 32-bit byte offsets from the buffer's base.
    size_t total = 0;
    for (int i = 0; i < n_tex; i++) total += pyramid_footprint_entries(h->tex_w[i], h->tex_h[i]);
    if (total * 16 > 0xFFFFFFFFull)
        return set_err(MWB_EINVAL, "textures too large: the footprint tables take " + std::to_string(total * 16) +
                                       " bytes, byte offsets into them must fit 32 bits");
    std::vector<uint32_t> all;
    all.reserve(total * 4);
    MwbTexDesc desc[MWB_MAX_TEX];
    memset(desc, 0, sizeof(desc));
    for (int i = 0; i < n_tex; i++) {
        desc[i].w = h->tex_w[i]; desc[i].h = h->tex_h[i]; desc[i].n_levels = (int)h->tex_levels[i].size();
        desc[i].sc_s = (float)(512.0 / h->tex_w[i]); desc[i].sc_t = (float)(512.0 / h->tex_h[i]);
        append_pyramid_footprints(h->tex_levels[i], h->tex_w[i], h->tex_h[i], desc[i].level_off, all);
    }
    HIP_TRY(hipDeviceSynchronize());
    if (int rc = dev_realloc(h, &h->texels_dev, all.size())) return rc;
    HIP_TRY(hipMemcpy(h->texels_dev, all.data(), all.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->tex_desc_dev, desc, sizeof(desc), hipMemcpyHostToDevice));
    h->dev.texels = h->texels_dev;
    h->textures_dirty = false; h->have_textures = true;
    return MWB_OK;
}

// -------------------------------------------------------------------------------------- meshes
extern "C" int mwb_set_mesh(mwb_handle *h, int geom, int n_tris, const float *verts, const float *norms, const float *texcs, int tex_slot,
                            const float *min_coords, const float *max_coords, int n_nodes, int n_orders, const float *nodes, const int32_t *perm) {
    if (!h || !verts || !norms || !texcs || !min_coords || !max_coords || !nodes || !perm) return set_err(MWB_EINVAL, "mwb_set_mesh: null argument");
    if (geom < 0 || geom >= MWB_NUM_MESHES || n_tris <= 0 || n_tris >= (1 << 24) || n_nodes <= 0 || tex_slot >= MWB_MAX_TEX || (n_orders != 1 && n_orders != 8))
        return set_err(MWB_EINVAL, "mwb_set_mesh: bad geometry id / sizes");
    for (int ord = 0; ord < n_orders; ord++) {   // the hierarchy is walked by a kernel: every link must stay inside the arrays and move forward (the walk terminates)
        std::vector<char> seen((size_t)n_tris, 0);
        const float *on = nodes + (size_t)ord * n_nodes * 8;
        for (int i = 0; i < n_nodes; i++) {
            int32_t skip, fc;
            memcpy(&skip, on + (size_t)i * 8 + 3, 4); memcpy(&fc, on + (size_t)i * 8 + 7, 4);
            const int cnt = (int)((uint32_t)fc >> 24), first = (int)((uint32_t)fc & 0xFFFFFFu);
            if (skip <= i || skip > n_nodes || first + cnt > n_tris || (cnt == 0 && i + 1 >= n_nodes))
                return set_err(MWB_EINVAL, "mwb_set_mesh: malformed hierarchy");
            for (int k = 0; k < cnt; k++) seen[(size_t)first + k] = 1;
        }
        for (int i = 0; i < n_tris; i++)
            if (!seen[i] || perm[i] < 0 || perm[i] >= n_tris) return set_err(MWB_EINVAL, "mwb_set_mesh: the leaves must cover every triangle once");
    }
    mwb_handle::HostMesh &m = h->meshes[geom];
    m.set = true; m.n_tris = n_tris; m.n_nodes = n_nodes; m.n_orders = n_orders; m.tex_id = tex_slot;
    for (int k = 0; k < 3; k++) { m.min_c[k] = min_coords[k]; m.max_c[k] = max_coords[k]; }
    m.nodes.assign(nodes, nodes + (size_t)n_orders * n_nodes * 8);
    auto rec = [&](int tri, float *o) {   // v0.xyz e1.x | e1.yz e2.xy | e2.z idx 0 0 with e1 = v1 - v0, e2 = v2 - v0 in float32
        const float *v = verts + (size_t)tri * 9;
        const float e1[3] = {v[3] - v[0], v[4] - v[1], v[5] - v[2]}, e2[3] = {v[6] - v[0], v[7] - v[1], v[8] - v[2]};
        o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = e1[0]; o[4] = e1[1]; o[5] = e1[2]; o[6] = e2[0]; o[7] = e2[1]; o[8] = e2[2];
        int32_t idx = tri; memcpy(o + 9, &idx, 4); o[10] = 0; o[11] = 0;
    };
    m.tris.resize((size_t)n_tris * 12); m.tris2.resize((size_t)n_tris * 12); m.shade.assign((size_t)n_tris * 16, 0.0f);
    for (int i = 0; i < n_tris; i++) {
        rec(perm[i], &m.tris[(size_t)i * 12]);
        rec(i, &m.tris2[(size_t)i * 12]);
        float *o = &m.shade[(size_t)i * 16];
        memcpy(o, norms + (size_t)i * 9, 36);
        memcpy(o + 9, texcs + (size_t)i * 6, 24);
    }
    h->meshes_dirty = true;
    return MWB_OK;
}

extern "C" int mwb_set_mesh_dims(mwb_handle *h, int geom, double height, double scale, double radius, int is_f32) {
    if (!h) return set_err(MWB_EINVAL, "mwb_set_mesh_dims: null handle");
    if (geom < 0 || geom >= MWB_NUM_MESHES || !(height > 0) || !(scale > 0) || !(radius > 0) || !std::isfinite(scale) || !std::isfinite(radius))
        return set_err(MWB_EINVAL, "mwb_set_mesh_dims: bad argument");
    MwbDev &d = h->dev;
    int k = 0;
    while (k < d.n_mesh_dims && !(d.mesh_dims[k].geom == geom && d.mesh_dims[k].height == height)) k++;
    if (k == MWB_MAX_MESH_DIMS) return set_err(MWB_EINVAL, "mwb_set_mesh_dims: table full");
    d.mesh_dims[k].geom = geom; d.mesh_dims[k].height = height; d.mesh_dims[k].scale = scale; d.mesh_dims[k].radius = radius; d.mesh_dims[k].is_f32 = is_f32 ? 1 : 0;
    if (k == d.n_mesh_dims) d.n_mesh_dims++;
    return MWB_OK;
}

static int upload_meshes(mwb_handle *h) {   // the caller holds the device guard
    const MwbTaskRow &row = MWB_TASK_TABLE[h->dev.task];
    const int *need = row.meshes;
    for (int k = 0; k < row.n_meshes; k++) {
        if (!h->meshes[need[k]].set) return set_err(MWB_ESTATE, "reset / render requested before the task's meshes were set (mwb_set_mesh)");
        bool dims = false;
        for (int q = 0; q < h->dev.n_mesh_dims; q++) dims = dims || h->dev.mesh_dims[q].geom == need[k];
        if (!dims) return set_err(MWB_ESTATE, "reset requested before the task's mesh dimensions were set (mwb_set_mesh_dims)");
    }
    std::vector<float> all;
    MwbMeshDesc desc[MWB_NUM_MESHES];
    memset(desc, 0, sizeof(desc));
    for (int g = 0; g < MWB_NUM_MESHES; g++) {
        const mwb_handle::HostMesh &m = h->meshes[g];
        if (!m.set) continue;
        desc[g].n_tris = m.n_tris; desc[g].n_nodes = m.n_nodes; desc[g].tex_id = m.tex_id; desc[g].n_orders = m.n_orders;
        for (int k = 0; k < 3; k++) { desc[g].min_c[k] = m.min_c[k]; desc[g].max_c[k] = m.max_c[k]; }
        desc[g].node_off = (uint32_t)(all.size() / 4); all.insert(all.end(), m.nodes.begin(), m.nodes.end());
        desc[g].tri_off = (uint32_t)(all.size() / 4); all.insert(all.end(), m.tris.begin(), m.tris.end());
        desc[g].tri2_off = (uint32_t)(all.size() / 4); all.insert(all.end(), m.tris2.begin(), m.tris2.end());
        desc[g].shade_off = (uint32_t)(all.size() / 4); all.insert(all.end(), m.shade.begin(), m.shade.end());
    }
    HIP_TRY(hipDeviceSynchronize());
    if (int rc = dev_realloc(h, &h->mesh_data_dev, (all.size() + 3) / 4)) return rc;
    if (!all.empty()) HIP_TRY(hipMemcpy(h->mesh_data_dev, all.data(), all.size() * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(h->mesh_desc_dev, desc, sizeof(desc), hipMemcpyHostToDevice));
    h->dev.mesh_data = h->mesh_data_dev;
    h->meshes_dirty = false;
    return MWB_OK;
}

// ---------------------------------------------------------------------------------- simulation
// Something the frames of envs [first, first + count) depend on has been changed from outside without a render: their cached
// frames no longer show their state.  The callers have synchronised the device and hold the device guard.
static int invalidate_frames(mwb_handle *h, int first, int count) {
    if (!h->dev.frame_cached || count <= 0) return MWB_OK;
    HIP_TRY(hipMemset(h->dev.frame_cached + first, 0, (size_t)count));
    HIP_TRY(hipDeviceSynchronize());
    return MWB_OK;
}

// The counters kernels add to and the host reads: n of them to `out`, then (clear) zero again.  Synchronous.
static int read_counters(mwb_handle *h, unsigned long long *out, unsigned long long *counters_dev, size_t n, bool clear = true) {
    USE_DEVICE(h->cfg.device);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, counters_dev, n * sizeof(*out), hipMemcpyDeviceToHost));
    if (!clear) return MWB_OK;
    HIP_TRY(hipMemset(counters_dev, 0, n * sizeof(*out)));
    HIP_TRY(hipDeviceSynchronize());
    return MWB_OK;
}

extern "C" int mwb_seed(mwb_handle *h, const uint64_t *seeds) {
    if (!h || !seeds) return set_err(MWB_EINVAL, "mwb_seed: null argument");
    USE_DEVICE(h->cfg.device);
    std::vector<uint32_t> st((size_t)h->dev.N * MWB_MT_WORDS);
    uint32_t base[624];
    mwb_levels_mt_base(base);
    for (int e = 0; e < h->dev.N; e++) {
        uint32_t key[2];
        const int n = mwb_levels_seed_key(seeds[e], key);
        MwbLevelsPlainRow row = {&st[(size_t)e * MWB_MT_WORDS]};
        mwb_levels_init_by_array(row, base, key[0], key[1], n);
    }
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(h->dev.rng, st.data(), st.size() * 4, hipMemcpyHostToDevice));
    h->seeded = true;
    return invalidate_frames(h, 0, h->dev.N);
}

static int check_launch(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_err(MWB_EHIP, std::string(what) + " launch failed: " + hipGetErrorString(e));
    return MWB_OK;
}

#define EVN 7
static int timing_begin(mwb_handle *h, hipStream_t s) {
    h->timing_now = h->timing && (h->timing_tick++ % h->timing_period) == 0;
    if (!h->timing_now) return MWB_OK;
    if (h->ev_used + EVN > h->ev_pool.size() && h->ev_pool.size() >= (size_t)EVN * 65536)
        h->ev_used = 0;   // nobody read the samples for 65536 timed passes: start over instead of growing without bound
    if (h->ev_used + EVN > h->ev_pool.size()) {
        size_t old = h->ev_pool.size();
        h->ev_pool.resize(old + EVN * 256);
        for (size_t i = old; i < h->ev_pool.size(); i++) HIP_TRY(hipEventCreate(&h->ev_pool[i]));
    }
    h->ev = &h->ev_pool[h->ev_used];
    h->ev_used += EVN;
    HIP_TRY(hipEventRecord(h->ev[0], s));
    return MWB_OK;
}
#define TMARK(i) do { if (h->timing_now) HIP_TRY(hipEventRecord(h->ev[i], s)); } while (0)

static int render_tail(mwb_handle *h, int mode, hipStream_t s) {
    mwb_launch_prep(h->dev, mode, s);
    int rc = check_launch("prep_kernel"); if (rc) return rc;
    TMARK(3);
    mwb_launch_render(h->dev, mode, s, mode == 2 && h->bulk_fixed);   // mode 2: only a step's bulk launch
    rc = check_launch("render_kernel"); if (rc) return rc;
    TMARK(4);
    return MWB_OK;
}

// Fused frame stack: move the window on for the pass that is about to render (0 = a step, 2 = a reset of everything), copying
// the history back to the front first when the window has reached the end of its planes.
static int stack_advance(mwb_handle *h, int after_reset, hipStream_t s) {
    if (!h->stack_fused) return MWB_OK;
    const int cpf = h->stack_cpf, C = h->stack_n * cpf, from = h->stack_pos;
    int pos = after_reset ? 0 : from + cpf;
    if (!after_reset && pos + C > h->stack_planes) {
        mwb_launch_stack_slide(h->dev, h->stack, h->stack_n, h->stack_planes, h->stack_dtype, 0, from, 3, s, cpf);
        int rc = check_launch("stack_slide_kernel"); if (rc) return rc;
        pos = 0;
    }
    h->stack_pos = pos; h->dev.stk_pos = pos;
    return MWB_OK;
}

// Terminal observations (mwb_terminal_enable), immediately BEFORE the reset launch of a step: reset_list holds exactly the envs that
// ended and their state is still the terminal state - reset_kernel destroys it, and render_kernel mode 1 zeroes the regenerated
// envs' stack history.  Rank the ended envs, render their frames through the list path (prep mode 1 + render mode 1) with a copy of
// the MwbDev whose outputs point at the terminal buffers, then write the compact stacked rows.  The copy redirects everything
// mode 1 writes: obs, grey and the frame constants; depth, the fused stack, the workgroup time stamps and the last-frame cache are
// off (mode 1 writes no `cost` and, with reuse_pass 0, no reuse statistics).  step_pass = 1: the frame is the step's own, the render
// override (ovr_slot / ovr_pose) is honoured.  Tiled handles go through the same calls.
static int terminal_pass(mwb_handle *h, hipStream_t s) {
    if (!h->terminal_on) return MWB_OK;
    const MwbTerminal &t = h->terminal;
    mwb_launch_terminal_rank(t, h->dev.reset_set, s);
    int rc = check_launch("terminal_rank_kernel"); if (rc) return rc;
    MwbDev v = h->dev;
    v.obs = t.frames; v.grey = t.grey_frames; v.frame = t.frame_consts;
    v.depth = nullptr; v.want_depth = 0;
    v.stk = nullptr; v.wg_ts = nullptr;
    v.frame_cache = nullptr; v.depth_cache = nullptr; v.frame_cached = nullptr; v.frame_same = nullptr; v.reuse_pass = 0;
    v.step_pass = 1;
    mwb_launch_prep(v, 1, s);
    rc = check_launch("prep_kernel"); if (rc) return rc;
    mwb_launch_render(v, 1, s);
    rc = check_launch("render_kernel"); if (rc) return rc;
    mwb_launch_terminal_stack(t, h->stack, h->stack_planes, h->stack_pos, s);
    return check_launch("terminal_stack_kernel");
}
// a pass that is not a step has no terminal observations: count = 0, no rows, no causes
static int terminal_clear(mwb_handle *h, hipStream_t s) {
    if (!h->terminal_on) return MWB_OK;
    mwb_launch_terminal_clear(h->terminal, s);
    return check_launch("terminal_clear_kernel");
}

// Level sets (mwb_levels_enable), immediately before a reset launch: every env on reset_list gets its level and, in place of the
// stream its last episode left, the generator row of the level's seed.  tally: the pass is a step (the listed envs ended an episode)
static int levels_pass(mwb_handle *h, int tally, hipStream_t s) {
    if (!h->levels_on) return MWB_OK;
    const MwbDev &d = h->dev;
    mwb_launch_levels_assign(h->levels, d.reset_list, d.reset_count, d.rng, d.done, d.reward64, d.ep_steps, tally, s);
    return check_launch("levels_assign_kernel");
}

static int ensure_ready(mwb_handle *h, bool renders = true) {   // the caller holds the device guard
    if (!h->seeded) return set_err(MWB_ESTATE, "mwb_seed must be called before reset/step (the reference seeds from entropy; this library refuses to)");
    if (h->textures_dirty || !h->have_textures) { int rc = upload_textures(h); if (rc) return rc; rc = invalidate_frames(h, 0, h->dev.N); if (rc) return rc; }
    if (h->dev.ent_task && (h->meshes_dirty || !h->mesh_data_dev)) { int rc = upload_meshes(h); if (rc) return rc; rc = invalidate_frames(h, 0, h->dev.N); if (rc) return rc; }
    if (renders) h->have_obs = true;
    return MWB_OK;
}

extern "C" int mwb_reset(mwb_handle *h, const uint8_t *mask_dev, void *stream) {
    if (!h) return set_err(MWB_EINVAL, "null handle");
    USE_DEVICE(h->cfg.device);
    int rc = ensure_ready(h); if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    h->last_pass_repeat = false;
    h->dev.step_pass = 0; h->dev.reuse_pass = 0;   // every frame is rendered (and the last-frame cache refreshed)
    rc = timing_begin(h, s); if (rc) return rc;
    rc = stack_advance(h, mask_dev == nullptr, s); if (rc) return rc;   // a full reset restarts the window; a partial one is a step for the others
    rc = terminal_clear(h, s); if (rc) return rc;
    mwb_launch_mark_reset(h->dev, mask_dev, s);
    rc = check_launch("mark_reset_kernel"); if (rc) return rc;
    rc = levels_pass(h, 0, s); if (rc) return rc;   // a reset abandons episodes: nothing is tallied
    TMARK(1); TMARK(5);
    mwb_launch_reset(h->dev, MWB_RESET_MAX_BLOCKS, s);   // possibly every env: many blocks
    rc = check_launch("reset_kernel"); if (rc) return rc;
    h->have_world = true;
    TMARK(6); TMARK(2);
    rc = render_tail(h, 0, s); if (rc) return rc;
    mwb_launch_clear_list(h->dev, s);
    rc = check_launch("clear_list_kernel"); if (rc) return rc;
    // the first step's bulk render is dispatched by the frame costs this render just measured (not in env order)
    mwb_launch_order(h->dev, s);
    return check_launch("order_kernel");
}

// repeat == 0: one step (mwb_step); 1 .. MWB_MAX_REPEAT: the sub-steps of mwb_step_repeat
static int step_impl(mwb_handle *h, const int32_t *actions_dev, const uint8_t *skip_mask_dev, void *stream, int repeat = 0, const int32_t *counts_dev = nullptr);
extern "C" int mwb_step(mwb_handle *h, const int32_t *actions_dev, const uint8_t *skip_mask_dev, void *stream) {
    if (!h) return set_err(MWB_EINVAL, "null handle");
    h->dev.act_stride = 1;
    return step_impl(h, actions_dev, skip_mask_dev, stream);
}
extern "C" int mwb_step_i64(mwb_handle *h, const int64_t *actions_dev, const uint8_t *skip_mask_dev, void *stream) {
    if (!h) return set_err(MWB_EINVAL, "null handle");
    h->dev.act_stride = 2;   // little-endian: the low word of each int64 (actions are small non-negative integers)
    return step_impl(h, (const int32_t *)actions_dev, skip_mask_dev, stream);
}
extern "C" int mwb_step_repeat(mwb_handle *h, const int32_t *actions_dev, const int64_t *actions_i64_dev, const uint8_t *skip_mask_dev, int repeat,
                               const int32_t *counts_dev, void *stream) {
    if (!h) return set_err(MWB_EINVAL, "null handle");
    if (repeat < 1 || repeat > MWB_MAX_REPEAT) return set_err(MWB_EINVAL, "mwb_step_repeat: repeat must lie in 1 .. " + std::to_string(MWB_MAX_REPEAT));
    if ((actions_dev != nullptr) == (actions_i64_dev != nullptr)) return set_err(MWB_EINVAL, "mwb_step_repeat: exactly one of actions / actions_i64 must be given");
    h->dev.act_stride = actions_i64_dev ? 2 : 1;
    return step_impl(h, actions_i64_dev ? (const int32_t *)actions_i64_dev : actions_dev, skip_mask_dev, stream, repeat, counts_dev);
}
extern "C" int mwb_repeat_taken(mwb_handle *h, int32_t **dev) {
    if (!h || !dev) return set_err(MWB_EINVAL, "mwb_repeat_taken: null argument");
    *dev = h->rep_taken;
    return MWB_OK;
}
static int step_impl(mwb_handle *h, const int32_t *actions_dev, const uint8_t *skip_mask_dev, void *stream, int repeat, const int32_t *counts_dev) {
    USE_DEVICE(h->cfg.device);
    int rc = ensure_ready(h); if (rc) return rc;
    if (!actions_dev) return set_err(MWB_EINVAL, "mwb_step: null actions");
    hipStream_t s = (hipStream_t)stream;
    h->last_pass_repeat = repeat > 0;
    h->dev.reuse_pass = 1;   // an env the step kernel finds unchanged gets its last frame copied instead of rendered (d.frame_same)
    h->dev.step_pass = 1;   // the frames of this pass are the step's own (entity tasks: what a task rule removed is still drawn)
    rc = timing_begin(h, s); if (rc) return rc;
    rc = stack_advance(h, 0, s); if (rc) return rc;
    mwb_launch_step(h->dev, actions_dev, skip_mask_dev, s);
    rc = check_launch("step_kernel"); if (rc) return rc;
    // mwb_step_repeat: fold every sub-step's outputs (mwb_repeat_fold.h), then step the envs that are not frozen yet again.  A
    // masked env is frozen by the first fold, so the later launches need no skip mask; the order flip, the stack window and the
    // reset list move once (the flip is a no-op once order_state[1] is down, a finished env is frozen before it could be listed twice).
    for (int sub = 0; sub < repeat; sub++) {
        if (sub) {
            MwbDev dv = h->dev;
            dv.frozen = h->rep_frozen;
            mwb_launch_step(dv, actions_dev, nullptr, s);
            rc = check_launch("step_kernel"); if (rc) return rc;
        }
        mwb_launch_repeat_fold(h->dev, sub, sub == repeat - 1, repeat, skip_mask_dev, counts_dev, h->rep_sum, h->rep_taken, h->rep_same, h->rep_frozen, s);
        rc = check_launch("repeat_fold_kernel"); if (rc) return rc;
    }
    TMARK(1);
    if (!h->overlap_reset) {
        rc = terminal_pass(h, s); if (rc) return rc;
        rc = levels_pass(h, 1, s); if (rc) return rc;
        TMARK(5);
        mwb_launch_reset(h->dev, 1024, s);
        rc = check_launch("reset_kernel"); if (rc) return rc;
        TMARK(6); TMARK(2);
        rc = render_tail(h, 0, s); if (rc) return rc;
        mwb_launch_clear_list(h->dev, s);
        return check_launch("clear_list_kernel");
    }
    // fork: the few envs that ended are regenerated, prepared and rendered on the side stream while the
    // caller's stream renders everybody else; join before returning control of the outputs
    HIP_TRY(hipEventRecord(h->ev_fork, s));
    HIP_TRY(hipStreamWaitEvent(h->side, h->ev_fork, 0));
    rc = terminal_pass(h, h->side); if (rc) return rc;   // the ended envs' last frames, while their state is still there
    rc = levels_pass(h, 1, h->side); if (rc) return rc;   // ... and their next level's generator rows, ahead of reset_kernel
    if (h->timing_now) HIP_TRY(hipEventRecord(h->ev[5], h->side));
    mwb_launch_reset(h->dev, 1024, h->side);   // a handful of envs end per step - or all of them (mass time-out); started ahead of the bulk render
    rc = check_launch("reset_kernel"); if (rc) return rc;
    if (h->timing_now) HIP_TRY(hipEventRecord(h->ev[6], h->side));
    mwb_launch_render(h->dev, 1, h->side);   // reset_kernel has prepared the frame constants of the envs it regenerated
    rc = check_launch("render_kernel"); if (rc) return rc;
    mwb_launch_clear_list(h->dev, h->side);   // the list is consumed; off the critical path
    // also off the critical path: the next step's dispatch order, from the frame costs measured so far
    mwb_launch_order(h->dev, h->side);
    rc = check_launch("order_kernel"); if (rc) return rc;
    HIP_TRY(hipEventRecord(h->ev_join, h->side));
    TMARK(2);
    rc = render_tail(h, 2, s); if (rc) return rc;
    HIP_TRY(hipStreamWaitEvent(s, h->ev_join, 0));
    return MWB_OK;   // the map filled beside this step is adopted by the next step_kernel (device-side flip: graph-capturable)
}

extern "C" int mwb_render(mwb_handle *h, void *stream) {
    if (!h) return set_err(MWB_EINVAL, "null handle");
    USE_DEVICE(h->cfg.device);
    int rc = ensure_ready(h); if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    h->dev.reuse_pass = 0;
    h->dev.step_pass = 0;   // the current state (render_obs() called again shows what the task rule left)
    rc = timing_begin(h, s); if (rc) return rc;
    rc = terminal_clear(h, s); if (rc) return rc;
    TMARK(1); TMARK(5); TMARK(6); TMARK(2);
    return render_tail(h, 0, s);
}

// Frame constants of a view that is not the observation, kept apart from the observation's; the first such view allocates them
// (one dev_alloc: a failure leaves the handle as it was).  The caller holds the device guard.
static int ensure_view_frame(mwb_handle *h) {
    return h->view_frame ? MWB_OK : dev_alloc(h, &h->view_frame, (size_t)h->dev.N * h->dev.frame_words);
}

extern "C" int mwb_render_top_view(mwb_handle *h, uint8_t *out_dev, int width, int height, void *stream) {
    if (!h || !out_dev) return set_err(MWB_EINVAL, "mwb_render_top_view: null argument");
    if (width < 1 || height < 1 || width > 4096 || height > 4096) return set_err(MWB_EINVAL, "mwb_render_top_view: bad frame size");
    USE_DEVICE(h->cfg.device);
    int rc = ensure_ready(h, false); if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (h->dev.ent_task) {   // the current entity list (step_pass 0, as mwb_render), prepared into the view's own frame constants:
        // the observation's are left as they are, so no later observation, reward or done depends on this call
        rc = ensure_view_frame(h); if (rc) return rc;
        MwbDev v = h->dev;
        v.frame = h->view_frame; v.stk = nullptr; v.step_pass = 0; v.wg_ts = nullptr;
        mwb_launch_prep(v, 0, s);
        rc = check_launch("prep_kernel"); if (rc) return rc;
        mwb_launch_top_view_ents(v, out_dev, width, height, s);
        return check_launch("top_view_ents_kernel");
    }
    mwb_launch_prep(h->dev, 0, s);   // the state may have been set from outside since the last render
    rc = check_launch("prep_kernel"); if (rc) return rc;
    mwb_launch_top_view(h->dev, out_dev, width, height, s);
    return check_launch("top_view_kernel");
}

extern "C" int mwb_render_view(mwb_handle *h, uint8_t *out_dev, float *depth_dev, int width, int height, void *stream) {
    if (!h || !out_dev) return set_err(MWB_EINVAL, "mwb_render_view: null argument");
    if (width < 1 || height < 1 || width > 4096 || height > 4096) return set_err(MWB_EINVAL, "mwb_render_view: bad frame size");
    USE_DEVICE(h->cfg.device);
    int rc = ensure_ready(h, false); if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    rc = ensure_view_frame(h); if (rc) return rc;
    MwbDev v = h->dev;
    v.W = width; v.H = height; v.layout = MWB_LAYOUT_HWC; v.obs = out_dev; v.depth = depth_dev; v.want_depth = depth_dev ? 1 : 0;
    v.frame = h->view_frame; v.stk = nullptr; v.step_pass = 0; v.wg_ts = nullptr;
    v.frame_cache = nullptr; v.depth_cache = nullptr; v.frame_cached = nullptr; v.frame_same = nullptr; v.reuse_pass = 0;   // not the observation
    mwb_launch_prep(v, 0, s);
    rc = check_launch("prep_kernel"); if (rc) return rc;
    const int lrc = mwb_launch_render_view(v, s);
    if (lrc) return set_err(lrc == -1 ? MWB_EINVAL : MWB_EHIP, lrc == -1 ? "mwb_render_view: the world's room table does not fit LDS beside a tile" : "mwb_render_view: hipFuncSetAttribute failed");
    return check_launch("render_view_kernel");
}

extern "C" int mwb_visible_ents(mwb_handle *h, uint32_t *mask_dev, void *stream) {
    if (!h || !mask_dev) return set_err(MWB_EINVAL, "mwb_visible_ents: null argument");
    USE_DEVICE(h->cfg.device);
    int rc = ensure_ready(h, false); if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    mwb_launch_prep(h->dev, 0, s);   // the state may have been set from outside since the last render
    rc = check_launch("prep_kernel"); if (rc) return rc;
    mwb_launch_visible(h->dev, mask_dev, s);
    return check_launch("visible_kernel");
}

extern "C" int mwb_get_outputs(mwb_handle *h, mwb_outputs *out) {
    if (!h || !out) return set_err(MWB_EINVAL, "mwb_get_outputs: null argument");
    const MwbDev &d = h->dev;
    out->obs = d.obs; out->depth = d.depth; out->reward = d.reward; out->reward64 = d.reward64; out->done = d.done;
    out->ep_steps = d.ep_steps;
    out->obs_bytes = (size_t)d.N * d.W * d.H * 3;
    out->depth_bytes = d.want_depth ? (size_t)d.N * d.W * d.H * 4 : 0;
    out->stack = h->stack; out->stack_bytes = h->stack_bytes;
    out->feature = d.feature; out->goal_pos = d.goal_pos;
    out->pack = h->pack; out->pack_bytes = h->pack_bytes;
    return MWB_OK;
}

extern "C" int mwb_check(mwb_handle *h) {
    if (!h) return set_err(MWB_EINVAL, "mwb_check: null handle");
    USE_DEVICE(h->cfg.device);
    HIP_TRY(hipDeviceSynchronize());
    int32_t flag = 0;
    HIP_TRY(hipMemcpy(&flag, h->dev.error_flag, sizeof(flag), hipMemcpyDeviceToHost));
    if (flag) return set_err(MWB_ESTATE, "world generation failed for env " + std::to_string(flag - 1) + " (portal / placement condition the reference asserts on)");
    return MWB_OK;
}

// ---------------------------------------------------------------------------------- greyscale
extern "C" int mwb_grey_enable(mwb_handle *h) {
    if (!h) return set_err(MWB_EINVAL, "mwb_grey_enable: null handle");
    MwbDev &d = h->dev;
    if (d.grey) return set_err(MWB_ESTATE, "mwb_grey_enable: already enabled");
    if (h->terminal_on) return set_err(MWB_ESTATE, "mwb_grey_enable: enable greyscale before mwb_terminal_enable (it allocates the terminal grey frames)");
    if ((d.W * d.H) % 4) return set_err(MWB_EINVAL, "mwb_grey_enable: W*H must be a multiple of 4");
    if (d.tile_w > 0) return set_err(MWB_EINVAL, "mwb_grey_enable: not available when observations are rendered in tiles (large frames, MWB_TILE): use mwb_grey_convert");
    // the buffer is filled by the pass that writes obs: enabled after the first one it would lack the frame already rendered
    if (h->have_obs) return set_err(MWB_ESTATE, "mwb_grey_enable: must be called before the first mwb_reset / mwb_step / mwb_render");
    USE_DEVICE(h->cfg.device);
    AllocScope scope(h);
    float *p = nullptr;
    const size_t n = (size_t)d.N * d.W * d.H;
    int rc = dev_alloc(h, &p, n);
    if (rc) return rc;
    d.grey = p; h->grey_bytes = n * sizeof(float);
    scope.keep();
    return MWB_OK;
}

extern "C" int mwb_grey_output(mwb_handle *h, float **grey, size_t *bytes) {
    NEED(h, "handle", h->dev.grey, mwb_grey_enable);
    if (grey) *grey = h->dev.grey;
    if (bytes) *bytes = h->grey_bytes;
    return MWB_OK;
}

extern "C" int mwb_grey_convert(mwb_handle *h, const uint8_t *rgb_dev, float *grey_dev, int n_frames, int width, int height, int layout, void *stream) {
    if (!h || !rgb_dev || !grey_dev) return set_err(MWB_EINVAL, "mwb_grey_convert: null argument");
    if (width < 1 || height < 1 || width > 4096 || height > 4096) return set_err(MWB_EINVAL, "mwb_grey_convert: bad frame size");
    if (layout != MWB_LAYOUT_HWC && layout != MWB_LAYOUT_CWH) return set_err(MWB_EINVAL, "mwb_grey_convert: bad layout");
    const long long blocks = (long long)n_frames * ((width * height + 4095) / 4096);
    if (n_frames < 1 || blocks > 0x7fffffffLL) return set_err(MWB_EINVAL, "mwb_grey_convert: bad frame count");
    USE_DEVICE(h->cfg.device);
    mwb_launch_grey_convert(rgb_dev, grey_dev, n_frames, width * height, layout, (hipStream_t)stream);
    return check_launch("grey_convert_kernel");
}

// ---------------------------------------------------------------------------------- frame stack
extern "C" int mwb_stack_enable(mwb_handle *h, int nstack, int dtype) {
    if (!h) return set_err(MWB_EINVAL, "mwb_stack_enable: null handle");
    const MwbDev &d = h->dev;
    const int fused = (dtype & MWB_STACK_FUSED) != 0;
    const int sliding = fused || (dtype & MWB_STACK_SLIDING) != 0;
    const int grey = (dtype & MWB_STACK_GREY) != 0, cpf = grey ? 1 : 3;
    dtype &= ~(MWB_STACK_SLIDING | MWB_STACK_FUSED | MWB_STACK_GREY);
    if (nstack < 1 || nstack > 16 || (dtype != 0 && dtype != 1)) return set_err(MWB_EINVAL, "mwb_stack_enable: bad nstack / dtype");
    if (d.layout != MWB_LAYOUT_CWH) return set_err(MWB_EINVAL, "mwb_stack_enable: the frame stack is channel-first, create the handle with MWB_LAYOUT_CWH");
    if ((d.W * d.H) % 4) return set_err(MWB_EINVAL, "mwb_stack_enable: W*H must be a multiple of 4");
    if (h->stack) return set_err(MWB_ESTATE, "mwb_stack_enable: already enabled");
    // the terminal rows were laid out for the handle as mwb_terminal_enable found it; they are built from a fused window only
    if (h->terminal_on) return set_err(MWB_ESTATE, fused ? "mwb_stack_enable: enable the frame stack before mwb_terminal_enable (the terminal rows are laid out by it)"
                                                         : "mwb_stack_enable: a handle with mwb_terminal_enable takes the fused frame stack only (MWB_STACK_FUSED, enabled before it)");
    if (grey && dtype != 1) return set_err(MWB_EINVAL, "mwb_stack_enable: MWB_STACK_GREY needs dtype float32 (the reference defines no uint8 grey)");
    if (grey && !d.grey) return set_err(MWB_ESTATE, "mwb_stack_enable: MWB_STACK_GREY needs mwb_grey_enable first");
    // a fused window is filled by the render kernels as they produce frames: enabled after the first observation it would
    // lack the current frame until the next pass (the non-fused forms rebuild theirs from the observation buffer)
    if (fused && h->dev.tile_w > 0) return set_err(MWB_EINVAL, "mwb_stack_enable: MWB_STACK_FUSED is not available when observations are rendered in tiles (large frames, MWB_TILE): use MWB_STACK_SLIDING");
    if (fused && h->have_obs) return set_err(MWB_ESTATE, "mwb_stack_enable: MWB_STACK_FUSED must be enabled before the first mwb_reset / mwb_step / mwb_render");
    if (fused && dtype == 0 && (d.W * d.H) % 16) return set_err(MWB_EINVAL, "mwb_stack_enable: a fused uint8 stack needs W*H to be a multiple of 16");
    USE_DEVICE(h->cfg.device);
    const int planes = sliding ? nstack * cpf + cpf * MWB_STACK_SLACK_FRAMES : nstack * cpf;
    size_t bytes = (size_t)d.N * planes * d.W * d.H * (dtype == 1 ? 4 : 1);
    AllocScope scope(h);
    uint8_t *p = nullptr;
    int rc = dev_alloc(h, &p, bytes);
    if (rc) return rc;
    scope.keep();
    h->stack = p; h->stack_n = nstack; h->stack_dtype = dtype; h->stack_bytes = bytes;
    h->stack_planes = sliding ? planes : 0; h->stack_pos = 0; h->stack_fused = fused; h->stack_cpf = cpf;
    if (fused) {
        MwbDev &dd = h->dev;
        dd.stk = p; dd.stk_float = dtype == 1; dd.stk_C = nstack * cpf; dd.stk_K = planes; dd.stk_pos = 0; dd.stk_cpf = cpf;
    }
    return MWB_OK;
}

extern "C" int mwb_stack_update(mwb_handle *h, int after_reset, void *stream) {
    if (!h || !h->stack) return set_err(MWB_ESTATE, "mwb_stack_update: call mwb_stack_enable first");
    USE_DEVICE(h->cfg.device);
    if (h->stack_fused) return MWB_OK;   // the step / reset that produced the observation has already put it into the window
    if (h->stack_planes) {   // sliding window: the host owns the window position (mwb_stack_window)
        const int cpf = h->stack_cpf, C = h->stack_n * cpf, from = h->stack_pos;
        int mode = 0, pos = from + cpf;
        if (after_reset) { mode = 2; pos = 0; }
        else if (pos + C > h->stack_planes) { mode = 1; pos = 0; }
        mwb_launch_stack_slide(h->dev, h->stack, h->stack_n, h->stack_planes, h->stack_dtype, pos, from, mode, (hipStream_t)stream, cpf);
        h->stack_pos = pos;
        return check_launch("stack_slide_kernel");
    }
    mwb_launch_stack(h->dev, h->stack, h->stack_n, h->stack_dtype, after_reset, (hipStream_t)stream, h->stack_cpf);
    return check_launch("stack_kernel");
}

extern "C" int mwb_stack_window(mwb_handle *h, int *first_plane, int *planes_per_env) {
    if (!h || !h->stack) return set_err(MWB_ESTATE, "mwb_stack_window: call mwb_stack_enable first");
    if (first_plane) *first_plane = h->stack_planes ? h->stack_pos : 0;
    if (planes_per_env) *planes_per_env = h->stack_planes ? h->stack_planes : h->stack_n * h->stack_cpf;
    return MWB_OK;
}

// ---------------------------------------------------------------------------------- rollout storage
// frame ring + per-step rows; the arithmetic is mwb_rollout_map.h, the kernels mwb_rollout.hip
extern "C" int mwb_rollout_enable(mwb_handle *h, int num_steps, int nstack, unsigned flags) {
    if (!h) return set_err(MWB_EINVAL, "mwb_rollout_enable: null handle");
    const MwbDev &d = h->dev;
    if (num_steps < 1 || num_steps > (1 << 24) || nstack < 1 || nstack > 16 || (flags & ~(unsigned)MWB_ROLLOUT_GREY))
        return set_err(MWB_EINVAL, "mwb_rollout_enable: bad num_steps / nstack / flags");
    if (d.layout != MWB_LAYOUT_CWH) return set_err(MWB_EINVAL, "mwb_rollout_enable: stacked observations are channel-first, create the handle with MWB_LAYOUT_CWH");
    if ((d.W * d.H) % 4) return set_err(MWB_EINVAL, "mwb_rollout_enable: W*H must be a multiple of 4");
    if (h->rollout_on) return set_err(MWB_ESTATE, "mwb_rollout_enable: already enabled");
    const int grey = (flags & MWB_ROLLOUT_GREY) != 0;
    if (grey && !d.grey) return set_err(MWB_ESTATE, "mwb_rollout_enable: MWB_ROLLOUT_GREY needs mwb_grey_enable first");
    USE_DEVICE(h->cfg.device);
    MwbRollout r = {};
    r.N = d.N; r.T = num_steps; r.nstack = nstack; r.R = mwb_rollout_ring_slots(num_steps, nstack); r.grey = grey;
    r.base = 0; r.cursor = -1;
    r.frame_bytes = (size_t)d.W * d.H * (grey ? sizeof(float) : 3);
    const size_t N = (size_t)d.N, T1 = (size_t)num_steps + 1, ring_bytes = (size_t)r.R * N * r.frame_bytes;
    AllocScope scope(h);
    int rc = dev_alloc(h, &r.ring, ring_bytes);
    if (!rc) rc = dev_alloc(h, &r.age, T1 * N);
    if (!rc) rc = dev_alloc(h, &r.reward, (size_t)num_steps * N);
    if (!rc) rc = dev_alloc(h, &r.mask, T1 * N);
    if (!rc) rc = dev_alloc(h, &r.feature, T1 * N * 2);
    if (!rc) rc = dev_alloc(h, &r.rejected, (size_t)1);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    scope.keep();
    h->rollout = r; h->rollout_ring_bytes = ring_bytes; h->rollout_on = true;
    return MWB_OK;
}

extern "C" int mwb_rollout_push(mwb_handle *h, int after_reset, const uint8_t *fresh_dev, void *stream) {
    NEED(h, "handle", h->rollout_on, mwb_rollout_enable);
    MwbRollout &r = h->rollout;
    if (!after_reset && r.cursor < 0) return set_err(MWB_ESTATE, "mwb_rollout_push: the first push must follow a reset (after_reset != 0)");
    if (!after_reset && r.cursor >= r.T) return set_err(MWB_ESTATE, "mwb_rollout_push: the rollout holds num_steps steps already: call mwb_rollout_after_update");
    USE_DEVICE(h->cfg.device);
    const MwbDev &d = h->dev;
    hipStream_t s = (hipStream_t)stream;
    const int t = after_reset ? 0 : r.cursor + 1;
    // the frames of a slot are one contiguous slab in the order of the output buffer: a device-to-device copy, no kernel
    const size_t slab = (size_t)r.N * r.frame_bytes;
    const void *frames = r.grey ? (const void *)d.grey : (const void *)d.obs;
    HIP_TRY(hipMemcpyAsync(r.ring + (size_t)mwb_rollout_slot(r.base, t, 0, r.R) * slab, frames, slab, hipMemcpyDeviceToDevice, s));
    mwb_launch_rollout_push(r, t, after_reset != 0, fresh_dev, d.done, d.reward, d.feature, s);
    if (int rc = check_launch("rollout_push_kernel")) return rc;
    if (h->learner_on && !after_reset) {   // taken[t - 1]: the repeat's count, or 1 for a plain step and for a pass that is not a step
        mwb_launch_rollout_taken(r, h->learner, t, (h->last_pass_repeat && !fresh_dev) ? h->rep_taken : nullptr, s);
        if (int rc = check_launch("rollout_taken_kernel")) return rc;
    }
    r.cursor = t;
    return MWB_OK;
}

extern "C" int mwb_rollout_gather(mwb_handle *h, const int64_t *index_dev, int count, void *out_dev, int dtype, void *stream) {
    NEED(h, "handle", h->rollout_on, mwb_rollout_enable);
    const MwbRollout &r = h->rollout;
    if (dtype != 0 && dtype != 1) return set_err(MWB_EINVAL, "mwb_rollout_gather: dtype must be 0 (uint8) or 1 (float32)");
    if (r.grey && dtype == 0) return set_err(MWB_EINVAL, "mwb_rollout_gather: a grey rollout is gathered as float32 (the reference defines no uint8 grey)");
    if (count < 0) return set_err(MWB_EINVAL, "mwb_rollout_gather: count < 0");
    if (r.cursor < 0) return set_err(MWB_ESTATE, "mwb_rollout_gather: nothing has been pushed yet");
    if (count == 0) return MWB_OK;
    if (!index_dev || !out_dev) return set_err(MWB_EINVAL, "mwb_rollout_gather: null argument");
    if ((uintptr_t)out_dev & 15) return set_err(MWB_EINVAL, "mwb_rollout_gather: out_dev must be 16-byte aligned");
    USE_DEVICE(h->cfg.device);
    mwb_launch_rollout_gather(r, index_dev, count, out_dev, dtype, (hipStream_t)stream);
    return check_launch("rollout_gather_kernel");
}

// the windowed gather: the rule is mwb_rollout_window_map.h, the kernels mwb_rollout_window.hip
static int window_of(const mwb_handle *h, const struct mwb_rollout_window *w, const char *who, MwbWindow &out) {
    if (int limit = mwb_window_check(w->out_w, w->out_h, w->border, w->dx_lo, w->dx_hi, w->dy_lo, w->dy_hi))
        return set_err(MWB_EINVAL, std::string(who) + ": " + mwb_window_limit_text(limit));
    out = MwbWindow{h->dev.W, h->dev.H, w->out_w, w->out_h, w->border, w->dx_lo, w->dx_hi, w->dy_lo, w->dy_hi};
    return MWB_OK;
}

extern "C" int mwb_rollout_window_offsets(mwb_handle *h, const struct mwb_rollout_window *w, uint64_t seed, uint64_t call,
                                          const int64_t *index_dev, int count, int32_t *offsets_dev, void *stream) {
    if (!h) return set_err(MWB_EINVAL, "mwb_rollout_window_offsets: null handle");
    if (!w) return set_err(MWB_EINVAL, "mwb_rollout_window_offsets: null argument");
    MwbWindow win;
    if (int rc = window_of(h, w, "mwb_rollout_window_offsets", win)) return rc;
    if (count < 0) return set_err(MWB_EINVAL, "mwb_rollout_window_offsets: count < 0");
    if (count == 0) return MWB_OK;
    if (!index_dev || !offsets_dev) return set_err(MWB_EINVAL, "mwb_rollout_window_offsets: null argument");
    if ((uintptr_t)offsets_dev & 7) return set_err(MWB_EINVAL, "mwb_rollout_window_offsets: offsets_dev must be 8-byte aligned");
    USE_DEVICE(h->cfg.device);
    mwb_launch_rollout_window_offsets(win, mwb_window_key(seed, call), index_dev, count, offsets_dev, (hipStream_t)stream);
    return check_launch("rollout_window_offsets_kernel");
}

extern "C" int mwb_rollout_gather_window(mwb_handle *h, const int64_t *index_dev, int count, const struct mwb_rollout_window *w,
                                         const int32_t *offsets_dev, void *out_dev, int dtype, void *stream) {
    if (!h) return set_err(MWB_EINVAL, "mwb_rollout_gather_window: null handle");
    NEED(w, "argument", h->rollout_on, mwb_rollout_enable);
    const MwbRollout &r = h->rollout;
    MwbWindow win;
    if (int rc = window_of(h, w, "mwb_rollout_gather_window", win)) return rc;
    if (dtype != 0 && dtype != 1) return set_err(MWB_EINVAL, "mwb_rollout_gather_window: dtype must be 0 (uint8) or 1 (float32)");
    if (r.grey && dtype == 0) return set_err(MWB_EINVAL, "mwb_rollout_gather_window: a grey rollout is gathered as float32 (the reference defines no uint8 grey)");
    if (count < 0) return set_err(MWB_EINVAL, "mwb_rollout_gather_window: count < 0");
    if (r.cursor < 0) return set_err(MWB_ESTATE, "mwb_rollout_gather_window: nothing has been pushed yet");
    if (count == 0) return MWB_OK;
    if (!index_dev || !offsets_dev || !out_dev) return set_err(MWB_EINVAL, "mwb_rollout_gather_window: null argument");
    if ((uintptr_t)out_dev & 15) return set_err(MWB_EINVAL, "mwb_rollout_gather_window: out_dev must be 16-byte aligned");
    if ((uintptr_t)offsets_dev & 7) return set_err(MWB_EINVAL, "mwb_rollout_gather_window: offsets_dev must be 8-byte aligned");
    USE_DEVICE(h->cfg.device);
    mwb_launch_rollout_window(r, win, index_dev, count, offsets_dev, out_dev, dtype, (hipStream_t)stream);
    return check_launch("rollout_window_kernel");
}

extern "C" int mwb_rollout_after_update(mwb_handle *h, void *stream) {
    NEED(h, "handle", h->rollout_on, mwb_rollout_enable);
    MwbRollout &r = h->rollout;
    if (r.cursor < 0) return set_err(MWB_ESTATE, "mwb_rollout_after_update: nothing has been pushed yet");
    USE_DEVICE(h->cfg.device);
    mwb_launch_rollout_after_update(r, (hipStream_t)stream);
    if (int rc = check_launch("rollout_after_update_kernel")) return rc;
    r.base = mwb_rollout_next_base(r.base, r.T, r.R);
    r.cursor = 0;
    return MWB_OK;
}

extern "C" int mwb_rollout_info(mwb_handle *h, struct mwb_rollout_info *out) {
    NEED(h && out, "argument", h->rollout_on, mwb_rollout_enable);
    const MwbRollout &r = h->rollout;
    const size_t N = (size_t)r.N, T1 = (size_t)r.T + 1;
    memset(out, 0, sizeof(*out));
    out->reward = r.reward; out->mask = r.mask; out->feature = r.feature; out->age = r.age; out->ring = r.ring;
    out->reward_bytes = (size_t)r.T * N * sizeof(float); out->mask_bytes = T1 * N * sizeof(float);
    out->feature_bytes = T1 * N * 2 * sizeof(float); out->age_bytes = T1 * N; out->ring_bytes = h->rollout_ring_bytes;
    out->num_steps = r.T; out->nstack = r.nstack; out->grey = r.grey; out->cursor = r.cursor; out->base = r.base;
    return MWB_OK;
}

extern "C" int mwb_rollout_rejected(mwb_handle *h, unsigned long long *rows) {
    if (rows) *rows = 0;
    NEED(h && rows, "argument", h->rollout_on, mwb_rollout_enable);
    return read_counters(h, rows, h->rollout.rejected, 1);
}

// ------------------------------------------------------------------------------------ episode monitor
// returns, lengths, the log of the last episodes, evaluation quotas; the arithmetic is mwb_monitor_map.h, the kernels mwb_monitor.hip
static_assert(sizeof(mwb_monitor_counts) == 32, "two u64 counters, then the four u32 the kernels index with MWB_MON_*");
static_assert(offsetof(mwb_monitor_counts, dropped) == 8 * MWB_MON_DROPPED && offsetof(mwb_monitor_counts, remaining) == 16 + 4 * MWB_MON_REMAINING &&
              offsetof(mwb_monitor_counts, quota) == 16 + 4 * MWB_MON_QUOTA && offsetof(mwb_monitor_counts, last_base) == 16 + 4 * MWB_MON_BASE &&
              offsetof(mwb_monitor_counts, last_count) == 16 + 4 * MWB_MON_COUNT, "struct mwb_monitor_counts is what the kernels write");

extern "C" int mwb_monitor_enable(mwb_handle *h, int capacity, int quota_max) {
    if (!h) return set_err(MWB_EINVAL, "mwb_monitor_enable: null handle");
    if (capacity < 1 || capacity > MWB_MONITOR_MAX_CAPACITY) return set_err(MWB_EINVAL, "mwb_monitor_enable: capacity must lie in 1 .. " + std::to_string(MWB_MONITOR_MAX_CAPACITY));
    if (quota_max < 0 || quota_max > MWB_MONITOR_MAX_QUOTA) return set_err(MWB_EINVAL, "mwb_monitor_enable: quota_max must lie in 0 .. " + std::to_string(MWB_MONITOR_MAX_QUOTA));
    if (h->cfg.no_auto_reset) return set_err(MWB_EINVAL, "mwb_monitor_enable: the handle was created with no_auto_reset: a finished env stops, no later step belongs to an episode");
    if (h->monitor_on) return set_err(MWB_ESTATE, "mwb_monitor_enable: already enabled");
    USE_DEVICE(h->cfg.device);
    MwbMonitor m = {};
    m.N = h->dev.N; m.capacity = capacity; m.Q = quota_max; m.n_waves = (int)(((size_t)m.N + 63) / 64);
    const size_t N = (size_t)m.N, C = (size_t)capacity, QN = (size_t)quota_max * N, NW = (size_t)m.n_waves;
    // two passes over one list of pieces: sizes first, pointers after the allocation.  The first six are the host pack and lie
    // back to back (8-byte pieces first, so every piece is aligned to its element); every later piece starts on 256 bytes
    size_t at = 0;
    char *base = nullptr;
    auto piece = [&](auto *&p, size_t bytes, bool packed) {
        if (!packed) at = (at + 255) & ~(size_t)255;
        if (base) p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(base + at);
        at += bytes;
    };
    size_t pack_bytes = 0;
    auto carve = [&]() {
        at = 0;
        piece(m.last_return, N * 8, true); piece(m.last_len, N * 4, true); piece(m.last_calls, N * 4, true);
        piece(m.counts64, sizeof(mwb_monitor_counts), true); piece(m.logged, N, true); piece(m.retired, N, true);
        pack_bytes = at;
        piece(m.run_return, N * 8, false); piece(m.run_len, N * 4, false); piece(m.run_calls, N * 4, false); piece(m.finished, N * 4, false);
        piece(m.partial, N, false);
        piece(m.log_return, C * 8, false); piece(m.log_len, C * 4, false); piece(m.log_calls, C * 4, false); piece(m.log_env, C * 4, false);
        piece(m.tab_return, QN * 8, false); piece(m.tab_len, QN * 4, false);
        piece(m.wave_ballot, NW * 8, false); piece(m.wave_base, NW * 4, false); piece(m.wave_aux, NW * 4, false);
    };
    carve();
    AllocScope scope(h);
    if (int rc = dev_alloc(h, &base, at)) return rc;
    carve();
    m.counts32 = (uint32_t *)(m.counts64 + 2);
    if (!quota_max) { m.tab_return = nullptr; m.tab_len = nullptr; }
    mwb_launch_monitor_quota(m, 0, nullptr);   // quota 0, remaining = N, the table as NaN / -1
    if (int rc = check_launch("monitor_quota_kernel")) return rc;
    HIP_TRY(hipDeviceSynchronize());
    scope.keep();
    h->monitor = m; h->monitor_pack = m.last_return; h->monitor_pack_bytes = pack_bytes; h->monitor_on = true;
    return MWB_OK;
}

extern "C" int mwb_monitor_update(mwb_handle *h, const uint8_t *skip_mask_dev, const double *reward64_dev, const uint8_t *done_dev,
                                  const int32_t *taken_dev, void *stream) {
    NEED(h, "handle", h->monitor_on, mwb_monitor_enable);
    USE_DEVICE(h->cfg.device);
    // the sub-steps of the call: the repeat's count if that was the last pass, 1 (NULL) after a plain step - the rollout's rule
    const int32_t *taken = taken_dev ? taken_dev : (h->last_pass_repeat ? h->rep_taken : nullptr);
    mwb_launch_monitor_update(h->monitor, skip_mask_dev, reward64_dev ? reward64_dev : h->dev.reward64, done_dev ? done_dev : h->dev.done, taken,
                              (hipStream_t)stream);
    return check_launch("monitor update kernels");
}

extern "C" int mwb_monitor_clear(mwb_handle *h, const uint8_t *mask_dev, int partial, void *stream) {
    NEED(h, "handle", h->monitor_on, mwb_monitor_enable);
    USE_DEVICE(h->cfg.device);
    mwb_launch_monitor_clear(h->monitor, mask_dev, partial != 0, (hipStream_t)stream);
    return check_launch("monitor_clear_kernel");
}

extern "C" int mwb_monitor_quota(mwb_handle *h, int quota, void *stream) {
    NEED(h, "handle", h->monitor_on, mwb_monitor_enable);
    if (quota < 0 || quota > h->monitor.Q) return set_err(MWB_EINVAL, "mwb_monitor_quota: quota must lie in 0 .. quota_max = " + std::to_string(h->monitor.Q));
    USE_DEVICE(h->cfg.device);
    mwb_launch_monitor_quota(h->monitor, quota, (hipStream_t)stream);
    return check_launch("monitor_quota_kernel");
}

extern "C" int mwb_monitor_info(mwb_handle *h, struct mwb_monitor_info *out) {
    NEED(h && out, "argument", h->monitor_on, mwb_monitor_enable);
    const MwbMonitor &m = h->monitor;
    memset(out, 0, sizeof(*out));
    out->run_return = m.run_return; out->last_return = m.last_return;
    out->run_len = m.run_len; out->run_calls = m.run_calls; out->last_len = m.last_len; out->last_calls = m.last_calls; out->finished = m.finished;
    out->partial = m.partial; out->retired = m.retired; out->logged = m.logged;
    out->log_return = m.log_return; out->log_len = m.log_len; out->log_calls = m.log_calls; out->log_env = m.log_env;
    out->tab_return = m.tab_return; out->tab_len = m.tab_len;
    out->counts = m.counts64; out->host_pack = h->monitor_pack; out->host_pack_bytes = h->monitor_pack_bytes;
    out->num_envs = m.N; out->capacity = m.capacity; out->quota_max = m.Q;
    return MWB_OK;
}

extern "C" int mwb_monitor_read(mwb_handle *h, struct mwb_monitor_counts *out) {
    if (!h || !out) return set_err(MWB_EINVAL, "mwb_monitor_read: null argument");
    memset(out, 0, sizeof(*out));
    if (!h->monitor_on) return set_err(MWB_ESTATE, "mwb_monitor_read: call mwb_monitor_enable first");
    USE_DEVICE(h->cfg.device);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, h->monitor.counts64, sizeof(*out), hipMemcpyDeviceToHost));
    return MWB_OK;
}

// ------------------------------------------------------------------- rollout storage: the learner half
// the small columns and the returns scan; the arithmetic is mwb_returns_scan.h, the kernels mwb_rollout_learner.hip
static_assert(MWB_RETURNS_MAX_K == MWB_MAX_REPEAT, "the discount tables have one row per possible `taken`");
static_assert(MWB_SCAN_DISCOUNTED == MWB_RETURNS_DISCOUNTED && MWB_SCAN_GAE == MWB_RETURNS_GAE && MWB_SCAN_PSI == MWB_RETURNS_PSI, "mode numbers");

extern "C" int mwb_rollout_learner_enable(mwb_handle *h) {
    NEED(h, "handle", h->rollout_on, mwb_rollout_enable);
    if (h->learner_on) return set_err(MWB_ESTATE, "mwb_rollout_learner_enable: already enabled");
    USE_DEVICE(h->cfg.device);
    const size_t N = (size_t)h->rollout.N, T = (size_t)h->rollout.T, T1 = T + 1;
    MwbLearner l = {};
    AllocScope scope(h);
    int rc = dev_alloc(h, &l.action, T * N);
    if (!rc) rc = dev_alloc(h, &l.log_prob, T * N);
    if (!rc) rc = dev_alloc(h, &l.value, T1 * N);
    if (!rc) rc = dev_alloc(h, &l.taken, T * N);
    if (!rc) rc = dev_alloc(h, &l.ret, T1 * N);
    if (!rc) rc = dev_alloc(h, &l.adv, T * N);
    if (!rc) rc = dev_alloc(h, &l.psi_ret, T1 * N * 2);
    if (rc) return rc;
    HIP_TRY(hipMemsetD32((hipDeviceptr_t)l.taken, 1, T * N));   // a transition is one sub-step until a push says otherwise
    HIP_TRY(hipDeviceSynchronize());
    scope.keep();
    h->learner = l; h->learner_on = true;
    return MWB_OK;
}

extern "C" int mwb_rollout_learner_info(mwb_handle *h, struct mwb_rollout_learner_info *out) {
    NEED(h && out, "argument", h->learner_on, mwb_rollout_learner_enable);
    const MwbLearner &l = h->learner;
    const size_t N = (size_t)h->rollout.N, T = (size_t)h->rollout.T, T1 = T + 1;
    memset(out, 0, sizeof(*out));
    out->action = l.action; out->log_prob = l.log_prob; out->value = l.value; out->taken = l.taken; out->ret = l.ret; out->adv = l.adv;
    out->psi_ret = l.psi_ret;
    out->action_bytes = T * N * sizeof(int64_t); out->log_prob_bytes = T * N * sizeof(float); out->value_bytes = T1 * N * sizeof(float);
    out->taken_bytes = T * N * sizeof(int32_t); out->ret_bytes = T1 * N * sizeof(float); out->adv_bytes = T * N * sizeof(float);
    out->psi_ret_bytes = T1 * N * 2 * sizeof(float);
    return MWB_OK;
}

extern "C" int mwb_rollout_insert(mwb_handle *h, const int64_t *action_dev, const int32_t *action_i32_dev, const float *log_prob_dev,
                                  const float *value_dev, void *stream) {
    NEED(h, "handle", h->learner_on, mwb_rollout_learner_enable);
    if (action_dev && action_i32_dev) return set_err(MWB_EINVAL, "mwb_rollout_insert: at most one of action / action_i32 may be given");
    const MwbRollout &r = h->rollout;
    if (r.cursor < 1) return set_err(MWB_ESTATE, "mwb_rollout_insert: no transition has been pushed in this window yet");
    if (!action_dev && !action_i32_dev && !log_prob_dev && !value_dev) return MWB_OK;
    USE_DEVICE(h->cfg.device);
    mwb_launch_rollout_insert(r, h->learner, r.cursor - 1, action_dev, action_i32_dev, log_prob_dev, value_dev, (hipStream_t)stream);
    return check_launch("rollout_insert_kernel");
}

extern "C" int mwb_rollout_returns(mwb_handle *h, int mode, double gamma, double tau, const float *next_value_dev, const float *next_psi_dev,
                                   const float *reward_override_dev, void *stream) {
    NEED(h, "handle", h->learner_on, mwb_rollout_learner_enable);
    if (mode != MWB_RETURNS_DISCOUNTED && mode != MWB_RETURNS_GAE && mode != MWB_RETURNS_PSI) return set_err(MWB_EINVAL, "mwb_rollout_returns: unknown mode");
    const MwbRollout &r = h->rollout;
    if (r.cursor != r.T) return set_err(MWB_ESTATE, "mwb_rollout_returns: the rollout does not hold num_steps steps yet");
    const float *next = mode == MWB_RETURNS_PSI ? next_psi_dev : next_value_dev;
    if (!next) return set_err(MWB_EINVAL, mode == MWB_RETURNS_PSI ? "mwb_rollout_returns: MWB_RETURNS_PSI needs next_psi" : "mwb_rollout_returns: next_value is null");
    USE_DEVICE(h->cfg.device);
    MwbReturnsTables tab;
    mwb_returns_tables(gamma, tau, &tab);
    mwb_launch_rollout_returns(r, h->learner, mode, tab, next, reward_override_dev ? reward_override_dev : r.reward, (hipStream_t)stream);
    return check_launch("rollout_returns_kernel");
}

extern "C" int mwb_rollout_gather_cols(mwb_handle *h, const int64_t *index_dev, int count, const float *adv_src_dev, float *out_f32_dev,
                                       int64_t *out_action_dev, void *stream) {
    NEED(h, "handle", h->learner_on, mwb_rollout_learner_enable);
    if (count < 0) return set_err(MWB_EINVAL, "mwb_rollout_gather_cols: count < 0");
    if (count == 0) return MWB_OK;
    if (!index_dev || !out_f32_dev || !out_action_dev) return set_err(MWB_EINVAL, "mwb_rollout_gather_cols: null argument");
    USE_DEVICE(h->cfg.device);
    mwb_launch_rollout_gather_cols(h->rollout, h->learner, index_dev, count, adv_src_dev ? adv_src_dev : h->learner.adv, out_f32_dev, out_action_dev,
                                   (hipStream_t)stream);
    return check_launch("rollout_gather_cols_kernel");
}

// -------------------------------------------------------------------------------- terminal observations
// the frame an episode ended on, why it ended, compact stacked rows; the arithmetic is mwb_terminal_map.h, the kernels
// mwb_terminal.hip, the pass itself terminal_pass() above
extern "C" int mwb_terminal_enable(mwb_handle *h, int capacity, unsigned flags) {
    if (!h) return set_err(MWB_EINVAL, "mwb_terminal_enable: null handle");
    MwbDev &d = h->dev;
    if (h->terminal_on) return set_err(MWB_ESTATE, "mwb_terminal_enable: already enabled");
    if (!d.auto_reset) return set_err(MWB_EINVAL, "mwb_terminal_enable: the handle was created with no_auto_reset (its observation IS the terminal frame)");
    if (capacity < 1 || capacity > d.N) return set_err(MWB_EINVAL, "mwb_terminal_enable: capacity must lie in 1 .. num_envs");
    if (flags & ~(unsigned)MWB_TERMINAL_FLOAT) return set_err(MWB_EINVAL, "mwb_terminal_enable: unknown flag");
    if (h->stack && !h->stack_fused)
        return set_err(MWB_EINVAL, "mwb_terminal_enable: the handle's frame stack is not MWB_STACK_FUSED (the terminal rows are built from the fused window's history)");
    if (h->stack && (flags & MWB_TERMINAL_FLOAT) && h->stack_dtype != 1)
        return set_err(MWB_EINVAL, "mwb_terminal_enable: MWB_TERMINAL_FLOAT on a handle with a uint8 frame stack (the rows take the stack's dtype)");
    // the terminal frame of the very first step needs the buffers: nothing may have been rendered yet
    if (h->have_obs) return set_err(MWB_ESTATE, "mwb_terminal_enable: must be called before the first mwb_reset / mwb_step / mwb_render");
    USE_DEVICE(h->cfg.device);
    MwbTerminal t = {};
    t.N = d.N; t.capacity = capacity; t.plane = (size_t)d.W * d.H;
    t.nstack = h->stack ? h->stack_n : 1; t.cpf = h->stack ? h->stack_cpf : 3;
    t.rows_float = h->stack ? h->stack_dtype == 1 : (flags & MWB_TERMINAL_FLOAT) != 0;
    t.grey = h->stack && h->stack_cpf == 1;
    const size_t N = (size_t)d.N, rows_bytes = (size_t)capacity * t.nstack * t.cpf * t.plane * (t.rows_float ? 4 : 1);
    AllocScope scope(h);
    int rc = dev_alloc(h, &t.frames, N * t.plane * 3);
    if (!rc && d.grey) rc = dev_alloc(h, &t.grey_frames, N * t.plane);
    if (!rc) rc = dev_alloc(h, &t.frame_consts, N * d.frame_words);
    if (!rc) rc = dev_alloc(h, &t.cause, N);
    if (!rc) rc = dev_alloc(h, &t.row_of, N);
    if (!rc) rc = dev_alloc(h, &t.row_env, (size_t)capacity);
    if (!rc) rc = dev_alloc(h, &t.count, (size_t)1);
    if (!rc) rc = dev_alloc(h, &t.dropped, (size_t)1);
    if (!rc) rc = dev_alloc(h, &t.rows, rows_bytes);
    if (rc) return rc;
    HIP_TRY(hipMemset(t.row_of, 0xFF, N * sizeof(int32_t)));   // -1: no env has a row
    HIP_TRY(hipMemset(t.row_env, 0xFF, (size_t)capacity * sizeof(int32_t)));
    HIP_TRY(hipDeviceSynchronize());
    scope.keep();
    h->terminal = t; h->terminal_rows_bytes = rows_bytes; h->terminal_on = true;
    d.end_cause = t.cause;
    return MWB_OK;
}

extern "C" int mwb_terminal_info(mwb_handle *h, struct mwb_terminal_info *out) {
    NEED(h && out, "argument", h->terminal_on, mwb_terminal_enable);
    const MwbTerminal &t = h->terminal;
    memset(out, 0, sizeof(*out));
    out->cause = t.cause; out->frames = t.frames; out->grey = t.grey_frames; out->row_of = t.row_of; out->row_env = t.row_env; out->count = t.count;
    out->rows = t.rows;
    out->frames_bytes = (size_t)t.N * t.plane * 3; out->grey_bytes = t.grey_frames ? (size_t)t.N * t.plane * sizeof(float) : 0;
    out->rows_bytes = h->terminal_rows_bytes;
    out->capacity = t.capacity; out->rows_float = t.rows_float; out->planes = t.nstack * t.cpf; out->nstack = t.nstack;
    return MWB_OK;
}

extern "C" int mwb_terminal_dropped(mwb_handle *h, unsigned long long *envs) {
    if (envs) *envs = 0;
    NEED(h && envs, "argument", h->terminal_on, mwb_terminal_enable);
    return read_counters(h, envs, h->terminal.dropped, 1);
}

extern "C" int mwb_rollout_bootstrap(mwb_handle *h, const float *value_rows_dev, double gamma, void *stream) {
    NEED(h && value_rows_dev, "argument", h->terminal_on, mwb_terminal_enable);
    if (!h->rollout_on) return set_err(MWB_ESTATE, "mwb_rollout_bootstrap: call mwb_rollout_enable first");
    const MwbRollout &r = h->rollout;
    if (r.cursor < 1) return set_err(MWB_ESTATE, "mwb_rollout_bootstrap: no transition has been pushed in this window yet");
    USE_DEVICE(h->cfg.device);
    MwbReturnsTables tab;
    mwb_returns_tables(gamma, 1.0, &tab);
    const size_t at = (size_t)(r.cursor - 1) * r.N;
    mwb_launch_terminal_bootstrap(h->terminal, tab, r.reward + at, h->learner_on ? h->learner.taken + at : nullptr, value_rows_dev, (hipStream_t)stream);
    return check_launch("terminal_bootstrap_kernel");
}

// -------------------------------------------------------------------------------- level sets
// every regeneration of an env starts from the generator row of a level seed chosen on the device; the arithmetic is
// mwb_levels_map.h, the kernels mwb_levels.hip, the pass itself levels_pass() above
extern "C" int mwb_levels_enable(mwb_handle *h, int64_t num_levels, uint64_t start_level, const uint64_t *level_seeds_host, int mode,
                                 uint64_t sampler_seed, int64_t env_offset, int64_t env_stride, unsigned flags) {
    if (!h) return set_err(MWB_EINVAL, "mwb_levels_enable: null handle");
    if (h->levels_on) return set_err(MWB_ESTATE, "mwb_levels_enable: already enabled");
    if (num_levels < 1 || num_levels > MWB_LEVELS_MAX) return set_err(MWB_EINVAL, "mwb_levels_enable: num_levels must lie in 1 .. 2^31 - 1");
    if (level_seeds_host && num_levels > MWB_LEVELS_MAX_TABLE) return set_err(MWB_EINVAL, "mwb_levels_enable: a seed table holds at most 2^24 levels");
    if (mode != MWB_LEVELS_SEQUENTIAL && mode != MWB_LEVELS_UNIFORM && mode != MWB_LEVELS_TABLE) return set_err(MWB_EINVAL, "mwb_levels_enable: unknown mode");
    if (env_offset < 0) return set_err(MWB_EINVAL, "mwb_levels_enable: env_offset < 0");
    if (env_stride < 1) return set_err(MWB_EINVAL, "mwb_levels_enable: env_stride < 1");
    if (flags & ~(unsigned)MWB_LEVELS_TALLY) return set_err(MWB_EINVAL, "mwb_levels_enable: unknown flag");
    if ((flags & MWB_LEVELS_TALLY) && num_levels > MWB_LEVELS_MAX_TALLY) return set_err(MWB_EINVAL, "mwb_levels_enable: MWB_LEVELS_TALLY takes at most 2^22 levels");
    USE_DEVICE(h->cfg.device);
    MwbLevels v = {};
    v.N = h->dev.N; v.L = num_levels; v.start_level = start_level; v.env_offset = env_offset; v.env_stride = env_stride;
    const size_t N = (size_t)v.N, L = (size_t)num_levels;
    uint64_t *seeds = nullptr; uint32_t *base = nullptr;
    AllocScope scope(h);
    int rc = dev_alloc(h, &base, (size_t)624);
    if (!rc && level_seeds_host) rc = dev_alloc(h, &seeds, L);
    if (!rc) rc = dev_alloc(h, &v.params, (size_t)2);
    if (!rc) rc = dev_alloc(h, &v.index, 2 * N);   // index | prev_index, contiguous: one copy mirrors both
    if (!rc) rc = dev_alloc(h, &v.next_level, N);
    if (!rc) rc = dev_alloc(h, &v.episode_no, N);
    if (!rc) rc = dev_alloc(h, &v.rejected, (size_t)1);
    if (!rc && (flags & MWB_LEVELS_TALLY)) rc = dev_alloc(h, &v.tallies, 3 * L);
    if (rc) return rc;
    uint32_t base_host[624];
    mwb_levels_mt_base(base_host);   // the constant first loop of init_by_array: once, here
    const uint64_t params[2] = {(uint64_t)mode, sampler_seed};
    HIP_TRY(hipMemcpy(base, base_host, sizeof(base_host), hipMemcpyHostToDevice));
    if (seeds) HIP_TRY(hipMemcpy(seeds, level_seeds_host, L * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(v.params, params, sizeof(params), hipMemcpyHostToDevice));
    v.prev_index = v.index + N;
    HIP_TRY(hipMemset(v.index, 0xFF, 2 * N * sizeof(int32_t)));    // -1: no level yet, no previous one
    HIP_TRY(hipMemset(v.next_level, 0xFF, N * sizeof(int32_t)));   // -1: no request
    HIP_TRY(hipDeviceSynchronize());
    scope.keep();
    v.base = base; v.seeds = seeds;
    h->levels = v; h->levels_mode = mode; h->levels_sampler_seed = sampler_seed; h->levels_flags = flags; h->levels_on = true;
    h->seeded = true;   // every env is given a stream before it is generated
    return invalidate_frames(h, 0, h->dev.N);
}

extern "C" int mwb_levels_restart(mwb_handle *h, int mode, uint64_t sampler_seed, int clear_tally, void *stream) {
    NEED(h, "handle", h->levels_on, mwb_levels_enable);
    if (mode != MWB_LEVELS_SEQUENTIAL && mode != MWB_LEVELS_UNIFORM && mode != MWB_LEVELS_TABLE) return set_err(MWB_EINVAL, "mwb_levels_restart: unknown mode");
    USE_DEVICE(h->cfg.device);
    mwb_launch_levels_restart(h->levels, mode, sampler_seed, clear_tally != 0, (hipStream_t)stream);
    int rc = check_launch("levels_restart_kernel"); if (rc) return rc;
    h->levels_mode = mode; h->levels_sampler_seed = sampler_seed;
    return MWB_OK;
}

extern "C" int mwb_levels_info(mwb_handle *h, struct mwb_levels_info *out) {
    NEED(h && out, "argument", h->levels_on, mwb_levels_enable);
    const MwbLevels &v = h->levels;
    memset(out, 0, sizeof(*out));
    out->index = v.index; out->prev_index = v.prev_index; out->next_level = v.next_level; out->episode_no = v.episode_no;
    out->tallies = v.tallies; out->level_seeds = v.seeds;
    out->num_levels = v.L; out->start_level = v.start_level; out->sampler_seed = h->levels_sampler_seed;
    out->env_offset = v.env_offset; out->env_stride = v.env_stride;
    out->mode = h->levels_mode; out->flags = h->levels_flags;
    return MWB_OK;
}

extern "C" int mwb_levels_rejected(mwb_handle *h, unsigned long long *entries) {
    if (entries) *entries = 0;
    NEED(h && entries, "argument", h->levels_on, mwb_levels_enable);
    return read_counters(h, entries, h->levels.rejected, 1);
}

// ------------------------------------------------------------------------------ copying environments
// the first field of the two configurations that differs (num_envs and domain_rand may), or null.  Compared as the handles use
// them: defaults filled in (max_episode_steps <= 0, task_args 0, use_default_params)
static const char *config_difference(const mwb_handle *a, const mwb_handle *b) {
    const MwbDev &x = a->dev, &y = b->dev;
    if (a->cfg.abi_version != b->cfg.abi_version) return "abi_version";
    if (x.task != y.task) return "task";
    if (x.W != y.W) return "obs_width";
    if (x.H != y.H) return "obs_height";
    if (x.want_depth != y.want_depth) return "want_depth";
    if (x.layout != y.layout) return "layout";
    if (x.max_episode_steps != y.max_episode_steps) return "max_episode_steps";
    if (a->cfg.device != b->cfg.device) return "device";
    for (int i = 0; i < 4; i++) if (x.task_args[i] != y.task_args[i]) return "task_args";
    if (x.auto_reset != y.auto_reset) return "no_auto_reset";
    for (int i = 0; i < MWB_NPARAM; i++)
        for (int k = 0; k < 3; k++)
            if (x.params[i].def[k] != y.params[i].def[k] || x.params[i].lo[k] != y.params[i].lo[k] || x.params[i].hi[k] != y.params[i].hi[k]) return "params";
    return nullptr;
}

// the descriptor table for copies from src into dst: built once per pair of handles and kept by dst (four sources; a fifth one
// takes the oldest table's place).  Returns the slot, or a negative code.  The caller holds the device guard.
static int copy_table_for(mwb_handle *dst, mwb_handle *src) {
    for (int k = 0; k < 4; k++)
        if (dst->copy_table[k].src == src->serial) return k;
    std::vector<MwbCopyDesc> small, large;
    uint32_t chunks = 0;
    mwb_for_each_copied_array(src->dev, dst->dev, [&](const char *s, char *d, uint32_t rows, uint32_t elem, uint64_t ss, uint64_t ds) {
        MwbCopyDesc t;
        t.src = s; t.dst = d; t.rows = rows; t.elem = elem; t.src_stride = ss; t.dst_stride = ds; t.first_chunk = 0; t.pad = 0;
        if (elem <= MWB_COPY_SMALL_ELEM) { t.first_chunk = chunks; chunks += (rows + MWB_COPY_ROW_CHUNK - 1) / MWB_COPY_ROW_CHUNK; small.push_back(t); }
        else large.push_back(t);
    });
    std::vector<MwbCopyDesc> all(small);
    all.insert(all.end(), large.begin(), large.end());
    if (all.size() > MWB_COPY_TABLE_DESCS) return set_err(MWB_EINVAL, "mwb_copy_envs: descriptor table overflow");
    if (!dst->copy_tables) { int rc = dev_alloc(dst, &dst->copy_tables, (size_t)4 * MWB_COPY_TABLE_DESCS); if (rc) return rc; }
    const int k = dst->copy_table_next;
    dst->copy_table_next = (k + 1) % 4;
    if (dst->copy_table[k].src) HIP_TRY(hipDeviceSynchronize());   // a copy in flight may still be reading the table this one replaces
    dst->copy_table[k].src = 0;
    HIP_TRY(hipMemcpy(dst->copy_tables + (size_t)k * MWB_COPY_TABLE_DESCS, all.data(), all.size() * sizeof(MwbCopyDesc), hipMemcpyHostToDevice));
    dst->copy_table[k].src = src->serial; dst->copy_table[k].n_small = (int)small.size(); dst->copy_table[k].small_chunks = (int)chunks;
    dst->copy_table[k].n_large = (int)large.size();
    return k;
}

extern "C" int mwb_copy_envs(mwb_handle *dst, const int32_t *dst_idx_dev, mwb_handle *src, const int32_t *src_idx_dev, int count,
                             unsigned flags, void *stream) {
    if (!dst || !src) return set_err(MWB_EINVAL, "mwb_copy_envs: null handle");
    if (count < 0) return set_err(MWB_EINVAL, "mwb_copy_envs: count < 0");
    if (count > 0 && (!dst_idx_dev || !src_idx_dev)) return set_err(MWB_EINVAL, "mwb_copy_envs: null index list");
    if (flags & ~(unsigned)MWB_COPY_NO_RENDER) return set_err(MWB_EINVAL, "mwb_copy_envs: unknown flag");
    if (const char *f = config_difference(dst, src))
        return set_err(MWB_EINVAL, std::string("mwb_copy_envs: the handles' configurations differ in `") + f + "`");
    const bool render = !(flags & MWB_COPY_NO_RENDER), same = dst == src;
    // the frame stack (rules in include/miniworld_batch.h): nothing / the window is copied / the list render starts a new history
    bool copy_window = false;
    if (dst->stack) {
        const bool alike = src->stack && src->stack_n == dst->stack_n && src->stack_dtype == dst->stack_dtype && src->stack_cpf == dst->stack_cpf;
        if (alike) copy_window = true;
        else if (!dst->stack_fused) return set_err(MWB_EINVAL, "mwb_copy_envs: the destination's frame stack (not MWB_STACK_FUSED) can only be filled from a source with a stack of equal nstack, dtype and grey flag");
        else if (!render) return set_err(MWB_EINVAL, "mwb_copy_envs: MWB_COPY_NO_RENDER into a fused frame stack needs a source with a stack of equal nstack, dtype and grey flag");
    }
    if (count == 0) return MWB_OK;
    if (!src->have_world) return set_err(MWB_ESTATE, "mwb_copy_envs: the source has never been reset (it holds no worlds)");
    USE_DEVICE(dst->cfg.device);
    int rc;
    if (render) { rc = ensure_ready(dst); if (rc) return rc; }   // MWB_ESTATE without seed / textures / meshes: what mwb_render needs
    hipStream_t s = (hipStream_t)stream;
    MwbDev &d = dst->dev;
    rc = terminal_clear(dst, s); if (rc) return rc;   // a pass on dst that is no step
    if (!dst->copy_dst_pairs) { rc = dev_alloc(dst, &dst->copy_dst_pairs, (size_t)d.N); if (rc) return rc; }
    if (!dst->copy_src_mark) { rc = dev_alloc(dst, &dst->copy_src_mark, (size_t)d.N); if (rc) return rc; }
    if (!dst->copy_rejected) {
        rc = dev_alloc(dst, &dst->copy_rejected, (size_t)1); if (rc) return rc;
        HIP_TRY(hipDeviceSynchronize());   // the scratch is zero before a kernel on the caller's stream counts in it
    }
    if (dst->copy_pairs_cap < (size_t)count) {
        const size_t cap = (size_t)count < (size_t)d.N ? (size_t)d.N : (size_t)count;
        dst->copy_pairs_cap = 0;
        rc = dev_realloc(dst, &dst->copy_pairs, cap); if (rc) return rc;
        HIP_TRY(hipDeviceSynchronize());   // its zeroes are down before a kernel on the caller's stream writes it
        dst->copy_pairs_cap = cap;
    }
    const int slot = copy_table_for(dst, src);
    if (slot < 0) return slot;
    const mwb_handle::CopyTable &tab = dst->copy_table[slot];
    mwb_launch_copy_validate(dst_idx_dev, src_idx_dev, count, d.N, src->dev.N, same ? 1 : 0, dst->copy_dst_pairs, dst->copy_src_mark,
                             dst->copy_pairs, dst->copy_rejected, s);
    rc = check_launch("copy_validate_kernel"); if (rc) return rc;
    mwb_launch_copy_envs(dst->copy_tables + (size_t)slot * MWB_COPY_TABLE_DESCS, tab.n_small, tab.small_chunks, tab.n_large, dst->copy_pairs, count, s);
    rc = check_launch("copy_envs_kernel"); if (rc) return rc;
    mwb_launch_copy_seg_box(d, dst->copy_pairs, count, s);
    rc = check_launch("copy_seg_box_kernel"); if (rc) return rc;
    dst->have_world = true;
    if (dst->levels_on) {   // the level goes with the world: the source's index, or -1 (unknown) where the source has no level sets
        mwb_launch_levels_copy(dst->levels.index, src->levels_on ? src->levels.index : nullptr, dst->copy_pairs, count, s);
        rc = check_launch("levels_copy_kernel"); if (rc) return rc;
    }
    if (render) {   // the destinations through the compact-list path, as mwb_render draws them: the current state, every frame rendered
        d.step_pass = 0; d.reuse_pass = 0;
        dst->timing_now = false;
        mwb_launch_copy_list(d, dst->copy_pairs, count, 0, s);
        rc = check_launch("copy_list_kernel"); if (rc) return rc;
        mwb_launch_prep(d, 1, s);
        rc = check_launch("prep_kernel"); if (rc) return rc;
        mwb_launch_render(d, 1, s);
        rc = check_launch("render_kernel"); if (rc) return rc;
        mwb_launch_copy_list(d, dst->copy_pairs, count, 1, s);
        rc = check_launch("copy_list_kernel"); if (rc) return rc;
    } else {
        mwb_launch_copy_list(d, dst->copy_pairs, count, 2, s);
        rc = check_launch("copy_list_kernel"); if (rc) return rc;
    }
    if (copy_window) {   // after the render: the history the list path has just zeroed is the source's again
        const size_t plane = (size_t)d.W * d.H * (dst->stack_dtype == 1 ? 4 : 1), C = (size_t)dst->stack_n * dst->stack_cpf;
        const size_t kd = dst->stack_planes ? (size_t)dst->stack_planes : C, ks = src->stack_planes ? (size_t)src->stack_planes : C;
        const size_t pd = dst->stack_planes ? (size_t)dst->stack_pos : 0, ps = src->stack_planes ? (size_t)src->stack_pos : 0;
        mwb_launch_copy_stack((char *)dst->stack, kd * plane, pd * plane, (const char *)src->stack, ks * plane, ps * plane, C * plane, dst->copy_pairs, count, s);
        rc = check_launch("copy_stack_kernel"); if (rc) return rc;
    }
    return MWB_OK;
}

extern "C" int mwb_copy_rejected(mwb_handle *dst, unsigned long long *pairs) {
    if (!dst || !pairs) return set_err(MWB_EINVAL, "mwb_copy_rejected: null argument");
    *pairs = 0;
    return dst->copy_rejected ? read_counters(dst, pairs, dst->copy_rejected, 1) : MWB_OK;   // (no copy yet: nothing to read)
}

// bytes of per-env state one accepted pair of a copy from src into dst moves (the descriptor table's total); for measurements
extern "C" long long mwb_copy_env_bytes(mwb_handle *dst, mwb_handle *src) {
    if (!dst || !src) return set_err(MWB_EINVAL, "mwb_copy_env_bytes: null argument");
    if (const char *f = config_difference(dst, src))
        return set_err(MWB_EINVAL, std::string("mwb_copy_env_bytes: the handles' configurations differ in `") + f + "`");
    size_t total = 0;
    mwb_for_each_copied_array(src->dev, dst->dev, [&](const char *, char *, uint32_t rows, uint32_t elem, uint64_t, uint64_t) { total += (size_t)rows * elem; });
    return (long long)total;
}

// -------------------------------------------------------------------------------- introspection
extern "C" int mwb_num_boxes(mwb_handle *h) { return h ? h->dev.n_boxes : 0; }
extern "C" int mwb_room_words(mwb_handle *h) { return h ? h->dev.room_words : 0; }

// mwb_state <-> the device arrays.  The list of fields, the moves between the two layouts and everything mwb_set_state refuses
// are mwb_state_fields.h; this file gives them hipMemcpy.  All four functions are synchronous.
static int dev_move(void *dst, const void *src, size_t bytes, bool to_device) {
    HIP_TRY(hipMemcpy(dst, src, bytes, to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost));
    return MWB_OK;
}
#define STATE_RANGE(first, count) \
    if (first < 0 || count < 0 || first + count > h->dev.N) return set_err(MWB_EINVAL, std::string(__func__) + ": env range out of bounds")
// the stores of the setters, after whatever each of them refuses: the cached frames of the range no longer show its state
// (invalidated first: an error half-way leaves no stale frame trusted).  The caller has synchronised and holds the device guard.
static int put_state(mwb_handle *h, int first, int count, const mwb_state &in) {
    if (int rc = invalidate_frames(h, first, count)) return rc;
    return mwb_state_put(h->dev, first, count, &in, dev_move);
}

extern "C" int mwb_get_state(mwb_handle *h, int first, int count, mwb_state *o) {
    if (!h || !o) return set_err(MWB_EINVAL, "mwb_get_state: null argument");
    STATE_RANGE(first, count);
    USE_DEVICE(h->cfg.device);
    HIP_TRY(hipDeviceSynchronize());
    std::string why;
    const int rc = mwb_state_get(h->dev, first, count, o, dev_move, &why);
    return why.empty() ? rc : set_err(rc, why);
}

extern "C" int mwb_set_state(mwb_handle *h, int first, int count, const mwb_state *in) {
    if (!h || !in) return set_err(MWB_EINVAL, "mwb_set_state: null argument");
    STATE_RANGE(first, count);
    USE_DEVICE(h->cfg.device);
    HIP_TRY(hipDeviceSynchronize());
    std::string why;   // a refused call changes nothing: every check comes before the first store
    if (int rc = mwb_state_check(h->dev, first, count, in, dev_move, &why)) return why.empty() ? rc : set_err(rc, why);
    return put_state(h, first, count, *in);
}

extern "C" int mwb_set_agent(mwb_handle *h, int first, int count, const double *pos_xz, const double *dir, const int32_t *step_count) {
    if (!h) return set_err(MWB_EINVAL, "mwb_set_agent: null handle");
    STATE_RANGE(first, count);
    USE_DEVICE(h->cfg.device);
    HIP_TRY(hipDeviceSynchronize());
    std::vector<double> pos;
    mwb_state st = {};
    if (pos_xz) {
        pos.assign((size_t)count * 3, 0.0);
        for (int i = 0; i < count; i++) { pos[(size_t)i * 3] = pos_xz[i * 2]; pos[(size_t)i * 3 + 2] = pos_xz[i * 2 + 1]; }
        st.agent_pos = pos.data();
    }
    st.agent_dir = const_cast<double *>(dir); st.step_count = const_cast<int32_t *>(step_count);
    return put_state(h, first, count, st);
}

extern "C" int mwb_num_textures(mwb_handle *h) { return h ? h->dev.n_tex : 0; }

/* debugging aid (MWB_DEBUG bit 4 at mwb_create): start / end s_memrealtime ticks (100 MHz) of every workgroup of the last
 * bulk render launch; out: [2 * n] u64, returns n = workgroups or a negative code */
extern "C" int mwb_debug_wg_times(mwb_handle *h, unsigned long long *out, int max_wgs) {
    if (!h || !out) return set_err(MWB_EINVAL, "mwb_debug_wg_times: null argument");
    if (!h->dev.wg_ts) return set_err(MWB_ESTATE, "mwb_debug_wg_times: create the handle with MWB_DEBUG bit 4 set");
    USE_DEVICE(h->cfg.device);
    HIP_TRY(hipDeviceSynchronize());
    int n = h->dev.N + h->dev.split_envs;
    if (n > max_wgs) n = max_wgs;
    HIP_TRY(hipMemcpy(out, h->dev.wg_ts, (size_t)n * 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return n;
}

/* timing experiments (MWB_EXP bit 2 at mwb_create): the entity render kernel's mesh-walk counters since the last call with
 * reset != 0: sample rays entering the walk, walks started, node visits, triangle tests, wave loop iterations, wave calls */
extern "C" int mwb_debug_counters(mwb_handle *h, unsigned long long *out8, int reset) {
    if (!h || !out8) return set_err(MWB_EINVAL, "mwb_debug_counters: null argument");
    if (!h->dev.dbg_counters) return set_err(MWB_ESTATE, "mwb_debug_counters: create the handle with MWB_EXP bit 2 set");
    return read_counters(h, out8, h->dev.dbg_counters, 8, reset != 0);
}

/* frames the step passes (mwb_step / mwb_step_i64) took from the last-frame cache / rendered since the last call */
extern "C" int mwb_frame_reuse_stats(mwb_handle *h, unsigned long long out[2]) {
    if (!h || !out) return set_err(MWB_EINVAL, "mwb_frame_reuse_stats: null argument");
    return read_counters(h, out, h->dev.reuse_stats, 2);
}

/* which kernel a step's bulk render launch of this handle runs now: 0 generic (render_kernel / render_grey_kernel), 1 render_fixed_kernel */
extern "C" int mwb_bulk_variant(mwb_handle *h) {
    if (!h) return 0;
    return h->bulk_fixed && h->overlap_reset && !h->dev.grey ? 1 : 0;
}

extern "C" int mwb_set_domain_rand(mwb_handle *h, int domain_rand) {
    if (!h) return set_err(MWB_EINVAL, "mwb_set_domain_rand: null handle");
    USE_DEVICE(h->cfg.device);
    HIP_TRY(hipDeviceSynchronize());   // kernels in flight took the struct by value; order the change after them
    h->dev.domain_rand = domain_rand ? 1 : 0;
    h->cfg.domain_rand = h->dev.domain_rand;
    return invalidate_frames(h, 0, h->dev.N);
}

extern "C" int mwb_set_task_state(mwb_handle *h, int first, int count, const int64_t *episode_count, const int64_t *task_step_count,
                                  const int32_t *goal_idx) {
    if (!h) return set_err(MWB_EINVAL, "mwb_set_task_state: null handle");
    STATE_RANGE(first, count);
    for (int i = 0; goal_idx && i < count; i++)
        if (goal_idx[i] < 0 || goal_idx[i] > 1) return set_err(MWB_EINVAL, "mwb_set_task_state: goal_idx must be 0 or 1");
    USE_DEVICE(h->cfg.device);
    HIP_TRY(hipDeviceSynchronize());
    mwb_state st = {};
    st.episode_count = const_cast<int64_t *>(episode_count); st.task_step_count = const_cast<int64_t *>(task_step_count);
    st.goal_idx = const_cast<int32_t *>(goal_idx);
    return put_state(h, first, count, st);
}

extern "C" int mwb_intersect(mwb_handle *h, int env, int ent, double x, double z, double radius, int *result) {
    if (!h || !result) return set_err(MWB_EINVAL, "mwb_intersect: null argument");
    if (env < 0 || env >= h->dev.N) return set_err(MWB_EINVAL, "mwb_intersect: env out of range");
    if (ent < -1 || ent > h->dev.n_boxes) return set_err(MWB_EINVAL, "mwb_intersect: ent must be -1 .. number of boxes (= the agent)");
    USE_DEVICE(h->cfg.device);
    mwb_launch_intersect(h->dev, env, ent, x, z, radius, h->scratch_int_dev, 0);
    int rc = check_launch("intersect_kernel"); if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(result, h->scratch_int_dev, sizeof(int), hipMemcpyDeviceToHost));
    return MWB_OK;
}

extern "C" int mwb_get_geometry(mwb_handle *h, int env, float *rooms, int max_rooms, double *segs, int max_segs, int *n_rooms, int *n_segs) {
    if (!h || !n_rooms || !n_segs) return set_err(MWB_EINVAL, "mwb_get_geometry: null argument");
    const MwbDev &d = h->dev;
    if (env < 0 || env >= d.N) return set_err(MWB_EINVAL, "mwb_get_geometry: env out of range");
    USE_DEVICE(h->cfg.device);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(n_rooms, d.n_rrooms + env, sizeof(int), hipMemcpyDeviceToHost));   // the table's records, cut rooms included
    HIP_TRY(hipMemcpy(n_segs, d.n_segs + env, sizeof(int), hipMemcpyDeviceToHost));
    if (rooms) {
        int n = *n_rooms < max_rooms ? *n_rooms : max_rooms;
        if (n > 0) HIP_TRY(hipMemcpy(rooms, d.rooms + (size_t)env * d.R_max * d.room_words, (size_t)n * d.room_words * 4, hipMemcpyDeviceToHost));
    }
    if (segs) {   // device layout is transposed: element (i, c) of env e at segs[(i*4 + c) * N + e]
        int n = *n_segs < max_segs ? *n_segs : max_segs;
        if (n > 0)
            HIP_TRY(hipMemcpy2D(segs, sizeof(double), d.segs + env, (size_t)d.N * sizeof(double), sizeof(double), (size_t)n * 4,
                                hipMemcpyDeviceToHost));
    }
    return MWB_OK;
}

// -------------------------------------------------------------------------------------- timing
extern "C" int mwb_timing_enable(mwb_handle *h, int enable) {
    if (!h) return set_err(MWB_EINVAL, "mwb_timing_enable: null handle");
    USE_DEVICE(h->cfg.device);
    HIP_TRY(hipDeviceSynchronize());
    h->timing = enable != 0;
    h->timing_period = enable > 1 ? enable : 1;
    h->timing_tick = 0;
    h->ev_used = 0;
    if (h->timing && h->ev_pool.empty()) {   // the first block of events is created here, not inside somebody's timed region
        h->ev_pool.resize((size_t)EVN * 256);
        for (size_t i = 0; i < h->ev_pool.size(); i++) HIP_TRY(hipEventCreate(&h->ev_pool[i]));
    }
    return MWB_OK;
}

extern "C" int mwb_timing_read(mwb_handle *h, double *ms_step, double *ms_reset, double *ms_prep, double *ms_render, int *n) {
    if (!h) return set_err(MWB_EINVAL, "mwb_timing_read: null handle");
    USE_DEVICE(h->cfg.device);
    HIP_TRY(hipDeviceSynchronize());
    double acc[4] = {0, 0, 0, 0};
    int passes = (int)(h->ev_used / EVN);
    static const int A_[4] = {0, 5, 2, 3}, B_[4] = {1, 6, 3, 4};   // step, reset (its own stream), prep, render
    for (int p = 0; p < passes; p++)
        for (int i = 0; i < 4; i++) {
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, h->ev_pool[p * EVN + A_[i]], h->ev_pool[p * EVN + B_[i]]));
            acc[i] += ms;
        }
    int cnt = passes > 0 ? passes : 1;
    if (ms_step) *ms_step = acc[0] / cnt;
    if (ms_reset) *ms_reset = acc[1] / cnt;
    if (ms_prep) *ms_prep = acc[2] / cnt;
    if (ms_render) *ms_render = acc[3] / cnt;
    if (n) *n = passes;
    h->ev_used = 0;
    return MWB_OK;
}
