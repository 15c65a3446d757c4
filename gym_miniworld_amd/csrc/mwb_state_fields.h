// mwb_state_fields.h - the fields of mwb_state (include/miniworld_batch.h), each written down ONCE: mwb_get_state, mwb_set_state
// and its validation walk this list, as mwb_create and mwb_copy_envs walk the per-env array list of mwb_internal.h.  A new field
// that is a plain move is one new line here (and one in _lib.STATE_FIELDS, which tests/test_state_fields_host.py holds against
// this list).  Plain C++ over a `move` the caller supplies - int move(void *dst, const void *src, size_t bytes, bool to_device),
// 0 or a negative code: hipMemcpy in mwb_api.hip, memcpy over host arrays in tests/state_fields_host.cpp, where all of this runs
// without a device.
//
// Shapes.  mwb_state is env-major: [count][w] per env, [count][B][w] per box / entity slot.  The device arrays are [N][w] per
// env and [B][N][w] planes per slot (mwb_internal.h), so a slot field moves plane by plane.
#pragma once
#include <math.h>
#include <stddef.h>
#include <string.h>

#include <string>
#include <type_traits>
#include <vector>

#include "mwb_internal.h"

#define MWB_SF_BOX 1u        // per slot: [B][N][w] planes on the device, [count][B][w] in mwb_state (otherwise per env, [N][w])
#define MWB_SF_WRITE 2u      // mwb_set_state stores it (otherwise it is ignored there - or refused, if it is entity-only)
#define MWB_SF_ENT 4u        // exists for the entity-list tasks only
#define MWB_SF_FINITE 8u     // mwb_set_state refuses NaN / inf: the value goes straight into the step and render kernels
#define MWB_SF_POSITIVE 16u  // ... and values <= 0
#define MWB_SF_CODE 32u      // not a plain move: the explicit code below the list

struct MwbStateField {
    const char *name;
    size_t offset;   // of the pointer in mwb_state
    size_t width;    // elements per env, or per slot of an env
    unsigned flags;
};

// f(st.field, the MwbDev array behind it, MwbStateField) for every field, in the order of the struct.  st: mwb_state or const
// mwb_state.  An MWB_SF_CODE field hands f a null pointer of the field's type in place of an array: agent_pos is agent_x and
// agent_z (y = 0), box_pos is box_x, box_y and box_z, ent_order is ent_order and n_order, rng_pos and rng_keysum come from rng.
template <class State, class F>
static inline void mwb_for_each_state_field(State &st, const MwbDev &d, F &&f) {
#define MWB_FIELD(name, member, width, flags) f(st.name, d.member, MwbStateField{#name, offsetof(mwb_state, name), (size_t)(width), (unsigned)(flags)})
#define MWB_FIELD_CODE(name, width, flags) \
    f(st.name, (decltype(st.name))nullptr, MwbStateField{#name, offsetof(mwb_state, name), (size_t)(width), (unsigned)(flags) | MWB_SF_CODE})
    const unsigned BOX = MWB_SF_BOX, W = MWB_SF_WRITE, ENT = MWB_SF_ENT, FIN = MWB_SF_FINITE, POS = MWB_SF_POSITIVE, RO = 0;
    MWB_FIELD_CODE(agent_pos, 3, W | FIN);
    MWB_FIELD(agent_dir, agent_dir, 1, W | FIN);
    MWB_FIELD_CODE(box_pos, 3, BOX | W | FIN);
    MWB_FIELD(box_dir, box_dir, 1, BOX | W | FIN);
    MWB_FIELD(box_color, box_color, 3, BOX | W | FIN);
    MWB_FIELD(box_size, box_size, 1, BOX | W | FIN | POS);
    MWB_FIELD(cam, cam, 4, W | FIN);
    MWB_FIELD(sky_color, sky_color, 3, W | FIN);
    MWB_FIELD(light_pos, light_pos, 3, W | FIN);
    MWB_FIELD(light_color, light_color, 3, W | FIN);
    MWB_FIELD(light_ambient, light_ambient, 3, W | FIN);
    MWB_FIELD(step_count, step_count, 1, W);
    MWB_FIELD_CODE(rng_pos, 1, RO);
    MWB_FIELD_CODE(rng_keysum, 1, RO);
    MWB_FIELD(n_rooms, n_rooms, 1, RO);
    MWB_FIELD(n_segs, n_segs, 1, RO);
    MWB_FIELD(goal_idx, goal_idx, 1, W);                 // 0 or 1
    MWB_FIELD(episode_count, episode_count, 1, W);
    MWB_FIELD(task_step_count, task_step_count, 1, W);
    MWB_FIELD(goal_dist, goal_dist, 1, W | FIN);
    MWB_FIELD(rng_state, rng, MWB_MT_WORDS, W);          // the position (word 624) must lie in 0 .. 624
    MWB_FIELD(carrying, carrying, 1, W);                 // -1 or a box index
    MWB_FIELD(ent_meta, ent_meta, 1, BOX | ENT | W);     // only the alive bit may differ from what is there
    MWB_FIELD(ent_radius, ent_radius, 1, BOX | ENT | RO);
    MWB_FIELD(ent_height, ent_height, 1, BOX | ENT | RO);
    MWB_FIELD(ent_scale, ent_scale, 1, BOX | ENT | RO);
    MWB_FIELD_CODE(ent_order, d.n_boxes + 1, ENT | W);
    MWB_FIELD(task_f, task_f, 1, ENT | W);
    MWB_FIELD(task_i, task_i, 1, ENT | W);
    MWB_FIELD(text_tex, text_tex, 8, ENT | RO);
#undef MWB_FIELD
#undef MWB_FIELD_CODE
}

// envs first .. first + count of a device array -> rows of mwb_state, and back; B = 1: a per-env array
template <class T, class Move>
static inline int mwb_state_fetch(T *host, const T *dev, size_t N, size_t B, size_t first, size_t count, size_t w, Move &move) {
    if (!host) return 0;
    if (B == 1) return move(host, dev + first * w, count * w * sizeof(T), false);
    std::vector<T> plane(count * w);
    for (size_t b = 0; b < B; b++) {
        if (int rc = move(plane.data(), dev + (b * N + first) * w, plane.size() * sizeof(T), false)) return rc;
        for (size_t i = 0; i < count; i++)
            for (size_t k = 0; k < w; k++) host[(i * B + b) * w + k] = plane[i * w + k];
    }
    return 0;
}
template <class T, class Move>
static inline int mwb_state_store(const T *host, T *dev, size_t N, size_t B, size_t first, size_t count, size_t w, Move &move) {
    if (!host) return 0;
    if (B == 1) return move(dev + first * w, host, count * w * sizeof(T), true);
    std::vector<T> plane(count * w);
    for (size_t b = 0; b < B; b++) {
        for (size_t i = 0; i < count; i++)
            for (size_t k = 0; k < w; k++) plane[i * w + k] = host[(i * B + b) * w + k];
        if (int rc = move(dev + (b * N + first) * w, plane.data(), plane.size() * sizeof(T), true)) return rc;
    }
    return 0;
}

// mwb_state.ent_order rows (slots, -2 = the agent, -1 = end) -> the device's bytes and lengths; `ord` comes filled with
// MWB_ENT_AGENT.  Returns null, or why a row is refused.
static inline const char *mwb_state_pack_order(const int32_t *order, size_t count, int B, uint8_t *ord, int32_t *no) {
    for (size_t i = 0; i < count; i++) {
        int n = 0;
        uint32_t seen = 0;
        for (int k = 0; k <= B; k++) {
            const int v = order[i * (B + 1) + k];
            if (v == -1) break;
            if (v != -2 && (v < 0 || v >= B)) return "mwb_set_state: ent_order entries are slots, -2 (the agent) or -1 (end)";
            const uint32_t bit = 1u << (v == -2 ? 31 : v);
            if (seen & bit) return "mwb_set_state: ent_order lists an entity twice";
            seen |= bit;
            ord[i * MWB_ORDER_STRIDE + n++] = (uint8_t)(v == -2 ? MWB_ENT_AGENT : v);
        }
        no[i] = n;
    }
    return nullptr;
}

template <class Move>
static inline int mwb_state_get(const MwbDev &d, int first_env, int n_envs, mwb_state *o, Move &&move, std::string *err) {
    const size_t N = (size_t)d.N, B = (size_t)d.n_boxes, first = (size_t)first_env, count = (size_t)n_envs;
    bool ent = false;
    mwb_for_each_state_field(*o, d, [&](auto *host, auto *, const MwbStateField &f) { ent = ent || (host && (f.flags & MWB_SF_ENT)); });
    if (ent && !d.ent_task) { *err = "mwb_get_state: entity-list fields exist for the tasks >= MWB_TASK_PICKUPOBJS only"; return MWB_EINVAL; }
    int rc = 0;
    mwb_for_each_state_field(*o, d, [&](auto *host, auto *dev, const MwbStateField &f) {
        if (!rc && !(f.flags & MWB_SF_CODE)) rc = mwb_state_fetch(host, dev, N, (f.flags & MWB_SF_BOX) ? B : 1, first, count, f.width, move);
    });
    if (rc) return rc;
    if (o->agent_pos) {
        std::vector<double> x(count), z(count);
        if ((rc = mwb_state_fetch(x.data(), d.agent_x, N, 1, first, count, 1, move))) return rc;
        if ((rc = mwb_state_fetch(z.data(), d.agent_z, N, 1, first, count, 1, move))) return rc;
        for (size_t i = 0; i < count; i++) { o->agent_pos[i * 3] = x[i]; o->agent_pos[i * 3 + 1] = 0.0; o->agent_pos[i * 3 + 2] = z[i]; }
    }
    if (o->box_pos) {
        const double *const planes[3] = {d.box_x, d.box_y, d.box_z};
        std::vector<double> p(count * B);
        for (int c = 0; c < 3; c++) {
            if ((rc = mwb_state_fetch(p.data(), planes[c], N, B, first, count, 1, move))) return rc;
            for (size_t i = 0; i < count * B; i++) o->box_pos[i * 3 + c] = p[i];
        }
    }
    if (o->ent_order) {
        std::vector<uint8_t> ord(count * MWB_ORDER_STRIDE);
        std::vector<int32_t> no(count);
        if ((rc = mwb_state_fetch(ord.data(), d.ent_order, N, 1, first, count, MWB_ORDER_STRIDE, move))) return rc;
        if ((rc = mwb_state_fetch(no.data(), d.n_order, N, 1, first, count, 1, move))) return rc;
        for (size_t i = 0; i < count; i++)
            for (size_t k = 0; k <= B; k++) {
                const int v = ord[i * MWB_ORDER_STRIDE + k];
                o->ent_order[i * (B + 1) + k] = (int)k >= no[i] ? -1 : (v == MWB_ENT_AGENT ? -2 : v);
            }
    }
    if (o->rng_pos || o->rng_keysum) {
        std::vector<uint32_t> st(count * MWB_MT_WORDS);
        if ((rc = mwb_state_fetch(st.data(), d.rng, N, 1, first, count, MWB_MT_WORDS, move))) return rc;
        for (size_t i = 0; i < count; i++) {
            uint64_t sum = 0;
            for (int k = 0; k < 624; k++) sum += st[i * MWB_MT_WORDS + k];
            if (o->rng_keysum) o->rng_keysum[i] = (uint32_t)(sum & 0xFFFFFFFFu);
            if (o->rng_pos) o->rng_pos[i] = (int32_t)st[i * MWB_MT_WORDS + 624];
        }
    }
    return 0;
}

// Everything mwb_set_state refuses, before anything is changed; reads ent_meta through `move` for the alive-bit rule.
template <class Move>
static inline int mwb_state_check(const MwbDev &d, int first_env, int n_envs, const mwb_state *in, Move &&move, std::string *err) {
    const size_t N = (size_t)d.N, B = (size_t)d.n_boxes, first = (size_t)first_env, count = (size_t)n_envs;
    auto refuse = [&](const std::string &why) { *err = why; return MWB_EINVAL; };
    for (size_t i = 0; in->goal_idx && i < count; i++)
        if (in->goal_idx[i] < 0 || in->goal_idx[i] > 1) return refuse("mwb_set_state: goal_idx must be 0 or 1");
    for (size_t i = 0; in->carrying && i < count; i++)
        if (in->carrying[i] < -1 || in->carrying[i] >= d.n_boxes) return refuse("mwb_set_state: carrying must be -1 or a box index");
    for (size_t i = 0; in->rng_state && i < count; i++)
        if (in->rng_state[i * MWB_MT_WORDS + 624] > 624u) return refuse("mwb_set_state: MT19937 position must be 0..624");
    bool finite = true, ent = false, read_only = false;
    const char *not_positive = nullptr;
    mwb_for_each_state_field(*in, d, [&](auto *host, auto *, const MwbStateField &f) {
        if (!host) return;
        ent = ent || (f.flags & MWB_SF_ENT);
        read_only = read_only || ((f.flags & MWB_SF_ENT) && !(f.flags & MWB_SF_WRITE));
        if constexpr (std::is_same_v<decltype(host), double *>) {
            const size_t n = (f.flags & (MWB_SF_FINITE | MWB_SF_POSITIVE)) ? count * ((f.flags & MWB_SF_BOX) ? B : 1) * f.width : 0;
            for (size_t i = 0; i < n; i++) {
                if ((f.flags & MWB_SF_FINITE) && !std::isfinite(host[i])) finite = false;
                if ((f.flags & MWB_SF_POSITIVE) && !(host[i] > 0) && !not_positive) not_positive = f.name;
            }
        }
    });
    if (!finite) return refuse("mwb_set_state: non-finite value");
    if (not_positive) return refuse(std::string("mwb_set_state: ") + not_positive + " must be > 0");
    if (ent && !d.ent_task) return refuse("mwb_set_state: entity-list fields exist for the tasks >= MWB_TASK_PICKUPOBJS only");
    if (read_only) return refuse("mwb_set_state: ent_radius / ent_height / ent_scale / text_tex are read-only");
    if (in->ent_meta) {   // only the `alive` bit may differ (an entity PickupObjs removed): kinds and dimensions belong to the episode
        std::vector<int32_t> now(count * B);
        if (int rc = mwb_state_fetch(now.data(), d.ent_meta, N, B, first, count, 1, move)) return rc;
        for (size_t i = 0; i < count * B; i++)
            if ((in->ent_meta[i] & ~(1 << 9)) != (now[i] & ~(1 << 9))) return refuse("mwb_set_state: ent_meta may only change an entity's alive bit");
    }
    if (in->ent_order) {
        std::vector<uint8_t> ord(count * MWB_ORDER_STRIDE);
        std::vector<int32_t> no(count);
        if (const char *why = mwb_state_pack_order(in->ent_order, count, d.n_boxes, ord.data(), no.data())) return refuse(why);
    }
    return 0;
}

// The stores of every writable field given; nothing is checked here (mwb_state_check has, where the caller promises a check).
template <class Move>
static inline int mwb_state_put(const MwbDev &d, int first_env, int n_envs, const mwb_state *in, Move &&move) {
    const size_t N = (size_t)d.N, B = (size_t)d.n_boxes, first = (size_t)first_env, count = (size_t)n_envs;
    int rc = 0;
    if (in->agent_pos) {
        std::vector<double> x(count), z(count);
        for (size_t i = 0; i < count; i++) { x[i] = in->agent_pos[i * 3]; z[i] = in->agent_pos[i * 3 + 2]; }
        if ((rc = mwb_state_store(x.data(), d.agent_x, N, 1, first, count, 1, move))) return rc;
        if ((rc = mwb_state_store(z.data(), d.agent_z, N, 1, first, count, 1, move))) return rc;
    }
    if (in->box_pos) {
        double *const planes[3] = {d.box_x, d.box_y, d.box_z};
        std::vector<double> p(count * B);
        for (int c = 0; c < 3; c++) {
            for (size_t i = 0; i < count * B; i++) p[i] = in->box_pos[i * 3 + c];
            if ((rc = mwb_state_store(p.data(), planes[c], N, B, first, count, 1, move))) return rc;
        }
    }
    if (in->ent_order) {
        std::vector<uint8_t> ord(count * MWB_ORDER_STRIDE, (uint8_t)MWB_ENT_AGENT);
        std::vector<int32_t> no(count);
        (void)mwb_state_pack_order(in->ent_order, count, d.n_boxes, ord.data(), no.data());
        if ((rc = mwb_state_store(ord.data(), d.ent_order, N, 1, first, count, MWB_ORDER_STRIDE, move))) return rc;
        if ((rc = mwb_state_store(no.data(), d.n_order, N, 1, first, count, 1, move))) return rc;
    }
    mwb_for_each_state_field(*in, d, [&](auto *host, auto *dev, const MwbStateField &f) {
        if (!rc && (f.flags & MWB_SF_WRITE) && !(f.flags & MWB_SF_CODE))
            rc = mwb_state_store(host, dev, N, (f.flags & MWB_SF_BOX) ? B : 1, first, count, f.width, move);
    });
    return rc;
}
