// mwb_monitor_map.h - where an episode record of the monitor's log lives: the ring arithmetic of mwb_monitor_update and of
// reading the log back oldest first.
//
// Plain C++ without any HIP type, so that the same functions run in the kernels (mwb_monitor.hip), in the host API and in a host
// program (tests/test_monitor_host.py builds one around this header).
//
// The reference is the trainer's `episode_rewards = deque(maxlen=100)` with its loop over the envs after every step
// (pytorch-a2c-ppo-acktr/main.py:141,167-169): episodes are appended pass by pass and, inside a pass, in increasing env index.
// The log is a ring of `capacity` records and one counter, `total` = episodes ever appended:
//
//   a pass finishes c loggable episodes, ranks 0 .. c - 1        rank = loggable finishing envs with a smaller index
//   rank r goes to                                               slot (total + r) mod capacity
//   ... if it is one of the last `capacity` of the pass          r >= c - capacity (a deque(maxlen) keeps the last ones; the ranks
//                                                                that are written are at most `capacity` consecutive numbers, so
//                                                                no two of them share a slot: no race)
//   after the pass                                               total += c, whatever was written
//   the log holds                                                min(total, capacity) records, the oldest in slot
//                                                                total mod capacity once the ring is full, in slot 0 before
//
// capacity <= 65536 (mwb_monitor_enable) and ranks are env counts (< 2^31): base + rank fits 32 bits.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MWB_MONITOR_HD __host__ __device__
#else
#define MWB_MONITOR_HD
#endif

#define MWB_MONITOR_MAX_CAPACITY 65536
#define MWB_MONITOR_MAX_QUOTA 64

// slot of rank 0 of a pass that starts with `total` episodes appended (the one 64-bit division: once per pass, not per env)
MWB_MONITOR_HD static inline uint32_t mwb_monitor_base(uint64_t total, uint32_t capacity) { return (uint32_t)(total % capacity); }

// slot of rank `rank` of that pass, from its base
MWB_MONITOR_HD static inline uint32_t mwb_monitor_slot_from(uint32_t base, uint32_t rank, uint32_t capacity) { return (base + rank) % capacity; }

MWB_MONITOR_HD static inline uint32_t mwb_monitor_slot(uint64_t total, uint32_t rank, uint32_t capacity) {
    return mwb_monitor_slot_from(mwb_monitor_base(total, capacity), rank, capacity);
}

// is rank `rank` of a pass with c loggable episodes written at all
MWB_MONITOR_HD static inline int mwb_monitor_written(uint32_t rank, uint32_t c, uint32_t capacity) { return c <= capacity || rank >= c - capacity; }

// reading back: how many records are live, and the slot of the i-th oldest of them (i = 0 .. live - 1)
MWB_MONITOR_HD static inline uint32_t mwb_monitor_live(uint64_t total, uint32_t capacity) { return total < capacity ? (uint32_t)total : capacity; }
MWB_MONITOR_HD static inline uint32_t mwb_monitor_oldest(uint64_t total, uint32_t capacity) { return total < capacity ? 0u : mwb_monitor_base(total, capacity); }
MWB_MONITOR_HD static inline uint32_t mwb_monitor_read_slot(uint64_t total, uint32_t i, uint32_t capacity) {
    return mwb_monitor_slot_from(mwb_monitor_oldest(total, capacity), i, capacity);
}
