// Host program around gym_miniworld_amd/csrc/mwb_monitor_map.h (tests/test_monitor_host.py): plays the log of the episode monitor
// as the kernels do - a ring of `capacity` records and the counter `total` - with episode ids in place of records.
//
// stdin:  lines of "total capacity c": a log that has seen `total` episodes (ids 0 .. total - 1, appended one per pass) takes a
//         pass that finishes c episodes (ids total .. total + c - 1, rank r = id - total)
// stdout: per line   W r:slot ...        the ranks of that pass that are written, with their slots
//                    R id ...            the ring read oldest first after the pass
// exit 3: two written ranks of one pass shared a slot, or a slot was outside the ring
#include <stdio.h>

#include <vector>

#include "mwb_monitor_map.h"

static int pass(std::vector<long long> &ring, unsigned long long &total, uint32_t c, uint32_t capacity, bool print) {
    std::vector<char> hit(capacity, 0);
    if (print) printf("W");
    for (uint32_t r = 0; r < c; r++) {
        if (!mwb_monitor_written(r, c, capacity)) continue;
        const uint32_t slot = mwb_monitor_slot(total, r, capacity);
        if (slot >= capacity || hit[slot]) return 3;
        if (slot != mwb_monitor_slot_from(mwb_monitor_base(total, capacity), r, capacity)) return 3;
        hit[slot] = 1;
        ring[slot] = (long long)(total + r);
        if (print) printf(" %u:%u", r, slot);
    }
    if (print) printf("\n");
    total += c;
    return 0;
}

int main() {
    unsigned long long total0;
    uint32_t capacity, c;
    while (scanf("%llu %u %u", &total0, &capacity, &c) == 3) {
        if (capacity < 1 || capacity > MWB_MONITOR_MAX_CAPACITY) return 2;
        std::vector<long long> ring(capacity, -1);
        unsigned long long total = 0;
        while (total < total0)
            if (int rc = pass(ring, total, 1, capacity, false)) return rc;
        if (int rc = pass(ring, total, c, capacity, true)) return rc;
        printf("R");
        const uint32_t live = mwb_monitor_live(total, capacity);
        for (uint32_t i = 0; i < live; i++) printf(" %lld", ring[mwb_monitor_read_slot(total, i, capacity)]);
        printf("\n");
    }
    return 0;
}
