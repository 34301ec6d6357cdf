// obs_dest.h — internal, host only (no HIP): the env's table of obs destinations the delta writer
// may patch in place (gridenv.hip; include/gridenv.h gw_set_obs_delta).  A valid slot says "the env
// last wrote this buffer, in this dtype, and the slot's saved descriptors describe what it holds";
// the table only keeps the bookkeeping: which slot a pointer owns, least-recently-used eviction,
// forgetting.  The device copy of the descriptors and the last writer's event of slot i live in the
// env, indexed by the slot number (they are reused by whichever destination takes the slot next).
#pragma once
#include <cstdint>

namespace gwdest {

constexpr int SLOTS = 8;  // a 5-slot replay ring plus spares

struct Table {
    struct Slot {
        const void *ptr = nullptr;
        int dtype = 0;
        bool valid = false;
        uint64_t used = 0;  // clock of the last find / claim (least recently used = smallest)
    };
    Slot slot[SLOTS];
    uint64_t clock = 0;

    // the valid slot of (ptr, dtype), marked used now; -1: unknown (never written, forgotten,
    // evicted, or written in the other dtype)
    int find(const void *ptr, int dtype) {
        for (int i = 0; i < SLOTS; ++i)
            if (slot[i].valid && slot[i].ptr == ptr && slot[i].dtype == dtype) {
                slot[i].used = ++clock;
                return i;
            }
        return -1;
    }

    // the slot a full write of (ptr, dtype) fills: the one ptr already owns (a stale dtype is
    // replaced), else a free one, else the least recently used (evicting = forgetting)
    int claim(const void *ptr, int dtype) {
        int pick = -1;
        for (int i = 0; i < SLOTS && pick < 0; ++i)
            if (slot[i].valid && slot[i].ptr == ptr) pick = i;
        for (int i = 0; i < SLOTS && pick < 0; ++i)
            if (!slot[i].valid) pick = i;
        if (pick < 0) {
            pick = 0;
            for (int i = 1; i < SLOTS; ++i)
                if (slot[i].used < slot[pick].used) pick = i;
        }
        slot[pick].ptr = ptr;
        slot[pick].dtype = dtype;
        slot[pick].valid = true;
        slot[pick].used = ++clock;
        return pick;
    }

    // drop ptr's slot (null: every slot); returns how many were dropped
    int forget(const void *ptr) {
        int n = 0;
        for (int i = 0; i < SLOTS; ++i)
            if (slot[i].valid && (!ptr || slot[i].ptr == ptr)) {
                slot[i].valid = false;
                ++n;
            }
        return n;
    }

    int count() const {
        int n = 0;
        for (int i = 0; i < SLOTS; ++i) n += slot[i].valid ? 1 : 0;
        return n;
    }
};

}  // namespace gwdest
