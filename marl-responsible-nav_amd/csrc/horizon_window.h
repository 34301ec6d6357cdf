// horizon_window.h -- internal: what the kernels that fold levels of one agent's cells share (step_horizon.hip,
// step_plan.hip): the window of slots around the agent's present cell, the sizes of the node levels, a level's
// depths read by a transition code, and the ranking of a level's occupied slots into its ascending node list.
// Included inside namespace gw, after cf_env.h and step_horizon.h.
#pragma once

// k's cells are kept as slots of one square window around its present cell (r0, c0): slot (dr + R) * SIDE + dc + R.
// After h steps k is within Manhattan distance 2 h; nodes exist for the levels 1..H - 1 <= HZ_LEVELS.
constexpr int HZ_LEVELS = GW_HORIZON_MAX - 1;
constexpr int HZ_R = 2 * HZ_LEVELS, HZ_SIDE = 2 * HZ_R + 1, HZ_SLOTS = HZ_SIDE * HZ_SIDE;
constexpr int HZ_WORDS = (HZ_SLOTS + 31) / 32;
constexpr uint32_t HZ_NONE = 0xFFFFFFFFu;
// level h holds at most the 9 cells of one action (h = 1), else the 2 r^2 + 2 r + 1 cells within r = 2 h
__host__ __device__ constexpr int hz_cap(int h) { return h <= 1 ? 9 : 8 * h * h + 4 * h + 1; }
__host__ __device__ constexpr int hz_off(int h) {  // the first node of level h in the compact arrays
    int o = 0;
    for (int q = 1; q < h; ++q) o += hz_cap(q);
    return o;
}
constexpr int HZ_NODES = hz_off(HZ_LEVELS + 1);  // 9 + 41 + 85
static_assert(GW_HORIZON_MAX == step_horizon::HORIZON_MAX, "step_horizon.h restates GW_HORIZON_MAX");
static_assert(HZ_SLOTS < (int)step_horizon::END, "a window slot is a transition code below END");
static_assert(hz_cap(HZ_LEVELS) <= HZ_SLOTS && HZ_NODES == 135, "node levels of H <= 4");

template <int N>
struct HzWindow {
    int r0, c0, H, W;
    uint32_t w_magic;
    __device__ __forceinline__ int slot_of(int cell) const {
        const int r = (int)__umulhi((uint32_t)cell, w_magic), cc = cell - r * W;
        const int dr = min(max(r - r0, -HZ_R), HZ_R), dc = min(max(cc - c0, -HZ_R), HZ_R);
        return (dr + HZ_R) * HZ_SIDE + dc + HZ_R;  // in 0..HZ_SLOTS-1
    }
    __device__ __forceinline__ int cell_of(int slot) const {  // slot in 0..HZ_SLOTS-1; the cell clamped to the grid
        const int dr = slot / HZ_SIDE - HZ_R, dc = slot - (slot / HZ_SIDE) * HZ_SIDE - HZ_R;
        return min(max(r0 + dr, 0), H - 1) * W + min(max(c0 + dc, 0), W - 1);
    }
};

// A level's depths as step_horizon's functions read them: indexed by a transition code, clamped to the window
struct HzDepths {
    const uint8_t *d;
    __device__ __forceinline__ uint32_t operator[](uint32_t slot) const { return d[min(slot, (uint32_t)HZ_SLOTS - 1u)]; }
};

// The node list of a level: the set slots of `words`, ascending, into nodes[0..cap-1]; returns their number (at most
// cap).  A lane ranks its slots by population counts of the words: nothing wave-collective.
__device__ __forceinline__ int hz_list_nodes(const uint32_t (&words)[HZ_WORDS], int lane, int cap, uint8_t *nodes) {
    int nn = 0;
#pragma unroll
    for (int q = 0; q < HZ_WORDS; ++q) nn += __popc(words[q]);
    nn = min(nn, cap);
    for (int sl = lane; sl < HZ_SLOTS; sl += 64) {
        const int wq = sl >> 5;
        int rank = 0;
        bool set = false;
#pragma unroll
        for (int q = 0; q < HZ_WORDS; ++q) {
            const uint32_t below = (q < wq) ? words[q] : (q == wq) ? (words[q] & ((1u << (sl & 31)) - 1u)) : 0u;
            rank += __popc(below);
            set |= (q == wq) && ((words[q] >> (sl & 31)) & 1u);
        }
        if (set && rank < cap) nodes[rank] = (uint8_t)sl;
    }
    return nn;
}
