// tpl_mirror.h -- the left-right reflection of a state and of an action (include/tpl_learn.h states the rule), as the device
// functions that the samplers' mirrored form (tpl_replay_draw.h) and tpl_mirror_states share.
//
// The game is symmetric under it: the reflected board, with L <-> J and S <-> Z in the piece list and the reflected action,
// gives the reflected board with the same lines cleared, reward and ending.  In the column layout the board's reflection is a
// renaming of ten registers, the piece window's a 36-bit SWAR remap, and the action needs the width of one table entry, which
// comes out of a 64-bit literal (32 widths, two bits each) instead of a dependent load of the shape table.
//
// Every function takes `flip` and applies it with selects: a wave whose lanes disagree runs one straight-line path.
//
// The packed widths and rotation masks below, and what they say about a piece's distinct placements (right_most ..
// next_placement), also serve the placement family (tpl_placement.h).
#pragma once

#include "../tpl_device.h"

namespace tpl_learn {

// (width - 1) of shape table entry k = piece * 4 + (rotations & 3) at bits 2k, 2k + 1; entries 28..31 (piece id 7, "none")
// are the table's own (O's)
constexpr uint64_t packed_widths() {
    uint64_t v = 0;
    for (int k = 0; k < 32; ++k) v |= (uint64_t)(((tpl::kShapeTableHost[k].x >> 16) & 7u) - 1u) << (2 * k);
    return v;
}
constexpr uint64_t kWidthsLess1 = packed_widths();

// rotations % len of get_tetromino as r & (len - 1): len - 1 of piece p at bits 2p, 2p + 1 (len = [2, 4, 4, 4, 2, 2, 1, 1])
constexpr int kRotations[8] = TPL_PIECE_ROTATIONS;
constexpr uint32_t packed_rotation_masks() {
    uint32_t v = 0;
    for (int p = 0; p < 8; ++p) v |= (uint32_t)(kRotations[p] - 1) << (2 * p);
    return v;
}
constexpr uint32_t kRotationMasks = packed_rotation_masks();

// the shape table holds entry [p][r % len] at [p][r] for every r: the canonical rotation names the same entry
constexpr bool table_repeats_with_the_rotation_count() {
    for (int p = 0; p < 8; ++p)
        for (int r = 0; r < 4; ++r) {
            const tpl::ShapeWord a = tpl::kShapeTableHost[p * 4 + r], b = tpl::kShapeTableHost[p * 4 + (r & (kRotations[p] - 1))];
            if (a.x != b.x || a.y != b.y) return false;
        }
    return true;
}
static_assert(table_repeats_with_the_rotation_count(), "kRotations does not match the shape table");

// The distinct placements of piece `cur`: rotations r = 0 .. last_rotation(cur), locations l = 0 .. right_most(cur, r).  These
// are the only readers of the two literals.
__host__ __device__ constexpr uint32_t width_less1(uint32_t cur, uint32_t r) {                 // w - 1 of entry [cur][r]
    return (uint32_t)(kWidthsLess1 >> (2u * (cur * 4u + r))) & 3u;
}
__host__ __device__ constexpr uint32_t right_most(uint32_t cur, uint32_t r) { return 9u - width_less1(cur, r); }        // 10 - w
__host__ __device__ constexpr uint32_t location_count(uint32_t cur, uint32_t r) { return 10u - width_less1(cur, r); }   // 11 - w
__host__ __device__ constexpr uint32_t last_rotation(uint32_t cur) { return (kRotationMasks >> (2u * cur)) & 3u; }      // nrot - 1

__host__ __device__ constexpr uint32_t placement_count(uint32_t cur) {
    uint32_t total = 0u;
#pragma unroll
    for (uint32_t r = 0; r < 4u; ++r) total += r <= last_rotation(cur) ? location_count(cur, r) : 0u;
    return total;
}

// one step of the walk over them in ascending 10 r + l, from (0, 0) until r > last_rotation(cur); selects, no branch
__host__ __device__ constexpr void next_placement(uint32_t cur, uint32_t& r, uint32_t& l) {
    const bool wrap = l >= right_most(cur, r);
    l = wrap ? 0u : l + 1u;
    r += wrap ? 1u : 0u;
}

constexpr bool placement_counts_are(const uint32_t (&want)[8]) {
    for (uint32_t p = 0; p < 8u; ++p)
        if (placement_count(p) != want[p]) return false;
    return true;
}
static_assert(placement_counts_are({17, 34, 34, 34, 17, 17, 9, 9}), "the counts include/tpl_learn.h states");

// a' = 10 ((4 - r) & 3) + (10 - w - min(l, 10 - w)) for a = 10 r' + l, r = r' & 3, w the width of entry [cur][r]; below 40
__device__ __forceinline__ uint32_t mirror_action(uint32_t a, uint32_t cur, bool flip) {
    const uint32_t q = a / 10u, l = a - 10u * q, r = q & 3u;
    const uint32_t right = right_most(cur, r);
    const uint32_t m = 10u * ((4u - r) & 3u) + (right - min(l, right));
    return flip ? m : a;
}

// pi = [0, 2, 1, 3, 5, 4, 6, 7] on each of the twelve 3-bit entries of a 36-bit window: with an entry's bits b2 b1 b0,
// 1 <-> 2 flips b1 and b0 where b2 = 0 and b1 != b0, 4 <-> 5 flips b0 where b2 = 1 and b1 = 0
__device__ __forceinline__ uint64_t mirror_window(uint64_t w) {
    constexpr uint64_t kLow = 0x249249249ull;                    // bit 0 of every entry
    const uint64_t b0 = w & kLow, b1 = (w >> 1) & kLow, b2 = (w >> 2) & kLow;
    const uint64_t f1 = (b0 ^ b1) & ~b2;
    const uint64_t f0 = f1 | (b2 & ~b1);
    return w ^ (f0 | (f1 << 1));
}

// column x <-> column 9 - x, every window entry through pi; the counters, the state and the slot stay
__device__ __forceinline__ void mirror_board(tpl::Board& s, bool flip) {
#pragma unroll
    for (int x = 0; x < tpl::kCols / 2; ++x) {                   // constant indices: the ten words stay in registers
        const uint32_t lo = s.c[x], hi = s.c[tpl::kCols - 1 - x];
        s.c[x] = flip ? hi : lo;
        s.c[tpl::kCols - 1 - x] = flip ? lo : hi;
    }
    const uint64_t w = (uint64_t)s.window | ((uint64_t)s.window_hi << 32);
    const uint64_t m = mirror_window(w);
    s.window = flip ? (uint32_t)m : s.window;
    s.window_hi = flip ? (uint32_t)(m >> 32) : s.window_hi;
}

// the same on the 32-byte state: an involution on all 256 bits (bit 31 of B.y, which no field uses, is carried over)
__device__ __forceinline__ void mirror_planes(uint4& A, uint4& B, bool flip) {
    tpl::Board s;
    tpl::unpack_board(A, B, s);
    mirror_board(s, flip);
    const uint32_t spare = B.y & 0x80000000u;
    tpl::pack_board(s, A, B);
    B.y |= spare;
}

}  // namespace tpl_learn
