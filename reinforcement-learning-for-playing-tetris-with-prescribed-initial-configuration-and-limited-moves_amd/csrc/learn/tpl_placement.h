// tpl_placement.h -- what the placement family shares (afterstates.hip, heuristic.hip, beam.hip, ntuple.hip; include/tpl_learn.h
// states the rules): which of the 40 actions are one placement, the first move of a (board, action) pair and its reward, the
// board features, the score and its ordered key, the second ply's loop, and the argument checks of the entry points that read a pair of state planes.
#pragma once

#include "tpl_learn_internal.h"
#include "tpl_mirror.h"

namespace tpl_learn {

constexpr int kActions = TPL_NUM_ACTIONS;
constexpr int kFeatures = TPL_NUM_FEATURES;

// canonical[a] = 10 (r mod nrot(cur)) + min(l, 10 - w(cur, r)) for a = 10 r + l, r < 4, l < 10; reads tpl_mirror.h's packed
// widths and rotation masks instead of a dependent load of the shape table
__host__ __device__ constexpr uint32_t canonical_action(uint32_t cur, uint32_t r, uint32_t l) {
    const uint32_t right = right_most(cur, r);
    return 10u * (r & last_rotation(cur)) + (l < right ? l : right);
}

// tpl_mirror.h's walk visits exactly the actions that are their own canonical form, in ascending order, placement_count of them
constexpr bool walk_visits_the_canonical_actions() {
    for (uint32_t p = 0; p < 8u; ++p) {
        uint32_t r = 0u, l = 0u, steps = 0u;
        for (uint32_t a = 0; a < (uint32_t)kActions; ++a) {
            if (canonical_action(p, a / 10u, a % 10u) != a) continue;
            if (r > last_rotation(p) || 10u * r + l != a) return false;
            next_placement(p, r, l);
            ++steps;
        }
        if (r <= last_rotation(p) || steps != placement_count(p)) return false;
    }
    return true;
}
static_assert(walk_visits_the_canonical_actions(), "next_placement and placement_count do not match canonical_action");

// The first move of pair (state (A, B), action 10 r + l): `s` becomes the board the move leaves, its window not yet popped;
// `cur` is the piece that was placed and `running` whether the state was still in play (a finished board's move means
// nothing: the callers select on `running`).  Returns the rows cleared.  r and l are values, never register indices
// (move_board's comment says why).
__device__ __forceinline__ uint32_t first_move(const uint4& A, const uint4& B, const tpl::ShapeWord* shape, uint32_t r, uint32_t l,
                                               uint32_t L, uint32_t M, tpl::Board& s, uint32_t& cur, bool& running) {
    tpl::unpack_board(A, B, s);
    cur = s.window & 7u;
    running = s.state == tpl::ST_RUNNING;
    bool topout;
    return tpl::move_board(s, shape, r, l, L, M, topout);
}

// step_reward's rule (csrc/tpl_step.h) for a move that cleared n_clear rows and left `state`: one rounded multiply, then at most
// one rounded add; contraction off, or the pair becomes an FMA whose single rounding differs where r_line * n is not exact
__device__ __forceinline__ float move_reward(float r_line, float r_win, float r_lose, uint32_t n_clear, uint32_t state) {
#pragma clang fp contract(off)
    float reward = r_line * (float)n_clear;
    if (state == tpl::ST_WON) reward = reward + r_win;
    if (state >= tpl::ST_LOST_LIMIT) reward = reward + r_lose;
    return reward;
}

struct Features { uint32_t f[kFeatures]; };

// popcount(x) + acc: v_bcnt_u32_b32 adds its second operand
__device__ __forceinline__ uint32_t bcnt(uint32_t x, uint32_t acc) { return (uint32_t)__builtin_popcount(x) + acc; }
__device__ __forceinline__ uint32_t absdiff(uint32_t a, uint32_t b) { return max(a, b) - min(a, b); }

// features 3..11 of a board given as its ten column words (bit r = row r, row 0 = top; bits 20.. clear)
__device__ __forceinline__ void board_features(const uint32_t (&c)[tpl::kCols], Features& out) {
    constexpr uint32_t kFloor = tpl::kSentinelBit;            // row 20: the floor, filled
    uint32_t t[tpl::kCols];                                   // top of column x: row of its top-most filled cell, 20 if empty
#pragma unroll
    for (int x = 0; x < tpl::kCols; ++x) t[x] = (uint32_t)__builtin_ctz(c[x] | kFloor);

    uint32_t top_sum = 0, top_min = tpl::kRows, filled = 0;
    uint32_t col_trans = 0, hole_rows = 0, depth = 0;
#pragma unroll
    for (int x = 0; x < tpl::kCols; ++x) {
        top_sum += t[x];
        top_min = min(top_min, t[x]);
        filled = bcnt(c[x], filled);
        // rows r = 0..19 against r + 1 with the floor as row 20: pairs (r, r + 1), r < 19, and the floor term
        const uint32_t cf = c[x] | kFloor;
        col_trans = bcnt((cf ^ (cf >> 1)) & tpl::kColMask, col_trans);
        // holes of the column: the empty cells below its top
        hole_rows |= ~c[x] & (tpl::kColMask >> t[x] << t[x]);
        // the run of filled cells from the top down; it ends at the column's top-most hole unless it reaches the floor
        const uint32_t run = (uint32_t)__builtin_ctz(~(c[x] >> t[x]));
        depth += t[x] + run < (uint32_t)tpl::kRows ? run : 0u;
    }
    const uint32_t height_sum = tpl::kRows * tpl::kCols - top_sum;

    uint32_t bump = 0;
#pragma unroll
    for (int x = 0; x + 1 < tpl::kCols; ++x) bump += absdiff(t[x], t[x + 1]);

    // per row: wall | x = 0..9 | wall, the walls filled
    uint32_t row_trans = bcnt(~c[0] & tpl::kColMask, 0);
#pragma unroll
    for (int x = 0; x + 1 < tpl::kCols; ++x) row_trans = bcnt(c[x] ^ c[x + 1], row_trans);
    row_trans = bcnt(~c[tpl::kCols - 1] & tpl::kColMask, row_trans);

    // d_x = max(0, min(h_{x-1}, h_{x+1}) - h_x) = max(0, t_x - max(t_{x-1}, t_{x+1})), t = 0 beyond the walls (h = 20)
    uint32_t wells = 0;
#pragma unroll
    for (int x = 0; x < tpl::kCols; ++x) {
        const uint32_t left = x > 0 ? t[x - 1] : 0u, right = x + 1 < tpl::kCols ? t[x + 1] : 0u;
        const uint32_t side = max(left, right);
        const uint32_t d = t[x] > side ? t[x] - side : 0u;
        wells += __umul24(d, d + 1u) >> 1;
    }

    out.f[3] = height_sum - filled;                            // holes: the cells below the tops that are not filled
    out.f[4] = height_sum;
    out.f[5] = tpl::kRows - top_min;
    out.f[6] = bump;
    out.f[7] = row_trans;
    out.f[8] = col_trans;
    out.f[9] = wells;
    out.f[10] = (uint32_t)__builtin_popcount(hole_rows);
    out.f[11] = depth;
}

// phi of the board `s` that a move (or two) left: rows cleared, won, lost and board_features; all zero where `live` is false
__device__ __forceinline__ void moved_features(const tpl::Board& s, uint32_t n_clear, bool live, Features& out) {
    board_features(s.c, out);
    out.f[0] = n_clear;
    out.f[1] = s.state == tpl::ST_WON ? 1u : 0u;
    out.f[2] = s.state >= tpl::ST_LOST_LIMIT ? 1u : 0u;
#pragma unroll
    for (int k = 0; k < kFeatures; ++k) out.f[k] = live ? out.f[k] : 0u;
}

// w . phi left to right in float32: every product and every sum rounded once -- contraction off, as move_reward
__device__ __forceinline__ float placement_score(const float (&w)[kFeatures], const Features& phi) {
#pragma clang fp contract(off)
    float s = w[0] * (float)phi.f[0];
#pragma unroll
    for (int k = 1; k < kFeatures; ++k) s = s + w[k] * (float)phi.f[k];
    return s;
}

// float32 -> uint32 with the order of the floats; -0 and +0 get one image, as they compare equal
__device__ __forceinline__ uint32_t ordered_bits(float x) {
    uint32_t u = __float_as_uint(x);
    u = u == 0x80000000u ? 0u : u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

constexpr uint32_t kNoSecond = 255u;

// The second ply with the known next piece: the best  worth(s2, n2)  among the distinct placements of s1's current piece on s1,
// the popped and still running board a first move left, and in `second` the placement it belongs to.  Copies s1, moves (s2 is
// what the move leaves, its window not yet popped, n2 the rows it cleared; `worth` may change s2) and scores once per distinct
// placement in ascending b = 10 r2 + l2 -- 9, 17 or 34 trips, the same for the 40 lanes of a board -- and keeps a running
// best under a strict > on the ordered key, so the lowest b survives.  r2 and l2 are values out of the packed widths, never
// register indices.  The one loop of tpl_placement_search and tpl_ntuple_search: they enumerate and tie-break alike by it.
template <typename Worth>
__device__ __forceinline__ float best_second(const tpl::Board& s1, const tpl::ShapeWord* shape, uint32_t L, uint32_t M,
                                             uint32_t& second, Worth worth) {
    const uint32_t nxt = s1.window & 7u;
    const uint32_t last_rot = last_rotation(nxt);
    uint32_t best_key = 0u, r2 = 0u, l2 = 0u;
    float best = 0.0f;
#pragma unroll 1
    while (r2 <= last_rot) {
        tpl::Board s2 = s1;
        bool topout;
        const uint32_t n2 = tpl::move_board(s2, shape, r2, l2, L, M, topout);
        const float q = worth(s2, n2);
        const uint32_t key = ordered_bits(q);                           // never 0, so the first trip is taken
        if (key > best_key) { best_key = key; best = q; second = 10u * r2 + l2; }
        next_placement(nxt, r2, l2);
    }
    return best;
}

// the checks of every entry point that reads n states from a pair of planes; `name` leads the message.  L and M are the
// environment's (tpl_create): move_board adds up to four rows to `lines` before pack_board writes it into eight bits
inline int check_planes(const char* name, const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M) {
    if (!plane_a || !plane_b) return fail_msg(TPL_ERR_ARG, "%s: null pointer", name);
    if (n < 1) return fail_msg(TPL_ERR_ARG, "%s: n must be positive", name);
    if (n >= (((int64_t)1 << 31) + kActions - 1) / kActions)
        return fail_msg(TPL_ERR_ARG, "%s: n too large (40 n must stay below 2^31)", name);
    if (L < 1 || L > 250 || M < 1 || M > 254)
        return fail_msg(TPL_ERR_ARG, "%s: L and M must be in [1, 250] and [1, 254]", name);
    if (((uintptr_t)plane_a & 15u) || ((uintptr_t)plane_b & 15u))
        return fail_msg(TPL_ERR_ARG, "%s: planes must be 16-byte aligned", name);
    return TPL_OK;
}

// what every policy entry refuses besides check_planes (tpl_placement_act's list in include/tpl_learn.h)
inline int check_policy(const char* name, const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M,
                        const float* weights, int64_t boards_per_member, const uint8_t* action, const float* score) {
    if (const int rc = check_planes(name, plane_a, plane_b, n, L, M)) return rc;
    if (!weights || !action) return fail_msg(TPL_ERR_ARG, "%s: null pointer (weights and action are required)", name);
    if (boards_per_member < 1) return fail_msg(TPL_ERR_ARG, "%s: boards_per_member must be positive", name);
    if ((uintptr_t)weights & 15u) return fail_msg(TPL_ERR_ARG, "%s: weights must be 16-byte aligned", name);
    if ((uintptr_t)score & 3u) return fail_msg(TPL_ERR_ARG, "%s: score must be 4-byte aligned", name);
    return TPL_OK;
}

}  // namespace tpl_learn
