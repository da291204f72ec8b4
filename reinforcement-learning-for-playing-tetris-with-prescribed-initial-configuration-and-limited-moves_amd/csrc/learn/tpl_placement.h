// tpl_placement.h -- what the placement family shares (afterstates.hip, heuristic.hip; include/tpl_learn.h states the rules):
// which of the 40 actions are one placement, the first move of a (board, action) pair, and the argument checks of the entry
// points that read a pair of state planes.
#pragma once

#include "tpl_learn_internal.h"
#include "tpl_mirror.h"

namespace tpl_learn {

constexpr int kActions = TPL_NUM_ACTIONS;

// canonical[a] = 10 (r mod nrot(cur)) + min(l, 10 - w(cur, r)) for a = 10 r + l, r < 4, l < 10; reads tpl_mirror.h's packed
// widths and rotation masks instead of a dependent load of the shape table
__host__ __device__ __forceinline__ uint32_t canonical_action(uint32_t cur, uint32_t r, uint32_t l) {
    const uint32_t right = 9u - ((uint32_t)(kWidthsLess1 >> (2u * (cur * 4u + r))) & 3u);      // 10 - w
    const uint32_t rc = r & ((kRotationMasks >> (2u * cur)) & 3u);
    return 10u * rc + (l < right ? l : right);
}

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

// the checks of every entry point that reads n states from a pair of planes; `name` leads the message
inline int check_planes(const char* name, const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M) {
    if (!plane_a || !plane_b) return fail_msg(TPL_ERR_ARG, "%s: null pointer", name);
    if (n < 1) return fail_msg(TPL_ERR_ARG, "%s: n must be positive", name);
    if (n >= (((int64_t)1 << 31) + kActions - 1) / kActions)
        return fail_msg(TPL_ERR_ARG, "%s: n too large (40 n must stay below 2^31)", name);
    if (L < 1 || L > 255 || M < 1 || M > 255) return fail_msg(TPL_ERR_ARG, "%s: L and M must be in [1, 255]", name);
    if (((uintptr_t)plane_a & 15u) || ((uintptr_t)plane_b & 15u))
        return fail_msg(TPL_ERR_ARG, "%s: planes must be 16-byte aligned", name);
    return TPL_OK;
}

}  // namespace tpl_learn
