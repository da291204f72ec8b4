// afterstates.hip -- the 40 successors of a board: tpl_afterstates, tpl_canonical_action (include/tpl_learn.h states the rule).
//
// The environment answers "what if every board plays action a" by stepping its resident state; a learner that scores the
// placements of the current piece wants all 40 answers for one position.  This unit produces them without touching the
// position: for board i and action a = 10 r + l, pair (i, a) at index 40 i + a gets the 32-byte afterstate, the reward, done,
// the rows cleared and the canonical alias of a -- tpl_device.h's own unpack_board / move_board / next_window / pack_board, so
// an afterstate is what a non-auto-reset step leaves, up to window entries 2..11 on the refill move.
//
// Lane mapping: one lane per PAIR, lane j of the grid = pair j.  Every output is then one contiguous stream: a wave writes 1 KiB
// of each state plane with 16-byte stores, 256 B of rewards and 64 B of each byte array, all consecutive.  The read side is 32 B
// per board, taken by all 40 lanes of the board: a wave holds 1.6 boards, so its two 16-byte loads touch at most three boards
// (one or two 128-byte lines per plane) and the 40-fold reuse is served by the load unit, not by memory.  The other mapping,
// a lane per board looping over 40 actions, would take the ten column tops once per board instead of once per pair, but its
// stores are 640 B apart per lane (16 B per lane per row, 64 rows per wave store): the write side is 98 % of the traffic
// (1,560 B out against 32 B in), so it decides.  Per board: 32 B read, 40 x (32 + 4 + 1 + 1 + 1) = 1,560 B written.
#include "tpl_placement.h"

namespace tpl_learn {
namespace {

constexpr int kAfterBlock = 256;

struct AfterArgs {
    const uint4* a;              // [n]
    const uint4* b;
    uint32_t total;              // 40 n, below 2^31
    uint32_t L, M;
    float r_line, r_win, r_lose;
    uint4* out_a;                // [n][40], with out_b or not at all
    uint4* out_b;
    float* reward;               // [n][40], each optional
    uint8_t* done;
    uint8_t* cleared;
    uint8_t* canonical;
};

__global__ __launch_bounds__(kAfterBlock) void afterstates_kernel(const AfterArgs p) {
    __shared__ tpl::ShapeWord s_shape[32];
    if (threadIdx.x < 32) s_shape[threadIdx.x] = tpl::kShapeTable[threadIdx.x];
    __syncthreads();
    const uint32_t j = blockIdx.x * kAfterBlock + threadIdx.x;          // pair 40 i + a
    if (j >= p.total) return;
    const uint32_t i = j / kActions, a = j - i * kActions;
    const uint32_t r = a / 10u, l = a - r * 10u;
    const uint4 A = p.a[i], B = p.b[i];
    tpl::Board s;
    uint32_t cur;
    bool running;
    const uint32_t n_clear = first_move(A, B, s_shape, r, l, p.L, p.M, s, cur, running);
    tpl::next_window(s, false, 0);                                      // pieces.pop(0) without a refill: zeros enter
    const float reward = move_reward(p.r_line, p.r_win, p.r_lose, n_clear, s.state);

    // a finished board stays as it is, bit for bit, with reward 0, done 1, cleared 0 (a frozen board of tpl_step): selects
    if (p.out_a) {
        uint4 A2, B2;
        tpl::pack_board(s, A2, B2);
        B2.y |= B.y & 0x80000000u;                                      // the spare bit (the slot travels in the Board)
        p.out_a[j] = make_uint4(running ? A2.x : A.x, running ? A2.y : A.y, running ? A2.z : A.z, running ? A2.w : A.w);
        p.out_b[j] = make_uint4(running ? B2.x : B.x, running ? B2.y : B.y, running ? B2.z : B.z, running ? B2.w : B.w);
    }
    if (p.reward) p.reward[j] = running ? reward : 0.0f;
    if (p.done) p.done[j] = (uint8_t)(running ? (s.state != tpl::ST_RUNNING ? 1u : 0u) : 1u);
    if (p.cleared) p.cleared[j] = (uint8_t)(running ? n_clear : 0u);
    if (p.canonical) p.canonical[j] = (uint8_t)canonical_action(cur, r, l);
}

}  // namespace
}  // namespace tpl_learn

using namespace tpl_learn;

extern "C" int32_t tpl_canonical_action(int32_t cur, int32_t action) {
    if (cur < 0 || cur > 7 || action < 0 || action >= kActions) return -1;
    return (int32_t)canonical_action((uint32_t)cur, (uint32_t)action / 10u, (uint32_t)action % 10u);
}

extern "C" int tpl_afterstates(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line,
                               float r_win, float r_lose, void* out_a, void* out_b, float* reward, uint8_t* done,
                               uint8_t* cleared, uint8_t* canonical, void* stream) {
    if (const int rc = check_planes("tpl_afterstates", plane_a, plane_b, n, L, M)) return rc;
    if ((out_a == nullptr) != (out_b == nullptr)) return fail_msg(TPL_ERR_ARG, "tpl_afterstates: out_a and out_b go together");
    if (!out_a && !reward && !done && !cleared && !canonical)
        return fail_msg(TPL_ERR_ARG, "tpl_afterstates: at least one output must be given");
    if (((uintptr_t)out_a & 15u) || ((uintptr_t)out_b & 15u))
        return fail_msg(TPL_ERR_ARG, "tpl_afterstates: out_a and out_b must be 16-byte aligned");
    if ((uintptr_t)reward & 3u) return fail_msg(TPL_ERR_ARG, "tpl_afterstates: reward must be 4-byte aligned");
    AfterArgs p{};
    p.a = (const uint4*)plane_a; p.b = (const uint4*)plane_b; p.total = (uint32_t)(n * kActions);
    p.L = (uint32_t)L; p.M = (uint32_t)M; p.r_line = r_line; p.r_win = r_win; p.r_lose = r_lose;
    p.out_a = (uint4*)out_a; p.out_b = (uint4*)out_b;
    p.reward = reward; p.done = done; p.cleared = cleared; p.canonical = canonical;
    const dim3 grid((p.total + kAfterBlock - 1) / kAfterBlock), block(kAfterBlock);
    hipLaunchKernelGGL(afterstates_kernel, grid, block, 0, (hipStream_t)stream, p);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}
