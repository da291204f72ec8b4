// ntuple_rank.hip -- what a proved move label teaches an n-tuple table: tpl_ntuple_rank (include/tpl_learn.h states the rule).
//
// A label row says which placements of a board are proved winning (1) and which proved losing (2).  This unit scores every distinct
// placement exactly as the one-ply policy does, finds the best-scored proved win, the best-scored proved loss and the greedy choice,
// and says whether the table already prefers the win by more than the margin.  Where it does not, it hands out the two afterstates
// with the errors +1 and -1: the perceptron step on the hardest pair, which the existing add-only update kernels then make.  The
// table is only read here and only added to there, so a step leaves the same bytes in any order.
//
// Frame: ntuple_policy's (ntuple.hip) -- blocks of 320 threads = 8 boards x 40 actions, the shape table in LDS, first_move, the pop,
// the score and a 64-bit LDS maximum on ordered score << 32 | 39 - a -- with THREE maxima a board (over the proved wins, over the
// proved losses, over all distinct placements) where the policy has one, a label byte a lane, and no exploration draw.  The lane at
// a maximum holds the board its move left in registers and packs it from there.  The gap needs both scores in one lane, and a
// key's high word is the score up to the sign of a zero, which a difference can see: the two lanes put their scores, and whether
// each held a gamma * V term, in LDS, and lane 0 of the board subtracts after one more barrier.
//
// One kernel per plain table form, each a name and a geometry of tpl_ntuple.h as ntuple.hip's kernels are; the budget geometry
// alone reads the prune flag.  ntuple.hip is not touched.
#include <cmath>

#include "tpl_ntuple.h"

namespace tpl_learn {
namespace {

constexpr int kBoardsPerBlock = 8;
constexpr int kRankBlock = kBoardsPerBlock * kActions;        // 320 threads, five waves, eight whole boards
static_assert(kRankBlock % 64 == 0, "a block is whole waves");
constexpr uint32_t kUndecided = 255u;
constexpr uint32_t kLabelWin = 1u, kLabelLoss = 2u;

struct RankArgs {
    const uint4* a;              // [n]
    const uint4* b;
    uint32_t n;                  // boards; 40 n below 2^31
    uint32_t L, M;
    float r_line, r_win, r_lose, gamma;
    const int32_t* table;        // read only
    const uint8_t* label;        // [n][40]
    float margin;
    uint32_t prune;              // not 0: the dead-board prune (the budget geometry alone)
    uint8_t* win;                // [n] each
    uint8_t* loss;
    uint8_t* greedy;
    uint8_t* violated;
    float* gap;
    float* err_win;
    float* err_loss;
    uint4* win_a;
    uint4* win_b;
    uint4* loss_a;
    uint4* loss_b;
};

enum { kSlotWin = 0, kSlotLoss = 1, kSlotGreedy = 2, kSlots = 3 };

template <typename S>
__device__ __forceinline__ void ntuple_rank(const RankArgs& p) {
    __shared__ tpl::ShapeWord s_shape[32];
    __shared__ unsigned long long s_best[kSlots][kBoardsPerBlock];
    __shared__ float s_score[2][kBoardsPerBlock];                       // the scores of the pair, their own bits
    __shared__ uint32_t s_valued[2][kBoardsPerBlock];                   // whether each held a gamma * V term
    const uint32_t first = blockIdx.x * kBoardsPerBlock;                // the block's boards: first .. first + 7
    if (threadIdx.x < 32) s_shape[threadIdx.x] = tpl::kShapeTable[threadIdx.x];
    if (threadIdx.x < kSlots * kBoardsPerBlock) (&s_best[0][0])[threadIdx.x] = 0ull;   // below every key: a key's high word has a bit set
    __syncthreads();
    const uint32_t slot = threadIdx.x / kActions, a = threadIdx.x - slot * kActions;
    const uint32_t r = a / 10u, l = a - r * 10u;
    const uint32_t i = first + slot;
    const bool valid = i < p.n;                                         // whole boards: all 40 lanes of a board agree
    const uint32_t src = valid ? i : p.n - 1u;                          // past the end: the last board again, never written

    const uint4 A = p.a[src], B = p.b[src];
    const uint32_t label = p.label[src * (uint32_t)kActions + a];       // forty consecutive bytes a board
    tpl::Board s1;
    uint32_t cur;
    bool running;
    const uint32_t n1 = first_move(A, B, s_shape, r, l, p.L, p.M, s1, cur, running);
    tpl::next_window(s1, false, 0);                                     // tpl_afterstates' pop: the next piece becomes current
    const bool contends = valid && canonical_action(cur, r, l) == a;

    uint32_t scored = s1.state;                                         // the state the move is scored with
    if constexpr (kBudgetGeometry<S>) {
        tpl::Board pruned = s1;
        prune_dead<S>(pruned, p.L, p.M, p.prune);
        scored = pruned.state;
    }
    const bool valued = running && scored == tpl::ST_RUNNING;           // the score holds a gamma * V term

    float v = 0.0f;
    if (contends && valued) v = ntuple_value<S>(s1, p.L, p.M, p.table);
    float score;
    {
#pragma clang fp contract(off)
        const float reward = move_reward(p.r_line, p.r_win, p.r_lose, n1, scored);
        const float later = p.gamma * v;
        score = running ? (valued ? reward + later : reward) : 0.0f;
    }
    const unsigned long long key = ((unsigned long long)ordered_bits(score) << 32) | (uint32_t)(kActions - 1 - a);
    // a label on an alias or on a finished board, and every byte but 1 and 2, takes part in nothing
    const bool in_w = contends && running && label == kLabelWin;
    const bool in_x = contends && running && label == kLabelLoss;
    if (in_w) atomicMax(&s_best[kSlotWin][slot], key);
    if (in_x) atomicMax(&s_best[kSlotLoss][slot], key);
    if (contends) atomicMax(&s_best[kSlotGreedy][slot], key);
    __syncthreads();
    const bool decided = s_best[kSlotWin][slot] != 0ull && s_best[kSlotLoss][slot] != 0ull;
    const bool is_win = decided && in_w && s_best[kSlotWin][slot] == key;       // one lane per board: its keys are distinct
    const bool is_loss = decided && in_x && s_best[kSlotLoss][slot] == key;
    if (contends && s_best[kSlotGreedy][slot] == key) p.greedy[i] = (uint8_t)a;
    if (is_win || is_loss) {                                            // a labelled board runs: the afterstate is the move's
        const int side = is_win ? 0 : 1;
        s_score[side][slot] = score;
        s_valued[side][slot] = valued ? 1u : 0u;
        uint4 A2, B2;
        tpl::pack_board(s1, A2, B2);
        B2.y |= B.y & 0x80000000u;                                      // the spare bit (the slot travels in the Board)
        (is_win ? p.win : p.loss)[i] = (uint8_t)a;
        (is_win ? p.win_a : p.loss_a)[i] = A2;
        (is_win ? p.win_b : p.loss_b)[i] = B2;
    }
    __syncthreads();
    if (valid && a == 0u) {                                             // the board's own lane: the gap and what it teaches
        float gap = 0.0f, err_win = 0.0f, err_loss = 0.0f;
        bool violated = false;
        if (decided) {
            gap = s_score[0][slot] - s_score[1][slot];
            violated = gap <= p.margin;                                 // a tie violates at margin 0; a NaN does not
            err_win = violated && s_valued[0][slot] != 0u ? 1.0f : 0.0f;
            err_loss = violated && s_valued[1][slot] != 0u ? -1.0f : 0.0f;
        } else {                                                        // undecided: both afterstates are the state, bit for bit
            p.win[i] = (uint8_t)kUndecided;
            p.loss[i] = (uint8_t)kUndecided;
            p.win_a[i] = A; p.win_b[i] = B;
            p.loss_a[i] = A; p.loss_b[i] = B;
        }
        p.gap[i] = gap;
        p.violated[i] = violated ? (uint8_t)1 : (uint8_t)0;
        p.err_win[i] = err_win;
        p.err_loss[i] = err_loss;
    }
}

__global__ __launch_bounds__(kRankBlock) void ntuple_rank_kernel(const RankArgs p) { ntuple_rank<Shape2x4>(p); }
__global__ __launch_bounds__(kRankBlock) void ntuple_rank3_kernel(const RankArgs p) { ntuple_rank<Shape3x3>(p); }
__global__ __launch_bounds__(kRankBlock) void ntuple_rank_feature_kernel(const RankArgs p) { ntuple_rank<FeatureTable>(p); }
__global__ __launch_bounds__(kRankBlock) void ntuple_rank_budget_kernel(const RankArgs p) { ntuple_rank<BudgetTable>(p); }

}  // namespace
}  // namespace tpl_learn

using namespace tpl_learn;

extern "C" int tpl_ntuple_rank(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const int32_t* table,
                               int64_t entries, const uint8_t* label, float r_line, float r_win, float r_lose, float gamma,
                               float margin, int32_t prune, uint8_t* win, uint8_t* loss, uint8_t* greedy, uint8_t* violated,
                               float* gap, float* err_win, float* err_loss, void* win_a, void* win_b, void* loss_a, void* loss_b,
                               void* stream) {
    const char* name = "tpl_ntuple_rank";
    // a table of any other entry count is refused first, before any pointer is looked at
    if (entries != TPL_NTUPLE_ENTRIES && entries != TPL_NTUPLE_ENTRIES_3X3 && entries != TPL_NTUPLE_ENTRIES_FEAT &&
        entries != TPL_NTUPLE_ENTRIES_BUDGET)
        return fail_msg(TPL_ERR_ARG,
                        "%s: entries must be %d (\"2x4\"), %d (\"3x3\"), %d (\"feat\") or %d (\"feat+spare\"), the four plain forms -- a sum "
                        "or a staged table is taught no ranking --, got %lld",
                        name, (int)TPL_NTUPLE_ENTRIES, (int)TPL_NTUPLE_ENTRIES_3X3, (int)TPL_NTUPLE_ENTRIES_FEAT,
                        (int)TPL_NTUPLE_ENTRIES_BUDGET, (long long)entries);
    if (const int rc = check_planes(name, plane_a, plane_b, n, L, M)) return rc;
    if (const int rc = check_table(name, table)) return rc;
    if (!label) return fail_msg(TPL_ERR_ARG, "%s: null pointer (label is required)", name);
    if (!win || !loss || !greedy || !violated || !gap || !err_win || !err_loss || !win_a || !win_b || !loss_a || !loss_b)
        return fail_msg(TPL_ERR_ARG, "%s: null pointer (every output is required)", name);
    if (((uintptr_t)win_a & 15u) || ((uintptr_t)win_b & 15u) || ((uintptr_t)loss_a & 15u) || ((uintptr_t)loss_b & 15u))
        return fail_msg(TPL_ERR_ARG, "%s: win_a, win_b, loss_a and loss_b must be 16-byte aligned", name);
    if (((uintptr_t)gap & 3u) || ((uintptr_t)err_win & 3u) || ((uintptr_t)err_loss & 3u))
        return fail_msg(TPL_ERR_ARG, "%s: gap, err_win and err_loss must be 4-byte aligned", name);
    if (!std::isfinite(margin)) return fail_msg(TPL_ERR_ARG, "%s: margin must be finite", name);
    if (!std::isfinite(gamma)) return fail_msg(TPL_ERR_ARG, "%s: gamma must be finite", name);
    if (!std::isfinite(r_line) || !std::isfinite(r_win) || !std::isfinite(r_lose))
        return fail_msg(TPL_ERR_ARG, "%s: r_line, r_win and r_lose must be finite", name);
    if (prune != 0 && prune != 1) return fail_msg(TPL_ERR_ARG, "%s: prune must be 0 or 1", name);
    if (prune != 0 && entries != TPL_NTUPLE_ENTRIES_BUDGET)
        return fail_msg(TPL_ERR_ARG, "%s: prune = 1 is the dead-board prune of a budget table (\"feat+spare\", %d entries) alone", name,
                        (int)TPL_NTUPLE_ENTRIES_BUDGET);
    RankArgs p{};
    p.a = (const uint4*)plane_a; p.b = (const uint4*)plane_b; p.n = (uint32_t)n;
    p.L = (uint32_t)L; p.M = (uint32_t)M; p.r_line = r_line; p.r_win = r_win; p.r_lose = r_lose; p.gamma = gamma;
    p.table = table; p.label = label; p.margin = margin; p.prune = (uint32_t)prune;
    p.win = win; p.loss = loss; p.greedy = greedy; p.violated = violated; p.gap = gap; p.err_win = err_win; p.err_loss = err_loss;
    p.win_a = (uint4*)win_a; p.win_b = (uint4*)win_b; p.loss_a = (uint4*)loss_a; p.loss_b = (uint4*)loss_b;
    const dim3 grid((p.n + kBoardsPerBlock - 1) / kBoardsPerBlock), block(kRankBlock);
    if (entries == TPL_NTUPLE_ENTRIES) hipLaunchKernelGGL(ntuple_rank_kernel, grid, block, 0, (hipStream_t)stream, p);
    else if (entries == TPL_NTUPLE_ENTRIES_3X3) hipLaunchKernelGGL(ntuple_rank3_kernel, grid, block, 0, (hipStream_t)stream, p);
    else if (entries == TPL_NTUPLE_ENTRIES_FEAT) hipLaunchKernelGGL(ntuple_rank_feature_kernel, grid, block, 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(ntuple_rank_budget_kernel, grid, block, 0, (hipStream_t)stream, p);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}
