// ntuple_exact.hip -- the exact depth-first solver with its children ordered by an n-tuple table: tpl_ntuple_exact (include/tpl_learn.h
// states the rule).
//
// tpl_placement_exact (exact.hip) searches the whole game of a prescribed configuration depth first, and its linear weights do one
// thing: they order a node's children.  This unit is that search with the order taken from a table instead -- a child is worth
// reward + gamma V(afterstate), what the one-ply n-tuple policy scores a first move with, read in the game (L, B) of the iteration --
// so that a table trained on a tight pool decides which branch a proof tries first.  The children, the stop, the descent, the node
// cap and the budgets are exact.hip's, and so is what a finished search says: the order decides how many nodes a proof takes.
//
// Mapping: exact.hip's.  ONE CONFIGURATION PER WAVEFRONT, one wavefront a workgroup, no barrier in the search loop; lane k < 34 makes
// child k, the k-th distinct placement of the ply's piece in ascending b, and its 64-bit key (ordered_bits(value) << 32 | kSlotTop - k);
// a ballot over the won children is the stop; the running children are ranked by 34 lane reads of a key; the stack is dynamic LDS,
// one 80-byte record a depth -- the node's packed board, the number of its running children, a cursor and their placements in the
// order of the descent (no carry: a table's value reads the board alone); a later child is made again from its parent's record when the
// search comes back to it, without its value.  Nothing but the outputs goes to memory.
//
// The table is read from global memory, where it stays: a child's V is eleven gathers under a budget table and ten under a feature
// table (84 and 76 KB, which sit in L2), and up to 154 and 145 under the window forms -- the non-empty windows of the board.  One wave
// a workgroup cannot afford a copy in LDS.  The body is a template over the geometry of tpl_ntuple.h, reached through ntuple_value<S>,
// and each __global__ kernel names its geometry, as ntuple.hip's do.  The budget geometry hands ntuple_value the board and (L, B);
// prune_dead is not called: bounded_move has already turned a dead child lost.
#ifndef TPL_PLACEMENT_BOUND_UNIT
#define TPL_PLACEMENT_BOUND_UNIT
#endif
#include "tpl_beam.h"
#include "tpl_ntuple.h"

namespace tpl_learn {
namespace {

constexpr int kExactMaxMoves = 254;                           // M's limit (tpl_create's)
constexpr int kExactWave = 64;
constexpr int kExactMaxNodes = TPL_EXACT_MAX_NODES;
static_assert(kUnitBound, "the exact search is a unit of the bounded form");
static_assert(kMaxPlacements <= kExactWave, "a lane per child");

struct NTupleExactArgs {
    const uint16_t* rows;        // [n][20], bit x = column x
    const uint8_t* pieces;       // [n][M + 1]
    uint32_t n;                  // configurations = workgroups of one wave
    uint32_t L, M;
    const int32_t* table;        // of the kernel's geometry
    float r_line, r_win, r_lose, gamma;
    uint32_t max_nodes;          // in [1, 2^24]
    uint32_t shortest;           // 1: budgets need(root) .. M; 0: M alone
    uint8_t* solved;             // [n]
    uint8_t* proved;             // [n]
    int32_t* solution_len;       // [n]
    uint8_t* actions;            // [n][M]
    int32_t* bound;              // [n]: need(root)
    uint32_t* nodes;             // [n]: expansions, all iterations
};

// one depth of the stack
struct alignas(16) Frame {
    uint4 a, b;                  // the node's board; its window is not part of the rule
    uint32_t count;              // its running children
    uint32_t cursor;             // how many of them have been descended into
    uint8_t kids[36];            // their placements b = 10 r + l in the order of the descent, kMaxPlacements at most
};
static_assert(sizeof(Frame) == 80, "a record is 80 bytes");

// LDS written by one lane, read by another of the same wave: the accesses of a wave reach LDS in order, so this only keeps the
// compiler from moving them across and waits for the write
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// The child of `node` by placement (r, l) of piece `cur` in the game (L, B): the board the move leaves, dead turned lost, with `nxt`,
// the piece the child will play, as its falling piece.  Returns the rows the move cleared.  The expansion and the return both come
// here, so a child's second making gives the board of the first.
__device__ __forceinline__ uint32_t make_child(const Frame& node, uint32_t cur, uint32_t nxt, uint32_t r, uint32_t l,
                                               const tpl::ShapeWord* shape, uint32_t L, uint32_t B, tpl::Board& s) {
    tpl::unpack_board(node.a, node.b, s);
    s.window = cur;
    s.window_hi = 0u;
    const uint32_t n_clear = placed_move<kFeatures>(s, shape, r, l, L, B);
    bounded_move(s, L, B);
    s.window = nxt;
    return n_clear;
}

// what the one-ply policy scores the move with: reward, or reward + gamma V where the child runs; every product and sum rounded once
template <typename S>
__device__ __forceinline__ float child_value(const tpl::Board& s, uint32_t n_clear, uint32_t L, uint32_t B, const NTupleExactArgs& p) {
#pragma clang fp contract(off)
    const bool on = s.state == tpl::ST_RUNNING;
    float v = 0.0f;
    if (on) v = ntuple_value<S>(s, L, B, p.table);
    const float reward = move_reward(p.r_line, p.r_win, p.r_lose, n_clear, s.state);
    const float later = p.gamma * v;
    return on ? reward + later : reward;
}

__device__ __forceinline__ void store_frame(Frame& f, const tpl::Board& s) {
    uint4 A, B;
    tpl::pack_board(s, A, B);
    f.a = A;
    f.b = B;
}

// exact.hip's search loop, the value apart.  A wave's search is one long dependent chain -- a record read from LDS, a move, the
// table's gathers, a rank, a record written --, and here a trip to L2 or beyond is part of every link, so what hides it is other waves.
template <typename S>
__device__ __forceinline__ void ntuple_exact(const NTupleExactArgs& p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    Frame* const stack = reinterpret_cast<Frame*>(s_raw);      // [M]
    __shared__ tpl::ShapeWord s_shape[32];
    __shared__ uint8_t s_pieces[kExactMaxMoves + 2];
    const uint32_t lane = threadIdx.x, i = blockIdx.x;         // the grid is n blocks of one wave
    const uint32_t L = p.L, M = p.M;
    if (lane < 32) s_shape[lane] = tpl::kShapeTable[lane];
    for (uint32_t t = lane; t <= M; t += kExactWave) s_pieces[t] = p.pieces[(size_t)i * (M + 1u) + t] & 7u;   // masked as move_board masks them

    tpl::Board root;                                           // the root, as a full reset deals it: the same in every lane
    tpl::rows_to_cols(p.rows + (size_t)i * tpl::kRows, root.c);
    root.window = 0u; root.window_hi = 0u;
    root.state = tpl::ST_RUNNING; root.lines = 0u; root.moves = 0u; root.slot = 0u;
    const uint32_t bound = (move_bound_cells(root.c, L) + 3u) >> 2;          // need(root): no solution is shorter
    const uint32_t max_nodes = p.max_nodes;

    uint32_t nodes = 0u, length = 0u, last = kNoMove;          // expansions; the winning length, 0 while there is none, and its last move
    bool capped = false;
    if (bound <= M) {
#pragma unroll 1
        for (uint32_t B = p.shortest ? bound : M; B <= M && length == 0u && !capped; ++B) {
            wave_sync();                                       // the last iteration's reads of record 0 (and, the first time, the tables)
            if (lane == 0) store_frame(stack[0], root);
            wave_sync();
            uint32_t d = 0u;
#pragma unroll 1
            for (;;) {
                // expand the node at depth d
                if (nodes == max_nodes) { capped = true; break; }
                ++nodes;
                const uint32_t cur = uniform(s_pieces[d]), nxt = uniform(s_pieces[d + 1u]);      // d + 1 <= M: the list has M + 1 entries
                const uint32_t stride = placement_count(cur);
                const bool mine = lane < stride;
                const uint32_t k = mine ? lane : 0u;
                uint32_t r, l;
                const uint32_t b = nth_placement(cur, k, r, l);
                tpl::Board s;
                const uint32_t n_clear = make_child(stack[d], cur, nxt, r, l, s_shape, L, B, s);
                const float value = child_value<S>(s, n_clear, L, B, p);
                const uint32_t key_hi = ordered_bits(value), key_lo = kSlotTop - k;
                const bool won = mine && s.state == tpl::ST_WON, running = mine && s.state == tpl::ST_RUNNING;

                // the stop: the won child that comes first in the order
                if (__ballot(won) != 0ull) {
                    const unsigned long long top = wave_max(won ? ((unsigned long long)key_hi << 32) | key_lo : 0ull);
                    uint32_t r2, l2;
                    last = nth_placement(cur, kSlotTop - uniform((uint32_t)top), r2, l2);
                    length = d + 1u;
                    break;
                }

                // the order of the running children: a child's rank is the number of running children with a larger key
                const uint32_t run_hi = running ? key_hi : 0u, run_lo = running ? key_lo : 0u;
                const unsigned long long run_key = ((unsigned long long)run_hi << 32) | run_lo;
                uint32_t rank = 0u;
#pragma unroll
                for (int j = 0; j < kMaxPlacements; ++j) {
                    const unsigned long long other = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)run_hi, j) << 32) |
                                                     (uint32_t)__builtin_amdgcn_readlane((int)run_lo, j);
                    rank += other > run_key ? 1u : 0u;
                }
                const uint32_t count = (uint32_t)__builtin_popcountll(__ballot(running));
                if (running) {
                    stack[d].kids[rank] = (uint8_t)b;
                    if (rank == 0u && d + 1u < M) store_frame(stack[d + 1u], s);      // descended into at once (d + 1 < B <= M)
                }
                if (lane == 0) {
                    stack[d].count = count;
                    stack[d].cursor = count != 0u ? 1u : 0u;
                }
                wave_sync();
                if (count != 0u) { ++d; continue; }

                // no running child: back to the nearest node that has one left, and into it
                bool more = false;
#pragma unroll 1
                while (d > 0u) {
                    --d;
                    const uint32_t at = uniform(stack[d].cursor);
                    if (at < uniform(stack[d].count)) {
                        const uint32_t b2 = uniform(stack[d].kids[at]);
                        tpl::Board s2;
                        make_child(stack[d], uniform(s_pieces[d]), uniform(s_pieces[d + 1u]), b2 / 10u, b2 % 10u, s_shape, L, B, s2);
                        wave_sync();
                        if (lane == 0 && d + 1u < M) {
                            stack[d].cursor = at + 1u;
                            store_frame(stack[d + 1u], s2);
                        }
                        wave_sync();
                        ++d;
                        more = true;
                        break;
                    }
                }
                if (!more) break;                              // the root's children are used up: no win at this budget
            }
        }
    }
    wave_sync();

    if (capped) length = 0u;
    if (lane == 0) {
        p.solved[i] = length != 0u ? (uint8_t)1 : (uint8_t)0;
        p.proved[i] = capped ? (uint8_t)0 : (uint8_t)1;
        p.solution_len[i] = (int32_t)length;
        p.bound[i] = (int32_t)bound;
        p.nodes[i] = nodes;
    }
    // the solution: the child in hand at every depth of the path, then the won one
    for (uint32_t t = lane; t < M; t += kExactWave) {
        uint32_t a = kNoMove;
        if (t + 1u < length) a = stack[t].kids[stack[t].cursor - 1u];
        else if (t + 1u == length) a = last;
        p.actions[(size_t)i * M + t] = (uint8_t)a;
    }
}

// One wave a workgroup, each kernel bound to eight waves a SIMD, which every geometry fits without scratch: 55 VGPRs ("2x4"), 52
// ("3x3"), 59 ("feat") and 60 ("feat+spare") of the 64 the bound allows, 78 SGPRs (tools/kernel_resources.sh;
// profiles/learner/ntuple_exact_isa.log).
__global__ __launch_bounds__(kExactWave, 8) void ntuple_exact_kernel(const NTupleExactArgs p) { ntuple_exact<Shape2x4>(p); }
__global__ __launch_bounds__(kExactWave, 8) void ntuple_exact3_kernel(const NTupleExactArgs p) { ntuple_exact<Shape3x3>(p); }
__global__ __launch_bounds__(kExactWave, 8) void ntuple_exact_feature_kernel(const NTupleExactArgs p) { ntuple_exact<FeatureTable>(p); }
__global__ __launch_bounds__(kExactWave, 8) void ntuple_exact_budget_kernel(const NTupleExactArgs p) { ntuple_exact<BudgetTable>(p); }

}  // namespace
}  // namespace tpl_learn

using namespace tpl_learn;

extern "C" int tpl_ntuple_exact(const int16_t* rows, const uint8_t* pieces, int64_t n, int32_t L, int32_t M, const int32_t* table,
                                int64_t entries, float r_line, float r_win, float r_lose, float gamma, int32_t max_nodes,
                                int32_t shortest, uint8_t* solved, uint8_t* proved, int32_t* solution_len, uint8_t* actions,
                                int32_t* bound, uint32_t* nodes, void* stream) {
    const char* name = "tpl_ntuple_exact";
    // a table of any other entry count is refused first, before any pointer is looked at
    if (entries != TPL_NTUPLE_ENTRIES && entries != TPL_NTUPLE_ENTRIES_3X3 && entries != TPL_NTUPLE_ENTRIES_FEAT &&
        entries != TPL_NTUPLE_ENTRIES_BUDGET)
        return fail_msg(TPL_ERR_ARG,
                        "%s: entries must be %d (\"2x4\"), %d (\"3x3\"), %d (\"feat\") or %d (\"feat+spare\"), the four plain forms -- a sum "
                        "or a staged table orders no search --, got %lld",
                        name, (int)TPL_NTUPLE_ENTRIES, (int)TPL_NTUPLE_ENTRIES_3X3, (int)TPL_NTUPLE_ENTRIES_FEAT,
                        (int)TPL_NTUPLE_ENTRIES_BUDGET, (long long)entries);
    if (!rows || !pieces || !table || !solved || !proved || !solution_len || !actions || !bound || !nodes)
        return fail_msg(TPL_ERR_ARG, "%s: null pointer (every argument but the stream is required)", name);
    if (!(r_line - r_line == 0.0f) || !(r_win - r_win == 0.0f) || !(r_lose - r_lose == 0.0f))
        return fail_msg(TPL_ERR_ARG, "%s: r_line, r_win and r_lose must be finite", name);
    if (!(gamma - gamma == 0.0f)) return fail_msg(TPL_ERR_ARG, "%s: gamma must be finite", name);
    if (n < 1) return fail_msg(TPL_ERR_ARG, "%s: n must be positive", name);
    if (n >= ((int64_t)1 << 31)) return fail_msg(TPL_ERR_ARG, "%s: n too large (a workgroup per configuration: n must stay below 2^31)", name);
    if (L < 1 || L > 250 || M < 1 || M > kExactMaxMoves)
        return fail_msg(TPL_ERR_ARG, "%s: L and M must be in [1, 250] and [1, %d]", name, kExactMaxMoves);
    if (max_nodes < 1 || max_nodes > kExactMaxNodes) return fail_msg(TPL_ERR_ARG, "%s: max_nodes must be in [1, %d]", name, kExactMaxNodes);
    if (shortest != 0 && shortest != 1) return fail_msg(TPL_ERR_ARG, "%s: shortest must be 0 or 1", name);
    if ((uintptr_t)rows & 1u) return fail_msg(TPL_ERR_ARG, "%s: rows must be 2-byte aligned", name);
    if ((uintptr_t)table & 3u) return fail_msg(TPL_ERR_ARG, "%s: table must be 4-byte aligned", name);
    if ((uintptr_t)solution_len & 3u) return fail_msg(TPL_ERR_ARG, "%s: solution_len must be 4-byte aligned", name);
    if ((uintptr_t)bound & 3u) return fail_msg(TPL_ERR_ARG, "%s: bound must be 4-byte aligned", name);
    if ((uintptr_t)nodes & 3u) return fail_msg(TPL_ERR_ARG, "%s: nodes must be 4-byte aligned", name);
    NTupleExactArgs p{};
    p.rows = (const uint16_t*)rows; p.pieces = pieces; p.n = (uint32_t)n;
    p.L = (uint32_t)L; p.M = (uint32_t)M; p.table = table;
    p.r_line = r_line; p.r_win = r_win; p.r_lose = r_lose; p.gamma = gamma;
    p.max_nodes = (uint32_t)max_nodes; p.shortest = (uint32_t)shortest;
    p.solved = solved; p.proved = proved; p.solution_len = solution_len; p.actions = actions; p.bound = bound; p.nodes = nodes;
    const size_t stack = sizeof(Frame) * (size_t)p.M;          // at most 20,320 bytes
    const dim3 grid(p.n), block(kExactWave);
    if (entries == TPL_NTUPLE_ENTRIES) hipLaunchKernelGGL(ntuple_exact_kernel, grid, block, stack, (hipStream_t)stream, p);
    else if (entries == TPL_NTUPLE_ENTRIES_3X3) hipLaunchKernelGGL(ntuple_exact3_kernel, grid, block, stack, (hipStream_t)stream, p);
    else if (entries == TPL_NTUPLE_ENTRIES_FEAT) hipLaunchKernelGGL(ntuple_exact_feature_kernel, grid, block, stack, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(ntuple_exact_budget_kernel, grid, block, stack, (hipStream_t)stream, p);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}
