// ntuple_exact.hip -- the exact depth-first solver with its children ordered by an n-tuple table: tpl_ntuple_exact (include/tpl_learn.h
// states the rule).
//
// tpl_placement_exact (exact.hip) searches the whole game of a prescribed configuration depth first, and its linear weights do one
// thing: they order a node's children.  This unit is that search with the order taken from a table instead -- a child is worth
// reward + gamma V(afterstate), what the one-ply n-tuple policy scores a first move with, read in the game (L, B) of the iteration --
// so that a table trained on a tight pool decides which branch a proof tries first.  The children, the stop, the descent, the node
// cap and the budgets are exact.hip's, and so is what a finished search says: the order decides how many nodes a proof takes.
//
// The search, its mapping and its stack are tpl_exact.h's: ONE CONFIGURATION PER WAVEFRONT, the stack in dynamic LDS at 80 bytes a move.
// This unit's order carries nothing along a path -- a table's value reads the board alone -- and a child made again on the return is
// made without its value.
//
// The table is read from global memory, where it stays: a child's V is eleven gathers under a budget table and ten under a feature
// table (84 and 76 KB, which sit in L2), and up to 154 and 145 under the window forms -- the non-empty windows of the board.  One wave
// a workgroup cannot afford a copy in LDS.  The order is a template over the geometry of tpl_ntuple.h, reached through ntuple_value<S>,
// and each __global__ kernel names its geometry, as ntuple.hip's do.  The budget geometry hands ntuple_value the board and (L, B);
// prune_dead is not called: bounded_move has already turned a dead child lost.
//
// Built once more with TPL_EXACT_LIMITED_UNIT (ntuple_exact_limited.hip), as exact.hip is and for its reason: the same frame around the
// LIMITED search of tpl_exact.h, four kernels ntuple_exact*_limited_kernel behind tpl_ntuple_exact_limited.
#ifndef TPL_PLACEMENT_BOUND_UNIT
#define TPL_PLACEMENT_BOUND_UNIT
#endif
#include "tpl_beam.h"
#include "tpl_exact.h"
#include "tpl_ntuple.h"

namespace tpl_learn {
namespace {

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
#ifdef TPL_EXACT_LIMITED_UNIT
// the limited entry's own record: the twin's, the two numbers of the limited search and its seventh output
struct NTupleExactLimitedArgs : NTupleExactArgs {
    uint32_t first_limit;        // in [0, 65535]: the K every budget starts with
    uint32_t growth;             // 0: K + 1 ("add"); 1: max(1, 2 K) ("double")
    int32_t* limit;              // [n]: the K of the last iteration begun
};
using KernelArgs = NTupleExactLimitedArgs;
#define TPL_KERNEL(stem) stem##_limited_kernel
#define TPL_NTUPLE_EXACT_ENTRY tpl_ntuple_exact_limited
#define TPL_NTUPLE_EXACT_ENTRY_NAME "tpl_ntuple_exact_limited"
#else
using KernelArgs = NTupleExactArgs;
#define TPL_KERNEL(stem) stem##_kernel
#define TPL_NTUPLE_EXACT_ENTRY tpl_ntuple_exact
#define TPL_NTUPLE_EXACT_ENTRY_NAME "tpl_ntuple_exact"
#endif

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

// The table's order: the board the move leaves, dead turned lost, with the piece the child will play as its falling piece, worth what
// the one-ply policy scores the move with.  The table, the rewards and gamma are read from the kernel's arguments, which are SGPRs.
template <typename S>
struct TableOrder {
    using Carry = NoCarry;       // a table's value reads the board alone
    const NTupleExactArgs& p;
    __device__ __forceinline__ float child(const Frame<Carry>& node, uint32_t cur, const uint8_t* later, uint32_t r, uint32_t l,
                                           const tpl::ShapeWord* shape, uint32_t L, uint32_t B, tpl::Board& s, Carry&) const {
        tpl::unpack_board(node.a, node.b, s);
        s.window = cur;
        s.window_hi = 0u;
        const uint32_t n_clear = placed_move<kFeatures>(s, shape, r, l, L, B);
        bounded_move(s, L, B);
        s.window = uniform(later[0]);                          // depth d + 1 <= M: the list has M + 1 entries
        return child_value<S>(s, n_clear, L, B, p);
    }
};
using Stack = Frame<NoCarry>;

// A wave's search is one long dependent chain, and here a trip to L2 or beyond is part of every link -- the table's gathers --, so what
// hides it is other waves.
template <typename S>
__device__ __forceinline__ void ntuple_exact(const KernelArgs& p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    Stack* const stack = reinterpret_cast<Stack*>(s_raw);      // [M]
    __shared__ tpl::ShapeWord s_shape[32];
    __shared__ uint8_t s_pieces[kExactMaxMoves + 2];
    const uint32_t lane = threadIdx.x, i = blockIdx.x;         // the grid is n blocks of one wave
    const uint32_t L = p.L, M = p.M;
    if (lane < 32) s_shape[lane] = tpl::kShapeTable[lane];
    load_pieces(s_pieces, p.pieces, (size_t)i * (M + 1u), M, lane);

    tpl::Board root;                                           // the root, as a full reset deals it: the same in every lane
    tpl::rows_to_cols(p.rows + (size_t)i * tpl::kRows, root.c);
    fresh_root(root);
    const uint32_t bound = need_of(root, L);

    const TableOrder<S> order{p};
#ifdef TPL_EXACT_LIMITED_UNIT
    const Found f = search<TableOrder<S>, true>(order, stack, s_pieces, s_shape, root, bound, L, M, p.max_nodes, p.shortest, lane,
                                                Discrepancy{p.first_limit, p.growth});
#else
    const Found f = search(order, stack, s_pieces, s_shape, root, bound, L, M, p.max_nodes, p.shortest, lane);
#endif
    if (lane == 0) {
        p.solved[i] = f.length != 0u ? (uint8_t)1 : (uint8_t)0;
        p.proved[i] = f.capped ? (uint8_t)0 : (uint8_t)1;
        p.solution_len[i] = (int32_t)f.length;
        p.bound[i] = (int32_t)bound;
        p.nodes[i] = f.nodes;
#ifdef TPL_EXACT_LIMITED_UNIT
        p.limit[i] = (int32_t)f.limit;
#endif
    }
    write_path(stack, f, p.actions + (size_t)i * M, M, lane);
}

// One wave a workgroup, each kernel bound to eight waves a SIMD, which every geometry fits without scratch: 55 VGPRs ("2x4"), 52
// ("3x3"), 59 ("feat") and 60 ("feat+spare") of the 64 the bound allows, 78 SGPRs (tools/kernel_resources.sh;
// profiles/learner/ntuple_exact_isa.log).
__global__ __launch_bounds__(kExactWave, 8) void TPL_KERNEL(ntuple_exact)(const KernelArgs p) { ntuple_exact<Shape2x4>(p); }
__global__ __launch_bounds__(kExactWave, 8) void TPL_KERNEL(ntuple_exact3)(const KernelArgs p) { ntuple_exact<Shape3x3>(p); }
__global__ __launch_bounds__(kExactWave, 8) void TPL_KERNEL(ntuple_exact_feature)(const KernelArgs p) { ntuple_exact<FeatureTable>(p); }
__global__ __launch_bounds__(kExactWave, 8) void TPL_KERNEL(ntuple_exact_budget)(const KernelArgs p) { ntuple_exact<BudgetTable>(p); }

}  // namespace
}  // namespace tpl_learn

using namespace tpl_learn;

extern "C" int TPL_NTUPLE_EXACT_ENTRY(const int16_t* rows, const uint8_t* pieces, int64_t n, int32_t L, int32_t M, const int32_t* table,
                                      int64_t entries, float r_line, float r_win, float r_lose, float gamma, int32_t max_nodes,
                                      int32_t shortest,
#ifdef TPL_EXACT_LIMITED_UNIT
                                      int32_t first_limit, int32_t growth,
#endif
                                      uint8_t* solved, uint8_t* proved, int32_t* solution_len, uint8_t* actions, int32_t* bound,
                                      uint32_t* nodes,
#ifdef TPL_EXACT_LIMITED_UNIT
                                      int32_t* limit,
#endif
                                      void* stream) {
    const char* name = TPL_NTUPLE_EXACT_ENTRY_NAME;
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
    if (const int rc = check_search(name, n, 1, "a workgroup per configuration: n must stay below 2^31", 1, L, M, max_nodes)) return rc;
    if (shortest != 0 && shortest != 1) return fail_msg(TPL_ERR_ARG, "%s: shortest must be 0 or 1", name);
    if ((uintptr_t)rows & 1u) return fail_msg(TPL_ERR_ARG, "%s: rows must be 2-byte aligned", name);
    if ((uintptr_t)table & 3u) return fail_msg(TPL_ERR_ARG, "%s: table must be 4-byte aligned", name);
    if (const int rc = check_counts(name, solution_len, bound, nodes)) return rc;
    KernelArgs p{};
#ifdef TPL_EXACT_LIMITED_UNIT
    if (const int rc = check_discrepancy(name, first_limit, growth, limit)) return rc;
    p.first_limit = (uint32_t)first_limit; p.growth = (uint32_t)growth; p.limit = limit;
#endif
    p.rows = (const uint16_t*)rows; p.pieces = pieces; p.n = (uint32_t)n;
    p.L = (uint32_t)L; p.M = (uint32_t)M; p.table = table;
    p.r_line = r_line; p.r_win = r_win; p.r_lose = r_lose; p.gamma = gamma;
    p.max_nodes = (uint32_t)max_nodes; p.shortest = (uint32_t)shortest;
    p.solved = solved; p.proved = proved; p.solution_len = solution_len; p.actions = actions; p.bound = bound; p.nodes = nodes;
    const size_t stack = sizeof(Stack) * (size_t)p.M;          // at most 20,320 bytes
    const dim3 grid(p.n), block(kExactWave);
    if (entries == TPL_NTUPLE_ENTRIES) hipLaunchKernelGGL(TPL_KERNEL(ntuple_exact), grid, block, stack, (hipStream_t)stream, p);
    else if (entries == TPL_NTUPLE_ENTRIES_3X3) hipLaunchKernelGGL(TPL_KERNEL(ntuple_exact3), grid, block, stack, (hipStream_t)stream, p);
    else if (entries == TPL_NTUPLE_ENTRIES_FEAT)
        hipLaunchKernelGGL(TPL_KERNEL(ntuple_exact_feature), grid, block, stack, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(TPL_KERNEL(ntuple_exact_budget), grid, block, stack, (hipStream_t)stream, p);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}
