// ntuple_exact.hip -- the exact depth-first solver with its children ordered by an n-tuple table: tpl_ntuple_exact (include/tpl_learn.h
// states the rule).
//
// tpl_placement_exact (exact.hip) searches the whole game of a prescribed configuration depth first, and its linear weights do one
// thing: they order a node's children.  This unit is that search with the order taken from a table instead -- a child is worth
// reward + gamma V(afterstate), what the one-ply n-tuple policy scores a first move with, read in the game (L, B) of the iteration --
// so that a table trained on a tight pool decides which branch a proof tries first.  The children, the stop, the descent, the node
// cap and the budgets are exact.hip's, and so is what a finished search says: the order decides how many nodes a proof takes.
//
// The search, its mapping, its stack and the frame are tpl_exact.h's, the frame exact.hip's: prove_root, ONE CONFIGURATION PER
// WAVEFRONT, the stack in dynamic LDS at 80 bytes a move.  The order is tpl_exact_table.h's TableOrder, a template over the geometry of
// tpl_ntuple.h reached through ntuple_value<S>, and it says why the table stays in global memory.  What stands here is the argument
// record, the four __global__ kernels, each of which names its geometry as ntuple.hip's do, and the entry.
//
// Built once more with TPL_EXACT_LIMITED_UNIT (ntuple_exact_limited.hip), as exact.hip is and for its reason: the same frame around the
// LIMITED search of tpl_exact.h, four kernels ntuple_exact*_limited_kernel behind tpl_ntuple_exact_limited.
#ifndef TPL_PLACEMENT_BOUND_UNIT
#define TPL_PLACEMENT_BOUND_UNIT
#endif
#include "tpl_beam.h"
#include "tpl_exact.h"
#include "tpl_ntuple.h"
#include "tpl_exact_table.h"

namespace tpl_learn {
namespace {

#define TPL_KERNEL(stem) TPL_UNIT_PASTE4(stem, TPL_EXACT_LIMITED, _kernel, )
#define TPL_NTUPLE_EXACT_ENTRY TPL_UNIT_PASTE4(tpl_ntuple_exact, TPL_EXACT_LIMITED, , )
#define TPL_NTUPLE_EXACT_ENTRY_NAME "tpl_ntuple_exact" TPL_EXACT_LIMITED_NAME

struct NTupleExactArgs {
    const uint16_t* rows;        // [n][20], bit x = column x
    const uint8_t* pieces;       // [n][M + 1]
    uint32_t n;                  // configurations = workgroups of one wave
    uint32_t L, M;
    TableOrderArgs order;        // the table, the rewards and gamma
    uint32_t max_nodes;          // in [1, 2^24]
    uint32_t shortest;           // 1: budgets need(root) .. M; 0: M alone
    uint8_t* solved;             // [n]
    uint8_t* proved;             // [n]
    int32_t* solution_len;       // [n]
    uint8_t* actions;            // [n][M]
    int32_t* bound;              // [n]: need(root)
    uint32_t* nodes;             // [n]: expansions, all iterations
};
struct NTupleExactLimitedArgs : LimitedArgs<NTupleExactArgs> {};   // named, as the kernels' symbols carry the name
using KernelArgs = std::conditional_t<kLimitedUnit, NTupleExactLimitedArgs, NTupleExactArgs>;
using Stack = Frame<NoCarry>;

// A wave's search is one long dependent chain, and here a trip to L2 or beyond is part of every link -- the table's gathers --, so what
// hides it is other waves.  One wave a workgroup, each kernel bound to eight waves a SIMD, which every geometry fits without scratch:
// 55 VGPRs ("2x4"), 52 ("3x3"), 59 ("feat") and 60 ("feat+spare") of the 64 the bound allows, 78 SGPRs (tools/kernel_resources.sh;
// profiles/learner/ntuple_exact_isa.log).
template <typename S>
__device__ __forceinline__ void ntuple_exact(const KernelArgs& p) { prove_root<TableOrder<S>, kLimitedUnit>(p); }
__global__ __launch_bounds__(kExactWave, 8) void TPL_KERNEL(ntuple_exact)(const KernelArgs p) { ntuple_exact<Shape2x4>(p); }
__global__ __launch_bounds__(kExactWave, 8) void TPL_KERNEL(ntuple_exact3)(const KernelArgs p) { ntuple_exact<Shape3x3>(p); }
__global__ __launch_bounds__(kExactWave, 8) void TPL_KERNEL(ntuple_exact_feature)(const KernelArgs p) { ntuple_exact<FeatureTable>(p); }
__global__ __launch_bounds__(kExactWave, 8) void TPL_KERNEL(ntuple_exact_budget)(const KernelArgs p) { ntuple_exact<BudgetTable>(p); }

}  // namespace
}  // namespace tpl_learn

using namespace tpl_learn;

extern "C" int TPL_NTUPLE_EXACT_ENTRY(const int16_t* rows, const uint8_t* pieces, int64_t n, int32_t L, int32_t M, const int32_t* table,
                                      int64_t entries, float r_line, float r_win, float r_lose, float gamma, int32_t max_nodes,
                                      int32_t shortest, TPL_LIMITED(int32_t first_limit, int32_t growth,) uint8_t* solved,
                                      uint8_t* proved, int32_t* solution_len, uint8_t* actions, int32_t* bound, uint32_t* nodes,
                                      TPL_LIMITED(int32_t* limit,) void* stream) {
    const char* name = TPL_NTUPLE_EXACT_ENTRY_NAME;
    // a table of any other entry count is refused first, before any pointer is looked at
    if (const int rc = check_table_form(name, entries)) return rc;
    if (!rows || !pieces || !table || !solved || !proved || !solution_len || !actions || !bound || !nodes)
        return fail_msg(TPL_ERR_ARG, "%s: null pointer (every argument but the stream is required)", name);
    if (const int rc = check_table_numbers(name, r_line, r_win, r_lose, gamma)) return rc;
    if (const int rc = check_search(name, n, 1, "a workgroup per configuration: n must stay below 2^31", 1, L, M, max_nodes)) return rc;
    if (shortest != 0 && shortest != 1) return fail_msg(TPL_ERR_ARG, "%s: shortest must be 0 or 1", name);
    if ((uintptr_t)rows & 1u) return fail_msg(TPL_ERR_ARG, "%s: rows must be 2-byte aligned", name);
    if ((uintptr_t)table & 3u) return fail_msg(TPL_ERR_ARG, "%s: table must be 4-byte aligned", name);
    if (const int rc = check_counts(name, solution_len, bound, nodes)) return rc;
    KernelArgs p{};
    if (const int rc = take_limited(name, p TPL_LIMITED(, first_limit, growth, limit))) return rc;
    p.rows = (const uint16_t*)rows; p.pieces = pieces; p.n = (uint32_t)n;
    p.L = (uint32_t)L; p.M = (uint32_t)M; p.order = TableOrderArgs{table, r_line, r_win, r_lose, gamma};
    p.max_nodes = (uint32_t)max_nodes; p.shortest = (uint32_t)shortest;
    p.solved = solved; p.proved = proved; p.solution_len = solution_len; p.actions = actions; p.bound = bound; p.nodes = nodes;
    const size_t stack = sizeof(Stack) * (size_t)p.M;          // at most 20,320 bytes
    const auto kernel = entries == TPL_NTUPLE_ENTRIES        ? TPL_KERNEL(ntuple_exact)
                        : entries == TPL_NTUPLE_ENTRIES_3X3  ? TPL_KERNEL(ntuple_exact3)
                        : entries == TPL_NTUPLE_ENTRIES_FEAT ? TPL_KERNEL(ntuple_exact_feature)
                                                             : TPL_KERNEL(ntuple_exact_budget);
    hipLaunchKernelGGL(kernel, dim3(p.n), dim3(kExactWave), stack, (hipStream_t)stream, p);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}
