// ntuple_window.hip -- the exact depth-first search over the pieces a state's WINDOW shows, its children ordered by an n-tuple table:
// tpl_ntuple_window_prove (include/tpl_learn.h states the rule).
//
// tpl_placement_window_prove (exact_window.hip) proves what the known pieces of a state decide, and its linear weights do one thing:
// they order a node's children.  tpl_ntuple_exact (ntuple_exact.hip) is the root search with that order taken from a table.  This
// unit is the two put together: exact_window.hip's frame -- the packed planes, the horizon H = min(known, rem), the shifted game
// (L - lines, H), the skip mask, the verdicts -- around ntuple_exact.hip's search with shortest = 1, on the configuration whose rows
// are the board's and whose list is window entries 0 .. H - 1 and a 0.  What it writes for a board is byte for byte what
// tpl_ntuple_exact writes for that configuration, so a table trained on a tight pool decides which branch a window proof tries first.
//
// A child made at depth d carries list entry d + 1 as its falling piece, the piece it will play.  A child that runs has
// d + 1 < B <= H <= known, so that entry is a true piece of the episode: no value is read under a piece the agent does not know.
// The order reads the entry before it knows the child's state, so entry H -- index 12 where H = 12 -- is a defined 0 in LDS: the
// frame's list rule (tpl_exact.h: prove_window).
//
// The search, its mapping, its stack record and the frame are tpl_exact.h's.  ONE BOARD PER WAVEFRONT; STATIC LDS: twelve stack records
// of 80 bytes, the shape table and sixteen bytes of pieces.  The order is tpl_exact_table.h's TableOrder, a template over the geometry
// of tpl_ntuple.h reached through ntuple_value<S>; the table stays in global memory, as in ntuple_exact.hip and for the reason that
// header gives.  What stands here is the argument record, the four __global__ kernels, each of which names its geometry, and the entry.
//
// Built once more with TPL_EXACT_LIMITED_UNIT (ntuple_window_limited.hip), as exact.hip is and for its reason: the same frame around the
// LIMITED search of tpl_exact.h, four kernels ntuple_window*_limited_kernel behind tpl_ntuple_window_prove_limited.
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
#define TPL_NTUPLE_WINDOW_ENTRY TPL_UNIT_PASTE4(tpl_ntuple_window_prove, TPL_EXACT_LIMITED, , )
#define TPL_NTUPLE_WINDOW_ENTRY_NAME "tpl_ntuple_window_prove" TPL_EXACT_LIMITED_NAME

struct NTupleWindowArgs {
    const uint4* a;              // [n]: the packed planes
    const uint4* b;
    uint32_t n;
    uint32_t L, M;
    TableOrderArgs order;        // the table, the rewards and gamma
    uint32_t max_nodes;          // in [1, 2^24]
    const uint8_t* skip;         // [n] or NULL: a board with skip != 0 is not searched
    uint8_t* solved;             // [n]
    uint8_t* proved;             // [n]
    int32_t* solution_len;       // [n]
    uint8_t* plan;               // [n][12]
    int32_t* bound;              // [n]: need(board)
    uint32_t* nodes;             // [n]
    uint8_t* horizon;            // [n]: H
    uint8_t* verdict;            // [n]
};
struct NTupleWindowLimitedArgs : LimitedArgs<NTupleWindowArgs> {};   // named, as the kernels' symbols carry the name
using KernelArgs = std::conditional_t<kLimitedUnit, NTupleWindowLimitedArgs, NTupleWindowArgs>;

// one wave a workgroup, each kernel bound to eight waves a SIMD (tpl_exact.h says why; here a trip to L2 is part of every link)
template <typename S>
__device__ __forceinline__ void ntuple_window(const KernelArgs& p) { prove_window<TableOrder<S>, kLimitedUnit>(p); }
__global__ __launch_bounds__(kWindowWave, 8) void TPL_KERNEL(ntuple_window)(const KernelArgs p) { ntuple_window<Shape2x4>(p); }
__global__ __launch_bounds__(kWindowWave, 8) void TPL_KERNEL(ntuple_window3)(const KernelArgs p) { ntuple_window<Shape3x3>(p); }
__global__ __launch_bounds__(kWindowWave, 8) void TPL_KERNEL(ntuple_window_feature)(const KernelArgs p) { ntuple_window<FeatureTable>(p); }
__global__ __launch_bounds__(kWindowWave, 8) void TPL_KERNEL(ntuple_window_budget)(const KernelArgs p) { ntuple_window<BudgetTable>(p); }

}  // namespace
}  // namespace tpl_learn

using namespace tpl_learn;

extern "C" int TPL_NTUPLE_WINDOW_ENTRY(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const int32_t* table,
                                       int64_t entries, float r_line, float r_win, float r_lose, float gamma, int32_t max_nodes,
                                       TPL_LIMITED(int32_t first_limit, int32_t growth,) const uint8_t* skip, uint8_t* solved,
                                       uint8_t* proved, int32_t* solution_len, uint8_t* plan, int32_t* bound, uint32_t* nodes,
                                       TPL_LIMITED(int32_t* limit,) uint8_t* horizon, uint8_t* verdict, void* stream) {
    const char* name = TPL_NTUPLE_WINDOW_ENTRY_NAME;
    // a table of any other entry count is refused first, before any pointer is looked at (tpl_ntuple_exact's message)
    if (const int rc = check_table_form(name, entries)) return rc;
    if (!plane_a || !plane_b || !table || !solved || !proved || !solution_len || !plan || !bound || !nodes || !horizon || !verdict)
        return fail_msg(TPL_ERR_ARG, "%s: null pointer (every argument but skip and the stream is required)", name);
    if (const int rc = check_table_numbers(name, r_line, r_win, r_lose, gamma)) return rc;
    if (const int rc = check_search(name, n, 1, "a workgroup per board: n must stay below 2^31", 1, L, M, max_nodes)) return rc;
    if (((uintptr_t)plane_a & 15u) || ((uintptr_t)plane_b & 15u))
        return fail_msg(TPL_ERR_ARG, "%s: planes must be 16-byte aligned", name);
    if ((uintptr_t)table & 3u) return fail_msg(TPL_ERR_ARG, "%s: table must be 4-byte aligned", name);
    if (const int rc = check_counts(name, solution_len, bound, nodes)) return rc;
    KernelArgs p{};
    if (const int rc = take_limited(name, p TPL_LIMITED(, first_limit, growth, limit))) return rc;
    p.a = (const uint4*)plane_a; p.b = (const uint4*)plane_b; p.n = (uint32_t)n;
    p.L = (uint32_t)L; p.M = (uint32_t)M; p.order = TableOrderArgs{table, r_line, r_win, r_lose, gamma};
    p.max_nodes = (uint32_t)max_nodes; p.skip = skip;
    p.solved = solved; p.proved = proved; p.solution_len = solution_len; p.plan = plan; p.bound = bound; p.nodes = nodes;
    p.horizon = horizon; p.verdict = verdict;
    const auto kernel = entries == TPL_NTUPLE_ENTRIES        ? TPL_KERNEL(ntuple_window)
                        : entries == TPL_NTUPLE_ENTRIES_3X3  ? TPL_KERNEL(ntuple_window3)
                        : entries == TPL_NTUPLE_ENTRIES_FEAT ? TPL_KERNEL(ntuple_window_feature)
                                                             : TPL_KERNEL(ntuple_window_budget);
    hipLaunchKernelGGL(kernel, dim3(p.n), dim3(kWindowWave), 0, (hipStream_t)stream, p);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}
