// exact_window.hip -- the exact depth-first search over the pieces a state's WINDOW shows: tpl_placement_window_prove
// (include/tpl_learn.h states the rule).
//
// Every other exact search here reads a configuration's whole piece list, which an agent does not have.  A state does carry pieces:
// its 36-bit window holds known = 12 - moves mod 10 true ones, the falling one first (beam.hip).  A running board of the game (L, M)
// with `lines` cleared after `moves` moves has rem = M - moves moves left, and H = min(known, rem) of them have their piece in the
// window: the HORIZON.  For exact_nodes.hip's search that board is a fresh configuration of the game (L - lines, H) whose piece at
// depth d is window entry d -- so the frame shifts as that one does, takes the pieces out of the window instead of a list, and
// runs the same search word for word with shortest = 1.  What the result means depends on H: a win found is a win of the real game
// and a shortest one; no win with H = rem is the move bound's proof that none exists; no win with H < rem says only that none lies
// within the known pieces (the verdicts of include/tpl_learn.h).
//
// The search, its mapping, its stack record and that frame are tpl_exact.h's: prove_window, ONE BOARD PER WAVEFRONT, which unpacks its
// board from the two packed planes the beam kernels take.  No path is longer than the twelve window entries, so the stack is twelve
// records, 960 bytes of STATIC LDS, beside the shape table and the sixteen bytes of the list.  What stands here is the argument record,
// the kernel, which names exact.hip's linear order, and the entry.
//
// Built twice, as exact.hip is: as it stands on the twelve board features and through exact_window_move.hip on the fourteen.  And
// twice more with TPL_EXACT_LIMITED_UNIT (exact_window_limited.hip, exact_window_limited_move.hip), as exact.hip is and for its reason:
// the same frame around the LIMITED search, placement_window_prove_limited[_move]_kernel behind tpl_placement_window_prove_limited[_move].
#ifndef TPL_PLACEMENT_BOUND_UNIT
#define TPL_PLACEMENT_BOUND_UNIT
#endif
#include "tpl_beam.h"
#include "tpl_exact.h"

namespace tpl_learn {
namespace {

#define TPL_WINDOW_KERNEL TPL_UNIT_PASTE4(placement_window_prove, TPL_EXACT_LIMITED, TPL_UNIT_FORM, _kernel)
#define TPL_WINDOW_ENTRY TPL_UNIT_PASTE4(tpl_placement_window_prove, TPL_EXACT_LIMITED, TPL_UNIT_FORM, )
#define TPL_WINDOW_ENTRY_NAME "tpl_placement_window_prove" TPL_EXACT_LIMITED_NAME TPL_UNIT_FORM_NAME

struct WindowArgs {
    const uint4* a;              // [n]: the packed planes
    const uint4* b;
    uint32_t n;
    uint32_t L, M;
    const float* weights;        // [12], or the first 14 of a row of 16
    float spare_weight;
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
struct WindowLimitedArgs : LimitedArgs<WindowArgs> {};         // named, as the kernel's symbol carries the name
using KernelArgs = std::conditional_t<kLimitedUnit, WindowLimitedArgs, WindowArgs>;

// one wave a workgroup, bound to eight waves a SIMD (tpl_exact.h says why)
__global__ __launch_bounds__(kWindowWave, 8) void TPL_WINDOW_KERNEL(const KernelArgs p) {
    prove_window<LinearOrder<kUnitFeatures>, kLimitedUnit>(p);
}

}  // namespace
}  // namespace tpl_learn

using namespace tpl_learn;

extern "C" int TPL_WINDOW_ENTRY(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const float* weights,
                                float spare_weight, int32_t max_nodes, TPL_LIMITED(int32_t first_limit, int32_t growth,)
                                const uint8_t* skip, uint8_t* solved, uint8_t* proved, int32_t* solution_len, uint8_t* plan, int32_t* bound,
                                uint32_t* nodes, TPL_LIMITED(int32_t* limit,) uint8_t* horizon, uint8_t* verdict, void* stream) {
    const char* name = TPL_WINDOW_ENTRY_NAME;
    if (!plane_a || !plane_b || !weights || !solved || !proved || !solution_len || !plan || !bound || !nodes || !horizon || !verdict)
        return fail_msg(TPL_ERR_ARG, "%s: null pointer (every argument but skip and the stream is required)", name);
    if (!(spare_weight - spare_weight == 0.0f)) return fail_msg(TPL_ERR_ARG, "%s: spare_weight must be finite", name);
    if (const int rc = check_search(name, n, 1, "a workgroup per board: n must stay below 2^31", 1, L, M, max_nodes)) return rc;
    if (((uintptr_t)plane_a & 15u) || ((uintptr_t)plane_b & 15u))
        return fail_msg(TPL_ERR_ARG, "%s: planes must be 16-byte aligned", name);
    if ((uintptr_t)weights & 15u) return fail_msg(TPL_ERR_ARG, "%s: weights must be 16-byte aligned", name);
    if (const int rc = check_counts(name, solution_len, bound, nodes)) return rc;
    KernelArgs p{};
    if (const int rc = take_limited(name, p TPL_LIMITED(, first_limit, growth, limit))) return rc;
    p.a = (const uint4*)plane_a; p.b = (const uint4*)plane_b; p.n = (uint32_t)n;
    p.L = (uint32_t)L; p.M = (uint32_t)M; p.weights = weights; p.spare_weight = spare_weight; p.max_nodes = (uint32_t)max_nodes;
    p.skip = skip;
    p.solved = solved; p.proved = proved; p.solution_len = solution_len; p.plan = plan; p.bound = bound; p.nodes = nodes;
    p.horizon = horizon; p.verdict = verdict;
    hipLaunchKernelGGL(TPL_WINDOW_KERNEL, dim3(p.n), dim3(kWindowWave), 0, (hipStream_t)stream, p);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}
