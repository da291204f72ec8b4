// exact.hip -- an exact depth-first solver for prescribed configurations: tpl_placement_exact (include/tpl_learn.h states the rule).
//
// tpl_placement_solve_bound is a beam: its width cut is what keeps it from being a proof.  This kernel searches the same game with
// the same children -- solve.hip's expand() in the bounded form: placed_move, bounded_move, psi with the path's carry,
// placement_score, bounded_value -- depth first, a configuration a wavefront.  The search, its mapping, its stack and the frame
// around it are tpl_exact.h's: prove_root, the root as a full reset deals it and the configuration's whole piece list, the stack in
// dynamic LDS at 80 bytes a move.  What stands here is the argument record, the kernel, which names the linear order, and the entry.
//
// Built twice: as it stands, placement_exact_kernel on the twelve board features, and through exact_move.hip as
// placement_exact_move_kernel on the fourteen.  Both are units of the BOUNDED form (tpl_placement.h: kUnitBound): the prune is what
// makes the search finite in practice and its proof is the move bound's, so there is no unbounded twin and the entries carry no
// _bound in their names.
//
// Built twice more with TPL_EXACT_LIMITED_UNIT (exact_limited.hip, exact_limited_move.hip): the same frame around the LIMITED search of
// tpl_exact.h, as placement_exact_limited[_move]_kernel behind tpl_placement_exact_limited[_move].  Those are units of their own so
// that the plain kernels' code stays apart from theirs; tpl_exact.h says what the macro chooses.
#ifndef TPL_PLACEMENT_BOUND_UNIT
#define TPL_PLACEMENT_BOUND_UNIT
#endif
#include "tpl_beam.h"
#include "tpl_exact.h"

namespace tpl_learn {
namespace {

#define TPL_EXACT_KERNEL TPL_UNIT_PASTE4(placement_exact, TPL_EXACT_LIMITED, TPL_UNIT_FORM, _kernel)
#define TPL_EXACT_ENTRY TPL_UNIT_PASTE4(tpl_placement_exact, TPL_EXACT_LIMITED, TPL_UNIT_FORM, )
#define TPL_EXACT_ENTRY_NAME "tpl_placement_exact" TPL_EXACT_LIMITED_NAME TPL_UNIT_FORM_NAME

struct ExactArgs {
    const uint16_t* rows;        // [n][20], bit x = column x
    const uint8_t* pieces;       // [n][M + 1]
    uint32_t n;                  // configurations = workgroups of one wave
    uint32_t L, M;
    const float* weights;        // [12], or the first 14 of a row of 16
    float spare_weight;
    uint32_t max_nodes;          // in [1, 2^24]
    uint32_t shortest;           // 1: budgets need(root) .. M; 0: M alone
    uint8_t* solved;             // [n]
    uint8_t* proved;             // [n]
    int32_t* solution_len;       // [n]
    uint8_t* actions;            // [n][M]
    int32_t* bound;              // [n]: need(root)
    uint32_t* nodes;             // [n]: expansions, all iterations
};
struct ExactLimitedArgs : LimitedArgs<ExactArgs> {};           // named, as the kernel's symbol carries the name
using KernelArgs = std::conditional_t<kLimitedUnit, ExactLimitedArgs, ExactArgs>;

using Order = LinearOrder<kUnitFeatures>;
using Stack = Frame<Order::Carry>;

// One wave a workgroup, bound to eight waves a SIMD (tpl_exact.h says why): 64 VGPRs without scratch in both forms.  Left to itself the
// allocator takes 106 SGPRs, which is seven waves; bound to eight it takes 78 and no VGPR more.  The 32 stacks of a CU are 116 KB of
// its 160 at M = 40; at M = 254 LDS admits seven workgroups a CU.
__global__ __launch_bounds__(kExactWave, 8) void TPL_EXACT_KERNEL(const KernelArgs p) {
    prove_root<Order, kLimitedUnit>(p);
}

}  // namespace
}  // namespace tpl_learn

using namespace tpl_learn;

extern "C" int TPL_EXACT_ENTRY(const int16_t* rows, const uint8_t* pieces, int64_t n, int32_t L, int32_t M, const float* weights,
                               float spare_weight, int32_t max_nodes, int32_t shortest, TPL_LIMITED(int32_t first_limit, int32_t growth,)
                               uint8_t* solved, uint8_t* proved, int32_t* solution_len, uint8_t* actions, int32_t* bound, uint32_t* nodes,
                               TPL_LIMITED(int32_t* limit,) void* stream) {
    const char* name = TPL_EXACT_ENTRY_NAME;
    if (!rows || !pieces || !weights || !solved || !proved || !solution_len || !actions || !bound || !nodes)
        return fail_msg(TPL_ERR_ARG, "%s: null pointer (every argument but the stream is required)", name);
    if (!(spare_weight - spare_weight == 0.0f)) return fail_msg(TPL_ERR_ARG, "%s: spare_weight must be finite", name);
    if (const int rc = check_search(name, n, 1, "a workgroup per configuration: n must stay below 2^31", 1, L, M, max_nodes)) return rc;
    if (shortest != 0 && shortest != 1) return fail_msg(TPL_ERR_ARG, "%s: shortest must be 0 or 1", name);
    if ((uintptr_t)rows & 1u) return fail_msg(TPL_ERR_ARG, "%s: rows must be 2-byte aligned", name);
    if ((uintptr_t)weights & 15u) return fail_msg(TPL_ERR_ARG, "%s: weights must be 16-byte aligned", name);
    if (const int rc = check_counts(name, solution_len, bound, nodes)) return rc;
    KernelArgs p{};
    if (const int rc = take_limited(name, p TPL_LIMITED(, first_limit, growth, limit))) return rc;
    p.rows = (const uint16_t*)rows; p.pieces = pieces; p.n = (uint32_t)n;
    p.L = (uint32_t)L; p.M = (uint32_t)M; p.weights = weights; p.spare_weight = spare_weight;
    p.max_nodes = (uint32_t)max_nodes; p.shortest = (uint32_t)shortest;
    p.solved = solved; p.proved = proved; p.solution_len = solution_len; p.actions = actions; p.bound = bound; p.nodes = nodes;
    const size_t stack = sizeof(Stack) * (size_t)p.M;          // at most 20,320 bytes
    hipLaunchKernelGGL(TPL_EXACT_KERNEL, dim3(p.n), dim3(kExactWave), stack, (hipStream_t)stream, p);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}
