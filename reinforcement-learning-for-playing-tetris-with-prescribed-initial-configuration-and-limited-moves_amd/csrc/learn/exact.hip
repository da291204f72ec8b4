// exact.hip -- an exact depth-first solver for prescribed configurations: tpl_placement_exact (include/tpl_learn.h states the rule).
//
// tpl_placement_solve_bound is a beam: its width cut is what keeps it from being a proof.  This kernel searches the same game with
// the same children -- solve.hip's expand() in the bounded form: placed_move, bounded_move, psi with the path's carry,
// placement_score, bounded_value -- depth first, a configuration a wavefront.  The search, its mapping and its stack are tpl_exact.h's;
// this unit's frame is the root as a full reset deals it and the configuration's whole piece list, in dynamic LDS at 80 bytes a move,
// and its order is the linear one.
//
// Built twice: as it stands, placement_exact_kernel on the twelve board features, and through exact_move.hip as
// placement_exact_move_kernel on the fourteen.  Both are units of the BOUNDED form (tpl_placement.h: kUnitBound): the prune is what
// makes the search finite in practice and its proof is the move bound's, so there is no unbounded twin and the entries carry no
// _bound in their names.
//
// Built twice more with TPL_EXACT_LIMITED_UNIT (exact_limited.hip, exact_limited_move.hip): the same frame around the LIMITED search of
// tpl_exact.h, as placement_exact_limited[_move]_kernel behind tpl_placement_exact_limited[_move].  Those are units of their own so
// that the plain kernels are compiled from the text they always were.
#ifndef TPL_PLACEMENT_BOUND_UNIT
#define TPL_PLACEMENT_BOUND_UNIT
#endif
#include "tpl_beam.h"
#include "tpl_exact.h"

namespace tpl_learn {
namespace {

constexpr int kF = kUnitFeatures;

#ifdef TPL_EXACT_LIMITED_UNIT
#define TPL_EXACT_KERNEL TPL_UNIT_PASTE4(placement_exact_limited, TPL_UNIT_FORM, , _kernel)
#define TPL_EXACT_ENTRY TPL_UNIT_PASTE4(tpl_placement_exact_limited, TPL_UNIT_FORM, , )
#define TPL_EXACT_ENTRY_NAME "tpl_placement_exact_limited" TPL_UNIT_FORM_NAME
#else
#define TPL_EXACT_KERNEL TPL_UNIT_PASTE4(placement_exact, TPL_UNIT_FORM, , _kernel)
#define TPL_EXACT_ENTRY TPL_UNIT_PASTE4(tpl_placement_exact, TPL_UNIT_FORM, , )
#define TPL_EXACT_ENTRY_NAME "tpl_placement_exact" TPL_UNIT_FORM_NAME
#endif

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
#ifdef TPL_EXACT_LIMITED_UNIT
// the limited entry's own record: the twin's, the two numbers of the limited search and its seventh output
struct ExactLimitedArgs : ExactArgs {
    uint32_t first_limit;        // in [0, 65535]: the K every budget starts with
    uint32_t growth;             // 0: K + 1 ("add"); 1: max(1, 2 K) ("double")
    int32_t* limit;              // [n]: the K of the last iteration begun
};
using KernelArgs = ExactLimitedArgs;
#else
using KernelArgs = ExactArgs;
#endif

using Order = LinearOrder<kF>;
using Stack = Frame<Order::Carry>;

// One wave a workgroup, bound to eight waves a SIMD (tpl_exact.h says why): 64 VGPRs without scratch in both forms.  Left to itself the
// allocator takes 106 SGPRs, which is seven waves; bound to eight it takes 78 and no VGPR more.  The 32 stacks of a CU are 116 KB of
// its 160 at M = 40; at M = 254 LDS admits seven workgroups a CU.
__global__ __launch_bounds__(kExactWave, 8) void TPL_EXACT_KERNEL(const KernelArgs p) {
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

    const Order order(p.weights, p.spare_weight);
#ifdef TPL_EXACT_LIMITED_UNIT
    const Found f = search<Order, true>(order, stack, s_pieces, s_shape, root, bound, L, M, p.max_nodes, p.shortest, lane,
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

}  // namespace
}  // namespace tpl_learn

using namespace tpl_learn;

extern "C" int TPL_EXACT_ENTRY(const int16_t* rows, const uint8_t* pieces, int64_t n, int32_t L, int32_t M, const float* weights,
                               float spare_weight, int32_t max_nodes, int32_t shortest,
#ifdef TPL_EXACT_LIMITED_UNIT
                               int32_t first_limit, int32_t growth,
#endif
                               uint8_t* solved, uint8_t* proved, int32_t* solution_len, uint8_t* actions, int32_t* bound, uint32_t* nodes,
#ifdef TPL_EXACT_LIMITED_UNIT
                               int32_t* limit,
#endif
                               void* stream) {
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
#ifdef TPL_EXACT_LIMITED_UNIT
    if (const int rc = check_discrepancy(name, first_limit, growth, limit)) return rc;
    p.first_limit = (uint32_t)first_limit; p.growth = (uint32_t)growth; p.limit = limit;
#endif
    p.rows = (const uint16_t*)rows; p.pieces = pieces; p.n = (uint32_t)n;
    p.L = (uint32_t)L; p.M = (uint32_t)M; p.weights = weights; p.spare_weight = spare_weight;
    p.max_nodes = (uint32_t)max_nodes; p.shortest = (uint32_t)shortest;
    p.solved = solved; p.proved = proved; p.solution_len = solution_len; p.actions = actions; p.bound = bound; p.nodes = nodes;
    const size_t stack = sizeof(Stack) * (size_t)p.M;          // at most 20,320 bytes
    hipLaunchKernelGGL(TPL_EXACT_KERNEL, dim3(p.n), dim3(kExactWave), stack, (hipStream_t)stream, p);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}
