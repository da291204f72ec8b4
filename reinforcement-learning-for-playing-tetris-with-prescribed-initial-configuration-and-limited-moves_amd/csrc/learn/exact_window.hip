// exact_window.hip -- the exact depth-first search over the pieces a state's WINDOW shows: tpl_placement_window_prove
// (include/tpl_learn.h states the rule).
//
// Every other exact search here reads a configuration's whole piece list, which an agent does not have.  A state does carry pieces:
// its 36-bit window holds known = 12 - moves mod 10 true ones, the falling one first (beam.hip).  A running board of the game (L, M)
// with `lines` cleared after `moves` moves has rem = M - moves moves left, and H = min(known, rem) of them have their piece in the
// window: the HORIZON.  For exact_nodes.hip's search that board is a fresh configuration of the game (L - lines, H) whose piece at
// depth d is window entry d -- so the kernel here shifts as that one does, takes the pieces out of the window instead of a list, and
// runs the same search word for word with shortest = 1.  What the result means depends on H: a win found is a win of the real game
// and a shortest one; no win with H = rem is the move bound's proof that none exists; no win with H < rem says only that none lies
// within the known pieces (the verdicts of include/tpl_learn.h).
//
// The search, its mapping and its stack record are tpl_exact.h's, and the order is exact.hip's linear one.  ONE BOARD PER WAVEFRONT.  No
// path is longer than the twelve window entries, so the stack is twelve records, 960 bytes of STATIC LDS, beside the twelve pieces of
// the window, a byte each.  The wave unpacks its board from the two packed planes the beam kernels take.
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

constexpr int kF = kUnitFeatures;
constexpr int kWindowWave = kExactWave;
constexpr int kWindowDepth = tpl::kWindowEntries;             // 12: the longest horizon, and the plan's width
static_assert(kWindowDepth == TPL_WINDOW_PLAN, "the plan is as wide as the window");

#ifdef TPL_EXACT_LIMITED_UNIT
#define TPL_WINDOW_KERNEL TPL_UNIT_PASTE4(placement_window_prove_limited, TPL_UNIT_FORM, , _kernel)
#define TPL_WINDOW_ENTRY TPL_UNIT_PASTE4(tpl_placement_window_prove_limited, TPL_UNIT_FORM, , )
#define TPL_WINDOW_ENTRY_NAME "tpl_placement_window_prove_limited" TPL_UNIT_FORM_NAME
#else
#define TPL_WINDOW_KERNEL TPL_UNIT_PASTE4(placement_window_prove, TPL_UNIT_FORM, , _kernel)
#define TPL_WINDOW_ENTRY TPL_UNIT_PASTE4(tpl_placement_window_prove, TPL_UNIT_FORM, , )
#define TPL_WINDOW_ENTRY_NAME "tpl_placement_window_prove" TPL_UNIT_FORM_NAME
#endif

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
#ifdef TPL_EXACT_LIMITED_UNIT
// the limited entry's own record: the twin's, the two numbers of the limited search and its ninth output
struct WindowLimitedArgs : WindowArgs {
    uint32_t first_limit;        // in [0, 65535]: the K every budget starts with
    uint32_t growth;             // 0: K + 1 ("add"); 1: max(1, 2 K) ("double")
    int32_t* limit;              // [n]: the K of the last iteration begun, 0 where nothing was searched
};
using KernelArgs = WindowLimitedArgs;
#else
using KernelArgs = WindowArgs;
#endif

using Order = LinearOrder<kF>;
using Stack = Frame<Order::Carry>;

// one wave a workgroup, bound to eight waves a SIMD (tpl_exact.h says why)
__global__ __launch_bounds__(kWindowWave, 8) void TPL_WINDOW_KERNEL(const KernelArgs p) {
    __shared__ Stack stack[kWindowDepth];
    __shared__ tpl::ShapeWord s_shape[32];
    __shared__ uint8_t s_pieces[16];
    const uint32_t lane = threadIdx.x, i = blockIdx.x;         // the grid is n blocks of one wave
    const uint4 A = p.a[i], B = p.b[i];                        // one address for the wave
    tpl::Board at;
    tpl::unpack_board(A, B, at);
    const uint32_t lines = uniform(at.lines), moves = uniform(at.moves), state = uniform(at.state);
    const bool skipped = p.skip != nullptr && uniform(p.skip[i]) != 0u;
    // a board that is not running -- or that no environment of this game holds -- is finished: nothing to search
    const bool live = state == tpl::ST_RUNNING && lines < p.L && moves < p.M;
    const uint32_t known = (uint32_t)tpl::kWindowEntries - moves % (uint32_t)tpl::kWindowStride;
    const uint32_t rem = live ? p.M - moves : 0u;
    const uint32_t H = min(known, rem);                       // 0 for a finished board
    const uint32_t L = live ? p.L - lines : 1u;                // of the shifted game (L - lines, H)

    tpl::Board root;                                           // the board as the root of its shifted game: the same in every lane
#pragma unroll
    for (int x = 0; x < tpl::kCols; ++x) root.c[x] = uniform(at.c[x]);
    fresh_root(root);
    const uint32_t need = live ? need_of(root, L) : 0u;        // need(board): no win is shorter

    const bool last_known = H == rem;                          // the window reaches the end of the game
    if (lane == 0) {                                           // what the search does not decide, before it
        p.bound[i] = (int32_t)need;
        p.horizon[i] = (uint8_t)H;
    }

    Found f;
    f.nodes = 0u; f.length = 0u; f.last = kNoMove; f.capped = false; f.limit = 0u;
    if (live && !skipped) {
        if (lane < 32) s_shape[lane] = tpl::kShapeTable[lane];
        // window entry `lane`, masked as move_board masks it
        const unsigned long long window = ((unsigned long long)at.window_hi << 32) | at.window;
        if (lane < (uint32_t)kWindowDepth) s_pieces[lane] = (uint8_t)((uint32_t)(window >> (3u * lane)) & 7u);
        const Order order(p.weights, p.spare_weight);
#ifdef TPL_EXACT_LIMITED_UNIT
        f = search<Order, true>(order, stack, s_pieces, s_shape, root, need, L, H, p.max_nodes, 1u, lane,
                                Discrepancy{p.first_limit, p.growth});                             // the game (L, H), shortest
#else
        f = search(order, stack, s_pieces, s_shape, root, need, L, H, p.max_nodes, 1u, lane);      // the game (L, H), shortest
#endif
    }
    const bool solved = f.length != 0u, proved = !skipped && !f.capped;
    if (lane == 0) {
        p.solved[i] = solved ? (uint8_t)1 : (uint8_t)0;
        p.proved[i] = proved ? (uint8_t)1 : (uint8_t)0;
        p.solution_len[i] = (int32_t)f.length;
        p.nodes[i] = f.nodes;
        p.verdict[i] = !live || skipped ? (uint8_t)TPL_WINDOW_NONE
                       : solved               ? (uint8_t)TPL_WINDOW_WIN
                       : proved && last_known ? (uint8_t)TPL_WINDOW_LOSS
                                              : (uint8_t)TPL_WINDOW_OPEN;
#ifdef TPL_EXACT_LIMITED_UNIT
        p.limit[i] = (int32_t)f.limit;
#endif
    }
    write_path(stack, f, p.plan + (size_t)i * kWindowDepth, (uint32_t)kWindowDepth, lane);      // the plan
}

}  // namespace
}  // namespace tpl_learn

using namespace tpl_learn;

extern "C" int TPL_WINDOW_ENTRY(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const float* weights,
                                float spare_weight, int32_t max_nodes,
#ifdef TPL_EXACT_LIMITED_UNIT
                                int32_t first_limit, int32_t growth,
#endif
                                const uint8_t* skip, uint8_t* solved, uint8_t* proved, int32_t* solution_len, uint8_t* plan, int32_t* bound,
                                uint32_t* nodes,
#ifdef TPL_EXACT_LIMITED_UNIT
                                int32_t* limit,
#endif
                                uint8_t* horizon, uint8_t* verdict, void* stream) {
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
#ifdef TPL_EXACT_LIMITED_UNIT
    if (const int rc = check_discrepancy(name, first_limit, growth, limit)) return rc;
    p.first_limit = (uint32_t)first_limit; p.growth = (uint32_t)growth; p.limit = limit;
#endif
    p.a = (const uint4*)plane_a; p.b = (const uint4*)plane_b; p.n = (uint32_t)n;
    p.L = (uint32_t)L; p.M = (uint32_t)M; p.weights = weights; p.spare_weight = spare_weight; p.max_nodes = (uint32_t)max_nodes;
    p.skip = skip;
    p.solved = solved; p.proved = proved; p.solution_len = solution_len; p.plan = plan; p.bound = bound; p.nodes = nodes;
    p.horizon = horizon; p.verdict = verdict;
    hipLaunchKernelGGL(TPL_WINDOW_KERNEL, dim3(p.n), dim3(kWindowWave), 0, (hipStream_t)stream, p);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}
