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
// The order reads the entry before it knows the child's state, so entry H -- index 12 where H = 12 -- is a defined 0 in LDS.
//
// The search, its mapping and its stack record are tpl_exact.h's.  ONE BOARD PER WAVEFRONT; STATIC LDS: twelve stack records of 80 bytes,
// the shape table and sixteen bytes of pieces.  The table stays in global memory, as in ntuple_exact.hip and for its reason.  The order
// is a template over the geometry of tpl_ntuple.h and each __global__ kernel names its geometry.
//
// Built once more with TPL_EXACT_LIMITED_UNIT (ntuple_window_limited.hip), as exact.hip is and for its reason: the same frame around the
// LIMITED search of tpl_exact.h, four kernels ntuple_window*_limited_kernel behind tpl_ntuple_window_prove_limited.
#ifndef TPL_PLACEMENT_BOUND_UNIT
#define TPL_PLACEMENT_BOUND_UNIT
#endif
#include "tpl_beam.h"
#include "tpl_exact.h"
#include "tpl_ntuple.h"

namespace tpl_learn {
namespace {

constexpr int kWindowWave = kExactWave;
constexpr int kWindowDepth = tpl::kWindowEntries;             // 12: the longest horizon, and the plan's width
constexpr int kWindowList = 16;                               // the list in LDS: entries 0 .. H - 1 of the window, 0 behind them
static_assert(kWindowDepth == TPL_WINDOW_PLAN, "the plan is as wide as the window");
static_assert(kWindowDepth < kWindowList, "entry 12 of the list exists");

struct NTupleWindowArgs {
    const uint4* a;              // [n]: the packed planes
    const uint4* b;
    uint32_t n;
    uint32_t L, M;
    const int32_t* table;        // of the kernel's geometry
    float r_line, r_win, r_lose, gamma;
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
struct NTupleWindowLimitedArgs : NTupleWindowArgs {
    uint32_t first_limit;        // in [0, 65535]: the K every budget starts with
    uint32_t growth;             // 0: K + 1 ("add"); 1: max(1, 2 K) ("double")
    int32_t* limit;              // [n]: the K of the last iteration begun, 0 where nothing was searched
};
using KernelArgs = NTupleWindowLimitedArgs;
#define TPL_KERNEL(stem) stem##_limited_kernel
#define TPL_NTUPLE_WINDOW_ENTRY tpl_ntuple_window_prove_limited
#define TPL_NTUPLE_WINDOW_ENTRY_NAME "tpl_ntuple_window_prove_limited"
#else
using KernelArgs = NTupleWindowArgs;
#define TPL_KERNEL(stem) stem##_kernel
#define TPL_NTUPLE_WINDOW_ENTRY tpl_ntuple_window_prove
#define TPL_NTUPLE_WINDOW_ENTRY_NAME "tpl_ntuple_window_prove"
#endif

// what the one-ply policy scores the move with: reward, or reward + gamma V where the child runs; every product and sum rounded once
template <typename S>
__device__ __forceinline__ float child_value(const tpl::Board& s, uint32_t n_clear, uint32_t L, uint32_t B, const NTupleWindowArgs& p) {
#pragma clang fp contract(off)
    const bool on = s.state == tpl::ST_RUNNING;
    float v = 0.0f;
    if (on) v = ntuple_value<S>(s, L, B, p.table);
    const float reward = move_reward(p.r_line, p.r_win, p.r_lose, n_clear, s.state);
    const float later = p.gamma * v;
    return on ? reward + later : reward;
}

// The table's order, as ntuple_exact.hip has it: the board the move leaves, dead turned lost, with the piece the child will play as its
// falling piece, worth what the one-ply policy scores the move with.  The table, the rewards and gamma are kernel arguments: SGPRs.
template <typename S>
struct TableOrder {
    using Carry = NoCarry;       // a table's value reads the board alone
    const NTupleWindowArgs& p;
    __device__ __forceinline__ float child(const Frame<Carry>& node, uint32_t cur, const uint8_t* later, uint32_t r, uint32_t l,
                                           const tpl::ShapeWord* shape, uint32_t L, uint32_t B, tpl::Board& s, Carry&) const {
        tpl::unpack_board(node.a, node.b, s);
        s.window = cur;
        s.window_hi = 0u;
        const uint32_t n_clear = placed_move<kFeatures>(s, shape, r, l, L, B);
        bounded_move(s, L, B);
        s.window = uniform(later[0]);                          // depth d + 1 <= H <= 12: the list has 16 entries
        return child_value<S>(s, n_clear, L, B, p);
    }
};
using Stack = Frame<NoCarry>;

template <typename S>
__device__ __forceinline__ void ntuple_window(const KernelArgs& p) {
    __shared__ Stack stack[kWindowDepth];
    __shared__ tpl::ShapeWord s_shape[32];
    __shared__ uint8_t s_pieces[kWindowList];
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
        // list entry `lane`: the window's, masked as move_board masks it, below the horizon and 0 from it on
        const unsigned long long window = ((unsigned long long)at.window_hi << 32) | at.window;
        if (lane < (uint32_t)kWindowList) s_pieces[lane] = lane < H ? (uint8_t)((uint32_t)(window >> (3u * lane)) & 7u) : (uint8_t)0;
        const TableOrder<S> order{p};
#ifdef TPL_EXACT_LIMITED_UNIT
        f = search<TableOrder<S>, true>(order, stack, s_pieces, s_shape, root, need, L, H, p.max_nodes, 1u, lane,
                                        Discrepancy{p.first_limit, p.growth});                     // the game (L, H), shortest
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

// one wave a workgroup, each kernel bound to eight waves a SIMD (tpl_exact.h says why; here a trip to L2 is part of every link)
__global__ __launch_bounds__(kWindowWave, 8) void TPL_KERNEL(ntuple_window)(const KernelArgs p) { ntuple_window<Shape2x4>(p); }
__global__ __launch_bounds__(kWindowWave, 8) void TPL_KERNEL(ntuple_window3)(const KernelArgs p) { ntuple_window<Shape3x3>(p); }
__global__ __launch_bounds__(kWindowWave, 8) void TPL_KERNEL(ntuple_window_feature)(const KernelArgs p) { ntuple_window<FeatureTable>(p); }
__global__ __launch_bounds__(kWindowWave, 8) void TPL_KERNEL(ntuple_window_budget)(const KernelArgs p) { ntuple_window<BudgetTable>(p); }

}  // namespace
}  // namespace tpl_learn

using namespace tpl_learn;

extern "C" int TPL_NTUPLE_WINDOW_ENTRY(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const int32_t* table,
                                       int64_t entries, float r_line, float r_win, float r_lose, float gamma, int32_t max_nodes,
#ifdef TPL_EXACT_LIMITED_UNIT
                                       int32_t first_limit, int32_t growth,
#endif
                                       const uint8_t* skip, uint8_t* solved, uint8_t* proved, int32_t* solution_len, uint8_t* plan,
                                       int32_t* bound, uint32_t* nodes,
#ifdef TPL_EXACT_LIMITED_UNIT
                                       int32_t* limit,
#endif
                                       uint8_t* horizon, uint8_t* verdict, void* stream) {
    const char* name = TPL_NTUPLE_WINDOW_ENTRY_NAME;
    // a table of any other entry count is refused first, before any pointer is looked at (tpl_ntuple_exact's message)
    if (entries != TPL_NTUPLE_ENTRIES && entries != TPL_NTUPLE_ENTRIES_3X3 && entries != TPL_NTUPLE_ENTRIES_FEAT &&
        entries != TPL_NTUPLE_ENTRIES_BUDGET)
        return fail_msg(TPL_ERR_ARG,
                        "%s: entries must be %d (\"2x4\"), %d (\"3x3\"), %d (\"feat\") or %d (\"feat+spare\"), the four plain forms -- a sum "
                        "or a staged table orders no search --, got %lld",
                        name, (int)TPL_NTUPLE_ENTRIES, (int)TPL_NTUPLE_ENTRIES_3X3, (int)TPL_NTUPLE_ENTRIES_FEAT,
                        (int)TPL_NTUPLE_ENTRIES_BUDGET, (long long)entries);
    if (!plane_a || !plane_b || !table || !solved || !proved || !solution_len || !plan || !bound || !nodes || !horizon || !verdict)
        return fail_msg(TPL_ERR_ARG, "%s: null pointer (every argument but skip and the stream is required)", name);
    if (!(r_line - r_line == 0.0f) || !(r_win - r_win == 0.0f) || !(r_lose - r_lose == 0.0f))
        return fail_msg(TPL_ERR_ARG, "%s: r_line, r_win and r_lose must be finite", name);
    if (!(gamma - gamma == 0.0f)) return fail_msg(TPL_ERR_ARG, "%s: gamma must be finite", name);
    if (const int rc = check_search(name, n, 1, "a workgroup per board: n must stay below 2^31", 1, L, M, max_nodes)) return rc;
    if (((uintptr_t)plane_a & 15u) || ((uintptr_t)plane_b & 15u))
        return fail_msg(TPL_ERR_ARG, "%s: planes must be 16-byte aligned", name);
    if ((uintptr_t)table & 3u) return fail_msg(TPL_ERR_ARG, "%s: table must be 4-byte aligned", name);
    if (const int rc = check_counts(name, solution_len, bound, nodes)) return rc;
    KernelArgs p{};
#ifdef TPL_EXACT_LIMITED_UNIT
    if (const int rc = check_discrepancy(name, first_limit, growth, limit)) return rc;
    p.first_limit = (uint32_t)first_limit; p.growth = (uint32_t)growth; p.limit = limit;
#endif
    p.a = (const uint4*)plane_a; p.b = (const uint4*)plane_b; p.n = (uint32_t)n;
    p.L = (uint32_t)L; p.M = (uint32_t)M; p.table = table;
    p.r_line = r_line; p.r_win = r_win; p.r_lose = r_lose; p.gamma = gamma;
    p.max_nodes = (uint32_t)max_nodes; p.skip = skip;
    p.solved = solved; p.proved = proved; p.solution_len = solution_len; p.plan = plan; p.bound = bound; p.nodes = nodes;
    p.horizon = horizon; p.verdict = verdict;
    const dim3 grid(p.n), block(kWindowWave);
    if (entries == TPL_NTUPLE_ENTRIES) hipLaunchKernelGGL(TPL_KERNEL(ntuple_window), grid, block, 0, (hipStream_t)stream, p);
    else if (entries == TPL_NTUPLE_ENTRIES_3X3) hipLaunchKernelGGL(TPL_KERNEL(ntuple_window3), grid, block, 0, (hipStream_t)stream, p);
    else if (entries == TPL_NTUPLE_ENTRIES_FEAT)
        hipLaunchKernelGGL(TPL_KERNEL(ntuple_window_feature), grid, block, 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(TPL_KERNEL(ntuple_window_budget), grid, block, 0, (hipStream_t)stream, p);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}
