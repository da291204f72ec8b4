// tpl_exact.h -- what the five proof units share (exact.hip, exact_nodes.hip, exact_window.hip, ntuple_exact.hip, ntuple_window.hip;
// include/tpl_learn.h states their rules): the stack record, the exact depth-first search, the write-out of a win's path, the two
// FRAMES a search stands in -- prove_root around a configuration's whole game, prove_window around the pieces a state's window shows
// --, the limited units' argument record and the argument checks the entries have in common.  What a unit keeps is its argument
// record, its entry and its ORDER: what a node's child is worth.  The linear order is here (LinearOrder); the table's is
// tpl_exact_table.h's, so that the linear units do not parse the table geometry.  exact_nodes.hip has a frame of its own: a finished
// node's exit, a game per node and a stride over the launch.
//
// The search is of the game (L, M) from a root with 0 lines and 0 moves, in the bounded form (tpl_placement.h: kUnitBound): the move
// bound's prune is what makes it finite in practice and its proof is the bound's.  Within the prune it visits every running board,
// or it stops at a node budget and says so.  With `shortest` it deepens the budget B from need(root) to M, so the first win it meets
// is a shortest one.
//
// Mapping: ONE SEARCH PER WAVEFRONT, one wavefront a workgroup, so the data-dependent loop holds no barrier at all; what one lane
// writes to LDS for the others is ordered by wave_sync(), which emits no instruction but the wait for the write.
//   the node    being expanded is read from its stack record by every lane; lane k < 34 makes child k, the k-th distinct placement of
//               the ply's piece in ascending b, and its 64-bit key (ordered_bits(value) << 32 | kSlotTop - k), so a larger key comes
//               first in the rule's order.  The other lanes idle: the search is divergent by nature.
//   the stop    a ballot over the won children; if any is set the largest won key names the child the solution ends with.
//   the order   the running children are ranked by their keys: 34 lane reads of a key, a compare and an add each.  A running
//               child writes its placement to place `rank` of the record's list; the one of rank 0 also writes the next record, since
//               it is descended into at once.
//   the stack   LDS, one 80-byte record a depth: the node's packed board (two uint4), what the order carries along the path, the
//               number of its running children, a cursor, and the list.  A running child at depth d + 1 has made d + 1 < B <= M
//               moves, so M records hold every path: 3,200 bytes at M = 40, 20,320 at M = 254, 960 for the twelve of a window.
//   the return  a later child is made again from its parent's record and the list's placement when the search comes back to it, as
//               the beam makes a kept candidate again in its phase C.
// Nothing but the outputs goes to memory.  A wave's search is one long dependent chain -- a record read from LDS, a move, the child's
// value, a rank, a record written -- so what hides its latency is other waves: every kernel is bound to eight waves a SIMD, 64 VGPRs
// without scratch, since everything the 34 children share sits in SGPRs (tools/kernel_resources.sh;
// profiles/learner/exact_refactor_isa.log).
//
// An ORDER is a small struct the unit's kernel names, the same in every lane:
//   Order(p)     a frame builds it from the unit's argument record just ahead of the search -- a window frame only for a board it
//                searches --, so what the order reads of the record is loaded there;
//   Carry        what a record keeps of the path for the order: the linear weights' carry word, or NoCarry (a table's value reads the
//                board alone), which takes no room in the record;
//   child(...)   the child of a record by placement (r, l) of piece `cur` in the game (L, B) -- the board the move leaves, dead turned
//                lost (placed_move, bounded_move) -- its Carry, and its value.  `later` points at the list behind `cur`: its first
//                entry is the piece the child will play.  The expansion and the return both come here, so a child's second making
//                gives the board of the first; the return drops the value.
#pragma once

#include "tpl_beam.h"

namespace tpl_learn {

constexpr int kExactWave = 64;
constexpr int kExactMaxMoves = 254;                           // M's limit (tpl_create's)
constexpr int kExactMaxNodes = TPL_EXACT_MAX_NODES;
static_assert(kUnitBound, "the exact search is a unit of the bounded form");
static_assert(kMaxPlacements <= kExactWave, "a lane per child");

// A unit built with TPL_EXACT_LIMITED_UNIT (the *_limited*.hip files) is its twin's text around the LIMITED search.  The macro chooses
// here, once: kLimitedUnit, which the unit hands its frame; the _limited in its kernels' and its entry's names; and TPL_LIMITED(...),
// the text only the limited entry has -- its three extra parameters.  Everything else is `if constexpr` on the constant.
#ifdef TPL_EXACT_LIMITED_UNIT
constexpr bool kLimitedUnit = true;
#define TPL_EXACT_LIMITED _limited
#define TPL_EXACT_LIMITED_NAME "_limited"
#define TPL_LIMITED(...) __VA_ARGS__
#else
constexpr bool kLimitedUnit = false;
#define TPL_EXACT_LIMITED
#define TPL_EXACT_LIMITED_NAME ""
#define TPL_LIMITED(...)
#endif

// one depth of the stack
template <typename Carry>
struct alignas(16) Frame {
    uint4 a, b;                  // the node's board; its window is not part of the rule
    [[no_unique_address]] Carry carry;                         // of the path to the node, for the order
    uint32_t count;              // its running children
    uint32_t cursor;             // how many of them have been descended into
    uint8_t kids[36];            // their placements b = 10 r + l in the order of the descent, kMaxPlacements at most
};
struct NoCarry {};               // of an order whose value reads the board alone: no room in the record
static_assert(sizeof(Frame<uint32_t>) == 80 && sizeof(Frame<NoCarry>) == 80, "a record is 80 bytes");

// LDS written by one lane, read by another of the same wave: the accesses of a wave reach LDS in order, so this only keeps the
// compiler from moving them across and waits for the write
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

template <typename Carry>
__device__ __forceinline__ void store_frame(Frame<Carry>& f, const tpl::Board& s, Carry carry) {
    uint4 A, B;
    tpl::pack_board(s, A, B);
    f.a = A;
    f.b = B;
    f.carry = carry;
}

// a fresh root of a game: 0 lines, 0 moves, running; the columns are left to the caller
__device__ __forceinline__ void fresh_root(tpl::Board& root) {
    root.window = 0u; root.window_hi = 0u;
    root.state = tpl::ST_RUNNING; root.lines = 0u; root.moves = 0u; root.slot = 0u;
}

// need(root): no solution of the game with L lines owed is shorter
__device__ __forceinline__ uint32_t need_of(const tpl::Board& root, uint32_t L) { return (move_bound_cells(root.c, L) + 3u) >> 2; }

// the M + 1 entries of a piece list from pieces[first] on into LDS, masked as move_board masks them
__device__ __forceinline__ void load_pieces(uint8_t* s_pieces, const uint8_t* pieces, size_t first, uint32_t M, uint32_t lane) {
    for (uint32_t t = lane; t <= M; t += kExactWave) s_pieces[t] = pieces[first + t] & 7u;
}

// The LINEAR order of exact.hip, exact_nodes.hip and exact_window.hip on the unit's F board features: a child exactly as solve.hip's
// expand() makes a bounded candidate -- the board the move leaves, dead turned lost, the carry of the path with the move's, and the
// value of psi under the weights.  One row of weights for the whole grid: scalar loads, and they stay in SGPRs.
template <int F>
struct LinearOrder {
    using Carry = uint32_t;      // of the path to the node (tpl_placement.h)
    float w[F];
    float spare_weight;
    __device__ __forceinline__ LinearOrder(const float* weights, float spare) : spare_weight(spare) {
#pragma unroll
        for (int q = 0; q < F; ++q) w[q] = weights[q];
    }
    template <typename Args>     // of a frame's argument record
    __device__ __forceinline__ explicit LinearOrder(const Args& p) : LinearOrder(p.weights, p.spare_weight) {}
    __device__ __forceinline__ float child(const Frame<Carry>& node, uint32_t cur, const uint8_t*, uint32_t r, uint32_t l,
                                           const tpl::ShapeWord* shape, uint32_t L, uint32_t B, tpl::Board& s, Carry& carry) const {
        tpl::unpack_board(node.a, node.b, s);
        s.window = cur;
        s.window_hi = 0u;
        carry = node.carry + placed_move<F>(s, shape, r, l, L, B);
        const int32_t spare = bounded_move(s, L, B);
        FeatureSet<F> psi;
        moved_features(s, carry, true, psi);
        return bounded_value(placement_score(w, psi), spare_weight, spare);
    }
};

struct Found {                   // as declared: the result of no search at all
    uint32_t nodes = 0u, length = 0u, last = kNoMove;         // expansions, all iterations; the winning length, 0 if none, and its last move
    bool capped = false;
    uint32_t limit = 0u;                                      // the limited search alone: the K of the last iteration begun, 0 if none
};

// The LIMITED search's two numbers (include/tpl_learn.h: tpl_placement_exact_limited): the first discrepancy limit of every budget and
// how the limit grows, 0 by one ("add"), 1 by doubling ("double").  The plain search takes none.
struct Discrepancy {
    uint32_t first, growth;
};
constexpr uint32_t kLimitTop = 65535u;                        // K's clamp; a K >= 8,382 never cuts, so the clamp ends nothing

// a limited entry's argument record: its twin's, the two numbers of the limited search and one more output
template <typename Twin>
struct LimitedArgs : Twin {
    uint32_t first_limit;        // in [0, 65535]: the K every budget starts with
    uint32_t growth;             // 0: K + 1 ("add"); 1: max(1, 2 K) ("double")
    int32_t* limit;              // [n]: the K of the last iteration begun, 0 where nothing was searched
};
// what a frame hands the search of a record's two numbers; a plain record has none, and the plain search reads none
template <bool Limited, typename Args>
__device__ __forceinline__ Discrepancy discrepancy_of(const Args& p) {
    if constexpr (Limited) return Discrepancy{p.first_limit, p.growth};
    else return Discrepancy{0u, 0u};
}

// The search of the game (L, M) from `root` -- 0 lines, 0 moves -- whose piece at depth d is s_pieces[d]; every argument is the same
// in every lane.  `need` is need(root), and need > M is decided without a node.  The caller has filled s_shape and s_pieces, entries
// 0 .. M.  On return the path of a win is in the stack: the child in hand at every depth, then `last`.
//
// Limited = true is the limited-discrepancy order: an iteration is (B, K), the game (L, B) searched with at most K steps off the
// order on a path.  A node holds `rem`, what is left of K on the path to it: of its running children those of rank <= rem are kept,
// the one of rank j is searched with rem - j, and a dropped child sets `cut`.  A budget's iterations go on from a fresh root with the
// next K until one cuts nothing -- that one has visited what the plain iteration visits.  rem, K and cut are the same in every lane
// and stay in SGPRs; a record keeps its rem in the upper half of `count`, which is 34 at most, so a record stays 80 bytes.
template <typename Order, bool Limited = false>
__device__ __forceinline__ Found search(const Order& order, Frame<typename Order::Carry>* stack, const uint8_t* s_pieces,
                                        const tpl::ShapeWord* s_shape, const tpl::Board& root, uint32_t need, uint32_t L, uint32_t M,
                                        uint32_t max_nodes, uint32_t shortest, uint32_t lane, Discrepancy disc = Discrepancy{0u, 0u}) {
    using Carry = typename Order::Carry;
    uint32_t nodes = 0u, length = 0u, last = kNoMove;
    bool capped = false;
    uint32_t limit = 0u;
    if (need <= M) {
#pragma unroll 1
        for (uint32_t B = shortest ? need : M; B <= M && length == 0u && !capped; ++B) {
            uint32_t K = disc.first;                           // Limited: every budget starts at the first limit
#pragma unroll 1
            for (;;) {                                         // Limited: the iterations (B, K) of one budget; the plain search has one
                bool cut = false;
                uint32_t rem = K;                              // of the node at depth d
                if constexpr (Limited) limit = K;
                wave_sync();                                   // the last iteration's reads of record 0 (and, the first time, the tables)
                if (lane == 0) store_frame(stack[0], root, Carry{});
                wave_sync();
                uint32_t d = 0u;
#pragma unroll 1
                for (;;) {
                    // expand the node at depth d
                    if (nodes == max_nodes) { capped = true; break; }
                    ++nodes;
                    const uint32_t cur = uniform(s_pieces[d]);
                    const uint32_t stride = placement_count(cur);
                    const bool mine = lane < stride;
                    const uint32_t k = mine ? lane : 0u;
                    uint32_t r, l;
                    const uint32_t b = nth_placement(cur, k, r, l);
                    tpl::Board s;
                    Carry carry;
                    const float value = order.child(stack[d], cur, s_pieces + d + 1u, r, l, s_shape, L, B, s, carry);
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
                    uint32_t count = (uint32_t)__builtin_popcountll(__ballot(running));
                    if constexpr (Limited) {                   // the children of rank <= rem are kept; a dropped one is a cut
                        if (count > rem + 1u) { count = rem + 1u; cut = true; }
                    }
                    if (running && (!Limited || rank < count)) {
                        stack[d].kids[rank] = (uint8_t)b;
                        if (rank == 0u && d + 1u < M) store_frame(stack[d + 1u], s, carry);  // descended into at once (d + 1 < B <= M)
                    }
                    if (lane == 0) {
                        stack[d].count = Limited ? count | (rem << 16) : count;
                        stack[d].cursor = count != 0u ? 1u : 0u;
                    }
                    wave_sync();
                    if (count != 0u) { ++d; continue; }        // Limited: the child of rank 0 keeps the node's rem

                    // no running child: back to the nearest node that has one left, and into it
                    bool more = false;
#pragma unroll 1
                    while (d > 0u) {
                        --d;
                        const uint32_t at = uniform(stack[d].cursor);
                        const uint32_t word = uniform(stack[d].count);
                        if (at < (Limited ? word & 0xFFFFu : word)) {
                            if constexpr (Limited) rem = (word >> 16) - at;  // the child of rank `at`: at < count <= rem + 1
                            const uint32_t b2 = uniform(stack[d].kids[at]);
                            tpl::Board s2;
                            Carry carry2;
                            order.child(stack[d], uniform(s_pieces[d]), s_pieces + d + 1u, b2 / 10u, b2 % 10u, s_shape, L, B, s2, carry2);
                            wave_sync();
                            if (lane == 0 && d + 1u < M) {
                                stack[d].cursor = at + 1u;
                                store_frame(stack[d + 1u], s2, carry2);
                            }
                            wave_sync();
                            ++d;
                            more = true;
                            break;
                        }
                    }
                    if (!more) break;                          // the root's children are used up: no win at this budget
                }
                if constexpr (!Limited) break;
                else {
                    if (!cut || capped || length != 0u) break;     // nothing dropped: (L, B) is searched out -- or the search is over
                    K = min(disc.growth != 0u ? max(1u, 2u * K) : K + 1u, kLimitTop);
                }
            }
        }
    }
    wave_sync();
    Found out;
    out.nodes = nodes;
    out.length = capped ? 0u : length;
    out.last = last;
    out.capped = capped;
    out.limit = limit;
    return out;
}

// the path of a win from the stack: the child in hand at every depth, then the won one; 255 behind the end, up to `width`
template <typename Carry>
__device__ __forceinline__ void write_path(const Frame<Carry>* stack, const Found& f, uint8_t* out, uint32_t width, uint32_t lane) {
    for (uint32_t t = lane; t < width; t += kExactWave) {
        uint32_t a = kNoMove;
        if (t + 1u < f.length) a = stack[t].kids[stack[t].cursor - 1u];
        else if (t + 1u == f.length) a = f.last;
        out[t] = (uint8_t)a;
    }
}

// The ROOT FRAME (exact.hip, ntuple_exact.hip): configuration blockIdx.x of the record `p` -- its rows as a full reset deals them, its
// whole piece list, the game (L, M) -- searched under `order`, and what the search found written out.  The stack is the launch's
// dynamic LDS, M records of 80 bytes; the shape table and the list are static.  A limited unit's record is LimitedArgs of its twin's.
template <typename Order, bool Limited, typename Args>
__device__ __forceinline__ void prove_root(const Args& p) {
    using Stack = Frame<typename Order::Carry>;
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

    const Order order(p);
    const Found f = search<Order, Limited>(order, stack, s_pieces, s_shape, root, bound, L, M, p.max_nodes, p.shortest, lane,
                                           discrepancy_of<Limited>(p));
    if (lane == 0) {
        p.solved[i] = f.length != 0u ? (uint8_t)1 : (uint8_t)0;
        p.proved[i] = f.capped ? (uint8_t)0 : (uint8_t)1;
        p.solution_len[i] = (int32_t)f.length;
        p.bound[i] = (int32_t)bound;
        p.nodes[i] = f.nodes;
        if constexpr (Limited) p.limit[i] = (int32_t)f.limit;
    }
    write_path(stack, f, p.actions + (size_t)i * M, M, lane);
}

constexpr int kWindowWave = kExactWave;
constexpr int kWindowDepth = tpl::kWindowEntries;             // 12: the longest horizon, and the plan's width
constexpr int kWindowList = 16;                               // the list in LDS: entries 0 .. H - 1 of the window, 0 behind them
static_assert(kWindowDepth == TPL_WINDOW_PLAN, "the plan is as wide as the window");
static_assert(kWindowDepth < kWindowList, "entry 12 of the list exists");

// The WINDOW FRAME (exact_window.hip, ntuple_window.hip): board blockIdx.x of the packed planes, a running board of the game
// (p.L, p.M) with `lines` cleared after `moves` moves.  It has rem = M - moves moves left and its window shows known = 12 - moves mod
// 10 true pieces, so H = min(known, rem) moves have their piece known: the HORIZON.  The board is searched as a fresh root of the
// shifted game (L - lines, H) with shortest = 1, its list window entries 0 .. H - 1, and the verdict says what the result means.  No
// path is longer than twelve entries: the stack is twelve records of STATIC LDS beside the shape table and the list.
//
// One list rule for every order: sixteen entries, the window's below H and 0 from H on.  An order that values a child under the
// piece it will play (TableOrder) reads list entry d + 1 before it knows whether the child runs; a child that runs has
// d + 1 < B <= H, a true piece of the episode, and any other child's value is its reward alone.  So the read reaches entry H at most
// -- index 12 where H = 12 -- and that entry is a defined 0, never a piece the agent does not know and never stale LDS.  The linear
// order reads nothing behind `cur`.
template <typename Order, bool Limited, typename Args>
__device__ __forceinline__ void prove_window(const Args& p) {
    __shared__ Frame<typename Order::Carry> stack[kWindowDepth];
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
    if (live && !skipped) {
        if (lane < 32) s_shape[lane] = tpl::kShapeTable[lane];
        // list entry `lane`: the window's, masked as move_board masks it, below the horizon and 0 from it on
        const unsigned long long window = ((unsigned long long)at.window_hi << 32) | at.window;
        if (lane < (uint32_t)kWindowList) s_pieces[lane] = lane < H ? (uint8_t)((uint32_t)(window >> (3u * lane)) & 7u) : (uint8_t)0;
        const Order order(p);
        f = search<Order, Limited>(order, stack, s_pieces, s_shape, root, need, L, H, p.max_nodes, 1u, lane,
                                   discrepancy_of<Limited>(p));                                    // the game (L, H), shortest
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
        if constexpr (Limited) p.limit[i] = (int32_t)f.limit;
    }
    write_path(stack, f, p.plan + (size_t)i * kWindowDepth, (uint32_t)kWindowDepth, lane);      // the plan
}

// What every entry of the five units refuses of n, the game and the node budget, in the order they all test them; `name` leads the
// message.  A launch is `waves_each` workgroups for each of n, and `each` says so in the refusal; n_cfg is 1 where there is no pool.
inline int check_search(const char* name, int64_t n, int64_t waves_each, const char* each, int64_t n_cfg, int32_t L, int32_t M,
                        int32_t max_nodes) {
    if (n < 1) return fail_msg(TPL_ERR_ARG, "%s: n must be positive", name);
    if (n >= (((int64_t)1 << 31) + waves_each - 1) / waves_each) return fail_msg(TPL_ERR_ARG, "%s: n too large (%s)", name, each);
    if (n_cfg < 1 || n_cfg >= ((int64_t)1 << 31)) return fail_msg(TPL_ERR_ARG, "%s: n_cfg must be in [1, 2^31)", name);
    if (L < 1 || L > 250 || M < 1 || M > kExactMaxMoves)
        return fail_msg(TPL_ERR_ARG, "%s: L and M must be in [1, 250] and [1, %d]", name, kExactMaxMoves);
    if (max_nodes < 1 || max_nodes > kExactMaxNodes) return fail_msg(TPL_ERR_ARG, "%s: max_nodes must be in [1, %d]", name, kExactMaxNodes);
    return TPL_OK;
}

// the three int32 outputs of a search: the last of every entry's checks
inline int check_counts(const char* name, const int32_t* solution_len, const int32_t* bound, const uint32_t* nodes) {
    if ((uintptr_t)solution_len & 3u) return fail_msg(TPL_ERR_ARG, "%s: solution_len must be 4-byte aligned", name);
    if ((uintptr_t)bound & 3u) return fail_msg(TPL_ERR_ARG, "%s: bound must be 4-byte aligned", name);
    if ((uintptr_t)nodes & 3u) return fail_msg(TPL_ERR_ARG, "%s: nodes must be 4-byte aligned", name);
    return TPL_OK;
}

// what the two table entries refuse of a table's entry count, first of all, and of the rewards and gamma
inline int check_table_form(const char* name, int64_t entries) {
    if (entries != TPL_NTUPLE_ENTRIES && entries != TPL_NTUPLE_ENTRIES_3X3 && entries != TPL_NTUPLE_ENTRIES_FEAT &&
        entries != TPL_NTUPLE_ENTRIES_BUDGET)
        return fail_msg(TPL_ERR_ARG,
                        "%s: entries must be %d (\"2x4\"), %d (\"3x3\"), %d (\"feat\") or %d (\"feat+spare\"), the four plain forms -- a sum "
                        "or a staged table orders no search --, got %lld",
                        name, (int)TPL_NTUPLE_ENTRIES, (int)TPL_NTUPLE_ENTRIES_3X3, (int)TPL_NTUPLE_ENTRIES_FEAT,
                        (int)TPL_NTUPLE_ENTRIES_BUDGET, (long long)entries);
    return TPL_OK;
}
inline int check_table_numbers(const char* name, float r_line, float r_win, float r_lose, float gamma) {
    if (!(r_line - r_line == 0.0f) || !(r_win - r_win == 0.0f) || !(r_lose - r_lose == 0.0f))
        return fail_msg(TPL_ERR_ARG, "%s: r_line, r_win and r_lose must be finite", name);
    if (!(gamma - gamma == 0.0f)) return fail_msg(TPL_ERR_ARG, "%s: gamma must be finite", name);
    return TPL_OK;
}

// what every limited entry refuses of its own three arguments, after its twin's checks of n, the game and the node budget
inline int check_discrepancy(const char* name, int32_t first_limit, int32_t growth, const int32_t* limit) {
    if (first_limit < 0 || first_limit > (int32_t)kLimitTop)
        return fail_msg(TPL_ERR_ARG, "%s: first_limit must be in [0, %d]", name, (int)kLimitTop);
    if (growth != 0 && growth != 1) return fail_msg(TPL_ERR_ARG, "%s: growth must be 0 (add) or 1 (double)", name);
    if (!limit) return fail_msg(TPL_ERR_ARG, "%s: null pointer (limit is required)", name);
    if ((uintptr_t)limit & 3u) return fail_msg(TPL_ERR_ARG, "%s: limit must be 4-byte aligned", name);
    return TPL_OK;
}

// the last of an entry's checks: a limited record takes its three arguments, checked; a plain one has none to take
template <typename Twin>
inline int take_limited(const char* name, LimitedArgs<Twin>& p, int32_t first_limit, int32_t growth, int32_t* limit) {
    if (const int rc = check_discrepancy(name, first_limit, growth, limit)) return rc;
    p.first_limit = (uint32_t)first_limit; p.growth = (uint32_t)growth; p.limit = limit;
    return TPL_OK;
}
template <typename Args>
inline int take_limited(const char*, Args&) { return TPL_OK; }

}  // namespace tpl_learn
