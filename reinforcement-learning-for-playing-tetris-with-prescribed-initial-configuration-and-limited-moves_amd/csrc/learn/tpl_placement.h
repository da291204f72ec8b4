// tpl_placement.h -- what the placement family shares (afterstates.hip, heuristic.hip, beam.hip, ntuple.hip; include/tpl_learn.h
// states the rules): which of the 40 actions are one placement, the first move of a (board, action) pair and its reward, the
// board features, the score and its ordered key, the second ply's loop, and the argument checks of the entry points that read a pair of state planes.
//
// Two feature sets.  kFeatures = 12 describes the board a move leaves.  kMoveFeatures = 14 adds the two features of the move itself,
// landing height and eroded cells; placed_move<14> is the one place they are made, from move_trace's drop and cleared-row mask.
// What a path carries of its moves is one word, the CARRY: the rows cleared at 12, and at 14 the rows cleared, the landing sum and the
// eroded sum in 8 + 14 + 10 bits, so that the carries of two moves add field by field with one add.
#pragma once

#include "tpl_learn_internal.h"
#include "tpl_mirror.h"

namespace tpl_learn {

constexpr int kActions = TPL_NUM_ACTIONS;
constexpr int kFeatures = TPL_NUM_FEATURES;
constexpr int kMoveFeatures = TPL_NUM_MOVE_FEATURES;

// A unit of the linear placement family (heuristic.hip, beam.hip, solve.hip) is written once and built twice (beam.hip and solve.hip
// four times: the bound switch below): as it stands on the
// twelve board features, and once more on the fourteen through its twin (heuristic_move.hip, ...), which defines
// TPL_PLACEMENT_MOVE_UNIT and includes it.  Two units and not two instances in one: with both feature sets in one translation unit the
// compiler orders a few instructions of the 12-feature kernels differently (profiles/learner/move_features_isa.log).  kUnitFeatures is
// the unit's feature set; TPL_UNIT_KERNEL(placement_act) and TPL_UNIT_ENTRY(tpl_placement_act) are the names of a kernel and an entry
// point in it: placement_act_kernel / tpl_placement_act, or placement_act_move_kernel / tpl_placement_act_move.
#ifdef TPL_PLACEMENT_MOVE_UNIT
constexpr int kUnitFeatures = kMoveFeatures;
#define TPL_UNIT_FORM _move
#define TPL_UNIT_FORM_NAME "_move"
#else
constexpr int kUnitFeatures = kFeatures;
#define TPL_UNIT_FORM
#define TPL_UNIT_FORM_NAME ""
#endif
// The bound switch stands beside the feature set: a unit that defines TPL_PLACEMENT_BOUND_UNIT before it includes its twin
// (beam_bound.hip, solve_move_bound.hip, ...) is the BOUNDED form of that twin (include/tpl_learn.h: the move bound) --
// placement_solve_bound_kernel / tpl_placement_solve_bound, placement_solve_move_bound_kernel / tpl_placement_solve_move_bound.
// kUnitBound is the switch; bounded_move below is the one place where the two forms part.
#ifdef TPL_PLACEMENT_BOUND_UNIT
constexpr bool kUnitBound = true;
#define TPL_UNIT_BOUND _bound
#define TPL_UNIT_BOUND_NAME "_bound"
#else
constexpr bool kUnitBound = false;
#define TPL_UNIT_BOUND
#define TPL_UNIT_BOUND_NAME ""
#endif
#define TPL_UNIT_PASTE4_(a, b, c, d) a##b##c##d
#define TPL_UNIT_PASTE4(a, b, c, d) TPL_UNIT_PASTE4_(a, b, c, d)
#define TPL_UNIT_KERNEL(stem) TPL_UNIT_PASTE4(stem, TPL_UNIT_FORM, TPL_UNIT_BOUND, _kernel)
#define TPL_UNIT_ENTRY(stem) TPL_UNIT_PASTE4(stem, TPL_UNIT_FORM, TPL_UNIT_BOUND, )
#define TPL_UNIT_ENTRY_NAME(stem) #stem TPL_UNIT_FORM_NAME TPL_UNIT_BOUND_NAME
constexpr int kMoveWeightStride = TPL_MOVE_WEIGHT_STRIDE;
// floats between two weight rows of feature set kF
template <int kF> constexpr int weight_stride() { return kF == kMoveFeatures ? kMoveWeightStride : kF; }

// the carry's fields at 14 features: a path clears at most 253 rows, lands at most 254 * 38 = 9,652 half rows and erodes at most
// 4 (L + 3) <= 1,012 cells
constexpr uint32_t kLandShift = 8u, kErodedShift = 22u;
static_assert(254u * 38u < (1u << (kErodedShift - kLandShift)) && 4u * 253u < (1u << (32u - kErodedShift)), "the sums fit their fields");

// canonical[a] = 10 (r mod nrot(cur)) + min(l, 10 - w(cur, r)) for a = 10 r + l, r < 4, l < 10; reads tpl_mirror.h's packed
// widths and rotation masks instead of a dependent load of the shape table
__host__ __device__ constexpr uint32_t canonical_action(uint32_t cur, uint32_t r, uint32_t l) {
    const uint32_t right = right_most(cur, r);
    return 10u * (r & last_rotation(cur)) + (l < right ? l : right);
}

// tpl_mirror.h's walk visits exactly the actions that are their own canonical form, in ascending order, placement_count of them
constexpr bool walk_visits_the_canonical_actions() {
    for (uint32_t p = 0; p < 8u; ++p) {
        uint32_t r = 0u, l = 0u, steps = 0u;
        for (uint32_t a = 0; a < (uint32_t)kActions; ++a) {
            if (canonical_action(p, a / 10u, a % 10u) != a) continue;
            if (r > last_rotation(p) || 10u * r + l != a) return false;
            next_placement(p, r, l);
            ++steps;
        }
        if (r <= last_rotation(p) || steps != placement_count(p)) return false;
    }
    return true;
}
static_assert(walk_visits_the_canonical_actions(), "next_placement and placement_count do not match canonical_action");

// What move_board (csrc/tpl_device.h) keeps to itself of the move it is about to make on `s`: the drop -- the row of the piece's top-most
// mask row after the fall, from the column tops under the piece exactly as move_board takes it --, the rows that are full once the
// piece is locked and that move_board will clear (bit r = row r), and the shape word with the piece's column nibbles and height.  A
// top-out makes no move: drop and clear are 0.  Called on the board BEFORE the move.  The board itself is still made by move_board
// alone: this only reads, so nothing it says can change a game, and the environment's header stays as it is (its digest names
// the committed profiles).  The tops are move_board's own expressions, which the compiler shares between the two; the rest, some
// eighty instructions a pair, is made twice.
struct MoveTrace { uint32_t drop, clear, shape; };

__device__ __forceinline__ MoveTrace move_trace(const tpl::Board& s, const tpl::ShapeWord* shape, uint32_t rot, uint32_t loc) {
    const tpl::ShapeWord sh = shape[(s.window & 7u) * 4u + (rot & 3u)];
    const uint32_t w = (sh.x >> 16) & 7u;
    const uint32_t h = (sh.x >> 19) & 7u;
    loc = min(loc, (uint32_t)tpl::kCols - w);
    // the tops of the four columns under the piece as bytes, plus the table's per-column bias: drop = min - 4
    uint32_t t[tpl::kCols];
#pragma unroll
    for (int k = 0; k < tpl::kCols; ++k) t[k] = (uint32_t)__builtin_ctz(s.c[k] | tpl::kSentinelBit);
    const uint32_t p0 = t[0] | (t[1] << 8) | (t[2] << 16) | (t[3] << 24);
    const uint32_t p1 = t[4] | (t[5] << 8) | (t[6] << 16) | (t[7] << 24);
    const uint32_t p2 = t[8] | (t[9] << 8);
    const uint32_t word = loc >> 2;
    const uint32_t lo = word == 0u ? p0 : word == 1u ? p1 : p2;
    const uint32_t hi = word == 0u ? p1 : word == 1u ? p2 : 0u;
    const uint32_t sums = __builtin_amdgcn_alignbyte(hi, lo, loc & 3u) + sh.y;
    const uint32_t best = min(min(sums & 0xFFu, (sums >> 8) & 0xFFu), min((sums >> 16) & 0xFFu, sums >> 24));
    const bool topout = best < 4u;
    const uint32_t drop = topout ? 0u : best - 4u;
    // the rows that are full with the piece's column nibbles, shifted down by drop, in their columns
    const uint64_t placed = (uint64_t)(sh.x & 0xFFFFu) << (4u * loc);
    const uint32_t plo = (uint32_t)placed, phi = (uint32_t)(placed >> 32);
    uint32_t full = 0xFFFFFFFFu;
#pragma unroll
    for (int k = 0; k < 8; ++k) full &= s.c[k] | (((plo >> (4 * k)) & 0xFu) << drop);
    full &= s.c[8] | ((phi & 0xFu) << drop);
    full &= s.c[9] | (((phi >> 4) & 0xFu) << drop);
    MoveTrace trace;
    trace.drop = drop;
    trace.clear = topout ? 0u : full & (((1u << h) - 1u) << drop);
    trace.shape = sh.x;
    return trace;
}

// move_board(s, r, l) and the carry of the move.  At 12 features that is the rows cleared and the code is move_board's.  At 14 it
// is  n | landing_height << 8 | eroded_cells << 22  (include/tpl_learn.h, features 12 and 13): with drop the row of the piece's top
// mask row and h the shape's height the piece lies in rows drop .. drop + h - 1, so landing_height = 39 - 2 drop - h; the piece's
// cells in cleared rows are the bits of its four column nibbles at the cleared rows' offsets below drop, and eroded_cells is n times
// their count.  A top-out makes no move: both are 0.
template <int kF = kFeatures>
__device__ __forceinline__ uint32_t placed_move(tpl::Board& s, const tpl::ShapeWord* shape, uint32_t r, uint32_t l, uint32_t L,
                                                uint32_t M) {
    bool topout;
    if constexpr (kF == kMoveFeatures) {
        // both features before the move, so that one word and not the trace lives across it
        const MoveTrace trace = move_trace(s, shape, r, l);
        const uint32_t h = (trace.shape >> 19) & 7u;
        const uint32_t rows = (trace.clear >> trace.drop) & 0xFu;            // the cleared rows among the piece's, bit i = mask row i
        const uint32_t cells = (uint32_t)__builtin_popcount(trace.shape & 0xFFFFu & (rows * 0x1111u));
        const uint32_t eroded = __umul24((uint32_t)__builtin_popcount(rows), cells);
        const uint32_t landing = 39u - 2u * trace.drop - h;
        const uint32_t features = (landing << kLandShift) | (eroded << kErodedShift);
        const uint32_t n = tpl::move_board(s, shape, r, l, L, M, topout);
        return n | (topout ? 0u : features);
    } else {
        return tpl::move_board(s, shape, r, l, L, M, topout);
    }
}

// The first move of pair (state (A, B), action 10 r + l): `s` becomes the board the move leaves, its window not yet popped;
// `cur` is the piece that was placed and `running` whether the state was still in play (a finished board's move means
// nothing: the callers select on `running`).  Returns the move's carry: the rows cleared at 12 features.  r and l are values,
// never register indices (move_board's comment says why).
template <int kF = kFeatures>
__device__ __forceinline__ uint32_t first_move(const uint4& A, const uint4& B, const tpl::ShapeWord* shape, uint32_t r, uint32_t l,
                                               uint32_t L, uint32_t M, tpl::Board& s, uint32_t& cur, bool& running) {
    tpl::unpack_board(A, B, s);
    cur = s.window & 7u;
    running = s.state == tpl::ST_RUNNING;
    return placed_move<kF>(s, shape, r, l, L, M);
}

// step_reward's rule (csrc/tpl_step.h) for a move that cleared n_clear rows and left `state`: one rounded multiply, then at most
// one rounded add; contraction off, or the pair becomes an FMA whose single rounding differs where r_line * n is not exact
__device__ __forceinline__ float move_reward(float r_line, float r_win, float r_lose, uint32_t n_clear, uint32_t state) {
#pragma clang fp contract(off)
    float reward = r_line * (float)n_clear;
    if (state == tpl::ST_WON) reward = reward + r_win;
    if (state >= tpl::ST_LOST_LIMIT) reward = reward + r_lose;
    return reward;
}

template <int kF> struct FeatureSet { uint32_t f[kF]; };
using Features = FeatureSet<kFeatures>;

// popcount(x) + acc: v_bcnt_u32_b32 adds its second operand
__device__ __forceinline__ uint32_t bcnt(uint32_t x, uint32_t acc) { return (uint32_t)__builtin_popcount(x) + acc; }
__device__ __forceinline__ uint32_t absdiff(uint32_t a, uint32_t b) { return max(a, b) - min(a, b); }

// features 3..11 of a board given as its ten column words (bit r = row r, row 0 = top; bits 20.. clear)
template <int kF>
__device__ __forceinline__ void board_features(const uint32_t (&c)[tpl::kCols], FeatureSet<kF>& out) {
    constexpr uint32_t kFloor = tpl::kSentinelBit;            // row 20: the floor, filled
    uint32_t t[tpl::kCols];                                   // top of column x: row of its top-most filled cell, 20 if empty
#pragma unroll
    for (int x = 0; x < tpl::kCols; ++x) t[x] = (uint32_t)__builtin_ctz(c[x] | kFloor);

    uint32_t top_sum = 0, top_min = tpl::kRows, filled = 0;
    uint32_t col_trans = 0, hole_rows = 0, depth = 0;
#pragma unroll
    for (int x = 0; x < tpl::kCols; ++x) {
        top_sum += t[x];
        top_min = min(top_min, t[x]);
        filled = bcnt(c[x], filled);
        // rows r = 0..19 against r + 1 with the floor as row 20: pairs (r, r + 1), r < 19, and the floor term
        const uint32_t cf = c[x] | kFloor;
        col_trans = bcnt((cf ^ (cf >> 1)) & tpl::kColMask, col_trans);
        // holes of the column: the empty cells below its top
        hole_rows |= ~c[x] & (tpl::kColMask >> t[x] << t[x]);
        // the run of filled cells from the top down; it ends at the column's top-most hole unless it reaches the floor
        const uint32_t run = (uint32_t)__builtin_ctz(~(c[x] >> t[x]));
        depth += t[x] + run < (uint32_t)tpl::kRows ? run : 0u;
    }
    const uint32_t height_sum = tpl::kRows * tpl::kCols - top_sum;

    uint32_t bump = 0;
#pragma unroll
    for (int x = 0; x + 1 < tpl::kCols; ++x) bump += absdiff(t[x], t[x + 1]);

    // per row: wall | x = 0..9 | wall, the walls filled
    uint32_t row_trans = bcnt(~c[0] & tpl::kColMask, 0);
#pragma unroll
    for (int x = 0; x + 1 < tpl::kCols; ++x) row_trans = bcnt(c[x] ^ c[x + 1], row_trans);
    row_trans = bcnt(~c[tpl::kCols - 1] & tpl::kColMask, row_trans);

    // d_x = max(0, min(h_{x-1}, h_{x+1}) - h_x) = max(0, t_x - max(t_{x-1}, t_{x+1})), t = 0 beyond the walls (h = 20)
    uint32_t wells = 0;
#pragma unroll
    for (int x = 0; x < tpl::kCols; ++x) {
        const uint32_t left = x > 0 ? t[x - 1] : 0u, right = x + 1 < tpl::kCols ? t[x + 1] : 0u;
        const uint32_t side = max(left, right);
        const uint32_t d = t[x] > side ? t[x] - side : 0u;
        wells += __umul24(d, d + 1u) >> 1;
    }

    out.f[3] = height_sum - filled;                            // holes: the cells below the tops that are not filled
    out.f[4] = height_sum;
    out.f[5] = tpl::kRows - top_min;
    out.f[6] = bump;
    out.f[7] = row_trans;
    out.f[8] = col_trans;
    out.f[9] = wells;
    out.f[10] = (uint32_t)__builtin_popcount(hole_rows);
    out.f[11] = depth;
}

// phi of the board `s` that a move (or more) left, `carry` being the summed carries of the moves: rows cleared, won, lost and
// board_features, at 14 features the landing and eroded sums behind them; all zero where `live` is false
template <int kF>
__device__ __forceinline__ void moved_features(const tpl::Board& s, uint32_t carry, bool live, FeatureSet<kF>& out) {
    board_features(s.c, out);
    if constexpr (kF == kMoveFeatures) {
        out.f[0] = carry & ((1u << kLandShift) - 1u);
        out.f[12] = (carry >> kLandShift) & ((1u << (kErodedShift - kLandShift)) - 1u);
        out.f[13] = carry >> kErodedShift;
    } else {
        out.f[0] = carry;
    }
    out.f[1] = s.state == tpl::ST_WON ? 1u : 0u;
    out.f[2] = s.state >= tpl::ST_LOST_LIMIT ? 1u : 0u;
#pragma unroll
    for (int k = 0; k < kF; ++k) out.f[k] = live ? out.f[k] : 0u;
}

// w . phi left to right in float32: every product and every sum rounded once -- contraction off, as move_reward
template <int kF>
__device__ __forceinline__ float placement_score(const float (&w)[kF], const FeatureSet<kF>& phi) {
#pragma clang fp contract(off)
    float s = w[0] * (float)phi.f[0];
#pragma unroll
    for (int k = 1; k < kF; ++k) s = s + w[k] * (float)phi.f[k];
    return s;
}

// The move bound (include/tpl_learn.h): the least number of cells that must still be added to a board given as its ten column
// words (bits 20.. clear) before `lines_left` more rows can have been cleared -- the sum of the lines_left smallest row costs, a row
// with f < 10 filled cells costing 10 - f and a full row or a fresh one 10.  Three steps, no register indexed by a value:
//   the fills    a bit-sliced add of the ten words into four planes (bit r of p3 p2 p1 p0 = fill(r)): three carry-save adders on
//                nine words, one on their sums, a half adder for the tenth, then the carries -- some thirty bitwise operations;
//   the counts   h(f) = the rows with fill f, f = 1 .. 9: the planes or their complements under one mask, and a popcount;
//   the sum      greedy from the cheapest: take min(h(f), left) rows at 10 - f for f = 9 .. 1, and what is left at 10 -- the rows with
//                fill 0 or 10 and, past the twentieth, the fresh rows that L up to 250 asks for cost the same.
__device__ __forceinline__ void carry_save(uint32_t a, uint32_t b, uint32_t c, uint32_t& sum, uint32_t& carry) {
    const uint32_t ab = a ^ b;
    sum = ab ^ c;
    carry = (a & b) | (ab & c);
}

__device__ __forceinline__ uint32_t move_bound_cells(const uint32_t (&c)[tpl::kCols], uint32_t lines_left) {
    static_assert(tpl::kCols == 10, "the adder tree is written for ten columns");
    uint32_t s0, s1, s2, s3, k0, k1, k2, k3;
    carry_save(c[0], c[1], c[2], s0, k0);
    carry_save(c[3], c[4], c[5], s1, k1);
    carry_save(c[6], c[7], c[8], s2, k2);
    carry_save(s0, s1, s2, s3, k3);
    const uint32_t p0 = s3 ^ c[9], k4 = s3 & c[9];            // the ones; k0 .. k4 are twos
    uint32_t t0, m0, p1, m1;
    carry_save(k0, k1, k2, t0, m0);
    carry_save(t0, k3, k4, p1, m1);                            // m0 and m1 are fours; a fill is at most ten, so one eight at most
    const uint32_t p2 = m0 ^ m1, p3 = m0 & m1;
    uint32_t left = lines_left, cells = 0u;
#pragma unroll
    for (int f = 9; f >= 1; --f) {
        const uint32_t rows = tpl::kColMask & ((f & 1) ? p0 : ~p0) & ((f & 2) ? p1 : ~p1) & ((f & 4) ? p2 : ~p2) & ((f & 8) ? p3 : ~p3);
        const uint32_t take = min((uint32_t)__builtin_popcount(rows), left);
        cells += __umul24(take, (uint32_t)(10 - f));
        left -= take;
    }
    return cells + __umul24(left, 10u);                        // at most 2,500
}

// What a running board with `lines` rows cleared after `moves` moves still owes and still has under the game's L and M: cells as
// above for the L - lines rows owed, spare = 4 (M - moves) - cells, both 0 for a finished board; spare < 0 is a DEAD board.
struct MoveBound { uint32_t cells; int32_t spare; };
__device__ __forceinline__ MoveBound move_bound(const tpl::Board& s, uint32_t L, uint32_t M) {
    const bool running = s.state == tpl::ST_RUNNING;
    MoveBound out;
    out.cells = running ? move_bound_cells(s.c, L > s.lines ? L - s.lines : 0u) : 0u;
    out.spare = running ? 4 * ((int32_t)M - (int32_t)s.moves) - (int32_t)out.cells : 0;
    return out;
}

// The one place where a bounded kernel parts from its twin (include/tpl_learn.h, the bounded form), after the move and before psi:
// a running board that is dead becomes lost at the limit, and the spare cells of the board as it then stands are returned for the
// value's last term.  In an unbounded unit this is nothing and returns 0.
__device__ __forceinline__ int32_t bounded_move(tpl::Board& s, uint32_t L, uint32_t M) {
    if constexpr (kUnitBound) {
        const MoveBound bound = move_bound(s, L, M);
        const bool dead = bound.spare < 0;
        s.state = dead ? (uint32_t)tpl::ST_LOST_LIMIT : s.state;
        return dead ? 0 : bound.spare;
    } else {
        return 0;
    }
}

// value = w . phi, then + spare_weight * float(spare): one rounded multiply and one rounded add, made last; contraction off
__device__ __forceinline__ float bounded_value(float score, float spare_weight, int32_t spare) {
#pragma clang fp contract(off)
    const float term = spare_weight * (float)spare;
    return score + term;
}

// float32 -> uint32 with the order of the floats; -0 and +0 get one image, as they compare equal
__device__ __forceinline__ uint32_t ordered_bits(float x) {
    uint32_t u = __float_as_uint(x);
    u = u == 0x80000000u ? 0u : u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

constexpr uint32_t kNoSecond = 255u;

// The second ply with the known next piece: the best  worth(s2, n2)  among the distinct placements of s1's current piece on s1,
// the popped and still running board a first move left, and in `second` the placement it belongs to.  Copies s1, moves (s2 is
// what the move leaves, its window not yet popped, n2 the move's carry: the rows it cleared at 12 features; `worth` may change s2) and scores once per distinct
// placement in ascending b = 10 r2 + l2 -- 9, 17 or 34 trips, the same for the 40 lanes of a board -- and keeps a running
// best under a strict > on the ordered key, so the lowest b survives.  r2 and l2 are values out of the packed widths, never
// register indices.  The one loop of tpl_placement_search and tpl_ntuple_search: they enumerate and tie-break alike by it.
template <int kF = kFeatures, typename Worth>
__device__ __forceinline__ float best_second(const tpl::Board& s1, const tpl::ShapeWord* shape, uint32_t L, uint32_t M,
                                             uint32_t& second, Worth worth) {
    const uint32_t nxt = s1.window & 7u;
    const uint32_t last_rot = last_rotation(nxt);
    uint32_t best_key = 0u, r2 = 0u, l2 = 0u;
    float best = 0.0f;
#pragma unroll 1
    while (r2 <= last_rot) {
        tpl::Board s2 = s1;
        const uint32_t n2 = placed_move<kF>(s2, shape, r2, l2, L, M);
        const float q = worth(s2, n2);
        const uint32_t key = ordered_bits(q);                           // never 0, so the first trip is taken
        if (key > best_key) { best_key = key; best = q; second = 10u * r2 + l2; }
        next_placement(nxt, r2, l2);
    }
    return best;
}

// the checks of every entry point that reads n states from a pair of planes; `name` leads the message.  L and M are the
// environment's (tpl_create): move_board adds up to four rows to `lines` before pack_board writes it into eight bits
inline int check_planes(const char* name, const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M) {
    if (!plane_a || !plane_b) return fail_msg(TPL_ERR_ARG, "%s: null pointer", name);
    if (n < 1) return fail_msg(TPL_ERR_ARG, "%s: n must be positive", name);
    if (n >= (((int64_t)1 << 31) + kActions - 1) / kActions)
        return fail_msg(TPL_ERR_ARG, "%s: n too large (40 n must stay below 2^31)", name);
    if (L < 1 || L > 250 || M < 1 || M > 254)
        return fail_msg(TPL_ERR_ARG, "%s: L and M must be in [1, 250] and [1, 254]", name);
    if (((uintptr_t)plane_a & 15u) || ((uintptr_t)plane_b & 15u))
        return fail_msg(TPL_ERR_ARG, "%s: planes must be 16-byte aligned", name);
    return TPL_OK;
}

// what every policy entry refuses besides check_planes (tpl_placement_act's list in include/tpl_learn.h)
inline int check_policy(const char* name, const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M,
                        const float* weights, int64_t boards_per_member, const uint8_t* action, const float* score) {
    if (const int rc = check_planes(name, plane_a, plane_b, n, L, M)) return rc;
    if (!weights || !action) return fail_msg(TPL_ERR_ARG, "%s: null pointer (weights and action are required)", name);
    if (boards_per_member < 1) return fail_msg(TPL_ERR_ARG, "%s: boards_per_member must be positive", name);
    if ((uintptr_t)weights & 15u) return fail_msg(TPL_ERR_ARG, "%s: weights must be 16-byte aligned", name);
    if ((uintptr_t)score & 3u) return fail_msg(TPL_ERR_ARG, "%s: score must be 4-byte aligned", name);
    return TPL_OK;
}

}  // namespace tpl_learn
