// tpl_ntuple.h -- what the units that read an n-tuple table share (ntuple.hip, ntuple_beam.hip; include/tpl_learn.h states the
// rule): the geometry of the two table shapes, of their sum, of a staged table of any of the three, of a feature table and of a budget
// table, the counter index, the
// 32-bit addressing of an entry, the sum and the value of a running board, and the shape, form and table checks of the entry points.
#pragma once

#include "tpl_placement.h"

namespace tpl_learn {

constexpr int kCounterLines = 16, kCounterMoves = 64;
constexpr int kCounters = kCounterLines * kCounterMoves;      // 1,024

// The geometry of a table, one trait per TPL_NTUPLE_SHAPE_*: a window of kWindowCols adjacent columns by kWindowRows rows, its
// top-left cell at column x < kTupleCols and row y < kTupleRows, so that every window lies inside the board.  The device bodies
// below are templates over it; each __global__ kernel names its trait.
struct Shape2x4 {
    static constexpr int kWindowCols = 2, kWindowRows = 4;
    static constexpr int kTupleCols = tpl::kCols - 1;         // x = 0..8: columns x and x + 1
    static constexpr int kTupleRows = tpl::kRows - 3;         // y = 0..16: rows y .. y + 3
    static constexpr int kTuples = kTupleCols * kTupleRows;   // 153
    static constexpr int kPatterns = 256;
    static constexpr int kPieceStride = kTuples * kPatterns;
    static constexpr int kCounterBase = 8 * kPieceStride;     // 313,344
    static constexpr int kEntries = kCounterBase + kCounters;
    // the pattern of tuple (x, y): the two columns' nibbles at row y
    static __device__ __forceinline__ uint32_t pattern(const uint32_t (&c)[tpl::kCols], int x, uint32_t y) {
        return ((c[x] >> y) & 15u) | (((c[x + 1] >> y) & 15u) << 4);
    }
    // the pattern of the reflected window: the nibbles swapped
    static __device__ __forceinline__ uint32_t mirrored(uint32_t q) { return (q >> 4) | ((q & 15u) << 4); }
};
static_assert(Shape2x4::kEntries == TPL_NTUPLE_ENTRIES, "the table layout of include/tpl_learn.h");

struct Shape3x3 {
    static constexpr int kWindowCols = 3, kWindowRows = 3;
    static constexpr int kTupleCols = tpl::kCols - 2;         // x = 0..7: columns x, x + 1 and x + 2
    static constexpr int kTupleRows = tpl::kRows - 2;         // y = 0..17: rows y .. y + 2
    static constexpr int kTuples = kTupleCols * kTupleRows;   // 144
    static constexpr int kPatterns = 512;
    static constexpr int kPieceStride = kTuples * kPatterns;
    static constexpr int kCounterBase = 8 * kPieceStride;     // 589,824
    static constexpr int kEntries = kCounterBase + kCounters;
    // the pattern of tuple (x, y): the three columns' triplets at row y
    static __device__ __forceinline__ uint32_t pattern(const uint32_t (&c)[tpl::kCols], int x, uint32_t y) {
        return ((c[x] >> y) & 7u) | (((c[x + 1] >> y) & 7u) << 3) | (((c[x + 2] >> y) & 7u) << 6);
    }
    // the pattern of the reflected window: the outer triplets swapped, the middle one stays
    static __device__ __forceinline__ uint32_t mirrored(uint32_t q) { return (q >> 6) | (q & 0x38u) | ((q & 7u) << 6); }
};
static_assert(Shape3x3::kEntries == TPL_NTUPLE_ENTRIES_3X3, "the table layout of include/tpl_learn.h");

// k = 64 min(max(L - lines, 0), 15) + min(max(M - moves, 0), 63)
__device__ __forceinline__ uint32_t counter_index(uint32_t L, uint32_t M, uint32_t lines, uint32_t moves) {
    const int left_l = min(max((int)L - (int)lines, 0), kCounterLines - 1);
    const int left_m = min(max((int)M - (int)moves, 0), kCounterMoves - 1);
    return (uint32_t)(left_l * kCounterMoves + left_m);
}

// entry `index` of the table through a 32-bit byte offset from the (uniform) base: the largest buffer, a staged sum table, is 29 MB, and an
// index the compiler has to widen costs a 64-bit shift and a 64-bit add per look-up
template <typename T>
__device__ __forceinline__ T* entry(T* table, uint32_t index) {
    return (T*)((const char*)table + index * (uint32_t)sizeof(T));
}

// The index of pattern q of tuple (x, y) among the rows of the piece that start at `base`, a multiple of kPatterns: the row,
// then q in its low eight (3 x 3: nine) bits.  | q and not + q: the sum is the same, but as a function's + the compiler reassociates it and then
// addresses the gathers with 64-bit adds (172 vector instructions for 156 in ntuple_value_kernel).
template <typename S>
__device__ __forceinline__ uint32_t tuple_entry(uint32_t base, int x, uint32_t y, uint32_t q) {
    static_assert((S::kPatterns & (S::kPatterns - 1)) == 0 && S::kPatterns == 1 << (S::kWindowCols * S::kWindowRows) &&
                      S::kPieceStride % S::kPatterns == 0,
                  "a row's index has the pattern's low bits clear");
    return (base + ((uint32_t)(x * S::kTupleRows) + y) * (uint32_t)S::kPatterns) | q;
}

// The integer value of a running board with column words c (bits 20.. clear), falling piece `piece` and counter entry k: the
// sum over the tuples with a non-zero pattern plus the counter, exact in 64 bits.  `at`: the entry of `table` where the table of
// shape S starts, a multiple of kPatterns (tuple_entry) -- 0, or a stage's block of a staged table: a lane's own offset joins the
// 32-bit index, and the pointer stays the wave's.
template <typename S>
__device__ __forceinline__ long long ntuple_sum(const uint32_t (&c)[tpl::kCols], uint32_t piece, uint32_t k, const int32_t* table,
                                                uint32_t at = 0u) {
    const uint32_t base = at + piece * (uint32_t)S::kPieceStride;
    long long sum = *entry(table, at + (uint32_t)S::kCounterBase + k);
#pragma unroll 1
    for (uint32_t y = 0; y < (uint32_t)S::kTupleRows; ++y) {
        int32_t v[S::kTupleCols];
#pragma unroll
        for (int x = 0; x < S::kTupleCols; ++x) {
            const uint32_t q = S::pattern(c, x, y);
            const int32_t e = *entry(table, tuple_entry<S>(base, x, y, q));
            v[x] = q ? e : 0;
        }
#pragma unroll
        for (int x = 0; x < S::kTupleCols; ++x) sum += v[x];
    }
    return sum;
}

// The composite geometry of a SUM TABLE (include/tpl_learn.h): a whole table of shape First at the buffer's base, then a whole
// table of shape Second, each with its own counters.  It has no windows of its own: the bodies that read a table (value_lane,
// ntuple_policy, ntuple_beam) reach it through board_sum alone, so they stay written once.
template <typename A, typename B, int kEntriesOfFirst>
struct SumOf {
    using First = A;
    using Second = B;
    static constexpr uint32_t kSecondAt = kEntriesOfFirst;    // the entry where the second part starts
    static constexpr int kEntries = kEntriesOfFirst + B::kEntries;
};
using ShapeSum = SumOf<Shape2x4, Shape3x3, TPL_NTUPLE_ENTRIES>;
static_assert(ShapeSum::kSecondAt + TPL_NTUPLE_ENTRIES_3X3 == TPL_NTUPLE_ENTRIES_SUM && (ShapeSum::kSecondAt * sizeof(int32_t)) % 16 == 0 &&
                  (ShapeSum::kSecondAt * 2 * sizeof(int64_t)) % 16 == 0,
              "the sum table's layout of include/tpl_learn.h: the second part is a 16-byte aligned table (and coherence buffer)");

// The integer value of a running board under the table of geometry S.  A plain shape: ntuple_sum.  A sum of shapes: the two parts'
// sums, integers added before the one rounding -- two gather loops one after the other from one (uniform) table pointer, each
// part with its own counter base, so no more gathers are in flight than in the wider of the two.
template <typename S>
struct BoardSum {
    static __device__ __forceinline__ long long of(const uint32_t (&c)[tpl::kCols], uint32_t piece, uint32_t k, const int32_t* table) {
        return ntuple_sum<S>(c, piece, k, table);
    }
};
template <typename A, typename B, int kEntriesOfFirst>
struct BoardSum<SumOf<A, B, kEntriesOfFirst>> {
    static __device__ __forceinline__ long long of(const uint32_t (&c)[tpl::kCols], uint32_t piece, uint32_t k, const int32_t* table) {
        return ntuple_sum<A>(c, piece, k, table) + ntuple_sum<B>(c, piece, k, table + kEntriesOfFirst);
    }
};

// The geometry of a STAGED TABLE of the form S (include/tpl_learn.h): TPL_NTUPLE_STAGES whole tables of S one behind the other, then
// the stage map, an int32 per counter index.  Like SumOf it has no windows of its own and is reached through board_sum alone: the
// state's k picks the block, one dword gathered from the 4 KB map, and the block's offset goes into ntuple_sum's 32-bit index.
template <typename S>
struct StagedOf {
    using Stage = S;
    static constexpr uint32_t kStride = S::kEntries;          // entries from a stage's block to the next
    static constexpr uint32_t kMapAt = TPL_NTUPLE_STAGES * kStride;
    static constexpr int kEntries = kMapAt + kCounters;
};
static_assert(StagedOf<Shape2x4>::kEntries == TPL_NTUPLE_ENTRIES_STAGED && StagedOf<Shape3x3>::kEntries == TPL_NTUPLE_ENTRIES_STAGED_3X3 &&
                  StagedOf<ShapeSum>::kEntries == TPL_NTUPLE_ENTRIES_STAGED_SUM,
              "the staged tables' layout of include/tpl_learn.h");
static_assert(Shape2x4::kEntries % 512 == 0 && Shape3x3::kEntries % 512 == 0,
              "every stage's block, and every part in it, starts at a multiple of both shapes' kPatterns (tuple_entry) and of 16 bytes");
static_assert((unsigned long long)StagedOf<ShapeSum>::kEntries * sizeof(int32_t) < (1ull << 31), "byte offsets fit 32 bits");

// The offset of the block of the stage that counter index k falls in: (map[k] & 7) * stride.  The mask is the rule, not a guard: a
// map that holds anything addresses a block of the buffer.  `map_at`: the entry of `table` where the map starts.
__device__ __forceinline__ uint32_t stage_offset(const int32_t* table, uint32_t map_at, uint32_t k, uint32_t stride) {
    return ((uint32_t)*entry(table, map_at + k) & (uint32_t)(TPL_NTUPLE_STAGES - 1)) * stride;
}

// The board sum of the form S from the block that starts at entry `at`: ntuple_sum, or for a sum of shapes the two parts' sums.
template <typename S>
struct BlockSum {
    static __device__ __forceinline__ long long of(const uint32_t (&c)[tpl::kCols], uint32_t piece, uint32_t k, const int32_t* table, uint32_t at) {
        return ntuple_sum<S>(c, piece, k, table, at);
    }
};
template <typename A, typename B, int kEntriesOfFirst>
struct BlockSum<SumOf<A, B, kEntriesOfFirst>> {
    static __device__ __forceinline__ long long of(const uint32_t (&c)[tpl::kCols], uint32_t piece, uint32_t k, const int32_t* table, uint32_t at) {
        return ntuple_sum<A>(c, piece, k, table, at) + ntuple_sum<B>(c, piece, k, table, at + (uint32_t)kEntriesOfFirst);
    }
};
template <typename S>
struct BoardSum<StagedOf<S>> {
    static __device__ __forceinline__ long long of(const uint32_t (&c)[tpl::kCols], uint32_t piece, uint32_t k, const int32_t* table) {
        return BlockSum<S>::of(c, piece, k, table, stage_offset(table, StagedOf<S>::kMapAt, k, StagedOf<S>::kStride));
    }
};

// The geometry of a FEATURE TABLE (include/tpl_learn.h, "Feature tuples"): per falling piece nine rows of 256 bins, row j looked up
// at min(phi_{3 + j}, 255) of the board, then the counters.  It has no windows: it is reached through BoardSum alone, like SumOf.
struct FeatureTable {
    static constexpr int kFeatureRows = TPL_NTUPLE_FEATURES, kBins = TPL_NTUPLE_FEATURE_BINS;
    static constexpr int kPieceStride = kFeatureRows * kBins;  // 2,304
    static constexpr int kCounterBase = 8 * kPieceStride;      // 18,432
    static constexpr int kEntries = kCounterBase + kCounters;
};
static_assert(FeatureTable::kEntries == TPL_NTUPLE_ENTRIES_FEAT && FeatureTable::kFeatureRows == kFeatures - 3,
              "the feature table's layout of include/tpl_learn.h: phi_3 .. phi_11");

// the nine bins of a board: board_features on the column words, each clamped to the last bin (only wells can pass it)
__device__ __forceinline__ void feature_bins(const uint32_t (&c)[tpl::kCols], uint32_t (&q)[FeatureTable::kFeatureRows]) {
    Features phi;
    board_features(c, phi);
#pragma unroll
    for (int j = 0; j < FeatureTable::kFeatureRows; ++j) q[j] = min(phi.f[3 + j], (uint32_t)(FeatureTable::kBins - 1));
}

// the index of bin q of feature j among the rows of the piece that start at `base`
__device__ __forceinline__ uint32_t feature_entry(uint32_t base, int j, uint32_t q) { return base + (uint32_t)(j * FeatureTable::kBins) + q; }

// The integer value of a running board under a feature table: the nine gathers, all in flight at once, and the counter.  Every one of
// them is used: a board without holes reads bin 0.
__device__ __forceinline__ long long feature_sum(const uint32_t (&c)[tpl::kCols], uint32_t piece, uint32_t k, const int32_t* table) {
    uint32_t q[FeatureTable::kFeatureRows];
    feature_bins(c, q);
    const uint32_t base = piece * (uint32_t)FeatureTable::kPieceStride;
    int32_t v[FeatureTable::kFeatureRows];
#pragma unroll
    for (int j = 0; j < FeatureTable::kFeatureRows; ++j) v[j] = *entry(table, feature_entry(base, j, q[j]));
    long long sum = *entry(table, (uint32_t)FeatureTable::kCounterBase + k);
#pragma unroll
    for (int j = 0; j < FeatureTable::kFeatureRows; ++j) sum += v[j];
    return sum;
}

template <>
struct BoardSum<FeatureTable> {
    static __device__ __forceinline__ long long of(const uint32_t (&c)[tpl::kCols], uint32_t piece, uint32_t k, const int32_t* table) {
        return feature_sum(c, piece, k, table);
    }
};
// a window table with a feature table behind it: the window part's gather loop, then the nine gathers, integers added before the one rounding
template <typename A, int kEntriesOfFirst>
struct BoardSum<SumOf<A, FeatureTable, kEntriesOfFirst>> {
    static __device__ __forceinline__ long long of(const uint32_t (&c)[tpl::kCols], uint32_t piece, uint32_t k, const int32_t* table) {
        return ntuple_sum<A>(c, piece, k, table) + feature_sum(c, piece, k, table + kEntriesOfFirst);
    }
};
using Shape3x3Feature = SumOf<Shape3x3, FeatureTable, TPL_NTUPLE_ENTRIES_3X3>;
static_assert(Shape3x3Feature::kEntries == TPL_NTUPLE_ENTRIES_3X3_FEAT && (Shape3x3Feature::kSecondAt * sizeof(int32_t)) % 16 == 0,
              "the 3 x 3 + feature table's layout of include/tpl_learn.h: the feature part is a 16-byte aligned table");

// The geometry of a BUDGET TABLE (include/tpl_learn.h, "The budget table"): a feature table with a tenth row per falling piece, read
// at the spare cells of the move bound.  That row is indexed by the board's own lines and moves under the game's L and M -- not by the
// clamped counter index k --, so this geometry is not reached through BoardSum, which sees k alone: ntuple_value below hands the
// board and the game to budget_sum, and every other geometry goes the way it went.
struct BudgetTable {
    static constexpr int kFeatureRows = TPL_NTUPLE_FEATURES, kBins = TPL_NTUPLE_FEATURE_BINS;
    static constexpr int kRows = TPL_NTUPLE_BUDGET_ROWS;      // the nine feature rows, then the spare row
    static constexpr int kSpareRow = kFeatureRows;
    static constexpr int kPieceStride = kRows * kBins;        // 2,560
    static constexpr int kCounterBase = 8 * kPieceStride;     // 20,480
    static constexpr int kEntries = kCounterBase + kCounters;
};
static_assert(BudgetTable::kEntries == TPL_NTUPLE_ENTRIES_BUDGET && BudgetTable::kRows == BudgetTable::kFeatureRows + 1,
              "the budget table's layout of include/tpl_learn.h");

// sbin of a board: 0 where it is dead, else min(spare + 1, 255) of move_bound as it stands (a finished board has spare 0: bin 1)
__device__ __forceinline__ uint32_t spare_bin(const tpl::Board& s, uint32_t L, uint32_t M) {
    const MoveBound bound = move_bound(s, L, M);
    return bound.spare < 0 ? 0u : (uint32_t)min(bound.spare + 1, BudgetTable::kBins - 1);
}

// the ten bins of a board: feature_bins, then sbin
__device__ __forceinline__ void budget_bins(const tpl::Board& s, uint32_t L, uint32_t M, uint32_t (&q)[BudgetTable::kRows]) {
    uint32_t f[FeatureTable::kFeatureRows];
    feature_bins(s.c, f);
#pragma unroll
    for (int j = 0; j < BudgetTable::kFeatureRows; ++j) q[j] = f[j];
    q[BudgetTable::kSpareRow] = spare_bin(s, L, M);
}

// the index of bin q of row j among the rows of the piece that start at `base`
__device__ __forceinline__ uint32_t budget_entry(uint32_t base, int j, uint32_t q) { return base + (uint32_t)(j * BudgetTable::kBins) + q; }

// The integer value of a running board under a budget table: the ten gathers, all in flight at once, and the counter
__device__ __forceinline__ long long budget_sum(const tpl::Board& s, uint32_t L, uint32_t M, const int32_t* table) {
    uint32_t q[BudgetTable::kRows];
    budget_bins(s, L, M, q);
    const uint32_t base = (s.window & 7u) * (uint32_t)BudgetTable::kPieceStride;
    int32_t v[BudgetTable::kRows];
#pragma unroll
    for (int j = 0; j < BudgetTable::kRows; ++j) v[j] = *entry(table, budget_entry(base, j, q[j]));
    long long sum = *entry(table, (uint32_t)BudgetTable::kCounterBase + counter_index(L, M, s.lines, s.moves));
#pragma unroll
    for (int j = 0; j < BudgetTable::kRows; ++j) sum += v[j];
    return sum;
}

// whether a geometry's policies know the dead-board prune: the budget table's alone
template <typename S> struct KnowsBudget { static constexpr bool value = false; };
template <> struct KnowsBudget<BudgetTable> { static constexpr bool value = true; };
template <typename S> constexpr bool kBudgetGeometry = KnowsBudget<S>::value;

// The prune (include/tpl_learn.h): with `prune` set, a RUNNING board that is dead becomes lost at the limit, and the caller scores
// and expands it as any board in that state.  Nothing, and no code, under any other geometry.
template <typename S>
__device__ __forceinline__ void prune_dead(tpl::Board& s, uint32_t L, uint32_t M, uint32_t prune) {
    if constexpr (kBudgetGeometry<S>) {
        const bool dead = prune != 0u && s.state == tpl::ST_RUNNING && move_bound(s, L, M).spare < 0;
        s.state = dead ? (uint32_t)tpl::ST_LOST_LIMIT : s.state;
    }
}

// V of a state that runs: one rounding from the 64-bit sum to float32, then an exact scaling by 2^-16
template <typename S>
__device__ __forceinline__ float ntuple_value(const tpl::Board& s, uint32_t L, uint32_t M, const int32_t* table) {
    long long sum;
    if constexpr (kBudgetGeometry<S>) sum = budget_sum(s, L, M, table);
    else sum = BoardSum<S>::of(s.c, s.window & 7u, counter_index(L, M, s.lines, s.moves), table);
    return (float)sum * 0x1p-16f;
}

// Which kernels an entry launches: the two shapes of tpl_ntuple_shape, and their sum, which is no `shape` of the C interface.  The
// _staged entries take all three as their `form` (tpl_ntuple_form has the enumerators' values).
// kFeature and k3x3Feature are the two tpl_ntuple_feature_form of the _feature entries, which no other entry takes.
// kBudget is the budget table of the _budget entries, which take no form: there is one.
enum class Form { k2x4, k3x3, kSum, kFeature, k3x3Feature, kBudget };
inline Form feature_form_of(int32_t form) { return form == TPL_NTUPLE_FEATURE_FORM_3X3 ? Form::k3x3Feature : Form::kFeature; }   // after check_feature_form

// a feature form the library does not know is refused first, before any pointer is looked at
inline int check_feature_form(const char* name, int32_t form) {
    if (form != TPL_NTUPLE_FEATURE_FORM_ALONE && form != TPL_NTUPLE_FEATURE_FORM_3X3)
        return fail_msg(TPL_ERR_ARG, "%s: form must be TPL_NTUPLE_FEATURE_FORM_ALONE (0) or TPL_NTUPLE_FEATURE_FORM_3X3 (1), got %d", name,
                        (int)form);
    return TPL_OK;
}
inline Form form_of(int32_t shape) { return shape == TPL_NTUPLE_SHAPE_3X3 ? Form::k3x3 : Form::k2x4; }   // after check_shape
static_assert((int)Form::k2x4 == TPL_NTUPLE_FORM_2X4 && (int)Form::k3x3 == TPL_NTUPLE_FORM_3X3 && (int)Form::kSum == TPL_NTUPLE_FORM_SUM,
              "a checked `form` converts to Form");

// a form the library does not know is refused first, before any pointer is looked at
inline int check_form(const char* name, int32_t form) {
    if (form != TPL_NTUPLE_FORM_2X4 && form != TPL_NTUPLE_FORM_3X3 && form != TPL_NTUPLE_FORM_SUM)
        return fail_msg(TPL_ERR_ARG, "%s: form must be TPL_NTUPLE_FORM_2X4 (0), TPL_NTUPLE_FORM_3X3 (1) or TPL_NTUPLE_FORM_SUM (2), got %d",
                        name, (int)form);
    return TPL_OK;
}

// a shape the library does not know is refused first, before any pointer is looked at
inline int check_shape(const char* name, int32_t shape) {
    if (shape != TPL_NTUPLE_SHAPE_2X4 && shape != TPL_NTUPLE_SHAPE_3X3)
        return fail_msg(TPL_ERR_ARG, "%s: shape must be TPL_NTUPLE_SHAPE_2X4 (0) or TPL_NTUPLE_SHAPE_3X3 (1), got %d", name, (int)shape);
    return TPL_OK;
}

// the checks the entries share beyond check_planes
inline int check_table(const char* name, const void* table) {
    if (!table) return fail_msg(TPL_ERR_ARG, "%s: null pointer (table is required)", name);
    if ((uintptr_t)table & 15u) return fail_msg(TPL_ERR_ARG, "%s: table must be 16-byte aligned", name);
    return TPL_OK;
}

}  // namespace tpl_learn
