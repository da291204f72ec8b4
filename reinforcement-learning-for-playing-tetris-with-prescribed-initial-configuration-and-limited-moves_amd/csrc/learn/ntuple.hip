// ntuple.hip -- an n-tuple afterstate value function, its greedy / epsilon-greedy placement policy and its temporal-difference
// update: tpl_ntuple_value, tpl_ntuple_act, tpl_ntuple_search, tpl_ntuple_update, tpl_ntuple_update_trace,
// tpl_ntuple_update_coherent, their _shaped twins, the _sum twins of the first three and the _staged twins of value, act, search
// and update_trace (include/tpl_learn.h states the rule).
//
// The value of a board is a sum of table look-ups: 153 windows of two adjacent columns by four rows, each a 256-entry row of an
// int32 table chosen by the piece that falls next, plus one entry for the lines and moves that are left.  In the column layout a
// window's pattern is two shifts and two masks on column words that move_board leaves in registers, the sum is an exact integer,
// and the update is integer adds -- so value, policy and update are bit-reproducible whatever order anything runs in.
//
// Lane mapping.  value and update: a lane per state; a lane's 153 gathers (or adds) go out nine at a time, one trip of a loop
// over the window's top row y per nine column pairs, so nine are in flight per lane.  act: a lane per (board, action) PAIR in
// placement_policy's frame (heuristic.hip: blocks of 320 threads = 8 boards x 40 actions, first_move, a 64-bit LDS maximum on
// ordered score << 32 | 39 - a): the lanes of the distinct placements that leave the game running evaluate the board their move
// left, the chosen lane packs that board from its own registers -- nothing is enumerated twice.  The mapping rejected for act
// is a lane per board looping over the placements: it would have a fortieth of the gathers in flight, and the gathers, not the
// moves, are what a pair costs (DESIGN.md section 9 has the counts).
//
// search is act two plies deep in the same frame (ntuple_policy<kDepth> is the one body of both kernels): a lane whose first move
// leaves the game running holds that board in registers and loops over the distinct placements of the next piece -- 9, 17 or 34
// trips, the same for the 40 lanes of a board -- each trip a copy, a move, the pop and the 153 gathers on the board in
// registers.  A lane per (board, a, b) TRIPLE would have more gathers in flight, but 1,156 triples are no multiple of 64, the
// first move's board would be handed through LDS and the arg-max would have two levels; act measured bound by instruction issue
// and not by its gathers, so the loop is the form that is built.  What it leaves on the table first is the alias lanes, which
// idle through the loop.
//
// The all-empty pattern contributes nothing and is never updated: it is most of a board, and it would be the one address every
// board adds to.  The look-up is still made (the address is in bounds, and the 64 lanes of a wave share it where their pieces
// agree) and dropped by a select, so that the gathers stay straight-line code.  The counter entries -- 1,024, shared by every
// board with the same lines and moves left, which boards in lockstep have -- are summed per block in LDS first and only the
// non-zero sums go to memory.
//
// update_trace is update over the last `horizon` states of every board, kept in a ring of slots: a lane per (board, age) PAIR,
// the age in blockIdx.y, so that a wave's lanes read consecutive 16-byte words of one slot at every age and the decayed rate is
// one value per block.  There is one update kernel, ntuple_trace_kernel: tpl_ntuple_update launches it on its planes as a ring of
// one slot with a horizon of one, where age 0 has no younger slot to look at and a weight of exactly 1.  A lane first looks at the state field of the younger slots (a dword each, coalesced) and leaves where
// one of them does not run: what lies behind belongs to an earlier episode.  With kSymmetric every add is made a second time,
// at the entry of the reflected board (the piece through pi, tuple column 8 - x, the pattern's nibbles swapped), which keeps a
// mirror-symmetric table mirror-symmetric.  Ages of one board add in any order: the adds are integers and nothing is read.
//
// update_coherent is update_trace with a step size per entry, alpha = |E| / A from the signed and the absolute sum of the steps
// the entry was sent (a second buffer, 16 bytes an entry).  Two kernels in update_trace's frame, one after the other: the step
// kernel gathers an entry's pair in one 16-byte load, nine (symmetric: eighteen) in flight per lane as in value, and adds
// rint(rate * w * alpha * e) to the table; the accumulate kernel adds d and |d| to the pair with two 64-bit atomics.  Each reads
// only what the other writes, so the bytes of both buffers are again the same in any order.  The two share walk_entries, the walk
// over a state's entries with the per-entry action handed in; ntuple_trace_kernel keeps its own loop, since on the shared walk
// its instructions came out in another order (profiles/learner/README.md).
//
// Table shapes.  The geometry of the windows is a compile-time trait (Shape2x4, Shape3x3: the window, the tuple counts, the
// patterns per tuple, the piece stride, the counter base, pattern(c, x, y) and mirrored(q)), and everything above is a __device__
// template over it: ntuple_sum, tuple_entry, the trace kernel's loop, walk_entries, ntuple_policy.  Each __global__ kernel is a
// name and a trait: ntuple_*_kernel with Shape2x4 -- the numbers in this comment are that shape's -- and ntuple3_*_kernel with
// Shape3x3, 144 windows of three columns by three rows, eight (symmetric: sixteen) gathers or adds in flight per trip over 18
// rows.  The update bodies take the kernel's argument struct BY VALUE: by reference those kernels came out 18 instructions longer.
// The shape is an argument of the _shaped entries only; it picks the kernel on the host and is never seen on the device.
// The traits, ntuple_sum and ntuple_value live in tpl_ntuple.h, which the n-tuple beam (ntuple_beam.hip) includes as well.
//
// Two shapes summed (tpl_ntuple_value_sum, tpl_ntuple_act_sum, tpl_ntuple_search_sum).  ShapeSum is a composite trait: a 2 x 4
// table and a 3 x 3 table behind one pointer, whose board sum is the two gather loops one after the other (tpl_ntuple.h).  The
// three ntuple_sum_*_kernel are value_lane and ntuple_policy named with it, on the unchanged argument structs.  The updates have
// no such kernel: they never read the table, so the host sends one error array through the existing kernels once per part.
//
// Staged tables (the _staged entries).  StagedOf<S> is a second composite trait: eight tables of the form S and a map from the
// counter index to one of them (tpl_ntuple.h), so value_lane and ntuple_policy named with it are the nine ntuple_staged*_kernel,
// and a leaf of the two-ply search reads the block of its OWN lines and moves left.  The update does get kernels of its own here:
// where a state's adds go depends on its stage, so staged_trace_lane is trace_lane with the block's offset in every index.  It
// reads the map, which nothing writes, and adds to the blocks, which it never reads.
//
// Feature tuples (the _feature entries).  FeatureTable is a geometry without windows: nine rows of 256 bins per falling piece, row j
// read at min(phi_{3 + j}, 255) of board_features on the column words the lane holds (tpl_ntuple.h).  value_lane and ntuple_policy named
// with it, and with SumOf<Shape3x3, FeatureTable>, are the six ntuple_feature*_kernel.  The update is a kernel of its own,
// ntuple_feature_trace_kernel: a state's ten adds fall on a table of 19,456 entries that fits LDS whole, so a block sums its states'
// adds there and flushes what is not zero.  There is no staged and no coherent form.
//
// The budget table (the _budget entries).  BudgetTable is FeatureTable with a tenth row read at the spare cells of the move bound
// (tpl_ntuple.h).  That row needs the board's own lines and moves, which no BoardSum sees, so ntuple_value hands the board and the game to
// budget_sum: value_lane and ntuple_policy named with it are ntuple_budget_{value,act,search}_kernel.  The policies take the prune flag
// behind their argument struct; ntuple_policy reads it under `if constexpr` on the geometry, so every other instantiation is the code it
// was.  The update is ntuple_budget_trace_kernel, the feature update with eleven adds a state on an 84 KB image.
#include <algorithm>
#include <cmath>

#include "tpl_ntuple.h"

namespace tpl_learn {
namespace {

constexpr int kStateBlock = 256;                              // value and update: a lane per state
constexpr int kBoardsPerBlock = 8;
constexpr int kActBlock = kBoardsPerBlock * kActions;         // act: 320 threads, five waves, eight whole boards
static_assert(kActBlock % 64 == 0, "a block is whole waves");
static_assert(kCounters % kStateBlock == 0, "the counter sums are zeroed and flushed in whole rounds of a block");

struct ValueArgs {
    const uint4* a;              // [n]
    const uint4* b;
    uint32_t n;
    uint32_t L, M;
    const int32_t* table;        // [the shape's entries]
    float* value;                // [n]
};

template <typename S>
__device__ __forceinline__ void value_lane(const ValueArgs& p) {
    const uint32_t i = blockIdx.x * kStateBlock + threadIdx.x;
    if (i >= p.n) return;
    tpl::Board s;
    tpl::unpack_board(p.a[i], p.b[i], s);
    float v = 0.0f;
    if (s.state == tpl::ST_RUNNING) v = ntuple_value<S>(s, p.L, p.M, p.table);
    p.value[i] = v;
}

__global__ __launch_bounds__(kStateBlock) void ntuple_value_kernel(const ValueArgs p) { value_lane<Shape2x4>(p); }
__global__ __launch_bounds__(kStateBlock) void ntuple3_value_kernel(const ValueArgs p) { value_lane<Shape3x3>(p); }
__global__ __launch_bounds__(kStateBlock) void ntuple_sum_value_kernel(const ValueArgs p) { value_lane<ShapeSum>(p); }
__global__ __launch_bounds__(kStateBlock) void ntuple_staged_value_kernel(const ValueArgs p) { value_lane<StagedOf<Shape2x4>>(p); }
__global__ __launch_bounds__(kStateBlock) void ntuple_staged3_value_kernel(const ValueArgs p) { value_lane<StagedOf<Shape3x3>>(p); }
__global__ __launch_bounds__(kStateBlock) void ntuple_staged_sum_value_kernel(const ValueArgs p) { value_lane<StagedOf<ShapeSum>>(p); }
__global__ __launch_bounds__(kStateBlock) void ntuple_feature_value_kernel(const ValueArgs p) { value_lane<FeatureTable>(p); }
__global__ __launch_bounds__(kStateBlock) void ntuple_feature3_value_kernel(const ValueArgs p) { value_lane<Shape3x3Feature>(p); }
__global__ __launch_bounds__(kStateBlock) void ntuple_budget_value_kernel(const ValueArgs p) { value_lane<BudgetTable>(p); }

// ---- tpl_ntuple_feature_bins: the nine bins of every state, running or not ----
struct BinsArgs {
    const uint4* a;              // [n]
    const uint4* b;
    uint32_t n;
    uint8_t* bins;               // [n][9]
};

__global__ __launch_bounds__(kStateBlock) void ntuple_feature_bins_kernel(const BinsArgs p) {
    const uint32_t i = blockIdx.x * kStateBlock + threadIdx.x;
    if (i >= p.n) return;
    tpl::Board s;
    tpl::unpack_board(p.a[i], p.b[i], s);
    uint32_t q[FeatureTable::kFeatureRows];
    feature_bins(s.c, q);
#pragma unroll
    for (int j = 0; j < FeatureTable::kFeatureRows; ++j) p.bins[i * (uint32_t)FeatureTable::kFeatureRows + j] = (uint8_t)q[j];
}

// ---- tpl_ntuple_budget_bins: the ten bins of every state, running or not ----
struct BudgetBinsArgs {
    const uint4* a;              // [n]
    const uint4* b;
    uint32_t n;
    uint32_t L, M;
    uint8_t* bins;               // [n][10]
};

__global__ __launch_bounds__(kStateBlock) void ntuple_budget_bins_kernel(const BudgetBinsArgs p) {
    const uint32_t i = blockIdx.x * kStateBlock + threadIdx.x;
    if (i >= p.n) return;
    tpl::Board s;
    tpl::unpack_board(p.a[i], p.b[i], s);
    uint32_t q[BudgetTable::kRows];
    budget_bins(s, p.L, p.M, q);
#pragma unroll
    for (int j = 0; j < BudgetTable::kRows; ++j) p.bins[i * (uint32_t)BudgetTable::kRows + j] = (uint8_t)q[j];
}

// d = (int32) rint(rate * e): the product rounded once, clamped to +-2^24, 0 for a NaN
__device__ __forceinline__ int32_t update_step(float rate, float e) {
    const float x = rate * e;
    if (x != x) return 0;
    return (int32_t)rintf(fminf(fmaxf(x, -0x1p24f), 0x1p24f));
}

struct TraceArgs {
    const uint4* a;              // [slots][n], slot-major: the state of board i at age k in slot (head - k) mod slots
    const uint4* b;
    uint32_t n, slots, head;     // slots * n below 2^31 / 40: every index and byte offset fits 32 bits
    uint32_t L, M;
    uint32_t* table;             // [the shape's entries]: added to, never read
    const float* error;          // [n]
    float rate, decay;
};

constexpr uint32_t kPieceMirror = 0x76453120u;                // pi = [0, 2, 1, 3, 5, 4, 6, 7] (tpl_mirror.h), a nibble per piece

// Age blockIdx.y of the boards blockIdx.x * 256 ..: d = update_step(rate * decay^age, e) on the state of that age, where it
// and every younger state of the board run.  The weight is `age` rounded multiplies on a block-uniform value, as the rule has it.
template <typename S, bool kSymmetric>
__device__ __forceinline__ void trace_lane(const TraceArgs p) {
    __shared__ uint32_t s_counter[kCounters];
#pragma unroll
    for (int t = threadIdx.x; t < kCounters; t += kStateBlock) s_counter[t] = 0u;
    __syncthreads();
    const uint32_t age = blockIdx.y;                                    // below the horizon, which is at most `slots`
    float w = 1.0f;
    for (uint32_t k = 0; k < age; ++k) w = __fmul_rn(w, p.decay);
    const float rate = __fmul_rn(p.rate, w);
    const uint32_t i = blockIdx.x * kStateBlock + threadIdx.x;
    if (i < p.n) {
        bool open = true;
        for (uint32_t k = 0; k < age; ++k) {                            // the younger states: only the word that holds the state
            const uint32_t slot = p.head >= k ? p.head - k : p.head + p.slots - k;
            open = open && ((p.b[slot * p.n + i].y >> 28) & 3u) == tpl::ST_RUNNING;
        }
        const uint32_t d = (uint32_t)update_step(rate, p.error[i]);
        if (open && d != 0u) {
            const uint32_t slot = p.head >= age ? p.head - age : p.head + p.slots - age;
            tpl::Board s;
            tpl::unpack_board(p.a[slot * p.n + i], p.b[slot * p.n + i], s);
            if (s.state == tpl::ST_RUNNING) {
                atomicAdd(&s_counter[counter_index(p.L, p.M, s.lines, s.moves)], d);      // once, symmetric or not
                const uint32_t piece = s.window & 7u;
                const uint32_t base = piece * (uint32_t)S::kPieceStride;
                const uint32_t mirror_base = ((kPieceMirror >> (4u * piece)) & 7u) * (uint32_t)S::kPieceStride;
#pragma unroll 1
                for (uint32_t y = 0; y < (uint32_t)S::kTupleRows; ++y) {
#pragma unroll
                    for (int x = 0; x < S::kTupleCols; ++x) {
                        const uint32_t q = S::pattern(s.c, x, y);
                        if (q) {
                            atomicAdd(entry(p.table, tuple_entry<S>(base, x, y, q)), d);
                            if constexpr (kSymmetric) {                 // both adds, also where the two entries are one
                                const uint32_t swapped = S::mirrored(q);
                                atomicAdd(entry(p.table, tuple_entry<S>(mirror_base, S::kTupleCols - 1 - x, y, swapped)), d);
                            }
                        }
                    }
                }
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int t = threadIdx.x; t < kCounters; t += kStateBlock) {
        const uint32_t sum = s_counter[t];
        if (sum) atomicAdd(p.table + S::kCounterBase + t, sum);
    }
}

template <bool kSymmetric>
__global__ __launch_bounds__(kStateBlock) void ntuple_trace_kernel(const TraceArgs p) { trace_lane<Shape2x4, kSymmetric>(p); }
template <bool kSymmetric>
__global__ __launch_bounds__(kStateBlock) void ntuple3_trace_kernel(const TraceArgs p) { trace_lane<Shape3x3, kSymmetric>(p); }

// ---- the feature table's update: tpl_ntuple_update_trace_feature ----
// What a lane does before its adds, trace_lane's lines for the state of board i at age `age`: the younger states'
// state words, the step and the state of that age.  True where the lane adds: `d` is not 0 and `s` runs.
__device__ __forceinline__ bool feature_trace_state(const TraceArgs& p, uint32_t i, uint32_t age, float rate, uint32_t& d, tpl::Board& s) {
    bool open = true;
    for (uint32_t k = 0; k < age; ++k) {
        const uint32_t slot = p.head >= k ? p.head - k : p.head + p.slots - k;
        open = open && ((p.b[slot * p.n + i].y >> 28) & 3u) == tpl::ST_RUNNING;
    }
    d = (uint32_t)update_step(rate, p.error[i]);
    if (!open || d == 0u) return false;
    const uint32_t slot = p.head >= age ? p.head - age : p.head + p.slots - age;
    tpl::unpack_board(p.a[slot * p.n + i], p.b[slot * p.n + i], s);
    return s.state == tpl::ST_RUNNING;
}

// rate * decay^age: `age` rounded multiplies on a block-uniform value, as the rule has it
__device__ __forceinline__ float aged_rate(const TraceArgs& p, uint32_t age) {
    float w = 1.0f;
    for (uint32_t k = 0; k < age; ++k) w = __fmul_rn(w, p.decay);
    return __fmul_rn(p.rate, w);
}

// The update kernel: a block holds an image of the WHOLE table in LDS (19,456 dwords, 76 KB of the 160 KB a gfx950 workgroup may
// declare: two blocks a CU), walks the states i = blockIdx.x * 512 + tid, + 512 gridDim.x, ... of its age, adds every state's ten
// entries (symmetric: nineteen) there with LDS atomics, and flushes the non-zero sums with one atomic add to memory each.  All adds are
// integers modulo 2^32, so the bytes are those of an atomic add to memory per entry -- the form this one was measured against
// (profiles/learner/ntuple_feature_update_forms.log): boards in lockstep send ten million adds to a few thousand addresses.
constexpr int kCombineBlock = 512;
// The blocks of one age, at the most: two blocks of 76 KB fit the 160 KB of a CU's LDS, and the MI355X this was measured on has 256
// CUs -- one resident round of the device.  An ASSUMPTION about the device, not a bound: with more blocks each would zero and scan the
// whole image for fewer states, with fewer CUs the blocks run in more than one round.  Other caps were not measured.
constexpr uint32_t kCombineBlocksPerCU = 2, kCombineCUs = 256, kCombineMaxBlocks = kCombineBlocksPerCU * kCombineCUs;
static_assert(FeatureTable::kEntries % kCombineBlock == 0, "the image is zeroed and flushed in whole rounds of a block");

template <bool kSymmetric>
__global__ __launch_bounds__(kCombineBlock) void ntuple_feature_trace_kernel(const TraceArgs p) {
    __shared__ uint32_t s_sum[FeatureTable::kEntries];
#pragma unroll 1
    for (int t = threadIdx.x; t < FeatureTable::kEntries; t += kCombineBlock) s_sum[t] = 0u;
    __syncthreads();
    const uint32_t age = blockIdx.y;
    const float rate = aged_rate(p, age);
#pragma unroll 1
    for (uint32_t i = blockIdx.x * kCombineBlock + threadIdx.x; i < p.n; i += gridDim.x * kCombineBlock) {
        uint32_t d;
        tpl::Board s;
        if (!feature_trace_state(p, i, age, rate, d, s)) continue;
        atomicAdd(&s_sum[(uint32_t)FeatureTable::kCounterBase + counter_index(p.L, p.M, s.lines, s.moves)], d);
        uint32_t q[FeatureTable::kFeatureRows];
        feature_bins(s.c, q);
        const uint32_t piece = s.window & 7u;
        const uint32_t base = piece * (uint32_t)FeatureTable::kPieceStride;
        const uint32_t mirror_base = ((kPieceMirror >> (4u * piece)) & 7u) * (uint32_t)FeatureTable::kPieceStride;
#pragma unroll
        for (int j = 0; j < FeatureTable::kFeatureRows; ++j) {
            atomicAdd(&s_sum[feature_entry(base, j, q[j])], d);
            if constexpr (kSymmetric) atomicAdd(&s_sum[feature_entry(mirror_base, j, q[j])], d);
        }
    }
    __syncthreads();
#pragma unroll 1
    for (int t = threadIdx.x; t < FeatureTable::kEntries; t += kCombineBlock) {
        const uint32_t sum = s_sum[t];
        if (sum) atomicAdd(p.table + t, sum);
    }
}

// ---- the budget table's update: tpl_ntuple_update_trace_budget ----
// ntuple_feature_trace_kernel on the budget table: the image is 21,504 dwords, 84 KB, so ONE block fits the 160 KB of a CU's LDS, and it
// is a block of 1,024 threads -- the sixteen waves the two feature blocks of 512 bring to a CU between them.  A state's eleven entries
// (symmetric: twenty-one) go to the image with LDS atomics; every index is below kEntries by the two clamps of the rule.
constexpr int kBudgetBlock = 1024;
constexpr uint32_t kBudgetMaxBlocks = kCombineCUs;            // one block a CU: one resident round of the device, as above an assumption
static_assert(BudgetTable::kEntries % kBudgetBlock == 0, "the image is zeroed and flushed in whole rounds of a block");
static_assert(BudgetTable::kEntries * sizeof(uint32_t) <= 160 * 1024, "the image fits the LDS a gfx950 workgroup may declare");

template <bool kSymmetric>
__global__ __launch_bounds__(kBudgetBlock) void ntuple_budget_trace_kernel(const TraceArgs p) {
    __shared__ uint32_t s_sum[BudgetTable::kEntries];
#pragma unroll 1
    for (int t = threadIdx.x; t < BudgetTable::kEntries; t += kBudgetBlock) s_sum[t] = 0u;
    __syncthreads();
    const uint32_t age = blockIdx.y;
    const float rate = aged_rate(p, age);
#pragma unroll 1
    for (uint32_t i = blockIdx.x * kBudgetBlock + threadIdx.x; i < p.n; i += gridDim.x * kBudgetBlock) {
        uint32_t d;
        tpl::Board s;
        if (!feature_trace_state(p, i, age, rate, d, s)) continue;
        atomicAdd(&s_sum[(uint32_t)BudgetTable::kCounterBase + counter_index(p.L, p.M, s.lines, s.moves)], d);
        uint32_t q[BudgetTable::kRows];
        budget_bins(s, p.L, p.M, q);
        const uint32_t piece = s.window & 7u;
        const uint32_t base = piece * (uint32_t)BudgetTable::kPieceStride;
        const uint32_t mirror_base = ((kPieceMirror >> (4u * piece)) & 7u) * (uint32_t)BudgetTable::kPieceStride;
#pragma unroll
        for (int j = 0; j < BudgetTable::kRows; ++j) {
            atomicAdd(&s_sum[budget_entry(base, j, q[j])], d);
            if constexpr (kSymmetric) atomicAdd(&s_sum[budget_entry(mirror_base, j, q[j])], d);
        }
    }
    __syncthreads();
#pragma unroll 1
    for (int t = threadIdx.x; t < BudgetTable::kEntries; t += kBudgetBlock) {
        const uint32_t sum = s_sum[t];
        if (sum) atomicAdd(p.table + t, sum);
    }
}

// ---- the staged update: tpl_ntuple_update_trace_staged ----
struct StagedTraceArgs {
    TraceArgs t;                 // t.table: entry 0 of the part that is updated, in the block of stage 0
    const int32_t* map;          // [1,024], read and never written: the stage of counter index k is map[k] & 7
    uint32_t stride;             // entries from a stage's block to the next: the whole form's, a multiple of 512
};

// trace_lane on a staged table: the same lane, rate, trace cut and step, with every add at the block of the state's stage -- the
// windows through the offset in `base`, the counter sums, still one per k and per block in LDS, through the offset of k's own stage
// at the flush.  The reflected board has the state's lines and moves, so its adds go to the same block.
template <typename S, bool kSymmetric>
__device__ __forceinline__ void staged_trace_lane(const StagedTraceArgs p) {
    __shared__ uint32_t s_counter[kCounters];
#pragma unroll
    for (int t = threadIdx.x; t < kCounters; t += kStateBlock) s_counter[t] = 0u;
    __syncthreads();
    const uint32_t age = blockIdx.y;
    float w = 1.0f;
    for (uint32_t k = 0; k < age; ++k) w = __fmul_rn(w, p.t.decay);
    const float rate = __fmul_rn(p.t.rate, w);
    const uint32_t i = blockIdx.x * kStateBlock + threadIdx.x;
    if (i < p.t.n) {
        bool open = true;
        for (uint32_t k = 0; k < age; ++k) {
            const uint32_t slot = p.t.head >= k ? p.t.head - k : p.t.head + p.t.slots - k;
            open = open && ((p.t.b[slot * p.t.n + i].y >> 28) & 3u) == tpl::ST_RUNNING;
        }
        const uint32_t d = (uint32_t)update_step(rate, p.t.error[i]);
        if (open && d != 0u) {
            const uint32_t slot = p.t.head >= age ? p.t.head - age : p.t.head + p.t.slots - age;
            tpl::Board s;
            tpl::unpack_board(p.t.a[slot * p.t.n + i], p.t.b[slot * p.t.n + i], s);
            if (s.state == tpl::ST_RUNNING) {
                const uint32_t k = counter_index(p.t.L, p.t.M, s.lines, s.moves);
                atomicAdd(&s_counter[k], d);
                const uint32_t at = stage_offset(p.map, 0u, k, p.stride);
                const uint32_t piece = s.window & 7u;
                const uint32_t base = at + piece * (uint32_t)S::kPieceStride;
                const uint32_t mirror_base = at + ((kPieceMirror >> (4u * piece)) & 7u) * (uint32_t)S::kPieceStride;
#pragma unroll 1
                for (uint32_t y = 0; y < (uint32_t)S::kTupleRows; ++y) {
#pragma unroll
                    for (int x = 0; x < S::kTupleCols; ++x) {
                        const uint32_t q = S::pattern(s.c, x, y);
                        if (q) {
                            atomicAdd(entry(p.t.table, tuple_entry<S>(base, x, y, q)), d);
                            if constexpr (kSymmetric) {
                                const uint32_t swapped = S::mirrored(q);
                                atomicAdd(entry(p.t.table, tuple_entry<S>(mirror_base, S::kTupleCols - 1 - x, y, swapped)), d);
                            }
                        }
                    }
                }
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int t = threadIdx.x; t < kCounters; t += kStateBlock) {
        const uint32_t sum = s_counter[t];
        if (sum) atomicAdd(entry(p.t.table, stage_offset(p.map, 0u, (uint32_t)t, p.stride) + (uint32_t)S::kCounterBase + (uint32_t)t), sum);
    }
}

template <bool kSymmetric>
__global__ __launch_bounds__(kStateBlock) void ntuple_staged_trace_kernel(const StagedTraceArgs p) {
    staged_trace_lane<Shape2x4, kSymmetric>(p);
}
template <bool kSymmetric>
__global__ __launch_bounds__(kStateBlock) void ntuple_staged3_trace_kernel(const StagedTraceArgs p) {
    staged_trace_lane<Shape3x3, kSymmetric>(p);
}

// ---- the coherent update: tpl_ntuple_update_coherent ----
// Two kernels in ntuple_trace_kernel's frame (a lane per (board, age), the age in blockIdx.y): the step kernel reads the coherence
// buffer and adds to the table, the accumulate kernel adds to the coherence buffer.  Neither reads what it adds to, so the bytes of
// both buffers are the same whatever order the adds arrive in.

struct CoherentArgs {
    TraceArgs t;
    longlong2* coherence;        // [the shape's entries]: x = E, the signed sum; y = A, the absolute sum
};

// What a lane of either kernel does before its walk, ntuple_trace_kernel's lines: the decayed rate of the block's age, the younger
// states' state words, the step and the state of that age.  True where the lane adds: `rate` is rate * w_age, `d` is not 0 and
// `s` runs.
__device__ __forceinline__ bool coherent_lane(const TraceArgs& p, float& rate, float& e, int32_t& d, tpl::Board& s) {
    const uint32_t age = blockIdx.y;
    float w = 1.0f;
    for (uint32_t k = 0; k < age; ++k) w = __fmul_rn(w, p.decay);
    rate = __fmul_rn(p.rate, w);
    const uint32_t i = blockIdx.x * kStateBlock + threadIdx.x;
    if (i >= p.n) return false;
    bool open = true;
    for (uint32_t k = 0; k < age; ++k) {
        const uint32_t slot = p.head >= k ? p.head - k : p.head + p.slots - k;
        open = open && ((p.b[slot * p.n + i].y >> 28) & 3u) == tpl::ST_RUNNING;
    }
    e = p.error[i];
    d = update_step(rate, e);
    if (!open || d == 0) return false;
    const uint32_t slot = p.head >= age ? p.head - age : p.head + p.slots - age;
    tpl::unpack_board(p.a[slot * p.n + i], p.b[slot * p.n + i], s);
    return s.state == tpl::ST_RUNNING;
}

// The walk over the tuple entries of a running state: apply(j, gather(j)) for every tuple with a non-zero pattern and, with
// kSymmetric, for its sigma-image as well -- both, also where the two are one entry.  gather(j) is made for all nine (3 x 3: eight) tuples
// of a row before the first apply and also where the pattern is empty (the index is in bounds), so that what it loads is in flight
// nine (eighteen) at a time and stays straight-line code; an action that loads nothing returns an empty struct.
template <typename S, bool kSymmetric, typename Gather, typename Apply>
__device__ __forceinline__ void walk_entries(const tpl::Board& s, Gather&& gather, Apply&& apply) {
    const uint32_t piece = s.window & 7u;
    const uint32_t base = piece * (uint32_t)S::kPieceStride;
    const uint32_t mirror_base = ((kPieceMirror >> (4u * piece)) & 7u) * (uint32_t)S::kPieceStride;
    using G = decltype(gather(0u));
#pragma unroll 1
    for (uint32_t y = 0; y < (uint32_t)S::kTupleRows; ++y) {
        uint32_t j[S::kTupleCols], jm[S::kTupleCols];
        G g[S::kTupleCols], gm[S::kTupleCols];
#pragma unroll
        for (int x = 0; x < S::kTupleCols; ++x) {
            const uint32_t q = S::pattern(s.c, x, y);
            j[x] = tuple_entry<S>(base, x, y, q);
            g[x] = gather(j[x]);
            if constexpr (kSymmetric) {
                jm[x] = tuple_entry<S>(mirror_base, S::kTupleCols - 1 - x, y, S::mirrored(q));
                gm[x] = gather(jm[x]);
            }
        }
#pragma unroll
        for (int x = 0; x < S::kTupleCols; ++x) {
            if (j[x] & (uint32_t)(S::kPatterns - 1)) {                  // the pattern, in the index's low bits
                apply(j[x], g[x]);
                if constexpr (kSymmetric) apply(jm[x], gm[x]);
            }
        }
    }
}

// alpha of an entry with the pair c = (E, A): 1 where A <= 0, else min(|E| / A, 1) -- the magnitude as an unsigned value, both
// conversions to nearest even, the quotient rounded once
__device__ __forceinline__ float step_size(const longlong2 c) {
    if (c.y <= 0) return 1.0f;
    const unsigned long long mag = c.x < 0 ? 0ull - (unsigned long long)c.x : (unsigned long long)c.x;
    return fminf(__fdiv_rn((float)mag, (float)c.y), 1.0f);
}

// s = (int32) rint(((rate * w_k) * alpha_j) * e), `rate` being rate * w_k
__device__ __forceinline__ uint32_t coherent_step(float rate, const longlong2 c, float e) {
    return (uint32_t)update_step(__fmul_rn(rate, step_size(c)), e);
}

// The step phase.  The counter entries are summed per block in LDS first, as in ntuple_trace_kernel; 32 bits are enough here,
// since the table's own adds wrap in 32 bits.
template <typename S, bool kSymmetric>
__device__ __forceinline__ void coherent_step_lane(const CoherentArgs p) {
    __shared__ uint32_t s_counter[kCounters];
#pragma unroll
    for (int t = threadIdx.x; t < kCounters; t += kStateBlock) s_counter[t] = 0u;
    __syncthreads();
    tpl::Board s;
    float rate, e;
    int32_t d;
    if (coherent_lane(p.t, rate, e, d, s)) {
        const uint32_t k = counter_index(p.t.L, p.t.M, s.lines, s.moves);
        atomicAdd(&s_counter[k], coherent_step(rate, *entry(p.coherence, (uint32_t)S::kCounterBase + k), e));
        walk_entries<S, kSymmetric>(
            s, [&](uint32_t j) { return *entry(p.coherence, j); },
            [&](uint32_t j, const longlong2 c) {
                const uint32_t step = coherent_step(rate, c, e);
                if (step) atomicAdd(entry(p.t.table, j), step);
            });
    }
    __syncthreads();
#pragma unroll
    for (int t = threadIdx.x; t < kCounters; t += kStateBlock) {
        const uint32_t sum = s_counter[t];
        if (sum) atomicAdd(p.t.table + S::kCounterBase + t, sum);
    }
}

template <bool kSymmetric>
__global__ __launch_bounds__(kStateBlock) void ntuple_coherent_step_kernel(const CoherentArgs p) {
    coherent_step_lane<Shape2x4, kSymmetric>(p);
}
template <bool kSymmetric>
__global__ __launch_bounds__(kStateBlock) void ntuple3_coherent_step_kernel(const CoherentArgs p) {
    coherent_step_lane<Shape3x3, kSymmetric>(p);
}

struct Nothing {};

// The accumulate phase: E += d and A += |d|, wrapping in 64 bits.  The counters' sums are 64 bits wide in LDS as well: 256 lanes
// of 2^24 each do not fit 32, and E and A do not wrap there.
template <typename S, bool kSymmetric>
__device__ __forceinline__ void coherent_accumulate_lane(const CoherentArgs p) {
    __shared__ unsigned long long s_signed[kCounters], s_absolute[kCounters];
#pragma unroll
    for (int t = threadIdx.x; t < kCounters; t += kStateBlock) s_signed[t] = s_absolute[t] = 0ull;
    __syncthreads();
    unsigned long long* const sums = (unsigned long long*)p.coherence;  // entry j: E at word 2 j, A at word 2 j + 1
    tpl::Board s;
    float rate, e;
    int32_t d;
    if (coherent_lane(p.t, rate, e, d, s)) {
        const unsigned long long signed_d = (unsigned long long)(long long)d;
        const unsigned long long absolute_d = (unsigned long long)(d < 0 ? -(long long)d : (long long)d);
        const uint32_t k = counter_index(p.t.L, p.t.M, s.lines, s.moves);
        atomicAdd(&s_signed[k], signed_d);
        atomicAdd(&s_absolute[k], absolute_d);
        walk_entries<S, kSymmetric>(
            s, [](uint32_t) { return Nothing{}; },
            [&](uint32_t j, Nothing) {
                atomicAdd(entry(sums, 2u * j), signed_d);
                atomicAdd(entry(sums, 2u * j + 1u), absolute_d);
            });
    }
    __syncthreads();
#pragma unroll
    for (int t = threadIdx.x; t < kCounters; t += kStateBlock) {
        const unsigned long long sum = s_signed[t], absolute = s_absolute[t];
        if (sum) atomicAdd(sums + 2 * (S::kCounterBase + t), sum);
        if (absolute) atomicAdd(sums + 2 * (S::kCounterBase + t) + 1, absolute);
    }
}

template <bool kSymmetric>
__global__ __launch_bounds__(kStateBlock) void ntuple_coherent_accumulate_kernel(const CoherentArgs p) {
    coherent_accumulate_lane<Shape2x4, kSymmetric>(p);
}
template <bool kSymmetric>
__global__ __launch_bounds__(kStateBlock) void ntuple3_coherent_accumulate_kernel(const CoherentArgs p) {
    coherent_accumulate_lane<Shape3x3, kSymmetric>(p);
}

struct ActArgs {
    const uint4* a;              // [n]
    const uint4* b;
    uint32_t n;                  // boards; 40 n below 2^31
    uint32_t L, M;
    float r_line, r_win, r_lose, gamma;
    const int32_t* table;
    uint32_t explore_below;      // (uint32)(epsilon * 2^24): a board explores iff the top 24 bits of its hash are below
    uint64_t key;                // replay_key(seed, step)
    uint8_t* action;             // [n]
    float* score;                // [n], optional: the greedy maximum
    uint4* after_a;              // [n], with after_b or not at all: the chosen placement's afterstate
    uint4* after_b;
    float* value;                // [n], optional: V of that afterstate
};

constexpr uint32_t kGreedy = 0xFFFFFFFFu;

// The policy of kDepth plies on the block's eight boards (the header comment has the frame).  What a first move that leaves the
// game running is worth beyond its reward is the one thing that differs: V of the board it left at one ply, best_second's W at
// two.  At two plies V of the afterstate is not on the way to the score, so the one chosen lane of a board sums it afterwards,
// and only where `value` is asked for.
// `prune` (the budget geometry alone reads it; tpl_ntuple.h: prune_dead): a move that leaves a running, dead board is scored as one
// that ends lost at the limit, at either ply, and nothing is searched below it.  `goes_on`, s1 and the afterstate's V stay the true
// board's: what is written to after_a / after_b and `value` is what the environment will hold.
template <typename S, int kDepth>
__device__ __forceinline__ void ntuple_policy(const ActArgs& p, uint8_t* second_out, uint32_t prune = 0u) {
    __shared__ tpl::ShapeWord s_shape[32];
    __shared__ unsigned long long s_best[kBoardsPerBlock];
    __shared__ uint32_t s_pick[kBoardsPerBlock];                        // which distinct placement an exploring board plays
    const uint32_t first = blockIdx.x * kBoardsPerBlock;                // the block's boards: first .. first + 7
    if (threadIdx.x < 32) s_shape[threadIdx.x] = tpl::kShapeTable[threadIdx.x];
    if (threadIdx.x < kBoardsPerBlock) {
        s_best[threadIdx.x] = 0ull;                                     // below every key: a key's high word has a bit set
        const uint32_t board = min(first + threadIdx.x, p.n - 1u);
        const uint4 B = p.b[board];
        const uint64_t h = draw_hash(p.key, board);
        const bool explores = tpl::packed_state(B) == tpl::ST_RUNNING && (uint32_t)(h >> 40) < p.explore_below;
        s_pick[threadIdx.x] = explores ? __umulhi((uint32_t)h, placement_count(B.w & 7u)) : kGreedy;
    }
    __syncthreads();
    const uint32_t slot = threadIdx.x / kActions, a = threadIdx.x - slot * kActions;
    const uint32_t r = a / 10u, l = a - r * 10u;
    const uint32_t i = first + slot;
    const bool valid = i < p.n;                                         // whole boards: all 40 lanes of a board agree
    const uint32_t src = valid ? i : p.n - 1u;                          // past the end: the last board again, never written

    const uint4 A = p.a[src], B = p.b[src];
    tpl::Board s1;
    uint32_t cur;
    bool running;
    const uint32_t n1 = first_move(A, B, s_shape, r, l, p.L, p.M, s1, cur, running);
    tpl::next_window(s1, false, 0);                                     // tpl_afterstates' pop: the next piece becomes current
    const bool contends = valid && canonical_action(cur, r, l) == a;
    const bool goes_on = running && s1.state == tpl::ST_RUNNING;
    // the rank of a distinct placement among its piece's, in ascending a: the locations of the rotations before it, then l
    uint32_t rank = l;
#pragma unroll
    for (uint32_t q = 0; q < 3u; ++q) rank += q < r ? location_count(cur, q) : 0u;

    uint32_t scored = s1.state;                                         // the state the first move is scored with
    bool searched = goes_on;                                            // goes_on, unless the prune ends the move
    if constexpr (kBudgetGeometry<S>) {
        tpl::Board pruned = s1;
        prune_dead<S>(pruned, p.L, p.M, prune);
        scored = pruned.state;
        searched = running && scored == tpl::ST_RUNNING;
    }

    float v = 0.0f;                                                     // V of a state that does not run
    uint32_t second = kNoSecond;
    if constexpr (kDepth == 2) {
        // W = the best  r2 + gamma V(s2)  (r2 alone where the second move ends the game) of the next piece on s1
        if (contends && searched)
            v = best_second(s1, s_shape, p.L, p.M, second, [&](tpl::Board& s2, uint32_t n2) {
#pragma clang fp contract(off)
                tpl::next_window(s2, false, 0);                         // the piece after the next: the original window entry 2
                prune_dead<S>(s2, p.L, p.M, prune);
                const bool on = s2.state == tpl::ST_RUNNING;
                float v2 = 0.0f;
                if (on) v2 = ntuple_value<S>(s2, p.L, p.M, p.table);
                const float reward = move_reward(p.r_line, p.r_win, p.r_lose, n2, s2.state);
                const float later = p.gamma * v2;
                return on ? reward + later : reward;
            });
    } else {
        if (contends && goes_on) v = ntuple_value<S>(s1, p.L, p.M, p.table);
    }
    float score;
    {
#pragma clang fp contract(off)
        const float reward = move_reward(p.r_line, p.r_win, p.r_lose, n1, scored);
        const float later = p.gamma * v;
        score = running ? (searched ? reward + later : reward) : 0.0f;
    }
    const unsigned long long key = ((unsigned long long)ordered_bits(score) << 32) | (uint32_t)(kActions - 1 - a);
    if (contends) atomicMax(&s_best[slot], key);
    __syncthreads();
    const bool greedy = contends && s_best[slot] == key;                // one lane per board: the keys of a board are distinct
    const uint32_t pick = s_pick[slot];
    const bool chosen = pick == kGreedy ? greedy : contends && rank == pick;
    if (greedy && p.score) p.score[i] = score;                          // the TD target, whatever is played
    if constexpr (kDepth == 2) {
        if (p.value) {                                                  // uniform; v was W, the second ply's, until here
            v = 0.0f;
            if (chosen && goes_on) v = ntuple_value<S>(s1, p.L, p.M, p.table);
        }
    }
    if (chosen) {
        p.action[i] = (uint8_t)a;
        if constexpr (kDepth == 2) {
            if (second_out) second_out[i] = (uint8_t)second;
        }
        if (p.value) p.value[i] = v;
        if (p.after_a) {                                                // a finished board stays as it is, bit for bit
            uint4 A2, B2;
            tpl::pack_board(s1, A2, B2);
            B2.y |= B.y & 0x80000000u;                                  // the spare bit (the slot travels in the Board)
            p.after_a[i] = make_uint4(running ? A2.x : A.x, running ? A2.y : A.y, running ? A2.z : A.z, running ? A2.w : A.w);
            p.after_b[i] = make_uint4(running ? B2.x : B.x, running ? B2.y : B.y, running ? B2.z : B.z, running ? B2.w : B.w);
        }
    }
}

struct SearchArgs {
    ActArgs act;
    uint8_t* second;             // [n], optional: the second placement behind the action played, 255 where there is none
};

__global__ __launch_bounds__(kActBlock) void ntuple_act_kernel(const ActArgs p) { ntuple_policy<Shape2x4, 1>(p, nullptr); }
__global__ __launch_bounds__(kActBlock) void ntuple_search_kernel(const SearchArgs p) { ntuple_policy<Shape2x4, 2>(p.act, p.second); }
__global__ __launch_bounds__(kActBlock) void ntuple3_act_kernel(const ActArgs p) { ntuple_policy<Shape3x3, 1>(p, nullptr); }
__global__ __launch_bounds__(kActBlock) void ntuple3_search_kernel(const SearchArgs p) { ntuple_policy<Shape3x3, 2>(p.act, p.second); }
__global__ __launch_bounds__(kActBlock) void ntuple_sum_act_kernel(const ActArgs p) { ntuple_policy<ShapeSum, 1>(p, nullptr); }
__global__ __launch_bounds__(kActBlock) void ntuple_sum_search_kernel(const SearchArgs p) { ntuple_policy<ShapeSum, 2>(p.act, p.second); }
__global__ __launch_bounds__(kActBlock) void ntuple_staged_act_kernel(const ActArgs p) { ntuple_policy<StagedOf<Shape2x4>, 1>(p, nullptr); }
__global__ __launch_bounds__(kActBlock) void ntuple_staged_search_kernel(const SearchArgs p) {
    ntuple_policy<StagedOf<Shape2x4>, 2>(p.act, p.second);
}
__global__ __launch_bounds__(kActBlock) void ntuple_staged3_act_kernel(const ActArgs p) { ntuple_policy<StagedOf<Shape3x3>, 1>(p, nullptr); }
__global__ __launch_bounds__(kActBlock) void ntuple_staged3_search_kernel(const SearchArgs p) {
    ntuple_policy<StagedOf<Shape3x3>, 2>(p.act, p.second);
}
__global__ __launch_bounds__(kActBlock) void ntuple_staged_sum_act_kernel(const ActArgs p) { ntuple_policy<StagedOf<ShapeSum>, 1>(p, nullptr); }
// Four waves a SIMD, 128 vector registers: at the default budget the compiler made room for the block's offset by issuing the second
// ply's gathers one at a time, in both parts (1.63 times ntuple_sum_search_kernel with one stage live; 1.05 with nine in flight:
// profiles/learner/README.md).  The other staged kernels keep their twins' loops at the default.
__global__ __launch_bounds__(kActBlock) __attribute__((amdgpu_waves_per_eu(4, 4))) void ntuple_staged_sum_search_kernel(const SearchArgs p) {
    ntuple_policy<StagedOf<ShapeSum>, 2>(p.act, p.second);
}

__global__ __launch_bounds__(kActBlock) void ntuple_feature_act_kernel(const ActArgs p) { ntuple_policy<FeatureTable, 1>(p, nullptr); }
__global__ __launch_bounds__(kActBlock) void ntuple_feature_search_kernel(const SearchArgs p) { ntuple_policy<FeatureTable, 2>(p.act, p.second); }
__global__ __launch_bounds__(kActBlock) void ntuple_feature3_act_kernel(const ActArgs p) { ntuple_policy<Shape3x3Feature, 1>(p, nullptr); }
__global__ __launch_bounds__(kActBlock) void ntuple_feature3_search_kernel(const SearchArgs p) {
    ntuple_policy<Shape3x3Feature, 2>(p.act, p.second);
}

struct BudgetActArgs {
    ActArgs act;
    uint32_t prune;              // not 0: the dead-board prune
};
struct BudgetSearchArgs {
    SearchArgs search;
    uint32_t prune;
};
__global__ __launch_bounds__(kActBlock) void ntuple_budget_act_kernel(const BudgetActArgs p) { ntuple_policy<BudgetTable, 1>(p.act, nullptr, p.prune); }
__global__ __launch_bounds__(kActBlock) void ntuple_budget_search_kernel(const BudgetSearchArgs p) {
    ntuple_policy<BudgetTable, 2>(p.search.act, p.search.second, p.prune);
}

}  // namespace
}  // namespace tpl_learn

using namespace tpl_learn;

extern "C" int64_t tpl_ntuple_entries(int32_t shape) {
    if (shape == TPL_NTUPLE_SHAPE_2X4) return TPL_NTUPLE_ENTRIES;
    if (shape == TPL_NTUPLE_SHAPE_3X3) return TPL_NTUPLE_ENTRIES_3X3;
    return -1;
}

namespace {

// what tpl_ntuple_value, tpl_ntuple_value_shaped (its shape checked before it comes here) and tpl_ntuple_value_sum share: the
// checks and the launch
int launch_value(const char* name, const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const int32_t* table,
                 float* value, Form form, void* stream, bool staged = false) {
    if (const int rc = check_planes(name, plane_a, plane_b, n, L, M)) return rc;
    if (const int rc = check_table(name, table)) return rc;
    if (!value) return fail_msg(TPL_ERR_ARG, "%s: null pointer (value is required)", name);
    if ((uintptr_t)value & 3u) return fail_msg(TPL_ERR_ARG, "%s: value must be 4-byte aligned", name);
    ValueArgs p{};
    p.a = (const uint4*)plane_a; p.b = (const uint4*)plane_b; p.n = (uint32_t)n;
    p.L = (uint32_t)L; p.M = (uint32_t)M; p.table = table; p.value = value;
    const dim3 grid((p.n + kStateBlock - 1) / kStateBlock), block(kStateBlock);
    if (form == Form::kBudget) {
        hipLaunchKernelGGL(ntuple_budget_value_kernel, grid, block, 0, (hipStream_t)stream, p);
    } else if (form == Form::kFeature || form == Form::k3x3Feature) {
        const auto kernel = form == Form::kFeature ? ntuple_feature_value_kernel : ntuple_feature3_value_kernel;
        hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, p);
    } else if (staged) {
        const auto kernel = form == Form::kSum ? ntuple_staged_sum_value_kernel
                                               : form == Form::k3x3 ? ntuple_staged3_value_kernel : ntuple_staged_value_kernel;
        hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, p);
    } else if (form == Form::kSum) hipLaunchKernelGGL(ntuple_sum_value_kernel, grid, block, 0, (hipStream_t)stream, p);
    else if (form == Form::k3x3) hipLaunchKernelGGL(ntuple3_value_kernel, grid, block, 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(ntuple_value_kernel, grid, block, 0, (hipStream_t)stream, p);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}

// what tpl_ntuple_act (depth = 1, second = null) and tpl_ntuple_search (depth = 2), their _shaped twins (the shape checked
// before they come here) and their _sum twins share: the checks and the launch
int launch_ntuple_policy(const char* name, int depth, const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M,
                         float r_line, float r_win, float r_lose, float gamma, const int32_t* table, float epsilon, uint64_t seed,
                         uint64_t step, uint8_t* action, uint8_t* second, float* score, void* after_a, void* after_b, float* value,
                         Form form, void* stream, bool staged = false, int32_t prune = 0) {
    if (const int rc = check_planes(name, plane_a, plane_b, n, L, M)) return rc;
    if (const int rc = check_table(name, table)) return rc;
    if (!action) return fail_msg(TPL_ERR_ARG, "%s: null pointer (action is required)", name);
    if ((after_a == nullptr) != (after_b == nullptr)) return fail_msg(TPL_ERR_ARG, "%s: after_a and after_b go together", name);
    if (((uintptr_t)after_a & 15u) || ((uintptr_t)after_b & 15u))
        return fail_msg(TPL_ERR_ARG, "%s: after_a and after_b must be 16-byte aligned", name);
    if (((uintptr_t)score & 3u) || ((uintptr_t)value & 3u))
        return fail_msg(TPL_ERR_ARG, "%s: score and value must be 4-byte aligned", name);
    if (!(epsilon >= 0.0f && epsilon <= 1.0f)) return fail_msg(TPL_ERR_ARG, "%s: epsilon must be in [0, 1]", name);
    if (!std::isfinite(gamma)) return fail_msg(TPL_ERR_ARG, "%s: gamma must be finite", name);
    ActArgs p{};
    p.a = (const uint4*)plane_a; p.b = (const uint4*)plane_b; p.n = (uint32_t)n;
    p.L = (uint32_t)L; p.M = (uint32_t)M; p.r_line = r_line; p.r_win = r_win; p.r_lose = r_lose; p.gamma = gamma;
    p.table = table;
    p.explore_below = (uint32_t)(epsilon * 0x1p24f);                    // exact: a power of two; 2^24 at epsilon = 1, above every hash
    p.key = replay_key(seed, step);
    p.action = action; p.score = score; p.after_a = (uint4*)after_a; p.after_b = (uint4*)after_b; p.value = value;
    const dim3 grid((p.n + kBoardsPerBlock - 1) / kBoardsPerBlock), block(kActBlock);
    const bool wide = form == Form::k3x3;
    if (form == Form::kBudget) {                                        // the one form that knows the prune
        const uint32_t flag = prune != 0 ? 1u : 0u;
        if (depth == 2) {
            const BudgetSearchArgs q{{p, second}, flag};
            hipLaunchKernelGGL(ntuple_budget_search_kernel, grid, block, 0, (hipStream_t)stream, q);
        } else {
            const BudgetActArgs q{p, flag};
            hipLaunchKernelGGL(ntuple_budget_act_kernel, grid, block, 0, (hipStream_t)stream, q);
        }
    } else if (form == Form::kFeature || form == Form::k3x3Feature) {
        if (depth == 2) {
            const SearchArgs q{p, second};
            const auto kernel = form == Form::kFeature ? ntuple_feature_search_kernel : ntuple_feature3_search_kernel;
            hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, q);
        } else {
            const auto kernel = form == Form::kFeature ? ntuple_feature_act_kernel : ntuple_feature3_act_kernel;
            hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, p);
        }
    } else if (staged && depth == 2) {
        const SearchArgs q{p, second};
        const auto kernel = form == Form::kSum ? ntuple_staged_sum_search_kernel : wide ? ntuple_staged3_search_kernel : ntuple_staged_search_kernel;
        hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, q);
    } else if (staged) {
        const auto kernel = form == Form::kSum ? ntuple_staged_sum_act_kernel : wide ? ntuple_staged3_act_kernel : ntuple_staged_act_kernel;
        hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, p);
    } else if (depth == 2) {
        const SearchArgs q{p, second};
        if (form == Form::kSum) hipLaunchKernelGGL(ntuple_sum_search_kernel, grid, block, 0, (hipStream_t)stream, q);
        else if (wide) hipLaunchKernelGGL(ntuple3_search_kernel, grid, block, 0, (hipStream_t)stream, q);
        else hipLaunchKernelGGL(ntuple_search_kernel, grid, block, 0, (hipStream_t)stream, q);
    } else if (form == Form::kSum) {
        hipLaunchKernelGGL(ntuple_sum_act_kernel, grid, block, 0, (hipStream_t)stream, p);
    } else if (wide) {
        hipLaunchKernelGGL(ntuple3_act_kernel, grid, block, 0, (hipStream_t)stream, p);
    } else {
        hipLaunchKernelGGL(ntuple_act_kernel, grid, block, 0, (hipStream_t)stream, p);
    }
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}

}  // namespace

extern "C" int tpl_ntuple_value(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const int32_t* table,
                                float* value, void* stream) {
    return launch_value("tpl_ntuple_value", plane_a, plane_b, n, L, M, table, value, Form::k2x4, stream);
}

extern "C" int tpl_ntuple_value_shaped(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M,
                                       const int32_t* table, float* value, int32_t shape, void* stream) {
    if (const int rc = check_shape("tpl_ntuple_value_shaped", shape)) return rc;
    return launch_value("tpl_ntuple_value_shaped", plane_a, plane_b, n, L, M, table, value, form_of(shape), stream);
}

extern "C" int tpl_ntuple_value_sum(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const int32_t* table,
                                    float* value, void* stream) {
    return launch_value("tpl_ntuple_value_sum", plane_a, plane_b, n, L, M, table, value, Form::kSum, stream);
}

extern "C" int tpl_ntuple_act(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line, float r_win,
                              float r_lose, float gamma, const int32_t* table, float epsilon, uint64_t seed, uint64_t step,
                              uint8_t* action, float* score, void* after_a, void* after_b, float* value, void* stream) {
    return launch_ntuple_policy("tpl_ntuple_act", 1, plane_a, plane_b, n, L, M, r_line, r_win, r_lose, gamma, table, epsilon, seed,
                                step, action, nullptr, score, after_a, after_b, value, Form::k2x4, stream);
}

extern "C" int tpl_ntuple_act_shaped(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line,
                                     float r_win, float r_lose, float gamma, const int32_t* table, float epsilon, uint64_t seed,
                                     uint64_t step, uint8_t* action, float* score, void* after_a, void* after_b, float* value,
                                     int32_t shape, void* stream) {
    if (const int rc = check_shape("tpl_ntuple_act_shaped", shape)) return rc;
    return launch_ntuple_policy("tpl_ntuple_act_shaped", 1, plane_a, plane_b, n, L, M, r_line, r_win, r_lose, gamma, table, epsilon,
                                seed, step, action, nullptr, score, after_a, after_b, value, form_of(shape), stream);
}

extern "C" int tpl_ntuple_act_sum(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line, float r_win,
                                  float r_lose, float gamma, const int32_t* table, float epsilon, uint64_t seed, uint64_t step,
                                  uint8_t* action, float* score, void* after_a, void* after_b, float* value, void* stream) {
    return launch_ntuple_policy("tpl_ntuple_act_sum", 1, plane_a, plane_b, n, L, M, r_line, r_win, r_lose, gamma, table, epsilon,
                                seed, step, action, nullptr, score, after_a, after_b, value, Form::kSum, stream);
}

extern "C" int tpl_ntuple_search(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line,
                                 float r_win, float r_lose, float gamma, const int32_t* table, float epsilon, uint64_t seed,
                                 uint64_t step, uint8_t* action, uint8_t* second, float* score, void* after_a, void* after_b,
                                 float* value, void* stream) {
    return launch_ntuple_policy("tpl_ntuple_search", 2, plane_a, plane_b, n, L, M, r_line, r_win, r_lose, gamma, table, epsilon,
                                seed, step, action, second, score, after_a, after_b, value, Form::k2x4, stream);
}

extern "C" int tpl_ntuple_search_shaped(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line,
                                        float r_win, float r_lose, float gamma, const int32_t* table, float epsilon, uint64_t seed,
                                        uint64_t step, uint8_t* action, uint8_t* second, float* score, void* after_a, void* after_b,
                                        float* value, int32_t shape, void* stream) {
    if (const int rc = check_shape("tpl_ntuple_search_shaped", shape)) return rc;
    return launch_ntuple_policy("tpl_ntuple_search_shaped", 2, plane_a, plane_b, n, L, M, r_line, r_win, r_lose, gamma, table,
                                epsilon, seed, step, action, second, score, after_a, after_b, value, form_of(shape), stream);
}

extern "C" int tpl_ntuple_search_sum(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line,
                                     float r_win, float r_lose, float gamma, const int32_t* table, float epsilon, uint64_t seed,
                                     uint64_t step, uint8_t* action, uint8_t* second, float* score, void* after_a, void* after_b,
                                     float* value, void* stream) {
    return launch_ntuple_policy("tpl_ntuple_search_sum", 2, plane_a, plane_b, n, L, M, r_line, r_win, r_lose, gamma, table, epsilon,
                                seed, step, action, second, score, after_a, after_b, value, Form::kSum, stream);
}

extern "C" int tpl_ntuple_value_staged(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M,
                                       const int32_t* table, float* value, int32_t form, void* stream) {
    if (const int rc = check_form("tpl_ntuple_value_staged", form)) return rc;
    return launch_value("tpl_ntuple_value_staged", plane_a, plane_b, n, L, M, table, value, (Form)form, stream, true);
}

extern "C" int tpl_ntuple_act_staged(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line,
                                     float r_win, float r_lose, float gamma, const int32_t* table, float epsilon, uint64_t seed,
                                     uint64_t step, uint8_t* action, float* score, void* after_a, void* after_b, float* value,
                                     int32_t form, void* stream) {
    if (const int rc = check_form("tpl_ntuple_act_staged", form)) return rc;
    return launch_ntuple_policy("tpl_ntuple_act_staged", 1, plane_a, plane_b, n, L, M, r_line, r_win, r_lose, gamma, table, epsilon,
                                seed, step, action, nullptr, score, after_a, after_b, value, (Form)form, stream, true);
}

extern "C" int tpl_ntuple_search_staged(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line,
                                        float r_win, float r_lose, float gamma, const int32_t* table, float epsilon, uint64_t seed,
                                        uint64_t step, uint8_t* action, uint8_t* second, float* score, void* after_a, void* after_b,
                                        float* value, int32_t form, void* stream) {
    if (const int rc = check_form("tpl_ntuple_search_staged", form)) return rc;
    return launch_ntuple_policy("tpl_ntuple_search_staged", 2, plane_a, plane_b, n, L, M, r_line, r_win, r_lose, gamma, table,
                                epsilon, seed, step, action, second, score, after_a, after_b, value, (Form)form, stream, true);
}

namespace {

// what the three updates refuse alike; `coherence`: where the entry takes a coherence buffer, the address of its pointer
int check_update(const char* name, int32_t shape, const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M,
                 const int32_t* table, const float* error, float rate, const int64_t* const* coherence = nullptr,
                 bool staged = false) {
    if (const int rc = staged ? check_form(name, shape) : check_shape(name, shape)) return rc;
    if (const int rc = check_planes(name, plane_a, plane_b, n, L, M)) return rc;
    if (const int rc = check_table(name, table)) return rc;
    if (coherence && !*coherence) return fail_msg(TPL_ERR_ARG, "%s: null pointer (coherence is required)", name);
    if (coherence && ((uintptr_t)*coherence & 15u)) return fail_msg(TPL_ERR_ARG, "%s: coherence must be 16-byte aligned", name);
    if (!error) return fail_msg(TPL_ERR_ARG, "%s: null pointer (error is required)", name);
    if ((uintptr_t)error & 3u) return fail_msg(TPL_ERR_ARG, "%s: error must be 4-byte aligned", name);
    if (!std::isfinite(rate)) return fail_msg(TPL_ERR_ARG, "%s: rate must be finite", name);
    return TPL_OK;
}

// what the three updates share beyond check_update: the arguments and the launch, an age of the ring per grid row
// `coherence` null: the trace kernel; otherwise the two phases of the coherent update, one after the other on the stream
int launch_update(int32_t shape, const void* ring_a, const void* ring_b, int64_t n, int32_t slots, int32_t head, int32_t horizon,
                  int32_t L, int32_t M, int32_t* table, const float* error, float rate, float decay, bool symmetric, void* stream,
                  int64_t* coherence = nullptr) {
    TraceArgs p{};
    p.a = (const uint4*)ring_a; p.b = (const uint4*)ring_b; p.n = (uint32_t)n; p.slots = (uint32_t)slots; p.head = (uint32_t)head;
    p.L = (uint32_t)L; p.M = (uint32_t)M; p.table = (uint32_t*)table; p.error = error; p.rate = rate; p.decay = decay;
    const dim3 grid((p.n + kStateBlock - 1) / kStateBlock, (uint32_t)horizon), block(kStateBlock);
    const bool wide = shape == TPL_NTUPLE_SHAPE_3X3;
    if (coherence) {
        const CoherentArgs c{p, (longlong2*)coherence};
        auto step = symmetric ? ntuple_coherent_step_kernel<true> : ntuple_coherent_step_kernel<false>;
        auto accumulate = symmetric ? ntuple_coherent_accumulate_kernel<true> : ntuple_coherent_accumulate_kernel<false>;
        if (wide) {
            step = symmetric ? ntuple3_coherent_step_kernel<true> : ntuple3_coherent_step_kernel<false>;
            accumulate = symmetric ? ntuple3_coherent_accumulate_kernel<true> : ntuple3_coherent_accumulate_kernel<false>;
        }
        hipLaunchKernelGGL(step, grid, block, 0, (hipStream_t)stream, c);
        TPL_LEARN_HIP(hipGetLastError());
        hipLaunchKernelGGL(accumulate, grid, block, 0, (hipStream_t)stream, c);
    } else {
        auto trace = symmetric ? ntuple_trace_kernel<true> : ntuple_trace_kernel<false>;
        if (wide) trace = symmetric ? ntuple3_trace_kernel<true> : ntuple3_trace_kernel<false>;
        hipLaunchKernelGGL(trace, grid, block, 0, (hipStream_t)stream, p);
    }
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}

// what the two ring updates refuse beyond check_update, in this order
int check_ring(const char* name, int64_t n, int32_t slots, int32_t head, int32_t horizon, float decay) {
    if (slots < 1 || slots > TPL_NTUPLE_TRACE_MAX + 1)
        return fail_msg(TPL_ERR_ARG, "%s: slots must be in [1, %d]", name, TPL_NTUPLE_TRACE_MAX + 1);
    if (head < 0 || head >= slots) return fail_msg(TPL_ERR_ARG, "%s: head must be in [0, slots)", name);
    if (horizon < 1 || horizon > slots || horizon > TPL_NTUPLE_TRACE_MAX)
        return fail_msg(TPL_ERR_ARG, "%s: horizon must be in [1, min(slots, %d)]", name, TPL_NTUPLE_TRACE_MAX);
    if ((int64_t)slots * n >= (((int64_t)1 << 31) + kActions - 1) / kActions)
        return fail_msg(TPL_ERR_ARG, "%s: 40 * slots * n must stay below 2^31", name);
    if (!(decay >= 0.0f && decay <= 1.0f)) return fail_msg(TPL_ERR_ARG, "%s: decay must be in [0, 1]", name);
    return TPL_OK;
}

// the planes are a ring of one slot: age 0 alone, whose weight is decay^0 = 1 whatever the decay
int update_planes(const char* name, const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, int32_t* table,
                  const float* error, float rate, int32_t shape, void* stream) {
    if (const int rc = check_update(name, shape, plane_a, plane_b, n, L, M, table, error, rate)) return rc;
    return launch_update(shape, plane_a, plane_b, n, 1, 0, 1, L, M, table, error, rate, 0.0f, false, stream);
}

int update_ring(const char* name, const void* ring_a, const void* ring_b, int64_t n, int32_t slots, int32_t head, int32_t horizon,
                int32_t L, int32_t M, int32_t* table, const int64_t* const* coherence, const float* error, float rate, float decay,
                int32_t symmetric, int32_t shape, void* stream) {
    if (const int rc = check_update(name, shape, ring_a, ring_b, n, L, M, table, error, rate, coherence)) return rc;
    if (const int rc = check_ring(name, n, slots, head, horizon, decay)) return rc;
    return launch_update(shape, ring_a, ring_b, n, slots, head, horizon, L, M, table, error, rate, decay, symmetric != 0, stream,
                         coherence ? (int64_t*)*coherence : nullptr);
}

}  // namespace

extern "C" int tpl_ntuple_update(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, int32_t* table,
                                 const float* error, float rate, void* stream) {
    return update_planes("tpl_ntuple_update", plane_a, plane_b, n, L, M, table, error, rate, TPL_NTUPLE_SHAPE_2X4, stream);
}

extern "C" int tpl_ntuple_update_shaped(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, int32_t* table,
                                        const float* error, float rate, int32_t shape, void* stream) {
    return update_planes("tpl_ntuple_update_shaped", plane_a, plane_b, n, L, M, table, error, rate, shape, stream);
}

extern "C" int tpl_ntuple_update_trace(const void* ring_a, const void* ring_b, int64_t n, int32_t slots, int32_t head,
                                       int32_t horizon, int32_t L, int32_t M, int32_t* table, const float* error, float rate,
                                       float decay, int32_t symmetric, void* stream) {
    return update_ring("tpl_ntuple_update_trace", ring_a, ring_b, n, slots, head, horizon, L, M, table, nullptr, error, rate, decay,
                       symmetric, TPL_NTUPLE_SHAPE_2X4, stream);
}

extern "C" int tpl_ntuple_update_trace_shaped(const void* ring_a, const void* ring_b, int64_t n, int32_t slots, int32_t head,
                                              int32_t horizon, int32_t L, int32_t M, int32_t* table, const float* error, float rate,
                                              float decay, int32_t symmetric, int32_t shape, void* stream) {
    return update_ring("tpl_ntuple_update_trace_shaped", ring_a, ring_b, n, slots, head, horizon, L, M, table, nullptr, error, rate,
                       decay, symmetric, shape, stream);
}

// The staged update: the part updates of the form, each on its part of every block -- the part's entry 0 in stage 0 as the kernel's
// table, the whole form's entries as the stride between blocks, the map behind the eighth block.
extern "C" int tpl_ntuple_update_trace_staged(const void* ring_a, const void* ring_b, int64_t n, int32_t slots, int32_t head,
                                              int32_t horizon, int32_t L, int32_t M, int32_t* table, const float* error, float rate,
                                              float decay, int32_t symmetric, int32_t form, void* stream) {
    const char* const name = "tpl_ntuple_update_trace_staged";
    if (const int rc = check_update(name, form, ring_a, ring_b, n, L, M, table, error, rate, nullptr, true)) return rc;
    if (const int rc = check_ring(name, n, slots, head, horizon, decay)) return rc;
    const uint32_t stride = form == TPL_NTUPLE_FORM_SUM ? (uint32_t)ShapeSum::kEntries
                                                        : form == TPL_NTUPLE_FORM_3X3 ? (uint32_t)Shape3x3::kEntries : (uint32_t)Shape2x4::kEntries;
    StagedTraceArgs p{};
    p.t.a = (const uint4*)ring_a; p.t.b = (const uint4*)ring_b; p.t.n = (uint32_t)n; p.t.slots = (uint32_t)slots;
    p.t.head = (uint32_t)head; p.t.L = (uint32_t)L; p.t.M = (uint32_t)M; p.t.error = error; p.t.rate = rate; p.t.decay = decay;
    p.map = table + (size_t)TPL_NTUPLE_STAGES * stride;
    p.stride = stride;
    const dim3 grid((p.t.n + kStateBlock - 1) / kStateBlock, (uint32_t)horizon), block(kStateBlock);
    if (form != TPL_NTUPLE_FORM_3X3) {                                  // the 2 x 4 part, at the block's base
        p.t.table = (uint32_t*)table;
        hipLaunchKernelGGL(symmetric ? ntuple_staged_trace_kernel<true> : ntuple_staged_trace_kernel<false>, grid, block, 0,
                           (hipStream_t)stream, p);
        TPL_LEARN_HIP(hipGetLastError());
    }
    if (form != TPL_NTUPLE_FORM_2X4) {                                  // the 3 x 3 part: of a sum, behind the 2 x 4 part
        p.t.table = (uint32_t*)table + (form == TPL_NTUPLE_FORM_SUM ? ShapeSum::kSecondAt : 0u);
        hipLaunchKernelGGL(symmetric ? ntuple_staged3_trace_kernel<true> : ntuple_staged3_trace_kernel<false>, grid, block, 0,
                           (hipStream_t)stream, p);
        TPL_LEARN_HIP(hipGetLastError());
    }
    return TPL_OK;
}

extern "C" int tpl_ntuple_update_coherent(const void* ring_a, const void* ring_b, int64_t n, int32_t slots, int32_t head,
                                          int32_t horizon, int32_t L, int32_t M, int32_t* table, int64_t* coherence,
                                          const float* error, float rate, float decay, int32_t symmetric, void* stream) {
    const int64_t* const given = coherence;
    return update_ring("tpl_ntuple_update_coherent", ring_a, ring_b, n, slots, head, horizon, L, M, table, &given, error, rate,
                       decay, symmetric, TPL_NTUPLE_SHAPE_2X4, stream);
}

extern "C" int tpl_ntuple_update_coherent_shaped(const void* ring_a, const void* ring_b, int64_t n, int32_t slots, int32_t head,
                                                 int32_t horizon, int32_t L, int32_t M, int32_t* table, int64_t* coherence,
                                                 const float* error, float rate, float decay, int32_t symmetric, int32_t shape,
                                                 void* stream) {
    const int64_t* const given = coherence;
    return update_ring("tpl_ntuple_update_coherent_shaped", ring_a, ring_b, n, slots, head, horizon, L, M, table, &given, error,
                       rate, decay, symmetric, shape, stream);
}

// ---- feature tuples: the _feature entries ----
extern "C" int tpl_ntuple_value_feature(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const int32_t* table,
                                        float* value, int32_t form, void* stream) {
    if (const int rc = check_feature_form("tpl_ntuple_value_feature", form)) return rc;
    return launch_value("tpl_ntuple_value_feature", plane_a, plane_b, n, L, M, table, value, feature_form_of(form), stream);
}

extern "C" int tpl_ntuple_act_feature(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line,
                                      float r_win, float r_lose, float gamma, const int32_t* table, float epsilon, uint64_t seed,
                                      uint64_t step, uint8_t* action, float* score, void* after_a, void* after_b, float* value,
                                      int32_t form, void* stream) {
    if (const int rc = check_feature_form("tpl_ntuple_act_feature", form)) return rc;
    return launch_ntuple_policy("tpl_ntuple_act_feature", 1, plane_a, plane_b, n, L, M, r_line, r_win, r_lose, gamma, table, epsilon,
                                seed, step, action, nullptr, score, after_a, after_b, value, feature_form_of(form), stream);
}

extern "C" int tpl_ntuple_search_feature(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line,
                                         float r_win, float r_lose, float gamma, const int32_t* table, float epsilon, uint64_t seed,
                                         uint64_t step, uint8_t* action, uint8_t* second, float* score, void* after_a, void* after_b,
                                         float* value, int32_t form, void* stream) {
    if (const int rc = check_feature_form("tpl_ntuple_search_feature", form)) return rc;
    return launch_ntuple_policy("tpl_ntuple_search_feature", 2, plane_a, plane_b, n, L, M, r_line, r_win, r_lose, gamma, table,
                                epsilon, seed, step, action, second, score, after_a, after_b, value, feature_form_of(form), stream);
}

// what tpl_ntuple_update_trace_feature and tpl_ntuple_update_trace_budget share: the checks and the launch of the kernel that holds
// the whole table of `form` in LDS
static int update_whole_table(const char* name, Form form, const void* ring_a, const void* ring_b, int64_t n, int32_t slots, int32_t head,
                              int32_t horizon, int32_t L, int32_t M, int32_t* table, const float* error, float rate, float decay,
                              int32_t symmetric, void* stream) {
    if (const int rc = check_planes(name, ring_a, ring_b, n, L, M)) return rc;
    if (const int rc = check_table(name, table)) return rc;
    if (!error) return fail_msg(TPL_ERR_ARG, "%s: null pointer (error is required)", name);
    if ((uintptr_t)error & 3u) return fail_msg(TPL_ERR_ARG, "%s: error must be 4-byte aligned", name);
    if (!std::isfinite(rate)) return fail_msg(TPL_ERR_ARG, "%s: rate must be finite", name);
    if (const int rc = check_ring(name, n, slots, head, horizon, decay)) return rc;
    TraceArgs p{};
    p.a = (const uint4*)ring_a; p.b = (const uint4*)ring_b; p.n = (uint32_t)n; p.slots = (uint32_t)slots; p.head = (uint32_t)head;
    p.L = (uint32_t)L; p.M = (uint32_t)M; p.table = (uint32_t*)table; p.error = error; p.rate = rate; p.decay = decay;
    if (form == Form::kBudget) {                                        // at 2^20 boards a lane walks 2^20 / 1,024 / 256 = 4 states
        const uint32_t blocks = std::min<uint32_t>((p.n + kBudgetBlock - 1) / kBudgetBlock, kBudgetMaxBlocks);
        hipLaunchKernelGGL(symmetric ? ntuple_budget_trace_kernel<true> : ntuple_budget_trace_kernel<false>,
                           dim3(blocks, (uint32_t)horizon), dim3(kBudgetBlock), 0, (hipStream_t)stream, p);
    } else {                                                            // at 2^20 boards a lane walks 2^20 / 512 / 512 = 4 states
        const uint32_t blocks = std::min<uint32_t>((p.n + kCombineBlock - 1) / kCombineBlock, kCombineMaxBlocks);
        hipLaunchKernelGGL(symmetric ? ntuple_feature_trace_kernel<true> : ntuple_feature_trace_kernel<false>,
                           dim3(blocks, (uint32_t)horizon), dim3(kCombineBlock), 0, (hipStream_t)stream, p);
    }
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}

extern "C" int tpl_ntuple_update_trace_feature(const void* ring_a, const void* ring_b, int64_t n, int32_t slots, int32_t head,
                                               int32_t horizon, int32_t L, int32_t M, int32_t* table, const float* error, float rate,
                                               float decay, int32_t symmetric, void* stream) {
    return update_whole_table("tpl_ntuple_update_trace_feature", Form::kFeature, ring_a, ring_b, n, slots, head, horizon, L, M, table,
                              error, rate, decay, symmetric, stream);
}

// check_planes without a game: the bins read neither L nor M.  The same refusals in the same words, in its order.
static int check_state_planes(const char* name, const void* plane_a, const void* plane_b, int64_t n) {
    if (!plane_a || !plane_b) return fail_msg(TPL_ERR_ARG, "%s: null pointer", name);
    if (n < 1) return fail_msg(TPL_ERR_ARG, "%s: n must be positive", name);
    if (n >= (((int64_t)1 << 31) + kActions - 1) / kActions)
        return fail_msg(TPL_ERR_ARG, "%s: n too large (40 n must stay below 2^31)", name);
    if (((uintptr_t)plane_a & 15u) || ((uintptr_t)plane_b & 15u))
        return fail_msg(TPL_ERR_ARG, "%s: planes must be 16-byte aligned", name);
    return TPL_OK;
}

// Not a hot-path entry: it exists so that the device feature code can be held to the host mirror without the gathers, and a lane's
// nine byte stores are not coalesced.
extern "C" int tpl_ntuple_feature_bins(const void* plane_a, const void* plane_b, int64_t n, uint8_t* bins, void* stream) {
    const char* const name = "tpl_ntuple_feature_bins";
    if (const int rc = check_state_planes(name, plane_a, plane_b, n)) return rc;
    if (!bins) return fail_msg(TPL_ERR_ARG, "%s: null pointer (bins is required)", name);
    BinsArgs p{};
    p.a = (const uint4*)plane_a; p.b = (const uint4*)plane_b; p.n = (uint32_t)n; p.bins = bins;
    hipLaunchKernelGGL(ntuple_feature_bins_kernel, dim3((p.n + kStateBlock - 1) / kStateBlock), dim3(kStateBlock), 0, (hipStream_t)stream, p);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}

// ---- the budget table: the _budget entries ----
extern "C" int tpl_ntuple_value_budget(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const int32_t* table,
                                       float* value, void* stream) {
    return launch_value("tpl_ntuple_value_budget", plane_a, plane_b, n, L, M, table, value, Form::kBudget, stream);
}

extern "C" int tpl_ntuple_act_budget(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line,
                                     float r_win, float r_lose, float gamma, const int32_t* table, float epsilon, uint64_t seed,
                                     uint64_t step, uint8_t* action, float* score, void* after_a, void* after_b, float* value,
                                     int32_t prune, void* stream) {
    return launch_ntuple_policy("tpl_ntuple_act_budget", 1, plane_a, plane_b, n, L, M, r_line, r_win, r_lose, gamma, table, epsilon,
                                seed, step, action, nullptr, score, after_a, after_b, value, Form::kBudget, stream, false, prune);
}

extern "C" int tpl_ntuple_search_budget(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line,
                                        float r_win, float r_lose, float gamma, const int32_t* table, float epsilon, uint64_t seed,
                                        uint64_t step, uint8_t* action, uint8_t* second, float* score, void* after_a, void* after_b,
                                        float* value, int32_t prune, void* stream) {
    return launch_ntuple_policy("tpl_ntuple_search_budget", 2, plane_a, plane_b, n, L, M, r_line, r_win, r_lose, gamma, table, epsilon,
                                seed, step, action, second, score, after_a, after_b, value, Form::kBudget, stream, false, prune);
}

extern "C" int tpl_ntuple_update_trace_budget(const void* ring_a, const void* ring_b, int64_t n, int32_t slots, int32_t head,
                                              int32_t horizon, int32_t L, int32_t M, int32_t* table, const float* error, float rate,
                                              float decay, int32_t symmetric, void* stream) {
    return update_whole_table("tpl_ntuple_update_trace_budget", Form::kBudget, ring_a, ring_b, n, slots, head, horizon, L, M, table,
                              error, rate, decay, symmetric, stream);
}

// Not a hot-path entry, as tpl_ntuple_feature_bins is none: a lane's ten byte stores are not coalesced.
extern "C" int tpl_ntuple_budget_bins(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, uint8_t* bins,
                                      void* stream) {
    const char* const name = "tpl_ntuple_budget_bins";
    if (const int rc = check_planes(name, plane_a, plane_b, n, L, M)) return rc;
    if (!bins) return fail_msg(TPL_ERR_ARG, "%s: null pointer (bins is required)", name);
    BudgetBinsArgs p{};
    p.a = (const uint4*)plane_a; p.b = (const uint4*)plane_b; p.n = (uint32_t)n; p.L = (uint32_t)L; p.M = (uint32_t)M; p.bins = bins;
    hipLaunchKernelGGL(ntuple_budget_bins_kernel, dim3((p.n + kStateBlock - 1) / kStateBlock), dim3(kStateBlock), 0, (hipStream_t)stream, p);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}
