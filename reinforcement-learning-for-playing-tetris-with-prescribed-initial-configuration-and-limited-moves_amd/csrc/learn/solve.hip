// solve.hip -- a whole-game beam solver for prescribed configurations: tpl_placement_solve (include/tpl_learn.h states the rule).
//
// tpl_placement_beam plans from an environment state, whose window shows at most twelve pieces.  A prescribed configuration is a
// board and the WHOLE list of its M + 1 pieces, so a search over it may run all M plies.  This kernel runs the placement beam --
// tpl_placement_beam's candidates, features, score rule and order -- through the list, stops at the first ply at which a candidate
// is won, and returns that candidate's moves.
//
// Mapping: ONE CONFIGURATION PER WORKGROUP of 256 threads, in beam.hip's frame (tpl_beam.h: slots, the selection rounds, the stable
// compaction); its phases A, B and C are beam.hip's.  What differs:
//   the piece   of ply j is pieces[j - 1] of the list, kept in LDS; a node's board carries no window.  expand() writes the
//               ply's piece into the unpacked board before the move, so nothing depends on twelve entries or on a refill.
//   the stop    phase A also keeps, per lane, the largest key among its WON candidates; one shuffle reduction and four LDS words
//               give the block their maximum after the barrier that phase A ends with anyway.  If any candidate is won that
//               maximum is the won candidate that comes first in the rule's order (keys are the order), and the search ends
//               BEFORE the cut: phase B and C do not run at that ply, and the second wave finds the ply's first candidate of all
//               for best_value while lane 0 walks the tape.
//   the path    up to 254 placements a node.  A node's path is not stored with it: every ply writes, for each kept candidate, two
//               bytes (its parent's place in the old beam, its placement) to a TAPE in LDS, [ply][place].  At the winning ply one
//               lane walks the tape back from the won candidate's parent, at most 253 dependent LDS reads, into a 256-byte path
//               buffer that the block then stores with one byte per lane.  The tape is dynamic LDS, 2 W M bytes: 1,280 at
//               W = 16, M = 40 and 32,512 at the limits (W = 64, M = 254), where the kernel's 58 KB still leave two groups a CU.
//               (Two beams of whole paths would be the same 32 KB at the limits and would copy up to 254 bytes per kept node and
//               ply.)
// Nothing but the outputs goes to memory.
//
// This unit is built twice (tpl_placement.h: kUnitFeatures): as it stands, placement_solve_kernel on the twelve board features, and
// through solve_move.hip as placement_solve_move_kernel on the fourteen with landing height and eroded cells.  There a node's `cleared`
// word is the carry of its path (tpl_placement.h): over the 254 moves of the longest game the landing sum is at most 254 * 38 = 9,652,
// which fits its 14 bits.
//
// And twice more in the BOUNDED form (tpl_placement.h: kUnitBound; include/tpl_learn.h: the move bound), through solve_bound.hip and
// solve_move_bound.hip: placement_solve_bound_kernel and placement_solve_move_bound_kernel.  expand() then turns a dead child into a lost
// one and adds the spare term (bounded_move, bounded_value); the root's need is written as `bound`; and `complete` stays 1 while every
// cut keeps all its RUNNING candidates -- phase A counts them (a wave sum, four LDS words), phase C counts the kept ones that run where
// the twin only sets a flag.  Whatever else the bounded form needs stands under #ifdef TPL_PLACEMENT_BOUND_UNIT, so the two unbounded
// kernels are what they were, instruction for instruction (profiles/learner/bound_isa.log).
#include "tpl_beam.h"

namespace tpl_learn {
namespace {

constexpr int kF = kUnitFeatures;
constexpr int kSolveMaxMoves = 254;                           // M's limit (tpl_create's): a path fits kBeamBlock bytes
static_assert(kSolveMaxMoves + 1 <= kBeamBlock, "one lane per piece of the list and per byte of the path");
static_assert(kMaxWidth <= 256, "a parent's place fits the tape's low byte");

struct SolveArgs {
    const uint16_t* rows;        // [n][20], bit x = column x
    const uint8_t* pieces;       // [n][M + 1]
    uint32_t n;                  // configurations = workgroups
    uint32_t L, M;
    const float* weights;        // [12], or the first 14 of a row of 16
    uint32_t width;              // W in [1, 64]
    uint8_t* solved;             // [n]
    int32_t* solution_len;       // [n]
    uint8_t* actions;            // [n][M]
    float* best_value;           // [n][M], optional
#ifdef TPL_PLACEMENT_BOUND_UNIT
    float spare_weight;          // the bounded form's: the weight of a node's spare cells
    int32_t* bound;              // [n]: need(root)
    uint8_t* complete;           // [n]: 1 iff no cut dropped a running candidate
#endif
};

__device__ __forceinline__ float spare_weight_of(const SolveArgs& p) {
#ifdef TPL_PLACEMENT_BOUND_UNIT
    return p.spare_weight;
#else
    return 0.0f;
#endif
}

// Candidate k of running parent q under the ply's piece `cur`: the board the move leaves, the move's carry with the parent's (the
// rows cleared at 12 features), and the value of psi = (cleared, won, lost, features 3..11[, landing sum, eroded sum]).  Phases A and C and the winning ply all come here, so a candidate's
// second making gives the bits of the first.  In the bounded form a dead child is lost before psi is made, and its spare cells enter
// the value last (tpl_placement.h: bounded_move).
__device__ __forceinline__ float expand(const Beam& parent, uint32_t q, uint32_t k, uint32_t cur, const tpl::ShapeWord* shape,
                                        uint32_t L, uint32_t M, const float (&w)[kF], float spare_weight, tpl::Board& s,
                                        uint32_t& cleared, uint32_t& b) {
    uint32_t r, l;
    b = nth_placement(cur, k, r, l);
    tpl::unpack_board(parent.a[q], parent.b[q], s);
    s.window = cur;                                           // the list's piece; the entries behind it are not part of the rule
    s.window_hi = 0u;
    cleared = parent.cleared[q] + placed_move<kF>(s, shape, r, l, L, M);
    const int32_t spare = bounded_move(s, L, M);
    FeatureSet<kF> psi;
    moved_features(s, cleared, true, psi);
    if constexpr (kUnitBound) return bounded_value(placement_score(w, psi), spare_weight, spare);
    else return placement_score(w, psi);
}

// the sum of a wave's 64 values, in every lane
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ unsigned long long max4(const unsigned long long* v) {
    unsigned long long top = 0ull;
#pragma unroll
    for (int k = 0; k < kBeamBlock / 64; ++k) top = v[k] > top ? v[k] : top;
    return top;
}

// Five waves a SIMD, five workgroups a CU, as placement_beam_kernel has: 95 VGPRs without scratch once the weight row sits in SGPRs
// (tools/kernel_resources.sh; left to itself the allocator takes 105, which is four groups).
// The bounded form carries the four fill planes of move_bound_cells beside the board: bound to five it spills two registers (8 bytes of
// scratch a lane), so it is bound to four groups a CU, as the 14-feature beam is.
#ifdef TPL_PLACEMENT_BOUND_UNIT
#define TPL_SOLVE_BOUNDS __launch_bounds__(kBeamBlock, 4)
#else
#define TPL_SOLVE_BOUNDS __launch_bounds__(kBeamBlock, 5)
#endif
__global__ TPL_SOLVE_BOUNDS void TPL_UNIT_KERNEL(placement_solve)(const SolveArgs p) {
    extern __shared__ __attribute__((aligned(16))) uint16_t s_tape[];   // [M][W]: parent's place | placement << 8
    __shared__ tpl::ShapeWord s_shape[32];
    __shared__ Beam s_beam[2];
    __shared__ unsigned long long s_key[kMaxCandidates];
    __shared__ unsigned long long s_sel[kMaxWidth];
    __shared__ unsigned long long s_wave[2][kBeamBlock / 64];
    __shared__ unsigned long long s_won[kBeamBlock / 64];
    __shared__ uint32_t s_cols[tpl::kCols];
    __shared__ uint32_t s_running[2];
    __shared__ uint8_t s_pieces[kBeamBlock];
    __shared__ uint8_t s_path[kBeamBlock];
#ifdef TPL_PLACEMENT_BOUND_UNIT
    __shared__ uint32_t s_runs[kBeamBlock / 64];               // the running candidates of a ply, wave by wave
#endif
    const uint32_t tid = threadIdx.x, i = blockIdx.x;          // the grid is n blocks
    const uint32_t M = p.M, W = p.width;
    if (tid < 32) s_shape[tid] = tpl::kShapeTable[tid];
    if (tid <= M) s_pieces[tid] = p.pieces[(size_t)i * (M + 1u) + tid] & 7u;     // masked as move_board masks them
    s_path[tid] = (uint8_t)kNoMove;
    if (tid < (uint32_t)tpl::kCols) {                          // column tid of the board: bit r = row r
        const uint16_t* rows = p.rows + (size_t)i * tpl::kRows;
        uint32_t c = 0u;
#pragma unroll
        for (int r = 0; r < tpl::kRows; ++r) c |= (((uint32_t)rows[r] >> tid) & 1u) << r;
        s_cols[tid] = c;
    }
    __syncthreads();
    if (tid == 0) {                                            // Beam_0: the root alone, as a full reset deals it
        tpl::Board s;
#pragma unroll
        for (int x = 0; x < tpl::kCols; ++x) s.c[x] = s_cols[x];
        s.window = 0u; s.window_hi = 0u;
        s.state = tpl::ST_RUNNING; s.lines = 0u; s.moves = 0u; s.slot = 0u;
        uint4 A, B;
        tpl::pack_board(s, A, B);
        s_beam[0].a[0] = A;
        s_beam[0].b[0] = B;
        s_beam[0].value[0] = 0.0f;
        s_beam[0].cleared[0] = 0u;
#ifdef TPL_PLACEMENT_BOUND_UNIT
        p.bound[i] = (int32_t)((move_bound_cells(s.c, p.L) + 3u) >> 2);      // need(root): no solution is shorter
#endif
    }
    __syncthreads();
    float w[kF];                                               // one row for the whole grid: scalar loads, the weights stay in SGPRs
#pragma unroll
    for (int q = 0; q < kF; ++q) w[q] = p.weights[q];
    float* const best_value = p.best_value ? p.best_value + (size_t)i * M : nullptr;
    const float spare_weight = spare_weight_of(p);
    uint32_t complete = 1u;                                    // the bounded form's: no cut has dropped a running candidate

    uint32_t nodes = 1u, plies = 0u, length = 0u;              // plies run; the winning ply, 0 while there is none
#pragma unroll 1
    for (uint32_t ply = 0; ply < M; ++ply) {
        const Beam& parent = s_beam[ply & 1u];
        Beam& child = s_beam[(ply & 1u) ^ 1u];
        const uint32_t cur = s_pieces[ply];
        const uint32_t stride = placement_count(cur);
        const uint32_t total = nodes * stride;                 // at most 64 x 34 slots
        plies = ply + 1u;
        if (tid == 0) s_running[ply & 1u] = 0u;                // read last two plies ago

        // A: the keys, and per lane the largest won one
        unsigned long long won_mine = 0ull;
        uint32_t runs_mine = 0u;
#pragma unroll 1
        for (uint32_t slot = tid; slot < total; slot += kBeamBlock) {
            const Slot c = slot_of(parent, slot, stride);
            unsigned long long key = 0ull;
            if (c.finished) {
                if (c.k == 0u) key = ((unsigned long long)ordered_bits(parent.value[c.q]) << 32) | (kSlotTop - slot);
            } else {
                tpl::Board s;
                uint32_t cleared, b;
                const float value = expand(parent, c.q, c.k, cur, s_shape, p.L, M, w, spare_weight, s, cleared, b);
                key = ((unsigned long long)ordered_bits(value) << 32) | (kSlotTop - slot);
                if (s.state == tpl::ST_WON) won_mine = key > won_mine ? key : won_mine;
                if constexpr (kUnitBound) runs_mine += s.state == tpl::ST_RUNNING ? 1u : 0u;
            }
            s_key[slot] = key;
        }
        won_mine = wave_max(won_mine);
        if ((tid & 63u) == 0u) s_won[tid >> 6] = won_mine;
#ifdef TPL_PLACEMENT_BOUND_UNIT
        runs_mine = wave_sum(runs_mine);
        if ((tid & 63u) == 0u) s_runs[tid >> 6] = runs_mine;
#endif
        __syncthreads();

        // the stop: a won candidate anywhere in the ply, before the cut
        const unsigned long long won = max4(s_won);
        if (won != 0ull) {                                     // the same words for every lane
            length = ply + 1u;
            if (tid == 0) {                                    // the won candidate that comes first: its placement, then the tape
                const Slot c = slot_of(parent, kSlotTop - (uint32_t)won, stride);
                uint32_t r, l;
                s_path[ply] = (uint8_t)nth_placement(cur, c.k, r, l);
                uint32_t place = c.q;
                for (uint32_t t = ply; t-- > 0u;) {
                    const uint32_t e = s_tape[t * W + place];
                    s_path[t] = (uint8_t)(e >> 8);
                    place = e & 0xFFu;
                }
            }
            if ((tid >> 6) == 1u && best_value) {              // the second wave: the candidate that comes first of all, made again
                unsigned long long top = 0ull;
#pragma unroll 1
                for (uint32_t slot = tid & 63u; slot < total; slot += 64u) top = s_key[slot] > top ? s_key[slot] : top;
                top = wave_max(top);
                if (tid == 64u) {
                    const Slot c = slot_of(parent, kSlotTop - (uint32_t)top, stride);
                    float value = parent.value[c.q];
                    if (!c.finished) {
                        tpl::Board s;
                        uint32_t cleared, b;
                        value = expand(parent, c.q, c.k, cur, s_shape, p.L, M, w, spare_weight, s, cleared, b);
                    }
                    best_value[ply] = value;
                }
            }
            break;
        }

#ifdef TPL_PLACEMENT_BOUND_UNIT
        uint32_t runs = 0u;                                    // read before phase B's barriers, written again a ply later
#pragma unroll
        for (int v = 0; v < kBeamBlock / 64; ++v) runs += s_runs[v];
#endif

        // B: the min(W, count) largest keys, best first
        const uint32_t kept = select_keys(s_key, s_sel, s_wave, total, W, tid);

        // C: the kept candidates, in candidate order
        if (tid < kept) {
            const uint32_t low = (uint32_t)s_sel[tid];
            const uint32_t place = place_of(s_sel, kept, low);
            const Slot c = slot_of(parent, kSlotTop - low, stride);
            const uint32_t q = c.q;
            float value;
            if (c.finished) {
                child.a[place] = parent.a[q];
                child.b[place] = parent.b[q];
                child.cleared[place] = parent.cleared[q];
                value = parent.value[q];
                s_tape[ply * W + place] = (uint16_t)(q | (kNoMove << 8));
            } else {
                tpl::Board s;
                uint32_t cleared, b;
                value = expand(parent, q, c.k, cur, s_shape, p.L, M, w, spare_weight, s, cleared, b);
                uint4 A, B;
                tpl::pack_board(s, A, B);
                child.a[place] = A;
                child.b[place] = B;
                child.cleared[place] = cleared;
                s_tape[ply * W + place] = (uint16_t)(q | (b << 8));
                if constexpr (kUnitBound) {                    // counted: the cut is complete where every running candidate is kept
                    if (s.state == tpl::ST_RUNNING) atomicAdd(&s_running[ply & 1u], 1u);
                } else {
                    if (s.state == tpl::ST_RUNNING) s_running[ply & 1u] = 1u;
                }
            }
            child.value[place] = value;
            if (tid == 0 && best_value) best_value[ply] = value;   // lane 0 owns sel[0], the best
        }
        __syncthreads();
        nodes = kept;
#ifdef TPL_PLACEMENT_BOUND_UNIT
        complete = s_running[ply & 1u] == runs ? complete : 0u;
#endif
        if (s_running[ply & 1u] == 0u) break;                  // no node of the new beam runs: this beam found no win
    }
    __syncthreads();                                           // the path

    if (tid == 0) {
        p.solved[i] = length != 0u ? (uint8_t)1 : (uint8_t)0;
        p.solution_len[i] = (int32_t)length;
#ifdef TPL_PLACEMENT_BOUND_UNIT
        p.complete[i] = (uint8_t)complete;
#endif
    }
    if (tid < M) p.actions[(size_t)i * M + tid] = s_path[tid];
    if (best_value && tid >= plies && tid < M) best_value[tid] = 0.0f;
}

}  // namespace
}  // namespace tpl_learn

using namespace tpl_learn;

// the bounded entries take spare_weight behind the width and bound and complete behind best_value (include/tpl_learn.h)
#ifdef TPL_PLACEMENT_BOUND_UNIT
#define TPL_SOLVE_SPARE_PARAM float spare_weight,
#define TPL_SOLVE_BOUND_PARAMS int32_t* bound, uint8_t* complete,
#else
#define TPL_SOLVE_SPARE_PARAM
#define TPL_SOLVE_BOUND_PARAMS
#endif

extern "C" int TPL_UNIT_ENTRY(tpl_placement_solve)(const int16_t* rows, const uint8_t* pieces, int64_t n, int32_t L, int32_t M,
                                   const float* weights, int32_t width, TPL_SOLVE_SPARE_PARAM uint8_t* solved,
                                   int32_t* solution_len, uint8_t* actions, float* best_value, TPL_SOLVE_BOUND_PARAMS
                                   void* stream) {
    const char* name = TPL_UNIT_ENTRY_NAME(tpl_placement_solve);
#ifdef TPL_PLACEMENT_BOUND_UNIT
    if (!bound || !complete) return fail_msg(TPL_ERR_ARG, "%s: null pointer (bound and complete are required)", name);
    if (!(spare_weight - spare_weight == 0.0f)) return fail_msg(TPL_ERR_ARG, "%s: spare_weight must be finite", name);
    if ((uintptr_t)bound & 3u) return fail_msg(TPL_ERR_ARG, "%s: bound must be 4-byte aligned", name);
#endif
    if (!rows || !pieces || !weights || !solved || !solution_len || !actions)
        return fail_msg(TPL_ERR_ARG, "%s: null pointer (only best_value is optional)", name);
    if (n < 1) return fail_msg(TPL_ERR_ARG, "%s: n must be positive", name);
    if (n >= ((int64_t)1 << 31)) return fail_msg(TPL_ERR_ARG, "%s: n too large (a workgroup per configuration: n must stay below 2^31)", name);
    if (L < 1 || L > 250 || M < 1 || M > kSolveMaxMoves)
        return fail_msg(TPL_ERR_ARG, "%s: L and M must be in [1, 250] and [1, %d]", name, kSolveMaxMoves);
    if (width < 1 || width > kMaxWidth) return fail_msg(TPL_ERR_ARG, "%s: width must be in [1, %d]", name, kMaxWidth);
    if ((uintptr_t)rows & 1u) return fail_msg(TPL_ERR_ARG, "%s: rows must be 2-byte aligned", name);
    if ((uintptr_t)weights & 15u) return fail_msg(TPL_ERR_ARG, "%s: weights must be 16-byte aligned", name);
    if ((uintptr_t)solution_len & 3u) return fail_msg(TPL_ERR_ARG, "%s: solution_len must be 4-byte aligned", name);
    if ((uintptr_t)best_value & 3u) return fail_msg(TPL_ERR_ARG, "%s: best_value must be 4-byte aligned", name);
    SolveArgs p{};
    p.rows = (const uint16_t*)rows; p.pieces = pieces; p.n = (uint32_t)n;
    p.L = (uint32_t)L; p.M = (uint32_t)M; p.weights = weights; p.width = (uint32_t)width;
    p.solved = solved; p.solution_len = solution_len; p.actions = actions; p.best_value = best_value;
#ifdef TPL_PLACEMENT_BOUND_UNIT
    p.spare_weight = spare_weight; p.bound = bound; p.complete = complete;
#endif
    const size_t tape = ((size_t)2 * p.width * p.M + 15u) & ~(size_t)15u;         // at most 32,512 bytes
    hipLaunchKernelGGL(TPL_UNIT_KERNEL(placement_solve), dim3(p.n), dim3(kBeamBlock), tape, (hipStream_t)stream, p);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}
