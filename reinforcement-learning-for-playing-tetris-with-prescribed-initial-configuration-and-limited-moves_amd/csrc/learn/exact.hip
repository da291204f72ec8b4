// exact.hip -- an exact depth-first solver for prescribed configurations: tpl_placement_exact (include/tpl_learn.h states the rule).
//
// tpl_placement_solve_bound is a beam: its width cut is what keeps it from being a proof.  This kernel searches the same game with
// the same children -- solve.hip's expand() in the bounded form: placed_move, bounded_move, psi with the path's carry,
// placement_score, bounded_value -- depth first.  Within the move bound's prune it visits every running board, or it stops at a node
// budget and says so.  With `shortest` it deepens the budget B from need(root) to M, so the first win it meets is a shortest one.
//
// Mapping: ONE CONFIGURATION PER WAVEFRONT, one wavefront a workgroup, so the data-dependent search loop holds no barrier at all; what
// one lane writes to LDS for the others is ordered by wave_sync(), which emits no instruction but the wait for the write.
//   the node    being expanded is read from its stack record by every lane; lane k < 34 makes child k, the k-th distinct placement of
//               the ply's piece in ascending b, and its 64-bit key (ordered_bits(value) << 32 | kSlotTop - k), so a larger key comes
//               first in the rule's order.  The other lanes idle: the search is divergent by nature.
//   the stop    a ballot over the won children; if any is set the largest won key names the child the solution ends with.
//   the order   the running children are ranked by their keys: 34 lane reads of a key, a compare and an add each.  A running
//               child writes its placement to place `rank` of the record's list; the one of rank 0 also writes the next record, since
//               it is descended into at once.
//   the stack   dynamic LDS, one 80-byte record a depth: the node's packed board (two uint4), its carry word, the number of its
//               running children, a cursor, and the list.  A running child at depth d + 1 has made d + 1 < B <= M moves, so M records
//               hold every path: 3,200 bytes at M = 40, 20,320 at M = 254.
//   the return  a later child is made again from its parent's record and the list's placement when the search comes back to it, as
//               the beam makes a kept candidate again in its phase C.
// Nothing but the outputs goes to memory.
//
// Built twice: as it stands, placement_exact_kernel on the twelve board features, and through exact_move.hip as
// placement_exact_move_kernel on the fourteen.  Both are units of the BOUNDED form (tpl_placement.h: kUnitBound): the prune is what
// makes the search finite in practice and its proof is the move bound's, so there is no unbounded twin and the entries carry no
// _bound in their names.
#ifndef TPL_PLACEMENT_BOUND_UNIT
#define TPL_PLACEMENT_BOUND_UNIT
#endif
#include "tpl_beam.h"

namespace tpl_learn {
namespace {

constexpr int kF = kUnitFeatures;
constexpr int kExactMaxMoves = 254;                           // M's limit (tpl_create's)
constexpr int kExactWave = 64;
constexpr int kExactMaxNodes = TPL_EXACT_MAX_NODES;
static_assert(kUnitBound, "the exact search is a unit of the bounded form");
static_assert(kMaxPlacements <= kExactWave, "a lane per child");

#define TPL_EXACT_KERNEL TPL_UNIT_PASTE4(placement_exact, TPL_UNIT_FORM, , _kernel)
#define TPL_EXACT_ENTRY TPL_UNIT_PASTE4(tpl_placement_exact, TPL_UNIT_FORM, , )
#define TPL_EXACT_ENTRY_NAME "tpl_placement_exact" TPL_UNIT_FORM_NAME

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

// one depth of the stack
struct alignas(16) Frame {
    uint4 a, b;                  // the node's board; its window is not part of the rule
    uint32_t carry;              // of the path to the node (tpl_placement.h)
    uint32_t count;              // its running children
    uint32_t cursor;             // how many of them have been descended into
    uint8_t kids[36];            // their placements b = 10 r + l in the order of the descent, kMaxPlacements at most
};
static_assert(sizeof(Frame) == 80, "a record is 80 bytes");

// LDS written by one lane, read by another of the same wave: the accesses of a wave reach LDS in order, so this only keeps the
// compiler from moving them across and waits for the write
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// The child of `node` by placement (r, l) of piece `cur` in the game (L, B), exactly as solve.hip's expand() makes a bounded candidate:
// the board the move leaves, dead turned lost, the carry of the path with the move's, and the value.  The expansion and the return
// both come here, so a child's second making gives the board of the first.
__device__ __forceinline__ float make_child(const Frame& node, uint32_t cur, uint32_t r, uint32_t l, const tpl::ShapeWord* shape,
                                            uint32_t L, uint32_t B, const float (&w)[kF], float spare_weight, tpl::Board& s,
                                            uint32_t& carry) {
    tpl::unpack_board(node.a, node.b, s);
    s.window = cur;
    s.window_hi = 0u;
    carry = node.carry + placed_move<kF>(s, shape, r, l, L, B);
    const int32_t spare = bounded_move(s, L, B);
    FeatureSet<kF> psi;
    moved_features(s, carry, true, psi);
    return bounded_value(placement_score(w, psi), spare_weight, spare);
}

__device__ __forceinline__ void store_frame(Frame& f, const tpl::Board& s, uint32_t carry) {
    uint4 A, B;
    tpl::pack_board(s, A, B);
    f.a = A;
    f.b = B;
    f.carry = carry;
}

// One wave a workgroup, bound to eight waves a SIMD.  A wave's search is one long dependent chain -- a record read from LDS, a move,
// the features, a rank, a record written -- so what hides its latency is other waves, and the kernel fits the most a SIMD takes: 64
// VGPRs without scratch in both forms, since everything the 34 children share sits in SGPRs (tools/kernel_resources.sh;
// profiles/learner/exact_isa.log).  Left to itself the allocator takes 106 SGPRs, which is seven waves; bound to eight it takes 78
// and no VGPR more.  The 32 stacks of a CU are 116 KB of its 160 at M = 40; at M = 254 LDS admits seven workgroups a CU.
__global__ __launch_bounds__(kExactWave, 8) void TPL_EXACT_KERNEL(const ExactArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    Frame* const stack = reinterpret_cast<Frame*>(s_raw);      // [M]
    __shared__ tpl::ShapeWord s_shape[32];
    __shared__ uint8_t s_pieces[kExactMaxMoves + 2];
    const uint32_t lane = threadIdx.x, i = blockIdx.x;         // the grid is n blocks of one wave
    const uint32_t L = p.L, M = p.M;
    if (lane < 32) s_shape[lane] = tpl::kShapeTable[lane];
    for (uint32_t t = lane; t <= M; t += kExactWave) s_pieces[t] = p.pieces[(size_t)i * (M + 1u) + t] & 7u;   // masked as move_board masks them

    tpl::Board root;                                           // the root, as a full reset deals it: the same in every lane
    tpl::rows_to_cols(p.rows + (size_t)i * tpl::kRows, root.c);
    root.window = 0u; root.window_hi = 0u;
    root.state = tpl::ST_RUNNING; root.lines = 0u; root.moves = 0u; root.slot = 0u;
    const uint32_t bound = (move_bound_cells(root.c, L) + 3u) >> 2;          // need(root): no solution is shorter

    float w[kF];                                               // one row for the whole grid: scalar loads, the weights stay in SGPRs
#pragma unroll
    for (int q = 0; q < kF; ++q) w[q] = p.weights[q];
    const float spare_weight = p.spare_weight;
    const uint32_t max_nodes = p.max_nodes;

    uint32_t nodes = 0u, length = 0u, last = kNoMove;          // expansions; the winning length, 0 while there is none, and its last move
    bool capped = false;
    if (bound <= M) {
#pragma unroll 1
        for (uint32_t B = p.shortest ? bound : M; B <= M && length == 0u && !capped; ++B) {
            wave_sync();                                       // the last iteration's reads of record 0 (and, the first time, the tables)
            if (lane == 0) store_frame(stack[0], root, 0u);
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
                uint32_t r, l, carry;
                const uint32_t b = nth_placement(cur, k, r, l);
                tpl::Board s;
                const float value = make_child(stack[d], cur, r, l, s_shape, L, B, w, spare_weight, s, carry);
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
                const uint32_t count = (uint32_t)__builtin_popcountll(__ballot(running));
                if (running) {
                    stack[d].kids[rank] = (uint8_t)b;
                    if (rank == 0u && d + 1u < M) store_frame(stack[d + 1u], s, carry);      // descended into at once (d + 1 < B <= M)
                }
                if (lane == 0) {
                    stack[d].count = count;
                    stack[d].cursor = count != 0u ? 1u : 0u;
                }
                wave_sync();
                if (count != 0u) { ++d; continue; }

                // no running child: back to the nearest node that has one left, and into it
                bool more = false;
#pragma unroll 1
                while (d > 0u) {
                    --d;
                    const uint32_t at = uniform(stack[d].cursor);
                    if (at < uniform(stack[d].count)) {
                        const uint32_t b2 = uniform(stack[d].kids[at]);
                        tpl::Board s2;
                        uint32_t carry2;
                        make_child(stack[d], uniform(s_pieces[d]), b2 / 10u, b2 % 10u, s_shape, L, B, w, spare_weight, s2, carry2);
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
                if (!more) break;                              // the root's children are used up: no win at this budget
            }
        }
    }
    wave_sync();

    if (capped) length = 0u;
    if (lane == 0) {
        p.solved[i] = length != 0u ? (uint8_t)1 : (uint8_t)0;
        p.proved[i] = capped ? (uint8_t)0 : (uint8_t)1;
        p.solution_len[i] = (int32_t)length;
        p.bound[i] = (int32_t)bound;
        p.nodes[i] = nodes;
    }
    // the solution: the child in hand at every depth of the path, then the won one
    for (uint32_t t = lane; t < M; t += kExactWave) {
        uint32_t a = kNoMove;
        if (t + 1u < length) a = stack[t].kids[stack[t].cursor - 1u];
        else if (t + 1u == length) a = last;
        p.actions[(size_t)i * M + t] = (uint8_t)a;
    }
}

}  // namespace
}  // namespace tpl_learn

using namespace tpl_learn;

extern "C" int TPL_EXACT_ENTRY(const int16_t* rows, const uint8_t* pieces, int64_t n, int32_t L, int32_t M, const float* weights,
                               float spare_weight, int32_t max_nodes, int32_t shortest, uint8_t* solved, uint8_t* proved,
                               int32_t* solution_len, uint8_t* actions, int32_t* bound, uint32_t* nodes, void* stream) {
    const char* name = TPL_EXACT_ENTRY_NAME;
    if (!rows || !pieces || !weights || !solved || !proved || !solution_len || !actions || !bound || !nodes)
        return fail_msg(TPL_ERR_ARG, "%s: null pointer (every argument but the stream is required)", name);
    if (!(spare_weight - spare_weight == 0.0f)) return fail_msg(TPL_ERR_ARG, "%s: spare_weight must be finite", name);
    if (n < 1) return fail_msg(TPL_ERR_ARG, "%s: n must be positive", name);
    if (n >= ((int64_t)1 << 31)) return fail_msg(TPL_ERR_ARG, "%s: n too large (a workgroup per configuration: n must stay below 2^31)", name);
    if (L < 1 || L > 250 || M < 1 || M > kExactMaxMoves)
        return fail_msg(TPL_ERR_ARG, "%s: L and M must be in [1, 250] and [1, %d]", name, kExactMaxMoves);
    if (max_nodes < 1 || max_nodes > kExactMaxNodes) return fail_msg(TPL_ERR_ARG, "%s: max_nodes must be in [1, %d]", name, kExactMaxNodes);
    if (shortest != 0 && shortest != 1) return fail_msg(TPL_ERR_ARG, "%s: shortest must be 0 or 1", name);
    if ((uintptr_t)rows & 1u) return fail_msg(TPL_ERR_ARG, "%s: rows must be 2-byte aligned", name);
    if ((uintptr_t)weights & 15u) return fail_msg(TPL_ERR_ARG, "%s: weights must be 16-byte aligned", name);
    if ((uintptr_t)solution_len & 3u) return fail_msg(TPL_ERR_ARG, "%s: solution_len must be 4-byte aligned", name);
    if ((uintptr_t)bound & 3u) return fail_msg(TPL_ERR_ARG, "%s: bound must be 4-byte aligned", name);
    if ((uintptr_t)nodes & 3u) return fail_msg(TPL_ERR_ARG, "%s: nodes must be 4-byte aligned", name);
    ExactArgs p{};
    p.rows = (const uint16_t*)rows; p.pieces = pieces; p.n = (uint32_t)n;
    p.L = (uint32_t)L; p.M = (uint32_t)M; p.weights = weights; p.spare_weight = spare_weight;
    p.max_nodes = (uint32_t)max_nodes; p.shortest = (uint32_t)shortest;
    p.solved = solved; p.proved = proved; p.solution_len = solution_len; p.actions = actions; p.bound = bound; p.nodes = nodes;
    const size_t stack = sizeof(Frame) * (size_t)p.M;          // at most 20,320 bytes
    hipLaunchKernelGGL(TPL_EXACT_KERNEL, dim3(p.n), dim3(kExactWave), stack, (hipStream_t)stream, p);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}
