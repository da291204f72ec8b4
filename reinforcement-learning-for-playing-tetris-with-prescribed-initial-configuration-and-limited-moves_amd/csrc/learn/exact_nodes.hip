// exact_nodes.hip -- the exact depth-first search started at a NODE of a prescribed game, and the proved labels of a node's moves:
// tpl_placement_exact_nodes and tpl_placement_exact_labels (include/tpl_learn.h states both rules).
//
// A node -- a board, the lines cleared and the moves made so far, the piece list of its configuration -- is, for the search of
// exact.hip, a fresh configuration of the SHIFTED game: the same board, the list from pieces[moves] on, and (L - lines, M - moves)
// for (L, M).  The move, the terminal tests, cells, spare, the board features and the carry read nothing else.  So both kernels here
// shift first -- two subtractions and an offset into the list -- and then run exact.hip's search word for word on a root with 0
// lines, 0 moves and carry 0.  The game is then a value of the wave, not of the launch: L and M below are read per node and made
// uniform, which costs scalar registers and nothing else.
//
// Mapping: exact.hip's frame.  ONE NODE PER WAVEFRONT, one wavefront a workgroup, no barrier; lanes 0 .. 33 a child each, 64-bit keys
// ranked across the wave, the stack in dynamic LDS at 80 bytes a depth, indexed by the depth FROM THE NODE and sized by the launch's
// M, which no shifted game exceeds.
//   placement_exact_nodes_kernel    a wave a node: the search, and the six outputs of tpl_placement_exact counted from the node.
//   placement_exact_labels_kernel   a wave a (node, placement b): the one move b of the node's piece, made as the search makes a child,
//                                   then the verdict of the move -- at once where the child is finished, and by the same search from
//                                   the child, one more shift, where it runs.
// A node whose lines, moves or entry are out of range is finished: its outputs are written and nothing else is read.
//
// The search loop is exact.hip's, duplicated: that unit stays as it is, with its instructions (profiles/learner/exact_nodes_isa.log).
// Built twice, as exact.hip is: as it stands on the twelve board features and through exact_nodes_move.hip on the fourteen.
#ifndef TPL_PLACEMENT_BOUND_UNIT
#define TPL_PLACEMENT_BOUND_UNIT
#endif
#include "tpl_beam.h"

namespace tpl_learn {
namespace {

constexpr int kF = kUnitFeatures;
constexpr int kNodesMaxMoves = 254;                           // M's limit (tpl_create's)
constexpr int kNodesWave = 64;
constexpr int kNodesMaxNodes = TPL_EXACT_MAX_NODES;
static_assert(kUnitBound, "the exact search is a unit of the bounded form");
static_assert(kMaxPlacements <= kNodesWave, "a lane per child");

#define TPL_NODES_KERNEL TPL_UNIT_PASTE4(placement_exact_nodes, TPL_UNIT_FORM, , _kernel)
#define TPL_NODES_ENTRY TPL_UNIT_PASTE4(tpl_placement_exact_nodes, TPL_UNIT_FORM, , )
#define TPL_NODES_ENTRY_NAME "tpl_placement_exact_nodes" TPL_UNIT_FORM_NAME
#define TPL_LABELS_KERNEL TPL_UNIT_PASTE4(placement_exact_labels, TPL_UNIT_FORM, , _kernel)
#define TPL_LABELS_ENTRY TPL_UNIT_PASTE4(tpl_placement_exact_labels, TPL_UNIT_FORM, , )
#define TPL_LABELS_ENTRY_NAME "tpl_placement_exact_labels" TPL_UNIT_FORM_NAME

// what both kernels read
struct NodeInputs {
    const uint16_t* rows;        // [n][20], bit x = column x
    const uint8_t* lines;        // [n]
    const uint8_t* moves;        // [n]
    const uint32_t* entry;       // [n]: the node's list is pieces[entry]
    const uint8_t* pieces;       // [n_cfg][M + 1]
    uint32_t n, n_cfg;
    uint32_t L, M;
    const float* weights;        // [12], or the first 14 of a row of 16
    float spare_weight;
    uint32_t max_nodes;          // in [1, 2^24]
};

struct NodesArgs {
    NodeInputs in;
    uint32_t shortest;           // 1: budgets need(node) .. M - moves of the shifted game; 0: M - moves alone
    uint8_t* solved;             // [n]
    uint8_t* proved;             // [n]
    int32_t* solution_len;       // [n], from the node
    uint8_t* actions;            // [n][M], from the node
    int32_t* bound;              // [n]: need(node)
    uint32_t* nodes;             // [n]
};

struct LabelsArgs {
    NodeInputs in;
    uint8_t* label;              // [n][40]
    int32_t* length;             // [n][40]
    uint32_t* nodes;             // [n][40]
};

// one depth of the stack (exact.hip's record)
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

// the child of `node` by placement (r, l) of piece `cur` in the game (L, B), as exact.hip makes it
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

// a node's place in the game, the same in every lane; a node that is not `live` is finished
struct Place {
    uint32_t L, M;               // of the shifted game: lines still owed, moves still left
    size_t first;                // index into pieces of the node's current piece
    bool live;
};
__device__ __forceinline__ Place place_of_node(const NodeInputs& in, uint32_t i) {
    const uint32_t lines = uniform(in.lines[i]), moves = uniform(in.moves[i]), entry = uniform(in.entry[i]);
    Place at;
    at.live = lines < in.L && moves < in.M && entry < in.n_cfg;
    at.L = at.live ? in.L - lines : 1u;
    at.M = at.live ? in.M - moves : 1u;
    at.first = at.live ? (size_t)entry * (in.M + 1u) + moves : (size_t)0;    // first + at.M = entry (M + 1) + M: the list's last
    return at;
}

// a fresh root of a shifted game: 0 lines, 0 moves, running; the columns are left to the caller
__device__ __forceinline__ void fresh_root(tpl::Board& root) {
    root.window = 0u; root.window_hi = 0u;
    root.state = tpl::ST_RUNNING; root.lines = 0u; root.moves = 0u; root.slot = 0u;
}

struct Found {
    uint32_t nodes, length, last, bound;                       // expansions; the winning length, 0 if none, and its last move; need(root)
    bool capped;
};

// exact.hip's search of the game (L, M) from `root` -- the same in every lane, 0 lines, 0 moves, carry 0 -- whose piece at depth d is
// pieces[first + d] & 7, d <= M.  The caller has filled s_shape.  On return the path of a win is in the stack: the child in hand at
// every depth, then `last`.
__device__ __forceinline__ Found search(Frame* stack, uint8_t* s_pieces, const tpl::ShapeWord* s_shape, const tpl::Board& root,
                                        const uint8_t* pieces, size_t first, uint32_t L, uint32_t M, const float (&w)[kF],
                                        float spare_weight, uint32_t max_nodes, uint32_t shortest, uint32_t lane) {
    for (uint32_t t = lane; t <= M; t += kNodesWave) s_pieces[t] = pieces[first + t] & 7u;   // masked as move_board masks them
    Found out;
    out.bound = (move_bound_cells(root.c, L) + 3u) >> 2;      // need(root): no solution is shorter
    out.nodes = 0u; out.length = 0u; out.last = kNoMove; out.capped = false;
    uint32_t nodes = 0u, length = 0u, last = kNoMove;
    bool capped = false;
    if (out.bound <= M) {
#pragma unroll 1
        for (uint32_t B = shortest ? out.bound : M; B <= M && length == 0u && !capped; ++B) {
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
    out.nodes = nodes;
    out.length = capped ? 0u : length;
    out.last = last;
    out.capped = capped;
    return out;
}

// One wave a workgroup, bound to eight waves a SIMD as exact.hip's kernel is and for its reason: a wave's search is one dependent
// chain, and what hides its latency is other waves (tools/kernel_resources.sh; profiles/learner/exact_nodes_isa.log).
__global__ __launch_bounds__(kNodesWave, 8) void TPL_NODES_KERNEL(const NodesArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    Frame* const stack = reinterpret_cast<Frame*>(s_raw);      // [M]
    __shared__ tpl::ShapeWord s_shape[32];
    __shared__ uint8_t s_pieces[kNodesMaxMoves + 2];
    const uint32_t lane = threadIdx.x, i = blockIdx.x;         // the grid is n blocks of one wave
    const uint32_t M = p.in.M;
    const Place at = place_of_node(p.in, i);
    if (!at.live) {                                            // a finished node: nothing to search, nothing more is read
        if (lane == 0) {
            p.solved[i] = (uint8_t)0;
            p.proved[i] = (uint8_t)1;
            p.solution_len[i] = 0;
            p.bound[i] = 0;
            p.nodes[i] = 0u;
        }
        for (uint32_t t = lane; t < M; t += kNodesWave) p.actions[(size_t)i * M + t] = (uint8_t)kNoMove;
        return;
    }
    if (lane < 32) s_shape[lane] = tpl::kShapeTable[lane];

    tpl::Board root;                                           // the node as the root of its shifted game: the same in every lane
    tpl::rows_to_cols(p.in.rows + (size_t)i * tpl::kRows, root.c);
    fresh_root(root);

    float w[kF];                                               // one row for the whole grid: scalar loads, the weights stay in SGPRs
#pragma unroll
    for (int q = 0; q < kF; ++q) w[q] = p.in.weights[q];

    const Found f = search(stack, s_pieces, s_shape, root, p.in.pieces, at.first, at.L, at.M, w, p.in.spare_weight, p.in.max_nodes,
                           p.shortest, lane);
    if (lane == 0) {
        p.solved[i] = f.length != 0u ? (uint8_t)1 : (uint8_t)0;
        p.proved[i] = f.capped ? (uint8_t)0 : (uint8_t)1;
        p.solution_len[i] = (int32_t)f.length;
        p.bound[i] = (int32_t)f.bound;
        p.nodes[i] = f.nodes;
    }
    // the solution from the node: the child in hand at every depth of the path, then the won one; 255 up to the launch's M
    for (uint32_t t = lane; t < M; t += kNodesWave) {
        uint32_t a = kNoMove;
        if (t + 1u < f.length) a = stack[t].kids[stack[t].cursor - 1u];
        else if (t + 1u == f.length) a = f.last;
        p.actions[(size_t)i * M + t] = (uint8_t)a;
    }
}

// One wave a (node, action): block 40 i + b.  The move is made by every lane alike, so the child is a value of the wave; its verdict
// is read through `uniform`, and the branch on it is scalar.
__global__ __launch_bounds__(kNodesWave, 8) void TPL_LABELS_KERNEL(const LabelsArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    Frame* const stack = reinterpret_cast<Frame*>(s_raw);      // [M]
    __shared__ tpl::ShapeWord s_shape[32];
    __shared__ uint8_t s_pieces[kNodesMaxMoves + 2];
    const uint32_t lane = threadIdx.x, slot = blockIdx.x;      // the grid is 40 n blocks of one wave
    const uint32_t i = slot / (uint32_t)kActions, b = slot - i * (uint32_t)kActions;
    const Place at = place_of_node(p.in, i);
    uint32_t label = TPL_LABEL_NONE, length = 0u, nodes = 0u;
    if (at.live) {
        const uint32_t cur = uniform(p.in.pieces[at.first]) & 7u;
        const uint32_t r = b / 10u, l = b - 10u * r;
        if (canonical_action(cur, r, l) == b) {                // a distinct placement of the node's piece
            if (lane < 32) s_shape[lane] = tpl::kShapeTable[lane];
            wave_sync();
            tpl::Board s;
            tpl::rows_to_cols(p.in.rows + (size_t)i * tpl::kRows, s.c);
            fresh_root(s);
            s.window = cur;
            placed_move<kF>(s, s_shape, r, l, at.L, at.M);     // as the search makes a child: the move, then the bound's verdict
            bounded_move(s, at.L, at.M);
            const uint32_t state = uniform(s.state);
            if (state == tpl::ST_WON) {
                label = TPL_LABEL_WIN;
                length = 1u;
            } else if (state != tpl::ST_RUNNING) {
                label = TPL_LABEL_LOSS;
            } else {
                // the running child is a node one move on: it owes what the move did not clear and has a move less
                const uint32_t child_L = at.L - uniform(s.lines), child_M = at.M - 1u;
                tpl::Board root;
#pragma unroll
                for (int x = 0; x < tpl::kCols; ++x) root.c[x] = uniform(s.c[x]);
                fresh_root(root);
                float w[kF];
#pragma unroll
                for (int q = 0; q < kF; ++q) w[q] = p.in.weights[q];
                const Found f = search(stack, s_pieces, s_shape, root, p.in.pieces, at.first + 1u, child_L, child_M, w,
                                       p.in.spare_weight, p.in.max_nodes, 1u, lane);
                nodes = f.nodes;
                label = f.capped ? TPL_LABEL_OPEN : f.length != 0u ? TPL_LABEL_WIN : TPL_LABEL_LOSS;
                length = f.length != 0u ? 1u + f.length : 0u;
            }
        }
    }
    if (lane == 0) {
        p.label[slot] = (uint8_t)label;
        p.length[slot] = (int32_t)length;
        p.nodes[slot] = nodes;
    }
}

// what both entries refuse of the arguments they share; `name` leads the message
int check_nodes(const char* name, const int16_t* rows, const uint8_t* lines, const uint8_t* moves, const uint32_t* entry,
                const uint8_t* pieces, int64_t n, int64_t n_cfg, int32_t L, int32_t M, const float* weights, float spare_weight,
                int32_t max_nodes, int64_t waves_per_node) {
    if (!rows || !lines || !moves || !entry || !pieces || !weights)
        return fail_msg(TPL_ERR_ARG, "%s: null pointer (every argument but the stream is required)", name);
    if (!(spare_weight - spare_weight == 0.0f)) return fail_msg(TPL_ERR_ARG, "%s: spare_weight must be finite", name);
    if (n < 1) return fail_msg(TPL_ERR_ARG, "%s: n must be positive", name);
    if (n >= (((int64_t)1 << 31) + waves_per_node - 1) / waves_per_node)
        return fail_msg(TPL_ERR_ARG, "%s: n too large (%d workgroup(s) per node: their number must stay below 2^31)", name,
                        (int)waves_per_node);
    if (n_cfg < 1 || n_cfg >= ((int64_t)1 << 31)) return fail_msg(TPL_ERR_ARG, "%s: n_cfg must be in [1, 2^31)", name);
    if (L < 1 || L > 250 || M < 1 || M > kNodesMaxMoves)
        return fail_msg(TPL_ERR_ARG, "%s: L and M must be in [1, 250] and [1, %d]", name, kNodesMaxMoves);
    if (max_nodes < 1 || max_nodes > kNodesMaxNodes) return fail_msg(TPL_ERR_ARG, "%s: max_nodes must be in [1, %d]", name, kNodesMaxNodes);
    if ((uintptr_t)rows & 1u) return fail_msg(TPL_ERR_ARG, "%s: rows must be 2-byte aligned", name);
    if ((uintptr_t)entry & 3u) return fail_msg(TPL_ERR_ARG, "%s: entry must be 4-byte aligned", name);
    if ((uintptr_t)weights & 15u) return fail_msg(TPL_ERR_ARG, "%s: weights must be 16-byte aligned", name);
    return TPL_OK;
}

NodeInputs node_inputs(const int16_t* rows, const uint8_t* lines, const uint8_t* moves, const uint32_t* entry, const uint8_t* pieces,
                       int64_t n, int64_t n_cfg, int32_t L, int32_t M, const float* weights, float spare_weight, int32_t max_nodes) {
    NodeInputs in{};
    in.rows = (const uint16_t*)rows; in.lines = lines; in.moves = moves; in.entry = entry; in.pieces = pieces;
    in.n = (uint32_t)n; in.n_cfg = (uint32_t)n_cfg; in.L = (uint32_t)L; in.M = (uint32_t)M;
    in.weights = weights; in.spare_weight = spare_weight; in.max_nodes = (uint32_t)max_nodes;
    return in;
}

}  // namespace
}  // namespace tpl_learn

using namespace tpl_learn;

extern "C" int TPL_NODES_ENTRY(const int16_t* rows, const uint8_t* lines, const uint8_t* moves, const uint32_t* entry,
                               const uint8_t* pieces, int64_t n, int64_t n_cfg, int32_t L, int32_t M, const float* weights,
                               float spare_weight, int32_t max_nodes, int32_t shortest, uint8_t* solved, uint8_t* proved,
                               int32_t* solution_len, uint8_t* actions, int32_t* bound, uint32_t* nodes, void* stream) {
    const char* name = TPL_NODES_ENTRY_NAME;
    if (!solved || !proved || !solution_len || !actions || !bound || !nodes)
        return fail_msg(TPL_ERR_ARG, "%s: null pointer (every argument but the stream is required)", name);
    if (const int rc = check_nodes(name, rows, lines, moves, entry, pieces, n, n_cfg, L, M, weights, spare_weight, max_nodes, 1)) return rc;
    if (shortest != 0 && shortest != 1) return fail_msg(TPL_ERR_ARG, "%s: shortest must be 0 or 1", name);
    if ((uintptr_t)solution_len & 3u) return fail_msg(TPL_ERR_ARG, "%s: solution_len must be 4-byte aligned", name);
    if ((uintptr_t)bound & 3u) return fail_msg(TPL_ERR_ARG, "%s: bound must be 4-byte aligned", name);
    if ((uintptr_t)nodes & 3u) return fail_msg(TPL_ERR_ARG, "%s: nodes must be 4-byte aligned", name);
    NodesArgs p{};
    p.in = node_inputs(rows, lines, moves, entry, pieces, n, n_cfg, L, M, weights, spare_weight, max_nodes);
    p.shortest = (uint32_t)shortest;
    p.solved = solved; p.proved = proved; p.solution_len = solution_len; p.actions = actions; p.bound = bound; p.nodes = nodes;
    const size_t stack = sizeof(Frame) * (size_t)p.in.M;       // at most 20,320 bytes
    hipLaunchKernelGGL(TPL_NODES_KERNEL, dim3(p.in.n), dim3(kNodesWave), stack, (hipStream_t)stream, p);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}

extern "C" int TPL_LABELS_ENTRY(const int16_t* rows, const uint8_t* lines, const uint8_t* moves, const uint32_t* entry,
                                const uint8_t* pieces, int64_t n, int64_t n_cfg, int32_t L, int32_t M, const float* weights,
                                float spare_weight, int32_t max_nodes, uint8_t* label, int32_t* length, uint32_t* nodes, void* stream) {
    const char* name = TPL_LABELS_ENTRY_NAME;
    if (!label || !length || !nodes) return fail_msg(TPL_ERR_ARG, "%s: null pointer (every argument but the stream is required)", name);
    if (const int rc = check_nodes(name, rows, lines, moves, entry, pieces, n, n_cfg, L, M, weights, spare_weight, max_nodes, kActions))
        return rc;
    if ((uintptr_t)length & 3u) return fail_msg(TPL_ERR_ARG, "%s: length must be 4-byte aligned", name);
    if ((uintptr_t)nodes & 3u) return fail_msg(TPL_ERR_ARG, "%s: nodes must be 4-byte aligned", name);
    LabelsArgs p{};
    p.in = node_inputs(rows, lines, moves, entry, pieces, n, n_cfg, L, M, weights, spare_weight, max_nodes);
    p.label = label; p.length = length; p.nodes = nodes;
    const size_t stack = sizeof(Frame) * (size_t)p.in.M;       // at most 20,320 bytes
    hipLaunchKernelGGL(TPL_LABELS_KERNEL, dim3(p.in.n * (uint32_t)kActions), dim3(kNodesWave), stack, (hipStream_t)stream, p);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}
