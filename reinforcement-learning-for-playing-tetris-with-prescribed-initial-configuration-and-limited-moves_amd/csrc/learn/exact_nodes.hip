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
// The search, its mapping and its stack are tpl_exact.h's, and the order is exact.hip's linear one.  ONE NODE PER WAVEFRONT; the stack is
// dynamic LDS at 80 bytes a depth, indexed by the depth FROM THE NODE and sized by the launch's M, which no shifted game exceeds.
//   placement_exact_nodes_kernel    a wave a node: the search, and the six outputs of tpl_placement_exact counted from the node.
//   placement_exact_labels_kernel   a wave a (node, placement b): the one move b of the node's piece, made as the search makes a child,
//                                   then the verdict of the move -- at once where the child is finished, and by the same search from
//                                   the child, one more shift, where it runs.
// A node whose lines, moves or entry are out of range is finished: its outputs are written and nothing else is read.
//
// Built twice, as exact.hip is: as it stands on the twelve board features and through exact_nodes_move.hip on the fourteen.
#ifndef TPL_PLACEMENT_BOUND_UNIT
#define TPL_PLACEMENT_BOUND_UNIT
#endif
#include "tpl_beam.h"
#include "tpl_exact.h"

namespace tpl_learn {
namespace {

constexpr int kF = kUnitFeatures;

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

using Order = LinearOrder<kF>;
using Stack = Frame<Order::Carry>;

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

// one wave a workgroup, bound to eight waves a SIMD (tpl_exact.h says why)
__global__ __launch_bounds__(kExactWave, 8) void TPL_NODES_KERNEL(const NodesArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    Stack* const stack = reinterpret_cast<Stack*>(s_raw);      // [M]
    __shared__ tpl::ShapeWord s_shape[32];
    __shared__ uint8_t s_pieces[kExactMaxMoves + 2];
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
        for (uint32_t t = lane; t < M; t += kExactWave) p.actions[(size_t)i * M + t] = (uint8_t)kNoMove;
        return;
    }
    if (lane < 32) s_shape[lane] = tpl::kShapeTable[lane];

    tpl::Board root;                                           // the node as the root of its shifted game: the same in every lane
    tpl::rows_to_cols(p.in.rows + (size_t)i * tpl::kRows, root.c);
    fresh_root(root);

    const Order order(p.in.weights, p.in.spare_weight);
    load_pieces(s_pieces, p.in.pieces, at.first, at.M, lane);
    const uint32_t bound = need_of(root, at.L);
    const Found f = search(order, stack, s_pieces, s_shape, root, bound, at.L, at.M, p.in.max_nodes, p.shortest, lane);
    if (lane == 0) {
        p.solved[i] = f.length != 0u ? (uint8_t)1 : (uint8_t)0;
        p.proved[i] = f.capped ? (uint8_t)0 : (uint8_t)1;
        p.solution_len[i] = (int32_t)f.length;
        p.bound[i] = (int32_t)bound;
        p.nodes[i] = f.nodes;
    }
    write_path(stack, f, p.actions + (size_t)i * M, M, lane);      // the solution from the node; 255 up to the launch's M
}

// One wave a (node, action): block 40 i + b.  The move is made by every lane alike, so the child is a value of the wave; its verdict
// is read through `uniform`, and the branch on it is scalar.
__global__ __launch_bounds__(kExactWave, 8) void TPL_LABELS_KERNEL(const LabelsArgs p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
    Stack* const stack = reinterpret_cast<Stack*>(s_raw);      // [M]
    __shared__ tpl::ShapeWord s_shape[32];
    __shared__ uint8_t s_pieces[kExactMaxMoves + 2];
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
                const Order order(p.in.weights, p.in.spare_weight);
                load_pieces(s_pieces, p.in.pieces, at.first + 1u, child_M, lane);
                const Found f = search(order, stack, s_pieces, s_shape, root, need_of(root, child_L), child_L, child_M, p.in.max_nodes, 1u,
                                       lane);
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
    char each[80];
    snprintf(each, sizeof(each), "%d workgroup(s) per node: their number must stay below 2^31", (int)waves_per_node);
    if (const int rc = check_search(name, n, waves_per_node, each, n_cfg, L, M, max_nodes)) return rc;
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
    if (const int rc = check_counts(name, solution_len, bound, nodes)) return rc;
    NodesArgs p{};
    p.in = node_inputs(rows, lines, moves, entry, pieces, n, n_cfg, L, M, weights, spare_weight, max_nodes);
    p.shortest = (uint32_t)shortest;
    p.solved = solved; p.proved = proved; p.solution_len = solution_len; p.actions = actions; p.bound = bound; p.nodes = nodes;
    const size_t stack = sizeof(Stack) * (size_t)p.in.M;       // at most 20,320 bytes
    hipLaunchKernelGGL(TPL_NODES_KERNEL, dim3(p.in.n), dim3(kExactWave), stack, (hipStream_t)stream, p);
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
    const size_t stack = sizeof(Stack) * (size_t)p.in.M;       // at most 20,320 bytes
    hipLaunchKernelGGL(TPL_LABELS_KERNEL, dim3(p.in.n * (uint32_t)kActions), dim3(kExactWave), stack, (hipStream_t)stream, p);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}
