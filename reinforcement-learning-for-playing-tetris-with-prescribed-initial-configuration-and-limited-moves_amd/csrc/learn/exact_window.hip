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
// Mapping: exact_nodes.hip's frame.  ONE BOARD PER WAVEFRONT, one wavefront a workgroup, no barrier; lanes 0 .. 33 a child each, 64-bit
// keys ranked across the wave, the stack in LDS at 80 bytes a depth.  No path is longer than the twelve window entries, so the stack
// is twelve records, 960 bytes of STATIC LDS, beside the twelve pieces of the window, a byte each.  The wave unpacks its board from
// the two packed planes the beam kernels take.
//
// The search loop is exact_nodes.hip's, duplicated: that unit and exact.hip stay as they are, with their instructions
// (profiles/learner/exact_window_isa.log).  Built twice, as they are: as it stands on the twelve board features and through
// exact_window_move.hip on the fourteen.
#ifndef TPL_PLACEMENT_BOUND_UNIT
#define TPL_PLACEMENT_BOUND_UNIT
#endif
#include "tpl_beam.h"

namespace tpl_learn {
namespace {

constexpr int kF = kUnitFeatures;
constexpr int kWindowWave = 64;
constexpr int kWindowDepth = tpl::kWindowEntries;             // 12: the longest horizon, and the plan's width
constexpr int kWindowMaxNodes = TPL_EXACT_MAX_NODES;
static_assert(kUnitBound, "the exact search is a unit of the bounded form");
static_assert(kMaxPlacements <= kWindowWave, "a lane per child");
static_assert(kWindowDepth == TPL_WINDOW_PLAN, "the plan is as wide as the window");

#define TPL_WINDOW_KERNEL TPL_UNIT_PASTE4(placement_window_prove, TPL_UNIT_FORM, , _kernel)
#define TPL_WINDOW_ENTRY TPL_UNIT_PASTE4(tpl_placement_window_prove, TPL_UNIT_FORM, , )
#define TPL_WINDOW_ENTRY_NAME "tpl_placement_window_prove" TPL_UNIT_FORM_NAME

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

struct Found {
    uint32_t nodes, length, last;                              // expansions; the winning length, 0 if none, and its last move
    bool capped;
};

// exact_nodes.hip's search, shortest, of the game (L, H), H <= 12, from `root` -- the same in every lane, 0 lines, 0 moves, carry 0 --
// whose piece at depth d is s_pieces[d]; `need` is need(root), and need > H is decided without a node.  The caller has filled
// s_shape and s_pieces.  On return the path of a win is in the stack: the child in hand at every depth, then `last`.
__device__ __forceinline__ Found search(Frame* stack, const uint8_t* s_pieces, const tpl::ShapeWord* s_shape, const tpl::Board& root,
                                        uint32_t need, uint32_t L, uint32_t H, const float (&w)[kF], float spare_weight,
                                        uint32_t max_nodes, uint32_t lane) {
    uint32_t nodes = 0u, length = 0u, last = kNoMove;
    bool capped = false;
#pragma unroll 1
    for (uint32_t B = need; B <= H && length == 0u && !capped; ++B) {
        wave_sync();                                           // the last iteration's reads of record 0 (and, the first time, the tables)
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
                if (rank == 0u && d + 1u < H) store_frame(stack[d + 1u], s, carry);      // descended into at once (d + 1 < B <= H <= 12)
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
                    if (lane == 0 && d + 1u < H) {
                        stack[d].cursor = at + 1u;
                        store_frame(stack[d + 1u], s2, carry2);
                    }
                    wave_sync();
                    ++d;
                    more = true;
                    break;
                }
            }
            if (!more) break;                                  // the root's children are used up: no win at this budget
        }
    }
    wave_sync();
    Found out;
    out.nodes = nodes;
    out.length = capped ? 0u : length;
    out.last = last;
    out.capped = capped;
    return out;
}

// One wave a workgroup, bound to eight waves a SIMD as exact_nodes.hip's kernels are and for their reason: a wave's search is one
// dependent chain, and what hides its latency is other waves (tools/kernel_resources.sh; profiles/learner/exact_window_isa.log).
__global__ __launch_bounds__(kWindowWave, 8) void TPL_WINDOW_KERNEL(const WindowArgs p) {
    __shared__ Frame stack[kWindowDepth];
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
    root.window = 0u; root.window_hi = 0u;
    root.state = tpl::ST_RUNNING; root.lines = 0u; root.moves = 0u; root.slot = 0u;
    const uint32_t need = live ? (move_bound_cells(root.c, L) + 3u) >> 2 : 0u;      // need(board): no win is shorter

    const bool last_known = H == rem;                          // the window reaches the end of the game
    if (lane == 0) {                                           // what the search does not decide, before it
        p.bound[i] = (int32_t)need;
        p.horizon[i] = (uint8_t)H;
    }

    Found f;
    f.nodes = 0u; f.length = 0u; f.last = kNoMove; f.capped = false;
    if (live && !skipped) {
        if (lane < 32) s_shape[lane] = tpl::kShapeTable[lane];
        // window entry `lane`, masked as move_board masks it
        const unsigned long long window = ((unsigned long long)at.window_hi << 32) | at.window;
        if (lane < (uint32_t)kWindowDepth) s_pieces[lane] = (uint8_t)((uint32_t)(window >> (3u * lane)) & 7u);
        float w[kF];                                           // one row for the whole grid: scalar loads, the weights stay in SGPRs
#pragma unroll
        for (int q = 0; q < kF; ++q) w[q] = p.weights[q];
        f = search(stack, s_pieces, s_shape, root, need, L, H, w, p.spare_weight, p.max_nodes, lane);
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
    }
    // the plan: the child in hand at every depth of the path, then the won one; 255 behind the end
    if (lane < (uint32_t)kWindowDepth) {
        uint32_t a = kNoMove;
        if (lane + 1u < f.length) a = stack[lane].kids[stack[lane].cursor - 1u];
        else if (lane + 1u == f.length) a = f.last;
        p.plan[(size_t)i * kWindowDepth + lane] = (uint8_t)a;
    }
}

}  // namespace
}  // namespace tpl_learn

using namespace tpl_learn;

extern "C" int TPL_WINDOW_ENTRY(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const float* weights,
                                float spare_weight, int32_t max_nodes, const uint8_t* skip, uint8_t* solved, uint8_t* proved,
                                int32_t* solution_len, uint8_t* plan, int32_t* bound, uint32_t* nodes, uint8_t* horizon,
                                uint8_t* verdict, void* stream) {
    const char* name = TPL_WINDOW_ENTRY_NAME;
    if (!plane_a || !plane_b || !weights || !solved || !proved || !solution_len || !plan || !bound || !nodes || !horizon || !verdict)
        return fail_msg(TPL_ERR_ARG, "%s: null pointer (every argument but skip and the stream is required)", name);
    if (!(spare_weight - spare_weight == 0.0f)) return fail_msg(TPL_ERR_ARG, "%s: spare_weight must be finite", name);
    if (n < 1) return fail_msg(TPL_ERR_ARG, "%s: n must be positive", name);
    if (n >= ((int64_t)1 << 31)) return fail_msg(TPL_ERR_ARG, "%s: n too large (a workgroup per board: n must stay below 2^31)", name);
    if (L < 1 || L > 250 || M < 1 || M > 254) return fail_msg(TPL_ERR_ARG, "%s: L and M must be in [1, 250] and [1, 254]", name);
    if (max_nodes < 1 || max_nodes > kWindowMaxNodes)
        return fail_msg(TPL_ERR_ARG, "%s: max_nodes must be in [1, %d]", name, kWindowMaxNodes);
    if (((uintptr_t)plane_a & 15u) || ((uintptr_t)plane_b & 15u))
        return fail_msg(TPL_ERR_ARG, "%s: planes must be 16-byte aligned", name);
    if ((uintptr_t)weights & 15u) return fail_msg(TPL_ERR_ARG, "%s: weights must be 16-byte aligned", name);
    if ((uintptr_t)solution_len & 3u) return fail_msg(TPL_ERR_ARG, "%s: solution_len must be 4-byte aligned", name);
    if ((uintptr_t)bound & 3u) return fail_msg(TPL_ERR_ARG, "%s: bound must be 4-byte aligned", name);
    if ((uintptr_t)nodes & 3u) return fail_msg(TPL_ERR_ARG, "%s: nodes must be 4-byte aligned", name);
    WindowArgs p{};
    p.a = (const uint4*)plane_a; p.b = (const uint4*)plane_b; p.n = (uint32_t)n;
    p.L = (uint32_t)L; p.M = (uint32_t)M; p.weights = weights; p.spare_weight = spare_weight; p.max_nodes = (uint32_t)max_nodes;
    p.skip = skip;
    p.solved = solved; p.proved = proved; p.solution_len = solution_len; p.plan = plan; p.bound = bound; p.nodes = nodes;
    p.horizon = horizon; p.verdict = verdict;
    hipLaunchKernelGGL(TPL_WINDOW_KERNEL, dim3(p.n), dim3(kWindowWave), 0, (hipStream_t)stream, p);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}
