// beam.hip -- a beam search over the known piece window with the linear placement policy's score: tpl_placement_beam
// (include/tpl_learn.h states the rule).
//
// An environment state's window holds the episode's true next pieces, 12 - moves mod 10 of them, so a search from it may go
// that deep.  Exhaustive depth costs 34^D moves; a beam of width W keeps the W best nodes of every ply and costs
// 34 (1 + W (D - 1)).
//
// Mapping: ONE BOARD PER WORKGROUP of 256 threads (four waves).  Both beams (the parents of a ply and its children: packed
// 32-byte boards, rows cleared so far, value, path) and the candidate keys live in LDS, 26 KB in all, so six groups share a
// CU.  All nodes of ply j were popped j times from one root, so they have one current piece and one count S of distinct
// placements (9, 17 or 34): candidate (node q, k-th distinct placement) is slot q S + k, slots in candidate order, and the
// lanes take slots t, t + 256, ...  A ply is three phases:
//   A  every lane moves, scores and keys its slots:  key = ordered_bits(value) << 32 | (4095 - slot)  -- the rule's total order
//      (value descending, candidate index ascending) as one unsigned maximum, every key distinct and none zero.  A finished
//      parent's slot 0 carries its own value; its other slots hold 0, below every key.
//   B  selection: W rounds of a maximum, each taking the largest key not yet taken into sel[round]; after min(W, count) rounds
//      sel[] holds the kept keys, best first.  Every lane caches the largest of its own slots and every wave the largest of
//      its lanes (a shuffle reduction) in one LDS word; a round reads the four words, and only the wave whose key was taken --
//      the keys are distinct, so it is one wave and one lane of it -- rescans its slots (one lane, up to nine LDS reads) and
//      reduces again (six shuffle steps on 64 bits).  So a round is four broadcast reads and a barrier for three waves and that
//      rescan and reduction for the fourth; no round is a pass of all lanes over the keys.  (The same rounds with an LDS
//      atomicMax from every lane measured ten times the two-ply kernel at D = 2, W = 34 on an MI355X, where both make the same
//      moves: 256 atomics on one address a round.  Counting every key against every other is count^2; a radix select is six
//      passes of histogram atomics that all land in the few bins of the common exponent.)
//   C  compaction in candidate order: lane e < kept owns sel[e]; its place in the new beam is the number of kept keys with a
//      lower slot (at most 64 broadcast reads of the low words), it makes its move AGAIN (so no board but the parents' is
//      kept for the 2,176 candidates), pops the window, packs the child and writes it there.  Lane 0 owns sel[0], the best.
// After the last ply lane 0's node is the choice.  Nothing but the outputs goes to memory.
// The frame -- the beam in LDS, slot decoding, phase B and the place of phase C -- is tpl_beam.h's, shared with the n-tuple beam
// (ntuple_beam.hip); phase A's value and what a kept candidate stores are this kernel's.
//
// This unit is built twice (tpl_placement.h: kUnitFeatures): as it stands, placement_beam_kernel on the twelve board features, and
// through beam_move.hip as placement_beam_move_kernel on the fourteen with landing height and eroded cells.  There a node's `cleared`
// word is the carry of its path (tpl_placement.h): rows cleared, landing sum and eroded sum in 8 + 14 + 10 bits -- the beam in LDS is
// the same size.
//
// And twice more in the BOUNDED form (tpl_placement.h: kUnitBound; include/tpl_learn.h: the move bound), through beam_bound.hip and
// beam_move_bound.hip: placement_beam_bound_kernel and placement_beam_move_bound_kernel.  expand() then turns a dead child into a lost one
// and adds the spare term (bounded_move, bounded_value); nothing else differs, and the two unbounded kernels are what they were,
// instruction for instruction (profiles/learner/bound_isa.log).
#include "tpl_beam.h"

namespace tpl_learn {
namespace {

constexpr int kF = kUnitFeatures;

struct BeamArgs {
    const uint4* a;              // [n]
    const uint4* b;
    uint32_t n;                  // boards = workgroups
    uint32_t L, M;
    const float* weights;        // [P][12] or, at 14 features, [P][16]; P = ceil(n / per_member)
    uint32_t per_member;         // boards per weight row, in [1, n]
    uint32_t depth, width;       // D in [1, 12], W in [1, 64]
    uint8_t* action;             // [n]
    uint8_t* plan;               // [n][depth], optional
    float* score;                // [n], optional
#ifdef TPL_PLACEMENT_BOUND_UNIT
    float spare_weight;          // the bounded form's: the weight of a node's spare cells, one for the whole launch
#endif
};

__device__ __forceinline__ float spare_weight_of(const BeamArgs& p) {
#ifdef TPL_PLACEMENT_BOUND_UNIT
    return p.spare_weight;
#else
    return 0.0f;
#endif
}

// Candidate k of running parent q: the board the move leaves (window not yet popped), the move's carry with the parent's (the rows
// cleared at 12 features), and the value of psi = (cleared, won, lost, features 3..11[, landing sum, eroded sum]).  Phases A and C both come here, so a winner's second making of its
// move gives the bits of the first.  In the bounded form a dead child is lost before psi is made, and its spare cells enter the value
// last (tpl_placement.h: bounded_move).
__device__ __forceinline__ float expand(const Beam& parent, uint32_t q, uint32_t k, const tpl::ShapeWord* shape, uint32_t L,
                                        uint32_t M, const float (&w)[kF], float spare_weight, tpl::Board& s, uint32_t& cleared,
                                        uint32_t& b) {
    const uint4 A = parent.a[q], B = parent.b[q];
    uint32_t r, l, cur;
    b = nth_placement(B.w & 7u, k, r, l);
    bool running;                                             // the callers expand running parents only (Slot::finished)
    cleared = parent.cleared[q] + first_move<kF>(A, B, shape, r, l, L, M, s, cur, running);
    const int32_t spare = bounded_move(s, L, M);
    FeatureSet<kF> psi;
    moved_features(s, cleared, true, psi);
    if constexpr (kUnitBound) return bounded_value(placement_score(w, psi), spare_weight, spare);
    else return placement_score(w, psi);
}

// The 12-feature kernel takes 95 VGPRs by itself: five workgroups a CU.  Left to itself the 14-feature one takes more than 128, which
// is three; bound to the 96 of five it spills 20 bytes to scratch, so it is bound to four (tools/kernel_resources.sh).  The bounded
// forms carry the fill planes of move_bound_cells: left to itself the bounded 12-feature kernel takes 133, so both are bound to four.
#if defined(TPL_PLACEMENT_MOVE_UNIT) || defined(TPL_PLACEMENT_BOUND_UNIT)
#define TPL_BEAM_BOUNDS __launch_bounds__(kBeamBlock, 4)
#else
#define TPL_BEAM_BOUNDS __launch_bounds__(kBeamBlock)
#endif
__global__ TPL_BEAM_BOUNDS void TPL_UNIT_KERNEL(placement_beam)(const BeamArgs p) {
    constexpr int kStride = weight_stride<kF>();
    __shared__ tpl::ShapeWord s_shape[32];
    __shared__ __attribute__((aligned(16))) float s_w[kStride];
    __shared__ Beam s_beam[2];
    __shared__ unsigned long long s_key[kMaxCandidates];
    __shared__ unsigned long long s_sel[kMaxWidth];
    __shared__ unsigned long long s_wave[2][kBeamBlock / 64];
    __shared__ uint32_t s_best;
    const uint32_t tid = threadIdx.x, i = blockIdx.x;          // the grid is n blocks
    if (tid < 32) s_shape[tid] = tpl::kShapeTable[tid];
    if (tid < kFeatures / 4) ((float4*)s_w)[tid] = ((const float4*)(p.weights + (size_t)(i / p.per_member) * kStride))[tid];
    if constexpr (kF == kMoveFeatures) {                       // entries 14 and 15 are not read
        if (tid == kFeatures / 4) ((float2*)s_w)[6] = ((const float2*)(p.weights + (size_t)(i / p.per_member) * kStride))[6];
    }
    if (tid == 0) {                                            // Beam_0: the root alone
        s_beam[0].a[0] = p.a[i];
        s_beam[0].b[0] = p.b[i];
        s_beam[0].value[0] = 0.0f;
        s_beam[0].cleared[0] = 0u;
#pragma unroll
        for (int k = 0; k < kMaxDepth / 4; ++k) s_beam[0].path[0][k] = 0xFFFFFFFFu;
        s_best = 0u;
    }
    __syncthreads();
    float w[kF];
#pragma unroll
    for (int q = 0; q < kFeatures / 4; ++q) {
        const float4 v = ((const float4*)s_w)[q];
        w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
    }
    if constexpr (kF == kMoveFeatures) {
        const float2 v = ((const float2*)s_w)[6];
        w[kF - 2] = v.x; w[kF - 1] = v.y;
    }
    const float spare_weight = spare_weight_of(p);
    const uint4 rootA = s_beam[0].a[0], rootB = s_beam[0].b[0];
    const unsigned long long window = ((unsigned long long)(rootB.z >> 28) << 32) | rootB.w;
    // the plies: none for a finished board, else as many as the window has true pieces
    const uint32_t known = (uint32_t)tpl::kWindowEntries - tpl::packed_moves(rootA) % (uint32_t)tpl::kWindowStride;
    const uint32_t plies = tpl::packed_state(rootB) != tpl::ST_RUNNING ? 0u : min(p.depth, known);
    if (plies == 0u) {
        FeatureSet<kF> zero;
#pragma unroll
        for (int k = 0; k < kF; ++k) zero.f[k] = 0u;
        if (tid == 0) s_beam[0].value[0] = placement_score(w, zero);
        __syncthreads();
    }

    uint32_t nodes = 1u;
#pragma unroll 1
    for (uint32_t ply = 0; ply < plies; ++ply) {
        const Beam& parent = s_beam[ply & 1u];
        Beam& child = s_beam[(ply & 1u) ^ 1u];
        const uint32_t cur = (uint32_t)(window >> (3u * ply)) & 7u;
        const uint32_t stride = placement_count(cur);
        const uint32_t total = nodes * stride;                 // at most 64 x 34 slots

        // A: the keys
#pragma unroll 1
        for (uint32_t slot = tid; slot < total; slot += kBeamBlock) {
            const Slot c = slot_of(parent, slot, stride);
            unsigned long long key = 0ull;
            if (c.finished) {
                if (c.k == 0u) key = ((unsigned long long)ordered_bits(parent.value[c.q]) << 32) | (kSlotTop - slot);
            } else {
                tpl::Board s;
                uint32_t cleared, b;
                const float value = expand(parent, c.q, c.k, s_shape, p.L, p.M, w, spare_weight, s, cleared, b);
                key = ((unsigned long long)ordered_bits(value) << 32) | (kSlotTop - slot);
            }
            s_key[slot] = key;
        }
        __syncthreads();

        // B: the min(W, count) largest keys, best first
        const uint32_t kept = select_keys(s_key, s_sel, s_wave, total, p.width, tid);

        // C: the kept candidates, in candidate order
        if (tid < kept) {
            const uint32_t low = (uint32_t)s_sel[tid];
            const uint32_t place = place_of(s_sel, kept, low);
            const Slot c = slot_of(parent, kSlotTop - low, stride);
            const uint32_t q = c.q;
            uint32_t path[kMaxDepth / 4];
#pragma unroll
            for (int j = 0; j < kMaxDepth / 4; ++j) path[j] = parent.path[q][j];
            if (c.finished) {
                child.a[place] = parent.a[q];
                child.b[place] = parent.b[q];
                child.value[place] = parent.value[q];
                child.cleared[place] = parent.cleared[q];
            } else {
                tpl::Board s;
                uint32_t cleared, b;
                const float value = expand(parent, q, c.k, s_shape, p.L, p.M, w, spare_weight, s, cleared, b);
                tpl::next_window(s, false, 0);                 // tpl_afterstates' pop
                uint4 A, B;
                tpl::pack_board(s, A, B);
                child.a[place] = A;
                child.b[place] = B;
                child.value[place] = value;
                child.cleared[place] = cleared;
                path_append(path, ply, b);
            }
#pragma unroll
            for (int j = 0; j < kMaxDepth / 4; ++j) child.path[place][j] = path[j];
            if (tid == 0) s_best = place;
        }
        __syncthreads();
        nodes = kept;
    }

    // the choice: the best node of the last beam
    const Beam& last = s_beam[plies & 1u];
    const uint32_t best = s_best;
    if (tid == 0) {
        p.action[i] = plies == 0u ? (uint8_t)0 : (uint8_t)(last.path[best][0] & 0xFFu);
        if (p.score) p.score[i] = last.value[best];
    }
    if (p.plan && tid < p.depth) p.plan[(size_t)i * p.depth + tid] = (uint8_t)(last.path[best][tid >> 2] >> (8u * (tid & 3u)));
}

}  // namespace
}  // namespace tpl_learn

using namespace tpl_learn;

// the bounded entries take spare_weight behind the width (include/tpl_learn.h)
#ifdef TPL_PLACEMENT_BOUND_UNIT
#define TPL_BEAM_SPARE_PARAM float spare_weight,
#else
#define TPL_BEAM_SPARE_PARAM
#endif

extern "C" int TPL_UNIT_ENTRY(tpl_placement_beam)(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const float* weights,
                                  int64_t boards_per_member, int32_t depth, int32_t width, TPL_BEAM_SPARE_PARAM uint8_t* action,
                                  uint8_t* plan, float* score, void* stream) {
    const char* name = TPL_UNIT_ENTRY_NAME(tpl_placement_beam);
    if (const int rc = check_policy(name, plane_a, plane_b, n, L, M, weights, boards_per_member, action, score)) return rc;
    if (depth < 1 || depth > kMaxDepth) return fail_msg(TPL_ERR_ARG, "%s: depth must be in [1, %d]", name, kMaxDepth);
    if (width < 1 || width > kMaxWidth) return fail_msg(TPL_ERR_ARG, "%s: width must be in [1, %d]", name, kMaxWidth);
    BeamArgs p{};
    p.a = (const uint4*)plane_a; p.b = (const uint4*)plane_b; p.n = (uint32_t)n;
    p.L = (uint32_t)L; p.M = (uint32_t)M; p.weights = weights;
    p.per_member = (uint32_t)(boards_per_member < n ? boards_per_member : n);     // anything above n is the single-policy case
    p.depth = (uint32_t)depth; p.width = (uint32_t)width;
    p.action = action; p.plan = plan; p.score = score;
#ifdef TPL_PLACEMENT_BOUND_UNIT
    if (!(spare_weight - spare_weight == 0.0f)) return fail_msg(TPL_ERR_ARG, "%s: spare_weight must be finite", name);
    p.spare_weight = spare_weight;
#endif
    hipLaunchKernelGGL(TPL_UNIT_KERNEL(placement_beam), dim3(p.n), dim3(kBeamBlock), 0, (hipStream_t)stream, p);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}
