// ntuple_beam.hip -- a beam search over the known piece window with an n-tuple table at the leaves: tpl_ntuple_beam and, with a
// sum table there (ShapeSum of tpl_ntuple.h: ntuple_beam_sum_kernel), tpl_ntuple_beam_sum; with a staged table of any form
// (StagedOf: the three ntuple_staged_beam*_kernel), where every leaf reads the block of its own lines and moves left,
// tpl_ntuple_beam_staged; with a budget table (BudgetTable: ntuple_budget_beam_kernel), and with it the dead-board prune,
// tpl_ntuple_beam_budget (include/tpl_learn.h states the rule).
//
// The frame is placement_beam_kernel's (tpl_beam.h; beam.hip's comment has the reasons): ONE BOARD PER WORKGROUP of 256 threads,
// both beams and the candidate keys in LDS -- 25 KB in all, so six groups share a CU --, and a ply in three phases: A keys every
// candidate slot, B takes the W largest keys in W rounds of a maximum, C writes the kept candidates in candidate order.  Nothing but
// the outputs goes to memory.  What differs is what a candidate is worth:
//   A  a lane that holds a running child gathers the child's table entries as ntuple_sum does -- nine (3 x 3: eight) in flight per
//      trip over the rows, from a table that stays in L2 -- and folds the path's rewards over gamma * V from the leaf inwards:
//      tail = r_j + gamma V, then tail = r_k + gamma tail for k = j - 1 .. 1.  The fold needs every reward of the path, not their
//      sum; only the last move of a path can end the game, so an earlier reward is r_line * rows and a node carries the rows
//      cleared at every ply, three bits a ply, in one word.  (G + gamma^j V, accumulated forwards, is other arithmetic: it breaks the
//      equality with tpl_ntuple_search at two plies.)
//   C  makes a kept candidate's move again for its board, but does NOT gather again: the value is the high word of the key, through
//      the inverse of ordered_bits.  ordered_bits sends -0 to +0's key, so phase A notes a -0 in bit 0 of the key, BELOW the slot --
//      slots are distinct, so the bit never decides an order -- and phase C gives the node the bits phase A computed.
// The prune (the budget geometry alone; tpl_ntuple.h: prune_dead) is made where a child is made, behind expand in phases A and C: a
// child that is left running and dead becomes lost at the limit there, so phase A folds it as a lost node and phase C packs a finished
// node that no later ply expands.  The root's one-ply afterstate is made by first_move and not by expand: it stays the true board.
// After the last ply lane 0 holds the choice and, where `after` is asked for, makes the root's move `action` once more: the one-ply
// afterstate, as ntuple_act_kernel's chosen lane packs it.
#include <cmath>

#include "tpl_beam.h"
#include "tpl_ntuple.h"

namespace tpl_learn {
namespace {

constexpr int kMaxPlies = TPL_NTUPLE_BEAM_MAX_DEPTH;          // one less than the placement beam's: the leaf's piece must be known
static_assert(kMaxPlies == kMaxDepth - 1, "the leaf reads window entry d of the root");
static_assert(3 * (kMaxPlies - 1) <= 32, "the rows of the plies before the last fit one word, three bits a ply");

struct NTupleBeamArgs {
    const uint4* a;              // [n]
    const uint4* b;
    uint32_t n;                  // boards = workgroups
    uint32_t L, M;
    float r_line, r_win, r_lose, gamma;
    const int32_t* table;        // [the shape's entries]
    uint32_t depth, width;       // D in [1, 11], W in [1, 64]
    uint8_t* action;             // [n]
    uint8_t* plan;               // [n][depth], optional
    float* score;                // [n], optional
    uint4* after_a;              // [n], with after_b or not at all: the one-ply afterstate of `action`
    uint4* after_b;
};

// Candidate k of running parent q: `s` becomes the child -- the move made and the window popped, as tpl_afterstates does --, `b` its
// placement; returns the rows the move cleared.  Phases A and C both come here.
__device__ __forceinline__ uint32_t expand(const Beam& parent, uint32_t q, uint32_t k, const tpl::ShapeWord* shape, uint32_t L,
                                           uint32_t M, tpl::Board& s, uint32_t& b) {
    const uint4 A = parent.a[q], B = parent.b[q];
    uint32_t r, l, cur;
    b = nth_placement(B.w & 7u, k, r, l);
    bool running;                                             // the callers expand running parents only (Slot::finished)
    const uint32_t n = first_move(A, B, shape, r, l, L, M, s, cur, running);
    tpl::next_window(s, false, 0);
    return n;
}

// The value of child `s` at ply `ply` (0-based), reached by a move that cleared n rows, behind a path whose earlier moves cleared
// `rows` (three bits a ply): the rule's fold, every product and sum rounded once.
template <typename S>
__device__ __forceinline__ float folded_value(const NTupleBeamArgs& p, const tpl::Board& s, uint32_t n, uint32_t rows, uint32_t ply) {
#pragma clang fp contract(off)
    const bool on = s.state == tpl::ST_RUNNING;
    float v = 0.0f;
    if (on) v = ntuple_value<S>(s, p.L, p.M, p.table);
    const float reward = move_reward(p.r_line, p.r_win, p.r_lose, n, s.state);
    const float later = p.gamma * v;
    float tail = on ? reward + later : reward;
#pragma unroll 1
    for (uint32_t k = ply; k-- > 0u;) {                        // the moves before: each left the game running
        const float before = move_reward(p.r_line, p.r_win, p.r_lose, (rows >> (3u * k)) & 7u, tpl::ST_RUNNING);
        const float rest = p.gamma * tail;
        tail = before + rest;
    }
    return tail;
}

// the float whose ordered_bits is `key` (for the one key that two floats share, +0)
__device__ __forceinline__ float ordered_value(uint32_t key) {
    return __uint_as_float((key & 0x80000000u) ? key ^ 0x80000000u : ~key);
}

template <typename S>
__device__ __forceinline__ void ntuple_beam(const NTupleBeamArgs& p, uint32_t prune = 0u) {
    __shared__ tpl::ShapeWord s_shape[32];
    __shared__ Beam s_beam[2];
    __shared__ unsigned long long s_key[kMaxCandidates];
    __shared__ unsigned long long s_sel[kMaxWidth];
    __shared__ unsigned long long s_wave[2][kBeamBlock / 64];
    __shared__ uint32_t s_best;
    const uint32_t tid = threadIdx.x, i = blockIdx.x;          // the grid is n blocks
    if (tid < 32) s_shape[tid] = tpl::kShapeTable[tid];
    if (tid == 0) {                                            // Beam_0: the root alone
        s_beam[0].a[0] = p.a[i];
        s_beam[0].b[0] = p.b[i];
        s_beam[0].value[0] = 0.0f;                             // a finished board's score
        s_beam[0].cleared[0] = 0u;
#pragma unroll
        for (int k = 0; k < kMaxDepth / 4; ++k) s_beam[0].path[0][k] = 0xFFFFFFFFu;
        s_best = 0u;
    }
    __syncthreads();
    const uint4 rootA = s_beam[0].a[0], rootB = s_beam[0].b[0];
    const unsigned long long window = ((unsigned long long)(rootB.z >> 28) << 32) | rootB.w;
    // the plies: none for a finished board, else as many as leave the leaf's piece a true one
    const uint32_t known = (uint32_t)tpl::kWindowEntries - 1u - tpl::packed_moves(rootA) % (uint32_t)tpl::kWindowStride;
    const uint32_t plies = tpl::packed_state(rootB) != tpl::ST_RUNNING ? 0u : min(p.depth, known);

    uint32_t nodes = 1u;
#pragma unroll 1
    for (uint32_t ply = 0; ply < plies; ++ply) {
        const Beam& parent = s_beam[ply & 1u];
        Beam& child = s_beam[(ply & 1u) ^ 1u];
        const uint32_t cur = (uint32_t)(window >> (3u * ply)) & 7u;
        const uint32_t stride = placement_count(cur);
        const uint32_t total = nodes * stride;                 // at most 64 x 34 slots

        // A: the keys.  Low word: (kSlotTop - slot) << 1 | (the value is -0)
#pragma unroll 1
        for (uint32_t slot = tid; slot < total; slot += kBeamBlock) {
            const Slot c = slot_of(parent, slot, stride);
            const uint32_t low = (kSlotTop - slot) << 1;
            unsigned long long key = 0ull;
            if (c.finished) {
                if (c.k == 0u) key = ((unsigned long long)ordered_bits(parent.value[c.q]) << 32) | low;
            } else {
                tpl::Board s;
                uint32_t b;
                const uint32_t n = expand(parent, c.q, c.k, s_shape, p.L, p.M, s, b);
                prune_dead<S>(s, p.L, p.M, prune);
                const float value = folded_value<S>(p, s, n, parent.cleared[c.q], ply);
                key = ((unsigned long long)ordered_bits(value) << 32) | low | (__float_as_uint(value) == 0x80000000u ? 1u : 0u);
            }
            s_key[slot] = key;
        }
        __syncthreads();

        // B: the min(W, count) largest keys, best first
        const uint32_t kept = select_keys(s_key, s_sel, s_wave, total, p.width, tid);

        // C: the kept candidates, in candidate order
        if (tid < kept) {
            const unsigned long long key = s_sel[tid];
            const uint32_t low = (uint32_t)key;
            const uint32_t place = place_of(s_sel, kept, low);
            const Slot c = slot_of(parent, kSlotTop - (low >> 1), stride);
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
                uint32_t b;
                const uint32_t n = expand(parent, q, c.k, s_shape, p.L, p.M, s, b);
                prune_dead<S>(s, p.L, p.M, prune);
                uint4 A, B;
                tpl::pack_board(s, A, B);
                child.a[place] = A;
                child.b[place] = B;
                child.value[place] = (low & 1u) ? -0.0f : ordered_value((uint32_t)(key >> 32));
                child.cleared[place] = parent.cleared[q] | (n << (3u * ply));     // read by the plies behind this one only
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
        const uint32_t action = plies == 0u ? 0u : last.path[best][0] & 0xFFu;
        p.action[i] = (uint8_t)action;
        if (p.score) p.score[i] = last.value[best];
        if (p.after_a) {                                       // a finished board stays as it is, bit for bit
            uint4 A = rootA, B = rootB;
            if (plies != 0u) {
                tpl::Board s;
                uint32_t cur;
                bool running;
                first_move(rootA, rootB, s_shape, action / 10u, action % 10u, p.L, p.M, s, cur, running);
                tpl::next_window(s, false, 0);
                tpl::pack_board(s, A, B);
                B.y |= rootB.y & 0x80000000u;                  // the spare bit (the slot travels in the Board)
            }
            p.after_a[i] = A;
            p.after_b[i] = B;
        }
    }
    if (p.plan && tid < p.depth) p.plan[(size_t)i * p.depth + tid] = (uint8_t)(last.path[best][tid >> 2] >> (8u * (tid & 3u)));
}

__global__ __launch_bounds__(kBeamBlock) void ntuple_beam_kernel(const NTupleBeamArgs p) { ntuple_beam<Shape2x4>(p); }
__global__ __launch_bounds__(kBeamBlock) void ntuple_beam3_kernel(const NTupleBeamArgs p) { ntuple_beam<Shape3x3>(p); }
__global__ __launch_bounds__(kBeamBlock) void ntuple_beam_sum_kernel(const NTupleBeamArgs p) { ntuple_beam<ShapeSum>(p); }
__global__ __launch_bounds__(kBeamBlock) void ntuple_feature_beam_kernel(const NTupleBeamArgs p) { ntuple_beam<FeatureTable>(p); }
__global__ __launch_bounds__(kBeamBlock) void ntuple_feature3_beam_kernel(const NTupleBeamArgs p) { ntuple_beam<Shape3x3Feature>(p); }
struct BudgetBeamArgs {
    NTupleBeamArgs beam;
    uint32_t prune;              // not 0: the dead-board prune
};
__global__ __launch_bounds__(kBeamBlock) void ntuple_budget_beam_kernel(const BudgetBeamArgs p) { ntuple_beam<BudgetTable>(p.beam, p.prune); }
__global__ __launch_bounds__(kBeamBlock) void ntuple_staged_beam_kernel(const NTupleBeamArgs p) { ntuple_beam<StagedOf<Shape2x4>>(p); }
__global__ __launch_bounds__(kBeamBlock) void ntuple_staged_beam3_kernel(const NTupleBeamArgs p) { ntuple_beam<StagedOf<Shape3x3>>(p); }
// four waves a SIMD: as for ntuple_staged_sum_search_kernel (ntuple.hip), the gathers of a leaf go out nine and eight at a time
// under this budget and one at a time under the default one (1.22 times ntuple_beam_sum_kernel with one stage live; 0.86 so)
__global__ __launch_bounds__(kBeamBlock) __attribute__((amdgpu_waves_per_eu(4, 4))) void ntuple_staged_beam_sum_kernel(const NTupleBeamArgs p) { ntuple_beam<StagedOf<ShapeSum>>(p); }

}  // namespace
}  // namespace tpl_learn

using namespace tpl_learn;

namespace {

// what tpl_ntuple_beam (its shape checked before it comes here), tpl_ntuple_beam_sum and tpl_ntuple_beam_staged (its form checked
// before) share: the checks and the launch
int launch_ntuple_beam(const char* name, const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line,
                       float r_win, float r_lose, float gamma, const int32_t* table, int32_t depth, int32_t width, uint8_t* action,
                       uint8_t* plan, float* score, void* after_a, void* after_b, Form form, void* stream, bool staged = false,
                       int32_t prune = 0) {
    if (const int rc = check_planes(name, plane_a, plane_b, n, L, M)) return rc;
    if (const int rc = check_table(name, table)) return rc;
    if (!action) return fail_msg(TPL_ERR_ARG, "%s: null pointer (action is required)", name);
    if ((after_a == nullptr) != (after_b == nullptr)) return fail_msg(TPL_ERR_ARG, "%s: after_a and after_b go together", name);
    if (((uintptr_t)after_a & 15u) || ((uintptr_t)after_b & 15u))
        return fail_msg(TPL_ERR_ARG, "%s: after_a and after_b must be 16-byte aligned", name);
    if ((uintptr_t)score & 3u) return fail_msg(TPL_ERR_ARG, "%s: score must be 4-byte aligned", name);
    if (!std::isfinite(gamma)) return fail_msg(TPL_ERR_ARG, "%s: gamma must be finite", name);
    if (depth < 1 || depth > kMaxPlies) return fail_msg(TPL_ERR_ARG, "%s: depth must be in [1, %d]", name, kMaxPlies);
    if (width < 1 || width > kMaxWidth) return fail_msg(TPL_ERR_ARG, "%s: width must be in [1, %d]", name, kMaxWidth);
    NTupleBeamArgs p{};
    p.a = (const uint4*)plane_a; p.b = (const uint4*)plane_b; p.n = (uint32_t)n;
    p.L = (uint32_t)L; p.M = (uint32_t)M; p.r_line = r_line; p.r_win = r_win; p.r_lose = r_lose; p.gamma = gamma;
    p.table = table; p.depth = (uint32_t)depth; p.width = (uint32_t)width;
    p.action = action; p.plan = plan; p.score = score; p.after_a = (uint4*)after_a; p.after_b = (uint4*)after_b;
    if (form == Form::kBudget) {
        const BudgetBeamArgs q{p, prune != 0 ? 1u : 0u};
        hipLaunchKernelGGL(ntuple_budget_beam_kernel, dim3(p.n), dim3(kBeamBlock), 0, (hipStream_t)stream, q);
    } else if (form == Form::kFeature || form == Form::k3x3Feature) {
        const auto kernel = form == Form::kFeature ? ntuple_feature_beam_kernel : ntuple_feature3_beam_kernel;
        hipLaunchKernelGGL(kernel, dim3(p.n), dim3(kBeamBlock), 0, (hipStream_t)stream, p);
    } else if (staged) {
        const auto kernel = form == Form::kSum ? ntuple_staged_beam_sum_kernel
                                               : form == Form::k3x3 ? ntuple_staged_beam3_kernel : ntuple_staged_beam_kernel;
        hipLaunchKernelGGL(kernel, dim3(p.n), dim3(kBeamBlock), 0, (hipStream_t)stream, p);
    } else if (form == Form::kSum) hipLaunchKernelGGL(ntuple_beam_sum_kernel, dim3(p.n), dim3(kBeamBlock), 0, (hipStream_t)stream, p);
    else if (form == Form::k3x3) hipLaunchKernelGGL(ntuple_beam3_kernel, dim3(p.n), dim3(kBeamBlock), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(ntuple_beam_kernel, dim3(p.n), dim3(kBeamBlock), 0, (hipStream_t)stream, p);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}

}  // namespace

extern "C" int tpl_ntuple_beam(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line, float r_win,
                               float r_lose, float gamma, const int32_t* table, int32_t depth, int32_t width, uint8_t* action,
                               uint8_t* plan, float* score, void* after_a, void* after_b, int32_t shape, void* stream) {
    if (const int rc = check_shape("tpl_ntuple_beam", shape)) return rc;
    return launch_ntuple_beam("tpl_ntuple_beam", plane_a, plane_b, n, L, M, r_line, r_win, r_lose, gamma, table, depth, width, action,
                              plan, score, after_a, after_b, form_of(shape), stream);
}

extern "C" int tpl_ntuple_beam_sum(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line,
                                   float r_win, float r_lose, float gamma, const int32_t* table, int32_t depth, int32_t width,
                                   uint8_t* action, uint8_t* plan, float* score, void* after_a, void* after_b, void* stream) {
    return launch_ntuple_beam("tpl_ntuple_beam_sum", plane_a, plane_b, n, L, M, r_line, r_win, r_lose, gamma, table, depth, width,
                              action, plan, score, after_a, after_b, Form::kSum, stream);
}

extern "C" int tpl_ntuple_beam_staged(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line,
                                      float r_win, float r_lose, float gamma, const int32_t* table, int32_t depth, int32_t width,
                                      uint8_t* action, uint8_t* plan, float* score, void* after_a, void* after_b, int32_t form,
                                      void* stream) {
    if (const int rc = check_form("tpl_ntuple_beam_staged", form)) return rc;
    return launch_ntuple_beam("tpl_ntuple_beam_staged", plane_a, plane_b, n, L, M, r_line, r_win, r_lose, gamma, table, depth, width,
                              action, plan, score, after_a, after_b, (Form)form, stream, true);
}

extern "C" int tpl_ntuple_beam_feature(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line,
                                       float r_win, float r_lose, float gamma, const int32_t* table, int32_t depth, int32_t width,
                                       uint8_t* action, uint8_t* plan, float* score, void* after_a, void* after_b, int32_t form,
                                       void* stream) {
    if (const int rc = check_feature_form("tpl_ntuple_beam_feature", form)) return rc;
    return launch_ntuple_beam("tpl_ntuple_beam_feature", plane_a, plane_b, n, L, M, r_line, r_win, r_lose, gamma, table, depth, width,
                              action, plan, score, after_a, after_b, feature_form_of(form), stream);
}

extern "C" int tpl_ntuple_beam_budget(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line,
                                      float r_win, float r_lose, float gamma, const int32_t* table, int32_t depth, int32_t width,
                                      uint8_t* action, uint8_t* plan, float* score, void* after_a, void* after_b, int32_t prune,
                                      void* stream) {
    return launch_ntuple_beam("tpl_ntuple_beam_budget", plane_a, plane_b, n, L, M, r_line, r_win, r_lose, gamma, table, depth, width,
                              action, plan, score, after_a, after_b, Form::kBudget, stream, false, prune);
}
