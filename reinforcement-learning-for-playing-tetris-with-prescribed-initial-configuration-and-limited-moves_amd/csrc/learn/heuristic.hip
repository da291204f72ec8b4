// heuristic.hip -- board features of every placement and a linear placement policy on them, one ply or two: tpl_placement_features,
// tpl_placement_act, tpl_placement_search (include/tpl_learn.h states the rules).
//
// The classical Tetris controller scores the board a placement leaves by a linear function of a few hand-made features and
// plays the best one.  In the column layout every such feature is a few ctz / popcount / xor operations on the ten column
// words that move_board leaves in registers, so features, score and arg-max are one kernel: 32 B read per board, one byte
// (five with the best score) written, nothing in between goes to memory.
//
// Lane mapping: one lane per (board, action) PAIR, as afterstates.hip, in blocks of 320 threads = 8 boards x 40 actions (five
// waves), so no board straddles a block and a board's arg-max is one LDS word.  The arg-max is a 64-bit LDS atomic maximum per
// board on  key = order-preserving image of the float32 score << 32 | (39 - a) : the largest score wins, among equal scores
// the lowest action; alias lanes (a != canonical[a]) do not take part.  The lane whose key comes back writes the board's
// outputs.  A maximum is order independent, so the result is deterministic.  Thread t < 8 of a block fetches the weight row of
// the block's board t into LDS (the one division by boards_per_member happens there, in eight lanes of 320); the pair lanes
// read their board's row back with three 16-byte LDS reads, the 40 lanes of a board from one address.
// The other mapping -- a lane per board looping over the 40 actions -- unpacks once per board and has no cross-lane step, but
// the move and the features, which are nine tenths of a pair's instructions, are per pair either way; it diverges on
// nrot(cur), and has a fortieth of the lanes (DESIGN.md section 9 has the instruction counts).
//
// That frame -- block prologue, lane decode, first move, arg-max and the winner's stores -- is written once, in
// placement_policy<kPlies>; placement_act_kernel and placement_search_kernel are its two instances.  What a lane's first move
// is worth is the one thing that differs: its own score at one ply, the best second placement's (best_second) at two.
//
// This unit is built twice (tpl_placement.h: kUnitFeatures): as it stands on the twelve board features, and through heuristic_move.hip
// on the fourteen that add landing height and eroded cells -- placement_features_move_kernel, placement_act_move_kernel,
// placement_search_move_kernel and the tpl_placement_*_move entries.  What differs is the carry of a move (placed_move), the width of
// a weight row and of a feature record.
#include "tpl_placement.h"

namespace tpl_learn {
namespace {

constexpr int kF = kUnitFeatures;
constexpr int kBoardsPerBlock = 8;
constexpr int kActBlock = kBoardsPerBlock * kActions;        // 320 threads: five waves, eight whole boards
constexpr int kFeatureBlock = 256;
static_assert(kActBlock % 64 == 0, "a block is whole waves");

struct FeatureArgs {
    const uint4* a;              // [n]
    const uint4* b;
    uint32_t total;              // 40 n, below 2^31
    uint32_t L, M;
    void* features;              // [n][40] records: 24 bytes = three 8-byte words at 12 features, 32 bytes = two 16-byte words at 14
    uint8_t* canonical;          // [n][40], optional
};

// phi(s, a) of every pair: the kF features of what action a = 10 r + l leaves of state i; all zero for a finished board
__global__ __launch_bounds__(kFeatureBlock) void TPL_UNIT_KERNEL(placement_features)(const FeatureArgs p) {
    __shared__ tpl::ShapeWord s_shape[32];
    if (threadIdx.x < 32) s_shape[threadIdx.x] = tpl::kShapeTable[threadIdx.x];
    __syncthreads();
    const uint32_t j = blockIdx.x * kFeatureBlock + threadIdx.x;        // pair 40 i + a
    if (j >= p.total) return;
    const uint32_t i = j / kActions, a = j - i * kActions;
    const uint32_t r = a / 10u, l = a - r * 10u;
    tpl::Board s;
    uint32_t cur;
    bool running;
    const uint32_t n_clear = first_move<kF>(p.a[i], p.b[i], s_shape, r, l, p.L, p.M, s, cur, running);
    FeatureSet<kF> phi;
    moved_features(s, n_clear, running, phi);
    if constexpr (kF == kMoveFeatures) {
        uint4* rec = (uint4*)p.features + 2u * (size_t)j;
        rec[0] = make_uint4(phi.f[0] | (phi.f[1] << 16), phi.f[2] | (phi.f[3] << 16), phi.f[4] | (phi.f[5] << 16),
                            phi.f[6] | (phi.f[7] << 16));
        rec[1] = make_uint4(phi.f[8] | (phi.f[9] << 16), phi.f[10] | (phi.f[11] << 16), phi.f[kF - 2] | (phi.f[kF - 1] << 16), 0u);
    } else {
        uint2* rec = (uint2*)p.features + 3u * (size_t)j;
        rec[0] = make_uint2(phi.f[0] | (phi.f[1] << 16), phi.f[2] | (phi.f[3] << 16));
        rec[1] = make_uint2(phi.f[4] | (phi.f[5] << 16), phi.f[6] | (phi.f[7] << 16));
        rec[2] = make_uint2(phi.f[8] | (phi.f[9] << 16), phi.f[10] | (phi.f[11] << 16));
    }
    if (p.canonical) p.canonical[j] = (uint8_t)canonical_action(cur, r, l);
}

struct PolicyArgs {
    const uint4* a;              // [n]
    const uint4* b;
    uint32_t n;                  // boards; 40 n below 2^31
    uint32_t L, M;
    const float* weights;        // [P][12] or, at 14 features, [P][16]; P = ceil(n / per_member)
    uint32_t per_member;         // boards per weight row, in [1, n]
    uint8_t* action;             // [n]
    uint8_t* second;             // [n], optional; null at one ply
    float* score;                // [n], optional
};

// The policy of kPlies plies on the block's eight boards (the header comment has the frame).  A lane's value is the score of
// what its first move leaves; at two plies, where that move leaves the game running, it is best_second's instead.  Alias lanes
// and lanes whose first move ended the game (or whose board is finished: all-zero features) keep the one-ply score.
template <int kPlies>
__device__ __forceinline__ void placement_policy(const PolicyArgs& p) {
    __shared__ tpl::ShapeWord s_shape[32];
    constexpr int kStride = weight_stride<kF>();
    __shared__ __attribute__((aligned(16))) float s_w[kBoardsPerBlock][kStride];
    __shared__ unsigned long long s_best[kBoardsPerBlock];
    const uint32_t first = blockIdx.x * kBoardsPerBlock;                // the block's boards: first .. first + 7
    if (threadIdx.x < 32) s_shape[threadIdx.x] = tpl::kShapeTable[threadIdx.x];
    if (threadIdx.x < kBoardsPerBlock) {
        s_best[threadIdx.x] = 0ull;                                     // below every key: a key's high word has a bit set
        const uint32_t board = min(first + threadIdx.x, p.n - 1u);
        const float4* row = (const float4*)(p.weights + (size_t)(board / p.per_member) * kStride);
        float4* dst = (float4*)s_w[threadIdx.x];
        dst[0] = row[0]; dst[1] = row[1]; dst[2] = row[2];
        if constexpr (kF == kMoveFeatures) ((float2*)dst)[6] = ((const float2*)row)[6];       // entries 14 and 15 are not read
    }
    __syncthreads();
    const uint32_t slot = threadIdx.x / kActions, a = threadIdx.x - slot * kActions;
    const uint32_t r = a / 10u, l = a - r * 10u;
    const uint32_t i = first + slot;
    const bool valid = i < p.n;                                         // whole boards: all 40 lanes of a board agree
    const uint32_t src = valid ? i : p.n - 1u;                          // past the end: the last board again, never written

    tpl::Board s1;
    uint32_t cur;
    bool running;
    const uint32_t n1 = first_move<kF>(p.a[src], p.b[src], s_shape, r, l, p.L, p.M, s1, cur, running);
    const bool contends = valid && canonical_action(cur, r, l) == a;
    // the weight row, read back here and not ahead of the first move: there both kernels measured 2 % slower on an MI355X
    // at the same instruction counts (profiles/learner/README.md)
    float w[kF];
    const float4* row = (const float4*)s_w[slot];
#pragma unroll
    for (int q = 0; q < kFeatures / 4; ++q) {
        const float4 v = row[q];
        w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
    }
    if constexpr (kF == kMoveFeatures) {
        const float2 v = ((const float2*)row)[6];
        w[kF - 2] = v.x; w[kF - 1] = v.y;
    }
    bool goes_on = false;
    if constexpr (kPlies == 2) {
        tpl::next_window(s1, false, 0);                                 // tpl_afterstates' pop: the next piece becomes current
        goes_on = contends && running && s1.state == tpl::ST_RUNNING;
    }

    float value;
    uint32_t second = kNoSecond;
    if (goes_on) {
        value = best_second<kF>(s1, s_shape, p.L, p.M, second, [&](const tpl::Board& s2, uint32_t n2) {
            FeatureSet<kF> psi;
            moved_features(s2, n1 + n2, true, psi);                     // the carries of both moves, the board of the second
            return placement_score(w, psi);
        });
    } else {
        FeatureSet<kF> phi;
        moved_features(s1, n1, running, phi);
        value = placement_score(w, phi);
    }
    const unsigned long long key = ((unsigned long long)ordered_bits(value) << 32) | (uint32_t)(kActions - 1 - a);
    if (contends) atomicMax(&s_best[slot], key);
    __syncthreads();
    if (contends && s_best[slot] == key) {                              // one lane per board: the keys of a board are distinct
        p.action[i] = (uint8_t)a;
        if (kPlies == 2 && p.second) p.second[i] = (uint8_t)second;
        if (p.score) p.score[i] = value;
    }
}

__global__ __launch_bounds__(kActBlock) void TPL_UNIT_KERNEL(placement_act)(const PolicyArgs p) { placement_policy<1>(p); }
__global__ __launch_bounds__(kActBlock) void TPL_UNIT_KERNEL(placement_search)(const PolicyArgs p) { placement_policy<2>(p); }

}  // namespace
}  // namespace tpl_learn

using namespace tpl_learn;

namespace {

// what tpl_placement_act (plies = 1, second = null) and tpl_placement_search (plies = 2) share: the checks and the launch
int launch_policy(const char* name, int plies, const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M,
                  const float* weights, int64_t boards_per_member, uint8_t* action, uint8_t* second, float* score, void* stream) {
    if (const int rc = check_policy(name, plane_a, plane_b, n, L, M, weights, boards_per_member, action, score)) return rc;
    PolicyArgs p{};
    p.a = (const uint4*)plane_a; p.b = (const uint4*)plane_b; p.n = (uint32_t)n;
    p.L = (uint32_t)L; p.M = (uint32_t)M; p.weights = weights;
    p.per_member = (uint32_t)(boards_per_member < n ? boards_per_member : n);     // anything above n is the single-policy case
    p.action = action; p.second = second; p.score = score;
    const dim3 grid((p.n + kBoardsPerBlock - 1) / kBoardsPerBlock), block(kActBlock);
    hipLaunchKernelGGL(plies == 2 ? TPL_UNIT_KERNEL(placement_search) : TPL_UNIT_KERNEL(placement_act), grid, block, 0,
                       (hipStream_t)stream, p);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}

}  // namespace

extern "C" int TPL_UNIT_ENTRY(tpl_placement_features)(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M,
                                      int16_t* features, uint8_t* canonical, void* stream) {
    const char* name = TPL_UNIT_ENTRY_NAME(tpl_placement_features);
    constexpr unsigned align = kF == kMoveFeatures ? 16u : 8u;                       // the width of a record's stores
    if (const int rc = check_planes(name, plane_a, plane_b, n, L, M)) return rc;
    if (!features) return fail_msg(TPL_ERR_ARG, "%s: null pointer (features is required)", name);
    if ((uintptr_t)features & (align - 1u)) return fail_msg(TPL_ERR_ARG, "%s: features must be %u-byte aligned", name, align);
    FeatureArgs p{};
    p.a = (const uint4*)plane_a; p.b = (const uint4*)plane_b; p.total = (uint32_t)(n * kActions);
    p.L = (uint32_t)L; p.M = (uint32_t)M; p.features = features; p.canonical = canonical;
    const dim3 grid((p.total + kFeatureBlock - 1) / kFeatureBlock), block(kFeatureBlock);
    hipLaunchKernelGGL(TPL_UNIT_KERNEL(placement_features), grid, block, 0, (hipStream_t)stream, p);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}

extern "C" int TPL_UNIT_ENTRY(tpl_placement_act)(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const float* weights,
                                 int64_t boards_per_member, uint8_t* action, float* score, void* stream) {
    return launch_policy(TPL_UNIT_ENTRY_NAME(tpl_placement_act), 1, plane_a, plane_b, n, L, M, weights, boards_per_member, action, nullptr, score, stream);
}

extern "C" int TPL_UNIT_ENTRY(tpl_placement_search)(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const float* weights,
                                    int64_t boards_per_member, uint8_t* action, uint8_t* second, float* score, void* stream) {
    return launch_policy(TPL_UNIT_ENTRY_NAME(tpl_placement_search), 2, plane_a, plane_b, n, L, M, weights, boards_per_member, action, second, score,
                         stream);
}
