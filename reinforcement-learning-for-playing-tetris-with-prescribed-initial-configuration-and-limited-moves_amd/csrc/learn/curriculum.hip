// curriculum.hip -- outcomes per configuration and a reweighted pool: tpl_config_index, tpl_pool_tally, tpl_pool_resample
// (include/tpl_learn.h, "Per-configuration tallies and the resampled pool", states the rules).
//
// The environment keeps neither the pool entry a board was dealt nor an episode number: a running board's episode began at
// birth = clock - moves_used and its entry is assign_config(global index, birth, seed) in the buffer whose bit it carries
// (csrc/tpl_device.h).  Everything here is computed from the side with that rule -- tpl_device.h's own assign_config, unpack_board
// and, for the move, tpl_placement.h's first_move, the body the afterstate kernel uses -- and only READS the environment: the step
// kernel, the planes, the clocks and the statistics stay as they are.
//
// config_index_kernel and pool_tally_kernel: one lane per board, 256 lanes a block.  A lane reads its 32 state bytes (two 16-byte loads,
// 1 KiB a wave and plane), its group's clock (8 bytes per 32 boards: two addresses a wave) and, for the tally, its action.
//
// The tally's adds.  A board ends about once in M steps, so a wave of 64 has one or two ends a step and most waves of a small batch
// none: the adds are rare and, over a pool of 65,536 entries, scattered -- one no-return integer atomic per end is all there is to
// do.  Over a pool of a few entries every end of the chip lands on the same few words, and adds to one word serialise at the memory
// side; so a wave COMBINES its ends before they leave it: while ends are pending the first pending lane's (slot, entry) is broadcast
// (v_readlane), the lanes that hold the same key are counted by a ballot and a popcount, and the leader makes one add of the count
// (and one of the wins among them).  The loop runs once per DISTINCT key of the wave: once or twice where the adds are scattered (the
// same atomics as without it, plus two ballots), once where they collide (one add instead of up to 64).  Integer adds commute: the
// bytes do not depend on the order, nor on the grouping.  Blocks are not combined (an LDS image of the tallies would serve pools of
// a few hundred entries only, and the large pools are the ones training uses).
//
// pool_resample_kernel: EIGHT lanes per draw.  A record is 40 bytes of rows and M + 1 bytes of pieces; one lane per draw would store
// them with 5 + (M + 1) instructions whose 64 lanes each hit another line.  Eight lanes share a draw: all eight make the same binary
// search over the inclusive prefix sums (the same addresses: one request serves them, log2(n_cfg) dependent L2 reads), then lanes 0 .. 4 copy the rows as
// 8-byte words and all eight copy the pieces bytewise, lane k the bytes k, k + 8, ... -- a draw's 40 and M + 1 bytes leave as
// contiguous runs.  Everything is integers: the draw is draw_hash of replay_key(seed, round) (tpl_learn_internal.h), the target its
// 64 x 64-bit multiply-high with the total, the search exact.
#include "tpl_placement.h"

namespace tpl_learn {
namespace {

constexpr int kCurriculumBlock = 256;
constexpr int kLanesPerDraw = 8;
constexpr int kRowBytes = tpl::kRows * 2;                       // 40: five 8-byte words

struct AssignArgs {
    const uint4* a;              // [n]
    const uint4* b;
    const unsigned long long* clock;   // [ceil(n / 32)]
    uint32_t n;
    int64_t global_offset;
    uint32_t seed_mix;           // tpl::assign_seed(seed)
    int32_t mode;
    uint32_t n_cfg[2];           // by the slot bit; 0 = no such buffer
    uint32_t offset_mod[2];      // global_offset mod n_cfg
};

// the pool entry of the episode board i is playing, given its moves_used and slot bit (csrc/tpl_step.h: current_config)
__device__ __forceinline__ uint32_t entry_of(const AssignArgs& p, uint32_t i, uint32_t moves, uint32_t slot) {
    const uint32_t n_cfg = slot ? p.n_cfg[1] : p.n_cfg[0];
    const uint32_t offset_mod = slot ? p.offset_mod[1] : p.offset_mod[0];
    const uint64_t birth = (uint64_t)p.clock[i >> tpl::kClockShift] - moves;
    return n_cfg ? tpl::assign_config(p.global_offset, offset_mod, i, birth, p.seed_mix, n_cfg, p.mode) : 0u;
}

__global__ __launch_bounds__(kCurriculumBlock) void config_index_kernel(const AssignArgs p, uint32_t* index, uint8_t* slot_out) {
    const uint32_t i = blockIdx.x * kCurriculumBlock + threadIdx.x;
    if (i >= p.n) return;
    const uint4 A = p.a[i], B = p.b[i];
    const uint32_t slot = tpl::packed_slot(B);
    // a frozen board's clock runs on while its moves_used stands still: its birth is gone, and its entry is left as the caller has it
    if (index && tpl::packed_state(B) == tpl::ST_RUNNING) index[i] = entry_of(p, i, tpl::packed_moves(A), slot);
    if (slot_out) slot_out[i] = (uint8_t)slot;
}

struct TallyArgs {
    AssignArgs at;
    uint32_t L, M;
    const void* action;          // [n] of 1 << int_shift bytes each, little-endian: the low 32 bits are the action (tpl_step's reading)
    uint32_t int_shift;
    int32_t* episodes[2];        // by the slot bit, each with wins[.] or null
    int32_t* wins[2];
};

__global__ __launch_bounds__(kCurriculumBlock) void pool_tally_kernel(const TallyArgs p) {
    __shared__ tpl::ShapeWord s_shape[32];
    if (threadIdx.x < 32) s_shape[threadIdx.x] = tpl::kShapeTable[threadIdx.x];
    __syncthreads();
    const uint32_t i = blockIdx.x * kCurriculumBlock + threadIdx.x;
    const bool valid = i < p.at.n;
    bool end = false, won = false;
    uint32_t entry = 0u, slot = 0u;
    if (valid) {
        const uint4 A = p.at.a[i], B = p.at.b[i];
        uint32_t action;
        if (p.int_shift == 0u) action = ((const uint8_t*)p.action)[i];
        else action = *(const uint32_t*)((const char*)p.action + ((size_t)i << p.int_shift));
        const uint32_t rot = action / 10u, loc = action - rot * 10u;       // tpl_step's split: rot is taken mod 4 by the move
        const uint32_t moves = tpl::packed_moves(A);                       // before the move: birth = clock - moves_used
        tpl::Board s;
        uint32_t cur;
        bool running;
        first_move(A, B, s_shape, rot, loc, p.L, p.M, s, cur, running);
        slot = s.slot;
        end = running && s.state != tpl::ST_RUNNING && (slot ? p.episodes[1] : p.episodes[0]) != nullptr;
        won = s.state == tpl::ST_WON;
        if (end) entry = entry_of(p.at, i, moves, slot);
    }
    // one add per distinct (slot, entry) of the wave
    const uint32_t lane = __lane_id();
    unsigned long long pending = __ballot(end);
    while (pending) {
        const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)pending) - 1);
        const uint32_t key_entry = (uint32_t)__builtin_amdgcn_readlane((int)entry, leader);
        const uint32_t key_slot = (uint32_t)__builtin_amdgcn_readlane((int)slot, leader);
        const bool mine = end && entry == key_entry && slot == key_slot;
        const unsigned long long group = __ballot(mine), group_won = __ballot(mine && won);
        if (lane == (uint32_t)leader) {
            atomicAdd((key_slot ? p.episodes[1] : p.episodes[0]) + key_entry, (int32_t)__popcll(group));
            if (group_won) atomicAdd((key_slot ? p.wins[1] : p.wins[0]) + key_entry, (int32_t)__popcll(group_won));
        }
        pending &= ~group;
    }
}

struct ResampleArgs {
    const uint8_t* rows;         // [n_cfg][40]
    const uint8_t* pieces;       // [n_cfg][record]
    const long long* prefix;     // [n_cfg] inclusive sums of the weights
    uint32_t n_cfg, record;      // record = M + 1
    uint64_t count, key;         // key = replay_key(seed, round)
    uint8_t* rows_out;           // [count][40]
    uint8_t* pieces_out;         // [count][record]
    int32_t* source;             // [count]
};

__global__ __launch_bounds__(kCurriculumBlock) void pool_resample_kernel(const ResampleArgs p) {
    const uint64_t t = (uint64_t)blockIdx.x * kCurriculumBlock + threadIdx.x;
    const uint64_t j = t / kLanesPerDraw;
    const uint32_t sub = (uint32_t)t % kLanesPerDraw;
    if (j >= p.count) return;
    const uint64_t total = (uint64_t)p.prefix[p.n_cfg - 1u];
    const uint64_t target = __umul64hi(draw_hash(p.key, j), total);        // below total
    // the first entry whose inclusive sum is above the target: it exists (the last sum is the total), and a weight of 0 repeats the
    // sum before it, so such an entry is never the first.  lo stays inside [0, n_cfg) whatever the sums hold.
    uint32_t lo = 0u, hi = p.n_cfg - 1u;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)p.prefix[mid] > target) hi = mid; else lo = mid + 1u;
    }
    if (sub < (uint32_t)(kRowBytes / 8))
        ((uint2*)(p.rows_out + j * kRowBytes))[sub] = ((const uint2*)(p.rows + (size_t)lo * kRowBytes))[sub];
    const uint8_t* from = p.pieces + (size_t)lo * p.record;
    uint8_t* to = p.pieces_out + j * p.record;
    for (uint32_t k = sub; k < p.record; k += kLanesPerDraw) to[k] = from[k];
    if (sub == 0u) p.source[j] = (int32_t)lo;
}

// what tpl_config_index and tpl_pool_tally check of the environment they read, and the assignment's arguments
int assign_args(const char* name, const void* plane_a, const void* plane_b, const void* clock, int64_t n, int64_t global_offset,
                uint64_t seed, int32_t assign_mode, int64_t n_cfg0, int64_t n_cfg1, AssignArgs& at) {
    if (!plane_a || !plane_b || !clock) return fail_msg(TPL_ERR_ARG, "%s: null pointer (planes and clock are required)", name);
    if (n < 1 || n >= ((int64_t)1 << 31)) return fail_msg(TPL_ERR_ARG, "%s: n must be in [1, 2^31)", name);
    if (((uintptr_t)plane_a & 15u) || ((uintptr_t)plane_b & 15u)) return fail_msg(TPL_ERR_ARG, "%s: planes must be 16-byte aligned", name);
    if ((uintptr_t)clock & 7u) return fail_msg(TPL_ERR_ARG, "%s: clock must be 8-byte aligned", name);
    if (global_offset < 0) return fail_msg(TPL_ERR_ARG, "%s: global_offset must not be negative", name);
    if (assign_mode != 0 && assign_mode != 1) return fail_msg(TPL_ERR_ARG, "%s: assign_mode must be 0 (hash) or 1 (sequential)", name);
    if (n_cfg0 < 0 || n_cfg1 < 0 || n_cfg0 >= ((int64_t)1 << 32) || n_cfg1 >= ((int64_t)1 << 32))
        return fail_msg(TPL_ERR_ARG, "%s: n_cfg out of range (each buffer holds 0 .. 2^32 - 1 entries)", name);
    if (n_cfg0 == 0 && n_cfg1 == 0) return fail_msg(TPL_ERR_ARG, "%s: no pool (both n_cfg are 0)", name);
    at.a = (const uint4*)plane_a; at.b = (const uint4*)plane_b; at.clock = (const unsigned long long*)clock; at.n = (uint32_t)n;
    at.global_offset = global_offset; at.seed_mix = tpl::assign_seed(seed); at.mode = assign_mode;
    at.n_cfg[0] = (uint32_t)n_cfg0; at.n_cfg[1] = (uint32_t)n_cfg1;
    at.offset_mod[0] = n_cfg0 ? (uint32_t)((uint64_t)global_offset % (uint64_t)n_cfg0) : 0u;
    at.offset_mod[1] = n_cfg1 ? (uint32_t)((uint64_t)global_offset % (uint64_t)n_cfg1) : 0u;
    return TPL_OK;
}

}  // namespace
}  // namespace tpl_learn

using namespace tpl_learn;

extern "C" int tpl_config_index(const void* plane_a, const void* plane_b, const void* clock, int64_t n, int64_t global_offset,
                                uint64_t seed, int32_t assign_mode, int64_t n_cfg0, int64_t n_cfg1, uint32_t* index, uint8_t* slot,
                                void* stream) {
    AssignArgs at{};
    if (const int rc = assign_args("tpl_config_index", plane_a, plane_b, clock, n, global_offset, seed, assign_mode, n_cfg0, n_cfg1, at))
        return rc;
    if (!index && !slot) return fail_msg(TPL_ERR_ARG, "tpl_config_index: at least one output must be given");
    if ((uintptr_t)index & 3u) return fail_msg(TPL_ERR_ARG, "tpl_config_index: index must be 4-byte aligned");
    const dim3 grid((at.n + kCurriculumBlock - 1) / kCurriculumBlock), block(kCurriculumBlock);
    hipLaunchKernelGGL(config_index_kernel, grid, block, 0, (hipStream_t)stream, at, index, slot);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}

extern "C" int tpl_pool_tally(const void* plane_a, const void* plane_b, const void* clock, int64_t n, int32_t L, int32_t M,
                              const void* action, int32_t dtype, int64_t global_offset, uint64_t seed, int32_t assign_mode,
                              int64_t n_cfg0, int64_t n_cfg1, int32_t* episodes0, int32_t* wins0, int32_t* episodes1, int32_t* wins1,
                              void* stream) {
    TallyArgs p{};
    if (const int rc = assign_args("tpl_pool_tally", plane_a, plane_b, clock, n, global_offset, seed, assign_mode, n_cfg0, n_cfg1, p.at))
        return rc;
    if (L < 1 || L > 250 || M < 1 || M > 254) return fail_msg(TPL_ERR_ARG, "tpl_pool_tally: L and M must be in [1, 250] and [1, 254]");
    if (!action) return fail_msg(TPL_ERR_ARG, "tpl_pool_tally: null pointer (action is required)");
    if (dtype != TPL_U8 && dtype != TPL_I32 && dtype != TPL_I64)
        return fail_msg(TPL_ERR_ARG, "tpl_pool_tally: dtype must be TPL_U8, TPL_I32 or TPL_I64");
    const uint32_t shift = dtype == TPL_U8 ? 0u : dtype == TPL_I32 ? 2u : 3u;
    if ((uintptr_t)action & ((1u << shift) - 1u)) return fail_msg(TPL_ERR_ARG, "tpl_pool_tally: action is not aligned to its type");
    if ((episodes0 == nullptr) != (wins0 == nullptr) || (episodes1 == nullptr) != (wins1 == nullptr))
        return fail_msg(TPL_ERR_ARG, "tpl_pool_tally: a buffer's episodes and wins go together");
    if (!episodes0 && !episodes1) return fail_msg(TPL_ERR_ARG, "tpl_pool_tally: at least one buffer's tallies must be given");
    if ((episodes0 && n_cfg0 == 0) || (episodes1 && n_cfg1 == 0))
        return fail_msg(TPL_ERR_ARG, "tpl_pool_tally: tallies given for a buffer of 0 entries");
    if (((uintptr_t)episodes0 | (uintptr_t)wins0 | (uintptr_t)episodes1 | (uintptr_t)wins1) & 3u)
        return fail_msg(TPL_ERR_ARG, "tpl_pool_tally: tallies must be 4-byte aligned");
    p.L = (uint32_t)L; p.M = (uint32_t)M; p.action = action; p.int_shift = shift;
    p.episodes[0] = episodes0; p.wins[0] = wins0; p.episodes[1] = episodes1; p.wins[1] = wins1;
    const dim3 grid((p.at.n + kCurriculumBlock - 1) / kCurriculumBlock), block(kCurriculumBlock);
    hipLaunchKernelGGL(pool_tally_kernel, grid, block, 0, (hipStream_t)stream, p);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}

extern "C" int tpl_pool_resample(const void* rows, const void* pieces, int64_t n_cfg, int32_t M, const int64_t* prefix,
                                 int64_t count, uint64_t seed, uint64_t round, void* rows_out, void* pieces_out, int32_t* source,
                                 void* stream) {
    if (!rows || !pieces || !prefix || !rows_out || !pieces_out || !source) return fail_msg(TPL_ERR_ARG, "tpl_pool_resample: null pointer");
    if (n_cfg < 1 || n_cfg >= ((int64_t)1 << 31)) return fail_msg(TPL_ERR_ARG, "tpl_pool_resample: n_cfg must be in [1, 2^31)");
    if (count < 1 || count >= ((int64_t)1 << 31)) return fail_msg(TPL_ERR_ARG, "tpl_pool_resample: count must be in [1, 2^31)");
    if (M < 1 || M > 254) return fail_msg(TPL_ERR_ARG, "tpl_pool_resample: M must be in [1, 254]");
    if (((uintptr_t)rows & 7u) || ((uintptr_t)rows_out & 7u) || ((uintptr_t)prefix & 7u))
        return fail_msg(TPL_ERR_ARG, "tpl_pool_resample: rows, rows_out and prefix must be 8-byte aligned");
    if ((uintptr_t)source & 3u) return fail_msg(TPL_ERR_ARG, "tpl_pool_resample: source must be 4-byte aligned");
    if (rows == rows_out || pieces == pieces_out) return fail_msg(TPL_ERR_ARG, "tpl_pool_resample: the outputs must not be the inputs");
    ResampleArgs p{};
    p.rows = (const uint8_t*)rows; p.pieces = (const uint8_t*)pieces; p.prefix = (const long long*)prefix;
    p.n_cfg = (uint32_t)n_cfg; p.record = (uint32_t)M + 1u; p.count = (uint64_t)count; p.key = replay_key(seed, round);
    p.rows_out = (uint8_t*)rows_out; p.pieces_out = (uint8_t*)pieces_out; p.source = source;
    const uint64_t lanes = (uint64_t)count * kLanesPerDraw;
    const dim3 grid((uint32_t)((lanes + kCurriculumBlock - 1) / kCurriculumBlock)), block(kCurriculumBlock);
    hipLaunchKernelGGL(pool_resample_kernel, grid, block, 0, (hipStream_t)stream, p);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}
