// replay.hip -- the packed replay ring: push one actor_rollout chunk, sample one minibatch.
//
// A transition is an 80-byte record (include/tpl_learn.h): s and s' as the environment's 32-byte resident state, then the
// reward, action and done.  Against the 868-byte float32 observation that is 2 x 32 B for both states: a ring of 2^24
// transitions is 1.3 GB.  The observation of s is made only when a minibatch is drawn, with the environment's own two
// stages (tpl_observe.h), so it is bit-identical to tpl_expand_states of the same planes; s' leaves as planes, to be
// read by the target network's policy kernel in place.
//
//   push    one lane per transition (t, i): three 16-byte loads of the chunk (s, and s' = the state recorded at t + 1,
//           or the resident planes after the chunk for the last step), the three scalars, five 16-byte stores.
//           Consecutive lanes write consecutive records, so every wave store covers 1,280 contiguous bytes.
//   sample  one lane per draw: the slot is a hash of (seed, update, i), the record comes in as five 16-byte loads
//           (random slots: the 80 B are the whole traffic of the read side), s is turned into 217 feature bytes in LDS
//           and leaves as the wave's contiguous span of the observation with 16-byte non-temporal stores -- observe.hip's
//           scheme, so a draw costs 80 B read and 868 B (f32) / 434 B (bf16) + 32 B + 6 B written.
//   n-step  tpl_replay_sample_nstep: the same kernels in emit_draw's n-step form (tpl_replay_draw.h), which adds up to
//           n_step - 1 successor tail words and one s' read per draw, and writes the return, discount and step count.
#include "tpl_replay_draw.h"

#include <cstdarg>
#include <cstdio>

namespace tpl_learn {

static thread_local char g_err[512] = "";

int fail_msg(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

namespace {

using tpl::obs::kObsWaves;
using tpl::obs::kWaveLds;

constexpr int kPushBlock = 256;
constexpr int64_t kMaxSize = (int64_t)1 << 32;     // the slot map takes size below 2^32 (343 GB of records: beyond HBM)

struct PushArgs {
    uint4* ring;                 // [capacity][5]
    int64_t capacity, head, total, n;
    const uint8_t* actions;
    const float* rewards;
    const uint8_t* dones;
    const uint4* states_a;
    const uint4* states_b;
    const uint4* plane_a;
    const uint4* plane_b;
};

__global__ __launch_bounds__(kPushBlock) void replay_push_kernel(const PushArgs p) {
    const int64_t j = (int64_t)blockIdx.x * kPushBlock + threadIdx.x;     // transition t * n + i of the chunk
    if (j >= p.total) return;
    const uint4 sa = p.states_a[j], sb = p.states_b[j];
    const int64_t nx = j + p.n;
    uint4 na, nb;
    if (nx < p.total) {
        na = p.states_a[nx]; nb = p.states_b[nx];
    } else {                                                              // the last step: s' is the resident state
        const int64_t i = j - (p.total - p.n);
        na = p.plane_a[i]; nb = p.plane_b[i];
    }
    const uint4 tail = make_uint4(__float_as_uint(p.rewards[j]), (uint32_t)p.actions[j] | ((uint32_t)p.dones[j] << 8), 0u, 0u);
    int64_t slot = p.head + j;                                            // head < capacity and j < capacity
    if (slot >= p.capacity) slot -= p.capacity;
    uint4* const rec = p.ring + slot * 5;
    rec[0] = sa; rec[1] = sb; rec[2] = na; rec[3] = nb; rec[4] = tail;
}

template <typename T, int kN = 0>                      // kN: emit_draw's form (0: 1-step)
__global__ __launch_bounds__(64 * kObsWaves) void replay_sample_kernel(const SampleArgs p) {
    __shared__ __attribute__((aligned(16))) uint8_t s_rows[kObsWaves][kWaveLds];
    const int lane = threadIdx.x & 63;
    const int64_t base = ((int64_t)blockIdx.x * kObsWaves + (threadIdx.x >> 6)) * 64;     // the wave's first draw
    if (base >= p.batch) return;                                                          // wave-uniform
    const int count = (int)((p.batch - base) < 64 ? (p.batch - base) : 64);
    const int64_t slot = lane < count ? replay_slot(p.key, (uint64_t)(base + lane), (uint64_t)p.size) : 0;
    emit_draw<T, kN>(p, s_rows[threadIdx.x >> 6], lane, count, base, slot);
}

}  // namespace

int launch_nstep_uniform(const SampleArgs& p, int32_t dtype, hipStream_t stream) {
    const dim3 grid((unsigned)((p.batch + 64 * kObsWaves - 1) / (64 * kObsWaves))), block(64 * kObsWaves);
    dispatch_nstep(p.n_step, [&](auto n) {
        if (dtype == TPL_F32)
            hipLaunchKernelGGL((replay_sample_kernel<float, decltype(n)::value>), grid, block, 0, stream, p);
        else
            hipLaunchKernelGGL((replay_sample_kernel<__hip_bfloat16, decltype(n)::value>), grid, block, 0, stream, p);
    });
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}
}  // namespace tpl_learn

using namespace tpl_learn;

extern "C" const char* tpl_learn_last_error(void) { return g_err; }

extern "C" size_t tpl_replay_record_bytes(void) { return (size_t)TPL_REPLAY_RECORD_BYTES; }

extern "C" int64_t tpl_replay_index(uint64_t seed, uint64_t update, int64_t i, int64_t size) {
    if (size < 1 || size >= kMaxSize || i < 0) return -1;
    return replay_slot(replay_key(seed, update), (uint64_t)i, (uint64_t)size);
}

extern "C" int tpl_replay_push(void* ring, int64_t capacity, int64_t head, int32_t num_steps, int64_t n, const uint8_t* actions,
                               const float* rewards, const uint8_t* dones, const void* states_a, const void* states_b,
                               const void* plane_a, const void* plane_b, void* stream) {
    if (!ring || !actions || !rewards || !dones || !states_a || !states_b || !plane_a || !plane_b)
        return fail_msg(TPL_ERR_ARG, "tpl_replay_push: null pointer");
    if (capacity < 1 || capacity >= kMaxSize) return fail_msg(TPL_ERR_ARG, "tpl_replay_push: capacity must be in [1, 2^32)");
    if (num_steps < 1 || n < 1) return fail_msg(TPL_ERR_ARG, "tpl_replay_push: num_steps and n must be positive");
    if ((int64_t)num_steps * n > capacity)
        return fail_msg(TPL_ERR_ARG, "tpl_replay_push: a chunk of %d x %lld transitions exceeds the capacity %lld", num_steps,
                        (long long)n, (long long)capacity);
    if (head < 0 || head >= capacity) return fail_msg(TPL_ERR_ARG, "tpl_replay_push: head must be in [0, capacity)");
    if (((uintptr_t)ring & 15u) || ((uintptr_t)states_a & 15u) || ((uintptr_t)states_b & 15u) || ((uintptr_t)plane_a & 15u) ||
        ((uintptr_t)plane_b & 15u))
        return fail_msg(TPL_ERR_ARG, "tpl_replay_push: ring, states and planes must be 16-byte aligned");
    PushArgs p{};
    p.ring = (uint4*)ring; p.capacity = capacity; p.head = head; p.total = (int64_t)num_steps * n; p.n = n;
    p.actions = actions; p.rewards = rewards; p.dones = dones;
    p.states_a = (const uint4*)states_a; p.states_b = (const uint4*)states_b;
    p.plane_a = (const uint4*)plane_a; p.plane_b = (const uint4*)plane_b;
    const dim3 grid((unsigned)((p.total + kPushBlock - 1) / kPushBlock)), block(kPushBlock);
    hipLaunchKernelGGL(replay_push_kernel, grid, block, 0, (hipStream_t)stream, p);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}

extern "C" int tpl_replay_sample(const void* ring, int64_t capacity, int64_t size, int64_t batch, uint64_t seed, uint64_t update,
                                 int32_t L, int32_t M, void* obs, int32_t dtype, void* next_a, void* next_b, uint8_t* action,
                                 float* reward, uint8_t* done, int64_t* index, void* stream) {
    if (!ring || !obs || !next_a || !next_b || !action || !reward || !done)
        return fail_msg(TPL_ERR_ARG, "tpl_replay_sample: null pointer");
    if (capacity < 1 || capacity >= kMaxSize) return fail_msg(TPL_ERR_ARG, "tpl_replay_sample: capacity must be in [1, 2^32)");
    if (size < 1 || size > capacity) return fail_msg(TPL_ERR_ARG, "tpl_replay_sample: size must be in [1, capacity] (an empty ring has nothing to draw)");
    if (batch < 1) return fail_msg(TPL_ERR_ARG, "tpl_replay_sample: batch must be positive");
    if (batch > ((int64_t)1 << 31) / TPL_OBS_DIM) return fail_msg(TPL_ERR_ARG, "tpl_replay_sample: batch too large");
    if (L < 1 || L > 255 || M < 1 || M > 255) return fail_msg(TPL_ERR_ARG, "tpl_replay_sample: L and M must be in [1, 255]");
    if (dtype != TPL_F32 && dtype != TPL_BF16) return fail_msg(TPL_ERR_ARG, "tpl_replay_sample: unknown observation dtype %d", dtype);
    if (((uintptr_t)ring & 15u) || ((uintptr_t)obs & 15u) || ((uintptr_t)next_a & 15u) || ((uintptr_t)next_b & 15u))
        return fail_msg(TPL_ERR_ARG, "tpl_replay_sample: ring, obs and planes must be 16-byte aligned");
    SampleArgs p{};
    p.ring = (const uint4*)ring; p.size = size; p.batch = batch; p.key = replay_key(seed, update);
    p.L = (uint32_t)L; p.M = (uint32_t)M; p.obs = obs; p.next_a = (uint4*)next_a; p.next_b = (uint4*)next_b;
    p.action = action; p.reward = reward; p.done = done; p.index = index;
    const dim3 grid((unsigned)((batch + 64 * kObsWaves - 1) / (64 * kObsWaves))), block(64 * kObsWaves);
    if (dtype == TPL_F32)
        hipLaunchKernelGGL(replay_sample_kernel<float>, grid, block, 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(replay_sample_kernel<__hip_bfloat16>, grid, block, 0, (hipStream_t)stream, p);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}

extern "C" int tpl_replay_sample_nstep(const void* ring, const void* tree, int64_t capacity, int64_t size, int64_t head,
                                       int64_t stride, int32_t n_step, float gamma, int64_t batch, uint64_t seed, uint64_t update,
                                       int32_t L, int32_t M, void* obs, int32_t dtype, void* next_a, void* next_b, uint8_t* action,
                                       float* ret, float* discount, uint8_t* done, uint8_t* steps, int64_t* index, float* prob,
                                       void* stream) {
    if (!ring || !obs || !next_a || !next_b || !action || !ret || !discount || !done || !steps)
        return fail_msg(TPL_ERR_ARG, "tpl_replay_sample_nstep: null pointer");
    if (tree && (!index || !prob))
        return fail_msg(TPL_ERR_ARG, "tpl_replay_sample_nstep: null pointer (a tree needs index and prob)");
    if (!tree && prob) return fail_msg(TPL_ERR_ARG, "tpl_replay_sample_nstep: prob must be NULL without a tree");
    if (capacity < 1 || capacity >= kMaxSize) return fail_msg(TPL_ERR_ARG, "tpl_replay_sample_nstep: capacity must be in [1, 2^32)");
    if (size < 1 || size > capacity)
        return fail_msg(TPL_ERR_ARG, "tpl_replay_sample_nstep: size must be in [1, capacity] (an empty ring has nothing to draw)");
    if (batch < 1) return fail_msg(TPL_ERR_ARG, "tpl_replay_sample_nstep: batch must be positive");
    if (batch > ((int64_t)1 << 31) / TPL_OBS_DIM) return fail_msg(TPL_ERR_ARG, "tpl_replay_sample_nstep: batch too large");
    if (L < 1 || L > 255 || M < 1 || M > 255) return fail_msg(TPL_ERR_ARG, "tpl_replay_sample_nstep: L and M must be in [1, 255]");
    if (dtype != TPL_F32 && dtype != TPL_BF16)
        return fail_msg(TPL_ERR_ARG, "tpl_replay_sample_nstep: unknown observation dtype %d", dtype);
    if (((uintptr_t)ring & 15u) || ((uintptr_t)obs & 15u) || ((uintptr_t)next_a & 15u) || ((uintptr_t)next_b & 15u))
        return fail_msg(TPL_ERR_ARG, "tpl_replay_sample_nstep: ring, obs and planes must be 16-byte aligned");
    if (n_step < 1 || n_step > TPL_NSTEP_MAX)
        return fail_msg(TPL_ERR_ARG, "tpl_replay_sample_nstep: n_step must be in [1, %d]", TPL_NSTEP_MAX);
    if (!(gamma >= 0.0f && gamma <= 1.0f)) return fail_msg(TPL_ERR_ARG, "tpl_replay_sample_nstep: gamma must be in [0, 1]");
    if (stride < 1 || stride > capacity) return fail_msg(TPL_ERR_ARG, "tpl_replay_sample_nstep: stride must be in [1, capacity]");
    if (head < 0 || head >= capacity) return fail_msg(TPL_ERR_ARG, "tpl_replay_sample_nstep: head must be in [0, capacity)");
    if (size < capacity && head != size)
        return fail_msg(TPL_ERR_ARG, "tpl_replay_sample_nstep: head must equal size until the ring is full");
    SampleArgs p{};
    p.ring = (const uint4*)ring; p.size = size; p.batch = batch; p.key = replay_key(seed, update);
    p.L = (uint32_t)L; p.M = (uint32_t)M; p.obs = obs; p.next_a = (uint4*)next_a; p.next_b = (uint4*)next_b;
    p.action = action; p.reward = ret; p.done = done; p.index = index;
    p.capacity = capacity; p.head = head; p.stride = stride; p.n_step = n_step; p.gamma = gamma;
    p.discount = discount; p.steps = steps;
    if (tree) return launch_nstep_prioritized(p, tree, capacity, prob, dtype, (hipStream_t)stream);
    return launch_nstep_uniform(p, dtype, (hipStream_t)stream);
}
