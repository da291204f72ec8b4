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
//   mirror  tpl_replay_sample_mirror: any of those forms with emit_draw's mirrored form on top (tpl_mirror.h), which reflects
//           s, a and s' of a draw left to right on the draw's coin -- vector ALU work only, no traffic of its own;
//           tpl_mirror_states applies the same device functions to planes a caller holds.
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

template <typename T, int kN = 0, bool kMirror = false>      // emit_draw's form (kN = 0: 1-step)
__global__ __launch_bounds__(64 * kObsWaves) void replay_sample_kernel(const SampleArgs p) {
    __shared__ __attribute__((aligned(16))) uint8_t s_rows[kObsWaves][kWaveLds];
    const int lane = threadIdx.x & 63;
    const int64_t base = ((int64_t)blockIdx.x * kObsWaves + (threadIdx.x >> 6)) * 64;     // the wave's first draw
    if (base >= p.batch) return;                                                          // wave-uniform
    const int count = (int)((p.batch - base) < 64 ? (p.batch - base) : 64);
    const int64_t slot = lane < count ? replay_slot(p.key, (uint64_t)(base + lane), (uint64_t)p.size) : 0;
    emit_draw<T, kN, kMirror>(p, s_rows[threadIdx.x >> 6], lane, count, base, slot);
}

}  // namespace

int launch_uniform(const SampleArgs& p, int32_t dtype, hipStream_t stream) {
    const dim3 grid((unsigned)((p.batch + 64 * kObsWaves - 1) / (64 * kObsWaves))), block(64 * kObsWaves);
    dispatch_form(p, [&](auto n, auto m) {
        constexpr int kN = decltype(n)::value;
        constexpr bool kMirror = decltype(m)::value;
        if (dtype == TPL_F32)
            hipLaunchKernelGGL((replay_sample_kernel<float, kN, kMirror>), grid, block, 0, stream, p);
        else
            hipLaunchKernelGGL((replay_sample_kernel<__hip_bfloat16, kN, kMirror>), grid, block, 0, stream, p);
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

namespace tpl_learn {
namespace {

// tpl_replay_sample_nstep and tpl_replay_sample_mirror: one set of checks, in the name of `fn`.  n_step = 0 (the mirror entry
// only) is the 1-step form, which takes no head, stride, gamma, discount or steps.
int sample_checked(const char* fn, const void* ring, const void* tree, int64_t capacity, int64_t size, int64_t head,
                   int64_t stride, int32_t n_step, float gamma, int64_t batch, uint64_t seed, uint64_t update, int32_t L, int32_t M,
                   void* obs, int32_t dtype, void* next_a, void* next_b, uint8_t* action, float* ret, float* discount, uint8_t* done,
                   uint8_t* steps, int64_t* index, float* prob, int32_t mirror, uint8_t* mirrored, void* stream) {
    const bool one_step = n_step == 0;
    if (!ring || !obs || !next_a || !next_b || !action || !ret || !done) return fail_msg(TPL_ERR_ARG, "%s: null pointer", fn);
    if (!one_step && (!discount || !steps)) return fail_msg(TPL_ERR_ARG, "%s: null pointer", fn);
    if (one_step && (discount || steps))
        return fail_msg(TPL_ERR_ARG, "%s: discount and steps must be NULL in the 1-step form (n_step = 0)", fn);
    if (tree && (!index || !prob)) return fail_msg(TPL_ERR_ARG, "%s: null pointer (a tree needs index and prob)", fn);
    if (!tree && prob) return fail_msg(TPL_ERR_ARG, "%s: prob must be NULL without a tree", fn);
    if (capacity < 1 || capacity >= kMaxSize) return fail_msg(TPL_ERR_ARG, "%s: capacity must be in [1, 2^32)", fn);
    if (size < 1 || size > capacity)
        return fail_msg(TPL_ERR_ARG, "%s: size must be in [1, capacity] (an empty ring has nothing to draw)", fn);
    if (batch < 1) return fail_msg(TPL_ERR_ARG, "%s: batch must be positive", fn);
    if (batch > ((int64_t)1 << 31) / TPL_OBS_DIM) return fail_msg(TPL_ERR_ARG, "%s: batch too large", fn);
    if (L < 1 || L > 255 || M < 1 || M > 255) return fail_msg(TPL_ERR_ARG, "%s: L and M must be in [1, 255]", fn);
    if (dtype != TPL_F32 && dtype != TPL_BF16) return fail_msg(TPL_ERR_ARG, "%s: unknown observation dtype %d", fn, dtype);
    if (((uintptr_t)ring & 15u) || ((uintptr_t)obs & 15u) || ((uintptr_t)next_a & 15u) || ((uintptr_t)next_b & 15u))
        return fail_msg(TPL_ERR_ARG, "%s: ring, obs and planes must be 16-byte aligned", fn);
    if (mirror < 0 || mirror > 2) return fail_msg(TPL_ERR_ARG, "%s: mirror must be 0 (never), 1 (the coin) or 2 (always)", fn);
    if (!one_step) {
        if (n_step < 1 || n_step > TPL_NSTEP_MAX) return fail_msg(TPL_ERR_ARG, "%s: n_step must be in [1, %d]", fn, TPL_NSTEP_MAX);
        if (!(gamma >= 0.0f && gamma <= 1.0f)) return fail_msg(TPL_ERR_ARG, "%s: gamma must be in [0, 1]", fn);
        if (stride < 1 || stride > capacity) return fail_msg(TPL_ERR_ARG, "%s: stride must be in [1, capacity]", fn);
        if (head < 0 || head >= capacity) return fail_msg(TPL_ERR_ARG, "%s: head must be in [0, capacity)", fn);
        if (size < capacity && head != size) return fail_msg(TPL_ERR_ARG, "%s: head must equal size until the ring is full", fn);
    }
    SampleArgs p{};
    p.ring = (const uint4*)ring; p.size = size; p.batch = batch; p.key = replay_key(seed, update);
    p.L = (uint32_t)L; p.M = (uint32_t)M; p.obs = obs; p.next_a = (uint4*)next_a; p.next_b = (uint4*)next_b;
    p.action = action; p.reward = ret; p.done = done; p.index = index;
    p.n_step = n_step;
    if (!one_step) {
        p.capacity = capacity; p.head = head; p.stride = stride; p.gamma = gamma;
        p.discount = discount; p.steps = steps;
    }
    p.mirror = mirror; p.mirrored = mirrored;
    if (mirror == 0 && mirrored)                                 // the plain kernels know nothing of it
        TPL_LEARN_HIP(hipMemsetAsync(mirrored, 0, (size_t)batch, (hipStream_t)stream));
    if (tree) return launch_prioritized(fn, p, tree, capacity, prob, dtype, (hipStream_t)stream);
    return launch_uniform(p, dtype, (hipStream_t)stream);
}

struct MirrorArgs {
    int64_t count;
    const uint4* a;
    const uint4* b;
    uint4* out_a;
    uint4* out_b;
    const uint8_t* action;       // optional, with out_action
    uint8_t* out_action;
};

__global__ __launch_bounds__(kPushBlock) void mirror_states_kernel(const MirrorArgs p) {
    const int64_t i = (int64_t)blockIdx.x * kPushBlock + threadIdx.x;
    if (i >= p.count) return;
    uint4 A = p.a[i], B = p.b[i];
    const uint32_t cur = B.w & 7u;                               // entry 0 of the window, before the reflection
    mirror_planes(A, B, true);
    p.out_a[i] = A;
    p.out_b[i] = B;
    if (p.action) p.out_action[i] = (uint8_t)mirror_action(p.action[i], cur, true);
}

}  // namespace
}  // namespace tpl_learn

extern "C" int tpl_replay_sample_nstep(const void* ring, const void* tree, int64_t capacity, int64_t size, int64_t head,
                                       int64_t stride, int32_t n_step, float gamma, int64_t batch, uint64_t seed, uint64_t update,
                                       int32_t L, int32_t M, void* obs, int32_t dtype, void* next_a, void* next_b, uint8_t* action,
                                       float* ret, float* discount, uint8_t* done, uint8_t* steps, int64_t* index, float* prob,
                                       void* stream) {
    if (n_step < 1) return fail_msg(TPL_ERR_ARG, "tpl_replay_sample_nstep: n_step must be in [1, %d]", TPL_NSTEP_MAX);
    return sample_checked("tpl_replay_sample_nstep", ring, tree, capacity, size, head, stride, n_step, gamma, batch, seed, update,
                          L, M, obs, dtype, next_a, next_b, action, ret, discount, done, steps, index, prob, 0, nullptr, stream);
}

extern "C" int tpl_replay_sample_mirror(const void* ring, const void* tree, int64_t capacity, int64_t size, int64_t head,
                                        int64_t stride, int32_t n_step, float gamma, int64_t batch, uint64_t seed, uint64_t update,
                                        int32_t L, int32_t M, void* obs, int32_t dtype, void* next_a, void* next_b, uint8_t* action,
                                        float* ret, float* discount, uint8_t* done, uint8_t* steps, int64_t* index, float* prob,
                                        int32_t mirror, uint8_t* mirrored, void* stream) {
    if (n_step < 0) return fail_msg(TPL_ERR_ARG, "tpl_replay_sample_mirror: n_step must be in [0, %d]", TPL_NSTEP_MAX);
    return sample_checked("tpl_replay_sample_mirror", ring, tree, capacity, size, head, stride, n_step, gamma, batch, seed, update,
                          L, M, obs, dtype, next_a, next_b, action, ret, discount, done, steps, index, prob, mirror, mirrored,
                          stream);
}

extern "C" int tpl_mirror_states(int64_t count, const void* a, const void* b, void* out_a, void* out_b, const uint8_t* action,
                                 uint8_t* out_action, void* stream) {
    if (!a || !b || !out_a || !out_b) return fail_msg(TPL_ERR_ARG, "tpl_mirror_states: null pointer");
    if ((action == nullptr) != (out_action == nullptr))
        return fail_msg(TPL_ERR_ARG, "tpl_mirror_states: action and out_action go together");
    if (count < 1 || count >= ((int64_t)1 << 31)) return fail_msg(TPL_ERR_ARG, "tpl_mirror_states: count must be in [1, 2^31)");
    if (((uintptr_t)a & 15u) || ((uintptr_t)b & 15u) || ((uintptr_t)out_a & 15u) || ((uintptr_t)out_b & 15u))
        return fail_msg(TPL_ERR_ARG, "tpl_mirror_states: planes must be 16-byte aligned");
    MirrorArgs p{};
    p.count = count; p.a = (const uint4*)a; p.b = (const uint4*)b; p.out_a = (uint4*)out_a; p.out_b = (uint4*)out_b;
    p.action = action; p.out_action = out_action;
    const dim3 grid((unsigned)((count + kPushBlock - 1) / kPushBlock)), block(kPushBlock);
    hipLaunchKernelGGL(mirror_states_kernel, grid, block, 0, (hipStream_t)stream, p);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}
