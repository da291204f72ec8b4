// priority.hip -- proportional prioritized replay: a 16-ary float64 sum tree over the ring's slots (include/tpl_learn.h
// states the layout and the rules; _learn_lib's numpy mirror restates them).
//
//   push      one lane per pushed slot sets its leaf to the running maximum, then one launch per level re-sums the parents of
//             the pushed range(s): the parents of a contiguous range are a contiguous range.
//   update    three steps, each a launch, since each must see every write of the one before in any workgroup: zero the
//             drawn leaves; max-combine the clamped priorities with a 64-bit atomicMax on the leaves' bit patterns (positive
//             doubles order like their bits, so duplicates resolve to the largest whatever the order) and fold the batch
//             maximum into the header; then one launch per level re-sums the touched ancestors.  Re-summing a node is
//             idempotent, so a node touched twice is written twice with the same value.  No sum uses an atomic: every
//             node is one lane's left-to-right sum of its 128-byte child line, bit-reproducible.
//   sample    one lane per draw descends from the root (one 128-byte line per level, eight 16-byte loads), then does what
//             the uniform sampler does with the slot it reached (tpl_replay_draw.h).
#include "tpl_replay_draw.h"

#include <cmath>

namespace tpl_learn {
namespace {

using tpl::obs::kObsWaves;
using tpl::obs::kWaveLds;

constexpr int kFan = TPL_PRIORITY_FANOUT;
constexpr int kHeaderWords = TPL_PRIORITY_HEADER_BYTES / 8;
constexpr int kMaxLevels = 9;                        // capacity < 2^32 = 16^8: levels 0 .. 8
constexpr int kBlock = 256;
constexpr int64_t kMaxCapacity = (int64_t)1 << 32;

// where each level starts, in doubles from the tree's base, and how many nodes it holds
struct Layout {
    int32_t levels;
    int64_t offset[kMaxLevels];
    int64_t count[kMaxLevels];
    int64_t words;                                   // the whole image
};

Layout layout(int64_t capacity) {
    Layout l{};
    int64_t n = capacity, at = kHeaderWords;
    for (int k = 0;; ++k) {
        l.offset[k] = at;
        l.count[k] = n;
        at += (n + kFan - 1) / kFan * kFan;
        l.levels = k + 1;
        if (n == 1) break;
        n = (n + kFan - 1) / kFan;
    }
    l.words = at;
    return l;
}

__host__ __device__ inline double draw_target(uint64_t key, int64_t i, int64_t batch, double total) {
#pragma clang fp contract(off)
    const uint64_t h = draw_hash(key, (uint64_t)i);
    const double U = (double)(h >> 11) * 0x1.0p-53;
    return (((double)i + U) * total) / (double)batch;
}

// node j of the level at `node` := its 16 children at `child` (one line), added left to right
__device__ __forceinline__ void resum(const double* child, double* node, int64_t j) {
#pragma clang fp contract(off)
    const double2* const c = (const double2*)(child + j * kFan);
    double2 v[kFan / 2];
#pragma unroll
    for (int q = 0; q < kFan / 2; ++q) v[q] = c[q];
    double s = v[0].x;
    s += v[0].y;
#pragma unroll
    for (int q = 1; q < kFan / 2; ++q) {
        s += v[q].x;
        s += v[q].y;
    }
    node[j] = s;
}

__global__ __launch_bounds__(64) void priority_init_kernel(double* tree, int64_t capacity, int64_t levels) {
    if (threadIdx.x == 0) {
        tree[0] = 1.0;
        ((int64_t*)tree)[1] = capacity;
        ((int64_t*)tree)[2] = levels;
    }
}

// leaves [lo0, lo0 + n0) and [lo1, lo1 + n1) := the running maximum
__global__ __launch_bounds__(kBlock) void priority_push_kernel(double* tree, int64_t lo0, int64_t n0, int64_t lo1, int64_t n1) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= n0 + n1) return;
    const int64_t leaf = t < n0 ? lo0 + t : lo1 + (t - n0);
    tree[kHeaderWords + leaf] = tree[0];
}

// nodes [lo0, lo0 + n0) and [lo1, lo1 + n1) of one level re-summed from the level below
__global__ __launch_bounds__(kBlock) void priority_resum_range_kernel(double* tree, int64_t child_off, int64_t node_off, int64_t lo0,
                                                                      int64_t n0, int64_t lo1, int64_t n1) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= n0 + n1) return;
    resum(tree + child_off, tree + node_off, t < n0 ? lo0 + t : lo1 + (t - n0));
}

__global__ __launch_bounds__(kBlock) void priority_zero_kernel(double* tree, const int64_t* index, int64_t batch, int64_t capacity) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= batch) return;
    const int64_t x = index[t];
    if (x >= 0 && x < capacity) tree[kHeaderWords + x] = 0.0;
}

__global__ __launch_bounds__(kBlock) void priority_max_kernel(double* tree, const int64_t* index, const double* priority,
                                                              int64_t batch, int64_t capacity) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double p = 0.0;                                  // 0: no contribution to the batch maximum
    if (t < batch) {
        const int64_t x = index[t];
        if (x >= 0 && x < capacity) {
            p = fmin(fmax(priority[t], TPL_PRIORITY_MIN), TPL_PRIORITY_MAX);      // NaN -> the lower bound
            atomicMax((unsigned long long*)(tree + kHeaderWords + x), (unsigned long long)__double_as_longlong(p));
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) p = fmax(p, __shfl_xor(p, off, 64));
    if ((threadIdx.x & 63) == 0 && p > 0.0)
        atomicMax((unsigned long long*)tree, (unsigned long long)__double_as_longlong(p));
}

// the level-k ancestors of the batch's leaves re-summed (index[t] >> 4k)
__global__ __launch_bounds__(kBlock) void priority_resum_index_kernel(double* tree, int64_t child_off, int64_t node_off, int shift,
                                                                      const int64_t* index, int64_t batch, int64_t capacity) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= batch) return;
    const int64_t x = index[t];
    if (x >= 0 && x < capacity) resum(tree + child_off, tree + node_off, x >> shift);
}

struct DescentArgs {
    const double* tree;
    Layout lay;
    int64_t root;                                    // offset of the root (a runtime index into `lay` would take scratch)
    int64_t capacity;
    float* prob;
};

// the slot of draw i (and its leaf priority): from the root, one 128-byte line per level.  The levels are unrolled so that
// every layout offset is a constant index into the kernel's arguments.
__device__ __forceinline__ int64_t descend(const DescentArgs& d, double u, double& leaf) {
#pragma clang fp contract(off)
    const int top = d.lay.levels - 1;
    int64_t j = 0;
    leaf = d.tree[d.lay.offset[0]];                  // a one-slot ring: the root is the leaf (overwritten below otherwise)
#pragma unroll
    for (int k = kMaxLevels - 1; k >= 1; --k) {
        if (k > top) continue;
        const double2* const line = (const double2*)(d.tree + d.lay.offset[k - 1] + j * kFan);
        double2 v[kFan / 2];
#pragma unroll
        for (int q = 0; q < kFan / 2; ++q) v[q] = line[q];
        int pick = -1, last = 0;
        double picked = 0.0, last_v = 0.0;
#pragma unroll
        for (int c = 0; c < kFan; ++c) {
            const double x = (c & 1) ? v[c >> 1].y : v[c >> 1].x;
            if (pick < 0) {
                if (u < x) {
                    pick = c;
                    picked = x;
                } else {
                    u -= x;
                }
            }
            if (x > 0.0) {
                last = c;
                last_v = x;
            }
        }
        if (pick < 0) {                              // rounding left u at or past the sum: the last non-empty child
            pick = last;
            picked = last_v;
        }
        j = j * kFan + pick;
        leaf = picked;
    }
    return j < d.capacity ? j : d.capacity - 1;      // a consistent tree never reaches a padding child; stay in the ring
}

template <typename T, int kN = 0, bool kMirror = false>      // emit_draw's form (kN = 0: 1-step)
__global__ __launch_bounds__(64 * kObsWaves) void replay_sample_prioritized_kernel(const SampleArgs p, const DescentArgs d) {
    __shared__ __attribute__((aligned(16))) uint8_t s_rows[kObsWaves][kWaveLds];
    const int lane = threadIdx.x & 63;
    const int64_t base = ((int64_t)blockIdx.x * kObsWaves + (threadIdx.x >> 6)) * 64;     // the wave's first draw
    if (base >= p.batch) return;                                                          // wave-uniform
    const int count = (int)((p.batch - base) < 64 ? (p.batch - base) : 64);
    int64_t slot = 0;
    if (lane < count) {
        const double total = d.tree[d.root];
        double leaf;
        slot = descend(d, draw_target(p.key, base + lane, p.batch, total), leaf);
        d.prob[base + lane] = (float)(leaf / total);
    }
    emit_draw<T, kN, kMirror>(p, s_rows[threadIdx.x >> 6], lane, count, base, slot);
}

unsigned blocks(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

int check_tree(const char* fn, const void* tree, int64_t capacity) {
    if (!tree) return fail_msg(TPL_ERR_ARG, "%s: null pointer", fn);
    if (capacity < 1 || capacity >= kMaxCapacity) return fail_msg(TPL_ERR_ARG, "%s: capacity must be in [1, 2^32)", fn);
    if ((uintptr_t)tree & 127u) return fail_msg(TPL_ERR_ARG, "%s: the tree must be 128-byte aligned", fn);
    return TPL_OK;
}

}  // namespace

int launch_prioritized(const char* fn, const SampleArgs& p, const void* tree, int64_t capacity, float* prob, int32_t dtype,
                       hipStream_t stream) {
    if (int e = check_tree(fn, tree, capacity)) return e;
    DescentArgs d{};
    d.tree = (const double*)tree; d.lay = layout(capacity); d.root = d.lay.offset[d.lay.levels - 1]; d.capacity = capacity;
    d.prob = prob;
    const dim3 grid((unsigned)((p.batch + 64 * kObsWaves - 1) / (64 * kObsWaves))), block(64 * kObsWaves);
    dispatch_form(p, [&](auto n, auto m) {
        constexpr int kN = decltype(n)::value;
        constexpr bool kMirror = decltype(m)::value;
        if (dtype == TPL_F32)
            hipLaunchKernelGGL((replay_sample_prioritized_kernel<float, kN, kMirror>), grid, block, 0, stream, p, d);
        else
            hipLaunchKernelGGL((replay_sample_prioritized_kernel<__hip_bfloat16, kN, kMirror>), grid, block, 0, stream, p, d);
    });
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}

}  // namespace tpl_learn

using namespace tpl_learn;

extern "C" size_t tpl_priority_tree_bytes(int64_t capacity) {
    if (capacity < 1 || capacity >= kMaxCapacity) return 0;
    return (size_t)layout(capacity).words * 8;
}

extern "C" double tpl_priority_target(uint64_t seed, uint64_t update, int64_t i, int64_t batch, double total) {
    if (batch < 1 || i < 0 || i >= batch) return -1.0;
    return draw_target(replay_key(seed, update), i, batch, total);
}

extern "C" int tpl_priority_init(void* tree, int64_t capacity, void* stream) {
    if (int e = check_tree("tpl_priority_init", tree, capacity)) return e;
    const Layout l = layout(capacity);
    TPL_LEARN_HIP(hipMemsetAsync(tree, 0, (size_t)l.words * 8, (hipStream_t)stream));
    hipLaunchKernelGGL(priority_init_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (double*)tree, capacity, (int64_t)l.levels);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}

extern "C" int tpl_priority_push(void* tree, int64_t capacity, int64_t head, int64_t count, void* stream) {
    if (int e = check_tree("tpl_priority_push", tree, capacity)) return e;
    if (head < 0 || head >= capacity) return fail_msg(TPL_ERR_ARG, "tpl_priority_push: head must be in [0, capacity)");
    if (count < 1 || count > capacity) return fail_msg(TPL_ERR_ARG, "tpl_priority_push: count must be in [1, capacity]");
    const Layout l = layout(capacity);
    const hipStream_t s = (hipStream_t)stream;
    // the leaves: [head, end0) and, when the push wraps, [0, end1)
    const int64_t end0 = head + count < capacity ? head + count : capacity, end1 = head + count - end0;
    double* const t = (double*)tree;
    hipLaunchKernelGGL(priority_push_kernel, dim3(blocks(count)), dim3(kBlock), 0, s, t, head, end0 - head, (int64_t)0, end1);
    TPL_LEARN_HIP(hipGetLastError());
    for (int k = 1; k < l.levels; ++k) {
        const int sh = 4 * k;
        int64_t lo0 = head >> sh, hi0 = ((end0 - 1) >> sh) + 1, lo1 = 0, hi1 = end1 > 0 ? ((end1 - 1) >> sh) + 1 : 0;
        if (hi1 >= lo0) {                            // the two ranges touch: one range
            lo0 = 0;
            hi1 = 0;
        }
        const int64_t n = (hi0 - lo0) + (hi1 - lo1);
        hipLaunchKernelGGL(priority_resum_range_kernel, dim3(blocks(n)), dim3(kBlock), 0, s, t, l.offset[k - 1], l.offset[k], lo0,
                           hi0 - lo0, lo1, hi1 - lo1);
        TPL_LEARN_HIP(hipGetLastError());
    }
    return TPL_OK;
}

extern "C" int tpl_priority_update(void* tree, int64_t capacity, int64_t batch, const int64_t* index, const double* priority,
                                   void* stream) {
    if (int e = check_tree("tpl_priority_update", tree, capacity)) return e;
    if (!index || !priority) return fail_msg(TPL_ERR_ARG, "tpl_priority_update: null pointer");
    if (batch < 1 || batch >= ((int64_t)1 << 31)) return fail_msg(TPL_ERR_ARG, "tpl_priority_update: batch must be in [1, 2^31)");
    if (((uintptr_t)index & 7u) || ((uintptr_t)priority & 7u))
        return fail_msg(TPL_ERR_ARG, "tpl_priority_update: index and priority must be 8-byte aligned");
    const Layout l = layout(capacity);
    const hipStream_t s = (hipStream_t)stream;
    double* const t = (double*)tree;
    hipLaunchKernelGGL(priority_zero_kernel, dim3(blocks(batch)), dim3(kBlock), 0, s, t, index, batch, capacity);
    TPL_LEARN_HIP(hipGetLastError());
    hipLaunchKernelGGL(priority_max_kernel, dim3(blocks(batch)), dim3(kBlock), 0, s, t, index, priority, batch, capacity);
    TPL_LEARN_HIP(hipGetLastError());
    for (int k = 1; k < l.levels; ++k) {
        hipLaunchKernelGGL(priority_resum_index_kernel, dim3(blocks(batch)), dim3(kBlock), 0, s, t, l.offset[k - 1], l.offset[k],
                           4 * k, index, batch, capacity);
        TPL_LEARN_HIP(hipGetLastError());
    }
    return TPL_OK;
}

extern "C" int tpl_replay_sample_prioritized(const void* ring, const void* tree, int64_t capacity, int64_t size, int64_t batch,
                                             uint64_t seed, uint64_t update, int32_t L, int32_t M, void* obs, int32_t dtype,
                                             void* next_a, void* next_b, uint8_t* action, float* reward, uint8_t* done,
                                             int64_t* index, float* prob, void* stream) {
    if (!ring || !obs || !next_a || !next_b || !action || !reward || !done || !index || !prob)
        return fail_msg(TPL_ERR_ARG, "tpl_replay_sample_prioritized: null pointer");
    if (int e = check_tree("tpl_replay_sample_prioritized", tree, capacity)) return e;
    if (size < 1 || size > capacity)
        return fail_msg(TPL_ERR_ARG, "tpl_replay_sample_prioritized: size must be in [1, capacity] (an empty ring has nothing to draw)");
    if (batch < 1) return fail_msg(TPL_ERR_ARG, "tpl_replay_sample_prioritized: batch must be positive");
    if (batch > ((int64_t)1 << 31) / TPL_OBS_DIM) return fail_msg(TPL_ERR_ARG, "tpl_replay_sample_prioritized: batch too large");
    if (L < 1 || L > 255 || M < 1 || M > 255) return fail_msg(TPL_ERR_ARG, "tpl_replay_sample_prioritized: L and M must be in [1, 255]");
    if (dtype != TPL_F32 && dtype != TPL_BF16)
        return fail_msg(TPL_ERR_ARG, "tpl_replay_sample_prioritized: unknown observation dtype %d", dtype);
    if (((uintptr_t)ring & 15u) || ((uintptr_t)obs & 15u) || ((uintptr_t)next_a & 15u) || ((uintptr_t)next_b & 15u))
        return fail_msg(TPL_ERR_ARG, "tpl_replay_sample_prioritized: ring, obs and planes must be 16-byte aligned");
    SampleArgs p{};
    p.ring = (const uint4*)ring; p.size = size; p.batch = batch; p.key = replay_key(seed, update);
    p.L = (uint32_t)L; p.M = (uint32_t)M; p.obs = obs; p.next_a = (uint4*)next_a; p.next_b = (uint4*)next_b;
    p.action = action; p.reward = reward; p.done = done; p.index = index;
    DescentArgs d{};
    d.tree = (const double*)tree; d.lay = layout(capacity); d.root = d.lay.offset[d.lay.levels - 1]; d.capacity = capacity;
    d.prob = prob;
    const dim3 grid((unsigned)((batch + 64 * kObsWaves - 1) / (64 * kObsWaves))), block(64 * kObsWaves);
    if (dtype == TPL_F32)
        hipLaunchKernelGGL(replay_sample_prioritized_kernel<float>, grid, block, 0, (hipStream_t)stream, p, d);
    else
        hipLaunchKernelGGL(replay_sample_prioritized_kernel<__hip_bfloat16>, grid, block, 0, (hipStream_t)stream, p, d);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}
