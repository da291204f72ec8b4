// tpl_learn_internal.h -- what the translation units of libtpl_learn.so share: error reporting and the sampling hash.
// The learner library is separate from libtetris_piclim.so and links nothing of it: it includes the environment's device
// headers (board layout, observation stages) and takes every environment buffer as a raw device pointer.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/tpl_learn.h"

namespace tpl_learn {

// sets the calling thread's tpl_learn_last_error() message and returns `code`
int fail_msg(int code, const char* fmt, ...);

#define TPL_LEARN_HIP(call)                                                                                       \
    do {                                                                                                          \
        hipError_t e_ = (call);                                                                                   \
        if (e_ != hipSuccess) return ::tpl_learn::fail_msg(TPL_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;

__host__ __device__ inline uint64_t mix64(uint64_t z) {            // the splitmix64 finaliser
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// draw i of update `update`: position i + 1 of the splitmix64 stream keyed by (seed, update), mapped to [0, size) by the high
// half of the 64 x 64-bit product (size < 2^32).  _learn_lib.replay_indices restates it in numpy.
__host__ __device__ inline uint64_t replay_key(uint64_t seed, uint64_t update) { return mix64(seed + kGolden * (update + 1)); }

// h_i: the one 64-bit word of draw i.  The uniform slot is its product's high half, the prioritized target takes h_i >> 11 and
// the mirror coin (include/tpl_learn.h) is its bit 0.
__host__ __device__ inline uint64_t draw_hash(uint64_t key, uint64_t i) { return mix64(key + kGolden * (i + 1)); }

__host__ __device__ inline int64_t replay_slot(uint64_t key, uint64_t i, uint64_t size) {
    const uint64_t h = draw_hash(key, i);
#ifdef __HIP_DEVICE_COMPILE__
    return (int64_t)__umul64hi(h, size);
#else
    return (int64_t)(((unsigned __int128)h * size) >> 64);
#endif
}

}  // namespace tpl_learn
