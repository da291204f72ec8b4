// pack.hip -- the three policy images of libtetris_piclim.so (bf16: policy_mlp.hip, float32: policy_f32.hip, split:
// policy_split.hip) packed on the device, straight from the float32 parameter tensors of a PolicyMLP.
//
// The host packers (tpl_policy_pack / _f32 / _split) loop over the image's fragments and fetch, for each element, the
// weight it holds; each kernel here is that loop body with one thread per element of the image, run over the whole image
// (pads included, so no memset is needed).  The layouts are restated from the packers -- their constants live inside
// those units -- and the tests hold the two byte for byte, on random weights and on bf16 rounding ties.
//
// Arithmetic: the bf16 rounding is the packers' integer round-to-nearest-even; layer 1's 0/1 features carry halved weights
// (a multiplication by 0.5); the split image's pieces come from two float32 subtractions.  Contraction is off, so that no
// product and difference fuse into one rounding the host does not make.
#include "tpl_learn_internal.h"

namespace tpl_learn {
namespace {

constexpr int kHidden = 128, kObs = 217, kOut = 14;
constexpr int kBiasFloats = 4 * kHidden + 16;                 // 526 used + 2 pads
constexpr int kBlock = 256;

struct Params {
    const float* w[5];
    const float* b[5];
};

// --- the packers' index maps (include: policy_mlp.hip / tpl_policy.h) ---
__device__ __forceinline__ int std_feature(int k) {          // internal layer-1 feature -> observation index, -1 = pad
    if (k < 200) return (k % 20) * 10 + (k / 20);
    return k < kObs ? k : -1;
}
__device__ __forceinline__ int frag_k(int s, int g, int j) { return 32 * s + 16 * (j >> 2) + 4 * g + (j & 3); }
__device__ __forceinline__ int frag_k1(int s, int g, int j) { return 32 * s + 4 * g + (j >> 1) + 16 * (j & 1); }

__device__ __forceinline__ uint16_t bf16_rne(float f) {
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x40u);
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

// the weight element (lane, j) of the A fragment (output tile m, k-step s) of layer l (0..4) holds, scaled as the bf16 and
// split packers scale it
__device__ __forceinline__ float fragment_weight(const Params& p, int l, int m, int s, int lane, int j) {
#pragma clang fp contract(off)
    const int c = lane & 15, g = lane >> 4;
    const bool first = l == 0;
    int k = first ? frag_k1(s, g, j) : frag_k(s, g, j);
    const float scale = (first && k != 214 && k != 215) ? 0.5f : 1.0f;
    if (first) k = std_feature(k);
    const int in = first ? kObs : kHidden, rows = l == 4 ? kOut : kHidden;
    const int row = 16 * m + c;
    return (k >= 0 && k < in && row < rows) ? scale * p.w[l][(size_t)row * in + k] : 0.0f;
}

__device__ __forceinline__ float bias_value(const Params& p, int e) {     // e in [0, kBiasFloats)
    const int l = e / kHidden, k = e - l * kHidden;
    if (l < 4) return p.b[l][k];
    return k < kOut ? p.b[4][k] : 0.0f;
}

// ---- bf16 image (policy_mlp.hip): five layers of [m][s][lane][8] bf16 at kOffW*, then the float32 biases
namespace bf {
constexpr int kKs1 = 7, kKsH = 4, kMt = 8;
constexpr int kOff[6] = {0, 57344, 90112, 122880, 155648, 159744};          // W1..W5, biases
constexpr int kImageBytes = kOff[5] + kBiasFloats * 4;                       // 161,856
}  // namespace bf

__global__ __launch_bounds__(kBlock) void pack_bf16_kernel(const Params p, uint8_t* image) {
    using namespace bf;
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e < kOff[5] / 2) {                                                   // a bf16 weight
        int l = 0;
        while (e * 2 >= kOff[l + 1]) ++l;
        const int local = e - kOff[l] / 2, ks = l == 0 ? kKs1 : kKsH;
        const int j = local & 7, lane = (local >> 3) & 63, ms = local >> 9;
        ((uint16_t*)image)[e] = bf16_rne(fragment_weight(p, l, ms / ks, ms % ks, lane, j));
    } else if (e < kOff[5] / 2 + kBiasFloats) {
        const int b = e - kOff[5] / 2;
        ((float*)(image + kOff[5]))[b] = bias_value(p, b);
    }
}

// ---- float32 image (policy_f32.hip): A fragments four k-steps to a 16-byte piece per lane, [(tile, q4)][lane][q & 3]
namespace f32 {
constexpr int kKs1 = 56, kKsH = 32;
constexpr int kChunkOff[7] = {0, 57344, 114688, 180224, 245760, 311296, 319488};   // W1 tiles 0-3, 4-7, W2, W3, W4, W5; biases
constexpr int kImageBytes = kChunkOff[6] + kBiasFloats * 4;                          // 321,600
}  // namespace f32

__global__ __launch_bounds__(kBlock) void pack_f32_kernel(const Params p, uint8_t* image) {
    using namespace f32;
    const int e = blockIdx.x * kBlock + threadIdx.x;
    float* const img = (float*)image;
    if (e < kChunkOff[6] / 4) {
        int ch = 0;
        while (e * 4 >= kChunkOff[ch + 1]) ++ch;
        const int local = e - kChunkOff[ch] / 4;
        const int r = local & 3, lane = (local >> 2) & 63, tq = local >> 8;
        const int c = lane & 15, g = lane >> 4;
        float v;
        if (ch < 2) {                                                       // layer 1: k-step q of group g = feature 4q + g
            const int q = 4 * (tq % (kKs1 / 4)) + r, m = 4 * ch + tq / (kKs1 / 4);
            const int k = std_feature(4 * q + g);
            v = k >= 0 ? p.w[0][(size_t)(16 * m + c) * kObs + k] : 0.0f;
        } else {                                                            // k-step q = 4 * (input tile) + reg
            const int l = ch - 1, q4 = tq % (kKsH / 4), m = tq / (kKsH / 4);
            const int k = 16 * q4 + 4 * g + r, row = 16 * m + c;
            v = row < (l == 4 ? kOut : kHidden) ? p.w[l][(size_t)row * kHidden + k] : 0.0f;
        }
        img[e] = v;
    } else if (e < kChunkOff[6] / 4 + kBiasFloats) {
        const int b = e - kChunkOff[6] / 4;
        img[e] = bias_value(p, b);
    }
}

// ---- split image (policy_split.hip): every weight as three bf16 pieces, in ten chunks of [..][lane][8] fragments
namespace sp {
constexpr int kKs1 = 7, kKsH = 4, kMt = 8;
constexpr int kPlane1 = kMt * kKs1 * 1024, kPlane5 = kKsH * 1024, kHalfH = 3 * kMt * kKsH * 1024 / 2;
constexpr int kChunkOff[11] = {0, 57344, 114688, 172032, 221184, 270336, 319488, 368640, 417792, 466944, 479232};
constexpr int kImageBytes = kChunkOff[10] + kBiasFloats * 4;
}  // namespace sp

__device__ __forceinline__ uint16_t split_piece(float v, int piece) {     // piece 0, 1, 2 of x = x_h + x_l + x_ll
#pragma clang fp contract(off)
    float r = v;
    uint16_t out = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const uint16_t h = bf16_rne(r);
        if (i == piece) out = h;
        r -= __uint_as_float((uint32_t)h << 16);
    }
    return out;
}

__global__ __launch_bounds__(kBlock) void pack_split_kernel(const Params p, uint8_t* image) {
    using namespace sp;
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e < kChunkOff[10] / 2) {
        int ch = 0;
        while (e * 2 >= kChunkOff[ch + 1]) ++ch;
        const int local = e - kChunkOff[ch] / 2;                            // bf16 elements into the chunk
        const int j = local & 7, lane = (local >> 3) & 63, frag = local >> 9;   // 1024-byte fragment within the chunk
        int l, piece, m, s;
        if (ch < 3) {                                                       // layer 1: chunk = piece, fragment m * 7 + s
            l = 0; piece = ch; m = frag / kKs1; s = frag % kKs1;
        } else if (ch < 9) {                                                // hidden: fragment ((s & 1) * 3 + piece) * 8 + m
            l = 1 + (ch - 3) / 2;
            const int half = (ch - 3) & 1, sp3 = frag / kMt;
            m = frag % kMt; piece = sp3 % 3; s = 2 * half + sp3 / 3;
        } else {                                                            // head: fragment piece * 4 + s
            l = 4; m = 0; piece = frag / kKsH; s = frag % kKsH;
        }
        ((uint16_t*)image)[e] = split_piece(fragment_weight(p, l, m, s, lane, j), piece);
    } else if (e < kChunkOff[10] / 2 + kBiasFloats) {
        const int b = e - kChunkOff[10] / 2;
        ((float*)(image + kChunkOff[10]))[b] = bias_value(p, b);
    }
}

static_assert(bf::kImageBytes == 161856 && f32::kImageBytes == 321600 && sp::kImageBytes == 481344, "image sizes");
static_assert(sp::kChunkOff[3] == 3 * sp::kPlane1 && sp::kChunkOff[9] + 3 * sp::kPlane5 == sp::kChunkOff[10] &&
              sp::kChunkOff[4] - sp::kChunkOff[3] == sp::kHalfH, "split chunk table");

}  // namespace
}  // namespace tpl_learn

using namespace tpl_learn;

extern "C" size_t tpl_learn_image_bytes(int32_t kind) {
    switch (kind) {
        case TPL_IMAGE_BF16: return (size_t)bf::kImageBytes;
        case TPL_IMAGE_F32: return (size_t)f32::kImageBytes;
        case TPL_IMAGE_SPLIT: return (size_t)sp::kImageBytes;
        default: return 0;
    }
}

extern "C" int tpl_learn_pack(int32_t kind, const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                              const float* b3, const float* w4, const float* b4, const float* w5, const float* b5, void* image,
                              void* stream) {
    if (!w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !w4 || !b4 || !w5 || !b5 || !image)
        return fail_msg(TPL_ERR_ARG, "tpl_learn_pack: null pointer");
    const size_t bytes = tpl_learn_image_bytes(kind);
    if (bytes == 0) return fail_msg(TPL_ERR_ARG, "tpl_learn_pack: unknown image kind %d", kind);
    if ((uintptr_t)image & 15u) return fail_msg(TPL_ERR_ARG, "tpl_learn_pack: image must be 16-byte aligned");
    const Params p{{w1, w2, w3, w4, w5}, {b1, b2, b3, b4, b5}};
    // one thread per weight element (2-byte bf16 or 4-byte float) and per bias float
    const size_t elems = kind == TPL_IMAGE_F32 ? bytes / 4 : (bytes - kBiasFloats * 4) / 2 + kBiasFloats;
    const dim3 grid((unsigned)((elems + kBlock - 1) / kBlock)), block(kBlock);
    if (kind == TPL_IMAGE_BF16)
        hipLaunchKernelGGL(pack_bf16_kernel, grid, block, 0, (hipStream_t)stream, p, (uint8_t*)image);
    else if (kind == TPL_IMAGE_F32)
        hipLaunchKernelGGL(pack_f32_kernel, grid, block, 0, (hipStream_t)stream, p, (uint8_t*)image);
    else
        hipLaunchKernelGGL(pack_split_kernel, grid, block, 0, (hipStream_t)stream, p, (uint8_t*)image);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}
