// bound.hip -- the move bound by itself: tpl_move_bound on environment states and tpl_move_bound_rows on configurations
// (include/tpl_learn.h states the rule and its proof; move_bound_cells in tpl_placement.h is the device function, the one the bounded
// placement kernels call after every move).
//
// Mapping: ONE BOARD PER LANE, blocks of 256.  A state is 32 bytes read and 8 written; a configuration is its twenty 16-bit rows, which
// a lane turns into the ten column words that the device function takes -- two hundred bit moves, made once per configuration.
#include "tpl_placement.h"

namespace tpl_learn {
namespace {

constexpr int kBoundBlock = 256;

__global__ __launch_bounds__(kBoundBlock) void move_bound_kernel(const uint4* a, const uint4* b, uint32_t n, uint32_t L, uint32_t M,
                                                                int32_t* cells_out, int32_t* spare_out) {
    const uint32_t i = blockIdx.x * kBoundBlock + threadIdx.x;
    if (i >= n) return;
    tpl::Board s;
    tpl::unpack_board(a[i], b[i], s);
    const MoveBound bound = move_bound(s, L, M);
    cells_out[i] = (int32_t)bound.cells;
    spare_out[i] = bound.spare;
}

__global__ __launch_bounds__(kBoundBlock) void move_bound_rows_kernel(const uint16_t* rows, uint32_t n, uint32_t L, int32_t* cells_out) {
    const uint32_t i = blockIdx.x * kBoundBlock + threadIdx.x;
    if (i >= n) return;
    const uint16_t* mine = rows + (size_t)i * tpl::kRows;
    uint32_t c[tpl::kCols];
#pragma unroll
    for (int x = 0; x < tpl::kCols; ++x) c[x] = 0u;
#pragma unroll
    for (int r = 0; r < tpl::kRows; ++r) {
        const uint32_t row = mine[r];
#pragma unroll
        for (int x = 0; x < tpl::kCols; ++x) c[x] |= ((row >> x) & 1u) << r;
    }
    cells_out[i] = (int32_t)move_bound_cells(c, L);
}

}  // namespace
}  // namespace tpl_learn

using namespace tpl_learn;

extern "C" int tpl_move_bound(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, int32_t* cells_out,
                              int32_t* spare_out, void* stream) {
    const char* name = "tpl_move_bound";
    if (const int rc = check_planes(name, plane_a, plane_b, n, L, M)) return rc;
    if (!cells_out || !spare_out) return fail_msg(TPL_ERR_ARG, "%s: null pointer (cells_out and spare_out are required)", name);
    if (((uintptr_t)cells_out & 3u) || ((uintptr_t)spare_out & 3u))
        return fail_msg(TPL_ERR_ARG, "%s: cells_out and spare_out must be 4-byte aligned", name);
    const uint32_t blocks = (uint32_t)((n + kBoundBlock - 1) / kBoundBlock);
    hipLaunchKernelGGL(move_bound_kernel, dim3(blocks), dim3(kBoundBlock), 0, (hipStream_t)stream, (const uint4*)plane_a,
                       (const uint4*)plane_b, (uint32_t)n, (uint32_t)L, (uint32_t)M, cells_out, spare_out);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}

extern "C" int tpl_move_bound_rows(const int16_t* rows, int64_t n, int32_t L, int32_t* cells_out, void* stream) {
    const char* name = "tpl_move_bound_rows";
    if (!rows || !cells_out) return fail_msg(TPL_ERR_ARG, "%s: null pointer", name);
    if (n < 1) return fail_msg(TPL_ERR_ARG, "%s: n must be positive", name);
    if (n >= ((int64_t)1 << 31)) return fail_msg(TPL_ERR_ARG, "%s: n too large (n must stay below 2^31)", name);
    if (L < 1 || L > 250) return fail_msg(TPL_ERR_ARG, "%s: L must be in [1, 250]", name);
    if ((uintptr_t)rows & 1u) return fail_msg(TPL_ERR_ARG, "%s: rows must be 2-byte aligned", name);
    if ((uintptr_t)cells_out & 3u) return fail_msg(TPL_ERR_ARG, "%s: cells_out must be 4-byte aligned", name);
    const uint32_t blocks = (uint32_t)((n + kBoundBlock - 1) / kBoundBlock);
    hipLaunchKernelGGL(move_bound_rows_kernel, dim3(blocks), dim3(kBoundBlock), 0, (hipStream_t)stream, (const uint16_t*)rows,
                       (uint32_t)n, (uint32_t)L, cells_out);
    TPL_LEARN_HIP(hipGetLastError());
    return TPL_OK;
}
