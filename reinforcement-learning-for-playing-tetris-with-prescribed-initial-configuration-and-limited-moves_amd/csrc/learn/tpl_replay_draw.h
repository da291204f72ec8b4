// tpl_replay_draw.h -- what the uniform and the prioritized sampler share: their arguments and the body that turns one drawn
// slot into the minibatch's outputs (replay.hip states the scheme).
#pragma once

#include "tpl_learn_internal.h"
#include "../tpl_observe.h"

namespace tpl_learn {

struct SampleArgs {
    const uint4* ring;
    int64_t size, batch;
    uint64_t key;
    uint32_t L, M;
    void* obs;
    uint4* next_a;
    uint4* next_b;
    uint8_t* action;
    float* reward;
    uint8_t* done;
    int64_t* index;
};

// Called by the whole wave: lanes < count hold draw base + lane, which took `slot`.  Gathers the record, expands s into the
// wave's LDS rows (`rows`, tpl::obs::kWaveLds bytes) and writes every output of the draw.
template <typename T>
__device__ __forceinline__ void emit_draw(const SampleArgs& p, uint8_t* rows, int lane, int count, int64_t base, int64_t slot) {
    int lines_left = 0;
    if (lane < count) {
        const int64_t i = base + lane;
        const uint4* const rec = p.ring + slot * 5;
        const uint4 sa = rec[0], sb = rec[1], na = rec[2], nb = rec[3], tail = rec[4];
        tpl::Board s;
        tpl::unpack_board(sa, sb, s);
        lines_left = tpl::obs::board_to_bytes(s, p.L, p.M, rows, lane);
        p.next_a[i] = na;
        p.next_b[i] = nb;
        p.reward[i] = __uint_as_float(tail.x);
        p.action[i] = (uint8_t)(tail.y & 0xFFu);
        p.done[i] = (uint8_t)((tail.y >> 8) & 0xFFu);
        if (p.index) p.index[i] = slot;
    }
    tpl::obs::store_span<T>(rows, lane, count, base, lines_left, (T*)p.obs);
}

}  // namespace tpl_learn
