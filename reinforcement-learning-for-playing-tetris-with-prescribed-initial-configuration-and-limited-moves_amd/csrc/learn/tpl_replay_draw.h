// tpl_replay_draw.h -- what the uniform and the prioritized sampler share: their arguments and the body that turns one drawn
// slot into the minibatch's outputs (replay.hip states the scheme).
#pragma once

#include <type_traits>

#include "tpl_learn_internal.h"
#include "tpl_mirror.h"
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
    // the n-step form only (tpl_replay_sample_nstep; include/tpl_learn.h states the rule); zero in the 1-step form
    int64_t capacity, head, stride;
    int32_t n_step;
    float gamma;
    float* discount;
    uint8_t* steps;
    // the mirrored form only (tpl_replay_sample_mirror): the mode (1: the coin, 2: always) and where each draw's coin goes
    int32_t mirror;
    uint8_t* mirrored;                // optional
};

// the slot k * stride after `slot` (k * stride <= age < capacity: one wrap at most)
__device__ __forceinline__ int64_t successor(const SampleArgs& p, int64_t slot, int64_t k) {
    const int64_t s = slot + k * p.stride;
    return s >= p.capacity ? s - p.capacity : s;
}

// The mirrored form's part of a draw: s, s' and the action of draw i reflected (tpl_mirror.h) where the draw's coin says so;
// returns the action.  The coin is bit 0 of the draw's hash word -- the expression the caller made the slot from, so one
// computation after inlining -- or set for every draw in mode 2.  Without kMirror nothing is compiled in.
template <bool kMirror>
__device__ __forceinline__ uint32_t reflect_draw(const SampleArgs& p, int64_t i, tpl::Board& s, uint4& na, uint4& nb, uint32_t action) {
    if constexpr (kMirror) {
        const bool flip = p.mirror == 2 || (draw_hash(p.key, (uint64_t)i) & 1u) != 0u;
        action = mirror_action(action, s.window & 7u, flip);
        mirror_board(s, flip);
        mirror_planes(na, nb, flip);
        if (p.mirrored) p.mirrored[i] = flip ? 1 : 0;
    }
    return action;
}

// Called by the whole wave: lanes < count hold draw base + lane, which took `slot`.  Gathers the record, expands s into the
// wave's LDS rows (`rows`, tpl::obs::kWaveLds bytes) and writes every output of the draw.
//
// kN = 0: the 1-step form of tpl_replay_sample and tpl_replay_sample_prioritized.  kN >= 1: the n-step form for n_step <= kN.
// Its lane issues the tail words (word 4 of the record, 16 B) of successors 1 .. n_step - 1 before it waits on any, each
// predicated on the successor's existence; both loops run over the compile-time kN, so no register array is indexed at run
// time.  Then K, R and the discount, then one dependent 32-byte load of s' from successor K - 1 (none when K = 1).
//
// kMirror: reflect_draw between unpack_board and board_to_bytes -- s is reflected before it is expanded, s' on its way out,
// the action with the drawn record's current piece; all by selects on the lane's coin.
template <typename T, int kN = 0, bool kMirror = false>
__device__ __forceinline__ void emit_draw(const SampleArgs& p, uint8_t* rows, int lane, int count, int64_t base, int64_t slot) {
    int lines_left = 0;
    if constexpr (kN == 0) {
        if (lane < count) {
            const int64_t i = base + lane;
            const uint4* const rec = p.ring + slot * 5;
            const uint4 sa = rec[0], sb = rec[1], tail = rec[4];
            uint4 na = rec[2], nb = rec[3];
            tpl::Board s;
            tpl::unpack_board(sa, sb, s);
            const uint32_t action = reflect_draw<kMirror>(p, i, s, na, nb, tail.y & 0xFFu);
            lines_left = tpl::obs::board_to_bytes(s, p.L, p.M, rows, lane);
            p.next_a[i] = na;
            p.next_b[i] = nb;
            p.reward[i] = __uint_as_float(tail.x);
            p.action[i] = (uint8_t)action;
            p.done[i] = (uint8_t)((tail.y >> 8) & 0xFFu);
            if (p.index) p.index[i] = slot;
        }
    } else if (lane < count) {
#pragma clang fp contract(off)
        const int64_t i = base + lane;
        const uint4* const rec = p.ring + slot * 5;
        const uint4 sa = rec[0], sb = rec[1], tail = rec[4];
        uint4 na = rec[2], nb = rec[3];
        int64_t age = p.head - 1 - slot;                  // transitions pushed after this one
        if (age < 0) age += p.capacity;
        uint2 t[kN];                                      // successor k: reward bits, action | done << 8
#pragma unroll
        for (int k = 1; k < kN; ++k) {                    // predicated by address: a successor that is not taken reads the
            const bool has = k < p.n_step && (int64_t)k * p.stride <= age;     // drawn record's tail again (a line already
            const uint4 w = p.ring[(has ? successor(p, slot, k) : slot) * 5 + 4];   // in flight: no new traffic)
            t[k] = make_uint2(w.x, w.y);
        }
        float ret = __uint_as_float(tail.x), g = 1.0f;
        uint32_t done = (tail.y >> 8) & 0xFFu;
        int last = 0;                                     // K - 1
#pragma unroll
        for (int k = 1; k < kN; ++k) {                    // selects, not branches: every use stays after every load
            const bool take = done == 0u && k < p.n_step && (int64_t)k * p.stride <= age;
            const float gk = g * p.gamma;
            const float rk = ret + gk * __uint_as_float(t[k].x);
            g = take ? gk : g;
            ret = take ? rk : ret;
            done = take ? (t[k].y >> 8) & 0xFFu : done;
            last = take ? k : last;
        }
        if (last > 0) {                                   // s' of successor K - 1
            const uint4* const nrec = p.ring + successor(p, slot, last) * 5;
            na = nrec[2];
            nb = nrec[3];
        }
        tpl::Board s;
        tpl::unpack_board(sa, sb, s);
        const uint32_t action = reflect_draw<kMirror>(p, i, s, na, nb, tail.y & 0xFFu);
        lines_left = tpl::obs::board_to_bytes(s, p.L, p.M, rows, lane);
        p.next_a[i] = na;
        p.next_b[i] = nb;
        p.reward[i] = ret;
        p.action[i] = (uint8_t)action;
        p.done[i] = (uint8_t)done;
        p.discount[i] = done ? 0.0f : g * p.gamma;
        p.steps[i] = (uint8_t)(last + 1);
        if (p.index) p.index[i] = slot;
    }
    tpl::obs::store_span<T>(rows, lane, count, base, lines_left, (T*)p.obs);
}

// f(std::integral_constant<int, kN>) with kN the smallest of 1, 4, 8 and 16 that holds n_step
template <typename F>
inline void dispatch_nstep(int32_t n_step, F&& f) {
    if (n_step <= 1) f(std::integral_constant<int, 1>{});
    else if (n_step <= 4) f(std::integral_constant<int, 4>{});
    else if (n_step <= 8) f(std::integral_constant<int, 8>{});
    else f(std::integral_constant<int, TPL_NSTEP_MAX>{});
}

// f(std::integral_constant<int, kN>, std::bool_constant<kMirror>) for the form that p names: p.n_step = 0 is the 1-step form
// (kN = 0), p.mirror != 0 the mirrored one
template <typename F>
inline void dispatch_form(const SampleArgs& p, F&& f) {
    auto with_n = [&](auto n) {
        if (p.mirror != 0) f(n, std::true_type{});
        else f(n, std::false_type{});
    };
    if (p.n_step == 0) with_n(std::integral_constant<int, 0>{});
    else dispatch_nstep(p.n_step, with_n);
}

// The launch of dispatch_form's form in each draw mode (replay.hip, priority.hip), for tpl_replay_sample_nstep and
// tpl_replay_sample_mirror, which check every argument but the tree's; launch_prioritized checks those (in the name of
// `fn`) before it enqueues anything.
int launch_uniform(const SampleArgs& p, int32_t dtype, hipStream_t stream);
int launch_prioritized(const char* fn, const SampleArgs& p, const void* tree, int64_t capacity, float* prob, int32_t dtype,
                       hipStream_t stream);

}  // namespace tpl_learn
