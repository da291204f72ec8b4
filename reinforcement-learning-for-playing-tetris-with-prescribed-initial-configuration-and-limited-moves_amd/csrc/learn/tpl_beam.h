// tpl_beam.h -- the frame the two beam kernels share (beam.hip: placement_beam_kernel; ntuple_beam.hip: ntuple_beam_kernel,
// ntuple_beam3_kernel; include/tpl_learn.h states the rules): the limits, a beam in LDS, the k-th distinct placement, what a
// candidate slot stands for, the selection rounds (phase B) and the place of a kept candidate in the new beam (phase C).  What a
// candidate is worth (phase A) and what a kept one stores are each kernel's own.
#pragma once

#include "tpl_placement.h"

namespace tpl_learn {

constexpr int kMaxDepth = TPL_BEAM_MAX_DEPTH;
constexpr int kMaxWidth = TPL_BEAM_MAX_WIDTH;
constexpr int kMaxPlacements = 34;                            // distinct placements of L, J and T
constexpr int kMaxCandidates = kMaxWidth * kMaxPlacements;    // 2,176
constexpr int kBeamBlock = 256;
constexpr uint32_t kNoMove = 255u;
constexpr uint32_t kSlotTop = 4095u;                          // low key word = kSlotTop - slot, never 0
static_assert(kMaxCandidates <= (int)kSlotTop, "a slot fits the low word's twelve bits");
static_assert(kMaxDepth == tpl::kWindowEntries && kMaxDepth % 4 == 0, "a path is three words of four placements");

// A beam in LDS.  `cleared` is what a node carries of its moves for the kernel's value: placement_beam_kernel keeps the rows cleared
// on the way, the n-tuple kernels the rows cleared at every ply, three bits a ply.
struct Beam {
    uint4 a[kMaxWidth], b[kMaxWidth];                         // the node's board, popped once per move made
    float value[kMaxWidth];
    uint32_t cleared[kMaxWidth];                              // rows cleared on the way (above)
    uint32_t path[kMaxWidth][kMaxDepth / 4];                  // a placement a byte, kNoMove behind the last
};

// the k-th distinct placement of piece `cur` in ascending b = 10 r + l: rotation r has location_count(cur, r) of them
__device__ __forceinline__ uint32_t nth_placement(uint32_t cur, uint32_t k, uint32_t& r, uint32_t& l) {
    const uint32_t last_rot = last_rotation(cur);
    r = 0u;
    l = k;
#pragma unroll
    for (int step = 0; step < 3; ++step) {
        const uint32_t count = location_count(cur, r);
        const bool over = l >= count && r < last_rot;
        l -= over ? count : 0u;
        r += over ? 1u : 0u;
    }
    return 10u * r + l;
}

// What slot q S + k stands for: parent q, its k-th distinct placement, and whether the parent is a finished game (then slot k = 0
// carries it and its other slots are no candidates).  Phases A and C both decode a slot here.
struct Slot { uint32_t q, k; bool finished; };
__device__ __forceinline__ Slot slot_of(const Beam& parent, uint32_t slot, uint32_t stride) {
    Slot c;
    c.q = slot / stride;
    c.k = slot - c.q * stride;
    c.finished = tpl::packed_state(parent.b[c.q]) != tpl::ST_RUNNING;
    return c;
}

// the largest of a wave's 64 values, in every lane
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long other = __shfl_xor(v, off);
        v = other > v ? other : v;
    }
    return v;
}

// Phase B: the min(width, count) largest of the `total` keys in s_key, best first, into s_sel; returns how many.  The callers'
// barrier stands between the last write of a key and this.  s_wave[round & 1] holds the largest untaken key of each wave.
__device__ __forceinline__ uint32_t select_keys(const unsigned long long* s_key, unsigned long long* s_sel,
                                                unsigned long long (*s_wave)[kBeamBlock / 64], uint32_t total, uint32_t width,
                                                uint32_t tid) {
    unsigned long long mine = 0ull;
#pragma unroll 1
    for (uint32_t slot = tid; slot < total; slot += kBeamBlock) {
        const unsigned long long key = s_key[slot];
        mine = key > mine ? key : mine;
    }
    unsigned long long wave_best = wave_max(mine);
    if ((tid & 63u) == 0u) s_wave[0][tid >> 6] = wave_best;
    __syncthreads();
    uint32_t kept = 0u;
#pragma unroll 1
    for (uint32_t round = 0; round < width; ++round) {
        unsigned long long top = 0ull;
#pragma unroll
        for (int v = 0; v < kBeamBlock / 64; ++v) top = s_wave[round & 1u][v] > top ? s_wave[round & 1u][v] : top;
        if (top == 0ull) break;                                // fewer candidates than W: the same words for every lane
        if (tid == 0) s_sel[round] = top;
        kept = round + 1u;
        if (wave_best == top) {                                // this wave's key was taken: its owner looks for its next one
            if (mine == top) {
                mine = 0ull;
#pragma unroll 1
                for (uint32_t slot = tid; slot < total; slot += kBeamBlock) {
                    const unsigned long long key = s_key[slot];
                    mine = key < top && key > mine ? key : mine;
                }
            }
            wave_best = wave_max(mine);
        }
        if ((tid & 63u) == 0u) s_wave[(round & 1u) ^ 1u][tid >> 6] = wave_best;
        __syncthreads();
    }
    return kept;
}

// Phase C: the place in the new beam of the kept key whose low word is `low`: the number of kept keys with a lower slot (the low
// word falls as the slot rises)
__device__ __forceinline__ uint32_t place_of(const unsigned long long* s_sel, uint32_t kept, uint32_t low) {
    uint32_t place = 0u;
#pragma unroll 1
    for (uint32_t e = 0; e < kept; ++e) place += (uint32_t)s_sel[e] > low ? 1u : 0u;
    return place;
}

// byte `ply` of a path: 0xFF -> b.  ply is the same for the whole block, the word is picked by selects
__device__ __forceinline__ void path_append(uint32_t (&path)[kMaxDepth / 4], uint32_t ply, uint32_t b) {
    const uint32_t put = ~((kNoMove ^ b) << (8u * (ply & 3u)));
#pragma unroll
    for (int j = 0; j < kMaxDepth / 4; ++j) path[j] &= (ply >> 2) == (uint32_t)j ? put : 0xFFFFFFFFu;
}

}  // namespace tpl_learn
