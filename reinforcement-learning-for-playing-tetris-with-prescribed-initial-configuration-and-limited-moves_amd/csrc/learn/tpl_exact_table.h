// tpl_exact_table.h -- the TABLE's order of the exact search (tpl_exact.h): what ntuple_exact.hip and ntuple_window.hip rank a node's
// children by.  A child is worth reward + gamma V(afterstate), what the one-ply n-tuple policy scores a first move with, read in the
// game (L, B) of the iteration.  The order carries nothing along a path -- a table's value reads the board alone -- and a child made
// again on the return is made without its value.
//
// The table is read from global memory, where it stays: a child's V is eleven gathers under a budget table and ten under a feature
// table (84 and 76 KB, which sit in L2), and up to 154 and 145 under the window forms -- the non-empty windows of the board.  One wave
// a workgroup cannot afford a copy in LDS.  The order is a template over the geometry of tpl_ntuple.h, reached through ntuple_value<S>.
// The budget geometry hands ntuple_value the board and (L, B); prune_dead is not called: bounded_move has already turned a dead child
// lost.
#pragma once

#include "tpl_exact.h"
#include "tpl_ntuple.h"

namespace tpl_learn {

// what the order reads, a member of both units' argument records at byte 32: kernel arguments, so SGPRs
struct TableOrderArgs {
    const int32_t* table;        // of the kernel's geometry
    float r_line, r_win, r_lose, gamma;
};

// what the one-ply policy scores the move with: reward, or reward + gamma V where the child runs; every product and sum rounded once
template <typename S>
__device__ __forceinline__ float child_value(const tpl::Board& s, uint32_t n_clear, uint32_t L, uint32_t B, const TableOrderArgs& p) {
#pragma clang fp contract(off)
    const bool on = s.state == tpl::ST_RUNNING;
    float v = 0.0f;
    if (on) v = ntuple_value<S>(s, L, B, p.table);
    const float reward = move_reward(p.r_line, p.r_win, p.r_lose, n_clear, s.state);
    const float later = p.gamma * v;
    return on ? reward + later : reward;
}

// The table's order: the board the move leaves, dead turned lost, with the piece the child will play as its falling piece, worth what
// the one-ply policy scores the move with.
template <typename S>
struct TableOrder {
    using Carry = NoCarry;       // a table's value reads the board alone
    const TableOrderArgs& p;
    template <typename Args>     // of a frame's argument record
    __device__ __forceinline__ explicit TableOrder(const Args& args) : p(args.order) {}
    __device__ __forceinline__ float child(const Frame<Carry>& node, uint32_t cur, const uint8_t* later, uint32_t r, uint32_t l,
                                           const tpl::ShapeWord* shape, uint32_t L, uint32_t B, tpl::Board& s, Carry&) const {
        tpl::unpack_board(node.a, node.b, s);
        s.window = cur;
        s.window_hi = 0u;
        const uint32_t n_clear = placed_move<kFeatures>(s, shape, r, l, L, B);
        bounded_move(s, L, B);
        s.window = uniform(later[0]);                          // depth d + 1 <= M: both frames' lists have that entry
        return child_value<S>(s, n_clear, L, B, p);
    }
};

}  // namespace tpl_learn
