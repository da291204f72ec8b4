/*
 * tpl_learn.h -- C ABI of the learner library (libtpl_learn.so): a packed replay ring on the device, its samplers (uniform,
 * prioritized, n-step, each optionally mirrored), device-side packing of a PolicyMLP's parameters into the three policy
 * images of libtetris_piclim.so, the enumeration of a board's 40 afterstates, and board features of every placement with a
 * linear placement policy on them: one ply, two plies, or a beam over the known piece window; and a learned evaluation of the board a
 * placement leaves: an n-tuple value function with its placement policy and its temporal-difference update.
 *
 * Conventions (as include/tetris_piclim.h)
 *   - every function returns 0 on success or a negative tpl_status (TPL_ERR_ARG, TPL_ERR_HIP, ...);
 *     tpl_learn_last_error() gives the message of the calling thread's last failure.
 *   - every data pointer is a DEVICE pointer; `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *     Calls only enqueue work; argument errors come back before any HIP call is made.
 *
 * Replay record (TPL_REPLAY_RECORD_BYTES = 80, 16-byte aligned), one per transition (s, a, r, done, s'):
 *   bytes  0..15  s  plane A      16..31  s  plane B         (the 32-byte state of tpl_actor_rollout's states_a / states_b)
 *         32..47  s' plane A      48..63  s' plane B
 *         64..67  reward f32      68 action u8   69 done u8   70..79 zero
 * Ring indexing: a push of a [T][n] chunk at host-side head h writes transition (t, board i) to slot (h + t*n + i) mod capacity.
 */
#ifndef TPL_LEARN_H
#define TPL_LEARN_H

#include <stddef.h>
#include <stdint.h>

#include "tetris_piclim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TPL_REPLAY_RECORD_BYTES 80

typedef enum { TPL_IMAGE_BF16 = 0, TPL_IMAGE_F32 = 1, TPL_IMAGE_SPLIT = 2 } tpl_image_kind;

/* Message of the last failure of this library on this thread ("" if none). */
const char* tpl_learn_last_error(void);

/* Bytes of one replay record (80). */
size_t tpl_replay_record_bytes(void);

/* Appends one tpl_actor_rollout chunk of `num_steps` x `n` transitions to `ring` ([capacity] records).
 * actions u8 / rewards f32 / dones u8 [num_steps][n]; states_a / states_b [num_steps][n] 16-byte words (the state BEFORE
 * each step); plane_a / plane_b: the environment's resident planes after the chunk (tpl_state_ptrs), i.e. s' of the last
 * step.  s' of step t < num_steps - 1 is the recorded state of step t + 1 -- so the environment must auto-reset: the s' of
 * a done transition is then the freshly reset board, which the done flag masks.  Transition (t, i) lands in slot
 * (head + t*n + i) mod capacity; num_steps * n must not exceed capacity (no slot is written twice in one push). */
int tpl_replay_push(void* ring, int64_t capacity, int64_t head, int32_t num_steps, int64_t n, const uint8_t* actions,
                    const float* rewards, const uint8_t* dones, const void* states_a, const void* states_b,
                    const void* plane_a, const void* plane_b, void* stream);

/* One minibatch of `batch` transitions drawn uniformly with replacement from slots [0, size) of the ring: draw i takes
 * slot tpl_replay_index(seed, update, i, size).  Writes, for every draw i:
 *   obs [batch][217] of `dtype` (TPL_F32 / TPL_BF16): the observation of s, bit-identical to tpl_expand_states (L, M);
 *   next_a / next_b [batch] 16-byte words: the planes of s' (e.g. the resident planes of a `batch`-board environment);
 *   action u8, reward f32, done u8 [batch]; index i64 [batch] the slot drawn (optional, may be NULL).
 * `obs` must be 16-byte aligned. */
int tpl_replay_sample(const void* ring, int64_t capacity, int64_t size, int64_t batch, uint64_t seed, uint64_t update,
                      int32_t L, int32_t M, void* obs, int32_t dtype, void* next_a, void* next_b, uint8_t* action,
                      float* reward, uint8_t* done, int64_t* index, void* stream);

/* The sampling hash on the host (for tests and callers that want to know the draws): splitmix64 of the stream keyed by
 * (seed, update) at position i, mapped to [0, size) by the high half of a 64 x 64-bit product.  size < 2^32. */
int64_t tpl_replay_index(uint64_t seed, uint64_t update, int64_t i, int64_t size);

/* Device-side tpl_policy_pack / tpl_policy_pack_f32 / tpl_policy_pack_split: the ten float32 parameter arrays of
 * Model(217, 14) (device pointers, torch layout) -> the image of that kind (device, 16-byte aligned), byte-identical to the
 * host packer's.  tpl_learn_image_bytes(kind) equals tpl_policy_image_bytes[_f32|_split](). */
size_t tpl_learn_image_bytes(int32_t kind);
int tpl_learn_pack(int32_t kind, const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                   const float* b3, const float* w4, const float* b4, const float* w5, const float* b5, void* image,
                   void* stream);

/* Prioritized replay (proportional, Schaul et al. 2016): a 16-ary float64 sum tree over the ring's slots, on the device.
 *
 * Tree image, tpl_priority_tree_bytes(capacity) bytes, 128-byte aligned; every word is a little-endian f64 / i64:
 *   bytes 0..127   header: word 0 the running maximum priority (f64, 1.0 after init), word 1 the capacity (i64),
 *                  word 2 the number of levels (i64), words 3..15 zero
 *   level 0        the `capacity` leaf priorities, one per ring slot (f64; an unfilled slot holds 0)
 *   level k >= 1   n_k = ceil(n_{k-1} / 16) nodes: node j is children 16j .. 16j+15 of level k-1 added left to right in
 *                  float64, one rounding per add; a missing child counts as 0.  The top level has one node, the root: the total.
 *   Level 0 starts at byte 128, level k + 1 at the start of level k plus 8 * n_k rounded up to 128 bytes, so the 16 children
 *   of a node are one 128-byte line; the padding is zero.  A draw reads ceil(log16 capacity) lines.
 *
 * Push: every slot of [head, head + count) mod capacity gets the running maximum.  Update: the priorities are clamped to
 * fmin(fmax(p, 1e-12), 1e30) (NaN -> 1e-12); a slot named more than once in one batch takes the largest of its new
 * priorities; the running maximum becomes max(old, max of the batch).  Indices outside [0, capacity) are ignored.
 * Draw i of a prioritized minibatch (stratified): u_i = ((i + U_i) * total) / batch in float64, U_i = (h_i >> 11) * 2^-53 with
 * h_i the splitmix64 value tpl_replay_index maps; from the root, take the first child k with u < c_k, else u -= c_k; if no
 * child is taken (rounding), the last child with c_k > 0.  Zero-priority slots are never drawn. */
#define TPL_PRIORITY_HEADER_BYTES 128
#define TPL_PRIORITY_FANOUT 16
#define TPL_PRIORITY_MIN 1e-12
#define TPL_PRIORITY_MAX 1e30

/* Bytes of the tree of a ring of `capacity` slots (0 unless capacity is in [1, 2^32)). */
size_t tpl_priority_tree_bytes(int64_t capacity);

/* Zeroes the tree and writes its header (running maximum 1.0). */
int tpl_priority_init(void* tree, int64_t capacity, void* stream);

/* The slots of one tpl_replay_push at `head` of `count` transitions get the running maximum; their ancestors are re-summed. */
int tpl_priority_push(void* tree, int64_t capacity, int64_t head, int64_t count, void* stream);

/* Priority write-back of one minibatch: index i64 [batch], priority f64 [batch] (already (|delta| + eps)^alpha). */
int tpl_priority_update(void* tree, int64_t capacity, int64_t batch, const int64_t* index, const double* priority,
                        void* stream);

/* tpl_replay_sample with the draws taken from the tree instead of uniformly: the same outputs, `index` required, and
 * prob f32 [batch] = (float)(leaf / total) of each draw. */
int tpl_replay_sample_prioritized(const void* ring, const void* tree, int64_t capacity, int64_t size, int64_t batch,
                                  uint64_t seed, uint64_t update, int32_t L, int32_t M, void* obs, int32_t dtype, void* next_a,
                                  void* next_b, uint8_t* action, float* reward, uint8_t* done, int64_t* index, float* prob,
                                  void* stream);

/* u_i of draw i on the host (for tests): ((i + U_i) * total) / batch; -1 if batch < 1, i < 0 or i >= batch. */
double tpl_priority_target(uint64_t seed, uint64_t update, int64_t i, int64_t batch, double total);

/* n-step returns.  Every push of a [T][stride] chunk advances the head by T * stride, so global transition g = tau * stride + i
 * (step tau, board i) lives in slot g mod capacity and the same board's next transition is `stride` slots later.  For a drawn
 * slot j of a ring with host-side `head` and filled `size` (size < capacity only with head == size):
 *   age(j) = (head - 1 - j) mod capacity               transitions pushed after slot j
 *   successor k of j = slot (j + k * stride) mod capacity, which exists iff k * stride <= age(j)
 *   K: go k = 0, 1, ... while k < n_step and successor k exists; stop AFTER the first record with done != 0 (it is included),
 *      so 1 <= K <= n_step
 *   R (float32, no fused multiply-add): g_0 = 1, R = r_0; for k = 1 .. K-1: g_k = g_{k-1} * gamma, R = R + g_k * r_k, each
 *      product and each sum rounded once
 *   done = the done byte of record K-1;  discount = 0 if done, else g_{K-1} * gamma (float32: gamma^K as an iterated product)
 *   s' = the s' planes of successor K-1;  obs (of s), action, index and prob: those of slot j;  steps = K.
 * At n_step = 1 the outputs are tpl_replay_sample's / tpl_replay_sample_prioritized's bit for bit, with discount gamma or 0. */
#define TPL_NSTEP_MAX 16

/* One minibatch with n-step returns.  tree == NULL: draw i takes tpl_replay_sample's slot (index optional, prob must be NULL);
 * otherwise tpl_replay_sample_prioritized's (index and prob required).  ret, discount f32 and done, steps u8 [batch] are
 * required.  Refused besides the two samplers' own checks: n_step outside [1, TPL_NSTEP_MAX], gamma outside [0, 1] or NaN,
 * stride outside [1, capacity], head outside [0, capacity), size < capacity with head != size. */
int tpl_replay_sample_nstep(const void* ring, const void* tree, int64_t capacity, int64_t size, int64_t head, int64_t stride,
                            int32_t n_step, float gamma, int64_t batch, uint64_t seed, uint64_t update, int32_t L, int32_t M,
                            void* obs, int32_t dtype, void* next_a, void* next_b, uint8_t* action, float* ret, float* discount,
                            uint8_t* done, uint8_t* steps, int64_t* index, float* prob, void* stream);

/* Mirror symmetry.  The game is exactly symmetric under the left-right reflection: reflect the board, swap L <-> J and S <-> Z in
 * the piece list, reflect the action, and the move gives the reflected board with the same lines cleared, reward and ending.
 *
 * Mirror of a 32-byte state (planes A, B): column word x <-> column word 9 - x; each of the twelve 3-bit window entries p
 * (the four bits kept in B.z included) becomes pi(p), pi = TPL_PIECE_MIRROR = [0, 2, 1, 3, 5, 4, 6, 7] (ids I0 L1 J2 T3 S4 Z5
 * O6, 7 = none); lines, moves, state, slot and the unused bit 31 of B.y stay.  An involution on all 256 bits.
 * Mirror of an action a (u8) taken in state s: r = (a / 10) & 3, l = a % 10, w = the width of shape table entry [cur(s)][r]
 * with cur(s) = window entry 0 of s (for cur = 7 the table's entry as it stands: O's), l_eff = min(l, 10 - w),
 *   a' = 10 * ((4 - r) & 3) + (10 - w - l_eff)            always below 40; mirroring twice gives 10 * r + l_eff.
 * Mirror of the observation: cell 10 y + x <-> cell 10 y + 9 - x, 200 + p -> 200 + pi(p), 207 + p -> 207 + pi(p) (p < 7),
 * features 214..216 fixed -- the observation of the mirrored state is this permutation of the observation of the state, bit
 * for bit in float32 and bf16.
 * A mirrored draw: obs is that of the mirrored s, next_a / next_b the mirrored s' (n-step: the s' of the last record taken),
 * action the drawn record's, mirrored with the drawn record's cur.  The return, done, discount, steps, index and prob are
 * those of the plain draw: priorities belong to the slot, mirrored or not.
 * `mirror`: TPL_MIRROR_NEVER; TPL_MIRROR_COIN: draw i is mirrored iff bit 0 of h_i, the splitmix64 word at position i + 1 of the
 * stream keyed by (seed, update) that tpl_replay_index maps and tpl_priority_target takes its U_i from (which use its top bits);
 * TPL_MIRROR_ALWAYS. */
typedef enum { TPL_MIRROR_NEVER = 0, TPL_MIRROR_COIN = 1, TPL_MIRROR_ALWAYS = 2 } tpl_mirror_mode;
#define TPL_PIECE_MIRROR {0, 2, 1, 3, 5, 4, 6, 7}

/* One minibatch in any of the four draw forms, mirrored as `mirror` says.  n_step >= 1: tpl_replay_sample_nstep's arguments,
 * checks and outputs.  n_step = 0: the 1-step form of tpl_replay_sample (tree == NULL) / tpl_replay_sample_prioritized, whose
 * outputs it writes (`ret` is their reward); head, stride and gamma are not read and discount and steps must be NULL.
 * mirrored u8 [batch] (optional, may be NULL): 1 where draw i was reflected, else 0 (all 0 at TPL_MIRROR_NEVER).
 * At TPL_MIRROR_NEVER every output is the corresponding existing entry's byte for byte (the same kernels). */
int tpl_replay_sample_mirror(const void* ring, const void* tree, int64_t capacity, int64_t size, int64_t head, int64_t stride,
                             int32_t n_step, float gamma, int64_t batch, uint64_t seed, uint64_t update, int32_t L, int32_t M,
                             void* obs, int32_t dtype, void* next_a, void* next_b, uint8_t* action, float* ret, float* discount,
                             uint8_t* done, uint8_t* steps, int64_t* index, float* prob, int32_t mirror, uint8_t* mirrored,
                             void* stream);

/* The mirror of `count` states: planes a / b [count] 16-byte words -> out_a / out_b (which may be a / b themselves).  With
 * action and out_action u8 [count] (both or neither; out_action may be action): out_action[i] = the mirror of action[i] taken
 * in state i as given.  The device function is the samplers'. */
int tpl_mirror_states(int64_t count, const void* a, const void* b, void* out_a, void* out_b, const uint8_t* action,
                      uint8_t* out_action, void* stream);

/* Afterstates.  For a 32-byte state s (planes A, B) and each of the 40 actions a = 10 r + l (r = a / 10 in 0..3, l = a % 10), what
 * playing a from s leaves -- without touching s.  Outputs are laid out [n][40]: pair (i, a) at index 40 i + a.
 *
 * Finished board (state(s) != running): the afterstate is s bit for bit, reward 0, done 1, cleared 0 -- a frozen board of tpl_step.
 * Running board: the move of the environment's device code as it stands (move_board(s, shape, r, l, L, M, topout) of
 * csrc/tpl_device.h: on a top-out the board and moves stay, the state becomes lost), then the piece window popped by one entry
 * WITHOUT a refill (next_window(s, false, 0): a 36-bit shift, zeros enter at the top).  cleared = the rows cleared (0..4),
 * done = (state' != running), reward = r_line * cleared (+ r_win when the move wins) (+ r_lose when it loses) in float32: one
 * rounded multiply and at most one rounded add, never fused (0.1f * 3 + x differs in the last bit when fused) -- step_reward's
 * rule.  The slot bit and the unused bit 31 of B.y are carried over.
 * canonical[a] = 10 * (r mod nrot(cur)) + min(l, 10 - w(cur, r)): cur = window entry 0 of s, nrot = TPL_PIECE_ROTATIONS,
 * w = the width of shape table entry [cur][r] as the table stands (so cur = 7 reads O's).  Two actions with one canonical value
 * are the same placement -- the right clamp and `rotations % len` alias 6 to 31 of the 40 -- and a == canonical[a] marks the
 * distinct ones: 17 for I, 34 for L, J and T, 17 for S and Z, 9 for O.  canonical is computed for finished boards too.  (So a
 * uniform draw over 0..39 is not uniform over placements: it plays the right-most location most often.  tpl_ntuple_act below
 * explores uniformly over the DISTINCT placements.)
 *
 * Relation to the step: for a running board the afterstate is what a non-auto-reset tpl_step with the same reward parameters
 * leaves in the planes, and reward and done are the step's -- with ONE exception: on the move at which the environment refills
 * the window ((moves + 1) % 10 == 0 with a pool loaded) window entries 2..11 (bits 6..31 of B.w, bits 28..31 of B.z) are the
 * pool's next piece word there and the shifted-down rest here.  Entries 0 and 1 -- all that the observation reads -- are equal
 * by construction of the piece words.  So AN AFTERSTATE'S WINDOW IS GOOD FOR `cur` AND `next` ONLY: a search deeper than one
 * ply must start from environment states. */
#define TPL_PIECE_ROTATIONS {2, 4, 4, 4, 2, 2, 1, 1}

/* The 40 afterstates of each of `n` states: plane_a / plane_b [n] 16-byte words (read only) -> out_a / out_b [n][40] 16-byte
 * words (both or neither; e.g. the resident planes of a 40 n-board environment, tpl_state_ptrs), reward f32, done u8, cleared u8,
 * canonical u8 [n][40], each optional; at least one output.  Refused before any HIP call: n < 1, 40 n >= 2^31, a NULL or
 * misaligned (16 bytes) plane pointer, only one of out_a / out_b, no output at all, L outside [1, 250] or M outside
 * [1, 254] (tpl_create's limits: lines + 4 must fit the eight bits of B.z that hold it). */
int tpl_afterstates(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line, float r_win,
                    float r_lose, void* out_a, void* out_b, float* reward, uint8_t* done, uint8_t* cleared, uint8_t* canonical,
                    void* stream);

/* canonical[action] for current piece `cur` (0..7) on the host, for tests; -1 if cur or action (0..39) is out of range. */
int32_t tpl_canonical_action(int32_t cur, int32_t action);

/* Placement features and a linear placement policy on them (csrc/learn/heuristic.hip).
 *
 * phi(s, a), for a 32-byte state s and action a = 10 r + l, is TPL_NUM_FEATURES = 12 small non-negative integers.  Finished board
 * (state(s) != running): all twelve are 0.  Running board: move_board(s, shape, r, l, L, M, topout) exactly as tpl_afterstates
 * makes it (a top-out leaves the board as it was); n = the rows cleared, state' the new state, c_x the column words afterwards
 * (bit r = row r, row 0 = top).  "Filled" and "empty" speak of this board after the clear;
 * h_x = 20 - (row of the top-most filled cell of column x), 0 for an empty column.
 *    0 cleared             n (0..4)
 *    1 won                 1 if state' = won
 *    2 lost                1 if state' = lost at the limit or topped out
 *    3 holes               empty cells with at least one filled cell above them in their column
 *    4 aggregate_height    sum_x h_x
 *    5 max_height          max_x h_x
 *    6 bumpiness           sum_{x = 0..8} |h_x - h_{x+1}|
 *    7 row_transitions     each of the 20 rows read wall, x = 0..9, wall with the walls filled: adjacent pairs of different
 *                          occupancy (an empty row gives 2)
 *    8 column_transitions  per column the adjacent pairs (row r, row r + 1), r = 0..18, of different occupancy, plus 1 if row 19
 *                          is empty (the floor is filled; nothing is counted above row 0)
 *    9 wells               sum_x d_x (d_x + 1) / 2, d_x = max(0, min(h_{x-1}, h_{x+1}) - h_x) with h_{-1} = h_10 = 20
 *   10 rows_with_holes     rows that contain at least one hole
 *   11 hole_depth          over the columns that have a hole: the filled cells of the column above its top-most hole
 * Every value fits an int16.  These twelve describe the board a move leaves; the two features of the move itself, landing height and
 * eroded cells, are features 12 and 13 of the 14-feature form below (tpl_placement_*_move).
 *
 * Score: with weights w[12] (float32), score = w_0 phi_0 + w_1 phi_1 + ... + w_11 phi_11 from left to right in float32: every
 * phi_f converts exactly, every product and every sum is rounded once, never fused (move_reward's discipline).
 * Choice: the arg-max of the score over the distinct placements (a == canonical[a]), the lowest a on ties (-0 and +0 tie).  A
 * finished board so gets action 0 and the score of twelve zeros.  THE WEIGHTS MUST BE FINITE (device memory cannot be checked
 * here), and of a size that no score overflows: the choice among scores that are not numbers is unspecified, though it is still
 * one distinct placement per board.
 * Population: board i uses weight row i / boards_per_member of a [P][12] array, P = ceil(n / boards_per_member); the last member
 * may be short; boards_per_member >= n is the single-policy case.
 * With w = (r_line, r_win, r_lose, 0, ..., 0) the score is tpl_afterstates' reward (adding a zero changes no value, and at most
 * one of won / lost is set), bit for bit wherever that reward is not -0: the choice is the best immediate reward's. */
#define TPL_NUM_FEATURES 12

/* phi of all 40 actions of each of `n` states: plane_a / plane_b [n] 16-byte words (read only) -> features i16 [n][40][12], one
 * contiguous 24-byte record per pair (8-byte aligned, written with 8-byte stores), and canonical u8 [n][40] (optional, as
 * tpl_afterstates').  Refused before any HIP call: n < 1, 40 n >= 2^31, a NULL or misaligned (16 bytes) plane pointer, features
 * NULL or not 8-byte aligned, L outside [1, 250] or M outside [1, 254]. */
int tpl_placement_features(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, int16_t* features,
                           uint8_t* canonical, void* stream);

/* The chosen action of each of `n` states in one kernel (features, score and arg-max stay in registers and LDS: 32 bytes read
 * and 1 or 5 written per board): weights f32 [P][12] (16-byte aligned), action u8 [n], score f32 [n] (optional: the chosen
 * action's score).  Refused before any HIP call: tpl_placement_features' plane, n, L and M checks, weights or action NULL,
 * boards_per_member < 1, weights not 16-byte or score not 4-byte aligned. */
int tpl_placement_act(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const float* weights,
                      int64_t boards_per_member, uint8_t* action, float* score, void* stream);

/* Two plies with the known next piece.  Window entry 1 of a state is the piece after the current one, and an afterstate's window is
 * good for exactly these two entries (above), so two plies is the deepest search from an AFTERSTATE that is exact without a pool
 * (tpl_placement_beam below goes deeper from environment states).
 * For a state s with weight row w[12], cur = window entry 0 of s, nxt = window entry 1:
 *   Finished board (state(s) != running): action 0, second 255, score = the score of twelve zeros -- the one-ply rule.
 *   Running board: for every distinct first placement a (a == canonical(cur, a)), move_board(s, a) exactly as tpl_afterstates makes
 *   it gives n1 rows cleared, state1 and the board s1, whose window is popped by one entry, so that its current piece is nxt.
 *     state1 != running (the first move ends the game): psi(a) = phi(s, a), the twelve one-ply features; V(a) = score(w, psi(a));
 *       second(a) = 255.
 *     otherwise, for every distinct second placement b (b == canonical(nxt, b)), move_board(s1, b) gives n2, state2 and the board s2:
 *       psi(a, b) = (n1 + n2, won2, lost2, features 3..11 of s2) -- feature 0 is 0..8 and converts exactly;
 *       score(a, b) = the score rule above on psi(a, b): left to right in float32, every product and sum rounded once, never fused;
 *       V(a) = max over b of score(a, b); second(a) = the lowest b at that maximum (-0 and +0 tie; V(a) is that b's score).
 *   Choice: action = the lowest a at the maximum of V, second = second(action), score = V(action).
 * nxt = 7 ("none": the piece list ends after cur) is what move_board and the shape table make of it: O's entry, nine placements.
 * The weight rows of a population and THE FINITENESS CAVEAT are tpl_placement_act's.
 * After a non-auto-reset step with `action`, a board that still runs has a one-ply choice (tpl_placement_act, w_0 = 0) of `second`
 * with the same score: the second ply is the one-ply rule on the board the step leaves.
 *
 * One kernel: 32 bytes read per board, action u8 [n], second u8 [n] (optional), score f32 [n] (optional) written; an output that is
 * not given is not written.  Refused before any HIP call: everything tpl_placement_act refuses. */
int tpl_placement_search(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const float* weights,
                         int64_t boards_per_member, uint8_t* action, uint8_t* second, float* score, void* stream);

/* Beam search over the known piece window.  An afterstate's window is good for two entries, but an ENVIRONMENT STATE carries more:
 * at moves = m the first 12 - (m mod 10) entries of its window are the episode's true next pieces (the refill at a multiple of ten
 * loads a word whose first two entries are the two that were left) -- never fewer than three, twelve right after a reset or a
 * refill.  tpl_placement_beam searches them with a beam: exhaustive depth costs 34^D moves, a beam of width W 34 (1 + W (D - 1)).
 *
 * For a state s with weight row w[12], a depth D in [1, TPL_BEAM_MAX_DEPTH] and a width W in [1, TPL_BEAM_MAX_WIDTH]:
 *   Finished board (state(s) != running): action 0, every plan entry 255, score = the score of twelve zeros -- the one-ply rule.
 *   Running board: the effective depth is d = min(D, 12 - moves(s) mod 10), from the state's bits as they stand (pool or not).
 *   A NODE is a board (its window popped once per move made, by next_window(s, false, 0) as tpl_afterstates does), the rows cleared
 *   on the way c, the path of placements, and a value.  Beam_0 is the root alone (c = 0, empty path).
 *   For ply j = 1 .. d the CANDIDATES are listed in order: over the nodes q = 0, 1, ... of Beam_{j-1} in their stored order,
 *     a node whose state is not running gives one candidate, itself, value and path unchanged (index 0 within the node);
 *     a running node gives one candidate per distinct placement b of its current piece (b == canonical(cur, b), cur = window entry 0
 *     of the node; cur = 7 is what move_board and the shape table make of it: O's nine placements) in ascending b: the child is
 *     move_board(node, b) exactly as tpl_afterstates makes it, then the pop; with n the rows it cleared,
 *       psi = (c + n, won, lost, features 3..11 of the child's board)      -- feature 0 is at most 48 and converts exactly
 *       value = the score rule above on psi: left to right in float32, every product and sum rounded once, never fused;
 *     the child's c is c + n and its path the node's with b appended.
 *   Candidates are ordered by (value descending, candidate index ascending); -0 and +0 tie.
 *   Beam_j = the min(W, count) best candidates STORED IN CANDIDATE ORDER -- a stable compaction, not a sort -- so every beam is in
 *   lexicographic order of its paths, and ties fall as in tpl_placement_act and tpl_placement_search.
 *   Choice: the best node of Beam_d under the same order: action = the first placement of its path, score = its value,
 *   plan[0 .. D) = its path padded with 255.
 * Consequences:
 *   D = 1, any W: action and score are tpl_placement_act's, bit for bit.
 *   D = 2, W >= 34: action, plan[1] and score are tpl_placement_search's action, second and score, bit for bit, on every state.
 *   Playing `plan` move by move on a non-auto-reset environment without a pool (no refill: the same pop) reaches a board whose psi
 *   (rows cleared in total, won, lost, features 3..11) scores `score` under w, bit for bit.
 * The weight rows of a population and THE FINITENESS CAVEAT are tpl_placement_act's.  Boards that different paths reach are not
 * merged, and the pool is never read for pieces beyond the window. */
#define TPL_BEAM_MAX_DEPTH 12
#define TPL_BEAM_MAX_WIDTH 64

/* One kernel, a workgroup per board, both beams and the candidate keys in LDS (csrc/learn/beam.hip): 32 bytes read per board,
 * action u8 [n], plan u8 [n][depth] (optional), score f32 [n] (optional) written; an output that is not given is not written.
 * Refused before any HIP call: everything tpl_placement_act refuses, depth outside [1, TPL_BEAM_MAX_DEPTH], width outside
 * [1, TPL_BEAM_MAX_WIDTH]. */
int tpl_placement_beam(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const float* weights,
                       int64_t boards_per_member, int32_t depth, int32_t width, uint8_t* action, uint8_t* plan,
                       float* score, void* stream);

/* A whole-game beam solver for prescribed configurations.  tpl_placement_beam plans from an environment state, which shows at most
 * twelve pieces.  A prescribed CONFIGURATION is a board and the whole list of its pieces, so the same beam can run through all of a
 * game: tpl_placement_solve does, stops at the first ply at which it sees a win, and returns the moves.
 *
 * For a configuration -- rows[20] (16-bit words, bit x = column x, row 0 = top) and pieces[M + 1] --, one weight row w[12] and a
 * width W in [1, TPL_BEAM_MAX_WIDTH], in tpl_placement_beam's terms:
 *   Beam_0 is the ROOT alone, c = 0, empty path: the state a full reset deals from the configuration -- 0 lines, 0 moves, running.
 *   For ply j = 1 .. M: the current piece of every running node of Beam_{j-1} is pieces[j - 1] & 7, TAKEN FROM THE LIST (a popped
 *     window is good for its twelve entries only; the features never read the entries behind the current piece, and they are no part
 *     of this rule).  The CANDIDATES are listed exactly as tpl_placement_beam lists them: over the nodes in their stored order, a
 *     finished node gives itself, a running node one child per distinct placement b of the current piece in ascending b, each
 *     move_board(node, b) as tpl_afterstates makes it; with n the rows it cleared,
 *       psi = (c + n, won, lost, features 3..11 of the child's board)      -- c + n is at most 253 and converts exactly
 *       value = the score rule on psi: left to right in float32, every product and sum rounded once, never fused.
 *     Candidates are ordered by (value descending, candidate index ascending); -0 and +0 tie.
 *     best_value[j - 1] = the value of the candidate that comes first in that order.
 *     STOP ON A WIN: if ANY candidate of ply j is won -- all candidates are looked at, BEFORE the cut, so a won candidate is never lost
 *     to the cut and j is the first ply at which this beam sees a win -- the search ends: solved = 1, solution_len = j, and the
 *     solution is the path of the won candidate that comes first in the order.
 *     Otherwise Beam_j = the min(W, count) best candidates STORED IN CANDIDATE ORDER (the stable compaction).  If no node of Beam_j
 *     runs, the search ends with solved = 0, solution_len = 0 and a path of 255s.
 *   At ply M every child is finished (the move limit), so the search ends by then.
 *   best_value is +0 beyond the plies that were run.
 * solved = 0 MEANS THAT THIS BEAM, WITH THESE WEIGHTS AT THIS WIDTH, FOUND NO WIN.  IT DOES NOT MEAN THAT THE CONFIGURATION HAS NONE:
 * nothing here proves a configuration unwinnable.
 * Consequences:
 *   1. Playing the solution move by move from the configuration ends won after exactly solution_len moves, on any correct
 *      implementation of the game.
 *   2. For j <= min(12, plies run) and an environment freshly reset to the configuration, best_value[j - 1] is the score of
 *      tpl_placement_beam at depth j and width W, bit for bit: the same nodes, the same candidates, and the best candidate is always
 *      kept.  Where the candidate that comes first at the winning ply j <= 12 is itself won, the beam's plan[0 .. j) is the solution.
 *   3. At any fixed W the result is a function of the inputs alone; nothing is written but the outputs.
 * THE FINITENESS CAVEAT of the weights is tpl_placement_act's.  The piece ids cannot be checked on the device: they are masked to
 * three bits as move_board masks them (7 plays O's entry); the caller checks them where it can (load_configs' rule: 0..6).
 *
 * One kernel, a workgroup per configuration in tpl_placement_beam's frame (csrc/learn/solve.hip); the paths are kept as a tape of
 * (parent, placement) per ply and node in LDS and walked back at the winning ply.  rows i16 [n][20] and pieces u8 [n][M + 1] are read;
 * solved u8 [n], solution_len i32 [n], actions u8 [n][M] (the solution's placements b = 10 r + l, 255 behind the end) and best_value
 * f32 [n][M] (optional; an output that is not given is not written) are written in full.
 * Refused before any HIP call: n < 1, n >= 2^31 (the grid), a NULL rows, pieces, weights, solved, solution_len or actions, weights
 * not 16-byte aligned, solution_len or best_value not 4-byte aligned, rows not 2-byte aligned, L outside [1, 250] or M outside
 * [1, 254], width outside [1, TPL_BEAM_MAX_WIDTH]. */
int tpl_placement_solve(const int16_t* rows, const uint8_t* pieces, int64_t n, int32_t L, int32_t M, const float* weights,
                        int32_t width, uint8_t* solved, int32_t* solution_len, uint8_t* actions, float* best_value, void* stream);

/* The 14-feature form: the twelve board features and the two features of the move itself -- the Dellacherie / BCTS controller's
 * landing height and eroded piece cells.  A move budget rewards clearing rows soon and low down; these two measure that, and the
 * twelve cannot: they see the board a move leaves, not how the piece came to lie in it.
 *
 * For a running state s and action a = 10 r + l, `drop` is move_board's drop: the row of the piece's top-most mask row after the fall,
 * taken from the column tops under the piece (not a cell-by-cell slide: a piece never slips under an overhang), and h the height of
 * shape table entry [cur][r].  A move that does not top out puts the piece's four cells into rows drop .. drop + h - 1; of those rows,
 * the ones that are full after the lock are cleared, n of them (feature 0).
 *   12 landing_height      39 - 2 drop - h: twice the height of the piece's centre above the floor, in half rows (0..38).  An I piece
 *                          flat on an empty floor gives 0, an O piece on an empty floor 1.
 *   13 eroded_cells        n x (the number of the piece's four cells that lay in cleared rows) (0..16).  A vertical I piece that
 *                          clears four rows gives 16.
 * Both are 0 for a top-out (the move is not made) and for a finished board, as the other twelve are.
 * phi14(s, a) = features 0..11 as above, then these two: TPL_NUM_MOVE_FEATURES = 14 values.
 * Weights: float32 [P][TPL_MOVE_WEIGHT_STRIDE = 16], 16-byte aligned; entries 14 and 15 of a row are never read.
 * Score: the score rule carried two terms further: w_0 phi_0 + ... + w_13 phi_13 from left to right in float32, every product and
 * every sum rounded once, never fused.  The arg-max, the ties, the rows of a population and THE FINITENESS CAVEAT are unchanged.
 * With w_12 = w_13 = 0 (and finite scores) every choice is the 12-feature form's: the two added terms are +-0, and adding a zero
 * changes no value but the sign of a zero, which the order does not see.
 *
 * Deeper than one ply both features ACCUMULATE ALONG THE PATH exactly as `cleared` does:
 *   two plies   psi(a, b) = (n1 + n2, won2, lost2, features 3..11 of s2, land1 + land2, erod1 + erod2); where the first move ends
 *               the game psi(a) = phi14(s, a).
 *   beam, solve a node carries the sums of its path, a child's psi has its node's sums plus its move's; a finished node passes on
 *               unchanged and a finished root scores fourteen zeros.  The landing sum is at most 254 * 38 and the eroded sum at most
 *               4 (L + 3), so the kernels keep (cleared, landing, eroded) in 8 + 14 + 10 bits of the one word a node had for `cleared`.
 * Everything else -- candidates, order, the stable compaction, the solver's stop at the first won candidate, the tape, best_value,
 * the consequences listed with each rule -- is the 12-feature rule word for word, with `psi` read as above. */
#define TPL_NUM_MOVE_FEATURES 14
#define TPL_MOVE_WEIGHT_STRIDE 16

/* tpl_placement_features in the 14-feature form: features i16 [n][40][16], one contiguous 32-byte record per pair (16-byte aligned,
 * written with 16-byte stores), entries 14 and 15 zero; entries 0..11 and canonical are tpl_placement_features'.  Refused before any
 * HIP call: what tpl_placement_features refuses, with features not 16-byte aligned in place of its 8. */
int tpl_placement_features_move(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, int16_t* features,
                                uint8_t* canonical, void* stream);

/* tpl_placement_act, tpl_placement_search, tpl_placement_beam and tpl_placement_solve in the 14-feature form: the same arguments,
 * outputs and checks, with weights f32 [P][16] (tpl_placement_solve_move: one row, [16], of which 14 are read).  Each is the same
 * kernel body as its twin, instantiated on the other feature set (csrc/learn/tpl_placement.h: placed_move). */
int tpl_placement_act_move(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const float* weights,
                           int64_t boards_per_member, uint8_t* action, float* score, void* stream);
int tpl_placement_search_move(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const float* weights,
                              int64_t boards_per_member, uint8_t* action, uint8_t* second, float* score, void* stream);
int tpl_placement_beam_move(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const float* weights,
                            int64_t boards_per_member, int32_t depth, int32_t width, uint8_t* action, uint8_t* plan,
                            float* score, void* stream);
int tpl_placement_solve_move(const int16_t* rows, const uint8_t* pieces, int64_t n, int32_t L, int32_t M, const float* weights,
                             int32_t width, uint8_t* solved, int32_t* solution_len, uint8_t* actions, float* best_value,
                             void* stream);

/* The move bound.  The game is named after its move limit; this is the one rule here that reasons about it.  For a board with
 * l = L - lines > 0 lines still owed and m = M - moves moves left:
 *   fill(r)   the number of filled cells of row r, r = 0 .. 19;
 *   cost(r)   10 - fill(r) where fill(r) < 10, and 10 where fill(r) = 10: a full row that stands on the board can never be cleared -- a
 *             piece has no cell in it, so it is never among the piece's rows -- and therefore costs what a fresh row costs;
 *   cells     the sum of the l smallest costs, the twenty costs extended by as many 10s as l asks for (L goes up to 250);
 *   need      ceil(cells / 4);
 *   spare     4 m - cells.
 * A running board is DEAD iff spare < 0, that is, need > m.  A finished board has cells = spare = 0 and is never dead.
 * A DEAD BOARD HAS NO WINNING CONTINUATION, WHATEVER PIECES COME.  Proof: a row is cleared only when all ten of its cells are filled.
 * Compaction keeps every surviving row's contents, and a fresh row enters empty.  Every move adds exactly four cells or tops out.  So
 * if l lines are still owed, at least the l cheapest rows must be completed, and the cells missing from them cannot be supplied in
 * fewer than a quarter as many moves.
 * The bound never calls a winnable board lost.  It is blind to geometry: a board that is not dead may still have no win.
 *
 * tpl_move_bound reads n environment states, one lane a board: cells_out i32 [n] and spare_out i32 [n], both 0 for a finished board
 * (a running state whose lines have reached L owes nothing: cells = 0).  Refused before any HIP call: what check_planes refuses for
 * tpl_afterstates' planes (NULL or misaligned planes, n < 1, 40 n >= 2^31, L outside [1, 250], M outside [1, 254]), a NULL or
 * misaligned (4 bytes) cells_out or spare_out.
 * tpl_move_bound_rows reads n configurations, rows i16 [n][20] as tpl_placement_solve takes them, as the states a full reset deals
 * (0 lines): cells_out i32 [n] = cells(board, L); ceil(cells / 4) is the least number of moves any solution can take.  Refused before
 * any HIP call: a NULL rows or cells_out, n < 1, n >= 2^31, L outside [1, 250], rows not 2-byte or cells_out not 4-byte aligned. */
int tpl_move_bound(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, int32_t* cells_out, int32_t* spare_out,
                   void* stream);
int tpl_move_bound_rows(const int16_t* rows, int64_t n, int32_t L, int32_t* cells_out, void* stream);

/* THE BOUNDED FORM of a placement kernel is its unbounded twin with two changes, both made in one place after the move
 * (csrc/learn/tpl_placement.h: bounded_move) and before psi is made:
 *   1. A move that leaves a running, dead board leaves it LOST: its state becomes lost-at-the-limit.  Feature 2 then reads 1 and the
 *      node is finished: it is not expanded, and it competes with its own value as any lost node does.
 *   2. value = w . phi as before, then + spare_weight * float(spare): one rounded multiply and one rounded add, made last, never
 *      fused.  spare is taken after change 1, so it is 0 for every finished node.  spare_weight is one finite float32 for the whole
 *      launch, whatever the number of weight rows.
 * With spare_weight = 0, on inputs where no child is dead, a bounded kernel writes the bytes of its twin (a value that is -0 in the
 * twin comes out +0: the order does not see the difference).
 *
 * tpl_placement_solve_bound, tpl_placement_solve_move_bound: tpl_placement_solve[_move] in the bounded form, with spare_weight behind
 * the width and two more outputs, both written in full:
 *   bound i32 [n]      need(root): no solution of the configuration is shorter;
 *   complete u8 [n]    1 iff at no ply run did the width cut drop a RUNNING candidate (dead children are lost, not running: dropping
 *                      them loses nothing, because they cannot win).
 * UNDER complete = 1, solved = 0 PROVES that no sequence of placements wins within M moves, and solved = 1 proves that solution_len is
 * the shortest there is: every running candidate of every ply was kept, so the search was exhaustive up to the bound's prune.  Without
 * complete, solved = 1 with solution_len == bound proves the same of that solution, and solved = 0 proves nothing.
 * Refused before any HIP call: what tpl_placement_solve refuses, a NULL bound or complete, bound not 4-byte aligned, a spare_weight
 * that is not finite.  The bounded kernels are bound to four workgroups a CU where their twin has five (csrc/learn/solve.hip).
 *
 * tpl_placement_beam_bound, tpl_placement_beam_move_bound: tpl_placement_beam[_move] in the bounded form, with spare_weight behind the
 * width; L and M are the environment's, and lines and moves are read from the state's bits.  Depth 1, width 1 is the bounded
 * one-ply player.  Consequence 2 of tpl_placement_solve holds between the bounded pair as it does between the unbounded one.
 * Refused before any HIP call: what tpl_placement_beam refuses, a spare_weight that is not finite. */
int tpl_placement_solve_bound(const int16_t* rows, const uint8_t* pieces, int64_t n, int32_t L, int32_t M, const float* weights,
                              int32_t width, float spare_weight, uint8_t* solved, int32_t* solution_len, uint8_t* actions,
                              float* best_value, int32_t* bound, uint8_t* complete, void* stream);
int tpl_placement_solve_move_bound(const int16_t* rows, const uint8_t* pieces, int64_t n, int32_t L, int32_t M, const float* weights,
                                   int32_t width, float spare_weight, uint8_t* solved, int32_t* solution_len, uint8_t* actions,
                                   float* best_value, int32_t* bound, uint8_t* complete, void* stream);
int tpl_placement_beam_bound(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const float* weights,
                             int64_t boards_per_member, int32_t depth, int32_t width, float spare_weight, uint8_t* action,
                             uint8_t* plan, float* score, void* stream);
int tpl_placement_beam_move_bound(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const float* weights,
                                  int64_t boards_per_member, int32_t depth, int32_t width, float spare_weight, uint8_t* action,
                                  uint8_t* plan, float* score, void* stream);

/* An exact depth-first solver for prescribed configurations.  What keeps tpl_placement_solve_bound from being a proof is its width
 * cut.  A depth-first search has no width: within the move bound's prune it visits every running board, or it stops at a node budget
 * and says so.  tpl_placement_exact searches the game of tpl_placement_solve_bound -- its configurations, its children, their values --
 * depth first, and with `shortest` it deepens the move budget from the bound upwards, so that the first win it meets is a shortest one.
 *
 * For a configuration -- rows[20] and pieces[M + 1] as tpl_placement_solve takes them --, one weight row w[12], one finite spare_weight,
 * max_nodes in [1, TPL_EXACT_MAX_NODES] and shortest = 0 or 1:
 *   ONE ITERATION AT BUDGET B searches the game (L, B) depth first from the ROOT: 0 lines, 0 moves, running, carry c = 0.
 *     Before a node at depth d is EXPANDED the node count is checked: if nodes == max_nodes THE WHOLE SEARCH ENDS with solved = 0,
 *     proved = 0, solution_len = 0 and a path of 255s; otherwise nodes += 1.
 *     To expand a node: its current piece is pieces[d] & 7, taken from the list; it has one child per distinct placement b of that piece
 *     in ascending b, each made and valued exactly as tpl_placement_solve_bound makes and values a candidate, under (L, B): move_board
 *     (node, b), whose move limit is B; a child left running and dead under (L, B) becomes LOST (the bounded form, change 1); with n the
 *     rows the move cleared,
 *       psi = (c + n, won, lost, features 3..11 of the child's board)
 *       value = the score rule on psi, then + spare_weight * float(spare) (the bounded form, change 2).
 *     The children are ordered by (value descending, b ascending); -0 and +0 tie.
 *     If ANY child is won the iteration ends with a WIN of length d + 1: the solution is the path to the node, then the won child that
 *     comes first in the order.
 *     Otherwise the RUNNING children are descended into, one after the other, in that order -- each expanded as above at depth d + 1
 *     with c + n for its carry --, and when they are used up the search returns to the node's parent.  A running child has made
 *     d + 1 < B moves, so no path is longer than B.
 *     The iteration ends WITHOUT A WIN when the root's children are used up.
 *   THE BUDGETS.  bound = need(root) (the move bound) is written in every case.
 *     shortest = 1: B = bound, bound + 1, .., M; the first iteration that wins ends the search with solved = 1, solution_len = B -- every
 *                   smaller budget was searched out without a win and no solution is shorter than bound, so the win is of length B exactly.
 *     shortest = 0: one iteration at B = M.
 *     If bound > M there is no iteration: solved = 0, proved = 1, nodes = 0.
 *     If no iteration wins: solved = 0, solution_len = 0, a path of 255s.
 *     nodes counts the expansions of all iterations, and max_nodes caps that sum.
 *   proved = 1 iff the search was not stopped by max_nodes.
 * UNDER proved = 1, solved = 0 PROVES that no sequence of placements wins within M moves: the only boards left unexpanded are dead ones
 * and finished ones, and a dead board has no winning continuation (the move bound's proof, above).  solved = 1 always comes with
 * proved = 1, and with shortest = 1 solution_len is then THE SHORTEST THERE IS.  WITH proved = 0 NOTHING IS PROVED: NOT THAT THERE IS A
 * WIN, AND NOT THAT THERE IS NONE.
 * Consequences:
 *   1. Playing the solution move by move from the configuration ends won after exactly solution_len moves, on any correct
 *      implementation of the game.
 *   2. Wherever tpl_placement_solve_bound reports complete = 1 for the same configuration, L, M, weights and spare_weight, this search
 *      with proved = 1 agrees with it on solved, and with shortest = 1 on solution_len as well.
 *   3. The result is a function of the inputs alone; nothing is written but the outputs.
 * The weights order the children and so decide how soon a win is met and how many nodes that takes; they do not decide WHETHER a
 * search that ends with proved = 1 finds one.  THE FINITENESS CAVEAT of the weights and the masking of the piece ids are
 * tpl_placement_solve's.  tpl_placement_exact_move is the 14-feature form: weights f32 [16] of which 14 are read, a node's carry holding
 * the landing and eroded sums of its path as the solver's does.
 *
 * One kernel, ONE CONFIGURATION PER WAVEFRONT (csrc/learn/exact.hip): lanes 0 .. 33 each make one child of the node being expanded, the
 * order comes from 64-bit keys ranked across the wave, and the stack -- a record of 80 bytes a depth -- is LDS sized by M.  rows
 * i16 [n][20] and pieces u8 [n][M + 1] are read; solved u8 [n], proved u8 [n], solution_len i32 [n], actions u8 [n][M] (the solution's
 * placements b = 10 r + l, 255 behind the end), bound i32 [n] and nodes u32 [n] are each written in full.
 * Refused before any HIP call: everything tpl_placement_solve_bound refuses of the arguments the two share (n < 1, n >= 2^31, a NULL
 * rows, pieces, weights, solved, solution_len, actions or bound, weights not 16-byte aligned, solution_len or bound not 4-byte
 * aligned, rows not 2-byte aligned, L outside [1, 250] or M outside [1, 254], a spare_weight that is not finite), a NULL proved or
 * nodes, nodes not 4-byte aligned, max_nodes outside [1, TPL_EXACT_MAX_NODES], shortest other than 0 or 1. */
#define TPL_EXACT_MAX_NODES (1 << 24)
int tpl_placement_exact(const int16_t* rows, const uint8_t* pieces, int64_t n, int32_t L, int32_t M, const float* weights,
                        float spare_weight, int32_t max_nodes, int32_t shortest, uint8_t* solved, uint8_t* proved,
                        int32_t* solution_len, uint8_t* actions, int32_t* bound, uint32_t* nodes, void* stream);
int tpl_placement_exact_move(const int16_t* rows, const uint8_t* pieces, int64_t n, int32_t L, int32_t M, const float* weights,
                             float spare_weight, int32_t max_nodes, int32_t shortest, uint8_t* solved, uint8_t* proved,
                             int32_t* solution_len, uint8_t* actions, int32_t* bound, uint32_t* nodes, void* stream);

/* The exact search FROM A NODE, and the proved labels of a node's moves (csrc/learn/exact_nodes.hip).  tpl_placement_exact proves
 * things about a configuration's root; these two prove them about any board of a prescribed game and about each move from it.
 *
 * A NODE of the game (L, M) is a board rows[20], the lines cleared and the moves made so far, and entry, the index of its
 * configuration's list in a shared pieces u8 [n_cfg][M + 1]: the piece at depth d from the node is pieces[entry][moves + d] & 7.  The
 * 34 children of a node and all nodes of one game name one list; nothing is copied.
 * THE SHIFTED GAME.  For the exact search a node is the same thing as a fresh configuration with board rows, piece list
 * pieces[entry][moves:] and the game (L - lines, M - moves): the move, the terminal tests (won: rows were cleared and lines >= L; lost
 * at the limit: moves >= M), cells, spare = 4 (B - moves) - cells, the board features and the carry, which is 0 at the start, read
 * nothing else, and every iteration's budget shifts by moves.
 *
 * tpl_placement_exact_nodes: for node i THE SEARCH IS tpl_placement_exact's, above, with the node for the root: running, carry 0,
 * the budgets B = moves + need(node) .. M (shortest = 1) or M alone, need(node) the move bound's need of the board with L - lines
 * rows owed; need(node) > M - moves is decided without expanding a node: solved = 0, proved = 1, nodes = 0.  THE SIX OUTPUTS ARE,
 * BYTE FOR BYTE, WHAT tpl_placement_exact WRITES FOR THE SHIFTED CONFIGURATION in the game (L - lines, M - moves) with the same
 * weights, spare_weight, max_nodes and shortest: solved, proved, solution_len and actions COUNTED FROM THE NODE, bound = need(node),
 * nodes.  actions is u8 [n][M] for the launch's M: the shifted game's M - moves placements, then 255s.  With lines = moves = 0 and
 * entry[i] = i it is tpl_placement_exact.  What proved = 1 and proved = 0 say is said there: WITH proved = 0 NOTHING IS PROVED.
 * A node with lines >= L, moves >= M or entry >= n_cfg cannot be refused by the host without a copy; THE KERNEL TREATS IT AS
 * FINISHED -- solved = 0, proved = 1, solution_len = 0, nodes = 0, bound = 0, a path of 255s -- AND READS NEITHER ITS BOARD NOR pieces
 * FOR IT: no index ever falls outside pieces.
 * One wavefront a node, the frame of tpl_placement_exact's kernel; the stack is indexed by the depth from the node and sized by M.
 * Refused before any HIP call: everything tpl_placement_exact refuses of the arguments the two share, a NULL lines, moves or entry,
 * entry not 4-byte aligned, n_cfg outside [1, 2^31).
 *
 * tpl_placement_exact_labels: for node i and every action b = 10 r + l < 40, label u8 [n][40], length i32 [n][40] and nodes u32
 * [n][40], each written in full.  Placement b of the node's current piece is made exactly as the search makes a child -- move_board
 * under (L, M) from the node's lines and moves, a child left running and dead becomes LOST (the bounded form, change 1) -- and then
 *   TPL_LABEL_NONE 0   b is not a distinct placement of the piece (canonical(cur, b) != b), or the node is finished as above:
 *                      length = 0, nodes = 0;
 *   TPL_LABEL_WIN  1   PROVED WINNING: the child is won (length = 1, nodes = 0), or the search of tpl_placement_exact_nodes from the
 *                      running child -- the node one move on, shortest = 1, max_nodes for this child alone -- ends solved:
 *                      length = 1 + its solution_len, the fewest moves from the node in which a game through b can be won;
 *   TPL_LABEL_LOSS 2   PROVED LOSING: the child is lost or dead (nodes = 0), or that search ends proved and not solved: no sequence of
 *                      placements after b wins within M moves.  length = 0;
 *   TPL_LABEL_OPEN 3   UNPROVED: that search was stopped by max_nodes.  length = 0.  LABEL 3 PROVES NOTHING: NOT THAT b WINS, AND NOT
 *                      THAT IT LOSES.
 * nodes is the child's search's.  By construction the labels of a node are tpl_placement_exact_nodes applied to its children.
 * A grid of 40 n wavefronts, one a (node, action).  Refused before any HIP call: what tpl_placement_exact_nodes refuses of the
 * arguments the two share, 40 n >= 2^31, a NULL label, length or nodes, length or nodes not 4-byte aligned.
 * The _move entries are the 14-feature forms, as tpl_placement_exact_move is. */
#define TPL_LABEL_NONE 0
#define TPL_LABEL_WIN 1
#define TPL_LABEL_LOSS 2
#define TPL_LABEL_OPEN 3
int tpl_placement_exact_nodes(const int16_t* rows, const uint8_t* lines, const uint8_t* moves, const uint32_t* entry,
                              const uint8_t* pieces, int64_t n, int64_t n_cfg, int32_t L, int32_t M, const float* weights,
                              float spare_weight, int32_t max_nodes, int32_t shortest, uint8_t* solved, uint8_t* proved,
                              int32_t* solution_len, uint8_t* actions, int32_t* bound, uint32_t* nodes, void* stream);
int tpl_placement_exact_nodes_move(const int16_t* rows, const uint8_t* lines, const uint8_t* moves, const uint32_t* entry,
                                   const uint8_t* pieces, int64_t n, int64_t n_cfg, int32_t L, int32_t M, const float* weights,
                                   float spare_weight, int32_t max_nodes, int32_t shortest, uint8_t* solved, uint8_t* proved,
                                   int32_t* solution_len, uint8_t* actions, int32_t* bound, uint32_t* nodes, void* stream);
int tpl_placement_exact_labels(const int16_t* rows, const uint8_t* lines, const uint8_t* moves, const uint32_t* entry,
                               const uint8_t* pieces, int64_t n, int64_t n_cfg, int32_t L, int32_t M, const float* weights,
                               float spare_weight, int32_t max_nodes, uint8_t* label, int32_t* length, uint32_t* nodes, void* stream);
int tpl_placement_exact_labels_move(const int16_t* rows, const uint8_t* lines, const uint8_t* moves, const uint32_t* entry,
                                    const uint8_t* pieces, int64_t n, int64_t n_cfg, int32_t L, int32_t M, const float* weights,
                                    float spare_weight, int32_t max_nodes, uint8_t* label, int32_t* length, uint32_t* nodes,
                                    void* stream);

/* The exact search OVER THE PIECES A STATE'S WINDOW SHOWS (csrc/learn/exact_window.hip).  The searches above read a configuration's
 * whole piece list, which an agent that plays from states does not have.  A state does carry pieces: its 36-bit window holds
 * known = 12 - moves % 10 true ones, the falling one first (tpl_placement_beam, above).  This entry proves what those pieces decide.
 *
 * tpl_placement_window_prove: n states in the two packed planes the beam entries take.  Take a RUNNING board of the game (L, M) with
 * `lines`, `moves` and window entries q[0..11], entry j at bits 3 j of window | window_hi << 32, masked & 7 as move_board masks them, and
 *   known = 12 - moves % 10,   rem = M - moves,   H = min(known, rem), the HORIZON.
 * THE SEARCH IS tpl_placement_exact_nodes' WITH shortest = 1: the root is the board, the game is (L - lines, H), the piece at depth d
 * is q[d]; there is no new search rule.  Equivalently, and this is what the tests hold it to: THE OUTPUTS ARE, BYTE FOR BYTE, WHAT
 * tpl_placement_exact_nodes WRITES for the node (rows, lines, M - H, entry i) over a list pieces'[i] with pieces'[i][M - H + d] = q[d]
 * for d < H -- solved, proved, solution_len, actions[0..H), bound and nodes.
 * Outputs per board, each written in full: solved u8, proved u8, solution_len i32, plan u8 [n][TPL_WINDOW_PLAN] (placements
 * b = 10 r + l, 255 behind the end), bound i32 (need(board) with L - lines rows owed), nodes u32, horizon u8 (H), and verdict u8:
 *   TPL_WINDOW_NONE 0   the board is finished or was skipped (below);
 *   TPL_WINDOW_WIN  1   solved: the plan wins THE REAL GAME in solution_len moves, and no shorter win exists, because a shorter win
 *                       would lie inside the horizon too;
 *   TPL_WINDOW_LOSS 2   proved, not solved, and H == rem: no sequence of placements wins -- the move bound's proof, as
 *                       tpl_placement_exact's;
 *   TPL_WINDOW_OPEN 3   everything else: max_nodes stopped the search, or it was searched out with H < rem, which says only that no
 *                       win lies within the known pieces.  VERDICT 3 PROVES NOTHING ABOUT THE GAME.
 * A board that is not running -- or whose lines >= L or moves >= M, which no environment of the game holds -- is FINISHED: verdict 0,
 * solved = 0, proved = 1, solution_len = 0, a plan of 255s, bound = 0, nodes = 0, horizon = 0, as tpl_placement_exact_nodes finishes
 * the node with moves = M.
 * skip (may be NULL) is a mask u8 [n]: a board with skip[i] != 0 is NOT SEARCHED and gets verdict 0, solved = 0, proved = 0,
 * solution_len = 0, a plan of 255s and nodes = 0; bound and horizon are still written.
 * weights is one row (12 floats, or in the _move form the first 14 of a row of 16), spare_weight and max_nodes are
 * tpl_placement_exact's: they order the children and cap the expansions, and decide no verdict but between 3 and the two others.
 * One wavefront a board, the frame of tpl_placement_exact's kernel with a stack of twelve records in static LDS.
 * Refused before any HIP call: everything tpl_placement_exact_nodes refuses of the arguments the two share (n outside [1, 2^31), L
 * or M out of range, max_nodes outside [1, TPL_EXACT_MAX_NODES], a spare_weight that is not finite, weights NULL or not 16-byte
 * aligned), a NULL plane or output, planes not 16-byte aligned, solution_len, bound or nodes not 4-byte aligned. */
#define TPL_WINDOW_PLAN 12
#define TPL_WINDOW_NONE 0
#define TPL_WINDOW_WIN 1
#define TPL_WINDOW_LOSS 2
#define TPL_WINDOW_OPEN 3
int tpl_placement_window_prove(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const float* weights,
                               float spare_weight, int32_t max_nodes, const uint8_t* skip, uint8_t* solved, uint8_t* proved,
                               int32_t* solution_len, uint8_t* plan, int32_t* bound, uint32_t* nodes, uint8_t* horizon,
                               uint8_t* verdict, void* stream);
int tpl_placement_window_prove_move(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const float* weights,
                                    float spare_weight, int32_t max_nodes, const uint8_t* skip, uint8_t* solved, uint8_t* proved,
                                    int32_t* solution_len, uint8_t* plan, int32_t* bound, uint32_t* nodes, uint8_t* horizon,
                                    uint8_t* verdict, void* stream);

/* An n-tuple afterstate value function, its placement policy and its temporal-difference update (csrc/learn/ntuple.hip).
 *
 * Table: TPL_NTUPLE_ENTRIES = 8 * 153 * 256 + 1024 = 314,368 int32 entries (1,257,472 bytes), 16-byte aligned, in units of 2^-16:
 *   tuple[p][t][q] at index (p * 153 + t) * 256 + q      p in 0..7, t in 0..152, q in 0..255
 *   counter[k]     at index 313,344 + k                   k in 0..1023
 * Patterns of a state s with column words c_0 .. c_9 (bit r = row r, row 0 = top): a tuple is t = 17 x + y, x in 0..8, y in 0..16,
 * and its pattern is  q(s, t) = ((c_x >> y) & 15) | (((c_{x+1} >> y) & 15) << 4)  -- two adjacent columns by four rows.  The piece
 * index p is window entry 0 of s (0..7), and the counter index is  k = 64 min(max(L - lines, 0), 15) + min(max(M - moves, 0), 63).
 * Value: V(s) = 0 for a state that is not running; otherwise
 *   V(s) = float32( sum over the t with q(s, t) != 0 of tuple[p][t][q(s, t)]  +  counter[k] ) * 2^-16
 * -- the sum exact in 64-bit integers, ONE rounding at the conversion, the scaling exact.  The all-empty pattern contributes nothing
 * and is never updated: it is most of a typical board, and it would be the one address that every board adds to.
 *
 * Policy on a state s, with reward parameters (r_line, r_win, r_lose) and a discount gamma:
 *   Finished board (state(s) != running): action 0, score 0; its afterstate is s itself, bit for bit, with value 0.
 *   Running board: every distinct placement a (a == canonical(cur, a)) gives (s_a, r_a, done_a) exactly as tpl_afterstates makes
 *   them;  score(a) = r_a if done_a, else r_a + gamma * V(s_a)  in float32: one rounded multiply and one rounded add, never fused.
 *   The greedy action is the lowest a at the maximum of score (-0 and +0 tie).
 * Exploration: h_i = position i + 1 of the splitmix64 stream keyed by (seed, step) -- the samplers' hash, with `step` where they
 * have `update`.  A running board i explores iff (h_i >> 40) < (uint32)(epsilon * 2^24); it then plays the j-th distinct placement
 * of its current piece in ascending order, j = ((h_i & 0xFFFFFFFF) * S) >> 32 with S the number of distinct placements (17, 34 or
 * 9, above): uniform over placements, not over the 40 actions.  `score` is ALWAYS the greedy maximum -- it is the TD target --
 * while `after` and `value` (V of `after`; 0 where the move ended the game) belong to the action that is played.
 *
 * Update, for each of n states with an error e_i: a state that is not running adds nothing; otherwise
 *   d_i = (int32) rint(rate * e_i)   -- the product rounded once in float32, clamped to +-2^24, 0 for a NaN --
 * is added to counter[k] and to tuple[p][t][q] of every tuple with a non-zero pattern.  The adds wrap as two's complement (the
 * caller keeps entries small).  The kernel only adds and never reads the table, so the table that results is the same whatever
 * order the adds arrive in: no float atomic, and two runs give the same bytes. */
#define TPL_NTUPLE_ENTRIES 314368

/* V of each of `n` states: plane_a / plane_b [n] 16-byte words (read only), table int32 [TPL_NTUPLE_ENTRIES] -> value f32 [n].
 * Refused before any HIP call: n < 1, 40 n >= 2^31, a NULL or misaligned (16 bytes) plane pointer, L outside [1, 250] or M
 * outside [1, 254] (tpl_afterstates' checks), table NULL or not 16-byte aligned, value NULL or not 4-byte aligned. */
int tpl_ntuple_value(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const int32_t* table,
                     float* value, void* stream);

/* The policy above on each of `n` states in one kernel: 32 bytes read per board besides the table gathers (at most 153 per
 * distinct placement that leaves the game running), and at most 1 + 4 + 32 + 4 bytes written: action u8 [n]; score f32 [n]
 * (optional); after_a / after_b [n] 16-byte words (both or neither); value f32 [n] (optional).  An output that is not given is not
 * written.  The afterstate comes out of the registers of the lane that made the chosen move.  Refused before any HIP call:
 * tpl_ntuple_value's plane, n, L, M and table checks, action NULL, only one of after_a / after_b or either misaligned (16 bytes),
 * score or value not 4-byte aligned, epsilon outside [0, 1] (a NaN included), gamma not finite. */
int tpl_ntuple_act(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line, float r_win,
                   float r_lose, float gamma, const int32_t* table, float epsilon, uint64_t seed, uint64_t step, uint8_t* action,
                   float* score, void* after_a, void* after_b, float* value, void* stream);

/* The policy two plies deep, with the known next piece.  In this game an afterstate knows the piece that falls next (window entry 1
 * of the state it came from), so  max_b (r_b + gamma V(s_ab))  is the value of the afterstate s_a itself, not a heuristic
 * extension: tpl_ntuple_act ranks placements by the table's approximation of that quantity, tpl_ntuple_search by the quantity, with
 * the table one move further out.  An afterstate's window is good for exactly two entries (above), so this is the deepest search
 * the table can make exactly.
 * For a state s with cur = window entry 0, nxt = window entry 1, and every distinct first placement a (a == canonical(cur, a)):
 *   move_board(s, a) and the pop give n1, state1, the board s1 and r1 = the reward of (n1, state1), exactly as tpl_ntuple_act
 *   makes them.
 *   Finished board (state(s) != running): action 0, score 0, second 255; its afterstate is s itself, bit for bit, with value 0.
 *   state1 != running (the first move ends the game): Q(a) = r1 and second(a) = 255.
 *   otherwise, for every distinct placement b of nxt (b == canonical(nxt, b)) in ascending b -- nxt = 7 ("none") is what move_board
 *   and the shape table make of it, O's nine placements, as in tpl_placement_search --, move_board(s1, b) and the pop give n2,
 *   state2, the board s2 and r2 = the reward of (n2, state2):
 *     q(a, b) = r2 + gamma * V(s2) if state2 runs, else r2     -- V as tpl_ntuple_value gives it: the piece index of s2 is window
 *                                                                 entry 2 of s, the counter index comes from s2's lines and moves;
 *     W(a) = max over b of q(a, b); second(a) = the lowest b at that maximum (-0 and +0 tie);
 *     Q(a) = r1 + gamma * W(a).
 *   Every product and every sum is rounded once in float32 and never fused.
 *   The greedy action is the lowest a at the maximum of Q (-0 and +0 tie).
 * Exploration is tpl_ntuple_act's draw unchanged -- the same hash of (seed, step, board), uniform over the distinct FIRST placements
 * -- so at equal (seed, step, epsilon) the same boards explore the same rank at both depths.  `score` is ALWAYS the greedy maximum
 * of Q; `action`, `second` = second(action), `after` = the ONE-PLY afterstate s1 of the action and `value` = V(s1) (0 where the move
 * ended the game) belong to the action that is played -- what tpl_ntuple_act gives for that action, so a TD(0) loop on afterstates
 * needs nothing else, and its target becomes the two-ply score.
 * After a non-auto-reset step with `action` on an environment without a pool, a board that still runs has a tpl_ntuple_act choice
 * (epsilon 0) of `second`: the second ply is the one-ply rule on the board the step leaves.
 *
 * One kernel (ntuple_search_kernel, tpl_ntuple_act's frame with a loop over b in the lanes whose first move leaves the game
 * running): 32 bytes read per board besides the table gathers, at most 1 + 1 + 4 + 32 + 4 bytes written: action u8 [n]; second u8
 * [n] (optional, no alignment requirement); score, after_a / after_b and value as tpl_ntuple_act's.  An output that is not given is
 * not written.  Refused before any HIP call: everything tpl_ntuple_act refuses. */
int tpl_ntuple_search(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line, float r_win,
                      float r_lose, float gamma, const int32_t* table, float epsilon, uint64_t seed, uint64_t step, uint8_t* action,
                      uint8_t* second, float* score, void* after_a, void* after_b, float* value, void* stream);

/* The update above: error f32 [n], one per state of plane_a / plane_b.  It is tpl_ntuple_update_trace (below) on the planes as a
 * ring of one slot, head 0, horizon 1, not symmetric, and it launches that entry's kernel (ntuple_trace_kernel<false>): age 0 has
 * the weight w_0 = 1 whatever the decay, so d is rint(rate * e).  Refused before any HIP call, under its own name:
 * tpl_ntuple_value's plane, n, L, M and table checks, error NULL or not 4-byte aligned, rate not finite. */
int tpl_ntuple_update(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, int32_t* table,
                      const float* error, float rate, void* stream);

/* The update with truncated TD(lambda) traces and, optionally, tied under the game's mirror symmetry (tpl_mirror.h).
 *
 * ring_a / ring_b: [slots][n] 16-byte words, slot-major, read only -- the last states of n boards.  The state of board i at age k
 * is in slot (head - k) mod slots; age 0 is the newest.  error f32 [n], one per board.  For board i with error e:
 *   weights  w_0 = 1.0f,  w_k = w_{k-1} * decay                      -- each product rounded once in float32
 *   for k = 0 .. horizon - 1 in order, with s the state at age k: if s is not running, STOP -- older ages belong to an earlier
 *   episode or were never filled.  Otherwise
 *     d_k = (int32) rint((rate * w_k) * e)   -- two products, each rounded once in float32 and never fused, clamped to +-2^24, 0 for
 *                                               a NaN: tpl_ntuple_update's step with rate * w_k as its rate, so d_0 is its d --
 *   is added, wrapping as two's complement, to counter[k(s)] and to tuple[p][17 x + y][q] of every tuple of s with q != 0, exactly
 *   as tpl_ntuple_update adds.
 * With symmetric != 0, d_k is ALSO added to the entries of the reflected state: tuple[pi(p)][17 (8 - x) + y][swap(q)] for those same
 * tuples, with pi = [0, 2, 1, 3, 5, 4, 6, 7] (L <-> J, S <-> Z) and swap(q) = (q >> 4) | ((q & 15) << 4).  The counter is added
 * ONCE.  Both tuple adds are made even where the two indices coincide (p = pi(p), x = 4 and q = swap(q)): such an entry takes
 * 2 d_k.  The kernel only adds and never reads the table, so the bytes that result do not depend on the order of the adds.
 *
 * Invariant.  Let sigma map the index of tuple[p][17 x + y][q] to that of tuple[pi(p)][17 (8 - x) + y][swap(q)] and fix the counter
 * indices; sigma is an involution.  A table is MIRROR-SYMMETRIC when table[sigma(j)] == table[j] for all j.  The zero table is, and
 * a symmetric update adds the same amount to j and to sigma(j), so it keeps a symmetric table symmetric.  The tuples of the
 * reflected state are the sigma-images of the state's, so under a symmetric table V(s) == V(mirror s) exactly, and
 * tpl_ntuple_value / tpl_ntuple_act / tpl_ntuple_search play it unchanged: symmetry is a property of the table's bytes.
 *
 * One kernel (ntuple_trace_kernel<symmetric>): a lane per (board, age), the age in the grid's y.  horizon = 1, decay anything,
 * symmetric = 0 leaves tpl_ntuple_update's bytes on slot `head`.  Refused before any HIP call: everything tpl_ntuple_update
 * refuses (ring_a / ring_b as its planes), slots outside [1, TPL_NTUPLE_TRACE_MAX + 1], head outside [0, slots), horizon outside
 * [1, min(slots, TPL_NTUPLE_TRACE_MAX)], 40 * slots * n >= 2^31, decay outside [0, 1] (a NaN included). */
#define TPL_NTUPLE_TRACE_MAX 16
int tpl_ntuple_update_trace(const void* ring_a, const void* ring_b, int64_t n, int32_t slots, int32_t head, int32_t horizon,
                            int32_t L, int32_t M, int32_t* table, const float* error, float rate, float decay,
                            int32_t symmetric, void* stream);

/* The update above with temporal-coherence step sizes (Beal & Smith): every table entry keeps the signed and the absolute sum of the
 * steps it has been sent, and learns at their ratio -- at the full rate while its errors keep their sign, slower where they
 * alternate, which is what an overshoot looks like.
 *
 * Coherence buffer: int64 [TPL_NTUPLE_ENTRIES][2] (5,029,888 bytes), 16-byte aligned: entry j holds the pair (E_j, A_j), the signed
 * and the absolute sum of the steps sent to table entry j.  A zeroed buffer is the start.
 * Step size of an entry:
 *   alpha_j = 1.0f                                             if A_j <= 0,
 *   alpha_j = fminf(__fdiv_rn((float) |E_j|, (float) A_j), 1.0f)  otherwise
 * -- |E_j| the magnitude as an UNSIGNED 64-bit value (so INT64_MIN is defined), both conversions to nearest even, the quotient
 * rounded once.
 * The update.  For board i, age k < horizon, with error e: the ring, the ages, w_k, the stop at the first state that does not run and
 *   d_k = (int32) rint((rate * w_k) * e)
 * are exactly tpl_ntuple_update_trace's.  Where the trace is open and d_k != 0, for every entry j that tpl_ntuple_update_trace would
 * add to -- the counter and every tuple with a non-zero pattern; with symmetric != 0 the sigma-images of the tuples as well, the
 * counter ONCE, both tuple adds also where the two indices coincide --:
 *   table[j] += s, wrapping, with  s = (int32) rint(((rate * w_k) * alpha_j) * e)   -- three products, each rounded once in float32
 *                                                                                     and never fused, clamped to +-2^24, 0 for a NaN;
 *   E_j += d_k  and  A_j += |d_k|, wrapping in 64 bits.
 * Read before add: every alpha_j of a call is read from the coherence buffer AS IT STOOD BEFORE THE CALL.  A call has two phases, the
 * step phase, which reads the coherence buffer and adds to the table, and the accumulate phase, which only adds to the coherence
 * buffer.  Neither reads what it adds to, so the bytes of both buffers do not depend on the order of the adds, and two runs give the
 * same bytes.
 * Consequences.  With a zeroed coherence buffer every alpha is 1 and (r * 1.0f) * e is r * e: the table bytes are
 * tpl_ntuple_update_trace's.  |s| <= |d_k|, and s is 0 where d_k is.  A coherence buffer is MIRROR-SYMMETRIC when its pairs at j and
 * sigma(j) are equal; a symmetric call adds the same amounts at j and sigma(j) in both buffers, so a mirror-symmetric pair (table,
 * coherence) stays mirror-symmetric.  An entry that is its own image takes 2 s, 2 d_k and 2 |d_k|.
 *
 * Two kernels on `stream`, one after the other (ntuple_coherent_step_kernel<symmetric>, ntuple_coherent_accumulate_kernel<symmetric>),
 * each a lane per (board, age); no sync and nothing allocated, so a call can be captured into a graph.  Refused before any HIP call,
 * under its own name: everything tpl_ntuple_update_trace refuses, in the same order, and, after the table checks, coherence NULL or
 * not 16-byte aligned. */
int tpl_ntuple_update_coherent(const void* ring_a, const void* ring_b, int64_t n, int32_t slots, int32_t head, int32_t horizon,
                               int32_t L, int32_t M, int32_t* table, int64_t* coherence, const float* error, float rate,
                               float decay, int32_t symmetric, void* stream);

/* Table shapes.  The geometry of the windows is a parameter of the table; everything else in the rule above is not.
 *
 * TPL_NTUPLE_SHAPE_2X4 = 0 is the rule as stated so far, unchanged in every byte: 153 windows of two adjacent columns by four rows.
 * TPL_NTUPLE_SHAPE_3X3 = 1: a tuple is t = 18 x + y, x in 0..7, y in 0..17 -- 144 tuples --, the window of columns x, x + 1, x + 2 and
 * rows y .. y + 2, and its pattern is
 *   q(s, t) = ((c_x >> y) & 7) | (((c_{x+1} >> y) & 7) << 3) | (((c_{x+2} >> y) & 7) << 6)          -- 512 patterns.
 * A 3 x 3 window holds a column together with BOTH of its neighbours, which no 2 x 4 window does: a well, or a notch under an
 * overhang, is one pattern of it and not a sum of two half-views.
 * Table: TPL_NTUPLE_ENTRIES_3X3 = 8 * 144 * 512 + 1024 = 590,848 int32 entries (2,363,392 bytes), 16-byte aligned, in units of 2^-16:
 *   tuple[p][t][q] at index ((p * 144 + t) * 512) | q      p in 0..7, t in 0..143, q in 0..511
 *   counter[k]     at index 589,824 + k                    k in 0..1023, the same k as above
 * Unchanged: the piece index p and the counter index k; the all-empty pattern contributes nothing and is never updated; the sum is
 * exact in 64-bit integers, rounded ONCE at the conversion and scaled by 2^-16; a state that is not running has V = 0; the policy,
 * the exploration draw, d_k, the trace rule, the step size alpha_j and the read-before-add rule of the coherent update.
 * Windows stay inside the board: no wall and no floor bits are added.  A wall column read as full would give every board with an
 * empty edge column one shared non-empty entry -- the hot address that skipping the all-empty pattern avoids.
 * Mirror image (symmetric != 0): d_k is also added to tuple[pi(p)][18 (7 - x) + y][swap(q)], where swap exchanges bits 0..2 of q with
 * bits 6..8 and leaves bits 3..5:  swap(q) = (q >> 6) | (q & 0x38) | ((q & 7) << 6).  Both tuple adds are made, also where the two
 * entries are one -- with eight window columns x never equals 7 - x, so in this shape no tuple entry is its own image; the rule is
 * worded for both shapes.  sigma, the invariant and its consequences read as above with these indices.
 * Coherence buffer: int64 [TPL_NTUPLE_ENTRIES_3X3][2] (9,453,568 bytes): of the shape's entry count, as the table.
 *
 * Each _shaped entry below is the entry of the same name with `shape` before `stream`; the entry without it is the _shaped one at
 * TPL_NTUPLE_SHAPE_2X4, through the same argument check and the same kernels.  table (and coherence) must hold the shape's
 * entries; device memory cannot be checked here.  Refused before anything else, and before any pointer is looked at: a shape that
 * is neither of the two.  The 3 x 3 kernels (ntuple3_*_kernel) are the same device bodies compiled for the other geometry: the
 * same lane mappings, eight (symmetric: sixteen) gathers or adds in flight per trip over y, 18 trips. */
typedef enum { TPL_NTUPLE_SHAPE_2X4 = 0, TPL_NTUPLE_SHAPE_3X3 = 1 } tpl_ntuple_shape;
#define TPL_NTUPLE_ENTRIES_3X3 590848

/* The entries of a table of `shape`: TPL_NTUPLE_ENTRIES, TPL_NTUPLE_ENTRIES_3X3, or -1 for a shape that is not known. */
int64_t tpl_ntuple_entries(int32_t shape);

int tpl_ntuple_value_shaped(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const int32_t* table,
                            float* value, int32_t shape, void* stream);
int tpl_ntuple_act_shaped(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line, float r_win,
                          float r_lose, float gamma, const int32_t* table, float epsilon, uint64_t seed, uint64_t step,
                          uint8_t* action, float* score, void* after_a, void* after_b, float* value, int32_t shape, void* stream);
int tpl_ntuple_search_shaped(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line, float r_win,
                             float r_lose, float gamma, const int32_t* table, float epsilon, uint64_t seed, uint64_t step,
                             uint8_t* action, uint8_t* second, float* score, void* after_a, void* after_b, float* value,
                             int32_t shape, void* stream);
int tpl_ntuple_update_shaped(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, int32_t* table,
                             const float* error, float rate, int32_t shape, void* stream);
int tpl_ntuple_update_trace_shaped(const void* ring_a, const void* ring_b, int64_t n, int32_t slots, int32_t head, int32_t horizon,
                                   int32_t L, int32_t M, int32_t* table, const float* error, float rate, float decay,
                                   int32_t symmetric, int32_t shape, void* stream);
int tpl_ntuple_update_coherent_shaped(const void* ring_a, const void* ring_b, int64_t n, int32_t slots, int32_t head,
                                      int32_t horizon, int32_t L, int32_t M, int32_t* table, int64_t* coherence, const float* error,
                                      float rate, float decay, int32_t symmetric, int32_t shape, void* stream);

/* Beam search over the known piece window with an n-tuple table at the leaves.  tpl_ntuple_search stops at two plies because an
 * AFTERSTATE knows its next piece and no more; an ENVIRONMENT STATE carries 12 - (moves mod 10) true pieces (tpl_placement_beam,
 * above), and the policy is always asked about environment states.  tpl_placement_beam gives this rule its nodes, its candidates
 * in order, the stable compaction and the ties; tpl_ntuple_search gives it the rewards and V.  There is no exploration: the policy
 * is greedy.
 *
 * For a state s, a table of `shape`, reward parameters (r_line, r_win, r_lose), a discount gamma, a depth D in
 * [1, TPL_NTUPLE_BEAM_MAX_DEPTH] and a width W in [1, TPL_BEAM_MAX_WIDTH]:
 *   Finished board (state(s) != running): action 0, score 0, every plan entry 255; `after` is s itself, bit for bit.
 *   Running board: the effective depth is d = min(D, 11 - moves(s) mod 10), from the state's bits as they stand (pool or not) -- ONE
 *   LESS than tpl_placement_beam's: the value of a leaf is read under the piece that falls next, window entry d of the root, and
 *   that entry must be a true piece.  11 - moves mod 10 is never below 2.
 *   A NODE is a board (its window popped once per move made, by next_window(s, false, 0) as tpl_afterstates does), its path of
 *   placements b_1 .. b_j, the rewards r_1 .. r_j of its moves -- each tpl_afterstates' reward of (rows cleared, state after) --
 *   and a value.  Beam_0 is the root alone (empty path).
 *   For ply j = 1 .. d the CANDIDATES are listed exactly as tpl_placement_beam lists them: over the nodes of Beam_{j-1} in their
 *   stored order, a node that does not run gives one candidate, itself, value and path unchanged; a running node gives one child
 *   per distinct placement b of its current piece in ascending b (piece 7 is O's nine placements): move_board(node, b), then the pop.
 *   The value of a child at ply j is folded from the leaf inwards:
 *       tail_j = r_j                       if the child does not run
 *       tail_j = r_j + gamma * V(child)    otherwise
 *       tail_k = r_k + gamma * tail_{k+1}  for k = j - 1 .. 1
 *       value  = tail_1
 *   -- V as tpl_ntuple_value_shaped gives it: the piece index is window entry 0 of the popped child (entry j of the root), the
 *   counter index comes from the child's lines and moves.  Every product and every sum is rounded once in float32 and never fused.
 *   (G + gamma^j * V, accumulated forwards, is other arithmetic and not this rule.)
 *   Candidates are ordered by (value descending, candidate index ascending); -0 and +0 tie.  Beam_j = the min(W, count) best
 *   candidates STORED IN CANDIDATE ORDER, each with its value as computed (a -0 stays a -0).
 *   Choice: the best node of Beam_d under the same order: action = the first placement of its path, score = its value,
 *   plan[0 .. D) = its path padded with 255.  after_a / after_b receive the ONE-PLY afterstate of `action`: row `action` of
 *   tpl_afterstates, which is what tpl_ntuple_act writes for that action.
 * Consequences:
 *   D = 1, any W: action, score and after are tpl_ntuple_act_shaped's at epsilon 0, bit for bit.
 *   D = 2, W >= 34, gamma >= 0: action and score are tpl_ntuple_search_shaped's, bit for bit.  x -> r1 + gamma * x is monotone under
 *   rounding, so the best of the folded values is the fold of the best.  plan[1] is the lowest b whose FOLDED value equals score;
 *   the search's `second` is the lowest b at the maximum of q; so plan[1] <= second, and they differ only where two different q round
 *   to one Q.
 *   Playing `plan` move by move on a non-auto-reset environment without a pool (no refill: the same pop) earns rewards and reaches a
 *   final board whose fold under the table -- the rewards earned, and V of the final board where it still runs -- is `score`, bit
 *   for bit.
 * THE FINITENESS CAVEAT is tpl_placement_act's, here for the reward parameters and gamma times the table's values.  Boards that
 * different paths reach are not merged, and the pool is never read for pieces beyond the window.
 *
 * One kernel per shape (ntuple_beam_kernel, ntuple_beam3_kernel: csrc/learn/ntuple_beam.hip), a workgroup per board in
 * tpl_placement_beam's frame: 32 bytes read per board besides the table gathers, action u8 [n], plan u8 [n][depth] (optional),
 * score f32 [n] (optional), after_a / after_b [n] 16-byte words (both or neither) written; an output that is not given is not
 * written.  Refused before any HIP call, under the entry's own name: a shape that is neither of the two, before anything else;
 * everything tpl_ntuple_act refuses for its planes, n, L, M, table, action, after, score and gamma, in that order; depth outside
 * [1, TPL_NTUPLE_BEAM_MAX_DEPTH]; width outside [1, TPL_BEAM_MAX_WIDTH]. */
#define TPL_NTUPLE_BEAM_MAX_DEPTH 11
int tpl_ntuple_beam(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line, float r_win,
                    float r_lose, float gamma, const int32_t* table, int32_t depth, int32_t width, uint8_t* action, uint8_t* plan,
                    float* score, void* after_a, void* after_b, int32_t shape, void* stream);

/* Two shapes summed in one value: the standard form of an n-tuple network, a 2 x 4 and a 3 x 3 table read for the same board.
 *
 * SUM TABLE: one int32 buffer of TPL_NTUPLE_ENTRIES_SUM = TPL_NTUPLE_ENTRIES + TPL_NTUPLE_ENTRIES_3X3 = 905,216 entries
 * (3,620,864 bytes), 16-byte aligned, in units of 2^-16: a whole 2 x 4 table at entry 0, then a whole 3 x 3 table at entry
 * 314,368 (byte 1,257,472, a multiple of 16), each with its own 1,024 counters.  Each part is by itself a valid table of its
 * shape for every entry above.
 * Value:   V(s) = float32(S_2x4 + S_3x3) * 2^-16   for a running s, 0 otherwise
 *   -- each S the exact 64-bit sum of its part as stated above: the non-empty tuples of the part's windows under the falling
 *   piece, plus the part's counter entry (the same k in both).  The two integers are added BEFORE the one rounding; this is not
 *   float32(S_2x4) + float32(S_3x3), which rounds twice and differs from it on sums wider than 24 bits.
 * Everything else is the rule of the entry of the same name with this V in place of the table's: the scores r + gamma V of
 * tpl_ntuple_act, the two-ply Q of tpl_ntuple_search, the fold, the candidates, the ties and the effective depth of
 * tpl_ntuple_beam; the epsilon draw, `second`, `plan`, `after` and `value`.  With one part all zero every output is, bit for bit,
 * what the other part gives under the entry of its shape.
 * Update: there is no new entry, and the layout is why.  The update kernels never read the table, so a TD error e of the summed
 * value is applied by sending the same error array through the _shaped update entry once per part: TPL_NTUPLE_SHAPE_2X4 at the
 * buffer's base, TPL_NTUPLE_SHAPE_3X3 at entry TPL_NTUPLE_ENTRIES.  This holds for tpl_ntuple_update_shaped, for
 * tpl_ntuple_update_trace_shaped (with symmetric != 0 each part under its own sigma, so a sum table is mirror-symmetric when both
 * parts are) and for tpl_ntuple_update_coherent_shaped, whose buffer is int64 [TPL_NTUPLE_ENTRIES_SUM][2] (14,483,456 bytes) laid
 * out the same way: the second part at entry 314,368, byte 5,029,888, again a multiple of 16.  Every add is an integer add of a
 * value that depends on no table entry, so the bytes of both buffers are the same whatever order the adds -- and the two calls'
 * kernels -- arrive in.  A state adds to the entries of both parts, about twice as many as under one shape: the step of V per unit
 * of rate roughly doubles, as it does under symmetry.
 *
 * Each _sum entry takes the arguments of the entry of the same name (tpl_ntuple_beam_sum: tpl_ntuple_beam's without `shape`), with
 * `table` a sum table, and refuses what that entry refuses, in its order, under its own name, before any HIP call.  The sum is NOT
 * a third tpl_ntuple_shape: tpl_ntuple_entries(2) stays -1 and the _shaped entries keep refusing it.  One kernel each
 * (ntuple_sum_value_kernel, ntuple_sum_act_kernel, ntuple_sum_search_kernel: csrc/learn/ntuple.hip; ntuple_beam_sum_kernel:
 * csrc/learn/ntuple_beam.hip) in the frames of their twins: the same device bodies under a composite geometry whose board sum is
 * the two parts' gather loops one after the other, from one table pointer. */
#define TPL_NTUPLE_ENTRIES_SUM (TPL_NTUPLE_ENTRIES + TPL_NTUPLE_ENTRIES_3X3)
int tpl_ntuple_value_sum(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const int32_t* table,
                         float* value, void* stream);
int tpl_ntuple_act_sum(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line, float r_win,
                       float r_lose, float gamma, const int32_t* table, float epsilon, uint64_t seed, uint64_t step,
                       uint8_t* action, float* score, void* after_a, void* after_b, float* value, void* stream);
int tpl_ntuple_search_sum(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line, float r_win,
                          float r_lose, float gamma, const int32_t* table, float epsilon, uint64_t seed, uint64_t step,
                          uint8_t* action, uint8_t* second, float* score, void* after_a, void* after_b, float* value,
                          void* stream);
int tpl_ntuple_beam_sum(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line, float r_win,
                        float r_lose, float gamma, const int32_t* table, int32_t depth, int32_t width, uint8_t* action,
                        uint8_t* plan, float* score, void* after_a, void* after_b, void* stream);

/* Staged tables: the weights split by game stage, the stage read from the lines and moves that are left.  In every table above the
 * move budget enters the value additively, V = f(board, piece) + counter[k]; a staged table holds TPL_NTUPLE_STAGES = 8 whole tables
 * and lets k choose which one is read, so that the same stack can be worth one thing with three moves left and another with thirty.
 *
 * STAGED TABLE of a FORM F -- TPL_NTUPLE_FORM_2X4 = 0, TPL_NTUPLE_FORM_3X3 = 1 (the two shapes) or TPL_NTUPLE_FORM_SUM = 2 (the sum
 * table) -- with E_F = 314,368, 590,848 or 905,216 entries: one int32 buffer, 16-byte aligned, of 8 E_F + 1,024 entries --
 *   TPL_NTUPLE_ENTRIES_STAGED     = 2,515,968   (10,063,872 bytes)
 *   TPL_NTUPLE_ENTRIES_STAGED_3X3 = 4,727,808   (18,911,232 bytes)
 *   TPL_NTUPLE_ENTRIES_STAGED_SUM = 7,242,752   (28,971,008 bytes)
 * -- counts that no table and no coherence buffer above has, so a buffer's form still follows from its entry count:
 *   block[g]  at entry g * E_F          g in 0..7: a whole table of form F, in units of 2^-16, with its own counters (a sum: both parts')
 *   map[k]    at entry 8 * E_F + k      k in 0..1023, the counter index: the STAGE MAP
 * E_F is a multiple of 512, so every block (and the second part of a sum's block) starts at a multiple of 16 bytes and of both
 * shapes' pattern counts, and the first E_F entries are by themselves a valid plain table of the form.
 * Stage:   g(s) = map[k(s)] & 7, k(s) the counter index of s under the game's L and M.  THE MASK IS PART OF THE RULE: a map that
 *   holds anything at all, random words included, names a block of the buffer, and no kernel trusts device memory for a bound.
 * Value:   V(s) is the value of form F stated above read from block[g(s)] -- the block's windows under the falling piece plus the
 *   block's OWN counter entry (of a sum: both parts'), exact in 64 bits, ONE rounding, times 2^-16; 0 for a state that is not running.
 * The stage is looked up wherever a table is read, state by state: the afterstates of tpl_ntuple_act, the second-ply boards of
 * tpl_ntuple_search and every child of tpl_ntuple_beam are each valued in the block of THEIR OWN lines and moves left, which differ
 * from the root's.  Everything else is the rule of the entry of the same name with this V: scores, Q, the fold, candidates, ties, the
 * effective depth, the epsilon draw, `second`, `plan`, `after`, `value`.  With eight equal blocks every output is, bit for bit, what
 * the block gives as a plain table under the entry of its form, whatever the map holds.  A map that uses two or four stages leaves
 * the other blocks untouched: they cost memory only.
 * Update (tpl_ntuple_update_trace_staged): tpl_ntuple_update_trace_shaped's rule -- d_k, the trace cut, the decay, the mirror image --
 *   with every add of a state made in block[g(that state)]: the windows' entries and the counter entry, at g * E_F + the index above.
 *   The reflected board has the state's lines and moves, hence its stage: a staged table whose blocks are each mirror-symmetric stays
 *   so.  For TPL_NTUPLE_FORM_SUM both parts of the block take the same d_k, each under its own sigma.  The map is READ and never
 *   written; the blocks are added to and never read, so the bytes are the same whatever order the adds arrive in.  The planes form
 *   (tpl_ntuple_update) is a ring of one slot: slots = 1, head = 0, horizon = 1.  There is NO coherent update of a staged table.
 *
 * Each _staged entry takes the arguments of its _shaped twin (tpl_ntuple_beam_staged: tpl_ntuple_beam's) with `form` in the place of
 * `shape` and `table` a staged table of that form, and refuses what the twin refuses, in its order, under its own name, before any
 * HIP call; refused before anything else, and before any pointer is looked at: a form that is none of the three.  Kernels: the device
 * bodies of the twins under a composite geometry (StagedOf: csrc/learn/tpl_ntuple.h) -- one extra dword gathered from the 4 KB map per
 * board sum, the block's offset inside the 32-bit entry index, the table pointer uniform -- ntuple_staged_{value,act,search}_kernel,
 * ntuple_staged3_*, ntuple_staged_sum_* (ntuple.hip) and ntuple_staged_beam_kernel, ntuple_staged_beam3_kernel,
 * ntuple_staged_beam_sum_kernel (ntuple_beam.hip).  The update launches ntuple_staged_trace_kernel<symmetric> on the 2 x 4 part of
 * every block, ntuple_staged3_trace_kernel<symmetric> on the 3 x 3 part, or both for a sum: a lane per (board, age), no sync and
 * nothing allocated. */
#define TPL_NTUPLE_STAGES 8
typedef enum { TPL_NTUPLE_FORM_2X4 = 0, TPL_NTUPLE_FORM_3X3 = 1, TPL_NTUPLE_FORM_SUM = 2 } tpl_ntuple_form;
#define TPL_NTUPLE_ENTRIES_STAGED (TPL_NTUPLE_STAGES * TPL_NTUPLE_ENTRIES + 1024)
#define TPL_NTUPLE_ENTRIES_STAGED_3X3 (TPL_NTUPLE_STAGES * TPL_NTUPLE_ENTRIES_3X3 + 1024)
#define TPL_NTUPLE_ENTRIES_STAGED_SUM (TPL_NTUPLE_STAGES * TPL_NTUPLE_ENTRIES_SUM + 1024)
int tpl_ntuple_value_staged(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const int32_t* table,
                            float* value, int32_t form, void* stream);
int tpl_ntuple_act_staged(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line, float r_win,
                          float r_lose, float gamma, const int32_t* table, float epsilon, uint64_t seed, uint64_t step,
                          uint8_t* action, float* score, void* after_a, void* after_b, float* value, int32_t form, void* stream);
int tpl_ntuple_search_staged(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line, float r_win,
                             float r_lose, float gamma, const int32_t* table, float epsilon, uint64_t seed, uint64_t step,
                             uint8_t* action, uint8_t* second, float* score, void* after_a, void* after_b, float* value,
                             int32_t form, void* stream);
int tpl_ntuple_beam_staged(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line, float r_win,
                           float r_lose, float gamma, const int32_t* table, int32_t depth, int32_t width, uint8_t* action,
                           uint8_t* plan, float* score, void* after_a, void* after_b, int32_t form, void* stream);
int tpl_ntuple_update_trace_staged(const void* ring_a, const void* ring_b, int64_t n, int32_t slots, int32_t head, int32_t horizon,
                                   int32_t L, int32_t M, int32_t* table, const float* error, float rate, float decay,
                                   int32_t symmetric, int32_t form, void* stream);

/* Feature tuples: n-tuple tables indexed by nine board features.  Every window above is local -- 2 x 4 or 3 x 3 cells --, and the
 * quantities that carry the hand-made score of tpl_placement_act are global counts: no sum of local windows can express a threshold
 * on them.  A feature tuple is a 256-entry row per (falling piece, feature), looked up at the feature's value: the
 * piecewise-constant generalisation of that linear score, learned by the TD rule above.
 *
 * Features: phi_3 .. phi_11 of the board as stated for tpl_placement_features -- holes, aggregate_height, max_height, bumpiness,
 *   row_transitions, column_transitions, wells, rows_with_holes, hole_depth --, numbered j = 0 .. 8 in that order.
 * Bin:     q_j = min(phi_{3+j}, 255).  Only wells can pass 255 (950 on a comb board); THE CLAMP IS PART OF THE RULE.
 * FEATURE TABLE: int32 [TPL_NTUPLE_ENTRIES_FEAT = 19,456] (77,824 bytes), 16-byte aligned, in units of 2^-16:
 *   feature[p][j][q]  at index (p * 9 + j) * 256 + q    p in 0..7 the falling piece, j in 0..8, q in 0..255: 18,432 entries
 *   counter[k]        at index 18,432 + k               k the counter index above
 * All nine feature entries and the counter are ALWAYS used.  There is no "empty pattern" exception: a board with 0 holes reads bin 0.
 * Value:   V(s) = float32(S) * 2^-16 for a running s, S the exact 64-bit sum of its ten entries, rounded once; 0 otherwise.
 * The sum form (TPL_NTUPLE_FEATURE_FORM_3X3): int32 [TPL_NTUPLE_ENTRIES_3X3_FEAT = 610,304], a whole 3 x 3 table at entry 0 and behind
 *   it, at entry 590,848 (byte 2,363,392, a multiple of 16), a whole feature table, each with its own counters.
 *   V(s) = float32(S_3x3 + S_feat) * 2^-16: the two integers are added BEFORE the one rounding, as in "Two shapes summed".  With one
 *   part all zero every output is, bit for bit, what the other part gives alone.
 * Mirror image: all nine features are invariant under the left-right reflection of the board, so sigma moves only the piece through
 *   pi (L <-> J, S <-> Z) and keeps j and q: sigma(feature[p][j][q]) = feature[pi(p)][j][q], the counters stay.
 * Update (tpl_ntuple_update_trace_feature): tpl_ntuple_update_trace's rule -- d_k, the trace cut, the decay -- with d_k added to the
 *   nine feature entries and the counter entry of every state that takes part.  With symmetric != 0 every feature add is made a
 *   second time at (pi(p), j, q), also where the two entries are one (the pieces I, T, O and 7); the counter is added once.  It adds
 *   to a feature table only: the 3 x 3 part of a sum form goes through tpl_ntuple_update_trace_shaped with the same errors, the
 *   feature part, at entry 590,848, through this entry.  Nothing is read, every add is an integer add modulo 2^32: the bytes are
 *   the same whatever order the adds arrive in.  A state adds to 10 entries where it adds to about 107 of a 3 x 3 table.
 * There are no staged and no coherent feature tables: each would be eight more kernels, and neither raised a win rate in the record.
 *
 * tpl_ntuple_value_feature, _act_feature, _search_feature and _beam_feature take the arguments of tpl_ntuple_value_shaped, _act_shaped,
 * _search_shaped and tpl_ntuple_beam with `form` (tpl_ntuple_feature_form) where those take `shape`, and keep their checks, in their
 * order, under their own names, their outputs, their exploration draw and their ties; refused before anything else, and before any
 * pointer is looked at: a form that is neither of the two.  tpl_ntuple_update_trace_feature takes tpl_ntuple_update_trace_shaped's
 * arguments without `shape`.  tpl_ntuple_feature_bins writes the nine bins of every state, running or not, as uint8 [n][9]: the device
 * feature code without the gathers, for tests and inspection -- NOT a hot-path entry (a lane's nine byte stores are not coalesced); it
 * takes no L and M and refuses what the planes and n of the other entries are refused for.  Kernels: the device bodies of the twins under the geometries FeatureTable and SumOf<Shape3x3,
 * FeatureTable> (csrc/learn/tpl_ntuple.h), whose board sum is board_features on the column words the lane holds, nine gathers and
 * the counter -- ntuple_feature_{value,act,search}_kernel, ntuple_feature3_* (ntuple.hip), ntuple_feature_beam_kernel and
 * ntuple_feature3_beam_kernel (ntuple_beam.hip); the update is ntuple_feature_trace_kernel<symmetric>, whose blocks sum
 * their states' adds in an LDS image of the whole table (76 KB) and flush the non-zero sums with one atomic add each. */
#define TPL_NTUPLE_FEATURES 9
#define TPL_NTUPLE_FEATURE_BINS 256
#define TPL_NTUPLE_ENTRIES_FEAT 19456
#define TPL_NTUPLE_ENTRIES_3X3_FEAT 610304
#define TPL_NTUPLE_FEATURE_FORM_ALONE 0
#define TPL_NTUPLE_FEATURE_FORM_3X3 1
typedef enum { TPL_NTUPLE_FEATURE_ALONE = TPL_NTUPLE_FEATURE_FORM_ALONE, TPL_NTUPLE_FEATURE_WITH_3X3 = TPL_NTUPLE_FEATURE_FORM_3X3 } tpl_ntuple_feature_form;
int tpl_ntuple_value_feature(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const int32_t* table,
                             float* value, int32_t form, void* stream);
int tpl_ntuple_act_feature(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line, float r_win,
                           float r_lose, float gamma, const int32_t* table, float epsilon, uint64_t seed, uint64_t step,
                           uint8_t* action, float* score, void* after_a, void* after_b, float* value, int32_t form, void* stream);
int tpl_ntuple_search_feature(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line, float r_win,
                              float r_lose, float gamma, const int32_t* table, float epsilon, uint64_t seed, uint64_t step,
                              uint8_t* action, uint8_t* second, float* score, void* after_a, void* after_b, float* value,
                              int32_t form, void* stream);
int tpl_ntuple_beam_feature(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line, float r_win,
                            float r_lose, float gamma, const int32_t* table, int32_t depth, int32_t width, uint8_t* action,
                            uint8_t* plan, float* score, void* after_a, void* after_b, int32_t form, void* stream);
int tpl_ntuple_update_trace_feature(const void* ring_a, const void* ring_b, int64_t n, int32_t slots, int32_t head, int32_t horizon,
                                    int32_t L, int32_t M, int32_t* table, const float* error, float rate, float decay,
                                    int32_t symmetric, void* stream);
int tpl_ntuple_feature_bins(const void* plane_a, const void* plane_b, int64_t n, uint8_t* bins, void* stream);

/* The budget table: a feature table with a row for the spare cells of the move bound, and the dead-board prune.  A feature table sees
 * the move budget only through one additive counter entry, clamped at 15 lines and 63 moves; it cannot see the one quantity the game
 * is named after, the cells a board can still waste, and its policies keep valuing children that the move bound proves lost.
 *
 * BUDGET TABLE ("feat+spare"): int32 [TPL_NTUPLE_ENTRIES_BUDGET = 8 * 10 * 256 + 1,024 = 21,504] (86,016 bytes), 16-byte aligned, in
 * units of 2^-16:
 *   row[p][j][q]   at index (p * 10 + j) * 256 + q    p in 0..7 the falling piece, j in 0..9, q in 0..255: 20,480 entries
 *   counter[k]     at index 20,480 + k                k the counter index above
 * Rows j = 0 .. 8 are the feature table's, read at q_j = min(phi_{3+j}, 255).  Row 9 is read at
 *   sbin = dead ? 0 : min(spare + 1, 255),   spare = 4 (M - moves) - cells,   cells = cells(board, max(L - lines, 0)),   dead = spare < 0
 * -- exactly the move bound above (csrc/learn/tpl_placement.h: move_bound), from the board's OWN lines and moves under the game's L and
 * M, never from the clamped counter index k: at L = 20, M = 100 a fresh empty board has spare 200 and reads bin 201.  BOTH CLAMPS ARE
 * PART OF THE RULE, so no state addresses outside the buffer.  A finished board has spare 0 and is not dead: bin 1 (only
 * tpl_ntuple_budget_bins shows it).  No other form has 21,504 entries.
 * All ten row entries and the counter are ALWAYS used.
 * Value:   V(s) = float32(S) * 2^-16 for a running s, S the exact 64-bit sum of its eleven entries, rounded once; 0 otherwise.
 * Mirror image: the nine features and spare are invariant under the left-right reflection of the board (a row's fill is), so sigma
 *   moves only the piece: sigma(row[p][j][q]) = row[pi(p)][j][q], the counters stay.
 * Update (tpl_ntuple_update_trace_budget): tpl_ntuple_update_trace_feature's rule with eleven adds a state: d_k goes to the ten row
 *   entries and the counter entry; with symmetric != 0 every row add is made a second time at (pi(p), j, q), also where the two
 *   entries are one, and the counter is added once.  Nothing is read: the bytes are the same whatever order the adds arrive in.
 * There are no staged, no coherent and no summed budget tables.
 *
 * THE PRUNE is a flag of the three policies, `prune`, 0 by default in every caller.  With prune != 0, wherever a move -- the first
 * move, the second move of tpl_ntuple_search_budget, a move of any ply of tpl_ntuple_beam_budget -- leaves a RUNNING board that is
 * dead, the move is scored as one that ends the game lost at the limit: its reward is move_reward with that state (r_line * rows +
 * r_lose), there is no gamma * V term, and nothing is searched below it (in the beam the child is a finished node that competes with
 * its own value).  The prune enters scores and the arg-max only: after_a / after_b and `value` stay the true, running afterstate of
 * the action played and the table's value of it, because the environment plays on.  The exploration draw stays uniform over the
 * distinct placements.  With prune = 0, and row 9 all zero, every output is what the _feature entries give for the feature table with
 * the same nine rows and counters, bit for bit.
 *
 * tpl_ntuple_value_budget, _act_budget, _search_budget and _beam_budget take the arguments of their _feature twins without `form`; the
 * three policies take one more int32 `prune` before `stream`.  They keep the twins' checks, in their order, under their own names,
 * their outputs, their exploration draw and their ties.  tpl_ntuple_update_trace_budget takes tpl_ntuple_update_trace_feature's
 * arguments and checks.  tpl_ntuple_budget_bins writes the ten bins of every state, running or not, as uint8 [n][10] -- for tests and
 * inspection, NOT a hot-path entry --; it reads L and M and refuses what tpl_ntuple_value_budget refuses for the planes, n, L and M,
 * and a NULL bins.  Kernels: the device bodies of the twins under the geometry BudgetTable (csrc/learn/tpl_ntuple.h), whose board sum
 * is feature_bins and move_bound on the board the lane holds, ten gathers and the counter -- ntuple_budget_{value,act,search,bins}_kernel
 * (ntuple.hip), ntuple_budget_beam_kernel (ntuple_beam.hip); the update is ntuple_budget_trace_kernel<symmetric>, whose blocks sum
 * their states' adds in an LDS image of the whole table (84 KB: one block a CU) and flush the non-zero sums with one atomic add each. */
#define TPL_NTUPLE_BUDGET_ROWS 10
#define TPL_NTUPLE_ENTRIES_BUDGET 21504
int tpl_ntuple_value_budget(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const int32_t* table,
                            float* value, void* stream);
int tpl_ntuple_act_budget(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line, float r_win,
                          float r_lose, float gamma, const int32_t* table, float epsilon, uint64_t seed, uint64_t step,
                          uint8_t* action, float* score, void* after_a, void* after_b, float* value, int32_t prune, void* stream);
int tpl_ntuple_search_budget(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line, float r_win,
                             float r_lose, float gamma, const int32_t* table, float epsilon, uint64_t seed, uint64_t step,
                             uint8_t* action, uint8_t* second, float* score, void* after_a, void* after_b, float* value,
                             int32_t prune, void* stream);
int tpl_ntuple_beam_budget(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, float r_line, float r_win,
                           float r_lose, float gamma, const int32_t* table, int32_t depth, int32_t width, uint8_t* action,
                           uint8_t* plan, float* score, void* after_a, void* after_b, int32_t prune, void* stream);
int tpl_ntuple_update_trace_budget(const void* ring_a, const void* ring_b, int64_t n, int32_t slots, int32_t head, int32_t horizon,
                                   int32_t L, int32_t M, int32_t* table, const float* error, float rate, float decay,
                                   int32_t symmetric, void* stream);
int tpl_ntuple_budget_bins(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, uint8_t* bins, void* stream);

/* The exact depth-first solver with its children ordered by an n-tuple table (csrc/learn/ntuple_exact.hip).  tpl_ntuple_exact IS
 * tpl_placement_exact WITH ONE THING REPLACED: the value that orders a node's children.  Everything else is that search's, word for
 * word: the iterations at budget B from bound = need(root) to M (shortest = 1) or at M alone (shortest = 0); the children of a node --
 * the distinct placements of pieces[d] & 7 in ascending b, each made by move_board in the game (L, B), a child left running and dead
 * under (L, B) turned LOST at the limit (the bounded form, change 1); the stop at the first ply with a won child, taking the first won
 * child in the order; the descent into the running children in the order; nodes, the max_nodes cap checked before every expansion,
 * proved, solved, solution_len, actions and bound; and the case bound > M, in which there is no iteration.
 *
 * THE VALUE of the child made at depth d (the node has made d moves, the child d + 1) is what the one-ply n-tuple policy with the
 * dead-board prune scores a first move with, in the game (L, B) OF THE CURRENT ITERATION: with n the rows the move cleared and `state`
 * the child's state after the bounded form's change 1,
 *   reward = the reward rule (tpl_afterstates) on (r_line, r_win, r_lose, n, state)
 *   value  = reward + gamma * V     if the child runs      (one rounded multiply, one rounded add, contraction off)
 *   value  = reward                 otherwise
 *   V      = the value of `table` on the child's board with pieces[d + 1] & 7 as the falling piece, its own lines and moves, under
 *            (L, B) -- the sum exact in 64 bits, ONE rounding, the scaling by 2^-16 exact, as every n-tuple value here.
 * pieces[d + 1] exists: d + 1 <= M and a list has M + 1 entries.  V IS READ AT B, NOT AT M: the counter index and, under a budget
 * table, spare = 4 (B - moves) - cells are taken under the iteration's budget, so an iteration at the exact budget reads the low-spare
 * bins that a table trained on a tight pool has filled.  The clamps of the tables -- min(phi, 255), sbin, the 16 x 64 counters -- are
 * part of the rule, so no state addresses an entry outside the buffer.  The children are ordered by (value descending, b ascending);
 * -0 and +0 tie.
 *
 * THE TABLE is one of the four plain forms, told apart by `entries`: TPL_NTUPLE_ENTRIES ("2x4"), TPL_NTUPLE_ENTRIES_3X3 ("3x3"),
 * TPL_NTUPLE_ENTRIES_FEAT ("feat") or TPL_NTUPLE_ENTRIES_BUDGET ("feat+spare").  Any other count -- a sum table's and a staged
 * table's among them -- is refused with a message that names the four.
 *
 * Two consequences, on which the tests rest:
 *   1. UNDER proved = 1, solved, bound and (with shortest = 1) solution_len ARE INDEPENDENT OF THE TABLE and of the reward and gamma,
 *      and equal tpl_placement_exact's under any weights: a finished search has visited every running board of its budgets or met a
 *      win at the first budget that has one, in whatever order.
 *   2. For a configuration PROVED UNWINNABLE, nodes is independent of the order too: every running board of every budget is expanded
 *      once, whatever comes first.
 * What the table decides is how many nodes a WIN takes -- how soon the first budget that has one meets it -- and so how many proofs fit
 * in max_nodes.  WITH proved = 0 NOTHING IS PROVED, as there.  The result is a function of the inputs alone; nothing is written but
 * the outputs.
 *
 * Four kernels, one per form, of tpl_placement_exact's frame: ONE CONFIGURATION PER WAVEFRONT, lanes 0 .. 33 a child each, the order
 * from 64-bit keys ranked across the wave, the stack -- a record of 80 bytes a depth, without a carry -- in LDS sized by M.  The table
 * is read from global memory: eleven gathers a running child under "feat+spare", ten under "feat", the non-empty windows and the
 * counter under the window forms.  rows i16 [n][20], pieces u8 [n][M + 1] and table i32 [entries] are read; solved u8 [n], proved
 * u8 [n], solution_len i32 [n], actions u8 [n][M], bound i32 [n] and nodes u32 [n] are each written in full.
 * Refused before any HIP call: an `entries` that is none of the four, first; everything tpl_placement_exact refuses of the arguments
 * the two share (a NULL rows, pieces, solved, proved, solution_len, actions, bound or nodes, n < 1, n >= 2^31, L outside [1, 250] or M
 * outside [1, 254], max_nodes outside [1, TPL_EXACT_MAX_NODES], shortest other than 0 or 1, rows not 2-byte aligned, solution_len,
 * bound or nodes not 4-byte aligned); a NULL table, a table not 4-byte aligned; an r_line, r_win, r_lose or gamma that is not finite. */
int tpl_ntuple_exact(const int16_t* rows, const uint8_t* pieces, int64_t n, int32_t L, int32_t M, const int32_t* table, int64_t entries,
                     float r_line, float r_win, float r_lose, float gamma, int32_t max_nodes, int32_t shortest, uint8_t* solved,
                     uint8_t* proved, int32_t* solution_len, uint8_t* actions, int32_t* bound, uint32_t* nodes, void* stream);

/* The exact search over a state's window with its children ordered by an n-tuple table (csrc/learn/ntuple_window.hip).
 * tpl_ntuple_window_prove IS tpl_placement_window_prove WITH ONE THING REPLACED, exactly as tpl_ntuple_exact is tpl_placement_exact
 * with one thing replaced: the value that orders a node's children.  Everything of the window frame is unchanged: the two packed
 * planes; which board is running, finished or skipped; known = 12 - moves % 10, rem = M - moves, H = min(known, rem); the outputs
 * solved, proved, solution_len, plan [TPL_WINDOW_PLAN], bound, nodes, horizon and verdict; what is written for a finished board and
 * for a skipped board (NOT SEARCHED; bound and horizon are still written); the verdicts TPL_WINDOW_NONE / WIN / LOSS / OPEN and
 * what they mean.  VERDICT 3 PROVES NOTHING ABOUT THE GAME.
 *
 * THE SEARCH of a running, unskipped board IS tpl_ntuple_exact's WITH shortest = 1, run on the configuration whose rows are the
 * board's and whose list is q[0], ..., q[H - 1], 0 -- q the window's entries, the falling piece first -- in the game (L - lines, H).
 * solved, proved, solution_len, actions[0 .. H), bound and nodes are BYTE FOR BYTE what tpl_ntuple_exact writes for that
 * configuration; plan is actions padded with 255 to twelve entries.  Two things follow:
 *   - V IS READ AT THE ITERATION'S BUDGET B, under (L - lines, B): the counter index is that of the shifted game at the child's own
 *     lines' and moves', and under a budget table spare = 4 (B - moves') - cells.  An iteration below the horizon therefore reads
 *     the low-spare bins, as tpl_ntuple_exact does.
 *   - NOTHING DEPENDS ON THE ABSOLUTE lines OR moves, only on what is left: the search starts from a fresh root of the shifted game.
 *
 * KNOWN PIECES.  The child made at depth d is valued with q[d + 1] as its falling piece.  A child that runs has
 * d + 1 < B <= H <= known, so q[d + 1] is a TRUE piece of the episode: NO VALUE IS EVER READ UNDER A PIECE THE AGENT DOES NOT KNOW.
 * List entry H (index 12 where H = 12) is a defined 0; it is never used for a value.
 *
 * THE TABLE is one of the four plain forms, told apart by `entries` as tpl_ntuple_exact tells them apart; any other count is refused
 * first, with tpl_ntuple_exact's message.
 *
 * Two consequences, inherited from the two parents, on which the tests rest:
 *   1. UNDER proved = 1, solved, solution_len, bound and verdict ARE INDEPENDENT OF THE TABLE, gamma and the reward, and equal
 *      tpl_placement_window_prove's on the same board wherever that one is proved too.
 *   2. For a board searched out without a win, nodes is independent of the order as well.
 *
 * Four kernels, one per form, of tpl_placement_window_prove's frame: ONE BOARD PER WAVEFRONT, the stack -- twelve records of 80
 * bytes, without a carry --, the shape table and sixteen bytes of pieces in static LDS, the table in global memory.
 * Refused before any HIP call: an `entries` that is none of the four, first; then whatever tpl_ntuple_exact refuses of table, r_line,
 * r_win, r_lose and gamma (a NULL table, a table not 4-byte aligned, a value that is not finite) and whatever
 * tpl_placement_window_prove refuses of the planes, n, L, M, max_nodes, skip and the outputs. */
int tpl_ntuple_window_prove(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const int32_t* table,
                            int64_t entries, float r_line, float r_win, float r_lose, float gamma, int32_t max_nodes,
                            const uint8_t* skip, uint8_t* solved, uint8_t* proved, int32_t* solution_len, uint8_t* plan,
                            int32_t* bound, uint32_t* nodes, uint8_t* horizon, uint8_t* verdict, void* stream);

/* The exact searches in LIMITED-DISCREPANCY ORDER (Harvey and Ginsberg; csrc/learn/tpl_exact.h: search<Order, Limited = true>).  A proof
 * fits max_nodes or it does not, and on a winnable board the node count is a matter of child order alone.  Plain depth-first search
 * spends a budget badly when the order is good but not perfect: one wrong choice near the root, and the whole subtree below it is
 * searched out before the second child is tried.  The limited search tries the paths that follow the order everywhere first, then
 * those that leave it once, then twice, and so on until an iteration cuts nothing.
 *
 * Each _limited entry is its twin -- tpl_placement_exact[_move], tpl_placement_window_prove[_move], tpl_ntuple_exact,
 * tpl_ntuple_window_prove -- with three more arguments: int32 first_limit in [0, 65535] and int32 growth in {0, 1} behind max_nodes and
 * shortest, and the output limit i32 [n] behind nodes.  The children, their values, their order, the stop, the node cap, the budgets,
 * the frames and the verdicts are the twin's.  THE RULE is the twin's search with one more loop and one more number at a node:
 *   AN ITERATION is (B, K): the game (L, B) as before, searched under the discrepancy limit K.  The root is given rem = K.
 *   A node with rem is EXPANDED exactly as in the plain search: the node count is checked and counted, every distinct placement of its
 *     piece is made, and a dead child is lost.
 *   If ANY child is won the iteration ends with the won child that comes first in the order, WHATEVER ITS RANK.
 *   Otherwise the running children are ranked as in the plain search (value descending, placement ascending), rank 0 first.
 *     Only the children of rank <= rem are kept: the node has min(count, rem + 1) children to descend into.
 *     If a running child was dropped, the iteration's flag `cut` is set.
 *     The kept child of rank j is searched with rem - j.
 *   When the root's children are used up:
 *     cut is set:   the next iteration is (B, K'), from a fresh root, with cut cleared;
 *     cut is clear: nothing was dropped, so the iteration visited every running board the plain iteration at B visits.  The game
 *                   (L, B) is searched out, and the search goes on to B + 1 with K back at first_limit, or ends, as the plain one.
 *   K' = K + 1 with growth = 0 ("add"), K' = max(1, 2 K) with growth = 1 ("double"); K' is clamped at 65,535 either way.  A path has
 *     at most 253 nodes above the one expanded and a rank is at most 33, so a K >= 8,382 never cuts.
 *   nodes counts the expansions of ALL iterations (B, K); nodes == max_nodes ends the whole search and proves nothing, as in the twin.
 *   limit is the K of the last iteration begun, and 0 where there was no iteration (bound > M; a finished or skipped board).
 * Consequences:
 *   1. VERDICTS DO NOT CHANGE.  Under proved = 1, solved, solution_len, bound and unwinnable (solved = 0) are the plain search's, for
 *      any first_limit and growth, because the last iteration at every budget cut nothing.  The window entries' verdicts (1 WIN,
 *      2 LOSS, 3 OPEN) are defined from solved, proved and the horizon as in the twin: VERDICT 3 STILL PROVES NOTHING ABOUT THE GAME.
 *   2. THE SOLUTION MAY DIFFER.  actions (plan) may name a different win of the same length.  It is still a shortest win, and it
 *      replays to a win in exactly solution_len moves.
 *   3. first_limit >= 8,382 gives the plain search's outputs BYTE FOR BYTE: all six (eight) outputs, the path as well.
 *   4. THE WORST CASE for a budget with no win is bounded.  If the plain search takes T nodes to search that budget out, the limited
 *      search takes at most 15 T under "double" -- the K values are 0, 1, 2, 4, .., 8,192 -- and up to 8,383 T under "add".  "add"
 *      found more wins at equal node budgets where it was measured; "double" is the choice where budgets below the shortest length must
 *      be exhausted.
 * With proved = 0 nothing is proved, as in the twin.  What limited-discrepancy order buys is proofs within max_nodes: whatever the plain
 * search proves within max_nodes under first_limit >= 8,382 it proves too; under a small first_limit a search may be capped that the
 * plain one finishes, and the other way round.
 * Kernels of the twins' frames with their own names and argument records: one wavefront a configuration or board, the same LDS, a
 * stack record of the same 80 bytes -- a node's rem is the upper half of its child count's word --, rem, K and cut in scalar
 * registers.  Refused before any HIP call: everything the twin refuses, first_limit outside [0, 65535], growth other than 0 or 1, a
 * NULL limit, limit not 4-byte aligned. */
int tpl_placement_exact_limited(const int16_t* rows, const uint8_t* pieces, int64_t n, int32_t L, int32_t M, const float* weights,
                                float spare_weight, int32_t max_nodes, int32_t shortest, int32_t first_limit, int32_t growth,
                                uint8_t* solved, uint8_t* proved, int32_t* solution_len, uint8_t* actions, int32_t* bound,
                                uint32_t* nodes, int32_t* limit, void* stream);
int tpl_placement_exact_limited_move(const int16_t* rows, const uint8_t* pieces, int64_t n, int32_t L, int32_t M, const float* weights,
                                     float spare_weight, int32_t max_nodes, int32_t shortest, int32_t first_limit, int32_t growth,
                                     uint8_t* solved, uint8_t* proved, int32_t* solution_len, uint8_t* actions, int32_t* bound,
                                     uint32_t* nodes, int32_t* limit, void* stream);
int tpl_placement_window_prove_limited(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const float* weights,
                                       float spare_weight, int32_t max_nodes, int32_t first_limit, int32_t growth, const uint8_t* skip,
                                       uint8_t* solved, uint8_t* proved, int32_t* solution_len, uint8_t* plan, int32_t* bound,
                                       uint32_t* nodes, int32_t* limit, uint8_t* horizon, uint8_t* verdict, void* stream);
int tpl_placement_window_prove_limited_move(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M,
                                            const float* weights, float spare_weight, int32_t max_nodes, int32_t first_limit,
                                            int32_t growth, const uint8_t* skip, uint8_t* solved, uint8_t* proved, int32_t* solution_len,
                                            uint8_t* plan, int32_t* bound, uint32_t* nodes, int32_t* limit, uint8_t* horizon,
                                            uint8_t* verdict, void* stream);
int tpl_ntuple_exact_limited(const int16_t* rows, const uint8_t* pieces, int64_t n, int32_t L, int32_t M, const int32_t* table,
                             int64_t entries, float r_line, float r_win, float r_lose, float gamma, int32_t max_nodes, int32_t shortest,
                             int32_t first_limit, int32_t growth, uint8_t* solved, uint8_t* proved, int32_t* solution_len,
                             uint8_t* actions, int32_t* bound, uint32_t* nodes, int32_t* limit, void* stream);
int tpl_ntuple_window_prove_limited(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const int32_t* table,
                                    int64_t entries, float r_line, float r_win, float r_lose, float gamma, int32_t max_nodes,
                                    int32_t first_limit, int32_t growth, const uint8_t* skip, uint8_t* solved, uint8_t* proved,
                                    int32_t* solution_len, uint8_t* plan, int32_t* bound, uint32_t* nodes, int32_t* limit,
                                    uint8_t* horizon, uint8_t* verdict, void* stream);

/* The ranking update: what a proved move label teaches a table (csrc/learn/ntuple_rank.hip).  tpl_placement_exact_labels labels every
 * placement of a board 1 (proved winning), 2 (proved losing) or 3 (unproved).  tpl_ntuple_rank reads such a row beside the board and a
 * table and says whether the table's one-ply policy already prefers a proved win to every proved loss; where it does not, it names the
 * hardest pair and the two afterstates to move.  It writes nothing but its outputs: THE TABLE IS READ ONLY.
 *
 * For a state s, its row label u8 [40], a table of one of the four plain forms (told apart by `entries` exactly as tpl_ntuple_exact
 * tells them: "2x4", "3x3", "feat", "feat+spare"; any other count is refused with the message that names the four), reward parameters, a
 * discount gamma, a margin and prune = 0 or 1:
 *   SCORES.  score(a) of every distinct placement a (a == canonical(cur, a)) is tpl_ntuple_act's score, bit for bit: the move and the pop
 *     of tpl_afterstates, reward = the reward rule on (rows cleared, state), score = reward where the move ends the game and
 *     reward + gamma * V(afterstate) where it runs -- one product and one add, each rounded once, never fused.  A finished board scores 0.
 *     prune is a flag of the budget form alone (prune = 1 with any other form is refused): with it a move into a RUNNING DEAD board is
 *     scored as lost at the limit, reward with r_lose and no gamma * V, as tpl_ntuple_act_budget scores it.
 *   SETS.  W = the distinct a with label[a] == 1, X = the distinct a with label[a] == 2.  Labels 0 and 3 take part in nothing, and
 *     neither does any other byte value, nor any label on an action that is not distinct: the row is not trusted to be well formed.
 *     LABEL 3 PROVES NOTHING AND TEACHES NOTHING.
 *   THE PAIR.  win = the lowest a at the maximum of score over W, loss = the lowest a at the maximum of score over X, greedy = the lowest
 *     a at the maximum over all distinct placements -- tpl_ntuple_act's action at epsilon 0; -0 and +0 tie (ordered_bits), as everywhere.
 *     A finished state, an empty W or an empty X is UNDECIDED: win = loss = 255, gap = 0, violated = 0, both errors 0, and both
 *     afterstates are the state itself, bit for bit (tpl_ntuple_act's convention).  greedy is still written, 0 for a finished board.
 *   THE VIOLATION.  gap = score(win) - score(loss), one float32 subtraction on the scores' own bits; violated = (gap <= margin).  A tie
 *     violates at margin 0 -- under the zero table every score ties and every decided node must teach.  A NaN gap does not violate.
 *   WHAT IS TAUGHT, a perceptron step on the hardest pair: err_win = +1.0f if violated AND score(win) held a gamma * V term (the child
 *     runs and the prune did not end it), else 0; err_loss = -1.0f under the same condition for loss, else 0.  A side that ended the game
 *     has no value to move and teaches nothing; the node can still be violated and is reported so.
 *     win_a / win_b and loss_a / loss_b are the two afterstates after the pop exactly as tpl_ntuple_act writes `after`: the true board,
 *     the spare bit kept, also under the prune.
 * TEACHING is two calls of the existing update entry of the table's form (tpl_ntuple_update_trace_shaped, _feature or _budget) on a ring
 * of one slot (slots = 1, head = 0, horizon = 1): the win planes with err_win, then the loss planes with err_loss; each adds
 * rint(rate * err) to the entries of its afterstate, with `symmetric` as given.  This entry never writes the table and the update never
 * reads it, so one step leaves the same bytes in any order of arrival, and two runs give the same table.
 *
 * One kernel per form (ntuple_rank_kernel, ntuple_rank3_kernel, ntuple_rank_feature_kernel, ntuple_rank_budget_kernel) in
 * tpl_ntuple_act's frame: eight boards a block, 40 lanes a board, three LDS maxima a board where the policy has one, no exploration
 * draw, no scratch.  Read: 32 + 40 bytes a board and the table gathers.  Written, each in full: win, loss, greedy, violated u8 [n];
 * gap, err_win, err_loss f32 [n]; win_a, win_b, loss_a, loss_b [n] 16-byte words.
 * Refused before any HIP call, under the entry's own name: an `entries` that is none of the four, first; then tpl_ntuple_act's plane, n,
 * L, M and table checks; a NULL label; any NULL output; a misaligned (16 bytes) afterstate plane or (4 bytes) float output; a margin,
 * gamma or reward parameter that is not finite; prune other than 0 or 1, or prune = 1 outside the budget form. */
int tpl_ntuple_rank(const void* plane_a, const void* plane_b, int64_t n, int32_t L, int32_t M, const int32_t* table, int64_t entries,
                    const uint8_t* label, float r_line, float r_win, float r_lose, float gamma, float margin, int32_t prune,
                    uint8_t* win, uint8_t* loss, uint8_t* greedy, uint8_t* violated, float* gap, float* err_win, float* err_loss,
                    void* win_a, void* win_b, void* loss_a, void* loss_b, void* stream);

/* Per-configuration tallies and the resampled pool (csrc/learn/curriculum.hip).  Which pool entry a board plays is not stored anywhere:
 * the environment derives it (csrc/tpl_device.h, tetris_piclim.h's tpl_create).  These three entries derive it the same way from the
 * side and only READ the environment -- the planes (tpl_state_ptrs), the step clocks (tpl_clock_ptr: one uint64 per 32 boards) and the
 * handle's global_offset, seed and assignment mode, all passed in by the caller: no entry of libtetris_piclim.so is involved.
 *
 * THE RULE.  A RUNNING board i made one move in every step of its episode, so the episode began at step  birth = clock[i / 32] -
 * moves_used(i),  and its entry is that of the episode of global board g = global_offset + i beginning at `birth`, in the buffer its slot
 * bit names (n_cfg0 entries for bit 0, n_cfg1 for bit 1):
 *   TPL_ASSIGN_SEQUENTIAL   (g mod n_cfg + low32(birth) mod n_cfg) mod n_cfg
 *   TPL_ASSIGN_HASH         x = (low32(g) + low32(birth) * 0x9E3779B1) ^ low32((g >> 32 & 0xFFFFFF) * 0x85EBCB)
 *                               ^ low32((birth >> 32 & 0xFFFFFF) * 0xC2B2AF) ^ (splitmix64(seed) >> 32),  all in 32 bits;
 *                           entry = (fmix32(x) * n_cfg) >> 32   (fmix32 = the murmur3 finaliser, splitmix64 = tpl_device.h's sm64)
 * An n_cfg of 0 (no such buffer) gives entry 0.
 *
 * tpl_config_index writes index[i] (uint32) for every RUNNING board and slot[i] (the bit) for every board; either output may be NULL,
 * not both.  A FINISHED, frozen board (auto_reset off) has no recoverable birth -- its clock runs on while moves_used stands still -- so
 * its index[i] is LEFT AS THE CALLER HAS IT: called on one buffer before every step, a finished board keeps the entry of the episode
 * it finished.  Refused: a null plane or clock, n outside [1, 2^31), planes not 16-byte or clock not 8-byte aligned, a negative
 * global_offset, an assign_mode other than 0 / 1, an n_cfg outside [0, 2^32), both n_cfg 0, both outputs null, a misaligned index.
 *
 * tpl_pool_tally is called just before tpl_step with the same `action` array (`dtype` TPL_U8 / TPL_I32 / TPL_I64; the low 32 bits are
 * the action, rot = action / 10 taken mod 4, loc = action mod 10, as tpl_step reads it).  For every RUNNING board it makes the move in
 * registers (the afterstate kernel's body) and, where the move ends the episode, adds 1 to episodes_s[entry] of the board's buffer s
 * and, where it ends won, 1 to wins_s[entry] (int32 [n_cfg_s] each).  Frozen boards add nothing; nothing of the environment is
 * written.  A buffer's pair may be NULL (both or neither; not both buffers'): ends on that buffer are not counted, so one launch serves
 * a pool in mid-swap.  No-return integer atomics, a wave's adds to one entry combined into one: the bytes do not depend on the order.
 * Refused: what tpl_config_index refuses for the environment, L outside [1, 250], M outside [1, 254], a null or misaligned action, a
 * bad dtype, a pair given by halves, no pair at all, a pair for a buffer of 0 entries, misaligned tallies.
 *
 * tpl_pool_resample gathers a reweighted pool.  rows uint16 [n_cfg][20], pieces uint8 [n_cfg][M + 1]; prefix int64 [n_cfg], the
 * INCLUSIVE prefix sums of non-negative int64 weights whose total prefix[n_cfg - 1] is in [1, 2^62) (the caller's to ensure; the
 * kernel stays inside the buffers whatever they hold).  Draw j < count:
 *   h_j = mix64(key + 0x9E3779B97F4A7C15 * (j + 1)),  key = mix64(seed + 0x9E3779B97F4A7C15 * (round + 1))   (tpl_replay_sample's stream)
 *   t_j = floor(h_j * total / 2^64);   source[j] = the first entry e with prefix[e] > t_j
 * and rows_out[j], pieces_out[j] are the records of entry source[j] (int32 [count]).  An entry of weight 0 is never drawn.  Integers
 * throughout: the outputs equal _learn_lib.pool_resample byte for byte.  Refused: a null pointer, n_cfg or count outside [1, 2^31), M
 * outside [1, 254], rows / rows_out / prefix not 8-byte or source not 4-byte aligned, an output that is its input. */
int tpl_config_index(const void* plane_a, const void* plane_b, const void* clock, int64_t n, int64_t global_offset, uint64_t seed,
                     int32_t assign_mode, int64_t n_cfg0, int64_t n_cfg1, uint32_t* index, uint8_t* slot, void* stream);
int tpl_pool_tally(const void* plane_a, const void* plane_b, const void* clock, int64_t n, int32_t L, int32_t M, const void* action,
                   int32_t dtype, int64_t global_offset, uint64_t seed, int32_t assign_mode, int64_t n_cfg0, int64_t n_cfg1,
                   int32_t* episodes0, int32_t* wins0, int32_t* episodes1, int32_t* wins1, void* stream);
int tpl_pool_resample(const void* rows, const void* pieces, int64_t n_cfg, int32_t M, const int64_t* prefix, int64_t count,
                      uint64_t seed, uint64_t round, void* rows_out, void* pieces_out, int32_t* source, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* TPL_LEARN_H */
