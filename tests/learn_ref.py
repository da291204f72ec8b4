"""Plain host references for the learner's device data (tests only): the 32-byte state and the 80-byte replay record restated
from their documented layouts (DESIGN.md sections 2 and 9, include/tpl_learn.h), and the 217-feature observation built from
decoded fields in float64.  Nothing here calls the environment or learner libraries."""
import numpy as np

OBS_DIM = 217
RECORD_BYTES = 80
_C20 = np.uint32(0xFFFFF)


def _u32(x):
    return np.ascontiguousarray(x).view(np.uint32).reshape(-1, 4)


def decode_state(a, b) -> dict:
    """uint32/int32 [K, 4] plane pairs -> rows uint16 [K, 20] (bit x = column x), cur, nxt, lines, moves, state (0..3),
    slot (0/1) as uint8 [K] and the 36-bit piece window as uint64 [K].

        A.x = col0 | col1<<20     A.y = col1>>12 | col2<<8 | moves[3:0]<<28
        A.z = col3 | col4<<20     A.w = col4>>12 | col5<<8 | moves[7:4]<<28
        B.x = col6 | col7<<20     B.y = col7>>12 | col8<<8 | state<<28 | slot<<30
        B.z = col9 | lines<<20 | window[35:32]<<28          B.w = window[31:0]
    (column word: bit r = row r; window: twelve 3-bit ids, entry 0 = the current piece, entry 1 = the next)"""
    A, B = _u32(a), _u32(b)
    s8, s12, s20, s28 = np.uint32(8), np.uint32(12), np.uint32(20), np.uint32(28)
    cols = np.stack([
        A[:, 0] & _C20, ((A[:, 0] >> s20) | (A[:, 1] << s12)) & _C20, (A[:, 1] >> s8) & _C20,
        A[:, 2] & _C20, ((A[:, 2] >> s20) | (A[:, 3] << s12)) & _C20, (A[:, 3] >> s8) & _C20,
        B[:, 0] & _C20, ((B[:, 0] >> s20) | (B[:, 1] << s12)) & _C20, (B[:, 1] >> s8) & _C20,
        B[:, 2] & _C20], axis=1)                                                   # [K, 10]
    rows = np.zeros((A.shape[0], 20), dtype=np.uint16)
    for r in range(20):
        for x in range(10):
            rows[:, r] |= (((cols[:, x] >> np.uint32(r)) & np.uint32(1)) << np.uint32(x)).astype(np.uint16)
    window = (B[:, 3].astype(np.uint64) | ((B[:, 2] >> s28).astype(np.uint64) << np.uint64(32)))
    return dict(rows=rows,
                cur=(window & np.uint64(7)).astype(np.uint8),
                nxt=((window >> np.uint64(3)) & np.uint64(7)).astype(np.uint8),
                lines=((B[:, 2] >> s20) & np.uint32(0xFF)).astype(np.uint8),
                moves=((A[:, 1] >> s28) | ((A[:, 3] >> s28) << np.uint32(4))).astype(np.uint8),
                state=((B[:, 1] >> s28) & np.uint32(3)).astype(np.uint8),
                slot=((B[:, 1] >> np.uint32(30)) & np.uint32(1)).astype(np.uint8),
                window=window)


def pack_state(rows, lines, moves, state, slot, window):
    """The inverse of decode_state: fields -> (A, B) uint32 [K, 4]."""
    rows = np.asarray(rows, dtype=np.uint32).reshape(-1, 20)
    k = rows.shape[0]
    cols = np.zeros((k, 10), dtype=np.uint32)
    for x in range(10):
        for r in range(20):
            cols[:, x] |= ((rows[:, r] >> np.uint32(x)) & np.uint32(1)) << np.uint32(r)
    u = lambda v: np.broadcast_to(np.asarray(v, dtype=np.uint64), (k,)).astype(np.uint32)
    window = np.broadcast_to(np.asarray(window, dtype=np.uint64), (k,))
    lines, moves, state, slot = u(lines), u(moves), u(state), u(slot)
    A, B = np.zeros((k, 4), np.uint32), np.zeros((k, 4), np.uint32)
    A[:, 0] = cols[:, 0] | (cols[:, 1] << np.uint32(20))
    A[:, 1] = (cols[:, 1] >> np.uint32(12)) | (cols[:, 2] << np.uint32(8)) | ((moves & np.uint32(15)) << np.uint32(28))
    A[:, 2] = cols[:, 3] | (cols[:, 4] << np.uint32(20))
    A[:, 3] = (cols[:, 4] >> np.uint32(12)) | (cols[:, 5] << np.uint32(8)) | ((moves >> np.uint32(4)) << np.uint32(28))
    B[:, 0] = cols[:, 6] | (cols[:, 7] << np.uint32(20))
    B[:, 1] = ((cols[:, 7] >> np.uint32(12)) | (cols[:, 8] << np.uint32(8)) | (state << np.uint32(28))
               | (slot << np.uint32(30)))
    B[:, 2] = cols[:, 9] | (lines << np.uint32(20)) | ((window >> np.uint64(32)).astype(np.uint32) << np.uint32(28))
    B[:, 3] = (window & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    return A, B


def decode_records(ring_bytes) -> dict:
    """[capacity, 80] (or flat) record bytes -> s (decode_state fields), the raw s / s' planes (uint32 [K, 4] each), reward
    bits uint32 [K], action u8, done u8 and the ten tail bytes 70..79 u8 [K, 10]."""
    rec = np.ascontiguousarray(ring_bytes, dtype=np.uint8).reshape(-1, RECORD_BYTES)
    words = rec.view(np.uint32)                                                     # [K, 20]
    out = dict(s=decode_state(words[:, 0:4], words[:, 4:8]))
    out.update(sa=words[:, 0:4].copy(), sb=words[:, 4:8].copy(), na=words[:, 8:12].copy(), nb=words[:, 12:16].copy(),
               reward_bits=words[:, 16].copy(), action=rec[:, 68].copy(), done=rec[:, 69].copy(), tail=rec[:, 70:80].copy())
    return out


def obs_from_fields(fields, L, M) -> np.ndarray:
    """float64 [K, 217]: the 200 cells row-major (cell 10 y + x = bit x of rows[y]), one-hot cur and one-hot nxt (id 7 sets
    nothing), L - lines and M - moves (negative values kept), and the terminal flag state != 0."""
    rows = np.asarray(fields["rows"]).view(np.uint16).reshape(-1, 20).astype(np.int64)
    k = rows.shape[0]
    out = np.zeros((k, OBS_DIM), dtype=np.float64)
    for y in range(20):
        for x in range(10):
            out[:, 10 * y + x] = (rows[:, y] >> x) & 1
    ids = np.arange(7)
    out[:, 200:207] = np.asarray(fields["cur"]).astype(np.int64)[:, None] == ids
    out[:, 207:214] = np.asarray(fields["nxt"]).astype(np.int64)[:, None] == ids
    out[:, 214] = float(L) - np.asarray(fields["lines"]).astype(np.float64)
    out[:, 215] = float(M) - np.asarray(fields["moves"]).astype(np.float64)
    out[:, 216] = np.asarray(fields["state"]) != 0
    return out


def mlp64(obs, params):
    """Model(217, 14) in float64 on the host: params = [(w, b)] * 5 as numpy arrays (torch layout), ReLU between layers."""
    x = np.asarray(obs, dtype=np.float64)
    for i, (w, b) in enumerate(params):
        x = x @ np.asarray(w, np.float64).T + np.asarray(b, np.float64)
        if i < 4:
            x = np.maximum(x, 0.0)
    return x


def random_fields(gen, k, M=255):
    """k states at the ends of every field: random boards (some empty, some full), moves 0..M, lines 0..255, state 0..3,
    slot 0/1 and all 36 window bits (so every piece id 0..7 as cur and nxt)."""
    rows = gen.integers(0, 1 << 10, (k, 20)).astype(np.uint16)
    rows[0::7] = 0
    rows[3::11] = 0x3FF
    moves = gen.integers(0, M + 1, k)
    moves[:2] = (0, M)
    lines = gen.integers(0, 256, k)
    lines[:2] = (255, 0)
    window = gen.integers(0, 1 << 36, k, dtype=np.int64).astype(np.uint64)
    window[:2] = ((1 << 36) - 1, 0)
    return dict(rows=rows, lines=lines, moves=moves, state=gen.integers(0, 4, k), slot=gen.integers(0, 2, k), window=window)
