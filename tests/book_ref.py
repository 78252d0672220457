"""Self-play's opening-book restart (gmz_engine_play_book of include/gmz.h) as a plain numpy model, written from the
header's text and not from openings.py or csrc/gmz_tree.hip: the two draw words, the multiply-shift, the square's
eight maps as numpy transposes and flips of the 2-D board, and one play_book step over host arrays (the move and the
end test are tests/game_ref.py's).  tests/test_book.py pins openings.py to it, tests/test_book_gpu.py the kernel."""
import numpy as np

import game_ref
from noise_ref import M32, _u64, mix32, row_word

SALT_OPEN = 0xB5297A4D  # GMZ_BOOK_SALT_OPEN
SALT_SYM = 0x27D4EB2F   # GMZ_BOOK_SALT_SYM


def h1(seed, key, serial):
    """The row hash the draw shares with the noise: mix32(lo(seed) ^ mix32(serial * C1 + key * C2))."""
    return mix32((_u64(seed) & M32) ^ mix32(row_word(serial, key)))


def word(seed, key, serial, salt):
    """w(salt) = mix32(h1 ^ hi(seed) ^ salt); broadcasts over key and serial."""
    return mix32(h1(seed, key, serial) ^ (_u64(seed) >> np.uint64(32)) ^ np.uint64(salt))


def draw(seed, key, serial, n, symmetry):
    """(t, d) of the game (key, serial): t = (w(SALT_OPEN) * n) >> 32, d = w(SALT_SYM) & 7 or 0."""
    t = (word(seed, key, serial, SALT_OPEN) * np.uint64(n)) >> np.uint64(32)
    d = word(seed, key, serial, SALT_SYM) & np.uint64(7)
    if not symmetry:
        d = d * np.uint64(0)
    return t.astype(np.int64), d.astype(np.int64)


def transform_board(board, size, d):
    """``board`` (size^2 cells) under symmetry d, as array operations on the 2-D board: the stone at (r, c) goes to
    (c, r) under bit 0 (a transpose), then to (S-1-r, c) under bit 1 (rows reversed), then to (r, S-1-c) under bit 2
    (columns reversed)."""
    b = np.asarray(board).reshape(size, size)
    if d & 1:
        b = b.T
    if d & 2:
        b = b[::-1, :]
    if d & 4:
        b = b[:, ::-1]
    return np.ascontiguousarray(b).reshape(-1)


def transform_cell(cell, size, d):
    """Where ``cell`` goes under symmetry d (-1 stays -1): a marker carried by transform_board."""
    if cell < 0:
        return -1
    m = np.zeros(size * size, np.int8)
    m[cell] = 1
    return int(np.argmax(transform_board(m, size, d)))


def play_book(state, actions, book, seed, symmetry, n_in_row, game_offset=0, tally=None):
    """One gmz_engine_play_book call on host arrays.  ``state``: dict(boards int8 [G, A], players int8 [G], last
    int32 [G], counts int32 [G], serial int32 [G], draw int32 [G]), changed in place; ``book`` = (boards [n, A],
    players, last, counts); ``tally`` int32 [n, 3] or None, changed in place.  Returns the status int8 [G]."""
    bb, bp, bl, bc = book
    n = len(bp)
    G, A = state["boards"].shape
    size = int(round(A ** 0.5))
    status = np.zeros(G, np.int8)
    for g in range(G):
        st, p, lm, mc = game_ref.play(state["boards"][g], int(state["players"][g]), int(state["last"][g]),
                                      int(state["counts"][g]), int(actions[g]), n_in_row, False)
        status[g] = st
        state["players"][g], state["last"][g], state["counts"][g] = p, lm, mc
        ended = st in (1, -1, 0)
        if not ended and state["serial"][g] != -1:
            continue
        if ended and state["serial"][g] >= 0 and tally is not None:
            tally[int(state["draw"][g]) >> 3, {1: 0, -1: 1, 0: 2}[st]] += 1
        state["serial"][g] += 1
        t, d = draw(seed, g + game_offset, int(state["serial"][g]), n, symmetry)
        t, d = int(t), int(d)
        state["boards"][g] = transform_board(np.asarray(bb)[t], size, d)
        state["players"][g] = bp[t]
        state["last"][g] = transform_cell(int(bl[t]), size, d)
        state["counts"][g] = bc[t]
        state["draw"][g] = 8 * t + d
    return status


def empty_state(G, A):
    """The state before the first call: empty boards, black to move, serial -1 everywhere."""
    return dict(boards=np.zeros((G, A), np.int8), players=np.ones(G, np.int8), last=np.full(G, -1, np.int32),
                counts=np.zeros(G, np.int32), serial=np.full(G, -1, np.int32), draw=np.full(G, -1, np.int32))
