"""The rules of the game as a plain numpy/Python model, and the directed positions the rule kernels are held to.

The model is written from what the reference's game.py means, not from csrc/gmz_device.h: a move wins when the
unbroken run of the mover's stones through it, along a row, a column or either diagonal, is at least n_in_row long
(overlines win); otherwise the game is drawn once move_count reaches size^2; otherwise it goes on.  The lines are
taken as numpy rows, columns and diagonals, so no flat-index stepping or border test of the kernels is repeated here.
tests/test_game_ref.py pins the model to the C oracle and to tests/golden/game_cases.npz;
tests/test_game_rules_gpu.py runs cases() through the kernels.

Status codes (include/gmz.h): +1/-1 winner, 0 draw, 2 not ended, 3 untouched (action < 0)."""
import functools
import math

import numpy as np

SIZES = (5, 6, 9, 15, 19, 22)
N_IN_ROWS = (3, 4, 5, 6)
PAIRS = tuple((s, n) for s in SIZES for n in N_IN_ROWS if n <= s)
DIRS = ((0, 1), (1, 0), (1, 1), (1, -1))


# ------------------------------------------------------------------------------------------ the model
def _line_through(b2, r, c, d):
    """The whole board line of direction DIRS[d] through (r, c) as a 1-D view, and the cell's index in it."""
    size = b2.shape[0]
    if d == 0:
        return b2[r, :], c
    if d == 1:
        return b2[:, c], r
    if d == 2:
        return np.diagonal(b2, c - r), min(r, c)
    cc = size - 1 - c  # the anti-diagonal is a diagonal of the mirrored board
    return np.diagonal(b2[:, ::-1], cc - r), min(r, cc)


def check_win(board, size, n_in_row, r, c):
    """True when the stone at (r, c) lies in an unbroken run of its colour at least n_in_row long."""
    b2 = np.asarray(board).reshape(size, size)
    p = int(b2[r, c])
    if p == 0:
        return False
    for d in range(4):
        line, i = _line_through(b2, r, c, d)
        line = line.tolist()
        lo = hi = i
        while lo > 0 and line[lo - 1] == p:
            lo -= 1
        while hi + 1 < len(line) and line[hi + 1] == p:
            hi += 1
        if hi - lo + 1 >= n_in_row:
            return True
    return False


def win_map(board, size, n_in_row):
    """check_win at every cell, uint8 [size^2] (an empty cell never wins)."""
    b = np.asarray(board).reshape(-1)
    out = np.zeros(size * size, np.uint8)
    for a in np.flatnonzero(b):
        out[a] = check_win(b, size, n_in_row, a // size, a % size)
    return out


def play(board, player, last, count, action, n_in_row, reset_finished):
    """One move on ``board`` (int8 [size^2], changed in place): -> (status, player, last, count) afterwards.
    action < 0 touches nothing (status 3); with reset_finished an ended game restarts empty, player 1 to move."""
    if action < 0:
        return 3, player, last, count
    A = board.size
    size = math.isqrt(A)
    board[action] = player
    count += 1
    if check_win(board, size, n_in_row, action // size, action % size):
        status = int(player)  # a win on the board's last empty cell is a win, not a draw
    elif count >= A:
        status = 0
    else:
        status = 2
    if reset_finished and status != 2:
        board[:] = 0
        return status, 1, -1, 0
    return status, -player, action, count


def board_state(board, size, player, last):
    """The observation planes, float32 [3, size, size]: the mover's stones, the opponent's, the last move."""
    b2 = np.asarray(board).reshape(size, size)
    out = np.zeros((3, size, size), np.float32)
    out[0] = b2 == player
    out[1] = b2 == -player
    if last is not None and last >= 0:
        out[2, last // size, last % size] = 1
    return out


# ------------------------------------------------------------------------------------------ directed positions
def _anchors(size, d, L):
    """Start cells of a run of L cells along DIRS[d] that touch every border and corner the direction allows, and
    one away from the borders."""
    m = size - L
    mid = (size // 2, m // 2)
    if d == 0:
        cand = [(0, 0), (0, m), (size - 1, 0), (size - 1, m), mid]
    elif d == 1:
        cand = [(0, 0), (m, 0), (0, size - 1), (m, size - 1), mid[::-1]]
    elif d == 2:
        cand = [(0, 0), (m, m), (0, m), (m, 0), (m // 2, (m + 1) // 2)]
    else:
        cand = [(0, size - 1), (m, L - 1), (0, L - 1), (m, size - 1), (m // 2, size - 1 - (m + 1) // 2)]
    out = []
    for rc in cand:
        if rc not in out:
            out.append(rc)
    return out


def _pattern(size):
    """A full board without three in a row in any direction: pairs along the rows, shifted two cells per row."""
    r, c = np.mgrid[0:size, 0:size]
    return np.where((c + 2 * r) % 4 < 2, 1, -1).astype(np.int8).reshape(-1)


@functools.lru_cache(maxsize=None)
def cases(size, n):
    """The positions of one (size, n_in_row): dict(boards int8 [G, A], players int8 [G] (the mover), last int32 [G],
    counts int32 [G], actions int32 [G], expect int8 [G] (the status the construction intends), tags [G]).  Arrays
    are read-only and shared."""
    A = size * size
    rows = []
    flip = [1]

    def add(tag, mover_cells, opp_cells, action, expect, board=None, count=None, mover=None):
        if mover is None:
            mover = flip[0]
            flip[0] = -flip[0]  # each colour moves in turn
        b = np.zeros(A, np.int8) if board is None else board.copy()
        b[list(mover_cells)] = mover
        b[list(opp_cells)] = -mover
        if action >= 0:
            b[action] = 0
        opp = [int(a) for a in np.flatnonzero(b == -mover)]
        rows.append((b, mover, opp[-1] if opp else -1, int(np.count_nonzero(b)) if count is None else count, action,
                     mover * expect if abs(expect) == 1 else expect, tag))

    flat = lambda r, c: r * size + c  # noqa: E731
    # runs of n - 1 (no win), n, n + 1 and n + 3 (overlines, longer than the n + 1 cells the walk takes per side)
    for d, (dr, dc) in enumerate(DIRS):
        for L in (n - 1, n, n + 1, n + 3):
            if L > size:
                continue
            anchors = _anchors(size, d, L)
            for ai, (r0, c0) in enumerate(anchors):
                cells = [flat(r0 + i * dr, c0 + i * dc) for i in range(L)]
                assert all(0 <= r0 + i * dr < size and 0 <= c0 + i * dc < size for i in range(L))
                # the last stone at each cell of the run at one anchor (a middle cell joins two fragments); at the
                # others at both ends, and in the middle too where the run is n or n + 1 long
                every = ai == (d + L) % len(anchors)
                some = {0, L // 2, L - 1} if L in (n, n + 1) else {0, L - 1}
                for j in (range(L) if every else sorted(some)):
                    add("run d%d L%d" % (d, L), cells, [], cells[j], 1 if L >= n else 2)
            # the opponent's colour inside the run: fragments of 1 and L - 2, or n after an end stone
            r0, c0 = anchors[-1]
            cells = [flat(r0 + i * dr, c0 + i * dc) for i in range(L)]
            if L == n and n >= 3:
                add("cut d%d" % d, cells, [cells[1]], cells[L - 1], 2)
                add("cut d%d" % d, cells, [cells[L // 2]], cells[0], 2)
            if L == n + 1:
                add("cut-end d%d" % d, cells, [cells[0]], cells[L - 1], 1)
                add("cut-end d%d" % d, cells, [cells[L - 1]], cells[1], 1)
    # n stones contiguous in flat index only: a row's end into the next row's start (step 1), a diagonal across the
    # right border (step size + 1), an anti-diagonal across the left border (step size - 1, column 0 to column
    # size - 1).  k stones before the border, n - k after it.
    for step in (1, size + 1, size - 1):
        for k in range(1, n):
            starts = {1: [flat(0, size - k), flat(size - 2, size - k)], size + 1: [flat(0, size - k)],
                      size - 1: [flat(0, k - 1)]}[step]
            for f0 in starts:
                cells = [f0 + i * step for i in range(n)]
                if cells[-1] >= A:
                    continue
                cols = [f % size for f in cells]
                assert abs(cols[k] - cols[k - 1]) == size - 1  # the chain does cross the border
                for j in sorted({0, k - 1, k, n - 1}):
                    add("wrap s%d" % (1 if step == 1 else 2 if step == size + 1 else 3), cells, [], cells[j], 2)
    # full boards: the last empty cell draws, or completes a line and wins (the win goes first)
    pat = _pattern(size)
    for a in sorted({0, size - 1, A // 2, A - size, A - 1}):
        for mover in (1, -1):
            add("draw", [], [], a, 0, board=pat * (pat[a] * mover), count=A - 1, mover=mover)
    for i, a in enumerate(sorted({0, size - 1, A // 2, A - size, A - 1})):
        r, c = divmod(a, size)
        for mover in (1, -1):
            if i % 2 == 0:
                c0 = min(max(c - n // 2, 0), size - n)
                line = [flat(r, c0 + t) for t in range(n)]
            else:
                r0 = min(max(r - n // 2, 0), size - n)
                line = [flat(r0 + t, c) for t in range(n)]
            add("last-cell win", line, [], a, 1, board=pat, count=A - 1, mover=mover)
    # the move count decides the draw, not the stones on the board
    add("count draw", [flat(1, 1)], [flat(2, 3)], flat(0, 0), 0, count=A - 1)
    add("count draw", [flat(1, 1)], [flat(2, 3)], flat(size - 1, size - 1), 0, count=A - 1)
    add("count win", [flat(0, t) for t in range(n)], [flat(2, 3)], flat(0, n - 1), 1, count=A - 1)
    add("count on", [flat(1, 1)], [flat(2, 3)], flat(0, 0), 2, count=A - 2)
    # no move: nothing changes
    add("none", [], [], -1, 3)
    add("none", [flat(0, t) for t in range(n - 1)], [flat(2, 1), flat(size - 1, size - 1)], -1, 3)
    add("none", [], [], -1, 3, board=pat, count=A)
    add("none", [flat(0, t) for t in range(n)], [flat(size - 1, 0)], -1, 3, mover=-1)  # a won position, left alone
    out = dict(boards=np.array([r[0] for r in rows], np.int8), players=np.array([r[1] for r in rows], np.int8),
               last=np.array([r[2] for r in rows], np.int32), counts=np.array([r[3] for r in rows], np.int32),
               actions=np.array([r[4] for r in rows], np.int32), expect=np.array([r[5] for r in rows], np.int8))
    for v in out.values():
        v.setflags(write=False)
    out["tags"] = tuple(r[6] for r in rows)
    return out


@functools.lru_cache(maxsize=None)
def played(size, n, reset_finished):
    """cases(size, n) after the move, by the model: dict(status int8 [G], boards, players, last, counts)."""
    c = cases(size, n)
    G = len(c["actions"])
    boards = c["boards"].copy()
    st, pl, lm, mc = np.zeros(G, np.int8), np.zeros(G, np.int8), np.zeros(G, np.int32), np.zeros(G, np.int32)
    for g in range(G):
        st[g], pl[g], lm[g], mc[g] = play(boards[g], int(c["players"][g]), int(c["last"][g]), int(c["counts"][g]),
                                          int(c["actions"][g]), n, reset_finished)
    out = dict(status=st, boards=boards, players=pl, last=lm, counts=mc)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def win_maps(size, n):
    """win_map of every board of played(size, n, False): uint8 [G, A]."""
    out = np.array([win_map(b, size, n) for b in played(size, n, False)["boards"]], np.uint8)
    out.setflags(write=False)
    return out
