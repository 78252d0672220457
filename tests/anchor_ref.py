"""numpy model of the anchor opponents' move rule, written from the rule's text, not from the kernel.

Score of an empty cell c (int64): for each side s in (p, -p), each direction d in (0,1), (1,0), (1,1), (1,-1) and each
offset o = 0..n-1, the window of the n cells c + (j - o) d, j = 0..n-1, counts if every cell is on the board and none
holds -s; with k stones of s in it and m = n - 1 - k it adds W_s[min(m, 4)].  kind 1 scores every empty cell 0.
The move is the empty cell with the largest (key, noise, -cell), key = float64(score) + scale * noise; -1 on a full
board."""
import numpy as np

W_OWN = (2 ** 26, 2 ** 13, 2 ** 6, 2 ** 2, 1)
W_OPP = (2 ** 20, 2 ** 10, 2 ** 5, 2 ** 1, 0)
DIRS = ((0, 1), (1, 0), (1, 1), (1, -1))
THREAT, UNIFORM = 0, 1


def scores(board, player, n=5, kind=THREAT):
    """int64 [A]: the score of every empty cell, -1 for an occupied one.  board: int8 [S, S] or [A].  The same sum
    as scores_by_cell, taken window by window: every window on the board adds its weight to each of its n cells."""
    b = np.asarray(board)
    S = int(round(b.size ** 0.5))
    b = b.reshape(S, S)
    total = np.zeros((S, S), np.int64)
    if kind == THREAT and n <= S:
        for s, w in ((player, W_OWN), (-player, W_OPP)):
            w = np.asarray(w, np.int64)
            for dr, dc in DIRS:
                ny = S - (n - 1) * dr                     # window starts: rows 0..ny-1,
                x0 = (n - 1) if dc < 0 else 0             # columns x0..x0+nx-1
                nx = S - (n - 1) * abs(dc)
                cut = [(slice(j * dr, j * dr + ny), slice(x0 + j * dc, x0 + j * dc + nx)) for j in range(n)]
                k = sum((b[c] == s).astype(np.int64) for c in cut)
                blocked = sum((b[c] == -s).astype(np.int64) for c in cut) > 0
                add = np.where(blocked, 0, w[np.minimum(n - 1 - k, 4)])
                for c in cut:
                    total[c] += add
    return np.where(b == 0, total, -1).reshape(-1).astype(np.int64)


def scores_by_cell(board, player, n=5, kind=THREAT):
    """scores, cell by cell exactly as the rule is worded (slow: small boards)."""
    b = np.asarray(board)
    S = int(round(b.size ** 0.5))
    b = b.reshape(S, S)
    out = np.full(S * S, -1, np.int64)
    for r in range(S):
        for c in range(S):
            if b[r, c] != 0:
                continue
            total = 0
            if kind == THREAT:
                for s, w in ((player, W_OWN), (-player, W_OPP)):
                    for dr, dc in DIRS:
                        for o in range(n):
                            cells = [(r + (j - o) * dr, c + (j - o) * dc) for j in range(n)]
                            if any(not (0 <= y < S and 0 <= x < S) for y, x in cells):
                                continue
                            vals = [int(b[y, x]) for y, x in cells]
                            if -s in vals:
                                continue
                            total += w[min(n - 1 - vals.count(s), 4)]
            out[r * S + c] = total
    return out


def choose(sc, noise=None, scale=0.0):
    """The move from the scores: the empty cell (score >= 0) with the largest (key, noise, -cell); -1 if none."""
    sc = np.asarray(sc, np.int64)
    nz = np.zeros(sc.size, np.float64) if noise is None else np.asarray(noise, np.float64).reshape(-1)
    empty = np.flatnonzero(sc >= 0)
    if empty.size == 0:
        return -1
    key = sc[empty].astype(np.float64) + np.float64(scale) * nz[empty]
    best = empty[key == key.max()]
    best = best[nz[best] == nz[best].max()]
    return int(best.min())


def move(board, player, n=5, noise=None, kind=THREAT, scale=0.0):
    """(scores int64 [A], move)."""
    sc = scores(board, player, n, kind)
    return sc, choose(sc, noise, scale)


def play_game(board, player, movers, noise_of, n=5):
    """A game from ``board`` (int8 [A], copied) with ``player`` to move, on the host: movers[i % 2] = (kind, scale)
    of the side that makes ply i, noise_of(ply) the noise row of that ply.  Returns (winner colour or 0, moves)."""
    b = np.array(board, np.int8).reshape(-1)
    S = int(round(b.size ** 0.5))
    moves, p = [], int(player)
    while True:
        kind, scale = movers[len(moves) % 2]
        _, a = move(b, p, n, noise_of(len(moves)), kind, scale)
        assert a >= 0 and b[a] == 0
        b[a] = p
        moves.append(a)
        if wins(b.reshape(S, S), a, n):
            return p, moves
        if not (b == 0).any():
            return 0, moves
        p = -p


def wins(b, a, n):
    """The stone on cell ``a`` of board b [S, S] is part of a line of at least n."""
    S = b.shape[0]
    r, c, p = a // S, a % S, b[a // S, a % S]
    for dr, dc in DIRS:
        run = 1
        for sgn in (1, -1):
            y, x = r + sgn * dr, c + sgn * dc
            while 0 <= y < S and 0 <= x < S and b[y, x] == p:
                run += 1
                y, x = y + sgn * dr, x + sgn * dc
        if run >= n:
            return True
    return False
