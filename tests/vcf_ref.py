"""numpy model of the forced-win (VCF, "victory by continuous fours") solver of DESIGN.md §8b, written from the rule's
text and window by window, not from the kernel (which works cell by cell).

A window is n consecutive cells in one of the directions (0,1), (1,0), (1,1), (1,-1), wholly on the board; cells are
numbered r * size + c; p is the attacker, the player to move.

  five(b, s)   the empty cells c for which some window holding c has n-1 stones of s and c as its only other cell;
  fours(b, s)  (only where five(b, s) is empty) the empty cells c for which some window holding c has n-2 stones of s
               and exactly two empty cells, c and e; T(c) is the set of all such e.

solve(b, d), d the attacker moves still allowed:
  1. nodes += 1; nodes > max_nodes stops the whole search with status 2;
  2. five(b, p) not empty: win, move = its smallest cell, length 1;
  3. d <= 1: fail;
  4. Fo = five(b, -p); two or more cells: fail;
  5. the cells of fours(b, p) in ascending order; with one cell in Fo only that cell, and only if it is a four;
  6. for each such c: T(c) has two or more cells: win, move c, length 2; otherwise p on c, -p on T(c)'s one cell,
     solve(b', d - 1): a win there is a win here with move c and length + 1;
  7. fail.

status 0 = no forced win within max_depth, 1 = found, 2 = node budget used up (nodes is then max_nodes + 1: the call
that went over is counted), 3 = board skipped.  move is -1 and length 0 unless status is 1."""
import numpy as np

import anchor_ref as A

DIRS = A.DIRS
NONE, FOUND, BUDGET, SKIPPED = 0, 1, 2, 3
MAX_DEPTH, MAX_NODES = 16, 1 << 20

_WINDOWS = {}


def windows(S, n):
    """int32 [W, n]: the cells of every window of an S x S board."""
    key = (S, n)
    if key not in _WINDOWS:
        out = []
        for dr, dc in DIRS:
            for r in range(S):
                for c in range(S):
                    re, ce = r + (n - 1) * dr, c + (n - 1) * dc
                    if 0 <= re < S and 0 <= ce < S:
                        out.append([(r + j * dr) * S + c + j * dc for j in range(n)])
        _WINDOWS[key] = np.asarray(out, np.int32).reshape(-1, n)
    return _WINDOWS[key]


def _counts(b, W, s):
    v = b[W]
    return v, (v == s).sum(axis=1), (v == 0).sum(axis=1)


def five(b, s, n=5):
    """Sorted list of five(b, s).  b: int8 [A]."""
    b = np.asarray(b, np.int8).reshape(-1)
    S = int(round(b.size ** 0.5))
    W = windows(S, n)
    v, own, emp = _counts(b, W, s)
    hit = np.flatnonzero((own == n - 1) & (emp == 1))
    return sorted({int(W[i][v[i] == 0][0]) for i in hit})


def fours(b, s, n=5):
    """{c: T(c)} for the cells of fours(b, s); meaningful where five(b, s) is empty."""
    b = np.asarray(b, np.int8).reshape(-1)
    S = int(round(b.size ** 0.5))
    W = windows(S, n)
    v, own, emp = _counts(b, W, s)
    T = {}
    for i in np.flatnonzero((own == n - 2) & (emp == 2)):
        x, y = (int(c) for c in W[i][v[i] == 0])
        T.setdefault(x, set()).add(y)
        T.setdefault(y, set()).add(x)
    return T


class _Budget(Exception):
    pass


def solve(board, player, n=5, max_depth=10, max_nodes=2048):
    """(status, move, length, nodes) of one board (int8 [S, S] or [A]) with ``player`` to move."""
    b = np.array(board, np.int8).reshape(-1)
    p = int(player)
    count = [0]

    def rec(d):
        count[0] += 1
        if count[0] > max_nodes:
            raise _Budget()
        f = five(b, p, n)
        if f:
            return f[0], 1
        if d <= 1:
            return None
        fo = five(b, -p, n)
        if len(fo) >= 2:
            return None
        T = fours(b, p, n)
        cand = sorted(T)
        if fo:
            cand = [c for c in cand if c == fo[0]]
        for c in cand:
            if len(T[c]) >= 2:
                return c, 2
            e = next(iter(T[c]))
            b[c], b[e] = p, -p
            r = rec(d - 1)
            b[c], b[e] = 0, 0
            if r is not None:
                return c, r[1] + 1
        return None

    try:
        r = rec(int(max_depth))
    except _Budget:
        return BUDGET, -1, 0, count[0]
    if r is None:
        return NONE, -1, 0, count[0]
    return FOUND, r[0], r[1], count[0]


def solve_batch(boards, players, n=5, max_depth=10, max_nodes=2048, game=None):
    """(status int8 [G], move int32 [G], length int32 [G], nodes int32 [G]); a negative game[g] skips board g."""
    G = len(boards)
    out = (np.zeros(G, np.int8), np.full(G, -1, np.int32), np.zeros(G, np.int32), np.zeros(G, np.int32))
    for g in range(G):
        if game is not None and game[g] < 0:
            out[0][g] = SKIPPED
            continue
        r = solve(boards[g], players[g], n, max_depth, max_nodes)
        for o, x in zip(out, r):
            o[g] = x
    return out


def mover_move(b, p, n, noise, mover):
    """The move of a side on board b [A]: mover = (kind, scale) as anchor_ref.play_game takes, or
    ("vcf", scale, depth, nodes): the solver's move where its status is 1, else the threat rule's.  Returns
    (move, True where the solver's move was played)."""
    if mover[0] == "vcf":
        _, scale, depth, nodes = mover
        st, mv, _, _ = solve(b, p, n, depth, nodes)
        if st == FOUND:
            return mv, True
        return A.move(b, p, n, noise, A.THREAT, scale)[1], False
    kind, scale = mover
    kind = {"threat": A.THREAT, "uniform": A.UNIFORM}.get(kind, kind)
    return A.move(b, p, n, noise, kind, scale)[1], False


def play_game(board, player, movers, noise_of, n=5, positions=None):
    """anchor_ref.play_game in which a side may also be ("vcf", scale, depth, nodes).  Returns (winner colour or 0,
    moves, solver moves played).  ``positions`` (a list) collects (board copy, player) before every ply."""
    b = np.array(board, np.int8).reshape(-1)
    S = int(round(b.size ** 0.5))
    moves, p, solved = [], int(player), 0
    while True:
        if positions is not None:
            positions.append((b.copy(), p))
        a, by_solver = mover_move(b, p, n, noise_of(len(moves)), movers[len(moves) % 2])
        assert a >= 0 and b[a] == 0
        solved += by_solver
        b[a] = p
        moves.append(a)
        if A.wins(b.reshape(S, S), a, n):
            return p, moves, solved
        if not (b == 0).any():
            return 0, moves, solved
        p = -p


def threat_game_positions(S, n, games, seed, scale=3e3):
    """(boards int8 [P, A], players int8 [P]): every position (the empty board included) of ``games`` games between
    two threat anchors with Gumbel noise of ``scale``, from the empty board, black first."""
    rs = np.random.RandomState(seed)
    pos = []
    for _ in range(games):
        play_game(np.zeros(S * S, np.int8), 1, [(A.THREAT, scale)] * 2, lambda ply: rs.gumbel(0, 1, S * S), n, pos)
    return np.stack([b for b, _ in pos]), np.array([p for _, p in pos], np.int8)
