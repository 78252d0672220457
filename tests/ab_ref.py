"""numpy model of the depth-limited alpha-beta anchor of DESIGN.md §8b ("The alpha-beta anchor"), written from the
rule's text and window by window, on top of anchor_ref.scores / choose, not from the kernel (which works cell by cell
on bit lines).  Every quantity is an integer (Python ints here), so the kernel must give the same output words.

A window is n consecutive cells in one of the directions (0,1), (1,0), (1,1), (1,-1), wholly on the board; cells are
numbered r * size + c; p is the player to move; score(b, s, c) is anchor_ref's threat score of the empty cell c with s
to move; five(b, s) is vcf_ref's.  WIN = 2^40.

  E(b, s)      over every window: k >= 1 stones of s and none of -s adds 2 * 8^(k-1), k >= 1 stones of -s and none of s
               subtracts 8^(k-1);
  cand(b, s)   the ``width`` empty cells with the largest (score, -cell);
  value(b, s, d, alpha, beta, ply), from s's side:
    1. nodes += 1; nodes > max_nodes stops the whole search with status 2;
    2. no empty cell: 0;                3. five(b, s) not empty: WIN - ply;           4. d == 0: E(b, s);
    5. best = -2^50;
    6. for c of cand(b, s) in order, s on c: v = -value(b', -s, d - 1, -beta, -alpha, ply + 1); v > best: best = v;
       v > alpha: alpha = v; alpha >= beta: stop;
    7. best.
  The root is value(b, p, plies, -2^50, 2^50, 0), except that a root with five(b, p) not empty answers with its smallest
  cell and the value WIN, and that the root's candidates are the ``width`` best empty cells in the anchor rule's order
  (key, noise, -cell), key = float64(score) + scale * noise[c]: anchor_ref.choose applied ``width`` times without
  replacement.  The root's move is the first candidate whose value is strictly larger than all before it.

status 0 = searched, 2 = node budget used up (nodes is then max_nodes + 1), 3 = skipped (a full board, or left out by
``game``; nodes 0).  move is -1 and value 0 unless status is 0."""
import numpy as np

import anchor_ref as A
import vcf_ref as V

WIN, INF = 1 << 40, 1 << 50
SEARCHED, BUDGET, SKIPPED = 0, 2, 3
MAX_PLIES, MAX_WIDTH, MAX_NODES = 8, 16, 1 << 20
PLIES, WIDTH, NODES = 4, 8, 2048  # the defaults


def _window_counts(b, s, n):
    """(stones of s, stones of -s) per window, int64 [W] each."""
    S = int(round(b.size ** 0.5))
    v = b[V.windows(S, n)]
    return (v == s).sum(axis=1).astype(np.int64), (v == -s).sum(axis=1).astype(np.int64)


def static_value(board, s, n=5):
    """E(b, s) as a Python int."""
    b = np.asarray(board, np.int8).reshape(-1)
    own, opp = _window_counts(b, int(s), n)
    plus = own[(own >= 1) & (opp == 0)]
    minus = opp[(opp >= 1) & (own == 0)]
    return int((2 * 8 ** (plus - 1)).sum()) - int((8 ** (minus - 1)).sum())


def cand(board, s, n=5, width=WIDTH):
    """The ``width`` empty cells with the largest (score, -cell), as a list (fewer when fewer are empty)."""
    sc = A.scores(board, int(s), n)
    empty = np.flatnonzero(sc >= 0)
    order = empty[np.lexsort((empty, -sc[empty]))]
    return [int(c) for c in order[:width]]


def root_cand(board, p, n=5, width=WIDTH, noise=None, scale=0.0):
    """The root's candidates: anchor_ref.choose applied ``width`` times without replacement."""
    sc = A.scores(board, int(p), n).copy()
    out = []
    for _ in range(width):
        c = A.choose(sc, noise, scale)
        if c < 0:
            break
        out.append(c)
        sc[c] = -1
    return out


class _Budget(Exception):
    pass


def search(board, player, n=5, plies=PLIES, width=WIDTH, max_nodes=NODES, noise=None, scale=0.0, prune=True):
    """(status, move, value, nodes) of one board (int8 [S, S] or [A]) with ``player`` to move.  ``prune=False`` turns
    the alpha/beta cut off (step 6 never stops): plain minimax over the same candidates."""
    b = np.array(board, np.int8).reshape(-1)
    p = int(player)
    if not (b == 0).any():
        return SKIPPED, -1, 0, 0
    count = [0]

    def value(s, d, alpha, beta, ply):
        count[0] += 1
        if count[0] > max_nodes:
            raise _Budget()
        if not (b == 0).any():
            return 0, -1
        own, opp = _window_counts(b, s, n)
        if ((own == n - 1) & (opp == 0)).any():
            return WIN - ply, (V.five(b, s, n)[0] if ply == 0 else -1)
        if d == 0:
            plus = own[(own >= 1) & (opp == 0)]
            minus = opp[(opp >= 1) & (own == 0)]
            return int((2 * 8 ** (plus - 1)).sum()) - int((8 ** (minus - 1)).sum()), -1
        best, move = -INF, -1
        for c in (root_cand(b, s, n, width, noise, scale) if ply == 0 else cand(b, s, n, width)):
            b[c] = s
            try:
                v = -value(-s, d - 1, -beta, -alpha, ply + 1)[0]
            finally:
                b[c] = 0
            if v > best:
                best, move = v, c
            if v > alpha:
                alpha = v
            if prune and alpha >= beta:
                break
        return best, move

    try:
        v, mv = value(p, int(plies), -INF, INF, 0)
    except _Budget:
        return BUDGET, -1, 0, count[0]
    return SEARCHED, mv, v, count[0]


def search_batch(boards, players, n=5, plies=PLIES, width=WIDTH, max_nodes=NODES, noise=None, scale=0.0, game=None):
    """(status int8 [G], move int32 [G], value int64 [G], nodes int32 [G]); ``noise``: float64 [G, A] or None; a
    negative game[g] skips board g."""
    G = len(boards)
    out = (np.zeros(G, np.int8), np.full(G, -1, np.int32), np.zeros(G, np.int64), np.zeros(G, np.int32))
    for g in range(G):
        if game is not None and game[g] < 0:
            out[0][g] = SKIPPED
            continue
        r = search(boards[g], players[g], n, plies, width, max_nodes, None if noise is None else noise[g], scale)
        for o, x in zip(out, r):
            o[g] = x
    return out


def mover_move(b, p, n, noise, mover):
    """The move of a side on board b [A] as the arena composes it: mover = ("ab", scale, depth, nodes, plies, width)
    plays the forced-win solver's move (vcf_ref.solve with depth and nodes) where its status is 1, else the alpha-beta
    move (``nodes`` its budget too) where that search finished (status 0), else the threat rule's; any other mover goes
    to vcf_ref.mover_move.  Returns (move, which): which = 2 for an alpha-beta move, 1 for a solver move, 0 otherwise."""
    if mover[0] != "ab":
        a, by_solver = V.mover_move(b, p, n, noise, mover)
        return a, int(by_solver)
    _, scale, depth, nodes, plies, width = mover
    st, mv, _, _ = V.solve(b, p, n, depth, nodes)
    if st == V.FOUND:
        return mv, 1
    st, mv, _, _ = search(b, p, n, plies, width, nodes, noise, scale)
    if st == SEARCHED:
        return mv, 2
    return A.move(b, p, n, noise, A.THREAT, scale)[1], 0


def play_game(board, player, movers, noise_of, n=5, positions=None):
    """vcf_ref.play_game in which a side may also be ("ab", scale, depth, nodes, plies, width).  Returns (winner colour
    or 0, moves, [threat / uniform moves, solver moves, alpha-beta moves] played)."""
    b = np.array(board, np.int8).reshape(-1)
    S = int(round(b.size ** 0.5))
    moves, p, by = [], int(player), [0, 0, 0]
    while True:
        if positions is not None:
            positions.append((b.copy(), p))
        a, which = mover_move(b, p, n, noise_of(len(moves)), movers[len(moves) % 2])
        assert a >= 0 and b[a] == 0
        by[which] += 1
        b[a] = p
        moves.append(a)
        if A.wins(b.reshape(S, S), a, n):
            return p, moves, by
        if not (b == 0).any():
            return 0, moves, by
        p = -p
