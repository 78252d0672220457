"""Opening builders — random line-free starts for self-play measurements (seeded_openings, random_openings) and the
arena's book (paired_openings).  numpy only: engine.py and arena.py re-export the names."""
import numpy as np


def _has_five(board, n_in_row=5):
    """Any run of n_in_row equal non-zero stones on an int8 [S,S] board (rows, columns, diagonals)."""
    S = board.shape[0]
    for b in (board, board.T):
        for k in range(S - n_in_row + 1):
            w = b[:, k:k + n_in_row]
            if ((w == w[:, :1]).all(axis=1) & (w[:, 0] != 0)).any():
                return True
    for b in (board, board[:, ::-1]):
        for off in range(-(S - n_in_row), S - n_in_row + 1):
            d = np.diagonal(b, off)
            for k in range(len(d) - n_in_row + 1):
                w = d[k:k + n_in_row]
                if w[0] != 0 and (w == w[0]).all():
                    return True
    return False


def _place_stones(rs, A, size, n, n_in_row):
    """n stones of alternating colour (black first) on random cells of an empty board with no n_in_row
    line, drawn from ``rs`` (redrawn until the board holds no line).  Returns (board int8[A], cells)."""
    while True:
        cells = rs.permutation(A)[:n]
        b = np.zeros(A, np.int8)
        b[cells[0::2]] = 1
        b[cells[1::2]] = -1
        if not _has_five(b.reshape(size, size), n_in_row):
            return b, cells


def _opening(rs, A, size, n, n_in_row):
    """One opening of n stones (_place_stones): (board int8[S,S], side to move, last move or -1)."""
    b, cells = _place_stones(rs, A, size, n, n_in_row)
    return b.reshape(size, size), 1 if n % 2 == 0 else -1, cells[-1] if n else -1


def _book(rows, size):
    """(board, side to move, last move, stones) per opening -> (boards int8 [G,S,S], players int8 [G], last_moves
    int32 [G], move_counts int32 [G])."""
    b, p, lm, n = zip(*rows) if rows else ((), (), (), ())
    return (np.array(b, np.int8).reshape(len(rows), size, size), np.array(p, np.int8), np.array(lm, np.int32),
            np.array(n, np.int32))


def seeded_openings(game_ids, size, seed, ks=(0, 4, 8), stagger=0, n_in_row=5):
    """SURVEY §8(d)'s synthetic starts: game ``gid`` draws from ``RandomState(seed + gid)`` an opening of
    k in ``ks`` stones (empty boards plus k in {0, 4, 8}) and, with ``stagger`` > 0, uniform(0, stagger)
    further stones (at most 2A/5 in all), so that the G games are spread over their lifetimes and some finish (and restart
    from the empty board) in any window of a few moves: the steady state a long self-play run is in.
    Returns (boards int8 [G,S,S], players int8 [G], last_moves int32 [G], move_counts int32 [G])."""
    A = size * size
    rows = []
    for gid in game_ids:
        rs = np.random.RandomState((int(seed) + int(gid)) % (2 ** 32))
        n = int(ks[rs.randint(len(ks))]) + (int(rs.randint(0, stagger + 1)) if stagger > 0 else 0)
        n = min(n, 2 * A // 5)  # small boards: room left to play, and a line-free draw stays likely
        rows.append(_opening(rs, A, size, n, n_in_row) + (n,))
    return _book(rows, size)


def random_openings(G, size, rs, max_stones, n_in_row=5):
    """Staggered game starts for measurements: game g gets an opening of uniform(0, max_stones) stones of
    alternating colour (black first) on random cells, with no n_in_row line on the board, the player to
    move after it and its last stone.  Returns (boards int8 [G,S,S], players int8 [G], last_moves int32 [G],
    move_counts int32 [G]) for BatchedSelfPlayEngine.set_positions / GameHistory.set_start."""
    counts = rs.randint(0, max_stones + 1, G)
    return _book([_opening(rs, size * size, size, int(n), n_in_row) + (int(n),) for n in counts], size)


def paired_openings(n, size, seed, stones=(2, 4, 6), n_in_row=5):
    """A book of ``n`` openings: opening i holds stones[i % len(stones)] stones of alternating colour (black
    first) on random cells, no n_in_row line (_place_stones), drawn from RandomState(seed + i).  Returns
    (boards int8 [n,S,S], players int8 [n] = side to move, last_moves int32 [n], move_counts int32 [n])."""
    rows = []
    for i in range(n):
        k = int(stones[i % len(stones)])
        rs = np.random.RandomState((int(seed) + i) % (2 ** 32))
        rows.append(_opening(rs, size * size, size, k, n_in_row) + (k,))
    return _book(rows, size)
