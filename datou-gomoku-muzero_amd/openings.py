"""Opening builders — random line-free starts for self-play measurements (seeded_openings, random_openings), the
arena's book (paired_openings), and self-play's book: its check (check_selfplay_book) and the host's copy of the
device's draw (book_draw, transform_opening; gmz_engine_play_book).  numpy only: engine.py and arena.py re-export the
names."""
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


# ------------------------------------------------------------------ self-play's book (gmz_engine_play_book)
BOOK_SALT_OPEN, BOOK_SALT_SYM = 0xB5297A4D, 0x27D4EB2F  # GMZ_BOOK_SALT_* of include/gmz.h
BOOK_MAX_OPENINGS = 1 << 20
_M32 = np.uint64(0xFFFFFFFF)


def _mix32(x):
    """mix32 of csrc/gmz_common.h on uint64 arrays that hold 32-bit words."""
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    return x ^ (x >> np.uint64(16))


def book_draw(seed, keys, serials, n, symmetry=True):
    """The opening and the symmetry that gmz_engine_play_book draws for the games (key, serial) under ``seed``: a
    pure function, so the host mirrors the device without a read-back.  ``keys`` (slot + the engine's game_offset)
    and ``serials`` broadcast; ``n`` openings.  Returns (t int64 in [0, n), d int64 in 0..7; all 0 without
    ``symmetry``)."""
    n = int(n)
    if not 1 <= n <= BOOK_MAX_OPENINGS:
        raise ValueError("book_draw: n must be in [1, 2^20]")
    seed = int(seed) % (1 << 64)
    lo, hi = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    k = (np.asarray(keys).astype(np.int64).astype(np.uint64) & _M32) * np.uint64(0x85EBCA77) & _M32
    s = (np.asarray(serials).astype(np.int64).astype(np.uint64) & _M32) * np.uint64(0x9E3779B1) & _M32
    h1 = _mix32(lo ^ _mix32((s + k) & _M32))
    t = (_mix32(h1 ^ hi ^ np.uint64(BOOK_SALT_OPEN)) * np.uint64(n)) >> np.uint64(32)
    d = _mix32(h1 ^ hi ^ np.uint64(BOOK_SALT_SYM)) & np.uint64(7)
    t, d = t.astype(np.int64), d.astype(np.int64)
    return t, (d if symmetry else np.zeros_like(d))


def symmetry_cells(size):
    """int64 [8, size^2]: row d holds, for every cell, the cell it goes to under symmetry d (bit 0 transposes, then
    bit 1 flips the row, then bit 2 flips the column)."""
    r, c = np.divmod(np.arange(size * size, dtype=np.int64), size)
    out = np.empty((8, size * size), np.int64)
    for d in range(8):
        rr, cc = (c, r) if d & 1 else (r, c)
        if d & 2:
            rr = size - 1 - rr
        if d & 4:
            cc = size - 1 - cc
        out[d] = rr * size + cc
    return out


def transform_opening(boards, last_moves, d, size):
    """Openings under the symmetries ``d`` (one per opening, 0..7): boards int8 [m, S, S] or [m, A] and last_moves
    int32 [m] (-1 stays -1) -> (boards int8 [m, S, S], last_moves int32 [m]).  The side to move and the stone count
    do not change."""
    A = size * size
    b = np.asarray(boards, dtype=np.int8).reshape(-1, A)
    m = b.shape[0]
    d = np.broadcast_to(np.asarray(d, dtype=np.int64), (m,))
    cells = symmetry_cells(size)[d]  # [m, A]: where each cell goes
    out = np.empty_like(b)
    np.put_along_axis(out, cells, b, axis=1)
    lm = np.asarray(last_moves, dtype=np.int32).reshape(m)
    ok = (lm >= 0) & (lm < A)
    moved = np.where(ok, cells[np.arange(m), np.where(ok, lm, 0)], -1).astype(np.int32)
    return out.reshape(m, size, size), moved


def _winning_cell(board, player, n_in_row):
    """An empty cell at which ``player`` completes n_in_row (records.find_winning_moves' 'five'), or None."""
    from .records import _five_at
    if int((board == player).sum()) < n_in_row - 1:
        return None
    for r, c in zip(*np.where(board == 0)):
        if _five_at(board, player, int(r), int(c), n_in_row):
            return int(r), int(c)
    return None


def check_selfplay_book(book, cfg):
    """The book of SelfPlay(book=...) as four arrays (boards int8 [n, A], players int8 [n], last_moves int32 [n],
    move_counts int32 [n]), refused (ValueError) unless every opening has its stone count, a side to move of +-1, at
    least NUM_TOP_ACTIONS legal cells (a restarted slot then needs the hidden-state slots of the empty board, as in
    the arena), no N_IN_ROW line on the board, and no cell at which the side to move wins at once: every game then
    lasts two plies or more, which the history's two banks need."""
    boards, players, last, counts = book
    boards = np.ascontiguousarray(boards, dtype=np.int8)
    n = boards.shape[0]
    A, S, N = cfg.ACTION_SPACE_SIZE, cfg.BOARD_SIZE, cfg.N_IN_ROW
    if n < 1 or boards.reshape(n, -1).shape[1] != A:
        raise ValueError("Self-play book: at least one opening of BOARD_SIZE x BOARD_SIZE cells is needed")
    if n > BOOK_MAX_OPENINGS:
        raise ValueError("Self-play book: at most 2^20 openings")
    boards = boards.reshape(n, A)
    counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(n)
    players = np.ascontiguousarray(players, dtype=np.int8).reshape(n)
    last = np.ascontiguousarray(last, dtype=np.int32).reshape(n)
    if not np.array_equal((boards != 0).sum(axis=1), counts):
        raise ValueError("Self-play book: an opening's stone count differs from its board")
    if not np.isin(players, (-1, 1)).all():
        raise ValueError("Self-play book: an opening's side to move must be +1 or -1")
    if not np.isin(boards, (-1, 0, 1)).all() or ((last < -1) | (last >= A)).any():
        raise ValueError("Self-play book: cells must be -1, 0 or +1 and last moves -1 or a cell")
    left = A - counts
    if (left < cfg.NUM_TOP_ACTIONS).any():
        raise ValueError("Self-play book: every opening must leave at least NUM_TOP_ACTIONS = %d legal cells (opening "
                         "%d leaves %d)" % (cfg.NUM_TOP_ACTIONS, int(np.argmin(left)), int(left.min())))
    for i in range(n):
        b = boards[i].reshape(S, S)
        if _has_five(b, N):
            raise ValueError("Self-play book: opening %d already holds %d in a row" % (i, N))
        w = _winning_cell(b, int(players[i]), N)
        if w is not None:
            raise ValueError("Self-play book: in opening %d the side to move wins at once at %s" % (i, w))
    return boards, players, last, counts


def selfplay_book_rows(book, cfg):
    """The rows of ``book`` that check_selfplay_book's two game rules keep (no line on the board, no immediate win
    for the side to move): a bool mask [n], for filtering paired_openings' output."""
    boards, players = np.asarray(book[0], dtype=np.int8), np.asarray(book[1]).reshape(-1)
    S, N = cfg.BOARD_SIZE, cfg.N_IN_ROW
    b = boards.reshape(len(players), S, S)
    return np.array([not _has_five(b[i], N) and _winning_cell(b[i], int(players[i]), N) is None
                     for i in range(len(players))], dtype=bool)


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
