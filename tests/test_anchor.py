"""Anchor opponents, host side (no GPU): the numpy model of the move rule (tests/anchor_ref.py) on hand-made positions,
the two dominance inequalities of its weights, gmz_game_anchor_move's refusals before any launch (fake pointers, never
dereferenced: the tests/test_abi.py pattern; no valid call is made with them), and the arena's check of an
AnchorPlayer."""
import ctypes

import numpy as np
import pytest

import anchor_ref as R

FN = "gmz_game_anchor_move"


def _board(S, black=(), white=()):
    b = np.zeros((S, S), np.int8)
    for r, c in black:
        b[r, c] = 1
    for r, c in white:
        b[r, c] = -1
    return b


def _full_but(S, hole=None):
    """A board with a stone on every cell (both colours, in shifted two-column stripes) but ``hole``."""
    b = np.zeros((S, S), np.int8)
    for r in range(S):
        for c in range(S):
            b[r, c] = 1 if ((c + 2 * (r // 2 % 2) + (r % 2)) // 2) % 2 == 0 else -1
    if hole is not None:
        b.reshape(-1)[hole] = 0
    return b


def hand_made():
    """[(name, board int8 [S,S], player to move, expected move)] at n = 5 (also run on the GPU by
    tests/test_anchor_gpu.py)."""
    S = 9
    cases = []
    # black to move holds (0,0)-(0,3), white holds (2,0)-(2,3): black completes its own five at (0,4), not the block
    cases.append(("own four and opponent four", _board(S, [(0, 0), (0, 1), (0, 2), (0, 3)],
                                                       [(2, 0), (2, 1), (2, 2), (2, 3)]), 1, 0 * S + 4))
    # the same with white to move: white's own four wins at (2,4)
    cases.append(("own four and opponent four, other side", cases[0][1].copy(), -1, 2 * S + 4))
    # white holds a four, black (to move) has scattered stones: the block at (2,4)
    cases.append(("opponent four only", _board(S, [(5, 5), (7, 1), (8, 8), (6, 3)],
                                               [(2, 0), (2, 1), (2, 2), (2, 3)]), 1, 2 * S + 4))
    cases.append(("full board", _full_but(S), 1, -1))
    cases.append(("one empty cell", _full_but(S, hole=31), -1, 31))
    # a four running into the right edge: the window that would continue off the board does not count, (0,4) is
    # the one completion
    cases.append(("four into the edge", _board(S, [(0, 5), (0, 6), (0, 7), (0, 8)], [(4, 4), (5, 4), (6, 5), (3, 7)]),
                  1, 0 * S + 4))
    # a four in the open: both ends complete it; (4,6) lies in more windows than (4,1), which is nearer the edge
    cases.append(("open four", _board(S, [(4, 2), (4, 3), (4, 4), (4, 5)], [(0, 0), (8, 8), (0, 8), (8, 1)]), 1,
                  4 * S + 6))
    return cases


def centre(S):
    """The empty board's move at n = 5: the cell in the most windows, lowest index first.  Up to 9x9 that is the
    centre (the lowest-index centre cell on an even size); from 10x10 every cell at least four cells from each edge
    lies in all 20 windows, and the first of that block is (4, 4)."""
    m = min((S - 1) // 2, 4)
    return m * S + m


@pytest.mark.parametrize("case", hand_made(), ids=[c[0] for c in hand_made()])
def test_model_on_hand_made_positions(case):
    name, board, player, want = case
    sc, mv = R.move(board, player, 5)
    assert mv == want, (name, mv)
    assert np.array_equal(sc, R.scores_by_cell(board, player, 5))
    assert np.array_equal(sc >= 0, board.reshape(-1) == 0)


def test_model_edge_window_and_win_over_block():
    cases = {c[0]: c for c in hand_made()}
    _, board, player, want = cases["four into the edge"]
    sc = R.scores(board, player, 5)
    assert sc[want] // R.W_OWN[0] == 1  # exactly one completing window: columns 4-8; columns 5-9 is off the board
    assert (np.delete(sc, want) < R.W_OPP[0]).all()
    _, board, player, want = cases["own four and opponent four"]
    sc = R.scores(board, player, 5)
    assert sc[want] >= R.W_OWN[0] > sc[2 * 9 + 4] >= R.W_OPP[0]  # the win outranks the block, the block the rest
    assert (np.delete(sc, [want, 2 * 9 + 4]) < R.W_OPP[0]).all()
    _, board, player, want = cases["open four"]
    sc = R.scores(board, player, 5)
    assert sc[4 * 9 + 6] > sc[4 * 9 + 1] >= R.W_OWN[0] and sc[4 * 9 + 6] - sc[4 * 9 + 1] < R.W_OWN[1]


@pytest.mark.parametrize("S", [5, 6, 7, 8, 9, 15, 19, 22])
def test_model_empty_board_prefers_the_centre(S):
    sc, mv = R.move(np.zeros((S, S), np.int8), 1, 5)
    assert mv == centre(S)
    # the score of a cell of the empty board is its window count (each window adds W_own[4] + W_opp[4] = 1): a
    # corner lies in three, the best cells in the most, and those are the centre block
    assert sc[0] == 3 and sc[mv] == sc.max() <= 20
    best = np.flatnonzero(sc == sc.max())
    assert best.size == (max(S - 8, 1) ** 2 if S % 2 else max(S - 8, 2) ** 2)
    assert R.move(np.zeros((S, S), np.int8), -1, 5)[1] == centre(S)


def test_model_noise_breaks_ties_and_uniform_ignores_the_board():
    rs = np.random.RandomState(0)
    b = _board(9, [(4, 4)], [(3, 3)])
    nz = rs.gumbel(0, 1, 81)
    sc = R.scores(b, 1, 5)
    mv = R.choose(sc, nz, 0.0)
    top = np.flatnonzero(sc == sc.max())
    assert mv == top[np.argmax(nz[top])]
    u = R.scores(b, 1, 5, R.UNIFORM)
    assert set(u.tolist()) == {0, -1} and np.array_equal(u < 0, b.reshape(-1) != 0)
    empty = np.flatnonzero(u == 0)
    assert R.choose(u, nz, 1.0) == empty[np.argmax(nz[empty])]
    # equal noise values: the lower index
    flat = np.zeros(81)
    assert R.choose(u, flat, 1.0) == empty[0]
    flat[[10, 50]] = 2.0
    assert R.choose(u, flat, 1.0) == 10


@pytest.mark.parametrize("S,n", [(5, 5), (6, 3), (7, 5), (9, 3), (6, 6), (5, 1)])
def test_model_window_sums_equal_the_cell_by_cell_rule(S, n):
    rs = np.random.RandomState(S * 10 + n)
    for fill in (0.0, 0.1, 0.5, 0.9):
        b = rs.choice(np.array([0, 1, -1], np.int8), size=(S, S), p=[1 - fill, fill / 2, fill / 2])
        for p in (1, -1):
            assert np.array_equal(R.scores(b, p, n), R.scores_by_cell(b, p, n)), (S, n, fill, p)


def test_weights_dominate():
    """At n = 5 a cell lies in at most 4 * 5 = 20 windows per side.  A cell that completes a five scores at least
    W_own[0]; one that does not scores at most 20 * (W_opp[0] + W_own[1]).  A cell that blocks a five scores at least
    W_opp[0]; one that neither wins nor blocks at most 20 * (W_own[1] + W_opp[1])."""
    assert R.W_OWN == (2 ** 26, 2 ** 13, 2 ** 6, 2 ** 2, 1) and R.W_OPP == (2 ** 20, 2 ** 10, 2 ** 5, 2 ** 1, 0)
    assert 20 * (R.W_OPP[0] + R.W_OWN[1]) < R.W_OWN[0]
    assert 20 * (R.W_OWN[1] + R.W_OPP[1]) < R.W_OPP[0]
    assert 20 * (R.W_OWN[0] + R.W_OPP[0]) < 2 ** 53  # every score and sum is exact as a double


# ---------------------------------------------------------------------------------------------- C boundary
def _args(fake, **kw):
    """A well-formed gmz_game_anchor_move argument list over fake pointers (4 boards of 6x6), single ones replaced."""
    names = ["boards", "players", "game", "noise", "noise_bytes", "G", "size", "n_in_row", "kind", "scale", "actions",
             "actions_bytes", "scores", "scores_bytes", "stream"]
    vals = dict.fromkeys(names, fake)
    vals.update(noise_bytes=4 * 36 * 8, G=4, size=6, n_in_row=5, kind=0, scale=0.0, actions_bytes=16,
                scores_bytes=4 * 36 * 8, stream=None)
    assert set(kw) <= set(names)
    vals.update(kw)
    return [vals[k] for k in names]


REFUSALS = [
    ("G", dict(G=0), "shape"), ("size 0", dict(size=0), "shape"), ("size 23", dict(size=23, n_in_row=5), "shape"),
    ("negative size", dict(size=-6), "shape"),
    ("n_in_row 0", dict(n_in_row=0), "n_in_row"), ("n_in_row > size", dict(n_in_row=7), "n_in_row"),
    ("kind 2", dict(kind=2), "kind"), ("kind -1", dict(kind=-1), "kind"),
    ("negative scale", dict(scale=-0.5), "scale"), ("infinite scale", dict(scale=float("inf")), "scale"),
    ("nan scale", dict(scale=float("nan")), "scale"),
    ("null boards", dict(boards=None), "null"), ("null players", dict(players=None), "null"),
    ("null actions", dict(actions=None), "null"),
    ("short noise", dict(noise_bytes=4 * 36 * 8 - 1), "noise"),
    ("short actions", dict(actions_bytes=15), "actions"),
    ("short scores", dict(scores_bytes=4 * 36 * 8 - 8), "scores"),
]


@pytest.mark.parametrize("what,wrong,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_anchor_move_refuses_before_any_launch(what, wrong, word):
    import datou_gomoku_muzero_amd._lib as L
    lib = L.load()
    fake = ctypes.c_void_p(1 << 20)
    assert lib.gmz_game_anchor_move(*_args(fake, **wrong)) < 0, what
    err = lib.gmz_last_error().decode()
    assert err.startswith(FN + ":") and word in err, (what, err)


def test_short_buffer_messages_name_both_sizes():
    import datou_gomoku_muzero_amd._lib as L
    lib = L.load()
    fake = ctypes.c_void_p(1 << 20)
    assert lib.gmz_game_anchor_move(*_args(fake, scores_bytes=100)) < 0
    err = lib.gmz_last_error().decode()
    assert "100" in err and str(4 * 36 * 8) in err
    # a short noise or scores capacity does not matter when that array is not given
    assert lib.gmz_game_anchor_move(*_args(fake, noise=None, noise_bytes=0, G=0)) < 0
    assert "shape" in lib.gmz_last_error().decode()


# ---------------------------------------------------------------------------------------------- arena
def test_arena_refuses_a_bad_anchor_player():
    import datou_gomoku_muzero_amd.arena as AR
    from datou_gomoku_muzero_amd.config import GmzConfig
    cfg = GmzConfig(BOARD_SIZE=6, NUM_SIMULATIONS=16)
    book = AR.paired_openings(2, 6, seed=1)
    with pytest.raises(ValueError, match="kind"):
        AR.Arena(cfg, None, AR.AnchorPlayer("minimax"), 4, book)
    with pytest.raises(ValueError, match="scale"):
        AR.Arena(cfg, AR.AnchorPlayer("threat", scale=-1.0), None, 4, book)
    with pytest.raises(ValueError, match="scale"):
        AR.Arena(cfg, None, AR.AnchorPlayer("uniform", scale=float("nan")), 4, book)
    assert AR.AnchorPlayer().checked() == ("threat", 0.0) and AR.AnchorPlayer("uniform").checked() == ("uniform", 1.0)
    assert AR.AnchorPlayer("threat", 0.25).checked() == ("threat", 0.25)
    assert AR.anchor_from_name("anchor:uniform", 2.0) == AR.AnchorPlayer("uniform", 2.0)
    assert AR.anchor_from_name("weights.pt") is None and AR.AnchorPlayer("threat").name == "anchor:threat"


def test_engine_names_the_two_kinds():
    import datou_gomoku_muzero_amd.engine as E
    assert E.anchor_kind("threat") == R.THREAT and E.anchor_kind("uniform") == R.UNIFORM
    with pytest.raises(ValueError):
        E.anchor_kind("random")
