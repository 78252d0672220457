"""The forced-win (VCF) solver, host side (no GPU): the numpy model of the rule (tests/vcf_ref.py) on hand-built
positions whose outcome follows from the rule's text, gmz_game_vcf's refusals before any launch (fake pointers, never
dereferenced: the tests/test_abi.py pattern; no valid call is made with them), and the arena's check of
AnchorPlayer("vcf")."""
import ctypes

import numpy as np
import pytest

import anchor_ref as R
import vcf_ref as V
from test_anchor import _board, _full_but

FN = "gmz_game_vcf"

# harmless white stones for the 9x9 positions: no two of them share a window with a third
_SPREAD = [(8, 8), (6, 8), (8, 6), (6, 6), (5, 2), (7, 2)]
# black's corner: three stones along row 0 and three down column 0, so that (0,0) makes a four in both lines with the
# single completions (0,4) and (4,0): a double four on the lowest cell of the board
_CORNER = [(0, 1), (0, 2), (0, 3), (1, 0), (2, 0), (3, 0)]


def hand_built():
    """[(name, board int8 [S,S], player, n, max_depth, max_nodes, (status, move, length), nodes or None)]: the
    expected outcome worked out by hand from the rule (also run on the GPU by tests/test_vcf_gpu.py)."""
    S = 9
    cases = []
    # cell 0 is the first four in ascending order and T(0) = {(0,4), (4,0)}
    double = _board(S, _CORNER, _SPREAD)
    cases.append(("double four", double, 1, 5, 10, 2048, (V.FOUND, 0, 2), 1))
    # white's four (8,0)-(8,3) leaves the one five cell (8,4); black's column (5,4)-(7,4) makes (8,4) a four with the
    # reply (4,4): the only candidate, then the corner's double four: three attacker moves
    forced = _board(S, _CORNER + [(5, 4), (6, 4), (7, 4)], [(8, 0), (8, 1), (8, 2), (8, 3), (2, 7), (4, 7)])
    cases.append(("the block is a four", forced, 1, 5, 10, 2048, (V.FOUND, 8 * S + 4, 3), 2))
    cases.append(("the block is a four, depth 2", forced, 1, 5, 2, 2048, (V.NONE, -1, 0), 2))
    cases.append(("the block is a four, one node", forced, 1, 5, 10, 1, (V.BUDGET, -1, 0), 2))
    # without (5,4) the block at (8,4) is no four: black must block and has no forced win, corner or not
    passive = _board(S, _CORNER + [(6, 4), (7, 4)], [(8, 0), (8, 1), (8, 2), (8, 3), (2, 7), (4, 7)])
    cases.append(("the block is no four", passive, 1, 5, 10, 2048, (V.NONE, -1, 0), 1))
    # white's open four (8,1)-(8,4) has the two five cells (8,0) and (8,5)
    lost = _board(S, _CORNER, [(8, 1), (8, 2), (8, 3), (8, 4), (2, 7), (4, 7)])
    cases.append(("two five cells against", lost, 1, 5, 10, 2048, (V.NONE, -1, 0), 1))
    # the same with white to move: white completes its five on the smaller cell
    cases.append(("own five first", lost, -1, 5, 10, 2048, (V.FOUND, 8 * S + 0, 1), 1))
    # (2,3) joins (2,0)-(2,2) and (2,4)-(2,5): a line of six, and no other five cell
    over = _board(S, [(2, 0), (2, 1), (2, 2), (2, 4), (2, 5)], _SPREAD[:5])
    cases.append(("overline", over, 1, 5, 10, 2048, (V.FOUND, 2 * S + 3, 1), 1))
    # (0,6)-(0,8) end at the edge and white holds (0,3): the one window is (0,4)-(0,8), so (0,4) and (0,5) are fours
    # with one reply each; (0,5) also joins the column (1,5)-(3,5), reply (4,5): a double four.  In ascending order
    # (0,4) comes first and is searched (and fails) before (0,5) wins
    edge = _board(S, [(0, 6), (0, 7), (0, 8), (1, 5), (2, 5), (3, 5)], [(0, 3)] + _SPREAD[:5])
    cases.append(("four against the edge", edge, 1, 5, 10, 2048, (V.FOUND, 5, 2), None))
    cases.append(("four against the edge, depth 1", edge, 1, 5, 1, 2048, (V.NONE, -1, 0), 1))
    # 5x5 with n = 5: a line of five cells is its own single window (n equal to the board size).  Four stones of the
    # attacker and one empty cell in it: a five on that cell, in a row, a column and on either diagonal
    for what, cells, hole in (("row", [(2, c) for c in range(5)], 3), ("column", [(r, 1) for r in range(5)], 0),
                              ("diagonal", [(i, i) for i in range(5)], 2),
                              ("anti-diagonal", [(i, 4 - i) for i in range(5)], 4)):
        r, c = cells[hole]
        one = _board(5, [x for x in cells if x != (r, c)])
        cases.append(("5x5 single window, " + what, one, 1, 5, 10, 2048, (V.FOUND, r * 5 + c, 1), 1))
    # the same window held by the defender and nothing else on the board: the one block is no four, so no win
    theirs = _board(5, [], [(2, c) for c in range(5) if c != 3])
    cases.append(("5x5 single window, the defender's", theirs, 1, 5, 10, 2048, (V.NONE, -1, 0), 1))
    # 6x6, four in a row: (0,0) makes a four along row 0 (reply (0,3)) and down column 0 (reply (3,0))
    small = _board(6, [(0, 1), (0, 2), (1, 0), (2, 0)], [(5, 5), (3, 5), (5, 3), (4, 1)])
    cases.append(("n_in_row 4 on 6x6", small, 1, 4, 10, 2048, (V.FOUND, 0, 2), 1))
    cases.append(("full board", _full_but(S), 1, 5, 10, 2048, (V.NONE, -1, 0), 1))
    cases.append(("empty board", np.zeros((S, S), np.int8), -1, 5, 16, 2048, (V.NONE, -1, 0), 1))
    return cases


@pytest.mark.parametrize("case", hand_built(), ids=[c[0] for c in hand_built()])
def test_model_on_hand_built_positions(case):
    name, board, player, n, depth, nodes, want, want_nodes = case
    st, mv, ln, nd = V.solve(board, player, n, depth, nodes)
    assert (st, mv, ln) == want, (name, st, mv, ln, nd)
    assert want_nodes is None or nd == want_nodes, (name, nd)
    assert 1 <= nd <= nodes + 1 and (nd == nodes + 1) == (st == V.BUDGET)


def test_model_edge_case_searches_the_lower_four_first():
    cases = {c[0]: c for c in hand_built()}
    board, player = cases["four against the edge"][1:3]
    T = V.fours(board.reshape(-1), player, 5)
    # the column's windows (0,5)-(4,5) and (1,5)-(5,5) make (4,5) and (5,5) fours as well
    assert sorted(T) == [4, 5, 41, 50] and T[4] == {5} and T[5] == {4, 41} and T[41] == {5, 50} and T[50] == {41}
    assert V.solve(board, player, 5)[3] > 2  # (0,4) was searched before (0,5) won
    board = cases["overline"][1]
    b = board.copy()
    b[2, 3] = 1
    assert V.five(board.reshape(-1), 1, 5) == [2 * 9 + 3] and R.wins(b, 2 * 9 + 3, 5) and b[2, :6].all()


@pytest.mark.parametrize("S,n", [(6, 4), (6, 5), (7, 3), (9, 5), (9, 9)])
def test_model_five_is_check_win(S, n):
    """five(b, s) is exactly the set of empty cells on which a stone of s makes a line of at least n (overlines
    included): the reference's check_win as tests/anchor_ref.py models it."""
    rs = np.random.RandomState(100 * S + n)
    hits = 0
    for fill in (0.2, 0.5, 0.8):
        for _ in range(6):
            b = rs.choice(np.array([0, 1, -1], np.int8), size=(S, S), p=[1 - fill, fill / 2, fill / 2])
            for s in (1, -1):
                want = []
                for c in np.flatnonzero(b.reshape(-1) == 0):
                    t = b.copy()
                    t.reshape(-1)[c] = s
                    if R.wins(t, int(c), n):
                        want.append(int(c))
                assert V.five(b.reshape(-1), s, n) == want
                hits += len(want)
    assert hits > 0


def test_model_play_game_with_a_solver_side():
    """A game with a ("vcf", ...) side: every solver move is the model's own solve() on that position, and a game of
    two threat sides equals anchor_ref.play_game."""
    S = 9
    solved_total = 0
    for seed in range(4):
        noise = np.random.RandomState(seed).gumbel(0, 1, (S * S + 1, S * S))
        pos = []
        w, moves, solved = V.play_game(np.zeros(S * S, np.int8), 1, [("vcf", 3e3, 10, 2048), ("threat", 3e3)],
                                       lambda ply: noise[ply], 5, pos)
        assert len(pos) == len(moves) and w in (-1, 0, 1)
        n = 0
        for ply in range(0, len(moves), 2):
            st, mv, _, _ = V.solve(pos[ply][0], pos[ply][1], 5, 10, 2048)
            if st == V.FOUND:
                assert moves[ply] == mv
                n += 1
            else:
                assert moves[ply] == R.move(pos[ply][0], pos[ply][1], 5, noise[ply], R.THREAT, 3e3)[1]
        assert n == solved
        solved_total += solved
        w2, m2 = R.play_game(np.zeros(S * S, np.int8), 1, [(R.THREAT, 3e3)] * 2, lambda ply: noise[ply], 5)
        again = V.play_game(np.zeros(S * S, np.int8), 1, [(R.THREAT, 3e3)] * 2, lambda ply: noise[ply], 5)
        assert again == (w2, m2, 0)
    assert solved_total > 0


# ---------------------------------------------------------------------------------------------- C boundary
NAMES = ["boards", "players", "game", "G", "size", "n_in_row", "max_depth", "max_nodes", "status", "status_bytes",
         "moves", "moves_bytes", "lengths", "lengths_bytes", "nodes", "nodes_bytes", "actions", "actions_bytes",
         "stream"]


def _args(fake, **kw):
    """A well-formed gmz_game_vcf argument list over fake pointers (4 boards of 6x6), single ones replaced."""
    vals = dict.fromkeys(NAMES, fake)
    vals.update(G=4, size=6, n_in_row=5, max_depth=10, max_nodes=2048, status_bytes=4, moves_bytes=16,
                lengths_bytes=16, nodes_bytes=16, actions_bytes=16, stream=None)
    assert set(kw) <= set(NAMES)
    vals.update(kw)
    return [vals[k] for k in NAMES]


REFUSALS = [
    ("G 0", dict(G=0), "G"), ("negative G", dict(G=-4), "G"),
    ("size 0", dict(size=0), "size"), ("negative size", dict(size=-6), "size"),
    ("size 23", dict(size=23), "size"),
    ("n_in_row 2", dict(n_in_row=2), "n_in_row"), ("n_in_row > size", dict(n_in_row=7), "n_in_row"),
    ("max_depth 0", dict(max_depth=0), "max_depth"), ("max_depth 17", dict(max_depth=17), "max_depth"),
    ("max_nodes 0", dict(max_nodes=0), "max_nodes"), ("max_nodes over", dict(max_nodes=(1 << 20) + 1), "max_nodes"),
    ("null boards", dict(boards=None), "null boards"), ("null players", dict(players=None), "null players"),
    ("null status", dict(status=None), "null status"), ("null moves", dict(moves=None), "null moves"),
    ("short status", dict(status_bytes=3), "status holds 3 bytes, G * 1 = 4"),
    ("short moves", dict(moves_bytes=15), "moves holds 15 bytes, G * 4 = 16"),
    ("short lengths", dict(lengths_bytes=12), "lengths holds 12 bytes, G * 4 = 16"),
    ("short nodes", dict(nodes_bytes=0), "nodes holds 0 bytes, G * 4 = 16"),
    ("short actions", dict(actions_bytes=8), "actions holds 8 bytes, G * 4 = 16"),
]


@pytest.mark.parametrize("what,wrong,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_vcf_refuses_before_any_launch(what, wrong, word):
    import datou_gomoku_muzero_amd._lib as L
    lib = L.load()
    fake = ctypes.c_void_p(1 << 20)
    assert lib.gmz_game_vcf(*_args(fake, **wrong)) < 0, what
    err = lib.gmz_last_error().decode()
    assert err.startswith(FN + ":") and word in err, (what, err)


def test_byte_counts_of_absent_arrays_are_ignored():
    """With lengths, nodes and actions null their byte counts do not matter: the next refusal is reported (G = 0
    here, so that no launch is made with the fake pointers)."""
    import datou_gomoku_muzero_amd._lib as L
    lib = L.load()
    fake = ctypes.c_void_p(1 << 20)
    absent = dict(lengths=None, lengths_bytes=0, nodes=None, nodes_bytes=0, actions=None, actions_bytes=0, game=None)
    for wrong, word in ((dict(G=0), "G"), (dict(max_depth=0), "max_depth")):
        assert lib.gmz_game_vcf(*_args(fake, **absent, **wrong)) < 0
        assert word in lib.gmz_last_error().decode() and "holds" not in lib.gmz_last_error().decode()
    assert L.ABI_VERSION == 10 == lib.gmz_abi_version()
    # the anchor entry keeps refusing a third kind
    assert lib.gmz_game_anchor_move(fake, fake, fake, fake, 4 * 36 * 8, 4, 6, 5, 2, 0.0, fake, 16, fake, 4 * 36 * 8,
                                    None) < 0
    assert "kind" in lib.gmz_last_error().decode()


# ---------------------------------------------------------------------------------------------- arena
def test_arena_checks_a_vcf_anchor():
    import datou_gomoku_muzero_amd.arena as AR
    import datou_gomoku_muzero_amd.engine as E
    from datou_gomoku_muzero_amd.config import GmzConfig
    a = AR.AnchorPlayer("vcf")
    assert a.checked() == ("vcf", 0.0, 10, 2048) and a.name == "anchor:vcf"
    assert (a.depth, a.nodes) == (E.VCF_DEPTH, E.VCF_NODES)
    assert AR.AnchorPlayer("vcf", 0.5, depth=16, nodes=1 << 20).checked() == ("vcf", 0.5, 16, 1 << 20)
    assert AR.anchor_from_name("anchor:vcf") == a
    assert AR.anchor_from_name("anchor:vcf", 0.25, 4, 64) == AR.AnchorPlayer("vcf", 0.25, 4, 64)
    assert AR.anchor_from_name("anchor:vcf", depth=4).checked() == ("vcf", 0.0, 4, 2048)
    # the two older kinds are what they were
    assert AR.AnchorPlayer().checked() == ("threat", 0.0) and AR.AnchorPlayer("uniform").checked() == ("uniform", 1.0)
    assert AR.anchor_from_name("anchor:threat", 2.0) == AR.AnchorPlayer("threat", 2.0)
    for bad in (0, 17, -1, 2.5, None, True):
        with pytest.raises(ValueError, match="depth"):
            AR.AnchorPlayer("vcf", depth=bad).checked()
    for bad in (0, (1 << 20) + 1, -5, 100.0, None):
        with pytest.raises(ValueError, match="nodes"):
            AR.AnchorPlayer("vcf", nodes=bad).checked()
    with pytest.raises(ValueError, match="scale"):
        AR.AnchorPlayer("vcf", scale=-1.0).checked()
    cfg = GmzConfig(BOARD_SIZE=6, NUM_SIMULATIONS=16)
    book = AR.paired_openings(2, 6, seed=1)
    with pytest.raises(ValueError, match="depth"):
        AR.Arena(cfg, None, AR.AnchorPlayer("vcf", depth=17), 4, book)
    with pytest.raises(ValueError, match="nodes"):
        AR.Arena(cfg, AR.AnchorPlayer("vcf", nodes=0), None, 4, book)
    with pytest.raises(ValueError):  # the threat launch's kinds stay two: the solver is a call of its own
        E.anchor_kind("vcf")
