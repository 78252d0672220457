"""The alpha-beta anchor, host side (no GPU): the numpy model of the rule (tests/ab_ref.py) on hand-built positions
whose outcome follows from the rule's text, pruned against unpruned search, gmz_game_alphabeta's refusals before any
launch (fake pointers, never dereferenced: the tests/test_conv_sizes.py pattern; no valid call is made with them),
and the arena's check of AnchorPlayer("ab")."""
import ctypes

import numpy as np
import pytest

import ab_ref as AB
import anchor_ref as R
import vcf_ref as V
from test_anchor import _board, _full_but
from test_vcf import _CORNER, _SPREAD

FN = "gmz_game_alphabeta"
S9 = 9


def hand_built():
    """[(name, board int8 [S,S], player, n, plies, width, max_nodes, (status, move or None, value or None), nodes or
    None)]: the expected outcome worked out by hand from the rule (also run on the GPU by tests/test_ab_gpu.py).
    None: not fixed by hand."""
    cases = []
    # black's open three (4,3)-(4,5): a stone on (4,2) or (4,6) leaves two five cells, white (whose stones share no
    # window) blocks one, and the node at ply 2 has five(b, black) not empty: WIN - 2.  One ply deep the reply is a
    # leaf and only E is seen
    three = _board(S9, [(4, 3), (4, 4), (4, 5)], _SPREAD[:3])
    for plies in (2, 3, 4):
        cases.append(("open three, plies %d" % plies, three, 1, 5, plies, 8, 2048, (AB.SEARCHED, None, AB.WIN - 2), None))
    # white's open four (8,1)-(8,4) has the two five cells (8,0) and (8,5): whatever black plays, white's node at ply 1
    # has a five.  Every candidate has the same value, so the move is the first: the threat rule's block, on (8,5),
    # which lies in more windows than (8,0)
    lost = _board(S9, _CORNER, [(8, 1), (8, 2), (8, 3), (8, 4), (2, 7), (4, 7)])
    assert R.move(lost, 1, 5)[1] == 8 * S9 + 5
    for plies, nodes in ((1, 9), (2, 9), (4, 9)):
        cases.append(("two fives against, plies %d" % plies, lost, 1, 5, plies, 8, 2048,
                      (AB.SEARCHED, 8 * S9 + 5, -(AB.WIN - 1)), nodes))
    # the same with white to move: the root's five, on the smaller cell, with the value WIN and one node
    cases.append(("root five", lost, -1, 5, 4, 8, 2048, (AB.SEARCHED, 8 * S9 + 0, AB.WIN), 1))
    cases.append(("full board", _full_but(S9), 1, 5, 4, 8, 2048, (AB.SKIPPED, -1, 0), 0))
    # one empty cell that is no five of white's: the root's one candidate, then a node with no empty cell: 0
    cases.append(("one empty cell", _full_but(S9, 40), -1, 5, 4, 8, 2048, (AB.SEARCHED, 40, 0), 2))
    # the empty board at one ply: 8 leaves; the centre's 20 windows each add 2 for the mover at the leaf (white: -1)
    cases.append(("empty board, one ply", np.zeros((S9, S9), np.int8), 1, 5, 1, 8, 2048, (AB.SEARCHED, 40, 20), 9))
    cases.append(("empty board at the budget", np.zeros((S9, S9), np.int8), 1, 5, 4, 8, 5, (AB.BUDGET, -1, 0), 6))
    return cases


@pytest.mark.parametrize("case", hand_built(), ids=[c[0] for c in hand_built()])
def test_model_on_hand_built_positions(case):
    name, board, player, n, plies, width, nodes, want, want_nodes = case
    st, mv, val, nd = AB.search(board, player, n, plies, width, nodes)
    assert st == want[0], (name, st, mv, val, nd)
    assert want[1] is None or mv == want[1], (name, mv)
    assert want[2] is None or val == want[2], (name, val)
    assert want_nodes is None or nd == want_nodes, (name, nd)
    assert (nd == nodes + 1) == (st == AB.BUDGET) and (mv == -1 and val == 0) == (st != AB.SEARCHED)


def test_model_open_three_needs_two_plies():
    three = hand_built()[0][1]
    st, mv, val, _ = AB.search(three, 1, 5, 1, 8, 2048)
    assert st == AB.SEARCHED and abs(val) < AB.WIN - 8  # a static value, no win seen
    _, mv2, val2, _ = AB.search(three, 1, 5, 2, 8, 2048)
    assert val2 == AB.WIN - 2 and mv2 in (4 * S9 + 2, 4 * S9 + 6)


def _static_by_hand(b, s, n):
    """E(b, s) cell by cell as the rule is worded, in Python ints."""
    S = b.shape[0]
    total = 0
    for dr, dc in R.DIRS:
        for r in range(S):
            for c in range(S):
                cells = [(r + j * dr, c + j * dc) for j in range(n)]
                if any(not (0 <= y < S and 0 <= x < S) for y, x in cells):
                    continue
                vals = [int(b[y, x]) for y, x in cells]
                if vals.count(s) >= 1 and vals.count(-s) == 0:
                    total += 2 * 8 ** (vals.count(s) - 1)
                if vals.count(-s) >= 1 and vals.count(s) == 0:
                    total -= 8 ** (vals.count(-s) - 1)
    return total


def test_model_static_value_and_candidates():
    b = _board(S9, [(4, 4)])
    assert AB.static_value(b, 1, 5) == 40 and AB.static_value(b, -1, 5) == -20
    # a window with stones of both colours counts for neither: black's column and diagonal from (0,0); white's row from
    # (0,1), column and diagonal
    b3 = _board(S9, [(0, 0)], [(0, 1)])
    assert AB.static_value(b3, 1, 5) == 2 * 2 - 3 and AB.static_value(b3, -1, 5) == 2 * 3 - 2
    # two black stones in a row: the 4 windows that hold both add 2 * 8 each
    b2 = _board(S9, [(4, 4), (4, 5)])
    assert AB.static_value(b2, 1, 5) == _static_by_hand(b2, 1, 5) > 4 * 16
    rs = np.random.RandomState(11)
    for S, n in ((6, 4), (7, 5), (9, 8)):
        for fill in (0.1, 0.4):
            b = rs.choice(np.array([0, 1, -1], np.int8), size=(S, S), p=[1 - fill, fill / 2, fill / 2])
            for s in (1, -1):
                assert AB.static_value(b, s, n) == _static_by_hand(b, s, n)
    # candidates: score descending, ties to the smaller cell; the root's are choose() without replacement
    sc = R.scores(b2, -1, 5)
    c = AB.cand(b2, -1, 5, 6)
    assert len(c) == 6 and all((sc[x], -x) > (sc[y], -y) for x, y in zip(c, c[1:]))
    assert (sc[c[-1]], -c[-1]) >= max((sc[x], -x) for x in range(81) if sc[x] >= 0 and x not in c)
    assert AB.root_cand(b2, -1, 5, 6) == c and AB.cand(_full_but(S9, 7), 1, 5, 6) == [7]
    noise = np.random.RandomState(3).gumbel(0, 1, 81)
    rc = AB.root_cand(b2, -1, 5, 6, noise, 3e3)
    assert rc[0] == R.choose(sc, noise, 3e3) and len(set(rc)) == 6 and rc != c
    key = sc.astype(np.float64) + 3e3 * noise
    assert all(key[x] >= key[y] for x, y in zip(rc, rc[1:]))


@pytest.mark.parametrize("S,n,plies,width", [(6, 4, 3, 4), (6, 4, 4, 3), (7, 5, 3, 5)])
def test_pruned_search_equals_plain_minimax(S, n, plies, width):
    """Turning the alpha/beta cut off changes neither the value nor the move, and never lowers the node count."""
    b, p = V.threat_game_positions(S, n, 3, seed=2)
    rs = np.random.RandomState(5)
    saved = wins = 0
    for i in range(0, len(b), 2):
        noise = rs.gumbel(0, 1, S * S) if i % 4 else None
        st, mv, val, nd = AB.search(b[i], p[i], n, plies, width, 1 << 20, noise, 0.5)
        st2, mv2, val2, nd2 = AB.search(b[i], p[i], n, plies, width, 1 << 20, noise, 0.5, prune=False)
        assert (st, mv, val) == (st2, mv2, val2) and nd <= nd2, (i, mv, mv2, val, val2, nd, nd2)
        saved += nd2 - nd
        wins += abs(val) >= AB.WIN - plies
    assert saved > 0 and wins > 0


def test_model_play_game_with_an_ab_side():
    """A game with an ("ab", ...) side: the solver's move where it finds a win, else the alpha-beta move, else the
    threat rule's; a game without one equals vcf_ref.play_game."""
    S, n = 6, 4
    side = ("ab", 3e3, 6, 64, 2, 4)
    total = [0, 0, 0]
    for seed in range(3):
        noise = np.random.RandomState(seed).gumbel(0, 1, (S * S + 1, S * S))
        pos = []
        w, moves, by = AB.play_game(np.zeros(S * S, np.int8), 1, [side, ("threat", 3e3)], lambda ply: noise[ply], n, pos)
        assert len(pos) == len(moves) and w in (-1, 0, 1) and sum(by) == len(moves)
        for ply in range(0, len(moves), 2):
            b, p = pos[ply]
            if V.solve(b, p, n, 6, 64)[0] == V.FOUND:
                want = V.solve(b, p, n, 6, 64)[1]
            else:
                st, mv, _, _ = AB.search(b, p, n, 2, 4, 64, noise[ply], 3e3)
                want = mv if st == AB.SEARCHED else R.move(b, p, n, noise[ply], R.THREAT, 3e3)[1]
            assert moves[ply] == want
        total = [x + y for x, y in zip(total, by)]
        sides = [("vcf", 3e3, 6, 64), ("threat", 3e3)]
        w2, m2, solved = V.play_game(np.zeros(S * S, np.int8), 1, sides, lambda ply: noise[ply], n)
        assert AB.play_game(np.zeros(S * S, np.int8), 1, sides, lambda ply: noise[ply], n)[:2] == (w2, m2)
    assert total[2] > 0


# ---------------------------------------------------------------------------------------------- C boundary
NAMES = ["boards", "players", "game", "noise", "noise_bytes", "scale", "G", "size", "n_in_row", "plies", "width",
         "max_nodes", "status", "status_bytes", "moves", "moves_bytes", "values", "values_bytes", "nodes", "nodes_bytes",
         "actions", "actions_bytes", "stream"]


def _args(fake, **kw):
    """A well-formed gmz_game_alphabeta argument list over fake pointers (4 boards of 6x6), single ones replaced."""
    vals = dict.fromkeys(NAMES, fake)
    vals.update(noise_bytes=4 * 36 * 8, scale=0.0, G=4, size=6, n_in_row=5, plies=4, width=8, max_nodes=2048,
                status_bytes=4, moves_bytes=16, values_bytes=32, nodes_bytes=16, actions_bytes=16, stream=None)
    assert set(kw) <= set(NAMES)
    vals.update(kw)
    return [vals[k] for k in NAMES]


REFUSALS = [
    ("G 0", dict(G=0), "G"), ("negative G", dict(G=-4), "G"),
    ("size 0", dict(size=0), "size"), ("negative size", dict(size=-6), "size"), ("size 23", dict(size=23), "size"),
    ("n_in_row 2", dict(n_in_row=2), "n_in_row"), ("n_in_row > size", dict(n_in_row=7), "n_in_row"),
    ("n_in_row 9", dict(n_in_row=9, size=12, noise_bytes=4 * 144 * 8), "n_in_row"),
    ("plies 0", dict(plies=0), "plies"), ("plies 9", dict(plies=9), "plies"),
    ("width 0", dict(width=0), "width"), ("width 17", dict(width=17), "width"),
    ("max_nodes 0", dict(max_nodes=0), "max_nodes"), ("max_nodes over", dict(max_nodes=(1 << 20) + 1), "max_nodes"),
    ("negative scale", dict(scale=-1.0), "scale"), ("scale nan", dict(scale=float("nan")), "scale"),
    ("scale inf", dict(scale=float("inf")), "scale"),
    ("null boards", dict(boards=None), "null boards"), ("null players", dict(players=None), "null players"),
    ("null status", dict(status=None), "null status"), ("null moves", dict(moves=None), "null moves"),
    ("short noise", dict(noise_bytes=4 * 36 * 8 - 1), "noise holds 1151 bytes, G * A * 8 = 1152"),
    ("short status", dict(status_bytes=3), "status holds 3 bytes, G * 1 = 4"),
    ("short moves", dict(moves_bytes=15), "moves holds 15 bytes, G * 4 = 16"),
    ("short values", dict(values_bytes=31), "values holds 31 bytes, G * 8 = 32"),
    ("short nodes", dict(nodes_bytes=0), "nodes holds 0 bytes, G * 4 = 16"),
    ("short actions", dict(actions_bytes=8), "actions holds 8 bytes, G * 4 = 16"),
]


@pytest.mark.parametrize("what,wrong,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_alphabeta_refuses_before_any_launch(what, wrong, word):
    import datou_gomoku_muzero_amd._lib as L
    lib = L.load()
    fake = ctypes.c_void_p(1 << 20)
    assert lib.gmz_game_alphabeta(*_args(fake, **wrong)) < 0, what
    err = lib.gmz_last_error().decode()
    assert err.startswith(FN + ":") and word in err, (what, err)


def test_byte_counts_of_absent_arrays_are_ignored():
    """With noise, values, nodes and actions null their byte counts do not matter: the next refusal is reported (so
    that no launch is made with the fake pointers).  The largest allowed arguments pass every range check."""
    import datou_gomoku_muzero_amd._lib as L
    lib = L.load()
    fake = ctypes.c_void_p(1 << 20)
    absent = dict(noise=None, noise_bytes=0, values=None, values_bytes=0, nodes=None, nodes_bytes=0, actions=None,
                  actions_bytes=0, game=None)
    for wrong, word in ((dict(G=0), "G"), (dict(plies=0), "plies")):
        assert lib.gmz_game_alphabeta(*_args(fake, **absent, **wrong)) < 0
        assert word in lib.gmz_last_error().decode() and "holds" not in lib.gmz_last_error().decode()
    top = dict(size=22, n_in_row=8, plies=8, width=16, max_nodes=1 << 20, scale=1e300, noise_bytes=4 * 484 * 8)
    assert lib.gmz_game_alphabeta(*_args(fake, **top, status_bytes=3)) < 0
    assert "status holds" in lib.gmz_last_error().decode()
    assert L.ABI_VERSION == 10 == lib.gmz_abi_version()


# ---------------------------------------------------------------------------------------------- arena
def test_arena_checks_an_ab_anchor():
    import datou_gomoku_muzero_amd.arena as AR
    import datou_gomoku_muzero_amd.engine as E
    from datou_gomoku_muzero_amd.config import GmzConfig
    a = AR.AnchorPlayer("ab")
    assert a.checked() == ("ab", 0.0, 10, 2048, 4, 8) and a.name == "anchor:ab"
    assert (a.plies, a.width, a.nodes) == (E.AB_PLIES, E.AB_WIDTH, E.AB_NODES) == (AB.PLIES, AB.WIDTH, AB.NODES)
    assert AR.AnchorPlayer("ab", 0.5, 16, 1 << 20, 8, 16).checked() == ("ab", 0.5, 16, 1 << 20, 8, 16)
    assert AR.AnchorPlayer("ab", plies=1, width=1).checked() == ("ab", 0.0, 10, 2048, 1, 1)
    assert AR.anchor_from_name("anchor:ab") == a
    assert AR.anchor_from_name("anchor:ab", 0.25, 4, 64, 2, 3) == AR.AnchorPlayer("ab", 0.25, 4, 64, 2, 3)
    assert AR.anchor_from_name("anchor:ab", plies=2, width=4).checked() == ("ab", 0.0, 10, 2048, 2, 4)
    # the older kinds are what they were: plies and width are not theirs to check or to report
    assert AR.AnchorPlayer().checked() == ("threat", 0.0) and AR.AnchorPlayer("uniform").checked() == ("uniform", 1.0)
    assert AR.AnchorPlayer("vcf", plies=0, width=99).checked() == ("vcf", 0.0, 10, 2048)
    assert AR.anchor_from_name("anchor:vcf", 0.25, 4, 64) == AR.AnchorPlayer("vcf", 0.25, 4, 64)
    for bad in (0, 9, -1, 2.5, None, True):
        with pytest.raises(ValueError, match="plies"):
            AR.AnchorPlayer("ab", plies=bad).checked()
    for bad in (0, 17, -2, 4.0, None, False):
        with pytest.raises(ValueError, match="width"):
            AR.AnchorPlayer("ab", width=bad).checked()
    with pytest.raises(ValueError, match="nodes"):
        AR.AnchorPlayer("ab", nodes=0).checked()
    with pytest.raises(ValueError, match="depth"):
        AR.AnchorPlayer("ab", depth=17).checked()
    with pytest.raises(ValueError, match="scale"):
        AR.AnchorPlayer("ab", scale=-1.0).checked()
    for bad in ("minimax", "random"):
        with pytest.raises(ValueError, match="'threat', 'uniform', 'vcf' or 'ab'"):
            AR.AnchorPlayer(bad).checked()
    cfg = GmzConfig(BOARD_SIZE=6, NUM_SIMULATIONS=16)
    book = AR.paired_openings(2, 6, seed=1)
    with pytest.raises(ValueError, match="plies"):
        AR.Arena(cfg, None, AR.AnchorPlayer("ab", plies=9), 4, book)
    with pytest.raises(ValueError, match="width"):
        AR.Arena(cfg, AR.AnchorPlayer("ab", width=0), None, 4, book)
    assert E.ANCHOR_KINDS == {"threat": 0, "uniform": 1}
    with pytest.raises(ValueError):  # the threat launch's kinds stay two: the search is a call of its own
        E.anchor_kind("ab")
