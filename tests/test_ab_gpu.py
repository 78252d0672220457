"""The alpha-beta anchor on the GPU (gmz_game_alphabeta, engine.alphabeta, BatchedSelfPlayEngine.ab_move,
arena.AnchorPlayer("ab")).  Every comparison is exact: status, move, value and node count are integers that the kernel
and the numpy model (tests/ab_ref.py) must give alike, since both walk the same tree in the same order.

  1. kernel against model on positions of model games between two threat anchors (noise scale 3e3, from the empty
     board: vcf_ref.threat_game_positions), 6x6 to 22x22, n = 4 and 5, in guarded buffers, budget 2,048; and at the
     edge shapes 5x5 with n = 5, 8x8 with n = 8 and 7x7 with n = 3;
  2. the limits: plies 1 and 8, width 1 and 16, max_nodes 1, 8 and 64 on the 9x9 batch of 65;
  3. the root's order under a noise row at scale 0 and 3e3, and ties without noise;
  4. game_dev with negative entries, actions_dev in/out, the nullable outputs, the hand-built positions;
  5. engine.alphabeta and ab_move;
  6. arena matches: anchor:ab against anchor:threat equals the model's games (one and two streams), against itself
     scores 0.5, against a HashNet side equals the same games played one at a time;  7. the command line.

The model's work in this file is about 10^5 nodes for test 1 and a third of that for the rest; it runs once per set of
arguments (functools.lru_cache) and its results are read-only."""
import functools
import json

import numpy as np
import pytest

import ab_ref as AB
import anchor_ref as R
import test_ab as TA
import vcf_ref as V

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NODES = 2048
# (size, n): (model games, seed) of the position pool.  The seeds are chosen so that the model's own results meet the
# conditions asserted in test 1 (seed 1 does everywhere).
POOLS = {(6, 4): (19, 1), (9, 5): (8, 1), (15, 5): (3, 1), (19, 5): (1, 1), (22, 5): (1, 1), (6, 5): (7, 1),
         (5, 5): (40, 1), (8, 8): (12, 1), (7, 3): (200, 1)}
ALL = 0  # a batch of the whole pool


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import datou_gomoku_muzero_amd._lib as L
    import datou_gomoku_muzero_amd.arena as AR
    import datou_gomoku_muzero_amd.engine as E
    from datou_gomoku_muzero_amd.config import GmzConfig
    return dict(L=L, AR=AR, E=E, Cfg=GmzConfig, lib=L.load())


@functools.lru_cache(maxsize=None)
def pool(S, n, G=ALL):
    """(boards int8 [P, A], players int8 [P]) of the model games, read-only: the whole pool, or G of its positions,
    evenly spaced."""
    games, seed = POOLS[(S, n)]
    b, p = V.threat_game_positions(S, n, games, seed)
    if G != ALL:
        assert len(b) >= G
        idx = np.linspace(0, len(b) - 1, G).astype(int)
        b, p = b[idx], p[idx]
    b.setflags(write=False)
    p.setflags(write=False)
    return b, p


@functools.lru_cache(maxsize=None)
def noise_rows(S, n, G, seed=9):
    z = np.random.RandomState(seed).gumbel(0, 1, (len(pool(S, n, G)[0]), S * S))
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def reference(S, n, G, plies, width, nodes=NODES, scale=None):
    """The model's (status, move, value, nodes) on pool(S, n, G): computed once, shared, read-only.  ``scale``: with
    noise_rows at that scale (None: no noise)."""
    b, p = pool(S, n, G)
    out = AB.search_batch(b, p, n, plies, width, nodes, None if scale is None else noise_rows(S, n, G),
                          0.0 if scale is None else scale)
    for o in out:
        o.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def threat_moves(S, n, G):
    b, p = pool(S, n, G)
    return np.array([R.choose(R.scores(b[i], p[i], n)) for i in range(len(b))], np.int32)


def deep_wins(val, plies):
    return (val >= AB.WIN - plies) & (val <= AB.WIN - 2)


def subset(S, n, G, plies, width):
    """Indices into the whole pool of a batch of G positions: one position with a win seen below the root for G = 1;
    otherwise up to G / 2 such wins and evenly spaced positions for the rest."""
    st, _, val, _ = reference(S, n, ALL, plies, width)
    P = st.size
    deep = np.flatnonzero(deep_wins(val, plies))
    if G == 1:
        return deep[:1]
    pick = [int(i) for i in deep[:G // 2]]
    pick += [int(i) for i in np.linspace(0, P - 1, G).astype(int) if i not in pick][:G - len(pick)]
    pick += [i for i in range(P) if i not in pick][:G - len(pick)]
    return np.array(sorted(pick))


def run_kernel(m, boards, players, n, plies, width, nodes, noise=None, scale=0.0, game=None, actions=None,
               outputs=True):
    """gmz_game_alphabeta into guarded buffers: dict(status, move, value, nodes, actions) as numpy (None where not
    asked for).  ``actions``: int32 [G] going in."""
    from kernel_guards import Buf
    L, lib = m["L"], m["lib"]
    G = boards.shape[0]
    S = int(round(boards[0].size ** 0.5))
    b = torch.from_numpy(np.array(boards, np.int8)).cuda()  # copies: the pools are read-only
    p = torch.from_numpy(np.array(players, np.int8)).cuda()
    gm = None if game is None else torch.from_numpy(np.ascontiguousarray(game, dtype=np.int32)).cuda()
    nz = None if noise is None else torch.from_numpy(np.array(noise, np.float64)).cuda()
    st = Buf(G, torch.int8, off=1, fill=-7)
    mv = Buf(G, torch.int32, off=1, fill=-7)
    vl = Buf(G, torch.int64, off=1, fill=-7) if outputs else None
    nd = Buf(G, torch.int32, off=1, fill=-7) if outputs else None
    ac = None if actions is None else Buf(G, torch.int32, off=1, fill=-7, data=actions)

    def pb(x):
        return (L.ptr(x.t), L.nbytes(x.t)) if x is not None else (None, 0)
    L.check(lib.gmz_game_alphabeta(L.ptr(b), L.ptr(p), L.ptr(gm), L.ptr(nz), L.nbytes(nz), float(scale), G, S, n, plies,
                                   width, nodes, *pb(st), *pb(mv), *pb(vl), *pb(nd), *pb(ac), L.stream_ptr()))
    torch.cuda.synchronize()
    bufs = dict(status=st, move=mv, value=vl, nodes=nd, actions=ac)
    assert all(x.intact() for x in bufs.values() if x is not None)
    return {k: (None if x is None else x.t.cpu().numpy()) for k, x in bufs.items()}


def assert_equal(got, want, what):
    for k, w in zip(("status", "move", "value", "nodes"), want):
        assert np.array_equal(got[k], w), (what, k, np.flatnonzero(got[k] != w)[:8])


# ---------------------------------------------------------------------------------------------- 1. kernel against model
# (size, n, batch, plies, width); a batch of 1 or 65 beside ALL is cut from the whole pool's results
CASES = [(6, 4, ALL, 3, 6), (6, 4, 1, 3, 6), (6, 4, 65, 3, 6), (9, 5, ALL, 3, 6), (9, 5, 1, 3, 6), (9, 5, 65, 3, 6),
         (9, 5, 65, 4, 8), (15, 5, 65, 4, 8), (19, 5, 17, 4, 8), (22, 5, 17, 4, 8), (6, 5, 65, 4, 8)]


@pytest.mark.parametrize("S,n,G,plies,width", CASES,
                         ids=["%dx%d-n%d-G%s-p%dw%d" % (c[0], c[0], c[1], c[2] or "all", c[3], c[4]) for c in CASES])
def test_kernel_equals_the_model(mods, S, n, G, plies, width):
    """Conditions on the model's own results, so that the batch cannot be trivial.  A whole pool (about 250
    positions): the move differs from the threat rule's on at least 20 %, at least 10 values are wins seen below the
    root (in [WIN - plies, WIN - 2]), at least 5 are losses (<= -(WIN - plies)), at most 5 % end at the node budget.
    A batch of 65: 10 moves differ and 3 wins — but on 6x6 with n = 5, where a line has two windows only and wins are
    rare, 2 wins.  A batch of 17 (19x19 and 22x22, one game's positions): 5 moves differ and 1 win.  A batch of 1:
    that position is a win seen below the root."""
    whole = (plies, width) == (3, 6)
    if whole:
        idx = subset(S, n, G, plies, width) if G != ALL else np.arange(len(pool(S, n)[0]))
        b, p = (x[idx] for x in pool(S, n))
        want = [w[idx] for w in reference(S, n, ALL, plies, width)]
        thr = threat_moves(S, n, ALL)[idx]
    else:
        b, p = pool(S, n, G)
        want = reference(S, n, G, plies, width)
        thr = threat_moves(S, n, G)
    st, mv, val, nd = want
    differ, wins = int(((mv != thr) & (st == AB.SEARCHED)).sum()), int(deep_wins(val, plies).sum())
    losses, spent = int((val <= -(AB.WIN - plies)).sum()), int((st == AB.BUDGET).sum())
    print("%dx%d n %d plies %d width %d: %d positions, %d moves differ, %d wins below the root, %d losses, %d at the "
          "budget, nodes mean %.1f max %d" % (S, S, n, plies, width, st.size, differ, wins, losses, spent, nd.mean(),
                                              nd.max()))
    if G == ALL:
        assert 200 <= st.size <= 300
        assert differ >= 0.2 * st.size and wins >= 10 and losses >= 5 and spent <= 0.05 * st.size
    elif G == 65:
        assert st.size == 65 and differ >= 10 and wins >= (2 if (S, n) == (6, 5) else 3)
    elif G == 17:
        assert st.size == 17 and differ >= 5 and wins >= 1
    else:
        assert st.size == 1 and wins == 1
    got = run_kernel(mods, b, p, n, plies, width, NODES)
    assert_equal(got, want, (S, n, G, plies, width))


@pytest.mark.parametrize("S,n", [(5, 5), (8, 8), (7, 3)], ids=["5x5-n5", "8x8-n8", "7x7-n3"])
def test_kernel_equals_the_model_at_the_edge_shapes(mods, S, n):
    """n equal to the board size (a line is its own single window; 8 is the search's largest n) and n = 3, the
    smallest: 65 evenly spaced positions each, plies 3, width 6.  Conditions on the model's own results.  With n = S
    wins hardly exist, so there: every board searched, none at the node budget, at least 10 moves differ from the
    threat rule's.  With n = 3 on 7x7: at least 3 wins seen below the root and at least 5 losses."""
    plies, width = 3, 6
    b, p = pool(S, n, 65)
    want = reference(S, n, 65, plies, width)
    st, mv, val, nd = want
    differ, wins = int(((mv != threat_moves(S, n, 65)) & (st == AB.SEARCHED)).sum()), int(deep_wins(val, plies).sum())
    losses, spent = int((val <= -(AB.WIN - plies)).sum()), int((st == AB.BUDGET).sum())
    print("%dx%d n %d: %d positions, %d searched, %d moves differ, %d wins below the root, %d losses, %d at the budget, "
          "nodes max %d" % (S, S, n, st.size, (st == AB.SEARCHED).sum(), differ, wins, losses, spent, nd.max()))
    assert st.size == 65
    if n == S:
        assert (st == AB.SEARCHED).all() and spent == 0 and differ >= 10
    else:
        assert wins >= 3 and losses >= 5
    assert_equal(run_kernel(mods, b, p, n, plies, width, NODES), want, (S, n, plies, width))


# ---------------------------------------------------------------------------------------------- 2. limits
@pytest.mark.parametrize("plies,width,nodes", [(1, 8, NODES), (8, 8, 256), (4, 1, NODES), (2, 16, NODES), (4, 8, 1),
                                               (4, 8, 8), (4, 8, 64)])
def test_limits(mods, plies, width, nodes):
    """The ends of every range on the 9x9 batch of 65.  To keep the model's work small, plies 8 runs with a budget of
    256 (most boards end at status 2) and width 16 with 2 plies (up to 273 nodes a board)."""
    b, p = pool(9, 5, 65)
    want = reference(9, 5, 65, plies, width, nodes)
    st, mv, val, nd = want
    print("plies %d width %d nodes %d: %d searched, %d at the budget, most nodes %d" %
          (plies, width, nodes, (st == AB.SEARCHED).sum(), (st == AB.BUDGET).sum(), nd.max()))
    assert nd.max() <= nodes + 1 and (nd[st == AB.BUDGET] == nodes + 1).all()
    assert (mv[st != AB.SEARCHED] == -1).all() and (val[st != AB.SEARCHED] == 0).all()
    if plies == 1:
        assert (st == AB.SEARCHED).all() and nd.max() <= 1 + width
    if plies == 8:
        assert (st == AB.BUDGET).sum() > 32  # most boards
    if width == 1:  # one line of play: at most plies + 1 nodes, and the move is the threat rule's (but a root five's)
        assert nd.max() <= plies + 1 and np.array_equal(mv[val != AB.WIN], threat_moves(9, 5, 65)[val != AB.WIN])
    if width == 16:
        assert nd.max() > 1 + 16
    if nodes < 256:
        assert (st == AB.BUDGET).any() and ((st == AB.SEARCHED).any() or nodes == 1)
    assert_equal(run_kernel(mods, b, p, 5, plies, width, nodes), want, (plies, width, nodes))


# ---------------------------------------------------------------------------------------------- 3. the root's order
@pytest.mark.parametrize("scale", [0.0, 3e3])
def test_root_order_follows_the_key(mods, scale):
    """With a noise row the root's candidates are the anchor rule's: at scale 0 the noise breaks ties only, at 3e3 it
    changes the candidates and so the move."""
    b, p = pool(9, 5, 65)
    z = noise_rows(9, 5, 65)
    want = reference(9, 5, 65, 2, 4, NODES, scale)
    plain = reference(9, 5, 65, 2, 4)
    changed = int((want[1] != plain[1]).sum())
    print("scale %g: %d of 65 moves differ from the search without noise" % (scale, changed))
    assert changed >= (10 if scale else 1)
    # one candidate: the move is anchor_ref.choose's under the same row
    one = reference(9, 5, 65, 2, 1, NODES, scale)
    assert all(one[1][i] == R.choose(R.scores(b[i], p[i], 5), z[i], scale) for i in range(65))
    assert_equal(run_kernel(mods, b, p, 5, 2, 4, NODES, z, scale), want, ("noise", scale))
    assert_equal(run_kernel(mods, b, p, 5, 2, 1, NODES, z, scale), one, ("noise, width 1", scale))


def test_ties_go_to_the_smaller_cell(mods):
    """No noise: on the empty 15x15 board every cell four or more from each edge scores 20, and the candidates are the
    first of them in cell order, at the root and below it; a null noise pointer equals a row of zeros."""
    S = 15
    b = np.zeros((2, S * S), np.int8)
    b[1, 7 * S + 7] = 1
    p = np.array([1, -1], np.int8)
    assert AB.root_cand(b[0], 1, 5, 4) == AB.cand(b[0], 1, 5, 4) == [4 * S + 4, 4 * S + 5, 4 * S + 6, 4 * S + 7]
    want = AB.search_batch(b, p, 5, 3, 4, NODES)
    assert_equal(run_kernel(mods, b, p, 5, 3, 4, NODES), want, "ties")
    assert_equal(run_kernel(mods, b, p, 5, 3, 4, NODES, np.zeros((2, S * S)), 1.0), want, "zero noise")


# ---------------------------------------------------------------------------------------------- 4. game / actions
def test_kernel_on_the_hand_built_positions(mods):
    for name, board, player, n, plies, width, nodes, want, want_nodes in TA.hand_built():
        got = run_kernel(mods, board.reshape(1, -1), np.array([player], np.int8), n, plies, width, nodes)
        model = AB.search(board, player, n, plies, width, nodes)
        assert tuple(int(got[k][0]) for k in ("status", "move", "value", "nodes")) == model, name
        assert int(got["status"][0]) == want[0] and (want[1] is None or int(got["move"][0]) == want[1]), name
        assert want[2] is None or int(got["value"][0]) == want[2], name
        assert want_nodes is None or int(got["nodes"][0]) == want_nodes, name


def test_skipped_boards_and_actions_in_place(mods):
    b, p = (np.array(x) for x in pool(9, 5, 65))
    want = [np.array(w) for w in reference(9, 5, 65, 3, 6, 64)]  # budget 64: searched boards and boards at the budget
    G = 65
    full = 5
    b[full] = TA._full_but(9).reshape(-1)  # a full board: status 3 without a game array too
    for w, x in zip(want, (AB.SKIPPED, -1, 0, 0)):
        w[full] = x
    rs = np.random.RandomState(7)
    game = np.arange(G, dtype=np.int32) * 3
    out = np.zeros(G, bool)
    out[rs.permutation(G)[:G // 3]] = True
    out[np.flatnonzero(want[0] == AB.SEARCHED)[:2]] = True  # searched boards among the skipped ones
    game[out] = -1 - rs.randint(0, 5, int(out.sum()))
    before = (1000 + np.arange(G)).astype(np.int32)
    got = run_kernel(mods, b, p, 5, 3, 6, 64, game=game, actions=before)
    done = (want[0] == AB.SEARCHED) & ~out
    assert done.any() and ((want[0] == AB.BUDGET) & ~out).any() and not out[full]
    assert (got["status"][out] == AB.SKIPPED).all() and (got["move"][out] == -1).all()
    assert (got["value"][out] == 0).all() and (got["nodes"][out] == 0).all()
    for k, w in zip(("status", "move", "value", "nodes"), want):
        assert np.array_equal(got[k][~out], w[~out]), k
    assert np.array_equal(got["actions"], np.where(done, want[1], before))  # every other entry bit for bit
    # no game array: every board is searched; values, nodes and actions are optional
    got = run_kernel(mods, b, p, 5, 3, 6, 64, outputs=False)
    assert got["value"] is None and got["nodes"] is None and got["actions"] is None
    assert np.array_equal(got["status"], want[0]) and np.array_equal(got["move"], want[1])
    got = run_kernel(mods, b, p, 5, 3, 6, 64, actions=before)
    assert_equal(got, want, "actions without game")
    assert np.array_equal(got["actions"], np.where(want[0] == AB.SEARCHED, want[1], before))


# ---------------------------------------------------------------------------------------------- 5. engine
def test_engine_wrapper(mods):
    m = mods
    E = m["E"]
    b, p = pool(9, 5, 65)
    want = reference(9, 5, 65, 4, 8)
    bt = torch.from_numpy(b.reshape(-1, 9, 9).copy()).cuda()
    pt = torch.from_numpy(p.copy()).cuda()
    got = E.alphabeta(bt, pt)  # 4 plies, width 8, 2,048 nodes
    assert [t.dtype for t in got] == [torch.int8, torch.int32, torch.int64, torch.int32]
    assert_equal(dict(zip(("status", "move", "value", "nodes"), (t.cpu().numpy() for t in got))), want,
                 "engine.alphabeta")
    act = torch.full((65,), -5, dtype=torch.int32, device="cuda")
    game = torch.arange(65, dtype=torch.int32)
    game[::2] = -1
    z = noise_rows(9, 5, 65)
    st, mv, _, _ = E.alphabeta(bt, pt, plies=2, width=4, noise=torch.from_numpy(z.copy()).cuda(), scale=3e3, game=game,
                               actions=act)
    w2 = reference(9, 5, 65, 2, 4, NODES, 3e3)
    live = (game >= 0).numpy()
    assert np.array_equal(st.cpu().numpy(), np.where(live, w2[0], AB.SKIPPED))
    assert np.array_equal(act.cpu().numpy(), np.where(live & (w2[0] == AB.SEARCHED), w2[1], -5))
    b4, p4 = pool(6, 4, 65)
    got = E.alphabeta(torch.from_numpy(b4.reshape(-1, 6, 6).copy()).cuda(), p4.copy(), 2, 4, n_in_row=4)
    assert_equal(dict(zip(("status", "move", "value", "nodes"), (t.cpu().numpy() for t in got))),
                 AB.search_batch(b4, p4, 4, 2, 4), "n_in_row 4")
    with pytest.raises(m["L"].GmzError, match="gmz_game_alphabeta: plies"):
        E.alphabeta(bt, pt, plies=9)
    with pytest.raises(m["L"].GmzError, match="gmz_game_alphabeta: width"):
        E.alphabeta(bt, pt, width=17)
    with pytest.raises(ValueError, match="actions"):
        E.alphabeta(bt, pt, actions=act.cpu())


def test_ab_move_on_the_engine_boards(mods):
    """ab_move works over the engine's own boards and action buffer in place: after anchor_move, the entries whose
    search finished hold the alpha-beta move and the others the threat rule's."""
    m = mods
    E = m["E"]
    G, S = 16, 9
    b, p = pool(9, 5, 65)
    b, p = b[10:10 + G], p[10:10 + G]
    cfg = m["Cfg"](BOARD_SIZE=S, NUM_SIMULATIONS=16, NUM_RES_BLOCKS=2)
    e = E.BatchedSelfPlayEngine(cfg, num_games=G, seed=0)
    e.set_positions(b.reshape(G, S, S).copy(), p.copy(), [-1] * G)
    z = torch.from_numpy(noise_rows(9, 5, 65)[10:10 + G].copy()).cuda()
    thr = e.anchor_move(z, "threat", 3e3).cpu().numpy().copy()
    act = e.ab_move(z, 3e3, plies=3, width=4, nodes=24)
    assert act is e.action
    want = AB.search_batch(b, p, 5, 3, 4, 24, z.cpu().numpy(), 3e3)
    assert (want[0] == AB.SEARCHED).any() and (want[0] == AB.BUDGET).any()
    assert np.array_equal(e.ab_status.cpu().numpy(), want[0]) and np.array_equal(e.ab_moves.cpu().numpy(), want[1])
    assert np.array_equal(act.cpu().numpy(), np.where(want[0] == AB.SEARCHED, want[1], thr))
    e.anchor_move(z, "threat", 3e3)
    act = e.ab_move()  # the defaults, no noise
    want = AB.search_batch(b, p, 5)
    assert np.array_equal(act.cpu().numpy(), np.where(want[0] == AB.SEARCHED, want[1], thr))
    with pytest.raises(ValueError, match="noise"):
        e.ab_move(z.cpu())
    e.close()


# ---------------------------------------------------------------------------------------------- the matches
N_OPENINGS = 4
AB_SIDE = ("ab", 3e3, 10, 2048, 2, 4)  # AnchorPlayer("ab", 3e3, plies=2, width=4).checked()


def _noise(m, A, key, ply, seed, out):
    L = m["L"]
    k = torch.tensor([key], dtype=torch.int32, device="cuda")
    p = torch.tensor([ply], dtype=torch.int32, device="cuda")
    L.check(m["lib"].gmz_gumbel_keyed(L.ptr(k), L.ptr(p), seed, 1, A, L.ptr(out), L.nbytes(out), L.stream_ptr()))
    return out.cpu().numpy()[0]


def _records(res):
    return {2 * g.opening + (g.first_mover == "b"): (g.winner_colour, g.length, g.moves) for g in res.games}


def _arena(m, cfg, sides, slots, book, seed, streams=1):
    ar = m["AR"].Arena(cfg, sides[0], sides[1], slots, book, seed=seed, record_moves=True, streams=streams)
    res = ar.run()
    finished = int(ar.match.finished.cpu()[0])
    ar.close()
    return res, finished


@functools.lru_cache(maxsize=None)
def _model_match(seed):
    """anchor:ab (A) against anchor:threat (B) on 9x9 by the model: ({game id: (winner, length, moves)}, [threat,
    solver, alpha-beta] moves played).  Needs the GPU for the keyed noise rows only."""
    import datou_gomoku_muzero_amd._lib as L
    import datou_gomoku_muzero_amd.arena as AR
    m = dict(L=L, lib=L.load())
    book = AR.paired_openings(N_OPENINGS, 9, seed)
    noise = torch.zeros(1, 81, dtype=torch.float64, device="cuda")
    sides = [AB_SIDE, ("threat", AB_SIDE[1])]
    out, by = {}, [0, 0, 0]
    for t in range(N_OPENINGS):
        for first in (0, 1):
            w, moves, k = AB.play_game(book[0][t].reshape(81), int(book[1][t]), [sides[first], sides[1 - first]],
                                       lambda ply: _noise(m, 81, t, ply, seed, noise), 5)
            out[2 * t + first] = (w, len(moves), moves)
            by = [x + y for x, y in zip(by, k)]
    return out, by


# ---------------------------------------------------------------------------------------------- 6.
@pytest.mark.parametrize("slots,streams", [(8, 1), (3, 1), (4, 2)])
def test_ab_against_threat_equals_the_model(mods, slots, streams):
    m = mods
    AR = m["AR"]
    seed = 5
    cfg = m["Cfg"](BOARD_SIZE=9, NUM_SIMULATIONS=16, NUM_RES_BLOCKS=2)
    book = AR.paired_openings(N_OPENINGS, 9, seed)
    want, by = _model_match(seed)
    print("model: %d threat, %d solver and %d alpha-beta moves in %d games" % (by[0], by[1], by[2], len(want)))
    assert by[2] >= 10  # the search's move was played, so the match is not the threat anchor's against itself
    ab = AR.AnchorPlayer("ab", AB_SIDE[1], plies=2, width=4)
    assert ab.checked() == AB_SIDE
    res, finished = _arena(m, cfg, [ab, AR.AnchorPlayer("threat", AB_SIDE[1])], slots, book, seed, streams)
    assert finished == 2 * N_OPENINGS == len(res.games)
    rec = _records(res)
    for gid, w in want.items():
        assert rec[gid] == w, gid
    assert res.moves_played == sum(g.length for g in res.games)


def test_ab_against_itself_scores_one_half(mods):
    m = mods
    AR = m["AR"]
    cfg = m["Cfg"](BOARD_SIZE=9, NUM_SIMULATIONS=16, NUM_RES_BLOCKS=2)
    book = AR.paired_openings(N_OPENINGS, 9, 3)
    sides = [AR.AnchorPlayer("ab", 3e3, plies=2, width=4), AR.AnchorPlayer("ab", 3e3, plies=2, width=4)]
    res, finished = _arena(m, cfg, sides, 4, book, 3)
    assert finished == 2 * N_OPENINGS and res.score_a == 0.5
    rec = _records(res)
    assert all(rec[2 * t][2] == rec[2 * t + 1][2] for t in range(N_OPENINGS))  # both games of a pair are one game


# ---------------------------------------------------------------------------------------------- 6. (a network side)
SEED_NET = 0


def _slow_match(m, cfg, net, anchor, book, seed):
    """HashNet (A) against an anchor (B, an ab_ref mover) one game at a time: the network's plies through a one-game
    engine, the anchor's through the model on the same keyed noise row.  ({game id: (winner, length, moves)}, [threat,
    solver, alpha-beta] moves played)."""
    E = m["E"]
    S = cfg.BOARD_SIZE
    A = S * S
    e = E.BatchedSelfPlayEngine(cfg, num_games=1, net=net, seed=seed)
    boards, players, last, _ = book
    noise = torch.zeros(1, A, dtype=torch.float64, device="cuda")
    out, by = {}, [0, 0, 0]
    for t in range(boards.shape[0]):
        for first in (0, 1):
            b, p, lm = boards[t].reshape(A).copy(), int(players[t]), int(last[t])
            moves = []
            while True:
                row = _noise(m, A, t, len(moves), seed, noise)
                if (first + len(moves)) % 2:
                    a, which = AB.mover_move(b, p, cfg.N_IN_ROW, row, anchor)
                    by[which] += 1
                    assert a >= 0 and b[a] == 0
                    b[a] = p
                    s = p if R.wins(b.reshape(S, S), a, cfg.N_IN_ROW) else (2 if (b == 0).any() else 0)
                else:
                    e.set_positions(b.reshape(1, S, S), [p], [lm])
                    _, _, act = e.search(gumbel=noise)
                    st = e.play(reset_finished=False)
                    a, s = int(act.cpu()[0]), int(st.cpu()[0])
                    assert b[a] == 0
                    b[a] = p
                moves.append(a)
                p, lm = -p, a
                if s != 2:
                    break
            out[2 * t + first] = (s, len(moves), moves)
    e.close()
    return out, by


def test_ab_against_a_network_equals_the_slow_path(mods):
    m = mods
    E, AR = m["E"], m["AR"]
    cfg = m["Cfg"](BOARD_SIZE=6, NUM_SIMULATIONS=32, MCTS_IMPLEMENTATION="MuZero", NUM_RES_BLOCKS=2)
    book = AR.paired_openings(N_OPENINGS, 6, SEED_NET)
    anchor = AR.AnchorPlayer("ab", depth=6, nodes=256, plies=2, width=4)
    slow, by = _slow_match(m, cfg, E.HashNetBackend(E.hidden_slots(cfg, 1), 36), anchor.checked(), book, SEED_NET)
    print("slow path: %d threat, %d solver and %d alpha-beta moves in %d games" % (by[0], by[1], by[2], len(slow)))
    assert by[2] >= 10
    res, finished = _arena(m, cfg, [E.HashNetBackend(E.hidden_slots(cfg, 4), 36), anchor], 4, book, SEED_NET)
    assert finished == 2 * N_OPENINGS
    rec = _records(res)
    assert sorted(rec) == sorted(slow)
    for gid, w in slow.items():
        assert rec[gid] == w, gid


# ---------------------------------------------------------------------------------------------- 7.
def test_command_line_names_the_ab_anchor(mods, capsys):
    rc = mods["AR"].main(["--a", "anchor:ab", "--b", "anchor:threat", "--games", "4", "--board-size", "6",
                          "--anchor-plies", "2", "--anchor-width", "4", "--anchor-nodes", "128", "--anchor-scale", "0.5",
                          "--slots", "4"])
    out = json.loads(capsys.readouterr().out.strip())
    assert rc == 0 and out["a"] == "anchor:ab" and out["b"] == "anchor:threat" and out["games"] == 4
    for flag, bad, word in (("--anchor-plies", "0", "plies"), ("--anchor-width", "17", "width")):
        with pytest.raises(ValueError, match=word):
            mods["AR"].main(["--a", "anchor:ab", "--b", "anchor:threat", "--games", "2", "--board-size", "6", flag, bad,
                             "--slots", "2"])
