"""Anchor opponents on the GPU (gmz_game_anchor_move, engine.anchor_move, arena.AnchorPlayer).  Every comparison is
exact: the kernel's scores are integers, its keys the model's IEEE doubles (tests/anchor_ref.py).

  1. kernel against model: scores and moves in guarded buffers, 5x5 to 22x22, n = 3 and 5, 1 / 7 / 64 boards, empty
     to nearly full boards, with and without noise, with a game array that leaves boards out; the hand-made positions;
  2. an arena match of a network against an anchor equals, move for move, the same games played one at a time: the
     network's plies through a one-game engine, the anchor's through the model on the same keyed noise row;
  3. the set of game records does not depend on the slot count or on streams=2;
  4. threat against threat, and a network against itself around an anchor match on the same engines: the two games
     of every opening are identical;
  5. anchors only: the match equals the model played on the host; accounting;
  6. a GomokuNetHip against the threat anchor; 7. the command line.

6x6 boards for the matches, at most 32 simulations and 8 slots."""
import numpy as np
import pytest

import anchor_ref as R
import test_anchor as TA

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SIZE, A, N_OPENINGS = 6, 36, 6
# the match seeds: chosen so that the slow path alone meets the conditions of test 2 (see _condition; of the seeds
# 0..5 MuZero / uniform misses them at 2 and AlphaZero / uniform at 5, where no game is drawn)
SEEDS = {("MuZero", "uniform"): 0, ("AlphaZero", "uniform"): 0, ("MuZero", "threat"): 0, ("AlphaZero", "threat"): 0}
SEED_HIP = 0


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import datou_gomoku_muzero_amd._lib as L
    import datou_gomoku_muzero_amd.arena as AR
    import datou_gomoku_muzero_amd.engine as E
    import datou_gomoku_muzero_amd.network as N
    import datou_gomoku_muzero_amd.weights as W
    from datou_gomoku_muzero_amd.config import GmzConfig
    return dict(L=L, AR=AR, E=E, N=N, W=W, Cfg=GmzConfig, lib=L.load())


# ---------------------------------------------------------------------------------------------- 1. kernel against model
FILLS = (0.0, 0.1, 0.5, 0.9)


def random_boards(S, G, rs):
    """(boards int8 [G,S,S], players int8 [G], random [G] bool): board g is filled to FILLS[k] for k = (g + G) % 5 < 4
    with stones of both colours on random cells (lines allowed: the rule does not care), and has one empty cell for
    k = 4 (random = False)."""
    boards = np.zeros((G, S * S), np.int8)
    rnd = np.ones(G, bool)
    for g in range(G):
        k = (g + G) % 5
        if k == 4:
            boards[g] = rs.choice(np.array([1, -1], np.int8), S * S)
            boards[g, rs.randint(S * S)] = 0
            rnd[g] = False
        else:
            cells = rs.permutation(S * S)[:int(round(FILLS[k] * S * S))]
            boards[g, cells] = rs.choice(np.array([1, -1], np.int8), cells.size)
    return boards.reshape(G, S, S), rs.choice(np.array([1, -1], np.int8), G), rnd


def noise_cases(G, AA, rs):
    """[(name, noise f64 [G,AA] or None, kind, scale)]"""
    gum = rs.gumbel(0, 1, (G, AA))
    coarse = rs.randint(0, 3, (G, AA)).astype(np.float64)  # equal values in every row: the index decides
    return [("null noise", None, R.THREAT, 0.0), ("noise breaks ties", gum, R.THREAT, 0.0),
            ("uniform", gum, R.UNIFORM, 1.0), ("threat with half noise", gum, R.THREAT, 0.5),
            ("equal noise, uniform", coarse, R.UNIFORM, 1.0), ("equal noise, threat", coarse, R.THREAT, 0.0)]


def model_moves(sc, noise, kind, scale):
    """The model's moves from the threat scores sc [G, AA] (kind 1: zeros on the empty cells)."""
    out = np.empty(sc.shape[0], np.int32)
    for g in range(sc.shape[0]):
        s = sc[g] if kind == R.THREAT else np.where(sc[g] >= 0, 0, -1)
        out[g] = R.choose(s, None if noise is None else noise[g], scale)
    return out


def run_kernel(m, boards, players, n, noise, kind, scale, game=None, want_scores=True):
    """gmz_game_anchor_move into guarded buffers: (actions int32 [G], scores int64 [G, AA] or None)."""
    from kernel_guards import Buf
    L, lib = m["L"], m["lib"]
    G, S = boards.shape[0], boards.shape[-1]
    b = torch.from_numpy(np.ascontiguousarray(boards)).cuda()
    p = torch.from_numpy(np.ascontiguousarray(players)).cuda()
    nz = None if noise is None else torch.from_numpy(np.ascontiguousarray(noise)).cuda()
    gm = None if game is None else torch.from_numpy(np.ascontiguousarray(game, dtype=np.int32)).cuda()
    act = Buf(G, torch.int32, off=1, fill=-7)
    sc = Buf(G * S * S, torch.int64, off=1, fill=-7) if want_scores else None
    L.check(lib.gmz_game_anchor_move(L.ptr(b), L.ptr(p), L.ptr(gm), L.ptr(nz), L.nbytes(nz), G, S, n, kind, scale,
                                     L.ptr(act.t), L.nbytes(act.t), L.ptr(sc.t) if sc else None,
                                     L.nbytes(sc.t) if sc else 0, L.stream_ptr()))
    torch.cuda.synchronize()
    assert act.intact() and (sc is None or sc.intact())
    return act.t.cpu().numpy(), (sc.t.cpu().numpy().reshape(G, S * S) if sc else None)


@pytest.mark.parametrize("n", [3, 5])
@pytest.mark.parametrize("S", [5, 6, 15, 19, 22])
def test_kernel_equals_the_model(mods, S, n):
    m = mods
    AA = S * S
    rs = np.random.RandomState(1000 * S + n)
    ties = differs = random_cases = 0
    for G in (1, 7, 64):
        boards, players, rnd = random_boards(S, G, rs)
        want_sc = np.stack([R.scores(boards[g], int(players[g]), n) for g in range(G)])
        assert np.array_equal(want_sc >= 0, boards.reshape(G, AA) == 0)
        lowest = np.array([np.flatnonzero(boards[g].reshape(-1) == 0)[0] for g in range(G)])
        game = None
        if G > 1:  # leave some boards out: slot numbers with holes, as play_refill keeps them
            game = np.arange(G, dtype=np.int32)
            game[rs.permutation(G)[:G // 3]] = -1
        for name, noise, kind, scale in noise_cases(G, AA, rs):
            want = model_moves(want_sc, noise, kind, scale)
            if name == "noise breaks ties":
                top = (want_sc == want_sc.max(axis=1, keepdims=True)).sum(axis=1)
                ties += int((top[rnd] > 1).sum())
            random_cases += int(rnd.sum())
            differs += int((want[rnd] != lowest[rnd]).sum())
            got, got_sc = run_kernel(m, boards, players, n, noise, kind, scale)
            wsc = want_sc if kind == R.THREAT else np.where(want_sc >= 0, 0, -1)
            assert np.array_equal(got_sc, wsc), (name, G)
            assert np.array_equal(got, want), (name, G, np.flatnonzero(got != want))
            if game is not None:
                got, got_sc = run_kernel(m, boards, players, n, noise, kind, scale, game)
                out = game < 0
                assert (got[out] == -1).all() and (got_sc[out] == -1).all() and out.any(), (name, G)
                assert np.array_equal(got[~out], want[~out]) and np.array_equal(got_sc[~out], wsc[~out]), (name, G)
        got, none = run_kernel(m, boards, players, n, None, R.THREAT, 0.0, want_scores=False)  # no scores asked for
        assert none is None and np.array_equal(got, model_moves(want_sc, None, R.THREAT, 0.0))
    # conditions on the model alone: noise did break ties, and the moves are not the first empty cell (a kernel
    # that ignored the scores and the noise could not pass)
    print("S %d n %d: %d random cases, %d differ from the lowest empty cell, %d boards with tied top scores" %
          (S, n, random_cases, differs, ties))
    assert ties > 0
    assert 2 * differs >= random_cases


def test_kernel_on_the_hand_made_positions(mods):
    m = mods
    cases = TA.hand_made()
    boards = np.stack([c[1] for c in cases])
    players = np.array([c[2] for c in cases], np.int8)
    want = np.array([c[3] for c in cases], np.int32)
    got, got_sc = run_kernel(m, boards, players, 5, None, R.THREAT, 0.0)
    assert np.array_equal(got, want)
    for g in range(len(cases)):
        assert np.array_equal(got_sc[g], R.scores(boards[g], int(players[g]), 5)), cases[g][0]
    for S in (5, 6, 15, 19, 22):  # the empty board
        got, _ = run_kernel(m, np.zeros((1, S, S), np.int8), np.ones(1, np.int8), 5, None, R.THREAT, 0.0)
        assert got.tolist() == [TA.centre(S)]


def test_engine_wrapper(mods):
    """engine.anchor_move (the module-level call) returns what the entry point writes, names the kinds, and refuses
    an unknown one."""
    m = mods
    rs = np.random.RandomState(3)
    boards, players, _ = random_boards(9, 7, rs)
    noise = rs.gumbel(0, 1, (7, 81))
    b, p = torch.from_numpy(boards).cuda(), torch.from_numpy(players).cuda()
    for kind, k, scale in (("threat", R.THREAT, 0.0), ("uniform", R.UNIFORM, 1.0), ("threat", R.THREAT, 0.5)):
        want, want_sc = run_kernel(m, boards, players, 5, noise, k, scale)
        act, sc = m["E"].anchor_move(b, p, torch.from_numpy(noise).cuda(), kind, scale, scores=True)
        assert np.array_equal(act.cpu().numpy(), want) and np.array_equal(sc.cpu().numpy(), want_sc)
        assert np.array_equal(m["E"].anchor_move(b, p, noise, kind, scale).cpu().numpy(), want)
    with pytest.raises(ValueError):
        m["E"].anchor_move(b, p, kind="minimax")
    with pytest.raises(m["L"].GmzError, match="gmz_game_anchor_move: n_in_row"):
        m["E"].anchor_move(b, p, n_in_row=10)


# ---------------------------------------------------------------------------------------------- the slow path
def _cfg(m, mode="MuZero", sims=32):
    return m["Cfg"](BOARD_SIZE=SIZE, NUM_SIMULATIONS=sims, MCTS_IMPLEMENTATION=mode, NUM_RES_BLOCKS=2)


def _noise(m, key, ply, seed, out):
    L = m["L"]
    k = torch.tensor([key], dtype=torch.int32, device="cuda")
    p = torch.tensor([ply], dtype=torch.int32, device="cuda")
    L.check(m["lib"].gmz_gumbel_keyed(L.ptr(k), L.ptr(p), seed, 1, A, L.ptr(out), L.nbytes(out), L.stream_ptr()))
    return out


def _slow_match(m, cfg, sides, book, seed):
    """The match played one game at a time: a network side (a backend) moves through a one-game engine
    (set_positions, search(gumbel=...), play), an anchor side ((kind, scale)) through the numpy model on the same
    keyed noise row copied to the host.  {game id: (winner colour, length, moves, fewest legal cells a search saw)}."""
    E = m["E"]
    engines = [None if isinstance(s, tuple) else E.BatchedSelfPlayEngine(cfg, num_games=1, net=s, seed=seed)
               for s in sides]
    boards, players, last, counts = book
    noise = torch.zeros(1, A, dtype=torch.float64, device="cuda")
    out = {}
    for t in range(boards.shape[0]):
        for first in (0, 1):
            b, p, lm = boards[t].reshape(A).copy(), int(players[t]), int(last[t])
            moves, fewest = [], A
            while True:
                k = (first + len(moves)) % 2
                _noise(m, t, len(moves), seed, noise)
                if engines[k] is None:
                    kind, scale = sides[k]
                    _, a = R.move(b, p, cfg.N_IN_ROW, noise.cpu().numpy()[0],
                                  R.THREAT if kind == "threat" else R.UNIFORM, scale)
                    assert a >= 0 and b[a] == 0
                    b[a] = p
                    s = p if R.wins(b.reshape(SIZE, SIZE), a, cfg.N_IN_ROW) else (2 if (b == 0).any() else 0)
                else:
                    e = engines[k]
                    e.set_positions(b.reshape(1, SIZE, SIZE), [p], [lm])
                    fewest = min(fewest, int((b == 0).sum()))
                    _, _, act = e.search(gumbel=noise)
                    st = e.play(reset_finished=False)
                    a, s = int(act.cpu()[0]), int(st.cpu()[0])
                    assert b[a] == 0
                    b[a] = p
                moves.append(a)
                p, lm = -p, a
                if s != 2:
                    break
            out[2 * t + first] = (s, len(moves), moves, fewest)
    for e in engines:
        if e is not None:
            e.close()
    return out


def _condition(cfg, kind, slow, book):
    """Test 2's conditions on the slow path alone.  Against the uniform anchor: two games in which the network
    searched below NUM_TOP_ACTIONS legal cells, and a draw.  Against the threat anchor (side B): an anchor win as
    first mover and one as second mover."""
    if kind == "uniform":
        low = sum(1 for r in slow.values() if r[3] < cfg.NUM_TOP_ACTIONS)
        draws = sum(1 for r in slow.values() if r[0] == 0)
        return low >= 2 and draws >= 1, dict(low=low, draws=draws)
    wins = [0, 0]  # anchor wins by (it moved first, it moved second)
    for gid, r in slow.items():
        first = gid & 1  # 1: B, the anchor, moves first and plays the opening's side to move
        anchor_colour = int(book[1][gid >> 1]) * (1 if first else -1)
        if r[0] == anchor_colour:
            wins[0 if first else 1] += 1
    return wins[0] >= 1 and wins[1] >= 1, dict(anchor_wins_first=wins[0], anchor_wins_second=wins[1])


def _hash_net(m, cfg, slots):
    return m["E"].HashNetBackend(m["E"].hidden_slots(cfg, slots), A)


def _records(res):
    return {2 * g.opening + (g.first_mover == "b"): (g.winner_colour, g.length, g.moves) for g in res.games}


def _arena(m, cfg, sides, slots, book, seed, streams=1):
    ar = m["AR"].Arena(cfg, sides[0], sides[1], slots, book, seed=seed, record_moves=True, streams=streams)
    res = ar.run()
    finished = int(ar.match.finished.cpu()[0])
    ar.close()
    return res, finished


def _assert_equal_to_slow(slow, res):
    rec = _records(res)
    assert sorted(rec) == sorted(slow)
    for gid, (w, n, moves, _) in slow.items():
        assert rec[gid] == (w, n, moves), gid


_CACHE = {}


def _hash_case(m, mode, kind):
    """HashNet (side A) against an anchor (side B): the slow path once, and the arena on 8 slots."""
    key = (mode, kind)
    if key not in _CACHE:
        cfg = _cfg(m, mode, 32 if mode == "MuZero" else 24)
        seed = SEEDS[key]
        book = m["AR"].paired_openings(N_OPENINGS, SIZE, seed)
        anchor = m["AR"].AnchorPlayer(kind)
        slow = _slow_match(m, cfg, [_hash_net(m, cfg, 1), anchor.checked()], book, seed)
        res, finished = _arena(m, cfg, [_hash_net(m, cfg, 8), anchor], 8, book, seed)
        _CACHE[key] = (cfg, seed, book, slow, res, finished)
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------- 2.
@pytest.mark.parametrize("kind", ["uniform", "threat"])
@pytest.mark.parametrize("mode", ["MuZero", "AlphaZero"])
def test_arena_equals_the_slow_path(mods, mode, kind):
    cfg, seed, book, slow, res, finished = _hash_case(mods, mode, kind)
    ok, what = _condition(cfg, kind, slow, book)
    print(mode, kind, "slow path:", what)
    assert ok, what
    assert len(slow) == 2 * N_OPENINGS == finished
    _assert_equal_to_slow(slow, res)
    assert sum(g.length for g in res.games) == res.moves_played


def test_the_anchor_may_be_side_a(mods):
    """The sides swapped: the anchor as A gives the same games under the other ids (game id = 2 * opening + first
    mover, and the first mover's letter changes with the sides)."""
    m = mods
    cfg, seed, book, slow, _, _ = _hash_case(m, "MuZero", "threat")
    res, _ = _arena(m, cfg, [m["AR"].AnchorPlayer("threat"), _hash_net(m, cfg, 8)], 8, book, seed)
    rec = _records(res)
    for gid, (w, n, moves, _) in slow.items():
        assert rec[gid ^ 1] == (w, n, moves), gid


# ---------------------------------------------------------------------------------------------- 3.
@pytest.mark.parametrize("slots,streams", [(2, 1), (2, 2), (5, 1), (8, 2)])
def test_records_do_not_depend_on_the_slots(mods, slots, streams):
    m = mods
    cfg, seed, book, slow, res8, _ = _hash_case(m, "MuZero", "threat")
    sides = [_hash_net(m, cfg, slots), m["AR"].AnchorPlayer("threat")]
    res, finished = _arena(m, cfg, sides, slots, book, seed, streams)
    assert _records(res) == _records(res8) and finished == 2 * N_OPENINGS
    _assert_equal_to_slow(slow, res)
    assert sum(g.length for g in res.games) == res.moves_played


# ---------------------------------------------------------------------------------------------- 4.
def _assert_pairs_split(res):
    rec = _records(res)
    for t in range(N_OPENINGS):
        assert rec[2 * t] == rec[2 * t + 1], t  # same winner colour, length and moves
    assert res.pair_scores == [0.5] * N_OPENINGS and res.score_a == 0.5


@pytest.mark.parametrize("streams", [1, 2])
def test_copy_against_copy(mods, streams):
    """Threat against threat, then on ONE arena's engines: HashNet against itself, HashNet against the threat anchor,
    HashNet against itself again.  The two games of every opening are identical each time, and the anchor match in
    between leaves the engines as a fresh arena's (the third match equals the first)."""
    m = mods
    AR = m["AR"]
    cfg = _cfg(m)
    book = AR.paired_openings(N_OPENINGS, SIZE, 11)
    res, _ = _arena(m, cfg, [AR.AnchorPlayer("threat"), AR.AnchorPlayer("threat")], 8, book, 11, streams)
    _assert_pairs_split(res)
    assert res.elo == 0.0 and len({tuple(g.moves) for g in res.games}) > 1
    nets = [_hash_net(m, cfg, 8), _hash_net(m, cfg, 8)]
    ar = AR.Arena(cfg, nets[0], nets[1], 8, book, seed=11, record_moves=True, streams=streams)
    first = ar.run()
    _assert_pairs_split(first)
    ar.set_sides(nets[0], AR.AnchorPlayer("threat"))
    mixed = ar.run()
    ar.set_sides(nets[0], nets[1])
    again = ar.run()
    ar.close()
    _assert_pairs_split(again)
    assert _records(again) == _records(first) != _records(mixed)
    fresh, _ = _arena(m, cfg, [_hash_net(m, cfg, 8), AR.AnchorPlayer("threat")], 8, book, 11, streams)
    assert _records(mixed) == _records(fresh)


# ---------------------------------------------------------------------------------------------- 5.
@pytest.mark.parametrize("slots,streams", [(8, 1), (3, 1), (4, 2)])
def test_anchors_only_equals_the_model_on_the_host(mods, slots, streams):
    m = mods
    AR = m["AR"]
    cfg = _cfg(m)
    seed = 5
    book = AR.paired_openings(N_OPENINGS, SIZE, seed)
    sides = [AR.AnchorPlayer("threat"), AR.AnchorPlayer("uniform")]
    ar = AR.Arena(cfg, sides[0], sides[1], slots, book, seed=seed, record_moves=True, streams=streams)
    res = ar.run()
    assert int(ar.match.finished.cpu()[0]) == 2 * N_OPENINGS == ar.finished() == len(res.games)
    ar.close()
    assert res.moves_played == sum(g.length for g in res.games) > 0
    rec = _records(res)
    noise = torch.zeros(1, A, dtype=torch.float64, device="cuda")
    kinds = [(R.THREAT, 0.0), (R.UNIFORM, 1.0)]
    for t in range(N_OPENINGS):
        for first in (0, 1):
            w, moves = R.play_game(book[0][t].reshape(A), int(book[1][t]), [kinds[first], kinds[1 - first]],
                                   lambda ply: _noise(m, t, ply, seed, noise).cpu().numpy()[0], cfg.N_IN_ROW)
            assert rec[2 * t + first] == (w, len(moves), moves), (t, first)
    assert res.score_a > 0.5  # the threat player is the stronger anchor


# ---------------------------------------------------------------------------------------------- 6.
def test_a_hip_network_against_the_threat_anchor(mods):
    m = mods
    cfg = _cfg(m)

    def net(slots):
        cn = m["Cfg"](BOARD_SIZE=SIZE, NUM_SIMULATIONS=cfg.NUM_SIMULATIONS, NUM_RES_BLOCKS=2)
        sd = m["W"].synthetic_state_dict(cn, seed=1, with_projection=False)
        return m["N"].GomokuNetHip(sd, cn, num_slots=m["E"].hidden_slots(cfg, slots), max_rows=slots, precision="fp16")

    book = m["AR"].paired_openings(N_OPENINGS, SIZE, SEED_HIP)
    anchor = m["AR"].AnchorPlayer("threat")
    slow = _slow_match(m, cfg, [net(1), anchor.checked()], book, SEED_HIP)
    res, finished = _arena(m, cfg, [net(8), anchor], 8, book, SEED_HIP)
    assert finished == 2 * N_OPENINGS
    _assert_equal_to_slow(slow, res)


# ---------------------------------------------------------------------------------------------- 7.
def test_command_line_names_the_anchor(mods, tmp_path, capsys):
    import json
    import test_arena
    pa, _, _ = test_arena._checkpoints(tmp_path)
    rc = mods["AR"].main(["--a", pa, "--b", "anchor:threat", "--games", "6", "--board-size", "6", "--sims", "16",
                          "--slots", "4", "--seed", "2"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert rc == 0 and len(lines) == 1
    out = json.loads(lines[0])
    assert out["b"] == "anchor:threat" and out["a"] == "a.pt" and out["games"] == 6 and out["moves_played"] > 0
    for k in ("a", "b"):
        assert sum(sum(out["tally"][k][side].values()) for side in ("black", "white")) == 6
    rc = mods["AR"].main(["--a", "anchor:uniform", "--b", "anchor:threat", "--games", "4", "--board-size", "6",
                          "--anchor-scale", "0.5", "--slots", "4"])
    out = json.loads(capsys.readouterr().out.strip())
    assert rc == 0 and out["a"] == "anchor:uniform" and out["b"] == "anchor:threat" and out["games"] == 4
