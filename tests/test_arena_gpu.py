"""Arena on the GPU (arena.py, gmz_engine_set_active / gmz_engine_play_refill / gmz_gumbel_keyed).  Every comparison
is exact: the arena runs the self-play engine's kernels on the same rows.

  1. active mask: inactive games are not searched, the others are searched bit for bit as without a mask;
  2. an arena match equals, move for move, the same games played one at a time with the pre-existing interfaces
     (a one-game engine per network, set_positions, search(gumbel=...), play), including games that run below
     NUM_TOP_ACTIONS legal cells (the case that catches a wrong host mirror of the legal counts);
  3. the set of game records does not depend on the slot count or on streams=2;
  4. a network against a copy of itself: the two games of every opening are identical, score exactly 0.5;
  5. accounting; 6. networks of different precision and depth in one match.

6x6 boards, at most 32 simulations and 8 slots, 2-block networks (one 4-block) with seeded random weights."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SIZE, A, N_OPENINGS = 6, 36, 6
# the match seeds: chosen so that the slow path alone meets test 2's condition (see _condition)
SEED_HASH = {"MuZero": 0, "AlphaZero": 0}
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


def _cfg(m, mode="MuZero", sims=32):
    return m["Cfg"](BOARD_SIZE=SIZE, NUM_SIMULATIONS=sims, MCTS_IMPLEMENTATION=mode, NUM_RES_BLOCKS=2)


# ---------------------------------------------------------------------------------------------- 1. active mask
def _per_game_counters(m, eng):
    parts = getattr(eng, "engines", [eng])
    out = []
    for e in parts:
        c = torch.zeros(e.G, 4, dtype=torch.int32, device="cuda")
        m["L"].check(m["lib"].gmz_engine_tree_counters(e.handle, m["L"].ptr(c), 0, m["L"].stream_ptr()))
        out.append(c)
    torch.cuda.synchronize()
    return torch.cat(out).cpu().numpy()


def _make(m, kind, G, seed):
    E = m["E"]
    if kind == "az":
        return E.BatchedSelfPlayEngine(_cfg(m, "AlphaZero", 24), num_games=G, seed=seed)
    if kind == "split":
        return E.SplitSelfPlayEngine(_cfg(m), num_games=G, seed=seed, parts=2)
    return E.BatchedSelfPlayEngine(_cfg(m), num_games=G, seed=seed, layout=kind)


@pytest.mark.parametrize("kind", ["dense", "lists", "az", "split"])
def test_active_mask(mods, kind):
    m = mods
    G = 8
    off = np.array([1, 4, 6])
    mask = np.ones(G, np.uint8)
    mask[off] = 0
    on = np.flatnonzero(mask)
    rs = np.random.RandomState(5)
    boards = np.zeros((G, SIZE, SIZE), np.int8)
    players, last = np.ones(G, np.int8), np.full(G, -1, np.int32)
    for g in range(G):  # 3 g line-free stones: game 7 is searched with 15, 14, 13 legal cells (< NUM_TOP_ACTIONS)
        b, cells = m["E"]._place_stones(rs, A, SIZE, 3 * g, 5)
        boards[g] = b.reshape(SIZE, SIZE)
        players[g] = 1 if g % 2 == 0 else -1
        last[g] = cells[-1] if g else -1
    ref, eng = _make(m, kind, G, 3), _make(m, kind, G, 3)
    for e in (ref, eng):
        e.set_positions(boards, players, last)
    eng.set_active(mask)
    for move in range(3):
        gum = rs.gumbel(0, 1, (G, A))
        before = [t.clone() for t in eng.game_state()]
        c0r, c0e = _per_game_counters(m, ref), _per_game_counters(m, eng)
        out = []
        for e in (ref, eng):
            pol, val, act = e.search(gumbel=gum)
            vis = e.root_stats()[0]
            st = e.play(reset_finished=False)
            torch.cuda.synchronize()
            out.append([t.cpu().numpy().copy() for t in (pol, val, act, vis, st)])
        r, x = out
        for k in range(5):  # policy, value, action, root visit counts, status: bit-identical for the active games
            assert np.array_equal(r[k][on], x[k][on]), (kind, move, k)
        assert (x[2][off] == -1).all() and (x[4][off] == 3).all()
        assert (r[2][on] >= 0).all()
        after = eng.game_state()
        for t0, t1 in zip(before, after):  # board, player, last move, move count unchanged
            assert torch.equal(t0[off], t1[off])
        for t0, t1 in zip(ref.game_state(), after):
            assert torch.equal(t0[on], t1[on])
        dr, de = _per_game_counters(m, ref) - c0r, _per_game_counters(m, eng) - c0e
        assert np.array_equal(dr[on], de[on]) and (de[off] == 0).all() and (dr[off] > 0).any()
    tr, te = ref.tree_counters(), eng.tree_counters()
    share = _per_game_counters(m, ref)[off].sum(axis=0)
    for i, k in enumerate(("backups", "backup_levels", "selects", "select_levels")):
        assert te[k] == tr[k] - int(share[i]) and te[k] > 0
    eng.set_active(None)  # back to every game: nobody is skipped
    _, _, act = eng.search(gumbel=rs.gumbel(0, 1, (G, A)))
    assert (act.cpu().numpy() >= 0).all()
    ref.close()
    eng.close()


# ---------------------------------------------------------------------------------------------- the slow path
def _noise(m, key, ply, seed, out):
    L = m["L"]
    k = torch.tensor([key], dtype=torch.int32, device="cuda")
    p = torch.tensor([ply], dtype=torch.int32, device="cuda")
    L.check(m["lib"].gmz_gumbel_keyed(L.ptr(k), L.ptr(p), seed, 1, A, L.ptr(out), L.nbytes(out), L.stream_ptr()))
    return out


def _slow_match(m, cfg, nets, book, seed, cfgs=None):
    """The match played one game at a time with pre-existing interfaces only (and gmz_gumbel_keyed for the noise):
    {game id: (winner colour, length, moves, fewest legal cells a search saw)}.  ``cfgs``: a configuration per
    network's engine (default ``cfg`` for both)."""
    E = m["E"]
    engines = [E.BatchedSelfPlayEngine(c, num_games=1, net=n, seed=seed) for n, c in zip(nets, cfgs or (cfg, cfg))]
    boards, players, last, counts = book
    noise = torch.zeros(1, A, dtype=torch.float64, device="cuda")
    out = {}
    for t in range(boards.shape[0]):
        for first in (0, 1):
            b, p, lm = boards[t].reshape(A).copy(), int(players[t]), int(last[t])
            moves, fewest = [], A
            while True:
                e = engines[(first + len(moves)) % 2]
                e.set_positions(b.reshape(1, SIZE, SIZE), [p], [lm])
                fewest = min(fewest, int((b == 0).sum()))
                _, _, act = e.search(gumbel=_noise(m, t, len(moves), seed, noise))
                st = e.play(reset_finished=False)
                a, s = int(act.cpu()[0]), int(st.cpu()[0])
                assert b[a] == 0
                moves.append(a)
                b[a], p, lm = p, -p, a
                if s != 2:
                    break
            out[2 * t + first] = (s, len(moves), moves, fewest)
    for e in engines:
        e.close()
    return out


def _condition(cfg, slow):
    """Test 2's condition on the slow path alone: two games searched below NUM_TOP_ACTIONS legal cells, a win and a
    draw."""
    low = sum(1 for r in slow.values() if r[3] < cfg.NUM_TOP_ACTIONS)
    wins = sum(1 for r in slow.values() if r[0] != 0)
    draws = sum(1 for r in slow.values() if r[0] == 0)
    return low >= 2 and wins >= 1 and draws >= 1, dict(low=low, wins=wins, draws=draws)


def _hash_nets(m, cfg, slots):
    return [m["E"].HashNetBackend(m["E"].hidden_slots(cfg, slots), A) for _ in range(2)]


def _hip_nets(m, cfg, slots, specs):
    """specs: (weights seed, blocks, precision) per network."""
    nets = []
    for wseed, blocks, prec in specs:
        cn = m["Cfg"](BOARD_SIZE=SIZE, NUM_SIMULATIONS=cfg.NUM_SIMULATIONS, NUM_RES_BLOCKS=blocks)
        sd = m["W"].synthetic_state_dict(cn, seed=wseed, with_projection=False)
        nets.append(m["N"].GomokuNetHip(sd, cn, num_slots=m["E"].hidden_slots(cfg, slots), max_rows=slots,
                                        precision=prec))
    return nets


def _records(res):
    return {2 * g.opening + (g.first_mover == "b"): (g.winner_colour, g.length, g.moves) for g in res.games}


def _arena(m, cfg, nets, slots, book, seed, streams=1, sims=None):
    ar = m["AR"].Arena(cfg, nets[0], nets[1], slots, book, seed=seed, record_moves=True, streams=streams, sims=sims)
    res = ar.run()
    tickets = ar.match.tickets.cpu().tolist()
    ar.close()
    return res, tickets


_CACHE = {}


def _hash_case(m, mode):
    """The HashNet match of tests 2, 3 and 5: the slow path once, and the arena on 8 slots."""
    if mode not in _CACHE:
        cfg = _cfg(m, mode, 32 if mode == "MuZero" else 24)
        seed = SEED_HASH[mode]
        book = m["AR"].paired_openings(N_OPENINGS, SIZE, seed)
        slow = _slow_match(m, cfg, _hash_nets(m, cfg, 1), book, seed)
        res, tickets = _arena(m, cfg, _hash_nets(m, cfg, 8), 8, book, seed)
        _CACHE[mode] = (cfg, seed, book, slow, res, tickets)
    return _CACHE[mode]


def _assert_equal_to_slow(slow, res):
    rec = _records(res)
    assert sorted(rec) == sorted(slow)
    for gid, (w, n, moves, _) in slow.items():
        assert rec[gid] == (w, n, moves), gid


# ---------------------------------------------------------------------------------------------- 2.
@pytest.mark.parametrize("mode", ["MuZero", "AlphaZero"])
def test_arena_equals_the_slow_path_hashnet(mods, mode):
    cfg, seed, book, slow, res, _ = _hash_case(mods, mode)
    ok, what = _condition(cfg, slow)
    print(mode, "slow path:", what)
    assert ok, what
    assert len(slow) == 12
    _assert_equal_to_slow(slow, res)


def test_arena_equals_the_slow_path_two_hip_networks(mods):
    m = mods
    cfg = _cfg(m)
    book = m["AR"].paired_openings(N_OPENINGS, SIZE, SEED_HIP)
    specs = [(1, 2, "fp16"), (2, 2, "fp16")]
    slow = _slow_match(m, cfg, _hip_nets(m, cfg, 1, specs), book, SEED_HIP)
    ok, what = _condition(cfg, slow)
    print("HIP slow path:", what)
    assert ok, what
    res, _ = _arena(m, cfg, _hip_nets(m, cfg, 8, specs), 8, book, SEED_HIP)
    _assert_equal_to_slow(slow, res)


# ---------------------------------------------------------------------------------------------- 3.
@pytest.mark.parametrize("slots,streams", [(3, 1), (8, 2)])
def test_records_do_not_depend_on_the_slots(mods, slots, streams):
    m = mods
    cfg, seed, book, slow, res8, _ = _hash_case(m, "MuZero")
    res, tickets = _arena(m, cfg, _hash_nets(m, cfg, slots), slots, book, seed, streams)
    assert _records(res) == _records(res8)
    _assert_equal_to_slow(slow, res)
    assert min(tickets) >= N_OPENINGS


# ---------------------------------------------------------------------------------------------- 4.
@pytest.mark.parametrize("net", ["hash", "hip"])
def test_a_network_against_its_copy_splits_every_pair(mods, net):
    m = mods
    cfg = _cfg(m)
    book = m["AR"].paired_openings(N_OPENINGS, SIZE, 11)
    nets = _hash_nets(m, cfg, 8) if net == "hash" else _hip_nets(m, cfg, 8, [(4, 2, "fp16"), (4, 2, "fp16")])
    res, _ = _arena(m, cfg, nets, 8, book, 11)
    rec = _records(res)
    for t in range(N_OPENINGS):
        assert rec[2 * t] == rec[2 * t + 1], t  # same winner colour, length and moves
    assert res.pair_scores == [0.5] * N_OPENINGS and res.score_a == 0.5
    assert res.elo == 0.0 and res.elo_lo == 0.0 and res.elo_hi == 0.0
    for side in ("black", "white"):
        assert res.tally["a"][side] == res.tally["b"][side]


# ---------------------------------------------------------------------------------------------- 5.
def test_accounting(mods):
    cfg, seed, book, slow, res, tickets = _hash_case(mods, "MuZero")
    games = 2 * N_OPENINGS
    for k in ("a", "b"):
        n = {side: sum(res.tally[k][side].values()) for side in ("black", "white")}
        assert n["black"] + n["white"] == games
        # the book's openings all have black to move: each network is black in the games it starts
        assert n == dict(black=N_OPENINGS, white=N_OPENINGS)
        assert sum(1 for g in res.games if g.first_mover == k) == N_OPENINGS
    for side, other in (("black", "white"),):
        assert res.tally["a"][side]["wins"] == res.tally["b"][other]["losses"]
        assert res.tally["a"][side]["draws"] == res.tally["b"][other]["draws"]
    assert sum(g.length for g in res.games) == res.moves_played > 0
    # every opening drawn per first mover (slots that raced for the last ticket may leave the counters above n;
    # Arena.run has checked that exactly 2 n games finished, and each id below holds one result)
    assert min(tickets) >= N_OPENINGS
    assert sorted((g.opening, g.first_mover) for g in res.games) == sorted(
        (t, k) for t in range(N_OPENINGS) for k in ("a", "b"))
    for g in res.games:
        assert len(g.moves) == g.length and len(set(g.moves)) == g.length
        assert g.length + int(book[3][g.opening]) <= A


# ---------------------------------------------------------------------------------------------- 6.
@pytest.mark.parametrize("specs", [[(1, 2, "fp16"), (1, 2, "bf16")], [(1, 2, "fp16"), (3, 4, "fp16")]],
                         ids=["fp16-bf16", "2-4-blocks"])
def test_different_precisions_and_depths(mods, specs):
    m = mods
    cfg = _cfg(m, sims=16)
    book = m["AR"].paired_openings(2, SIZE, 7)
    slow = _slow_match(m, cfg, _hip_nets(m, cfg, 1, specs), book, 7)
    res, tickets = _arena(m, cfg, _hip_nets(m, cfg, 4, specs), 4, book, 7)
    assert len(res.games) == 4 and min(tickets) >= 2
    _assert_equal_to_slow(slow, res)


# ---------------------------------------------------------------------------------------------- 7.
@pytest.mark.parametrize("mode,streams", [("MuZero", 1), ("MuZero", 2), ("AlphaZero", 1)])
def test_a_simulation_budget_per_network(mods, mode, streams):
    """Network A searches with 32 simulations, B with 12: the match equals the slow path whose two one-game engines
    were BUILT with 32 and with 12 simulations (an engine built for 32 and set to 12 searches as one built for 12)."""
    m = mods
    big, small = _cfg(m, mode, 32), _cfg(m, mode, 12)
    book = m["AR"].paired_openings(3, SIZE, 5)
    slow = _slow_match(m, big, _hash_nets(m, big, 1), book, 5, cfgs=(big, small))
    assert any(slow[2 * t][2] != slow[2 * t + 1][2] for t in range(3))  # the budgets matter: some pair differs
    res, _ = _arena(m, small, _hash_nets(m, big, 4), 4, book, 5, streams, sims=(32, 12))
    _assert_equal_to_slow(slow, res)


def test_set_simulations_refuses_a_budget_the_pools_were_not_built_for(mods):
    m = mods
    eng = m["E"].BatchedSelfPlayEngine(_cfg(m, "MuZero", 16), num_games=2, seed=1)
    for n in (0, -3, 17):
        with pytest.raises(m["L"].GmzError, match="num_simulations"):
            eng.set_simulations(n)
    eng.set_simulations(16)
    eng.set_simulations(8)
    eng.reset_games()
    eng.search()
    assert eng.waves_last == eng.waves_needed() > 0
    eng.close()


# ---------------------------------------------------------------------------------------------- command line
def test_command_line_prints_one_json_line(mods, tmp_path, capsys):
    """fp16 against bf16 with 16 against 8 simulations, from a torch.save file and a RecordStore checkpoint."""
    import json
    import test_arena as TA
    pa, pb, _ = TA._checkpoints(tmp_path)
    rc = mods["AR"].main(["--a", pa, "--b", pb, "--games", "6", "--board-size", "6", "--sims-a", "16", "--sims-b", "8",
                          "--precision-b", "bf16", "--slots", "4", "--seed", "2"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert rc == 0 and len(lines) == 1
    out = json.loads(lines[0])
    assert out["games"] == 6 and out["sims_a"] == 16 and out["sims_b"] == 8 and out["precision_b"] == "bf16"
    assert 0.0 <= out["score_a"] <= 1.0 and out["moves_played"] > 0
    for k in ("a", "b"):
        assert sum(sum(out["tally"][k][side].values()) for side in ("black", "white")) == 6
