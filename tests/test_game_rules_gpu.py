"""The rule kernels (check_win_dev and play_one of csrc/gmz_device.h) against the plain model of tests/game_ref.py on
its directed positions: every board size from the smallest to the largest the kernels take, n_in_row 3..6, runs along
each direction into each border and corner, overlines, interrupted runs, runs that are contiguous in flat index only,
draws, wins on the last empty cell, both colours, and rows without a move.  Three entry points, everything bit for
bit: gmz_game_check_win at every cell, gmz_game_play, and the engine's own play (k_play_engine) with and without the
restart of finished games.  tests/test_game_ref.py pins the model and the positions on the CPU."""
import numpy as np
import pytest

import game_ref as GR

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import datou_gomoku_muzero_amd._lib as L
    import datou_gomoku_muzero_amd.engine as E
    return dict(L=L, E=E, lib=L.load())


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _same(got, want, tags, what):
    got = got.cpu().numpy().reshape(np.shape(want))
    bad = np.flatnonzero((got != want).reshape(len(want), -1).any(axis=1))
    assert not len(bad), "%s differs in %d positions, first: #%d (%s)" % (what, len(bad), bad[0], tags[bad[0]])


@pytest.mark.parametrize("size,n", GR.PAIRS)
def test_check_win_at_every_cell(mods, size, n):
    """gmz_game_check_win at every cell of every position after its move, and -1 (no move) giving 0."""
    L, lib = mods["L"], mods["lib"]
    A = size * size
    c, after, want = GR.cases(size, n), GR.played(size, n, False), GR.win_maps(size, n)
    G = len(c["actions"])
    boards = _dev(after["boards"])
    out = torch.full((G, A), 7, dtype=torch.uint8, device="cuda")
    one = torch.empty(G, dtype=torch.uint8, device="cuda")
    for a in range(A):  # move a on every board: G threads per launch, the boards read in place
        moves = torch.full((G,), a, dtype=torch.int32, device="cuda")
        L.check(lib.gmz_game_check_win(L.ptr(boards), G, size, n, L.ptr(moves), L.ptr(one), L.stream_ptr()))
        out[:, a] = one
    _same(out, want, c["tags"], "check_win")
    moves = _dev(c["actions"])  # the move itself, -1 included
    L.check(lib.gmz_game_check_win(L.ptr(boards), G, size, n, L.ptr(moves), L.ptr(one), L.stream_ptr()))
    st = after["status"]
    _same(one, (np.abs(st) == 1).astype(np.uint8), c["tags"], "check_win at the move")


@pytest.mark.parametrize("size,n", GR.PAIRS)
def test_game_play(mods, size, n):
    """gmz_game_play: status, board, player, last move and move count after the move (it never restarts a game)."""
    L, lib = mods["L"], mods["lib"]
    c, want = GR.cases(size, n), GR.played(size, n, False)
    G = len(c["actions"])
    b, pl, lm, mc, act = (_dev(c[k]) for k in ("boards", "players", "last", "counts", "actions"))
    st = torch.full((G,), 9, dtype=torch.int8, device="cuda")
    L.check(lib.gmz_game_play(L.ptr(b), G, size, n, L.ptr(pl), L.ptr(lm), L.ptr(mc), L.ptr(act), L.ptr(st),
                              L.stream_ptr()))
    torch.cuda.synchronize()
    for got, key in ((st, "status"), (b, "boards"), (pl, "players"), (lm, "last"), (mc, "counts")):
        _same(got, want[key], c["tags"], key)


@pytest.mark.parametrize("size,n", GR.PAIRS)
def test_engine_play(mods, size, n):
    """k_play_engine through set_positions + play(action=...) + game_state(), once leaving finished games as they
    ended and once restarting them (empty board, player 1, no last move, count 0); a row without a move reports 3
    and keeps its state either way."""
    c = GR.cases(size, n)
    G = len(c["actions"])
    eng = mods["E"].BatchedSelfPlayEngine(None, num_games=G, BOARD_SIZE=size, N_IN_ROW=n, NUM_SIMULATIONS=2)
    for reset in (False, True):
        want = GR.played(size, n, reset)
        eng.set_positions(*(np.array(c[k]) for k in ("boards", "players", "last", "counts")))
        st = eng.play(action=np.array(c["actions"]), reset_finished=reset)
        b, pl, lm, mc = eng.game_state()
        torch.cuda.synchronize()
        for got, key in ((st, "status"), (b, "boards"), (pl, "players"), (lm, "last"), (mc, "counts")):
            _same(got, want[key], c["tags"], "%s (reset_finished=%s)" % (key, reset))
    # the restarted games are there: something finished, something went on, something was left alone
    assert {2, 3} < set(want["status"].tolist()) and (want["counts"][np.abs(want["status"]) < 2] == 0).all()
    assert eng.errors() == 0
    eng.close()


@pytest.mark.parametrize("size", [5, 22])
def test_observation_planes(mods, size):
    """gmz_game_board_state and k_begin_move's planes on positions with and without a last move, G = 7 (not a
    multiple of the four games a k_begin_move workgroup takes)."""
    L, lib, n, G = mods["L"], mods["lib"], 5, 7
    A = size * size
    c = GR.cases(size, n)
    pick = [g for g in range(len(c["actions"])) if c["tags"][g].startswith("cut")][:5]  # stones of both colours
    pick += [g for g in range(len(c["actions"])) if c["last"][g] < 0][:2]
    assert len(pick) == G and (c["last"][pick] >= 0).any() and (c["last"][pick] < 0).any()
    boards, players, last = c["boards"][pick], c["players"][pick], c["last"][pick]
    assert (boards == 1).any() and (boards == -1).any() and set(players.tolist()) == {1, -1}
    want = np.stack([GR.board_state(boards[g], size, int(players[g]), int(last[g])) for g in range(G)])
    obs = torch.full((G, 3, size, size), 7.0, dtype=torch.float32, device="cuda")
    b, pl, lm = _dev(boards), _dev(players), _dev(last)
    L.check(lib.gmz_game_board_state(L.ptr(b), G, size, L.ptr(pl), L.ptr(lm), L.ptr(obs), L.stream_ptr()))
    torch.cuda.synchronize()
    assert np.array_equal(obs.cpu().numpy(), want)
    eng = mods["E"].BatchedSelfPlayEngine(None, num_games=G, BOARD_SIZE=size, N_IN_ROW=n, NUM_SIMULATIONS=2)
    eng.set_positions(np.array(boards), np.array(players), np.array(last))
    eng.obs.fill_(7.0)
    L.check(lib.gmz_engine_begin_move(eng.handle, None, eng.seed, L.ptr(eng.obs), L.stream_ptr()))
    torch.cuda.synchronize()
    assert np.array_equal(eng.obs.cpu().numpy(), want)
    assert eng.errors() == 0
    eng.close()
