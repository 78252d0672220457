"""Arena, host side (no GPU): the three arena entry points refuse null or short arguments before any launch (fake
pointers, never dereferenced: the tests/test_conv_sizes.py pattern; no valid call is made with them), the Elo
difference and its pair interval against hand-computed values, the book of paired openings, and the book check."""
import ctypes
import math

import numpy as np
import pytest


def _lib():
    import datou_gomoku_muzero_amd._lib as L
    lib = L.load()
    return lib, ctypes.c_void_p(1 << 20), (lambda: lib.gmz_last_error().decode())


def test_set_active_and_gumbel_keyed_refuse_bad_arguments():
    lib, fake, err = _lib()
    assert lib.gmz_engine_set_active(None, fake, None) < 0
    assert "null engine" in err()
    assert lib.gmz_engine_set_simulations(None, 16) < 0
    assert "null engine" in err()
    G, A = 4, 36
    full = G * A * 8
    assert lib.gmz_gumbel_keyed(None, fake, 1, G, A, fake, full, None) < 0
    assert lib.gmz_gumbel_keyed(fake, None, 1, G, A, fake, full, None) < 0
    assert lib.gmz_gumbel_keyed(fake, fake, 1, G, A, None, full, None) < 0
    assert "null" in err()
    assert lib.gmz_gumbel_keyed(fake, fake, 1, 0, A, fake, full, None) < 0
    assert lib.gmz_gumbel_keyed(fake, fake, 1, G, 0, fake, full, None) < 0
    assert lib.gmz_gumbel_keyed(fake, fake, 1, G, 513, fake, 1 << 30, None) < 0
    assert lib.gmz_gumbel_keyed(fake, fake, 1, G, A, fake, full - 1, None) < 0
    assert str(full) in err(), err()


def _refill_args(fake, **kw):
    """A well-formed gmz_engine_play_refill argument list over fake pointers (8 slots, 6 openings, 6x6 moves), with
    single arguments replaced."""
    names = ["e", "action", "status", "book_boards", "book_players", "book_last", "book_counts", "n_openings", "tickets",
             "next_net", "slot_game", "slot_key", "slot_ply", "n_legal", "slot_capacity", "res_winner", "res_length",
             "res_moves", "moves_stride", "res_capacity", "finished", "stream"]
    vals = dict.fromkeys(names, fake)
    vals.update(n_openings=6, next_net=0, slot_capacity=8, moves_stride=36, res_capacity=12, stream=None)
    assert set(kw) <= set(names)
    vals.update(kw)
    return [vals[k] for k in names]


def test_play_refill_refuses_bad_arguments_before_touching_the_engine():
    lib, fake, err = _lib()
    for name in ("e", "action", "status", "book_boards", "book_players", "book_last", "book_counts", "tickets",
                 "slot_game", "slot_key", "slot_ply", "n_legal", "res_winner", "res_length", "finished"):
        assert lib.gmz_engine_play_refill(*_refill_args(fake, **{name: None})) < 0, name
        assert "null" in err(), (name, err())
    assert lib.gmz_engine_play_refill(*_refill_args(fake, n_openings=0)) < 0
    assert "n_openings" in err()
    assert lib.gmz_engine_play_refill(*_refill_args(fake, next_net=2)) < 0
    assert "next_net" in err()
    assert lib.gmz_engine_play_refill(*_refill_args(fake, res_capacity=11)) < 0  # 12 games
    assert "11" in err() and "12" in err(), err()
    assert lib.gmz_engine_play_refill(*_refill_args(fake, slot_capacity=0)) < 0
    assert "slot_capacity" in err()
    assert lib.gmz_engine_play_refill(*_refill_args(fake, moves_stride=0)) < 0
    assert "moves_stride" in err()


# ---------------------------------------------------------------------------------------------- Elo
@pytest.fixture(scope="module")
def AR():
    import datou_gomoku_muzero_amd.arena as AR
    return AR


def test_elo_from_score(AR):
    assert AR.elo_from_score(0.5) == 0.0
    assert AR.elo_from_score(0.75) == pytest.approx(400.0 * math.log10(3.0), abs=1e-9)  # 190.848...
    assert AR.elo_from_score(0.75) == pytest.approx(190.8485, abs=1e-4)
    assert AR.elo_from_score(0.25) == pytest.approx(-190.8485, abs=1e-4)
    assert AR.elo_from_score(10.0 / 11.0) == pytest.approx(400.0, abs=1e-9)
    assert AR.elo_from_score(0.0) == -math.inf and AR.elo_from_score(1.0) == math.inf


def test_pair_interval_by_hand(AR):
    # pairs 0.5, 0.5, 1, 0: mean 0.5, sum of squares 0.5, s = sqrt(0.5 / 3), half width 1.95996 * s / 2
    h = 1.959963984540054 * math.sqrt(0.5 / 3.0) / 2.0
    assert h == pytest.approx(0.400076, abs=1e-6)
    elo, lo, hi = AR.elo_interval([0.5, 0.5, 1.0, 0.0])
    assert elo == 0.0
    assert hi == pytest.approx(400.0 * math.log10((0.5 + h) / (0.5 - h)), abs=1e-9)
    assert hi == pytest.approx(381.84, abs=0.01) and lo == pytest.approx(-hi, abs=1e-9)
    # score 0.5 with no spread: a zero-width interval at 0
    assert AR.elo_interval([0.5, 0.5, 0.5]) == (0.0, 0.0, 0.0)
    # scores 1 and 0: infinities, no exception; one pair: no interval
    assert AR.elo_interval([1.0, 1.0, 1.0]) == (math.inf, math.inf, math.inf)
    assert AR.elo_interval([0.0, 0.0]) == (-math.inf, -math.inf, -math.inf)
    assert AR.elo_interval([0.75]) == (pytest.approx(190.8485, abs=1e-4), -math.inf, math.inf)
    # the upper end clipped at score 1
    elo, lo, hi = AR.elo_interval([1.0, 1.0, 0.5])
    assert hi == math.inf and math.isfinite(lo) and elo == pytest.approx(400.0 * math.log10(5.0), abs=1e-9)


def test_pair_interval_is_wider_than_the_naive_one_for_correlated_pairs(AR):
    """Openings that decide the game: A wins both games of one opening and loses both of the next.  Over pairs
    s = sqrt(6 * 0.25 / 5), half width 1.96 s / sqrt(6) = 0.438; over the 12 games taken as independent
    s = sqrt(12 * 0.25 / 11), half width 1.96 s / sqrt(12) = 0.295."""
    pairs = [1.0, 0.0] * 3
    games = [1.0, 1.0, 0.0, 0.0] * 3
    _, plo, phi = AR.score_interval(pairs)
    _, nlo, nhi = AR.score_interval(games)
    assert phi - plo == pytest.approx(2 * 1.959963984540054 * math.sqrt(0.3) / math.sqrt(6.0), abs=1e-12)
    assert nhi - nlo == pytest.approx(2 * 1.959963984540054 * math.sqrt(3.0 / 11.0) / math.sqrt(12.0), abs=1e-12)
    assert phi - plo > 1.4 * (nhi - nlo)
    e = AR.elo_interval(pairs)
    n = AR.naive_elo_interval(games)
    assert e[0] == n[0] == 0.0 and e[2] - e[1] > n[2] - n[1]
    # the other way round (every opening split 1-1): the pair interval has no width, the naive one has
    assert AR.elo_interval([0.5] * 6)[1:] == (0.0, 0.0) and AR.naive_elo_interval([1.0, 0.0] * 6)[2] > 100.0


def test_summarise_counts_by_network_and_colour(AR):
    # two openings, black to move in both; game id = 2 * opening + first mover (0 = A)
    #   id 0: A black, black wins -> A;  id 1: B black, black wins -> B;  id 2: A black, draw;  id 3: B black, white -> A
    res = AR.summarise(np.array([1, 1, 0, -1], np.int8), np.array([9, 9, 30, 12]), np.array([1, 1], np.int8),
                       np.arange(4 * 36).reshape(4, 36))
    t = res.tally
    assert t["a"]["black"] == dict(wins=1, draws=1, losses=0) and t["a"]["white"] == dict(wins=1, draws=0, losses=1)
    assert t["b"]["black"] == dict(wins=1, draws=0, losses=1) and t["b"]["white"] == dict(wins=0, draws=1, losses=1)
    assert res.pair_scores == [0.5, 0.75] and res.score_a == 0.625
    assert [g.winner for g in res.games] == ["a", "b", "draw", "a"]
    assert [g.first_mover for g in res.games] == ["a", "b", "a", "b"] and [g.opening for g in res.games] == [0, 0, 1, 1]
    assert res.games[3].moves == list(range(108, 120)) and res.games[3].length == 12
    with pytest.raises(RuntimeError):
        AR.summarise(np.array([1, 2], np.int8), np.array([9, 0]), np.array([1], np.int8))


# ---------------------------------------------------------------------------------------------- book
def test_paired_openings_are_deterministic_line_free_and_leave_room(AR):
    import datou_gomoku_muzero_amd.engine as E
    from datou_gomoku_muzero_amd.config import GmzConfig
    a = AR.paired_openings(9, 6, seed=3)
    b = AR.paired_openings(9, 6, seed=3)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert not np.array_equal(a[0], AR.paired_openings(9, 6, seed=4)[0])
    boards, players, last, counts = a
    assert boards.shape == (9, 6, 6) and boards.dtype == np.int8
    assert counts.tolist() == [2, 4, 6] * 3
    cfg = GmzConfig(BOARD_SIZE=6)
    for i in range(9):
        assert (boards[i] == 1).sum() == (boards[i] == -1).sum() == counts[i] // 2
        assert not E._has_five(boards[i], 5)
        assert players[i] == 1 and boards[i].flat[last[i]] == -1  # white placed the last stone
        assert 36 - counts[i] >= cfg.NUM_TOP_ACTIONS
    AR.check_book(a, cfg)
    odd = AR.paired_openings(2, 6, seed=0, stones=(3,))
    assert odd[1].tolist() == [-1, -1] and odd[3].tolist() == [3, 3]


def test_arena_rejects_a_book_that_leaves_fewer_cells_than_top_actions(AR):
    from datou_gomoku_muzero_amd.config import GmzConfig
    cfg = GmzConfig(BOARD_SIZE=6, NUM_SIMULATIONS=16)
    ok = AR.paired_openings(2, 6, seed=1, stones=(20,))  # 16 cells left: allowed
    AR.check_book(ok, cfg)
    bad = AR.paired_openings(2, 6, seed=1, stones=(4, 22))  # opening 1 leaves 14 < 16
    with pytest.raises(ValueError, match="NUM_TOP_ACTIONS"):
        AR.Arena(cfg, None, None, 4, bad)
    boards, players, last, counts = AR.paired_openings(2, 6, seed=1)
    with pytest.raises(ValueError, match="stone count"):
        AR.Arena(cfg, None, None, 4, (boards, players, last, counts + 1))


def _checkpoints(tmp_path, seeds=(1, 2)):
    """Two 6x6 two-block networks' weights: one in a torch.save file, one as a RecordStore trainer checkpoint."""
    import torch
    import datou_gomoku_muzero_amd.formats as F
    import datou_gomoku_muzero_amd.weights as W
    from datou_gomoku_muzero_amd.config import GmzConfig
    cfg = GmzConfig(BOARD_SIZE=6, NUM_RES_BLOCKS=2)
    sds = [{k: torch.as_tensor(np.asarray(v)) for k, v in
            W.synthetic_state_dict(cfg, seed=s, with_projection=False).items()} for s in seeds]
    pa, pb = str(tmp_path / "a.pt"), str(tmp_path / "b.db")
    torch.save(sds[0], pa)
    st = F.RecordStore(pb)
    st.save_trainer_state({"model_state_dict": sds[1], "train_step_count": 7})
    st.close()
    return pa, pb, sds


def test_load_checkpoint_reads_a_state_dict_file_and_a_record_store(AR, tmp_path):
    import torch
    pa, pb, sds = _checkpoints(tmp_path)
    for path, want in ((pa, sds[0]), (pb, sds[1])):
        got = AR.load_checkpoint(path)
        assert sorted(got) == sorted(want) and all(torch.equal(got[k], want[k]) for k in want)
        assert AR.blocks_of(got) == 2
    empty = str(tmp_path / "empty.db")
    import datou_gomoku_muzero_amd.formats as F
    F.RecordStore(empty).close()
    with pytest.raises(ValueError, match="no trainer checkpoint"):
        AR.load_checkpoint(empty)
