"""Self-play's opening book on the host (openings.book_draw, transform_opening, check_selfplay_book) against the
model of tests/book_ref.py, and gmz_engine_play_book's first refusal.  No GPU."""
import ctypes

import numpy as np
import pytest

import book_ref
import noise_ref

SEEDS = (0x9E3779B97F4A7C15, (5 << 32) | 7, 0xFFFFFFFF00000001, 12345)  # the first three: a non-zero high word
NS = (1, 2, 7, 1000, 1 << 20)
KEYS = np.arange(71).reshape(-1, 1)
SERIALS = np.arange(41).reshape(1, -1)


def _cfg(size=9, n_in_row=5, **kw):
    from datou_gomoku_muzero_amd.config import GmzConfig
    return GmzConfig(BOARD_SIZE=size, N_IN_ROW=n_in_row, **kw)


@pytest.mark.parametrize("n", NS)
def test_book_draw_equals_the_model(n):
    from datou_gomoku_muzero_amd import openings as O
    for seed in SEEDS:
        t, d = O.book_draw(seed, KEYS, SERIALS, n, True)
        mt, md = book_ref.draw(seed, KEYS, SERIALS, n, True)
        assert t.shape == (71, 41) and np.array_equal(t, mt) and np.array_equal(d, md)
        assert t.min() >= 0 and t.max() < n and d.min() >= 0 and d.max() <= 7
        t0, d0 = O.book_draw(seed, KEYS, SERIALS, n, False)
        assert np.array_equal(t0, t) and not d0.any()
    if n >= 7:  # the draw spreads: every symmetry and more than one opening appear
        assert len(np.unique(d)) == 8 and len(np.unique(t)) > 1


def test_draw_depends_on_seed_halves_key_and_serial():
    from datou_gomoku_muzero_amd import openings as O
    base = O.book_draw(SEEDS[1], KEYS, SERIALS, 1000)[0]
    assert not np.array_equal(base, O.book_draw(SEEDS[1] + 1, KEYS, SERIALS, 1000)[0])  # the low word
    assert not np.array_equal(base, O.book_draw(SEEDS[1] + (1 << 32), KEYS, SERIALS, 1000)[0])  # the high word
    assert not np.array_equal(base[1:], base[:-1]) and not np.array_equal(base[:, 1:], base[:, :-1])
    for bad in (0, (1 << 20) + 1):
        with pytest.raises(ValueError, match="2\\^20"):
            O.book_draw(1, 0, 0, bad)


@pytest.mark.parametrize("size", [5, 6, 9])
def test_transform_equals_the_model_and_the_maps_form_the_square_group(size):
    from datou_gomoku_muzero_amd import openings as O
    A = size * size
    rs = np.random.RandomState(size)
    boards = rs.randint(-1, 2, (8, A)).astype(np.int8)
    lasts = np.array([-1, 0, size - 1, A - size, A - 1, 1, size, A // 2 + 1], np.int32)
    for d in range(8):
        got_b, got_l = O.transform_opening(boards, lasts, np.full(8, d), size)
        assert got_b.shape == (8, size, size) and got_b.dtype == np.int8 and got_l.dtype == np.int32
        for i in range(8):
            assert np.array_equal(got_b[i].reshape(-1), book_ref.transform_board(boards[i], size, d))
            assert got_l[i] == book_ref.transform_cell(int(lasts[i]), size, d)
    # one d per opening
    ds = np.arange(8)[::-1]
    got_b, got_l = O.transform_opening(boards, lasts, ds, size)
    for i in range(8):
        assert np.array_equal(got_b[i].reshape(-1), book_ref.transform_board(boards[i], size, int(ds[i])))
    # the eight maps: distinct permutations, closed under composition, with the identity at d = 0
    cells = O.symmetry_cells(size)
    assert np.array_equal(cells[0], np.arange(A))
    assert all(np.array_equal(np.sort(cells[d]), np.arange(A)) for d in range(8))
    assert len({tuple(c) for c in cells}) == 8
    group = {tuple(c) for c in cells}
    for a in range(8):
        for b in range(8):
            assert tuple(cells[b][cells[a]]) in group  # a, then b
    asym = np.zeros(A, np.int8)
    asym[[0, 1, size + 2]] = (1, -1, 1)  # no symmetry of the square keeps it
    assert len({tuple(book_ref.transform_board(asym, size, d)) for d in range(8)}) == 8


def _book(size, rows):
    """rows: (black cells, white cells, side to move, last, count or None)."""
    A = size * size
    b = np.zeros((len(rows), A), np.int8)
    for i, r in enumerate(rows):
        b[i, list(r[0])] = 1
        b[i, list(r[1])] = -1
    counts = [int((b[i] != 0).sum()) if r[4] is None else r[4] for i, r in enumerate(rows)]
    return (b.reshape(-1, size, size), np.array([r[2] for r in rows], np.int8), np.array([r[3] for r in rows], np.int32),
            np.array(counts, np.int32))


def test_check_selfplay_book_refuses_each_bad_book_with_its_message():
    from datou_gomoku_muzero_amd import openings as O
    cfg = _cfg(9, 5, NUM_TOP_ACTIONS=16)
    good = ((0, 10), (1,), -1, 10, None)
    out = O.check_selfplay_book(_book(9, [good, ((), (), 1, -1, None)]), cfg)
    assert out[0].shape == (2, 81) and out[0].dtype == np.int8 and out[3].tolist() == [3, 0]
    five = ((0, 1, 2, 3, 4), (9, 10, 11, 12), -1, 4, None)
    with pytest.raises(ValueError, match="opening 1 already holds 5 in a row"):
        O.check_selfplay_book(_book(9, [good, five]), cfg)
    win = ((0, 1, 2, 3), (9, 10, 11, 20), 1, 20, None)  # black to move completes the row at cell 4
    with pytest.raises(ValueError, match="opening 1 the side to move wins at once at \\(0, 4\\)"):
        O.check_selfplay_book(_book(9, [good, win]), cfg)
    O.check_selfplay_book(_book(9, [good, win[:2] + (-1,) + win[3:]]), cfg)  # white to move: black's four is no win yet
    full = (tuple(range(0, 66, 2)), tuple(range(1, 66, 2)), 1, 65, None)  # 66 stones: 15 cells left
    with pytest.raises(ValueError, match="NUM_TOP_ACTIONS = 16 legal cells \\(opening 1 leaves 15\\)"):
        O.check_selfplay_book(_book(9, [good, full]), cfg)
    with pytest.raises(ValueError, match="stone count differs"):
        O.check_selfplay_book(_book(9, [good, ((0,), (1,), 1, 1, 3)]), cfg)
    for side in (0, 2):
        with pytest.raises(ValueError, match="side to move must be \\+1 or -1"):
            O.check_selfplay_book(_book(9, [good, ((0,), (1,), side, 1, None)]), cfg)
    with pytest.raises(ValueError, match="at least one opening"):
        O.check_selfplay_book(_book(6, [good]), cfg)
    # the rule is cfg.N_IN_ROW's: three in a row at 6x6
    cfg3 = _cfg(6, 3, NUM_TOP_ACTIONS=16)
    with pytest.raises(ValueError, match="wins at once at \\(0, 2\\)"):
        O.check_selfplay_book(_book(6, [((0, 1), (6, 12), 1, 12, None)]), cfg3)
    with pytest.raises(ValueError, match="already holds 3 in a row"):
        O.check_selfplay_book(_book(6, [((0, 7, 14), (1, 2), -1, 14, None)]), cfg3)


@pytest.mark.parametrize("size,n_in_row,stones", [(9, 5, (2, 4, 6)), (6, 3, (2, 4, 6)), (6, 3, (4, 6, 8))])
def test_check_selfplay_book_accepts_paired_openings_without_the_excluded_rows(size, n_in_row, stones):
    from datou_gomoku_muzero_amd import openings as O
    cfg = _cfg(size, n_in_row, NUM_TOP_ACTIONS=16)
    book = O.paired_openings(96, size, 11, stones=stones, n_in_row=n_in_row)
    keep = O.selfplay_book_rows(book, cfg)
    assert keep.dtype == bool and keep.shape == (96,) and keep.sum() >= 24
    kept = tuple(x[keep] for x in book)
    out = O.check_selfplay_book(kept, cfg)
    assert np.array_equal(out[0].reshape(kept[0].shape), kept[0]) and np.array_equal(out[3], kept[3])
    if not keep.all():  # a dropped row is one the check refuses
        i = int(np.flatnonzero(~keep)[0])
        with pytest.raises(ValueError, match="wins at once|in a row"):
            O.check_selfplay_book(tuple(x[i:i + 1] for x in book), cfg)
    else:
        assert n_in_row == 5  # at most three stones a side: too few for a four; at three in a row some rows go


def test_play_book_refuses_a_null_engine_before_anything_else():
    """The fake-pointer pattern of tests/test_conv_sizes.py: nothing is dereferenced on this path."""
    import datou_gomoku_muzero_amd._lib as L
    lib = L.load()
    fake = ctypes.c_void_p(1 << 20)
    rc = lib.gmz_engine_play_book(None, fake, fake, fake, 81, fake, 1, fake, 4, fake, 4, 1, 7, 1, fake, fake, 1, None, 0,
                                  None)
    assert rc < 0 and lib.gmz_last_error().decode() == "gmz_engine_play_book: null engine, action or status"


def test_the_draw_is_no_noise_word():
    """Neither draw word equals an h1 or h2 word of the noise for the same (seed, key, counter = serial), a = 0..A-1;
    and neither salt is a constant of the generator or the value mix32(a + 0x68E31DA4) that would make w an h2."""
    A = 361
    a = np.arange(A, dtype=np.uint64)
    salts = (book_ref.SALT_OPEN, book_ref.SALT_SYM)
    assert salts[0] != salts[1]
    for s in salts:
        assert s not in (0x9E3779B1, 0x85EBCA77, 0x68E31DA4, 0x1B873593, 0x7FEB352D, 0x846CA68B, 0)
        assert not (noise_ref.mix32((np.arange(512, dtype=np.uint64) + np.uint64(0x68E31DA4)) & noise_ref.M32)
                    == np.uint64(s)).any()
    for seed in SEEDS[:2]:
        for key, serial in ((0, 0), (3, 1), (70, 40), (1023, 7)):
            h1 = int(book_ref.h1(seed, key, serial))
            h2 = set(noise_ref.h2(seed, serial, key, a).tolist())
            for s in salts:
                w = int(book_ref.word(seed, key, serial, s))
                assert w != h1 and w not in h2


def test_host_constants_are_the_header_s():
    import os
    import re
    from conftest import REPO
    from datou_gomoku_muzero_amd import openings as O
    hdr = open(os.path.join(REPO, "include", "gmz.h")).read()
    got = {k: int(v, 16) for k, v in re.findall(r"#define GMZ_BOOK_SALT_(\w+) (0x[0-9A-Fa-f]+)u", hdr)}
    assert got == {"OPEN": O.BOOK_SALT_OPEN, "SYM": O.BOOK_SALT_SYM} == {"OPEN": book_ref.SALT_OPEN, "SYM": book_ref.SALT_SYM}


def test_history_sets_the_next_game_s_first_row_when_a_game_is_reported():
    """GameHistory.set_book on the host alone (CPU tensors stand in for the snapshot): slot 1's game ends in bank 0,
    its next game's first row in bank 1 is the count of (slot 1, serial 1); the game after it, back in bank 0, that of
    serial 2."""
    from datou_gomoku_muzero_amd.worker import GameHistory
    h = GameHistory.__new__(GameHistory)
    h.G, h.k, h.start = 3, 0, np.zeros((2, 3), np.int64)
    counts = lambda slots, serials: 10 * np.asarray(slots) + np.asarray(serials) + 2  # noqa: E731
    h.set_book(counts)
    assert h.start.tolist() == [[2, 12, 22], [0, 0, 0]]

    class _Ev:
        def synchronize(self):
            pass

    import torch
    def snap(status, mc, bank):
        t = lambda x, dt: torch.tensor(x, dtype=dt)  # noqa: E731
        return dict(status=t(status, torch.int8), mc=t(mc, torch.int32), bank=t(bank, torch.int64),
                    mf=t([0, 0, 0], torch.int32), mt=t([0, 0, 0], torch.int32), act=t([5, 5, 5], torch.int32), ev=_Ev())

    assert h.finished(snap([2, 1, 2], [4, 15, 30], [0, 0, 0])) == [(1, 0, 12, 4, 1, 0, 0)]
    assert h.start.tolist() == [[2, 0, 22], [0, 13, 0]]
    assert h.finished(snap([2, -1, 0], [5, 20, 35], [0, 1, 0])) == [(1, 1, 13, 8, -1, 0, 0), (2, 0, 22, 14, 0, 0, 0)]
    assert h.start.tolist() == [[2, 14, 0], [0, 0, 23]] and h.serial.tolist() == [0, 2, 1]
