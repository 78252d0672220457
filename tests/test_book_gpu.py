"""Self-play's restart from an opening book on the GPU: gmz_engine_play_book against the model of tests/book_ref.py
word for word, a book engine against an engine whose ended slots the test replaces through set_positions, two streams
against one, and loop.SelfPlay(book=...) through the history into the replay ring on both paths."""
import ctypes

import numpy as np
import pytest

import book_ref
import game_ref
from kernel_guards import Buf

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SEED = (0x5A17 << 32) | 0xC0FFEE  # a non-zero high word
FILL8, FILL32 = 0x55, 0x55555555


@pytest.fixture(scope="module")
def E():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import datou_gomoku_muzero_amd.engine as E
    import datou_gomoku_muzero_amd._lib as L
    L.load()
    return E


# ------------------------------------------------------------------------------------------ the entry point
def _raw_book(size, n_in_row, n):
    """A book for the kernel alone (nothing checks it): an asymmetric opening first (n = 1: the whole book), an empty
    board with last move -1 second, paired openings after them."""
    from datou_gomoku_muzero_amd import openings as O
    A = size * size
    asym = np.zeros(A, np.int8)
    asym[[1, size + 3]] = 1
    asym[2 * size] = -1
    rows = [(asym, -1, size + 3, 3), (np.zeros(A, np.int8), 1, -1, 0)]
    pb, pp, pl, pc = O.paired_openings(max(n - 2, 1), size, 40 + size, n_in_row=n_in_row)
    rows += [(pb[i].reshape(-1), int(pp[i]), int(pl[i]), int(pc[i])) for i in range(max(n - 2, 1))]
    rows = rows[:n]
    return (np.array([r[0] for r in rows], np.int8), np.array([r[1] for r in rows], np.int8),
            np.array([r[2] for r in rows], np.int32), np.array([r[3] for r in rows], np.int32))


def _lane_action(board, player, size, g):
    """The scripted move: the first empty cell from the start of the mover's own row on, so that a colour's stones
    line up and games end by a win after a few moves."""
    A = size * size
    row = (g + (0 if player == 1 else 2)) % size
    order = (np.arange(A) + row * size) % A
    empty = order[board[order] == 0]
    return int(empty[0]) if len(empty) else -1


class _Raw:
    """One engine driven through the raw entry point, every array the call writes behind guard words."""

    def __init__(self, E, size, n_in_row, G, offset, book, symmetry, with_tally=True):
        import datou_gomoku_muzero_amd._lib as L
        self.L, self.lib = L, L.load()
        self.eng = E.BatchedSelfPlayEngine(None, num_games=G, BOARD_SIZE=size, N_IN_ROW=n_in_row, NUM_SIMULATIONS=2,
                                           MCTS_IMPLEMENTATION="MuZero", game_offset=offset)
        self.eng.reset_games()
        self.G, self.A, self.n, self.symmetry = G, size * size, len(book[1]), symmetry
        self.book = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in book]
        self.status = Buf(G, torch.int8, off=3, fill=FILL8)
        self.serial = Buf(G, torch.int32, off=1, fill=FILL32, data=np.full(G, -1, np.int32))
        self.draw = Buf(G, torch.int32, off=2, fill=FILL32, data=np.full(G, -1, np.int32))
        self.tally = Buf(3 * self.n, torch.int32, off=1, fill=FILL32, data=np.zeros(3 * self.n, np.int32)) \
            if with_tally else None
        self.action = torch.full((G,), -1, dtype=torch.int32, device="cuda")

    def call(self, actions=None, **kw):
        L = self.L
        if actions is not None:
            self.action.copy_(torch.from_numpy(np.asarray(actions, np.int32)))
        b, p, lm, mc = self.book
        a = dict(e=self.eng.handle, action=L.ptr(self.action), status=L.ptr(self.status.t), boards=L.ptr(b),
                 boards_bytes=L.nbytes(b), players=L.ptr(p), players_bytes=L.nbytes(p), last=L.ptr(lm),
                 last_bytes=L.nbytes(lm), counts=L.ptr(mc), counts_bytes=L.nbytes(mc), n=self.n, seed=SEED,
                 symmetry=1 if self.symmetry else 0, serial=L.ptr(self.serial.t), draw=L.ptr(self.draw.t), cap=self.G,
                 tally=None if self.tally is None else L.ptr(self.tally.t),
                 tally_bytes=0 if self.tally is None else 12 * self.n, stream=L.stream_ptr())
        a.update(kw)
        return self.lib.gmz_engine_play_book(*a.values())

    def state(self):
        b, p, lm, mc = self.eng.game_state()
        torch.cuda.synchronize()
        out = dict(boards=b.reshape(self.G, self.A).cpu().numpy(), players=p.cpu().numpy(), last=lm.cpu().numpy(),
                   counts=mc.cpu().numpy(), serial=self.serial.t.cpu().numpy(), draw=self.draw.t.cpu().numpy())
        return out, self.status.t.cpu().numpy(), None if self.tally is None else self.tally.t.cpu().numpy().reshape(-1, 3)

    def intact(self):
        return all(x.intact() for x in (self.status, self.serial, self.draw, self.tally) if x is not None)


PLAY_CASES = [  # size, n_in_row, G, game_offset, openings, symmetry
    (6, 3, 1, 0, 1, True), (6, 3, 7, 5, 3, True), (6, 3, 300, 0, 64, False), (9, 5, 7, 0, 64, True),
    (9, 5, 300, 5, 3, True), (19, 5, 300, 0, 64, True), (19, 5, 7, 5, 1, False),
]


@pytest.mark.parametrize("size,n_in_row,G,offset,n,symmetry", PLAY_CASES)
def test_play_book_equals_the_model_word_for_word(E, size, n_in_row, G, offset, n, symmetry):
    A = size * size
    book = _raw_book(size, n_in_row, n)
    assert (book[2] == -1).any() or n == 1
    raw = _Raw(E, size, n_in_row, G, offset, book, symmetry)
    model = book_ref.empty_state(G, A)
    tally = np.zeros((n, 3), np.int32)

    def compare(want_status, what):
        got, status, got_tally = raw.state()
        for k in model:
            assert np.array_equal(got[k], model[k]), "%s: %s differs in slots %s" % (
                what, k, np.flatnonzero((got[k] != model[k]).reshape(G, -1).any(1))[:8])
        assert np.array_equal(status, want_status), what
        assert np.array_equal(got_tally, tally), what
        assert raw.intact(), what

    # the first call: every action -1 fills every slot at serial 0
    none = np.full(G, -1, np.int32)
    assert raw.call(none) == 0
    want = book_ref.play_book(model, none, book, SEED, symmetry, n_in_row, offset, tally)
    assert (want == 3).all() and (model["serial"] == 0).all() and not tally.any()
    compare(want, "fill")
    # directed slots, set in the engine and in the model alike: slot 0 two moves from a full board without a line,
    # slot 1 one move from a win that it plays at call 2, slot 2 never moves again
    pat = game_ref._pattern(size)
    full = pat.copy()
    a_own, a_opp = int(np.flatnonzero(pat == 1)[0]), int(np.flatnonzero(pat == -1)[-1])
    full[[a_own, a_opp]] = 0
    model["boards"][0], model["players"][0], model["last"][0], model["counts"][0] = full, 1, -1, A - 2
    if G >= 7:
        win = np.zeros(A, np.int8)
        win[size:size + n_in_row - 1] = -1  # white's open row on row 1, white to move
        win[[3 * size, 3 * size + 2, 4 * size + 1][:n_in_row - 1]] = 1
        model["boards"][1], model["players"][1], model["last"][1] = win, -1, 3 * size
        model["counts"][1] = int(np.count_nonzero(win))
    raw.eng.set_positions(model["boards"], model["players"], model["last"], model["counts"])
    seen, mixed, symmetries = set(), False, set(model["draw"] & 7)
    for call in range(1, 13):
        acts = np.full(G, -1, np.int32)
        for g in range(G):
            if g == 0:
                acts[g] = {1: a_own, 2: a_opp}.get(call, _lane_action(model["boards"][g], model["players"][g], size, g))
            elif g == 1 and G >= 7 and call <= 2:
                acts[g] = size + n_in_row - 1 if call == 2 else -1
            elif g == 2 or (g % 5 == 4 and call % 2 == 1) or call <= g % 3:
                pass  # untouched
            else:
                acts[g] = _lane_action(model["boards"][g], model["players"][g], size, g)
        assert raw.call(acts) == 0
        want = book_ref.play_book(model, acts, book, SEED, symmetry, n_in_row, offset, tally)
        compare(want, "call %d" % call)
        seen |= set(want.tolist())
        symmetries |= set((model["draw"] & 7).tolist())
        mixed = mixed or (0 in want and (abs(want) == 1).any() and 2 in want and 3 in want)
    assert 0 in seen  # the full board ended in a draw
    if G >= 7:
        assert mixed, "no call in which a draw, a win, a game going on and an untouched slot meet"
        assert tally.sum() == (model["serial"]).sum() > 0 and (model["serial"] >= 1).sum() >= 2
    if G == 300:
        assert symmetries == (set(range(8)) if symmetry else {0})
        assert tally.sum() >= 8  # black's lane holds five after nine plies: restarts well beyond the directed slots
    assert raw.eng.errors() == 0
    raw.eng.close()


def test_play_book_without_a_tally_and_every_refusal(E):
    size, G = 6, 7
    book = _raw_book(size, 3, 3)
    raw = _Raw(E, size, 3, G, 0, book, True, with_tally=False)
    model = book_ref.empty_state(G, size * size)
    none = np.full(G, -1, np.int32)
    assert raw.call(none) == 0  # a null tally is allowed
    book_ref.play_book(model, none, book, SEED, True, 3)
    got, status, _ = raw.state()
    assert all(np.array_equal(got[k], model[k]) for k in model) and (status == 3).all()
    raw.eng.close()

    raw = _Raw(E, size, 3, G, 0, book, True)
    err = lambda: raw.lib.gmz_last_error().decode()  # noqa: E731
    fake = ctypes.c_void_p(1 << 20)
    cases = [
        (dict(e=None), "null engine, action or status"), (dict(action=None), "null engine, action or status"),
        (dict(status=None), "null engine, action or status"), (dict(boards=None), "null book array"),
        (dict(players=None), "null book array"), (dict(last=None), "null book array"),
        (dict(counts=None), "null book array"), (dict(serial=None), "null serial or draw array"),
        (dict(draw=None), "null serial or draw array"), (dict(n=0), "n_openings must be in [1, 2^20]"),
        (dict(n=(1 << 20) + 1), "n_openings must be in [1, 2^20]"),
        (dict(boards_bytes=3 * 36 - 1), "book_boards holds 107 bytes, n_openings * board_size^2 = 108"),
        (dict(players_bytes=2), "book_players holds 2 bytes, n_openings = 3"),
        (dict(last_bytes=11), "hold 11 and 12 bytes, 4 * n_openings = 12"),
        (dict(counts_bytes=8), "hold 12 and 8 bytes, 4 * n_openings = 12"),
        (dict(cap=G - 1), "slot arrays hold 6 slots, the engine has 7"), (dict(cap=0), "slot_capacity must be >="),
        (dict(tally_bytes=35), "tally holds 35 bytes, 12 * n_openings = 36"),
        (dict(symmetry=2), "symmetry must be 0 or 1"), (dict(symmetry=-1), "symmetry must be 0 or 1"),
    ]
    before = raw.eng.game_state()
    for kw, text in cases:
        assert raw.call(none, **kw) < 0, kw
        assert err().startswith("gmz_engine_play_book: ") and text in err(), (kw, err())
    # a refusal that needs no engine comes before the handle is read
    assert raw.call(none, e=fake, n=0) < 0 and "n_openings" in err()
    torch.cuda.synchronize()
    assert raw.intact() and raw.status.untouched()
    assert (raw.serial.t == -1).all() and (raw.draw.t == -1).all() and not raw.tally.t.any()
    after = raw.eng.game_state()
    assert all(torch.equal(x, y) for x, y in zip(before, after))
    raw.eng.close()


# ------------------------------------------------------------------------------------------ engines
def _book6(cfg_kw=None):
    """A checked 6x6 three-in-a-row book: paired openings without the rows the win rule excludes."""
    from datou_gomoku_muzero_amd import openings as O
    from datou_gomoku_muzero_amd.config import from_any
    cfg = from_any(None, BOARD_SIZE=6, N_IN_ROW=3, **(cfg_kw or {}))
    book = O.paired_openings(40, 6, 5, n_in_row=3)
    keep = O.selfplay_book_rows(book, cfg)
    assert keep.sum() >= 8
    return tuple(x[keep] for x in book)


def _engine6(E, G, split=False, **kw):
    cls = E.SplitSelfPlayEngine if split else E.BatchedSelfPlayEngine
    e = cls(None, num_games=G, seed=SEED, BOARD_SIZE=6, N_IN_ROW=3, NUM_SIMULATIONS=16, MCTS_IMPLEMENTATION="MuZero", **kw)
    e.reset_games()
    return e


def _model_opening(book, slot, serial, size, symmetry=True):
    t, d = book_ref.draw(SEED, slot, serial, len(book[1]), symmetry)
    t, d = int(t), int(d)
    return (book_ref.transform_board(book[0][t].reshape(-1), size, d), int(book[1][t]),
            book_ref.transform_cell(int(book[2][t]), size, d), int(book[3][t]), t)


def _move(eng):
    pol, val, act = eng.search()
    status = eng.play(reset_finished=True)
    torch.cuda.synchronize()
    return [x.cpu().numpy().copy() for x in (pol, val, act, status)]


@pytest.mark.parametrize("budgets", [False, True])
def test_restart_equals_set_positions(E, budgets):
    """An engine with a book against one without, whose ended slots the test loads with the model's draw."""
    G, size, moves = 16, 6, 30
    book = _book6()
    a, b = _engine6(E, G), _engine6(E, G)
    a.set_book(book)
    a.fill_from_book()
    serial = np.zeros(G, np.int64)
    first = [_model_opening(book, g, 0, size) for g in range(G)]
    b.set_positions(np.array([o[0] for o in first]), [o[1] for o in first], [o[2] for o in first], [o[3] for o in first])
    rs = np.random.RandomState(3)
    restarts = 0
    for m in range(moves):
        if budgets:
            bud = rs.randint(1, 17, G).astype(np.int32)
            a.set_budgets(bud)
            b.set_budgets(bud)
        ra, rb = _move(a), _move(b)
        for x, y, name in zip(ra, rb, ("policy", "value", "action", "status")):
            assert x.tobytes() == y.tobytes(), "move %d: %s differs" % (m, name)
        ended = np.flatnonzero((rb[3] != 2) & (rb[3] != 3))
        if len(ended):
            bb, bp, bl, bc = (t.cpu().numpy().copy() for t in b.game_state())
            bb = bb.reshape(G, size * size)
            for g in ended:
                serial[g] += 1
                bb[g], bp[g], bl[g], bc[g], _ = _model_opening(book, g, int(serial[g]), size)
            b.set_positions(bb, bp, bl, bc)
            restarts += len(ended)
        sa, sb = a.game_state(), b.game_state()
        assert all(torch.equal(x, y) for x, y in zip(sa, sb)), "move %d: the positions differ" % m
    assert restarts >= G and a.errors() == 0 and b.errors() == 0
    a.sync_status()
    assert np.array_equal(a._book["serial"], serial)
    assert int(a.book_tally.sum()) == restarts
    a.close()
    b.close()


def test_two_streams_play_the_games_of_one_engine(E):
    G, moves = 16, 30
    book = _book6()
    one, two = _engine6(E, G), _engine6(E, G, split=True, parts=2)
    for e in (one, two):
        e.set_book(book)
        e.fill_from_book()
    assert two.engines[1]._book["buf"] is two.engines[0]._book["buf"]
    assert two.engines[1].book_tally.data_ptr() == two.book_tally.data_ptr()
    for m in range(moves):
        r1, r2 = _move(one), _move(two)
        for x, y, name in zip(r1, r2, ("policy", "value", "action", "status")):
            assert x.tobytes() == y.tobytes(), "move %d: %s differs" % (m, name)
    assert all(torch.equal(x, y) for x, y in zip(one.game_state(), two.game_state()))
    torch.cuda.synchronize()
    assert torch.equal(one.book_tally, two.book_tally) and int(one.book_tally.sum()) >= G
    one.close()
    two.close()


def test_engine_refuses_what_a_book_cannot_do(E):
    e = _engine6(E, 4)
    with pytest.raises(ValueError, match="no book is set"):
        e.fill_from_book()
    e.set_book(_book6())
    with pytest.raises(ValueError, match="fill_from_book"):
        e.play(action=np.full(4, -1, np.int32))
    e.fill_from_book()
    with pytest.raises(ValueError, match="already"):
        e.fill_from_book()
    with pytest.raises(ValueError, match="not this engine's size"):
        from datou_gomoku_muzero_amd import openings as O
        from datou_gomoku_muzero_amd.config import from_any
        e.set_book(E.BookBuffers(O.paired_openings(4, 9, 1), from_any(None, BOARD_SIZE=9)))
    e.close()


# ------------------------------------------------------------------------------------------ history and ring
def _selfplay_cfg(size, n_in_row):
    from datou_gomoku_muzero_amd.config import GmzConfig
    return GmzConfig(BOARD_SIZE=size, N_IN_ROW=n_in_row, NUM_SIMULATIONS=16, NUM_RES_BLOCKS=1)


@pytest.mark.parametrize("size,n_in_row,G,cap", [(6, 3, 16, 150), (9, 4, 8, 400)])
def test_selfplay_from_a_book_through_history_and_ring(E, size, n_in_row, G, cap):
    """Two SelfPlay instances with one seed and one book, one harvesting on the host, one ingesting on the device, until
    every slot has restarted at least twice (three and four in a row keep the games short; ``cap`` bounds the loop)."""
    from datou_gomoku_muzero_amd import loop as LP, openings as O, replay as RP, trainer as T, weights as W
    from datou_gomoku_muzero_amd.replay import slices_from_game
    cfg = _selfplay_cfg(size, n_in_row)
    book = O.paired_openings(24, size, 9, n_in_row=n_in_row)
    book = tuple(x[O.selfplay_book_rows(book, cfg)] for x in book)
    n = len(book[1])
    assert n >= 8 and len(set(book[3].tolist())) > 1  # openings of different stone counts
    sd = W.synthetic_state_dict(cfg, seed=1, with_projection=False)
    tcfg = T.TrainConfig(BOARD_SIZE=size, NUM_RES_BLOCKS=1, TRAIN_BUFFER_SIZE=128, ENABLE_PER=True)
    rb_host, rb_dev = RP.ReplayBuffer(tcfg, device="cuda"), RP.ReplayBuffer(tcfg, device="cuda")
    assert (tcfg.DISCOUNT, tcfg.NUM_UNROLL_STEPS, tcfg.N_STEPS) == (cfg.DISCOUNT, cfg.NUM_UNROLL_STEPS, cfg.N_STEPS)
    sp_host = LP.SelfPlay(cfg, G, sd, seed=SEED, book=book)
    sp_dev = LP.SelfPlay(cfg, G, sd, seed=SEED, book=book)
    sp_dev.ingest_into(rb_dev)
    serial = np.zeros(G, np.int64)  # of the next game reported per slot
    per_opening = np.zeros((n, 3), np.int64)

    def take(done_host, done_dev):
        assert [x[:5] for x in done_host] == done_dev
        for (g, winner, length, mf, mt, boards, players, lasts, pols, vals, acts) in done_host:
            want_b, want_p, want_l, stones, t = _model_opening(book, g, int(serial[g]), size)
            serial[g] += 1
            assert np.array_equal(boards[0], want_b) and players[0] == want_p and lasts[0] == want_l
            assert np.count_nonzero(boards[-1]) + 1 - stones == length == len(acts)
            per_opening[t, {1: 0, -1: 1, 0: 2}[winner]] += 1
            arrs = slices_from_game(boards, players, lasts, pols, vals, acts, winner, size, cfg.DISCOUNT, cfg.N_STEPS,
                                    cfg.NUM_UNROLL_STEPS)
            rb_host.add_arrays(*arrs, game=(winner, int(np.count_nonzero(boards[0])), 0))

    moves = 0
    while serial.min() < 3 and moves < cap:
        take(sp_host.step(), sp_dev.step())
        moves += 1
    take(sp_host.flush(), sp_dev.flush())
    assert serial.min() >= 2, "after %d moves a slot has restarted fewer than two times: %s" % (moves, serial)
    torch.cuda.synchronize()
    assert (rb_host.ptr, rb_host.count) == (rb_dev.ptr, rb_dev.count) and rb_dev.count == 128  # the ring wrapped
    for name in ("obs", "act", "rew", "pol", "val", "prio"):
        assert torch.equal(getattr(rb_host, name), getattr(rb_dev, name)), name
    entry = lambda e: (e.slot, e.kept, e.n, e.winner, e.start)  # noqa: E731
    assert [entry(e) for e in rb_host.games] == [entry(e) for e in rb_dev.games] and len(rb_dev.games) > 0
    assert any(e.start > 0 for e in rb_dev.games)
    for sp in (sp_host, sp_dev):
        tally = sp.book_tally().cpu().numpy()
        assert tally.shape == (n, 3) and np.array_equal(tally, per_opening)
        for eng in getattr(sp.eng, "engines", [sp.eng]):
            assert eng.errors() == 0
        sp.close()


def test_without_a_book_the_new_entry_point_is_never_called(E, monkeypatch):
    from datou_gomoku_muzero_amd import loop as LP, weights as W
    calls = [0]
    real = E.BatchedSelfPlayEngine._play_book

    def counted(self, a, s):
        calls[0] += 1
        return real(self, a, s)

    monkeypatch.setattr(E.BatchedSelfPlayEngine, "_play_book", counted)
    cfg = _selfplay_cfg(6, 3)
    sd = W.synthetic_state_dict(cfg, seed=1, with_projection=False)
    sp = LP.SelfPlay(cfg, 8, sd, seed=1)
    for _ in range(12):
        sp.step()
    sp.flush()
    assert calls[0] == 0 and sp.book_tally() is None
    sp.close()
    book = _book6()
    with pytest.raises(ValueError, match="not both"):
        LP.SelfPlay(cfg, 8, sd, seed=1, book=book, openings=book)
    sp = LP.SelfPlay(cfg, 8, sd, seed=1, book=book, book_symmetry=False)
    for _ in range(3):
        sp.step()
    assert calls[0] == 1 + 3  # the fill and one per move
    assert not (sp.eng.book_draws()[1]).any()  # no symmetry: every d is 0
    sp.close()
