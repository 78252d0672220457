"""tests/game_ref.py (the rules as a plain model, and the directed positions of tests/test_game_rules_gpu.py) pinned on
the CPU: to the reference's own recorded games and boards (tests/golden/game_cases.npz), to the C oracle on every
directed position, and to what each position was built to show."""
import numpy as np
import pytest

import game_ref as GR
import oracle


@pytest.mark.parametrize("size", (6, 9, 15, 19))
def test_model_matches_the_reference_s_recorded_games(golden, size):
    z = golden("game_cases.npz")
    p = "s%d_" % size
    d = {k: z[k] for k in z.files if k.startswith(p)}  # (an npz member is decompressed at every access)
    A = size * size
    for i in range(len(d[p + "moves"])):
        b = d[p + "boards"][i].copy()
        pl, lm, mv = int(d[p + "players"][i]), int(d[p + "lastmove"][i]), int(d[p + "moves"][i])
        obs = GR.board_state(b, size, pl, lm)
        assert np.array_equal(obs.reshape(3, A).astype(np.uint8), d[p + "obs"][i])
        mc = int(np.count_nonzero(b))
        st, pl2, lm2, mc2 = GR.play(b, pl, lm, mc, mv, 5, False)
        assert st == int(d[p + "ended"][i]) and (pl2, lm2, mc2) == (-pl, mv, mc + 1) and b[mv] == pl
        assert GR.check_win(b, size, 5, mv // size, mv % size) == bool(d[p + "wins"][i])
    for b, w in zip(d[p + "rand_boards"], d[p + "rand_wins"]):
        assert np.array_equal(GR.win_map(b, size, 5), w)


@pytest.mark.parametrize("size,n", GR.PAIRS)
def test_model_matches_the_oracle_on_the_directed_positions(size, n):
    c, after = GR.cases(size, n), GR.played(size, n, False)
    wins = GR.win_maps(size, n)
    for g in range(len(c["actions"])):
        b, a = after["boards"][g], int(c["actions"][g])
        stones = np.flatnonzero(b)
        assert not wins[g][b == 0].any()
        got = np.array([oracle.check_win(b, size, s // size, s % size, n) for s in stones], np.uint8)
        assert np.array_equal(got, wins[g][stones]), (g, c["tags"][g])
        if a >= 0:
            e = oracle.game_ended(b, size, a, int(after["counts"][g]), n)
            assert (2 if e is None else e) == after["status"][g], (g, c["tags"][g])
        lm = int(c["last"][g])
        assert np.array_equal(oracle.board_state(c["boards"][g], size, int(c["players"][g]), None if lm < 0 else lm),
                              GR.board_state(c["boards"][g], size, int(c["players"][g]), lm))


@pytest.mark.parametrize("size,n", GR.PAIRS)
def test_directed_positions_show_what_they_were_built_for(size, n):
    c = GR.cases(size, n)
    A, G = size * size, len(c["actions"])
    for reset in (False, True):
        p = GR.played(size, n, reset)
        assert np.array_equal(p["status"], c["expect"]), [c["tags"][g] for g in np.flatnonzero(p["status"] != c["expect"])]
        for g in range(G):
            a, st = int(c["actions"][g]), int(p["status"][g])
            before = (c["boards"][g], c["players"][g], c["last"][g], c["counts"][g])
            now = (p["boards"][g], p["players"][g], p["last"][g], p["counts"][g])
            if st == 3:  # untouched
                assert a < 0 and all(np.array_equal(x, y) for x, y in zip(before, now))
            elif reset and st != 2:  # restarted
                assert not now[0].any() and (now[1], now[2], now[3]) == (1, -1, 0)
            else:
                want = before[0].copy()
                want[a] = before[1]
                assert before[0][a] == 0 and np.array_equal(now[0], want)
                assert (now[1], now[2], now[3]) == (-before[1], a, before[3] + 1)
    tags = set(c["tags"])
    assert {"draw", "last-cell win", "count draw", "none"} <= tags and any(t.startswith("wrap s1") for t in tags)
    st = GR.played(size, n, False)["status"]
    assert {-1, 0, 1, 2, 3} == set(st.tolist())
    # both colours move, win and draw; every border cell of the board is the last stone of some winning run
    for col in (1, -1):
        m = c["players"] == col
        assert (st[m] == col).any() and (st[m] == 0).any() and (st[m] == 2).any()
    won = c["actions"][np.abs(st) == 1]
    r, q = won // size, won % size
    for edge in (r == 0, r == size - 1, q == 0, q == size - 1):
        assert edge.any()
    for corner in (0, size - 1, A - size, A - 1):
        assert corner in won
    # a win on the last empty cell is reported as a win, with the count at size^2
    m = np.array([t == "last-cell win" for t in c["tags"]])
    assert (np.abs(st[m]) == 1).all() and (c["counts"][m] == A - 1).all()


def test_the_generator_stays_small():
    total = sum(len(GR.cases(s, n)["actions"]) for s, n in GR.PAIRS)
    print("directed positions:", total)
    assert 2000 <= total <= 8000
    assert GR.PAIRS[0] == (5, 3) and GR.PAIRS[-1] == (22, 6) and len(GR.PAIRS) == 23


def test_lines_end_at_the_borders():
    """The four cases a flat-index walk gets wrong, spelled out on a 5x5 board with three in a row."""
    size, n = 5, 3
    b = np.zeros(25, np.int8)
    b[[3, 4, 5]] = 1  # row 0's end into row 1's start
    assert not GR.win_map(b, size, n).any()
    b[:] = 0
    b[[5, 1, 9]] = 1  # (1,0), (0,1) and, one flat anti-diagonal step before (1,0) wraps to, (1,4)
    assert not GR.win_map(b, size, n).any()
    b[:] = 0
    b[[3, 9, 15]] = -1  # (0,3), (1,4) and the flat diagonal step after it, (3,0)
    assert not GR.win_map(b, size, n).any()
    b[:] = 0
    b[[2, 6, 10]] = -1  # a true anti-diagonal into the left border
    assert GR.win_map(b, size, n).sum() == 3
