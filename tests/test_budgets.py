"""Per-game simulation budgets, host side (no GPU): gmz_engine_waves_for_budgets is gmz_engine_waves_for_legal
with each game's own budget (one schedule replay behind both), and the two new entry points refuse bad arguments
before any device work (fake pointers, never dereferenced: the tests/test_abi.py pattern)."""
import ctypes

import numpy as np
import pytest

BUDGETS = (1, 2, 15, 16, 17, 31, 32, 33, 50, 400)


def _lib():
    import datou_gomoku_muzero_amd._lib as L
    lib = L.load()
    return L, lib, (lambda: lib.gmz_last_error().decode())


def _cfg(L, size, sims, mode):
    return L.EngineCfg(1, size, 5, sims, 16, mode, 30, 0, 1.0, 1e-3, 0.997, 0)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize("size", [9, 15])
@pytest.mark.parametrize("mode", [0, 1])
def test_waves_for_budgets_equals_waves_for_legal_at_each_budget(size, mode):
    """Every legal count 0..A crossed with every budget in one call (game = (L, budget)): each game's waves equal
    gmz_engine_waves_for_legal's with a cfg whose num_simulations is that budget, and out_max is their maximum."""
    L, lib, err = _lib()
    A = size * size
    cap = _cfg(L, size, max(BUDGETS), mode)
    legal = np.repeat(np.arange(A + 1, dtype=np.int32), len(BUDGETS))
    budget = np.tile(np.array(BUDGETS, np.int32), A + 1)
    G = legal.size
    per = np.full(G, -7, np.int32)
    mx = ctypes.c_int32(-7)
    assert lib.gmz_engine_waves_for_budgets(ctypes.byref(cap), _p(legal), _p(budget), G, ctypes.byref(mx), _p(per)) == 0, err()
    want = np.empty(G, np.int32)
    out = ctypes.c_int32()
    for i in range(G):
        one = np.array([legal[i]], np.int32)
        c = _cfg(L, size, int(budget[i]), mode)
        assert lib.gmz_engine_waves_for_legal(ctypes.byref(c), _p(one), 1, ctypes.byref(out)) == 0
        want[i] = out.value
    assert np.array_equal(per, want), np.flatnonzero(per != want)[:8]
    assert mx.value == per.max() > 0
    # a sanity anchor that does not go through the library: AlphaZero takes one simulation per wave after the root's
    if mode == 0:
        assert np.array_equal(per[legal > 0], budget[legal > 0] - 1) and (per[legal == 0] == 0).all()
    # out_per_game is optional
    mx2 = ctypes.c_int32(-7)
    assert lib.gmz_engine_waves_for_budgets(ctypes.byref(cap), _p(legal), _p(budget), G, ctypes.byref(mx2), None) == 0
    assert mx2.value == mx.value


@pytest.mark.parametrize("size,sims,mode", [(9, 50, 1), (15, 400, 1), (9, 50, 0), (15, 33, 1)])
def test_null_budgets_mean_the_cfg_budget_for_every_game(size, sims, mode):
    L, lib, err = _lib()
    A = size * size
    cfg = _cfg(L, size, sims, mode)
    legal = np.arange(A + 1, dtype=np.int32)
    per = np.full(A + 1, -7, np.int32)
    mx, out = ctypes.c_int32(), ctypes.c_int32()
    assert lib.gmz_engine_waves_for_budgets(ctypes.byref(cfg), _p(legal), None, A + 1, ctypes.byref(mx), _p(per)) == 0, err()
    assert lib.gmz_engine_waves_for_legal(ctypes.byref(cfg), _p(legal), A + 1, ctypes.byref(out)) == 0
    assert mx.value == out.value == per.max()
    for n in range(A + 1):
        assert lib.gmz_engine_waves_for_legal(ctypes.byref(cfg), _p(legal[n:n + 1]), 1, ctypes.byref(out)) == 0
        assert per[n] == out.value, n


def test_budgets_outside_the_cfg_range_are_refused():
    L, lib, err = _lib()
    cfg = _cfg(L, 9, 50, 1)
    legal = np.full(4, 81, np.int32)
    per = np.full(4, -7, np.int32)
    mx = ctypes.c_int32(-7)
    for bad in (0, 51, -3):
        budget = np.array([50, 1, bad, 7], np.int32)
        assert lib.gmz_engine_waves_for_budgets(ctypes.byref(cfg), _p(legal), _p(budget), 4, ctypes.byref(mx), _p(per)) < 0
        assert "budget[2]" in err() and str(bad) in err() and "50" in err(), err()
        assert mx.value == -7 and (per == -7).all()  # nothing written
    ok = np.array([50, 1, 50, 7], np.int32)
    assert lib.gmz_engine_waves_for_budgets(ctypes.byref(cfg), _p(legal), _p(ok), 4, ctypes.byref(mx), _p(per)) == 0
    assert lib.gmz_engine_waves_for_budgets(None, _p(legal), _p(ok), 4, ctypes.byref(mx), _p(per)) < 0
    assert lib.gmz_engine_waves_for_budgets(ctypes.byref(cfg), None, _p(ok), 4, ctypes.byref(mx), _p(per)) < 0
    assert lib.gmz_engine_waves_for_budgets(ctypes.byref(cfg), _p(legal), _p(ok), 4, None, _p(per)) < 0
    assert "null" in err()


def test_set_budgets_refuses_a_null_engine_and_a_wrong_byte_count():
    """Before any device work: a null engine, and (over fake pointers, which no path below reads) byte counts that
    are 4 * G for no G, and a NULL array with a byte count."""
    L, lib, err = _lib()
    fake = ctypes.c_void_p(1 << 20)
    assert lib.gmz_engine_set_budgets(None, fake, 64, None) < 0
    assert "null engine" in err()
    assert lib.gmz_engine_set_budgets(None, None, 0, None) < 0
    assert "null engine" in err()
    for nbytes in (0, 1, 6, 63):
        assert lib.gmz_engine_set_budgets(fake, fake, nbytes, None) < 0, nbytes
        assert str(nbytes) + " bytes" in err() and "4 * G" in err(), err()
    assert lib.gmz_engine_set_budgets(fake, None, 64, None) < 0
    assert "budget_bytes = 0" in err(), err()
