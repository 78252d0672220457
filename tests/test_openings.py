"""The opening builders (openings.py): their outputs are pinned to the values they had when they lived in engine.py
and arena.py, the module needs no torch, and the old import paths still name the same functions."""
import hashlib
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

import datou_gomoku_muzero_amd.arena as AR
import datou_gomoku_muzero_amd.openings as O


def _digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode())
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()[:16]


@pytest.mark.parametrize("build,want", [
    (lambda: O.seeded_openings(range(8), 15, 1234, stagger=80), "96126c70b43c6c1c"),
    (lambda: O.seeded_openings(range(8), 6, 77), "1393a47644c7dca6"),
    (lambda: O.random_openings(8, 6, np.random.RandomState(11), 12), "17f9334dd7ac6e6f"),
    (lambda: AR.paired_openings(9, 6, seed=3), "81d99a8c2384e773"),
    (lambda: AR.paired_openings(2, 6, seed=0, stones=(3,)), "adeb37b6cb89abd7"),
], ids=["seeded-15-stagger", "seeded-6", "random-6", "paired-9", "paired-2-odd"])
def test_outputs_are_the_pinned_ones(build, want):
    out = build()
    assert [(a.dtype, a.ndim) for a in out] == [(np.int8, 3), (np.int8, 1), (np.int32, 1), (np.int32, 1)]
    assert _digest(out) == want


def test_the_arenas_book_needs_no_torch():
    code = ("import sys; import datou_gomoku_muzero_amd.arena as AR; AR.paired_openings(2, 6, 1); "
            "assert 'torch' not in sys.modules, 'torch was imported'")
    r = subprocess.run([sys.executable, "-c", code], cwd=REPO, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]


def test_old_import_paths_name_the_same_functions():
    import datou_gomoku_muzero_amd.engine as E
    for name in ("seeded_openings", "random_openings", "_place_stones", "_has_five"):
        assert getattr(E, name) is getattr(O, name), name
    assert AR.paired_openings is O.paired_openings
