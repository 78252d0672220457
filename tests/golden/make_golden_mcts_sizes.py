"""Reference search fixture at 13x13 (a board size between the original four), from the REFERENCE's mcts.py.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mcts_sizes.py

Uses make_golden.py's reference import, recorders and make_mcts_case, so mcts_mz13_50.npz has the format of
every other mcts_*.npz (tests/test_engine_gpu.py picks it up by name).  MuZero, 50 simulations, 5 positions
after an 8-stone opening.
"""
import make_golden as G

SCENARIOS = [("mz13_50", 13, "MuZero", 50, 22, 5, 8)]  # name, size, mode, sims, np seed, moves, opening stones


if __name__ == "__main__":
    for sc in SCENARIOS:
        G.make_mcts_case(*sc)
