"""Network fixtures at board sizes between the original four, from the REFERENCE's own network.py.

Run:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_net_sizes.py

Uses make_golden.py's reference import and its _net_case (the writer of net_c15.npz); like that file it
reads the reference at run time only, and the outputs are committed as small .npz files.  Each case is
GomokuNetEZ with 128 filters and 2 blocks on 2 observations and 2 actions, one per inference-tower path
(csrc/gmz_net.hip TowerCfg):
  net_c5.npz    5x5    several boards (five) packed into one workgroup
  net_c8.npz    8x8    A % 16 == 0: two boards whose packed run saves no tile
  net_c13.npz   13x13  one board, two LDS images
  net_c17.npz   17x17  one board, a single LDS image and the residual scratch
"""
import make_golden as G

CASES = [("net_c5.npz", 5, 25), ("net_c8.npz", 8, 28), ("net_c13.npz", 13, 33), ("net_c17.npz", 17, 37)]


if __name__ == "__main__":
    for fname, size, seed in CASES:
        G._net_case(fname, size, 128, 2, 64, seed=seed, n_rows=2, full_hidden=False)
