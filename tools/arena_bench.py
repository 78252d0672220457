"""Arena throughput: moves/s of arena.Arena in its steady state (every slot busy), one network against itself, at
the headline's shape (15x15, 400 simulations, 1,024 slots, 8 blocks, fp16) — to set beside ``python bench.py``'s
self-play headline on the same GPU (profiles/arena.txt).

  python tools/arena_bench.py [--streams 1,2 --steps 10 --warmup 3 --rounds 2]

The book holds more openings than the timed plies can finish, so no slot idles; a move is counted from the
statuses (arena's ``moves_played``).  Prints one JSON line per (round, streams)."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from datou_gomoku_muzero_amd import arena as AR, engine as E, network as N, weights as W  # noqa: E402
from datou_gomoku_muzero_amd.config import GmzConfig  # noqa: E402


def measure(cfg, sd, slots, streams, steps, warmup, precision, seed):
    nets = [N.GomokuNetHip(sd, cfg, num_slots=E.hidden_slots(cfg, slots), max_rows=slots, precision=precision)
            for _ in range(2)]
    book = AR.paired_openings(4 * slots, cfg.BOARD_SIZE, seed)
    ar = AR.Arena(cfg, nets[0], nets[1], slots, book, seed=seed, streams=streams)
    ar.start()
    for _ in range(warmup):
        ar.step()
    ar.join()
    m0 = sum(e.moves_played for e in ar.engines)
    t0 = time.perf_counter()
    for _ in range(steps):
        ar.step()
    ar.join()
    dt = time.perf_counter() - t0
    moves = sum(e.moves_played for e in ar.engines) - m0
    out = dict(streams=streams, slots=slots, steps=steps, moves=moves, seconds=round(dt, 4),
               moves_per_s=round(moves / dt, 1), finished=int(ar.match.finished[0]),
               waves_last=[e.waves_last for e in ar.engines])
    ar.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=15)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--slots", type=int, default=1024)
    ap.add_argument("--streams", default="1,2")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--seed", type=int, default=1234)
    a = ap.parse_args()
    cfg = GmzConfig(BOARD_SIZE=a.size, NUM_SIMULATIONS=a.sims, NUM_RES_BLOCKS=a.blocks)
    sd = W.synthetic_state_dict(cfg, seed=a.seed, with_projection=False)
    for r in range(a.rounds):
        for s in [int(x) for x in a.streams.split(",")]:
            out = measure(cfg, sd, a.slots, s, a.steps, a.warmup, a.precision, a.seed)
            out["round"] = r
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
