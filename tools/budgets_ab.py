"""Uniform simulation budgets against playout-cap randomisation (loop.SelfPlay(fast_sims=..., full_prob=...),
engine.set_budgets / gmz_engine_set_budgets), A/B in one process on one GPU at the headline self-play shape: 15x15,
400 simulations, 1,024 games on two HIP streams, 8 blocks, fp16, staggered openings.

  python tools/budgets_ab.py [--rounds 3 --moves 20 --warmup 5 --out profiles/budgets_ab.txt]

Two SelfPlay instances with the same weights, seed and openings: every game at 400 simulations, and each game at 400
with probability --full-prob and at --fast-sims otherwise, drawn per move.  After --warmup untimed moves of each, they
run --moves timed moves alternated --rounds times (a host clock around a device synchronise).  Per run: moves/s (games
x moves / s), the mean waves per move (per engine: every wave is one tower launch of its stream) and the mean tower
rows per wave (network rows of the selections, gmz_engine_tree_counters, over those launches: a game that has used its
budget leaves the remaining waves of its move).  One JSON line per run, then a summary with the ratio of the rates."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from datou_gomoku_muzero_amd import engine as E, loop as LP, weights as W  # noqa: E402
from datou_gomoku_muzero_amd.config import GmzConfig  # noqa: E402


def timed(sp, moves):
    engines = getattr(sp.eng, "engines", [sp.eng])
    sp.eng.tree_counters(reset=True)
    torch.cuda.synchronize()
    waves = 0
    full = 0
    t0 = time.perf_counter()
    for _ in range(moves):
        sp.step()
        waves += sum(e.waves_last for e in engines)
        if sp.budgets is not None:
            full += int((sp.budgets == sp.cfg.NUM_SIMULATIONS).sum())
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rows = sp.eng.tree_counters(reset=True)["selects"]
    return dict(seconds=round(dt, 4), moves_per_s=round(sp.G * moves / dt, 1), ms_per_move=round(dt / moves * 1e3, 2),
                waves_per_move=round(waves / len(engines) / moves, 2), tower_rows_per_wave=round(rows / max(waves, 1), 1),
                full_searches_percent=round(100.0 * full / (sp.G * moves), 1) if sp.budgets is not None else 100.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=15)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--streams", type=int, default=2)
    ap.add_argument("--fast-sims", type=int, default=32)
    ap.add_argument("--full-prob", type=float, default=0.25)
    ap.add_argument("--openings", type=int, default=80, help="staggered starts: up to this many stones")
    ap.add_argument("--moves", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
        if a.out:  # rewritten after every line: an interrupted run keeps what it measured
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    if not torch.cuda.is_available():
        sys.exit("tools/budgets_ab.py needs a GPU")
    emit("# tools/budgets_ab.py %s on %s" % (" ".join(sys.argv[1:]), torch.cuda.get_device_name(0)))
    cfg = GmzConfig(BOARD_SIZE=a.size, NUM_SIMULATIONS=a.sims, NUM_RES_BLOCKS=a.blocks)
    sd = W.synthetic_state_dict(cfg, seed=1, with_projection=False)
    sps = {}
    for name, kw in (("uniform", {}), ("mixed", dict(fast_sims=a.fast_sims, full_prob=a.full_prob))):
        op = E.random_openings(a.games, a.size, np.random.RandomState(a.seed + 17), a.openings, n_in_row=cfg.N_IN_ROW)
        sps[name] = LP.SelfPlay(cfg, a.games, sd, seed=a.seed, streams=a.streams, openings=op, **kw)
        for _ in range(a.warmup):
            sps[name].step()
        torch.cuda.synchronize()
    res = {"uniform": [], "mixed": []}
    for r in range(a.rounds):
        for name in (("uniform", "mixed") if r % 2 == 0 else ("mixed", "uniform")):  # the order in a round alternates
            out = timed(sps[name], a.moves)
            out.update(mode=name, round=r)
            res[name].append(out)
            emit(json.dumps(out))
    u = [x["moves_per_s"] for x in res["uniform"]]
    m = [x["moves_per_s"] for x in res["mixed"]]
    emit(json.dumps(dict(games=a.games, sims=a.sims, fast_sims=a.fast_sims, full_prob=a.full_prob, streams=a.streams,
                         uniform_moves_per_s=u, mixed_moves_per_s=m,
                         mixed_over_uniform=[round(y / x, 3) for x, y in zip(u, m)],
                         mixed_over_uniform_mean=round(float(np.mean(m) / np.mean(u)), 3),
                         uniform_waves_per_move=[x["waves_per_move"] for x in res["uniform"]],
                         mixed_waves_per_move=[x["waves_per_move"] for x in res["mixed"]],
                         uniform_rows_per_wave=[x["tower_rows_per_wave"] for x in res["uniform"]],
                         mixed_rows_per_wave=[x["tower_rows_per_wave"] for x in res["mixed"]])))
    for sp in sps.values():
        for e in getattr(sp.eng, "engines", [sp.eng]):
            assert e.errors() == 0
        sp.close()


if __name__ == "__main__":
    main()
