"""Re-analysis of the replay ring inside the C4 loop (loop.C4Loop(reanalyser=..., reanalyse_per_iter=...)), A/B in one
process on one GPU at C4's own workload: 15x15, 400 simulations, 1,024 games from staggered openings, 8 blocks,
B = 360, PER, a prefilled shard (bench.py's loop leg, driven through the same loop.run_c4), device ingest on.

  python tools/reanalyse_ab.py [--rounds 2 --iters 20 --warmup 6 --out profiles/reanalyse_ab.txt]

Three settings, alternated ``--rounds`` times after one untimed warm-up run: the feature off; one pass per iteration
through host memory (the planes read back and decoded on the host, Reanalyser.search_positions' upload, synchronise
and read-back per chunk, ReplayBuffer.rewrite_games_host, and nothing else); one pass per iteration on the device
(gmz_replay_positions, set_positions_device, gmz_replay_rewrite).  The off setting's repeats show the box's own
spread.  A pass re-searches up to ``--ra-positions`` positions in chunks of ``--ra-games`` engine rows; with both at
the self-play engine's 1,024 games (the default) a full pass is one search of as many rows as a self-play move, so
(ms per iteration with passes - ms per iteration without) is what a pass costs beside a move.  Age threshold 0: every
game in the ring is eligible, oldest search first.  run_c4 times its window with a host clock around a device
synchronise.  One JSON line per run, then a summary."""
import argparse
import gc
import json
import os
import sys
from types import SimpleNamespace

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from datou_gomoku_muzero_amd import loop as LP  # noqa: E402

SETTINGS = ("off", "host", "device")


def namespace(a, setting, iters=None):
    return SimpleNamespace(size=a.size, sims=a.sims, blocks=a.blocks, trainer_batch=a.batch, loop_buffer=a.buffer,
                           loop_update_interval=1000, loop_openings=a.openings, loop_games=a.games, seed=a.seed,
                           precision="fp16", loop_prefill=a.prefill, loop_moves_per_iter=1, loop_train_per_iter=1,
                           loop_concurrent=a.concurrent, loop_warmup=a.warmup,
                           loop_iters=a.iters if iters is None else iters, loop_device_ingest=not a.host_ingest,
                           loop_reanalyse=0 if setting == "off" else 1, loop_reanalyse_host=setting == "host",
                           loop_reanalyse_age=0, loop_reanalyse_games=a.ra_games, loop_reanalyse_positions=a.ra_positions)


def run(a, setting, emit, label=None, iters=None):
    d, dt = LP.run_c4(namespace(a, setting, iters), 0, 1, None, None, log=lambda s: None)
    its = max(d["moves"], 1)
    out = dict(setting=setting, seconds=round(dt, 4), iterations_per_s=round(its / dt, 3),
               ms_per_iteration=round(dt / its * 1e3, 2), moves_per_s=round(d["moves"] * a.games / dt, 1),
               steps_per_s=round(d["train_steps"] / dt, 2), games=d["games"], slices=d["slices"],
               reanalysed_games=d.get("reanalysed_games", 0), reanalysed_positions=d.get("reanalysed_positions", 0),
               reanalysed_positions_per_s=round(d.get("reanalysed_positions", 0) / dt, 1))
    if label:
        out["label"] = label
    emit(json.dumps(out))
    gc.collect()
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=15)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=360)
    ap.add_argument("--buffer", type=int, default=65536)
    ap.add_argument("--prefill", type=int, default=4096)
    ap.add_argument("--openings", type=int, default=80)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--ra-games", type=int, default=1024, help="rows of the re-analysis engine (a search chunk)")
    ap.add_argument("--ra-positions", type=int, default=1024, help="positions one pass holds at most")
    ap.add_argument("--concurrent", action="store_true", help="the trainer on its own HIP stream (loop_c4_concurrent)")
    ap.add_argument("--host-ingest", action="store_true", help="finished games through the host instead of gmz_replay_ingest")
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
    emit("# tools/reanalyse_ab.py %s on %s" % (" ".join(sys.argv[1:]), torch.cuda.get_device_name(0)))
    run(a, "device", emit, label="warm-up, not counted", iters=max(2, a.iters // 4))
    res = {s: [] for s in SETTINGS}
    for _ in range(a.rounds):
        for s in SETTINGS:
            res[s].append(run(a, s, emit))
    ms = {s: [r["ms_per_iteration"] for r in res[s]] for s in SETTINGS}
    off = float(np.mean(ms["off"]))
    summary = dict(
        iterations_per_s={s: [r["iterations_per_s"] for r in res[s]] for s in SETTINGS},
        ms_per_iteration=ms, off_spread_ms=round(max(ms["off"]) - min(ms["off"]), 2),
        off_spread_percent=round(100 * (max(ms["off"]) - min(ms["off"])) / off, 2),
        reanalysed_positions_per_s={s: [r["reanalysed_positions_per_s"] for r in res[s]] for s in ("host", "device")},
        positions_per_pass={s: [round(r["reanalysed_positions"] / a.iters, 1) for r in res[s]] for s in ("host", "device")},
        pass_ms_beside_a_move={s: [round(x - off, 2) for x in ms[s]] for s in ("host", "device")},
        device_over_host_percent=[round(100 * (h / d - 1), 2) for h, d in zip(ms["host"], ms["device"])])
    emit(json.dumps(summary))


if __name__ == "__main__":
    main()
