"""Host ingest against device ingest of finished games in the C4 loop (loop.C4Loop(device_ingest=...)), A/B in one
process on one GPU at C4's own workload: 15x15, 400 simulations, 1,024 games from staggered openings, 8 blocks,
B = 360, PER, a prefilled shard (bench.py's loop leg, driven through the same loop.run_c4).

  python tools/ingest_ab.py [--pairs 3 --iters 20 --warmup 6 --out profiles/replay_ingest_ab.txt]

After one untimed warm-up run, each setting (self-play + ingest only: train_steps_per_iter = 0; the bench's default
loop: one trainer step per move) runs host and device ingest alternated ``--pairs`` times; run_c4 times its window
with a host clock around a device synchronise.  A last device-ingest run brackets every gmz_replay_ingest call (the
job table's copy and the launch) with device events and reports their times and the finished games per move.
One JSON line per run, then a summary."""
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

from datou_gomoku_muzero_amd import loop as LP, replay as RP  # noqa: E402


def namespace(a, train_per_iter, device_ingest, iters=None):
    return SimpleNamespace(size=a.size, sims=a.sims, blocks=a.blocks, trainer_batch=a.batch, loop_buffer=a.buffer,
                           loop_update_interval=1000, loop_openings=a.openings, loop_games=a.games, seed=a.seed,
                           precision="fp16", loop_prefill=a.prefill, loop_moves_per_iter=1,
                           loop_train_per_iter=train_per_iter, loop_concurrent=a.concurrent, loop_warmup=a.warmup,
                           loop_iters=a.iters if iters is None else iters, loop_device_ingest=device_ingest)


def run(a, train_per_iter, device_ingest, emit, label=None, iters=None):
    d, dt = LP.run_c4(namespace(a, train_per_iter, device_ingest, iters), 0, 1, None, None, log=lambda s: None)
    out = dict(mode="device" if device_ingest else "host", train_steps_per_iter=train_per_iter, seconds=round(dt, 4),
               moves_per_s=round(d["moves"] * a.games / dt, 1), steps_per_s=round(d["train_steps"] / dt, 2),
               ms_per_move=round(dt / max(d["moves"], 1) * 1e3, 2), moves=d["moves"], games=d["games"],
               slices=d["slices"], games_per_move=round(d["games"] / max(d["moves"], 1), 2))
    if label:
        out["label"] = label
    emit(json.dumps(out))
    gc.collect()
    torch.cuda.empty_cache()
    return out


def timed_ingest(a, emit):
    """One device-ingest run with every ReplayBuffer.ingest_history call between two device events."""
    marks = []
    ingest = RP.ReplayBuffer.ingest_history

    def bracketed(self, hist, sn, games=None):
        st = torch.cuda.current_stream(hist.dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        got = ingest(self, hist, sn, games=games)
        e1.record(st)
        marks.append((e0, e1, len(got), sum(x[2] for x in got)))
        return got
    RP.ReplayBuffer.ingest_history = bracketed
    try:
        run(a, 1, True, emit, label="ingest bracketed by device events")
    finally:
        RP.ReplayBuffer.ingest_history = ingest
    torch.cuda.synchronize()
    rows = [(e0.elapsed_time(e1) * 1e3, g, s) for (e0, e1, g, s) in marks if g > 0]
    if rows:
        us = np.array([r[0] for r in rows])
        emit(json.dumps(dict(ingest_calls=len(rows), ingest_us_median=round(float(np.median(us)), 1),
                             ingest_us_min=round(float(us.min()), 1), ingest_us_max=round(float(us.max()), 1),
                             games_per_call_mean=round(float(np.mean([r[1] for r in rows])), 2),
                             slices_per_call_mean=round(float(np.mean([r[2] for r in rows])), 1))))


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
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--concurrent", action="store_true", help="the trainer on its own HIP stream (loop_c4_concurrent)")
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
    emit("# tools/ingest_ab.py %s on %s" % (" ".join(sys.argv[1:]), torch.cuda.get_device_name(0)))
    run(a, 1, False, emit, label="warm-up, not counted", iters=max(2, a.iters // 4))
    summary = []
    for tpi in (0, 1):
        res = {"host": [], "device": []}
        for _ in range(a.pairs):
            for dev in (False, True):
                r = run(a, tpi, dev, emit)
                res[r["mode"]].append(r)
        h = [r["moves_per_s"] for r in res["host"]]
        d = [r["moves_per_s"] for r in res["device"]]
        summary.append(dict(train_steps_per_iter=tpi, host_moves_per_s=h, device_moves_per_s=d,
                            host_spread=round(max(h) - min(h), 1), device_spread=round(max(d) - min(d), 1),
                            pair_gain_percent=[round(100 * (y / x - 1), 2) for x, y in zip(h, d)],
                            host_steps_per_s=[r["steps_per_s"] for r in res["host"]],
                            device_steps_per_s=[r["steps_per_s"] for r in res["device"]],
                            games_per_move=round(float(np.mean([r["games_per_move"] for r in res["host"] + res["device"]])), 2)))
    timed_ingest(a, emit)
    for s in summary:
        emit(json.dumps(s))


if __name__ == "__main__":
    main()
