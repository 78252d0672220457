"""The weight push (trainer parameters -> the self-play network's packed buffers), host path against device path, A/B
in one process on one GPU at C4's shape: 15x15, 8 blocks, fp16.

  python tools/weights_ab.py [--pairs 3 --loop --out profiles/weights_push_ab.txt]

Part 1, the push alone, alternated ``--pairs`` times after one untimed pass of each:
  host     Trainer.state_dict_cpu() + GomokuNetHip.load_state_dict(), host wall time up to a device synchronise (what
           loop.C4Loop.push_weights costs without device_weights: ~150 device-to-host copies, numpy's fold and
           fragment permutations, 19 uploads from pageable memory);
  device   Trainer.device_state_dict() + GomokuNetHip.load_device_state_dict(): the GPU time between two HIP events
           around the call on an idle stream (gmz_net_pack's three launches plus the host's part of the call, which
           the idle GPU waits for), the host wall time of the call itself (no synchronise inside: it returns when
           the launches are queued), and the three launches alone (the same events behind a few ms of queued work);
  copy     the yardstick: one device-to-device copy_ whose traffic (bytes read + bytes written) equals the pack's
           (the float32 sources it reads + the packed buffers it writes), by HIP events.
Acceptance: in every pair both device figures are below the host figure.

Part 2 (``--loop``), the C4 loop through loop.run_c4 (bench.py's loop leg) with the host push and with the device push,
at model_update_interval 1000 (the reference's: no push inside the window, the rates must be neutral) and 1 (a push
after every trainer step), alternated ``--rounds`` times: self-play moves/s and trainer steps/s.  One JSON line per
measurement, then a summary."""
import argparse
import gc
import json
import os
import sys
import time
from types import SimpleNamespace

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from datou_gomoku_muzero_amd import loop as LP, network as N, trainer as T  # noqa: E402
from datou_gomoku_muzero_amd.config import GmzConfig  # noqa: E402


def event_ms(fn, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def push_ab(a, emit):
    cfg = GmzConfig(BOARD_SIZE=a.size, NUM_RES_BLOCKS=a.blocks)
    tcfg = T.TrainConfig(BOARD_SIZE=a.size, NUM_RES_BLOCKS=a.blocks)
    tr = T.Trainer(tcfg, device="cuda", graph=False)
    net = N.GomokuNetHip(tr.state_dict_cpu(), cfg, precision=a.precision)
    dsd = tr.device_state_dict()
    read = sum(dsd[k].numel() * 4 for k, _ in N.device_pack_sources(cfg))
    written = sum(t.numel() * t.element_size() for t in net._tensors.values())
    half = (read + written) // 2
    src = torch.empty(half, dtype=torch.uint8, device="cuda")
    dst = torch.empty(half, dtype=torch.uint8, device="cuda")
    busy = torch.randn(8192, 8192, dtype=torch.float16, device="cuda")
    busy_out = torch.empty_like(busy)

    def host():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        net.load_state_dict(tr.state_dict_cpu())
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def device():
        wall = []

        def call():
            t0 = time.perf_counter()
            net.load_device_state_dict(tr.device_state_dict())
            wall.append((time.perf_counter() - t0) * 1e3)
        gpu = event_ms(call)
        # the launches alone: queued behind a few ms of other work, so the first event's time stamp is taken when
        # the three launches already wait in the stream and the host's part of the call is not inside the interval
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        for _ in range(8):
            torch.mm(busy, busy, out=busy_out)
        e0.record()
        net.load_device_state_dict(tr.device_state_dict())
        e1.record()
        torch.cuda.synchronize()
        return gpu, wall[0], e0.elapsed_time(e1)

    host(), device(), event_ms(lambda: dst.copy_(src))  # untimed: the job table, the allocator, the code objects
    pairs = []
    for i in range(a.pairs):
        h = host()
        g, w, k = device()
        c = event_ms(lambda: dst.copy_(src), reps=5)
        pairs.append(dict(pair=i, host_wall_ms=round(h, 3), device_gpu_ms=round(g, 4), device_host_wall_ms=round(w, 4),
                          device_kernels_ms=round(k, 4), copy_gpu_ms=round(c, 4),
                          device_gb_per_s=round((read + written) / k / 1e6, 1),
                          copy_gb_per_s=round(2 * half / c / 1e6, 1), kernels_over_copy=round(k / c, 2),
                          host_over_device_gpu=round(h / g, 1)))
        emit(json.dumps(pairs[-1]))
    ok = all(p["device_gpu_ms"] < p["host_wall_ms"] and p["device_host_wall_ms"] < p["host_wall_ms"] for p in pairs)
    emit(json.dumps(dict(push=dict(bytes_read=read, bytes_written=written, launches=3, pairs=len(pairs),
                                   device_below_host_in_every_pair=ok))))
    del tr, net
    gc.collect()
    torch.cuda.empty_cache()
    return ok


def loop_ab(a, emit):
    def run(interval, device_weights, label=None):
        ns = SimpleNamespace(size=a.size, sims=a.sims, blocks=a.blocks, trainer_batch=a.batch, loop_buffer=a.buffer,
                             loop_update_interval=interval, loop_openings=a.openings, loop_games=a.games, seed=a.seed,
                             precision=a.precision, loop_prefill=a.prefill, loop_moves_per_iter=1, loop_train_per_iter=1,
                             loop_concurrent=a.concurrent, loop_warmup=a.warmup, loop_iters=a.iters,
                             loop_device_ingest=True, loop_device_batches=a.device_batches, loop_device_weights=device_weights)
        d, dt = LP.run_c4(ns, 0, 1, None, None, log=lambda s: None)
        out = dict(interval=interval, push="device" if device_weights else "host", seconds=round(dt, 4),
                   moves_per_s=round(d["moves"] * a.games / dt, 1), steps_per_s=round(d["train_steps"] / dt, 2),
                   weight_pushes=d["weight_pushes"], push_ms_alone=round(d["push_ms"], 3))
        if label:
            out["label"] = label
        emit(json.dumps(out))
        gc.collect()
        torch.cuda.empty_cache()
        return out

    run(1, True, label="warm-up, not counted")
    res = {}
    for r in range(a.rounds):
        for interval in (1000, 1):
            for dw in ((False, True) if r % 2 == 0 else (True, False)):  # the order inside a pair alternates
                res.setdefault((interval, dw), []).append(run(interval, dw))
    summary = {}
    for interval in (1000, 1):
        h, d = res[(interval, False)], res[(interval, True)]
        for k in ("moves_per_s", "steps_per_s"):
            hv, dv = [r[k] for r in h], [r[k] for r in d]
            summary["interval_%d_%s" % (interval, k)] = dict(
                host=hv, device=dv, host_spread_percent=round(100 * (max(hv) - min(hv)) / np.mean(hv), 2),
                device_over_host_percent=round(100 * (np.mean(dv) / np.mean(hv) - 1), 2))
    emit(json.dumps(summary))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=15)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--loop", action="store_true", help="also the loop A/B (part 2)")
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=360)
    ap.add_argument("--buffer", type=int, default=65536)
    ap.add_argument("--prefill", type=int, default=4096)
    ap.add_argument("--openings", type=int, default=80)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--concurrent", action="store_true", help="the trainer on its own HIP stream")
    ap.add_argument("--device-batches", action="store_true", help="training batches by gmz_replay_gather too")
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
    emit("# tools/weights_ab.py %s on %s" % (" ".join(sys.argv[1:]), torch.cuda.get_device_name(0)))
    ok = push_ab(a, emit)
    if a.loop:
        loop_ab(a, emit)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
