"""Training batches by torch (ReplayBuffer.sample + Trainer.step) against batches in HIP (Trainer.step_from:
gmz_replay_per_sample + gmz_replay_gather), A/B in one process on one GPU at C4's trainer shape: 15x15, 8 blocks,
B = 360, PER on, a full ring; once with the bench's shard capacity (65,536) and once with the default (1,000,000).

  python tools/batch_ab.py [--pairs 3 --steps 60 --warmup 12 --out profiles/replay_batch_ab.txt]

One trainer and one ring serve both paths (step and step_from mix on one trainer).  After a warm-up that crosses the
graph capture and runs both paths, the two alternate ``--pairs`` times; each run is ``--steps`` steps followed by
update_priorities, timed by a host clock around a device synchronise (steps/s).  In every step one device event is
recorded in front of the draw and one at the start of the captured step's replay: their distance is the device time
of building the batch (the stream is in order, so the first event waits for the previous step).
One JSON line per run, then a summary per ring size."""
import argparse
import gc
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from datou_gomoku_muzero_amd import replay as RP, trainer as T, weights as W  # noqa: E402


def full_ring(cfg, capacity, seed):
    """A full device ring: 4,096 synthetic slices repeated on the device, priorities |x| + 1e-6."""
    rb = RP.ReplayBuffer(cfg, capacity=capacity, device="cuda")
    n = min(4096, capacity)
    rb.add_arrays(*W.synthetic_slices(n, cfg.BOARD_SIZE, cfg.NUM_UNROLL_STEPS, np.random.RandomState(seed)))
    for t in (rb.obs, rb.act, rb.rew, rb.pol, rb.val):
        for lo in range(n, capacity, n):
            m = min(n, capacity - lo)
            t[lo:lo + m] = t[:m]
    rb.count, rb.ptr = capacity, 0
    g = torch.Generator(device="cuda").manual_seed(seed)
    rb.prio[:] = torch.randn(capacity, device="cuda", generator=g).abs() + 1e-6
    return rb


def run(tr, rb, mode, steps, rng, marks):
    B = tr.cfg.PHYSICAL_BATCH_SIZE
    st = torch.cuda.current_stream()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record(st)
        marks.append([e0, None])
        if mode == "hip":
            logs, td, idx = tr.step_from(rb, rng, sync=False)
        else:
            batch, idx, w = rb.sample(B, rng)
            logs, td = tr.step(batch, w, sync=False)
        rb.update_priorities(idx, td)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=15)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--batch", type=int, default=360)
    ap.add_argument("--buffers", type=int, nargs="+", default=[65536, 1000000])
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--pairs", type=int, default=3)
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
    prop = torch.cuda.get_device_properties(0)
    emit("# tools/batch_ab.py %s on %s (%s, %d CUs), torch %s" % (
        " ".join(sys.argv[1:]), prop.name, getattr(prop, "gcnArchName", "?"), prop.multi_processor_count,
        torch.__version__))
    torch.backends.cudnn.benchmark = True
    torch.manual_seed(a.seed)
    np.random.seed(a.seed)
    rng = np.random.RandomState(a.seed + 1)
    for capacity in a.buffers:
        cfg = T.TrainConfig(BOARD_SIZE=a.size, NUM_RES_BLOCKS=a.blocks, PHYSICAL_BATCH_SIZE=a.batch,
                            TRAIN_BUFFER_SIZE=capacity, ENABLE_PER=True)
        tr = T.Trainer(cfg, device="cuda")
        rb = full_ring(cfg, capacity, a.seed)
        marks = []
        graph_step = tr._graph_step

        def marked():  # the start of the captured step: the batch is in the static inputs
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record(torch.cuda.current_stream())
            if marks and marks[-1][1] is None:
                marks[-1][1] = e1
            return graph_step()
        tr._graph_step = marked
        for mode in ("torch", "hip"):  # crosses the eager steps and the capture, then both paths replayed
            run(tr, rb, mode, a.warmup, rng, marks)
        res = {"torch": [], "hip": []}
        for _ in range(a.pairs):
            for mode in ("torch", "hip"):
                del marks[:]
                dt = run(tr, rb, mode, a.steps, rng, marks)
                us = np.array([e0.elapsed_time(e1) * 1e3 for e0, e1 in marks if e1 is not None])
                out = dict(buffer=capacity, mode=mode, steps=a.steps, seconds=round(dt, 4),
                           steps_per_s=round(a.steps / dt, 3), ms_per_step=round(dt / a.steps * 1e3, 3),
                           batch_us_median=round(float(np.median(us)), 1), batch_us_min=round(float(us.min()), 1),
                           batch_us_max=round(float(us.max()), 1))
                emit(json.dumps(out))
                res[mode].append(out)
        t, h = res["torch"], res["hip"]
        emit(json.dumps(dict(
            buffer=capacity, torch_steps_per_s=[r["steps_per_s"] for r in t], hip_steps_per_s=[r["steps_per_s"] for r in h],
            torch_spread=round(max(r["steps_per_s"] for r in t) - min(r["steps_per_s"] for r in t), 3),
            hip_spread=round(max(r["steps_per_s"] for r in h) - min(r["steps_per_s"] for r in h), 3),
            pair_gain_percent=[round(100 * (y["steps_per_s"] / x["steps_per_s"] - 1), 2) for x, y in zip(t, h)],
            torch_batch_us_median=[r["batch_us_median"] for r in t], hip_batch_us_median=[r["batch_us_median"] for r in h])))
        tr._graph_step = graph_step
        del tr, rb, marks
        gc.collect()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
