"""Dynamics-tower time per board size (profiles/tower_board_sizes.txt): for every size 5..19, the HIP tower's time
per launch of 1,024 rows (f16, 8 blocks; HIP events around the tower launch alone, network.KernelTimer) after
warm-up, over about a second of launches, the four original sizes measured a second time at the end for the
spread; then PyTorch's fp16 channels-last forward of the same tower (BatchNorm folded into the convs: its fastest
eager form) at 8, 11 and 13.

    python tools/tower_board_sizes.py [--out FILE] [--sizes 5,6,...] [--torch-sizes 8,11,13]
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from datou_gomoku_muzero_amd import _lib, network as N, weights as W  # noqa: E402
from datou_gomoku_muzero_amd.config import GmzConfig  # noqa: E402

ROWS, BLOCKS = 1024, 8
PARENT = (6, 9, 15, 19)  # the original sizes; every other size must not be slower than the next larger one of them
NEXT_PARENT ={5: 6, 7: 9, 8: 9, 10: 15, 11: 15, 12: 15, 13: 15, 14: 15, 16: 19, 17: 19, 18: 19}


def flops(size):
    return ROWS * (1 + 2 * BLOCKS) * size * size * 128 * 128 * 9 * 2.0


def hip_tower_ms(size, seconds=1.0):
    cfg = GmzConfig(BOARD_SIZE=size, NUM_RES_BLOCKS=BLOCKS)
    sd = W.synthetic_state_dict(cfg, seed=size, with_projection=False)
    net = N.GomokuNetHip(sd, cfg, num_slots=2 * ROWS, max_rows=ROWS)
    A = size * size
    g = torch.Generator(device="cuda").manual_seed(size)
    h = torch.rand(ROWS * A * 128, generator=g, device="cuda").half()  # non-negative, like a ReLU output
    net.pool[:ROWS * A * 128] = h.view(torch.int16)
    i_s = torch.arange(ROWS, dtype=torch.int32, device="cuda")
    o_s = i_s + ROWS
    act = torch.randint(0, A, (ROWS,), generator=g, device="cuda", dtype=torch.int32)
    lg = torch.empty(ROWS, A, device="cuda")
    v, r = torch.empty(ROWS, device="cuda"), torch.empty(ROWS, device="cuda")
    st = _lib.stream_ptr()
    net.tower_timer = N.KernelTimer()
    for _ in range(5):
        net.recurrent(i_s, act, o_s, lg, v, r, st)
    torch.cuda.synchronize()
    _, warm, _ = net.tower_timer.summary()
    net.tower_timer.reset()
    n = int(min(4000, max(20, seconds * 1000.0 / max(warm, 1e-3))))
    for _ in range(n):
        net.recurrent(i_s, act, o_s, lg, v, r, st)
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b, _ in net.tower_timer.pairs)
    assert torch.isfinite(lg).all()
    return n, sum(ms) / n, ms[n // 2], ms[0]


def torch_tower_ms(size, seconds=1.0):
    cfg = GmzConfig(BOARD_SIZE=size, NUM_RES_BLOCKS=BLOCKS)
    sd = W.synthetic_state_dict(cfg, seed=size, with_projection=False)

    def folded(conv, bn):
        s, b = N.fold_bn(sd, bn)
        w = torch.from_numpy(np.asarray(sd[conv], np.float32) * s[:, None, None, None])
        return (w.cuda().half().contiguous(memory_format=torch.channels_last), torch.from_numpy(b).cuda().half())

    stem = folded("dynamics_net.conv.weight", "dynamics_net.bn")
    blocks = [(folded("dynamics_net.resblocks.%d.conv1.weight" % i, "dynamics_net.resblocks.%d.bn1" % i),
               folded("dynamics_net.resblocks.%d.conv2.weight" % i, "dynamics_net.resblocks.%d.bn2" % i))
              for i in range(BLOCKS)]
    emb = torch.from_numpy(np.asarray(sd["dynamics_net.action_embed_conv.weight"], np.float32)).cuda().half()
    A = size * size
    g = torch.Generator(device="cuda").manual_seed(size)
    h = torch.rand(ROWS, 128, size, size, generator=g, device="cuda").half().contiguous(memory_format=torch.channels_last)
    act = torch.randint(0, A, (ROWS,), generator=g, device="cuda")

    @torch.no_grad()
    def forward():
        plane = F.one_hot(act, A).half().view(-1, 1, size, size)
        x = torch.cat((h, F.conv2d(plane, emb)), 1).contiguous(memory_format=torch.channels_last)
        x = F.relu(F.conv2d(x, stem[0], stem[1], padding=1))
        for (w1, b1), (w2, b2) in blocks:
            t = F.relu(F.conv2d(x, w1, b1, padding=1))
            x = F.relu(F.conv2d(t, w2, b2, padding=1) + x)
        return x

    for _ in range(5):
        forward()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    forward()
    e1.record()
    torch.cuda.synchronize()
    n = int(min(2000, max(10, seconds * 1000.0 / max(e0.elapsed_time(e1), 1e-3))))
    e0.record()
    for _ in range(n):
        forward()
    e1.record()
    torch.cuda.synchronize()
    return n, e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default=",".join(str(s) for s in N.BOARD_SIZES))
    ap.add_argument("--torch-sizes", default="8,11,13")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("# dynamics tower, %d rows per launch, f16, %d blocks (%d 3x3 convs 128->128); HIP events around the tower "
        "launch; lib %s" % (ROWS, BLOCKS, 1 + 2 * BLOCKS, os.path.basename(_lib.LIB_PATH)))
    say("# size launches  mean_ms median_ms  min_ms  TFLOP/s(mean)")
    res = {}
    sizes = [int(s) for s in args.sizes.split(",") if s]
    for size in sizes + [s for s in sizes if s in PARENT]:
        n, mean, med, mn = hip_tower_ms(size)
        res.setdefault(size, []).append(mean)
        say("%4d %8d %9.4f %9.4f %7.4f %10.1f%s" % (size, n, mean, med, mn, flops(size) / mean * 1e-9,
                                                   "   (second pass)" if len(res[size]) > 1 else ""))
    spread = max((abs(a - b) / min(a, b) for a, b in (v for v in res.values() if len(v) == 2)), default=0.0)
    say("# spread between the two passes of the original sizes: up to %.2f %%" % (100 * spread))
    for size in sizes:
        nx = NEXT_PARENT.get(size)
        if nx in res:
            ok = res[size][0] <= max(res[nx]) * (1 + spread)
            say("# %2d vs %2d: %.4f vs %.4f ms  %s" % (size, nx, res[size][0], max(res[nx]),
                                                      "ok" if ok else "SLOWER than the next larger original size"))
    for size in [int(s) for s in args.torch_sizes.split(",") if s]:
        n, ms = torch_tower_ms(size)
        say("# PyTorch fp16 channels-last tower %2dx%-2d: %.4f ms per %d rows (%d forwards)%s" % (
            size, size, ms, ROWS, n, "  = %.1f x the HIP tower" % (ms / res[size][0]) if size in res else ""))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
