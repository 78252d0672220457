"""Arena throughput: moves/s of arena.Arena in its steady state (every slot busy), one network against itself or
against an anchor opponent, at the headline's shape (15x15, 400 simulations, 1,024 slots, 8 blocks, fp16) — to set
beside ``python bench.py``'s self-play headline on the same GPU (profiles/arena.txt, profiles/arena_anchor.txt).

  python tools/arena_bench.py [--streams 1,2 --steps 10 --warmup 3 --rounds 2] [--b anchor:threat]
  python tools/arena_bench.py --b anchor:vcf [--anchor-depth 10 --anchor-nodes 2048]
  python tools/arena_bench.py --b anchor:threat,anchor:ab [--anchor-plies 4 --anchor-width 8]   (alternated)
  python tools/arena_bench.py --anchor-launch 200      (the anchor launch alone, by event timing)
  python tools/arena_bench.py --vcf-launch 50          (the solver launch alone, on positions of threat-anchor games)
  python tools/arena_bench.py --ab-launch 20           (the alpha-beta launch alone, on the same positions)

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


def measure(cfg, sd, slots, streams, steps, warmup, precision, seed, side_b="self", depth=None, nodes=None, plies=None,
            width=None):
    anchor = AR.anchor_from_name(side_b, depth=depth, nodes=nodes, plies=plies, width=width)
    nets = [N.GomokuNetHip(sd, cfg, num_slots=E.hidden_slots(cfg, slots), max_rows=slots, precision=precision)
            for _ in range(1 if anchor else 2)]
    # 8 games per slot: against the threat anchor a game lasts some 8 plies, so the default 13 plies finish fewer
    book = AR.paired_openings(4 * slots, cfg.BOARD_SIZE, seed)
    ar = AR.Arena(cfg, nets[0], anchor or nets[1], slots, book, seed=seed, streams=streams)
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
    out = dict(b=side_b, streams=streams, slots=slots, steps=steps, moves=moves, seconds=round(dt, 4),
               moves_per_s=round(moves / dt, 1), finished=int(ar.match.finished[0]),
               waves_last=[e.waves_last for e in ar.engines])
    ar.close()
    return out


def timed_launches(fn, warmup, reps):
    """Microseconds per call of ``fn``, by two HIP events around ``reps`` calls after ``warmup`` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return round(1000.0 * ev[0].elapsed_time(ev[1]) / reps, 2)


def launch_then_slowest(search, b, p, warmup, reps, out):
    """One ``search(boards, players)`` launch for its results (the fourth: nodes per board), then into ``out`` its time
    on all boards and on the board of the most nodes alone, which bounds what one wave holds.  Returns the results."""
    res = search(b, p)
    out["us_per_launch"] = timed_launches(lambda: search(b, p), warmup, reps)
    worst = int(res[3].argmax())
    bw, pw = b[worst:worst + 1], p[worst:worst + 1]
    out["us_slowest_board_alone"] = timed_launches(lambda: search(bw, pw), warmup, reps)
    return res


def anchor_launch(size, boards, reps, seed):
    """Microseconds per gmz_game_anchor_move launch on ``boards`` mid-game boards, by HIP events over ``reps``
    launches (threat rule with Gumbel noise, and the uniform rule)."""
    import numpy as np
    rs = np.random.RandomState(seed)
    b, p, _, _ = E.random_openings(boards, size, rs, 60)
    b, p = torch.from_numpy(b).cuda(), torch.from_numpy(p).cuda()
    noise = torch.from_numpy(rs.gumbel(0, 1, (boards, size * size))).cuda()
    out = dict(size=size, boards=boards, reps=reps)
    for kind, scale in (("threat", 0.0), ("uniform", 1.0)):
        out["us_per_launch_" + kind] = timed_launches(lambda: E.anchor_move(b, p, noise, kind, scale), 10, reps)
    return out


def threat_positions(size, boards, seed, scale=3e3):
    """``boards`` positions taken from games between two threat anchors (noise ``scale``, from the empty board, played
    by the numpy model tests/vcf_ref.py), on the device: (boards int8 [boards, size, size], players int8 [boards])."""
    import numpy as np
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import vcf_ref  # the numpy model: its games are the positions (tests/test_vcf_gpu.py uses the same)
    games, bb, pp = 0, np.zeros((0, size * size), np.int8), np.zeros(0, np.int8)
    while bb.shape[0] < boards:
        games += max(boards // 32, 1)
        bb, pp = vcf_ref.threat_game_positions(size, 5, games, seed, scale)
    b = torch.from_numpy(bb[:boards].reshape(boards, size, size).copy()).cuda()
    return b, torch.from_numpy(pp[:boards].copy()).cuda()


def ab_launch(size, boards, reps, seed, plies, width, nodes):
    """Microseconds per gmz_game_alphabeta launch on the positions of threat_positions, by HIP events over ``reps``
    launches; the same launch on the slowest board alone; and the node counts, whose largest bounds the launch."""
    import numpy as np
    b, p = threat_positions(size, boards, seed)
    out = dict(size=size, boards=boards, reps=reps, plies=plies, width=width, nodes=nodes)
    st, _, val, nd = launch_then_slowest(lambda bb, pp: E.alphabeta(bb, pp, plies, width, nodes), b, p, 2, reps, out)
    nd, val = nd.cpu().numpy(), val.cpu().numpy()
    out.update(searched=int((st == 0).sum()), at_budget=int((st == 2).sum()), wins=int((val >= (1 << 39)).sum()),
               losses=int((val <= -(1 << 39)).sum()), nodes_mean=round(float(nd.mean()), 2),
               nodes_p99=int(np.percentile(nd, 99)), nodes_max=int(nd.max()))
    out["us_per_node_slowest_board"] = round(out["us_slowest_board_alone"] / max(int(nd.max()), 1), 3)
    return out


def vcf_launch(size, boards, reps, seed, depth, nodes, scale=3e3):
    """Microseconds per gmz_game_vcf launch on ``boards`` positions taken from games between two threat anchors
    (noise scale 3e3, from the empty board, played by the numpy model tests/vcf_ref.py), by HIP events over ``reps``
    launches; and the same launch on the slowest board alone."""
    import numpy as np
    b, p = threat_positions(size, boards, seed, scale)
    out = dict(size=size, boards=boards, reps=reps, depth=depth, nodes=nodes)
    st, _, ln, nd = launch_then_slowest(lambda bb, pp: E.vcf(bb, pp, depth, nodes), b, p, 3, reps, out)
    nd = nd.cpu().numpy()
    out.update(wins=int((st == 1).sum()), wins_len3=int(((st == 1) & (ln >= 3)).sum()), at_budget=int((st == 2).sum()),
               nodes_mean=round(float(nd.mean()), 2), nodes_p99=int(np.percentile(nd, 99)), nodes_max=int(nd.max()))
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
    ap.add_argument("--b", default="self", help="side B: 'self' (the network against itself), anchor:threat, "
                                                "anchor:uniform, anchor:vcf or anchor:ab; a comma-separated list "
                                                "runs its sides in turn in every round (alternated runs)")
    ap.add_argument("--anchor-launch", type=int, default=0, metavar="REPS",
                    help="time the anchor launch alone on --slots boards over REPS launches, and stop")
    ap.add_argument("--anchor-depth", type=int, default=None, help="anchor:vcf / anchor:ab: attacker moves looked ahead (10)")
    ap.add_argument("--anchor-nodes", type=int, default=None, help="anchor:vcf / anchor:ab: node budget per board (2048)")
    ap.add_argument("--anchor-plies", type=int, default=None, help="anchor:ab: plies looked ahead (4)")
    ap.add_argument("--anchor-width", type=int, default=None, help="anchor:ab: candidates per node (8)")
    ap.add_argument("--ab-launch", type=int, default=0, metavar="REPS",
                    help="time the alpha-beta launch alone on --slots positions over REPS launches, and stop")
    ap.add_argument("--vcf-launch", type=int, default=0, metavar="REPS",
                    help="time the solver launch alone on --slots positions over REPS launches, and stop")
    a = ap.parse_args()
    if a.vcf_launch:
        print(json.dumps(vcf_launch(a.size, a.slots, a.vcf_launch, a.seed, a.anchor_depth or E.VCF_DEPTH,
                                    a.anchor_nodes or E.VCF_NODES)), flush=True)
        return
    if a.ab_launch:
        print(json.dumps(ab_launch(a.size, a.slots, a.ab_launch, a.seed, a.anchor_plies or E.AB_PLIES,
                                   a.anchor_width or E.AB_WIDTH, a.anchor_nodes or E.AB_NODES)), flush=True)
        return
    if a.anchor_launch:
        print(json.dumps(anchor_launch(a.size, a.slots, a.anchor_launch, a.seed)), flush=True)
        return
    cfg = GmzConfig(BOARD_SIZE=a.size, NUM_SIMULATIONS=a.sims, NUM_RES_BLOCKS=a.blocks)
    sd = W.synthetic_state_dict(cfg, seed=a.seed, with_projection=False)
    for r in range(a.rounds):
        for side_b in a.b.split(","):
            for s in [int(x) for x in a.streams.split(",")]:
                out = measure(cfg, sd, a.slots, s, a.steps, a.warmup, a.precision, a.seed, side_b, a.anchor_depth,
                              a.anchor_nodes, a.anchor_plies, a.anchor_width)
                out["round"] = r
                print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
