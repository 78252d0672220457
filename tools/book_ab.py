"""Self-play that restarts finished games from an opening book (loop.SelfPlay(book=...), engine.set_book /
gmz_engine_play_book) against empty-board restarts, A/B in one process on one GPU at the headline self-play shape:
15x15, 400 simulations, 1,024 games on two HIP streams, 8 blocks, fp16.

  python tools/book_ab.py [--rounds 3 --moves 20 --warmup 40 --out profiles/book_selfplay.txt]

The book is paired_openings(--book, size, seed) without the rows check_selfplay_book's win rule excludes.  Two SelfPlay
instances with the same weights and seed: one restarts from the book, one from the empty board (its first games too).
After --warmup untimed moves of each (long enough that games end in the timed windows), they run --moves timed moves
alternated --rounds times (a host clock around a device synchronise).  Per run: moves/s (games x moves / s) and the
games that finished in the window.  One JSON line per run, then a summary with the ratio of the rates per round and the
spread of the empty-board rounds, the yardstick.  Last, the launches alone on one 512-game part, device events around
--launches launches each: gmz_engine_play and gmz_engine_play_book with every action -1 (no slot restarts), and
gmz_engine_play_book with every slot restarting (its serial array refilled with -1 before each launch; the refill is
timed alone too, and subtracted)."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from datou_gomoku_muzero_amd import loop as LP, openings as O, weights as W  # noqa: E402
from datou_gomoku_muzero_amd._lib import check, ptr  # noqa: E402
from datou_gomoku_muzero_amd.config import GmzConfig  # noqa: E402


def timed(sp, moves):
    torch.cuda.synchronize()
    done = 0
    t0 = time.perf_counter()
    for _ in range(moves):
        done += len(sp.step())
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dict(seconds=round(dt, 4), moves_per_s=round(sp.G * moves / dt, 1), ms_per_move=round(dt / moves * 1e3, 2),
                games_finished=done)


def event_us(fn, n):
    """Mean microseconds per call of ``fn`` over ``n`` calls on the current stream, by device events."""
    for _ in range(10):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return round(a.elapsed_time(b) * 1e3 / n, 3)


def launches(eng, n):
    """The play launches alone on ``eng`` (a BatchedSelfPlayEngine with a book): see the module docstring."""
    none = torch.full((eng.G,), -1, dtype=torch.int32, device=eng.device)
    serial = eng._book["slot_serial"]
    s = eng._stream()
    out = dict(games=eng.G, launches=n)
    out["k_play_engine_us"] = event_us(
        lambda: check(eng.lib.gmz_engine_play(eng.handle, ptr(none), ptr(eng.status), 1, s)), n)
    out["k_play_book_no_restart_us"] = event_us(lambda: eng._play_book(none, s), n)
    out["serial_refill_us"] = event_us(lambda: serial.fill_(-1), n)

    def refill_and_play():
        serial.fill_(-1)
        eng._play_book(none, s)
    both = event_us(refill_and_play, n)
    out["k_play_book_every_slot_restarts_us"] = round(both - out["serial_refill_us"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=15)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--streams", type=int, default=2)
    ap.add_argument("--book", type=int, default=2048, help="openings drawn before the win rule filters them")
    ap.add_argument("--moves", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=300)
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
        sys.exit("tools/book_ab.py needs a GPU")
    emit("# tools/book_ab.py %s on %s" % (" ".join(sys.argv[1:]), torch.cuda.get_device_name(0)))
    cfg = GmzConfig(BOARD_SIZE=a.size, NUM_SIMULATIONS=a.sims, NUM_RES_BLOCKS=a.blocks)
    book = O.paired_openings(a.book, a.size, a.seed, n_in_row=cfg.N_IN_ROW)
    book = O.check_selfplay_book(tuple(x[O.selfplay_book_rows(book, cfg)] for x in book), cfg)
    emit(json.dumps(dict(book_openings=int(len(book[1])), drawn=a.book,
                         stones={int(k): int((book[3] == k).sum()) for k in np.unique(book[3])})))
    sd = W.synthetic_state_dict(cfg, seed=1, with_projection=False)
    sps = {}
    for name, kw in (("empty", {}), ("book", dict(book=book))):
        sps[name] = LP.SelfPlay(cfg, a.games, sd, seed=a.seed, streams=a.streams, **kw)
        for _ in range(a.warmup):
            sps[name].step()
        torch.cuda.synchronize()
    res = {"empty": [], "book": []}
    for r in range(a.rounds):
        for name in (("empty", "book") if r % 2 == 0 else ("book", "empty")):  # the order in a round alternates
            out = timed(sps[name], a.moves)
            out.update(mode=name, round=r)
            res[name].append(out)
            emit(json.dumps(out))
    e = [x["moves_per_s"] for x in res["empty"]]
    b = [x["moves_per_s"] for x in res["book"]]
    tally = sps["book"].book_tally().cpu().numpy()
    emit(json.dumps(dict(games=a.games, sims=a.sims, streams=a.streams, warmup=a.warmup, moves=a.moves,
                         empty_moves_per_s=e, book_moves_per_s=b,
                         book_over_empty=[round(y / x, 4) for x, y in zip(e, b)],
                         book_over_empty_mean=round(float(np.mean(b) / np.mean(e)), 4),
                         empty_spread=round((max(e) - min(e)) / float(np.mean(e)), 4),
                         empty_games_finished=[x["games_finished"] for x in res["empty"]],
                         book_games_finished=[x["games_finished"] for x in res["book"]],
                         book_tally_black_white_draw=tally.sum(0).tolist())))
    part = getattr(sps["book"].eng, "engines", [sps["book"].eng])[0]
    emit(json.dumps(launches(part, a.launches)))
    for sp in sps.values():
        for eng in getattr(sp.eng, "engines", [sp.eng]):
            assert eng.errors() == 0
        sp.close()


if __name__ == "__main__":
    main()
