"""Config C4: the reference's full loop — self-play, replay, training, weight push — on N GPUs.

The reference runs it as a process graph (main.py:91-109): NUM_WORKERS ``universal_worker`` +
one ``inference_server_worker`` for self-play, a ``data_loader_worker`` owning the PER replay buffer
(workers.py:379-439, replay_buffer.py:44-106) and one ``training_worker`` (workers.py:445-628) that
pushes ``ModelWeightsUpdate`` to the inference server every MODEL_UPDATE_INTERVAL steps
(workers.py:587-593).  Here, one process per GPU (rank r of N) holds ALL of those roles for its
own share of the work, time-sliced on its GPU:

  self-play   G games on the HIP engine (engine.BatchedSelfPlayEngine + network.GomokuNetHip), the
              move history kept on the device and harvested one move behind (worker.GameHistory);
  replay      every finished game becomes the reference's TrainingSlices (records.py semantics,
              built as arrays by ``replay.slices_from_game``) appended to THIS rank's device-resident
              replay shard (replay.ReplayBuffer) — no data crosses ranks; ``device_ingest=True``: the
              slices go from the device history into the shard by one HIP launch per move
              (gmz_replay_ingest, bit-identical; nothing but a job table crosses the bus);
              ``device_batches=True``: a training batch goes from the shard into the trainer's inputs by the
              PER draw and one gather launch in HIP (gmz_replay_per_sample, gmz_replay_gather; Trainer.step_from);
  re-analysis ``reanalyser`` (reanalysis.RingReanalyser) and ``reanalyse_per_iter`` > 0: after an iteration's moves
              that many passes search the shard's oldest-searched games again with the current network and
              rewrite their policy and value targets in the ring (MuZero Reanalyse; off by default); each rank
              re-analyses its own shard, no collectives;
  training    data-parallel: each rank samples its batch from its own shard; gradients are averaged
              by one flat-bucket all-reduce per step (RCCL over xGMI); PER (sharded):
              IS weights from the global slice count (all-reduce SUM) normalised by the global batch
              max (all-reduce MAX), the admission priority kept global (all-reduce MAX);
  weight push every ``model_update_interval`` trainer steps rank 0's weights are broadcast (one flat
              fp32 bucket, weight_sync.broadcast_state_dict) and every rank hot-swaps them into its
              inference network, as the inference server does on ModelWeightsUpdate; ``device_weights=True``
              (one rank): the trainer's live parameters are folded and packed into the inference networks'
              buffers by three HIP launches (gmz_net_pack, bit-identical), ordered by stream events, with no
              host wait and no host copy.

One *iteration* = ``moves_per_iter`` self-play moves of all G games, then ``train_steps_per_iter``
trainer steps (all ranks together, once every shard holds a batch).  ``concurrent=True`` (GPU): the
iteration's trainer steps and replay-shard updates are enqueued on a HIP stream of their own BEFORE
its moves, so the trainer's many short kernels run beside the self-play towers instead of after them
(the reference's trainer and self-play workers also run at the same time, main.py:91-109); the host
waits for the previous iteration's training before enqueueing the next, so the backlog stays one
iteration.  The self-play source and the inference network are pluggable (``SelfPlay`` on the GPU;
tests drive the same loop on CPU with scripted games over gloo).
"""
import time

import numpy as np
import torch

from .replay import ReplayBuffer, slices_from_game
from .weight_sync import broadcast_state_dict


BUDGET_SEED = 0x5EED0B  # SelfPlay's budget draws: RandomState(seed + BUDGET_SEED), G uniforms per move


def start_from_book(eng, hist, book, symmetry=True):
    """Self-play from a book of openings: the engine restarts ended games from it on the device (set_book,
    fill_from_book) and the history learns each game's first recorded row from the host's mirror of the draw."""
    eng.set_book(book, symmetry)
    eng.fill_from_book()
    hist.set_book(lambda slots, serials: eng.book_draws(slots, serials)[2])


class SelfPlay:
    """G games on this rank's GPU (the self-play half of the worker loop, worker.py)."""

    def __init__(self, cfg, num_games, state_dict, seed=0, precision="fp16", streams=None, openings=None,
                 fast_sims=None, full_prob=1.0, book=None, book_symmetry=True):
        from . import engine as E, network as N
        from .worker import GameHistory
        c = cfg
        if book is not None and openings is not None:
            raise ValueError("SelfPlay: give book= (every game starts from the book) or openings= (the first games' "
                             "positions), not both")
        self.cfg, self.G = c, int(num_games)
        self.net = N.GomokuNetHip(state_dict, c, num_slots=E.hidden_slots(c, self.G), max_rows=self.G,
                                  precision=precision)
        self.eng = E.make_engine(c, num_games=self.G, net=self.net, seed=seed, streams=streams)
        self.eng.reset_games()
        self.hist = GameHistory(self.G, c.ACTION_SPACE_SIZE, self.eng.device, min_game_len=2 * c.N_IN_ROW - 1)
        if openings is not None:  # (boards, players, last_moves, move_counts): e.g. engine.random_openings
            self.eng.set_positions(*openings)
            self.hist.set_start(openings[3])
        if book is not None:  # (boards, players, last_moves, move_counts): every game of every slot starts from an
            # opening drawn on the device, with one of the square's eight symmetries (engine.set_book)
            start_from_book(self.eng, self.hist, book, book_symmetry)
        dev = self.eng.device
        self.missed = (torch.zeros(self.G, dtype=torch.int32, device=dev), torch.zeros(self.G, dtype=torch.int32, device=dev))
        self.pending = None
        self.moves = 0
        # playout-cap randomisation: with fast_sims set, each game searches a move with NUM_SIMULATIONS with
        # probability full_prob and with fast_sims otherwise (engine.set_budgets); every position is recorded alike
        self.fast_sims, self.full_prob = None if fast_sims is None else int(fast_sims), float(full_prob)
        if self.fast_sims is not None:
            if not 1 <= self.fast_sims <= c.NUM_SIMULATIONS:
                raise ValueError("fast_sims must be in [1, NUM_SIMULATIONS = %d]" % c.NUM_SIMULATIONS)
            if not 0.0 <= self.full_prob <= 1.0:
                raise ValueError("full_prob must be in [0, 1]")
        self.budget_rs = np.random.RandomState((int(seed) + BUDGET_SEED) % (2 ** 32))
        self.budgets = None  # the last move's simulations per game (int32 [G]); None without fast_sims
        self.ingest_buffer = self.ingest_stream = None

    def ingest_into(self, buffer, stream=None):
        """Device hand-over: from now on ``step`` / ``flush`` write finished games straight into
        ``buffer`` (replay.ReplayBuffer.ingest_history, one HIP launch per move, on ``stream`` or the
        current one) and return only their (game, winner, n_moves, missed_fives, missed_totals)."""
        self.ingest_buffer, self.ingest_stream = buffer, stream

    def _finished(self, sn):
        if self.ingest_buffer is None:
            return self.hist.harvest(sn)
        if self.ingest_stream is None:
            return self.ingest_buffer.ingest_history(self.hist, sn)
        with torch.cuda.stream(self.ingest_stream):
            return self.ingest_buffer.ingest_history(self.hist, sn)

    def step(self):
        """Play one move of every game; returns the games that finished one move earlier
        (GameHistory.harvest tuples; after ``ingest_into`` their first five fields)."""
        e, h = self.eng, self.hist
        b, p, lm, mc = e.game_state()
        if self.fast_sims is not None:
            u = self.budget_rs.random_sample(self.G)
            self.budgets = np.where(u < self.full_prob, self.cfg.NUM_SIMULATIONS, self.fast_sims).astype(np.int32)
            e.set_budgets(self.budgets)
        pol, val, act = e.search()
        e.winning_scan(b, p, act, counters=self.missed)
        h.record(b, p, lm, mc, pol, val, act)
        status = e.play(reset_finished=True)
        sn = h.after_play(status, mc, act, *self.missed)
        done = self._finished(self.pending)
        self.pending = sn
        self.moves += 1
        return done

    def flush(self):
        done = self._finished(self.pending)
        self.pending = None
        return done

    def book_tally(self):
        """Finished games per opening of the book, int32 [n, 3] on the device (black won, white won, draw); None
        without a book."""
        return self.eng.book_tally

    def load_weights(self, sd):
        self.net.load_state_dict(sd)

    def load_device_weights(self, sd):
        """Device tensors (Trainer.device_state_dict) packed in place on the current stream, no host copy."""
        self.net.load_device_state_dict(sd)

    def close(self):
        self.eng.close()


class C4Loop:
    """The composed loop on one rank (see module docstring).  ``dist``: torch.distributed or None."""

    def __init__(self, selfplay, trainer, buffer, cfg, batch_size, dist=None, moves_per_iter=1,
                 train_steps_per_iter=1, model_update_interval=1000, seed=0, device="cuda", concurrent=False,
                 device_ingest=False, device_batches=False, reanalyser=None, reanalyse_per_iter=0,
                 device_weights=False):
        self.sp, self.tr, self.rb, self.cfg = selfplay, trainer, buffer, cfg
        self.B, self.dist = int(batch_size), dist
        self.moves_per_iter, self.train_steps_per_iter = int(moves_per_iter), int(train_steps_per_iter)
        self.model_update_interval = int(model_update_interval)
        self.rank = dist.get_rank() if dist is not None else 0
        self.world = dist.get_world_size() if dist is not None else 1
        self.rs = np.random.RandomState(seed + 1000003 * self.rank)
        self.device = torch.device(device)
        self.games = self.slices = self.train_steps = self.weight_pushes = 0
        self.game_lengths = []
        self.last_logs = None
        self.concurrent = bool(concurrent) and self.device.type == "cuda"
        # concurrent mode: every replay-shard and trainer operation goes to this stream (one ordering
        # for adds, samples, steps and priority updates); the self-play engines keep theirs
        self.train_stream = torch.cuda.Stream(self.device) if self.concurrent else None
        # the self-play engines fork every move from this stream: weight swaps are enqueued on it
        self.sp_stream = torch.cuda.current_stream(self.device) if self.device.type == "cuda" else None
        self._train_done = None
        # re-analysis of the shard's own games: passes per iteration, after its moves; ring reads and writes on the
        # stream of every other ring operation, the searches on the self-play stream
        self.ra, self.reanalyse_per_iter = reanalyser, int(reanalyse_per_iter) if reanalyser is not None else 0
        self.reanalysed_games = self.reanalysed_positions = 0
        if self.ra is not None:
            self.ra.ring_stream = self.train_stream
        # device_ingest: finished games go from the self-play history to the shard in HIP (one launch per
        # move, ReplayBuffer.ingest_history) on the stream of every other ring operation; off = the host path
        self.device_ingest = bool(device_ingest)
        if self.device_ingest:
            hist = getattr(selfplay, "hist", None)  # the ring reads its finished games and banks, and hands it an event
            if not all(hasattr(hist, k) for k in ("finished", "after_ingest", "board")) \
                    or not hasattr(selfplay, "ingest_into"):
                raise ValueError("device_ingest needs a self-play source with a device history (loop.SelfPlay)")
            if self.device.type != "cuda":
                raise ValueError("device_ingest needs the loop on a GPU")
            if (cfg.BOARD_SIZE, cfg.NUM_UNROLL_STEPS, cfg.N_STEPS, cfg.DISCOUNT) != tuple(
                    getattr(buffer.cfg, k) for k in ("BOARD_SIZE", "NUM_UNROLL_STEPS", "N_STEPS", "DISCOUNT")):
                raise ValueError("device_ingest: the loop's config and the buffer's disagree on the slices' geometry")
            selfplay.ingest_into(buffer, self.train_stream)
        # device_batches: a training batch goes from the shard to the trainer's inputs in HIP (the PER draw and one
        # gather launch, Trainer.step_from); off = ReplayBuffer.sample's torch indexing and Trainer.step's copies
        self.device_batches = bool(device_batches)
        if self.device_batches:
            if self.device.type != "cuda":
                raise ValueError("device_batches needs the loop on a GPU")
            buffer.need_device("device_batches")
            if not hasattr(trainer, "step_from") or int(trainer.cfg.PHYSICAL_BATCH_SIZE) != self.B:
                raise ValueError("device_batches: the trainer steps on its PHYSICAL_BATCH_SIZE, not on a batch of %d"
                                 % self.B)

        # device_weights: a push packs the trainer's live parameters into the inference networks in HIP
        # (GomokuNetHip.load_device_state_dict), ordered between the two streams by events; off = the host path
        self.device_weights = bool(device_weights)
        if self.device_weights:
            if self.device.type != "cuda":
                raise ValueError("device_weights needs the loop on a GPU")
            if self.world > 1:
                # BatchNorm running statistics differ per rank, so rank 0's would still have to be broadcast
                raise ValueError("device_weights: a multi-rank push stays on the host path (world = %d)" % self.world)
            if not hasattr(trainer, "device_state_dict") or not hasattr(selfplay, "load_device_weights"):
                raise ValueError("device_weights needs Trainer.device_state_dict and a self-play source with "
                                 "load_device_weights (loop.SelfPlay)")

    # ---------------------------------------------------------------- pieces
    def _add_games(self, done):
        c = self.cfg
        for item in done:
            g, winner, n, mf, mt = item[:5]
            if not self.device_ingest:  # device_ingest: SelfPlay.step has written the slices already
                arrs = slices_from_game(*item[5:], winner, c.BOARD_SIZE, c.DISCOUNT, c.N_STEPS, c.NUM_UNROLL_STEPS)
                # the directory entry re-analysis reads: the stones under the first recorded position, this step
                self.rb.add_arrays(*arrs, game=(winner, int(np.count_nonzero(item[5][0])), self.train_steps))
            self.games += 1
            self.slices += n
            self.game_lengths.append(n)

    def _all_ready(self):
        """Every rank's shard holds a batch (all ranks must step together: the all-reduce)."""
        ok = 1.0 if len(self.rb) >= self.B else 0.0
        if self.dist is None or self.world == 1:
            return ok > 0
        t = torch.tensor([ok], dtype=torch.float32)
        if self.dist.get_backend() != "gloo":
            t = t.to(self.device)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MIN)
        return float(t.item()) > 0

    def push_weights(self):
        """ModelWeightsUpdate (workers.py:587-593): rank 0's trainer weights -> every rank's inference net."""
        if self.device_weights:
            return self._push_device_weights()
        if self.train_stream is not None:
            self.train_stream.synchronize()  # the step that made these weights has finished
        sd = self.tr.state_dict_cpu()
        if self.dist is not None and self.world > 1:
            dev = "cpu" if self.dist.get_backend() == "gloo" else self.device
            sd = broadcast_state_dict(sd, src=0, device=dev)
        if self.sp_stream is not None:
            # on the self-play stream, not the trainer's (concurrent mode calls this from inside the train
            # stream's context): the copies of the new weights are then ordered before the next move's
            # kernels, and after the previous move's, which join this stream.  With RCCL the broadcast
            # filled its device buffers on the CURRENT stream (the trainer's in concurrent mode), so the
            # self-play stream waits for that stream before it reads them
            cur = torch.cuda.current_stream(self.device)
            if cur != self.sp_stream:
                self.sp_stream.wait_stream(cur)
            with torch.cuda.stream(self.sp_stream):
                self.sp.load_weights(sd)
                if self.ra is not None:
                    self.ra.load_weights(sd)
        else:
            self.sp.load_weights(sd)
            if self.ra is not None:
                self.ra.load_weights(sd)
        self.weight_pushes += 1

    def _push_device_weights(self):
        """The push with no host wait and no host copy: the self-play stream waits for the step that made the weights
        (an event on the stream that step was enqueued on: the train stream in concurrent mode), packs them into
        self-play's network and the re-analyser's, and the trainer's stream waits for the packs before its next step
        may overwrite the parameters they read."""
        cur = torch.cuda.current_stream(self.device)
        sd = self.tr.device_state_dict()
        two = cur != self.sp_stream
        if two:
            made = torch.cuda.Event()
            made.record(cur)
            self.sp_stream.wait_event(made)
        with torch.cuda.stream(self.sp_stream):
            self.sp.load_device_weights(sd)
            if self.ra is not None:
                self.ra.load_device_weights(sd)
            if two:
                packed = torch.cuda.Event()
                packed.record(self.sp_stream)
        if two:
            cur.wait_event(packed)
        self.weight_pushes += 1

    def train_step(self):
        if self.device_batches:
            logs, td, idx = self.tr.step_from(self.rb, self.rs, dist=self.dist, sync=False)
        else:
            batch, idx, w = self.rb.sample(self.B, self.rs, dist=self.dist)
            logs, td = self.tr.step(batch, w, sync=False)
        self.rb.update_priorities(idx, td, dist=self.dist)
        self.last_logs = logs
        self.train_steps += 1
        self.rb.step = self.train_steps  # the version of the games ingested from now on
        if self.train_steps % self.model_update_interval == 0:
            self.push_weights()

    # ---------------------------------------------------------------- one iteration
    def iteration(self):
        if self.concurrent:
            return self._iteration_concurrent()
        for _ in range(self.moves_per_iter):
            self._add_games(self.sp.step())
        self._reanalyse()
        if self.train_steps_per_iter > 0 and self._all_ready():
            for _ in range(self.train_steps_per_iter):
                self.train_step()

    def _iteration_concurrent(self):
        ts = self.train_stream
        if self._train_done is not None:
            self._train_done.synchronize()  # the previous iteration's training: backlog <= one iteration
        if self.train_steps_per_iter > 0 and self._all_ready():
            ts.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(ts):
                for _ in range(self.train_steps_per_iter):
                    self.train_step()
        done = []
        for _ in range(self.moves_per_iter):
            done += self.sp.step()
        with torch.cuda.stream(ts):  # after this iteration's steps on the same stream
            self._add_games(done)
        self._reanalyse()  # ring work on the train stream after the adds, searches on this one
        self._train_done = torch.cuda.Event()
        self._train_done.record(ts)

    def _reanalyse(self):
        """``reanalyse_per_iter`` passes over the shard at the current trainer step.  One host call each, with no
        append inside it: on the ring's stream the rewrite lands before any later append can recycle its slots."""
        for _ in range(self.reanalyse_per_iter):
            g, p = self.ra.pass_(self.train_steps)
            self.reanalysed_games += g
            self.reanalysed_positions += p

    def run(self, iterations):
        for _ in range(iterations):
            self.iteration()
        if self.train_stream is not None:
            torch.cuda.current_stream(self.device).wait_stream(self.train_stream)
        return self.stats()

    def stats(self):
        return {"moves": int(getattr(self.sp, "moves", 0)), "games": self.games, "slices": self.slices,
                "train_steps": self.train_steps, "weight_pushes": self.weight_pushes, "buffer": len(self.rb),
                "reanalysed_games": self.reanalysed_games, "reanalysed_positions": self.reanalysed_positions}


def run_c4(args, rank, world, dist, backend, log=print):
    """bench.py's C4 leg: the composed loop on this rank, timed; returns this rank's counts + time."""
    from . import trainer as T, weights as W
    from .config import GmzConfig
    torch.backends.cudnn.benchmark = True
    cfg = GmzConfig(BOARD_SIZE=args.size, NUM_SIMULATIONS=args.sims, NUM_RES_BLOCKS=args.blocks,
                    REANALYSIS_AGE_THRESHOLD=int(getattr(args, "loop_reanalyse_age", 900)))
    tcfg = T.TrainConfig(BOARD_SIZE=args.size, NUM_RES_BLOCKS=args.blocks, PHYSICAL_BATCH_SIZE=args.trainer_batch,
                         TRAIN_BUFFER_SIZE=args.loop_buffer, ENABLE_PER=True,
                         MODEL_UPDATE_INTERVAL=args.loop_update_interval)
    tr = T.Trainer(tcfg, device="cuda")
    sd = tr.state_dict_cpu()  # the trainer's initial weights (rank 0's, broadcast by Trainer) feed self-play
    openings = None
    if getattr(args, "loop_openings", 0) > 0:  # staggered starts: games at every stage from the first move on
        from .engine import random_openings
        openings = random_openings(args.loop_games, args.size, np.random.RandomState(args.seed + 17 * rank),
                                   args.loop_openings, n_in_row=cfg.N_IN_ROW)
    sp = SelfPlay(cfg, args.loop_games, sd, seed=args.seed + 7919 * rank, precision=getattr(args, "precision", "fp16"),
                  openings=openings)
    rb = ReplayBuffer(tcfg, device="cuda")
    if args.loop_prefill:
        from .weights import synthetic_slices
        rb.add_arrays(*synthetic_slices(args.loop_prefill, args.size, tcfg.NUM_UNROLL_STEPS,
                                        np.random.RandomState(args.seed + 31 * rank)))
    ra, ra_passes = None, int(getattr(args, "loop_reanalyse", 0))
    if ra_passes > 0:  # re-analysis of the shard's own games (off unless asked for)
        from .reanalysis import RingReanalyser
        ra = RingReanalyser(cfg, rb, sd, num_games=int(getattr(args, "loop_reanalyse_games", 256)),
                            max_positions=getattr(args, "loop_reanalyse_positions", None),
                            seed=args.seed + 104729 * (rank + 1), precision=getattr(args, "precision", "fp16"))
        ra.host = ra.host or bool(getattr(args, "loop_reanalyse_host", False))  # the A/B's host path
    loop = C4Loop(sp, tr, rb, tcfg, args.trainer_batch, dist=dist if world > 1 else None,
                  moves_per_iter=args.loop_moves_per_iter, train_steps_per_iter=args.loop_train_per_iter,
                  model_update_interval=args.loop_update_interval, seed=args.seed,
                  concurrent=getattr(args, "loop_concurrent", False),
                  device_ingest=getattr(args, "loop_device_ingest", False),
                  device_batches=getattr(args, "loop_device_batches", False), reanalyser=ra,
                  reanalyse_per_iter=ra_passes, device_weights=getattr(args, "loop_device_weights", False))
    t_w = time.perf_counter()
    loop.run(args.loop_warmup)
    torch.cuda.synchronize()
    log("rank %d: C4 loop warm-up %.1f s" % (rank, time.perf_counter() - t_w))
    s0 = loop.stats()
    if dist is not None and world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    loop.run(args.loop_iters)
    torch.cuda.synchronize()
    if dist is not None and world > 1:
        dist.barrier()
    dt = time.perf_counter() - t0
    s1 = loop.stats()
    d = {k: s1[k] - s0[k] for k in ("moves", "games", "slices", "train_steps", "weight_pushes")}
    if ra is not None:
        d.update({k: s1[k] - s0[k] for k in ("reanalysed_games", "reanalysed_positions")})
    d["buffer"] = s1["buffer"]
    # one ModelWeightsUpdate (workers.py:587-593) on its own, after the timed window: rank 0's trainer
    # weights -> broadcast -> every rank's inference network; the timed window runs the reference's
    # interval (1000 steps), so this is what a push adds once per interval
    n_push = 3
    if dist is not None and world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    t_p = time.perf_counter()
    for _ in range(n_push):
        loop.push_weights()
    torch.cuda.synchronize()
    d["push_ms"] = (time.perf_counter() - t_p) / n_push * 1e3
    sp.close()
    if ra is not None:
        ra.close()
    return d, dt
