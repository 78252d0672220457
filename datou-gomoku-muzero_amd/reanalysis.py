"""Re-analysis mode: stored games searched again with the current network.

The reference's ``universal_worker`` in worker mode 1 (workers.py:243-305) takes ONE game at a time
from the database (db_manager.py:163-181), runs ``mcts_engine.search`` position after position
(move ``i`` = ``board_states[i]``, player ``+1`` on even moves, last move ``actions[i-1]``,
move_count ``i``; workers.py:256-265), recomputes the n-step value targets from the new search values
(workers.py:290-291), rewrites the game's slices (db_manager.py:183-221) and reports how many
missed wins the new policies correct (workers.py:270-288, ``ReAnalysisStatus``).

Here the positions of MANY games are searched in one batch on the HIP engine: every position is an
independent search, so P positions fill ceil(P / G) batched searches of G games (the tail batch is
padded with empty boards whose results are dropped).  The missed-win census runs on the device with
the batched winning-move scan (``gmz_game_winning_scan``), one launch per batch.  The per-position
results are those of the reference's sequential searches with the same Gumbel noise (tested against
the oracle in tests/test_reanalysis_gpu.py).

``RingReanalyser`` is the same re-search for the composed loop (loop.C4Loop): its games are the ones in the
trainer's device replay ring (replay.ReplayBuffer.games), decoded from the ring's own planes and rewritten in
place by two HIP launches (gmz_replay_positions, gmz_replay_rewrite), so the batches the trainer draws carry
targets of the current network.  The missed-win census stays with the database path.
"""
import contextlib
from dataclasses import dataclass

import numpy as np
import torch

from . import records as R
from .replay import RotatingTables, rewrite_jobs, ring_positions_host, ring_rows


@dataclass
class ReanalysedGame:
    """One game's re-analysis: new search policies f64[n, A] and values f32[n], the n-step value
    targets written to the slices, and the workers.py:270-288 correction counters."""
    policies: np.ndarray
    values: np.ndarray
    value_targets: list
    corrected_fives: int
    original_fives: int
    corrected_totals: int
    original_totals: int


def positions_of(record, board_size):
    """workers.py:256-262 -> boards int8[n,S,S], players int8[n], last_moves int32[n] (-1 none),
    move_counts int32[n] for every move of a stored game."""
    n = len(record.actions)
    S = board_size
    boards = np.stack([np.asarray(b, dtype=np.int8).reshape(S, S) for b in record.board_states[:n]]) if n else \
        np.zeros((0, S, S), np.int8)
    players = np.array([1 if i % 2 == 0 else -1 for i in range(n)], dtype=np.int8)
    last = np.array([-1] + [int(a) for a in record.actions[:n - 1]], dtype=np.int32)[:n]
    return boards, players, last, np.arange(n, dtype=np.int32)


class Reanalyser:
    """Batched re-analysis on a ``BatchedSelfPlayEngine`` (its G games are the batch)."""

    def __init__(self, engine):
        self.eng = engine
        self.G, self.S, self.A = engine.G, engine.size, engine.A

    def search_positions(self, boards, players, last_moves, move_counts, gumbel=None):
        """Independent searches of P positions -> (policy f64[P,A], value f32[P], action int32[P],
        win classes uint8[P,A] of the position for the player to move: 0 none, 1 five,
        2 open_four, 3 combo).  ``gumbel``: optional f64[P,A] root noise (default: the engine's
        device noise)."""
        eng, G, S, A = self.eng, self.G, self.S, self.A
        P = len(boards)
        pol = np.zeros((P, A), np.float64)
        val = np.zeros(P, np.float32)
        act = np.full(P, -1, np.int32)
        cls = np.zeros((P, A), np.uint8)
        for lo in range(0, P, G):
            n = min(G, P - lo)
            b = np.zeros((G, S, S), np.int8)
            p = np.ones(G, np.int8)
            lm = np.full(G, -1, np.int32)
            mc = np.zeros(G, np.int32)
            b[:n], p[:n], lm[:n], mc[:n] = boards[lo:lo + n], players[lo:lo + n], last_moves[lo:lo + n], \
                move_counts[lo:lo + n]
            eng.set_positions(b, p, lm, mc)
            g = None
            if gumbel is not None:
                g = np.zeros((G, A), np.float64)
                g[:n] = gumbel[lo:lo + n]
            pt, vt, at = eng.search(gumbel=g)
            bd = torch.from_numpy(b).to(eng.device)
            ct = eng.winning_scan(bd, torch.from_numpy(p).to(eng.device))
            if eng.device.type == "cuda":
                torch.cuda.synchronize()
            pol[lo:lo + n] = pt[:n].cpu().numpy()
            val[lo:lo + n] = vt[:n].cpu().numpy()
            act[lo:lo + n] = at[:n].cpu().numpy()
            cls[lo:lo + n] = ct[:n].cpu().numpy()
        bad = act < 0  # no legal move: mcts.py returns (zeros, 0.0, -1)
        pol[bad], val[bad] = 0.0, 0.0
        return pol, val, act, cls

    def reanalyse(self, records, gumbel=None, discount=0.997, n_steps=10):
        """Re-analyse whole games -> [ReanalysedGame].  ``gumbel``: optional f64[total positions, A]
        in game-then-move order (the order of the reference's sequential searches)."""
        per = [positions_of(r, self.S) for r in records]
        counts = [len(x[0]) for x in per]
        if sum(counts) == 0:
            return [ReanalysedGame(np.zeros((0, self.A)), np.zeros(0, np.float32), [], 0, 0, 0, 0) for _ in records]
        cat = [np.concatenate([x[k] for x in per]) for k in range(4)]
        pol, val, act, cls = self.search_positions(*cat, gumbel=gumbel)
        out, off = [], 0
        for rec, n in zip(records, counts):
            p, v, c = pol[off:off + n], val[off:off + n], cls[off:off + n]
            of = ot = cf = ct = 0
            for i in range(n):  # workers.py:270-288
                wins = c[i] != 0
                if not wins.any():
                    continue
                if not wins[int(rec.actions[i])]:
                    ot += 1
                    five = bool((c[i] == 1).any())
                    of += five
                    if wins[int(np.argmax(p[i]))]:
                        ct += 1
                        cf += five
            rewards = np.array(rec.rewards, dtype=np.float32)
            targets = R.compute_n_step_returns(rewards, list(v), discount, n_steps) if n else []
            out.append(ReanalysedGame(p, v, targets, cf, of, ct, ot))
            off += n
        return out


class RingReanalyser:
    """MuZero Reanalyse on the trainer's replay ring: the games the ring holds (replay.ReplayBuffer.games) are
    searched again with the current network and their policy and n-step value targets rewritten in place.

    It owns a network (``state_dict``: network.GomokuNetHip; None: the engine's hash backend) and an engine of
    ``num_games`` slots of its own (the self-play engine's boards and trees are live), and staging for
    ``max_positions`` positions (default 4 * num_games; at least A, so that any one game fits).  With the ring on
    the GPU a pass never leaves the device: gmz_replay_positions decodes ring slices into the engine's inputs
    (BatchedSelfPlayEngine.set_positions_device), the searches' policies and values are copied into the staging, and
    one gmz_replay_rewrite writes the targets.  Ring reads and writes go on ``ring_stream`` (None: the current
    stream; the loop's train stream in concurrent mode: the stream of every other ring operation), the searches on
    the current stream, events between the two.  The host never waits for the work a pass enqueues, nor for anything
    in front of it on either stream: the padding mask of a short chunk is built on the device
    (set_active_device), and the one host wait is for the table set of two passes back, an event long passed
    (replay.RotatingTables, as the ingest's job tables).  An explicit ``gumbel`` (tests) is a pageable upload per chunk
    and does block.
    With the ring on the CPU (or ``host`` set) the same pass goes through the host (:meth:`pass_host`)."""

    def __init__(self, cfg, buffer, state_dict=None, num_games=256, max_positions=None, seed=0, precision="fp16"):
        from . import engine as E
        from .config import from_any
        c = self.cfg = from_any(cfg)
        rc = buffer.cfg
        if (c.BOARD_SIZE, c.NUM_UNROLL_STEPS) != (rc.BOARD_SIZE, rc.NUM_UNROLL_STEPS):
            raise ValueError("RingReanalyser: the engine's config and the buffer's disagree on the slices' geometry")
        self.rb, self.G, self.A = buffer, int(num_games), int(c.ACTION_SPACE_SIZE)
        self.max_positions = int(4 * self.G if max_positions is None else max_positions)
        if self.max_positions < self.A:
            raise ValueError("RingReanalyser: max_positions %d cannot hold one game of %d moves" %
                             (self.max_positions, self.A))
        self.net = None
        if state_dict is not None:
            from . import network as N
            self.net = N.GomokuNetHip(state_dict, c, num_slots=E.hidden_slots(c, self.G), max_rows=self.G,
                                      precision=precision)
        self.eng = E.BatchedSelfPlayEngine(c, num_games=self.G, net=self.net, seed=seed)
        self.searcher = Reanalyser(self.eng)  # the host path's batched searches
        dev, G, A, M = self.eng.device, self.G, self.A, self.max_positions
        self.ring_stream = None
        self.host = buffer.obs.device.type != "cuda"  # True: every pass goes through pass_host (a CPU ring; A/B)
        self.games = self.positions = 0
        self.last_pass = ([], 0)
        self.pol_new = torch.zeros(M, A, dtype=torch.float64, device=dev)
        self.val_new = torch.zeros(M, dtype=torch.float32, device=dev)
        self.board = torch.zeros(G, A, dtype=torch.int8, device=dev)
        self.player = torch.ones(G, dtype=torch.int8, device=dev)
        self.last = torch.full((G,), -1, dtype=torch.int32, device=dev)
        self.count = torch.zeros(G, dtype=torch.int32, device=dev)
        self._row = torch.arange(G, device=dev)  # row < n: the active mask of a chunk of n positions, made on the device
        self._tables = None     # replay.RotatingTables of (row table, job table), built by the first device pass
        self._loaded = None     # the engine's last read of board/player/last/count (the next decode waits for it)
        self._rewritten = None  # the last rewrite's read of the staging (the next pass's copies wait for it)

    def load_weights(self, sd):
        if self.net is not None:
            self.net.load_state_dict(sd)

    def load_device_weights(self, sd):
        """Device tensors (Trainer.device_state_dict) packed in place on the current stream, no host copy."""
        if self.net is not None:
            self.net.load_device_state_dict(sd)

    def close(self):
        self.eng.close()

    def _take(self, step, age):
        take, P = [], 0
        for e in self.rb.eligible(step, self.cfg.REANALYSIS_AGE_THRESHOLD if age is None else age):
            if P + e.kept > self.max_positions:
                break
            take.append(e)
            P += e.kept
        return take, P

    def pass_(self, step, age=None, gumbel=None):
        """One re-analysis pass at trainer step ``step``: the eligible games (version <= step - age; ``age`` None =
        cfg.REANALYSIS_AGE_THRESHOLD), oldest search first, as many as the staging holds, are searched position by
        position in chunks of ``num_games`` and their ring targets rewritten; their entries' version becomes
        ``step``.  ``gumbel``: optional f64 [positions, A] root noise in staging order (default: the engine's device
        noise).  Returns (games, positions)."""
        if self.host:
            return self.pass_host(step, age, gumbel)
        take, P = self._take(step, age)
        if not take:
            return 0, 0
        rb, eng, G, A = self.rb, self.eng, self.G, self.A
        dev = eng.device
        cur = torch.cuda.current_stream(dev)
        rs = self.ring_stream if self.ring_stream is not None else cur
        two = rs != cur
        rows, J = ring_rows(take, rb.N), len(take)
        if self._tables is None:  # (row table, job table); the one host wait is for the set of two passes back
            self._tables = RotatingTables(dev, (self.max_positions, 2), (self.max_positions, 6))
        tab = self._tables.take()
        with torch.cuda.stream(rs):
            rows_pin, rows_dev = tab.upload(0, rows)
            jobs_pin, jobs_dev = tab.upload(1, rewrite_jobs(take))
        if two and self._rewritten is not None:
            cur.wait_event(self._rewritten)  # the staging is free again
        for lo in range(0, P, G):
            n = min(G, P - lo)
            if two and self._loaded is not None:
                rs.wait_event(self._loaded)  # the engine has taken the previous chunk's positions
            rb.decode_positions(rows_pin[lo:lo + n], rows_dev[lo:lo + n], n, self.board, self.player, self.last,
                                self.count, stream=rs)
            if two:
                ev = torch.cuda.Event()
                ev.record(rs)
                cur.wait_event(ev)
            legal = np.zeros(G, np.int32)
            legal[:n] = A - rows[lo:lo + n, 1]
            eng.set_positions_device(self.board, self.player, self.last, self.count, legal)
            if two:
                self._loaded = torch.cuda.Event()
                self._loaded.record(cur)
            if n == G:
                eng.set_active(None)
            else:  # the padding rows stay out of the search; no upload, so nothing blocks the host
                eng.set_active_device((self._row < n).to(torch.uint8), np.arange(G) < n)
            g = None
            if gumbel is not None:
                g = np.zeros((G, A), np.float64)
                g[:n] = gumbel[lo:lo + n]
            pol, val, _ = eng.search(gumbel=g)
            self.pol_new[lo:lo + n].copy_(pol[:n])
            self.val_new[lo:lo + n].copy_(val[:n])
        if two:
            ev = torch.cuda.Event()
            ev.record(cur)
            rs.wait_event(ev)
        rb.rewrite_games(self.pol_new, self.val_new, P, jobs_pin, jobs_dev, J, stream=rs)
        done = torch.cuda.Event()
        done.record(rs)
        tab.event = self._rewritten = done
        return self._stamp(take, P, step)

    def pass_host(self, step, age=None, gumbel=None):
        """:meth:`pass_` through host memory: the planes are read back and decoded on the host, the positions go
        through Reanalyser.search_positions (an upload, a synchronise and a read-back per chunk) and the targets
        through ReplayBuffer.rewrite_games_host.  The same games, searches and targets as the device path."""
        take, P = self._take(step, age)
        if not take:
            return 0, 0
        on_ring = (lambda: torch.cuda.stream(self.ring_stream)) if self.ring_stream is not None else contextlib.nullcontext
        with on_ring():
            pos = ring_positions_host(self.rb, ring_rows(take, self.rb.N))
        self.eng.set_active(None)  # search_positions pads with empty boards and searches every row
        pol, val, _, _ = self.searcher.search_positions(*pos, gumbel=gumbel)
        with on_ring():
            self.rb.rewrite_games_host(take, pol, val)
        return self._stamp(take, P, step)

    def _stamp(self, take, P, step):
        for e in take:
            e.version = int(step)
        # (after a device pass rows 0..P-1 of pol_new / val_new hold these games' results until the next pass)
        self.last_pass = (take, P)
        self.games += len(take)
        self.positions += P
        return len(take), P


def reanalysis_step(reanalyser, store, current_trainer_step, cfg, max_games=64, ui_queue=None, gumbel=None):
    """One pass of worker mode 1 (workers.py:248-305) over up to ``max_games`` games at once:
    lock the oldest eligible games, re-analyse them in batched searches, rewrite their slices
    (RecordStore.finish_reanalysis_for_game) and post one ``ReAnalysisStatus`` per game.  Returns
    the number of games re-analysed (0: nothing eligible).  Locked games are unlocked on error."""
    locked = store.sample_and_lock_games_for_reanalysis(current_trainer_step, cfg.REANALYSIS_AGE_THRESHOLD,
                                                        max_games)
    if not locked:
        return 0
    try:
        res = reanalyser.reanalyse([rec for _, rec in locked], gumbel=gumbel, discount=cfg.DISCOUNT,
                                   n_steps=cfg.N_STEPS)
    except Exception:
        for gid, _ in locked:
            store.unlock_game_on_error(gid)
        raise
    done = 0
    for (gid, rec), r in zip(locked, res):
        if len(r.policies) != len(rec.actions) or not len(rec.actions):
            store.unlock_game_on_error(gid)
            continue
        if store.finish_reanalysis_for_game(gid, list(r.policies), r.value_targets, current_trainer_step,
                                            cfg.NUM_UNROLL_STEPS):
            done += 1
            if ui_queue is not None:
                ui_queue.put(R.ReAnalysisStatus(1, r.corrected_fives, r.original_fives, r.corrected_totals,
                                                r.original_totals))
    return done
