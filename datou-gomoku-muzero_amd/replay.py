"""The replay ring: the trainer's device-resident buffer of TrainingSlices, its directory of games, the job tables of
its HIP entry points (csrc/gmz_replay.hip) and the calls themselves: appends (``add_arrays`` of ``slices_from_game``;
``ingest_history``: gmz_replay_ingest on ``replay_jobs``' table), batches (``sample``; ``sample_indices(hip=True)`` +
``gather_into``: gmz_replay_per_sample, gmz_replay_gather) and re-analysis (``ring_rows`` -> gmz_replay_positions,
``rewrite_jobs`` -> gmz_replay_rewrite; host twins ``ring_positions_host``, ``rewrite_games_host``).  The record
layouts of include/gmz.h are built here and nowhere else.  Every host path stays: the tests compare the HIP paths
against them and a ring on the CPU runs on them.
"""
import ctypes

import numpy as np
import torch

from . import _lib as L
from . import records as R
from .worker import board_states_to_obs


def slices_from_game(boards, players, lasts, pols, vals, acts, winner, H, discount, n_steps, unroll):
    """One finished game -> the reference's TrainingSlices as stacked arrays (workers.py:183-222,
    same values as records.build_game_record's slice list):
    obs uint8 [n, U+1, 3, H, H], act int32 [n, U], rew f32 [n, U], pol f32 [n, U+1, A], val f32 [n, U+1]."""
    n, U = len(acts), unroll
    A = H * H
    obs = board_states_to_obs(np.asarray(boards).reshape(n, A), np.asarray(players), np.asarray(lasts), H)
    rew = R.final_rewards(n, winner)
    vt = np.asarray(R.compute_n_step_returns(rew.tolist(), list(vals), discount, n_steps), dtype=np.float32)
    pad = lambda x, k, v=0: np.concatenate([x, np.full((k,) + x.shape[1:], v, dtype=x.dtype)])  # noqa: E731
    win = lambda x, w: np.lib.stride_tricks.sliding_window_view(x, w, axis=0)[:n]  # noqa: E731
    o = win(pad(obs.astype(np.uint8), U + 1), U + 1)           # [n, 3, H, H, U+1]
    a = win(pad(np.asarray(acts, np.int32), U, -1), U)         # [n, U]
    r = win(pad(rew.astype(np.float32), U), U)
    p = win(pad(np.asarray(pols, np.float32).reshape(n, A), U + 1), U + 1)  # [n, A, U+1]
    v = win(pad(vt, U + 1), U + 1)
    return (np.ascontiguousarray(np.moveaxis(o, -1, 1)), np.ascontiguousarray(a), np.ascontiguousarray(r),
            np.ascontiguousarray(np.moveaxis(p, -1, 1)), np.ascontiguousarray(v))


def replay_jobs(games, ptr, count, N):
    """Job table of gmz_replay_ingest for ``games`` = [(slot, bank, row0, n_moves, winner), ...] appended in
    this order to a ring of N slices at ``ptr`` holding ``count``: what ReplayBuffer.add_arrays does game by
    game (a game longer than the ring keeps its newest N slices, written from ``ptr`` on), with every
    slice that a later game of the same table would overwrite left out, so no two kept slices share a
    ring slot.  Such slices are always the oldest of their game: a drop from the front.
    Returns (jobs int32 [J, 8] = game, bank, row0, n, winner, drop, slot, first; new ptr; new count)."""
    N, p = int(N), int(ptr)
    starts = []
    for (_, _, _, n, _) in games:
        k = min(int(n), N)
        starts.append(p)
        p = (p + k) % N
        count = min(N, int(count) + k)
    rows, cover = [], 0  # cover: ring slots written by the games after this one, a run from this game's end on
    for (g, bk, s0, n, w), st in zip(reversed(games), reversed(starts)):
        k = min(int(n), N)
        over = min(k, max(0, cover - (N - k)))
        if k > over:
            rows.append((g, bk, s0, n, w, n - k + over, (st + over) % N, 0))
        cover = min(N, cover + k)
    jobs = np.asarray(rows[::-1], dtype=np.int32).reshape(-1, 8)
    if len(jobs):
        kept = jobs[:, 3] - jobs[:, 5]
        jobs[:, 7] = np.cumsum(kept) - kept
    return jobs, p, count


def rewrite_jobs(entries):
    """Job table of gmz_replay_rewrite for ``entries`` (RingGame, in staging order) -> int32 [J, 6] = slot, kept, n,
    drop, winner, first (the staged rows before the game's)."""
    jobs = np.array([[e.slot, e.kept, e.n, e.drop, e.winner, 0] for e in entries], dtype=np.int32).reshape(-1, 6)
    jobs[:, 5] = np.cumsum(jobs[:, 1]) - jobs[:, 1]
    return jobs


def ring_rows(entries, N):
    """The (ring slot, move count) of every surviving slice of ``entries`` (RingGame) in staging order (game
    after game, positions drop..n-1) -> int32 [P, 2]; the move count of position t is start + t."""
    rows = [np.stack([(e.slot + np.arange(e.kept)) % N, e.start + e.drop + np.arange(e.kept)], 1) for e in entries]
    return np.concatenate(rows).astype(np.int32) if rows else np.zeros((0, 2), np.int32)


def ring_positions_host(rb, rows):
    """The host's decode of ring slices into search positions (the twin of gmz_replay_positions): ``rows`` int32
    [P, 2] of (slot, move count) -> boards int8 [P, S, S], players int8 [P] (+1 on even counts), last_moves int32 [P]
    (-1: none), move_counts int32 [P], from the step-0 planes of ``rb.obs``."""
    S = int(rb.cfg.BOARD_SIZE)
    P = len(rows)
    idx = torch.as_tensor(rows[:, 0].astype(np.int64)).to(rb.obs.device)
    planes = rb.obs[idx, 0].cpu().numpy().reshape(P, 3, S * S)
    mc = rows[:, 1].astype(np.int32)
    players = np.where(mc % 2 == 0, 1, -1).astype(np.int8)
    boards = (planes[:, 0] != 0) * players[:, None] - (planes[:, 1] != 0) * players[:, None]
    last = np.where(planes[:, 2].any(1), planes[:, 2].argmax(1), -1).astype(np.int32)
    return boards.astype(np.int8).reshape(P, S, S), players, last, mc


def discount_table(cfg):
    """discount ** i for i = 0..N_STEPS as the C doubles the ingest and the rewrite take by value (the device never
    calls pow)."""
    n = int(cfg.N_STEPS)
    return (ctypes.c_double * (n + 1))(*[cfg.DISCOUNT ** i for i in range(n + 1)])


def static_input_spec(cfg, B):
    """The trainer's seven static inputs for a batch of ``B`` as (name, dtype, shape): what Trainer._prepare
    allocates and gmz_replay_gather or Trainer._augment_into_static's copies write."""
    U, H = int(cfg.NUM_UNROLL_STEPS), int(cfg.BOARD_SIZE)
    f32, i64 = torch.float32, torch.int64
    return (("observations", f32, (B, U + 1, 3, H, H)), ("actions", i64, (B, U)), ("rewards", f32, (B, U)),
            ("policies", f32, (B, U + 1, H * H)), ("values", f32, (B, U + 1)), ("augmented actions", i64, (B, U)),
            ("weights", f32, (B,)))


class RotatingTables:
    """Two sets of int32 tables, each a pinned host tensor and its device copy per shape of ``shapes``, used in turn
    behind events, so the host fills one set while a launch still reads the other.  :meth:`take` hands out the next
    set after waiting for that set's own ``event`` (its use two turns back: long passed); the user uploads its
    tables (:meth:`_TableSet.upload`) and stores the event recorded after its launch in ``event``."""

    class _TableSet:
        def __init__(self, device, shapes):
            self.pinned = [torch.zeros(*s, dtype=torch.int32).pin_memory() for s in shapes]
            self.dev = [torch.zeros(*s, dtype=torch.int32, device=device) for s in shapes]
            self.event = None

        def upload(self, i, rows):
            """``rows`` (numpy int32 [n, cols]) into table ``i``, its device copy on the current stream; both whole."""
            pinned, dev, n = self.pinned[i], self.dev[i], len(rows)
            pinned[:n] = torch.from_numpy(rows)
            dev[:n].copy_(pinned[:n], non_blocking=True)
            return pinned, dev

    def __init__(self, device, *shapes):
        self.shapes, self._k = shapes, 0
        self._sets = [self._TableSet(device, shapes) for _ in range(2)]

    def take(self):
        t = self._sets[self._k & 1]
        self._k += 1
        if t.event is not None:
            t.event.synchronize()
        return t


class RingGame:
    """One game with slices in a ReplayBuffer's ring (an entry of its game directory): ``slot`` the ring slot of its
    oldest surviving slice (slice k of the survivors is at (slot + k) mod N), ``kept`` surviving slices, ``n`` moves
    recorded (``drop`` = n - kept slices lost from the front), ``winner``, ``start`` stones on the board at its first
    recorded position, ``version`` the trainer step at which its targets were last searched, ``seq`` append order."""
    __slots__ = ("slot", "kept", "n", "winner", "start", "version", "seq")

    def __init__(self, slot, kept, n, winner, start, version, seq):
        self.slot, self.kept, self.n, self.winner = int(slot), int(kept), int(n), int(winner)
        self.start, self.version, self.seq = int(start), int(version), int(seq)

    @property
    def drop(self):
        return self.n - self.kept

    def __repr__(self):
        return "RingGame(%s)" % ", ".join("%s=%d" % (k, getattr(self, k)) for k in self.__slots__)


class ReplayBuffer:
    """Device-resident ring of TrainingSlices with the sampling of replay_buffer.py:44-106.

    Slices live in HBM as observation planes uint8 [N, U+1, 3, H, W] (0/1 planes), actions int32,
    rewards f32, policies f32 [N, U+1, A], values f32; priorities f32 [N].  Sampling: uniform
    without replacement (ENABLE_PER off, the reference default) or stratified proportional PER
    (segment i of the total priority, one uniform draw each; prefix sums + binary search give the
    same leaf as the reference's sum-tree descent), IS weights (count * p / total)^-beta / max.

    ``games`` is the host-side directory of the games whose slices the ring holds (RingGame, oldest first): made by
    :meth:`ingest_history` and by :meth:`add_arrays` with ``game=``, trimmed by every append, read by re-analysis
    (:meth:`eligible`, reanalysis.RingReanalyser).  Slices appended without it (:meth:`add`, synthetic prefill) have
    no entry and are never re-analysed."""

    def __init__(self, cfg, capacity=None, device="cuda"):
        c = cfg
        self.cfg, self.N = c, int(capacity or c.TRAIN_BUFFER_SIZE)
        U, H, A = c.NUM_UNROLL_STEPS, c.BOARD_SIZE, c.BOARD_SIZE * c.BOARD_SIZE
        d = torch.device(device)
        self.obs = torch.zeros(self.N, U + 1, 3, H, H, dtype=torch.uint8, device=d)
        self.act = torch.zeros(self.N, U, dtype=torch.int32, device=d)
        self.rew = torch.zeros(self.N, U, dtype=torch.float32, device=d)
        self.pol = torch.zeros(self.N, U + 1, A, dtype=torch.float32, device=d)
        self.val = torch.zeros(self.N, U + 1, dtype=torch.float32, device=d)
        self.prio = torch.zeros(self.N, dtype=torch.float32, device=d)
        self.ptr, self.count, self.max_priority, self.device = 0, 0, 1.0, d
        self._per_ws = None  # gmz_replay_per_sample's workspace (sample_indices(hip=True)), built at first use
        self._ingest_tables = None  # ingest_history's job tables (RotatingTables), built at first use
        self.games, self._seq = [], 0  # the game directory (RingGame, oldest first) and its append counter
        self.step = 0  # the trainer step ingest_history stamps on new entries (the loop keeps it current)

    def __len__(self):
        return self.count

    def need_device(self, what):
        """The refusal of every HIP path on a ring that is not in device memory."""
        if self.obs.device.type != "cuda":
            raise ValueError("%s needs a device-resident ReplayBuffer, not one on %s" % (what, self.obs.device))

    def add(self, slices):
        """Append TrainingSlice-like objects (observation, action_history, reward_history,
        policy_history, value_history)."""
        if len(slices) == 0:
            return
        self.add_arrays(*(np.stack([np.asarray(getattr(s, f)) for s in slices]) for f in (
            "observation", "action_history", "reward_history", "policy_history", "value_history")))

    def add_arrays(self, obs, act, rew, pol, val, game=None):
        """Append n slices given as stacked arrays/tensors (obs [n,U+1,3,H,W] 0/1, act [n,U] int,
        rew [n,U], pol [n,U+1,A], val [n,U+1]); the ring semantics of :meth:`add`.  ``game`` = (winner, start,
        version): the slices are one whole game's, in move order (slices_from_game), and it gets a directory
        entry (RingGame); without it no entry is made."""
        n = moves = int(obs.shape[0])
        if n == 0:
            return
        if n > self.N:  # only the newest N survive the ring
            obs, act, rew, pol, val = obs[-self.N:], act[-self.N:], rew[-self.N:], pol[-self.N:], val[-self.N:]
            n = self.N
        self._trim(n)
        if game is not None:
            self._note_game(self.ptr, n, moves, *game)
        idx = ((torch.arange(n) + self.ptr) % self.N).to(self.device)
        def dv(x, dt):
            if isinstance(x, np.ndarray) and not x.flags.writeable:
                x = np.array(x)  # torch.as_tensor warns on (and would alias) a read-only numpy array
            return torch.as_tensor(x).to(self.device, dt)
        self.obs[idx] = dv(obs, torch.uint8)
        self.act[idx] = dv(act, torch.int32)
        self.rew[idx] = dv(rew, torch.float32)
        self.pol[idx] = dv(pol, torch.float32)
        self.val[idx] = dv(val, torch.float32)
        if self.cfg.ENABLE_PER:
            self.prio[idx] = torch.as_tensor(self.max_priority, dtype=torch.float32, device=self.device)
        else:
            self.prio[idx] = 1.0
        self.ptr = (self.ptr + n) % self.N
        self.count = min(self.N, self.count + n)

    # ---------------------------------------------------------------- game directory
    def _trim(self, k):
        """The directory before ``k`` slices are appended at ``ptr``: the slots they overwrite hold the oldest
        slices of the oldest games (replay_jobs), so those entries' slot, kept and drop advance, and an entry
        with nothing left goes.  A trimmed game stays whole for re-analysis: its surviving slices t >= drop read
        positions t..t+U and values t+N_STEPS only."""
        N, k, gone = self.N, min(int(k), self.N), 0
        for e in self.games:
            d = (e.slot - self.ptr) % N  # the entry's oldest slice is the d-th slot the append writes
            if d >= k:
                break
            over = min(k - d, e.kept)
            e.slot, e.kept = (e.slot + over) % N, e.kept - over
            if e.kept:
                break
            gone += 1
        del self.games[:gone]

    def _note_game(self, slot, kept, n, winner, start, version):
        self.games.append(RingGame(slot, kept, n, winner, start, version, self._seq))
        self._seq += 1

    def note_jobs(self, jobs, appended, version=None):
        """The directory's half of an ingest, before ``ptr`` moves: ``jobs`` is replay_jobs' table (a game's first
        recorded row is its ``start``) of games that append ``appended`` slices in all at ``ptr``."""
        self._trim(appended)
        v = self.step if version is None else version
        for (_, _, row0, n, winner, drop, slot, _) in np.asarray(jobs).reshape(-1, 8).tolist():
            self._note_game(slot, n - drop, n, winner, row0, v)

    def eligible(self, step, age):
        """The games whose targets are at least ``age`` trainer steps old at ``step`` (version <= step - age), oldest
        search first: ordered by (version, seq)."""
        lim = int(step) - int(age)
        return sorted((e for e in self.games if e.version <= lim), key=lambda e: (e.version, e.seq))

    # ---------------------------------------------------------------- re-analysis: positions out, targets in
    def decode_positions(self, rows_host, rows_dev, P, board, player, last, count, stream=None):
        """gmz_replay_positions on ``stream`` (default: the current one): rows 0..P-1 of the engine inputs ``board``
        int8 [G, A], ``player`` int8 [G], ``last`` int32 [G], ``count`` int32 [G] decoded from the step-0 planes of
        the ring slots the (slot, move count) table names (``rows_host`` pinned int32 [>= P, 2], ``rows_dev`` its
        device copy; ring_rows), rows P..G-1 empty boards."""
        c = self.cfg
        return L.call("gmz_replay_positions", int(c.BOARD_SIZE), int(c.NUM_UNROLL_STEPS), int(self.N), self.obs,
                      L.nbytes(self.obs), rows_host, int(P), rows_dev, L.nbytes(rows_dev), int(player.shape[0]), board,
                      L.nbytes(board), player, L.nbytes(player), last, L.nbytes(last), count, L.nbytes(count),
                      L.stream_ptr(stream))

    def rewrite_games(self, pol_new, val_new, P, jobs_host, jobs_dev, n_jobs, stream=None):
        """gmz_replay_rewrite on ``stream`` (default: the current one): the staged search results ``pol_new`` f64
        [>= P, A] and ``val_new`` f32 [>= P] become the policy and n-step value targets of the ring slices of the
        ``n_jobs`` games in the table (``jobs_host`` pinned int32 [>= n_jobs, 6], ``jobs_dev`` its device copy;
        rewrite_jobs); discount, n-step and unroll from the ring's config."""
        c = self.cfg
        return L.call("gmz_replay_rewrite", int(c.BOARD_SIZE), int(c.NUM_UNROLL_STEPS), int(c.N_STEPS), int(self.N),
                      self.pol, L.nbytes(self.pol), self.val, L.nbytes(self.val), pol_new, L.nbytes(pol_new), val_new,
                      L.nbytes(val_new), int(P), jobs_host, int(n_jobs), jobs_dev, L.nbytes(jobs_dev),
                      discount_table(c), L.stream_ptr(stream))

    def rewrite_games_host(self, entries, pol_new, val_new):
        """New search results into the ring slices of ``entries`` (RingGame, in staging order) on the host:
        ``pol_new`` f64 [P, A] and ``val_new`` f32 [P] hold, game after game, the rows of positions drop..n-1.  Each
        game's policy and n-step value targets are slices_from_game's for the new policies and values (the
        positions before ``drop`` reach no surviving slice), assigned to its ring rows by torch indexing; planes,
        actions, rewards and priorities stay.  The reference of gmz_replay_rewrite, and the path of a ring on the
        CPU."""
        c = self.cfg
        H, A = int(c.BOARD_SIZE), int(c.BOARD_SIZE) ** 2
        pol_new = np.asarray(pol_new, dtype=np.float64).reshape(-1, A)
        val_new = np.asarray(val_new, dtype=np.float32).reshape(-1)
        first = 0
        for e in entries:
            n, drop = e.n, e.drop
            pols, vals = np.zeros((n, A), np.float64), np.zeros(n, np.float32)
            pols[drop:], vals[drop:] = pol_new[first:first + e.kept], val_new[first:first + e.kept]
            _, _, _, p, v = slices_from_game(np.zeros((n, A), np.int8), np.ones(n, np.int8), np.full(n, -1, np.int32),
                                             pols, vals, np.zeros(n, np.int32), e.winner, H, c.DISCOUNT, c.N_STEPS,
                                             c.NUM_UNROLL_STEPS)
            idx = ((torch.arange(e.kept) + e.slot) % self.N).to(self.device)
            self.pol[idx] = torch.from_numpy(np.array(p[drop:])).to(self.device)  # (copies: the views may be read-only)
            self.val[idx] = torch.from_numpy(np.array(v[drop:])).to(self.device)
            first += e.kept

    # ---------------------------------------------------------------- device ingest
    def admission_priority(self):
        """The priority of newly added slices as a device f32 scalar, or None for 1.0 (PER off, or no
        priority updated yet): what gmz_replay_ingest reads on the device, so nothing synchronises."""
        m = self.max_priority
        if not self.cfg.ENABLE_PER or (not torch.is_tensor(m) and float(m) == 1.0):
            return None
        if not (torch.is_tensor(m) and m.dtype == torch.float32 and m.device == self.obs.device):
            m = self.max_priority = torch.as_tensor(m, dtype=torch.float32).to(self.obs.device)
        return m

    def ingest_history(self, hist, sn, games=None):
        """The finished games of ``hist``'s snapshot ``sn`` (worker.GameHistory) appended on the device: their
        slices go from the history's banks into this ring by one HIP launch (gmz_replay_ingest) on the
        current stream, bit-identical to GameHistory.harvest + slices_from_game + :meth:`add_arrays`
        game by game in slot order; only the job table (32 bytes per game) crosses the bus.  ``games``:
        ``hist.finished(sn)`` when the caller has taken it already.  The launch's event goes to the history
        (GameHistory.after_ingest): its next ``record`` waits for it before it rewrites a bank.  Returns the
        per-game (game slot, winner, n_moves, missed_fives, missed_totals)."""
        c = self.cfg
        U, H = int(c.NUM_UNROLL_STEPS), int(c.BOARD_SIZE)
        self.need_device("ingest_history")
        if getattr(hist, "A", None) != H * H or tuple(self.obs.shape[1:]) != (U + 1, 3, H, H):
            raise ValueError("history of %s actions does not fit a ring of %dx%d boards, %d unroll steps"
                             % (getattr(hist, "A", None), H, H, U))
        if U < 1 or self.N < 1:
            raise ValueError("ring of %d slices, %d unroll steps: smaller than one slice" % (self.N, U))
        if hist.board.device != self.obs.device:
            raise ValueError("history on %s, ring on %s" % (hist.board.device, self.obs.device))
        if games is None:
            games = hist.finished(sn)
        if not games:
            return []
        jobs, new_ptr, new_count = replay_jobs([x[:5] for x in games], self.ptr, self.count, self.N)
        J = len(jobs)
        if J > hist.G:
            raise ValueError("%d finished games in one snapshot of %d slots" % (J, hist.G))
        if J:  # (J = 0: later games of the snapshot overwrite every slice; nothing to launch)
            stream = torch.cuda.current_stream(self.obs.device)
            stream.wait_event(sn["ev"])  # the banks' rows were written before the snapshot
            if self._ingest_tables is None or self._ingest_tables.shapes[0][0] < hist.G:
                self._ingest_tables = RotatingTables(self.obs.device, (hist.G, 8))
            tab = self._ingest_tables.take()
            pinned, dev = tab.upload(0, jobs)
            L.call("gmz_replay_ingest", H, U, int(c.N_STEPS), hist.G, hist.L, hist.board, hist.player, hist.last,
                   hist.pol, hist.val, hist.act, self.obs, self.act, self.rew, self.pol, self.val, self.prio, self.N,
                   pinned, J, dev, L.nbytes(dev), discount_table(c), self.admission_priority(), L.stream_ptr(stream))
            tab.event = torch.cuda.Event()
            tab.event.record(stream)
            hist.after_ingest(tab.event)
        # the game directory (re-analysis): trimmed by what the games append, then one entry per job; then ptr moves
        self.note_jobs(jobs, sum(min(int(x[3]), self.N) for x in games))
        self.ptr, self.count = new_ptr, new_count
        return [(g, w, n, mf, mt) for (g, _, _, n, w, mf, mt) in games]

    # ---------------------------------------------------------------- batches
    def sample(self, B, rng=np.random, dist=None):
        """replay_buffer.py:58-94.  ``dist``: torch.distributed when this buffer is one rank's shard of
        a data-parallel trainer (sharded PER): each rank samples its B slices from its
        own shard (rank chosen uniformly, then proportional within the shard, so a slice's sampling
        probability is p_i / (N * T_rank)); the IS weights use the GLOBAL slice count (one all-reduce
        SUM) and are normalised by the max over the global batch (one all-reduce MAX).  With one rank
        this is exactly the reference's (count * p_i / T)^-beta / max.  The draw is :meth:`sample_indices`'s;
        the batch is the ring's rows at its indices by torch indexing."""
        got = self.sample_indices(B, rng, dist)
        if got is None:
            return None
        idx, w = got
        batch = (self.obs[idx].float(), self.act[idx], self.rew[idx], self.pol[idx], self.val[idx])
        return batch, idx, w

    def sample_indices(self, B, rng=np.random, dist=None, hip=False):
        """The index and weight half of :meth:`sample` -> (idx int64 [B], w f32 [B]), or None when the ring holds
        fewer than B slices.  PER off: ``rng.choice`` without replacement, weights of one.  PER on: no host
        synchronisation: the reference's per-segment draws uniform(seg*i, seg*(i+1)) = seg * (i + random_sample())
        take B host uniforms (``rng.random_sample(B)``); the total stays on the device.  ``hip``: with PER on, the
        draw (priorities' prefix sums, the search, the probabilities) is gmz_replay_per_sample on the current stream,
        in the summation order include/gmz.h states, instead of torch's cumsum and searchsorted; the IS weights and
        the sharded-PER all-reduces are the same lines, fed with either's probabilities.  With PER off both settings
        draw the same host permutation."""
        if hip:
            self.need_device("sample_indices(hip=True)")
        if self.count < B:
            return None
        if not self.cfg.ENABLE_PER:
            idx = torch.from_numpy(rng.choice(self.count, B, replace=False)).to(self.device)
            return idx, torch.ones(B, device=self.device)
        r = torch.from_numpy(rng.random_sample(B)).to(self.device, non_blocking=True)
        if hip:
            ws = self._per_ws
            if ws is None:  # sized for a full ring: the need grows with count
                need = L.query("gmz_replay_per_sample_workspace_bytes", int(self.N), int(B))
                ws = self._per_ws = torch.empty((need + 7) // 8, dtype=torch.float64, device=self.device)
            idx = torch.empty(B, dtype=torch.int64, device=self.device)
            prob = torch.empty(B, dtype=torch.float64, device=self.device)
            L.call("gmz_replay_per_sample", self.prio, r, int(self.count), int(B), idx, L.nbytes(idx), prob,
                   L.nbytes(prob), ws, L.nbytes(ws), L.stream_ptr())
        else:
            p = self.prio[: self.count].double()
            cum = torch.cumsum(p, 0)
            total = cum[-1]
            u = (torch.arange(B, device=self.device, dtype=torch.float64) + r) * (total / B)
            idx = torch.searchsorted(cum, u).clamp_max(self.count - 1)
            prob = p[idx] / total
        count = float(self.count)
        if dist is not None and dist.get_world_size() > 1:
            count = _allreduce(torch.tensor([count], dtype=torch.float64, device=self.device), dist)
            prob = prob / dist.get_world_size()
        w = (count * prob) ** (-self.cfg.PER_BETA)
        wmax = w.max()
        if dist is not None and dist.get_world_size() > 1:
            wmax = _allreduce(wmax.reshape(1), dist, max_op=True)[0]
        return idx, (w / wmax).float()

    def gather_into(self, dst, idx, w, k, flip):
        """The batch of ring slots ``idx`` (int64 [B], repeats allowed) under the board symmetry (k quarter turns,
        then the mirror when ``flip``) written into ``dst``, a 7-tuple shaped like Trainer._static
        (static_input_spec; ``w`` None = weights of one): one HIP launch (gmz_replay_gather) on the current stream,
        bit-identical to Trainer._augment_into_static on the batch :meth:`sample` builds by torch indexing."""
        c = self.cfg
        U, H = int(c.NUM_UNROLL_STEPS), int(c.BOARD_SIZE)
        dev = self.obs.device
        self.need_device("gather_into")
        if tuple(self.obs.shape[1:]) != (U + 1, 3, H, H):
            raise ValueError("ring planes %s do not hold %d unroll steps of %dx%d boards" % (tuple(self.obs.shape), U, H, H))
        if not torch.is_tensor(idx) or idx.dtype != torch.int64 or idx.dim() != 1 or idx.device != dev \
                or not idx.is_contiguous():
            raise ValueError("idx must be a contiguous int64 vector on %s" % dev)
        B = int(idx.shape[0])
        if w is not None and (not torch.is_tensor(w) or w.dtype != torch.float32 or tuple(w.shape) != (B,)
                              or w.device != dev or not w.is_contiguous()):
            raise ValueError("w must be None or a contiguous float32 vector of %d weights on %s" % (B, dev))
        want = static_input_spec(c, B)
        if len(dst) != len(want):
            raise ValueError("dst holds %d tensors, not the trainer's %d static inputs" % (len(dst), len(want)))
        for t, (name, dt, shape) in zip(dst, want):
            if not torch.is_tensor(t) or t.dtype != dt or tuple(t.shape) != shape or t.device != dev \
                    or not t.is_contiguous():
                raise ValueError("dst %s: expected a contiguous %s tensor of shape %s on %s, got %s %s on %s" % (
                    name, dt, shape, dev, getattr(t, "dtype", type(t)), tuple(getattr(t, "shape", ())),
                    getattr(t, "device", None)))
        if int(k) not in (0, 1, 2, 3):
            raise ValueError("k = %r is not a number of quarter turns 0..3" % (k,))
        sized = [x for t in dst for x in (t, L.nbytes(t))]
        L.call("gmz_replay_gather", H, U, int(self.N), int(self.count), B, self.obs, self.act, self.rew, self.pol,
               self.val, idx, w, int(k), int(bool(flip)), *sized, L.stream_ptr())

    def update_priorities(self, idx, td, dist=None):
        """replay_buffer.py:96-101; with ``dist`` the running max priority (the priority of newly added
        slices) is kept global by an all-reduce MAX, so every shard admits new slices alike."""
        if not self.cfg.ENABLE_PER:
            return
        p = td.abs().to(self.device).float() + self.cfg.PER_EPSILON
        m = torch.maximum(torch.as_tensor(self.max_priority, device=self.device, dtype=torch.float32), p.max())
        if dist is not None and dist.get_world_size() > 1:
            m = _allreduce(m.reshape(1), dist, max_op=True)[0]
        self.max_priority = m  # device scalar
        self.prio[idx] = p


def _allreduce(t, dist, max_op=False):
    """All-reduce a small tensor (SUM or MAX) on any backend: RCCL takes device tensors, gloo host
    tensors.  Returns the reduced tensor on ``t``'s device."""
    op = dist.ReduceOp.MAX if max_op else dist.ReduceOp.SUM
    if dist.get_backend() == "gloo" and t.is_cuda:
        h = t.cpu()
        dist.all_reduce(h, op=op)
        out = h.to(t.device)
    else:
        dist.all_reduce(t, op=op)
        out = t
    return out
