"""BatchedSelfPlayEngine — G concurrent games searched and played on one MI355X.

Host orchestration of the HIP kernels in csrc/gmz_tree.hip (C ABI: include/gmz.h).  One call of
:meth:`search` performs, for every game at once, exactly what one ``MuZeroMCTS.search(game)``
(/root/reference/mcts.py:288-362) or ``AlphaZeroMCTS.search(game)`` (mcts.py:197-280) does for
one game; :meth:`play` is ``game.do_move`` + ``get_game_ended`` (workers.py:178-181).

The network is a pluggable *device backend* (``initial`` / ``recurrent`` writing straight into
the engine's slot-indexed buffers) — the in-process replacement of the reference's
InferenceServer queue round trip (workers.py:331-369).  Backends: ``HashNetBackend`` (tree
parity) and ``network.GomokuNetHip`` (GomokuNetEZ on MFMA kernels).

Everything stays resident in HBM; the only host<->device traffic per move is the game status
(G bytes) used to size the next move's wave loop, plus whatever the caller copies out.
"""
import contextlib
import ctypes

import numpy as np
import torch

from . import _lib
from .config import from_any
from ._lib import GmzError, bufs, check, ptr
from .openings import _has_five, _place_stones, random_openings, seeded_openings  # noqa: F401  (re-exported)
from .openings import book_draw, check_selfplay_book


class HashNetBackend:
    """HashNet test network on the device (oracle/hashnet.py definition, csrc/gmz_hashnet.hip)."""

    def __init__(self, num_slots, action_space, device="cuda"):
        self.A = action_space
        self.pool = torch.zeros(num_slots, dtype=torch.int32, device=device)  # uint32 ids

    def ensure_slots(self, n, stream=None):
        """At least ``n`` hidden-state slots (a larger pool, contents not kept: called between moves); the old
        pool is recorded on ``stream`` (default: the current one), the stream that used it."""
        if n > self.pool.numel():
            self.pool.record_stream(stream if stream is not None else torch.cuda.current_stream(self.pool.device))
            self.pool = torch.zeros(int(n * 1.25) + 1, dtype=torch.int32, device=self.pool.device)

    def split(self, parts, max_grid=0):
        """Backends over disjoint equal slices of the pool (SplitSelfPlayEngine)."""
        n = self.pool.numel() // parts
        out = []
        for i in range(parts):
            q = HashNetBackend.__new__(HashNetBackend)
            q.A, q.pool = self.A, self.pool[i * n:(i + 1) * n]
            out.append(q)
        return out

    def initial(self, obs, out_slot, logits, value, stream):
        check(_lib.load().gmz_hashnet_initial(ptr(obs), obs.shape[0], self.A, ptr(out_slot), ptr(self.pool),
                                              ptr(logits), ptr(value), stream))

    def recurrent(self, in_slot, action, out_slot, logits, value, reward, stream):
        check(_lib.load().gmz_hashnet_recurrent(ptr(self.pool), ptr(in_slot), ptr(action), ptr(out_slot),
                                                in_slot.shape[0], self.A, ptr(logits), ptr(value), ptr(reward),
                                                stream))


class _PinnedPair:
    """Two pinned host buffers that take turns carrying a small array to one device tensor with no host wait: a
    slot is written again only after its own last copy (two uploads ago: long done) has finished."""

    def __init__(self, shape, dtype):
        self.host = [torch.zeros(shape, dtype=dtype).pin_memory() for _ in range(2)]
        self.events = [None, None]
        self.flip = 0

    def upload(self, values, dev, stream=None):
        """``values`` (a numpy array of the buffers' shape) into ``dev`` on ``stream`` (None: the current one)."""
        i = self.flip
        self.flip ^= 1
        if self.events[i] is not None:
            self.events[i].synchronize()
        self.host[i].numpy()[:] = values
        with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():
            dev.copy_(self.host[i], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        self.events[i] = ev


class BatchedSelfPlayEngine:
    """G games per GPU.  ``cfg``: any object with the reference config attribute names."""

    def __init__(self, cfg=None, num_games=1, net=None, device="cuda", seed=0, descent_hint=None, game_offset=0,
                 wpb=None, layout=None, pair=None, **overrides):
        self.cfg = from_any(cfg, **overrides)
        c = self.cfg
        if c.MCTS_IMPLEMENTATION not in ("AlphaZero", "MuZero"):
            raise ValueError("Unknown MCTS implementation in config: '%s'" % c.MCTS_IMPLEMENTATION)  # workers.py:140-142
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.G, self.A, self.size = int(num_games), c.ACTION_SPACE_SIZE, c.BOARD_SIZE
        if layout is None:
            layout = default_layout(self.G)
        if layout not in ("dense", "lists"):
            raise ValueError("layout: 'dense' (every node's full child row) or 'lists' (compact child lists)")
        if descent_hint is None:
            # dense rows: the hint kernels (cached exp rows + next-visit prefetch) at every G measured; the
            # no-hint dense kernels keep the reference's exp(logit + t - max) form (A/B and tests).
            # Compact lists always use the cached exp rows; there the hint only switches the prefetch,
            # which measured slower (8,192 games: 110 vs 125 us; profiles/r03_tree_layout_ab.txt)
            descent_hint = layout == "dense"
        self.mode = 1 if c.MCTS_IMPLEMENTATION == "MuZero" else 0
        self.slots_per_game = c.NUM_SIMULATIONS + 2
        if wpb not in (None, 1, 4):
            raise ValueError("wpb: games per workgroup of the fused expand/select kernel must be None, 1 or 4")
        self.descent_hint = bool(descent_hint)
        self.layout = layout
        # two waves per game in the fused expand/select kernel (MuZero, dense rows with the hint, 129..256
        # actions; k_expand_select_pair): None = default_pair(G)
        pair_ok = self.mode == 1 and layout == "dense" and self.descent_hint and 128 < self.A <= 256
        self.pair = bool(pair_ok and (default_pair(self.G) if pair is None else pair))
        # flags (include/gmz.h): bit 0 no hint; bits 1 / 2 force 4-wave / 1-wave workgroups (None: by occupancy);
        # bit 3 compact child lists for non-root nodes; bit 4 two waves per game
        flags = ((0 if descent_hint else 1) | {None: 0, 4: 2, 1: 4}[wpb] | (8 if layout == "lists" else 0)
                 | (16 if self.pair else 0))
        self.ecfg = engine_cfg(c, self.G, flags, game_offset)
        h = ctypes.c_void_p()
        check(self.lib.gmz_engine_create(ctypes.byref(self.ecfg), ctypes.byref(h)))
        self.handle = h
        self.seed = int(seed)
        self.fuse_waves = True  # expand/backup + next select in one launch (False: the two entry points)
        G, A, dev = self.G, self.A, self.device
        # hidden-state slots per game by legal-move count (gmz_engine_set_hidden_bases): MuZero creates one
        # node per wave (mcts.py:320-350), so a game needs waves(L) + 2 slots, not num_simulations + 2
        self._slot_need = slot_need_table(self.ecfg, A, self.mode, self.lib)
        self._run_cfg = self.ecfg  # the budget the searches run with (set_simulations)
        self._sims_tables = {c.NUM_SIMULATIONS: (self.ecfg, self._slot_need)}
        self.net = net if net is not None else HashNetBackend(G * int(self._slot_need[A]), A, device)
        f32, i32 = torch.float32, torch.int32
        self.obs = torch.zeros(G, 3, c.BOARD_SIZE, c.BOARD_SIZE, dtype=f32, device=dev)
        self.logits = torch.zeros(G, A, dtype=f32, device=dev)
        self.value = torch.zeros(G, dtype=f32, device=dev)
        self.reward = torch.zeros(G, dtype=f32, device=dev)
        self.in_slot = torch.zeros(G, dtype=i32, device=dev)
        self.out_slot = torch.zeros(G, dtype=i32, device=dev)
        self.act_req = torch.zeros(G, dtype=i32, device=dev)
        # hidden-state slot of each game's root (= its node 0): hbase[g], rewritten when the bases move, and
        # beside it each game's slot budget (gmz_engine_set_hidden_budget): one device buffer [2G]
        self._hb_dev = torch.empty(2 * G, dtype=i32, device=dev)
        self.root_slot = self._hb_dev[:G]
        self.hidden_budget = self._hb_dev[G:]
        self.root_slot.copy_(torch.arange(G, dtype=i32, device=dev) * self.slots_per_game)
        self.hidden_budget.fill_(self.slots_per_game)
        self._hb_stage = _PinnedPair(2 * G, i32)
        self._hb_last = None  # the bases last handed to the engine (host copy)
        self.hidden_slots_used = 0
        self.policy = torch.zeros(G, A, dtype=torch.float64, device=dev)
        self.root_value = torch.zeros(G, dtype=f32, device=dev)
        self.action = torch.zeros(G, dtype=i32, device=dev)
        self.status = torch.zeros(G, dtype=torch.int8, device=dev)
        self._status_host = torch.zeros(G, dtype=torch.int8).pin_memory()
        self._err_host = torch.zeros(1, dtype=i32).pin_memory()  # the engine's error word, copied with each status
        self._status_event = None
        self._n_legal = np.full(G, A, dtype=np.int32)
        self._active = None  # host copy of set_active's mask (None: every game is searched)
        self._budgets = None  # host copy of set_budgets' simulations per game (None: every game the engine's)
        self._bud_dev = self._bud_stage = None  # its device copy and the staging pair (made at the first call)
        self._refill = None  # play_refill's slot arrays and pinned read-back buffers (arena)
        self._refill_pending = False
        self._book = None  # set_book's device book, slot arrays and the host's serial mirror (self-play restarts)
        self._fill_actions = None  # fill_from_book's actions: -1 everywhere
        self._state_ptrs = None  # device pointers of the engine-owned game state (anchor_move, vcf_move)
        self.vcf_status = self.vcf_moves = None  # the last vcf_move launch's statuses and moves (made at the first)
        self.ab_status = self.ab_moves = None  # the same of ab_move
        self.finished_seen = 0  # the match's finished-games counter as of the last status read (play_refill)
        self.moves_played = 0   # moves counted from the statuses read after play_refill calls
        self._hb_net = None     # the backend whose pool the last placement was checked against
        self._last_reset = True
        self.waves_last = 0
        self.tree_timer = None  # optional network.KernelTimer around the fused expand/backup+select launches
        # the packed per-game hidden-state bases and budgets from the start, so a direct ABI caller
        # (begin_move / select without search_steps) already uses slots inside the network's pool
        self._place_hidden(self._stream())

    # ------------------------------------------------------------------ lifecycle
    def close(self):
        if getattr(self, "handle", None):
            self.lib.gmz_engine_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self, stream=None):
        return _lib.stream_ptr(stream)

    # ------------------------------------------------------------------ game state
    def game_state(self):
        """Copies of the engine-owned game state: boards int8[G,S,S], players int8[G],
        last_moves int32[G], move_counts int32[G] (device tensors)."""
        G, A, dev = self.G, self.A, self.device
        b = torch.empty(G, A, dtype=torch.int8, device=dev)
        p = torch.empty(G, dtype=torch.int8, device=dev)
        lm = torch.empty(G, dtype=torch.int32, device=dev)
        mc = torch.empty(G, dtype=torch.int32, device=dev)
        check(self.lib.gmz_engine_copy_state(self.handle, 0, ptr(b), ptr(p), ptr(lm), ptr(mc), self._stream()))
        return b.view(G, self.size, self.size), p, lm, mc

    def set_positions(self, boards, players, last_moves, move_counts=None):
        """Load G positions: boards int8[G,S,S], players ±1, last_moves (-1 = none)."""
        G, A, dev = self.G, self.A, self.device
        b = torch.as_tensor(np.ascontiguousarray(boards, dtype=np.int8).reshape(G, A))
        nz = (b != 0).sum(dim=1).to(torch.int32)
        p = torch.as_tensor(np.ascontiguousarray(players, dtype=np.int8).reshape(G))
        lm = torch.as_tensor(np.ascontiguousarray(last_moves, dtype=np.int32).reshape(G))
        mc = nz if move_counts is None else torch.as_tensor(np.asarray(move_counts, dtype=np.int32).reshape(G))
        b, p, lm, mc = (t.to(dev).contiguous() for t in (b, p, lm, mc))
        check(self.lib.gmz_engine_copy_state(self.handle, 1, ptr(b), ptr(p), ptr(lm), ptr(mc), self._stream()))
        torch.cuda.current_stream().synchronize()
        self._n_legal = (A - nz.numpy()).astype(np.int32)
        self._status_event = None

    def set_positions_device(self, boards, players, last_moves, move_counts, n_legal_host):
        """:meth:`set_positions` on device tensors (boards int8 [G, A] or [G, S, S], players int8 [G], last_moves
        int32 [G], move_counts int32 [G], contiguous, on this engine's device): four device copies on the current
        stream, no synchronisation and nothing read back.  The legal-move counts the host needs to size the searches
        come from the caller: ``n_legal_host`` int [G], A minus the stones on each board (0 for a row that
        set_active leaves out)."""
        G, A, dev = self.G, self.A, self.device
        want = ((boards, torch.int8, G * A), (players, torch.int8, G), (last_moves, torch.int32, G),
                (move_counts, torch.int32, G))
        for t, dt, numel in want:
            if not torch.is_tensor(t) or t.dtype != dt or t.numel() != numel or t.device.type != dev.type \
                    or not t.is_contiguous():
                raise ValueError("set_positions_device: expected a contiguous %s tensor of %d elements on %s" %
                                 (dt, numel, dev))
        nl = np.array(n_legal_host, dtype=np.int32).reshape(-1)
        if nl.shape != (G,) or nl.min() < 0 or nl.max() > A:
            raise ValueError("set_positions_device: n_legal_host must hold %d counts in 0..%d" % (G, A))
        check(self.lib.gmz_engine_copy_state(self.handle, 1, ptr(boards), ptr(players), ptr(last_moves),
                                             ptr(move_counts), self._stream()))
        self._n_legal = nl
        self._status_event = None

    def set_active(self, mask=None):
        """Search only the games whose ``mask`` byte is nonzero (uint8/bool [G], host array; None: every game,
        the default).  An inactive game joins no wave and adds nothing to the tree counters; search() gives it
        action -1 and play() leaves it untouched with status 3.  The other games are searched exactly as
        without a mask (gmz_engine_set_active).  Holds from the next search on."""
        if mask is None:
            self._active = None
            check(self.lib.gmz_engine_set_active(self.handle, None, self._stream()))
            return
        m = np.ascontiguousarray(np.asarray(mask).reshape(self.G) != 0)
        d = torch.as_tensor(m.astype(np.uint8)).to(self.device)
        check(self.lib.gmz_engine_set_active(self.handle, ptr(d), self._stream()))
        d.record_stream(torch.cuda.current_stream(self.device))
        self._active = m

    def set_active_device(self, mask_dev, mask_host):
        """:meth:`set_active` without the upload: ``mask_dev`` is the mask as a contiguous uint8 [G] tensor on this
        engine's device (copied into the engine on the current stream), ``mask_host`` the same mask on the host,
        which sizes the searches.  No synchronisation."""
        if not torch.is_tensor(mask_dev) or mask_dev.dtype != torch.uint8 or mask_dev.numel() != self.G \
                or mask_dev.device.type != self.device.type or not mask_dev.is_contiguous():
            raise ValueError("set_active_device: expected a contiguous uint8 tensor of %d bytes on %s" %
                             (self.G, self.device))
        m = np.ascontiguousarray(np.asarray(mask_host).reshape(self.G) != 0)
        check(self.lib.gmz_engine_set_active(self.handle, ptr(mask_dev), self._stream()))
        mask_dev.record_stream(torch.cuda.current_stream(self.device))
        self._active = m

    def set_simulations(self, n):
        """Simulations per search from the next search on, 1 <= n <= the NUM_SIMULATIONS the engine was built
        with: the searches are then those of an engine built with n (gmz_engine_set_simulations).  Between
        moves only."""
        n = int(n)
        if n == self._run_cfg.num_simulations:
            return
        if self._budgets is not None and n < int(self._budgets.max()):
            raise ValueError("set_simulations: %d is below the largest per-game budget (%d); change or clear "
                             "set_budgets first" % (n, int(self._budgets.max())))
        check(self.lib.gmz_engine_set_simulations(self.handle, n))
        if n not in self._sims_tables:
            ec = _lib.EngineCfg.from_buffer_copy(self.ecfg)
            ec.num_simulations = n
            self._sims_tables[n] = (ec, slot_need_table(ec, self.A, self.mode, self.lib))
        self._run_cfg, self._slot_need = self._sims_tables[n]

    def set_budgets(self, sims=None, stream=None):
        """A simulation budget per game from the next search on: ``sims`` an integer array [G] with
        1 <= sims[g] <= the current simulations (NUM_SIMULATIONS, or set_simulations'), or None for the engine's
        budget in every game again.  Game g is then searched exactly as by an engine built with sims[g]
        simulations, in the same launches as the others; a game that has used its budget leaves the remaining
        waves (gmz_engine_set_budgets).  The array goes up through a pinned staging pair on ``stream`` (default:
        the current one), with no host wait.  Between moves only; not with play_refill (the arena)."""
        s = self._stream(stream)
        if sims is None:
            if self._budgets is not None:
                check(self.lib.gmz_engine_set_budgets(self.handle, None, 0, s))
                self._budgets = None
            return
        if self._refill is not None:
            raise ValueError("set_budgets: not on an engine that play_refill drives (the arena's slots change games)")
        a = np.asarray(sims)
        if a.shape != (self.G,) or a.dtype.kind not in "iu":
            raise ValueError("set_budgets: expected an integer array of %d simulation counts" % self.G)
        cap = self._run_cfg.num_simulations
        if a.min() < 1 or a.max() > cap:
            raise ValueError("set_budgets: every budget must be in [1, %d] (the engine's simulations), got %d..%d" %
                             (cap, int(a.min()), int(a.max())))
        a = a.astype(np.int32)
        if self._budgets is not None and np.array_equal(a, self._budgets):
            return  # the engine holds these already
        if self._bud_dev is None:
            self._bud_dev = torch.empty(self.G, dtype=torch.int32, device=self.device)
            self._bud_stage = _PinnedPair(self.G, torch.int32)
        self._bud_stage.upload(a, self._bud_dev, stream)
        check(self.lib.gmz_engine_set_budgets(self.handle, ptr(self._bud_dev), _lib.nbytes(self._bud_dev), s))
        self._budgets = a

    @property
    def budgets(self):
        """The budgets set_budgets holds (int32 [G], a copy), None when none are set."""
        return None if self._budgets is None else self._budgets.copy()

    def _budget_waves(self, nl):
        """(waves of the slowest game, waves per game) of searches at the legal counts ``nl`` with each game's own
        budget (gmz_engine_waves_for_budgets)."""
        nl = np.ascontiguousarray(nl, dtype=np.int32)
        per = np.empty(self.G, np.int32)
        out = ctypes.c_int32()
        check(self.lib.gmz_engine_waves_for_budgets(
            ctypes.byref(self._run_cfg), nl.ctypes.data_as(ctypes.c_void_p),
            self._budgets.ctypes.data_as(ctypes.c_void_p), self.G, ctypes.byref(out),
            per.ctypes.data_as(ctypes.c_void_p)))
        return out.value, per

    def _budget_need(self, nl):
        """Hidden-state slots per game at the legal counts ``nl`` with budgets set: a game's own waves + 2 for
        MuZero, its own budget + 2 for AlphaZero (slot_need_table's rule per game)."""
        if self.mode == 0:
            return self._budgets.astype(np.int64) + 2
        return self._budget_waves(nl)[1].astype(np.int64) + 2

    def _legal_counts(self):
        """The legal-move count each game's coming search sees: 0 for a game outside the active mask."""
        return self._n_legal if self._active is None else np.where(self._active, self._n_legal, 0).astype(np.int32)

    def reset_games(self, mask=None):
        m = None
        if mask is not None:
            m = torch.as_tensor(np.asarray(mask, dtype=np.uint8)).to(self.device)
            self._n_legal[np.asarray(mask, dtype=bool)] = self.A
        else:
            self._n_legal[:] = self.A
        check(self.lib.gmz_engine_reset_games(self.handle, ptr(m), self._stream()))

    # ------------------------------------------------------------------ search
    def sync_status(self):
        """Wait for the last play's status read-back (if one is pending): raises on the engine's error bits, and
        brings the legal counts (and play_refill's counters) up to date.  search_steps calls it."""
        if self._status_event is not None:
            self._status_event.synchronize()
            err = int(self._err_host[0])
            if err:  # a void search must not reach self-play records or the replay buffer
                what = []
                if err & 1 or not err & 2:
                    what.append("a search passed its game's hidden-state "
                                "slot budget, so that game's search result is void")
                if err & 2:
                    what.append("a game's simulation budget was outside [1, the engine's simulations] and was clamped "
                                "into it, so that game was not searched with the budget asked for "
                                "(gmz_engine_set_budgets)")
                raise GmzError("engine error bits 0x%x after the last move: %s (gmz_engine_errors)" %
                               (err, "; ".join(what)))
            if self._refill_pending:  # play_refill: the slots' legal counts come back exact (0 = idle slot)
                r = self._refill
                self._n_legal[:] = r["host"].numpy()[:self.G]
                self.finished_seen = int(r["host"][self.G])
                self.moves_played += int((self._status_host.numpy() != 3).sum())
                self._refill_pending = False
                self._status_event = None
                return
            st = self._status_host.numpy()
            ended = st != 2
            played = st != 3
            self._n_legal[played & ~ended] -= 1
            if self._last_reset and self._book is not None:  # restarted from the book: the draw is a pure function
                again = np.nonzero(played & ended)[0]
                self._book["serial"][again] += 1
                self._n_legal[again] = self.A - self.book_draws(again)[2]
            elif self._last_reset:
                self._n_legal[played & ended] = self.A
            else:
                self._n_legal[played & ended] = np.maximum(self._n_legal[played & ended] - 1, 0)
            self._status_event = None

    def _place_hidden(self, s, stream=None):
        """Give every game the hidden-state slots its coming search can use: waves(L) + 2 for MuZero at
        its legal count L (num_simulations + 2 for AlphaZero), packed game after game into the network's
        pool.  L is known exactly after set_positions / reset_games; after a play() whose status has not
        been read yet it is the last search's L - 1, or A for a game that ended and restarted: the larger
        need of the two is taken.  The bases change only when a game's need does (late-game positions with
        fewer than NUM_TOP_ACTIONS legal moves); then they are copied to the device on the search's stream."""
        nl = self._legal_counts()
        if self._budgets is not None:  # each game at its own budget for the coming search, the same rule
            if self._status_event is not None:
                need = np.maximum(self._budget_need(np.clip(self._n_legal - 1, 0, self.A)),
                                  self._budget_need(np.full(self.G, self.A, np.int32)))
            else:
                need = self._budget_need(np.clip(nl, 0, self.A))
        elif self._status_event is not None:  # a move was played since nl was read (play_refill: or a slot was
            # refilled from an opening with >= NUM_TOP_ACTIONS legal cells, whose need is that of the empty board)
            need = np.maximum(self._slot_need[np.clip(self._n_legal - 1, 0, self.A)], self._slot_need[self.A])
        else:
            need = self._slot_need[np.clip(nl, 0, self.A)]
        base = np.zeros(self.G, np.int64)
        np.cumsum(need[:-1], out=base[1:])
        total = int(base[-1] + need[-1])
        key = np.concatenate([base, need])
        if self._hb_last is not None and np.array_equal(key, self._hb_last):
            if self._hb_net is not self.net:  # the backend was changed between moves: its pool must hold the slots
                if hasattr(self.net, "ensure_slots"):
                    self.net.ensure_slots(total, stream)
                self._hb_net = self.net
            return
        if total >= 2 ** 31:
            raise ValueError("hidden-state pool: %d slots exceed the int32 slot index" % total)
        if hasattr(self.net, "ensure_slots"):
            self.net.ensure_slots(total, stream)
        self._hb_net = self.net
        self._hb_stage.upload(key, self._hb_dev, stream)  # on the search's stream
        check(self.lib.gmz_engine_set_hidden_bases(self.handle, ptr(self.root_slot), s))
        check(self.lib.gmz_engine_set_hidden_budget(self.handle, ptr(self.hidden_budget), s))
        self._hb_last = key
        self.hidden_slots_used = total

    def errors(self, reset=False):
        """Sticky error bits of the engine's kernels (synchronises the device; gmz_engine_errors): bit 0 = a
        search created more nodes than its game's hidden-state budget (its result is void; no other game's
        states were touched); bit 1 = a simulation budget handed to gmz_engine_set_budgets was outside [1, the
        engine's simulations] and was clamped into that range (that game searched with 1 or with the engine's
        budget; every other game is untouched)."""
        out = ctypes.c_int32()
        check(self.lib.gmz_engine_errors(self.handle, ctypes.byref(out), 1 if reset else 0))
        return out.value

    def waves_needed(self):
        if self._budgets is not None:  # the slowest game at its own budget
            return self._budget_waves(self._legal_counts())[0]
        out = ctypes.c_int32()
        nl = np.ascontiguousarray(self._legal_counts(), dtype=np.int32)
        check(self.lib.gmz_engine_waves_for_legal(ctypes.byref(self._run_cfg), nl.ctypes.data_as(ctypes.c_void_p),
                                                  self.G, ctypes.byref(out)))
        return out.value

    def search(self, gumbel=None, stream=None):
        """One search for every game (mcts.py:288-362 / 197-280).  ``gumbel``: optional f64[G,A]
        noise (host or device); default = device noise from (seed, move counter).
        Returns device tensors (policy f64[G,A], value f32[G], action int32[G])."""
        for _ in self.search_steps(gumbel, stream):
            pass
        return self.policy, self.root_value, self.action

    def search_steps(self, gumbel=None, stream=None):
        """:meth:`search` as a generator that yields after each simulation wave has been enqueued
        (SplitSelfPlayEngine interleaves the waves of engines on different streams)."""
        s = self._stream(stream)
        L = self.lib
        g = None
        if gumbel is not None:
            g = torch.as_tensor(gumbel, dtype=torch.float64).to(self.device).contiguous()
        self._place_hidden(s, stream)
        check(L.gmz_engine_begin_move(self.handle, ptr(g), self.seed, ptr(self.obs), s))
        self.net.initial(self.obs, self.root_slot, self.logits, self.value, s)
        check(L.gmz_engine_set_root(self.handle, ptr(self.logits), ptr(self.value), s))
        self.sync_status()  # previous move's status → legal counts (overlaps the root inference)
        waves = self.waves_needed()
        self.waves_last = waves
        rw = ptr(self.reward) if self.mode == 1 else None
        if waves > 0:
            check(L.gmz_engine_select(self.handle, ptr(self.in_slot), ptr(self.act_req), ptr(self.out_slot),
                                      ptr(self.obs), s))
        for w in range(waves):
            if self.mode == 1:
                self.net.recurrent(self.in_slot, self.act_req, self.out_slot, self.logits, self.value, self.reward, s)
            else:
                self.net.initial(self.obs, self.out_slot, self.logits, self.value, s)
            if w + 1 < waves and self.fuse_waves:  # backup of this wave + selection of the next in one launch
                if self.tree_timer is not None:
                    self.tree_timer.start()
                check(L.gmz_engine_expand_backup_select(self.handle, ptr(self.logits), ptr(self.value), rw,
                                                        ptr(self.in_slot), ptr(self.act_req), ptr(self.out_slot),
                                                        ptr(self.obs), s))
                if self.tree_timer is not None:
                    self.tree_timer.stop(0)
            else:
                check(L.gmz_engine_expand_backup(self.handle, ptr(self.logits), ptr(self.value), rw, s))
                if w + 1 < waves:
                    check(L.gmz_engine_select(self.handle, ptr(self.in_slot), ptr(self.act_req), ptr(self.out_slot),
                                              ptr(self.obs), s))
            yield w
        check(L.gmz_engine_finish_move(self.handle, ptr(self.policy), ptr(self.root_value), ptr(self.action), s))

    def play(self, action=None, reset_finished=True, stream=None):
        """do_move + get_game_ended for all games.  Returns the device status tensor
        (+1/-1 winner, 0 draw, 2 ongoing, 3 untouched)."""
        s = self._stream(stream)
        a = self.action if action is None else torch.as_tensor(action, dtype=torch.int32).to(self.device)
        if self._book is not None and reset_finished:  # ended games restart from the book, not from the empty board
            if (self._book["serial"] < 0).any():
                raise ValueError("play: a book is set (set_book); fill_from_book() places the first games")
            self._play_book(a, s)
        else:
            check(self.lib.gmz_engine_play(self.handle, ptr(a), ptr(self.status), 1 if reset_finished else 0, s))
        self._post_status(stream)
        self._last_reset = bool(reset_finished)
        return self.status

    # ------------------------------------------------------------------ self-play's opening book
    def set_book(self, book, symmetry=True, tally=None):
        """Ended games restart from a book of openings instead of the empty board (gmz_engine_play_book): ``book`` =
        (boards, players, last_moves, move_counts) that openings.check_selfplay_book accepts under this engine's
        configuration, uploaded once, or a BookBuffers that another engine made (the parts of a split engine share
        one).  Each new game of slot g draws its opening and, with ``symmetry``, one of the square's eight maps from
        (seed, g + game_offset, the slot's game serial) alone: openings.book_draw gives the host the same draw, so
        nothing is read back.  ``tally``: an int32 [n, 3] device tensor to count the finished games per opening in
        (black won, white won, draw; default: a new one, ``book_tally``).  Call fill_from_book() next; from then on
        play(reset_finished=True) restarts from the book.  Between moves only."""
        if self._refill is not None:
            raise ValueError("set_book: not on an engine that play_refill drives (the arena has its own book)")
        bb = book if isinstance(book, BookBuffers) else BookBuffers(book, self.cfg, self.device)
        if bb.A != self.A:
            raise ValueError("set_book: the book's boards are not this engine's size")
        G, dev = self.G, self.device
        if tally is None:
            tally = torch.zeros(bb.n, 3, dtype=torch.int32, device=dev)
        if not torch.is_tensor(tally) or tally.dtype != torch.int32 or tally.numel() != 3 * bb.n \
                or tally.device.type != dev.type or not tally.is_contiguous():
            raise ValueError("set_book: tally must be a contiguous int32 [%d, 3] tensor on %s" % (bb.n, dev))
        self._book = dict(buf=bb, symmetry=bool(symmetry), tally=tally,
                          slot_serial=torch.full((G,), -1, dtype=torch.int32, device=dev),
                          slot_draw=torch.full((G,), -1, dtype=torch.int32, device=dev),
                          serial=np.full(G, -1, np.int64), keys=np.arange(G, dtype=np.int64) + int(self.ecfg.game_offset))
        return bb

    @property
    def book_tally(self):
        """Finished games per opening of the book, int32 [n, 3] on the device: black won, white won, draw."""
        return None if self._book is None else self._book["tally"]

    def book_draws(self, slots=None, serials=None):
        """(opening t, symmetry d, stones) of the games ``serials`` of the slots ``slots`` (default: every slot's
        current game), computed on the host (openings.book_draw)."""
        k = self._book
        slots = np.arange(self.G) if slots is None else np.asarray(slots, dtype=np.int64)
        serials = k["serial"][slots] if serials is None else np.asarray(serials, dtype=np.int64)
        t, d = book_draw(self.seed, k["keys"][slots], serials, k["buf"].n, k["symmetry"])
        return t, d, k["buf"].counts_host[t]

    def _play_book(self, a, s):
        k = self._book
        bb = k["buf"]
        check(self.lib.gmz_engine_play_book(
            self.handle, ptr(a), ptr(self.status), *bufs(bb.boards, bb.players, bb.last_moves, bb.move_counts), bb.n,
            self.seed % (1 << 64), 1 if k["symmetry"] else 0, ptr(k["slot_serial"]), ptr(k["slot_draw"]), self.G,
            *bufs(k["tally"]), s))

    def fill_from_book(self, stream=None):
        """The first game of every slot from the book (one gmz_engine_play_book launch with every action -1): serial 0
        everywhere.  The legal counts are known on the host at once; nothing is read back."""
        k = self._book
        if k is None:
            raise ValueError("fill_from_book: no book is set (set_book)")
        if (k["serial"] >= 0).any():
            raise ValueError("fill_from_book: the slots hold games from the book already")
        if self._fill_actions is None:
            self._fill_actions = torch.full((self.G,), -1, dtype=torch.int32, device=self.device)
        self.sync_status()
        self._play_book(self._fill_actions, self._stream(stream))
        k["serial"][:] = 0
        self._n_legal = (self.A - self.book_draws()[2]).astype(np.int32)
        self._status_event = None

    def _post_status(self, stream):
        """The status and the engine's error word to their pinned buffers behind a play launch, and the event that
        sync_status waits for."""
        self._status_host.copy_(self.status, non_blocking=True)
        check(self.lib.gmz_engine_errors_async(self.handle, ptr(self._err_host), self._stream(stream)))
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream() if stream is None else stream)
        self._status_event = ev

    def play_refill(self, match, next_net, action=None, stream=None):
        """play(reset_finished=False) plus an arena's bookkeeping in one launch (gmz_engine_play_refill):
        finished games go to ``match``'s result arrays, idle slots start the next opening of network
        ``next_net`` (the one that moves next on this engine) or go inactive.  ``match``: a MatchBuffers,
        shared by the engines of one match.  The slots' legal counts, the status and the match's
        finished-games counter come back through the pinned buffers and the event play() uses, and are read
        at the next search (one ply behind); no host synchronisation here.  Call it from the torch stream
        context of ``stream``.  The first call (``action`` = -1 everywhere) fills the slots."""
        s = self._stream(stream)
        G, dev = self.G, self.device
        if match.A != self.A:
            raise ValueError("play_refill: the book's boards are not this engine's size")
        if self._budgets is not None:
            raise ValueError("play_refill: not with per-game budgets (set_budgets); a refilled slot starts another "
                             "game, whose budget nobody set")
        r = self._refill
        if r is None:
            i32 = torch.int32
            r = self._refill = dict(
                game=torch.full((G,), -1, dtype=i32, device=dev), key=torch.zeros(G, dtype=i32, device=dev),
                ply=torch.zeros(G, dtype=i32, device=dev),
                back=torch.zeros(G + 1, dtype=i32, device=dev),  # legal counts [G], then the finished counter
                host=torch.zeros(G + 1, dtype=i32).pin_memory())
        a = self.action if action is None else torch.as_tensor(action, dtype=torch.int32).to(dev)
        m = match
        check(self.lib.gmz_engine_play_refill(
            self.handle, ptr(a), ptr(self.status), ptr(m.boards), ptr(m.players), ptr(m.last_moves), ptr(m.move_counts),
            m.n_openings, ptr(m.tickets), int(next_net), ptr(r["game"]), ptr(r["key"]), ptr(r["ply"]), ptr(r["back"]), G,
            ptr(m.winner), ptr(m.length), ptr(m.moves), m.A, m.winner.numel(), ptr(m.finished), s))
        r["back"][G:].copy_(m.finished, non_blocking=True)
        r["host"].copy_(r["back"], non_blocking=True)
        self._post_status(stream)
        self._refill_pending = True
        self._active = None  # the device mask is the slots' own now; idle slots report 0 legal cells
        self._last_reset = False
        return self.status

    def keyed_gumbel(self, out, stream=None):
        """The arena's noise for the coming search into ``out`` f64[G,A]: row g from (seed, the slot's opening,
        its game's ply) alone (gmz_gumbel_keyed with play_refill's slot arrays)."""
        r = self._refill
        check(self.lib.gmz_gumbel_keyed(ptr(r["key"]), ptr(r["ply"]), self.seed, self.G, self.A, ptr(out),
                                        _lib.nbytes(out), self._stream(stream)))
        return out

    def _game_ptrs(self):
        """Device pointers of the engine's own boards and players (fetched once), and of play_refill's ``game`` row
        (None on an engine that play_refill does not drive)."""
        if self._state_ptrs is None:
            p = [ctypes.c_void_p() for _ in range(4)]
            check(self.lib.gmz_engine_game_state(self.handle, *[ctypes.byref(x) for x in p]))
            self._state_ptrs = p
        game = self._refill["game"] if self._refill is not None else None
        return self._state_ptrs[0], self._state_ptrs[1], ptr(game)

    def anchor_move(self, noise=None, kind="threat", scale=0.0, stream=None):
        """An anchor opponent's move (gmz_game_anchor_move, see ``anchor_move``) for the side to move on the
        engine's own device boards, in one launch on ``stream`` with no host wait: into ``self.action``, which is
        returned and which play_refill(action=...) takes.  ``noise``: f64[G,A] on the device (keyed_gumbel's) or
        None.  On an engine that play_refill drives, an idle slot gets -1."""
        _call_anchor_move(self.lib, self._game_ptrs(), self.G, self.size, self.cfg.N_IN_ROW,
                          _noise_arg("anchor_move", noise, self.device), kind, scale, self.action, None, stream)
        return self.action

    def vcf_move(self, depth=None, nodes=None, stream=None):
        """The forced-win solver (gmz_game_vcf, see ``vcf``) for the side to move on the engine's own device boards,
        in one launch on ``stream`` with no host wait: where it finds a win its move replaces the entry of
        ``self.action`` (after anchor_move: the threat rule's move), every other entry stays.  Returns
        ``self.action``; the statuses and moves of the launch stay in ``self.vcf_status`` / ``self.vcf_moves``."""
        if self.vcf_status is None:
            self.vcf_status, self.vcf_moves = _status_pair(self.G, self.device)
        outs = self.vcf_status, self.vcf_moves, None, None, self.action
        _call_vcf(self.lib, self._game_ptrs(), self.G, self.size, self.cfg.N_IN_ROW,
                  VCF_DEPTH if depth is None else depth, VCF_NODES if nodes is None else nodes, outs, stream)
        return self.action

    def ab_move(self, noise=None, scale=0.0, plies=None, width=None, nodes=None, stream=None):
        """The alpha-beta anchor (gmz_game_alphabeta, see ``alphabeta``) for the side to move on the engine's own
        device boards, in one launch on ``stream`` with no host wait: where the search finished its move replaces the
        entry of ``self.action`` (after anchor_move: the threat rule's move), every other entry stays.  ``noise``:
        f64[G,A] on the device (keyed_gumbel's) or None.  Returns ``self.action``; the statuses and moves of the
        launch stay in ``self.ab_status`` / ``self.ab_moves``."""
        if self.ab_status is None:
            self.ab_status, self.ab_moves = _status_pair(self.G, self.device)
        outs = self.ab_status, self.ab_moves, None, None, self.action
        _call_alphabeta(self.lib, self._game_ptrs(), self.G, self.size, self.cfg.N_IN_ROW,
                        _noise_arg("ab_move", noise, self.device), scale, AB_PLIES if plies is None else plies,
                        AB_WIDTH if width is None else width, AB_NODES if nodes is None else nodes, outs, stream)
        return self.action

    def winning_scan(self, boards, players, action=None, counters=None, stream=None):
        """workers.py:49-123 find_winning_moves_rebuilt on the device for G positions (see
        ``winning_scan``); ``counters`` = (missed_fives, missed_totals) int32[G] accumulated in place."""
        return winning_scan(boards, players, action, self.cfg.N_IN_ROW, counters, stream, self.lib)

    def tree_counters(self, reset=False):
        """Work done by the fused expand/backup + select launches since the last reset, summed over
        games: dict(backups, backup_levels, selects, select_levels) (gmz_engine_tree_counters)."""
        c = torch.zeros(self.G, 4, dtype=torch.int32, device=self.device)
        check(self.lib.gmz_engine_tree_counters(self.handle, ptr(c), 1 if reset else 0, self._stream()))
        t = c.to(torch.int64).sum(0).tolist()
        return dict(backups=t[0], backup_levels=t[1], selects=t[2], select_levels=t[3])

    def max_visited_children(self):
        """Largest visited-children count of any non-root node in the current trees (diagnostics, synchronous)."""
        out = ctypes.c_int32()
        check(self.lib.gmz_engine_max_visited_children(self.handle, ctypes.byref(out)))
        return out.value

    def root_stats(self):
        G, A, dev = self.G, self.A, self.device
        visits = torch.zeros(G, A, dtype=torch.int32, device=dev)
        rn = torch.zeros(G, dtype=torch.int32, device=dev)
        rw = torch.zeros(G, dtype=torch.float32, device=dev)
        mx = torch.zeros(G, dtype=torch.float32, device=dev)
        mn = torch.zeros(G, dtype=torch.float32, device=dev)
        check(self.lib.gmz_engine_root_stats(self.handle, ptr(visits), ptr(rn), ptr(rw), ptr(mx), ptr(mn),
                                             self._stream()))
        return visits, rn, rw, mx, mn


# the CUs a two-stream engine's tower leaves to the other part's latency-bound tree and head kernels: a 512-game tree
# launch is 512 waves at 4 waves per SIMD (the 15x15 hint kernel's 105 VGPRs), which 32 free CUs hold in one round
# and 24 in two — the cliff below.  Sweep with the round-6 tower
# (tools/cap_sweep.sh, profiles/r06_tower_cap_sweep.txt, 1,024 games, two rounds): cap 192 12,270-12,347 moves/s, 208
# 12,279-12,285, 216 12,321-12,342, 224 = 256 - 32: 12,465-12,515, 232 10,364-10,381, 240 10,257-10,340, no cap 11,357
TOWER_FREE_CUS = 32


class SplitSelfPlayEngine:
    """G games as ``parts`` BatchedSelfPlayEngines of G/parts games, each on its own HIP stream, with
    their simulation waves interleaved on the host (same public interface as BatchedSelfPlayEngine).

    Why: one tower launch fills every CU (a persistent workgroup per CU), and the tree / head kernels
    between two towers are short and latency-bound.  With two halves on two streams and each half's
    tower grid capped at all CUs but TOWER_FREE_CUS (``max_grid``), one half's tree and head kernels run on the
    CUs the other half's tower leaves free, and each tower's ramp-up and tail overlap the other
    half's work (measured with tools/dual_stream_probe.py).  Every game's search is
    exactly the unsplit engine's: part i plays games [i*G/parts, (i+1)*G/parts) with ``game_offset``
    so the device Gumbel noise per game is unchanged, its outputs are row views of the full
    tensors.  Layout and descent hint default per part (from G/parts games: ``default_layout(g)``);
    every default uses the cached-exp softmax, so the results equal one engine's with
    all G games whatever layout each side picks.  Calls fork from the caller's stream and join back."""

    def __init__(self, cfg=None, num_games=2, net=None, device="cuda", seed=0, parts=2, max_grid=None,
                 descent_hint=None, layout=None, pair=None, **overrides):
        self.cfg = from_any(cfg, **overrides)
        c = self.cfg
        G = int(num_games)
        if parts < 1 or G % parts:
            raise ValueError("SplitSelfPlayEngine: num_games must be a multiple of parts")
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.G, self.A, self.size, self.parts = G, c.ACTION_SPACE_SIZE, c.BOARD_SIZE, int(parts)
        self.mode = 1 if c.MCTS_IMPLEMENTATION == "MuZero" else 0
        self.slots_per_game = c.NUM_SIMULATIONS + 2
        g = self.g = G // parts
        # descent_hint / layout None: each part's defaults — the cached-exp softmax in every part, as one
        # engine with every game (the layout may differ per part: results are identical)
        if max_grid is None:  # every CU but TOWER_FREE_CUS for the other part's tree and head kernels
            max_grid = tower_grid_cap(self.device) if parts > 1 else 0
        if net is None:
            net = HashNetBackend(hidden_slots(c, G), self.A, device)
        self.net = net
        nets = net.split(parts, max_grid) if parts > 1 else [net]
        if layout is None:
            layout = default_layout(g)
        self.engines = [BatchedSelfPlayEngine(c, g, nets[i], device, seed, descent_hint, game_offset=i * g,
                                              layout=layout, pair=pair) for i in range(parts)]
        self.streams = engine_streams(self.device, parts)
        dev = self.device
        self.policy = torch.zeros(G, self.A, dtype=torch.float64, device=dev)
        self.root_value = torch.zeros(G, dtype=torch.float32, device=dev)
        self.action = torch.zeros(G, dtype=torch.int32, device=dev)
        self.status = torch.zeros(G, dtype=torch.int8, device=dev)
        for i, e in enumerate(self.engines):  # the parts write straight into row slices
            sl = slice(i * g, (i + 1) * g)
            e.policy, e.root_value, e.action, e.status = self.policy[sl], self.root_value[sl], self.action[sl], self.status[sl]
        self.waves_last = 0

    def _fork(self, stream=None):
        main = stream if stream is not None else torch.cuda.current_stream(self.device)
        fork_streams(main, self.streams)
        return main

    def _rows(self, x, i):
        return None if x is None else x[i * self.g:(i + 1) * self.g]

    # ------------------------------------------------------------------ interface of BatchedSelfPlayEngine
    def close(self):
        for e in self.engines:
            e.close()

    def search(self, gumbel=None, stream=None):
        g = None
        if gumbel is not None:  # to the device on the caller's stream, before the fork
            g = torch.as_tensor(gumbel, dtype=torch.float64).to(self.device).contiguous()
        main = self._fork(stream)
        interleave([(torch.cuda.stream(st), e.search_steps(self._rows(g, i), st))  # one wave of each part in turn
                    for i, (e, st) in enumerate(zip(self.engines, self.streams))])
        join_streams(main, self.streams)
        self.waves_last = max(e.waves_last for e in self.engines)
        return self.policy, self.root_value, self.action

    def play(self, action=None, reset_finished=True, stream=None):
        a = None if action is None else torch.as_tensor(action, dtype=torch.int32).to(self.device)
        main = self._fork(stream)
        for i, (e, st) in enumerate(zip(self.engines, self.streams)):
            with torch.cuda.stream(st):
                e.play(self._rows(a, i), reset_finished)
        join_streams(main, self.streams)
        return self.status

    def set_book(self, book, symmetry=True, tally=None):
        """BatchedSelfPlayEngine.set_book: one book and one tally shared by the parts.  With game_offset the parts
        draw what one engine with every game draws."""
        bb = self.engines[0].set_book(book, symmetry, tally)
        for e in self.engines[1:]:
            e.set_book(bb, symmetry, self.engines[0].book_tally)
        return bb

    @property
    def book_tally(self):
        return self.engines[0].book_tally

    def book_draws(self, slots=None, serials=None):
        slots = np.arange(self.G) if slots is None else np.asarray(slots, dtype=np.int64)
        if serials is None:
            serials = np.concatenate([e._book["serial"] for e in self.engines])[slots]
        e = self.engines[0]  # its keys are the slots themselves (game_offset 0), and every part shares seed and book
        k = e._book
        t, d = book_draw(e.seed, slots, serials, k["buf"].n, k["symmetry"])
        return t, d, k["buf"].counts_host[t]

    def fill_from_book(self, stream=None):
        main = self._fork(stream)
        for e, st in zip(self.engines, self.streams):
            with torch.cuda.stream(st):
                e.fill_from_book()
        join_streams(main, self.streams)

    def set_active(self, mask=None):
        for i, e in enumerate(self.engines):
            e.set_active(None if mask is None else np.asarray(mask).reshape(self.G)[i * self.g:(i + 1) * self.g])

    def set_budgets(self, sims=None):
        """BatchedSelfPlayEngine.set_budgets, each part its own rows; uploaded on the caller's stream, which the
        parts' streams join at the next search."""
        if sims is not None:
            sims = np.asarray(sims)
            if sims.shape != (self.G,):
                raise ValueError("set_budgets: expected an integer array of %d simulation counts" % self.G)
            cap = self.engines[0]._run_cfg.num_simulations
            if sims.dtype.kind not in "iu" or sims.min() < 1 or sims.max() > cap:  # before any part uploads
                raise ValueError("set_budgets: every budget must be an integer in [1, %d]" % cap)
        for i, e in enumerate(self.engines):
            e.set_budgets(None if sims is None else sims[i * self.g:(i + 1) * self.g])

    @property
    def budgets(self):
        parts = [e._budgets for e in self.engines]
        return None if parts[0] is None else np.concatenate(parts)

    def reset_games(self, mask=None):
        for i, e in enumerate(self.engines):
            e.reset_games(None if mask is None else np.asarray(mask)[i * self.g:(i + 1) * self.g])

    def game_state(self):
        parts = [e.game_state() for e in self.engines]
        return tuple(torch.cat([p[k] for p in parts]) for k in range(4))

    def set_positions(self, boards, players, last_moves, move_counts=None):
        b = np.asarray(boards).reshape(self.G, -1)
        p, lm = np.asarray(players).reshape(self.G), np.asarray(last_moves).reshape(self.G)
        mc = None if move_counts is None else np.asarray(move_counts).reshape(self.G)
        for i, e in enumerate(self.engines):
            e.set_positions(self._rows(b, i), self._rows(p, i), self._rows(lm, i), self._rows(mc, i))

    def winning_scan(self, boards, players, action=None, counters=None, stream=None):
        return winning_scan(boards, players, action, self.cfg.N_IN_ROW, counters, stream, self.lib)

    def tree_counters(self, reset=False):
        out = dict(backups=0, backup_levels=0, selects=0, select_levels=0)
        for e in self.engines:
            for k, v in e.tree_counters(reset).items():
                out[k] += v
        return out

    def root_stats(self):
        parts = [e.root_stats() for e in self.engines]
        return tuple(torch.cat([p[k] for p in parts]) for k in range(5))


class MatchBuffers:
    """Device arrays of one arena match, shared by its engines (BatchedSelfPlayEngine.play_refill): the book of
    openings (boards int8[n,S,S], players int8[n] = side to move, last_moves int32[n], move_counts int32[n]), the
    two ticket counters, the finished-games counter and the result arrays indexed by game id = 2 * opening +
    first mover (winner colour, length, and the moves when ``record_moves``)."""

    def __init__(self, boards, players, last_moves, move_counts, record_moves=False, device="cuda"):
        b = np.ascontiguousarray(boards, dtype=np.int8)
        n = b.shape[0]
        self.n_openings, self.A = int(n), int(b[0].size)
        dev = torch.device(device)
        self.boards = torch.as_tensor(b.reshape(n, self.A)).to(dev)
        self.players = torch.as_tensor(np.ascontiguousarray(players, dtype=np.int8).reshape(n)).to(dev)
        self.last_moves = torch.as_tensor(np.ascontiguousarray(last_moves, dtype=np.int32).reshape(n)).to(dev)
        self.move_counts = torch.as_tensor(np.ascontiguousarray(move_counts, dtype=np.int32).reshape(n)).to(dev)
        self.tickets = torch.zeros(2, dtype=torch.int32, device=dev)
        self.finished = torch.zeros(1, dtype=torch.int32, device=dev)
        self.winner = torch.full((2 * n,), 2, dtype=torch.int8, device=dev)  # 2 = not finished
        self.length = torch.zeros(2 * n, dtype=torch.int32, device=dev)
        self.moves = torch.full((2 * n, self.A), -1, dtype=torch.int16, device=dev) if record_moves else None


class BookBuffers:
    """Self-play's book of openings on the device (BatchedSelfPlayEngine.set_book), checked by
    openings.check_selfplay_book under ``cfg``: boards int8 [n, A], players int8 [n] = side to move, last_moves
    int32 [n], move_counts int32 [n]; ``counts_host`` is the stone count per opening for the host's mirror."""

    def __init__(self, book, cfg, device="cuda"):
        b, p, lm, mc = check_selfplay_book(book, cfg)
        self.n, self.A = int(b.shape[0]), int(b.shape[1])
        dev = torch.device(device)
        self.boards, self.players, self.last_moves, self.move_counts = (torch.as_tensor(x).to(dev) for x in (b, p, lm, mc))
        self.counts_host = mc.astype(np.int64)


def engine_cfg(c, num_games, flags=0, game_offset=0):
    """The gmz_engine_cfg (include/gmz.h) of ``num_games`` games under the configuration ``c``."""
    mode = 1 if c.MCTS_IMPLEMENTATION == "MuZero" else 0
    return _lib.EngineCfg(int(num_games), c.BOARD_SIZE, c.N_IN_ROW, c.NUM_SIMULATIONS, c.NUM_TOP_ACTIONS, mode,
                          int(c.C_VISIT), flags, float(c.C_SCALE), float(c.VALUE_MINMAX_DELTA), float(c.DISCOUNT),
                          int(game_offset))


def slot_need(ecfg, mode, L, lib=None):
    """Hidden-state slots one game's search can use at the legal-move count ``L``: MuZero creates the
    root and one node per wave (mcts.py:320-350), i.e. gmz_engine_waves_for_legal(L) + 1, plus one
    spare; AlphaZero one node per simulation (mcts.py:233-268): num_simulations + 2."""
    if mode == 0:
        return ecfg.num_simulations + 2
    out = ctypes.c_int32()
    one = np.array([L], np.int32)
    check((lib if lib is not None else _lib.load()).gmz_engine_waves_for_legal(
        ctypes.byref(ecfg), one.ctypes.data_as(ctypes.c_void_p), 1, ctypes.byref(out)))
    return out.value + 2


def slot_need_table(ecfg, A, mode, lib=None):
    """slot_need by legal-move count L = 0..A (int64 [A + 1])."""
    return np.array([slot_need(ecfg, mode, n, lib) for n in range(A + 1)], np.int64)


def hidden_slots(cfg, num_games):
    """Initial size of the network's hidden-state pool for ``num_games`` games: every game at a legal
    count >= NUM_TOP_ACTIONS (MuZero C2: 102 slots per game instead of NUM_SIMULATIONS + 2 = 402; the
    pool grows if late-game positions need more, BatchedSelfPlayEngine._place_hidden)."""
    c = from_any(cfg)
    ecfg = engine_cfg(c, 1)
    return int(num_games) * slot_need(ecfg, ecfg.mode, c.ACTION_SPACE_SIZE)


def tower_grid_cap(device):
    """The tower grid of one part of a two-stream engine or arena: every CU but TOWER_FREE_CUS (at least half)."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    return max(cus // 2, cus - TOWER_FREE_CUS)


def fork_streams(main, streams):
    """Every stream of ``streams`` waits for what ``main`` holds now."""
    ev = torch.cuda.Event()
    ev.record(main)
    for st in streams:
        st.wait_event(ev)


def join_streams(main, streams):
    """``main`` waits for what every stream of ``streams`` holds now."""
    for st in streams:
        ev = torch.cuda.Event()
        ev.record(st)
        main.wait_event(ev)


def interleave(items):
    """Drive (context, generator) pairs one next() each in turn, each under its context, until all are exhausted
    (search_steps generators on different streams: their waves alternate on the host)."""
    live = list(items)
    while live:
        for item in list(live):
            ctx, gen = item
            with ctx:
                try:
                    next(gen)
                except StopIteration:
                    live.remove(item)


_ENGINE_STREAMS = {}


def engine_streams(device, parts):
    """The HIP streams of the split engines: created once per device and process and shared by every
    SplitSelfPlayEngine (one at a time).  HIP maps each new stream onto the device's hardware queues
    round-robin (GPU_MAX_HW_QUEUES, 4 on MI355X), so streams created later — a second engine's, after a
    trainer's side streams — can land on the queue of the default stream or of each other and serialise
    the two halves: measured 123 vs 90 ms per move for the same worker (profiles/r03_worker_streams.txt)."""
    key = (str(torch.device(device)), parts)
    if key not in _ENGINE_STREAMS:
        _ENGINE_STREAMS[key] = [torch.cuda.Stream(device) for _ in range(parts)]
    return _ENGINE_STREAMS[key]


def default_layout(num_games):
    """Tree layout of the non-root nodes of one engine: 'dense' (a 16-B edge per action) or 'lists'
    (compact lists of the visited children, gmz_engine_cfg.flags bit 3), as measured on k_expand_select
    (profiles/r03_tree_layout_ab.txt): the dense rows in the latency-bound regime (one wave per SIMD
    or less, below 4,096 games), the lists from 4,096 (fewer bytes and instructions per tree level).
    Results are identical either way (tests/test_tree_lists_gpu.py)."""
    return "lists" if num_games >= 4096 else "dense"


def default_pair(num_games):
    """Two waves per game in the fused expand/select kernel (k_expand_select_pair) when one wave per game
    would leave the SIMDs at one wave or fewer: as measured."""
    return PAIR_DEFAULT and num_games <= PAIR_MAX_GAMES


PAIR_DEFAULT = False
PAIR_MAX_GAMES = 2048


def default_streams(cfg, num_games):
    """HIP streams for G games, as measured (profiles/r02_dual_stream_sweep.txt, r02_configs_two_streams.txt):
    two half-size engines for 15x15 MuZero from 256 games up (+5-7 % moves/s: the 0.8 ms tower leaves
    room beside it for the other half's ~0.1 ms of tree and head kernels); one engine otherwise (19x19:
    the 2.6 ms tower dwarfs the rest and loses more to the capped grid, -2 %; 9x9 AlphaZero: -4 %)."""
    c = from_any(cfg)
    if c.BOARD_SIZE == 15 and c.MCTS_IMPLEMENTATION == "MuZero" and num_games >= 256 and num_games % 2 == 0:
        return 2
    return 1


def make_engine(cfg=None, num_games=1, net=None, device="cuda", seed=0, streams=None, **kw):
    """BatchedSelfPlayEngine, or SplitSelfPlayEngine over ``streams`` HIP streams when streams > 1
    (None: default_streams(cfg, num_games))."""
    if streams is None:
        streams = default_streams(cfg, num_games)
    if streams > 1:
        return SplitSelfPlayEngine(cfg, num_games, net, device, seed, parts=streams, **kw)
    return BatchedSelfPlayEngine(cfg, num_games, net, device, seed, **kw)


def _board_args(who, boards, players, game=None, checked=True):
    """(boards, players, game) of the free functions below as contiguous tensors on the boards' device, with G and
    S: (b, p, gm or None, G, S).  ``checked``: ValueError under the caller's name ``who`` unless the boards are int8
    [G, S, S] and players (and game) hold G entries."""
    b = torch.as_tensor(boards).contiguous()
    if checked and (b.dtype != torch.int8 or b.dim() < 2):
        raise ValueError("%s: boards must be int8 [G, S, S]" % who)
    G, S = b.shape[0], b.shape[-1]
    p = torch.as_tensor(players, dtype=torch.int8).to(b.device).contiguous()
    gm = None if game is None else torch.as_tensor(game, dtype=torch.int32).to(b.device).contiguous()
    if checked and (b.numel() != G * S * S or p.numel() != G or (gm is not None and gm.numel() != G)):
        raise ValueError("%s: expected boards [G, S, S] with players (and game) of G entries" % who)
    return b, p, gm, G, S


def winning_scan(boards, players, actions=None, n_in_row=5, counters=None, stream=None, lib=None):
    """Batched workers.py:49-123 ``find_winning_moves_rebuilt`` (``gmz_game_winning_scan``).

    boards int8[G,S,S] and players int8[G] (the player to move) on the device.  Without
    ``actions``: returns uint8[G,S*S] cell classes (0 none, 1 five, 2 open_four, 3 combo).  With
    ``actions`` int32[G] and ``counters`` = (missed_fives, missed_totals) int32[G] device tensors:
    adds the workers.py:191-203 missed-win counts of this position (action < 0: game skipped)."""
    L = lib if lib is not None else _lib.load()
    b, p, _, G, S = _board_args("winning_scan", boards, players, checked=False)
    cls, mf, mt, a = None, None, None, None
    if actions is None:
        cls = torch.zeros(G, S * S, dtype=torch.uint8, device=b.device)
    else:
        a = torch.as_tensor(actions, dtype=torch.int32).to(b.device).contiguous()
        mf, mt = counters
    check(L.gmz_game_winning_scan(ptr(b), ptr(p), ptr(a), G, S, int(n_in_row), ptr(cls), ptr(mf), ptr(mt),
                                  _lib.stream_ptr(stream)))
    return cls


def _noise_arg(who, noise, device):
    """An engine method's ``noise`` as it is, once checked: None, or a contiguous float64 tensor on ``device``."""
    if noise is not None and (not torch.is_tensor(noise) or noise.dtype != torch.float64
                              or noise.device.type != device.type or not noise.is_contiguous()):
        raise ValueError("%s: noise must be a contiguous float64 tensor on %s" % (who, device))
    return noise


def _actions_arg(who, actions, device):
    """A search's ``actions`` as it is, once checked: None, or a contiguous int32 tensor on ``device``."""
    if actions is not None and (not torch.is_tensor(actions) or actions.dtype != torch.int32
                                or actions.device != device or not actions.is_contiguous()):
        raise ValueError("%s: actions must be a contiguous int32 tensor on the boards' device (updated in place)" % who)
    return actions


def _status_pair(G, device):
    """The (status int8[G], moves int32[G]) that a search launch on an engine's own boards leaves behind."""
    return torch.zeros(G, dtype=torch.int8, device=device), torch.full((G,), -1, dtype=torch.int32, device=device)


# One caller per anchor entry point spells its argument list (include/gmz.h).  state: (boards, players, game) pointers
def _call_anchor_move(L, state, G, S, n, noise, kind, scale, actions, scores, stream):
    check(L.gmz_game_anchor_move(*state, *bufs(noise), G, S, int(n), anchor_kind(kind), float(scale),
                                 *bufs(actions, scores), _lib.stream_ptr(stream)))


def _call_vcf(L, state, G, S, n, depth, nodes, outs, stream):
    check(L.gmz_game_vcf(*state, G, S, int(n), int(depth), int(nodes), *bufs(*outs), _lib.stream_ptr(stream)))


def _call_alphabeta(L, state, G, S, n, noise, scale, plies, width, nodes, outs, stream):
    check(L.gmz_game_alphabeta(*state, *bufs(noise), float(scale), G, S, int(n), int(plies), int(width), int(nodes),
                               *bufs(*outs), _lib.stream_ptr(stream)))


ANCHOR_KINDS = {"threat": 0, "uniform": 1}
VCF_DEPTH, VCF_NODES = 10, 2048  # the solver's defaults
AB_PLIES, AB_WIDTH, AB_NODES = 4, 8, 2048  # the alpha-beta anchor's defaults


def anchor_kind(kind):
    """gmz_game_anchor_move's ``kind`` of an anchor's name: 0 for 'threat', 1 for 'uniform'."""
    if kind not in ANCHOR_KINDS:
        raise ValueError("anchor kind must be 'threat' or 'uniform', got %r" % (kind,))
    return ANCHOR_KINDS[kind]


def anchor_move(boards, players, noise=None, kind="threat", scale=0.0, n_in_row=5, game=None, scores=False,
                stream=None):
    """The move of a fixed non-network opponent on G boards (``gmz_game_anchor_move``; the rule: DESIGN.md §8b).

    boards int8[G,S,S] and players int8[G] (the player to move) on the device; ``noise`` f64[G,S*S] or None (= 0).
    ``kind`` 'threat' scores each empty cell by the lines it completes, blocks, builds or breaks, 'uniform' scores
    them all 0; the move is the empty cell with the largest (score + scale * noise, noise, -cell).  With Gumbel noise
    kind='uniform', scale=1 is a uniformly random legal move and kind='threat', scale=0 the deterministic threat
    player whose ties the noise breaks.  ``game`` int32[G]: a negative entry leaves that board out.  Returns
    actions int32[G] (-1: full board or left out), or (actions, scores int64[G,S*S]) with ``scores`` (-1 for an
    occupied cell)."""
    b, p, gm, G, S = _board_args("anchor_move", boards, players, game)
    nz = None if noise is None else torch.as_tensor(noise, dtype=torch.float64).to(b.device).contiguous()
    act = torch.empty(G, dtype=torch.int32, device=b.device)
    sc = torch.empty(G, S * S, dtype=torch.int64, device=b.device) if scores else None
    _call_anchor_move(_lib.load(), (ptr(b), ptr(p), ptr(gm)), G, S, n_in_row, nz, kind, scale, act, sc, stream)
    return (act, sc) if scores else act


def vcf(boards, players, depth=VCF_DEPTH, nodes=VCF_NODES, game=None, actions=None, stream=None, n_in_row=5):
    """The forced-win (VCF) solver on G boards (``gmz_game_vcf``; the rule: DESIGN.md §8b): an exact depth-first
    search, at most ``depth`` attacker moves deep and ``nodes`` nodes per board, for a win of the player to move by
    fours that each force the reply, in one launch.

    boards int8[G,S,S] and players int8[G] on the device.  ``game`` int32[G]: a negative entry skips that board.
    ``actions`` int32[G] on the device is updated in place: entry g becomes the solver's move where it found a win
    and stays as it is everywhere else.  Returns (status int8[G]: 0 none, 1 found, 2 node budget used up, 3 skipped;
    move int32[G], -1 unless status is 1; length int32[G], the attacker moves of the line; nodes int32[G])."""
    b, p, gm, G, S = _board_args("vcf", boards, players, game)
    actions = _actions_arg("vcf", actions, b.device)
    st, mv, ln, nd = (torch.empty(G, dtype=d, device=b.device) for d in (torch.int8,) + 3 * (torch.int32,))
    _call_vcf(_lib.load(), (ptr(b), ptr(p), ptr(gm)), G, S, n_in_row, depth, nodes, (st, mv, ln, nd, actions), stream)
    return st, mv, ln, nd


def alphabeta(boards, players, plies=AB_PLIES, width=AB_WIDTH, nodes=AB_NODES, noise=None, scale=0.0, game=None,
              actions=None, stream=None, n_in_row=5):
    """The depth-limited alpha-beta anchor on G boards (``gmz_game_alphabeta``; the rule: DESIGN.md §8b): a fixed
    negamax search ``plies`` deep over the ``width`` best cells of the threat rule's scores at every node, at most
    ``nodes`` nodes per board, in one launch.

    boards int8[G,S,S] and players int8[G] on the device; ``noise`` f64[G,S*S] or None (= 0) and ``scale`` order the
    root's candidates as ``anchor_move`` orders its cells.  ``game`` int32[G]: a negative entry skips that board.
    ``actions`` int32[G] on the device is updated in place: entry g becomes the move where the search finished and
    stays as it is everywhere else.  Returns (status int8[G]: 0 searched, 2 node budget used up, 3 skipped or a full
    board; move int32[G], -1 unless status is 0; value int64[G], the root's value from the mover's side; nodes
    int32[G])."""
    b, p, gm, G, S = _board_args("alphabeta", boards, players, game)
    actions = _actions_arg("alphabeta", actions, b.device)
    nz = None if noise is None else torch.as_tensor(noise, dtype=torch.float64).to(b.device).contiguous()
    st, mv, val, nd = (torch.empty(G, dtype=d, device=b.device)
                       for d in (torch.int8, torch.int32, torch.int64, torch.int32))
    _call_alphabeta(_lib.load(), (ptr(b), ptr(p), ptr(gm)), G, S, n_in_row, nz, scale, plies, width, nodes,
                    (st, mv, val, nd, actions), stream)
    return st, mv, val, nd
