"""Arena — one network against another on the GPU: a match of 2 * n_openings games from a book of openings, each
opening played once with each network moving first, and the Elo difference with an interval over the pairs.

The searches are the self-play engine's (engine.BatchedSelfPlayEngine, csrc/gmz_tree.hip); what the match adds on
the device is one launch per ply (gmz_engine_play_refill: play, record finished games, start the next opening in
idle slots) and the keyed Gumbel noise (gmz_gumbel_keyed).  DESIGN.md §8b has the invariants:

  * alternation: every active slot of an engine has the same network to move, and the two networks alternate ply
    by ply; a game whose first mover is A starts on an even ply of its engine, one whose first mover is B on an odd
    ply, so an idle slot draws its next game from the counter of the network that moves next;
  * tickets: two atomic counters (openings started with A / with B moving first); game id = 2 * opening + first
    mover; a game's content does not depend on the slot that draws it;
  * noise: keyed by (seed, opening index, ply of the game) — not by the slot, not by who moves first;
  * the host's legal-count mirror comes back exact with each status, one ply behind.

Either side may be an AnchorPlayer instead of a network: a fixed opponent that does not search ("threat": complete a
five, block one, otherwise build or break lines; "uniform": a random legal move; "vcf": the threat player with a
forced-win solver in front of it, gmz_game_vcf; "ab": a depth-limited alpha-beta search over the threat rule's scores
between the two, gmz_game_alphabeta), whose move is one launch (gmz_game_anchor_move; two for "vcf", three for "ab") on
the engine's boards.  Anchors stay the same from run to run, so a score against one is an
absolute strength reading.

    python -m datou_gomoku_muzero_amd.arena --a CKPT --b CKPT --games N [--precision-a fp16 --precision-b bf16
                                                                         --sims-a 400 --sims-b 200]
    python -m datou_gomoku_muzero_amd.arena --a CKPT --b anchor:threat --games N [--anchor-scale X]
    python -m datou_gomoku_muzero_amd.arena --a CKPT --b anchor:vcf --games N [--anchor-depth 10 --anchor-nodes 2048]
    python -m datou_gomoku_muzero_amd.arena --a CKPT --b anchor:ab --games N [--anchor-plies 4 --anchor-width 8
                                                                            --anchor-nodes 2048]
"""
import argparse
import json
import math
import os
import sys
from dataclasses import dataclass, field

import numpy as np

from .openings import paired_openings  # noqa: F401  (the book's builder, numpy only)

Z95 = 1.959963984540054  # the normal distribution's 97.5 % point


# ---------------------------------------------------------------------------------------------- Elo
def elo_from_score(s):
    """Elo difference of a player scoring ``s`` (0..1) per game: -400 log10(1 / s - 1); -inf / +inf at 0 / 1."""
    if s <= 0.0:
        return -math.inf
    if s >= 1.0:
        return math.inf
    return -400.0 * math.log10(1.0 / s - 1.0)


def score_interval(samples, z=Z95):
    """(mean, lo, hi) of independent samples of a score in [0, 1]: the normal approximation mean -+ z * s / sqrt(n)
    with the sample standard deviation (n - 1), clipped to [0, 1]; fewer than two samples give [0, 1]."""
    x = np.asarray(samples, dtype=np.float64)
    n = x.size
    if n == 0:
        return 0.5, 0.0, 1.0
    m = float(x.mean())
    if n < 2:
        return m, 0.0, 1.0
    h = z * float(x.std(ddof=1)) / math.sqrt(n)
    return m, max(0.0, m - h), min(1.0, m + h)


def elo_interval(pair_scores, z=Z95):
    """(elo, lo, hi) from the PAIR scores (A's mean score over the two games of each opening): the two games of an
    opening are not independent, the pairs are.  A score of 0 or 1 gives -inf / +inf."""
    m, lo, hi = score_interval(pair_scores, z)
    return elo_from_score(m), elo_from_score(lo), elo_from_score(hi)


def naive_elo_interval(game_scores, z=Z95):
    """The same over single games as if they were independent (for comparison: too narrow when the two games of an
    opening go the same way)."""
    m, lo, hi = score_interval(game_scores, z)
    return elo_from_score(m), elo_from_score(lo), elo_from_score(hi)


# ---------------------------------------------------------------------------------------------- book
def check_book(openings, cfg):
    """The book as four arrays, refused (ValueError) unless every opening leaves at least NUM_TOP_ACTIONS legal
    cells: for any such legal count the search's wave count is the empty board's, so a slot may start an opening
    one ply before the host learns which one (the engine's hidden-state placement)."""
    boards, players, last, counts = openings
    boards = np.ascontiguousarray(boards, dtype=np.int8)
    n = boards.shape[0]
    A = cfg.ACTION_SPACE_SIZE
    if n < 1 or boards.reshape(n, -1).shape[1] != A:
        raise ValueError("Arena: the book needs at least one opening of BOARD_SIZE x BOARD_SIZE cells")
    boards = boards.reshape(n, A)
    counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(n)
    players = np.ascontiguousarray(players, dtype=np.int8).reshape(n)
    last = np.ascontiguousarray(last, dtype=np.int32).reshape(n)
    if not np.array_equal((boards != 0).sum(axis=1), counts):
        raise ValueError("Arena: an opening's stone count differs from its board")
    if not np.isin(players, (-1, 1)).all():
        raise ValueError("Arena: an opening's side to move must be +1 or -1")
    left = A - counts
    if (left < cfg.NUM_TOP_ACTIONS).any():
        raise ValueError("Arena: every opening must leave at least NUM_TOP_ACTIONS = %d legal cells (opening %d "
                         "leaves %d)" % (cfg.NUM_TOP_ACTIONS, int(np.argmin(left)), int(left.min())))
    return boards, players, last, counts


# ---------------------------------------------------------------------------------------------- result
@dataclass
class GameResult:
    opening: int
    first_mover: str      # "a" or "b"
    winner: str           # "a", "b" or "draw"
    winner_colour: int    # +1 black, -1 white, 0 draw
    length: int           # moves played after the opening
    moves: list = None    # the moves when recorded


@dataclass
class MatchResult:
    games: list
    tally: dict = field(default_factory=dict)  # tally[net][colour] = dict(wins, draws, losses)
    score_a: float = 0.5
    elo: float = 0.0
    elo_lo: float = -math.inf
    elo_hi: float = math.inf
    pair_scores: list = field(default_factory=list)
    plies: int = 0
    moves_played: int = 0
    seconds: float = 0.0

    def as_dict(self):
        def f(x):
            return x if math.isfinite(x) else ("inf" if x > 0 else "-inf")
        return dict(games=len(self.games), score_a=self.score_a, elo=f(self.elo), elo_lo=f(self.elo_lo),
                    elo_hi=f(self.elo_hi), tally=self.tally, plies=self.plies, moves_played=self.moves_played,
                    seconds=self.seconds)


def summarise(winner_colour, length, book_players, moves=None):
    """MatchResult from the result arrays indexed by game id = 2 * opening + first mover (0 = A, 1 = B): the first
    mover plays the opening's side to move."""
    n = len(book_players)
    tally = {k: {c: dict(wins=0, draws=0, losses=0) for c in ("black", "white")} for k in ("a", "b")}
    games, score = [], np.zeros((n, 2))
    for gid in range(2 * n):
        t, first = gid >> 1, gid & 1
        w = int(winner_colour[gid])
        if w not in (-1, 0, 1):
            raise RuntimeError("arena: game %d has no result" % gid)
        first_colour = int(book_players[t])
        colour = {("a", "b")[first]: first_colour, ("b", "a")[first]: -first_colour}
        names = {v: k for k, v in colour.items()}
        for net in ("a", "b"):
            slot = tally[net]["black" if colour[net] == 1 else "white"]
            slot["draws" if w == 0 else "wins" if w == colour[net] else "losses"] += 1
        score[t, first] = 0.5 if w == 0 else (1.0 if w == colour["a"] else 0.0)
        mv = None
        if moves is not None:
            mv = [int(x) for x in moves[gid][:int(length[gid])]]
        games.append(GameResult(t, ("a", "b")[first], "draw" if w == 0 else names[w], w, int(length[gid]), mv))
    pairs = score.mean(axis=1)
    elo, lo, hi = elo_interval(pairs)
    return MatchResult(games=games, tally=tally, score_a=float(pairs.mean()), elo=elo, elo_lo=lo, elo_hi=hi,
                       pair_scores=[float(x) for x in pairs])


# ---------------------------------------------------------------------------------------------- anchors
ANCHOR_PREFIX = "anchor:"


@dataclass
class AnchorPlayer:
    """A fixed opponent that does not search a tree (engine.anchor_move), as a side of an Arena.
    ``kind`` "threat": the one-ply threat player; "uniform": a random legal move; "vcf": the forced-win solver's move
    (engine.vcf: at most ``depth`` attacker moves and ``nodes`` nodes per board) where it finds a win by continuous
    fours, the threat player's move everywhere else; "ab": the solver's move where a forced win exists, else the move
    of the alpha-beta search (engine.alphabeta: ``plies`` deep over the ``width`` best cells of a node, at most ``nodes``
    nodes per board, the budget of each of the two searches) where that search finished, else the threat player's.
    ``scale`` multiplies the keyed Gumbel noise added to the cell scores (None: 0 for threat, vcf and ab, where the
    noise only breaks ties, and 1 for uniform)."""
    kind: str = "threat"
    scale: float = None
    depth: int = 10
    nodes: int = 2048
    plies: int = 4
    width: int = 8

    def checked(self):
        """(kind, scale) with the default scale filled in, (kind, scale, depth, nodes) for "vcf" and (kind, scale,
        depth, nodes, plies, width) for "ab"; ValueError for an unknown kind, a scale that is negative or not finite,
        for "vcf" and "ab" a depth outside [1, 16] or nodes outside [1, 1 << 20], or, for "ab", plies outside [1, 8]
        or a width outside [1, 16]."""
        if self.kind not in ("threat", "uniform", "vcf", "ab"):
            raise ValueError("AnchorPlayer: kind must be 'threat', 'uniform', 'vcf' or 'ab', got %r" % (self.kind,))
        scale = (1.0 if self.kind == "uniform" else 0.0) if self.scale is None else float(self.scale)
        if not (scale >= 0.0 and math.isfinite(scale)):
            raise ValueError("AnchorPlayer: scale must be finite and >= 0, got %r" % (self.scale,))
        if self.kind not in ("vcf", "ab"):
            return self.kind, scale
        limits = [("depth", self.depth, 16), ("nodes", self.nodes, 1 << 20)]
        if self.kind == "ab":
            limits += [("plies", self.plies, 8), ("width", self.width, 16)]
        for what, v, hi in limits:
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= hi:
                raise ValueError("AnchorPlayer: %s must be an integer in [1, %d], got %r" % (what, hi, v))
        return (self.kind, scale) + tuple(int(v) for _, v, _ in limits)

    @property
    def name(self):
        return ANCHOR_PREFIX + self.kind


def anchor_from_name(name, scale=None, depth=None, nodes=None, plies=None, width=None):
    """AnchorPlayer of "anchor:threat" / "anchor:uniform" / "anchor:vcf" / "anchor:ab" (``depth`` and ``nodes``: the
    solver's limits, ``plies``, ``width`` and ``nodes``: the alpha-beta search's; None = AnchorPlayer's defaults); None
    for any other string (a checkpoint path)."""
    if isinstance(name, str) and name.startswith(ANCHOR_PREFIX):
        a = AnchorPlayer(name[len(ANCHOR_PREFIX):], scale)
        for what, v in (("depth", depth), ("nodes", nodes), ("plies", plies), ("width", width)):
            if v is not None:
                setattr(a, what, v)
        return a
    return None


# ---------------------------------------------------------------------------------------------- arena
def default_arena_streams(cfg, num_slots):
    """Engines (HIP streams) of an arena, as measured (profiles/arena.txt): two half-size engines offset by one ply
    where self-play splits too (engine.default_streams: 15x15 MuZero from 256 slots; 12,705-12,717 against
    11,702-11,748 moves/s at 1,024 slots, 400 simulations), one engine otherwise."""
    from .engine import default_streams
    return default_streams(cfg, num_slots)


class Arena:
    """A match between two sides, each an engine backend (network.GomokuNetHip of any precision or depth, or
    engine.HashNetBackend) or an AnchorPlayer, on ``num_slots`` slots.  ``openings``: (boards, players, last_moves,
    move_counts) as paired_openings returns; every opening is played twice, once with each side moving first.
    ``streams=2``: two engines of num_slots / 2 slots on two HIP streams, offset by one ply so that both sides work
    at every ply; the games are the same ones.  ``sims=(n_a, n_b)``: a simulation budget per network (ignored for
    an anchor side).  On an anchor's ply an engine runs the keyed noise, the anchor's launch (for "vcf" the threat
    launch, then the solver's over the same actions; for "ab" the alpha-beta launch between the two) and play_refill,
    and no search."""

    def __init__(self, cfg, net_a, net_b, num_slots, openings, seed=0, record_moves=False, streams=None,
                 device="cuda", sims=None, **overrides):
        from . import engine as E
        from .config import from_any
        self.cfg = from_any(cfg, **overrides)
        # per side: None for a network, (kind, scale) for an anchor
        self.anchors = [s.checked() if isinstance(s, AnchorPlayer) else None for s in (net_a, net_b)]
        self.book = check_book(openings, self.cfg)
        # simulations per search of network A and of network B (default: the configuration's for both); the
        # engines are built for the larger budget
        self.sims = (self.cfg.NUM_SIMULATIONS,) * 2 if sims is None else (int(sims[0]), int(sims[1]))
        searching = [n for n, a in zip(self.sims, self.anchors) if a is None]  # an anchor does not search
        if searching and min(searching) < 1:
            raise ValueError("Arena: sims must be positive")
        built = max(searching) if searching else 1  # anchors only: the engines keep the boards, their trees idle
        if built != self.cfg.NUM_SIMULATIONS:
            self.cfg = from_any(self.cfg, NUM_SIMULATIONS=built)
        self.n_openings = self.book[0].shape[0]
        if streams is None:
            streams = default_arena_streams(self.cfg, num_slots)
        if streams not in (1, 2):
            raise ValueError("Arena: streams must be 1 or 2")
        if num_slots < streams or num_slots % streams:
            raise ValueError("Arena: num_slots must be a positive multiple of streams")
        import torch
        self.torch, self.E = torch, E
        self.device = torch.device(device)
        self.seed, self.record_moves, self.parts = int(seed), bool(record_moves), int(streams)
        self.num_slots = int(num_slots)
        g = self.num_slots // self.parts
        self.streams = E.engine_streams(self.device, self.parts) if self.parts > 1 else [None]
        self.nets = self._views(net_a, net_b)
        # an engine starts with its first mover's backend, or the other side's when that one is an anchor (anchors
        # only: None, the engine's own HashNetBackend, never run)
        first = [self.nets[i][i % 2] if self.nets[i][i % 2] is not None else self.nets[i][1 - i % 2]
                 for i in range(self.parts)]
        self.engines = [E.BatchedSelfPlayEngine(self.cfg, g, first[i], device, self.seed) for i in range(self.parts)]
        self.A = self.cfg.ACTION_SPACE_SIZE
        self.gumbel = [torch.zeros(g, self.A, dtype=torch.float64, device=self.device) for _ in range(self.parts)]
        self.match = None

    def _views(self, net_a, net_b):
        """Per engine the pair (A's backend, B's backend), None in an anchor's place: with two engines a view of
        each network per engine, with its own pool slice and workspace."""
        if self.parts == 1:
            return [tuple(None if a is not None else n for n, a in zip((net_a, net_b), self.anchors))]
        cap = self.E.tower_grid_cap(self.device)
        va, vb = [[None] * self.parts if a is not None else n.split(self.parts, cap)
                  for n, a in zip((net_a, net_b), self.anchors)]
        return [(va[i], vb[i]) for i in range(self.parts)]

    def set_sides(self, side_a, side_b, sims=None):
        """Other sides (backends or AnchorPlayers) for the next run() on the same engines, streams and book.  A
        network side's simulations (``sims``, default: kept) must be within what the engines were built for."""
        anchors = [s.checked() if isinstance(s, AnchorPlayer) else None for s in (side_a, side_b)]
        sims = self.sims if sims is None else (int(sims[0]), int(sims[1]))
        searching = [n for n, a in zip(sims, anchors) if a is None]
        if searching and not 1 <= min(searching) <= max(searching) <= self.cfg.NUM_SIMULATIONS:
            raise ValueError("Arena.set_sides: sims must be in [1, %d], what the engines were built for" %
                             self.cfg.NUM_SIMULATIONS)
        self.anchors, self.sims = anchors, sims
        self.nets = self._views(side_a, side_b)

    def close(self):
        for e in self.engines:
            e.close()

    def _ctx(self, i):
        import contextlib
        st = self.streams[i]
        return self.torch.cuda.stream(st) if st is not None else contextlib.nullcontext()

    def start(self):
        """Fresh match buffers, and the slots filled with the first games: engine i's first mover is network i % 2."""
        torch = self.torch
        m = self.match = self.E.MatchBuffers(*self.book, record_moves=self.record_moves, device=self.device)
        g = self.engines[0].G
        none = torch.full((g,), -1, dtype=torch.int32, device=self.device)
        self._main = torch.cuda.current_stream(self.device)
        if self.parts > 1:
            self.E.fork_streams(self._main, self.streams)
        for i, e in enumerate(self.engines):
            e.finished_seen = e.moves_played = 0
            with self._ctx(i):
                e.play_refill(m, i % 2, action=none, stream=self.streams[i])
        self.ply = 0

    def step(self):
        """One ply of every engine: engine i searches with network (ply + i) % 2 under the keyed noise, plays, and
        refills its idle slots with openings of the other network, which moves next.  Where that side is an anchor
        the search is one launch of its move rule on the same noise."""
        gens, actions = [], [None] * self.parts
        for i, e in enumerate(self.engines):
            k = (self.ply + i) % 2
            with self._ctx(i):
                e.keyed_gumbel(self.gumbel[i], self.streams[i])
                if self.anchors[k] is not None:
                    kind, scale = self.anchors[k][:2]
                    if kind in ("vcf", "ab"):
                        # the threat rule's move, the alpha-beta move over it where that search finished ("ab"), then
                        # the solver's over both where it found a win
                        depth, nodes = self.anchors[k][2:4]
                        e.anchor_move(self.gumbel[i], "threat", scale, self.streams[i])
                        if kind == "ab":
                            e.ab_move(self.gumbel[i], scale, *self.anchors[k][4:], nodes=nodes, stream=self.streams[i])
                        actions[i] = e.vcf_move(depth, nodes, stream=self.streams[i])
                    else:
                        actions[i] = e.anchor_move(self.gumbel[i], kind, scale, self.streams[i])
                    continue
                e.net = self.nets[i][k]
                e.set_simulations(self.sims[k])
                gens.append((self._ctx(i), e.search_steps(self.gumbel[i], self.streams[i])))
        self.E.interleave(gens)  # one wave of each engine in turn
        for i, e in enumerate(self.engines):
            if actions[i] is not None:
                # no search has read the last ply's status (a search does, to size its waves): read it before this
                # ply's play_refill overwrites the pinned buffers, or the counters and the legal counts lose a ply
                e.sync_status()
            with self._ctx(i):
                e.play_refill(self.match, (self.ply + i + 1) % 2, action=actions[i], stream=self.streams[i])
        self.ply += 1

    def finished(self):
        """Games finished as of the statuses read so far (one ply behind the device)."""
        return max(e.finished_seen for e in self.engines)

    def join(self):
        """The engines' streams joined into the caller's, and the last ply's statuses read."""
        if self.parts > 1:
            self.E.join_streams(self._main, self.streams)
        for e in self.engines:
            e.sync_status()
        self.torch.cuda.synchronize(self.device)

    def run(self):
        """Play the match to its end: the loop ends when the finished-games counter, read one ply behind, reaches
        2 * n_openings (a ply or two with every slot idle at the end).  Returns a MatchResult."""
        import time
        torch = self.torch
        total = 2 * self.n_openings
        torch.cuda.synchronize(self.device)
        t0 = time.perf_counter()
        self.start()
        # a game lasts at most A plies; the slots take the 2n games in ceil(2n / slots) rounds per network turn
        limit = 2 * (self.A + 2) * (total // self.num_slots + 2) + 8
        while self.finished() < total:
            if self.ply >= limit:
                raise RuntimeError("arena: %d plies played and the match has not ended" % self.ply)
            self.step()
        self.join()
        seconds = time.perf_counter() - t0
        m = self.match
        if int(m.finished[0]) != total:
            raise RuntimeError("arena: %d of %d games finished" % (int(m.finished[0]), total))
        moves = m.moves.cpu().numpy() if m.moves is not None else None
        res = summarise(m.winner.cpu().numpy(), m.length.cpu().numpy(), self.book[1], moves)
        res.plies, res.seconds = self.ply, seconds
        res.moves_played = sum(e.moves_played for e in self.engines)
        return res


# ---------------------------------------------------------------------------------------------- conveniences
def blocks_of(state_dict):
    """NUM_RES_BLOCKS of a GomokuNetEZ state dict (its representation tower's residual blocks)."""
    ids = {int(k.split(".")[2]) for k in state_dict if k.startswith("representation_net.resblocks.")}
    return max(ids) + 1 if ids else 0


def play_match(sd_a, sd_b, cfg, games, num_slots=None, precision_a="fp16", precision_b="fp16", seed=0,
               stones=(2, 4, 6), record_moves=False, streams=None, device="cuda", sims=None, anchor_scale=None,
               anchor_depth=None, anchor_nodes=None, anchor_plies=None, anchor_width=None):
    """A match of ``games`` games (rounded up to an even number: games / 2 openings from paired_openings) between
    the networks of two state dicts, which may differ in depth and precision.  Either side may instead be an
    AnchorPlayer or its name ("anchor:threat", "anchor:uniform", "anchor:vcf", "anchor:ab", with ``anchor_scale``, for
    the solver ``anchor_depth`` and ``anchor_nodes`` and for the alpha-beta search ``anchor_plies``, ``anchor_width``
    and ``anchor_nodes``).  Returns a MatchResult."""
    from . import engine as E, network as N
    from .config import from_any
    sides = [anchor_from_name(sd, anchor_scale, anchor_depth, anchor_nodes, anchor_plies, anchor_width) or sd
             for sd in (sd_a, sd_b)]
    c = from_any(cfg)
    if sims is not None:
        searching = [n for n, sd in zip(sims, sides) if not isinstance(sd, AnchorPlayer)]
        c = from_any(c, NUM_SIMULATIONS=max(searching) if searching else 1)
    n = max(1, (int(games) + 1) // 2)
    slots = int(num_slots) if num_slots else min(1024, 2 * n)
    if streams == 2 and slots % 2:
        slots += 1
    nets = []
    for sd, prec in zip(sides, (precision_a, precision_b)):
        if isinstance(sd, AnchorPlayer):
            nets.append(sd)
            continue
        cn = from_any(c, NUM_RES_BLOCKS=blocks_of(sd))
        nets.append(N.GomokuNetHip(sd, cn, num_slots=E.hidden_slots(c, slots), max_rows=slots, device=device,
                                   precision=prec))
    arena = Arena(c, nets[0], nets[1], slots, paired_openings(n, c.BOARD_SIZE, seed, stones, c.N_IN_ROW), seed=seed,
                  record_moves=record_moves, streams=streams, device=device, sims=sims)
    try:
        return arena.run()
    finally:
        arena.close()


def load_checkpoint(path):
    """A network state dict from a RecordStore database's trainer checkpoint (formats.RecordStore) or from a file
    written by torch.save, read with torch.load(weights_only=True)."""
    import torch
    with open(path, "rb") as f:
        head = f.read(16)
    if head.startswith(b"SQLite format 3"):
        from .formats import RecordStore
        st = RecordStore(path)
        try:
            ts = st.load_trainer_state()
        finally:
            st.close(checkpoint=False)
        if ts is None:
            raise ValueError("%s holds no trainer checkpoint" % path)
        return ts["model_state_dict"]
    sd = torch.load(path, map_location="cpu", weights_only=True)
    return sd["model_state_dict"] if isinstance(sd, dict) and "model_state_dict" in sd else sd


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m datou_gomoku_muzero_amd.arena", description="A match between two network checkpoints on the GPU: paired openings, "
                                             "wins / draws / losses and the Elo difference as one JSON line.")
    ap.add_argument("--a", required=True, help="checkpoint of network A (RecordStore .db or torch.save file), or "
                                               "anchor:threat / anchor:uniform / anchor:vcf / anchor:ab for a fixed opponent")
    ap.add_argument("--b", required=True,
                    help="checkpoint of network B, or anchor:threat / anchor:uniform / anchor:vcf / anchor:ab")
    ap.add_argument("--anchor-scale", type=float, default=None,
                    help="noise scale of an anchor side (default: 0 for threat, vcf and ab, 1 for uniform)")
    ap.add_argument("--anchor-depth", type=int, default=None,
                    help="attacker moves the solver of anchor:vcf and anchor:ab looks ahead (default 10, at most 16)")
    ap.add_argument("--anchor-nodes", type=int, default=None,
                    help="node budget per board of the anchor:vcf solver and of each of anchor:ab's two searches "
                         "(default 2048)")
    ap.add_argument("--anchor-plies", type=int, default=None,
                    help="plies the anchor:ab search looks ahead (default 4, at most 8)")
    ap.add_argument("--anchor-width", type=int, default=None,
                    help="candidate cells per node of the anchor:ab search (default 8, at most 16)")
    ap.add_argument("--games", type=int, required=True)
    ap.add_argument("--precision-a", default="fp16", choices=("fp16", "bf16"))
    ap.add_argument("--precision-b", default="fp16", choices=("fp16", "bf16"))
    ap.add_argument("--board-size", type=int, default=15)
    ap.add_argument("--sims", type=int, default=400, help="NUM_SIMULATIONS of both networks' searches")
    ap.add_argument("--sims-a", type=int, default=None, help="simulations per search of network A (default --sims)")
    ap.add_argument("--sims-b", type=int, default=None, help="simulations per search of network B (default --sims)")
    ap.add_argument("--mode", default="MuZero", choices=("MuZero", "AlphaZero"))
    ap.add_argument("--slots", type=int, default=0)
    ap.add_argument("--streams", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    from .config import GmzConfig
    cfg = GmzConfig(BOARD_SIZE=a.board_size, NUM_SIMULATIONS=a.sims, MCTS_IMPLEMENTATION=a.mode)
    sims = (a.sims_a or a.sims, a.sims_b or a.sims)
    sides = [anchor_from_name(x, a.anchor_scale, a.anchor_depth, a.anchor_nodes, a.anchor_plies, a.anchor_width)
             or load_checkpoint(x) for x in (a.a, a.b)]
    res = play_match(sides[0], sides[1], cfg, a.games, a.slots or None, a.precision_a, a.precision_b, a.seed,
                     streams=a.streams, sims=sims)
    out = res.as_dict()
    names = [s.name if isinstance(s, AnchorPlayer) else os.path.basename(x) for s, x in zip(sides, (a.a, a.b))]
    out.update(sims_a=sims[0], sims_b=sims[1], a=names[0], b=names[1], precision_a=a.precision_a,
               precision_b=a.precision_b)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
