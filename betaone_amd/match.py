"""
betaone_amd/match.py -- head-to-head matches between two networks on the GPU, and the AlphaGo Zero promotion gate.

    python -m betaone_amd.match BEST.pth CANDIDATE.pth --games N --slots G --cohorts K --sims S \\
        [--openings FILE] [--open-plies P] [--t-final T] [--out match.json] [--promote DEST --threshold 0.55] [--pgn games.pgn] \\
        [--tablebases DIR [--tb-search] [--tb-adjudicate]]

Net A (the first checkpoint) and net B (the second) share ONE evaluate stage (fused_net.PairedNet): row g of every evaluation is
evaluated by the net of the side to move at game g's root (bo_match_select sets the per-row selector on the device, right before each
forward).  The searches are the reference's (mcts.py) with no Dirichlet noise; moves are sampled at temperature 1 while the
fullmove number is below `open_plies`, then at `t_final` (t_final > 0: the device turn; t_final = 0: the argmax of pi, on the host
turn -- slower).  Per-game RNG seeds come from selfplay_main.game_seed, so a match is reproducible bit for bit.

Scheduling (MatchScheduler): every opening is played twice, once with each colour.  The slots of a cohort form two lanes; a game is
admitted to a free slot with the colour assignment that puts its rows on the net its lane needs at the cohort ply of its first search
(lane 0 needs net (ply & 1), lane 1 the other: every active slot plays one move per cohort ply, so the side to move -- and the net --
of a slot flips with the ply's parity).  Each net's rows then form one contiguous run of the batch and at most one tile of the two-net
head kernels is mixed.  Only a game for which no pending game of the right colour is left breaks the rule (counted in `lane_breaks`);
the selector is computed from the real root either way, so the results never depend on the lanes.

Results (JSON, printed): W/D/L from B's view, score, Elo difference -400 log10(1/s - 1) with a 95 % interval (pentanomial over
opening pairs when openings are given, per-game trinomial otherwise), likelihood of superiority, and per game the opening, colours,
UCI moves, result and termination.  --tablebases DIR: both nets see the same endgame tables -- --tb-search scores covered leaves of
every search from them, --tb-adjudicate ends a game at a position they give as drawn (a draw) or as lost for the side to move (a loss
for that side; termination "adjudication", a PGN tag Termination "adjudication").  --promote DEST writes B's state_dict to DEST (through a temporary file and os.replace) only when
B's score >= --threshold: main.py's best_model.pth convention with the AlphaGo Zero gate.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import re
import stat
import tempfile
import time
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

START_FEN = "rnbqkbnr/pppppppp/8/8/8/8/PPPPPPPP/RNBQKBNR w KQkq - 0 1"


# ---- checkpoints -----------------------------------------------------------------------------------------------------------------
def net_shape(state_dict) -> Tuple[int, int, int]:
    """(plain residual blocks, SE residual blocks, filters) of a PolicyValueNet state_dict, read from its keys (network.py: the plain
    blocks come first, an SE block has residual_tower.<i>.seblock.*)."""
    blocks, se = set(), set()
    for k in state_dict:
        m = re.match(r"residual_tower\.(\d+)\.", k)
        if m:
            blocks.add(int(m.group(1)))
            if ".seblock." in k:
                se.add(int(m.group(1)))
    if "conv_input.weight" not in state_dict:
        raise ValueError("not a PolicyValueNet state_dict (no conv_input.weight)")
    filters = int(state_dict["conv_input.weight"].shape[0])
    if blocks and sorted(blocks) != list(range(len(blocks))):
        raise ValueError("residual_tower blocks are not numbered 0..n-1")
    return len(blocks) - len(se), len(se), filters


def build_net(state_dict, device="cpu"):
    """A PolicyValueNet of the checkpoint's own shape (not config's) with its weights, in eval mode."""
    from . import dropin

    dropin.install()
    import config
    import network

    shape = net_shape(state_dict)
    saved = (config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS)
    config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = shape
    try:
        net = network.PolicyValueNet()
    finally:
        config.RESIDUAL_BLOCKS, config.SE_RESIDUAL_BLOCKS, config.CONV_FILTERS = saved
    net.load_state_dict(state_dict)
    return net.to(device).eval()


def load_state_dict(path: str):
    import torch

    sd = torch.load(path, map_location="cpu")
    if isinstance(sd, dict) and "state_dict" in sd and "conv_input.weight" not in sd:
        sd = sd["state_dict"]
    return sd


def promote(state_dict, dest: str, score: float, threshold: float) -> bool:
    """Write state_dict to dest only if score >= threshold: through a temporary file in dest's directory and os.replace, so that
    dest is either the old file or the whole new one, never a partial write."""
    if not score >= threshold:
        return False
    import torch

    d = os.path.dirname(os.path.abspath(dest))
    if os.path.exists(dest):  # (mkstemp makes the file 0600: keep the destination's mode, or give a new file the umask's)
        mode = stat.S_IMODE(os.stat(dest).st_mode)
    else:
        umask = os.umask(0)
        os.umask(umask)
        mode = 0o666 & ~umask
    fd, tmp = tempfile.mkstemp(prefix=".promote-", suffix=".tmp", dir=d)
    try:
        os.chmod(tmp, mode)
        with os.fdopen(fd, "wb") as f:
            torch.save(state_dict, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, dest)
    except BaseException:
        if os.path.exists(tmp):
            os.unlink(tmp)
        raise
    return True


# ---- statistics -------------------------------------------------------------------------------------------------------------------
def elo(score: float) -> float:
    if score <= 0.0:
        return -math.inf
    if score >= 1.0:
        return math.inf
    return -400.0 * math.log10(1.0 / score - 1.0)


def _interval(mean: float, var: float, n: int) -> Tuple[float, float]:
    if n < 1:
        return -math.inf, math.inf
    se = math.sqrt(max(var, 0.0) / n)
    lo, hi = mean - 1.959963984540054 * se, mean + 1.959963984540054 * se
    return elo(lo), elo(hi)


def match_stats(results: Sequence[float], pairs: Optional[Sequence[Tuple[float, float]]] = None) -> Dict:
    """results: B's score per game (1, 0.5, 0).  pairs: B's two scores of each opening played with both colours -- the interval is then
    the pentanomial one (the pair's mean score as the sample), else the per-game trinomial one."""
    n = len(results)
    w = sum(1 for r in results if r == 1.0)
    d = sum(1 for r in results if r == 0.5)
    l = n - w - d
    s = (w + 0.5 * d) / n if n else float("nan")
    out = {"games": n, "wins": w, "draws": d, "losses": l, "score": s, "elo": elo(s) if n else float("nan")}
    if pairs:
        ps = [(a + b) / 2.0 for a, b in pairs]
        m = sum(ps) / len(ps)
        var = sum((p - m) ** 2 for p in ps) / len(ps)
        lo, hi = _interval(m, var, len(ps))
        out["interval"] = "pentanomial"
        out["pentanomial"] = [sum(1 for a, b in pairs if a + b == k / 2.0) for k in range(5)]
    else:
        var = sum((r - s) ** 2 for r in results) / n if n else 0.0
        lo, hi = _interval(s, var, n)
        out["interval"] = "trinomial"
    out["elo_95"] = [lo, hi]
    out["los"] = 0.5 * (1.0 + math.erf((w - l) / math.sqrt(2.0 * (w + l)))) if w + l else 0.5
    return out


# ---- scheduling -------------------------------------------------------------------------------------------------------------------
@dataclass
class MatchGame:
    game_id: int
    opening: int                    # index into the scheduler's openings
    fen: Optional[str]
    moves: str                      # UCI prefix ("" if none)
    net_of_white: int               # 0: A plays white, 1: B plays white
    black_first: bool               # the side to move at the game's first searched root is black
    slot: int = -1
    first_step: int = -1
    lane_break: bool = False


def parse_openings(text: str) -> List[Tuple[Optional[str], str]]:
    """One opening per line: a FEN (or 'startpos'), optionally followed by '; <uci moves>'.  Blank lines and '#' comments skipped."""
    out = []
    for line in text.splitlines():
        line = line.split("#", 1)[0].strip()
        if not line:
            continue
        fen, _, moves = line.partition(";")
        fen = fen.strip()
        out.append((None if fen in ("", "startpos") else fen, " ".join(moves.split())))
    return out


def black_first(fen: Optional[str], moves: str) -> bool:
    parts = (fen or START_FEN).split()
    black = len(parts) > 1 and parts[1] == "b"
    return black ^ (len(moves.split()) % 2 == 1)


class MatchScheduler:
    """Which game goes into which slot.  n_slots slots in `cohorts` equal cohorts; slot s is in lane (s % Gc) >= Gc / 2 of its cohort.
    Game 2i and 2i + 1 play opening i % len(openings) with opposite colours; a slot freed for a game whose first search is at cohort
    ply `step` takes the first pending game whose net at that root is the lane's: net_of_white ^ black_first == (lane + step) & 1."""

    def __init__(self, openings: Sequence[Tuple[Optional[str], str]], n_games: int, n_slots: int, cohorts: int = 1):
        if n_slots % cohorts or (n_slots // cohorts) < 2 or (n_slots // cohorts) % 2:
            raise ValueError("MatchScheduler: the slots must split into cohorts of an even number (>= 2) of slots")
        self.openings = list(openings) or [(None, "")]
        self.Gc = n_slots // cohorts
        self.pending: List[MatchGame] = []
        for gid in range(int(n_games)):
            o = (gid // 2) % len(self.openings)
            fen, moves = self.openings[o]
            # the colours of a pair are fixed at admission (the first of the two takes the one its lane needs)
            self.pending.append(MatchGame(gid, o, fen, moves, -1, black_first(fen, moves)))
        self.admitted: Dict[int, MatchGame] = {}
        self.lane_breaks = 0

    def lane(self, slot: int) -> int:
        return int((slot % self.Gc) >= self.Gc // 2)

    @staticmethod
    def lane_net(lane: int, step: int) -> int:
        return (lane + step) & 1

    def admit(self, slot: int, step: int) -> Optional[MatchGame]:
        """The game for `slot`, whose first search runs at cohort ply `step` (None: no game left)."""
        if not self.pending:
            return None
        need = self.lane_net(self.lane(slot), step)
        pick = None
        for i, g in enumerate(self.pending):
            now = need ^ int(g.black_first)
            partner = self.admitted.get(g.game_id ^ 1)
            if partner is None or partner.net_of_white != now:
                pick = i
                break
        g = self.pending.pop(pick if pick is not None else 0)
        partner = self.admitted.get(g.game_id ^ 1)
        if pick is None:  # every pending game has the other colour fixed already: take the first one anyway
            g.net_of_white = 1 - partner.net_of_white
            g.lane_break = True
            self.lane_breaks += 1
        else:
            g.net_of_white = need ^ int(g.black_first)
        g.slot, g.first_step = slot, step
        self.admitted[g.game_id] = g
        return g


# ---- the match ----------------------------------------------------------------------------------------------------------------------
def game_result(fin, net_of_white: int) -> Tuple[float, str]:
    """(B's score, termination) of a FinishedGame: terminal 1 = the side to move in the final position is mated; terminal 3 = it lost
    without being mated (the tablebases give the position as lost: "adjudication").  A draw the tablebases called is an adjudication too."""
    adjudicated = bool(getattr(fin, "adjudicated", False))
    if fin.terminal in (1, 3):
        white_won = fin.positions[-1].turn != 1
        winner = net_of_white if white_won else 1 - net_of_white
        how = "checkmate" if fin.terminal == 1 else "adjudication" if adjudicated else "resignation"
        return (1.0 if winner == 1 else 0.0), how
    return 0.5, ("adjudication" if adjudicated and fin.terminal == 2 else "draw" if fin.terminal == 2 else "move_limit")


def play_match(ro, sched: MatchScheduler, step_of=None, seed_iteration: int = 0, log=None, finished: Optional[Dict] = None) -> Dict:
    """Drive `ro` (a CohortRollout / Rollout over a PairedNet, or a stand-in with the same start_games / play_ply) until every game of
    `sched` is finished.  step_of(slot) -> the cohort ply at which a game started in `slot` during play_ply makes its first search.
    finished: a dict that receives game_id -> FinishedGame (for write_match_pgn)."""
    from . import engine as E
    from .selfplay_main import game_seed

    if step_of is None:
        Gc = sched.Gc
        parts = getattr(ro, "parts", [ro])
        step_of = lambda s: parts[s // Gc]._step + 1  # (refilled inside ply_begin: the slot sits that ply out)
    games: Dict[int, Dict] = {}
    by_slot: Dict[int, MatchGame] = {}

    def on_finished(fin):
        g = by_slot.pop(fin.slot)
        r, how = game_result(fin, g.net_of_white)
        if finished is not None:
            finished[g.game_id] = fin
        games[g.game_id] = {"game_id": g.game_id, "opening": g.opening, "fen": g.fen or START_FEN, "prefix": g.moves,
                            "white": "AB"[g.net_of_white], "black": "AB"[1 - g.net_of_white],
                            "moves": [E.move_to_uci(m) for m in fin.moves], "result_b": r, "termination": how,
                            "plies": len(fin.moves), "slot": g.slot, "lane_break": g.lane_break}
        if log is not None:
            log(f"[match] game {g.game_id}: {games[g.game_id]['white']} (white) vs {games[g.game_id]['black']}: B scores {r} ({how}, {len(fin.moves)} plies)")

    def refill(slot):
        g = sched.admit(slot, step_of(slot))
        if g is None:
            return None
        by_slot[slot] = g
        return (g.game_id, game_seed(seed_iteration, g.game_id), g.fen, g.moves, g.net_of_white)

    slots, ids, seeds, fens, moves, nows = [], [], [], [], [], []
    for s in range(sched.Gc * (len(getattr(ro, "parts", [ro])))):
        g = sched.admit(s, 0)
        if g is None:
            break
        by_slot[s] = g
        slots.append(s); ids.append(g.game_id); seeds.append(game_seed(seed_iteration, g.game_id))
        fens.append(g.fen); moves.append(g.moves); nows.append(g.net_of_white)
    t0 = time.perf_counter()
    plies0, sims0 = ro.n_plies, ro.n_sims
    ro.start_games(slots, ids, seeds, fens, moves if any(moves) else None, nows)
    while by_slot:
        ro.play_ply(on_finished=on_finished, refill=refill)
    if hasattr(ro, "drain"):
        ro.drain()
    seconds = time.perf_counter() - t0
    return {"games": [games[k] for k in sorted(games)], "seconds": seconds, "plies": ro.n_plies - plies0, "sims": ro.n_sims - sims0,
            "lane_breaks": sched.lane_breaks}


def write_match_pgn(fh, played: Dict, finished: Dict, a: str, b: str, device="cuda:0", date: Optional[str] = None) -> int:
    """Every game of a match as PGN, in game-id order: White / Black "A (path)" or "B (path)", Round "<opening + 1>.<1|2>", the
    opening's prefix moves with a {book} comment."""
    from . import pgn_write

    games = played["games"]
    names = {"A": f"A ({a})", "B": f"B ({b})"}
    tags = [{"Event": "BetaOne match", "Date": date or pgn_write.today(), "Round": f"{g['opening'] + 1}.{g['game_id'] % 2 + 1}",
             "White": names[g["white"]], "Black": names[g["black"]],
             **({"Termination": "adjudication"} if g["termination"] == "adjudication" else {})} for g in games]
    fins = [finished[g["game_id"]] for g in games]
    return pgn_write.write_pgn(fh, fins, tags=tags, device=device, book_plies=[int(getattr(f, "first_ply", 0)) for f in fins])


def summarize(played: Dict, with_pairs: bool) -> Dict:
    games = played["games"]
    res = [g["result_b"] for g in games]
    pairs = None
    if with_pairs:
        byid = {g["game_id"]: g["result_b"] for g in games}
        pairs = [(byid[i], byid[i + 1]) for i in range(0, len(games) - 1, 2) if i in byid and i + 1 in byid]
    st = match_stats(res, pairs or None)
    sec = played["seconds"]
    st.update(plies=played["plies"], seconds=sec, plies_per_second=played["plies"] / sec if sec > 0 else 0.0,
              nodes_per_second=played["sims"] / sec if sec > 0 else 0.0, lane_breaks=played["lane_breaks"])
    return st


def json_safe(x):
    """x with every non-finite float replaced by None (an Elo of a 0 % / 100 % score, an interval bound outside (0, 1)): the file
    stays standard JSON."""
    if isinstance(x, float):
        return x if math.isfinite(x) else None
    if isinstance(x, dict):
        return {k: json_safe(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [json_safe(v) for v in x]
    return x


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m betaone_amd.match", description="Play checkpoint A against checkpoint B on the GPU.")
    ap.add_argument("a", help="checkpoint A (the current best)")
    ap.add_argument("b", help="checkpoint B (the candidate)")
    ap.add_argument("--games", type=int, default=100)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--cohorts", type=int, default=1)
    ap.add_argument("--sims", type=int, default=800)
    ap.add_argument("--mcts-batch", type=int, default=96)
    ap.add_argument("--openings", default=None, help="file: one FEN (or 'startpos') per line, optionally '; <uci moves>'")
    ap.add_argument("--open-plies", type=int, default=8, help="moves with a fullmove number below this are sampled at temperature 1")
    ap.add_argument("--t-final", type=float, default=0.1, help="temperature after that (0: argmax, on the slower host turn)")
    ap.add_argument("--max-game-moves", type=int, default=512)
    ap.add_argument("--seed-iteration", type=int, default=0, help="the iteration argument of selfplay_main.game_seed")
    ap.add_argument("--out", default=None)
    ap.add_argument("--promote", default=None, metavar="DEST")
    ap.add_argument("--threshold", type=float, default=0.55)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--pgn", default=None, metavar="FILE", help="also write every game as PGN (SAN rendered on the GPU)")
    from .selfplay_main import tb_arguments, tb_check_arguments, tb_rollout_kw

    tb_arguments(ap)
    args = ap.parse_args(argv)
    tb_check_arguments(ap, args)

    import torch

    from .fused_net import PairedNet
    from .rollout import CohortRollout

    sd_a, sd_b = load_state_dict(args.a), load_state_dict(args.b)
    dev = torch.device(args.device)
    net_a, net_b = build_net(sd_a, dev), build_net(sd_b, dev)
    openings = parse_openings(open(args.openings).read()) if args.openings else [(None, "")]
    pair = PairedNet(net_a, net_b, batch=args.slots // args.cohorts, device=dev)
    print(f"[match] A {net_shape(sd_a)} vs B {net_shape(sd_b)}: evaluate stage {pair.route}")
    ro = CohortRollout(pair, args.slots, cohorts=args.cohorts, num_simulations=args.sims, mcts_batch_size=args.mcts_batch,
                       dirichlet_alpha=0.0, temperature=(args.open_plies, 1.0, args.t_final), max_game_moves=args.max_game_moves,
                       rng_mode="native", device=str(dev), **tb_rollout_kw(args, str(dev)))
    sched = MatchScheduler(openings, args.games, args.slots, args.cohorts)
    finished: Optional[Dict] = {} if args.pgn else None
    try:
        played = play_match(ro, sched, seed_iteration=args.seed_iteration, log=print, finished=finished)
        pair.check_overflow()
    finally:
        ro.close()
    if args.pgn:
        with open(args.pgn, "w", encoding="utf-8", newline="\n") as fh:
            write_match_pgn(fh, played, finished, args.a, args.b, device=str(dev))
    st = summarize(played, with_pairs=args.openings is not None)
    st["route"] = pair.route
    st["promoted"] = promote(sd_b, args.promote, st["score"], args.threshold) if args.promote else False
    out = {"a": args.a, "b": args.b, "settings": {k: getattr(args, k) for k in ("games", "slots", "cohorts", "sims", "mcts_batch", "openings",
                                                                             "open_plies", "t_final", "max_game_moves", "seed_iteration",
                                                                             "threshold", "tablebases", "tb_search", "tb_adjudicate")},
           "summary": st, "games": played["games"]}
    print(f"[match] B vs A: +{st['wins']} ={st['draws']} -{st['losses']}  score {st['score']:.3f}  Elo {st['elo']:+.1f} "
          f"[{st['elo_95'][0]:+.1f}, {st['elo_95'][1]:+.1f}] ({st['interval']})  LOS {st['los']:.3f}  "
          f"{st['plies_per_second']:.0f} plies/s  {st['nodes_per_second']:.0f} nodes/s" + ("  -> promoted" if st["promoted"] else ""))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(json_safe(out), f, indent=1, allow_nan=False)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
