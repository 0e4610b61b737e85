"""betaone_amd/resign.py -- calibration report of resignation from the root values kept in BOG2 records.

    python -m betaone_amd.resign DATA_DIR/iter_N/ --threshold -0.9 [--plies 1] [--json]

Reads every games_rank*.bog of the directory (every rank's file) and reports, from the recorded per-ply root values v_i, on the host:
games resigned; plies played and the mean length of resigned and of full games; the check games (resignation disabled for them) and
the false positives among them; a table over thresholds of the false-positive rate and the plies that would have been saved; and the
highest threshold of the table whose false-positive rate is below 5 %.

The rule (DESIGN "Resignation") fires at ply i when v_j < t for j = i, i - 2, ..., i - 2 (K - 1), all >= 0: the side to move at ply i
and its previous K - 1 searches.  A false positive is a check game in which the rule fires (first at ply i) for a side that does not end
up mated: the game is not lost by the side to move at ply i's parity (terminal 1 with that side to move in the final position).
Plies saved at a threshold: over the games that ran to their end, n_plies - i where the rule first fires at ply i.
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import sys
from typing import Dict, List, Optional, Sequence

import numpy as np

THRESHOLDS = (-0.99, -0.98, -0.97, -0.96, -0.95, -0.9, -0.85, -0.8, -0.75, -0.7, -0.6, -0.5)
MAX_FALSE_POSITIVE_RATE = 0.05


def first_firing(values, threshold: float, plies: int = 1) -> Optional[int]:
    """First ply i at which the rule fires on the recorded values, else None."""
    below = np.asarray(values, dtype=np.float32) < np.float32(threshold)
    run = np.zeros(2, dtype=np.int64)  # consecutive own searches below t, per ply parity
    for i, b in enumerate(below):
        run[i & 1] = run[i & 1] + 1 if b else 0
        if run[i & 1] >= plies:
            return i
    return None


def _lost_by(game) -> Optional[int]:
    """Parity of the side that ended mated (terminal 1, or 3: resigned = treated as mated at the last position), else None."""
    return int(game["n_plies"]) & 1 if int(game["terminal"]) in (1, 3) else None


def report(games: Sequence[dict], threshold: float, plies: int = 1, thresholds: Sequence[float] = THRESHOLDS) -> Dict:
    """games: unpacked compact records (records.unpack_games); those without root values (BOG1) are counted but not analysed."""
    games = list(games)
    n_pl = [int(g["n_plies"]) for g in games]
    resigned = [g for g in games if int(g["terminal"]) == 3]
    full = [g for g in games if int(g["terminal"]) != 3]
    valued = [g for g in full if g.get("root_values") is not None]
    checks = [g for g in valued if g.get("resign_check")]

    def fp_of(g, t):
        i = first_firing(g["root_values"], t, plies)
        if i is None:
            return None, False
        return i, _lost_by(g) != (i & 1)

    fired = fps = 0
    for g in checks:
        i, fp = fp_of(g, threshold)
        fired += i is not None
        fps += fp
    ts = sorted(set(float(t) for t in thresholds) | {float(threshold)})
    table = []
    for t in ts:
        n_fp = sum(fp_of(g, t)[1] for g in checks)
        saved = 0
        for g in valued:
            i = first_firing(g["root_values"], t, plies)
            if i is not None:
                saved += int(g["n_plies"]) - i
        table.append(dict(threshold=t, false_positives=int(n_fp), false_positive_rate=(n_fp / len(checks)) if checks else None,
                          plies_saved=int(saved)))
    ok = [r["threshold"] for r in table if r["false_positive_rate"] is not None and r["false_positive_rate"] < MAX_FALSE_POSITIVE_RATE]
    return dict(games=len(games), resigned=len(resigned), plies=int(sum(n_pl)),
                mean_plies_resigned=float(np.mean([int(g["n_plies"]) for g in resigned])) if resigned else None,
                mean_plies_full=float(np.mean([int(g["n_plies"]) for g in full])) if full else None,
                games_with_values=len(valued) + sum(1 for g in resigned if g.get("root_values") is not None),
                threshold=float(threshold), plies_rule=int(plies), check_games=len(checks), check_fired=int(fired),
                false_positives=int(fps), false_positive_rate=(fps / len(checks)) if checks else None, table=table,
                recommended_threshold=max(ok) if ok else None)


def print_report(rep: Dict, fh=sys.stdout) -> None:
    w = fh.write
    w(f"games {rep['games']}, resigned {rep['resigned']}, plies {rep['plies']}\n")
    w(f"mean plies: resigned games {rep['mean_plies_resigned']}, full games {rep['mean_plies_full']}\n")
    w(f"check games {rep['check_games']}: rule fired in {rep['check_fired']} at t = {rep['threshold']:+.3f}, K = {rep['plies_rule']}; "
      f"false positives {rep['false_positives']} (rate {rep['false_positive_rate']})\n")
    w("threshold  false positives  rate     plies saved\n")
    for r in rep["table"]:
        rate = "-" if r["false_positive_rate"] is None else f"{r['false_positive_rate']:.4f}"
        w(f"{r['threshold']:+9.3f}  {r['false_positives']:15d}  {rate:>7}  {r['plies_saved']:11d}\n")
    w(f"highest threshold with a false-positive rate below {MAX_FALSE_POSITIVE_RATE:.0%}: {rep['recommended_threshold']}\n")


def load_dir(path: str) -> List[dict]:
    from . import records

    files = sorted(glob.glob(os.path.join(path, "*" + records.COMPACT_SUFFIX))) if os.path.isdir(path) else [path]
    games = []
    for f in files:
        games.extend(records.load_games(f))
    return games


def main(argv=None, out=None) -> Dict:
    ap = argparse.ArgumentParser(prog="python -m betaone_amd.resign", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("path", help="DATA_DIR/iter_N/ (every games_rank*.bog in it) or one .bog file")
    ap.add_argument("--threshold", type=float, required=True, help="the run's --resign-threshold (the false positives are counted at it)")
    ap.add_argument("--plies", type=int, default=1, help="the run's --resign-plies")
    ap.add_argument("--json", action="store_true", help="one JSON line instead of the text report")
    args = ap.parse_args(argv)
    out = out or sys.stdout
    rep = report(load_dir(args.path), args.threshold, args.plies)
    if args.json:
        out.write(json.dumps(rep) + "\n")
    else:
        print_report(rep, out)
    return rep


if __name__ == "__main__":
    main()
