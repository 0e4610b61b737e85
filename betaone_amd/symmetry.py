"""betaone_amd/symmetry.py -- the two exact board symmetries of chess on the host: what csrc/bo_sym.h does inside the replay samplers,
restated in NumPy / torch for validation and for people (no kernel: none of this is on a hot path).

A transform code t has bit 0 = colour flip (colours swapped, ranks mirrored, turn toggled; always valid) and bit 1 = file mirror
(a <-> h; valid when the position has no castling right).

    perm = action_permutation(t)            # perm[a] = the policy index of the transformed move; an involution on 0..4671
    back = unmap_logits(logits_of_T_x, applied)   # row b, column a = the logit the net gave T x for the twin of move a
    transform_fen(fen, t), transform_uci("e2e4", t)
"""
from __future__ import annotations

import numpy as np
import torch

NUM_ACTIONS = 4672
PLANES = 73
COLOUR, MIRROR = 1, 2
CODES = {"colour": (COLOUR,), "mirror": (MIRROR,), "both": (COLOUR, MIRROR, COLOUR | MIRROR)}   # validate --symmetry: the passes of each choice

_perm_cache = {}


def action_permutation(t: int) -> np.ndarray:
    """perm [4672] int64: perm[a] = the index of move a's twin under t, by the closed form of csrc/bo_sym.h sym_action.  With
    a = from * 73 + plane (utils.move_to_index): the from square is mirrored (^ 56, ^ 7); a queen plane's direction index d of
    N NE E SE S SW W NW goes to (4 - d) % 8 under the colour flip and (-d) % 8 under the file mirror, the distance is kept; a knight
    plane's k goes to (3 - k) % 8 and 7 - k; an underpromotion plane is relative to the pawn's colour already, and the file mirror
    swaps its capture sides (direction 2 - d)."""
    t = int(t)
    if t not in (0, 1, 2, 3):
        raise ValueError(f"transform code {t}: 0..3")
    if t not in _perm_cache:
        a = np.arange(NUM_ACTIONS, dtype=np.int64)
        frm, p = a // PLANES, a % PLANES
        for bit, sq_xor, q_of, n_of in ((COLOUR, 56, lambda d: (4 - d) % 8, lambda k: (3 - k) % 8), (MIRROR, 7, lambda d: (-d) % 8, lambda k: 7 - k)):
            if not t & bit:
                continue
            frm = frm ^ sq_xor
            queen, knight = p < 56, (p >= 56) & (p < 64)
            under = p >= 64
            pq = q_of(p // 7) * 7 + p % 7
            pn = 56 + n_of(p - 56)
            pu = 64 + ((p - 64) // 3) * 3 + (2 - (p - 64) % 3) if bit == MIRROR else p
            p = np.where(queen, pq, np.where(knight, pn, np.where(under, pu, p)))
        perm = frm * PLANES + p
        perm.setflags(write=False)
        _perm_cache[t] = perm
    return _perm_cache[t]


def unmap_logits(logits: torch.Tensor, applied) -> torch.Tensor:
    """logits [n, 4672] of a batch that was sampled under the codes applied [n] (GpuReplayBuffer.batch*(sym=...)'s last element), gathered
    back into the original indexing: out[b, a] = logits[b, perm_applied[b][a]] -- the logit the net gave the twin of move a."""
    applied = torch.as_tensor(applied, device=logits.device).reshape(-1).long()
    if logits.dim() != 2 or logits.shape[1] != NUM_ACTIONS or applied.numel() != logits.shape[0]:
        raise ValueError(f"unmap_logits: logits {tuple(logits.shape)}, {applied.numel()} codes")
    table = torch.from_numpy(np.stack([action_permutation(t) for t in range(4)])).to(logits.device)
    return torch.gather(logits, 1, table[applied])


def _mirror_row(row: str) -> str:
    return row[::-1]   # (a run of empty squares is its own mirror image)


def transform_fen(fen: str, t: int) -> str:
    """The FEN of the transformed position.  Both counters are kept.  A file mirror of a position with castling rights is refused."""
    t = int(t)
    if t not in (0, 1, 2, 3):
        raise ValueError(f"transform code {t}: 0..3")
    f = fen.split()
    if len(f) != 6:
        raise ValueError(f"transform_fen: {fen!r}: six fields")
    rows, turn, castling, ep = f[0].split("/"), f[1], f[2], f[3]
    if t & MIRROR:
        if castling != "-":
            raise ValueError(f"transform_fen: the file mirror needs a position without castling rights, not {castling!r}")
        rows = [_mirror_row(r) for r in rows]
    if t & COLOUR:
        rows = [r.swapcase() for r in rows[::-1]]
        turn = "b" if turn == "w" else "w"
        if castling != "-":
            castling = "".join(c for c in "KQkq" if c in castling.swapcase())
    if ep != "-":
        ep = transform_uci(ep, t)
    return " ".join(["/".join(rows), turn, castling, ep, f[4], f[5]])


def transform_uci(uci: str, t: int) -> str:
    """A move (or a square) in UCI notation under t: files a <-> h under the mirror, ranks 1 <-> 8 under the colour flip; a promotion
    piece is kept."""
    t = int(t)
    out = list(uci)
    for i, c in enumerate(out[:4]):
        if i % 2 == 0 and t & MIRROR:
            out[i] = "hgfedcba"["abcdefgh".index(c)]
        elif i % 2 == 1 and t & COLOUR:
            out[i] = "87654321"["12345678".index(c)]
    return "".join(out)
