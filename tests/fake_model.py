"""
tests/fake_model.py -- deterministic, platform-independent stand-ins used by the golden generator
and by the parity tests (test infrastructure).

* FakeNet: logits/value are a pure INTEGER-hash function of the input planes, so that they are
  bit-identical on any host, for any batch size and any row order (BLAS-free).
* hash_init_: fills a PolicyValueNet's parameters and BN buffers from an integer hash of
  (state_dict key, flat index), so that "random-init" weights need no torch RNG and no files.
"""
from __future__ import annotations

import hashlib
import zlib

import numpy as np

NUM_ACTIONS = 4672
PLANES = 120 * 64

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _splitmix64(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        x = (x + np.uint64(0x9E3779B97F4A7C15)) & _M64
        z = x
        z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & _M64
        z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & _M64
        return z ^ (z >> np.uint64(31))


_W = None


def planes_hash(planes: np.ndarray) -> np.ndarray:
    """uint64 hash per row of planes[B, 120, 8, 8] (entries are small non-negative integers)."""
    global _W
    if _W is None:
        _W = _splitmix64(np.arange(PLANES, dtype=np.uint64))
    x = np.ascontiguousarray(planes, dtype=np.float32).reshape(-1, PLANES)
    xi = x.astype(np.int64).astype(np.uint64)
    with np.errstate(over="ignore"):
        return (xi * _W[None, :]).sum(axis=1, dtype=np.uint64)


# Evaluation families of the degenerate-row tests (tests/degenerate_eval_cases.py): what a trained net hands the tree step and the
# plain hash net never does.  `family=None` leaves the bits of every earlier caller unchanged.
#   peak          logits spread over 400: a float32 softmax gives exact zeros and denormals at legal moves
#   illegal_mass  scale 6 with +300 on eight actions that leave the board (from a1 southwards, from h8 northwards: legal in no
#                 position at all), so every legal prior is exactly 0
#   v_pm1         value = sign(v): evaluations of exactly +-1
#   v_zero        value = +0.0 where v > 0, otherwise -0.0
# A policy family combines with a value family through `value=` (tests/fast_degenerate_cases.py): "v_pm1", "v_zero", or
#   v_m1          value = -1 at every row: whoever moved into a leaf sees +1, so a step's descents all follow one line
# and `peak_scale` sharpens the peak family further (one legal move holds all the mass: a search that runs down a single line).
FAMILIES = ("peak", "illegal_mass", "v_pm1", "v_zero")
POLICY_FAMILIES, VALUE_FAMILIES = ("peak", "illegal_mass"), ("v_pm1", "v_zero", "v_m1")
ILLEGAL_MASS_ACTIONS = (28, 29, 30, 31, 63 * 73, 63 * 73 + 1, 63 * 73 + 2, 63 * 73 + 3)


def fake_logits_values(planes: np.ndarray, scale: float = 6.0, salt: int = 0, family=None, value=None, peak_scale: float = 400.0):
    """planes[B,120,8,8] -> (logits f32[B,4672], values f32[B])."""
    if family is not None:
        assert family in FAMILIES, family
        scale = peak_scale if family == "peak" else 6.0
    if value is not None:
        assert family in (None,) + POLICY_FAMILIES and value in VALUE_FAMILIES, (family, value)
    h = planes_hash(planes) ^ np.uint64(salt)
    a = np.arange(NUM_ACTIONS, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = _splitmix64(h[:, None] + a[None, :] * np.uint64(0xD1B54A32D192ED03))
    u = (z >> np.uint64(40)).astype(np.float64) / float(1 << 24)
    logits = ((u - 0.5) * scale).astype(np.float32)
    zv = _splitmix64(h ^ np.uint64(0xABCDEF0123456789))
    v = ((zv >> np.uint64(40)).astype(np.float64) / float(1 << 24) * 2.0 - 1.0) * 0.9
    v = v.astype(np.float32)
    if family == "illegal_mass":
        logits[:, list(ILLEGAL_MASS_ACTIONS)] += np.float32(300.0)
    value = family if value is None else value
    if value == "v_pm1":
        v = np.sign(v).astype(np.float32)
    elif value == "v_zero":
        v = np.where(v > 0, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    elif value == "v_m1":
        v = np.full_like(v, -1.0)
    return logits, v


def family_eval(family, salt: int, value=None, peak_scale: float = 400.0):
    """planes -> (torch.softmax of the family's logits in float32, values): the evaluator the degenerate-row tests hand to the
    engine and to the oracle alike."""
    import torch

    def fn(planes):
        logits, v = fake_logits_values(planes, salt=salt, family=family, value=value, peak_scale=peak_scale)
        return torch.softmax(torch.from_numpy(logits), dim=1).numpy(), v

    return fn


def planes_key(planes_row: np.ndarray) -> str:
    """stable text key of one encoded position (sha1 of the float32 bytes)."""
    return hashlib.sha1(np.ascontiguousarray(planes_row, dtype=np.float32).tobytes()).hexdigest()


class FakeNet:
    """torch-module-like callable: model(x) -> (logits[B,4672], value[B,1]) as torch tensors."""

    def __init__(self, scale: float = 6.0, salt: int = 0, family=None):
        self.scale, self.salt, self.family = scale, salt, family
        # the model's part of a seam key: a family's name where a plain net has its scale, so the two cannot collide
        self.model_id = f"{scale}:{salt}" if family is None else f"{family}:{salt}"
        self.calls = []

    def __call__(self, x):
        import torch

        planes = x.detach().cpu().numpy()
        logits, v = fake_logits_values(planes, self.scale, self.salt, self.family)
        self.calls.append(planes.shape[0])
        return torch.from_numpy(logits), torch.from_numpy(v).unsqueeze(1)

    def eval(self):
        return self

    def to(self, *_a, **_k):
        return self


def hash_init_(model, gain: float = 0.5):
    """Deterministically fill every parameter/buffer of a torch module from an integer hash."""
    import torch

    sd = model.state_dict()
    new = {}
    for name, t in sd.items():
        n = t.numel()
        if name.endswith("num_batches_tracked"):
            new[name] = torch.zeros_like(t)
            continue
        seed = np.uint64(zlib.crc32(name.encode()))
        with np.errstate(over="ignore"):
            z = _splitmix64(seed * np.uint64(0x100000001B3) + np.arange(n, dtype=np.uint64))
        u = (z >> np.uint64(40)).astype(np.float64) / float(1 << 24) * 2.0 - 1.0  # [-1, 1)
        if name.endswith("running_var"):
            vals = 1.0 + 0.5 * np.abs(u)
        elif name.endswith("running_mean"):
            vals = 0.1 * u
        elif "bn" in name.split(".")[-2] and name.endswith("weight"):
            vals = 1.0 + 0.1 * u
        elif name.endswith("bias"):
            vals = 0.1 * u
        else:
            fan_in = int(np.prod(t.shape[1:])) if t.dim() > 1 else int(t.shape[0])
            vals = u * gain * np.sqrt(3.0 / max(1, fan_in))
        new[name] = torch.from_numpy(vals.astype(np.float32)).reshape(t.shape).to(t.dtype)
    model.load_state_dict(new)
    return model
