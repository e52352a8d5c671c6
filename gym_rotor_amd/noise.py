"""The library's own noise source: `noise_fill` fills any number of float32 tensors — standard normal or uniform in (-1, 1), each
scaled and shifted — from one counter-based stream, sixteen tensors per launch (qr_noise_fill), and `DeviceNoise` keeps a seed and
a draw counter for it.

The stream (include/quadrotor_hip.h, QrNoiseFill; restated in NumPy by tests/noise_ref.py): element e of a tensor is position e % 4 of
quad q = e // 4, whose four words are Philox4x32-10 under the 64-bit seed with the counter (q_lo, q_hi ^ draw_hi, draw_lo,
0xC0000000 | stream).  So a value is a function of (seed, draw, stream, e, kind, a, b) alone — not of the torch version, the
generator's state, the other tensors of the call or how the call is split into launches — and the draw number may live on the
device: with `draw_dev` the launch reads it there, which is what lets a captured graph draw fresh noise at every replay without
`register_generator_state`.  `Td3Updater` / `SacUpdater` (noise_source="device") key it by the replay buffer's minibatch counter.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch

from . import _checks as ck
from . import _lib

KINDS = tuple(_lib.NOISE_KIND_ID)


def _per_tensor(v, n: int, name: str, conv):
    vs = list(v) if isinstance(v, (list, tuple)) else [v] * n
    if len(vs) != n:
        raise ValueError(f"noise_fill: {name} is one value or one per tensor ({n}), got {len(vs)}")
    return [conv(x) for x in vs]


def _kind(x) -> int:
    if x not in _lib.NOISE_KIND_ID:
        raise ValueError(f"noise_fill: kind must be one of {KINDS}, got {x!r}")
    return _lib.NOISE_KIND_ID[x]


def _finite(x) -> float:
    x = float(x)
    if not math.isfinite(x) or abs(x) > 3.4028234663852886e38:
        raise ValueError(f"noise_fill: a and b must be finite float32 numbers, got {x}")
    return x


def check_seed(what: str, seed) -> int:
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError(f"{what}: seed must lie in [0, 2^64), got {seed}")
    return seed


def noise_fill(tensors: Sequence[torch.Tensor], *, seed: int, draw: int, streams: Sequence[int], kind="normal", a=0.0, b=1.0,
               draw_dev: Optional[torch.Tensor] = None) -> None:
    """Fill every tensor of `tensors` in place: kind "normal": a + b * z with z standard normal (a the mean, b the standard deviation);
    "uniform": a + b * s with s uniform in (-1, 1), each as one fused multiply-add.  tensors: contiguous float32 tensors on one device,
    none empty; streams: one id below 2^30 per tensor, pairwise distinct — tensor i's values are a function of (seed, draw, streams[i])
    and of nothing else in the call; kind, a, b: one value, or one per tensor.  seed: 0 <= seed < 2^64; draw: 0 <= draw < 2^63, the
    draw number, or with draw_dev — an int64 device tensor of one element — ignored: the launch reads the number there (and never writes
    it).  Never use a (seed, draw, stream) triple for two tensors.  Sixteen tensors go into one launch; more are split into launches
    of sixteen, which cannot change a value.  Every check comes before the first launch."""
    what = "noise_fill"
    tensors = [tensors] if isinstance(tensors, torch.Tensor) else list(tensors)
    n = len(tensors)
    if n < 1:
        raise ValueError(f"{what}: no tensors")
    streams = [int(s) for s in streams]
    if len(streams) != n or len(set(streams)) != n or min(streams) < 0 or max(streams) >= _lib.NOISE_MAX_STREAM:
        raise ValueError(f"{what}: streams must be {n} pairwise distinct ids in [0, 2^30), got {streams}")
    kinds, a, b = _per_tensor(kind, n, "kind", _kind), _per_tensor(a, n, "a", _finite), _per_tensor(b, n, "b", _finite)
    seed, draw = check_seed(what, seed), int(draw)
    if draw_dev is None and not 0 <= draw < 2 ** 63:
        raise ValueError(f"{what}: draw must lie in [0, 2^63), got {draw}")
    dev = tensors[0].device if isinstance(tensors[0], torch.Tensor) else None
    for i, t in enumerate(tensors):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != dev or not t.is_contiguous() or t.numel() < 1:
            raise ValueError(f"{what}: tensors[{i}] must be a non-empty contiguous float32 tensor on {dev}")
    ck.scalar(what, "draw_dev", draw_dev, torch.int64, dev)
    m = _lib.NOISE_MAX_SLOTS
    if any(sum((t.numel() + 3) // 4 for t in tensors[i:i + m]) >= 2 ** 31 for i in range(0, n, m)):
        raise ValueError(f"{what}: a launch's sixteen tensors hold at most 2^31 - 1 quads of four elements")
    ck.require_gpu(dev)
    for i in range(0, n, m):
        _lib.launch(dev, "qr_noise_fill", _lib.noise_fill_args(tensors[i:i + m], kinds[i:i + m], a[i:i + m], b[i:i + m], streams[i:i + m], seed=seed,
                                                               draw=0 if draw_dev is not None else draw, draw_dev=draw_dev))


class DeviceNoise:
    """A seed and a draw counter for `noise_fill`.  `fill(tensors, ...)` draws with the current number and advances the host counter
    `draw` by one, so successive calls never repeat a (seed, draw, stream) triple.  `bind(counter)` makes the launches read the
    number from an int64 device tensor of one element instead — a counter that something else advances on the device, such as
    `ReplayBuffer.state[2:3]`; this object reads it and never writes it (the host counter keeps counting the calls all the same)."""

    def __init__(self, seed: int = 0, device="cuda"):
        self.seed = check_seed("DeviceNoise", seed)
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None and torch.cuda.is_available():
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.draw = 0
        self.draw_dev: Optional[torch.Tensor] = None

    def bind(self, counter: Optional[torch.Tensor]) -> "DeviceNoise":
        self.draw_dev = ck.scalar("DeviceNoise.bind", "the counter", counter, torch.int64, self.device)
        return self

    def fill(self, tensors, *, streams: Optional[Sequence[int]] = None, kind="normal", a=0.0, b=1.0) -> None:
        """`noise_fill` with this object's seed and draw number; streams: by default 0, 1, ... in the tensors' order."""
        tensors = [tensors] if isinstance(tensors, torch.Tensor) else list(tensors)
        for i, t in enumerate(tensors):
            if not isinstance(t, torch.Tensor) or t.device != self.device:
                raise ValueError(f"DeviceNoise.fill: tensors[{i}] must be a tensor on {self.device}")
        noise_fill(tensors, seed=self.seed, draw=self.draw, streams=range(len(tensors)) if streams is None else streams, kind=kind, a=a, b=b,
                   draw_dev=self.draw_dev)
        self.draw += 1
