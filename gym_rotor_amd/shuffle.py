"""A keyed permutation of [0, n) on the device (qr_shuffle): `shuffle` — PPO's epoch shuffle with no sort, no state and no stored table.

perm is a bijection of [0, n) and a function of (seed, draw, stream, n) alone (include/quadrotor_hip.h, QrShuffle; restated in NumPy by
tests/shuffle_ref.py): a balanced Feistel network on 2w bits, 4^w the first power of four at or above n, under eight keys taken from
the `noise_fill` stream (seed, draw, stream), walked until the result is below n.  So a slice out[i] = perm(first + i) holds the values of
those positions of the whole — a rank can form just its own rows — and the draw number may live on the device: with `draw_dev` the
launch reads it there, which is what lets a captured graph shuffle afresh at every replay.  It is another family of permutations than
`torch.randperm`'s or numpy's, and nothing is stored.  `ppo_stream` numbers the streams `PpoUpdater` draws from.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _checks as ck
from . import _lib
from .noise import check_seed

PPO_STREAM = 3 << 27                  # above every `es.es_stream` id, below `offpolicy.COLLECTOR_STREAM`
PPO_STREAM_NAMES = ("shuffle", "noise")


def ppo_stream(k: int, name: str) -> int:
    """The stream id of agent k's `name` ("shuffle": the epoch permutation, "noise": the spatial term's row) in `PpoUpdater`."""
    k = int(k)
    if name not in PPO_STREAM_NAMES or not 0 <= k < 1 << 16:
        raise ValueError(f"ppo_stream: agent 0 <= k < 65536 and a name of {PPO_STREAM_NAMES}, got {k}, {name!r}")
    return PPO_STREAM | (k << 8) | PPO_STREAM_NAMES.index(name)


def shuffle(out: torch.Tensor, *, n: int, seed: int, draw: int, stream: int, first: int = 0, draw_dev: Optional[torch.Tensor] = None,
            max_workgroups: int = 0) -> torch.Tensor:
    """out[i] = perm(first + i) for i < out.numel(), in one launch; returns out.  out: a contiguous int64 tensor (empty: nothing is
    launched); 1 <= n < 2^32; 0 <= first and first + out.numel() <= n; 0 <= seed < 2^64; stream < 2^30; draw: 0 <= draw < 2^63, the draw
    number, or with draw_dev — an int64 device tensor of one element — ignored: the launch reads the number there (and never writes
    it).  max_workgroups: 0, or a cap on the grid (it cannot change a value).  Never use a (seed, draw, stream) triple for a noise
    tensor as well.  Every check comes before the launch."""
    what = "shuffle"
    if not isinstance(out, torch.Tensor) or out.dtype != torch.int64 or not out.is_contiguous():
        raise ValueError(f"{what}: out must be a contiguous int64 tensor")
    n, first, stream, draw, max_workgroups = int(n), int(first), int(stream), int(draw), int(max_workgroups)
    if not 1 <= n < _lib.SHUFFLE_MAX_N:
        raise ValueError(f"{what}: n must lie in [1, 2^32), got {n}")
    if first < 0 or first + out.numel() > n:
        raise ValueError(f"{what}: the slice [{first}, {first + out.numel()}) must lie in [0, {n})")
    if not 0 <= stream < _lib.NOISE_MAX_STREAM:
        raise ValueError(f"{what}: stream must lie in [0, 2^30), got {stream}")
    if max_workgroups < 0:
        raise ValueError(f"{what}: max_workgroups must be >= 0")
    seed = check_seed(what, seed)
    if draw_dev is None and not 0 <= draw < 2 ** 63:
        raise ValueError(f"{what}: draw must lie in [0, 2^63), got {draw}")
    dev = out.device
    ck.scalar(what, "draw_dev", draw_dev, torch.int64, dev)
    ck.require_gpu(dev)
    _lib.launch(dev, "qr_shuffle", _lib.shuffle_args(out, n=n, first=first, seed=seed, draw=0 if draw_dev is not None else draw, draw_dev=draw_dev,
                                                     stream=stream, max_workgroups=max_workgroups))
    return out
