"""The argument checks of the host-side ops (td3, sac, policy, optim, offpolicy, es, episodes, rollout, noise, shuffle): a new op's
checks come from here.  Each takes `what` — the public function's name — and `name` — the argument's — and raises
ValueError(f"{what}: {name} must be ...") naming the dtype, shape and device it asks for; the message is formed on failure only.
`require_gpu` is the one place the GPU-only RuntimeError is raised: call it after every ValueError a function can raise.
"""
from __future__ import annotations

import math

import torch

F32, I64 = torch.float32, torch.int64


def require_gpu(dev) -> None:
    if dev.type != "cuda":
        raise RuntimeError("gym_rotor_amd ops run on the GPU only (no CPU kernel exists)")


def _refusal(what: str, name: str, dtype, want, dev) -> ValueError:
    """The one wording: want a shape (str entries: open extents), or a number of entries."""
    kind = " / ".join(str(d)[6:] for d in (dtype if type(dtype) is tuple else (dtype,)))
    if type(want) is int:
        return ValueError(f"{what}: {name} must be a contiguous {kind} tensor of {want} entries on {dev}")
    return ValueError(f"{what}: {name} must be a contiguous {kind} [{', '.join(map(str, want))}] tensor on {dev}")


def tensor(what: str, name: str, x, dtype, shape: tuple, dev, optional: bool = False):
    """x is a contiguous tensor of `dtype` (one, or a tuple of allowed ones) and `shape` on `dev`; a str entry of shape is an open
    extent (and its label in the message).  optional: None passes.  Returns x."""
    if x is None and optional:
        return None
    if (isinstance(x, torch.Tensor) and (x.dtype == dtype or (type(dtype) is tuple and x.dtype in dtype)) and x.device == dev
            and x.is_contiguous()
            and (x.shape == shape or (x.dim() == len(shape) and all(type(s) is str or n == s for n, s in zip(x.shape, shape))))):
        return x
    raise _refusal(what, name, dtype, shape, dev)


def flat(what: str, name: str, x, dtype, numel: int, dev, optional: bool = False):
    """x is a contiguous tensor of `dtype` with `numel` entries, of any shape, on `dev`.  optional: None passes.  Returns x."""
    if x is None and optional:
        return None
    if isinstance(x, torch.Tensor) and x.dtype == dtype and x.device == dev and x.numel() == numel and x.is_contiguous():
        return x
    raise _refusal(what, name, dtype, int(numel), dev)


def named(what: str, name: str, tensors, shapes: dict, dev, by_numel: bool = False, optional: bool = False) -> None:
    """`tensor` — by_numel: `flat` — over several float32 tensors in one loop (an op's gradients, an actor's weights, SAC's draws):
    tensors[n] for every n of shapes = {n: shape}; name.format(n) names it in the message, formed on failure only."""
    for n, s in shapes.items():
        x = tensors.get(n)
        if x is None and optional:
            continue
        if not (isinstance(x, torch.Tensor) and x.dtype == F32 and x.device == dev and x.is_contiguous()
                and (x.numel() == math.prod(s) if by_numel else x.shape == s)):
            raise _refusal(what, name.format(n), F32, math.prod(s) if by_numel else s, dev)


def actor(what: str, actor, sizes, D: int, A: int, dev, squash: int, log_std_head: bool, form: str) -> dict:
    """An actor (`ActorParams`) beside a twin critic that reads D + A: one of `sizes` (the rollout's), of the form the launch takes
    (`form`: the message otherwise), its tensors of their shapes on `dev`.  Returns {name: shape} of the tensors the launch reads."""
    if actor.dims not in sizes:
        raise ValueError(f"{what}: actor sizes {actor.dims} are not among {sizes} (obs, hidden, action)")
    if actor.squash != squash or ((actor.log_std_w is None or actor.log_std_b is None) if log_std_head else actor.log_std_w is not None):
        raise ValueError(f"{what}: {form}")
    if (actor.dims[0], actor.dims[2]) != (D, A):
        raise ValueError(f"{what}: the actor maps {actor.dims[0]} -> {actor.dims[2]}, the critic reads {D} + {A}")
    Da, Ha, Aa = actor.dims
    shapes = {"fc1_w": (Ha, Da), "fc1_b": (Ha,), "fc2_w": (Ha, Ha), "fc2_b": (Ha,), "mean_w": (Aa, Ha), "mean_b": (Aa,)}
    if log_std_head:
        shapes.update(log_std_w=(Aa, Ha), log_std_b=(Aa,))
    named(what, "actor tensor {}", vars(actor), shapes, dev)   # (log_std is not read: whatever it holds is not checked)
    return shapes


def scalar(what: str, name: str, x, dtype, dev, optional: bool = True):
    """A device scalar: a tensor of `dtype` with one entry on `dev` (alpha_grad, entropy_coef_dev, status, draw_dev, an optimiser's
    step).  optional: None passes.  Returns x."""
    if (x is not None or not optional) and (not isinstance(x, torch.Tensor) or x.dtype != dtype or x.device != dev or x.numel() != 1):
        kind = str(dtype)[6:]
        raise ValueError(f"{what}: {name} must be {'an' if kind[0] in 'aeiou' else 'a'} {kind} tensor of one entry on {dev}")
    return x


def workspace(what: str, x, numel: int, dev):
    """None, or a contiguous float64 tensor of one dimension and at least `numel` elements on `dev`."""
    if x is not None and (not isinstance(x, torch.Tensor) or x.dtype != torch.float64 or x.device != dev or x.dim() != 1
                          or not x.is_contiguous() or x.numel() < numel):
        raise ValueError(f"{what}: workspace must be a contiguous float64 tensor of at least {numel} elements on {dev}")
    return x


def rows(what: str, name: str, t, width: int, dev) -> int:
    """Row count of a contiguous float32 [rows, width] tensor."""
    if isinstance(t, torch.Tensor) and t.dtype == F32 and t.device == dev and t.dim() == 2 and t.shape[1] == width and t.is_contiguous():
        return t.shape[0]
    raise ValueError(f"{what}: {name} must be a contiguous float32 [rows, {width}] tensor on {dev}")


def index(what: str, x, dev, all_rows: int) -> int:
    """The minibatch size: all_rows for index None, else the length of the contiguous int64 [B] tensor."""
    if x is None:
        return all_rows
    if isinstance(x, torch.Tensor) and x.dtype == I64 and x.device == dev and x.dim() == 1 and x.is_contiguous():
        return x.numel()
    raise ValueError(f"{what}: index must be a contiguous int64 [B] tensor on {dev}")


def state(what: str, x, dev):
    """None, or a replay buffer's int64 [3] device counters (count, current_size, draw)."""
    return tensor(what, "state", x, I64, (3,), dev, True)


def column(what: str, name: str, t, n: int, dev) -> int:
    """Element stride of a float32 tensor of n elements with one stride ([n], [n, 1] or a column of a wider tensor)."""
    if not isinstance(t, torch.Tensor) or t.dtype != F32 or t.device != dev or t.numel() != n:
        raise ValueError(f"{what}: {name} must be float32 with {n} elements on {dev}")
    dims = [(m, s) for m, s in zip(t.shape, t.stride()) if m > 1]
    if len(dims) > 1 or (dims and dims[0][1] < 1):
        raise ValueError(f"{what}: {name} must have one positive element stride, got shape {tuple(t.shape)} strides {t.stride()}")
    return dims[0][1] if dims else 1


def element_stride(what: str, name: str, t: torch.Tensor) -> int:
    """The one stride between consecutive elements of `t` in row-major order (a column of a contiguous [.., n_agents] tensor)."""
    dims = [(n, s) for n, s in zip(t.shape, t.stride()) if n > 1]
    for (_, s), (n1, s1) in zip(dims, dims[1:]):
        if s != s1 * n1:
            raise ValueError(f"{what}: {name} must have one element stride (a column of a contiguous tensor), got shape {tuple(t.shape)} "
                             f"strides {t.stride()}")
    stride = dims[-1][1] if dims else 1
    if stride < 1:
        raise ValueError(f"{what}: {name} must have a positive element stride")
    return stride


def strided_rows(what: str, name: str, a, n_rows: int, width: int, dev, wider: bool = False) -> int:
    """Row stride of float32 [n_rows, width] rows that lie one row stride apart with unit column stride (a per-agent view of wider
    rows passes as it is); wider: any width >= `width`."""
    if (not isinstance(a, torch.Tensor) or a.dtype != F32 or a.device != dev or a.dim() != 2 or a.shape[0] != n_rows
            or (a.shape[1] < width if wider else a.shape[1] != width) or (a.shape[1] > 1 and a.stride(1) != 1) or a.stride(0) < a.shape[1]):
        raise ValueError(f"{what}: {name} must be float32 [{n_rows}, {'>= ' if wider else ''}{width}] rows with unit column stride on {dev}")
    return a.stride(0) if n_rows > 1 else max(a.shape[1], 1)


def rows_view(what: str, name: str, t, T: int, N: int, A: int, col_offset: int, dev) -> int:
    """Row stride of a float32 [T, N, >= col_offset + A] tensor whose rows lie one row stride apart (a storage's own [T, N, 5] rows, or
    a per-agent view of them)."""
    if t.dtype != F32 or t.device != dev or t.dim() != 3 or tuple(t.shape[:2]) != (T, N) or t.shape[2] < col_offset + A:
        raise ValueError(f"{what}: {name} must be float32 [{T}, {N}, >= {col_offset + A}] on {dev}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    rs = t.stride(1)
    if (t.shape[2] > 1 and t.stride(2) != 1) or rs < t.shape[2] or (T > 1 and t.stride(0) != N * rs):
        raise ValueError(f"{what}: {name} must be rows of a contiguous [T, N, W] tensor, got strides {t.stride()}")
    return rs


def pair_of(what: str, name: str, x, B: int, widths, dev) -> tuple:
    """(None, None) for None, or a pair of None / contiguous float32 [B, widths[m]] tensors."""
    if x is None:
        return (None, None)
    x = tuple(x)
    if len(x) != 2:
        raise ValueError(f"{what}: {name} must be a pair, one entry per agent")
    for m, e in enumerate(x):
        tensor(what, f"{name}[{m}]", e, F32, (B, widths[m]), dev, True)
    return x


def nonneg(what: str, names: tuple, *values) -> None:
    """Each value is finite and >= 0; names: theirs, in order."""
    for k, v in enumerate(values):
        if not 0.0 <= float(v) < math.inf:
            raise ValueError(f"{what}: {names[k]} must be finite and >= 0, got {v}")


LAMS = ("lam_T", "lam_S", "lam_M", "max_action")   # the names of the smoothness weights every actor-gradient op checks


def alpha(what: str, a, dev) -> tuple:
    """SAC's temperature as the launches take it, (alpha, alpha_dev): a finite Python float >= 0 and None, or 0.0 and the float32
    device tensor of one element that wins over it."""
    if isinstance(a, torch.Tensor):
        if a.dtype != F32 or a.device != dev or a.numel() != 1:
            raise ValueError(f"{what}: alpha must be a Python float or a float32 tensor of one element on {dev}")
        return 0.0, a
    nonneg(what, ("alpha",), a)
    return a, None


def reset_flags(what: str, done, truncated, T: int, N: int, dev) -> int:
    """done [T, N, n_agents] and truncated [T, N] (or None), contiguous bool / uint8 on dev; returns n_agents >= 1."""
    for name, t, nd in (("done", done, 3), ("truncated", truncated, 2)):
        if name == "truncated" and t is None:
            continue
        if t.dtype not in (torch.bool, torch.uint8) or t.device != dev or not t.is_contiguous() or t.dim() != nd or tuple(t.shape[:2]) != (T, N):
            raise ValueError(f"{what}: {name} must be contiguous bool / uint8 [{T}, {N}{', n_agents' if nd == 3 else ''}] on {dev}")
    if done.shape[2] < 1:
        raise ValueError(f"{what}: done needs at least one agent column")
    return done.shape[2]


def obs_rows(what: str, obs, n_rows: int, dev, at_least: bool = False):
    """The one or two per-agent observation row tensors a PPO critic reads from (an agent it does not read may be None): each
    contiguous float32 [.., D_k] with n_rows rows (at_least: or more).  Returns ([rows 0, rows 1], their widths without trailing
    zeros) — what `CriticParams.as_c` takes."""
    obs = list(obs) + [None] * (2 - len(obs))
    widths = []
    for k, r in enumerate(obs[:2]):
        if r is None:
            widths.append(0)
            continue
        n = r[..., 0].numel() if isinstance(r, torch.Tensor) and r.dim() >= 2 else -1
        if n < 0 or r.dtype != F32 or r.device != dev or not r.is_contiguous() or (n < n_rows if at_least else n != n_rows):
            raise ValueError(f"{what}: observation rows {k} must be contiguous float32 [{'>= ' if at_least else ''}{n_rows} rows, D] on {dev}")
        widths.append(r.shape[-1])
    while widths and widths[-1] == 0:
        widths.pop()
    return obs, widths
