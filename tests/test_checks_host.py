"""The shared argument checks (gym_rotor_amd/_checks.py) and the one launch tail (_lib.launch, _lib.workspace_bytes) without a GPU:
one case per clause of the tensor check, the element-stride rules, the alpha parse, and how a launch hands its arguments on."""
import contextlib
import ctypes as C
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gym_rotor_amd import _checks as ck  # noqa: E402
from gym_rotor_amd import _lib as L  # noqa: E402

CPU = torch.device("cpu")
F32 = torch.float32


# ---------------------------------------------------------------- the tensor check
@pytest.mark.parametrize("clause, make", [
    ("wrong dtype", lambda: torch.zeros(3, 4, dtype=torch.float64)),
    ("wrong device", lambda: torch.zeros(3, 4, device="meta")),
    ("wrong rank", lambda: torch.zeros(3, 4, 1)),
    ("wrong extent", lambda: torch.zeros(3, 5)),
    ("non-contiguous view", lambda: torch.zeros(4, 3).t()),
    ("None where not allowed", lambda: None),
])
def test_tensor_check_refuses(clause, make):
    with pytest.raises(ValueError) as e:
        ck.tensor("some_op", "some_arg", make(), F32, (3, 4), CPU)
    msg = str(e.value)
    assert msg.startswith("some_op: some_arg must be") and "float32" in msg and "[3, 4]" in msg and "cpu" in msg, clause


def test_tensor_check_passes():
    x = torch.zeros(3, 4)
    assert ck.tensor("some_op", "some_arg", x, F32, (3, 4), CPU) is x
    assert ck.tensor("some_op", "some_arg", None, F32, (3, 4), CPU, optional=True) is None    # None where allowed
    with pytest.raises(ValueError, match="some_op: some_arg must be a contiguous float32 \\[3, 4\\] tensor on cpu"):
        ck.tensor("some_op", "some_arg", torch.zeros(3), F32, (3, 4), CPU, optional=True)      # ... which excuses nothing else
    flag = torch.zeros(3, 4, dtype=torch.uint8)
    assert ck.tensor("some_op", "flag", flag, (torch.bool, torch.uint8), (3, 4), CPU) is flag  # one of several dtypes
    with pytest.raises(ValueError, match="bool / uint8"):
        ck.tensor("some_op", "flag", x, (torch.bool, torch.uint8), (3, 4), CPU)
    assert ck.rows("some_op", "obs", torch.zeros(7, 4), 4, CPU) == 7                           # an open extent, returned
    for bad in (torch.zeros(7, 5), torch.zeros(7), torch.zeros(7, 4, 1)):
        with pytest.raises(ValueError, match="some_op: obs must be a contiguous float32 \\[rows, 4\\] tensor on cpu"):
            ck.rows("some_op", "obs", bad, 4, CPU)
    assert ck.index("some_op", None, CPU, 9) == 9 and ck.index("some_op", torch.zeros(5, dtype=torch.int64), CPU, 9) == 5
    with pytest.raises(ValueError, match="some_op: index must be a contiguous int64 \\[B\\] tensor on cpu"):
        ck.index("some_op", torch.zeros(5, dtype=torch.int32), CPU, 9)


def test_flat_scalar_and_gpu_only():
    assert ck.flat("some_op", "y", torch.zeros(6, 1), F32, 6, CPU) is not None                 # any shape of that many entries
    for bad in (torch.zeros(5), torch.zeros(6, dtype=torch.float64), torch.zeros(12)[::2], torch.zeros(6, device="meta"), None):
        with pytest.raises(ValueError, match="some_op: y must be a contiguous float32 tensor of 6 entries on cpu"):
            ck.flat("some_op", "y", bad, F32, 6, CPU)
    assert ck.flat("some_op", "y", None, F32, 6, CPU, optional=True) is None
    one = torch.zeros(1, 1)
    assert ck.scalar("some_op", "alpha_grad", one, F32, CPU) is one and ck.scalar("some_op", "alpha_grad", None, F32, CPU) is None
    for bad in (torch.zeros(2), torch.zeros(1, dtype=torch.float64), torch.zeros(1, device="meta"), 0.5):
        with pytest.raises(ValueError, match="some_op: alpha_grad must be a float32 tensor of one entry on cpu"):
            ck.scalar("some_op", "alpha_grad", bad, F32, CPU)
    with pytest.raises(ValueError, match="some_op: draw_dev must be an int64 tensor of one entry on cpu"):
        ck.scalar("some_op", "draw_dev", one, torch.int64, CPU)
    with pytest.raises(RuntimeError, match="GPU only"):
        ck.require_gpu(CPU)
    ck.require_gpu(torch.device("cuda", 0))                                                    # (asks the device's type only)
    with pytest.raises(ValueError, match="some_op: step must be an int64 tensor of one entry on cpu"):
        ck.scalar("some_op", "step", None, torch.int64, CPU, optional=False)                   # a required one
    ck.nonneg("some_op", ("lam_T", "lam_S"), 0.0, 3)
    for bad in (-1e-9, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="some_op: lam_S must be finite and >= 0"):
            ck.nonneg("some_op", ("lam_T", "lam_S"), 0.0, bad)


def test_named_loops_over_tensor_and_flat():
    shapes = {"w": (3, 4), "b": (3,)}
    good = {"w": torch.zeros(3, 4), "b": torch.zeros(3)}
    ck.named("some_op", "grads[{!r}]", good, shapes, CPU)
    ck.named("some_op", "grads[{!r}]", {"w": torch.zeros(12), "b": torch.zeros(3, 1)}, shapes, CPU, by_numel=True)   # entries, any shape
    ck.named("some_op", "{}", {"w": None}, shapes, CPU, optional=True)                         # None and missing pass when optional
    for bad in (torch.zeros(4, 3), torch.zeros(3, 4, dtype=torch.float64), torch.zeros(3, 4, device="meta"), torch.zeros(4, 3).t(), None):
        with pytest.raises(ValueError, match="some_op: grads\\['w'\\] must be a contiguous float32 \\[3, 4\\] tensor on cpu"):
            ck.named("some_op", "grads[{!r}]", dict(good, w=bad), shapes, CPU)
    with pytest.raises(ValueError, match="some_op: grads\\['b'\\] must be a contiguous float32 tensor of 3 entries on cpu"):
        ck.named("some_op", "grads[{!r}]", dict(good, b=torch.zeros(4)), shapes, CPU, by_numel=True)
    with pytest.raises(ValueError, match="some_op: w must be"):
        ck.named("some_op", "{}", {"w": torch.zeros(3)}, shapes, CPU, optional=True)           # optional excuses nothing else


# ---------------------------------------------------------------- column / element_stride
def test_column_and_element_stride():
    n = 6
    wide = torch.zeros(n, 3)
    for t, stride in ((torch.zeros(n), 1), (torch.zeros(n, 1), 1), (wide[:, 1], 3)):
        assert ck.column("some_op", "rwd", t, n, CPU) == stride
        assert ck.element_stride("some_op", "rwd", t) == stride
    transposed = torch.zeros(2, 3).t()                                                         # [3, 2] with strides (1, 3): two strides
    with pytest.raises(ValueError, match="some_op: rwd must have one positive element stride"):
        ck.column("some_op", "rwd", transposed, n, CPU)
    with pytest.raises(ValueError, match="some_op: rwd must have one element stride"):
        ck.element_stride("some_op", "rwd", transposed)
    assert ck.element_stride("some_op", "adv", torch.zeros(4, 5, 2)[..., 1]) == 2              # a column of a contiguous [T, N, n_agents]
    for one in (torch.zeros(1), torch.zeros(1, 1), wide[:1, 1]):                               # n = 1: nothing to stride over
        assert ck.column("some_op", "rwd", one, 1, CPU) == 1 and ck.element_stride("some_op", "rwd", one) == 1
    for bad in (torch.zeros(n + 1), torch.zeros(n, dtype=torch.float64), torch.zeros(n, device="meta"), None):
        with pytest.raises(ValueError, match="some_op: rwd must be float32 with 6 elements on cpu"):
            ck.column("some_op", "rwd", bad, n, CPU)


def test_strided_rows():
    rows = torch.zeros(6, 5)
    assert ck.strided_rows("some_op", "action", rows, 6, 4, CPU, wider=True) == 5
    assert ck.strided_rows("some_op", "action", rows[:, :4], 6, 4, CPU) == 5                   # a per-agent view of wider rows
    assert ck.strided_rows("some_op", "action", rows[:1, :4], 1, 4, CPU) == 4                  # one row: its own width
    for bad in (rows[:, :3], torch.zeros(6, 10)[:, ::2], torch.zeros(5, 6).t(), torch.zeros(5, 5), torch.zeros(6, 5, dtype=torch.float64)):
        with pytest.raises(ValueError, match="some_op: action must be float32 \\[6, >= 4\\] rows with unit column stride on cpu"):
            ck.strided_rows("some_op", "action", bad, 6, 4, CPU, wider=True)


# ---------------------------------------------------------------- the alpha parse
def test_alpha_parse():
    assert ck.alpha("some_op", 0.25, CPU) == (0.25, None)
    dev = torch.full((1,), 0.25)
    a, a_dev = ck.alpha("some_op", dev, CPU)
    assert a == 0.0 and a_dev is dev                                                           # the device word wins over the float
    for bad in (-0.1, float("inf")):
        with pytest.raises(ValueError, match="some_op: alpha must be finite and >= 0"):
            ck.alpha("some_op", bad, CPU)
    for bad in (torch.zeros(2), torch.zeros(1, dtype=torch.float64)):
        with pytest.raises(ValueError, match="some_op: alpha must be a Python float or a float32 tensor of one element on cpu"):
            ck.alpha("some_op", bad, CPU)


# ---------------------------------------------------------------- _lib.launch / _lib.workspace_bytes
class _Struct(C.Structure):
    _fields_ = [("a", C.c_int32)]


def test_launch_hands_its_arguments_on(monkeypatch):
    """The entry is looked up by name at call time; a Structure arrives by reference, None, ints and ctypes arrays as they are, the
    stream last; the return code goes through _lib.check under the entry's name — which, as every launch's did before, reports a
    refusal of the library (negative) as ValueError and a hipError_t (positive) as QuadrotorLibError."""
    calls, rc = [], [0]

    class Library:
        def qr_some_entry(self, *args):
            calls.append(args)
            return rc[0]

    entered = []
    monkeypatch.setattr(L, "load", lambda: Library())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=1234))
    monkeypatch.setattr(torch.cuda, "device", lambda device: entered.append(device) or contextlib.nullcontext())
    s, arr = _Struct(7), (_Struct * 2)()
    L.launch(CPU, "qr_some_entry", s, None, 5, arr)
    (by_ref, none, five, as_is, stream), = calls
    assert C.cast(by_ref, C.POINTER(_Struct)).contents.a == 7 and C.addressof(C.cast(by_ref, C.POINTER(_Struct)).contents) == C.addressof(s)
    assert none is None and five == 5 and as_is is arr and stream == 1234 and entered == [CPU]
    with pytest.raises(AttributeError, match="qr_no_such_entry"):
        L.launch(CPU, "qr_no_such_entry")
    rc[0] = -3
    with pytest.raises(ValueError, match="qr_some_entry: QR_E_SIZE"):
        L.launch(CPU, "qr_some_entry", s)
    rc[0] = 700
    with pytest.raises(L.QuadrotorLibError, match="qr_some_entry: hipError_t 700"):
        L.launch(CPU, "qr_some_entry", s)


def test_workspace_bytes(monkeypatch):
    seen = []

    class Library:
        def qr_some_workspace_bytes(self, *args):
            seen.append(args)
            return 4096 if args[-1] >= 0 else -3

    monkeypatch.setattr(L, "load", lambda: Library())
    assert L.workspace_bytes("qr_some_workspace_bytes", 23, torch.Size([16])[0], 128.0, 0) == 4096
    assert seen == [(23, 16, 128, 0)] and all(type(v) is int for v in seen[0])
    with pytest.raises(ValueError, match="qr_some_workspace_bytes: QR_E_SIZE"):
        L.workspace_bytes("qr_some_workspace_bytes", 23, 16, 128, -1)
