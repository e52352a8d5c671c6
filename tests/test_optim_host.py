"""The device-side optimiser step (qr_adamw_step, DeviceAdamW, PpoUpdater) without a GPU: the float64 restatement the GPU tests
compare against (tests/optim_ref.py), checked against torch's own clip_grad_norm_ + AdamW + CosineAnnealingWarmRestarts on double
tensors; the C-ABI struct mirror and argument errors; the host-side argument checks; the state_dict round trip; the minibatch
slicing."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from optim_ref import run_f64, run_torch, schedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, SIZE, ALIGN = -1, -3, -4


@pytest.mark.parametrize("max_norm", [0.5, 1e3, -1.0])             # clipping active in every step, never, off
def test_float64_restatement_reproduces_torch(max_norm):
    rng = np.random.default_rng(11)
    shapes = [(5, 3), (5,), (2, 5), (1, 2)]
    p = [rng.normal(size=s) for s in shapes]
    grads = [[rng.normal(size=s) for s in shapes] for _ in range(7)]
    hyper = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=max_norm, t0=3, eta_min=1e-4)   # 7 steps: two restarts
    p64, m64, v64, infos = run_f64(p, grads, **hyper)
    pt, mt, vt, norms = run_torch(p, grads, torch.float64, **hyper)
    for got, want in ((p64, pt), (m64, mt), (v64, vt)):
        for a, b in zip(got, want):
            assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())
    assert [i["t"] for i in infos] == list(range(1, 8))
    assert np.allclose([i["lr_t"] for i in infos[:4]], [3e-3, schedule(1, 3e-3, 3, 1e-4), schedule(2, 3e-3, 3, 1e-4), 3e-3], rtol=1e-15)
    if max_norm >= 0:
        assert np.allclose([i["total_norm"] for i in infos], norms, rtol=1e-12)
        assert all((i["clip_coef"] < 1.0) == (max_norm == 0.5) for i in infos)
    else:
        assert all(i["clip_coef"] == 1.0 for i in infos)


def test_struct_mirrors_the_header(tmp_path):
    from gym_rotor_amd import _lib as L
    ct = L.QrAdamWGroup
    lines = ['printf("QrAdamWGroup %zu\\n", sizeof(QrAdamWGroup));']
    lines += [f'printf("QrAdamWGroup.{f} %zu\\n", offsetof(QrAdamWGroup, {f}));' for f, _ in ct._fields_]
    lines.append('printf("abi %d\\n", QR_ABI_VERSION);')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "quadrotor_hip.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["QrAdamWGroup"]) == C.sizeof(ct) == 248
    for f, _ in ct._fields_:
        assert int(out[f"QrAdamWGroup.{f}"]) == getattr(ct, f).offset, f
    assert "qr_adamw_step" in L.SYMBOLS and hasattr(L.load(), "qr_adamw_step")
    assert int(out["abi"]) == L.ABI_VERSION == 16


def _fake(n_tensors=7, counts=(368, 16, 256, 16, 64, 4, 4)):
    """A QrAdamWGroup on fake device addresses that passes every check but the last one made: its step pointer is not 8-byte aligned
    (never launched: every case of the test below returns before a launch)."""
    from gym_rotor_amd import _lib as L
    g = L.QrAdamWGroup()
    g.n_tensors = n_tensors
    for k in range(n_tensors):
        g.param[k], g.grad[k], g.count[k] = 0x10000 + 0x1000 * k, 0x80000 + 0x1000 * k, counts[k]
    g.exp_avg, g.exp_avg_sq, g.step, g.stats = 0x100000, 0x200000, 0x300004, 0x400000
    g.lr, g.eta_min, g.t0 = 3e-4, 1e-5, 1_000_000
    g.beta1, g.beta2, g.eps, g.weight_decay, g.max_norm = 0.9, 0.999, 1e-8, 1e-2, 100.0
    return g


def test_abi_argument_errors_without_gpu():
    from gym_rotor_amd import _lib as L
    lib = L.load()

    def call(groups, n=None):
        arr = (L.QrAdamWGroup * len(groups))(*groups)
        return lib.qr_adamw_step(arr, len(groups) if n is None else n, None)

    assert lib.qr_adamw_step(None, 1, None) == NULL
    assert call([_fake()]) == ALIGN                                   # every other check passes: only the step pointer is misaligned
    for n in (0, -1, 9):
        assert call([_fake()], n) == SIZE

    def expect(code, what, **edit):
        g = _fake()
        for k, v in edit.items():
            if isinstance(v, tuple):
                getattr(g, k)[v[0]] = v[1]
            else:
                setattr(g, k, v)
        assert g.step is None or g.step & 7                           # (the fake's own fault is still there: nothing can launch)
        assert call([g]) == code, (what, edit)

    for k in (0, 6):
        expect(NULL, "param", param=(k, None))
        expect(NULL, "grad", grad=(k, None))
    for n in ("exp_avg", "exp_avg_sq", "step"):
        expect(NULL, n, **{n: None})
    expect(ALIGN, "stats is optional", stats=None)                    # (ALIGN = reached the last check)
    expect(ALIGN, "unused slots are not read", n_tensors=6, param=(6, None), grad=(6, None), count=(6, -1))
    expect(ALIGN, "one tensor of one entry", n_tensors=1, count=(0, 1))
    expect(ALIGN, "the largest group", count=(0, 65536 - 360))
    expect(SIZE, "one entry more", count=(0, 65536 - 360 + 1))
    for n in (0, -1, 9):
        expect(SIZE, "n_tensors", n_tensors=n)
    expect(SIZE, "count", count=(3, 0))
    expect(SIZE, "count", count=(3, -4))
    nan, inf = float("nan"), float("inf")
    for name in ("lr", "eta_min", "eps", "weight_decay"):
        for bad in (-1e-3, nan, inf):
            expect(SIZE, name, **{name: bad})
        expect(ALIGN, name + " = 0 is legal", **{name: 0.0})
    for name in ("beta1", "beta2"):
        for bad in (-0.1, 1.0, 1.5, nan):
            expect(SIZE, name, **{name: bad})
        expect(ALIGN, name + " = 0 is legal", **{name: 0.0})
    expect(SIZE, "t0", t0=-1)
    expect(ALIGN, "t0 = 0 is legal", t0=0)
    expect(SIZE, "max_norm", max_norm=nan)
    expect(ALIGN, "max_norm < 0 and infinite are legal", max_norm=-1.0)
    expect(ALIGN, "max_norm < 0 and infinite are legal", max_norm=inf)

    def aligned(**edit):                                              # the step pointer aligned: the fault named is the only one
        g = _fake()
        g.step = 0x300000
        for k, v in edit.items():
            if isinstance(v, tuple):
                getattr(g, k)[v[0]] = v[1]
            else:
                setattr(g, k, v)
        first = _fake()
        first.step = 0x300000
        return call([g]), call([first, first, g])                     # alone, and as the last group of a launch

    for edit in (dict(param=(2, 0x12002)), dict(grad=(6, 0x86001)), dict(exp_avg=0x100002), dict(exp_avg_sq=0x200001), dict(stats=0x400002),
                 dict(step=0x300001), dict(step=0x300004)):
        assert aligned(**edit) == (ALIGN, ALIGN), edit
    assert aligned(lr=-1.0) == (SIZE, SIZE) and aligned(beta2=1.0) == (SIZE, SIZE) and aligned(n_tensors=0) == (SIZE, SIZE)
    assert aligned(exp_avg=None) == (NULL, NULL) and aligned(param=(6, None)) == (NULL, NULL) and aligned(step=None) == (NULL, NULL)


def _module():
    torch.manual_seed(3)
    return torch.nn.Sequential(torch.nn.Linear(5, 4), torch.nn.Linear(4, 2))


def _with_grads(m):
    for p in m.parameters():
        p.grad = torch.ones_like(p)
    return m


def test_device_adamw_argument_checks():
    from gym_rotor_amd import DeviceAdamW, adamw_step
    m = _with_grads(_module())
    opt = DeviceAdamW(m.parameters(), lr=1e-3, max_norm=100.0, t0=1_000_000, eta_min=1e-5)
    assert opt.numel == 34 and opt.exp_avg.shape == (34,) and opt.step_count.dtype == torch.int64 and opt.stats.shape == (4,)
    assert opt.betas == (float(np.float32(0.9)), float(np.float32(0.999))) and opt.eps == float(np.float32(1e-8))
    with pytest.raises(RuntimeError, match="GPU only"):              # every check passes: no CPU kernel exists
        opt.step()
    with pytest.raises(RuntimeError, match="GPU only"):
        DeviceAdamW.step_all([opt, DeviceAdamW(_with_grads(_module()).parameters(), lr=1e-3)])
    with pytest.raises(ValueError, match="parameter 0 must be a contiguous float32"):
        DeviceAdamW([torch.zeros(4, 6).t()], lr=1e-3)
    with pytest.raises(ValueError, match="parameter 1 must be a contiguous float32"):
        DeviceAdamW([torch.zeros(4), torch.zeros(4, dtype=torch.float64)], lr=1e-3)
    with pytest.raises(ValueError, match="parameter 0 must be a contiguous float32"):
        DeviceAdamW([torch.zeros(0)], lr=1e-3)
    with pytest.raises(ValueError, match="parameter 1 is on meta"):
        DeviceAdamW([torch.zeros(4), torch.zeros(4, device="meta")], lr=1e-3)
    with pytest.raises(ValueError, match="1..8 parameter tensors, got 9"):
        DeviceAdamW([torch.zeros(2) for _ in range(9)], lr=1e-3)
    with pytest.raises(ValueError, match="1..8 parameter tensors, got 0"):
        DeviceAdamW([], lr=1e-3)
    with pytest.raises(ValueError, match="at most 65536"):
        DeviceAdamW([torch.zeros(65536), torch.zeros(1)], lr=1e-3)
    for bad in (dict(lr=-1.0), dict(lr=float("nan")), dict(betas=(0.9, 1.0)), dict(betas=(-0.1, 0.9)), dict(eps=-1.0), dict(weight_decay=float("inf")),
                dict(t0=-1), dict(max_norm=float("nan")), dict(eta_min=-1e-5)):
        with pytest.raises(ValueError, match="DeviceAdamW"):
            DeviceAdamW(m.parameters(), **{"lr": 1e-3, **bad})
    # .grad: missing, wrong dtype, not contiguous, another device
    ps = list(m.parameters())
    ps[1].grad = None
    with pytest.raises(ValueError, match="parameter 1 has no .grad"):
        opt.step()
    ps[1].grad = torch.ones_like(ps[1])
    w = torch.zeros(4, 6).t().contiguous().requires_grad_()
    w.grad = torch.zeros(4, 6).t()
    with pytest.raises(ValueError, match=r"\.grad of parameter 0 must be a contiguous float32"):
        DeviceAdamW([w], lr=1e-3).step()
    with pytest.raises(ValueError, match="one device"):
        other = DeviceAdamW([torch.zeros(3, device="meta")], lr=1e-3)
        DeviceAdamW.step_all([opt, other])
    with pytest.raises(ValueError, match="appears twice"):
        DeviceAdamW.step_all([opt, opt])
    DeviceAdamW.step_all([])                                          # nothing to do
    # the functional form and the torch op
    p, g = [torch.zeros(3), torch.zeros(2)], [torch.zeros(3), torch.zeros(2)]
    st = dict(exp_avg=torch.zeros(5), exp_avg_sq=torch.zeros(5), step=torch.zeros(1, dtype=torch.int64), stats=None)
    with pytest.raises(RuntimeError, match="GPU only"):
        adamw_step(p, g, **st, lr=1e-3)
    with pytest.raises(ValueError, match="as many gradients"):
        adamw_step(p, g[:1], **st, lr=1e-3)
    with pytest.raises(ValueError, match="gradient 1 must be"):
        adamw_step(p, [g[0], torch.zeros(3)], **st, lr=1e-3)
    with pytest.raises(ValueError, match="exp_avg must be"):
        adamw_step(p, g, **{**st, "exp_avg": torch.zeros(4)}, lr=1e-3)
    with pytest.raises(ValueError, match="step must be an int64"):
        adamw_step(p, g, **{**st, "step": torch.zeros(1, dtype=torch.int32)}, lr=1e-3)
    with pytest.raises(ValueError, match="stats must be"):
        adamw_step(p, g, **{**st, "stats": torch.zeros(3)}, lr=1e-3)
    assert hasattr(torch.ops.gym_rotor_amd, "qr_adamw_step")
    with pytest.raises(RuntimeError, match="GPU only"):
        torch.ops.gym_rotor_amd.qr_adamw_step(p, g, st["exp_avg"], st["exp_avg_sq"], st["step"], None, 1e-3, 0.9, 0.999, 1e-8, 1e-2, -1.0, 0, 0.0)


def test_state_dict_round_trip_and_readbacks():
    from gym_rotor_amd import DeviceAdamW
    m = _module()
    a = DeviceAdamW(m.parameters(), lr=2e-4, max_norm=100.0, t0=10, eta_min=1e-5)
    a.exp_avg.copy_(torch.randn(34)); a.exp_avg_sq.copy_(torch.rand(34)); a.step_count.fill_(13)
    sd = a.state_dict()
    assert set(sd) == {"step", "exp_avg", "exp_avg_sq", "hyper"} and sd["exp_avg"].data_ptr() != a.exp_avg.data_ptr()
    b = DeviceAdamW(_module().parameters(), lr=1.0)
    ptrs = (b.exp_avg.data_ptr(), b.exp_avg_sq.data_ptr(), b.step_count.data_ptr())
    b.load_state_dict(sd)
    assert torch.equal(b.exp_avg, a.exp_avg) and torch.equal(b.exp_avg_sq, a.exp_avg_sq) and b.steps == a.steps == 13
    assert b.hyper() == a.hyper() and ptrs == (b.exp_avg.data_ptr(), b.exp_avg_sq.data_ptr(), b.step_count.data_ptr())
    a.exp_avg.zero_()                                                 # the dict holds copies
    assert not torch.equal(sd["exp_avg"], a.exp_avg)
    assert b.current_lr() == schedule(13, 2e-4, 10, 1e-5) and DeviceAdamW(m.parameters(), lr=7e-4).current_lr() == 7e-4
    # the launch struct of the continued run is that of the original, field by field (the pointers aside)
    _with_grads(m)
    ga, gb = a._fill(), DeviceAdamW(m.parameters(), lr=1.0)
    gb.load_state_dict(sd)
    gb = gb._fill()
    for f in ("n_tensors", "lr", "eta_min", "t0", "beta1", "beta2", "eps", "weight_decay", "max_norm"):
        assert getattr(ga, f) == getattr(gb, f), f
    assert list(ga.count) == list(gb.count) == [20, 4, 8, 2, 0, 0, 0, 0] and list(ga.param) == list(gb.param)
    with pytest.raises(ValueError, match="exp_avg must be"):
        DeviceAdamW([torch.zeros(3)], lr=1e-3).load_state_dict(sd)


def test_minibatch_slicing():
    from gym_rotor_amd import minibatch_slices
    sl = minibatch_slices(210, 128)
    assert sl == [slice(0, 128), slice(128, 210)]
    perm = torch.randperm(210, generator=torch.Generator().manual_seed(1))
    parts = [perm[s] for s in sl]
    assert [p.numel() for p in parts] == [128, 82] and torch.equal(torch.cat(parts).sort().values, torch.arange(210))
    assert all(p.is_contiguous() and p.data_ptr() % 8 == 0 for p in parts)
    assert minibatch_slices(256, 128) == [slice(0, 128), slice(128, 256)] and minibatch_slices(5, 128) == [slice(0, 5)]
    assert [s.stop - s.start for s in minibatch_slices(7, 3)] == [3, 3, 1]
    with pytest.raises(ValueError):
        minibatch_slices(0, 128)
    with pytest.raises(ValueError):
        minibatch_slices(10, 0)


def test_ppo_updater_argument_checks():
    from gym_rotor_amd import DeviceAdamW, PpoUpdater
    from test_critic_host import _Critic
    from test_ppo_actor_host import _Actor
    from test_ppo_critic_host import _cpu_storage
    actor, critic = _Actor(23, 16, 4), _Critic(23, 62)
    oa, oc = DeviceAdamW(actor.parameters(), lr=3e-4), DeviceAdamW(critic.parameters(), lr=2e-4)
    assert oa.numel == 728 and oc.numel == 5457
    up = PpoUpdater([actor], [critic], [oa], [oc], K_epochs=2, lam_T=0.0, lam_S=0.0, lam_M=0.0)
    assert up.critic_inputs == [(0,)] and up.entropy_coef == 1e-2
    with pytest.raises(ValueError, match="one actor, critic"):
        PpoUpdater([actor], [critic, critic], [oa], [oc])
    with pytest.raises(ValueError, match=">= 1"):
        PpoUpdater([actor], [critic], [oa], [oc], K_epochs=0)
    with pytest.raises(ValueError, match="2 agents"):
        up.update(_cpu_storage("decoupled"), torch.zeros(3, 5, 2))
    with pytest.raises(RuntimeError, match="GPU only"):              # the first actor_loss of the loop: no CPU kernel exists
        up.update(_cpu_storage(), torch.zeros(3, 5, 1))
    assert up.entropy_coef == 1e-2 * 0.99                             # decayed once, before use
