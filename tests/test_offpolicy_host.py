"""qr_adamw_polyak_step, PolyakAdamW and the off-policy updaters without a GPU: the struct mirror, every argument error of the C entry
and of the Python layers (all raised before a launch), the float64 restatement of tests/offpolicy_ref.py against torch's own
clip_grad_norm_ + AdamW + scheduler + the soft-update line on double tensors for a twelve-tensor group, and why the group of twelve
exists: one joint clip is not two clips of six."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from offpolicy_ref import polyak_f64, polyak_step_f64, run_polyak_f64
from optim_ref import adamw_step_f64, run_torch
from test_sac_critic_host import _SacActor
from test_td3_critic_host import _Actor, _Twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, SIZE, ALIGN = -1, -3, -4
TWIN = lambda D, H: [(H, D), (H,), (H, H), (H,), (1, H), (1,)] * 2


def test_struct_mirrors_the_header(tmp_path):
    from gym_rotor_amd import _lib as L
    ct = L.QrAdamWPolyakGroup
    lines = ['printf("S %zu\\n", sizeof(QrAdamWPolyakGroup));']
    lines += [f'printf("{f} %zu\\n", offsetof(QrAdamWPolyakGroup, {f}));' for f, _ in ct._fields_]
    lines.append('printf("abi %d\\n", QR_ABI_VERSION);')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "quadrotor_hip.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["S"]) == C.sizeof(ct) == 552
    for f, _ in ct._fields_:
        assert int(out[f]) == getattr(ct, f).offset, f
    assert "qr_adamw_polyak_step" in L.SYMBOLS and hasattr(L.load(), "qr_adamw_polyak_step")
    assert int(out["abi"]) == L.ABI_VERSION == 16                     # only a struct and an entry were added
    assert (L.POLYAK_MAX_GROUPS, L.POLYAK_MAX_TENSORS) == (7, 16) and L.POLYAK_MAX_GROUPS * 552 <= 4096 < 8 * 552


COUNTS = (5 * 9, 5, 25, 5, 5, 1) * 2


def _fake(n_tensors=12, targets=True):
    """A group on fake device addresses that passes every check but the last one made: its step pointer is not 8-byte aligned (never
    launched: every case below returns before a launch)."""
    from gym_rotor_amd import _lib as L
    g = L.QrAdamWPolyakGroup()
    g.n_tensors = n_tensors
    for k in range(n_tensors):
        g.param[k], g.grad[k], g.count[k] = 0x10000 + 0x1000 * k, 0x80000 + 0x1000 * k, COUNTS[k]
        g.target[k] = 0x500000 + 0x1000 * k if targets else None
    g.exp_avg, g.exp_avg_sq, g.step, g.stats = 0x100000, 0x200000, 0x300004, 0x400000
    g.lr, g.eta_min, g.t0, g.tau = 2e-4, 1e-5, 1_000_000, 0.005
    g.beta1, g.beta2, g.eps, g.weight_decay, g.max_norm = 0.9, 0.999, 1e-8, 1e-2, 100.0
    return g


def _edit(g, edit):
    for k, v in edit.items():
        if isinstance(v, tuple):
            getattr(g, k)[v[0]] = v[1]
        else:
            setattr(g, k, v)
    return g


def test_abi_argument_errors_without_gpu():
    from gym_rotor_amd import _lib as L
    lib = L.load()

    def call(groups, n=None):
        arr = (L.QrAdamWPolyakGroup * len(groups))(*groups)
        return lib.qr_adamw_polyak_step(arr, len(groups) if n is None else n, None)

    assert lib.qr_adamw_polyak_step(None, 1, None) == NULL
    assert call([_fake()]) == ALIGN                                   # every other check passes: only the step pointer is misaligned
    for n in (0, -1, 8):
        assert call([_fake()] * 8, n) == SIZE
    assert call([_fake()] * 7) == ALIGN                               # seven groups are a legal launch

    def expect(code, what, one_entry=False, **edit):
        g = _edit(_fake(), dict(n_tensors=1, count=(0, 1)) if one_entry else {})
        _edit(g, edit)
        assert g.step is None or g.step & 7                           # (the fake's own fault is still there: nothing can launch)
        assert call([g]) == code, (what, edit)

    for k in (0, 11):
        expect(NULL, "param", param=(k, None))
        expect(NULL, "grad", grad=(k, None))
        expect(ALIGN, "a target is optional", target=(k, None))
        expect(SIZE, "a target that is its parameter", target=(k, 0x10000 + 0x1000 * k))
        expect(ALIGN, "target alignment", target=(k, 0x500002))
    for n in ("exp_avg", "exp_avg_sq", "step"):
        expect(NULL, n, **{n: None})
    expect(ALIGN, "stats is optional", stats=None)
    expect(ALIGN, "unused slots are not read", n_tensors=11, param=(11, None), grad=(11, None), count=(11, -1), target=(11, 0x10000 + 0x1000 * 11))
    expect(ALIGN, "the largest group", count=(0, 65536 - (sum(COUNTS) - COUNTS[0])))
    expect(SIZE, "one entry more", count=(0, 65536 - (sum(COUNTS) - COUNTS[0]) + 1))
    for n in (0, -1, 17):
        expect(SIZE, "n_tensors", n_tensors=n)
    expect(SIZE, "reserved0", reserved0=1)
    expect(SIZE, "count", count=(3, 0))
    nan, inf = float("nan"), float("inf")
    for name in ("lr", "eta_min", "eps", "weight_decay"):
        for bad in (-1e-3, nan, inf):
            expect(SIZE, name, **{name: bad})
    for name in ("beta1", "beta2"):
        for bad in (-0.1, 1.0, nan):
            expect(SIZE, name, **{name: bad})
    expect(SIZE, "t0", t0=-1)
    expect(SIZE, "max_norm", max_norm=nan)
    for bad in (-1e-9, 1.0 + 1e-9, nan, inf):
        expect(SIZE, "tau", tau=bad)
    for ok in (0.0, 1.0):
        expect(ALIGN, "tau's ends are legal", tau=ok)
    expect(SIZE, "exp_out on twelve tensors", exp_out=0x600000)
    expect(SIZE, "exp_out on one tensor of two entries", n_tensors=1, count=(0, 2), exp_out=0x600000)
    expect(SIZE, "exp_out on two tensors of one entry", n_tensors=2, count=(0, 1), exp_out=0x600000)
    expect(ALIGN, "exp_out on one entry", one_entry=True, exp_out=0x600000)
    sixteen = _fake()
    sixteen.n_tensors = 16
    for k in range(16):
        sixteen.param[k], sixteen.grad[k], sixteen.target[k], sixteen.count[k] = 0x10000 + 64 * k, 0x80000 + 64 * k, None, 1
    assert call([sixteen]) == ALIGN                                   # sixteen tensors are a legal group

    def aligned(**edit):                                              # the step pointer aligned: the fault named is the only one
        g, first = _edit(_fake(), dict(step=0x300000)), _edit(_fake(), dict(step=0x300000))
        _edit(g, edit)
        return call([g]), call([first, first, g])                     # alone, and as the last group of a launch

    for edit in (dict(param=(2, 0x12002)), dict(grad=(11, 0x86001)), dict(target=(5, 0x505001)), dict(exp_avg=0x100002), dict(stats=0x400002),
                 dict(step=0x300004)):
        assert aligned(**edit) == (ALIGN, ALIGN), edit
    assert aligned(n_tensors=1, count=(0, 1), exp_out=0x600002) == (ALIGN, ALIGN)
    assert aligned(tau=2.0) == (SIZE, SIZE) and aligned(n_tensors=0) == (SIZE, SIZE) and aligned(exp_out=0x600000) == (SIZE, SIZE)
    assert aligned(exp_avg=None) == (NULL, NULL) and aligned(param=(11, None)) == (NULL, NULL)


def _twin_inputs(seed, D=9, H=5, scale=(1.0, 1.0)):
    """A twelve-tensor twin critic (odd sizes), targets, and gradient sets whose Q1 / Q2 halves have the 2-norms `scale`."""
    rng = np.random.default_rng(seed)
    shapes = TWIN(D, H)
    p, t = [rng.uniform(-0.5, 0.5, s) for s in shapes], [rng.uniform(-0.5, 0.5, s) for s in shapes]

    def grads(s1, s2):
        g = [rng.normal(size=s) for s in shapes]
        n1, n2 = (np.sqrt(sum((a * a).sum() for a in h)) for h in (g[:6], g[6:]))
        return [a * s1 / n1 for a in g[:6]] + [a * s2 / n2 for a in g[6:]]

    return p, t, grads


def test_restatement_reproduces_torch_for_twelve_tensors():
    """adamw + the soft-update line + exp in float64 against torch's own pieces on double tensors, clipping active in steps 1 and 3."""
    p, t, grads = _twin_inputs(5)
    sets = [grads(0.3, 0.2), grads(2.0, 1.5), grads(0.5, 0.1), grads(0.9, 0.9), grads(0.2, 0.2)]
    hyper = dict(lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=1.0, t0=3, eta_min=1e-5)
    tau = 0.005
    got_p, got_m, got_v, got_t, infos = run_polyak_f64(p, sets, t, tau=tau, **hyper)
    assert [i["clip_coef"] < 1.0 for i in infos] == [False, True, False, True, False]
    # torch: the same steps one by one, the reference's line after each (td3.py:207-208)
    want_t = [torch.as_tensor(a).clone() for a in t]
    for j in range(len(sets)):
        pj, _, _, _ = run_torch(p, sets[:j + 1], torch.float64, **hyper)
        want_t = [tau * torch.as_tensor(a) + (1 - tau) * b for a, b in zip(pj, want_t)]
    want_p, want_m, want_v, _ = run_torch(p, sets, torch.float64, **hyper)
    for got, want in ((got_p, want_p), (got_m, want_m), (got_v, want_v), (got_t, [w.numpy() for w in want_t])):
        for a, b in zip(got, want):
            assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())
    # polyak off in some steps: the targets move only in the others; mixed targets: None stays None
    _, _, _, some, _ = run_polyak_f64(p, sets, t, polyak_steps={1, 4}, tau=tau, **hyper)
    p1 = run_polyak_f64(p, sets[:2], t, polyak_steps=set(), tau=tau, **hyper)[0]
    once = polyak_f64(p1, t, tau)
    assert all(np.array_equal(a, b) for a, b in zip(polyak_f64(got_p, once, tau), some))
    mixed = polyak_step_f64(p, sets[0], [np.zeros_like(a) for a in p], [np.zeros_like(a) for a in p], 0, [None] + t[1:], tau=tau, **hyper)[3]
    assert mixed[0] is None and all(m is not None for m in mixed[1:])
    # exp_out: exp of the NEW one-entry parameter
    la, _, _, _, e, _ = polyak_step_f64([np.array([0.25])], [np.array([-0.7])], [np.zeros(1)], [np.zeros(1)], 0, exp_out=True, lr=3e-4)
    ref = torch.nn.Parameter(torch.tensor([0.25], dtype=torch.float64))
    opt = torch.optim.AdamW([ref], lr=3e-4)
    ref.grad = torch.tensor([-0.7], dtype=torch.float64)
    opt.step()
    assert abs(la[0][0] - float(ref.detach())) <= 1e-15 and abs(e - float(ref.detach().exp())) <= 1e-15 and la[0][0] > 0.25


def test_one_joint_clip_is_not_two_clips_of_six():
    """Why the group of twelve exists.  Each half's gradient norm (0.8, 0.75) is below max_norm = 1, the joint norm (1.097) above it:
    the reference's clip_grad_norm_(critic.parameters()) scales all twelve gradients by 1 / 1.097, two groups of six scale nothing —
    and the parameters after one step differ."""
    p, _, grads = _twin_inputs(7)
    g = grads(0.8, 0.75)
    hyper = dict(lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=1.0, t0=1_000_000, eta_min=1e-5)
    zeros = lambda xs: [np.zeros_like(a) for a in xs]
    joint_p, joint_m, _, info = adamw_step_f64(p, g, zeros(p), zeros(p), 0, **hyper)
    assert info["total_norm"] > 1.0 and abs(info["total_norm"] - np.hypot(0.8, 0.75)) < 1e-12 and info["clip_coef"] < 1.0
    halves = [adamw_step_f64(p[h], g[h], zeros(p[h]), zeros(p[h]), 0, **hyper) for h in (slice(0, 6), slice(6, 12))]
    assert all(h[3]["total_norm"] < 1.0 and h[3]["clip_coef"] == 1.0 for h in halves)
    split_m = halves[0][1] + halves[1][1]
    # exp_avg shows the coefficient directly: (1 - beta1) * clip * g
    for a, b, gk in zip(joint_m, split_m, g):
        assert np.allclose(a, b * info["clip_coef"], rtol=1e-12) and np.abs(a - b).max() > 0.05 * 0.1 * np.abs(gk).max()
    # torch's joint clip agrees with the joint restatement, not with the split one
    want_p, want_m, _, norms = run_torch(p, [g], torch.float64, **hyper)
    assert abs(norms[0] - info["total_norm"]) < 1e-12
    for a, b, c, gk in zip(joint_m, want_m, split_m, g):               # the split moments are off by (1 - beta1) (1 - clip) |g|
        assert np.abs(a - b).max() <= 1e-15 and np.isclose(np.abs(c - b).max(), 0.1 * (1.0 - info["clip_coef"]) * np.abs(gk).max(), rtol=1e-9)
    assert all(np.abs(a - b).max() <= 1e-15 for a, b in zip(joint_p, want_p))
    # Adam's first step is lr * g / (|g| + eps'), blind to the gradient's scale: the parameters differ only where |g| is near eps.  A
    # second step whose joint norm (0.36) is below max_norm mixes unclipped gradients into moments that were clipped (joint) or not
    # (split), and the parameters part by a few per cent of lr
    g2 = grads(0.3, 0.2)
    j2 = adamw_step_f64(joint_p, g2, joint_m, adamw_step_f64(p, g, zeros(p), zeros(p), 0, **hyper)[2], 1, **hyper)[0]
    s2 = [adamw_step_f64(h[0], g2[sl], h[1], h[2], 1, **hyper)[0] for h, sl in zip(halves, (slice(0, 6), slice(6, 12)))]
    assert max(np.abs(a - b).max() for a, b in zip(j2, s2[0] + s2[1])) > 1e-7


def _with_grads(m):
    for q in m.parameters():
        q.grad = torch.ones_like(q)
    return m


def test_polyak_adamw_argument_checks():
    from gym_rotor_amd import DeviceAdamW, PolyakAdamW, adamw_polyak_step
    twin, twin_t = _with_grads(_Twin(27, 5)), _Twin(27, 5)
    ps, ts = list(twin.parameters()), [q.data for q in twin_t.parameters()]
    opt = PolyakAdamW(ps, targets=ts, lr=2e-4, max_norm=100.0, t0=1_000_000, eta_min=1e-5)
    assert len(opt.params) == 12 and opt.numel == 2 * (27 * 5 + 5 + 25 + 5 + 5 + 1) and opt.exp_avg.shape == (opt.numel,)
    assert opt.tau == 0.005 and opt.exp_out is None and isinstance(opt, DeviceAdamW)
    g = opt._fill(True)
    assert g.n_tensors == 12 and list(g.target[:12]) == [t.data_ptr() for t in ts] and g.target[12] is None and g.tau == 0.005
    assert list(opt._fill(False).target) == [None] * 16                # polyak=False: the launch has no target
    for call in (lambda: opt.step(), lambda: opt.step(polyak=False), lambda: PolyakAdamW.step_all([(opt, True)])):
        with pytest.raises(RuntimeError, match="GPU only"):          # every check passes: no CPU kernel exists
            call()
    with pytest.raises(ValueError, match="1..16 parameter tensors, got 17"):
        PolyakAdamW([torch.zeros(2) for _ in range(17)], lr=1e-3)
    with pytest.raises(ValueError, match="1..16 parameter tensors, got 0"):
        PolyakAdamW([], lr=1e-3)
    with pytest.raises(ValueError, match="parameter 1 must be a contiguous float32"):
        PolyakAdamW([torch.zeros(4), torch.zeros(4, dtype=torch.float64)], lr=1e-3)
    with pytest.raises(ValueError, match="parameter 1 is on meta"):
        PolyakAdamW([torch.zeros(4), torch.zeros(4, device="meta")], lr=1e-3)
    with pytest.raises(ValueError, match="at most 65536"):
        PolyakAdamW([torch.zeros(65536), torch.zeros(1)], lr=1e-3)
    with pytest.raises(ValueError, match="targets holds 11 entries for 12"):
        PolyakAdamW(ps, targets=ts[:11], lr=1e-3)
    with pytest.raises(ValueError, match="target 3 must be a contiguous float32 tensor of 5 entries"):
        PolyakAdamW(ps, targets=ts[:3] + [torch.zeros(6)] + ts[4:], lr=1e-3)
    with pytest.raises(ValueError, match="target 0 must be"):
        PolyakAdamW(ps, targets=[ts[0].double()] + ts[1:], lr=1e-3)
    with pytest.raises(ValueError, match="target 2 is its own parameter"):
        PolyakAdamW(ps, targets=ts[:2] + [ps[2].data] + ts[3:], lr=1e-3)
    assert PolyakAdamW(ps, targets=[None] + ts[1:], lr=1e-3)._fill().target[0] is None
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="tau must lie"):
            PolyakAdamW(ps, targets=ts, tau=bad, lr=1e-3)
    for bad in (dict(lr=-1.0), dict(betas=(0.9, 1.0)), dict(eps=-1.0), dict(t0=-1), dict(max_norm=float("nan")), dict(eta_min=-1e-5)):
        with pytest.raises(ValueError, match="PolyakAdamW"):
            PolyakAdamW(ps, **{"lr": 1e-3, **bad})
    one = torch.zeros(1, requires_grad=True)
    with pytest.raises(ValueError, match="exp_out needs a group of one entry"):
        PolyakAdamW(ps, exp_out=torch.zeros(1), lr=1e-3)
    with pytest.raises(ValueError, match="exp_out must be a float32 tensor of one entry"):
        PolyakAdamW([one], exp_out=torch.zeros(2), lr=1e-3)
    with pytest.raises(ValueError, match="exp_out must be"):
        PolyakAdamW([one], exp_out=one.data, lr=1e-3)
    la = PolyakAdamW([one], exp_out=torch.zeros(1), lr=3e-4)
    with pytest.raises(ValueError, match="parameter 0 has no .grad"):
        la.step()
    one.grad = torch.zeros(1)
    assert la._fill().exp_out is not None and la._fill(False).exp_out is not None     # exp_out does not depend on polyak
    with pytest.raises(ValueError, match="appears twice"):
        PolyakAdamW.step_all([(opt, True), (opt, False)])
    with pytest.raises(ValueError, match="takes PolyakAdamW"):
        PolyakAdamW.step_all([DeviceAdamW([torch.zeros(2)], lr=1e-3)])
    with pytest.raises(ValueError, match="one device"):
        PolyakAdamW.step_all([opt, PolyakAdamW([torch.zeros(3, device="meta")], lr=1e-3)])
    PolyakAdamW.step_all([])
    # state_dict: DeviceAdamW's, the addresses kept
    opt.exp_avg.copy_(torch.randn(opt.numel)); opt.step_count.fill_(4)
    other = PolyakAdamW(list(_Twin(27, 5).parameters()), lr=1.0)
    ptrs = (other.exp_avg.data_ptr(), other.exp_avg_sq.data_ptr(), other.step_count.data_ptr())
    other.load_state_dict(opt.state_dict())
    assert torch.equal(other.exp_avg, opt.exp_avg) and other.steps == 4 and other.hyper() == opt.hyper()
    assert ptrs == (other.exp_avg.data_ptr(), other.exp_avg_sq.data_ptr(), other.step_count.data_ptr())
    # the functional form and the torch op
    p, g = [torch.zeros(3), torch.zeros(2)], [torch.zeros(3), torch.zeros(2)]
    st = dict(exp_avg=torch.zeros(5), exp_avg_sq=torch.zeros(5), step=torch.zeros(1, dtype=torch.int64), stats=None)
    with pytest.raises(RuntimeError, match="GPU only"):
        adamw_polyak_step(p, g, [torch.zeros(3), None], **st, lr=1e-3)
    with pytest.raises(ValueError, match="as many gradients"):
        adamw_polyak_step(p, g[:1], None, **st, lr=1e-3)
    with pytest.raises(ValueError, match="one entry per parameter"):
        adamw_polyak_step(p, g, [None], **st, lr=1e-3)
    with pytest.raises(ValueError, match="target 1 must be"):
        adamw_polyak_step(p, g, [None, torch.zeros(3)], **st, lr=1e-3)
    with pytest.raises(ValueError, match="tau must lie"):
        adamw_polyak_step(p, g, None, **st, tau=-1.0, lr=1e-3)
    with pytest.raises(ValueError, match="exp_avg must be"):
        adamw_polyak_step(p, g, None, **{**st, "exp_avg": torch.zeros(4)}, lr=1e-3)
    with pytest.raises(ValueError, match="exp_out must be"):
        adamw_polyak_step(p, g, None, **st, exp_out=torch.zeros(1), lr=1e-3)
    assert hasattr(torch.ops.gym_rotor_amd, "qr_adamw_polyak_step")
    with pytest.raises(RuntimeError, match="GPU only"):
        torch.ops.gym_rotor_amd.qr_adamw_polyak_step(p, g, [torch.zeros(2)], [1], st["exp_avg"], st["exp_avg_sq"], st["step"], None, None, 0.005, 1e-3,
                                                     0.9, 0.999, 1e-8, 1e-2, -1.0, 0, 0.0)


def test_updater_argument_checks():
    from gym_rotor_amd import ReplayBuffer, SacUpdater, Td3Updater
    a, c, at, ct = _Actor(23, 16, 4), _Twin(27, 5), _Actor(23, 16, 4), _Twin(27, 5)
    nominal = [torch.zeros(4)]
    up = Td3Updater([a], [c], [at], [ct], nominal=nominal, batch_size=8)
    assert (up.policy_update_freq, up.tau, up.discount, up.grad_max_norm, up.lr_a, up.lr_c) == (3, 0.005, 0.99, 100.0, [3e-4], [2e-4])
    assert len(up.critic_opts[0].params) == 12 and len(up.actor_opts[0].params) == 6 and up.critic_opts[0].targets[0].data_ptr() == ct.fc1.weight.data_ptr()
    assert up.critic_opts[0].hyper()["t0"] == 1_000_000 and up.critic_opts[0].eta_min == 1e-5 and up.actor_opts[0].max_norm == 100.0
    with pytest.raises(ValueError, match="mode must be one of"):
        Td3Updater([a], [c], [at], [ct], mode="coupled", nominal=nominal)
    with pytest.raises(ValueError, match="one actor, critic and critic target per agent"):
        Td3Updater([a], [c, c], [at], [ct], nominal=nominal)
    with pytest.raises(ValueError, match="one actor target per agent"):
        Td3Updater([a], [c], [at, at], [ct], nominal=nominal)
    with pytest.raises(ValueError, match="'single' is one agent"):
        Td3Updater([a], [c], [at], [ct], mode="ctde", nominal=nominal)
    with pytest.raises(ValueError, match="lam_M != 0 needs"):
        Td3Updater([a], [c], [at], [ct])
    with pytest.raises(ValueError, match="has no layer fc4"):
        Td3Updater([a], [a], [at], [ct], nominal=nominal)
    for bad in (dict(tau=1.5), dict(policy_update_freq=0), dict(batch_size=0), dict(discount=-1.0), dict(max_action=0.0), dict(lr_a=[1e-3, 1e-3]),
                dict(target_noise=-1.0), dict(lr_c=-1.0), dict(grad_max_norm=float("nan"))):
        with pytest.raises(ValueError):
            Td3Updater([a], [c], [at], [ct], nominal=nominal, **bad)
    buf = ReplayBuffer(16, [23], [4], "cpu")
    with pytest.raises(ValueError, match="cannot draw 8 of 0"):
        up.update(buf)
    with pytest.raises(ValueError, match="2 agents"):
        up.update(ReplayBuffer(16, [15, 3], [4, 1], "cpu"))
    with pytest.raises(ValueError, match="must be a ReplayBuffer"):
        up.update({})
    with pytest.raises(ValueError, match="iterations must be >= 1"):
        up.update(buf, 0)
    with pytest.raises(ValueError, match="use_device_state"):
        up.capture(buf)
    assert up.total_it == 0
    sa = _SacActor(23, 16, 4)
    sup = SacUpdater([sa], [c], [ct], nominal=nominal, automatic_entropy_tuning=True, batch_size=8)
    assert len(sup.actor_opts[0].params) == 8 and sup.actor_opts[0].targets is None and sup.alpha_opts[0].exp_out is sup.alpha[0]
    assert float(sup.alpha[0]) == float(np.float32(0.05)) and float(sup.log_alpha[0].detach()) == 0.0
    assert sup.alpha_opts[0].max_norm == -1.0 and sup.alpha_opts[0].t0 == 0 and sup.alpha_opts[0].lr == 3e-4
    fixed = SacUpdater([sa], [c], [ct], nominal=nominal)
    assert fixed.alpha == [0.05] and fixed.alpha_opts == [None] and fixed.policy_update_freq == 3
    with pytest.raises(ValueError, match="has no layer mean_linear"):
        SacUpdater([a], [c], [ct], nominal=nominal)
    with pytest.raises(ValueError, match="sac_alpha must be"):
        SacUpdater([sa], [c], [ct], nominal=nominal, sac_alpha=-1.0)
    with pytest.raises(ValueError, match="target_entropy is None"):
        SacUpdater([sa], [c], [ct], nominal=nominal, target_entropy=[-4.0, -1.0])
    with pytest.raises(ValueError, match="cannot draw"):
        sup.update(buf)
