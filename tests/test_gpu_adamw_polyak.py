"""adamw_polyak_kernel on the GPU (qr_adamw_polyak_step, PolyakAdamW, the torch op): the bits of DeviceAdamW where both take a group, the
float64 restatement of tests/offpolicy_ref.py under the bar of tests/test_gpu_optim.py (`_check`: torch's own float32 error, or the
rounding term), the targets against `soft_update` run after the step bit for bit, exp_out against numpy's float64 exp, the shape
limits, several groups per launch, guarded buffers and a NaN gradient."""
import numpy as np
import pytest
import torch

from offpolicy_ref import run_polyak_f64
from optim_ref import run_torch
from test_gpu_optim import HYPER, K, NORMS, SENTINEL, _check, _cuda, _guarded, _inputs, _np

pytestmark = pytest.mark.gpu
TAU = 0.005
TWIN = [(5, 9), (5,), (5, 5), (5,), (1, 5), (1,)] * 2                # hidden width 5: odd sizes, twelve tensors, 172 entries


def _twin_inputs(seed=3):
    """Float32 parameters, targets and K gradient sets of the total norms NORMS (above max_norm = 1 in steps 2 and 4)."""
    rng = np.random.default_rng(seed)
    p = [(rng.uniform(-1, 1, s) * 0.5).astype(np.float32) for s in TWIN]
    t = [(rng.uniform(-1, 1, s) * 0.5).astype(np.float32) for s in TWIN]
    sets = []
    for norm in NORMS:
        g = [rng.normal(size=s) for s in TWIN]
        scale = norm / np.sqrt(sum((a * a).sum() for a in g))
        sets.append([(a * scale).astype(np.float32) for a in g])
    return p, t, sets


def _run(p, sets, targets=None, polyak=True, exp_out=None, hyper=HYPER, tau=TAU, soft_after=False):
    """K steps of a fresh PolyakAdamW on clones.  soft_after: step with polyak=False and run soft_update after each step.  Returns
    (params, exp_avg, exp_avg_sq per tensor, targets, optimiser, stats per step)."""
    from gym_rotor_amd import PolyakAdamW, soft_update
    params = [torch.nn.Parameter(_cuda(a)) for a in p]
    tg = None if targets is None else [None if a is None else _cuda(a) for a in targets]
    opt = PolyakAdamW(params, targets=tg, tau=tau, exp_out=exp_out, **hyper)
    hist = []
    for g in sets:
        for q, gk in zip(params, g):
            q.grad = _cuda(gk)
        opt.step(polyak=polyak and not soft_after)
        if soft_after:
            pairs = [(q.data, t) for q, t in zip(params, tg) if t is not None]
            soft_update([a for a, _ in pairs], [b for _, b in pairs], tau)
        hist.append(opt.stats.clone())
    torch.cuda.synchronize()
    sizes = [q.numel() for q in params]
    return [q.data for q in params], list(opt.exp_avg.split(sizes)), list(opt.exp_avg_sq.split(sizes)), tg, opt, hist


@pytest.mark.parametrize("name", ["actor_23_16_4", "critic_23_62"])
def test_bits_of_device_adamw(name):
    """A 7-tensor actor group and a 6-tensor critic group without targets: DeviceAdamW's bits over 3 steps."""
    from test_gpu_optim import _device_run
    p, sets = _inputs(name)
    a = _device_run(p, sets[:3], HYPER)
    b = _run(p, sets[:3])
    for x, y in zip(a[0] + a[1] + a[2], b[0] + b[1] + b[2]):
        assert torch.equal(x, y)
    assert torch.equal(a[3].step_count, b[4].step_count) and int(b[4].step_count) == 3
    assert all(torch.equal(x, y) for x, y in zip(a[4], b[5])) and torch.equal(a[3].stats, b[4].stats)


@pytest.fixture(scope="module")
def twin():
    p, t, sets = _twin_inputs()
    return dict(p=p, t=t, sets=sets, f64=run_polyak_f64(p, sets, t, tau=TAU, **HYPER), t32=run_torch(p, sets, torch.float32, "cuda", **HYPER))


def test_twin_critic_against_float64_and_soft_update(twin):
    d = twin
    p64, m64, v64, t64, infos = d["f64"]
    coefs = [i["clip_coef"] for i in infos]
    assert any(c < 1.0 for c in coefs) and any(c == 1.0 for c in coefs)              # clipping active in some steps, inactive in others
    fused = _run(d["p"], d["sets"], d["t"])
    _check("twin 12 tensors", fused[:3], (p64, m64, v64), d["t32"], K, HYPER["lr"])
    assert int(fused[4].step_count) == K and float(fused[4].stats[3]) == K
    for st, info in zip(fused[5], infos):
        st = _np(st).astype(np.float64)
        assert abs(st[0] - info["total_norm"]) <= 2.0 ** -22 * info["total_norm"] and abs(st[1] - info["clip_coef"]) <= 2.0 ** -22 * info["clip_coef"]
    # the targets: the bits of soft_update run after each step; and against the float64 line four half-ulps of the largest value per
    # step (float32(1 - tau), the two products, the sum; the parameter's own error enters times tau)
    after = _run(d["p"], d["sets"], d["t"], soft_after=True)
    assert all(torch.equal(a, b) for a, b in zip(fused[3], after[3]))
    for a, w in zip(fused[3], t64):
        assert np.abs(_np(a).astype(np.float64) - w).max() <= K * 4 * 2.0 ** -24 * max(1.0, np.abs(w).max())
    # the parameters and moments do not depend on polyak
    plain = _run(d["p"], d["sets"], d["t"], polyak=False)
    for x, y in zip(fused[0] + fused[1] + fused[2], plain[0] + plain[1] + plain[2]):
        assert torch.equal(x, y)
    assert all(torch.equal(t, _cuda(t0)) for t, t0 in zip(plain[3], d["t"]))           # polyak=False: the targets are untouched
    assert all(torch.equal(x, y) for x, y in zip(fused[0], after[0]))


def test_mixed_targets_leave_the_others_alone(twin):
    d = twin
    targets = [a if k % 3 else None for k, a in enumerate(d["t"])]
    sizes = [a.size for a in d["p"]]
    buf, mask, views = _guarded(sizes)                                                 # twins of ALL twelve, sentinels where there is no target
    for v, a in zip(views, targets):
        if a is not None:
            v.copy_(_cuda(a).reshape(-1))
    from gym_rotor_amd import PolyakAdamW
    params = [torch.nn.Parameter(_cuda(a)) for a in d["p"]]
    opt = PolyakAdamW(params, targets=[None if a is None else v for v, a in zip(views, targets)], tau=TAU, **HYPER)
    for g in d["sets"][:2]:
        for q, gk in zip(params, g):
            q.grad = _cuda(gk)
        opt.step()
    torch.cuda.synchronize()
    full = _run(d["p"], d["sets"][:2], d["t"])
    assert bool((buf[mask] == SENTINEL).all())
    for k, (v, a) in enumerate(zip(views, targets)):
        if a is None:
            assert bool((v == SENTINEL).all()), k
        else:
            assert torch.equal(v, full[3][k].reshape(-1)), k
    assert all(torch.equal(q.data, x) for q, x in zip(params, full[0]))


def test_shape_limits_and_exp_out():
    rng = np.random.default_rng(8)
    # sixteen tensors of one entry each, every one with a target
    p = [rng.uniform(-1, 1, (1,)).astype(np.float32) for _ in range(16)]
    t = [rng.uniform(-1, 1, (1,)).astype(np.float32) for _ in range(16)]
    sets = [[rng.normal(size=(1,)).astype(np.float32) for _ in range(16)] for _ in range(2)]
    got = _run(p, sets, t)
    after = _run(p, sets, t, soft_after=True)
    f64 = run_polyak_f64(p, sets, t, tau=TAU, **HYPER)
    _check("16 x 1", got[:3], f64[:3], run_torch(p, sets, torch.float32, "cuda", **HYPER), 2, HYPER["lr"])
    assert all(torch.equal(a, b) for a, b in zip(got[3] + got[0], after[3] + after[0]))
    # one tensor of 65 536 entries: 256 entries per thread
    p, t = [rng.uniform(-1, 1, (65536,)).astype(np.float32)], [rng.uniform(-1, 1, (65536,)).astype(np.float32)]
    sets = [[rng.normal(size=(65536,)).astype(np.float32) * 0.01] for _ in range(2)]
    got, after = _run(p, sets, t), _run(p, sets, t, soft_after=True)
    f64 = run_polyak_f64(p, sets, t, tau=TAU, **HYPER)
    _check("1 x 65536", got[:3], f64[:3], run_torch(p, sets, torch.float32, "cuda", **HYPER), 2, HYPER["lr"])
    assert torch.equal(got[3][0], after[3][0]) and torch.equal(got[0][0], after[0][0])
    # one entry with exp_out: SAC's log_alpha (AdamW at lr_a, no clip, no schedule)
    hyper = dict(lr=3e-4, betas=HYPER["betas"], eps=HYPER["eps"], weight_decay=HYPER["weight_decay"])
    p, sets = [np.array([0.3], dtype=np.float32)], [[np.array([g], dtype=np.float32)] for g in (-0.8, 1.7, -0.2)]
    buf, mask, (alpha,) = _guarded([1])
    with_exp, without = _run(p, sets, exp_out=alpha, hyper=hyper), _run(p, sets, hyper=hyper)
    assert torch.equal(with_exp[0][0], without[0][0]) and torch.equal(with_exp[1][0], without[1][0]) and torch.equal(with_exp[2][0], without[2][0])
    want = np.exp(np.float64(_np(with_exp[0][0])[0]))
    assert abs(np.float64(_np(alpha)[0]) - want) <= np.spacing(np.float32(want)) and bool((buf[mask] == SENTINEL).all())
    assert abs(_np(with_exp[0][0])[0] - run_polyak_f64(p, sets, [None], **hyper)[0][0][0]) <= 3 * 2.0 ** -24 * (4 * 0.3 + 16 * 3e-4)
    # exp_out is written whatever polyak says
    alpha2 = torch.zeros(1, device="cuda")
    _run(p, sets, exp_out=alpha2, hyper=hyper, polyak=False)
    assert torch.equal(alpha2, alpha)


def _nine(twin, poison=None):
    """Nine optimisers over groups of 12, 16, 1 (with exp_out), ... tensors, with their gradients set."""
    from gym_rotor_amd import PolyakAdamW
    rng = np.random.default_rng(21)
    opts = []
    for j in range(9):
        if j % 3 == 0:
            shapes, tg = TWIN, True
        elif j % 3 == 1:
            shapes, tg = [(3,)] * 16, True
        else:
            shapes, tg = [(1,)], False
        params = [torch.nn.Parameter(_cuda((rng.uniform(-1, 1, s) * 0.5).astype(np.float32))) for s in shapes]
        for q in params:
            q.grad = _cuda(rng.normal(size=tuple(q.shape)).astype(np.float32))
        targets = [_cuda(rng.uniform(-1, 1, s).astype(np.float32)) for s in shapes] if tg else None
        exp_out = None if tg else torch.zeros(1, device="cuda")
        opts.append(PolyakAdamW(params, targets=targets, tau=TAU, exp_out=exp_out, **HYPER))
    if poison is not None:
        opts[poison].params[3].grad.view(-1)[0] = float("nan")
    return opts


def _state(o):
    return [q.data for q in o.params] + [o.exp_avg, o.exp_avg_sq, o.step_count, o.stats] + [t for t in (o.targets or [])] + ([o.exp_out] if o.exp_out is not None else [])


def test_groups_per_launch_and_nan_isolation(twin):
    from gym_rotor_amd import PolyakAdamW, _lib
    assert _lib.POLYAK_MAX_GROUPS == 7
    one_by_one = _nine(twin)
    for o in one_by_one:
        o.step()
    for n in (7, 8, 9):                                               # one full launch; 7 + 1; 7 + 2
        together = _nine(twin)
        PolyakAdamW.step_all(together[:n])
        torch.cuda.synchronize()
        for a, b in zip(one_by_one[:n], together[:n]):
            assert all(torch.equal(x, y) for x, y in zip(_state(a), _state(b)))
        assert all(int(o.step_count) == 0 for o in together[n:])
    mixed = _nine(twin)
    PolyakAdamW.step_all([(o, j % 2 == 0) for j, o in enumerate(mixed)])  # polyak per group
    fresh = _nine(twin)
    for j, (a, b, c) in enumerate(zip(mixed, one_by_one, fresh)):
        assert all(torch.equal(x, y) for x, y in zip(a.params, b.params))
        if a.targets is not None:
            assert all(torch.equal(x, y) for x, y in zip(a.targets, (b if j % 2 == 0 else c).targets))
    # a NaN gradient stays in its own group
    bad = _nine(twin, poison=3)
    PolyakAdamW.step_all(bad)
    torch.cuda.synchronize()
    assert bool(torch.isnan(bad[3].params[3].data).all()) and bool(torch.isnan(bad[3].stats[0]))
    for j, (a, b) in enumerate(zip(bad, one_by_one)):
        if j != 3:
            assert all(torch.equal(x, y) for x, y in zip(_state(a), _state(b))), j


def test_guarded_buffers_and_torch_op(twin):
    """Parameters, moments, stats, targets and exp_out in guarded buffers: nothing outside is written; the functional form and the
    torch op give the class's bits."""
    from gym_rotor_amd import adamw_polyak_step
    d = twin
    sizes = [a.size for a in d["p"]]
    total = sum(sizes)
    ref = _run(d["p"], d["sets"][:2], d["t"])

    def guarded_run(call):
        buf, mask, views = _guarded(sizes + sizes + [total, total, 4])
        ibuf, imask, (step,) = _guarded([1], torch.int64, gap=2)
        params, targets, (m, v, stats) = views[:12], views[12:24], views[24:]
        for q, a, t, b in zip(params, d["p"], targets, d["t"]):
            q.copy_(_cuda(a).reshape(-1)); t.copy_(_cuda(b).reshape(-1))
        m.zero_(); v.zero_(); stats.zero_(); step.zero_()
        keep = ibuf[imask].clone()
        for s in d["sets"][:2]:
            call(params, [_cuda(g).reshape(-1) for g in s], targets, m, v, step, stats)
        torch.cuda.synchronize()
        assert bool((buf[mask] == SENTINEL).all()) and torch.equal(ibuf[imask], keep) and int(step) == 2
        assert all(torch.equal(a, b.reshape(-1)) for a, b in zip(params, ref[0])) and all(torch.equal(a, b.reshape(-1)) for a, b in zip(targets, ref[3]))
        assert torch.equal(m, ref[4].exp_avg) and torch.equal(v, ref[4].exp_avg_sq) and torch.equal(stats, ref[4].stats)

    guarded_run(lambda p, g, t, m, v, step, stats: adamw_polyak_step(p, g, t, m, v, step, stats, tau=TAU, **HYPER))
    h = HYPER
    guarded_run(lambda p, g, t, m, v, step, stats: torch.ops.gym_rotor_amd.qr_adamw_polyak_step(
        p, g, t, list(range(12)), m, v, step, stats, None, TAU, h["lr"], h["betas"][0], h["betas"][1], h["eps"], h["weight_decay"], h["max_norm"],
        h["t0"], h["eta_min"]))
    # the one-entry group with exp_out, everything guarded
    buf, mask, (p, m, v, stats, alpha) = _guarded([1, 1, 1, 4, 1])
    ibuf, imask, (step,) = _guarded([1], torch.int64, gap=2)
    p.fill_(0.3); m.zero_(); v.zero_(); stats.zero_(); step.zero_()
    adamw_polyak_step([p], [torch.full((1,), -0.8, device="cuda")], None, m, v, step, stats, alpha, lr=3e-4)
    torch.cuda.synchronize()
    assert bool((buf[mask] == SENTINEL).all()) and int(step) == 1 and float(p) > 0.3
    assert abs(np.float64(float(alpha)) - np.exp(np.float64(float(p)))) <= np.spacing(np.float32(np.exp(np.float64(float(p)))))
