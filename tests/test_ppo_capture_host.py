"""The replayable PPO update without a GPU (qr_ppo_actor_grad_dev; entropy_coef_dev=, PpoUpdater's device sources, capture,
state_dict): every error code of the new C entry on made-up addresses, every ValueError of the new arguments — each before a launch —
and the state's round trip."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_critic_host import _Critic  # noqa: E402
from test_ppo_actor_host import _Actor, _fake, _host_args  # noqa: E402
from test_ppo_critic_host import _cpu_storage  # noqa: E402

from gym_rotor_amd import DeviceAdamW, PpoUpdater, _lib as L  # noqa: E402

NULL, KIND, SIZE, ALIGN = -1, -2, -3, -4


def _call(q, b, g, word, entry="qr_ppo_actor_grad_dev"):
    lib = L.load()
    ref = lambda x: None if x is None else C.byref(x)
    if entry == "qr_ppo_actor_grad":
        return lib.qr_ppo_actor_grad(ref(q), ref(b), ref(g), None)
    return lib.qr_ppo_actor_grad_dev(ref(q), ref(b), ref(g), word, None)


def test_dev_entry_error_codes():
    """`_fake` passes every check but the workspace's size (one byte short), the last one: so SIZE means "every other check passed"."""
    q, b, g = _fake()
    for word in (None, 0x900000, 0x900004):
        assert _call(q, b, g, word) == SIZE
        assert _call(None, b, g, word) == NULL and _call(q, None, g, word) == NULL and _call(q, b, None, word) == NULL
    for word in (0x900001, 0x900002, 0x900003):
        assert _call(q, b, g, word) == ALIGN
    # the existing entry's codes, in its order, with a word and without one
    edits = [(NULL, "q", "fc1_w", None), (NULL, "g", "log_std", None), (NULL, "g", "stats", None), (NULL, "b", "obs", None), (NULL, "b", "noise", None),
             (KIND, "q", "squash", L.ACTOR_TANH_SAMPLE), (SIZE, "q", "hidden_dim", 4), (SIZE, "b", "batch", 0), (SIZE, "b", "max_workgroups", -1),
             (ALIGN, "b", "obs", 0x100002), (ALIGN, "g", "fc2_w", 0x800001), (ALIGN, "b", "index", 0x170004), (ALIGN, "b", "workspace", 0x1A0004)]
    for code, which, name, value in edits:
        for word in (None, 0x900000):
            q, b, g = _fake()
            setattr({"q": q, "b": b, "g": g}[which], name, value)
            assert _call(q, b, g, word) == code == _call(q, b, g, None, "qr_ppo_actor_grad"), (which, name, value)
    # a misaligned word is seen before the workspace is measured, and not before a NULL pointer or a bad size
    q, b, g = _fake()
    b.obs = None
    assert _call(q, b, g, 0x900002) == NULL
    q, b, g = _fake()
    b.batch = 0
    assert _call(q, b, g, 0x900002) == SIZE


def test_entropy_coef_dev_argument_checks():
    from gym_rotor_amd import ActorParams, actor_loss, ppo_actor_grad
    m = _Actor(23, 16, 4)
    actor = ActorParams.from_module(m)
    bad = (torch.zeros(1, dtype=torch.float64), torch.zeros(2), torch.zeros(0), torch.zeros(1, device="meta"), 0.01)
    for word in bad:
        with pytest.raises(ValueError, match="entropy_coef_dev"):
            ppo_actor_grad(actor, **_host_args(), entropy_coef_dev=word)
    with pytest.raises(RuntimeError, match="GPU only"):     # a good word: every check passed, there is no CPU kernel
        ppo_actor_grad(actor, **_host_args(), entropy_coef_dev=torch.zeros(1))
    st = _cpu_storage()
    for word in bad:
        with pytest.raises(ValueError, match="entropy_coef_dev"):
            st.actor_grad(0, actor, torch.zeros(3, 5, 1), entropy_coef_dev=word)
        with pytest.raises(ValueError, match="entropy_coef_dev"):
            actor_loss(m, st, 0, torch.zeros(3, 5, 1), entropy_coef_dev=word)
    with pytest.raises(RuntimeError, match="GPU only"):
        actor_loss(m, st, 0, torch.zeros(3, 5, 1), entropy_coef_dev=torch.zeros(3)[1:2])
    assert hasattr(torch.ops.gym_rotor_amd, "qr_ppo_actor_grad_dev") and hasattr(torch.ops.gym_rotor_amd, "qr_shuffle")
    a = _host_args()
    with pytest.raises(RuntimeError, match="GPU only"):
        torch.ops.gym_rotor_amd.qr_ppo_actor_grad_dev([p.data for p in m.parameters()],
                                                      a["obs"], None, None, None, a["action"], a["logp_old"], a["advantage"], None, None, None,
                                                      [torch.zeros_like(p) for p in m.parameters()], torch.zeros(4), torch.zeros(1), 0, 0.2, 0.0, 0.0,
                                                      0.0, 1.0)


def _updater(**kw):
    actor, critic = _Actor(23, 16, 4), _Critic(23, 62)
    oa, oc = DeviceAdamW(actor.parameters(), lr=3e-4), DeviceAdamW(critic.parameters(), lr=2e-4)
    return PpoUpdater([actor], [critic], [oa], [oc], K_epochs=2, nominal=[torch.zeros(4)], **kw), actor, critic


def test_updater_source_arguments():
    up, _, _ = _updater(noise=[torch.zeros(23)])
    assert (up.shuffle_source, up.noise_source, up.seed, up.noise_std) == ("torch", "torch", 0, 0.05)
    assert up.state is None and up.entropy_dev is None and not up.device_sources
    for kw in (dict(shuffle_source="device"), dict(noise_source="device"), dict(shuffle_source="device", noise_source="device", seed=2 ** 64 - 1)):
        up, _, _ = _updater(**kw)
        assert up.device_sources and up.state.dtype == torch.int64 and up.state.tolist() == [0, 0] and (up.epoch_draw, up.minibatch_draw) == (0, 0)
        assert up.entropy_dev.dtype == torch.float32 and up.entropy_dev.tolist() == [C.c_float(1e-2).value]
        if kw.get("noise_source") == "device":
            assert [tuple(t.shape) for t in up.noise] == [(23,)] and up.noise[0].dtype == torch.float32
    for bad in (dict(shuffle_source="philox"), dict(noise_source="philox"), dict(noise_source=None), dict(seed=-1), dict(seed=2 ** 64),
                dict(noise_source="device", noise=[torch.zeros(23)]), dict(noise_std=-0.1), dict(noise_std=float("nan")), dict(noise_std=float("inf"))):
        with pytest.raises(ValueError):
            _updater(**bad)
    up, _, _ = _updater(shuffle_source="device", noise=[torch.zeros(23)])
    with pytest.raises(ValueError, match="generator"):
        up.update(_cpu_storage(), torch.zeros(3, 5, 1), generator=torch.Generator())
    assert up.entropy_coef == 1e-2                                   # refused before the decay
    with pytest.raises(RuntimeError, match="GPU only"):              # the shuffle, the epoch's first launch: no CPU kernel exists
        up.update(_cpu_storage(), torch.zeros(3, 5, 1))
    assert up.entropy_coef == 1e-2 * 0.99 and up.entropy_dev.tolist() == [C.c_float(1e-2 * 0.99).value]
    assert (up.epoch_draw, up.minibatch_draw) == (0, 0) and up.state.tolist() == [0, 0]     # a refused launch draws nothing
    assert up._perm.shape == (15,) and up._perm.dtype == torch.int64


def test_capture_checks():
    adv = torch.zeros(3, 5, 1)
    for kw in (dict(noise=[torch.zeros(23)]), dict(shuffle_source="device", noise=[torch.zeros(23)]), dict(noise_source="device")):
        up, _, _ = _updater(**kw)
        with pytest.raises(ValueError, match="needs shuffle_source='device' and noise_source='device'"):
            up.capture(_cpu_storage(), adv)
    up, actor, critic = _updater(shuffle_source="device", noise_source="device")
    with pytest.raises(ValueError, match="2 agents"):
        up.capture(_cpu_storage("decoupled"), torch.zeros(3, 5, 2))
    with pytest.raises(ValueError, match="run update"):              # no update yet
        up.capture(_cpu_storage(), adv)
    with pytest.raises(RuntimeError, match="GPU only"):
        up.update(_cpu_storage(), adv)
    with pytest.raises(ValueError, match="run update"):              # ... and none that got as far as the .grad tensors
        up.capture(_cpu_storage(), adv)
    for p in list(actor.parameters()) + list(critic.parameters()):
        p.grad = torch.zeros_like(p)
    with pytest.raises(ValueError, match="T \\* N = 20 rows, the last update ran on 15"):
        up.capture(_cpu_storage(T_=4), torch.zeros(4, 5, 1))
    with pytest.raises(RuntimeError, match="GPU only"):              # every check passed
        up.capture(_cpu_storage(), adv)
    assert (up.epoch_draw, up.minibatch_draw) == (0, 0)


def test_state_dict_round_trip():
    up, _, _ = _updater(shuffle_source="device", noise_source="device", seed=11)
    assert up.state_dict() == {"seed": 11, "epoch_draw": 0, "minibatch_draw": 0, "entropy_coef": 1e-2}
    state, word = up.state, up.entropy_dev
    sd = {"seed": 2 ** 63 + 5, "epoch_draw": 2 ** 40 + 4, "minibatch_draw": 9, "entropy_coef": 1e-2 * 0.99 ** 3}
    up.load_state_dict(sd)
    assert up.state_dict() == sd and up.state is state and up.entropy_dev is word      # copied into the existing tensors
    assert state.tolist() == [2 ** 40 + 4, 9] and word.tolist() == [C.c_float(sd["entropy_coef"]).value]
    other, _, _ = _updater(shuffle_source="device", noise_source="device")
    other.load_state_dict(up.state_dict())
    assert other.state_dict() == sd and torch.equal(other.state, state) and torch.equal(other.entropy_dev, word)
    for bad in (dict(sd, seed=-1), dict(sd, epoch_draw=-1), dict(sd, minibatch_draw=2 ** 63)):
        with pytest.raises(ValueError):
            other.load_state_dict(bad)
    assert other.state_dict() == sd                                  # a refused state changes nothing
    plain, _, _ = _updater(noise=[torch.zeros(23)])                  # torch sources: the same keys, no device tensors
    plain.load_state_dict(sd)
    assert plain.state_dict() == sd and plain.state is None and plain.entropy_coef == sd["entropy_coef"]
