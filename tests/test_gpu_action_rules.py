"""The two action rules of qr_rollout_actor (qr_actor.h: actor_sample) on their edges, from head outputs that are known exactly and
injected noise, against the float64 rules of tests/action_ref.py under bars derived there from the documented accuracy of each
instruction (nothing fitted to a device result; no element masked out).

The heads are controlled through the weights: mean_w = 0 (and log_std_w = 0 where there is a head), so the mean head IS mean_b and
the log-std head IS log_std_b, bit for bit — the MFMA actor adds its transpose-reduced zeros to the bias, the VALU / LDS actor runs
fmaf(0, h, bias) — while fc1 / fc2 stay random and the matrix path still runs.  One launch = one step of 133 envs (two tiles and a
ragged one) with one (log_std, pre) pair per action component; the grids (action_ref.bias_sets, eps_column) walk
  TANH_SAMPLE  log_std_b in {-25, -20, -19.999, -5, 0, 1.999, 2, 3} x pre in {0, +-0.3, +-2, +-5, +-9, +-20}            22 launches
  TANH_MEAN    log_std in {-20, -5, -1, 0, 1} x pre, for max_action in {1, 0.5, 0.05}                                   14 launches each
  TANH_MEAN with a log-std head (the host accepts the combination): log_std_b as for TANH_SAMPLE, clamped to [-20, 2]      22 launches
and every component's 133 draws are 0, +-2^-20, +-0.5, +-1, +-3, +-5.9, the three float32 numbers around each value that puts u on
tanh's last float32 steps below one (TANH_SAMPLE) or mean + sd eps on +-max_action (TANH_MEAN), and fixed normals.  Components 0..3
are the MFMA actor, component 4 (Decoupled) the VALU / LDS actor; helper-wave and plain launches; sampled and deterministic."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import action_ref as AR  # noqa: E402

pytestmark = pytest.mark.gpu
KINDS = {"coupled": 4, "decoupled": 5}


class _Rig:
    """One env of RULE_N envs with in-launch resets (so that helper_rollout picks between the helper-wave and the plain launch), fixed
    observation rows and random fc1 / fc2; `launch` runs one sampled and one deterministic step under the given biases."""

    def __init__(self, kind, helper, general):
        from gym_rotor_amd import QuadVecEnv, random_actors
        self.kind, self.A = kind, KINDS[kind]
        self.env = QuadVecEnv(kind, AR.RULE_N, device="cuda", obs_rows=True, seed=3, auto_reset=True, helper_rollout=helper)
        self.env.reset("train")
        self.env.get_norm_error_state()
        plan = self.env.launch_plan(1, "sac" if general else "ppo")
        assert plan["help"] == int(helper) and plan["policy"] == (2 if general else 1), plan
        gen = torch.Generator("cuda").manual_seed(7)
        self.base = random_actors(kind, "cuda", generator=gen)
        self.obs = [torch.randn(AR.RULE_N, a.dims[0], device="cuda", generator=gen) * 2.0 for a in self.base]

    def launch(self, rule, pre, ls, eps, max_action=1.0):
        from gym_rotor_amd import ActorParams, _lib
        actors, col = [], 0
        for b in self.base:
            n = b.dims[2]
            mb = torch.from_numpy(pre[col:col + n].copy()).cuda()
            lb = torch.from_numpy(ls[col:col + n].copy()).cuda()
            zero = torch.zeros_like(b.mean_w)
            if rule == "mean":
                actors.append(ActorParams(b.fc1_w, b.fc1_b, b.fc2_w, b.fc2_b, zero, mb, lb))
            else:
                squash = _lib.ACTOR_TANH_SAMPLE if rule == "sample" else _lib.ACTOR_TANH_MEAN
                actors.append(ActorParams(b.fc1_w, b.fc1_b, b.fc2_w, b.fc2_b, zero, mb, None, torch.zeros_like(b.mean_w), lb, squash))
            col += n
        noise = torch.from_numpy(eps).cuda()
        out = self.env.rollout_actor(actors, 1, obs=self.obs, noise=noise, max_action=max_action)
        got = [out["action"][0].clone(), out["logprob"][0].clone()]
        det = self.env.rollout_actor(actors, 1, obs=self.obs, deterministic=True, max_action=max_action)
        got += [det["action"][0].clone(), det["logprob"][0].clone()]
        torch.cuda.synchronize()
        return [g.cpu().numpy() for g in got]


class _Worst:
    """Largest error / bar ratio per assertion, with the error and the bar where it occurred."""

    def __init__(self):
        self.rows = {}

    def take(self, name, err, bar, where):
        err, bar = np.broadcast_arrays(np.asarray(err, np.float64), np.asarray(bar, np.float64))
        ratio = err / bar
        k = np.unravel_index(np.argmax(ratio), ratio.shape)
        if name not in self.rows or ratio[k] > self.rows[name][0]:
            self.rows[name] = (float(ratio[k]), float(err[k]), float(bar[k]), where, tuple(int(i) for i in k))
        bad = np.argwhere(err > bar)
        assert bad.size == 0, (name, where, len(bad), bad[:4].tolist(), err[tuple(bad[0])], bar[tuple(bad[0])])

    def report(self, label):
        for name, (ratio, err, bar, where, k) in self.rows.items():
            print(f"[action rules] {label}: {name}: worst error / bar {ratio:.3f} (error {err:.3e}, bar {bar:.3e}) at {where} element {k}")


@pytest.mark.parametrize("helper", [True, False])
@pytest.mark.parametrize("kind", list(KINDS))
def test_tanh_sample_rule_on_its_edges(kind, helper):
    """(i) a against tanh(u) under sac_action_bar; (ii) logp against sac_logp_from_action at the returned a under sac_logp_bar — tight
    at |a| = 1, which is what sees a missing 1e-6, a wrong sign, or a clamp on sd that the -log_std term does not get; (iii) never
    |a| > 1, never a non-finite log-prob; (iv) the same for the deterministic action tanh(pre) with z = 0."""
    rig, worst = _Rig(kind, helper, general=True), _Worst()
    saturated = clamped = 0
    for j, row in enumerate(AR.bias_sets(AR.SAC_LS, rig.A)):
        pre, ls, eps = AR.rule_launch("sample", row, index=j)
        a, logp, a_det, logp_det = rig.launch("sample", pre, ls, eps)
        where = f"launch {j} (log_std_b {ls.tolist()}, pre {pre.tolist()})"
        p64, l64, e64 = pre.astype(np.float64), ls.astype(np.float64), eps[0].astype(np.float64)
        want_a, _, u, lsc = AR.tanh_sample_rule(p64, l64, e64)
        assert (np.abs(a) <= 1.0).all() and (np.abs(a_det) <= 1.0).all(), where                                  # (iii)
        assert np.isfinite(logp).all() and np.isfinite(logp_det).all(), where
        worst.take("(i) action", np.abs(a - want_a), AR.sac_action_bar(p64, lsc, e64), where)
        worst.take("(ii) logp at the returned action", np.abs(logp - AR.sac_logp_from_action(lsc, e64, a)), AR.sac_logp_bar(lsc, e64, a), where)
        worst.take("(iv) deterministic action", np.abs(a_det - np.tanh(p64)), AR.sac_action_bar(p64, lsc, None), where)
        worst.take("(iv) deterministic logp", np.abs(logp_det - AR.sac_logp_from_action(lsc, None, a_det)), AR.sac_logp_bar(lsc, None, a_det), where)
        saturated += int((np.abs(a) == 1.0).sum())
        clamped += int(((l64 < -20.0) | (l64 > 2.0)).sum())
    assert saturated > 100 and clamped > 0            # the grid reached |a| = 1 and log_std beyond both clamps
    worst.report(f"TANH_SAMPLE {kind}, helper {helper}")
    print(f"[action rules] TANH_SAMPLE {kind}, helper {helper}: {saturated} actions of exactly +-1")


MEAN_CASES = [("mean", m) for m in AR.MAX_ACTIONS] + [("mean_head", 0.5)]


@pytest.mark.parametrize("helper", [True, False])
@pytest.mark.parametrize("rule,max_action", MEAN_CASES)
@pytest.mark.parametrize("kind", list(KINDS))
def test_tanh_mean_rule_on_its_edges(kind, rule, max_action, helper):
    """The action against clip(mean + sd eps, +-max_action) under mean_action_bar, exactly +-max_action wherever float64 is outside
    by more than that bar, never beyond it; logp against the Normal log-prob of the RETURNED (clamped) action about the float64 mean
    under mean_logp_bar — asserted in relative form where the bar exceeds 1e-2 (the same inequality divided by the value: at
    log_std = -20 the value is ~1e16 and the bar ~1e-5 of it); the deterministic action clip(tanh(pre)) and its log-prob."""
    head = rule == "mean_head"
    rig, worst = _Rig(kind, helper, general=head), _Worst()
    ma = float(np.float32(max_action))
    at_clamp = inside = 0
    rel_err = rel_bar = 0.0
    for j, row in enumerate(AR.bias_sets(AR.SAC_LS if head else AR.MEAN_LS, rig.A)):
        pre, ls, eps = AR.rule_launch(rule, row, max_action, index=j)
        a, logp, a_det, logp_det = rig.launch(rule, pre, ls, eps, max_action)
        where = f"launch {j} (log_std {ls.tolist()}, pre {pre.tolist()})"
        p64, l64, e64 = pre.astype(np.float64), ls.astype(np.float64), eps[0].astype(np.float64)
        lsc = np.clip(l64, AR.LOG_STD_MIN, AR.LOG_STD_MAX) if head else l64
        want_a, _, mean = AR.tanh_mean_rule(p64, l64, e64, ma, clamp_log_std=head)
        assert (np.abs(a) <= np.float32(ma)).all() and (np.abs(a_det) <= np.float32(ma)).all(), where
        assert np.isfinite(logp).all() and np.isfinite(logp_det).all(), where
        bar_a = AR.mean_action_bar(p64, lsc, e64)
        worst.take("action", np.abs(a - want_a), bar_a, where)
        raw = mean + np.exp(lsc) * e64
        assert (a[raw > ma + bar_a] == np.float32(ma)).all() and (a[raw < -ma - bar_a] == np.float32(-ma)).all(), where
        at_clamp += int((np.abs(a) == np.float32(ma)).sum()); inside += int((np.abs(a) < np.float32(ma)).sum())
        lsb = np.broadcast_to(lsc, a.shape)
        for name, aa, lp in (("logp at the returned action", a, logp), ("deterministic logp", a_det, logp_det)):
            want = AR.normal_logp_from_action(mean, lsb, aa)
            bar, err = AR.mean_logp_bar(p64, lsb, aa), np.abs(lp - want)
            big = bar > 1e-2
            scale = np.where(big, np.abs(want), 1.0)
            assert (scale > 0).all(), where
            worst.take(name, err / scale, bar / scale, where)
            far = big & (np.abs(aa - mean) >= 0.01)             # the clamp holds the action away from the mean: the bar is small beside the value
            if far.any():
                rel_err, rel_bar = max(rel_err, float((err / scale)[far].max())), max(rel_bar, float((bar / scale)[far].max()))
        worst.take("deterministic action", np.abs(a_det - np.clip(mean, -ma, ma)), AR.mean_action_bar(p64, lsc, None), where)
    assert at_clamp > 100 and inside > 100
    label = f"TANH_MEAN{' with a log-std head' if head else ''} {kind}, max_action {max_action}, helper {helper}"
    worst.report(label)
    print(f"[action rules] {label}: {at_clamp} actions at the clamp; where the bar exceeds 1e-2 and |a - mean| >= 0.01: "
          f"worst relative error {rel_err:.3e}, largest relative bar {rel_bar:.3e}")
    assert rel_bar <= 1e-4                            # (there the relative form has teeth: 2 (2e-7 / 0.01 + exp_rel(20)) = 9e-5)
