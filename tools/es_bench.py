#!/usr/bin/env python
"""What one evolution-strategy generation costs: two arms alternated call by call in one process,
    (a) what a user writes without the ES entries: `ActorPopulation.perturb` with torch's generator (it returns eps, a second copy of
        the population), the common episodes tiled as `evaluate.evaluate_population` tiles them, `env.evaluate_population`, the
        per-policy mean, centered ranks from two argsorts, one weighted sum per tensor into .grad, `DeviceAdamW.step_all`,
    (b) `EvolutionStrategy.step()`,
at Coupled, P = 1024 policies x E = 64 episodes x 1000 steps.

    python tools/es_bench.py [--population 1024] [--episodes 64] [--max-steps 1000] [--reps 20] [--json PATH]

HIP events around one generation, median of --reps with min .. max.  Both arms share the evaluation launch, so each is also
reported without it: a second event pair around the `evaluate_population` call of either env (set on the env objects here, the
library is untouched) gives that launch's own time, which is subtracted repetition by repetition.  Condition, printed with its numbers:
(b)'s median lies below (a)'s minimum, on the whole generation and on the part outside the evaluation."""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


class Actor(torch.nn.Module):
    def __init__(self, d, h, a):
        super().__init__()
        self.fc1, self.fc2, self.mean_linear = torch.nn.Linear(d, h), torch.nn.Linear(h, h), torch.nn.Linear(h, a)
        self.log_std = torch.nn.Parameter(torch.zeros(1, a))


def weights(m):
    return [m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, m.mean_linear.weight, m.mean_linear.bias]


def timed_evaluation(env, log):
    """Wrap env.evaluate_population in an event pair; every call appends its pair to `log`."""
    inner = env.evaluate_population

    def evaluate_population(*args, **kw):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = inner(*args, **kw)
        b.record()
        log.append((a, b))
        return out
    env.evaluate_population = evaluate_population


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--population", type=int, default=1024)
    ap.add_argument("--episodes", type=int, default=64)
    ap.add_argument("--max-steps", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("es_bench.py measures on the GPU; there is none")
    from gym_rotor_amd import ActorParams, ActorPopulation, DeviceAdamW, EvolutionStrategy, QuadVecEnv
    from gym_rotor_amd.evaluate import _prepare_episodes, _tile_episodes
    from gym_rotor_amd.policy import population_layout, population_view
    kind, P, E, T, sigma, seed = "coupled", args.population, args.episodes, args.max_steps, 0.05, 1992
    torch.manual_seed(0)
    module_b = Actor(23, 16, 4).cuda()
    module_a = copy.deepcopy(module_b)
    names = ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "mean_w", "mean_b")

    # arm (b)
    strategy = EvolutionStrategy(kind, [module_b], population=P, episodes_per_policy=E, sigma=sigma, seed=seed, max_steps=T)
    log_b = []
    timed_evaluation(strategy.env, log_b)

    # arm (a)
    src, src_obs = _prepare_episodes(kind, E, 0, seed, device="cuda")
    env = QuadVecEnv(kind, population_layout(P, E)[1], seed=seed, goal_mode=0, autotune=False, device="cuda")
    log_a = []
    timed_evaluation(env, log_a)
    gen = torch.Generator("cuda").manual_seed(seed)
    opt = DeviceAdamW(weights(module_a), lr=1e-2, weight_decay=0.0)
    for p in weights(module_a):
        p.grad = torch.zeros_like(p)

    def arm_a():
        base = [ActorParams.from_module(module_a)]
        pop, eps = ActorPopulation.perturb(base, P, sigma, generator=gen)
        obs = _tile_episodes(src, src_obs, env, P)
        out = env.evaluate_population(pop, E, max_steps=T, obs=obs)
        fit = population_view(out["benchmark"], P, E).mean(1)
        ranks = fit.argsort().argsort()
        u = (ranks.double() / (P - 1) - 0.5).float()
        for n, p in zip(names, weights(module_a)):
            p.grad.copy_(torch.tensordot(u, eps[0][n], dims=1) / (-(P * sigma)))
        DeviceAdamW.step_all([opt])

    arms = (arm_a, strategy.step)
    for _ in range(3):
        for f in arms:
            f()
    torch.cuda.synchronize()
    log_a.clear(), log_b.clear()
    whole = ([], [])
    for _ in range(args.reps):
        for m, f in zip(whole, arms):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            m.append(a.elapsed_time(b))
    evals = [[a.elapsed_time(b) for a, b in log] for log in (log_a, log_b)]
    rest = [[w - e for w, e in zip(ws, es)] for ws, es in zip(whole, evals)]
    stat = lambda m: (statistics.median(m), min(m), max(m))
    fmt = lambda t: f"{t[0]:.4f} ms ({t[1]:.4f} .. {t[2]:.4f})"
    wa, wb, ea, eb, ra, rb = stat(whole[0]), stat(whole[1]), stat(evals[0]), stat(evals[1]), stat(rest[0]), stat(rest[1])
    ok_whole, ok_rest = wb[0] < wa[1], rb[0] < ra[1]
    print(f"{kind} P = {P} E = {E} max_steps = {T}, {args.reps} repetitions, arms alternated ({torch.cuda.get_device_name(0)}):\n"
          f"  (a) perturb + tile + evaluate_population + torch ranks and sums + DeviceAdamW    {fmt(wa)}\n"
          f"  (b) EvolutionStrategy.step()                                                     {fmt(wb)}\n"
          f"  the evaluation launch inside (a) {fmt(ea)}, inside (b) {fmt(eb)}\n"
          f"  (a) without the evaluation launch                                                {fmt(ra)}\n"
          f"  (b) without the evaluation launch                                                {fmt(rb)}\n"
          f"  median of (b) below (a)'s minimum: whole generation {ok_whole} (a / b {wa[0] / wb[0]:.2f}), outside the evaluation {ok_rest} "
          f"(a / b {ra[0] / rb[0]:.2f})", flush=True)
    # the two entries alone, Coupled's six tensors: ten calls back to back per sample (a call is tens of µs), median of --reps samples.
    # The utility kernel's float64 pass over the fitness is serial on one lane — twice, and in every workgroup, under "standardize".
    from gym_rotor_amd import es as ES
    base = [ActorParams.from_module(module_b)]
    flat_grads = [torch.empty_like(p) for p in weights(module_b)]
    streams = [ES.es_stream(0, n) for n in names]
    parts = {}
    for n_pol in (P, ES.MAX_POLICIES):
        pop = ES.population_like(base, n_pol)
        fit = torch.randn(n_pol, device="cuda")
        stats, ws = torch.empty(4, dtype=torch.float64, device="cuda"), torch.empty(ES.es_workspace_numel(n_pol), dtype=torch.float64, device="cuda")
        calls = {"es_perturb": lambda: ES.es_perturb(base, pop, sigma=sigma, seed=seed, generation=1)}
        for shaping in ES.SHAPINGS:
            calls[f"es_gradient {shaping}"] = lambda shaping=shaping: ES.es_gradient(fit, flat_grads, sigma=sigma, seed=seed, generation=1, streams=streams,
                                                                                    shaping=shaping, stats=stats, workspace=ws)
        for label, f in calls.items():
            f()
            torch.cuda.synchronize()
            samples = []
            for _ in range(args.reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(10):
                    f()
                b.record()
                b.synchronize()
                samples.append(a.elapsed_time(b) * 100.0)   # µs per call
            parts[f"{label} P={n_pol}"] = stat(samples)
            t = parts[f"{label} P={n_pol}"]
            print(f"  {label:28s} P = {n_pol:5d}: {t[0]:.1f} us per call ({t[1]:.1f} .. {t[2]:.1f}), ten calls back to back", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "kind": kind, "P": P, "E": E, "max_steps": T, "reps": args.reps,
                       "torch_ms": wa, "es_ms": wb, "torch_eval_ms": ea, "es_eval_ms": eb, "torch_rest_ms": ra, "es_rest_ms": rb,
                       "below_torch_min": bool(ok_whole), "rest_below_torch_min": bool(ok_rest), "entries_us": parts}, f, indent=1)


if __name__ == "__main__":
    main()
