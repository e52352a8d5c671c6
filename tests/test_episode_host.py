"""Per-episode training statistics (qr_episode_scan; episodes.episode_scan, EpisodeTracker, OffPolicyCollector(track_episodes=)) without
a GPU: the NumPy restatement of tests/episode_ref.py on the hand-made rows and against a literal transcription of the reference's
bookkeeping with its 4-decimal rounding, `EpisodeTracker.update_torch` on CPU tensors against the restatement, the new struct and
the QR_EP_* indices against the compiled header, every error code of the entry and every ValueError of the Python side."""
import ctypes as C
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import episode_ref as E  # noqa: E402

from gym_rotor_amd import _lib as L  # noqa: E402
from gym_rotor_amd.episodes import EpisodeTracker, episode_scan, episode_workspace_numel, summarize  # noqa: E402
from gym_rotor_amd.td3 import TimeLimitRule  # noqa: E402

DIMS = {1: (23,), 2: (15, 3)}   # observation widths of Coupled and Decoupled


def rows(T, N, G, seed=0, planted=True):
    """Random rows with (T >= 3, N >= 65) the hand-made ones planted."""
    reward, done, truncated, final = E.random_rows(T, N, G, seed=seed, d=DIMS[G])
    places = E.plant(reward, done, truncated, final) if planted else {}
    return (reward, done, truncated, final), places


def storage_of(rows_, device="cpu", final_obs=True):
    """What the tracker reads of a RolloutStorage."""
    reward, done, truncated, final = rows_
    T, N, G = reward.shape
    dev = torch.device(device)
    s = types.SimpleNamespace(T=T, N=N, n_agents=G, device=dev)
    s.reward, s.done, s.truncated = (torch.from_numpy(x.copy()).to(dev) for x in (reward, done, truncated))
    s.final_obs = [torch.from_numpy(f.copy()).to(dev) for f in final] if final_obs else None
    s.reset_mask = lambda: s.done.any(-1) | s.truncated
    return s


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check_against(ref, got_last, got, what=""):
    """Carries, dense rows, counts, minima, maxima and lengths bit for bit; the float64 sums within the bound of any summation order."""
    for name in ("run_return", "run_length", "ep_return", "ep_length", "ep_flags", "ep_final_error"):
        if name in got and got[name] is not None:
            assert same_bits(got[name], ref[name]), (what, name)
    for k in range(E.K):
        if k in E.SUM_FIELDS:
            assert abs(got_last[k] - ref["last"][k]) <= E.sum_bound(ref["terms"][k]), (what, k, got_last[k], ref["last"][k])
        else:
            assert got_last[k] == ref["last"][k], (what, k, got_last[k], ref["last"][k])


# ---------------------------------------------------------------- the restatement
def test_hand_made_values():
    assert float(np.float64(E.F03)) <= 0.03 < float(np.float64(E.F03_UP))
    assert abs(np.float64(E.B1_DOWN) * np.pi) <= 0.03 < abs(np.float64(E.B1_UP) * np.pi) and E.B1_UP == np.nextafter(E.B1_DOWN, np.float32(1))


@pytest.mark.parametrize("G", [1, 2])
def test_restatement_on_hand_made_rows(G):
    T, N = 3, 65
    (reward, done, truncated, final), places = rows(T, N, G, seed=1)
    r = E.scan(reward, done, truncated, np.zeros((N, G)), np.zeros(N, dtype=np.int32), final)
    for (t, n), (flags, length) in places.items():
        assert r["ep_flags"][t, n] == flags and r["ep_length"][t, n] == length, (t, n)
    assert (r["ep_length"][:, 63] == 0).all() and r["run_length"][63] == T and r["run_return"][63, 0] == 0.75   # no end: the carry holds it
    assert r["run_length"][0] == 0 and r["run_length"][64] == 0 and r["run_length"][1] == 1
    assert r["ep_return"][0, 0, 0] == 0.25 and r["ep_return"][2, 0, 0] == 0.5 and r["ep_return"][1, 64, 0] == -1.0
    assert r["ep_final_error"][2, 0, 0] == E.F03 and r["ep_final_error"][2, 64, 1] == E.F03_UP
    if G == 2:
        assert r["ep_final_error"][2, 64, 3] == np.float32(np.float64(E.B1_UP) * np.pi) and r["ep_flags"][1, 1] == 0x90
    else:
        assert (r["ep_final_error"][..., 3] == 0).all()
    m = r["ep_length"] > 0
    assert np.array_equal(m, done.any(-1) | truncated) and (r["ep_flags"][~m] == 0).all() and (r["ep_return"][~m] == 0).all()
    last = r["last"]
    assert last[E.COUNT] == m.sum() and last[E.LENGTH_SUM] == r["ep_length"].sum() and last[E.LENGTH_MAX] == r["ep_length"].max()
    assert last[E.TRUNCATED] == truncated.sum() and last[E.DONE] == (done[..., 0]).sum()
    assert last[E.RETURN_MIN] == r["ep_return"][..., 0][m].min() and last[E.RETURN_MAX] == r["ep_return"][..., 0][m].max()
    assert 0 < last[E.SOLVED] < last[E.TRUNCATED]
    # without the terminal observation: no error, nothing solved; not recorded: an empty vector, same rows
    bare = E.scan(reward, done, truncated, np.zeros((N, G)), np.zeros(N, dtype=np.int32), None)
    assert (bare["ep_final_error"] == 0).all() and (bare["ep_flags"] & 0x30 == 0).all() and bare["last"][E.SOLVED] == 0 and bare["last"][E.EX_SUM] == 0
    assert np.array_equal(bare["ep_flags"] & 0x8F, r["ep_flags"] & 0x8F) and same_bits(bare["ep_return"], r["ep_return"])
    quiet = E.scan(reward, done, truncated, np.zeros((N, G)), np.zeros(N, dtype=np.int32), final, record=False)
    assert same_bits(quiet["last"], E.empty()) and same_bits(quiet["ep_return"], r["ep_return"]) and same_bits(quiet["run_return"], r["run_return"])


@pytest.mark.parametrize("G", [1, 2])
def test_restatement_carries_over_horizons(G):
    """Two and three scans with the carries handed on equal one scan of the concatenated rows."""
    N = 65
    (reward, done, truncated, final), _ = rows(9, N, G, seed=2)
    whole = E.scan(reward, done, truncated, np.zeros((N, G)), np.zeros(N, dtype=np.int32), final)
    for cuts in ((0, 4, 9), (0, 3, 6, 9)):
        ret, length, total = np.zeros((N, G)), np.zeros(N, dtype=np.int32), E.empty()
        for a, b in zip(cuts[:-1], cuts[1:]):
            r = E.scan(reward[a:b], done[a:b], truncated[a:b], ret, length, [f[a:b] for f in final])
            ret, length, total = r["run_return"], r["run_length"], E.fold(total, r["last"])
            assert same_bits(r["ep_return"], whole["ep_return"][a:b]) and same_bits(r["ep_length"], whole["ep_length"][a:b])
        assert same_bits(ret, whole["run_return"]) and same_bits(length, whole["run_length"])
        for k in range(E.K):
            if k in E.SUM_FIELDS:
                assert abs(total[k] - whole["last"][k]) <= E.sum_bound(whole["terms"][k]), k
            else:
                assert total[k] == whole["last"][k], k
    assert (whole["ep_length"] > 4).any()   # an episode spans a boundary


@pytest.mark.parametrize("G", [1, 2])
def test_restatement_against_the_references_loop(G):
    """main.py's bookkeeping, transcribed with its per-step rounding to 4 decimals, env by env.  Each rounding moves the running sum by
    at most 0.5e-4, one per step of the episode, and the float64 additions on either side by at most length * 2^-52 * max |sum|; so
    |return - reference's| <= length * 0.5e-4 + length * 2^-52 * (length + 1).  Lengths, flags and solved bits: identical."""
    T, N = 40, 24
    (reward, done, truncated, final), _ = rows(T, N, G, seed=3, planted=False)
    r = E.scan(reward, done, truncated, np.zeros((N, G)), np.zeros(N, dtype=np.int32), final)
    seen, worst = 0, 0.0
    for n in range(N):
        log = E.reference_log(reward[:, n], done[:, n], truncated[:, n], [f[:, n] for f in final])
        ends = np.nonzero(r["ep_length"][:, n])[0]
        assert [e[0] - 1 for e in log] == ends.tolist()
        for (total_timesteps, steps, ret, flags, solved, _), t in zip(log, ends):
            assert r["ep_length"][t, n] == steps and (r["ep_flags"][t, n] & 0x8F) == flags
            assert [bool(r["ep_flags"][t, n] & (0x10 << g)) for g in range(G)] == solved
            for g in range(G):
                diff = abs(r["ep_return"][t, n, g] - ret[g])
                assert diff <= steps * 0.5e-4 + steps * 2.0 ** -52 * (steps + 1), (n, t, g, diff)
                worst = max(worst, diff)
            seen += 1
    assert seen > 3 * N and worst > 1e-6                      # the deviation is real, and bounded
    assert (r["ep_flags"] & 0x30).any() and (r["ep_length"] > 8).any()


def test_boundary_rows_against_the_references_loop():
    """The dedicated boundary rows: ex at float32(0.03) and its upper neighbour, eb1 at the float32 neighbours of 0.03 / pi."""
    T, N = 3, 65
    (reward, done, truncated, final), places = rows(T, N, 2, seed=4)
    r = E.scan(reward, done, truncated, np.zeros((N, 2)), np.zeros(N, dtype=np.int32), final)
    for n in (0, 1, 63, 64):
        log = E.reference_log(reward[:, n], done[:, n], truncated[:, n], [f[:, n] for f in final])
        assert len(log) == sum(1 for (t, m) in places if m == n)
        for total_timesteps, steps, ret, flags, solved, _ in log:
            got = int(r["ep_flags"][total_timesteps - 1, n])
            assert got & 0x8F == flags and [bool(got & 0x10), bool(got & 0x20)] == solved and got == places[(total_timesteps - 1, n)][0]


def test_warm_up_is_not_logged():
    """main.py:218: an episode is written to log_step only once total_timesteps >= start_timesteps."""
    (reward, done, truncated, final), _ = rows(40, 1, 1, seed=5, planted=False)
    log = E.reference_log(reward[:, 0], done[:, 0], truncated[:, 0], [f[:, 0] for f in final], start_log=20)
    assert [e[5] for e in log] == [e[0] >= 20 for e in log] and any(e[5] for e in log) and not all(e[5] for e in log)


# ---------------------------------------------------------------- the torch twin on CPU tensors
@pytest.mark.parametrize("G,final", [(1, True), (2, True), (2, False)])
def test_update_torch_is_the_restatement(G, final):
    T, N = 3, 65
    tr = EpisodeTracker(types.SimpleNamespace(N=N, n_agents=G, device="cpu", T=T, final_obs=[None] if final else None), dense=True)
    assert same_bits(tr.total.numpy(), E.empty(True)) and same_bits(tr.last.numpy(), E.empty())
    ret, length, total = np.zeros((N, G)), np.zeros(N, dtype=np.int32), E.empty(True)
    for call, record in enumerate((True, False, True)):
        r4, _ = rows(T, N, G, seed=10 + call)
        s = storage_of(r4, final_obs=final)
        ref = E.scan(*r4[:3], ret, length, r4[3] if final else None, record=record)
        last = tr.update_torch(s, record=record)
        got = {"run_return": tr.run_return.numpy(), "run_length": tr.run_length.numpy(), "ep_return": tr.ep_return.numpy(),
               "ep_length": tr.ep_length.numpy(), "ep_flags": tr.ep_flags.numpy(), "ep_final_error": tr.ep_final_error.numpy()}
        check_against(ref, last.numpy(), got, (G, final, call))
        ret, length = ref["run_return"], ref["run_length"]
        total[:E.K] = E.fold(total[:E.K], ref["last"])
        total[E.STEPS_SEEN] += T
        assert np.allclose(tr.total.numpy(), total, rtol=1e-14, atol=0) and tr.total[E.STEPS_SEEN] == T * (call + 1)
        if not record:
            assert same_bits(last.numpy(), E.empty())
    eps = tr.episodes()
    t, n = np.nonzero(ref["ep_length"])
    assert eps["timestep"].tolist() == (2 * T + t + 1).tolist() and eps["env"].tolist() == n.tolist()
    assert same_bits(eps["returns"].numpy(), ref["ep_return"][t, n]) and same_bits(eps["flags"].numpy(), ref["ep_flags"][t, n])
    assert tr.episodes(storage_t0=100)["timestep"][0] == eps["timestep"][0] + 100
    sm = tr.summary("last")
    assert sm["episodes"] == len(t) and sm["steps_seen"] == 3 * T and len(sm["return_mean"]) == G
    assert abs(sm["return_mean"][0] - ref["ep_return"][t, n, 0].mean()) < 1e-12 and abs(sm["return_std"][0] - ref["ep_return"][t, n, 0].std()) < 1e-9
    assert sm["length_max"] == ref["ep_length"].max() and 0 < sm["truncated_rate"] < 1
    assert tr.summary("total")["episodes"] > sm["episodes"]
    tr.reset()
    assert same_bits(tr.total.numpy(), E.empty(True)) and not tr.run_return.any() and not tr.run_length.any()
    assert tr.summary("total")["episodes"] == 0 and np.isnan(tr.summary("total")["length_mean"])


def test_summarize_of_an_empty_vector():
    s = summarize(E.empty(True), 2)
    assert s["episodes"] == 0 and s["steps_seen"] == 0 and all(np.isnan(x) for x in s["return_mean"] + s["solved_rate"])


# ---------------------------------------------------------------- the struct, the indices and the C entry's errors
def test_struct_and_indices_mirror_the_header(tmp_path):
    lines = ['printf("abi %d\\n", QR_ABI_VERSION);', 'printf("QrEpisodeScan %zu\\n", sizeof(QrEpisodeScan));']
    lines += [f'printf("QrEpisodeScan.{f} %zu\\n", offsetof(QrEpisodeScan, {f}));' for f, _ in L.QrEpisodeScan._fields_]
    lines += [f'printf("QR_EP_{name} %d\\n", (int)QR_EP_{name});' for name in L.EP_INDEX]
    lines += [f'printf("QR_EP_FLAG_{name} %d\\n", (int)QR_EP_FLAG_{name});' for name in ("DONE0", "SOLVED0", "TRUNCATED")]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "quadrotor_hip.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", f"-I{ROOT}/include", str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["QrEpisodeScan"]) == C.sizeof(L.QrEpisodeScan)
    for f, _ in L.QrEpisodeScan._fields_:
        assert int(out[f"QrEpisodeScan.{f}"]) == getattr(L.QrEpisodeScan, f).offset, f
    for name, value in L.EP_INDEX.items():
        assert int(out[f"QR_EP_{name}"]) == value, name
    header = open(os.path.join(ROOT, "include", "quadrotor_hip.h")).read()
    assert sorted(re.findall(r"#define QR_EP_(?!FLAG_)(\w+)", header)) == sorted(L.EP_INDEX)   # every index of the header is bound
    assert (int(out["QR_EP_FLAG_DONE0"]), int(out["QR_EP_FLAG_SOLVED0"]), int(out["QR_EP_FLAG_TRUNCATED"])) == \
        (L.EP_FLAG_DONE0, L.EP_FLAG_SOLVED0, L.EP_FLAG_TRUNCATED) == (E.FLAG_DONE0, E.FLAG_SOLVED0, E.FLAG_TRUNCATED)
    mine = {k: getattr(E, k) for k in ("COUNT", "RETURN_SUM", "RETURN_SQ", "RETURN_MIN", "RETURN_MAX", "LENGTH_SUM", "LENGTH_MAX", "DONE",
                                       "TRUNCATED", "SOLVED", "EX_SUM", "EB1_SUM", "STEPS_SEEN")}
    assert all(L.EP_INDEX[k] == v for k, v in mine.items()) and (E.K, E.KT) == (L.EP_FIELDS, L.EP_TOTAL_FIELDS)
    assert same_bits(np.array(L.episode_empty()), E.empty(True))
    lib = L.load()
    assert {"qr_episode_scan", "qr_episode_workspace_bytes"} <= set(L.SYMBOLS) and hasattr(lib, "qr_episode_scan")
    assert int(out["abi"]) == L.ABI_VERSION == lib.qr_abi_version()   # a struct and two entries were added: the version stays


NULL, SIZE, ALIGN = -1, -3, -4
INF, NAN = float("inf"), float("nan")


def _fake_scan(na=2, n_envs=65, final=True):
    """A QrEpisodeScan over made-up, aligned addresses that passes every check but for what a case changes: each case fails one, so
    nothing is ever launched."""
    e = L.QrEpisodeScan()
    names = ("reward", "done", "truncated", "final_obs0", "final_obs1", "run_return", "run_length", "ep_return", "ep_length", "ep_flags",
             "ep_final_error", "last", "total", "workspace")
    for i, name in enumerate(names):
        setattr(e, name, 0x100000 * (i + 1))
    if not final:
        e.final_obs0 = e.final_obs1 = e.ep_final_error = None
    e.workspace_bytes = L.load().qr_episode_workspace_bytes(n_envs)
    e.n_envs, e.n_steps, e.n_agents, e.d0, e.d1, e.record, e.reserved0 = n_envs, 3, na, 15, 3, 1, 0
    e.x_lim, e.pos_tol, e.rot_tol = 1.0, 0.03, 0.03
    return e


SCAN_CASES = [
    ("n_steps", 0, SIZE), ("n_steps", -2, SIZE), ("n_envs", -1, SIZE), ("n_agents", 0, SIZE), ("n_agents", 3, SIZE), ("reserved0", 1, SIZE),
    ("d0", 2, SIZE), ("d1", 0, SIZE), ("x_lim", 0.0, SIZE), ("x_lim", -1.0, SIZE), ("x_lim", NAN, SIZE), ("x_lim", INF, SIZE),
    ("pos_tol", -1e-9, SIZE), ("pos_tol", NAN, SIZE), ("pos_tol", INF, SIZE), ("rot_tol", -0.03, SIZE), ("rot_tol", NAN, SIZE), ("rot_tol", INF, SIZE),
    ("workspace_bytes", 2 * 18 * 8 - 1, SIZE), ("workspace_bytes", 0, SIZE),
    ("reward", None, NULL), ("done", None, NULL), ("truncated", None, NULL), ("run_return", None, NULL), ("run_length", None, NULL),
    ("last", None, NULL), ("total", None, NULL), ("workspace", None, NULL), ("final_obs1", None, NULL), ("final_obs0", None, NULL),
    ("reward", 0x100004, ALIGN), ("reward", 0x100002, ALIGN), ("final_obs0", 0x400002, ALIGN), ("final_obs1", 0x500001, ALIGN),
    ("run_return", 0x600004, ALIGN), ("run_length", 0x700002, ALIGN), ("ep_return", 0x800004, ALIGN), ("ep_length", 0x900002, ALIGN),
    ("ep_final_error", 0xB00008, ALIGN), ("last", 0xC00004, ALIGN), ("total", 0xD00004, ALIGN), ("workspace", 0xE00004, ALIGN)]


@pytest.mark.parametrize("name,value,want", SCAN_CASES)
def test_episode_scan_errors(name, value, want):
    lib = L.load()
    e = _fake_scan()
    setattr(e, name, value)
    assert lib.qr_episode_scan(C.byref(e), None) == want   # (final_obs0 NULL with ep_final_error given: NULL too)
    assert lib.qr_episode_scan(None, None) == NULL


def test_episode_scan_error_order_and_what_is_allowed():
    lib = L.load()
    e = _fake_scan()
    e.reward, e.n_steps = None, 0
    assert lib.qr_episode_scan(C.byref(e), None) == SIZE       # sizes before pointers
    e = _fake_scan()
    e.done, e.last = None, 0xC00004
    assert lib.qr_episode_scan(C.byref(e), None) == NULL       # pointers before alignment
    e = _fake_scan(na=1)                                       # one agent: agent 1's members are not read, reward needs 4 bytes only
    e.final_obs1, e.d1, e.reward = None, 0, 0x100004
    e.n_envs = 0                                               # and no env: nothing is launched
    assert lib.qr_episode_scan(C.byref(e), None) == 0
    e = _fake_scan(final=False)                                # no terminal observation: final_obs1 is not asked for
    e.pos_tol = e.rot_tol = 0.0
    e.n_envs = 0
    for name in ("ep_return", "ep_length", "ep_flags"):        # every optional output NULL
        setattr(e, name, None)
    assert lib.qr_episode_scan(C.byref(e), None) == 0
    e.d0 = 2                                                   # d0 is checked even then
    assert lib.qr_episode_scan(C.byref(e), None) == SIZE
    assert lib.qr_episode_workspace_bytes(-1) == SIZE and lib.qr_episode_workspace_bytes(0) == 18 * 8
    assert lib.qr_episode_workspace_bytes(64) == 18 * 8 and lib.qr_episode_workspace_bytes(65) == 2 * 18 * 8
    assert lib.qr_episode_workspace_bytes(64 * 257 + 1) == 258 * 18 * 8 == 8 * episode_workspace_numel(64 * 257 + 1)


# ---------------------------------------------------------------- the Python side's checks, all before a launch
def test_episode_scan_checks():
    T, N, G = 3, 65, 2
    r4, _ = rows(T, N, G, seed=6)
    s = storage_of(r4)
    f64, i32 = dict(dtype=torch.float64), dict(dtype=torch.int32)
    good = dict(reward=s.reward, done=s.done, truncated=s.truncated, run_return=torch.zeros(N, G, **f64), run_length=torch.zeros(N, **i32),
                last=torch.zeros(18, **f64), total=torch.zeros(19, **f64), final_obs=s.final_obs, ep_return=torch.zeros(T, N, G, **f64),
                ep_length=torch.zeros(T, N, **i32), ep_flags=torch.zeros(T, N, dtype=torch.uint8), ep_final_error=torch.zeros(T, N, 4),
                workspace=torch.zeros(36, **f64))
    bad = [dict(reward=s.reward.double()), dict(reward=s.reward[..., 0]), dict(reward=s.reward.transpose(0, 1)), dict(reward=torch.zeros(T, N, 3)),
           dict(reward=None), dict(done=s.done.to(torch.uint8)), dict(done=s.done[:, :64]), dict(truncated=s.truncated[:2]), dict(truncated=None),
           dict(run_return=torch.zeros(N, G)), dict(run_return=torch.zeros(N, **f64)), dict(run_length=torch.zeros(N, dtype=torch.int64)),
           dict(last=torch.zeros(19, **f64)), dict(total=torch.zeros(18, **f64)), dict(last=torch.zeros(18)), dict(final_obs=s.final_obs[:1]),
           dict(final_obs=[s.final_obs[0][..., :2], s.final_obs[1]]), dict(final_obs=[s.final_obs[0], s.final_obs[1][:2]]),
           dict(final_obs=[s.final_obs[0].double(), s.final_obs[1]]), dict(ep_return=torch.zeros(T, N, **f64)), dict(ep_length=torch.zeros(T, N)),
           dict(ep_flags=torch.zeros(T, N, dtype=torch.bool)), dict(ep_final_error=torch.zeros(T, N, 3)), dict(final_obs=None),
           dict(workspace=torch.zeros(35, **f64)), dict(workspace=torch.zeros(36)), dict(x_lim=0.0), dict(x_lim=NAN), dict(rule=TimeLimitRule(1.0, -0.1)),
           dict(rule=(1.0, 0.03, INF)), dict(rule=TimeLimitRule(-2.0))]
    for change in bad:
        with pytest.raises(ValueError):
            episode_scan(**dict(good, **change))
    for change in (dict(), dict(final_obs=None, ep_final_error=None), dict(workspace=None, ep_return=None, ep_flags=None), dict(x_lim=2.0, record=False)):
        with pytest.raises(RuntimeError):                      # all checks passed: there is no CPU kernel
            episode_scan(**dict(good, **change))
    assert not good["run_return"].any() and not good["last"].any()


def test_tracker_checks():
    with pytest.raises(ValueError):
        EpisodeTracker(types.SimpleNamespace(N=4, n_agents=3, device="cpu"))
    with pytest.raises(ValueError):
        EpisodeTracker(types.SimpleNamespace(num_envs=0, n_agents=1, device="cpu"))
    with pytest.raises(ValueError):
        EpisodeTracker(types.SimpleNamespace(num_envs=4, n_agents=1, device="cpu"), rule=TimeLimitRule(0.0))
    env = types.SimpleNamespace(num_envs=65, n_agents=2, device="cpu", x_lim=1.5)
    tr = EpisodeTracker(env, dense=True)
    assert tr.rule == TimeLimitRule(1.5, 0.03, 0.03) and tr.ep_return is None and tr.workspace.numel() == 36
    with pytest.raises(ValueError):
        tr.episodes()                                          # no update yet
    with pytest.raises(ValueError):
        tr.summary("all")
    r4, _ = rows(3, 65, 2, seed=7)
    for wrong in (storage_of(rows(3, 66, 2, planted=False)[0]), storage_of(rows(3, 65, 1, planted=False)[0])):
        with pytest.raises(ValueError):
            tr.update(wrong)
    with pytest.raises(RuntimeError):
        tr.update(storage_of(r4))                              # checks passed, dense rows made for T = 3: there is no CPU kernel
    assert tr.ep_return.shape == (3, 65, 2)
    with pytest.raises(ValueError):
        tr.update(storage_of(rows(4, 65, 2, planted=False)[0]))   # another horizon than the dense rows'
    plain = EpisodeTracker(env)
    with pytest.raises(ValueError):
        plain.episodes()
    plain.update_torch(storage_of(r4))
    assert plain.ep_return is None and plain.summary()["episodes"] > 0


def test_collector_makes_no_tracker_unless_asked():
    from test_replay_rule_host import _Env
    from gym_rotor_amd.offpolicy import OffPolicyCollector
    from gym_rotor_amd.td3 import ReplayBuffer
    env, buf = _Env(), ReplayBuffer(100, (15, 3), (4, 1), "cpu")
    col = OffPolicyCollector(env, buf, horizon=3)
    assert col.episodes is None and not any(isinstance(v, EpisodeTracker) for v in vars(col).values())
    col = OffPolicyCollector(env, buf, horizon=3, track_episodes=True)
    assert isinstance(col.episodes, EpisodeTracker) and col.episodes.rule == TimeLimitRule(1.5, 0.03, 0.03) and col.episodes.N == env.num_envs
    assert not col.episodes.dense and col.episodes.device == torch.device("cpu")
