"""NumPy restatement of the time-limit "solved" done rule (qr_replay_add_rule; td3.ReplayBuffer.add / append with time_limit="solved"):
a literal loop over the transitions with the reference's expressions (main.py:163-173, utils/utils.py:21-39) in float64 on the float32
inputs, and the hand-made rows every test of the rule plants in its storage."""
import numpy as np

import replay_ref as R

X_LIM, POS_TOL, ROT_TOL = 1.0, 0.03, 0.03


def stored_done(obs, final_obs, reward, done, truncated, x_lim=X_LIM, pos_tol=POS_TOL, rot_tol=ROT_TOL):
    """float32 [T, N, n_agents]: the done_n the reference stores for each transition.  obs: per agent [T + 1, N, D_k]; final_obs: per agent
    [T, N, D_k] or None; reward, done [T, N, n_agents]; truncated [T, N] (set where episode_timesteps == max_steps)."""
    T, N, na = done.shape
    out = np.zeros((T, N, na), dtype=np.float32)
    for t in range(T):
        for n in range(N):
            done_n = [bool(done[t, n, k]) for k in range(na)]
            rwd_n = reward[t, n]
            if truncated[t, n]:   # episode_timesteps == max_steps; the env was re-sampled, so the returned observation is final_obs
                obs_next_n = [(obs[k][t + 1, n] if final_obs is None else final_obs[k][t, n]).astype(np.float64) for k in range(na)]
                ex = obs_next_n[0][0:3] * x_lim
                done_n[0] = True if (abs(ex) <= pos_tol).all() and rwd_n[0] != -1. else False
                if na == 2:   # MODUL
                    eb1 = obs_next_n[1][0] * np.pi
                    done_n[1] = True if abs(eb1) <= rot_tol and rwd_n[1] != -1. else False
            out[t, n] = done_n
    return out


def append(buf, count, obs, final_obs, action, reward, done, truncated, **rule):
    """replay_ref.append with the rule's done in the rows it writes.  Returns the next count."""
    nxt = R.append(buf, count, obs, final_obs, action, reward, done, truncated)
    capacity = buf[0]["obs"].shape[0]
    n = action.shape[0] * action.shape[1]
    rows = (count + np.arange(n)) % capacity
    stored = stored_done(obs, final_obs, reward, done, truncated, **rule).reshape(n, -1)
    for k, b in enumerate(buf):
        b["done"][rows] = stored[:, k]
    return nxt


# ---------------------------------------------------------------- hand-made rows
F03 = np.float32(0.03)                               # (double) 0.029999999329447746 <= 0.03
F03_UP = np.nextafter(F03, np.float32(1))            # (double) 0.030000001192092896 >  0.03
B1 = np.float32(0.03 / np.pi)                        # agent 1: the float32 nearest 0.03 / pi and its two neighbours
B1_DOWN, B1_UP = np.nextafter(B1, np.float32(0)), np.nextafter(B1, np.float32(1))

# name: (truncated, own done of both agents, ex words, eb1 word, reward of both agents, expected done of agent 0, of agent 1)
CASES = {
    "solved":            (1, 0, (0.01, -0.02, 0.0), 0.001, 0.5, 1.0, 1.0),
    "solved_crashed":    (1, 0, (0.01, -0.02, 0.0), 0.001, -1.0, 0.0, 0.0),
    "own_done_far":      (1, 1, (0.5, 0.0, 0.0), 0.5, 0.5, 0.0, 0.0),
    "own_done_no_limit": (0, 1, (0.5, 0.0, 0.0), 0.5, 0.5, 1.0, 1.0),
    "no_limit":          (0, 0, (0.0, 0.0, 0.0), 0.0, 0.5, 0.0, 0.0),
    "one_axis_out":      (1, 0, (0.01, 0.01, 0.031), 0.001, 0.5, 0.0, 1.0),
    "at_tolerance":      (1, 0, (F03, -F03, F03), B1_DOWN, 0.5, 1.0, 1.0),
    "above_tolerance":   (1, 0, (0.0, 0.0, F03_UP), B1_UP, 0.5, 0.0, 0.0),
    "below_minus":       (1, 1, (0.0, -F03_UP, 0.0), -B1_UP, 0.5, 0.0, 0.0),
    "nearest":           (1, 0, (0.0, 0.0, 0.0), B1, 0.5, 1.0, float(abs(np.float64(B1) * np.pi) <= ROT_TOL)),
}


def plant(storage, places):
    """Write the hand-made cases into a storage made by test_replay_host.fake_storage (torch tensors on any device), in place.
    places: {(t, n): case name}.  The observation words go where the transition's obs_next comes from: final_obs where the storage has
    it (every planted time-limit row has truncated set), obs[t + 1] otherwise."""
    na = storage.n_agents
    for (t, n), name in places.items():
        trunc, own, ex, eb1, rwd, _, _ = CASES[name]
        storage.truncated[t, n] = bool(trunc)
        storage.done[t, n] = bool(own)
        storage.reward[t, n] = float(rwd)
        src = [o[t + 1, n] for o in storage.obs] if storage.final_obs is None else [f[t, n] for f in storage.final_obs]
        for c in range(3):
            src[0][c] = float(ex[c])
        if na == 2:
            src[1][0] = float(eb1)


def expected(places, na):
    """{(t, n): the done the rule stores per agent} of the planted rows."""
    return {p: CASES[name][5:5 + na] for p, name in places.items()}


def places(T, N):
    """Every case in the first tile (t = 0) and in the second (t = 1, transitions 64 .. 127 for N = 65), and three in the last, partial
    tile when the horizon ends in one (the last three envs of the last step)."""
    names = list(CASES)
    out = {(0, i): nm for i, nm in enumerate(names)}
    out.update({(1, 5 + i): nm for i, nm in enumerate(names)})
    out.update({(T - 1, N - 3 + i): nm for i, nm in enumerate(("solved", "solved_crashed", "own_done_no_limit"))})
    return out
