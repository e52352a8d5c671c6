"""NumPy restatement of qr_episode_scan (include/quadrotor_hip.h): a plain per-env loop in float64 over the rows of one horizon that
returns the carries, the dense rows and the K statistics fields — and, beside it, a literal transcription of the reference's
bookkeeping (main.py:132-137, 169-173, 180, 212-235), 4-decimal rounding of the running return included, and the hand-made rows the
host and the GPU tests plant."""
import numpy as np

# the QR_EP_* indices, written out (tests/test_episode_host.py holds them against the header)
COUNT, RETURN_SUM, RETURN_SQ, RETURN_MIN, RETURN_MAX, LENGTH_SUM, LENGTH_MAX, DONE, TRUNCATED, SOLVED, EX_SUM, EB1_SUM = 0, 1, 3, 5, 7, 9, 10, 11, 13, 14, 16, 17
K, STEPS_SEEN, KT = 18, 18, 19
FLAG_DONE0, FLAG_SOLVED0, FLAG_TRUNCATED = 0x01, 0x10, 0x80
MIN_FIELDS, MAX_FIELDS = (5, 6), (7, 8, 10)


def empty(total=False):
    v = np.zeros(KT if total else K)
    v[[5, 6]], v[[7, 8]] = np.inf, -np.inf
    return v


def fold(a, b):
    """`total` (or `last`) a with the statistics b folded in: sums and counts add, minima and maxima fold."""
    out = np.array(a, dtype=np.float64)
    for k in range(K):
        out[k] = min(a[k], b[k]) if k in MIN_FIELDS else max(a[k], b[k]) if k in MAX_FIELDS else a[k] + b[k]
    return out


def scan(reward, done, truncated, run_return, run_length, final_obs=None, x_lim=1.0, pos_tol=0.03, rot_tol=0.03, record=True):
    """reward [T, N, G] float32, done [T, N, G] bool, truncated [T, N] bool, the carries run_return [N, G] float64 and run_length [N]
    int32 (not modified), final_obs None or a list of [T, N, D_k] float32.  Returns a dict: run_return, run_length (the new carries),
    ep_return, ep_length, ep_flags, ep_final_error (dense), last [K] (sums taken env by env, t by t), terms (per summed field the
    list of its terms, for the error bound of another summation order)."""
    T, N, G = reward.shape
    ret, length = np.array(run_return, dtype=np.float64), np.array(run_length, dtype=np.int32)
    ep_return, ep_length = np.zeros((T, N, G)), np.zeros((T, N), dtype=np.int32)
    ep_flags, ep_err = np.zeros((T, N), dtype=np.uint8), np.zeros((T, N, 4), dtype=np.float32)
    last = empty()
    terms = {k: [] for k in (RETURN_SUM, RETURN_SUM + 1, RETURN_SQ, RETURN_SQ + 1, EX_SUM, EB1_SUM)}
    for n in range(N):
        for t in range(T):
            for g in range(G):
                ret[n, g] += np.float64(reward[t, n, g])
            length[n] += 1
            limit = bool(truncated[t, n])
            if not (limit or done[t, n].any()):
                continue
            ex, eb1, solved = np.zeros(3), 0.0, [False, False]
            if final_obs is not None:
                ex = final_obs[0][t, n, :3].astype(np.float64) * np.float64(x_lim)
                solved[0] = bool((np.abs(ex) <= pos_tol).all()) and reward[t, n, 0] != np.float32(-1.0)
                if G == 2:
                    eb1 = float(np.float64(final_obs[1][t, n, 0]) * np.pi)
                    solved[1] = abs(eb1) <= rot_tol and reward[t, n, 1] != np.float32(-1.0)
            flags = FLAG_TRUNCATED if limit else 0
            for g in range(G):
                flags |= (FLAG_DONE0 << g) if done[t, n, g] else 0
                flags |= (FLAG_SOLVED0 << g) if limit and solved[g] else 0
            ep_return[t, n], ep_length[t, n], ep_flags[t, n] = ret[n], length[n], flags
            ep_err[t, n, :3], ep_err[t, n, 3] = ex.astype(np.float32), np.float32(eb1)
            if record:
                last[COUNT] += 1
                for g in range(G):
                    last[RETURN_SUM + g] += ret[n, g]
                    last[RETURN_SQ + g] += ret[n, g] * ret[n, g]
                    last[RETURN_MIN + g], last[RETURN_MAX + g] = min(last[RETURN_MIN + g], ret[n, g]), max(last[RETURN_MAX + g], ret[n, g])
                    last[DONE + g] += bool(done[t, n, g])
                    last[SOLVED + g] += bool(limit and solved[g])
                    terms[RETURN_SUM + g].append(ret[n, g])
                    terms[RETURN_SQ + g].append(ret[n, g] * ret[n, g])
                last[LENGTH_SUM] += length[n]
                last[LENGTH_MAX] = max(last[LENGTH_MAX], length[n])
                last[TRUNCATED] += limit
                last[EX_SUM] += np.abs(ex).max()
                last[EB1_SUM] += abs(eb1)
                terms[EX_SUM].append(np.abs(ex).max())
                terms[EB1_SUM].append(abs(eb1))
            ret[n], length[n] = 0.0, 0
    return {"run_return": ret, "run_length": length, "ep_return": ep_return, "ep_length": ep_length, "ep_flags": ep_flags,
            "ep_final_error": ep_err, "last": last, "terms": terms}


SUM_FIELDS = (RETURN_SUM, RETURN_SUM + 1, RETURN_SQ, RETURN_SQ + 1, EX_SUM, EB1_SUM)


def sum_bound(terms):
    """The bound on the difference between two float64 sums of the same n terms taken in any two orders: each is within
    (n - 1) * 2^-53 * sum |x| of the exact sum to first order, so the test allows that much against the restatement's own sum."""
    x = np.abs(np.asarray(terms, dtype=np.float64))
    return max(len(x) - 1, 0) * 2.0 ** -53 * float(x.sum())


def reference_log(reward, done, truncated, final_obs, x_lim=1.0, start_log=0, t_base=0):
    """main.py:132-137, 169-173, 180, 212-235 for ONE env, transcribed: rows reward [T, G], done [T, G], truncated [T] (the loop's
    `episode_timesteps == self.max_steps`), final_obs the list of [T, D_k] obs_next rows.  Returns the printed episodes as tuples
    (total_timesteps, episode_timesteps, episode_reward list, ended_by flags, solved list) — the running reward rounded to 4
    decimals at every step as the reference does."""
    T, G = reward.shape
    episode_reward, episode_timesteps, out = [0.0] * G, 0, []
    for t in range(T):
        total_timesteps = t_base + t + 1
        episode_timesteps += 1
        rwd_n, done_n, done_episode = [float(r) for r in reward[t]], [bool(d) for d in done[t]], False
        own = list(done_n)
        ex = final_obs[0][t, :3].astype(np.float64) * x_lim
        eb1 = float(np.float64(final_obs[1][t, 0]) * np.pi) if G == 2 else 0.0
        solved = [False] * G
        if truncated[t]:
            done_episode = True
            done_n[0] = True if (abs(ex) <= 0.03).all() and rwd_n[0] != -1. else False
            if G == 2:
                done_n[1] = True if abs(eb1) <= 0.03 and rwd_n[1] != -1. else False
            solved = list(done_n)
        episode_reward = [float('{:.4f}'.format(episode_reward[agent_id] + r)) for agent_id, r in zip(range(G), rwd_n)]
        if any(own) or done_episode:   # (the reference tests the overwritten done_n: with done_episode set that is the same condition)
            flags = sum(FLAG_DONE0 << g for g in range(G) if own[g]) | (FLAG_TRUNCATED if truncated[t] else 0)
            out.append((total_timesteps, episode_timesteps, episode_reward, flags, solved, total_timesteps >= start_log))
            episode_reward, episode_timesteps = [0.0] * G, 0
    return out


# ---- the hand-made rows (T >= 3; envs 0, 63 and 64 of N = 65) -----------------------------------------------------------------------------
F03 = np.float32(0.03)                                   # as a double slightly below 0.03: inside the tolerance
F03_UP = np.nextafter(F03, np.float32(1.0))              # its upper neighbour: outside
B1 = np.float32(0.03 / np.pi)
B1_DOWN = B1 if np.float64(B1) * np.pi <= 0.03 else np.nextafter(B1, np.float32(0.0))    # the float32 neighbours of 0.03 / pi
B1_UP = np.nextafter(B1_DOWN, np.float32(1.0))


def plant(reward, done, truncated, final_obs):
    """Write the hand-made rows into a horizon with T >= 3 and N >= 65, in place; G = reward.shape[-1].  Returns {(t, n): (flags, length
    as counted from a zero carry)} of the planted episode ends.
      env 0:  ends at t = 0 by agent 0's done; ends again at t = T - 1 by truncated with ex = float32(0.03) (solved) and, two agents,
              eb1 at the lower neighbour (solved): two episodes of one env inside the horizon, the first at t = 0, the last at T - 1
      env 63: no episode end
      env 64: t = 0 ends by the LAST agent's done only; t = 1 by truncated only with reward -1 (not solved) and ex inside;
              t = 2 by both truncated and agent 0's done, ex at the upper neighbour (not solved), eb1 at the upper neighbour (not solved)
      env 1:  truncated at t = 1, ex inside, eb1 = B1_UP: agent 0 solved, agent 1 not"""
    T, N, G = reward.shape
    last = G - 1
    for n in (0, 1, 63, 64):
        done[:, n], truncated[:, n] = False, False
        reward[:, n] = np.float32(0.25)
        for f in final_obs:
            f[:, n] = np.float32(0.5)
    inside = np.array([F03, -F03, 0.0], dtype=np.float32)
    out = {}
    done[0, 0, 0] = True
    out[(0, 0)] = (FLAG_DONE0, 1)
    truncated[T - 1, 0] = True
    final_obs[0][T - 1, 0, :3] = inside
    flags = FLAG_TRUNCATED | FLAG_SOLVED0
    if G == 2:
        final_obs[1][T - 1, 0, 0] = -B1_DOWN
        flags |= FLAG_SOLVED0 << 1
    out[(T - 1, 0)] = (flags, T - 1)
    done[0, 64, last] = True
    out[(0, 64)] = (FLAG_DONE0 << last, 1)
    truncated[1, 64] = True
    reward[1, 64] = np.float32(-1.0)
    final_obs[0][1, 64, :3] = inside
    if G == 2:
        final_obs[1][1, 64, 0] = np.float32(0.0)
    out[(1, 64)] = (FLAG_TRUNCATED, 1)
    truncated[2, 64], done[2, 64, 0] = True, True
    final_obs[0][2, 64, :3] = np.array([0.0, F03_UP, 0.0], dtype=np.float32)
    if G == 2:
        final_obs[1][2, 64, 0] = B1_UP
    out[(2, 64)] = (FLAG_TRUNCATED | FLAG_DONE0, 1)
    truncated[1, 1] = True
    final_obs[0][1, 1, :3] = inside
    if G == 2:
        final_obs[1][1, 1, 0] = B1_UP
    out[(1, 1)] = (FLAG_TRUNCATED | FLAG_SOLVED0, 2)
    return out


def random_rows(T, N, G, seed=0, d=(15, 4), p_done=0.08, p_trunc=0.1):
    """A horizon of random rows: rewards in (-1, 1) with some exact -1 rows, ends at a rate that gives several episodes per env, terminal
    observations scaled so that time-limit rows fall on both sides of the tolerances without sitting on them."""
    rng = np.random.default_rng(seed)
    reward = rng.uniform(-1, 1, (T, N, G)).astype(np.float32)
    reward[rng.random((T, N, G)) < 0.1] = np.float32(-1.0)
    done = rng.random((T, N, G)) < p_done
    truncated = rng.random((T, N)) < p_trunc
    final_obs = [rng.uniform(-1, 1, (T, N, d[k])).astype(np.float32) for k in range(G)]
    near = rng.random((T, N)) < 0.5
    final_obs[0][near, :3] *= np.float32(0.02)
    if G == 2:
        final_obs[1][near, 0] *= np.float32(0.005)
    return reward, done, truncated, final_obs
