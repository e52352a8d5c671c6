// qr_replay_walk.h — the body of replay_add_kernel and replay_add_rule_kernel: included by qr_replay.h INSIDE each of the two kernels
// (no include guard), which define `a` (ReplayAddArgs), `rule` (ReplayRule) and `kRule` (constexpr bool) before it.
  const int k = (int)blockIdx.y >= kReplaySegments;
  const int seg = (int)blockIdx.y - kReplaySegments * k;
  const int64_t count = a.state ? a.state[0] : a.count;
  if (count < 0 || count >= a.capacity) return;   // (device counters that do not describe this buffer: write nothing)
  const int na = a.n_agents;
  const bool act = seg == 2, scalar = seg >= 3;
  const uint32_t w = scalar ? 1u : (uint32_t)(act ? (k ? a.A1 : a.A0) : (k ? a.D1 : a.D0));
  const uint32_t magic = act ? (k ? a.mA1 : a.mA0) : (k ? a.mD1 : a.mD0);
  const float* obs = k ? a.obs1 : a.obs0;
  const float* fin = k ? a.final1 : a.final0;
  const int64_t next = k ? a.next1 : a.next0;
  const int col = k ? a.col1 : a.col0;
  float* dst = seg == 0 ? (k ? a.b_obs1 : a.b_obs0) : seg == 1 ? (k ? a.b_next1 : a.b_next0) : seg == 2 ? (k ? a.b_act1 : a.b_act0)
             : seg == 3 ? (k ? a.b_rwd1 : a.b_rwd0) : (k ? a.b_done1 : a.b_done0);
  const int64_t tiles = (a.rows + kReplayTile - 1) / kReplayTile;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t j0 = tile * kReplayTile;
    const int64_t left = a.rows - j0;
    const uint32_t elems = (uint32_t)(left < kReplayTile ? left : kReplayTile) * w;
    for (uint32_t l = threadIdx.x; l < elems; l += 256) {
      const uint32_t jl = w == 1 ? l : __umulhi(l, magic);
      const uint32_t c = l - jl * w;
      const int64_t j = j0 + jl;
      int64_t row = count + j;
      row = row >= a.capacity ? row - a.capacity : row;
      const int64_t e = j0 * (int64_t)w + l;   // = j * w + c
      float v;
      if (seg == 0) {
        v = obs[e];
      } else if (seg == 1) {
        bool reset = false;
        if (fin) {
          reset = a.done[j * na] != 0;
          if (na > 1) reset = reset | (a.done[j * na + 1] != 0);
          if (a.truncated) reset = reset | (a.truncated[j] != 0);
        }
        v = reset ? fin[e] : obs[next + e];
      } else if (seg == 2) {
        v = a.action[j * a.action_row + col + c];
      } else if (seg == 3) {
        v = a.reward[j * na + k];
      } else {
        v = a.done[j * na + k] != 0 ? 1.0f : 0.0f;
        if constexpr (kRule) {
          if (a.truncated[j] != 0) {   // (so obs_next of this row is final_obs wherever final_obs is given)
            const int64_t D = k ? a.D1 : a.D0;
            const float* src = fin ? fin + j * D : obs + next + j * D;
            bool solved;
            if (k == 0) {
              solved = fabs((double)src[0] * rule.x_lim) <= rule.pos_tol;
              solved = solved & (fabs((double)src[1] * rule.x_lim) <= rule.pos_tol);
              solved = solved & (fabs((double)src[2] * rule.x_lim) <= rule.pos_tol);
            } else {
              solved = fabs((double)src[0] * kReplayPi) <= rule.rot_tol;
            }
            v = (solved & (a.reward[j * na + k] != -1.0f)) ? 1.0f : 0.0f;
          }
        }
      }
      dst[row * (int64_t)w + c] = v;
    }
  }
