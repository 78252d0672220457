// gmz_replay.hip — finished self-play games from the device history (worker.GameHistory) straight into the trainer's
// device replay ring (trainer.ReplayBuffer), one launch per self-play move.
//
// Bit-exact restatement of records.final_rewards + records.compute_n_step_returns + loop.slices_from_game (built
// with -ffp-contract=off): the ring holds what the host path would have uploaded, bit for bit.
//   rewards        d = n-1-t: +1 when d mod 4 is 0 or 3, -1 otherwise (r[n-1] = 1, r[n-2] = -1, r[i] = -r[i+2]);
//                  all zero for a draw; 0 past the game.
//   value targets  s = 0.0; s = s + pw[i] * r[t+i] in f64, in order, i < n_steps and t+i < n;
//                  out = (float)s + v32[t+n_steps] * (float)pw[n_steps] (both f32) when t+n_steps < n, else (float)s
//                  (numpy 2: python-float * float32 and python-float + float32 are float32 operations).
//                  pw[i] = discount**i comes from the host by value: the device never calls pow.
//   planes         u8: own stones, opponent stones, the last move when it is >= 0; zero past the game.
//   policies       f64 -> f32, round to nearest; zero past the game.
//   actions        -1 past the game.
// One workgroup per kept slice; the slice's game is found by a binary search over the job table's prefix.
#include "gmz_common.h"

#include <algorithm>
#include <vector>

namespace gmz {

struct ReplayJob {  // include/gmz.h's job record; worker.py builds it as 8 int32
  int32_t game, bank, row0, n, winner, drop, slot, first;
};
static_assert(sizeof(ReplayJob) == 32, "job record layout");

struct ReplayPow {
  double pw[GMZ_REPLAY_MAX_N_STEPS + 1];
};

struct ReplayArgs {
  const int8_t *board;
  const int8_t *player;
  const int32_t *last;
  const double *pol;
  const float *val;
  const int32_t *act;
  uint8_t *r_obs;
  int32_t *r_act;
  float *r_rew;
  float *r_pol;
  float *r_val;
  float *r_prio;
  const ReplayJob *jobs;
  const float *prio;
  int A, U, n_steps, G, L, N, n_jobs;
};

__device__ __forceinline__ float final_reward(int n, int winner, int t) {
  if (winner == 0 || t >= n) return 0.0f;
  const int d = (n - 1 - t) & 3;
  return (d == 0 || d == 3) ? 1.0f : -1.0f;
}

__global__ __launch_bounds__(256) void k_replay_ingest(const ReplayArgs a, const ReplayPow P) {
  const int b = (int)blockIdx.x;
  // last job whose first kept slice is <= b
  int lo = 0, hi = a.n_jobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.jobs[mid].first <= b) lo = mid; else hi = mid - 1;
  }
  const ReplayJob j = a.jobs[lo];
  const int kk = b - j.first;
  // the host validated the table it was given; a device copy that differs from it writes nothing
  if (j.game < 0 || j.game >= a.G || (j.bank != 0 && j.bank != 1) || j.row0 < 0 || j.n < 1 ||
      (long)j.row0 + j.n > a.L || j.drop < 0 || j.drop >= j.n || j.slot < 0 || j.slot >= a.N || kk < 0 ||
      kk >= j.n - j.drop || j.n - j.drop > a.N)
    return;
  const int t0 = j.drop + kk, n = j.n, A = a.A, U = a.U;
  const size_t ring = (size_t)((j.slot + (long)kk) % a.N);
  const size_t hrow = ((size_t)j.bank * a.G + j.game) * a.L + j.row0;  // history row of the game's first move
  const int tid = (int)threadIdx.x, nt = (int)blockDim.x;

  for (int u = tid; u <= U; u += nt) {
    const int t = t0 + u;
    float v = 0.0f;
    if (t < n) {
      double s = 0.0;
      for (int i = 0; i < a.n_steps && t + i < n; ++i) s = s + P.pw[i] * (double)final_reward(n, j.winner, t + i);
      v = (float)s;
      if (t + a.n_steps < n) v = v + a.val[hrow + t + a.n_steps] * (float)P.pw[a.n_steps];
    }
    a.r_val[ring * (U + 1) + u] = v;
    if (u < U) {
      a.r_rew[ring * U + u] = final_reward(n, j.winner, t);
      a.r_act[ring * U + u] = t < n ? a.act[hrow + t] : -1;
    }
  }
  if (tid == 0) a.r_prio[ring] = a.prio ? *a.prio : 1.0f;

  uint8_t *obs = a.r_obs + ring * (size_t)(U + 1) * 3 * A;
  float *pol = a.r_pol + ring * (size_t)(U + 1) * A;
  for (int idx = tid; idx < (U + 1) * A; idx += nt) {
    const int u = idx / A, c = idx - u * A, t = t0 + u;
    uint8_t own = 0, opp = 0, lastp = 0;
    float p = 0.0f;
    if (t < n) {
      const int8_t st = a.board[(hrow + t) * A + c], pl = a.player[hrow + t];
      own = st == pl;
      opp = (int)st == -(int)pl;
      lastp = a.last[hrow + t] == c;  // c >= 0: a last move of -1 (none) sets nothing
      p = (float)a.pol[(hrow + t) * A + c];
    }
    uint8_t *o = obs + (size_t)u * 3 * A + c;
    o[0] = own;
    o[A] = opp;
    o[2 * A] = lastp;
    pol[idx] = p;
  }
}

}  // namespace gmz

using namespace gmz;

GMZ_EXPORT int gmz_replay_ingest(int board_size, int unroll, int n_steps, int G, int L, const int8_t *hist_board_dev,
                                 const int8_t *hist_player_dev, const int32_t *hist_last_dev,
                                 const double *hist_policy_dev, const float *hist_value_dev,
                                 const int32_t *hist_action_dev, uint8_t *ring_obs_dev, int32_t *ring_act_dev,
                                 float *ring_rew_dev, float *ring_pol_dev, float *ring_val_dev, float *ring_prio_dev,
                                 int N, const void *jobs_host, int n_jobs, const void *jobs_dev, size_t jobs_dev_bytes,
                                 const double *discount_pow, const float *priority_dev, void *stream) {
  if (board_size < 5 || board_size > 22)
    return fail("gmz_replay_ingest: board_size " + std::to_string(board_size) + " outside 5..22");
  if (unroll < 1) return fail("gmz_replay_ingest: unroll " + std::to_string(unroll) + " < 1");
  if (n_steps < 1 || n_steps > GMZ_REPLAY_MAX_N_STEPS)
    return fail("gmz_replay_ingest: n_steps " + std::to_string(n_steps) + " outside 1.." +
                std::to_string(GMZ_REPLAY_MAX_N_STEPS));
  if (G < 1 || L < 1 || N < 1) return fail("gmz_replay_ingest: G, L and N must be positive");
  if (n_jobs < 0) return fail("gmz_replay_ingest: n_jobs < 0");
  if (n_jobs == 0) return 0;
  if (!jobs_host || !jobs_dev || !discount_pow) return fail("gmz_replay_ingest: jobs_host, jobs_dev or discount_pow is NULL");
  if (!hist_board_dev || !hist_player_dev || !hist_last_dev || !hist_policy_dev || !hist_value_dev || !hist_action_dev ||
      !ring_obs_dev || !ring_act_dev || !ring_rew_dev || !ring_pol_dev || !ring_val_dev || !ring_prio_dev)
    return fail("gmz_replay_ingest: a history or ring pointer is NULL");
  if (jobs_dev_bytes < (size_t)n_jobs * sizeof(ReplayJob))
    return fail("gmz_replay_ingest: device job table of " + std::to_string(jobs_dev_bytes) + " bytes is short of " +
                std::to_string(n_jobs) + " jobs x " + std::to_string(sizeof(ReplayJob)));
  const ReplayJob *jobs = (const ReplayJob *)jobs_host;
  long total = 0;
  std::vector<std::pair<long, long>> spans;  // kept slices as linear [begin, end) ring ranges
  spans.reserve(2 * (size_t)n_jobs);
  for (int i = 0; i < n_jobs; ++i) {
    const ReplayJob &j = jobs[i];
    const std::string at = "gmz_replay_ingest: job " + std::to_string(i) + ": ";
    if (j.game < 0 || j.game >= G) return fail(at + "game " + std::to_string(j.game) + " outside 0.." + std::to_string(G - 1));
    if (j.bank != 0 && j.bank != 1) return fail(at + "bank " + std::to_string(j.bank) + " is neither 0 nor 1");
    if (j.row0 < 0 || j.n < 1 || (long)j.row0 + j.n > L)
      return fail(at + "rows " + std::to_string(j.row0) + "+" + std::to_string(j.n) + " pass the history's L = " +
                  std::to_string(L));
    if (j.winner < -1 || j.winner > 1) return fail(at + "winner " + std::to_string(j.winner) + " outside -1..1");
    if (j.drop < 0 || j.drop >= j.n) return fail(at + "drop " + std::to_string(j.drop) + " outside 0..n-1");
    if (j.slot < 0 || j.slot >= N)
      return fail(at + "ring slot " + std::to_string(j.slot) + " outside 0.." + std::to_string(N - 1));
    if (j.first != total) return fail(at + "first " + std::to_string(j.first) + " is not the kept slices before it");
    const long kept = j.n - j.drop;
    total += kept;
    if (total > N)
      return fail("gmz_replay_ingest: the launch keeps more than the ring's N = " + std::to_string(N) + " slices");
    const long e = j.slot + kept;
    if (e <= N) spans.emplace_back(j.slot, e);
    else { spans.emplace_back(j.slot, (long)N); spans.emplace_back(0L, e - N); }
  }
  std::sort(spans.begin(), spans.end());
  for (size_t i = 1; i < spans.size(); ++i)
    if (spans[i].first < spans[i - 1].second)
      return fail("gmz_replay_ingest: kept slices of two jobs overlap at ring slot " + std::to_string(spans[i].first));
  ReplayArgs a;
  a.board = hist_board_dev; a.player = hist_player_dev; a.last = hist_last_dev; a.pol = hist_policy_dev;
  a.val = hist_value_dev; a.act = hist_action_dev;
  a.r_obs = ring_obs_dev; a.r_act = ring_act_dev; a.r_rew = ring_rew_dev; a.r_pol = ring_pol_dev; a.r_val = ring_val_dev;
  a.r_prio = ring_prio_dev;
  a.jobs = (const ReplayJob *)jobs_dev;
  a.prio = priority_dev;
  a.A = board_size * board_size; a.U = unroll; a.n_steps = n_steps; a.G = G; a.L = L; a.N = N; a.n_jobs = n_jobs;
  ReplayPow P;
  for (int i = 0; i <= GMZ_REPLAY_MAX_N_STEPS; ++i) P.pw[i] = i <= n_steps ? discount_pow[i] : 0.0;
  hipLaunchKernelGGL(k_replay_ingest, dim3((unsigned)total), dim3(256), 0, (hipStream_t)stream, a, P);
  GMZ_LAUNCH_CHECK();
  return 0;
}
