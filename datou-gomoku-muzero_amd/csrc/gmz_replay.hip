// gmz_replay.hip — finished self-play games from the device history (worker.GameHistory) straight into the trainer's
// device replay ring (replay.ReplayBuffer), one launch per self-play move; and, further down, training batches from
// that ring into the trainer's inputs (gmz_replay_gather) and the PER draw that picks them (gmz_replay_per_sample).
// Between the two: the ring's own games as engine positions and their re-searched targets back into the ring
// (gmz_replay_positions, gmz_replay_rewrite).
//
// Bit-exact restatement of records.final_rewards + records.compute_n_step_returns + replay.slices_from_game (built
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

struct ReplayJob {  // include/gmz.h's job record; replay.py builds it as 8 int32
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

// The n-step value target of position t of a game of n moves (the header's "value targets", in that operation
// order); val[row0 + i] is the search value of position i.  Shared by k_replay_ingest and k_replay_rewrite.
__device__ __forceinline__ float n_step_target(const ReplayPow &P, int n_steps, int n, int winner, int t,
                                               const float *val, long row0) {
  double s = 0.0;
  for (int i = 0; i < n_steps && t + i < n; ++i) s = s + P.pw[i] * (double)final_reward(n, winner, t + i);
  float v = (float)s;
  if (t + n_steps < n) v = v + val[row0 + t + n_steps] * (float)P.pw[n_steps];
  return v;
}

// The job of workgroup b: the last record (ReplayJob or RewriteJob) whose first slice is <= b.
template <typename Job>
__device__ __forceinline__ Job job_of_block(const Job *jobs, int n_jobs, int b) {
  int lo = 0, hi = n_jobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].first <= b) lo = mid; else hi = mid - 1;
  }
  return jobs[lo];
}

__global__ __launch_bounds__(256) void k_replay_ingest(const ReplayArgs a, const ReplayPow P) {
  const int b = (int)blockIdx.x;
  const ReplayJob j = job_of_block(a.jobs, a.n_jobs, b);
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
    a.r_val[ring * (U + 1) + u] = t < n ? n_step_target(P, a.n_steps, n, j.winner, t, a.val, (long)hrow) : 0.0f;
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

// ---------------------------------------------------------------------------------------------------------------
// Re-analysis of games that are already in the ring (reanalysis.RingReanalyser): ring slices become engine positions
// (gmz_replay_positions), and a search's new policies and values become ring targets (gmz_replay_rewrite).  Both are
// one pass of memory movement; the rewrite's value targets are n_step_target above, ingest's own.
//   positions   row r < P reads planes obs[slot, 0] of table row (slot, m): player = +1 for even m, else -1 (the
//               convention of every opening generator: black moves on even counts); cell = player where the own
//               plane is set, -player where the opponent plane is set, else 0; last = the set cell of plane 2 (the
//               largest when a ring row not written by a game holds several), -1 when the plane is empty;
//               move_count = m.  Rows P..G-1: empty board, player +1, last -1, count 0.
//   rewrite     slice t of a job (t = drop + k, ring slot (slot + k) mod N), unroll step u, t + u < n:
//               pol[u, :] = (float)pol_new[first + t + u - drop, :], val[u] = n_step_target(t + u) over the new values.
//               Entries past the game, and every other ring array, are not touched.
// One workgroup per row / per surviving slice.
struct PositionRow {  // include/gmz.h's row record: 2 int32
  int32_t slot, m;
};
static_assert(sizeof(PositionRow) == 8, "row record layout");

struct PositionArgs {
  const uint8_t *r_obs;
  const PositionRow *rows;
  int8_t *board;
  int8_t *player;
  int32_t *last;
  int32_t *count;
  int A, U, N, P;
};

__global__ __launch_bounds__(256) void k_replay_positions(const PositionArgs a) {
  __shared__ int s_last;
  const int r = (int)blockIdx.x, A = a.A, tid = (int)threadIdx.x, nt = (int)blockDim.x;
  int8_t *board = a.board + (size_t)r * A;
  if (r >= a.P) {  // padding row
    for (int c = tid; c < A; c += nt) board[c] = 0;
    if (tid == 0) { a.player[r] = 1; a.last[r] = -1; a.count[r] = 0; }
    return;
  }
  const PositionRow row = a.rows[r];
  // the host validated the table it was given; a device copy that differs from it writes nothing
  if (row.slot < 0 || row.slot >= a.N || row.m < 0 || row.m >= A) return;
  const int8_t pl = (row.m & 1) ? -1 : 1;
  const uint8_t *o = a.r_obs + (size_t)row.slot * (size_t)(a.U + 1) * 3 * A;
  if (tid == 0) s_last = -1;
  __syncthreads();
  for (int c = tid; c < A; c += nt) {
    board[c] = o[c] ? pl : (o[A + c] ? (int8_t)-pl : (int8_t)0);
    if (o[2 * A + c]) atomicMax(&s_last, c);
  }
  __syncthreads();
  if (tid == 0) { a.player[r] = pl; a.last[r] = s_last; a.count[r] = row.m; }
}

struct RewriteJob {  // include/gmz.h's job record: 6 int32
  int32_t slot, kept, n, drop, winner, first;
};
static_assert(sizeof(RewriteJob) == 24, "job record layout");

struct RewriteArgs {
  const double *pol_new;
  const float *val_new;
  float *r_pol;
  float *r_val;
  const RewriteJob *jobs;
  int A, U, n_steps, N, P, n_jobs;
};

__global__ __launch_bounds__(256) void k_replay_rewrite(const RewriteArgs a, const ReplayPow P) {
  const int b = (int)blockIdx.x;
  const RewriteJob j = job_of_block(a.jobs, a.n_jobs, b);
  const int kk = b - j.first;
  // the host validated the table it was given; a device copy that differs from it writes nothing
  if (j.slot < 0 || j.slot >= a.N || j.kept < 1 || j.kept > a.N || j.n < 1 || j.drop < 0 || j.drop != j.n - j.kept ||
      j.winner < -1 || j.winner > 1 || j.first < 0 || (long)j.first + j.kept > a.P || kk < 0 || kk >= j.kept)
    return;
  const int t0 = j.drop + kk, n = j.n, A = a.A, U = a.U;
  const size_t ring = (size_t)((j.slot + (long)kk) % a.N);
  const long row0 = (long)j.first - j.drop;  // staged row of position t: row0 + t, for t >= drop
  const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
  for (int u = tid; u <= U; u += nt) {
    const int t = t0 + u;
    if (t < n) a.r_val[ring * (U + 1) + u] = n_step_target(P, a.n_steps, n, j.winner, t, a.val_new, row0);
  }
  float *pol = a.r_pol + ring * (size_t)(U + 1) * A;
  for (int idx = tid; idx < (U + 1) * A; idx += nt) {
    const int u = idx / A, c = idx - u * A, t = t0 + u;
    if (t < n) pol[idx] = (float)a.pol_new[(size_t)(row0 + t) * A + c];
  }
}


// ---------------------------------------------------------------------------------------------------------------
// Training batches from the ring into the trainer's static inputs (replay.ReplayBuffer.gather_into), one launch.
//
// Bit-exact restatement of trainer.augment on batch = (obs[idx].float(), act[idx], rew[idx], pol[idx], val[idx]):
//   planes, policies  torch.rot90(x, k) then torch.flip of the last axis when flip.  Destination cell (i, j) reads the
//                     source cell through the inverse map: jj = flip ? H-1-j : j, then
//                     k = 0: (i, jj)   k = 1: (jj, H-1-i)   k = 2: (H-1-i, H-1-jj)   k = 3: (H-1-jj, i);
//                     u8 0/1 planes widen to f32 exactly.
//   augmented action  augment's own formulae on r = a // H, c = a % H (floor division, python's modulus):
//                     k = 1: r, c = c, H-1-r   k = 2: r, c = H-1-r, H-1-c   k = 3: r, c = H-1-c, r;
//                     flip: c = H-1-c; out = r * H + c.  The plain action output is a itself (-1 stays -1); for
//                     a = -1 the augmented output is what these formulae give (-1 under the identity), as augment's
//                     is: the loss masks those entries by the plain action.
// One workgroup per (sample, unroll step); writes run along the destination.  A row whose index lies outside
// 0..count-1 writes nothing.
struct GatherArgs {
  const uint8_t *r_obs;
  const int32_t *r_act;
  const float *r_rew;
  const float *r_pol;
  const float *r_val;
  const int64_t *idx;
  const float *w;
  float *o_obs;
  int64_t *o_act;
  float *o_rew;
  float *o_pol;
  float *o_val;
  int64_t *o_aug;
  float *o_w;
  int H, A, U, count, k, flip;
};

__device__ __forceinline__ int gather_src_cell(int d, int H, int k, int flip) {
  const int i = d / H, j = d - i * H, jj = flip ? H - 1 - j : j;
  int si, sj;
  if (k == 0) { si = i; sj = jj; }
  else if (k == 1) { si = jj; sj = H - 1 - i; }
  else if (k == 2) { si = H - 1 - i; sj = H - 1 - jj; }
  else { si = H - 1 - jj; sj = i; }
  return si * H + sj;
}

__device__ __forceinline__ int64_t gather_aug_action(int a, int H, int k, int flip) {
  int r = a / H;
  if (a < 0 && r * H != a) --r;  // floor division
  int c = a - r * H;             // python's modulus: 0..H-1
  int rr = r, cc = c;
  if (k == 1) { rr = c; cc = H - 1 - r; }
  else if (k == 2) { rr = H - 1 - r; cc = H - 1 - c; }
  else if (k == 3) { rr = H - 1 - c; cc = r; }
  if (flip) cc = H - 1 - cc;
  return (int64_t)rr * H + cc;
}

__global__ __launch_bounds__(256) void k_replay_gather(const GatherArgs a) {
  const int U1 = a.U + 1;
  const int b = (int)blockIdx.x / U1, u = (int)blockIdx.x - b * U1;
  const int64_t s = a.idx[b];
  if (s < 0 || s >= (int64_t)a.count) return;  // a row the host did not vouch for
  const int A = a.A, H = a.H, U = a.U, tid = (int)threadIdx.x, nt = (int)blockDim.x;
  if (tid == 0) {
    a.o_val[(size_t)b * U1 + u] = a.r_val[(size_t)s * U1 + u];
    if (u < U) {
      const int act = a.r_act[(size_t)s * U + u];
      a.o_act[(size_t)b * U + u] = (int64_t)act;
      a.o_aug[(size_t)b * U + u] = gather_aug_action(act, H, a.k, a.flip);
      a.o_rew[(size_t)b * U + u] = a.r_rew[(size_t)s * U + u];
    }
    if (u == 0) a.o_w[b] = a.w ? a.w[b] : 1.0f;
  }
  const uint8_t *so = a.r_obs + ((size_t)s * U1 + u) * 3 * A;
  const float *sp = a.r_pol + ((size_t)s * U1 + u) * A;
  float *dobs = a.o_obs + ((size_t)b * U1 + u) * 3 * A;
  float *dpol = a.o_pol + ((size_t)b * U1 + u) * A;
  for (int d = tid; d < A; d += nt) {
    const int src = gather_src_cell(d, H, a.k, a.flip);
    dobs[d] = (float)so[src];
    dobs[A + d] = (float)so[A + src];
    dobs[2 * A + d] = (float)so[2 * A + src];
    dpol[d] = sp[src];
  }
}

// ---------------------------------------------------------------------------------------------------------------
// The stratified proportional draw of ReplayBuffer.sample's PER branch, three launches, everything in f64.
//
// Summation order (fixed; p[j] = (double)prio[j] for j < count, 0.0 past count; "+" is one rounded f64 addition and
// every sum below runs left to right, starting from its first term):
//   group   g holds elements 16g .. 16g+15:          w[g][e] = p[16g] + p[16g+1] + ... + p[16g+e],   l[g] = w[g][15]
//   chunk   c holds groups 64c .. 64c+63:            S[c]    = l[64c] + l[64c+1] + ... + l[64c+63]
//   chunks  T[c] = S[0] + S[1] + ... + S[c]          (T[-1] = 0.0);   total = T[nchunks-1]
//   bases   b[c][0] = T[c-1],  b[c][t+1] = b[c][t] + l[64c+t]
//   cum[j]  = min(b[c][t] + w[64c+t][e], T[c])       for j = 1024c + 16t + e,
//             except cum[j] = T[c] for the last j < count of chunk c.
// Every term is >= 0, so each running sum is non-decreasing and cum is non-decreasing in j, with cum[count-1] = total.
//   u_i    = ((double)i + r_i) * (total / (double)B)
//   idx_i  = min(first j with cum[j] >= u_i, count-1)       prob_i = p[idx_i] / total
// Launch 1: one wave per chunk writes l and S.  Launch 2: one wave turns S into T in place.  Launch 3: one wave per
// draw: a binary search over T, the chunk's 64 bases by a 64-step running sum over lane values, a ballot, the group's
// 16 elements likewise.  Nothing depends on the grid: a wave's work is fixed by its chunk or its draw.
constexpr int PER_GROUP = 16, PER_GROUPS = 64, PER_CHUNK = PER_GROUP * PER_GROUPS;

__device__ __forceinline__ double bcast_d(double v, int lane) {
  return __hiloint2double(__shfl(__double2hiint(v), lane, 64), __shfl(__double2loint(v), lane, 64));
}

// running left-to-right sum over the wave's lane values from `start`: before = start + v[0] + ... + v[lane-1],
// returns the sum over all 64 lanes (wave-uniform)
__device__ __forceinline__ double wave_running_sum(double start, double v, int lane, double &before) {
  double acc = start;
  before = start;
#pragma unroll
  for (int t = 0; t < 64; ++t) {
    if (lane == t) before = acc;
    acc = acc + bcast_d(v, t);
  }
  return acc;
}

__global__ __launch_bounds__(256) void k_per_groups(const float *prio, int count, int nchunks, double *l, double *S) {
  const int lane = (int)threadIdx.x & 63;
  const int c = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (c >= nchunks) return;  // whole waves only
  const long g = (long)c * PER_GROUPS + lane;
  const long j0 = g * PER_GROUP;
  double s = 0.0;
  if (j0 < count) {
    s = (double)prio[j0];
    for (int e = 1; e < PER_GROUP; ++e)
      if (j0 + e < count) s = s + (double)prio[j0 + e];
    l[g] = s;
  }
  // S[c] = l[64c] + ... (groups past count are 0.0: x + 0.0 == x)
  double acc = bcast_d(s, 0);
#pragma unroll
  for (int t = 1; t < 64; ++t) acc = acc + bcast_d(s, t);
  if (lane == 0) S[c] = acc;
}

__global__ __launch_bounds__(64) void k_per_chunks(double *S, int nchunks) {
  const int lane = (int)threadIdx.x;
  double carry = 0.0;
  for (int c0 = 0; c0 < nchunks; c0 += 64) {
    const int c = c0 + lane;
    const double s = c < nchunks ? S[c] : 0.0;
    double before;
    carry = wave_running_sum(carry, s, lane, before);
    if (c < nchunks) S[c] = before + s;
  }
}

__global__ __launch_bounds__(256) void k_per_draw(const float *prio, const double *r, int count, int B, int nchunks,
                                                  const double *l, const double *T, int64_t *idx, double *prob) {
  const int lane = (int)threadIdx.x & 63;
  const int i = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (i >= B) return;  // whole waves only
  const double total = T[nchunks - 1];
  const double u = ((double)i + r[i]) * (total / (double)B);
  // first chunk with T[c] >= u
  int lo = 0, hi = nchunks;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (T[mid] >= u) hi = mid; else lo = mid + 1;
  }
  long j = (long)count - 1;  // the clamp: u beyond the total
  if (lo < nchunks) {
    const int c = lo;
    const long ngroups = ((long)count + PER_GROUP - 1) / PER_GROUP;
    const long g = (long)c * PER_GROUPS + lane;
    const double lg = g < ngroups ? l[g] : 0.0;
    double base;
    wave_running_sum(c > 0 ? T[c - 1] : 0.0, lg, lane, base);
    const unsigned long long m = __ballot(g < ngroups && base + lg >= u);
    const long last = ((long)(c + 1) * PER_CHUNK < count ? (long)(c + 1) * PER_CHUNK : (long)count) - 1;
    j = last;  // cum[last j of the chunk] = T[c] >= u
    if (m) {
      const int t = __ffsll((long long)m) - 1;
      const double bt = bcast_d(base, t);
      const long e0 = ((long)c * PER_GROUPS + t) * PER_GROUP;
      const long je = e0 + (lane & (PER_GROUP - 1));
      const double pe = (lane < PER_GROUP && je < count) ? (double)prio[je] : 0.0;
      double acc = bcast_d(pe, 0), w = acc;
#pragma unroll
      for (int e = 1; e < PER_GROUP; ++e) {
        acc = acc + bcast_d(pe, e);
        if (lane == e) w = acc;
      }
      const unsigned long long m2 = __ballot(lane < PER_GROUP && je < count && bt + w >= u);
      if (m2) {
        const long jf = e0 + (__ffsll((long long)m2) - 1);
        if (jf < j) j = jf;
      }
    }
  }
  if (lane == 0) {
    idx[i] = (int64_t)j;
    prob[i] = (double)prio[j] / total;
  }
}

static inline void per_sizes(int count, long &ngroups, long &nchunks) {
  ngroups = ((long)count + PER_GROUP - 1) / PER_GROUP;
  nchunks = ((long)count + PER_CHUNK - 1) / PER_CHUNK;
}

}  // namespace gmz

using namespace gmz;

// host helpers of the entry points' validation
static int below_one(const char *fn, const char *name, long v) {
  return fail(std::string(fn) + ": " + name + " " + std::to_string(v) + " < 1");
}

// the slices' geometry, the checks every entry point that takes it opens with (one without n_steps passes 1)
static int check_geometry(const char *fn, int board_size, int unroll, int n_steps = 1) {
  if (board_size < 5 || board_size > 22)
    return fail(std::string(fn) + ": board_size " + std::to_string(board_size) + " outside 5..22");
  if (unroll < 1) return below_one(fn, "unroll", unroll);
  if (n_steps < 1 || n_steps > GMZ_REPLAY_MAX_N_STEPS)
    return fail(std::string(fn) + ": n_steps " + std::to_string(n_steps) + " outside 1.." +
                std::to_string(GMZ_REPLAY_MAX_N_STEPS));
  return 0;
}

struct Capacity {  // a buffer's size in bytes against what the call writes or reads; `need` as the refusal words it
  const char *name;
  size_t have, need;
  std::string need_text;
};

// the first buffer of `caps` that is short, refused; 0 when every one holds its need
static int check_capacities(const char *fn, std::initializer_list<Capacity> caps) {
  for (const Capacity &c : caps)
    if (c.have < c.need)
      return fail(std::string(fn) + ": " + c.name + " of " + std::to_string(c.have) + " bytes is short of " +
                  (c.need_text.empty() ? std::to_string(c.need) : c.need_text));
  return 0;
}

static ReplayPow replay_pow(const double *discount_pow, int n_steps) {
  ReplayPow P;
  for (int i = 0; i <= GMZ_REPLAY_MAX_N_STEPS; ++i) P.pw[i] = i <= n_steps ? discount_pow[i] : 0.0;
  return P;
}

// ring slot runs as linear [begin, end) ranges: a run of `len` slots from `slot` that passes the ring's end is two
static inline void add_span(std::vector<std::pair<long, long>> &spans, long slot, long len, long N) {
  const long e = slot + len;
  if (e <= N) spans.emplace_back(slot, e);
  else { spans.emplace_back(slot, N); spans.emplace_back(0L, e - N); }
}

// the first ring slot two of the ranges share, or -1 (sorts the ranges)
static inline long first_overlap(std::vector<std::pair<long, long>> &spans) {
  std::sort(spans.begin(), spans.end());
  for (size_t i = 1; i < spans.size(); ++i)
    if (spans[i].first < spans[i - 1].second) return spans[i].first;
  return -1;
}

GMZ_EXPORT int gmz_replay_ingest(int board_size, int unroll, int n_steps, int G, int L, const int8_t *hist_board_dev,
                                 const int8_t *hist_player_dev, const int32_t *hist_last_dev,
                                 const double *hist_policy_dev, const float *hist_value_dev,
                                 const int32_t *hist_action_dev, uint8_t *ring_obs_dev, int32_t *ring_act_dev,
                                 float *ring_rew_dev, float *ring_pol_dev, float *ring_val_dev, float *ring_prio_dev,
                                 int N, const void *jobs_host, int n_jobs, const void *jobs_dev, size_t jobs_dev_bytes,
                                 const double *discount_pow, const float *priority_dev, void *stream) {
  const char *fn = "gmz_replay_ingest";
  if (check_geometry(fn, board_size, unroll, n_steps)) return -1;
  if (G < 1 || L < 1 || N < 1) return fail("gmz_replay_ingest: G, L and N must be positive");
  if (n_jobs < 0) return fail("gmz_replay_ingest: n_jobs < 0");
  if (n_jobs == 0) return 0;
  if (!jobs_host || !jobs_dev || !discount_pow) return fail("gmz_replay_ingest: jobs_host, jobs_dev or discount_pow is NULL");
  if (!hist_board_dev || !hist_player_dev || !hist_last_dev || !hist_policy_dev || !hist_value_dev || !hist_action_dev ||
      !ring_obs_dev || !ring_act_dev || !ring_rew_dev || !ring_pol_dev || !ring_val_dev || !ring_prio_dev)
    return fail("gmz_replay_ingest: a history or ring pointer is NULL");
  if (check_capacities(fn, {{"device job table", jobs_dev_bytes, (size_t)n_jobs * sizeof(ReplayJob),
                             std::to_string(n_jobs) + " jobs x " + std::to_string(sizeof(ReplayJob))}}))
    return -1;
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
    add_span(spans, j.slot, kept, N);
  }
  const long shared = first_overlap(spans);
  if (shared >= 0)
    return fail("gmz_replay_ingest: kept slices of two jobs overlap at ring slot " + std::to_string(shared));
  ReplayArgs a;
  a.board = hist_board_dev; a.player = hist_player_dev; a.last = hist_last_dev; a.pol = hist_policy_dev;
  a.val = hist_value_dev; a.act = hist_action_dev;
  a.r_obs = ring_obs_dev; a.r_act = ring_act_dev; a.r_rew = ring_rew_dev; a.r_pol = ring_pol_dev; a.r_val = ring_val_dev;
  a.r_prio = ring_prio_dev;
  a.jobs = (const ReplayJob *)jobs_dev;
  a.prio = priority_dev;
  a.A = board_size * board_size; a.U = unroll; a.n_steps = n_steps; a.G = G; a.L = L; a.N = N; a.n_jobs = n_jobs;
  hipLaunchKernelGGL(k_replay_ingest, dim3((unsigned)total), dim3(256), 0, (hipStream_t)stream, a,
                     replay_pow(discount_pow, n_steps));
  GMZ_LAUNCH_CHECK();
  return 0;
}

GMZ_EXPORT int gmz_replay_positions(int board_size, int unroll, int N, const uint8_t *ring_obs_dev,
                                    size_t ring_obs_bytes, const void *rows_host, int P, const void *rows_dev,
                                    size_t rows_dev_bytes, int G, int8_t *board_out_dev, size_t board_out_bytes,
                                    int8_t *player_out_dev, size_t player_out_bytes, int32_t *last_out_dev,
                                    size_t last_out_bytes, int32_t *count_out_dev, size_t count_out_bytes,
                                    void *stream) {
  const char *fn = "gmz_replay_positions";
  if (check_geometry(fn, board_size, unroll)) return -1;
  if (N < 1) return below_one(fn, "N", N);
  if (G < 1) return below_one(fn, "G", G);
  if (P < 1 || P > G) return fail("gmz_replay_positions: P " + std::to_string(P) + " outside 1..G = " + std::to_string(G));
  if (!ring_obs_dev || !rows_host || !rows_dev) return fail("gmz_replay_positions: ring_obs_dev, rows_host or rows_dev is NULL");
  if (!board_out_dev || !player_out_dev || !last_out_dev || !count_out_dev)
    return fail("gmz_replay_positions: an output pointer is NULL");
  const size_t A = (size_t)board_size * board_size, ng = (size_t)G;
  if (check_capacities(fn, {{"ring_obs", ring_obs_bytes, (size_t)N * (size_t)(unroll + 1) * 3 * A},
                            {"device row table", rows_dev_bytes, (size_t)P * sizeof(PositionRow)},
                            {"board_out", board_out_bytes, ng * A},
                            {"player_out", player_out_bytes, ng},
                            {"last_out", last_out_bytes, ng * 4},
                            {"count_out", count_out_bytes, ng * 4}}))
    return -1;
  const PositionRow *rows = (const PositionRow *)rows_host;
  for (int i = 0; i < P; ++i) {
    const std::string at = "gmz_replay_positions: row " + std::to_string(i) + ": ";
    if (rows[i].slot < 0 || rows[i].slot >= N)
      return fail(at + "ring slot " + std::to_string(rows[i].slot) + " outside 0.." + std::to_string(N - 1));
    if (rows[i].m < 0 || rows[i].m >= (int)A)
      return fail(at + "move count " + std::to_string(rows[i].m) + " outside 0.." + std::to_string(A - 1));
  }
  PositionArgs a;
  a.r_obs = ring_obs_dev; a.rows = (const PositionRow *)rows_dev;
  a.board = board_out_dev; a.player = player_out_dev; a.last = last_out_dev; a.count = count_out_dev;
  a.A = (int)A; a.U = unroll; a.N = N; a.P = P;
  hipLaunchKernelGGL(k_replay_positions, dim3((unsigned)G), dim3(256), 0, (hipStream_t)stream, a);
  GMZ_LAUNCH_CHECK();
  return 0;
}

GMZ_EXPORT int gmz_replay_rewrite(int board_size, int unroll, int n_steps, int N, float *ring_pol_dev,
                                  size_t ring_pol_bytes, float *ring_val_dev, size_t ring_val_bytes,
                                  const double *pol_new_dev, size_t pol_new_bytes, const float *val_new_dev,
                                  size_t val_new_bytes, int P, const void *jobs_host, int n_jobs, const void *jobs_dev,
                                  size_t jobs_dev_bytes, const double *discount_pow, void *stream) {
  const char *fn = "gmz_replay_rewrite";
  if (check_geometry(fn, board_size, unroll, n_steps)) return -1;
  if (N < 1) return below_one(fn, "N", N);
  if (P < 0) return fail("gmz_replay_rewrite: P " + std::to_string(P) + " < 0");
  if (n_jobs < 0) return fail("gmz_replay_rewrite: n_jobs < 0");
  if (n_jobs == 0) return 0;
  if (!jobs_host || !jobs_dev || !discount_pow) return fail("gmz_replay_rewrite: jobs_host, jobs_dev or discount_pow is NULL");
  if (!ring_pol_dev || !ring_val_dev || !pol_new_dev || !val_new_dev)
    return fail("gmz_replay_rewrite: a ring or staging pointer is NULL");
  const size_t A = (size_t)board_size * board_size, U1 = (size_t)unroll + 1;
  if (check_capacities(fn, {{"ring_pol", ring_pol_bytes, (size_t)N * U1 * A * sizeof(float)},
                            {"ring_val", ring_val_bytes, (size_t)N * U1 * sizeof(float)},
                            {"pol_new", pol_new_bytes, (size_t)P * A * sizeof(double)},
                            {"val_new", val_new_bytes, (size_t)P * sizeof(float)},
                            {"device job table", jobs_dev_bytes, (size_t)n_jobs * sizeof(RewriteJob)}}))
    return -1;
  const RewriteJob *jobs = (const RewriteJob *)jobs_host;
  long total = 0;
  std::vector<std::pair<long, long>> spans;
  spans.reserve(2 * (size_t)n_jobs);
  for (int i = 0; i < n_jobs; ++i) {
    const RewriteJob &j = jobs[i];
    const std::string at = "gmz_replay_rewrite: job " + std::to_string(i) + ": ";
    if (j.slot < 0 || j.slot >= N)
      return fail(at + "ring slot " + std::to_string(j.slot) + " outside 0.." + std::to_string(N - 1));
    if (j.kept < 1) return fail(at + "kept " + std::to_string(j.kept) + " < 1");
    if (j.kept > N) return fail(at + "kept " + std::to_string(j.kept) + " passes the ring's N = " + std::to_string(N));
    if (j.n < 1 || j.drop < 0 || j.drop != j.n - j.kept)
      return fail(at + "n " + std::to_string(j.n) + ", drop " + std::to_string(j.drop) + ", kept " +
                  std::to_string(j.kept) + ": drop is not n - kept");
    if (j.winner < -1 || j.winner > 1) return fail(at + "winner " + std::to_string(j.winner) + " outside -1..1");
    if (j.first != total) return fail(at + "first " + std::to_string(j.first) + " is not the staged rows before it");
    total += j.kept;
    if (total > P)
      return fail(at + "staged row " + std::to_string(total - 1) + " outside 0.." + std::to_string((long)P - 1));
    add_span(spans, j.slot, j.kept, N);
  }
  const long shared = first_overlap(spans);
  if (shared >= 0) return fail("gmz_replay_rewrite: the slices of two jobs overlap at ring slot " + std::to_string(shared));
  RewriteArgs a;
  a.pol_new = pol_new_dev; a.val_new = val_new_dev; a.r_pol = ring_pol_dev; a.r_val = ring_val_dev;
  a.jobs = (const RewriteJob *)jobs_dev;
  a.A = (int)A; a.U = unroll; a.n_steps = n_steps; a.N = N; a.P = P; a.n_jobs = n_jobs;
  hipLaunchKernelGGL(k_replay_rewrite, dim3((unsigned)total), dim3(256), 0, (hipStream_t)stream, a,
                     replay_pow(discount_pow, n_steps));
  GMZ_LAUNCH_CHECK();
  return 0;
}

GMZ_EXPORT int gmz_replay_gather(int board_size, int unroll, int N, int count, int B, const uint8_t *ring_obs_dev,
                                 const int32_t *ring_act_dev, const float *ring_rew_dev, const float *ring_pol_dev,
                                 const float *ring_val_dev, const int64_t *idx_dev, const float *w_dev, int k, int flip,
                                 float *obs_out_dev, size_t obs_out_bytes, int64_t *act_out_dev, size_t act_out_bytes,
                                 float *rew_out_dev, size_t rew_out_bytes, float *pol_out_dev, size_t pol_out_bytes,
                                 float *val_out_dev, size_t val_out_bytes, int64_t *act_aug_out_dev,
                                 size_t act_aug_out_bytes, float *w_out_dev, size_t w_out_bytes, void *stream) {
  const char *fn = "gmz_replay_gather";
  if (check_geometry(fn, board_size, unroll)) return -1;
  if (B < 1) return below_one(fn, "B", B);
  if (N < 1) return below_one(fn, "N", N);
  if (count < 1 || count > N)
    return fail("gmz_replay_gather: count " + std::to_string(count) + " outside 1..N = " + std::to_string(N));
  if (k < 0 || k > 3) return fail("gmz_replay_gather: k " + std::to_string(k) + " outside 0..3");
  if (flip != 0 && flip != 1) return fail("gmz_replay_gather: flip " + std::to_string(flip) + " is neither 0 nor 1");
  if (!ring_obs_dev || !ring_act_dev || !ring_rew_dev || !ring_pol_dev || !ring_val_dev)
    return fail("gmz_replay_gather: a ring pointer is NULL");
  if (!idx_dev) return fail("gmz_replay_gather: idx_dev is NULL");
  if (!obs_out_dev || !act_out_dev || !rew_out_dev || !pol_out_dev || !val_out_dev || !act_aug_out_dev || !w_out_dev)
    return fail("gmz_replay_gather: an output pointer is NULL");
  const size_t A = (size_t)board_size * board_size, U = (size_t)unroll, nb = (size_t)B;
  if ((nb * (U + 1) > (size_t)0x7fffffff))
    return fail("gmz_replay_gather: B * (unroll + 1) = " + std::to_string(nb * (U + 1)) + " passes one launch's grid");
  if (check_capacities(fn, {{"obs_out", obs_out_bytes, nb * (U + 1) * 3 * A * sizeof(float)},
                            {"act_out", act_out_bytes, nb * U * sizeof(int64_t)},
                            {"rew_out", rew_out_bytes, nb * U * sizeof(float)},
                            {"pol_out", pol_out_bytes, nb * (U + 1) * A * sizeof(float)},
                            {"val_out", val_out_bytes, nb * (U + 1) * sizeof(float)},
                            {"act_aug_out", act_aug_out_bytes, nb * U * sizeof(int64_t)},
                            {"w_out", w_out_bytes, nb * sizeof(float)}}))
    return -1;
  GatherArgs a;
  a.r_obs = ring_obs_dev; a.r_act = ring_act_dev; a.r_rew = ring_rew_dev; a.r_pol = ring_pol_dev; a.r_val = ring_val_dev;
  a.idx = idx_dev; a.w = w_dev;
  a.o_obs = obs_out_dev; a.o_act = act_out_dev; a.o_rew = rew_out_dev; a.o_pol = pol_out_dev; a.o_val = val_out_dev;
  a.o_aug = act_aug_out_dev; a.o_w = w_out_dev;
  a.H = board_size; a.A = (int)A; a.U = unroll; a.count = count; a.k = k; a.flip = flip;
  hipLaunchKernelGGL(k_replay_gather, dim3((unsigned)(nb * (U + 1))), dim3(256), 0, (hipStream_t)stream, a);
  GMZ_LAUNCH_CHECK();
  return 0;
}

GMZ_EXPORT int gmz_replay_per_sample_workspace_bytes(int count, int B, size_t *out) {
  const char *fn = "gmz_replay_per_sample_workspace_bytes";
  if (count < 1) return below_one(fn, "count", count);
  if (B < 1) return below_one(fn, "B", B);
  if (!out) return fail("gmz_replay_per_sample_workspace_bytes: out is NULL");
  long ngroups, nchunks;
  per_sizes(count, ngroups, nchunks);
  *out = (size_t)(ngroups + nchunks) * sizeof(double);
  return 0;
}

GMZ_EXPORT int gmz_replay_per_sample(const float *prio_dev, const double *r_dev, int count, int B, int64_t *idx_dev,
                                     size_t idx_bytes, double *prob_dev, size_t prob_bytes, void *workspace_dev,
                                     size_t ws_bytes, void *stream) {
  const char *fn = "gmz_replay_per_sample";
  if (count < 1) return below_one(fn, "count", count);
  if (B < 1) return below_one(fn, "B", B);
  if (!prio_dev) return fail("gmz_replay_per_sample: prio_dev is NULL");
  if (!r_dev) return fail("gmz_replay_per_sample: r_dev is NULL");
  if (!idx_dev) return fail("gmz_replay_per_sample: idx_dev is NULL");
  if (!prob_dev) return fail("gmz_replay_per_sample: prob_dev is NULL");
  if (!workspace_dev) return fail("gmz_replay_per_sample: workspace_dev is NULL");
  if ((uintptr_t)workspace_dev % sizeof(double))
    return fail("gmz_replay_per_sample: workspace_dev is not 8-byte aligned");
  long ngroups, nchunks;
  per_sizes(count, ngroups, nchunks);
  const size_t need = (size_t)(ngroups + nchunks) * sizeof(double);
  if (check_capacities(fn, {{"workspace", ws_bytes, need,
                             std::to_string(need) + " (gmz_replay_per_sample_workspace_bytes)"},
                            {"idx", idx_bytes, (size_t)B * sizeof(int64_t)},
                            {"prob", prob_bytes, (size_t)B * sizeof(double)}}))
    return -1;
  double *l = (double *)workspace_dev, *T = l + ngroups;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_per_groups, dim3((unsigned)((nchunks + 3) / 4)), dim3(256), 0, st, prio_dev, count, (int)nchunks,
                     l, T);
  GMZ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_per_chunks, dim3(1), dim3(64), 0, st, T, (int)nchunks);
  GMZ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_per_draw, dim3((unsigned)(((long)B + 3) / 4)), dim3(256), 0, st, prio_dev, r_dev, count, B,
                     (int)nchunks, (const double *)l, (const double *)T, idx_dev, prob_dev);
  GMZ_LAUNCH_CHECK();
  return 0;
}
