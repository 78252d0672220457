// gmz_game.hip — batched Gomoku board kernels for gfx950 (game.py restated for G boards at once).
//
// One wavefront per board; lanes cover cells / directions.  Integer work only: results are
// bit-exact with /root/reference/game.py by construction and checked against tests/golden.
//   check_win        game.py:25-58   (4 directions × 2 senses, runs capped at n_in_row+1)
//   board_state      game.py:12-17   (3 float32 planes)
//   play             game.py:20-23 do_move + game.py:60-63 get_game_ended
#include "gmz_common.h"
#include "gmz_device.h"


namespace gmz {

static thread_local std::string g_err;
void set_error(const std::string &m) { g_err = m; }
int fail(const std::string &m) {
  g_err = m;
  return -1;
}

__global__ void k_check_win(const int8_t *__restrict__ boards, int G, int size, int n_in_row,
                            const int32_t *__restrict__ moves, uint8_t *__restrict__ out) {
  int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  int mv = moves[g];
  out[g] = mv < 0 ? 0 : (uint8_t)check_win_dev(boards + (size_t)g * size * size, size, n_in_row, mv / size, mv % size);
}

__global__ void k_board_state(const int8_t *__restrict__ boards, int G, int size,
                              const int8_t *__restrict__ players, const int32_t *__restrict__ last_moves,
                              float *__restrict__ obs) {
  const int A = size * size;
  const int g = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G || i >= A) return;
  const int8_t b = boards[(size_t)g * A + i];
  const int p = players[g];
  float *o = obs + (size_t)g * 3 * A;
  o[i] = b == p ? 1.f : 0.f;
  o[A + i] = b == -p ? 1.f : 0.f;
  o[2 * A + i] = (last_moves[g] == i) ? 1.f : 0.f;
}

__global__ void k_play(int8_t *__restrict__ boards, int G, int size, int n_in_row, int8_t *__restrict__ players,
                       int32_t *__restrict__ last_moves, int32_t *__restrict__ move_counts,
                       const int32_t *__restrict__ actions, int8_t *__restrict__ status, int reset_finished) {
  int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  play_one(boards + (size_t)g * size * size, size, n_in_row, players + g, last_moves + g, move_counts + g,
           actions[g], status + g, reset_finished);
}

}  // namespace gmz

using namespace gmz;

GMZ_EXPORT const char *gmz_last_error(void) { return g_err.c_str(); }
GMZ_EXPORT int gmz_abi_version(void) { return GMZ_ABI_VERSION; }
GMZ_EXPORT int gmz_device_synchronize(void) {
  GMZ_HIP(hipDeviceSynchronize());
  return 0;
}

// workers.py:49-123 find_winning_moves_rebuilt for every empty cell of G boards at once: one
// workgroup per board (board in LDS), one thread per cell.  cls[g][cell] = 0 none, 1 'five',
// 2 'open_four', 3 'combo' (priority as the reference: five, then open four, then combos).  With
// actions != nullptr the per-game missed-win counters of workers.py:191-203 are accumulated:
// a position counts as missed when the winning set is non-empty and actions[g] is not in it
// (missed_fives also needs a 'five').  actions[g] < 0 leaves game g's counters untouched.
__global__ void __launch_bounds__(512) k_winning_scan(const int8_t *__restrict__ boards, const int8_t *__restrict__ players,
                                                      const int32_t *__restrict__ actions, int size, int n_in_row,
                                                      uint8_t *__restrict__ cls, int32_t *__restrict__ missed_fives,
                                                      int32_t *__restrict__ missed_totals) {
  __shared__ int8_t b[MAX_A];
  __shared__ int any_win, any_five, act_cls;
  const int g = blockIdx.x, A = size * size;
  const int8_t *src = boards + (size_t)g * A;
  for (int i = threadIdx.x; i < A; i += blockDim.x) b[i] = src[i];
  if (threadIdx.x == 0) {
    any_win = 0;
    any_five = 0;
    act_cls = 0;
  }
  __syncthreads();
  const int p = players[g], opp = -p;
  const int act = actions ? actions[g] : -1;
  for (int cell = threadIdx.x; cell < A; cell += blockDim.x) {
    int c = 0;
    if (b[cell] == 0) {
      const int r0 = cell / size, c0 = cell % size;
      const int dr[4] = {0, 1, 1, 1}, dc[4] = {1, 0, 1, -1};
      // 1. five (game.py:25-58 check_win with the stone placed, overlines included)
      bool five = false;
      for (int d = 0; d < 4 && !five; ++d) {
        int count = 1;
        for (int sgn = 1; sgn >= -1; sgn -= 2)
          for (int i = 1; i < n_in_row + 2; ++i) {
            const int nr = r0 + sgn * i * dr[d], nc = c0 + sgn * i * dc[d];
            if (nr >= 0 && nr < size && nc >= 0 && nc < size && b[nr * size + nc] == p) count++;
            else break;
          }
        five = count >= n_in_row;
      }
      if (five) {
        c = 1;
      } else {
        // 2. 9-cell windows through the move, off-board = opponent (workers.py:72-103)
        int n_o4 = 0, n_b4 = 0, n_o3 = 0;
        for (int d = 0; d < 4; ++d) {
          int t[9];
#pragma unroll
          for (int k = 0; k < 9; ++k) {
            const int i = k - 4, nr = r0 + i * dr[d], nc = c0 + i * dc[d];
            t[k] = (i == 0) ? p : ((nr >= 0 && nr < size && nc >= 0 && nc < size) ? (int)b[nr * size + nc] : opp);
          }
          bool o4 = false, b4 = false, o3 = false;
#pragma unroll
          for (int i = 0; i + 6 <= 9; ++i)
            o4 |= t[i] == 0 && t[i + 1] == p && t[i + 2] == p && t[i + 3] == p && t[i + 4] == p && t[i + 5] == 0;
#pragma unroll
          for (int i = 0; i + 5 <= 9; ++i) {
            const bool mid = t[i + 1] == p && t[i + 2] == p && t[i + 3] == p;
            b4 |= mid && ((t[i] == opp && t[i + 4] == 0) || (t[i] == 0 && t[i + 4] == opp));
            o3 |= mid && t[i] == 0 && t[i + 4] == 0;
          }
          n_o4 += o4;
          n_b4 += b4;
          n_o3 += o3;
        }
        if (n_o4 > 0) c = 2;
        else if (n_b4 >= 2 || (n_b4 >= 1 && n_o3 >= 1) || n_o3 >= 2) c = 3;
      }
    }
    if (cls) cls[(size_t)g * A + cell] = (uint8_t)c;
    if (c) {
      any_win = 1;  // benign races: every writer stores the same value
      if (c == 1) any_five = 1;
      if (cell == act) act_cls = c;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && act >= 0 && any_win && act_cls == 0) {
    missed_totals[g] += 1;
    if (any_five) missed_fives[g] += 1;
  }
}

GMZ_EXPORT int gmz_game_winning_scan(const int8_t *boards, const int8_t *players, const int32_t *actions, int G,
                                     int size, int n_in_row, uint8_t *cls, int32_t *missed_fives,
                                     int32_t *missed_totals, void *stream) {
  if (G <= 0 || size <= 0 || size * size > MAX_A) return fail("gmz_game_winning_scan: bad shape");
  if (!boards || !players) return fail("gmz_game_winning_scan: null board/player");
  if (actions && (!missed_fives || !missed_totals)) return fail("gmz_game_winning_scan: counters required with actions");
  if (!actions && !cls) return fail("gmz_game_winning_scan: nothing to compute");
  const int A = size * size;
  const int threads = A <= 256 ? 256 : 512;
  hipLaunchKernelGGL(k_winning_scan, dim3(G), dim3(threads), 0, (hipStream_t)stream, boards, players, actions, size,
                     n_in_row, cls, missed_fives, missed_totals);
  GMZ_LAUNCH_CHECK();
  return 0;
}

namespace gmz {

// One candidate of the anchor's arg-max over (key, noise, -cell), compared lexicographically; cell < 0 = none.
struct AnchorBest {
  double key, noise;
  int cell;
};

__device__ __forceinline__ bool anchor_better(const AnchorBest &x, const AnchorBest &y) {
  if (y.cell < 0) return x.cell >= 0;
  if (x.cell < 0) return false;
  if (x.key != y.key) return x.key > y.key;
  if (x.noise != y.noise) return x.noise > y.noise;
  return x.cell < y.cell;
}

// The anchor opponents' move rule: one workgroup per board (board in LDS), one thread per cell.
// An empty cell's score sums, over the n-cell windows through it in the four directions that lie on the board
// and hold stones of one colour only (or none), W_own[min(m, 4)] for the mover's windows and W_opp[min(m, 4)] for
// the opponent's, m = the stones the window still lacks once the cell is taken; kind 1 scores every empty cell 0.
// The move is the empty cell with the largest (score + scale * noise, noise, -cell); -1 on a full board and for
// a game whose game[g] is negative.  scores (nullable) int64[G][A]: the score, -1 for an occupied cell.
__global__ void __launch_bounds__(512) k_anchor_move(const int8_t *__restrict__ boards, const int8_t *__restrict__ players,
                                                     const int32_t *__restrict__ game, const double *__restrict__ noise,
                                                     int size, int n_in_row, int kind, double scale,
                                                     int32_t *__restrict__ actions, int64_t *__restrict__ scores) {
  __shared__ int8_t b[MAX_A];
  __shared__ double wave_key[512 / WAVE], wave_noise[512 / WAVE];
  __shared__ int wave_cell[512 / WAVE];
  const int g = blockIdx.x, A = size * size;
  if (game && game[g] < 0) {  // an idle arena slot (the whole workgroup leaves together)
    if (threadIdx.x == 0) actions[g] = -1;
    if (scores)
      for (int i = threadIdx.x; i < A; i += blockDim.x) scores[(size_t)g * A + i] = -1;
    return;
  }
  const int8_t *src = boards + (size_t)g * A;
  for (int i = threadIdx.x; i < A; i += blockDim.x) b[i] = src[i];
  __syncthreads();
  const int p = players[g];
  const int cell = threadIdx.x;  // blockDim.x >= A (gmz_game_anchor_move)
  AnchorBest best = {0.0, 0.0, -1};
  if (cell < A) {
    int64_t sc = -1;
    if (b[cell] == 0) {
      sc = 0;
      if (kind == 0) {
        const int64_t w_own[5] = {1 << 26, 1 << 13, 1 << 6, 1 << 2, 1};
        const int64_t w_opp[5] = {1 << 20, 1 << 10, 1 << 5, 1 << 1, 0};
        const int r0 = cell / size, c0 = cell % size;
        const int dr[4] = {0, 1, 1, 1}, dc[4] = {1, 0, 1, -1};
        for (int d = 0; d < 4; ++d)
          for (int o = 0; o < n_in_row; ++o) {
            const int rs = r0 - o * dr[d], cs = c0 - o * dc[d];  // the window's first cell; its last:
            const int re = rs + (n_in_row - 1) * dr[d], ce = cs + (n_in_row - 1) * dc[d];
            if (rs < 0 || re >= size || cs < 0 || cs >= size || ce < 0 || ce >= size) continue;
            int own = 0, opp = 0;
            for (int j = 0; j < n_in_row; ++j) {
              const int v = b[(rs + j * dr[d]) * size + cs + j * dc[d]];
              own += v == p;
              opp += v == -p;
            }
            if (opp == 0) sc += w_own[min(n_in_row - 1 - own, 4)];
            if (own == 0) sc += w_opp[min(n_in_row - 1 - opp, 4)];
          }
      }
      const double nz = noise ? noise[(size_t)g * A + cell] : 0.0;
      best.key = (double)sc + scale * nz;
      best.noise = nz;
      best.cell = cell;
    }
    if (scores) scores[(size_t)g * A + cell] = sc;
  }
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    AnchorBest o;
    o.key = __shfl_xor(best.key, off);
    o.noise = __shfl_xor(best.noise, off);
    o.cell = __shfl_xor(best.cell, off);
    if (anchor_better(o, best)) best = o;
  }
  const int wave = threadIdx.x / WAVE;
  if (threadIdx.x % WAVE == 0) {
    wave_key[wave] = best.key;
    wave_noise[wave] = best.noise;
    wave_cell[wave] = best.cell;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < (int)blockDim.x / WAVE; ++w) {
      const AnchorBest o = {wave_key[w], wave_noise[w], wave_cell[w]};
      if (anchor_better(o, best)) best = o;
    }
    actions[g] = best.cell;
  }
}

}  // namespace gmz

GMZ_EXPORT int gmz_game_anchor_move(const int8_t *boards, const int8_t *players, const int32_t *game, const double *noise,
                                    size_t noise_bytes, int G, int size, int n_in_row, int kind, double scale,
                                    int32_t *actions, size_t actions_bytes, int64_t *scores, size_t scores_bytes,
                                    void *stream) {
  if (G <= 0 || size <= 0 || size * size > MAX_A) return fail("gmz_game_anchor_move: bad shape");
  if (n_in_row < 1 || n_in_row > size) return fail("gmz_game_anchor_move: n_in_row must be in [1, size]");
  if (kind != 0 && kind != 1) return fail("gmz_game_anchor_move: kind must be 0 (threat) or 1 (uniform)");
  if (!(scale >= 0.0) || !std::isfinite(scale)) return fail("gmz_game_anchor_move: scale must be finite and >= 0");
  if (!boards || !players || !actions) return fail("gmz_game_anchor_move: null boards, players or actions");
  const size_t A = (size_t)size * size, cells = (size_t)G * A;
  if (noise && noise_bytes < cells * sizeof(double))
    return fail("gmz_game_anchor_move: noise holds " + std::to_string(noise_bytes) + " bytes, G * A * 8 = " +
                std::to_string(cells * sizeof(double)));
  if (actions_bytes < (size_t)G * sizeof(int32_t))
    return fail("gmz_game_anchor_move: actions holds " + std::to_string(actions_bytes) + " bytes, G * 4 = " +
                std::to_string((size_t)G * sizeof(int32_t)));
  if (scores && scores_bytes < cells * sizeof(int64_t))
    return fail("gmz_game_anchor_move: scores holds " + std::to_string(scores_bytes) + " bytes, G * A * 8 = " +
                std::to_string(cells * sizeof(int64_t)));
  const int threads = A <= 256 ? 256 : 512;
  hipLaunchKernelGGL(k_anchor_move, dim3(G), dim3(threads), 0, (hipStream_t)stream, boards, players, game, noise, size,
                     n_in_row, kind, scale, actions, scores);
  GMZ_LAUNCH_CHECK();
  return 0;
}

GMZ_EXPORT int gmz_game_check_win(const int8_t *boards, int G, int size, int n_in_row, const int32_t *moves,
                                  uint8_t *out, void *stream) {
  if (G <= 0 || size <= 0 || size * size > MAX_A) return fail("gmz_game_check_win: bad shape");
  hipLaunchKernelGGL(k_check_win, dim3((G + 255) / 256), dim3(256), 0, (hipStream_t)stream, boards, G, size,
                     n_in_row, moves, out);
  GMZ_LAUNCH_CHECK();
  return 0;
}

GMZ_EXPORT int gmz_game_board_state(const int8_t *boards, int G, int size, const int8_t *players,
                                    const int32_t *last_moves, float *obs, void *stream) {
  if (G <= 0 || size <= 0 || size * size > MAX_A) return fail("gmz_game_board_state: bad shape");
  int A = size * size;
  hipLaunchKernelGGL(k_board_state, dim3((A + 255) / 256, G), dim3(256), 0, (hipStream_t)stream, boards, G,
                     size, players, last_moves, obs);
  GMZ_LAUNCH_CHECK();
  return 0;
}

GMZ_EXPORT int gmz_game_play(int8_t *boards, int G, int size, int n_in_row, int8_t *players, int32_t *last_moves,
                             int32_t *move_counts, const int32_t *actions, int8_t *status, void *stream) {
  if (G <= 0 || size <= 0 || size * size > MAX_A) return fail("gmz_game_play: bad shape");
  hipLaunchKernelGGL(k_play, dim3((G + 255) / 256), dim3(256), 0, (hipStream_t)stream, boards, G, size, n_in_row,
                     players, last_moves, move_counts, actions, status, 0);
  GMZ_LAUNCH_CHECK();
  return 0;
}
