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

namespace gmz {

constexpr int VCF_MAX_DEPTH = 16, VCF_MAX_NODES = 1 << 20;
constexpr int VCF_MULTI = 0x4000;  // info bit: T(c) holds two or more cells (a cell index is below 512)

constexpr int VCF_LINES = 2 * 22 - 1;  // lines of one orientation on the largest board: its 43 diagonals

__device__ __forceinline__ uint64_t vcf_uniform(uint64_t x) {  // a wave-uniform 64-bit value, in scalar registers
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(x >> 32)) << 32) |
         (uint32_t)__builtin_amdgcn_readfirstlane((int)x);
}

// Cells j * 64 .. j * 64 + 63 of a cell mask kept as 32-bit words in LDS, wave-uniform.
__device__ __forceinline__ uint64_t vcf_word(const uint32_t *mask, int j) {
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)mask[2 * j + 1]) << 32) |
         (uint32_t)__builtin_amdgcn_readfirstlane((int)mask[2 * j]);
}

// The line of orientation d (0: (0,1), 1: (1,0), 2: (1,1), 3: (1,-1)) through cell (r, c) and the cell's bit in it.
// A step along the direction raises the bit index by one: the index is the column in a row and the row elsewhere.
__device__ __forceinline__ void vcf_line(int d, int r, int c, int size, int &line, int &pos) {
  line = d == 0 ? r : d == 1 ? c : d == 2 ? r - c + size - 1 : r + c;
  pos = d == 0 ? c : r;
}

__device__ __forceinline__ bool vcf_empty(const uint32_t (*lines)[4][VCF_LINES], int r, int c) {
  return !(((lines[0][0][r] | lines[1][0][r]) >> c) & 1);
}

// What the empty cell (r0, c0) is in one node of the forced-win search.  The board is kept as bit
// lines: lines[s][d][l] holds the stones of the attacker (s = 0) or the defender (s = 1) on line l of orientation d.
// Per direction the cells of the line at most n-1 steps from the cell, as far as the board goes (back against the
// direction, fwd along it), are a shifted piece of two line words (bit k + back = the cell k steps along), and every
// window of n cells that holds the cell is a run of n bits in it.  five_p / five_o: a window with n-1 stones of the
// attacker / of the defender (the cell is its one other cell); four: a window with n-2 attacker stones, no defender
// stone and so one more empty cell e; e1 the first such e, multi: another window gave a different e.
__device__ __forceinline__ void vcf_cell(const uint32_t (*lines)[4][VCF_LINES], int size, int n, int r0, int c0,
                                         bool &five_p, bool &five_o, bool &four, bool &multi, int &e1) {
  const int dr[4] = {0, 1, 1, 1}, dc[4] = {1, 0, 1, -1};
  const uint32_t run = (1u << n) - 1;
  const int cell = r0 * size + c0;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    int back = n - 1, fwd = n - 1;
    if (dr[d]) {
      back = min(back, r0);
      fwd = min(fwd, size - 1 - r0);
    }
    if (dc[d] > 0) {
      back = min(back, c0);
      fwd = min(fwd, size - 1 - c0);
    } else if (dc[d] < 0) {
      back = min(back, size - 1 - c0);
      fwd = min(fwd, c0);
    }
    if (back + fwd < n - 1) continue;  // no window through the cell lies on the board
    int line, pos;
    vcf_line(d, r0, c0, size, line, pos);
    const uint32_t span = (2u << (back + fwd)) - 1;  // back + fwd + 1 <= size bits
    const uint32_t own = (lines[0][d][line] >> (pos - back)) & span, opp = (lines[1][d][line] >> (pos - back)) & span;
    if (__popc(own) < n - 2 && __popc(opp) < n - 1) continue;
    const int step = dr[d] * size + dc[d];
    for (int w = 0; w <= back + fwd - (n - 1); ++w) {  // the window of bits [w, w + n)
      const uint32_t wm = run << w;
      const int n_own = __popc(own & wm), n_opp = __popc(opp & wm);
      five_p |= n_own == n - 1;
      five_o |= n_opp == n - 1;
      if (n_own == n - 2 && n_opp == 0) {
        const int e = cell + (__builtin_ctz(wm & ~own & ~(1u << back)) - back) * step;
        if (!four) e1 = e;
        else if (e != e1) multi = true;
        four = true;
      }
    }
  }
}

// The exact, depth-limited forced-win (VCF) search of DESIGN.md §8b for G boards: one wave per board, a workgroup of
// one wave, so a board at its node budget holds nothing but its own wave.  The search is serial and wave-uniform
// (every branch is taken on a ballot or on a value all lanes read from LDS); a node's work is wide: lane l classifies
// the cells l, l + 64, ... (up to 8), and a ballot per group of 64 cells gives the five and four masks in ascending
// cell order.  Below the root a node differs from the one above it by two stones, so it takes that node's masks and
// replies and classifies again only the cells within n-1 steps of a stone along a line (16 (n-1) cells: one per lane
// at n = 5).  The board (as bit lines in the four orientations, so that a cell reads two words per direction), per
// level the three masks, the candidates left, each four's reply (info) and the two stones played are in LDS; nothing
// is kept in global memory, and the only atomics are LDS ORs and ANDs on the bit lines and masks.
__global__ void __launch_bounds__(WAVE) k_vcf(const int8_t *__restrict__ boards, const int8_t *__restrict__ players,
                                              const int32_t *__restrict__ game, int size, int n, int max_depth,
                                              int max_nodes, int8_t *__restrict__ status, int32_t *__restrict__ moves,
                                              int32_t *__restrict__ lengths, int32_t *__restrict__ nodes,
                                              int32_t *__restrict__ actions) {
  __shared__ uint32_t lines[2][4][VCF_LINES];
  __shared__ uint16_t rc[MAX_A];                  // a cell's row << 8 | column
  __shared__ int16_t info[VCF_MAX_DEPTH][MAX_A];  // of a four cell c: T(c)'s first cell, | VCF_MULTI
  __shared__ uint32_t masks[VCF_MAX_DEPTH][3][2 * NJ];  // per level five(b, p), five(b, -p), fours(b, p): bit = cell
  __shared__ uint64_t cand[VCF_MAX_DEPTH][NJ];    // the level's candidates not yet tried
  __shared__ int16_t played[VCF_MAX_DEPTH][2];    // the attacker's four and the defender's reply on the board
  const int g = blockIdx.x, A = size * size, lane = threadIdx.x;
  if (game && game[g] < 0) {  // an idle arena slot: actions[g] stays as it is
    if (lane == 0) {
      status[g] = 3;
      moves[g] = -1;
      if (lengths) lengths[g] = 0;
      if (nodes) nodes[g] = 0;
    }
    return;
  }
  for (int i = lane; i < 2 * 4 * VCF_LINES; i += WAVE) (&lines[0][0][0])[i] = 0;
  __syncthreads();
  const int p = players[g];
  const int8_t *src = boards + (size_t)g * A;
  for (int i = lane; i < A; i += WAVE) {
    const int r = i / size, c = i - r * size, v = src[i];
    rc[i] = (uint16_t)(r << 8 | c);
    if (v != 0)
      for (int d = 0; d < 4; ++d) {
        int line, pos;
        vcf_line(d, r, c, size, line, pos);
        atomicOr(&lines[v == p ? 0 : 1][d][line], 1u << pos);
      }
  }
  __syncthreads();
  // a stone of side s goes on or off the cell: lane s * 4 + d flips its bit in orientation d (eight distinct words)
  auto flip = [&](int c0, int c1) {
    if (lane < 8) {
      const int s = lane >> 2, d = lane & 3, x = rc[s ? c1 : c0];
      int line, pos;
      vcf_line(d, x >> 8, x & 255, size, line, pos);
      lines[s][d][line] ^= 1u << pos;
    }
  };
  const int nj = (A + WAVE - 1) / WAVE;
  int level = 0, count = 0, st = 0, mv = -1, len = 0;
  for (;;) {  // solve() of the node at ``level``, with max_depth - level attacker moves left
    if (++count > max_nodes) {
      st = 2;
      break;
    }
    const bool leaf = max_depth - level <= 1;
    if (level == 0) {  // the root: every cell
#pragma unroll 1
      for (int j = 0; j < nj; ++j) {
        const int cell = j * WAVE + lane;
        bool five_p = false, five_o = false, four = false, multi = false;
        int e1 = 0;
        if (cell < A) {
          const int r0 = rc[cell] >> 8, c0 = rc[cell] & 255;
          if (vcf_empty(lines, r0, c0)) vcf_cell(lines, size, n, r0, c0, five_p, five_o, four, multi, e1);
        }
        const uint64_t wp = __ballot(five_p), wo = __ballot(five_o), wf = __ballot(four);
        if (four) info[0][cell] = (int16_t)(e1 | (multi ? VCF_MULTI : 0));
        if (lane < 2) {  // lane 0 the low words, lane 1 the high ones
          masks[0][0][2 * j + lane] = (uint32_t)(wp >> (32 * lane));
          masks[0][1][2 * j + lane] = (uint32_t)(wo >> (32 * lane));
          masks[0][2][2 * j + lane] = (uint32_t)(wf >> (32 * lane));
        }
      }
    } else {
      // below the root: the level above's masks and replies, with the cells put right that share a window with one
      // of the two stones just played (at most n-1 steps from it along a line), and the two cells themselves
      for (int i = lane; i < 3 * 2 * NJ; i += WAVE) (&masks[level][0][0])[i] = (&masks[level - 1][0][0])[i];
      for (int i = lane; i < A; i += WAVE) info[level][i] = info[level - 1][i];
      __syncthreads();
      const int dr[4] = {0, 1, 1, 1}, dc[4] = {1, 0, 1, -1};
      const int m = 2 * (n - 1);
      for (int idx = lane; idx < 8 * m + 2; idx += WAVE) {
        const bool self = idx >= 8 * m;
        int r, c;
        if (self) {
          const int x = rc[played[level - 1][idx - 8 * m]];
          r = x >> 8;
          c = x & 255;
        } else {
          const int s = idx / (4 * m), rem = idx - s * 4 * m, d = rem / m, kk = rem - d * m;
          const int k = kk - (n - 1) + (kk >= n - 1 ? 1 : 0);  // -(n-1) .. -1, 1 .. n-1
          const int x = rc[played[level - 1][s]];
          r = (x >> 8) + k * dr[d];
          c = (x & 255) + k * dc[d];
        }
        if (r < 0 || r >= size || c < 0 || c >= size) continue;
        const int cell = r * size + c;
        bool five_p = false, five_o = false, four = false, multi = false;
        int e1 = 0;
        if (!self && vcf_empty(lines, r, c)) vcf_cell(lines, size, n, r, c, five_p, five_o, four, multi, e1);
        // lanes that meet on a cell write the same; lanes on other cells of a word go through the LDS atomics
        const uint32_t bit = 1u << (cell & 31);
        uint32_t *w = &masks[level][0][cell >> 5];  // the same word of the next two masks: + 2 NJ, + 4 NJ
        five_p ? atomicOr(w, bit) : atomicAnd(w, ~bit);
        five_o ? atomicOr(w + 2 * NJ, bit) : atomicAnd(w + 2 * NJ, ~bit);
        four ? atomicOr(w + 4 * NJ, bit) : atomicAnd(w + 4 * NJ, ~bit);
        if (four) info[level][cell] = (int16_t)(e1 | (multi ? VCF_MULTI : 0));
      }
    }
    __syncthreads();
    int first_five = -1, fo_cell = -1, fo_count = 0;
    for (int j = 0; j < nj; ++j) {
      const uint64_t wp = vcf_word(masks[level][0], j), wo = vcf_word(masks[level][1], j);
      if (wp && first_five < 0) first_five = j * WAVE + __builtin_ctzll(wp);
      if (wo) {
        if (fo_count == 0) fo_cell = j * WAVE + __builtin_ctzll(wo);
        fo_count += __popcll(wo);
      }
    }
    if (first_five >= 0) {  // 2. the attacker completes a five
      st = 1;
      len = level + 1;
      mv = level ? played[0][0] : first_five;
      break;
    }
    // 3.-5. the candidates: none, the fours, or the one four that blocks
    if (lane == 0)
      for (int j = 0; j < nj; ++j) {
        uint64_t w = leaf || fo_count >= 2 ? 0 : (uint64_t)masks[level][2][2 * j + 1] << 32 | masks[level][2][2 * j];
        if (fo_count == 1) w = j == fo_cell / WAVE ? w & (1ull << (fo_cell % WAVE)) : 0;
        cand[level][j] = w;
      }
    __syncthreads();
    bool done = false;
    for (;;) {  // 6. the next candidate of this level, or back to the level above
      int c = -1;
      for (int j = 0; j < nj; ++j) {
        const uint64_t w = vcf_uniform(cand[level][j]);
        if (w) {
          c = j * WAVE + __builtin_ctzll(w);
          if (lane == 0) cand[level][j] = w & (w - 1);
          break;
        }
      }
      if (c < 0) {  // 7. no candidate won
        if (level == 0) {
          done = true;
          break;
        }
        --level;
        flip(played[level][0], played[level][1]);
        __syncthreads();
        continue;
      }
      const int inf = __builtin_amdgcn_readfirstlane((int)info[level][c]), e = inf & (MAX_A - 1);
      if (inf & VCF_MULTI) {  // a double four
        st = 1;
        len = level + 2;
        mv = level ? played[0][0] : c;
        done = true;
        break;
      }
      flip(c, e);
      if (lane == 0) {
        played[level][0] = (int16_t)c;
        played[level][1] = (int16_t)e;
      }
      ++level;
      __syncthreads();
      break;
    }
    if (done) break;
  }
  if (lane == 0) {
    status[g] = (int8_t)st;
    moves[g] = mv;
    if (lengths) lengths[g] = len;
    if (nodes) nodes[g] = count;
    if (actions && st == 1) actions[g] = mv;
  }
}

}  // namespace gmz

GMZ_EXPORT int gmz_game_vcf(const int8_t *boards, const int8_t *players, const int32_t *game, int G, int size,
                            int n_in_row, int max_depth, int max_nodes, int8_t *status, size_t status_bytes,
                            int32_t *moves, size_t moves_bytes, int32_t *lengths, size_t lengths_bytes, int32_t *nodes,
                            size_t nodes_bytes, int32_t *actions, size_t actions_bytes, void *stream) {
  if (G <= 0) return fail("gmz_game_vcf: bad shape: G must be >= 1");
  if (size <= 0 || size * size > MAX_A)
    return fail("gmz_game_vcf: bad shape: size must be >= 1 and size * size <= 512");
  if (n_in_row < 3 || n_in_row > size) return fail("gmz_game_vcf: n_in_row must be in [3, size]");
  if (max_depth < 1 || max_depth > VCF_MAX_DEPTH) return fail("gmz_game_vcf: max_depth must be in [1, 16]");
  if (max_nodes < 1 || max_nodes > VCF_MAX_NODES) return fail("gmz_game_vcf: max_nodes must be in [1, 1048576]");
  if (!boards || !players || !status || !moves)
    return fail(std::string("gmz_game_vcf: null ") +
                (!boards ? "boards" : !players ? "players" : !status ? "status" : "moves"));
  const struct {
    const char *name;
    const void *p;
    size_t have, each;
  } bufs[5] = {{"status", status, status_bytes, 1}, {"moves", moves, moves_bytes, 4},
               {"lengths", lengths, lengths_bytes, 4}, {"nodes", nodes, nodes_bytes, 4},
               {"actions", actions, actions_bytes, 4}};
  for (const auto &x : bufs)
    if (x.p && x.have < (size_t)G * x.each)
      return fail(std::string("gmz_game_vcf: ") + x.name + " holds " + std::to_string(x.have) + " bytes, G * " +
                  std::to_string(x.each) + " = " + std::to_string((size_t)G * x.each));
  hipLaunchKernelGGL(k_vcf, dim3(G), dim3(WAVE), 0, (hipStream_t)stream, boards, players, game, size, n_in_row,
                     max_depth, max_nodes, status, moves, lengths, nodes, actions);
  GMZ_LAUNCH_CHECK();
  return 0;
}

namespace gmz {

constexpr int AB_MAX_PLIES = 8, AB_MAX_WIDTH = 16, AB_MAX_NODES = 1 << 20, AB_MAX_N = 8;
constexpr int64_t AB_WIN = 1ll << 40, AB_INF = 1ll << 50;
// log2 of W_own[m] and of W_opp[m] (m = 0..4, five bits each); W_opp[4] is 0 and is left out by the caller
constexpr uint32_t AB_OWN_SHIFTS = 26u | 13u << 5 | 6u << 10 | 2u << 15 | 0u << 20;
constexpr uint32_t AB_OPP_SHIFTS = 20u | 10u << 5 | 5u << 10 | 1u << 15;

// The threat rule's score (k_anchor_move's) of the empty cell (r0, c0) for the side whose stones are
// lines[so], read from the bit lines as vcf_cell reads them: per direction a shifted piece of two line words, each
// window a run of n bits whose stones are two popcounts.
__device__ __forceinline__ int64_t ab_score(const uint32_t (*lines)[4][VCF_LINES], int size, int n, int r0, int c0,
                                            int so) {
  const int dr[4] = {0, 1, 1, 1}, dc[4] = {1, 0, 1, -1};
  const uint32_t run = (1u << n) - 1;
  int64_t sc = 0;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    int back = n - 1, fwd = n - 1;
    if (dr[d]) {
      back = min(back, r0);
      fwd = min(fwd, size - 1 - r0);
    }
    if (dc[d] > 0) {
      back = min(back, c0);
      fwd = min(fwd, size - 1 - c0);
    } else if (dc[d] < 0) {
      back = min(back, size - 1 - c0);
      fwd = min(fwd, c0);
    }
    if (back + fwd < n - 1) continue;  // no window through the cell lies on the board
    int line, pos;
    vcf_line(d, r0, c0, size, line, pos);
    const uint32_t span = (2u << (back + fwd)) - 1;  // back + fwd + 1 <= size bits
    const uint32_t own = (lines[so][d][line] >> (pos - back)) & span;
    const uint32_t opp = (lines[so ^ 1][d][line] >> (pos - back)) & span;
    for (int w = 0; w <= back + fwd - (n - 1); ++w) {  // the window of bits [w, w + n)
      const uint32_t wm = run << w;
      const int n_own = __popc(own & wm), n_opp = __popc(opp & wm);
      if (n_opp == 0) sc += 1ll << ((AB_OWN_SHIFTS >> (5 * min(n - 1 - n_own, 4))) & 31);
      if (n_own == 0 && n - 1 - n_opp < 4) sc += 1ll << ((AB_OPP_SHIFTS >> (5 * (n - 1 - n_opp))) & 31);
    }
  }
  return sc;
}

// The depth-limited alpha-beta anchor of DESIGN.md §8b for G boards, shaped like k_vcf: one wave per board, a workgroup
// of one wave, the board as k_vcf's bit lines in LDS, lane l owning the cells l, l + 64, ... (up to 8).  The search is
// serial and wave-uniform (every branch is taken on a value all lanes hold: a wave reduction made uniform, or a word
// all lanes read from LDS); a node's work is wide.  Every node takes one pass over the windows (lane l: the windows
// that start on its cells, four per cell), which gives five(b, s) by its smallest cell and the static value E(b, s);
// a node that goes on scores its empty cells (ab_score) and picks the ``width`` best with one wave butterfly each over
// the 64-bit key score << 9 | 511 - cell (the root: over (key, noise, -cell) with the double key of k_anchor_move).
// Nothing is kept from node to node but the board and, per level, alpha, beta, best and the candidates, all in LDS:
// an explicit stack, no recursion, no scratch, no global memory but the inputs and outputs, and no atomics but the
// LDS ORs that build the bit lines.  Each turn of the outer loop counts a node, so max_nodes bounds the launch.
__global__ void __launch_bounds__(WAVE) k_alphabeta(const int8_t *__restrict__ boards, const int8_t *__restrict__ players,
                                                    const int32_t *__restrict__ game, const double *__restrict__ noise,
                                                    double scale, int size, int n, int plies, int width, int max_nodes,
                                                    int8_t *__restrict__ status, int32_t *__restrict__ moves,
                                                    int64_t *__restrict__ values, int32_t *__restrict__ nodes,
                                                    int32_t *__restrict__ actions) {
  __shared__ uint32_t lines[2][4][VCF_LINES];  // [0]: the stones of p, [1]: of -p
  __shared__ uint16_t rc[MAX_A];               // a cell's row << 8 | column
  __shared__ int64_t s_alpha[AB_MAX_PLIES], s_beta[AB_MAX_PLIES], s_best[AB_MAX_PLIES];
  __shared__ int16_t s_cand[AB_MAX_PLIES][AB_MAX_WIDTH];
  __shared__ int32_t s_count[AB_MAX_PLIES], s_next[AB_MAX_PLIES];  // candidates of the level, and how many were played
  const int g = blockIdx.x, A = size * size, lane = threadIdx.x;
  const int nj = (A + WAVE - 1) / WAVE;
  for (int i = lane; i < 2 * 4 * VCF_LINES; i += WAVE) (&lines[0][0][0])[i] = 0;
  __syncthreads();
  const bool idle = game && game[g] < 0;  // an idle arena slot
  const int p = players[g];
  const int8_t *src = boards + (size_t)g * A;
  int stones = 0;
  if (!idle)
    for (int j = 0; j < nj; ++j) {
      const int i = j * WAVE + lane, v = i < A ? src[i] : 0;
      stones += __popcll(__ballot(v != 0));
      if (i < A) {
        const int r = i / size, c = i - r * size;
        rc[i] = (uint16_t)(r << 8 | c);
        if (v != 0)
          for (int d = 0; d < 4; ++d) {
            int line, pos;
            vcf_line(d, r, c, size, line, pos);
            atomicOr(&lines[v == p ? 0 : 1][d][line], 1u << pos);
          }
      }
    }
  if (idle || stones == A) {  // skipped: actions[g] stays as it is
    if (lane == 0) {
      status[g] = 3;
      moves[g] = -1;
      if (values) values[g] = 0;
      if (nodes) nodes[g] = 0;
    }
    return;
  }
  __syncthreads();
  const int dr[4] = {0, 1, 1, 1}, dc[4] = {1, 0, 1, -1};
  const uint32_t run = (1u << n) - 1;
  // a stone of side so goes on or off cell c: lane d flips its bit in orientation d
  auto flip = [&](int c, int so) {
    if (lane < 4) {
      const int x = rc[c];
      int line, pos;
      vcf_line(lane, x >> 8, x & 255, size, line, pos);
      lines[so][lane][line] ^= 1u << pos;
    }
  };
  int level = 0, count = 0, st = 0, mv = -1;
  int64_t val = 0, alpha = -AB_INF, beta = AB_INF;
  for (;;) {  // value() of the node at ``level`` (= ply; plies - level plies left), side level & 1 to move
    if (++count > max_nodes) {  // 1.
      st = 2;
      break;
    }
    const int so = level & 1;
    bool ends = true;
    int64_t v = 0;
    if (stones + level < A) {  // 2. (else: no empty cell, 0)
      // 3. and 4.: every window by its first cell
      int64_t e = 0;
      int fmin = MAX_A;
#pragma unroll 1
      for (int cell = lane; cell < A; cell += WAVE) {
        const int r = rc[cell] >> 8, c = rc[cell] & 255;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const int re = r + (n - 1) * dr[d], ce = c + (n - 1) * dc[d];
          if (re >= size || ce < 0 || ce >= size) continue;
          int line, pos;
          vcf_line(d, r, c, size, line, pos);
          const uint32_t own = (lines[so][d][line] >> pos) & run, opp = (lines[so ^ 1][d][line] >> pos) & run;
          const int n_own = __popc(own), n_opp = __popc(opp);
          if (n_opp == 0 && n_own > 0) {
            e += 2ll << (3 * (n_own - 1));
            if (n_own == n - 1) fmin = min(fmin, cell + __builtin_ctz(~own & run) * (dr[d] * size + dc[d]));
          } else if (n_own == 0 && n_opp > 0) {
            e -= 1ll << (3 * (n_opp - 1));
          }
        }
      }
      for (int off = WAVE / 2; off > 0; off >>= 1) {
        e += __shfl_xor(e, off);
        fmin = min(fmin, __shfl_xor(fmin, off));
      }
      fmin = __builtin_amdgcn_readfirstlane(fmin);
      if (fmin < MAX_A) {  // 3. the mover completes a five
        if (level == 0) {
          mv = fmin;
          val = AB_WIN;
          break;
        }
        v = AB_WIN - level;
      } else if (level == plies) {  // 4.
        v = (int64_t)vcf_uniform((uint64_t)e);
      } else {
        ends = false;
      }
    }
    if (!ends) {
      // 5. and the candidates of 6.
      int nc = 0;
      if (level == 0) {  // the anchor rule's order: (key, noise, -cell), key = (double)score + scale * noise
        double key[NJ], nz[NJ];
        uint32_t have = 0;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int cell = j * WAVE + lane;
          key[j] = nz[j] = 0.0;
          if (j < nj && cell < A) {
            const int r = rc[cell] >> 8, c = rc[cell] & 255;
            if (vcf_empty(lines, r, c)) {
              nz[j] = noise ? noise[(size_t)g * A + cell] : 0.0;
              key[j] = (double)ab_score(lines, size, n, r, c, so) + scale * nz[j];
              have |= 1u << j;
            }
          }
        }
        for (; nc < width; ++nc) {
          AnchorBest best = {0.0, 0.0, -1};
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            const AnchorBest o = {key[j], nz[j], (have >> j) & 1 ? j * WAVE + lane : -1};
            if (anchor_better(o, best)) best = o;
          }
          for (int off = WAVE / 2; off > 0; off >>= 1) {
            AnchorBest o;
            o.key = __shfl_xor(best.key, off);
            o.noise = __shfl_xor(best.noise, off);
            o.cell = __shfl_xor(best.cell, off);
            if (anchor_better(o, best)) best = o;
          }
          const int c = __builtin_amdgcn_readfirstlane(best.cell);
          if (c < 0) break;
          if ((c & (WAVE - 1)) == lane) have &= ~(1u << (c >> 6));
          if (lane == 0) s_cand[0][nc] = (int16_t)c;
        }
      } else {  // (score, -cell) as one word; 0: no cell (511 - cell > 0 for every cell)
        uint64_t key[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const int cell = j * WAVE + lane;
          key[j] = 0;
          if (j < nj && cell < A) {
            const int r = rc[cell] >> 8, c = rc[cell] & 255;
            if (vcf_empty(lines, r, c))
              key[j] = (uint64_t)ab_score(lines, size, n, r, c, so) << 9 | (uint64_t)(MAX_A - 1 - cell);
          }
        }
        for (; nc < width; ++nc) {
          uint64_t best = 0;
#pragma unroll
          for (int j = 0; j < NJ; ++j) best = key[j] > best ? key[j] : best;
          for (int off = WAVE / 2; off > 0; off >>= 1) {
            const uint64_t o = __shfl_xor((unsigned long long)best, off);
            best = o > best ? o : best;
          }
          best = vcf_uniform(best);
          if (best == 0) break;
#pragma unroll
          for (int j = 0; j < NJ; ++j)
            if (key[j] == best) key[j] = 0;
          if (lane == 0) s_cand[level][nc] = (int16_t)(MAX_A - 1 - (int)(best & (MAX_A - 1)));
        }
      }
      if (lane == 0) {
        s_alpha[level] = alpha;
        s_beta[level] = beta;
        s_best[level] = -AB_INF;
        s_count[level] = nc;
        s_next[level] = 0;
      }
      __syncthreads();
    } else {
      // 7. the value goes up, through every level that has no candidate left or is cut off (level >= 1 here: the
      // root has an empty cell, no five and plies >= 1)
      bool done = false;
      for (;;) {
        --level;
        const int next = __builtin_amdgcn_readfirstlane(s_next[level]);
        const int nc = __builtin_amdgcn_readfirstlane(s_count[level]);
        const int c = __builtin_amdgcn_readfirstlane((int)s_cand[level][next - 1]);
        flip(c, level & 1);
        v = -v;
        int64_t a = (int64_t)vcf_uniform((uint64_t)s_alpha[level]), best = (int64_t)vcf_uniform((uint64_t)s_best[level]);
        const int64_t b = (int64_t)vcf_uniform((uint64_t)s_beta[level]);
        if (v > best) {
          best = v;
          if (level == 0) mv = c;
        }
        if (v > a) a = v;
        __syncthreads();
        if (lane == 0) {
          s_best[level] = best;
          s_alpha[level] = a;
        }
        __syncthreads();
        if (a < b && next < nc) break;  // 6. the next candidate of this level
        if (level == 0) {
          val = best;
          done = true;
          break;
        }
        v = best;
      }
      if (done) break;
    }
    // 6. the next candidate of ``level`` goes on the board
    const int next = __builtin_amdgcn_readfirstlane(s_next[level]);
    const int c = __builtin_amdgcn_readfirstlane((int)s_cand[level][next]);
    alpha = -(int64_t)vcf_uniform((uint64_t)s_beta[level]);
    beta = -(int64_t)vcf_uniform((uint64_t)s_alpha[level]);
    __syncthreads();
    if (lane == 0) s_next[level] = next + 1;
    flip(c, level & 1);
    ++level;
    __syncthreads();
  }
  if (lane == 0) {
    status[g] = (int8_t)st;
    moves[g] = st == 0 ? mv : -1;
    if (values) values[g] = st == 0 ? val : 0;
    if (nodes) nodes[g] = count;
    if (actions && st == 0) actions[g] = mv;
  }
}

}  // namespace gmz

GMZ_EXPORT int gmz_game_alphabeta(const int8_t *boards, const int8_t *players, const int32_t *game, const double *noise,
                                  size_t noise_bytes, double scale, int G, int size, int n_in_row, int plies, int width,
                                  int max_nodes, int8_t *status, size_t status_bytes, int32_t *moves, size_t moves_bytes,
                                  int64_t *values, size_t values_bytes, int32_t *nodes, size_t nodes_bytes,
                                  int32_t *actions, size_t actions_bytes, void *stream) {
  if (G <= 0) return fail("gmz_game_alphabeta: bad shape: G must be >= 1");
  if (size <= 0 || size * size > MAX_A)
    return fail("gmz_game_alphabeta: bad shape: size must be >= 1 and size * size <= 512");
  if (n_in_row < 3 || n_in_row > size || n_in_row > AB_MAX_N)
    return fail("gmz_game_alphabeta: n_in_row must be in [3, min(size, 8)]");
  if (plies < 1 || plies > AB_MAX_PLIES) return fail("gmz_game_alphabeta: plies must be in [1, 8]");
  if (width < 1 || width > AB_MAX_WIDTH) return fail("gmz_game_alphabeta: width must be in [1, 16]");
  if (max_nodes < 1 || max_nodes > AB_MAX_NODES) return fail("gmz_game_alphabeta: max_nodes must be in [1, 1048576]");
  if (!(scale >= 0.0) || !std::isfinite(scale)) return fail("gmz_game_alphabeta: scale must be finite and >= 0");
  if (!boards || !players || !status || !moves)
    return fail(std::string("gmz_game_alphabeta: null ") +
                (!boards ? "boards" : !players ? "players" : !status ? "status" : "moves"));
  const size_t A = (size_t)size * size;
  const struct {
    const char *name, *unit;
    const void *p;
    size_t have, each;
  } bufs[6] = {{"noise", "G * A * 8", noise, noise_bytes, A * 8}, {"status", "G * 1", status, status_bytes, 1},
               {"moves", "G * 4", moves, moves_bytes, 4},         {"values", "G * 8", values, values_bytes, 8},
               {"nodes", "G * 4", nodes, nodes_bytes, 4},         {"actions", "G * 4", actions, actions_bytes, 4}};
  for (const auto &x : bufs)
    if (x.p && x.have < (size_t)G * x.each)
      return fail(std::string("gmz_game_alphabeta: ") + x.name + " holds " + std::to_string(x.have) + " bytes, " +
                  x.unit + " = " + std::to_string((size_t)G * x.each));
  hipLaunchKernelGGL(k_alphabeta, dim3(G), dim3(WAVE), 0, (hipStream_t)stream, boards, players, game, noise, scale, size,
                     n_in_row, plies, width, max_nodes, status, moves, values, nodes, actions);
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
