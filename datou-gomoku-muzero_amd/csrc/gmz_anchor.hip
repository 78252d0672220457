// gmz_anchor.hip — the arena's fixed non-network opponents for gfx950, integer work but the key.
//   k_anchor_move   gmz_game_anchor_move   the threat rule and the uniform rule: one workgroup per board, a thread per cell
//   k_vcf           gmz_game_vcf           the forced-win solver: one wave per board, the board as bit lines
//   k_alphabeta     gmz_game_alphabeta     the depth-limited alpha-beta search: one wave per board, the same bit lines
// Shared by the three: the threat rule's weights (threat_window), the arg-max over (key, noise, -cell) (AnchorBest),
// the skipped board's outputs and the C boundary's checks; by the two searches: gmz_lines.h.
#include "gmz_common.h"
#include "gmz_lines.h"

namespace gmz {

// log2 of the threat rule's W_own[m] and W_opp[m], m = 0..4 the stones a window still lacks once the cell is taken (five
// bits each, m = 0 lowest); W_opp[4] is 0, no power of two, and is left out.
constexpr uint32_t W_OWN_LOG2 = 26u | 13u << 5 | 6u << 10 | 2u << 15 | 0u << 20;
constexpr uint32_t W_OPP_LOG2 = 20u | 10u << 5 | 5u << 10 | 1u << 15;

// What a window of n cells through an empty cell adds to the cell's score: the window holds n_own stones of the mover
// and n_opp of the opponent, and counts for a side while the other has no stone in it.
__device__ __forceinline__ int64_t threat_window(int n, int n_own, int n_opp) {
  int64_t sc = 0;
  if (n_opp == 0) sc += 1ll << ((W_OWN_LOG2 >> (5 * min(n - 1 - n_own, 4))) & 31);
  if (n_own == 0 && n - 1 - n_opp < 4) sc += 1ll << ((W_OPP_LOG2 >> (5 * (n - 1 - n_opp))) & 31);
  return sc;
}

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

__device__ __forceinline__ AnchorBest anchor_wave_best(AnchorBest best) {  // the wave's best, in every lane
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    AnchorBest o;
    o.key = __shfl_xor(best.key, off);
    o.noise = __shfl_xor(best.noise, off);
    o.cell = __shfl_xor(best.cell, off);
    if (anchor_better(o, best)) best = o;
  }
  return best;
}

// A search's outputs for a board it skips (lane 0 writes them); actions[g] stays as it is.
template <typename T>
__device__ __forceinline__ void skip_board(int lane, int g, int8_t *status, int32_t *moves, T *extra, int32_t *nodes) {
  if (lane != 0) return;
  status[g] = 3;
  moves[g] = -1;
  if (extra) extra[g] = 0;
  if (nodes) nodes[g] = 0;
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
            sc += threat_window(n_in_row, own, opp);
          }
      }
      const double nz = noise ? noise[(size_t)g * A + cell] : 0.0;
      best.key = (double)sc + scale * nz;
      best.noise = nz;
      best.cell = cell;
    }
    if (scores) scores[(size_t)g * A + cell] = sc;
  }
  best = anchor_wave_best(best);
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

constexpr int VCF_MAX_DEPTH = 16, VCF_MAX_NODES = 1 << 20;
constexpr int VCF_MULTI = 0x4000;  // info bit: T(c) holds two or more cells (a cell index is below 512)

// What the empty cell (r0, c0) is in one node of the forced-win search, by walk_windows over the
// attacker's (side 0) and the defender's lines.  five_p / five_o: a window with n-1 stones of the attacker / of the
// defender (the cell is its one other cell); four: a window with n-2 attacker stones, no defender stone and so one
// more empty cell e; e1 the first such e, multi: another window gave a different e.  A direction with fewer than n-2
// attacker and fewer than n-1 defender stones in reach has none of these and is left out.
__device__ __forceinline__ void vcf_cell(const uint32_t (*lines)[4][LINES], int size, int n, int r0, int c0,
                                         bool &five_p, bool &five_o, bool &four, bool &multi, int &e1) {
  const int cell = r0 * size + c0;
  walk_windows(
      lines, size, n, r0, c0, 0, [&](uint32_t own, uint32_t opp) { return __popc(own) >= n - 2 || __popc(opp) >= n - 1; },
      [&](int d, int back, int w, uint32_t own, uint32_t, int n_own, int n_opp) {
        five_p |= n_own == n - 1;
        five_o |= n_opp == n - 1;
        if (n_own == n - 2 && n_opp == 0) {
          const int step = (d != 0) * size + (d == 0 || d == 2) - (d == 3);
          const int e = cell + (__builtin_ctz((((1u << n) - 1) << w) & ~own & ~(1u << back)) - back) * step;
          if (!four) e1 = e;
          else if (e != e1) multi = true;
          four = true;
        }
      });
}

// The exact, depth-limited forced-win (VCF) search of DESIGN.md §8b for G boards: one wave per board, a workgroup of
// one wave, so a board at its node budget holds nothing but its own wave.  The search is serial and wave-uniform
// (every branch is taken on a ballot or on a value all lanes read from LDS); a node's work is wide: lane l classifies
// the cells l, l + 64, ... (up to 8), and a ballot per group of 64 cells gives the five and four masks in ascending
// cell order.  Below the root a node differs from the one above it by two stones, so it takes that node's masks and
// replies and classifies again only the cells within n-1 steps of a stone along a line (16 (n-1) cells: one per lane
// at n = 5).  The board (gmz_lines.h), per level the three masks, the candidates left, each four's reply (info) and
// the two stones played are in LDS; nothing is kept in global memory, and the only atomics are LDS ORs and ANDs on the
// bit lines and masks.
__global__ void __launch_bounds__(WAVE) k_vcf(const int8_t *__restrict__ boards, const int8_t *__restrict__ players,
                                              const int32_t *__restrict__ game, int size, int n, int max_depth,
                                              int max_nodes, int8_t *__restrict__ status, int32_t *__restrict__ moves,
                                              int32_t *__restrict__ lengths, int32_t *__restrict__ nodes,
                                              int32_t *__restrict__ actions) {
  __shared__ uint32_t lines[2][4][LINES];
  __shared__ uint16_t rc[MAX_A];                  // a cell's row << 8 | column
  __shared__ int16_t info[VCF_MAX_DEPTH][MAX_A];  // of a four cell c: T(c)'s first cell, | VCF_MULTI
  __shared__ uint32_t masks[VCF_MAX_DEPTH][3][2 * NJ];  // per level five(b, p), five(b, -p), fours(b, p): bit = cell
  __shared__ uint64_t cand[VCF_MAX_DEPTH][NJ];    // the level's candidates not yet tried
  __shared__ int16_t played[VCF_MAX_DEPTH][2];    // the attacker's four and the defender's reply on the board
  const int g = blockIdx.x, A = size * size, lane = threadIdx.x;
  if (game && game[g] < 0) return skip_board(lane, g, status, moves, lengths, nodes);  // an idle arena slot
  load_lines(lines, rc, boards + (size_t)g * A, players[g], size, lane);
  // the attacker's stone goes on or off c0 and the defender's on or off c1: lane s * 4 + d flips side s in orientation d
  auto flip = [&](int c0, int c1) {
    if (lane < 8) flip_stone(lines, rc, size, lane >> 2, lane & 3, lane >> 2 ? c1 : c0);
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
          if (cell_empty(lines, r0, c0)) vcf_cell(lines, size, n, r0, c0, five_p, five_o, four, multi, e1);
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
        if (!self && cell_empty(lines, r, c)) vcf_cell(lines, size, n, r, c, five_p, five_o, four, multi, e1);
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
      const uint64_t wp = mask_word(masks[level][0], j), wo = mask_word(masks[level][1], j);
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
        const uint64_t w = uniform64(cand[level][j]);
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

constexpr int AB_MAX_PLIES = 8, AB_MAX_WIDTH = 16, AB_MAX_NODES = 1 << 20, AB_MAX_N = 8;
constexpr int64_t AB_WIN = 1ll << 40, AB_INF = 1ll << 50;

// The threat rule's score (k_anchor_move's) of the empty cell (r0, c0) for the side whose stones are
// lines[so], by walk_windows over every direction.
__device__ __forceinline__ int64_t ab_score(const uint32_t (*lines)[4][LINES], int size, int n, int r0, int c0, int so) {
  int64_t sc = 0;
  walk_windows(
      lines, size, n, r0, c0, so, [](uint32_t, uint32_t) { return true; },
      [&](int, int, int, uint32_t, uint32_t, int n_own, int n_opp) { sc += threat_window(n, n_own, n_opp); });
  return sc;
}

// The depth-limited alpha-beta anchor of DESIGN.md §8b for G boards, shaped like k_vcf: one wave per board, a workgroup
// of one wave, the board as bit lines in LDS (gmz_lines.h), lane l owning the cells l, l + 64, ... (up to 8).  The search
// is serial and wave-uniform (every branch is taken on a value all lanes hold: a wave reduction made uniform, or a word
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
  __shared__ uint32_t lines[2][4][LINES];  // [0]: the stones of p, [1]: of -p
  __shared__ uint16_t rc[MAX_A];           // a cell's row << 8 | column
  __shared__ int64_t s_alpha[AB_MAX_PLIES], s_beta[AB_MAX_PLIES], s_best[AB_MAX_PLIES];
  __shared__ int16_t s_cand[AB_MAX_PLIES][AB_MAX_WIDTH];
  __shared__ int32_t s_count[AB_MAX_PLIES], s_next[AB_MAX_PLIES];  // candidates of the level, and how many were played
  const int g = blockIdx.x, A = size * size, lane = threadIdx.x;
  const int nj = (A + WAVE - 1) / WAVE;
  if (game && game[g] < 0) return skip_board(lane, g, status, moves, values, nodes);  // an idle arena slot
  const int stones = load_lines(lines, rc, boards + (size_t)g * A, players[g], size, lane);
  if (stones == A) return skip_board(lane, g, status, moves, values, nodes);  // a full board
  const int dr[4] = {0, 1, 1, 1}, dc[4] = {1, 0, 1, -1};
  const uint32_t run = (1u << n) - 1;
  auto flip = [&](int c, int so) {  // a stone of side so goes on or off cell c: lane d flips it in orientation d
    if (lane < 4) flip_stone(lines, rc, size, so, lane, c);
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
          line_of(d, r, c, size, line, pos);
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
        v = (int64_t)uniform64((uint64_t)e);
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
            if (cell_empty(lines, r, c)) {
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
          const int c = __builtin_amdgcn_readfirstlane(anchor_wave_best(best).cell);
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
            if (cell_empty(lines, r, c))
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
          best = uniform64(best);
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
        int64_t a = (int64_t)uniform64((uint64_t)s_alpha[level]), best = (int64_t)uniform64((uint64_t)s_best[level]);
        const int64_t b = (int64_t)uniform64((uint64_t)s_beta[level]);
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
    alpha = -(int64_t)uniform64((uint64_t)s_beta[level]);
    beta = -(int64_t)uniform64((uint64_t)s_alpha[level]);
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

// ---------------------------------------------------------------------------------------------- the C boundary
// The refusals come in one order: shape, limits, nulls, bytes.
struct HeldBytes {
  const char *name, *unit;  // unit: the text of ``each`` times G
  const void *p;            // null: an optional buffer that is absent, not checked
  size_t have, each;
};

template <size_t N>
static int check_bytes(const char *fn, int G, const HeldBytes (&bufs)[N]) {
  for (const HeldBytes &x : bufs)
    if (x.p && x.have < (size_t)G * x.each)
      return fail(std::string(fn) + ": " + x.name + " holds " + std::to_string(x.have) + " bytes, " + x.unit + " = " +
                  std::to_string((size_t)G * x.each));
  return 0;
}

static int check_shape(const std::string &fn, int G, int size) {  // the two searches' wording
  if (G <= 0) return fail(fn + ": bad shape: G must be >= 1");
  if (size <= 0 || size * size > MAX_A) return fail(fn + ": bad shape: size must be >= 1 and size * size <= 512");
  return 0;
}

static int check_nulls(const std::string &fn, const void *boards, const void *players, const void *status,
                       const void *moves) {
  if (boards && players && status && moves) return 0;
  return fail(fn + ": null " + (!boards ? "boards" : !players ? "players" : !status ? "status" : "moves"));
}

}  // namespace gmz

using namespace gmz;

GMZ_EXPORT int gmz_game_anchor_move(const int8_t *boards, const int8_t *players, const int32_t *game, const double *noise,
                                    size_t noise_bytes, int G, int size, int n_in_row, int kind, double scale,
                                    int32_t *actions, size_t actions_bytes, int64_t *scores, size_t scores_bytes,
                                    void *stream) {
  if (G <= 0 || size <= 0 || size * size > MAX_A) return fail("gmz_game_anchor_move: bad shape");
  if (n_in_row < 1 || n_in_row > size) return fail("gmz_game_anchor_move: n_in_row must be in [1, size]");
  if (kind != 0 && kind != 1) return fail("gmz_game_anchor_move: kind must be 0 (threat) or 1 (uniform)");
  if (!(scale >= 0.0) || !std::isfinite(scale)) return fail("gmz_game_anchor_move: scale must be finite and >= 0");
  if (!boards || !players || !actions) return fail("gmz_game_anchor_move: null boards, players or actions");
  const size_t A = (size_t)size * size;
  const HeldBytes bufs[] = {{"noise", "G * A * 8", noise, noise_bytes, A * 8},
                            {"actions", "G * 4", actions, actions_bytes, 4},
                            {"scores", "G * A * 8", scores, scores_bytes, A * 8}};
  if (check_bytes("gmz_game_anchor_move", G, bufs)) return -1;
  const int threads = A <= 256 ? 256 : 512;
  hipLaunchKernelGGL(k_anchor_move, dim3(G), dim3(threads), 0, (hipStream_t)stream, boards, players, game, noise, size,
                     n_in_row, kind, scale, actions, scores);
  GMZ_LAUNCH_CHECK();
  return 0;
}

GMZ_EXPORT int gmz_game_vcf(const int8_t *boards, const int8_t *players, const int32_t *game, int G, int size,
                            int n_in_row, int max_depth, int max_nodes, int8_t *status, size_t status_bytes,
                            int32_t *moves, size_t moves_bytes, int32_t *lengths, size_t lengths_bytes, int32_t *nodes,
                            size_t nodes_bytes, int32_t *actions, size_t actions_bytes, void *stream) {
  if (check_shape("gmz_game_vcf", G, size)) return -1;
  if (n_in_row < 3 || n_in_row > size) return fail("gmz_game_vcf: n_in_row must be in [3, size]");
  if (max_depth < 1 || max_depth > VCF_MAX_DEPTH) return fail("gmz_game_vcf: max_depth must be in [1, 16]");
  if (max_nodes < 1 || max_nodes > VCF_MAX_NODES) return fail("gmz_game_vcf: max_nodes must be in [1, 1048576]");
  if (check_nulls("gmz_game_vcf", boards, players, status, moves)) return -1;
  const HeldBytes bufs[] = {{"status", "G * 1", status, status_bytes, 1},
                            {"moves", "G * 4", moves, moves_bytes, 4},
                            {"lengths", "G * 4", lengths, lengths_bytes, 4},
                            {"nodes", "G * 4", nodes, nodes_bytes, 4},
                            {"actions", "G * 4", actions, actions_bytes, 4}};
  if (check_bytes("gmz_game_vcf", G, bufs)) return -1;
  hipLaunchKernelGGL(k_vcf, dim3(G), dim3(WAVE), 0, (hipStream_t)stream, boards, players, game, size, n_in_row,
                     max_depth, max_nodes, status, moves, lengths, nodes, actions);
  GMZ_LAUNCH_CHECK();
  return 0;
}

GMZ_EXPORT int gmz_game_alphabeta(const int8_t *boards, const int8_t *players, const int32_t *game, const double *noise,
                                  size_t noise_bytes, double scale, int G, int size, int n_in_row, int plies, int width,
                                  int max_nodes, int8_t *status, size_t status_bytes, int32_t *moves, size_t moves_bytes,
                                  int64_t *values, size_t values_bytes, int32_t *nodes, size_t nodes_bytes,
                                  int32_t *actions, size_t actions_bytes, void *stream) {
  if (check_shape("gmz_game_alphabeta", G, size)) return -1;
  if (n_in_row < 3 || n_in_row > size || n_in_row > AB_MAX_N)
    return fail("gmz_game_alphabeta: n_in_row must be in [3, min(size, 8)]");
  if (plies < 1 || plies > AB_MAX_PLIES) return fail("gmz_game_alphabeta: plies must be in [1, 8]");
  if (width < 1 || width > AB_MAX_WIDTH) return fail("gmz_game_alphabeta: width must be in [1, 16]");
  if (max_nodes < 1 || max_nodes > AB_MAX_NODES) return fail("gmz_game_alphabeta: max_nodes must be in [1, 1048576]");
  if (!(scale >= 0.0) || !std::isfinite(scale)) return fail("gmz_game_alphabeta: scale must be finite and >= 0");
  if (check_nulls("gmz_game_alphabeta", boards, players, status, moves)) return -1;
  const HeldBytes bufs[] = {{"noise", "G * A * 8", noise, noise_bytes, (size_t)size * size * 8},
                            {"status", "G * 1", status, status_bytes, 1},
                            {"moves", "G * 4", moves, moves_bytes, 4},
                            {"values", "G * 8", values, values_bytes, 8},
                            {"nodes", "G * 4", nodes, nodes_bytes, 4},
                            {"actions", "G * 4", actions, actions_bytes, 4}};
  if (check_bytes("gmz_game_alphabeta", G, bufs)) return -1;
  hipLaunchKernelGGL(k_alphabeta, dim3(G), dim3(WAVE), 0, (hipStream_t)stream, boards, players, game, noise, scale, size,
                     n_in_row, plies, width, max_nodes, status, moves, values, nodes, actions);
  GMZ_LAUNCH_CHECK();
  return 0;
}
