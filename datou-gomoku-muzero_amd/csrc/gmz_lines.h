// gmz_lines.h — the bit-line board of the anchor opponents' searches (gmz_anchor.hip; internal, like gmz_device.h).
//
// lines[s][d][l] holds the stones of side s (0: the player to move at the root, 1: the other) on line l of orientation
// d (0: (0,1), 1: (1,0), 2: (1,1), 3: (1,-1)), so that a cell reads two words per direction and a window of n cells is a
// run of n bits.  The arrays are the kernels' own __shared__ ones; everything here takes pointers to them.
#pragma once
#include "gmz_common.h"

namespace gmz {

constexpr int LINES = 2 * 22 - 1;  // lines of one orientation on the largest board: its 43 diagonals

__device__ __forceinline__ uint64_t uniform64(uint64_t x) {  // a wave-uniform 64-bit value, in scalar registers
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(x >> 32)) << 32) |
         (uint32_t)__builtin_amdgcn_readfirstlane((int)x);
}

// Cells j * 64 .. j * 64 + 63 of a cell mask kept as 32-bit words in LDS, wave-uniform.
__device__ __forceinline__ uint64_t mask_word(const uint32_t *mask, int j) {
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)mask[2 * j + 1]) << 32) |
         (uint32_t)__builtin_amdgcn_readfirstlane((int)mask[2 * j]);
}

// The line of orientation d through cell (r, c) and the cell's bit in it.  A step along the direction raises the bit
// index by one: the index is the column in a row and the row elsewhere.
__device__ __forceinline__ void line_of(int d, int r, int c, int size, int &line, int &pos) {
  line = d == 0 ? r : d == 1 ? c : d == 2 ? r - c + size - 1 : r + c;
  pos = d == 0 ? c : r;
}

__device__ __forceinline__ bool cell_empty(const uint32_t (*lines)[4][LINES], int r, int c) {
  return !(((lines[0][0][r] | lines[1][0][r]) >> c) & 1);
}

// One wave builds the board of ``src`` (player p's stones are side 0): zeroes the lines, fills rc[cell] = row << 8 |
// column, ORs the stones in and returns how many there are, counted from the finished rows, which hold each stone once
// (wave-uniform).  The lines are complete on return.
__device__ __forceinline__ int load_lines(uint32_t (*lines)[4][LINES], uint16_t *rc, const int8_t *src, int p, int size,
                                          int lane) {
  for (int i = lane; i < 2 * 4 * LINES; i += WAVE) (&lines[0][0][0])[i] = 0;
  __syncthreads();
  for (int i = lane; i < size * size; i += WAVE) {
    const int r = i / size, c = i - r * size, v = src[i];
    rc[i] = (uint16_t)(r << 8 | c);
    if (v != 0)
      for (int d = 0; d < 4; ++d) {
        int line, pos;
        line_of(d, r, c, size, line, pos);
        atomicOr(&lines[v == p ? 0 : 1][d][line], 1u << pos);
      }
  }
  __syncthreads();
  return wave_sum_i(lane < size ? __popc(lines[0][0][lane] | lines[1][0][lane]) : 0);
}

// A stone of side s goes on or off the cell: the calling lane flips its bit in orientation d (one lane per (s, d)).
__device__ __forceinline__ void flip_stone(uint32_t (*lines)[4][LINES], const uint16_t *rc, int size, int s, int d,
                                           int cell) {
  const int x = rc[cell];
  int line, pos;
  line_of(d, x >> 8, x & 255, size, line, pos);
  lines[s][d][line] ^= 1u << pos;
}

// The windows of n cells through the empty cell (r0, c0), for the side whose stones are lines[so].  Per direction the
// cells of the line at most n-1 steps from the cell, as far as the board goes (back against the direction, fwd along
// it), are a shifted piece of two line words (bit k + back = the cell k steps along; back + fwd + 1 <= size bits), and
// every window that holds the cell is a run of n bits in it.  A direction with a window on the board is offered to
// dir(own, opp), which may turn it down; each of its windows, the bits [w, w + n), then goes to
// win(d, back, w, own, opp, n_own, n_opp) with the stones of either side in it counted.
template <typename Dir, typename Win>
__device__ __forceinline__ void walk_windows(const uint32_t (*lines)[4][LINES], int size, int n, int r0, int c0, int so,
                                             Dir &&dir, Win &&win) {
  const int dr[4] = {0, 1, 1, 1}, dc[4] = {1, 0, 1, -1};
  const uint32_t run = (1u << n) - 1;
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
    line_of(d, r0, c0, size, line, pos);
    const uint32_t span = (2u << (back + fwd)) - 1;
    const uint32_t own = (lines[so][d][line] >> (pos - back)) & span;
    const uint32_t opp = (lines[so ^ 1][d][line] >> (pos - back)) & span;
    if (!dir(own, opp)) continue;
    for (int w = 0; w <= back + fwd - (n - 1); ++w) {
      const uint32_t wm = run << w;
      win(d, back, w, own, opp, __popc(own & wm), __popc(opp & wm));
    }
  }
}

}  // namespace gmz
