// gmz_conv.hip — the trainer's 128 -> 128 3x3 convolutions (residual-block convs of GomokuNetEZ,
// network.py:30-48) as implicit-GEMM MFMA kernels on channels-last (NHWC) f16/bf16 activations.
//
// Forward y = conv(x, W) and the input gradient dx = conv(dy, W') (W'[c][o][t] = W[o][c][8 - t]:
// channels swapped, taps flipped) are the same kernel on differently packed weights; the weight
// gradient is k_conv3_wgrad + k_conv3_wgrad_reduce (below).  Replaces, for these layers, MIOpen's NHWC
// kernels plus the zeroing pass it runs before each of them (trainer.py, training step of
// loss.py:30-158).
//
// Work item = (board, half of the output channels; the halves on one XCD): 2N items for N boards, so the 256 CUs see ~3
// rounds at N = 360 instead of 1.4.  Two 256-thread workgroups per CU (one padded image each,
// 78 KB at 15x15).  Per item: the board's NHWC activations are DMA'd (global_load_lds) into the
// padded LDS image of k_tower3 (gmz_net.hip: cell (yy, xx) at yy*RS + xx*PS, conflict-free
// ds_read_b128 B fragments, every tap / k-step offset an immediate), then 36 k-steps (9 taps x 4
// k-steps of 32 input channels) of v_mfma_f32_16x16x32_{f16,bf16}: 4 waves = 2 groups of 2 n-tiles
// x 2 position groups of 8|7 16-position tiles (16 MFMAs per 2 weight-fragment loads per k-step:
// 4 tiles per wave ran into the vector-L1 bandwidth, 256 B of weights per MFMA).  A fragments (weights) stream global -> VGPR
// through a 3-deep register ring, shared by the waves of a channel group in L1.  Epilogue: f32 ->
// activation dtype, 8-byte stores of 4 consecutive channels.
// Board sizes: 6, 9, 15 and 19 (ConvSizes below; per-size position groups and residency in ConvCfg<H>).  At 19x19 the
// image is 117 KB, so one workgroup per CU; the weight gradient there stages each board in two row bands (WgLds).
// k_conv3_split (below k_conv3) is the same convolution on float32 activations with split-f16 operands, float32-grade:
// the target network's value trunk (gmz_conv3x3_forward_split).
#include <initializer_list>
#include <type_traits>

#include "gmz_common.h"

#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

namespace gmz {
namespace {

typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 b16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef uint16_t u16x4_t __attribute__((ext_vector_type(4)));

// depth of the weight-fragment register ring (k-steps in flight from L2): 3, the product; an A/B build sets 4 or 6
#ifndef GMZ_CONV_RD
#define GMZ_CONV_RD 3
#endif
constexpr int CC = 128;         // channels in and out
constexpr int CKSTEPS = 36;     // 9 taps x 4 k-steps of 32 input channels
constexpr int FRAG_BYTES = 294912;  // 36 k-steps x 8 n-tiles x 64 lanes x 16 B

__device__ __forceinline__ int csigma16(int j) { return j < 8 ? (j ^ 4) : j; }

// padded board image (same geometry as Img3 in gmz_net.hip)
template <int H>
struct CImg {
  static constexpr int HP = H + 2, PS = 272, RS = HP * PS - 32;
  static constexpr int BYTES = ((HP - 1) * RS + HP * PS + 255) / 256 * 256;
  static constexpr int RUN = (H - 1) * PS + 256;
  static constexpr int RUN_DMA = (RUN + 1023) / 1024;
};

template <typename T> struct Mfma;
template <> struct Mfma<__half> {
  typedef f16x8_t V;
  static __device__ __forceinline__ f32x4_t run(V a, V b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ uint16_t bits(float f) { return __builtin_bit_cast(uint16_t, (_Float16)f); }
  static __device__ __forceinline__ float value(uint16_t u) { return (float)__builtin_bit_cast(_Float16, u); }
};
template <> struct Mfma<__hip_bfloat16> {
  typedef b16x8_t V;
  static __device__ __forceinline__ f32x4_t run(V a, V b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ uint16_t bits(float f) { return __builtin_bit_cast(uint16_t, (__bf16)f); }
  static __device__ __forceinline__ float value(uint16_t u) { return __uint_as_float(((uint32_t)u) << 16); }
};

// lane group g of k-step s reads input-channel chunk 2s + {0, 8, 1, 9}[g] (8 channels per chunk)
__device__ __forceinline__ int chunk_of(int ks, int g) { return 2 * ks + ((g & 1) * 8 + (g >> 1)); }

// fragment (t, ks, nt, l, j) = Wx[n = nt*16 + (l & 15)][c = chunk_of(ks, l >> 4)*8 + j][t], with
// Wx = W (transpose = 0) or W'[n][c][t] = W[c][n][8 - t] (transpose = 1, the input gradient)
template <typename T>
__global__ void __launch_bounds__(256) k_pack_conv(const float *__restrict__ w, long s0, long s1, long s2, long s3,
                                                   int transpose, uint16_t *__restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;  // (t, ks, nt, l)
  if (i >= CKSTEPS * 8 * 64) return;
  const int l = i & 63, nt = (i >> 6) & 7, st = i >> 9, t = st >> 2, ks = st & 3;
  const int n = nt * 16 + (l & 15);
  u16x4_t lo, hi;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = chunk_of(ks, l >> 4) * 8 + j;
    const int o = transpose ? c : n, ci = transpose ? n : c, tt = transpose ? 8 - t : t;
    const float v = w[o * s0 + ci * s1 + (tt / 3) * s2 + (tt % 3) * s3];
    const uint16_t b = Mfma<T>::bits(v);
    if (j < 4) lo[j] = b;
    else hi[j - 4] = b;
  }
  uint4 r;
  r.x = (uint32_t)lo[0] | ((uint32_t)lo[1] << 16);
  r.y = (uint32_t)lo[2] | ((uint32_t)lo[3] << 16);
  r.z = (uint32_t)hi[0] | ((uint32_t)hi[1] << 16);
  r.w = (uint32_t)hi[2] | ((uint32_t)hi[3] << 16);
  *(uint4 *)(out + (size_t)i * 8) = r;
}

// Many weights packed in ONE launch (the trainer re-packs every cached conv weight right after its optimiser step,
// gmz_conv3x3_pack_many): grid.y = the table entry, grid.x covers one weight's fragments as k_pack_conv does.
struct PackJob {
  const float *w;
  long long s0, s1, s2, s3;
  uint16_t *out;
  int transpose, pad;
};

template <typename T>
__global__ void __launch_bounds__(256) k_pack_many(const PackJob *__restrict__ jobs) {
  const PackJob j = jobs[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;  // (t, ks, nt, l)
  if (i >= CKSTEPS * 8 * 64) return;
  const int l = i & 63, nt = (i >> 6) & 7, st = i >> 9, t = st >> 2, ks = st & 3;
  const int n = nt * 16 + (l & 15);
  u16x4_t lo, hi;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int c = chunk_of(ks, l >> 4) * 8 + e;
    const int o = j.transpose ? c : n, ci = j.transpose ? n : c, tt = j.transpose ? 8 - t : t;
    const uint16_t b = Mfma<T>::bits(j.w[o * j.s0 + ci * j.s1 + (tt / 3) * j.s2 + (tt % 3) * j.s3]);
    if (e < 4) lo[e] = b;
    else hi[e - 4] = b;
  }
  uint4 r;
  r.x = (uint32_t)lo[0] | ((uint32_t)lo[1] << 16);
  r.y = (uint32_t)lo[2] | ((uint32_t)lo[3] << 16);
  r.z = (uint32_t)hi[0] | ((uint32_t)hi[1] << 16);
  r.w = (uint32_t)hi[2] | ((uint32_t)hi[3] << 16);
  *(uint4 *)(j.out + (size_t)i * 8) = r;
}

// The BatchNorm whose backward the output feeds (BWD statistics, gmz_conv3x3_forward_bwdstats): its input
// x, its output y (after its ReLU) and its saved (mean, invstd) f32 [2][128]
struct BnBwd {
  const uint16_t *x, *y;
  const float *save;
  int relu;
};

// The dynamics trunk's first conv (network.py:79-96, 128 hidden + 16 action-embedding planes -> 128): its 16-plane
// part is the embedding of ONE one-hot action cell per board, so its output is a 3x3 stamp around that cell:
// out[o][q] += table[tap][o] where tap = (a - q) + (1, 1) in the 3x3 window, table[tap][o] = sum_c W[o][128 + c][tap]
// * embed[c] (f32).  Added in f32 before the output's single rounding, like the 144-channel conv's accumulation.
struct ActStamp {
  const int32_t *action;  // [N] action cell per board (nullptr: no stamp)
  const float *table;     // [9][128]
};

// The training-mode BatchNorm (+ residual, ReLU) whose output is this conv's input, applied in the board-staging
// prologue instead of a pass of its own (gmz_conv3x3_forward_bnapply; VERDICT r5 next #4, loss.py:70-111's residual
// blocks): the prologue reads the BatchNorm's input z (and the residual), stages relu?((z - mean) * gamma * invstd +
// beta (+ res)) into the LDS image and writes it to out, the normalised activation the backward needs — each of a
// board's two channel-half workgroups its own 64 channels.  Same arithmetic and rounding as k_bnl_apply (gmz_train.hip).
struct BnApply {
  const uint16_t *z, *res;  // [N][A][128] the BatchNorm's input, the residual (or nullptr)
  const float *gamma, *beta, *save;  // save = (mean, invstd) f32 [2][128] (gmz_bn_forward_deferred)
  uint16_t *out;  // [N][A][128] the BatchNorm's output = this conv's input
  int relu;
};

// Board sizes the 3x3 family is built for (forward family and weight gradient): the ONE list the dispatches and their
// error text come from.
template <int... Hs> struct SizeList {};
using ConvSizes = SizeList<6, 9, 15, 19>;

// Per-size configuration of k_conv3 (as TowerCfg<H> in gmz_net.hip).  PG = position groups per workgroup (2 PG waves);
// WG_PER_CU = workgroups of one CU's LDS (the padded image: 17 KB at 6x6, 33 KB at 9x9, 78 KB at 15x15, 117 KB at
// 19x19, where only one fits) = the kernel's minimum-residency launch bound; AB = the off-by-default A/B variants
// (BWD statistics, gmz_conv3x3_forward_bwdstats; the action stamp, gmz_conv3x3_forward_stamp) are built and accepted.
#ifndef GMZ_CONV_PG19
#define GMZ_CONV_PG19 2
#endif
template <int H> struct ConvCfg { static constexpr int PG = 2, WG_PER_CU = 2; static constexpr bool AB = H == 9 || H == 15; };
template <> struct ConvCfg<19> { static constexpr int PG = GMZ_CONV_PG19, WG_PER_CU = 1; static constexpr bool AB = false; };

// (Measured and removed: one workgroup per board computing both channel halves from one DMA — forward 33.9 vs 28.7 us,
// profiles/r04_trainer_ab_defer_target.txt; the next board's DMA issued before the epilogue; the timing ablations of
// profiles/r05_conv_ablations.txt and r06_conv_lds_ab.txt, built from commit 3a54982's gmz_conv.hip with GMZ_CONV_ABL.)
// BWD: the epilogue's statistics are the BatchNorm BACKWARD sums of the output taken as that BN's output
// gradient dy — sum dz and sum dz * xhat, dz = dy * [y > 0], xhat = (x - mean) * invstd (what k_bnl_red<.., 1, ..>
// reduces in a pass of its own) — instead of the forward sums of the output.
// PB: the statistics partials per BOARD (stats [C][N][3], slot = board) instead of per workgroup, so a
// consumer can take them over any board ranges: the trainer's batched consistency trunk (five unroll steps'
// observations as one launch, each step's BatchNorm statistics over its own boards; gmz_bn_forward_seg).
// BNA: the input is staged by the BatchNorm-apply prologue (BnApply ba) instead of the DMA of x.
template <int H, typename T, int PG, bool BWD = false, bool PB = false, bool BNA = false>
__global__ void __launch_bounds__(128 * PG, ConvCfg<H>::WG_PER_CU) k_conv3(const uint16_t *__restrict__ x, const uint16_t *__restrict__ wpk,
                                                  uint16_t *__restrict__ y, int N, const uint8_t *__restrict__ mask,
                                                  double *__restrict__ stats, const uint16_t *__restrict__ addend,
                                                  BnBwd bn, ActStamp as, BnApply ba) {
  using I = CImg<H>;
  using M = Mfma<T>;
  typedef typename M::V V;
  constexpr int A = H * H, NPT = (A + 15) / 16;
  constexpr int NTW = 2, PTW = (NPT + PG - 1) / PG, RD = GMZ_CONV_RD, NW = 2 * PG, NTHR = 64 * NW;
  constexpr int PS = I::PS, RS = I::RS;
  static_assert(CKSTEPS % RD == 0, "ring slots repeat per item");
  // the board's last tile (15x15: the corner cell alone) skips the k-steps whose tap reaches only the zero border
  // (gmz_common.h live_taps); only the PTW-tile k-loop holds it when NPT = PG (PTW - 1) + 1
  // REMAP would be the towers' 15x15 border-tile order (remap15, gmz_common.h): measured slower here (forward 29.0 vs
  // 27.5 us at 360 boards, trainer 40.4 vs 41.0 steps/s, profiles/r06_conv_remap_ab.txt) — this kernel's epilogue
  // stores straight to HBM, 8 B per lane, and a column tile's positions are 15 cells apart: scattered stores.  Off.
  constexpr bool REMAP = false;
  constexpr bool LAST_ONE = !REMAP && NPT == PG * (PTW - 1) + 1;
  constexpr unsigned LAST_TAPS = LAST_ONE ? live_taps(H, (NPT - 1) * 16, A) : 0x1ffu;
  static_assert(LAST_TAPS & 1u, "tap 0 of the last tile starts its accumulation");
  __shared__ __attribute__((aligned(16))) uint8_t img[I::BYTES];
  static_assert(I::BYTES >= PG * 64 * 2 * 4, "stats scratch fits in the image");
  static_assert(!PB || !BWD, "per-board statistics: forward sums");
  static_assert(!BNA || (!BWD && !PB), "BatchNorm-apply prologue: the forward with per-workgroup statistics");
  static_assert(NTHR % 16 == 0, "BNA: a thread's chunk of every cell it stages is tid & 15");
  __shared__ float pbred[PB ? PG * 64 * 2 : 1];  // PB: [PG][64 channels of this half][2], per board

  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int nq = w & 1, pg = w >> 1;
  const int g4 = lane >> 4;
  const int cg = (g4 & 1) * 8 + (g4 >> 1);
  // XCD-aware items: workgroups are dealt to the 8 XCDs round-robin by index, so workgroup i runs on
  // XCD i % 8; the two halves of a board are workgroups i and i ^ 8 (same XCD, dispatched together),
  // and the second one's board DMA is served by that XCD's L2 instead of HBM
  const int half0 = (blockIdx.x >> 3) & 1;
  // first board; also the statistics slot
  const int b0 = (int)((blockIdx.x >> 4) * 8 + (blockIdx.x & 7));
  const int bstride = (int)(gridDim.x >> 1);
  const int ntile0 = half0 * 4 + nq * NTW;  // this wave's first n-tile (of 8)

  // zero the image's border cells (2 HP + 2 H cells; every board's DMA rewrites the whole interior).  Indexed
  // uint4 stores compile to ds_write_b128 (8 lanes = one contiguous 128 B: conflict-free); the round-5 fill of the
  // whole 78 KB image as *(uint4 *)(img + 16 i) compiled to four ds_write_b32 per 16 B at a 16-B lane stride,
  // 4-way bank conflicted: 1.26 M of the kernel's 1.47 M conflict cycles (profiles/r06_conv_lds_ab.txt)
  {
    constexpr int HP = I::HP, NBORDER = 2 * HP + 2 * H;
    for (int i = tid; i < NBORDER * 16; i += NTHR) {
      const int k = i >> 4, r = k - 2 * HP;
      const int yy = k < HP ? 0 : k < 2 * HP ? HP - 1 : 1 + (r >> 1);
      const int xx = k < HP ? k : k < 2 * HP ? k - HP : (r & 1) * (HP - 1);
      ((uint4 *)(img + yy * RS + xx * PS))[i & 15] = make_uint4(0, 0, 0, 0);
    }
  }

  // tile pt, lane -> board position (A: a pad), in raster order or (15x15) the border-tile order
  auto tile_p = [&](int pt) {
    if constexpr (REMAP) {
      const int p = pt < NPT ? remap15(pt, csigma16(lane & 15)) : -1;
      return p < 0 ? A : p;
    }
    const int p = pt * 16 + csigma16(lane & 15);
    return (pt < NPT && p < A) ? p : A;
  };
  int pos[PTW];  // read base of each tile's cell; ~base for a pad (REMAP: a top-border address with the slot's key)
#pragma unroll
  for (int i = 0; i < PTW; ++i) {
    const int pt = pg + PG * i, p = tile_p(pt);
    const int pad = REMAP ? 16 * ((remap15_key0(pt) + csigma16(lane & 15)) & 15)
                          : ((A - 1) / H) * RS + ((A - 1) % H) * PS;  // the last cell: one broadcast address
    pos[i] = p < A ? (p / H) * RS + (p % H) * PS : ~pad;
  }
  const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc((void *)wpk, (short)0, FRAG_BYTES, 0x00020000);
  const int wvoff = ntile0 * 1024 + lane * 16;
  V ar[RD][NTW];
  auto loadA = [&](int slot, int st) {
    const int soff = (st < CKSTEPS ? st : st - CKSTEPS) * 8192;
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt)
      ar[slot][nt] = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, wvoff + nt * 1024, soff, 0));
  };
#pragma unroll
  for (int k = 0; k < RD - 1; ++k) loadA(k, k);
  __syncthreads();  // zeroed image before the first DMA
  // BatchNorm statistics of the (rounded) output over the boards in the mask: per lane, its 4
  // channels of each n-tile summed over its positions and boards
  float s1[NTW][4], s2[NTW][4];
#pragma unroll
  for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
    for (int e = 0; e < 4; ++e) s1[nt][e] = s2[nt][e] = 0.f;
  int nvalid = 0;

  // ---- board bd -> image interior: 1 KB pieces of each board row's run of cells
  auto dma = [&](int bd) {
    const uint8_t *src = (const uint8_t *)(x + (size_t)bd * A * CC);
    for (int j = w; j < H * I::RUN_DMA; j += NW) {
      const int yy = j / I::RUN_DMA, piece = j % I::RUN_DMA;
      const int o = piece * 1024 + lane * 16;
      const int xx = o / PS, ch = (o % PS) >> 4;
      if (o < I::RUN && ch < 16)
        __builtin_amdgcn_global_load_lds((const void *)(src + (yy * H + xx) * 256 + ch * 16),
                                         (__attribute__((address_space(3))) void *)(img + (yy + 1) * RS + PS + piece * 1024),
                                         16, 0, 0);
    }
  };
  // ---- BNA: board bd's BatchNorm output -> image interior (and out).  Thread tid always takes 8-channel chunk
  // tid & 15 of a cell (NTHR is a multiple of 16); its channels' constants are re-read per board (L1 hits: kept live
  // across the k-loop they spilled it), loads of U cells issued before any arithmetic
  auto bn_stage = [&](int bd) {
    // an opaque copy of tid per board: the 15 cells' addresses are re-derived here, not hoisted out of the board loop
    // and kept live across the k-loop (which spilled it)
    int t = tid;
    asm volatile("" : "+v"(t));
    const int bch = t & 15;
    float bmu[8], bsc[8], bsh[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = bch * 8 + j;
      bmu[j] = ba.save[c];
      bsc[j] = ba.gamma[c] * ba.save[CC + c];
      bsh[j] = ba.beta[c];
    }
    constexpr int NCH = A * 16, NI = (NCH + NTHR - 1) / NTHR, U = 8;
    const size_t base = (size_t)bd * NCH;
    const uint4 *zs = (const uint4 *)ba.z + base;
    const uint4 *rs = ba.res ? (const uint4 *)ba.res + base : nullptr;
    uint4 *os = (uint4 *)ba.out + base;
    const bool mine = (bch >> 3) == half0;  // this workgroup's channel half of the output
    // branch-free element math: no residual = adding -0.0 (the identity, signed zeros included), no ReLU = a max
    // with -inf; the same values as k_bnl_apply's conditional forms
    const uint32_t nz = M::bits(-0.f) * 0x10001u;
    const float lo = ba.relu ? 0.f : -__builtin_inff();
#pragma unroll
    for (int i0 = 0; i0 < NI; i0 += U) {
      uint4 zv[U], rv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = t + (i0 + u) * NTHR;
        rv[u] = make_uint4(nz, nz, nz, nz);
        if (i0 + u < NI && i < NCH) {
          zv[u] = zs[i];
          if (rs) rv[u] = rs[i];
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = t + (i0 + u) * NTHR;
        if (!(i0 + u < NI && i < NCH)) continue;
        const uint32_t *zw = (const uint32_t *)&zv[u], *rw = (const uint32_t *)&rv[u];
        uint32_t ow[4];
#pragma unroll
        for (int h = 0; h < 4; ++h) {
          uint32_t packed = 0;
#pragma unroll
          for (int e = 0; e < 2; ++e) {
            const int j = 2 * h + e;
            float v = (M::value((uint16_t)(zw[h] >> (16 * e))) - bmu[j]) * bsc[j] + bsh[j];
            v += M::value((uint16_t)(rw[h] >> (16 * e)));
            v = fmaxf(v, lo);
            packed |= (uint32_t)M::bits(v) << (16 * e);
          }
          ow[h] = packed;
        }
        const uint4 o = make_uint4(ow[0], ow[1], ow[2], ow[3]);
        const int p = i >> 4;
        ((uint4 *)(img + (p / H + 1) * RS + (p % H + 1) * PS))[bch] = o;
        if (mine) os[i] = o;
      }
    }
  };
  // the row-mask bytes of this workgroup's boards, one per lane (lane j: board b0 + j * bstride), loaded once here:
  // read per board, each byte was a vector load with a full round trip of its own between the board's barrier and
  // its first LDS read (profiles/r06_conv_mask_ab.txt)
  int mrow = 1;
  if (mask) {
    const int bj = b0 + lane * bstride;
    mrow = bj < N ? (int)mask[bj] : 0;
  }
  for (int b = b0, j = 0; b < N; b += bstride, ++j) {
    if constexpr (BNA) {
      bn_stage(b);
    } else {
      dma(b);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    const bool counted = stats && (!mask || (j < WAVE ? __builtin_amdgcn_readlane(mrow, j) != 0 : mask[b] != 0));
    nvalid += counted;

    f32x4_t acc[NTW][PTW];
    // lanes past the board read their pad address (~pos): the board's LAST cell, one broadcast address in its bank
    // group beside the valid positions' own slots (raster order), or a top-border address with the slot's key (15x15
    // border tiles)
    int bb[PTW];
#pragma unroll
    for (int i = 0; i < PTW; ++i) bb[i] = (pos[i] < 0 ? ~pos[i] : pos[i]) + cg * 16;
    auto kloop = [&](auto ntl_c) {
      constexpr int NTL = decltype(ntl_c)::value;
      V bf[2][NTL];
      constexpr int PGK = NTL == PTW ? 0 : 1;  // REMAP: the position group of this instantiation
      auto taps = [&](int i) -> unsigned {
        if constexpr (REMAP) return remap15_taps(PGK + PG * i);
        return (LAST_ONE && NTL == PTW && i == NTL - 1) ? LAST_TAPS : 0x1ffu;
      };
      auto live = [&](int i, int st) { return ((taps(i) >> (st >> 2)) & 1u) != 0; };
      auto first = [&](int i) { return 4 * __builtin_ctz(taps(i)); };
      auto readB = [&](int buf, int st) {
        const int tap = st >> 2, ks = st & 3;
        const int off = (tap / 3) * RS + (tap % 3) * PS + ks * 32;
#pragma unroll
        for (int i = 0; i < NTL; ++i)
          if (live(i, st)) bf[buf][i] = *(const V *)(img + bb[i] + off);
      };
      readB(0, 0);
#pragma unroll
      for (int st = 0; st < CKSTEPS; ++st) {
        loadA((st + RD - 1) % RD, st + RD - 1);
        if (st + 1 < CKSTEPS) readB((st + 1) & 1, st + 1);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < NTL; ++i)
          if (live(i, st))
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt)
              acc[nt][i] = M::run(ar[st % RD][nt], bf[st & 1][i], st == first(i) ? f32x4_t{0.f, 0.f, 0.f, 0.f} : acc[nt][i]);
        if (st + 1 < CKSTEPS) __builtin_amdgcn_sched_barrier(0);
      }
#pragma unroll
      for (int i = NTL; i < PTW; ++i)
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) acc[nt][i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    };
    if constexpr (PTW * PG == NPT) kloop(std::integral_constant<int, PTW>{});
    else if (pg + PG * (PTW - 1) < NPT) kloop(std::integral_constant<int, PTW>{});
    else kloop(std::integral_constant<int, PTW - 1>{});

    // ---- epilogue: 4 consecutive output channels of one position per lane -> 8-byte store
    uint16_t *dst = y + (size_t)b * A * CC;
    int say = -100, sax = -100;  // the action stamp's cell (never within reach when there is none)
    if (as.action) {
      const int av = as.action[b];
      say = av / H;
      sax = av - say * H;
    }
    const uint16_t *add = addend ? addend + (size_t)b * A * CC : nullptr;  // + addend, rounded once
    float mu[NTW][4], isd[NTW][4];  // BWD: the BatchNorm's mean / invstd of this lane's channels
    if constexpr (BWD) {
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = (ntile0 + nt) * 16 + g4 * 4 + e;
          mu[nt][e] = bn.save[c];
          isd[nt][e] = bn.save[CC + c];
        }
    }
#pragma unroll
    for (int i = 0; i < PTW; ++i) {
      const int p = tile_p(pg + PG * i);
      if (p >= A) continue;
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt) {
        const int n0 = (ntile0 + nt) * 16 + g4 * 4;
        u16x4_t o;
        {
          const int ddy = say - p / H + 1, ddx = sax - p % H + 1;
          if (ddy >= 0 && ddy <= 2 && ddx >= 0 && ddx <= 2) {
            const float *tb = as.table + (ddy * 3 + ddx) * CC + n0;
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[nt][i][e] += tb[e];
          }
        }
        if (add) {
          const u16x4_t ad = *(const u16x4_t *)(add + (size_t)p * CC + n0);
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = M::bits(acc[nt][i][e] + M::value(ad[e]));
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = M::bits(acc[nt][i][e]);
        }
        *(u16x4_t *)(dst + (size_t)p * CC + n0) = o;
        if (counted) {
          if constexpr (BWD) {  // the rounded output is the BatchNorm's dy
            const size_t k = ((size_t)b * A + p) * CC + n0;
            const u16x4_t xv = *(const u16x4_t *)(bn.x + k), yv = *(const u16x4_t *)(bn.y + k);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              float g = M::value(o[e]);
              if (bn.relu && !(M::value(yv[e]) > 0.f)) g = 0.f;
              s1[nt][e] += g;
              s2[nt][e] = fmaf(g, (M::value(xv[e]) - mu[nt][e]) * isd[nt][e], s2[nt][e]);
            }
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float v = M::value(o[e]);
              s1[nt][e] += v;
              s2[nt][e] = fmaf(v, v, s2[nt][e]);
            }
          }
        }
      }
    }
    if constexpr (PB) {  // this board's partials -> slot b, then the accumulators restart
      if (stats) {
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
              s1[nt][e] += __shfl_xor(s1[nt][e], o, 64);
              s2[nt][e] += __shfl_xor(s2[nt][e], o, 64);
            }
        if ((lane & 15) == 0) {
#pragma unroll
          for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const int cl = (nq * NTW + nt) * 16 + g4 * 4 + e;
              pbred[(pg * 64 + cl) * 2] = s1[nt][e];
              pbred[(pg * 64 + cl) * 2 + 1] = s2[nt][e];
            }
        }
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt)  // every lane: its accumulators now hold the group's reduced sums
#pragma unroll
          for (int e = 0; e < 4; ++e) s1[nt][e] = s2[nt][e] = 0.f;
        __syncthreads();
        if (tid < 64) {
          double a = 0.0, q = 0.0;
#pragma unroll
          for (int g = 0; g < PG; ++g) {
            a += (double)pbred[(g * 64 + tid) * 2];
            q += (double)pbred[(g * 64 + tid) * 2 + 1];
          }
          double *out = stats + ((size_t)(half0 * 64 + tid) * N + b) * 3;  // channel-major [C][N][3]
          out[0] = a;
          out[1] = q;
          out[2] = counted ? (double)A : 0.0;
        }
      }
    }
    __syncthreads();  // every wave is done reading the image before the next board's DMA
  }
  if (!stats || PB) return;
  // ---- per-workgroup partials: the 16 lanes of a lane group hold the same 4 channels at different
  // positions; then the PG position-group waves of a channel group meet in LDS (the image is free)
#pragma unroll
  for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) {
        s1[nt][e] += __shfl_xor(s1[nt][e], o, 64);
        s2[nt][e] += __shfl_xor(s2[nt][e], o, 64);
      }
  float *red = (float *)img;  // [PG][64 channels of this half][2]
  if ((lane & 15) == 0) {
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int cl = (nq * NTW + nt) * 16 + g4 * 4 + e;  // channel within this half
        red[(pg * 64 + cl) * 2] = s1[nt][e];
        red[(pg * 64 + cl) * 2 + 1] = s2[nt][e];
      }
  }
  __syncthreads();
  if (tid < 64) {
    double a = 0.0, q = 0.0;
#pragma unroll
    for (int g = 0; g < PG; ++g) {
      a += (double)red[(g * 64 + tid) * 2];
      q += (double)red[(g * 64 + tid) * 2 + 1];
    }
    double *out = stats + ((size_t)(half0 * 64 + tid) * bstride + b0) * 3;  // channel-major [C][slots][3]
    out[0] = a;
    out[1] = q;
    out[2] = (double)nvalid * A;
  }
}

// ---- split-f16 convolution: float32 activations in, float32 out, float32-grade accuracy on the f16 MFMA pipe (gfx950
// has no TF32 and float32 MFMA runs at 1/16 of the f16 rate): the target network's value trunk (loss.py:54-55).
// Every float32 v is split as hi = f16(v), lo = f16((v - float(hi)) * 2^11) (the scaling keeps lo out of the f16
// subnormals for ordinary activations; hi + lo * 2^-11 is v to max(2^-22 |v|, 2^-35)); then
//   main = sum hi_x hi_w,  corr = sum (hi_x lo_w + lo_x hi_w),  y = main + corr * 2^-11   (all float32; lo lo dropped).
// |v| >= 2^15 is outside the contract.  Same work item, padded image, weight-fragment ring and grid as k_conv3; the
// packed weights are [hi fragments | lo fragments] (2 x FRAG_BYTES, k_pack_split).  ONE image, two passes per board:
// pass 0 stages hi_x and issues, per k-step and B fragment, two MFMAs (hi_w -> main, lo_w -> corr); pass 1 re-stages
// the image with lo_x behind a barrier and runs the 36 k-steps with hi_w into corr: 108 MFMA k-steps per board, two
// LDS fills, no second image (19x19 fits).  global_load_lds cannot convert, so the board is staged through registers
// (as bn_stage does), split on the way and written with 16-byte LDS stores.
constexpr float SPLIT_SCALE = 2048.f, SPLIT_INV = 1.f / 2048.f;

__device__ __forceinline__ uint16_t split_hi(float v) { return __builtin_bit_cast(uint16_t, (_Float16)v); }
__device__ __forceinline__ uint16_t split_lo(float v) {
  const _Float16 h = (_Float16)v;
  return __builtin_bit_cast(uint16_t, (_Float16)((v - (float)h) * SPLIT_SCALE));
}

// fragment i = (t, ks, nt, l) of k_pack_conv's order, its hi half at out + 8 i and its lo half FRAG_BYTES further
__device__ __forceinline__ void pack_split_frag(const float *__restrict__ w, long s0, long s1, long s2, long s3,
                                                int transpose, uint16_t *__restrict__ out, int i) {
  const int l = i & 63, nt = (i >> 6) & 7, st = i >> 9, t = st >> 2, ks = st & 3;
  const int n = nt * 16 + (l & 15);
  uint32_t h[4] = {0, 0, 0, 0}, lw[4] = {0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = chunk_of(ks, l >> 4) * 8 + j;
    const int o = transpose ? c : n, ci = transpose ? n : c, tt = transpose ? 8 - t : t;
    const float v = w[o * s0 + ci * s1 + (tt / 3) * s2 + (tt % 3) * s3];
    h[j >> 1] |= (uint32_t)split_hi(v) << (16 * (j & 1));
    lw[j >> 1] |= (uint32_t)split_lo(v) << (16 * (j & 1));
  }
  *(uint4 *)(out + (size_t)i * 8) = make_uint4(h[0], h[1], h[2], h[3]);
  *(uint4 *)(out + FRAG_BYTES / 2 + (size_t)i * 8) = make_uint4(lw[0], lw[1], lw[2], lw[3]);
}

__global__ void __launch_bounds__(256) k_pack_split(const float *__restrict__ w, long s0, long s1, long s2, long s3,
                                                    int transpose, uint16_t *__restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < CKSTEPS * 8 * 64) pack_split_frag(w, s0, s1, s2, s3, transpose, out, i);
}

__global__ void __launch_bounds__(256) k_pack_split_many(const PackJob *__restrict__ jobs) {
  const PackJob j = jobs[blockIdx.y];
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < CKSTEPS * 8 * 64) pack_split_frag(j.w, j.s0, j.s1, j.s2, j.s3, j.transpose, j.out, i);
}

// The optional fused epilogue: eval-mode BatchNorm (running statistics) + residual + ReLU in k_bnl_apply's arithmetic,
// v = (acc - mean) * (gamma * (1 / sqrtf(var + eps))) + beta, + res, max 0.  gamma = nullptr: the plain convolution.
struct SplitBn {
  const float *gamma, *beta, *mean, *var;
  const float *res;  // float32 NHWC like y, or nullptr
  float eps;
  int relu;
};

template <int H, int PG>
__global__ void __launch_bounds__(128 * PG, ConvCfg<H>::WG_PER_CU) k_conv3_split(const float *__restrict__ x,
                                                                                const uint16_t *__restrict__ wpk,
                                                                                float *__restrict__ y, int N, SplitBn bn) {
  using I = CImg<H>;
  using M = Mfma<__half>;
  typedef typename M::V V;
  constexpr int A = H * H, NPT = (A + 15) / 16;
  constexpr int NTW = 2, PTW = (NPT + PG - 1) / PG, RD = GMZ_CONV_RD, NW = 2 * PG, NTHR = 64 * NW;
  constexpr int PS = I::PS, RS = I::RS;
  constexpr int NST = 2 * CKSTEPS;  // ring steps per board: pass 0's (hi_w and lo_w fragments), then pass 1's (hi_w)
  static_assert(NST % RD == 0, "ring slots repeat per item");
  static_assert(NTHR % 16 == 0, "a thread's chunk of every cell it stages is tid & 15");
  // the board's last tile skips the k-steps whose tap reaches only the zero border, as in k_conv3
  constexpr bool LAST_ONE = NPT == PG * (PTW - 1) + 1;
  constexpr unsigned LAST_TAPS = LAST_ONE ? live_taps(H, (NPT - 1) * 16, A) : 0x1ffu;
  __shared__ __attribute__((aligned(16))) uint8_t img[I::BYTES];

  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int nq = w & 1, pg = w >> 1;
  const int g4 = lane >> 4;
  const int cg = (g4 & 1) * 8 + (g4 >> 1);
  const int half0 = (blockIdx.x >> 3) & 1;  // the XCD-aware items of k_conv3
  const int b0 = (int)((blockIdx.x >> 4) * 8 + (blockIdx.x & 7));
  const int bstride = (int)(gridDim.x >> 1);
  const int ntile0 = half0 * 4 + nq * NTW;

  {  // zero the image's border cells; both stagings of every board rewrite the whole interior
    constexpr int HP = I::HP, NBORDER = 2 * HP + 2 * H;
    for (int i = tid; i < NBORDER * 16; i += NTHR) {
      const int k = i >> 4, r = k - 2 * HP;
      const int yy = k < HP ? 0 : k < 2 * HP ? HP - 1 : 1 + (r >> 1);
      const int xx = k < HP ? k : k < 2 * HP ? k - HP : (r & 1) * (HP - 1);
      ((uint4 *)(img + yy * RS + xx * PS))[i & 15] = make_uint4(0, 0, 0, 0);
    }
  }
  auto tile_p = [&](int pt) {
    const int p = pt * 16 + csigma16(lane & 15);
    return (pt < NPT && p < A) ? p : A;
  };
  int bb[PTW];  // B-fragment read base of each tile's cell; a pad lane reads the board's last cell (never stored)
#pragma unroll
  for (int i = 0; i < PTW; ++i) {
    const int p = tile_p(pg + PG * i), q = p < A ? p : A - 1;
    bb[i] = (q / H) * RS + (q % H) * PS + cg * 16;
  }
  const __amdgpu_buffer_rsrc_t wrsrc =
      __builtin_amdgcn_make_buffer_rsrc((void *)wpk, (short)0, 2 * FRAG_BYTES, 0x00020000);
  const int wvoff = ntile0 * 1024 + lane * 16;
  V arh[RD][NTW], arl[RD][NTW];
  // ring step s (mod NST): pass 0 k-step s loads the hi_w and lo_w fragments, pass 1 k-step s - CKSTEPS the hi_w ones
  auto loadA = [&](int slot, int s) {
    const int q = s % NST, st = q < CKSTEPS ? q : q - CKSTEPS;
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
      arh[slot][nt] = __builtin_bit_cast(V, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, wvoff + nt * 1024, st * 8192, 0));
      if (q < CKSTEPS)
        arl[slot][nt] = __builtin_bit_cast(
            V, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, wvoff + nt * 1024, FRAG_BYTES + st * 8192, 0));
    }
  };
#pragma unroll
  for (int k = 0; k < RD - 1; ++k) loadA(k, k);

  // ---- board bd -> image interior as f16 halves: thread tid takes 8-channel chunk tid & 15 of its cells (32 bytes of
  // float32, consecutive threads consecutive addresses), U cells' loads issued before any arithmetic
  auto stage = [&](int bd, auto lo_c) {
    constexpr bool LO = decltype(lo_c)::value;
    int t = tid;
    asm volatile("" : "+v"(t));  // re-derive the cells' addresses per staging (bn_stage: hoisted, they spilled)
    const int bch = t & 15;
    constexpr int NCH = A * 16, NI = (NCH + NTHR - 1) / NTHR, U = 4;  // (8: spills beside the accumulators)
    const float4 *src = (const float4 *)(x + (size_t)bd * A * CC);
#pragma unroll
    for (int i0 = 0; i0 < NI; i0 += U) {
      float4 va[U], vb[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = t + (i0 + u) * NTHR;
        if (i0 + u < NI && i < NCH) {
          va[u] = src[2 * i];
          vb[u] = src[2 * i + 1];
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = t + (i0 + u) * NTHR;
        if (!(i0 + u < NI && i < NCH)) continue;
        const float f[8] = {va[u].x, va[u].y, va[u].z, va[u].w, vb[u].x, vb[u].y, vb[u].z, vb[u].w};
        uint32_t ow[4];
#pragma unroll
        for (int h = 0; h < 4; ++h) {
          const uint16_t e0 = LO ? split_lo(f[2 * h]) : split_hi(f[2 * h]);
          const uint16_t e1 = LO ? split_lo(f[2 * h + 1]) : split_hi(f[2 * h + 1]);
          ow[h] = (uint32_t)e0 | ((uint32_t)e1 << 16);
        }
        const int p = i >> 4;
        ((uint4 *)(img + (p / H + 1) * RS + (p % H + 1) * PS))[bch] = make_uint4(ow[0], ow[1], ow[2], ow[3]);
      }
    }
  };

  for (int b = b0; b < N; b += bstride) {
    f32x4_t am[NTW][PTW], ac[NTW][PTW];  // main, corr
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
      for (int i = 0; i < PTW; ++i) am[nt][i] = ac[nt][i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    auto kloop = [&](auto ntl_c, auto pass_c) {
      constexpr int NTL = decltype(ntl_c)::value, PASS = decltype(pass_c)::value;
      // ONE B-fragment buffer per tile (k_conv3 holds two; here the accumulators take twice the registers): tile i's
      // fragment of the next k-step is read right after the MFMAs that consumed this one, the other tiles' MFMAs
      // (28 in pass 0, 14 in pass 1) between that read and its use
      V bf[NTL];
      auto live = [&](int i, int st) {
        const unsigned taps = (LAST_ONE && NTL == PTW && i == NTL - 1) ? LAST_TAPS : 0x1ffu;
        return ((taps >> (st >> 2)) & 1u) != 0;
      };
      auto readB = [&](int i, int st) {
        const int tap = st >> 2, ks = st & 3;
        bf[i] = *(const V *)(img + bb[i] + (tap / 3) * RS + (tap % 3) * PS + ks * 32);
      };
#pragma unroll
      for (int i = 0; i < NTL; ++i) readB(i, 0);
#pragma unroll
      for (int st = 0; st < CKSTEPS; ++st) {
        constexpr int S0 = PASS * CKSTEPS;
        loadA((S0 + st + RD - 1) % RD, S0 + st + RD - 1);
#pragma unroll
        for (int i = 0; i < NTL; ++i) {
          if (live(i, st)) {
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) {
              if constexpr (PASS == 0) {
                am[nt][i] = M::run(arh[(S0 + st) % RD][nt], bf[i], am[nt][i]);
                ac[nt][i] = M::run(arl[(S0 + st) % RD][nt], bf[i], ac[nt][i]);
              } else {
                ac[nt][i] = M::run(arh[(S0 + st) % RD][nt], bf[i], ac[nt][i]);
              }
            }
          }
          if (st + 1 < CKSTEPS && live(i, st + 1)) readB(i, st + 1);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    };
    auto pass = [&](auto pass_c) {
      if constexpr (PTW * PG == NPT) kloop(std::integral_constant<int, PTW>{}, pass_c);
      else if (pg + PG * (PTW - 1) < NPT) kloop(std::integral_constant<int, PTW>{}, pass_c);
      else kloop(std::integral_constant<int, PTW - 1>{}, pass_c);
    };
    stage(b, std::false_type{});
    __syncthreads();  // hi_x staged (first board: and the zeroed border)
    pass(std::integral_constant<int, 0>{});
    __syncthreads();  // every wave is done reading hi_x
    stage(b, std::true_type{});
    __syncthreads();
    pass(std::integral_constant<int, 1>{});

    // ---- epilogue: 4 consecutive output channels of one position per lane -> 16-byte store.  Its positions and
    // channels are re-derived from an opaque copy of the lane index: hoisted out of the board loop they are spilled
    // around the k-loops, whose accumulators leave no room for them
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const int eg4 = ln >> 4, ecol = csigma16(ln & 15);
    float *dst = y + (size_t)b * A * CC;
    const float *rsd = bn.res ? bn.res + (size_t)b * A * CC : nullptr;
    float mu[NTW][4], sc[NTW][4], sh[NTW][4];  // re-read per board (L1 hits) instead of kept live across the k-loops
    if (bn.gamma) {
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = (ntile0 + nt) * 16 + eg4 * 4 + e;
          mu[nt][e] = bn.mean[c];
          sc[nt][e] = bn.gamma[c] * (1.0f / sqrtf(bn.var[c] + bn.eps));
          sh[nt][e] = bn.beta[c];
        }
    }
#pragma unroll
    for (int i = 0; i < PTW; ++i) {
      const int pt = pg + PG * i, p = pt * 16 + ecol;
      if (pt >= NPT || p >= A) continue;
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt) {
        const int n0 = (ntile0 + nt) * 16 + eg4 * 4;
        f32x4_t o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = am[nt][i][e] + ac[nt][i][e] * SPLIT_INV;
        if (bn.gamma) {
          f32x4_t r = {0.f, 0.f, 0.f, 0.f};
          if (rsd) r = *(const f32x4_t *)(rsd + (size_t)p * CC + n0);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            float v = (o[e] - mu[nt][e]) * sc[nt][e] + sh[nt][e];
            if (rsd) v += r[e];
            o[e] = bn.relu ? fmaxf(v, 0.f) : v;
          }
        }
        *(f32x4_t *)(dst + (size_t)p * CC + n0) = o;
      }
    }
    __syncthreads();  // every wave is done reading lo_x before the next board's staging
  }
}

// ---- weight gradient: dW[o][c][t] = sum over boards n and positions p of dy[n][p][o] * x[n][p + d(t)][c]
// (d(t) = (t/3 - 1, t%3 - 1), zero outside the board), the GEMM M = o, N = c, K = (n, p) per tap.
// Workgroup = (tap row ty, chunk of boards): 8 waves = 4 (32 o) x 2 (64 c), accumulating the three taps
// of row ty (3 x 2 m-tiles x 4 n-tiles, 96 f32 per lane).  Per board the dy tile [position][128 o]
// and the zero-padded x image [(H+2) x (H+2) cells][128 c] are DMA'd into LDS in their HBM (NHWC)
// order with 288-byte rows; both MFMA operands need 8 consecutive positions (K) per lane and come from
// ds_read_b64_tr_b16 transposing reads (per 16-lane group a 4-row x 16-channel block, delivered
// channel-major).  K order inside a k-step: lane group g takes positions 4g..4g+3 (first read) and
// 16+4g..16+4g+3 (second), so the two groups of a 32-lane half read rows 4 apart = 1152 B = 32 banks
// apart, and the 288-B stride puts a group's 4 rows 8 banks apart: conflict-free.  With padded x the
// three taps of the row and the four n-tiles are immediate offsets from two base addresses per k-step.
// Partials per chunk go to a scratch [chunk][9][128][128] that k_conv3_wgrad_reduce sums into the f32
// weight gradient.
typedef short s16x4_t __attribute__((ext_vector_type(4)));

//
// Row bands (19x19): a whole board's tiles (384 dy rows + 21 x 21 x cells = 237,600 B) do not fit the 160 KB of LDS,
// so the board is processed as NB = 2 bands of BR = 10 | 9 board rows inside the per-board loop, the accumulators
// running on across bands.  A band holds its BR * H dy rows and — the workgroup's tap row ty being fixed — exactly the
// x rows those need: band-local row yy is board row r0 + yy + ty - 1 (r0 = the band's first row), HP cells wide with
// the zero border columns, so no border ROWS are stored: 192 x 288 + 10 x 21 x 288 = 115,776 B.  Same 288-B rows, same
// transposing reads, tap columns still +RB apart.  What no DMA writes changes per band and is zeroed before the band's
// DMA: the x row above the board (ty = 0, band 0, local row 0), the one below it (ty = 2, last band, its last local
// row), and the dy rows between the last band's positions and a full band's; the border columns and the dy rows past
// a full band are zeroed once.
template <int H>
struct WgLds {
  static constexpr int A = H * H, RB = 288, HP = H + 2;
  static constexpr int NB = H > 15 ? 2 : 1, BR = (H + NB - 1) / NB;  // row bands per board, board rows per band
  static constexpr int BA = BR * H;                                  // positions of a full band (NB = 1: the board)
  static constexpr int KS = (BA + 31) / 32, NPOS = KS * 32;
  static constexpr int DY_BYTES = NPOS * RB, X_OFF = DY_BYTES, X_BYTES = (NB == 1 ? HP : BR) * HP * RB;
  static constexpr int BYTES = DY_BYTES + X_BYTES;
  static constexpr int NPD = (BA * RB + 1023) / 1024;       // dy DMA pieces
  static constexpr int RUN = (H - 1) * RB + 256, RUN_DMA = (RUN + 1023) / 1024;  // one board row of x
};

__device__ __forceinline__ s16x4_t tr_read(const uint8_t *lds_base, int off) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t *)(
      (__attribute__((address_space(3))) uint8_t *)lds_base + off));
}

// the boards of one weight-gradient launch: up to 8 segments of nps boards each (board b of the launch is
// board b % nps of segment b / nps), so the gradient contributions of one weight over several uses (the
// dynamics trunk's convs in every unroll step) are one launch and one partial-sum reduction
constexpr int WG_MAX_SEGS = 8;
struct WgSrc {
  const uint16_t *x[WG_MAX_SEGS];
  const uint16_t *dy[WG_MAX_SEGS];
  int nps;
};

template <int H, typename T>
__global__ void __launch_bounds__(512, 1) k_conv3_wgrad(WgSrc src, int N, int nch, float *__restrict__ part) {
  using L = WgLds<H>;
  using M = Mfma<T>;
  typedef typename M::V V;
  constexpr int A = H * H, KS = L::KS, RB = L::RB, HP = L::HP;
  static_assert(L::BYTES <= 163840, "LDS budget");
  __shared__ __attribute__((aligned(16))) uint8_t smem[L::BYTES];
  uint8_t *xt = smem + L::X_OFF;

  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  // XCD-aware: workgroups are dealt to the 8 XCDs round-robin by index, so the three tap rows of a
  // chunk get indices 8 apart (same XCD, same L2): each board is fetched from HBM once, not 3 times
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
  const int ty = slot % 3, chunk = (slot / 3) * 8 + xcd;
  const int wo = w & 3, wc = w >> 2;
  const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
  const int ocol = (wo * 32 + 4 * pp) * 2, ccol = (wc * 64 + 4 * pp) * 2;  // this lane's column bytes

  auto zero_cell = [&](uint8_t *cellp, int i) { ((uint4 *)cellp)[i & 15] = make_uint4(0, 0, 0, 0); };
  // zero what no board's DMA writes: the dy rows past the board (positions A..NPOS-1 of the last k-step) and the x
  // image's border cells (ds_write_b128 stores, as in k_conv3); banded: the dy rows past a full band and the x
  // image's border columns
  if constexpr (L::NB == 1) {
    constexpr int NTAIL = L::NPOS - A, NBORDER = 2 * HP + 2 * H;
    for (int i = tid; i < (NTAIL + NBORDER) * 16; i += 512) {
      const int k = i >> 4;
      uint8_t *cellp;
      if (k < NTAIL) {
        cellp = smem + (A + k) * RB;
      } else {
        const int kb = k - NTAIL, r = kb - 2 * HP;
        const int yy = kb < HP ? 0 : kb < 2 * HP ? HP - 1 : 1 + (r >> 1);
        const int xx = kb < HP ? kb : kb < 2 * HP ? kb - HP : (r & 1) * (HP - 1);
        cellp = xt + (yy * HP + xx) * RB;
      }
      ((uint4 *)cellp)[i & 15] = make_uint4(0, 0, 0, 0);
    }
  } else {
    constexpr int NTAIL = L::NPOS - L::BA, NBORDER = 2 * L::BR;
    for (int i = tid; i < (NTAIL + NBORDER) * 16; i += 512) {
      const int k = i >> 4, kb = k - NTAIL;
      zero_cell(k < NTAIL ? smem + (L::BA + k) * RB : xt + ((kb >> 1) * HP + (kb & 1) * (HP - 1)) * RB, i);
    }
  }
  __syncthreads();

  f32x4_t acc[3][2][4];
#pragma unroll
  for (int tx = 0; tx < 3; ++tx)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) acc[tx][mt][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  for (int b = chunk; b < N; b += nch) {
    const int sg = b / src.nps, lb = b - sg * src.nps;
    const uint8_t *sd = (const uint8_t *)(src.dy[sg] + (size_t)lb * A * CC);
    const uint8_t *sx = (const uint8_t *)(src.x[sg] + (size_t)lb * A * CC);
    if constexpr (L::NB == 1) {
      // ---- dy rows 0..A-1 and the x image interior: LDS-linear 1 KB pieces, row pads skipped
      for (int j = w; j < L::NPD + H * L::RUN_DMA; j += 8) {
        if (j < L::NPD) {
          const int o = j * 1024 + lane * 16;
          const int row = o / RB, ch = (o % RB) >> 4;
          if (row < A && ch < 16)
            __builtin_amdgcn_global_load_lds((const void *)(sd + row * 256 + ch * 16),
                                             (__attribute__((address_space(3))) void *)(smem + j * 1024), 16, 0, 0);
        } else {
          const int jj = j - L::NPD, yy = jj / L::RUN_DMA, piece = jj % L::RUN_DMA;
          const int o = piece * 1024 + lane * 16;
          const int xx = o / RB, ch = (o % RB) >> 4;
          if (o < L::RUN && ch < 16)
            __builtin_amdgcn_global_load_lds((const void *)(sx + (yy * H + xx) * 256 + ch * 16),
                                             (__attribute__((address_space(3))) void *)(xt + ((yy + 1) * HP + 1) * RB + piece * 1024),
                                             16, 0, 0);
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
#pragma unroll 2
      for (int ks = 0; ks < KS; ++ks) {
        const int p0 = ks * 32 + 4 * g + q, p1 = p0 + 16;
        // x rows: cell (y + ty, x) of the padded image for tap column 0; columns 1, 2 are +RB, +2 RB.
        // Positions past the board (zero dy rows) read the last position's cells
        const int c0 = p0 < A ? p0 : A - 1, c1 = p1 < A ? p1 : A - 1;
        const int xb0 = ((c0 / H + ty) * HP + c0 % H) * RB + ccol, xb1 = ((c1 / H + ty) * HP + c1 % H) * RB + ccol;
        const int ab0 = p0 * RB + ocol, ab1 = p1 * RB + ocol;
        V af[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
          const s16x4_t lo = tr_read(smem, ab0 + mt * 32), hi = tr_read(smem, ab1 + mt * 32);
          af[mt] = __builtin_bit_cast(V, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
        }
#pragma unroll
        for (int tx = 0; tx < 3; ++tx) {
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) {
            const s16x4_t lo = tr_read(xt, xb0 + tx * RB + nt * 32), hi = tr_read(xt, xb1 + tx * RB + nt * 32);
            const V bf = __builtin_bit_cast(V, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) acc[tx][mt][nt] = M::run(af[mt], bf, acc[tx][mt][nt]);
          }
        }
      }
      __syncthreads();  // every wave is done with this board's tiles before the next DMA
    } else {
      for (int bd = 0; bd < L::NB; ++bd) {
        const int r0 = bd * L::BR, nrows = H - r0 < L::BR ? H - r0 : L::BR, npos = nrows * H;
        // ---- what this band's DMA leaves unwritten but the previous band's wrote: the dy rows npos..BA-1 (the last,
        // shorter band) and the x row outside the board (local row 0 above it, local row nrows - 1 below it)
        const int xr0 = r0 + ty - 1;  // board row of local x row 0
        const int zrow = xr0 < 0 ? 0 : xr0 + nrows > H ? nrows - 1 : -1;
        const int ntail = L::BA - npos, nz = ntail + (zrow >= 0 ? H : 0);
        for (int i = tid; i < nz * 16; i += 512) {
          const int k = i >> 4;
          zero_cell(k < ntail ? smem + (npos + k) * RB : xt + (zrow * HP + 1 + (k - ntail)) * RB, i);
        }
        // ---- dy rows 0..npos-1 (board positions r0 * H + row) and the x rows inside the board
        for (int j = w; j < L::NPD + nrows * L::RUN_DMA; j += 8) {
          if (j < L::NPD) {
            const int o = j * 1024 + lane * 16;
            const int row = o / RB, ch = (o % RB) >> 4;
            if (row < npos && ch < 16)
              __builtin_amdgcn_global_load_lds((const void *)(sd + (r0 * H + row) * 256 + ch * 16),
                                               (__attribute__((address_space(3))) void *)(smem + j * 1024), 16, 0, 0);
          } else {
            const int jj = j - L::NPD, yy = jj / L::RUN_DMA, piece = jj % L::RUN_DMA;
            const int o = piece * 1024 + lane * 16;
            const int xx = o / RB, ch = (o % RB) >> 4;
            if (yy != zrow && o < L::RUN && ch < 16)
              __builtin_amdgcn_global_load_lds((const void *)(sx + ((xr0 + yy) * H + xx) * 256 + ch * 16),
                                               (__attribute__((address_space(3))) void *)(xt + (yy * HP + 1) * RB + piece * 1024),
                                               16, 0, 0);
          }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
#pragma unroll 2
        for (int ks = 0; ks < KS; ++ks) {
          // the band's rows are already shifted by ty; positions past the band read its last position's cells
          const int p0 = ks * 32 + 4 * g + q, p1 = p0 + 16;
          const int c0 = p0 < npos ? p0 : npos - 1, c1 = p1 < npos ? p1 : npos - 1;
          const int xb0 = (c0 / H * HP + c0 % H) * RB + ccol, xb1 = (c1 / H * HP + c1 % H) * RB + ccol;
          const int ab0 = p0 * RB + ocol, ab1 = p1 * RB + ocol;
          // (the whole-board k-step above, restated: sharing it through a lambda changed the 9x9 / 15x15 kernels'
          // register allocation and schedule)
          V af[2];
#pragma unroll
          for (int mt = 0; mt < 2; ++mt) {
            const s16x4_t lo = tr_read(smem, ab0 + mt * 32), hi = tr_read(smem, ab1 + mt * 32);
            af[mt] = __builtin_bit_cast(V, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
          }
#pragma unroll
          for (int tx = 0; tx < 3; ++tx) {
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
              const s16x4_t lo = tr_read(xt, xb0 + tx * RB + nt * 32), hi = tr_read(xt, xb1 + tx * RB + nt * 32);
              const V bf = __builtin_bit_cast(V, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
#pragma unroll
              for (int mt = 0; mt < 2; ++mt) acc[tx][mt][nt] = M::run(af[mt], bf, acc[tx][mt][nt]);
            }
          }
        }
        __syncthreads();  // every wave is done with this band's tiles before the next DMA
      }
    }
  }
  // ---- acc[tx][mt][nt][e] = dW[o = 32 wo + 16 mt + 4 g + e][c = 64 wc + 16 nt + (lane & 15)][3 ty + tx]
  float *pc = part + (size_t)chunk * 9 * CC * CC;
#pragma unroll
  for (int tx = 0; tx < 3; ++tx)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int o = wo * 32 + 16 * mt + 4 * g + e, c = wc * 64 + 16 * nt + (lane & 15);
          pc[((size_t)(ty * 3 + tx) * CC + o) * CC + c] = acc[tx][mt][nt][e];
        }
}

// dW[o][c][ky][kx] (+)= sum over chunks of part[chunk][t][o][c], dW at element strides (s0, s1, s2, s3);
// 8 independent partial sums per thread keep 8 loads in flight
__global__ void __launch_bounds__(256) k_conv3_wgrad_reduce(const float *__restrict__ part, int nch, float *dw, long s0,
                                                            long s1, long s2, long s3, int accumulate) {
  const int i = blockIdx.x * 256 + threadIdx.x;  // (t, o, c)
  if (i >= 9 * CC * CC) return;
  const int c = i % CC, o = (i / CC) % CC, t = i / (CC * CC);
  constexpr size_t STR = 9 * CC * CC;
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int k = 0;
  for (; k + 8 <= nch; k += 8) {
#pragma unroll
    for (int u = 0; u < 8; ++u) s[u] += part[(size_t)(k + u) * STR + i];
  }
  for (; k < nch; ++k) s[0] += part[(size_t)k * STR + i];
  const float tot = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
  float *d = dw + o * s0 + c * s1 + (t / 3) * s2 + (t % 3) * s3;
  *d = accumulate ? *d + tot : tot;
}

static int cu_count_conv() {
  static int n = 0;
  if (!n) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    hipDeviceProp_t p;
    n = hipGetDeviceProperties(&p, dev) == hipSuccess ? p.multiProcessorCount : 256;
  }
  return n;
}

// two workgroups per board (one per half of the output channels), at most two per CU: a multiple of 16 (whole XCD
// pairs; workgroups past the boards do nothing).  The same grid at every board size: the statistics slot count below
// is a function of N alone (gmz_conv3x3_stats_slots takes no H), so at 19x19, where one workgroup per CU is resident,
// the workgroups past 2 CUs' worth queue behind the first ones instead of striding (only above 256 boards a launch)
int conv3_grid(int N) {
  const long items = (2L * N + 15) / 16 * 16, cap = 2L * 2 * cu_count_conv() / 16 * 16;
  return (int)(items < cap ? items : cap);
}

// statistics slots (partials) a launch writes: one per board pair of workgroups, or per board (per_board, the
// segmented consistency trunk).  The same function answers gmz_conv3x3_stats_slots and the capacity check before
// every launch, so the count asked for is the count the dispatch writes (ABI 10)
int conv3_stats_slots(int N, bool per_board = false) { return per_board ? N : conv3_grid(N) / 2; }
static int check_slots(const char *fn, const double *stats, int stats_slots, int N, bool per_board) {
  if (!stats) return 0;
  const int need = conv3_stats_slots(N, per_board);
  if (stats_slots != need)
    return fail(std::string(fn) + ": statistics buffer of " + std::to_string(stats_slots) + " slots, this launch writes " +
                std::to_string(need) + (per_board ? " (one per board)" : " (gmz_conv3x3_stats_slots)"));
  return 0;
}

// "6, 9, 15 or 19" from ConvSizes
template <int... Hs>
std::string sizes_text(SizeList<Hs...>) {
  const int v[] = {Hs...};
  constexpr int n = sizeof...(Hs);
  std::string t;
  for (int i = 0; i < n; ++i) t += (i == 0 ? "" : i == n - 1 ? " or " : ", ") + std::to_string(v[i]);
  return t;
}
int bad_size(const char *fn) { return fail(std::string(fn) + ": board size must be " + sizes_text(ConvSizes{})); }

// f(integral_constant<int, H>) for the H of the list, or -2 (not a supported size)
template <typename F, int... Hs>
int for_size(int H, SizeList<Hs...>, F &&f) {
  int rc = -2;
  (void)((H == Hs ? (rc = f(std::integral_constant<int, Hs>{}), true) : false) || ...);
  return rc;
}

template <int H, typename T, bool BWD, bool PB = false, bool BNA = false>
void launch_conv3_k(const void *x, const void *wpk, void *y, int N, const uint8_t *mask, double *stats, const void *addend,
                    const BnBwd &bn, hipStream_t st, const ActStamp &as = ActStamp{}, const BnApply &ba = BnApply{}) {
  constexpr int PG = ConvCfg<H>::PG;
  hipLaunchKernelGGL((k_conv3<H, T, PG, BWD, PB, BNA>), dim3(conv3_grid(N)), dim3(128 * PG), 0, st, (const uint16_t *)x,
                     (const uint16_t *)wpk, (uint16_t *)y, N, mask, stats, (const uint16_t *)addend, bn, as, ba);
}

template <int H, typename T>
int launch_conv3(const void *x, const void *wpk, void *y, int N, const uint8_t *mask, double *stats, const void *addend,
                 const BnBwd &bn, hipStream_t st, bool per_board = false, const ActStamp &as = ActStamp{},
                 const BnApply &ba = BnApply{}) {
  const bool bwd = bn.x != nullptr;
  if constexpr (!ConvCfg<H>::AB) {
    if (bwd || as.action)
      return fail("gmz_conv3x3: the BWD-statistics and action-stamp variants (off-by-default A/B paths) are built for "
                  "board sizes 9 and 15 only");
  }
  if (ba.z) launch_conv3_k<H, T, false, false, true>(x, wpk, y, N, mask, stats, addend, bn, st, as, ba);
  else if (per_board) launch_conv3_k<H, T, false, true>(x, wpk, y, N, mask, stats, addend, bn, st, as);
  else if (!bwd) launch_conv3_k<H, T, false>(x, wpk, y, N, mask, stats, addend, bn, st, as);
  else if constexpr (ConvCfg<H>::AB) launch_conv3_k<H, T, true>(x, wpk, y, N, mask, stats, addend, bn, st, as);
  GMZ_LAUNCH_CHECK();
  return 0;
}

// The one host path of the gmz_conv3x3_forward* entry points.  In this order: the operands of `need` non-null, N,
// `early`, the statistics slots (one per board pair of workgroups, or per board), the operands of `aligned` 16-B
// aligned, `late`, then dtype and board size into launch_conv3.  fn is the entry point's name (the slot check reports
// it), pfx what the other messages carry; early / late are an entry point's own refusal, worked out by it and reported
// here at its place in the order (empty: none).
int conv3_forward(const char *fn, const char *pfx, int dtype, int H, std::initializer_list<const void *> need,
                  std::initializer_list<const void *> aligned, const std::string &early, const std::string &late,
                  const void *x, const void *wpk, void *y, int N, const uint8_t *mask, double *stats, int stats_slots,
                  bool per_board, const void *addend, void *stream, const BnBwd &bn = BnBwd{},
                  const ActStamp &as = ActStamp{}, const BnApply &ba = BnApply{}) {
  for (const void *p : need)
    if (!p) return fail(std::string(pfx) + ": null operand");
  if (N <= 0) return fail(std::string(pfx) + ": N must be positive");
  if (!early.empty()) return fail(early);
  if (check_slots(fn, stats, stats_slots, N, per_board)) return -1;
  for (const void *p : aligned)
    if ((uintptr_t)p & 15) return fail(std::string(pfx) + ": operands must be 16-B aligned");
  if (!late.empty()) return fail(late);
  return by_dtype<false>(pfx, dtype, [&](auto t) {
    const int rc = for_size(H, ConvSizes{}, [&](auto h) {
      return launch_conv3<decltype(h)::value, dtype_of<decltype(t)>>(x, wpk, y, N, mask, stats, addend, bn,
                                                                     (hipStream_t)stream, per_board, as, ba);
    });
    return rc == -2 ? bad_size("gmz_conv3x3") : rc;
  });
}

template <int H>
int launch_conv3_split(const float *x, const void *wpk, float *y, int N, const SplitBn &bn, hipStream_t st) {
  constexpr int PG = ConvCfg<H>::PG;
  hipLaunchKernelGGL((k_conv3_split<H, PG>), dim3(conv3_grid(N)), dim3(128 * PG), 0, st, x, (const uint16_t *)wpk, y, N, bn);
  GMZ_LAUNCH_CHECK();
  return 0;
}

// chunks of boards: a multiple of 8 (one per XCD in each group of 24 workgroups), at most one
// workgroup per CU
int wgrad_chunks(int N) {
  int n = cu_count_conv() / 24 * 8;
  const int cap = (N + 7) / 8 * 8;
  return n < cap ? n : cap;
}

template <int H, typename T>
int launch_wgrad(const WgSrc &src, int N, float *part, hipStream_t st) {
  const int nch = wgrad_chunks(N);
  hipLaunchKernelGGL((k_conv3_wgrad<H, T>), dim3(3 * nch), dim3(512), 0, st, src, N, nch, part);
  GMZ_LAUNCH_CHECK();
  return 0;
}

}  // namespace
}  // namespace gmz

using namespace gmz;

GMZ_EXPORT int gmz_conv3x3_pack(int dtype, const float *w, int64_t s0, int64_t s1, int64_t s2, int64_t s3,
                                int transpose, void *packed, void *stream) {
  if (!w || !packed) return fail("gmz_conv3x3_pack: null operand");
  return by_dtype<false>("gmz_conv3x3_pack", dtype, [&](auto t) {  // the dtype is checked before the alignment
    // the kernel writes 16-byte fragments, as gmz_conv3x3_pack_split checks
    if ((uintptr_t)packed & 15) return fail("gmz_conv3x3_pack: packed must be 16-B aligned");
    const int n = CKSTEPS * 8 * 64;
    hipLaunchKernelGGL(k_pack_conv<dtype_of<decltype(t)>>, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, w,
                       (long)s0, (long)s1, (long)s2, (long)s3, transpose, (uint16_t *)packed);
    GMZ_LAUNCH_CHECK();
    return 0;
  });
}

GMZ_EXPORT int gmz_conv3x3_pack_job_bytes(size_t *out) {
  if (!out) return fail("gmz_conv3x3_pack_job_bytes: null");
  *out = sizeof(PackJob);
  return 0;
}

GMZ_EXPORT int gmz_conv3x3_pack_many(int dtype, const void *jobs, int n_jobs, void *stream) {
  if (!jobs || n_jobs <= 0 || n_jobs > 65535) return fail("gmz_conv3x3_pack_many: 1 <= n_jobs <= 65535 jobs");
  const dim3 grid((CKSTEPS * 8 * 64 + 255) / 256, n_jobs);
  return by_dtype<false>("gmz_conv3x3_pack_many", dtype, [&](auto t) {
    hipLaunchKernelGGL(k_pack_many<dtype_of<decltype(t)>>, grid, dim3(256), 0, (hipStream_t)stream, (const PackJob *)jobs);
    GMZ_LAUNCH_CHECK();
    return 0;
  });
}

GMZ_EXPORT int gmz_conv3x3_pack_split(const float *w, int64_t s0, int64_t s1, int64_t s2, int64_t s3, int transpose,
                                      void *packed, void *stream) {
  if (!w || !packed) return fail("gmz_conv3x3_pack_split: null operand");
  if ((uintptr_t)packed & 15) return fail("gmz_conv3x3_pack_split: packed must be 16-B aligned");
  const int n = CKSTEPS * 8 * 64;
  hipLaunchKernelGGL(k_pack_split, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, w, (long)s0, (long)s1,
                     (long)s2, (long)s3, transpose, (uint16_t *)packed);
  GMZ_LAUNCH_CHECK();
  return 0;
}

GMZ_EXPORT int gmz_conv3x3_pack_split_many(const void *jobs, int n_jobs, void *stream) {
  if (!jobs || n_jobs <= 0 || n_jobs > 65535) return fail("gmz_conv3x3_pack_split_many: 1 <= n_jobs <= 65535 jobs");
  const dim3 grid((CKSTEPS * 8 * 64 + 255) / 256, n_jobs);
  hipLaunchKernelGGL(k_pack_split_many, grid, dim3(256), 0, (hipStream_t)stream, (const PackJob *)jobs);
  GMZ_LAUNCH_CHECK();
  return 0;
}

GMZ_EXPORT int gmz_conv3x3_forward_split(int H, const float *x, const void *packed, float *y, int N, const float *gamma,
                                         const float *beta, const float *running_mean, const float *running_var,
                                         float eps, const float *res, int relu, void *stream) {
  if (!x || !packed || !y) return fail("gmz_conv3x3_forward_split: null operand");
  if (N <= 0) return fail("gmz_conv3x3_forward_split: N must be positive");
  if (!gamma) {
    if (beta || running_mean || running_var || res || relu)
      return fail("gmz_conv3x3_forward_split: without gamma (the plain convolution) beta, running_mean, running_var and "
                  "res must be NULL and relu 0");
  } else if (!beta || !running_mean || !running_var) {
    return fail("gmz_conv3x3_forward_split: the fused BatchNorm needs gamma, beta, running_mean and running_var");
  }
  if (((uintptr_t)x | (uintptr_t)packed | (uintptr_t)y | (uintptr_t)res) & 15)
    return fail("gmz_conv3x3_forward_split: operands must be 16-B aligned");
  if (y == x || (res && y == res)) return fail("gmz_conv3x3_forward_split: y must not alias x or res");
  const SplitBn bn = {gamma, beta, running_mean, running_var, res, eps, relu};
  const int rc = for_size(H, ConvSizes{}, [&](auto h) {
    return launch_conv3_split<decltype(h)::value>(x, packed, y, N, bn, (hipStream_t)stream);
  });
  return rc == -2 ? bad_size("gmz_conv3x3_forward_split") : rc;
}

GMZ_EXPORT int gmz_conv3x3_stats_slots(int N, int *slots) {
  if (N <= 0 || !slots) return fail("gmz_conv3x3_stats_slots: bad arguments");
  *slots = conv3_stats_slots(N, false);
  return 0;
}

GMZ_EXPORT int gmz_conv3x3_forward_stats(int dtype, int H, const void *x, const void *packed, void *y, int N,
                                         const uint8_t *mask, double *stats, int stats_slots, void *stream) {
  return conv3_forward("gmz_conv3x3_forward_stats", "gmz_conv3x3_forward", dtype, H, {x, packed, y}, {x, packed, y}, "", "",
                       x, packed, y, N, mask, stats, stats_slots, false, nullptr, stream);
}

GMZ_EXPORT int gmz_conv3x3_forward_board_stats(int dtype, int H, const void *x, const void *packed, void *y, int N,
                                               const uint8_t *mask, double *stats, int stats_slots, void *stream) {
  const char *fn = "gmz_conv3x3_forward_board_stats";
  return conv3_forward(fn, fn, dtype, H, {x, packed, y, stats}, {x, packed, y}, "", "", x, packed, y, N, mask, stats,
                       stats_slots, true, nullptr, stream);
}

GMZ_EXPORT int gmz_conv3x3_forward_stamp(int dtype, int H, const void *x, const void *packed, void *y, int N,
                                         const uint8_t *mask, double *stats, int stats_slots, const int32_t *action,
                                         const void *table, int table_dtype, size_t table_bytes, void *stream) {
  const char *fn = "gmz_conv3x3_forward_stamp";
  // the kernel reads the table as f32 [9][128]: any other dtype or size fails before the launch (ABI 10; the
  // round-5 faults were an f16 table built inside autocast, read past its 2,304 bytes)
  std::string table_err;
  if (table_dtype != 0) table_err = "gmz_conv3x3_forward_stamp: table_dtype must be 0 (f32)";
  else if (table_bytes != (size_t)9 * CC * sizeof(float))
    table_err = "gmz_conv3x3_forward_stamp: table of " + std::to_string(table_bytes) + " bytes, must be f32 [9][128] = 4608";
  return conv3_forward(fn, fn, dtype, H, {x, packed, y, action, table}, {x, packed, y}, table_err, "", x, packed, y, N, mask,
                       stats, stats_slots, false, nullptr, stream, BnBwd{}, ActStamp{action, (const float *)table});
}

GMZ_EXPORT int gmz_conv3x3_forward_bnapply(int dtype, int H, const void *bn_x, const void *bn_res, const float *gamma,
                                           const float *beta, const float *bn_save, int relu, void *bn_y,
                                           const void *packed, void *y, int N, const uint8_t *mask, double *stats,
                                           int stats_slots, void *stream) {
  const char *fn = "gmz_conv3x3_forward_bnapply";
  const bool alias = bn_y == bn_x || bn_y == bn_res || bn_y == y || y == bn_x;
  const BnApply ba = {(const uint16_t *)bn_x, (const uint16_t *)bn_res, gamma, beta, bn_save, (uint16_t *)bn_y, relu};
  return conv3_forward(fn, fn, dtype, H, {bn_x, gamma, beta, bn_save, bn_y, packed, y}, {bn_x, bn_res, bn_y, packed, y}, "",
                       alias ? "gmz_conv3x3_forward_bnapply: the BatchNorm output, its input and the conv output must not alias"
                             : "",
                       bn_y, packed, y, N, mask, stats, stats_slots, false, nullptr, stream, BnBwd{}, ActStamp{}, ba);
}

GMZ_EXPORT int gmz_conv3x3_forward(int dtype, int H, const void *x, const void *packed, void *y, int N, void *stream) {
  return gmz_conv3x3_forward_stats(dtype, H, x, packed, y, N, nullptr, nullptr, 0, stream);
}

GMZ_EXPORT int gmz_conv3x3_forward_add(int dtype, int H, const void *x, const void *packed, const void *addend, void *y,
                                       int N, void *stream) {
  const char *fn = "gmz_conv3x3_forward_add";
  return conv3_forward(fn, fn, dtype, H, {x, packed, y, addend}, {x, packed, y, addend}, "", "", x, packed, y, N, nullptr,
                       nullptr, 0, false, addend, stream);
}

GMZ_EXPORT int gmz_conv3x3_forward_bwdstats(int dtype, int H, const void *x, const void *packed, const void *addend,
                                            void *y, int N, const uint8_t *mask, const void *bn_x, const void *bn_y,
                                            const float *bn_save, int relu, double *stats, int stats_slots,
                                            void *stream) {
  const char *fn = "gmz_conv3x3_forward_bwdstats";
  const bool bn_odd = (((uintptr_t)bn_x | (uintptr_t)bn_y) & 7) != 0;
  const BnBwd bn = {(const uint16_t *)bn_x, (const uint16_t *)bn_y, bn_save, relu};
  return conv3_forward(fn, fn, dtype, H, {x, packed, y, bn_x, bn_y, bn_save, stats}, {x, packed, y, addend}, "",
                       bn_odd ? "gmz_conv3x3_forward_bwdstats: BN operands must be 8-B aligned" : "", x, packed, y, N, mask,
                       stats, stats_slots, false, addend, stream, bn);
}

GMZ_EXPORT int gmz_conv3x3_wgrad_workspace_bytes(int N, size_t *out) {
  if (N <= 0 || !out) return fail("gmz_conv3x3_wgrad_workspace_bytes: bad arguments");
  *out = (size_t)wgrad_chunks(N) * 9 * CC * CC * sizeof(float);
  return 0;
}

static int wgrad_launch(int dtype, int H, const WgSrc &src, int N, float *dw, int64_t s0, int64_t s1, int64_t s2,
                        int64_t s3, int accumulate, void *workspace, size_t workspace_bytes, hipStream_t st) {
  if (for_size(H, ConvSizes{}, [](auto) { return 0; }) == -2) return bad_size("gmz_conv3x3_wgrad");
  const size_t need = (size_t)wgrad_chunks(N) * 9 * CC * CC * sizeof(float);  // the partials k_conv3_wgrad writes
  if (workspace_bytes < need)
    return fail("gmz_conv3x3_wgrad: workspace of " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(N) +
                " boards need " + std::to_string(need) + " (gmz_conv3x3_wgrad_workspace_bytes)");
  float *part = (float *)workspace;
  const int rc = by_dtype<false>("gmz_conv3x3_wgrad", dtype, [&](auto t) {
    return for_size(H, ConvSizes{}, [&](auto h) {
      return launch_wgrad<decltype(h)::value, dtype_of<decltype(t)>>(src, N, part, st);
    });
  });
  if (rc) return rc;
  hipLaunchKernelGGL(k_conv3_wgrad_reduce, dim3((9 * CC * CC + 255) / 256), dim3(256), 0, st, (const float *)part,
                     wgrad_chunks(N), dw, (long)s0, (long)s1, (long)s2, (long)s3, accumulate);
  GMZ_LAUNCH_CHECK();
  return 0;
}

GMZ_EXPORT int gmz_conv3x3_wgrad(int dtype, int H, const void *x, const void *dy, int N, float *dw, int64_t s0,
                                 int64_t s1, int64_t s2, int64_t s3, int accumulate, void *workspace,
                                 size_t workspace_bytes, void *stream) {
  if (!x || !dy || !dw || !workspace) return fail("gmz_conv3x3_wgrad: null operand");
  if (N <= 0) return fail("gmz_conv3x3_wgrad: N must be positive");
  if (((uintptr_t)x | (uintptr_t)dy) & 15) return fail("gmz_conv3x3_wgrad: operands must be 16-B aligned");
  WgSrc src = {};
  src.x[0] = (const uint16_t *)x;
  src.dy[0] = (const uint16_t *)dy;
  src.nps = N;
  return wgrad_launch(dtype, H, src, N, dw, s0, s1, s2, s3, accumulate, workspace, workspace_bytes, (hipStream_t)stream);
}

GMZ_EXPORT int gmz_conv3x3_wgrad_segments(int dtype, int H, const void *const *x_segs, const void *const *dy_segs,
                                          int nseg, int n_per_seg, float *dw, int64_t s0, int64_t s1, int64_t s2,
                                          int64_t s3, int accumulate, void *workspace, size_t workspace_bytes,
                                          void *stream) {
  if (!x_segs || !dy_segs || !dw || !workspace) return fail("gmz_conv3x3_wgrad_segments: null operand");
  if (nseg < 1 || nseg > WG_MAX_SEGS || n_per_seg <= 0)
    return fail("gmz_conv3x3_wgrad_segments: need 1 <= nseg <= 8 segments of n_per_seg > 0 boards");
  WgSrc src = {};
  for (int i = 0; i < nseg; ++i) {
    if (!x_segs[i] || !dy_segs[i]) return fail("gmz_conv3x3_wgrad_segments: null segment");
    if (((uintptr_t)x_segs[i] | (uintptr_t)dy_segs[i]) & 15)
      return fail("gmz_conv3x3_wgrad_segments: operands must be 16-B aligned");
    src.x[i] = (const uint16_t *)x_segs[i];
    src.dy[i] = (const uint16_t *)dy_segs[i];
  }
  src.nps = n_per_seg;
  return wgrad_launch(dtype, H, src, nseg * n_per_seg, dw, s0, s1, s2, s3, accumulate, workspace, workspace_bytes,
                      (hipStream_t)stream);
}
