// gmz_pack.hip — network.pack_weights on the device (gmz_net_pack): the trainer's float32 parameters and BatchNorm
// buffers go into the packed buffers of a gmz_net_weights in place, bit for bit what numpy computes on the host.
//
// Built with -ffp-contract=off (EXACT_SRCS), and every float32 operation numpy performs is one correctly rounded
// operation here, in numpy's order.  Add, subtract and multiply are the hardware's (__fadd_rn, __fsub_rn, __fmul_rn).
// The square root and the divide go through float64 (sqrt_rn, div_rn below): this toolchain's __fsqrt_rn is the
// native approximate v_sqrt_f32 (1 ulp: it missed numpy in 17 of 128 stem biases), and whether `/` and sqrtf are
// correctly rounded is a compiler option.  A float64 quotient or root of float32 operands, rounded once more to
// float32, IS the correctly rounded float32 result: 53 >= 2 * 24 + 2 bits leave no double rounding.
//   fold_bn      s = g / sqrt(v + 1e-4f);  shift = b - (m * s)
//   conv weight  w * s[o], then ONE rounding to the 16-bit type (e16_bits below, integer arithmetic: no dependence
//                on the wave's denormal or rounding mode)
//   dyn_action   the 16 rounded products ((wd[n][128 + c][t] * s[n]) * emb[c]) summed as numpy's einsum sums them:
//                one sum over c = 0..15 in that order from 0 for a source whose channels are not contiguous (a
//                plain state_dict), four partial sums for a channel-contiguous one (k_pack_towers; both orders
//                are pinned against numpy by tests/test_net_pack.py)
//   head bias    (bias * s) + shift
//
// Three launches per push:
//   k_pack_towers   grid (16, 4*blocks + 1): every 3x3 conv of the two towers and the dynamics conv.  A block stages the
//                   (32 output channels) x (the 32 input channels of one k-step) x (9 taps) block of one weight through
//                   LDS (36 KB), so the global reads follow the source's memory order whichever it is (OIHW: 576-B
//                   runs; channels-last: 64-B runs) and every 16-B fragment store lands in a 2-KB contiguous run.
//   k_pack_reward   grid (ceil(A / 16), 4, 4): reward_fc.0 [64][C*A] (NCHW flatten) -> B fragments over the NHWC order;
//                   a block stages 16 outputs x 32 channels x 16 positions (64-B runs in, 1-KB runs out).
//   k_pack_misc     the stem, the 1x1 head convs, the zero-padded FC weights (padding written), transposes, biases.
#include "gmz_common.h"

namespace gmz {
namespace {

constexpr int C = 128;
constexpr int HD = 64;
constexpr int CONV_FRAG_U16 = 9 * 4 * 8 * 64 * 8;  // one packed 3x3 conv
constexpr float BN_EPS = 1e-4f;

// One source tensor: its device pointer and its strides in ELEMENTS (dimensions the tensor lacks: 0).
struct Job {
  const float *p;
  long long s0, s1, s2, s3;
};
static_assert(sizeof(Job) == 40, "gmz_net_pack job entry");

// The canonical job-table order (include/gmz.h): conv groups of 5 entries (weight, bn.weight, bn.bias,
// bn.running_mean, bn.running_var), then the single tensors.
enum { G_W = 0, G_GAMMA, G_BETA, G_MEAN, G_VAR, GROUP = 5 };
__host__ __device__ constexpr int n_groups(int blocks) { return 2 + 4 * blocks; }
enum {
  S_EMB = 0,
  S_PCONV_W, S_PCONV_B, S_PBN_G, S_PBN_B, S_PBN_M, S_PBN_V,
  S_VCONV_W, S_VCONV_B, S_VBN_G, S_VBN_B, S_VBN_M, S_VBN_V,
  S_PFC_W, S_PFC_B, S_VFC1_W, S_VFC1_B, S_VFC2_W, S_VFC2_B,
  S_RFC1_W, S_RFC1_B, S_RFC2_W, S_RFC2_B,
  N_SINGLES
};
__host__ __device__ constexpr int n_jobs(int blocks) { return GROUP * n_groups(blocks) + N_SINGLES; }

struct Dst {
  uint16_t *repr_stem_w, *repr_convs, *dyn_convs, *reward_fc1_w;
  float *repr_stem_b, *repr_bias, *dyn_bias, *dyn_action, *head_conv_w, *head_conv_b, *policy_fc_w, *policy_fc_b,
      *value_fc1_w, *value_fc1_b, *value_fc2_w, *value_fc2_b, *reward_fc1_b, *reward_fc2_w, *reward_fc2_b;
  int A, blocks;
};

__device__ __forceinline__ int r16(int x) { return (x + 15) / 16 * 16; }

// float32 -> the 16-bit type's bit pattern, round to nearest even.  F16: clamped to +-65504 first (network._e16_bits),
// f16 subnormals kept.  Bf16: no clamp.
template <bool BF16>
__host__ __device__ __forceinline__ uint16_t e16_bits(float f) {
  const uint32_t u = __builtin_bit_cast(uint32_t, f);
  const uint32_t sign = (u >> 16) & 0x8000u;
  uint32_t a = u & 0x7fffffffu;
  if constexpr (BF16) {
    if (a > 0x7f800000u) return (uint16_t)0x7fc0u;
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
  } else {
    if (a > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);
    if (a > 0x477fe000u) a = 0x477fe000u;  // 65504
    if (a >= 0x38800000u)                  // >= 2^-14: a normal f16; the carry of the rounding walks into the exponent
      return (uint16_t)(sign | ((a + 0xfffu + ((a >> 13) & 1u) - 0x38000000u) >> 13));
    const uint32_t e = a >> 23;
    if (e < 102u) return (uint16_t)sign;  // < 2^-25: rounds to zero
    const uint32_t m = (a & 0x7fffffu) | 0x800000u, sh = 126u - e;  // 14..24: the result counts units of 2^-24
    uint32_t q = m >> sh;
    const uint32_t rem = m & ((1u << sh) - 1u), half = 1u << (sh - 1u);
    if (rem > half || (rem == half && (q & 1u))) ++q;
    return (uint16_t)(sign | q);
  }
}

__device__ __forceinline__ uint4 pack8(const uint16_t (&b)[8]) {
  uint4 r;
  r.x = (uint32_t)b[0] | ((uint32_t)b[1] << 16);
  r.y = (uint32_t)b[2] | ((uint32_t)b[3] << 16);
  r.z = (uint32_t)b[4] | ((uint32_t)b[5] << 16);
  r.w = (uint32_t)b[6] | ((uint32_t)b[7] << 16);
  return r;
}

__device__ __forceinline__ float sqrt_rn(float x) { return (float)sqrt((double)x); }
__device__ __forceinline__ float div_rn(float a, float b) { return (float)((double)a / (double)b); }

// network.fold_bn for channel o of conv group g
__device__ __forceinline__ void fold_bn(const Job *g, int o, float &s, float &shift) {
  const float gamma = g[G_GAMMA].p[o * g[G_GAMMA].s0], beta = g[G_BETA].p[o * g[G_BETA].s0];
  const float mean = g[G_MEAN].p[o * g[G_MEAN].s0], var = g[G_VAR].p[o * g[G_VAR].s0];
  s = div_rn(gamma, sqrt_rn(__fadd_rn(var, BN_EPS)));
  shift = __fsub_rn(beta, __fmul_rn(mean, s));
}

// network.output_channel: the output channel of MFMA row m of n-tile nt
__device__ __forceinline__ int output_channel(int nt, int m) { return (nt >> 1) * 32 + 8 * (m >> 2) + 4 * (nt & 1) + (m & 3); }

// ------------------------------------------------------------------ towers
// blockIdx.y = layer: 0 .. 2*blocks-1 the representation tower's convs (conv group 1 + layer), then the dynamics
// conv (group 1 + 2*blocks, 144 input channels: the first 128 are packed, the last 16 fold into dyn_action) and the
// dynamics tower's convs.  blockIdx.x = u * 4 + ks: output channels 32u .. 32u+31 (n-tiles 2u, 2u+1), k-step ks =
// input channels [16 ks, 16 ks + 16) and [64 + 16 ks, 64 + 16 ks + 16) (network.conv_input_channel: lane group g reads
// chunk 2 ks + {0, 8, 1, 9}[g]).
constexpr int T_RS = 32 * 9 + 1;  // LDS row (one output channel: [32 channels][9 taps]) + 1: rows on different banks

template <bool BF16>
__global__ void __launch_bounds__(256) k_pack_towers(const Job *__restrict__ jobs, Dst d) {
  __shared__ float tile[32 * T_RS];
  __shared__ float scale[32];
  const int layer = blockIdx.y, u = blockIdx.x >> 2, ks = blockIdx.x & 3, tid = threadIdx.x;
  const int dl = layer - 2 * d.blocks;  // >= 0: layer dl of the dynamics net
  const Job *g = jobs + GROUP * (1 + layer);
  uint16_t *out = (dl < 0 ? d.repr_convs + (size_t)layer * CONV_FRAG_U16 : d.dyn_convs + (size_t)dl * CONV_FRAG_U16);
  float *bias = dl < 0 ? d.repr_bias + layer * C : d.dyn_bias + dl * C;
  const Job w = g[G_W];
  if (tid < 32) {
    float s, shift;
    fold_bn(g, 32 * u + tid, s, shift);
    scale[tid] = s;
    if (ks == 0) bias[32 * u + tid] = shift;
  }
  // stage [32 n][32 c][9 t]; consecutive threads follow the source's memory order
  const bool c_fastest = w.s1 == 1;  // channels-last ([o][ky][kx][c] in memory)
  for (int e = tid; e < 32 * 32 * 9; e += 256) {
    const int n = e / 288, r = e % 288;
    int cl, t;
    if (c_fastest) {
      t = r >> 5;
      cl = r & 31;
    } else {
      cl = r / 9;
      t = r % 9;
    }
    const int c = (cl >> 4) * 64 + 16 * ks + (cl & 15);
    tile[n * T_RS + cl * 9 + t] = w.p[(32 * u + n) * w.s0 + c * w.s1 + (t / 3) * w.s2 + (t % 3) * w.s3];
  }
  __syncthreads();
  for (int f = tid; f < 9 * 2 * 64; f += 256) {
    const int l = f & 63, b = (f >> 6) & 1, t = f >> 7, m = l & 15, grp = l >> 4;
    const int n = 8 * (m >> 2) + 4 * b + (m & 3);            // output_channel(2u + b, m) - 32u
    const int cl = (grp & 1) * 16 + (grp >> 1) * 8;          // chunk 2 ks + {0, 8, 1, 9}[grp]
    const float s = scale[n];
    uint16_t bits[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) bits[j] = e16_bits<BF16>(__fmul_rn(tile[n * T_RS + (cl + j) * 9 + t], s));
    *(uint4 *)(out + ((size_t)((t * 4 + ks) * 8 + 2 * u + b) * 64 + l) * 8) = pack8(bits);
  }
  if (dl == 0 && ks == 0) {  // dyn_action [9][C] from the dynamics conv's 16 action-embedding input channels
    const Job emb = jobs[GROUP * n_groups(d.blocks) + S_EMB];
    for (int e = tid; e < 32 * 9; e += 256) {
      const int n = e / 9, t = e % 9, o = 32 * u + n;
      const float s = scale[n];
      float prod[16];
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        const float wd = __fmul_rn(w.p[o * w.s0 + (C + c) * w.s1 + (t / 3) * w.s2 + (t % 3) * w.s3], s);
        prod[c] = __fmul_rn(wd, emb.p[c * emb.s0]);
      }
      float acc;
      if (c_fastest) {
        // numpy's einsum over a channel-contiguous operand (the host copy of a channels-last weight keeps its
        // strides, and so does w * s): its contiguous sum-of-products loop keeps four partial sums, lane i over
        // c = i (mod 4), adds the 16 products in the order c = 12.., 8.., 4.., 0.. and ends (l0 + l1) + (l2 + l3)
        float lane[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 3; k >= 0; --k)
#pragma unroll
          for (int i = 0; i < 4; ++i) lane[i] = __fadd_rn(prod[4 * k + i], lane[i]);
        acc = __fadd_rn(__fadd_rn(lane[0], lane[1]), __fadd_rn(lane[2], lane[3]));
      } else {  // any other layout: numpy's strided loop, one sum in channel order from 0
        acc = 0.0f;
#pragma unroll
        for (int c = 0; c < 16; ++c) acc = __fadd_rn(acc, prod[c]);
      }
      d.dyn_action[t * C + o] = acc;
    }
  }
}

// ------------------------------------------------------------------ reward_fc.0
// network.pack_reward_fc1: frag(kk, nt, l, j) = W[n = 16 nt + (l & 15)][c * A + p], k = p * C + c = 32 kk + 8 (l >> 4) + j.
// Block (pt, cq, nt): positions 16 pt .. 16 pt + 15, channels 32 cq .. 32 cq + 31, outputs 16 nt .. 16 nt + 15.
constexpr int R_CS = 17;            // LDS: [n][c][16 p] with the p row padded to 17, the n row to an odd length: the
constexpr int R_NS = 32 * R_CS + 1;  // 16 outputs a fragment read walks sit on 16 banks (2-way with the other c group)

template <bool BF16>
__global__ void __launch_bounds__(256) k_pack_reward(const Job *__restrict__ jobs, Dst d) {
  __shared__ float tile[16 * R_NS];
  const Job w = jobs[GROUP * n_groups(d.blocks) + S_RFC1_W];
  const int p0 = 16 * blockIdx.x, cq = blockIdx.y, nt = blockIdx.z, tid = threadIdx.x, A = d.A;
  for (int e = tid; e < 16 * 32 * 16; e += 256) {
    const int pp = e & 15, c = (e >> 4) & 31, n = e >> 9;
    if (p0 + pp < A)
      tile[n * R_NS + c * R_CS + pp] = w.p[(16 * nt + n) * w.s0 + (long long)((32 * cq + c) * A + p0 + pp) * w.s1];
  }
  __syncthreads();
  for (int f = tid; f < 16 * 64; f += 256) {
    const int l = f & 63, pp = f >> 6, n = l & 15, c0 = 8 * (l >> 4);
    if (p0 + pp >= A) break;
    uint16_t bits[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) bits[j] = e16_bits<BF16>(tile[n * R_NS + (c0 + j) * R_CS + pp]);
    const int kk = (p0 + pp) * 4 + cq;
    *(uint4 *)(d.reward_fc1_w + ((size_t)(kk * 4 + nt) * 64 + l) * 8) = pack8(bits);
  }
}

// ------------------------------------------------------------------ everything else
// blocks [0, np): policy_fc_w [r16(A)][r16(2A)], one element per thread; [np, np + nv): value_fc1_w [64][r16(A)];
// the last block: the stem, the head convs, the transposes and the bias copies.
template <bool BF16>
__global__ void __launch_bounds__(256) k_pack_misc(const Job *__restrict__ jobs, Dst d, int np, int nv) {
  const Job *S = jobs + GROUP * n_groups(d.blocks);
  const int tid = threadIdx.x, A = d.A, RA = r16(A), R2A = r16(2 * A);
  int b = blockIdx.x;
  if (b < np) {
    const int i = b * 256 + tid;
    if (i < RA * R2A) {
      const int r = i / R2A, c = i % R2A;
      const Job w = S[S_PFC_W];
      d.policy_fc_w[i] = (r < A && c < 2 * A) ? w.p[r * w.s0 + c * w.s1] : 0.0f;
    }
    return;
  }
  b -= np;
  if (b < nv) {
    const int i = b * 256 + tid;
    if (i < HD * RA) {
      const int r = i / RA, c = i % RA;
      const Job w = S[S_VFC1_W];
      d.value_fc1_w[i] = c < A ? w.p[r * w.s0 + c * w.s1] : 0.0f;
    }
    return;
  }
  __shared__ float scale[C];
  __shared__ float hs[3];
  if (tid < C) {  // the stem's BatchNorm (conv group 0)
    float s, shift;
    fold_bn(jobs, tid, s, shift);
    scale[tid] = s;
    d.repr_stem_b[tid] = shift;
  }
  if (tid >= C && tid < C + 3) {  // policy_bn (channels 0, 1) and value_bn: head_conv_b = (bias * s) + shift
    const int k = tid - C, o = k < 2 ? k : 0;
    const Job *bn = S + (k < 2 ? S_PBN_G : S_VBN_G);
    const Job cb = S[k < 2 ? S_PCONV_B : S_VCONV_B];
    const float gamma = bn[0].p[o * bn[0].s0], beta = bn[1].p[o * bn[1].s0];
    const float mean = bn[2].p[o * bn[2].s0], var = bn[3].p[o * bn[3].s0];
    const float s = div_rn(gamma, sqrt_rn(__fadd_rn(var, BN_EPS)));
    const float shift = __fsub_rn(beta, __fmul_rn(mean, s));
    hs[k] = s;
    d.head_conv_b[k] = __fadd_rn(__fmul_rn(cb.p[o * cb.s0], s), shift);
  }
  __syncthreads();
  {  // network.pack_stem: [8][64][8], k = tap * 3 + c (27, zero padded to 32)
    const Job w = jobs[G_W];
    for (int f = tid; f < 8 * 64; f += 256) {
      const int l = f & 63, nt = f >> 6, n = output_channel(nt, l & 15);
      uint16_t bits[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int k = 8 * (l >> 4) + j, t = k / 3, c = k % 3;
        bits[j] = k < 27 ? e16_bits<BF16>(__fmul_rn(w.p[n * w.s0 + c * w.s1 + (t / 3) * w.s2 + (t % 3) * w.s3], scale[n]))
                         : (uint16_t)0;
      }
      *(uint4 *)(d.repr_stem_w + (size_t)f * 8) = pack8(bits);
    }
  }
  for (int i = tid; i < 3 * C; i += 256) {  // head_conv_w [3][C]
    const int k = i / C, c = i % C;
    const Job w = S[k < 2 ? S_PCONV_W : S_VCONV_W];
    d.head_conv_w[i] = __fmul_rn(w.p[(k < 2 ? k : 0) * w.s0 + c * w.s1], hs[k]);
  }
  for (int i = tid; i < A; i += 256) d.policy_fc_b[i] = S[S_PFC_B].p[i * S[S_PFC_B].s0];
  if (tid < HD) {
    d.value_fc1_b[tid] = S[S_VFC1_B].p[tid * S[S_VFC1_B].s0];
    d.reward_fc1_b[tid] = S[S_RFC1_B].p[tid * S[S_RFC1_B].s0];
  }
  if (tid < 3) {
    d.value_fc2_b[tid] = S[S_VFC2_B].p[tid * S[S_VFC2_B].s0];
    d.reward_fc2_b[tid] = S[S_RFC2_B].p[tid * S[S_RFC2_B].s0];
  }
  if (tid < HD * 3) {  // [3][hd] -> [hd][3]
    const int h = tid / 3, k = tid % 3;
    d.value_fc2_w[tid] = S[S_VFC2_W].p[k * S[S_VFC2_W].s0 + h * S[S_VFC2_W].s1];
    d.reward_fc2_w[tid] = S[S_RFC2_W].p[k * S[S_RFC2_W].s0 + h * S[S_RFC2_W].s1];
  }
}

template <bool BF16>
int launch_pack(const Job *jobs, const Dst &d, hipStream_t s) {
  const int A = d.A, RA = (A + 15) / 16 * 16, R2A = (2 * A + 15) / 16 * 16;
  hipLaunchKernelGGL(k_pack_towers<BF16>, dim3(16, 4 * d.blocks + 1), dim3(256), 0, s, jobs, d);
  GMZ_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_pack_reward<BF16>, dim3((A + 15) / 16, 4, 4), dim3(256), 0, s, jobs, d);
  GMZ_LAUNCH_CHECK();
  const int np = (RA * R2A + 255) / 256, nv = (HD * RA + 255) / 256;
  hipLaunchKernelGGL(k_pack_misc<BF16>, dim3(np + nv + 1), dim3(256), 0, s, jobs, d, np, nv);
  GMZ_LAUNCH_CHECK();
  return 0;
}

constexpr int MAX_BLOCKS = 4096;  // grid.y of k_pack_towers = 4 * blocks + 1 <= 65535

}  // namespace
}  // namespace gmz

using namespace gmz;

GMZ_EXPORT int gmz_net_pack_job_bytes(int blocks, size_t *out) {
  if (!out) return fail("gmz_net_pack_job_bytes: null");
  if (blocks < 1 || blocks > MAX_BLOCKS)
    return fail("gmz_net_pack_job_bytes: blocks must be 1 to " + std::to_string(MAX_BLOCKS));
  *out = sizeof(Job) * (size_t)n_jobs(blocks);
  return 0;
}

GMZ_EXPORT int gmz_net_pack(const gmz_net_weights *w, const void *jobs, size_t jobs_bytes, void *stream) {
  if (!w) return fail("gmz_net_pack: null weights");
  if (w->channels != C) return fail("gmz_net_pack: channels must be 128");
  if (w->head_hidden != HD) return fail("gmz_net_pack: head_hidden must be 64");
  if (w->blocks < 1 || w->blocks > MAX_BLOCKS)
    return fail("gmz_net_pack: blocks must be 1 to " + std::to_string(MAX_BLOCKS));
  if (w->board_size < 5 || w->board_size > 19)  // the sizes the towers are built for, in every gmz_net_* call's words
    return fail("gmz_net_pack: board_size must be 5 to 19 (20 to 22, which the tree kernels accept, have no tower kernels)");
  if (w->dtype != GMZ_NET_F16 && w->dtype != GMZ_NET_BF16)
    return fail("gmz_net_pack: dtype must be GMZ_NET_F16 or GMZ_NET_BF16");
  const struct {
    const void *p;
    const char *name;
  } dsts[] = {{w->repr_stem_w, "repr_stem_w"},   {w->repr_stem_b, "repr_stem_b"},   {w->repr_convs, "repr_convs"},
              {w->repr_bias, "repr_bias"},       {w->dyn_convs, "dyn_convs"},       {w->dyn_bias, "dyn_bias"},
              {w->dyn_action, "dyn_action"},     {w->head_conv_w, "head_conv_w"},   {w->head_conv_b, "head_conv_b"},
              {w->policy_fc_w, "policy_fc_w"},   {w->policy_fc_b, "policy_fc_b"},   {w->value_fc1_w, "value_fc1_w"},
              {w->value_fc1_b, "value_fc1_b"},   {w->value_fc2_w, "value_fc2_w"},   {w->value_fc2_b, "value_fc2_b"},
              {w->reward_fc1_w, "reward_fc1_w"}, {w->reward_fc1_b, "reward_fc1_b"}, {w->reward_fc2_w, "reward_fc2_w"},
              {w->reward_fc2_b, "reward_fc2_b"}};
  for (const auto &t : dsts) {
    if (!t.p) return fail(std::string("gmz_net_pack: null destination ") + t.name);
    if ((uintptr_t)t.p & 15) return fail(std::string("gmz_net_pack: destination ") + t.name + " must be 16-byte aligned");
  }
  if (!jobs) return fail("gmz_net_pack: null job table");
  const size_t need = sizeof(Job) * (size_t)n_jobs(w->blocks);
  if (jobs_bytes != need)
    return fail("gmz_net_pack: job table of " + std::to_string(jobs_bytes) + " bytes, " + std::to_string(w->blocks) +
                " blocks need " + std::to_string(need) + " (gmz_net_pack_job_bytes)");
  Dst d;
  d.repr_stem_w = (uint16_t *)w->repr_stem_w;
  d.repr_convs = (uint16_t *)w->repr_convs;
  d.dyn_convs = (uint16_t *)w->dyn_convs;
  d.reward_fc1_w = (uint16_t *)w->reward_fc1_w;
  d.repr_stem_b = (float *)w->repr_stem_b;
  d.repr_bias = (float *)w->repr_bias;
  d.dyn_bias = (float *)w->dyn_bias;
  d.dyn_action = (float *)w->dyn_action;
  d.head_conv_w = (float *)w->head_conv_w;
  d.head_conv_b = (float *)w->head_conv_b;
  d.policy_fc_w = (float *)w->policy_fc_w;
  d.policy_fc_b = (float *)w->policy_fc_b;
  d.value_fc1_w = (float *)w->value_fc1_w;
  d.value_fc1_b = (float *)w->value_fc1_b;
  d.value_fc2_w = (float *)w->value_fc2_w;
  d.value_fc2_b = (float *)w->value_fc2_b;
  d.reward_fc1_b = (float *)w->reward_fc1_b;
  d.reward_fc2_w = (float *)w->reward_fc2_w;
  d.reward_fc2_b = (float *)w->reward_fc2_b;
  d.A = w->board_size * w->board_size;
  d.blocks = w->blocks;
  return w->dtype == GMZ_NET_BF16 ? launch_pack<true>((const Job *)jobs, d, (hipStream_t)stream)
                                  : launch_pack<false>((const Job *)jobs, d, (hipStream_t)stream);
}
