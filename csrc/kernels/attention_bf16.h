// The attention core on the bf16 matrix instruction: softmax(Q K^T) V per (group, head) for bf16 activations, head
// sizes d and dv that are multiples of 16 up to 128, plain, causal, grouped-query and grouped-query causal, gfx950.
// Opt-in (`math="bf16"`): the default stays the fp32-math kernels of attention_core.h, which widen bf16 rows while
// they stage them and run both products on v_mfma_f32_16x16x4_f32.  Here both products run on
// v_mfma_f32_16x16x32_bf16 with fp32 accumulation and the softmax stays in fp32.  The scheme's outline (swapped
// score product, online softmax in the lane that owns the query, the source policy `Src`) is the one
// attention_core.h describes; what follows is what this kernel does on its own.
//
//   * Split.  A block of 4 waves owns one (group, head, tile of B16_QT = 64 queries), a wave 16 of the queries.  The
//     block walks the keys B16_KT = 64 at a time: with 2 bytes per element a 64-key tile takes the LDS that 32 keys
//     take in fp32 (35,840 bytes at DMAX = 128: four blocks per CU).  K and V of tile t + 1 are fetched into registers
//     with predicated 16-byte loads while tile t is computed.
//   * K in LDS: rows of DMAX + 8 bf16, as loaded, no widening.  The A operand of a K = 32 step is, per lane, 8
//     consecutive channels of key `lane & 15`: one 16-byte read at row c, channel 32 t + 8 g.  A row is (DMAX + 8) / 2
//     dwords = 4 x odd (20, 36, 68), so the 16 lanes of a group start at 16 different multiples of 4 banks modulo 64:
//     each lane's four banks are its own, the read is conflict-free (and so is each half on 32 banks).
//   * Score product, swapped: S^T = K Q^T, M = key, N = query.  Q is held for the whole kernel as DMAX / 32 bf16x8
//     fragments (channels 32 t + 8 g .. + 7 of query c).  A lane of the result holds for query `lane & 15` the keys
//     16 u + 4 g + i, as in the fp32 kernel.  d % 32 == 16: a zero half-step.  K rows are staged up to the next
//     multiple of 32 channels with zeros behind d, and the Q fragment of those lanes is zero, so the last step adds
//     exact zeros; the K = 16 instruction would need a second operand shape for one slice.
//   * Probabilities: p = exp2(s log2 e - m log2 e) in fp32 (v_exp_f32, log2 e folded into one fma), rounded once to
//     bf16 (round to nearest even) and never written to LDS: the fragments u = 2 w and 2 w + 1 give a lane 8 keys,
//     and that is the B operand of one K = 32 step of O^T = V^T P^T when k slot (g, j) of step w is taken to mean the
//     key 32 w + 16 (j >> 2) + 4 g + (j & 3).  The row sum is taken from the unrounded fp32 probabilities.
//   * V in LDS: transposed and key-permuted, one row of B16_KT + 8 bf16 per channel, key 32 w + 16 hh + 4 g + i at
//     position 32 w + 8 g + 4 hh + i.  The A operand of the step above (channel 16 n + c, the lane's 8 keys) is then
//     one 16-byte read at row 16 n + c, position 32 w + 8 g; rows of 36 dwords = 4 x 9, conflict-free as for K.  The
//     transpose is paid once per block while staging, not once per wave while reading: a thread loads 8 channels of
//     4 consecutive keys (four 16-byte loads), transposes the 4 x 8 block in registers with 16 and / shift / or
//     pairs, and writes 8 rows of 4 keys (8-byte stores).  4 consecutive keys 4 q .. 4 q + 3 are consecutive
//     positions, so no lane exchange is needed.  (The LDS transpose read and key-pair packing by lane exchange were
//     not built: BASELINE.md "Round 22".)
//   * Online softmax: running maximum m, running sum l (this lane's keys, summed over the lane groups at the end) and
//     alpha in fp32 in the lane that owns the query; a row maximum is the in-lane registers plus two `__shfl_xor`
//     steps.  O stays in fp32 accumulators, is scaled by 1 / l and rounded once at the store.
//   * Fragments that hold no visible key are skipped, not computed and masked: `nu`, the number of 16-key fragments
//     of the tile a wave computes, ends at the key bound and, under the causal mask, at the wave's last query.  It is
//     wave-uniform, and it is used after both barriers only.
//
// Invariants carried over from attention_core.h.  K / V rows at or beyond the key bound are staged as zeros by
// predicated loads and their scores are set to -inf before the maximum is taken.  Queries beyond the count load
// zeros, are carried and not stored.  The key loop's trip count and the key bound are block-uniform, both barriers of
// an iteration come before the `active` test, and no barrier follows the loop.  Causal: blocks run heaviest query
// tile first; the key loop and the prefetch end at the tile's last query; a wave whose queries all lie before a
// tile skips it after the barriers; a future key's score becomes -inf in the statement that masks the keys beyond
// the count; where the running and the tile maximum are both -inf the exponents are taken against 0.  Channels
// heads * dv .. ld_out - 1 of a row are written as zeros.  Index math is 32-bit behind the front-end's refusals.
// Every global access is a 16-byte (Q, K, V) or 8-byte (out) vector: pointers and row strides must be multiples of
// 8 elements (`attention_vec8`).
#pragma once
#include "attention_core.h"

namespace adapt {
namespace attn {

constexpr int B16_QT = 64;    // queries per block (4 waves x 16)
constexpr int B16_KT = 64;    // keys per LDS tile
constexpr int B16_PAD = 8;    // bf16 of padding per LDS row

inline bool attention_vec8(uintptr_t ptrs, int strides) { return (strides & 7) == 0 && (ptrs & 15) == 0; }

__device__ __forceinline__ u32x4 ld8(const bf16* p) { return *(const u32x4*)p; }

// The kernel below is compiled without the packed fp32 instructions (the `target` attribute on it), and a function
// is inlined into it on its own only when it carries the same attribute.  The policies are shared with the fp32-math
// kernels and stay as they are, so their members are called through these wrappers, which ask for the inlining at
// the call
template <typename Src>
struct B16 {
  using Block = typename Src::Block;
  static __device__ __forceinline__ Block block(const Src& s, int grp, int h) { [[clang::always_inline]] return s.block(grp, h); }
  static __device__ __forceinline__ int dv(const Src& s) { [[clang::always_inline]] return s.dv(); }
  static __device__ __forceinline__ int nq(const Src& s) { [[clang::always_inline]] return s.nq(); }
  static __device__ __forceinline__ int nk(const Src& s) { [[clang::always_inline]] return s.nk(); }
  static __device__ __forceinline__ const bf16* q(const Src& s, const Block& b, int r) { [[clang::always_inline]] return s.q(b, r); }
  static __device__ __forceinline__ const bf16* k(const Src& s, const Block& b, int r) { [[clang::always_inline]] return s.k(b, r); }
  static __device__ __forceinline__ const bf16* v(const Src& s, const Block& b, int r) { [[clang::always_inline]] return s.v(b, r); }
  static __device__ __forceinline__ int out_row(const Src& s, const Block& b, int r) { [[clang::always_inline]] return s.out_row(b, r); }
};

// DMAX: the head sizes this instantiation holds in registers (d, dv <= DMAX, both multiples of 16)
template <int DMAX, typename Src, bool CAUSAL>
__global__ __launch_bounds__(256, DMAX == 128 ? 3 : DMAX == 64 ? 4 : 5) __attribute__((target("no-packed-fp32-ops")))
void attention_bf16_kernel(Src src, bf16* __restrict__ out, int ld_out, int qtiles) {
  constexpr int QT = B16_QT, KT = B16_KT;
  constexpr int NT = DMAX / 32;                       // K = 32 steps of the score product
  constexpr int ND = DMAX / 16;                       // 16-channel slices of the output
  constexpr int NU = KT / 16;                         // 16-key score fragments per tile
  constexpr int LDK = DMAX + B16_PAD;                 // bf16 per K row
  constexpr int LDV = KT + B16_PAD;                   // bf16 per transposed V row
  constexpr int NSK = KT * (DMAX / 8) / 256;          // staged K vectors per thread
  constexpr float LOG2E = 1.4426950408889634f;
  static_assert(KT == 64 && NSK >= 1, "the V staging below covers 16 key quads, one unit per thread");
  __shared__ __attribute__((aligned(16))) bf16 smem[KT * LDK + DMAX * LDV];
  bf16* sk = smem;
  bf16* sv = smem + KT * LDK;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int heads = src.heads, d = src.d, dv = B16<Src>::dv(src), Tq = B16<Src>::nq(src), Tk = B16<Src>::nk(src);
  int bid = blockIdx.x;
  int qt_;
  if constexpr (CAUSAL) {                             // the heaviest query tiles first, as in the core
    const int gh = gridDim.x / qtiles;
    qt_ = qtiles - 1 - bid / gh;
    bid %= gh;
  } else {
    qt_ = bid % qtiles;
    bid /= qtiles;
  }
  const int qt = qt_;
  const int h = bid % heads;
  const typename Src::Block b = B16<Src>::block(src, bid / heads, h);

  // what this thread stages of every key tile.  K: vector `idx` (8 channels) of the rows, d rounded up to 32 channels
  // with zeros behind d.  V: 8 channels of the key quad 4 vq .. 4 vq + 3, written transposed
  const int nkv = ((d + 31) & ~31) >> 3, nvv = dv >> 3;
  int krow[NSK], kcol[NSK];
  bool kval[NSK], kreal[NSK];
#pragma unroll
  for (int j = 0; j < NSK; ++j) {
    const int idx = tid + j * 256;
    kval[j] = idx < KT * nkv;
    krow[j] = kval[j] ? idx / nkv : 0;
    kcol[j] = kval[j] ? 8 * (idx - krow[j] * nkv) : 0;
    kreal[j] = kval[j] && kcol[j] < d;
  }
  // the quad on the fast lane index: 16 lanes write the 64 keys of one channel row, 128 contiguous bytes
  const bool vval = (tid >> 4) < nvv;
  const int vq = tid & 15;
  const int vcol = vval ? 8 * (tid >> 4) : 0;
  // key 4 vq + e = 32 w + 16 hh + 4 g + e stands at position 32 w + 8 g + 4 hh + e of a channel's row
  bf16* const vdst = sv + vcol * LDV + 32 * (vq >> 3) + 8 * (vq & 3) + 4 * ((vq >> 2) & 1);

  const int q0 = qt * QT + wave * 16;
  const bool active = q0 < Tq;                        // wave-uniform
  const int qtok = q0 + c;
  const bool qok = qtok < Tq;
  // block-uniform (from qt, never from wave): every wave passes both barriers of every iteration
  int kend = Tk;
  if constexpr (CAUSAL) kend = min(Tk, (qt + 1) * QT);

  bf16x8 qf[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    V8 x;
    x.u = u32x4{0u, 0u, 0u, 0u};
    if (qok && 32 * t + 8 * g < d) x.u = ld8(B16<Src>::q(src, b, qtok) + 32 * t + 8 * g);
    qf[t] = x.h;
  }
  f32x4 o[ND];
#pragma unroll
  for (int n = 0; n < ND; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;                       // l: this lane's keys only, summed over the groups at the end

  u32x4 pk[NSK], pv[4];
#pragma unroll
  for (int j = 0; j < NSK; ++j) {
    pk[j] = u32x4{0u, 0u, 0u, 0u};
    if (kreal[j] && krow[j] < kend) pk[j] = ld8(B16<Src>::k(src, b, krow[j]) + kcol[j]);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    pv[e] = u32x4{0u, 0u, 0u, 0u};
    if (vval && 4 * vq + e < kend) pv[e] = ld8(B16<Src>::v(src, b, 4 * vq + e) + vcol);
  }
  for (int k0 = 0; k0 < kend; k0 += KT) {             // the same trip count for every wave of the block
    __syncthreads();                                  // the previous tile has been read
#pragma unroll
    for (int j = 0; j < NSK; ++j)
      if (kval[j]) *(u32x4*)(sk + krow[j] * LDK + kcol[j]) = pk[j];
    if (vval) {
#pragma unroll
      for (int p = 0; p < 4; ++p) {                   // dword p of a key's vector: channels 2 p and 2 p + 1
        const uint32_t x0 = pv[0][p], x1 = pv[1][p], x2 = pv[2][p], x3 = pv[3][p];
        *(uint2*)(vdst + (2 * p) * LDV) = make_uint2((x0 & 0xffffu) | (x1 << 16), (x2 & 0xffffu) | (x3 << 16));
        *(uint2*)(vdst + (2 * p + 1) * LDV) = make_uint2((x0 >> 16) | (x1 & 0xffff0000u), (x2 >> 16) | (x3 & 0xffff0000u));
      }
    }
    __syncthreads();
    if (k0 + KT < kend) {                             // causal: no tile the block will not use is loaded
#pragma unroll
      for (int j = 0; j < NSK; ++j) {
        pk[j] = u32x4{0u, 0u, 0u, 0u};                // rows beyond the key bound are zeros, never loaded
        const int r = k0 + KT + krow[j];
        if (kreal[j] && r < kend) pk[j] = ld8(B16<Src>::k(src, b, r) + kcol[j]);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        pv[e] = u32x4{0u, 0u, 0u, 0u};
        const int r = k0 + KT + 4 * vq + e;
        if (vval && r < kend) pv[e] = ld8(B16<Src>::v(src, b, r) + vcol);
      }
    }
    if (!active) continue;                            // after both barriers: the wave only helps staging
    // the fragments of this tile that hold a key some query of the wave attends: wave-uniform, at least 1
    int nu = min(NU, (kend - k0 + 15) >> 4);
    if constexpr (CAUSAL) {
      if (k0 > q0 + 15) continue;                     // every key of the tile lies after the wave's 16 queries
      nu = min(nu, ((q0 + 15 - k0) >> 4) + 1);
    }
    // S^T = K Q^T: s[u][i] = score(key k0 + 16 u + 4 g + i, query c)
    f32x4 s[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      s[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (u < nu) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
          if (32 * t < d) {
            const bf16x8 kf = *(const bf16x8*)(sk + (16 * u + c) * LDK + 32 * t + 8 * g);
            s[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[t], s[u], 0, 0, 0);
          }
      }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int u = 0; u < NU; ++u)
      if (u < nu) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int key = k0 + 16 * u + 4 * g + i;
          bool masked = key >= Tk;
          if constexpr (CAUSAL) masked = masked || key > qtok;                  // before the maximum is taken
          if (masked) s[u][i] = -INFINITY;
          mx = fmaxf(mx, s[u][i]);
        }
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float mn = fmaxf(m, mx);
    float me = mn;                                    // what the exponents are taken against
    if constexpr (CAUSAL) {
      if (mn == -INFINITY) me = 0.f;                  // never exp(-inf - -inf): the core's guard
    }
    const float mel = me * LOG2E;
    const float alpha = __builtin_amdgcn_exp2f(__builtin_fmaf(m, LOG2E, -mel));   // 0 on the first tile (m = -inf)
    m = mn;
    float ps = 0.f;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      if (u < nu) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          s[u][i] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[u][i], LOG2E, -mel));   // masked keys: exp2(-inf) = 0
          ps += s[u][i];
        }
      } else {
        s[u] = f32x4{0.f, 0.f, 0.f, 0.f};             // the other half of a K = 32 step that is computed
      }
    }
    l = l * alpha + ps;
#pragma unroll
    for (int n = 0; n < ND; ++n) o[n] *= alpha;
    // O^T += V^T P^T: o[n][i] = O(query c, channel 16 n + 4 g + i); k slot (g, j) of step w is the key
    // 32 w + 16 (j >> 2) + 4 g + (j & 3), which is where the fragments 2 w and 2 w + 1 hold it
#pragma unroll
    for (int w = 0; w < NU / 2; ++w)
      if (2 * w < nu) {
        bf16x8 pb;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          pb[i] = f2bf(s[2 * w][i]);
          pb[4 + i] = f2bf(s[2 * w + 1][i]);
        }
#pragma unroll
        for (int n = 0; n < ND; ++n)
          if (16 * n < dv) {
            const bf16x8 vf = *(const bf16x8*)(sv + (16 * n + c) * LDV + 32 * w + 8 * g);
            o[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pb, o[n], 0, 0, 0);
          }
      }
  }
  if (!active) return;                                // no barrier follows
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (!qok) return;
  const float inv = 1.f / l;
  bf16* orow = out + B16<Src>::out_row(src, b, qtok) * ld_out;
#pragma unroll
  for (int n = 0; n < ND; ++n)
    if (16 * n < dv) st4(orow + h * dv + 16 * n + 4 * g, o[n] * inv);
  if (h == heads - 1)                                 // layout padding of the row: zeros
    for (int cc = heads * dv + g; cc < ld_out; cc += 4) st(orow + cc, 0.f);
}

// Launches `groups` groups of src at the smallest DMAX of 32, 64, 128 that holds both head sizes.  The caller has
// checked the head sizes (multiples of 16 up to 128), attention_vec8 and the 32-bit ranges.
template <typename Src, bool CAUSAL>
hipError_t attention_bf16_launch(const Src& src, bf16* out, int ld_out, int groups, hipStream_t s) {
  const int qtiles = (src.nq() + B16_QT - 1) / B16_QT;
  if ((long long)groups * src.heads * qtiles > 0x7fffffffll) return hipErrorInvalidValue;
  const dim3 grid(groups * src.heads * qtiles), block(256);
  const int dm = src.d > src.dv() ? src.d : src.dv();
  if (dm <= 32)
    hipLaunchKernelGGL((attention_bf16_kernel<32, Src, CAUSAL>), grid, block, 0, s, src, out, ld_out, qtiles);
  else if (dm <= 64)
    hipLaunchKernelGGL((attention_bf16_kernel<64, Src, CAUSAL>), grid, block, 0, s, src, out, ld_out, qtiles);
  else
    hipLaunchKernelGGL((attention_bf16_kernel<128, Src, CAUSAL>), grid, block, 0, s, src, out, ld_out, qtiles);
  return hipGetLastError();
}

}  // namespace attn
}  // namespace adapt
