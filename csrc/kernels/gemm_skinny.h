// Skinny GEMM for the one-token decode step: 1 <= M <= 32 rows through a 1x1 conv's packed weights,
//
//   out[m][n] = act( sum_k x[m][k] * W[n][k] + bias[n] (+ res[m][n]) ),   fp32 -> fp32 and bf16 -> bf16 (fp32 sums).
//
// The tile kernels run such a launch with 8 of 64 .. 256 tile rows filled and are bound by everything but the
// weights; this kernel streams W once, is bound by W's bytes, and keeps the M rows as the 16-wide free dimension
// of the matrix instruction.  W is pack_conv / pack_conv_f32's [Npad][Kpad] (k contiguous, zero-padded), read in
// place: no second copy of the weights.
//
// * Operands.  W is the A operand.  Lane (r = lane % 16, q = lane / 16) loads one 16-byte vector
//   W[n0 + r][k + VEC q ..] and lane (m, q) the same k of x[m][..].  fp32 (VEC 4): element s of both vectors feeds
//   step s of four v_mfma_f32_16x16x4_f32, so the instruction's k index q stands for k + 4 q + s in both operands
//   (head.hip's dense_partial_f32_kernel reads this way).  bf16 (VEC 8): one vector each is one
//   v_mfma_f32_16x16x32_bf16.  The accumulator lane (m, g) then holds channels n0 + 4 g .. + 3 of row m: 16-byte
//   (fp32) or 8-byte (bf16) stores.  Rows 17 .. 32 are a second row fragment (MF = 2) on the same W registers.
// * Work split.  grid (ceil(N / 16 F), KS), 256 threads.  A block owns 16 F channels, all rows and the chunks
//   [ks NCH / KS, (ks + 1) NCH / KS) of K, a chunk being 256 bytes of a weight row (KC = 64 fp32 / 128 bf16 k).  Its
//   four waves take the chunks interleaved, so the block walks a row in 1 KiB strides; a wave issues every load of
//   its next chunk (4 F weight and 4 MF activation vectors a lane) before the MFMAs of the current one, on two
//   register sets.  x comes from global memory (L2, at most 360 KB, reused over F fragments); W never sees LDS and
//   is loaded non-temporally.
// * Masks.  x vectors: row < M and k < K; W vectors: k < Kpad and the fragment's first channel < N (rows up to the
//   fragment boundary exist: the host checks Npad); stores: n < N and row < M.  K and N are multiples of VEC.
// * Merge.  The four waves' accumulators meet in LDS and are added in wave order.  KS == 1: epilogue.  KS > 1: the
//   block's sum goes to ws[ks][m][n] (fp32), and the arrival protocol of gemm_f32s.hip's fused fixup follows
//   unchanged: SC1 stores and loads of the partials, s_waitcnt vmcnt(0), barrier, one relaxed agent-scope fetch_add
//   on the channel tile's counter; the last arriver stores 0 back, adds the KS partials in split order (its own
//   from registers at its own index: bit-identical whoever is last) and runs the epilogue.  No spin, one launch.
// * Epilogue.  + bias (fp32), + residual (output type and shape), ReLU / ReLU6 (common.h act_relu), one rounding
//   to bf16 in the bf16 build.
#pragma once
#include "common.h"

namespace adapt {

template <typename T>
struct SkinnyParams {
  const T* x;          // [M][K]
  const T* w;          // [Npad][Kpad]
  const float* bias;   // [N]
  const T* res;        // [M][N] or nullptr
  T* out;              // [M][N]
  float* ws;           // KS > 1: [KS][M][N]
  int* counters;       // KS > 1: one per channel tile, zero before and after
  int M, N, K, Kpad, act;
};

constexpr int SK_CPOL_SC1 = 16;
constexpr int SK_LS = 4;               // 16-byte vectors a lane loads per weight row and chunk (4 q x 4 = 256 bytes)

template <typename T>
struct SkinnyType;
template <>
struct SkinnyType<float> {
  using Vec = f32x4;
  static constexpr int VEC = 4, KC = 64;
};
template <>
struct SkinnyType<bf16> {
  using Vec = bf16x8;
  static constexpr int VEC = 8, KC = 128;
};

// the builtin returns int: without the unsigned wrapper a low word with bit 31 set sign-extends over the high word
__device__ __forceinline__ unsigned sk_sgpr(unsigned v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ __amdgpu_buffer_rsrc_t sk_rsrc(const float* base) {
  const unsigned long long a = (unsigned long long)(uintptr_t)base;
  const unsigned long long u = ((unsigned long long)sk_sgpr((unsigned)(a >> 32)) << 32) | sk_sgpr((unsigned)a);
  return __builtin_amdgcn_make_buffer_rsrc((void*)(uintptr_t)u, (short)0, 0x7fffffff, 0x00020000);
}

template <typename Vec>
__device__ __forceinline__ Vec sk_zero() {
  return __builtin_bit_cast(Vec, (u32x4){0u, 0u, 0u, 0u});
}

// one wave's operands of one chunk: 4 F weight vectors and 4 MF activation vectors a lane
template <typename T, int F, int MF>
struct SkinnySet {
  typename SkinnyType<T>::Vec w[F][SK_LS], x[MF][SK_LS];
};

__device__ __forceinline__ f32x4 sk_mma(f32x4 w, f32x4 x, f32x4 acc) {
#pragma unroll
  for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w[s], x[s], acc, 0, 0, 0);
  return acc;
}
__device__ __forceinline__ f32x4 sk_mma(bf16x8 w, bf16x8 x, f32x4 acc) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, x, acc, 0, 0, 0);
}

__device__ __forceinline__ f32x4 sk_widen(const float* p) { return *(const f32x4*)p; }
__device__ __forceinline__ f32x4 sk_widen(const bf16* p) {
  const uint2 u = *(const uint2*)p;                       // 4 bf16: the high halves of 4 floats
  return (f32x4){__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                 __uint_as_float(u.y & 0xffff0000u)};
}
__device__ __forceinline__ void sk_store(float* p, f32x4 v) { *(f32x4*)p = v; }
__device__ __forceinline__ void sk_store(bf16* p, f32x4 v) {
  typedef bf16 bf16x4 __attribute__((ext_vector_type(4)));
  *(bf16x4*)p = (bf16x4){f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
}

// F x MF x 64 accumulator vectors of a block, as items of 256 threads: item -> (fragment, row fragment, lane)
template <int F, int MF>
struct SkinnyItems {
  static constexpr int NI = F * MF * 64, PER = (NI + 255) / 256;
};

// The tail every skinny kernel shares (gemm_skinny_mx.h too): merge of the four waves' accumulators, the split-K
// arrival protocol and the epilogue, as the header describes them.  `red` and `flag` are the block's LDS.
// P: SkinnyParams<T> or SkinnyMxParams (bias, res, out, ws, counters, M, N, act).
template <typename T, int F, int MF, typename P>
__device__ __forceinline__ void sk_finish(const f32x4 (&acc)[F][MF], f32x4 (&red)[4][SkinnyItems<F, MF>::NI],
                                          int& flag, const P& p, int nb0, int wave, int lane) {
  using IT = SkinnyItems<F, MF>;
  const int KS = gridDim.y, ks = blockIdx.y;
  // the four waves' sums meet in LDS (a wave without a chunk brings zeros) and are added in wave order
#pragma unroll
  for (int f = 0; f < F; ++f)
#pragma unroll
    for (int mf = 0; mf < MF; ++mf) red[wave][(f * MF + mf) * 64 + lane] = acc[f][mf];
  __syncthreads();
  f32x4 own[IT::PER];
  int om[IT::PER], on[IT::PER];                                // item j: row and first channel; row -1 = nothing
#pragma unroll
  for (int j = 0; j < IT::PER; ++j) {
    const int idx = threadIdx.x + 256 * j;
    own[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    om[j] = -1;
    on[j] = 0;
    if (idx < IT::NI) {
      const int fm = idx >> 6, l = idx & 63;
      const int m = 16 * (fm % MF) + (l & 15), n = nb0 + 16 * (fm / MF) + 4 * (l >> 4);
      own[j] = ((red[0][idx] + red[1][idx]) + red[2][idx]) + red[3][idx];
      if (m < p.M && n < p.N) {
        om[j] = m;
        on[j] = n;
      }
    }
  }
  if (KS > 1) {
    const __amdgpu_buffer_rsrc_t wsr = sk_rsrc(p.ws);
    const int MN = p.M * p.N;
#pragma unroll
    for (int j = 0; j < IT::PER; ++j)
      if (om[j] >= 0)
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, own[j]), wsr,
                                               (ks * MN + om[j] * p.N + on[j]) * 4, 0, SK_CPOL_SC1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
      const int old = __hip_atomic_fetch_add(p.counters + blockIdx.x, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int last = old == KS - 1;
      if (last) __hip_atomic_store(p.counters + blockIdx.x, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      flag = last;
    }
    __syncthreads();
    if (!flag) return;
#pragma unroll
    for (int j = 0; j < IT::PER; ++j) {
      if (om[j] < 0) continue;
      f32x4 sum = (f32x4){0.f, 0.f, 0.f, 0.f};
      for (int s = 0; s < KS; ++s) {
        if (s == ks) sum += own[j];
        else
          sum += __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                               wsr, (s * MN + om[j] * p.N + on[j]) * 4, 0, SK_CPOL_SC1));
      }
      own[j] = sum;
    }
  }
#pragma unroll
  for (int j = 0; j < IT::PER; ++j) {
    if (om[j] < 0) continue;
    const size_t o = (size_t)om[j] * p.N + on[j];
    f32x4 v = own[j] + *(const f32x4*)(p.bias + on[j]);
    if (p.res) v += sk_widen(p.res + o);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = act_relu(v[e], p.act);
    sk_store(p.out + o, v);
  }
}

template <typename T, int F, int MF>
__global__ __launch_bounds__(256, (F * MF >= 8) ? 1 : 2) void gemm_skinny_kernel(SkinnyParams<T> p) {
  using ST = SkinnyType<T>;
  using Vec = typename ST::Vec;
  using Set = SkinnySet<T, F, MF>;
  using IT = SkinnyItems<F, MF>;
  constexpr int VEC = ST::VEC, KC = ST::KC;
  __shared__ f32x4 red[4][IT::NI];
  __shared__ int flag;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int nb0 = blockIdx.x * 16 * F;
  const int KS = gridDim.y, ks = blockIdx.y;
  const int nch = (p.Kpad + KC - 1) / KC;
  const int c0 = (int)((long long)ks * nch / KS), c1 = (int)((long long)(ks + 1) * nch / KS);

  const T* wrow[F];
  bool fok[F];
#pragma unroll
  for (int f = 0; f < F; ++f) {
    fok[f] = nb0 + 16 * f < p.N;                               // a fragment past N: zero rows, not read
    wrow[f] = p.w + (size_t)(nb0 + 16 * f + r) * p.Kpad + VEC * q;
  }
  const T* xrow[MF];
  bool rok[MF];
#pragma unroll
  for (int mf = 0; mf < MF; ++mf) {
    rok[mf] = 16 * mf + r < p.M;
    xrow[mf] = p.x + (size_t)(rok[mf] ? 16 * mf + r : 0) * p.K + VEC * q;
  }
  auto load = [&](Set& s, int c) {
#pragma unroll
    for (int ls = 0; ls < SK_LS; ++ls) {
      const int k = c * KC + ls * 4 * VEC;                     // this lane's vector starts at k + VEC q
      const bool wk = k + VEC * q < p.Kpad, xk = k + VEC * q < p.K;
#pragma unroll
      for (int f = 0; f < F; ++f)
        s.w[f][ls] = (wk && fok[f]) ? __builtin_bit_cast(Vec, __builtin_nontemporal_load((const u32x4*)(wrow[f] + k)))
                                    : sk_zero<Vec>();
#pragma unroll
      for (int mf = 0; mf < MF; ++mf) s.x[mf][ls] = (xk && rok[mf]) ? *(const Vec*)(xrow[mf] + k) : sk_zero<Vec>();
    }
  };
  f32x4 acc[F][MF];
#pragma unroll
  for (int f = 0; f < F; ++f)
#pragma unroll
    for (int mf = 0; mf < MF; ++mf) acc[f][mf] = (f32x4){0.f, 0.f, 0.f, 0.f};
  auto mma = [&](const Set& s) {
#pragma unroll
    for (int ls = 0; ls < SK_LS; ++ls)
#pragma unroll
      for (int f = 0; f < F; ++f)
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) acc[f][mf] = sk_mma(s.w[f][ls], s.x[mf][ls], acc[f][mf]);
  };
  // this wave's chunks c0 + wave, + 4, ...: the next chunk's loads are in flight under the current chunk's MFMAs
  Set a, b;
  int c = c0 + wave;
  if (c < c1) {
    load(a, c);
    while (true) {
      if (c + 4 < c1) load(b, c + 4);
      mma(a);
      c += 4;
      if (c >= c1) break;
      if (c + 4 < c1) load(a, c + 4);
      mma(b);
      c += 4;
      if (c >= c1) break;
    }
  }
  sk_finish<T, F, MF>(acc, red, flag, p, nb0, wave, lane);
}

}  // namespace adapt
