// Skinny GEMM on MXFP4 weights for the one-token decode step: 1 <= M <= 32 bf16 rows through a 1x1 conv whose
// weights are OCP Microscaling e2m1 codes with one e8m0 scale per 32 consecutive k of a channel,
//
//   out[m][n] = act( sum_k x[m][k] * deq(W)[n][k] + bias[n] (+ res[m][n]) ),   bf16 -> bf16, fp32 sums.
//
// The bf16 skinny kernel (gemm_skinny.h) is bound by the 2 bytes per weight it streams; this one streams 4.25 bits.
// deq(W) = code x 2^(e - 127) has two significant bits, so it is a bf16 number: the kernel converts the codes to the
// exact bf16 operand of the bf16 matrix instruction and everything after the conversion is gemm_skinny.h's.
//
// * Layout (ops/mx.py pack_mxfp4).  Codes: [Npad][Kpad / 128][q = 4][s = 4] 32-bit words; word (q, s) of row n and
//   128-chunk c holds k = 128 c + 32 s + 8 q .. + 7, two codes a byte, the lower nibble the lower k.  Scales:
//   [Npad][Kpad / 128] dwords, byte s the e8m0 of block 4 c + s.  Padding (k >= K, n >= N) is zero codes, scale 127.
// * Operands.  Lane (r = lane % 16, q = lane / 16) takes its share of weight row n0 + r for a whole chunk as ONE
//   16-byte non-temporal load and one scale dword (a row's four q lanes load the same one).  Element s of the
//   vector, through four v_cvt_scalef32_pk_bf16_fp4 (byte b -> k pair 2 b, 2 b + 1; the scale operand is the fp32
//   bit pattern e << 23, so the product is formed in the conversion, not on the accumulator), is the A operand of
//   step s of four v_mfma_f32_16x16x32_bf16.  B of step s is lane (m, q)'s 16 bytes x[m][128 c + 32 s + 8 q ..].
//   Rows 17 .. 32 are a second row fragment (MF = 2) on the same converted registers.
// * Work split.  grid (ceil(N / 16 F), KS), 256 threads, F in 1 / 2 / 4 / 8.  A block owns 16 F channels, all rows
//   and the chunks [ks NCH / KS, (ks + 1) NCH / KS) of K, a chunk being 128 k: 64 bytes of codes a row, but 256
//   bytes of x a row, which is what fills the registers now (a set is 5 F + 16 MF VGPRs; a 256-k chunk at F = 8,
//   MF = 2 would need two sets of 144 next to 64 accumulators).  The four waves take the chunks interleaved, and a
//   wave issues every load of its next chunk before the conversions and MFMAs of the current one, on two sets.
//   x comes from global memory (L2) and is re-read by every channel tile: with 4-bit weights it is the larger
//   stream, which is why the tiles go up to F = 8 here.  Measured (BASELINE.md "Round 25"): F = 4 wins where N is
//   large enough to keep two blocks per CU (llama2_7b qkv, gate / up), F = 1 / 2 elsewhere, F = 8 nowhere yet.
// * Masks.  x vectors: row < M and k < K.  Codes and scales: the fragment's first channel < N (rows up to the
//   channel tile's end exist: the host checks Npad); chunks end at Kpad, so no k mask.  Stores: n < N and row < M.
// * Merge and epilogue: sk_finish of gemm_skinny.h, unchanged.
#pragma once
#include "gemm_skinny.h"

namespace adapt {

struct SkinnyMxParams {
  const bf16* x;            // [M][K]
  const uint32_t* codes;    // [Npad][Kpad / 128][4][4]
  const uint32_t* scales;   // [Npad][Kpad / 128]
  const float* bias;        // [N]
  const bf16* res;          // [M][N] or nullptr
  bf16* out;                // [M][N]
  float* ws;                // KS > 1: [KS][M][N]
  int* counters;            // KS > 1: one per channel tile, zero before and after
  int M, N, K, Kpad, act;
};

constexpr int MX_KC = 128;                // k per chunk

// one wave's operands of one chunk: F code vectors, F scale dwords and 4 MF activation vectors a lane
template <int F, int MF>
struct SkinnyMxSet {
  u32x4 w[F];
  uint32_t sc[F];
  bf16x8 x[MF][4];
};

// eight e2m1 codes of one word times 2^(e - 127): the exact bf16 A operand of one MFMA step
__device__ __forceinline__ bf16x8 mx_cvt(uint32_t word, uint32_t e) {
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  const float scale = __uint_as_float(e << 23);
  const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, scale, 0);
  const bf16x2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, scale, 1);
  const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, scale, 2);
  const bf16x2 d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, scale, 3);
  return (bf16x8){a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}

template <int F, int MF>
__global__ __launch_bounds__(256, (F * MF >= 8) ? 1 : 2) void gemm_skinny_mx_kernel(SkinnyMxParams p) {
  using Set = SkinnyMxSet<F, MF>;
  using IT = SkinnyItems<F, MF>;
  __shared__ f32x4 red[4][IT::NI];
  __shared__ int flag;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int nb0 = blockIdx.x * 16 * F;
  const int KS = gridDim.y, ks = blockIdx.y;
  const int nch = p.Kpad / MX_KC;
  const int c0 = (int)((long long)ks * nch / KS), c1 = (int)((long long)(ks + 1) * nch / KS);

  // row n0 + r of fragment f: its chunk c is 16 words at (row nch + c) 16, this lane's vector at + 4 q
  const size_t row0 = (size_t)(nb0 + r) * nch, fstep = (size_t)16 * nch;
  const uint32_t* wrow = p.codes + row0 * 16 + 4 * q;
  const uint32_t* srow = p.scales + row0;
  bool fok[F];
#pragma unroll
  for (int f = 0; f < F; ++f) fok[f] = nb0 + 16 * f < p.N;                  // a fragment past N is not read
  const bf16* xrow[MF];
  bool rok[MF];
#pragma unroll
  for (int mf = 0; mf < MF; ++mf) {
    rok[mf] = 16 * mf + r < p.M;
    xrow[mf] = p.x + (size_t)(rok[mf] ? 16 * mf + r : 0) * p.K + 8 * q;
  }
  auto load = [&](Set& s, int c) {
#pragma unroll
    for (int f = 0; f < F; ++f) {
      s.w[f] = fok[f] ? __builtin_nontemporal_load((const u32x4*)(wrow + (f * fstep + c) * 16)) : sk_zero<u32x4>();
      s.sc[f] = fok[f] ? __builtin_nontemporal_load(srow + f * fstep + c) : 0u;
    }
#pragma unroll
    for (int ls = 0; ls < 4; ++ls) {
      const int k = c * MX_KC + 32 * ls;                                    // this lane's vector starts at k + 8 q
      const bool xk = k + 8 * q < p.K;
#pragma unroll
      for (int mf = 0; mf < MF; ++mf)
        s.x[mf][ls] = (xk && rok[mf]) ? *(const bf16x8*)(xrow[mf] + k) : sk_zero<bf16x8>();
    }
  };
  f32x4 acc[F][MF];
#pragma unroll
  for (int f = 0; f < F; ++f)
#pragma unroll
    for (int mf = 0; mf < MF; ++mf) acc[f][mf] = (f32x4){0.f, 0.f, 0.f, 0.f};
  auto mma = [&](const Set& s) {
#pragma unroll
    for (int f = 0; f < F; ++f) {
      if (!fok[f]) continue;
#pragma unroll
      for (int ls = 0; ls < 4; ++ls) {
        const bf16x8 w = mx_cvt(s.w[f][ls], (s.sc[f] >> (8 * ls)) & 0xffu);
#pragma unroll
        for (int mf = 0; mf < MF; ++mf)
          acc[f][mf] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w, s.x[mf][ls], acc[f][mf], 0, 0, 0);
      }
    }
  };
  // this wave's chunks c0 + wave, + 4, ...: the next chunk's loads are in flight under the current chunk's work
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
  sk_finish<bf16, F, MF>(acc, red, flag, p, nb0, wave, lane);
}

}  // namespace adapt
