// Tile GEMM on MXFP4 weights for the prefill and every step above the skinny kernel's 32 rows: any M >= 1 bf16 rows
// through a 1x1 conv whose weights exist only as e2m1 codes and e8m0 scales (gemm_skinny_mx.h's layout, read as it
// is: no second packed form, no bf16 copy),
//
//   out[m][n] = act( sum_k x[m][k] * deq(W)[n][k] + bias[n] (+ res[m][n]) ),   bf16 -> bf16, fp32 sums.
//
// The skinny kernel holds every row in registers and reads x from global memory per channel tile: right at 32
// rows, hopeless at 1024.  Here the rows are tiled, x goes through LDS once per block and chunk, and a converted
// weight operand is used for MT matrix instructions, which is what pays for the conversions.
//
// * Operands: the swapped product, as in the skinny kernel.  W is the A operand of v_mfma_f32_16x16x32_bf16: lane
//   (r = lane % 16, q = lane / 16) loads the 16-byte code vector and the scale dword of row n0 + r for a whole 128-k
//   chunk, one chunk ahead, and `mx_cvt` (four v_cvt_scalef32_pk_bf16_fp4) of word s is A of k step s: the exact
//   bf16 value.  x is the B operand, so lane (m, g) of the accumulator holds channels n0 + 4 g .. + 3 of row m and
//   the epilogue (bias, residual, ReLU / ReLU6, one rounding) stores 8 bytes a lane.
// * Work split.  grid (row tiles x channel tiles, 1, KS), 256 threads.  A block owns BM = 16 MT rows and 64 F
//   channels; wave w owns the channel fragments w, w + 4, ... (F of them), all four waves share one x tile.  Per
//   k step a wave reads its MT B fragments from LDS once and uses them for F converted A operands: 4 MT
//   ds_read_b128 and 16 F conversions for 4 F MT MFMAs a chunk.  Instantiations (F, MT): (4, 8) 256 channels x
//   128 rows, 128 accumulator registers, 256 VGPRs and 64 KB of LDS: two blocks a CU, no scratch; (2, 4) and
//   (1, 4) at 64 rows for shapes that do not fill the chip with the wide tile.  Measured (BASELINE.md "Round 26"):
//   (4, 8) wins where it gives more than one block per CU, (1, 4) with split K below about 300 tiles, (2, 4)
//   between.
// * x through LDS.  The tile of a chunk is BM rows x 256 bytes, double-buffered (2 x 32 KB at BM = 128): thread
//   (row t / 16 + 16 j, granule t % 16) loads 16 bytes of MT rows of the NEXT chunk into registers under the
//   MFMAs of the current one, in two halves of MT / 2 rows, each stored two k steps after it was loaded (all MT
//   vectors at once spilled at (4, 8)); one barrier per chunk.  A row is 16 granules of 16 bytes
//   and spans all 64 banks, so the B-fragment read (16 lanes r, the same logical granule 4 s + q, 16 consecutive
//   rows) would hit one group of four banks 16 times.  Logical granule g of row m is therefore stored at physical
//   granule g ^ (m & 15): the 16 lanes of a q group read granules (4 s + q) ^ r, r = 0 .. 15, which are all
//   different, 256 distinct bytes, every bank once.  The store side is a permutation inside a row: 16 lanes still
//   write one whole row.  Measured: BASELINE.md "Round 26".
// * Masks.  x: rows >= M and k >= K are staged as zeros.  Codes and scales: read for a 16-channel fragment only when
//   its first channel < N (its rows exist: the host checks Npad against whole fragments); a chunk never passes
//   Kpad.  Stores: n < N and m < M.
// * Split-K over gridDim.z in whole chunks, merged by gemm_skinny.h's protocol: fp32 partials ws[ks][M][N] through
//   SC1 buffer stores, s_waitcnt vmcnt(0), barrier, one relaxed agent-scope fetch_add on the output tile's counter;
//   the last block to arrive stores 0 back, adds all KS partials in split order (its own read back like the others,
//   so the sum is bit-identical whoever is last and 128 accumulator registers need no second set) and runs the
//   epilogue.  The buffer resource is built per split on ws + ks M N with 64-bit arithmetic on unsigned halves
//   (sk_rsrc), so offsets stay below M N 4 < 2^31.
// * Block order.  blockIdx.x -> tile through xcd_remap, channel tile fastest: the tiles that share an x tile run
//   on one XCD next to each other and re-read it from that L2.
#pragma once
#include "gemm_skinny_mx.h"

namespace adapt {

// one wave's weight operands of one chunk: F code vectors and F scale dwords a lane
template <int F>
struct TileMxCodes {
  u32x4 w[F];
  uint32_t sc[F];
};

template <int F, int MT>
__global__ __launch_bounds__(256, 2) void gemm_tile_mx_kernel(SkinnyMxParams p) {
  constexpr int BM = 16 * MT, BN = 64 * F, ROWB = 2 * MX_KC, BUF = BM * ROWB;
  __shared__ __attribute__((aligned(16))) char xs[2 * BUF];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 15, q = lane >> 4;
  const int ntn = (p.N + BN - 1) / BN;
  const int tile = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = tile / ntn * BM, nb0 = tile % ntn * BN + 16 * wave;         // this wave's first fragment
  const int KS = gridDim.z, ks = blockIdx.z;
  const int nch = p.Kpad / MX_KC;
  const int c0 = (int)((long long)ks * nch / KS), c1 = (int)((long long)(ks + 1) * nch / KS);

  // weights: row nb0 + 64 f + r, its chunk c is 16 words at (row nch + c) 16, this lane's vector at + 4 q
  const size_t row0 = (size_t)(nb0 + r) * nch, fstep = (size_t)64 * nch;
  const uint32_t* wrow = p.codes + row0 * 16 + 4 * q;
  const uint32_t* srow = p.scales + row0;
  bool fok[F];
#pragma unroll
  for (int f = 0; f < F; ++f) fok[f] = nb0 + 64 * f < p.N;                    // a fragment past N is not read
  auto cload = [&](TileMxCodes<F>& s, int c) {
#pragma unroll
    for (int f = 0; f < F; ++f) {
      s.w[f] = fok[f] ? *(const u32x4*)(wrow + (f * fstep + c) * 16) : sk_zero<u32x4>();
      s.sc[f] = fok[f] ? srow[f * fstep + c] : 0u;
    }
  };

  // x staging: thread (rb = t / 16, g = t % 16) moves granule g of rows rb + 16 j; physical granule g ^ rb.  The
  // rows go in two halves of XH, each loaded two k steps before it is stored, so MT / 2 vectors are live, not MT
  constexpr int XH = MT / 2;
  const int g = threadIdx.x & 15, rb = threadIdx.x >> 4;
  const unsigned xg = ((unsigned)(m0 + rb) * p.K + 8 * g) * 2;                 // byte offsets: M K < 2^31 (host)
  char* xst = xs + rb * ROWB + 16 * (g ^ rb);
  auto xload = [&](u32x4 (&v)[XH], int c, int h) {
    const bool kok = c * MX_KC + 8 * g < p.K;
#pragma unroll
    for (int j = 0; j < XH; ++j)
      v[j] = (kok && m0 + rb + 16 * (h * XH + j) < p.M)
                 ? *(const u32x4*)((const char*)p.x + (xg + (unsigned)(16 * (h * XH + j) * p.K + c * MX_KC) * 2))
                 : sk_zero<u32x4>();
  };
  auto xstore = [&](const u32x4 (&v)[XH], int buf, int h) {
#pragma unroll
    for (int j = 0; j < XH; ++j) *(u32x4*)(xst + buf * BUF + (h * XH + j) * 16 * ROWB) = v[j];
  };

  // B fragments: lane (r, q) reads logical granule 4 s + q of rows 16 mt + r
  const char* xrd = xs + r * ROWB;
  int xo[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) xo[s] = 16 * ((4 * s + q) ^ r);
  f32x4 acc[F][MT];
#pragma unroll
  for (int f = 0; f < F; ++f)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[f][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  auto mma = [&](const TileMxCodes<F>& cs, int buf, int s) {                // k step s of the chunk in `buf`
    bf16x8 b[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) b[mt] = *(const bf16x8*)(xrd + buf * BUF + mt * 16 * ROWB + xo[s]);
#pragma unroll
    for (int f = 0; f < F; ++f) {
      if (!fok[f]) continue;
      const bf16x8 a = mx_cvt(cs.w[f][s], (cs.sc[f] >> (8 * s)) & 0xffu);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        acc[f][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[mt], acc[f][mt], 0, 0, 0);
    }
  };
  // chunk c from buffer `buf` and codes `cur`, with chunk c + 1 on its way: its codes into `next`, its x into
  // registers under the MFMAs and then into the other buffer, whose readers passed the last barrier
  u32x4 xr[XH];
  auto chunk = [&](const TileMxCodes<F>& cur, TileMxCodes<F>& next, int buf, int c) {
    const bool more = c + 1 < c1;
    if (more) {
      cload(next, c + 1);
      xload(xr, c + 1, 0);
    }
    mma(cur, buf, 0);
    mma(cur, buf, 1);
    if (more) {
      xstore(xr, buf ^ 1, 0);
      xload(xr, c + 1, 1);
    }
    mma(cur, buf, 2);
    mma(cur, buf, 3);
    if (more) xstore(xr, buf ^ 1, 1);
    __syncthreads();
    return more;
  };
  TileMxCodes<F> a, b;
  cload(a, c0);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    xload(xr, c0, h);
    xstore(xr, 0, h);
  }
  __syncthreads();
  for (int c = c0; chunk(a, b, 0, c) && chunk(b, a, 1, c + 1); c += 2) {
  }

  // lane (r, q) of fragment (f, mt): row m0 + 16 mt + r, channels nb0 + 64 f + 4 q .. + 3
  const int mrow = m0 + r, ncol = nb0 + 4 * q;
  const int MN = p.M * p.N;
  if (KS > 1) {
    int* flag = (int*)xs;                                  // the x tiles are done: every wave passed the last barrier
    const __amdgpu_buffer_rsrc_t own = sk_rsrc(p.ws + (size_t)ks * MN);
#pragma unroll
    for (int f = 0; f < F; ++f)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int m = mrow + 16 * mt, n = ncol + 64 * f;
        if (m < p.M && n < p.N)
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc[f][mt]), own, (m * p.N + n) * 4, 0,
                                                 SK_CPOL_SC1);
      }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
      const int old = __hip_atomic_fetch_add(p.counters + tile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int last = old == KS - 1;
      if (last) __hip_atomic_store(p.counters + tile, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      *flag = last;
    }
    __syncthreads();
    if (!*flag) return;
    // every split's partial, this block's own included (its stores are complete and went through the same path),
    // added in split order: the sum does not depend on which block came last
#pragma unroll
    for (int f = 0; f < F; ++f)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) acc[f][mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < KS; ++s) {
      const __amdgpu_buffer_rsrc_t part = sk_rsrc(p.ws + (size_t)s * MN);
#pragma unroll
      for (int f = 0; f < F; ++f)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const int m = mrow + 16 * mt, n = ncol + 64 * f;
          if (m < p.M && n < p.N)
            acc[f][mt] += __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(part, (m * p.N + n) * 4, 0,
                                                                                          SK_CPOL_SC1));
        }
    }
  }
#pragma unroll
  for (int f = 0; f < F; ++f)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const int m = mrow + 16 * mt, n = ncol + 64 * f;
      if (!(m < p.M && n < p.N)) continue;
      const size_t o = (size_t)m * p.N + n;
      f32x4 v = acc[f][mt] + *(const f32x4*)(p.bias + n);
      if (p.res) v += sk_widen(p.res + o);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = act_relu(v[e], p.act);
      sk_store(p.out + o, v);
    }
}

}  // namespace adapt
