// Wide heads of the attention core: softmax(Q K^T) V per (group, head) for head sizes d and dv that are multiples of
// 16 up to 512 with max(d, dv) > 128, fp32 and bf16 activations, gfx950.  attention_core.h describes the scheme this
// kernel shares (the swapped score product on v_mfma_f32_16x16x4_f32, the permuted k-step orders, the online
// softmax, the tails, the causal mask, the source policy `Src`); this header describes only what differs, the split
// of the work.
//
// Why another split.  The core keeps the Q and O of a wave's 16 queries in registers: at a head of 512 that is 256
// VGPRs before the prefetch, and a 32-key fp32 K / V tile is 132 KB of LDS, so one wave per SIMD at best.  Here the
// head is split over the waves of a block instead of the queries:
//
//   * A block of 4 waves owns one (group, head, tile of WQ = 16 R queries) and all four waves hold the *same*
//     queries.  The head is cut into 16-wide slices; wave w owns the slices t = w (mod 4) of d for the score product
//     and the slices n = w (mod 4) of dv for the output (d = dv = 160: 3, 3, 2, 2 slices; dv = 16 leaves three waves
//     without an output slice).  Per lane at DW = 512, R = 2 that is 64 VGPRs of Q fragments and 64 of O
//     accumulators, a quarter of the unsplit wave's, which is what lets two blocks share a CU.
//   * K and V of a tile of WK keys are staged once per block through padded LDS rows and fetched into registers one
//     tile ahead with predicated loads (rows at or beyond the key bound are zeros), as in the core.  A thread stages
//     one 4-element column of the head in every pass over the rows (256 threads = 256 / (DW / 4) rows per pass), so
//     its staging state is two columns and a row, not a table.
//   * Each wave computes the partial S^T = K Q^T over its slices of d and writes it (R WK / 16 f32x4 per lane) to an
//     LDS exchange area [4 waves][R WK / 16][64 lanes].  After one barrier every wave reads all four partials and
//     adds them in wave order 0, 1, 2, 3; a wave without a slice of d wrote zeros.  The fixed order is a correctness
//     condition: the four waves then hold bit-identical scores, so their replicated softmax state (m, l, alpha, p)
//     agrees and the O slices each of them owns belong to one softmax.
//   * Each wave runs the online softmax of the core on the full scores and then O^T += V^T P^T for its slices of dv
//     only, P from registers.  P never goes through LDS, only the partial scores do.
//   * Two barriers per key tile, and the two halves of the prefetch are never in registers together.  Barrier A: V
//     of the previous tile has been read, K of this tile (stored after the previous barrier B) is visible.  Then V
//     of this tile goes from registers to LDS, the loads of the next tile's K are issued, and the partial scores are
//     computed and written.  Barrier B: the partials and V are visible, and every wave has read this tile's K.  Then
//     the next tile's K goes from registers to LDS, the softmax runs, the loads of the next tile's V are issued and
//     P V runs under them.  The plain form (both halves fetched after one barrier, three barriers) holds 64 prefetch
//     VGPRs at DW = 512 next to 128 of Q and O; this form holds 32 at a time.  At the 256 VGPRs that two waves per
//     SIMD leave, DW = 512 compiles to 250 - 252 without scratch; with V's loads issued before the softmax the bf16
//     instantiation spilled two registers.  LDS rows have the compile-time length DW + 4 whatever d and dv are, so
//     every LDS offset is an immediate (with rows of d + 4 the per-pass addresses were loop-carried registers and
//     12 of them spilled).  The exchange area needs no barrier of its own: a
//     wave writes the partials of tile t + 1 after barrier A of t + 1, which every wave reaches after it has read
//     the partials of tile t.  The waves share their queries, so the key bound, the causal bound and the trip count
//     are block-uniform by construction and no branch that depends on `wave` stands in front of a barrier.
//
// Tiles.  WK = 16 and R = 2 at both DW.  LDS per block is 2 WK (DW + 4) floats of tiles plus 4 R (WK / 16) KB of
// exchange area: 74,240 bytes at DW = 512 (two blocks in a CU's 160 KB) and 41,472 at DW = 256.  WK = 32 at DW = 256
// has the same 66,048 bytes of tiles as WK = 16 at 512, but its exchange area is 16 KB at R = 2: 82,432 bytes, 512
// more than half a CU's LDS, so it would run one block per CU.
//
// Causal: kend = min(Tk, last query of the tile + 1); tiles above the diagonal are neither loaded nor computed; in
// the straddling tiles a future key's score becomes -inf in the statement that masks the keys beyond the count;
// where the running and the tile maximum are both -inf the exponents are taken against 0.
//
// Queries beyond the count are carried and not stored.  A wave stores its own slices of dv; wave 0 writes the row's
// layout padding as zeros for the last head.  Index math is 32-bit behind the front-end's refusals.
#pragma once
#include "attention_core.h"

namespace adapt {
namespace attn {

constexpr int WIDE_MAX = 512;   // the largest head size
constexpr int WIDE_R = 2;       // 16-query sets per block
constexpr int WIDE_WK = 16;     // keys per LDS tile
constexpr int WIDE_WQ = 16 * WIDE_R;

// 0: not a wide head, else the DW of the instantiation that serves it
inline int wide_dw(int d, int dv) {
  const int dm = d > dv ? d : dv;
  if (d < 16 || dv < 16 || d % 16 || dv % 16 || dm <= 128 || dm > WIDE_MAX) return 0;
  return dm <= 256 ? 256 : 512;
}

// DW: the compile-time bound on max(d, dv), 256 or 512.  CAUSAL: query i attends keys j <= i (nq() == nk())
template <typename T, int DW, typename Src, bool CAUSAL = false>
__global__ __launch_bounds__(256, 2) void attention_wide_kernel(Src src, T* __restrict__ out, int ld_out, int qtiles) {
  constexpr int R = WIDE_R, WK = WIDE_WK, WQ = WIDE_WQ;
  constexpr int NS = DW / 64;                         // 16-wide slices per wave: slice wave + 4 j
  constexpr int U = WK / 16;                          // 16-key sets per tile
  constexpr int CV = DW / 4;                          // 4-element columns of a staged row
  constexpr int RP = 256 / CV;                        // rows staged per pass of the block
  constexpr int NP = WK / RP;                         // passes per tile
  constexpr int TILE = WK * (DW + ATTN_PAD);
  static_assert(DW == 256 || DW == 512, "two instantiations");
  static_assert(WK % RP == 0 && WK % 16 == 0, "whole passes, whole key sets");
  static_assert((2 * TILE + 4 * R * U * 256) * 4 <= 81920, "two blocks per CU");
  __shared__ __attribute__((aligned(16))) float smem[2 * TILE + 4 * R * U * 256];
  float* sk = smem;
  float* sv = smem + TILE;
  f32x4* ex = (f32x4*)(smem + 2 * TILE);              // [4 waves][R * U][64 lanes]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int heads = src.heads, d = src.d, dv = src.dv(), Tq = src.nq(), Tk = src.nk();
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
  const int q0 = qt_ * WQ;
  const int h = bid % heads;
  const typename Src::Block b = src.block(bid / heads, h);
  constexpr int ldk = DW + ATTN_PAD, ldv = ldk;       // LDS row lengths: compile-time, so every LDS offset is an immediate

  // what this thread stages of every key tile: column `cv` of rows r0, r0 + RP, ... of K and of V
  const int cv = tid % CV, r0 = tid / CV;
  const bool kval = 4 * cv < d, vval = 4 * cv < dv;
  const int kcol = src.stage_col(b, false, 4 * cv), vcol = src.stage_col(b, true, 4 * cv);

  // block-uniform: the same queries, and so the same key bound, in all four waves
  int kend = Tk;
  if constexpr (CAUSAL) kend = min(Tk, q0 + WQ);
  int qtok[R];
  bool qok[R];
  f32x4 qf[R][NS], o[R][NS];
  float m[R], l[R];                                   // l: this lane's keys only, summed over the groups at the end
#pragma unroll
  for (int r = 0; r < R; ++r) {
    qtok[r] = q0 + 16 * r + c;
    qok[r] = qtok[r] < Tq;
    m[r] = -INFINITY;
    l[r] = 0.f;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      const int t = wave + 4 * j;
      qf[r][j] = o[r][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (qok[r] && 16 * t < d) qf[r][j] = ld4(src.q(b, qtok[r]) + 16 * t + 4 * g);
    }
  }

  // K of tile 0 goes straight to LDS, V of tile 0 waits in registers for the first barrier
  f32x4 pk[NP], pv[NP];
#pragma unroll
  for (int p = 0; p < NP; ++p) {
    const int row = p * RP + r0;
    pk[p] = pv[p] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (kval && row < kend) pk[p] = src.stage(b, false, row, kcol);
    if (vval && row < kend) pv[p] = src.stage(b, true, row, vcol);
  }
#pragma unroll
  for (int p = 0; p < NP; ++p)
    if (kval) *(f32x4*)(sk + (p * RP + r0) * ldk + 4 * cv) = pk[p];
  for (int k0 = 0; k0 < kend; k0 += WK) {             // the same trip count for every wave of the block
    const bool more = k0 + WK < kend;                 // block-uniform; causal: no tile the block will not use is loaded
    __syncthreads();                                  // V of the previous tile has been read; K of this one is visible
#pragma unroll
    for (int p = 0; p < NP; ++p)
      if (vval) *(f32x4*)(sv + (p * RP + r0) * ldv + 4 * cv) = pv[p];
    if (more) {                                       // K of the next tile: in flight under the score product
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const int row = k0 + WK + p * RP + r0;
        pk[p] = f32x4{0.f, 0.f, 0.f, 0.f};            // rows beyond the key bound are zeros, never loaded
        if (kval && row < kend) pk[p] = src.stage(b, false, row, kcol);
      }
    }
    // this wave's part of S^T = K Q^T: s[r][u][i] = score(key k0 + 16 u + 4 g + i, query q0 + 16 r + c) over its
    // slices of d; zeros where it has none
    f32x4 s[R][U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
      for (int r = 0; r < R; ++r) s[r][u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < NS; ++j) {
        const int t = wave + 4 * j;
        if (16 * t < d) {
          const f32x4 kf = *(const f32x4*)(sk + (16 * u + c) * ldk + 16 * t + 4 * g);
#pragma unroll
          for (int r = 0; r < R; ++r) {
            s[r][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.x, qf[r][j].x, s[r][u], 0, 0, 0);
            s[r][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.y, qf[r][j].y, s[r][u], 0, 0, 0);
            s[r][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.z, qf[r][j].z, s[r][u], 0, 0, 0);
            s[r][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.w, qf[r][j].w, s[r][u], 0, 0, 0);
          }
        }
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int u = 0; u < U; ++u) ex[(wave * R * U + r * U + u) * 64 + lane] = s[r][u];
    __syncthreads();                                  // the partials and V are visible; K of this tile has been read
    if (more) {
#pragma unroll
      for (int p = 0; p < NP; ++p)
        if (kval) *(f32x4*)(sk + (p * RP + r0) * ldk + 4 * cv) = pk[p];
    }
    // the whole scores, summed in wave order in every wave: bit-identical in all four
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const f32x4* e = ex + (r * U + u) * 64 + lane;
        s[r][u] = ((e[0] + e[R * U * 64]) + e[2 * R * U * 64]) + e[3 * R * U * 64];
      }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float mx = -INFINITY;
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int key = k0 + 16 * u + 4 * g + i;
          bool masked = key >= Tk;
          if constexpr (CAUSAL) masked = masked || key > qtok[r];               // before the maximum is taken
          if (masked) s[r][u][i] = -INFINITY;
          mx = fmaxf(mx, s[r][u][i]);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 16));
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float mn = fmaxf(m[r], mx);
      float me = mn;                                  // what the exponents are taken against
      if constexpr (CAUSAL) {
        if (mn == -INFINITY) me = 0.f;                // never exp(-inf - -inf): the core's guard
      }
      const float alpha = expf(m[r] - me);            // 0 on the first tile (m = -inf)
      m[r] = mn;
      float ps = 0.f;
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          s[r][u][i] = expf(s[r][u][i] - me);         // masked keys: exp(-inf) = 0
          ps += s[r][u][i];
        }
      l[r] = l[r] * alpha + ps;
#pragma unroll
      for (int j = 0; j < NS; ++j) o[r][j] *= alpha;
    }
    if (more) {                                       // V of the next tile: in flight under P V
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const int row = k0 + WK + p * RP + r0;
        pv[p] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (vval && row < kend) pv[p] = src.stage(b, true, row, vcol);
      }
    }
    // O^T += V^T P^T over this wave's slices of dv: o[r][j][i] = O(query q0 + 16 r + c, channel 16 (wave + 4 j) + 4 g + i)
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int j = 0; j < NS; ++j) {
        const int n = wave + 4 * j;
        if (16 * n < dv) {
          const float* vp = sv + (16 * u + 4 * g) * ldv + 16 * n + c;
          const float v0 = vp[0], v1 = vp[ldv], v2 = vp[2 * ldv], v3 = vp[3 * ldv];
#pragma unroll
          for (int r = 0; r < R; ++r) {
            o[r][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(v0, s[r][u].x, o[r][j], 0, 0, 0);
            o[r][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(v1, s[r][u].y, o[r][j], 0, 0, 0);
            o[r][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(v2, s[r][u].z, o[r][j], 0, 0, 0);
            o[r][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(v3, s[r][u].w, o[r][j], 0, 0, 0);
          }
        }
      }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {                       // no barrier follows
    float ls = l[r];
    ls += __shfl_xor(ls, 16);
    ls += __shfl_xor(ls, 32);
    if (!qok[r]) continue;
    const float inv = 1.f / ls;
    T* orow = out + src.out_row(b, qtok[r]) * ld_out;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      const int n = wave + 4 * j;
      if (16 * n < dv) st4(orow + h * dv + 16 * n + 4 * g, o[r][j] * inv);
    }
    if (h == heads - 1 && wave == 0)                  // layout padding of the row: zeros
      for (int cc = heads * dv + g; cc < ld_out; cc += 4) st(orow + cc, 0.f);
  }
}

// Launches `groups` groups of src on the wide kernel; the caller has checked wide_dw(d, dv) != 0, the 4-element
// alignment (attention_vec4) and the 32-bit ranges.
template <typename T, typename Src, bool CAUSAL = false>
hipError_t attention_wide_launch(const Src& src, T* out, int ld_out, int groups, hipStream_t s) {
  const int qtiles = (src.nq() + WIDE_WQ - 1) / WIDE_WQ;
  if ((long long)groups * src.heads * qtiles > 0x7fffffffll) return hipErrorInvalidValue;
  const dim3 grid(groups * src.heads * qtiles), block(256);
  if (wide_dw(src.d, src.dv()) == 256)
    hipLaunchKernelGGL((attention_wide_kernel<T, 256, Src, CAUSAL>), grid, block, 0, s, src, out, ld_out, qtiles);
  else
    hipLaunchKernelGGL((attention_wide_kernel<T, 512, Src, CAUSAL>), grid, block, 0, s, src, out, ld_out, qtiles);
  return hipGetLastError();
}

}  // namespace attn
}  // namespace adapt
