// The attention core, softmax(Q K^T) V per (group, head), fp32 and bf16 activations, gfx950: the one place the
// scheme is described, and the two kernel templates that run it for a source policy.  attention.hip (one
// [Q | K | V] buffer) instantiates them and keeps only its layout, its argument checks and its entry points.
// cross_attention.hip (three row pointers, two token counts) and window_attention.hip (Swin windows of an NHWC
// map, a bias row per query) follow the same scheme in kernels of their own: on these templates, with key loops
// that compiled to the same instructions, they measured up to 0.9 % and 0.7 % slower (BASELINE.md "Round 16").
//
// A group is what one softmax runs inside: an image, or one window of an image.  The 1/sqrt(d) scale is already
// in Q (runtime/plan.py folds it into the projection).  out has heads x dv true channels per row; channels
// heads * dv .. ld_out - 1 are layout padding and are written as zeros.  Columns of the sources outside the heads
// are never read.
//
// MFMA kernel (d and dv multiples of 16 up to 128, any token counts >= 1): flash-style on v_mfma_f32_16x16x4_f32,
// all math in fp32 whatever the activation type (bf16 is widened while staged and the output is rounded once).
//
//   * A block of 4 waves owns one (group, head, tile of ATTN_QT = 64 queries); a wave owns 16 of the queries and
//     keeps their Q in registers for the whole kernel.  The block walks the keys ATTN_KT = 32 at a time: the K and
//     V rows of a key tile are staged once through LDS (rows padded by 4 floats: the 16-byte K reads of 16 lanes
//     and the V reads of the 4 lane groups then spread over the banks), fetched into registers one tile ahead so
//     that the loads of tile t + 1 are in flight under the MFMAs of tile t.
//   * The score product is taken swapped, S^T = K Q^T: M = key, N = query, so a lane of the 16x16 result holds
//     for query `lane & 15` the four keys `4 * (lane >> 4) + i`.  That register i is exactly the B operand of
//     the O^T = V^T P^T product when its k-step i is taken to mean the keys {4g + i} (V rows are read in that
//     permuted order), so P never goes through LDS, and O^T has the query on `lane & 15` as well: the row
//     maximum, the row sum and the rescale factor of the online softmax all live in the lane that needs them.
//     A row reduction is the in-lane registers plus two `__shfl_xor` steps (16, 32) over the four lane groups.
//     The k-step order inside a 16-wide slice of d is likewise permuted (step (t, j) means
//     dd = 16 t + 4 (lane >> 4) + j), so K and Q are read 16 bytes at a time.
//   * Online softmax: running maximum m and running sum l per query; per key tile alpha = exp(m - m'),
//     p = exp(s - m') with the exact expf, O and l rescaled by alpha.  The scores never touch memory.
//
// Tails.  K / V rows at or beyond the key count are staged as zeros by predicated loads and their scores are set
// to -inf (a zero probability alone is not enough: 0 x NaN from a poisoned row is NaN); a tile never reads a row
// beyond the count, and the policy's bases use the query count for Q / out and the key count for K / V, so a tile
// cannot reach into a neighbouring group either.  Queries at or beyond the query count load zeros, are carried
// through the arithmetic and are not stored.  The key loop's trip count depends on the key count alone and both
// barriers of an iteration come before the `active` test, so a wave whose 16 queries are all beyond the count
// (three of the four at one query) still reaches every barrier: it only helps staging, and leaves after the loop.
//
// Causal mask (CAUSAL = true; self-attention only, so the token counts agree): query i attends keys j <= i, Keras'
// `_compute_causal_mask`.  The key tiles above the diagonal are skipped, not computed and discarded: a block's
// key loop, and with it the prefetch, ends at the last query of its 64-query tile (a block-uniform bound, so every
// wave still meets both barriers of every iteration); a wave whose 16 queries all lie before a tile's first key
// stages its share, passes the barriers and skips the tile's MFMAs, where `active` is tested; in the tiles that
// straddle the diagonal a key after the lane's query gets the score -inf in the statement that masks the keys
// beyond the count, so before the maximum is taken (masking the probabilities afterwards lets one large future
// score underflow every visible term).  exp(-inf - -inf) cannot arise: where the running and the tile maximum
// are both -inf the exponents are taken against 0.  The plain kernel's lane loops run over k <= q.
//
// One loop for every size.  A group of at most 64 tokens would fit in LDS whole; staging Swin's 49 tokens as one
// 64-key tile (no second pass) measured 2 - 11 % slower than the two-tile loop at d = 32 (BASELINE.md
// "Round 13"): half of the loads then sit in front of the first MFMA with nothing to hide under.
//
// Plain kernel (every other head size, a pointer that is not aligned to 4 elements, a stride that is not a
// multiple of 4): one wave per (group, head, query), lanes over the keys, two passes (maximum, then exp / sum /
// P V with the probabilities broadcast by `__shfl`), fp32, every access bounds-checked, no barrier.
//
// Index math is 32-bit; the front-ends refuse, per tensor, sizes whose element offsets would not fit.
//
// The source policy `Src` is a small struct passed by value that answers what differs between front-ends;
// everything resolves at compile time.  T is the activation type.
//
//   int heads, d;  int dv() const;          head count and head sizes
//   int nq() const;  int nk() const;        queries and keys per group (host and device)
//   struct Block;  Block block(grp, h);     what the policy keeps per (group, head): bases, columns
//   int stage_col(b, isv, c)                staging table hook: the column a staged K (isv = false) or V vector
//                                           is loaded at, c = 4 x its index in the head
//   f32x4 stage(b, isv, row, col)           that vector of key row `row`
//   const T* q(b, row), k(b, row), v(b, row)   the head's Q, K and V channels of a row
//   int out_row(b, row)                     the row of `out` that a query row's context goes to
#pragma once
#include "kernels.h"

namespace adapt {
namespace attn {

constexpr int ATTN_QT = 64;   // queries per block (4 waves x 16)
constexpr int ATTN_KT = 32;   // keys per LDS tile
constexpr int ATTN_PAD = 4;   // floats of padding per LDS row

__device__ __forceinline__ f32x4 ld4(const float* p) { return *(const f32x4*)p; }
__device__ __forceinline__ f32x4 ld4(const bf16* p) {
  union { uint2 u; bf16 e[4]; } t;
  t.u = *(const uint2*)p;
  return f32x4{bf2f(t.e[0]), bf2f(t.e[1]), bf2f(t.e[2]), bf2f(t.e[3])};
}
__device__ __forceinline__ void st4(float* p, f32x4 v) { *(f32x4*)p = v; }
__device__ __forceinline__ void st4(bf16* p, f32x4 v) {
  union { uint2 u; bf16 e[4]; } t;
  t.e[0] = f2bf(v.x); t.e[1] = f2bf(v.y); t.e[2] = f2bf(v.z); t.e[3] = f2bf(v.w);
  *(uint2*)p = t.u;
}
__device__ __forceinline__ float ld(const float* p) { return *p; }
__device__ __forceinline__ float ld(const bf16* p) { return bf2f(*p); }
__device__ __forceinline__ void st(float* p, float v) { *p = v; }
__device__ __forceinline__ void st(bf16* p, float v) { *p = f2bf(v); }

// DMAX: the head sizes this instantiation holds in registers (d, dv <= DMAX, both multiples of 16).  CAUSAL: query
// i attends keys j <= i (nq() == nk()); every line it adds is under `if constexpr`
template <typename T, int DMAX, typename Src, bool CAUSAL = false>
__global__ __launch_bounds__(256) void attention_mfma_kernel(Src src, T* __restrict__ out, int ld_out, int qtiles) {
  constexpr int ND = DMAX / 16;                       // 16-wide slices of d / dv
  constexpr int NST = ATTN_KT * DMAX / 512;           // staged 4-element vectors per thread (K and V together)
  __shared__ __attribute__((aligned(16))) float smem[2 * ATTN_KT * (DMAX + ATTN_PAD)];
  float* sk = smem;
  float* sv = smem + ATTN_KT * (DMAX + ATTN_PAD);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int heads = src.heads, d = src.d, dv = src.dv(), Tq = src.nq(), Tk = src.nk();
  int bid = blockIdx.x;
  int qt_;
  if constexpr (CAUSAL) {
    // a block's work grows with its query tile: the heaviest tiles are dispatched first and the light ones fill
    // the tail, and the tiles of one weight are consecutive blocks, so they spread over the XCDs alike (with the
    // tile fastest, XCD x of 8 got tiles {x, x + 8} of 16: 24 key-tile units on the last against 10 on the first)
    const int gh = gridDim.x / qtiles;
    qt_ = qtiles - 1 - bid / gh;
    bid %= gh;
  } else {
    qt_ = bid % qtiles;
    bid /= qtiles;
  }
  const int qt = qt_;
  const int h = bid % heads;
  const typename Src::Block b = src.block(bid / heads, h);
  const int ldk = d + ATTN_PAD, ldv = dv + ATTN_PAD;  // LDS row lengths

  // what this thread stages of every key tile: vector `idx` of the tile's K rows, then of its V rows
  const int nkv = d >> 2, nvv = dv >> 2;
  int srow[NST], sgcol[NST], sloff[NST];
  bool sval[NST], sisv[NST];
#pragma unroll
  for (int j = 0; j < NST; ++j) {
    int idx = tid + j * 256;
    sval[j] = idx < ATTN_KT * (nkv + nvv);
    sisv[j] = false;
    srow[j] = sgcol[j] = sloff[j] = 0;
    if (idx < ATTN_KT * nkv) {
      srow[j] = idx / nkv;
      const int v = idx - srow[j] * nkv;
      sgcol[j] = src.stage_col(b, false, 4 * v);
      sloff[j] = srow[j] * ldk + 4 * v;
    } else if (sval[j]) {
      idx -= ATTN_KT * nkv;
      sisv[j] = true;
      srow[j] = idx / nvv;
      const int v = idx - srow[j] * nvv;
      sgcol[j] = src.stage_col(b, true, 4 * v);
      sloff[j] = ATTN_KT * (DMAX + ATTN_PAD) + srow[j] * ldv + 4 * v;
    }
  }

  const int q0 = qt * ATTN_QT + wave * 16;
  const bool active = q0 < Tq;                        // wave-uniform
  const int qtok = q0 + c;
  const bool qok = qtok < Tq;
  const int qrow = qtok;
  f32x4 qf[ND];
#pragma unroll
  for (int t = 0; t < ND; ++t) {
    qf[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (qok && 16 * t < d) qf[t] = ld4(src.q(b, qrow) + 16 * t + 4 * g);
  }
  f32x4 o[ND];
#pragma unroll
  for (int n = 0; n < ND; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;                       // l: this lane's keys only, summed over the groups at the end

  // the keys this block walks: all of them, or under the causal mask those up to the last query of its tile.
  // Block-uniform (from qt, never from wave): every wave passes both barriers of every iteration
  int kend = Tk;
  if constexpr (CAUSAL) kend = min(Tk, (qt + 1) * ATTN_QT);
  f32x4 st_[NST];
#pragma unroll
  for (int j = 0; j < NST; ++j) {
    st_[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (sval[j] && srow[j] < kend) st_[j] = src.stage(b, sisv[j], srow[j], sgcol[j]);
  }
  for (int k0 = 0; k0 < kend; k0 += ATTN_KT) {        // the same trip count for every wave of the block
    __syncthreads();                                  // the previous tile has been read
#pragma unroll
    for (int j = 0; j < NST; ++j)
      if (sval[j]) *(f32x4*)(smem + sloff[j]) = st_[j];
    __syncthreads();
    if (k0 + ATTN_KT < kend) {                        // causal: no tile the block will not use is loaded
#pragma unroll
      for (int j = 0; j < NST; ++j) {
        st_[j] = f32x4{0.f, 0.f, 0.f, 0.f};           // rows beyond the key count are zeros, never loaded
        const int r = k0 + ATTN_KT + srow[j];
        if (sval[j] && r < kend) st_[j] = src.stage(b, sisv[j], r, sgcol[j]);
      }
    }
    if (!active) continue;                            // after both barriers: the wave only helps staging
    if constexpr (CAUSAL) {
      if (k0 > q0 + 15) continue;                     // every key of the tile lies after the wave's 16 queries
    }
    // S^T = K Q^T: s[u][i] = score(key k0 + 16 u + 4 g + i, query c)
    f32x4 s[ATTN_KT / 16];
#pragma unroll
    for (int u = 0; u < ATTN_KT / 16; ++u) {
      s[u] = f32x4{0.f, 0.f, 0.f, 0.f};             // here: in a loop of their own 3.5 - 5 % slower (Round 16)
#pragma unroll
      for (int t = 0; t < ND; ++t) {
        if (16 * t < d) {
          const f32x4 kf = *(const f32x4*)(sk + (16 * u + c) * ldk + 16 * t + 4 * g);
          s[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.x, qf[t].x, s[u], 0, 0, 0);
          s[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.y, qf[t].y, s[u], 0, 0, 0);
          s[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.z, qf[t].z, s[u], 0, 0, 0);
          s[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.w, qf[t].w, s[u], 0, 0, 0);
        }
      }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int u = 0; u < ATTN_KT / 16; ++u)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        bool masked = k0 + 16 * u + 4 * g + i >= Tk;
        if constexpr (CAUSAL) masked = masked || k0 + 16 * u + 4 * g + i > qtok;    // before the maximum is taken
        if (masked) s[u][i] = -INFINITY;
        mx = fmaxf(mx, s[u][i]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));               // finite: key k0 is in every tile
    const float mn = fmaxf(m, mx);
    float me = mn;                                    // what the exponents are taken against
    if constexpr (CAUSAL) {
      // a query that has seen no key yet and sees none in this tile (none with today's tiles: a processed tile
      // holds key q0 <= qtok): exp(-inf - 0) = 0 for alpha and every p, never exp(-inf - -inf)
      if (mn == -INFINITY) me = 0.f;
    }
    const float alpha = expf(m - me);                 // 0 on the first tile (m = -inf)
    m = mn;
    float ps = 0.f;
#pragma unroll
    for (int u = 0; u < ATTN_KT / 16; ++u)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        s[u][i] = expf(s[u][i] - me);                 // masked keys: exp(-inf) = 0
        ps += s[u][i];
      }
    l = l * alpha + ps;
#pragma unroll
    for (int n = 0; n < ND; ++n) o[n] *= alpha;
    // O^T += V^T P^T: o[n][j] = O(query c, channel 16 n + 4 g + j)
#pragma unroll
    for (int u = 0; u < ATTN_KT / 16; ++u)
#pragma unroll
      for (int n = 0; n < ND; ++n) {
        if (16 * n < dv) {
          const float* vp = sv + (16 * u + 4 * g) * ldv + 16 * n + c;
          o[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[0], s[u].x, o[n], 0, 0, 0);
          o[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[ldv], s[u].y, o[n], 0, 0, 0);
          o[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[2 * ldv], s[u].z, o[n], 0, 0, 0);
          o[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[3 * ldv], s[u].w, o[n], 0, 0, 0);
        }
      }
  }
  if (!active) return;                                // no barrier follows
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (!qok) return;
  const float inv = 1.f / l;
  T* orow = out + src.out_row(b, qrow) * ld_out;
#pragma unroll
  for (int n = 0; n < ND; ++n)
    if (16 * n < dv) st4(orow + h * dv + 16 * n + 4 * g, o[n] * inv);
  if (h == heads - 1)                                 // layout padding of the row: zeros
    for (int cc = heads * dv + g; cc < ld_out; cc += 4) st(orow + cc, 0.f);
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <typename T>
__device__ __forceinline__ float dot(const T* __restrict__ a, const T* __restrict__ b, int n) {
  float s = 0.f;
  for (int i = 0; i < n; ++i) s += ld(a + i) * ld(b + i);
  return s;
}

// Any head sizes, strides and alignment: one wave per (group, head, query); rows = groups x heads x queries.
template <typename T, typename Src, bool CAUSAL = false>
__global__ __launch_bounds__(256) void attention_plain_kernel(Src src, T* __restrict__ out, int ld_out, int rows) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= rows) return;                              // the whole wave leaves together; the kernel has no barrier
  const int heads = src.heads, d = src.d, dv = src.dv(), Tq = src.nq();
  const int q = w % Tq, r = w / Tq;
  int Tk = src.nk();
  if constexpr (CAUSAL) Tk = min(Tk, q + 1);          // keys k <= q; no barrier, so the trip count may differ per wave
  const int h = r % heads;
  const typename Src::Block b = src.block(r / heads, h);
  const T* qp = src.q(b, q);
  float mx = -INFINITY;
  for (int k = lane; k < Tk; k += 64) mx = fmaxf(mx, dot(qp, src.k(b, k), d));
  mx = wave_max(mx);
  T* orow = out + src.out_row(b, q) * ld_out;
  for (int c0 = 0; c0 < dv; c0 += 64) {               // 64 output channels at a time, one per lane
    const int cc = c0 + lane;
    float acc = 0.f, ls = 0.f;
    for (int kb = 0; kb < Tk; kb += 64) {
      const int k = kb + lane;
      const float p = k < Tk ? expf(dot(qp, src.k(b, k), d) - mx) : 0.f;
      ls += p;
      const int nk = min(64, Tk - kb);
      for (int kk = 0; kk < nk; ++kk) {
        const float pk = __shfl(p, kk);
        if (cc < dv) acc += pk * ld(src.v(b, kb + kk) + cc);
      }
    }
    const float l = wave_sum(ls);
    if (cc < dv) st(orow + h * dv + cc, acc / l);
  }
  if (h == heads - 1)
    for (int cc = heads * dv + lane; cc < ld_out; cc += 64) st(orow + cc, 0.f);
}

// The MFMA kernel moves 4 elements at a time: every pointer (or'ed into `ptrs`) aligned to 4 elements of
// `elem_size` bytes, every stride (or'ed into `strides`) a multiple of 4.
inline bool attention_vec4(uintptr_t ptrs, int strides, int elem_size) {
  return (strides & 3) == 0 && (ptrs & ((uintptr_t)elem_size * 4 - 1)) == 0;
}

// Launches `groups` groups of src: the MFMA kernel at the smallest DMAX of 32, 64, 128 that holds both head sizes
// when `mfma`, else the plain kernel.  The caller has checked the 32-bit ranges.  CAUSAL selects the masked
// instantiations (the caller has checked nq() == nk()); the default is the kernels as they were.
template <typename T, typename Src, bool CAUSAL = false>
hipError_t attention_core_launch(const Src& src, T* out, int ld_out, int groups, bool mfma, hipStream_t s) {
  if (mfma) {
    const int qtiles = (src.nq() + ATTN_QT - 1) / ATTN_QT;
    const dim3 grid(groups * src.heads * qtiles), block(256);
    const int dm = src.d > src.dv() ? src.d : src.dv();
    if (dm <= 32)
      hipLaunchKernelGGL((attention_mfma_kernel<T, 32, Src, CAUSAL>), grid, block, 0, s, src, out, ld_out, qtiles);
    else if (dm <= 64)
      hipLaunchKernelGGL((attention_mfma_kernel<T, 64, Src, CAUSAL>), grid, block, 0, s, src, out, ld_out, qtiles);
    else
      hipLaunchKernelGGL((attention_mfma_kernel<T, 128, Src, CAUSAL>), grid, block, 0, s, src, out, ld_out, qtiles);
  } else {
    const int rows = groups * src.heads * src.nq();
    hipLaunchKernelGGL((attention_plain_kernel<T, Src, CAUSAL>), dim3((rows + 3) / 4), dim3(256), 0, s, src, out, ld_out,
                       rows);
  }
  return hipGetLastError();
}

}  // namespace attn
}  // namespace adapt
