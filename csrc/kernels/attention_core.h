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
// Padding mask (MASKED = true; self-attention only, never with CAUSAL): the policy hands each group a row of nk()
// floats, and token j is padding iff -1 < mask[j] < 1 (the ids of an Embedding(mask_zero=True): the truncation
// toward zero the `embedding` kernel applies; a NaN is kept).  A padded token is masked as a key and, as a query,
// gets a row of zeros (Keras' row there is the plain mean of V; nothing at a kept position reads it).  Prologue:
// the block reads its group's mask and reduces kend = last kept key + 1 through four LDS words behind the tiles,
// one barrier that every wave meets before any wave-dependent branch.  The key loop and its prefetch end at kend,
// a bound that depends on the group alone, so tiles past it are never loaded; a block with kend = 0 writes zero
// rows and leaves.  A tile's 32 kept flags are fetched one tile ahead with its rows and staged behind them in LDS;
// a masked key's score becomes -inf in the statement that masks the keys beyond the count.  An interior tile that
// is wholly masked is computed and masked, not skipped: there m and the tile maximum are both -inf and the
// exponents are taken against 0, the guard the causal mode has.  A wave whose 16 queries are all padded passes
// the barriers, skips the MFMAs and stores zeros; 1 / l is 0 where l is 0.  The plain kernel finds kend per wave,
// its lane loops skip masked keys (their K and V rows are not read), and a padded query's row is zeros.
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
//   const float* key_mask(b)                MASKED only: the group's nk() mask values
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

// the padding test of a mask value: an id that truncates to 0.  A NaN compares false and is kept
__device__ __forceinline__ bool mask_kept(float v) { return !(v > -1.f && v < 1.f); }

// DMAX: the head sizes this instantiation holds in registers (d, dv <= DMAX, both multiples of 16).  CAUSAL: query
// i attends keys j <= i (nq() == nk()); every line it adds is under `if constexpr`.  MASKED: the padding mask of
// src.key_mask (nq() == nk(), never with CAUSAL), likewise.  The second launch bound (waves per SIMD) holds the MASKED
// instantiations at DMAX 32 and 64 to the occupancy the unmasked ones reach on their own, 6 and 4: without it the
// mask's few extra registers cost them a wave per SIMD (+11 % at 512 tokens, BASELINE.md "Round 19").  DMAX 128 runs
// 2 waves per SIMD either way.  For every other instantiation 1 leaves the compiler's choice, and their
// instructions, as they were
template <typename T, int DMAX, typename Src, bool CAUSAL = false, bool MASKED = false>
__global__ __launch_bounds__(256, MASKED ? (DMAX == 32 ? 6 : DMAX == 64 ? 4 : 1) : 1) void attention_mfma_kernel(Src src, T* __restrict__ out, int ld_out, int qtiles) {
  static_assert(!(CAUSAL && MASKED), "a padding mask together with the causal mask is not built");
  constexpr int ND = DMAX / 16;                       // 16-wide slices of d / dv
  constexpr int NST = ATTN_KT * DMAX / 512;           // staged 4-element vectors per thread (K and V together)
  constexpr int TILES = 2 * ATTN_KT * (DMAX + ATTN_PAD);
  // MASKED: behind the tiles the staged tile's ATTN_KT kept flags, then one partial key bound per wave
  __shared__ __attribute__((aligned(16))) float smem[TILES + (MASKED ? ATTN_KT + 4 : 0)];
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
  // the keys this block walks: all of them, under the causal mask those up to the last query of its tile, under
  // the padding mask those up to the group's last kept key.  Block-uniform (from qt or the group, never from
  // wave): every wave passes both barriers of every iteration
  int kend = Tk;
  if constexpr (CAUSAL) kend = min(Tk, (qt + 1) * ATTN_QT);
  [[maybe_unused]] const float* mk = nullptr;         // MASKED: the group's mask row
  [[maybe_unused]] bool qkeep = true, wkeep = true;   // MASKED: this lane's query is kept; any query of the wave is
  if constexpr (MASKED) {
    mk = src.key_mask(b);
    int ke = 0;
    for (int j = tid; j < Tk; j += 256)
      if (mask_kept(mk[j])) ke = j + 1;               // ascending: the thread's last kept key stays
#pragma unroll
    for (int o_ = 32; o_ > 0; o_ >>= 1) ke = max(ke, __shfl_xor(ke, o_));
    int* sbound = (int*)(smem + TILES + ATTN_KT);
    if (lane == 0) sbound[wave] = ke;
    __syncthreads();                                  // before any wave-dependent branch: all four waves meet it
    kend = __builtin_amdgcn_readfirstlane(max(max(sbound[0], sbound[1]), max(sbound[2], sbound[3])));
    qkeep = qok && mask_kept(mk[qok ? qtok : 0]);
    wkeep = __ballot(qkeep) != 0;                     // wave-uniform
    if (kend == 0) {                                  // no key kept in the group: zero rows, and the block leaves
      if (!qok) return;
      T* zrow = out + src.out_row(b, qrow) * ld_out;
#pragma unroll
      for (int n = 0; n < ND; ++n)
        if (16 * n < dv) st4(zrow + h * dv + 16 * n + 4 * g, f32x4{0.f, 0.f, 0.f, 0.f});
      if (h == heads - 1)
        for (int cc = heads * dv + g; cc < ld_out; cc += 4) st(zrow + cc, 0.f);
      return;
    }
  }
  f32x4 qf[ND];
#pragma unroll
  for (int t = 0; t < ND; ++t) {
    qf[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (MASKED) {
      if (qkeep && 16 * t < d) qf[t] = ld4(src.q(b, qrow) + 16 * t + 4 * g);      // a padded query's row is not read
    } else {
      if (qok && 16 * t < d) qf[t] = ld4(src.q(b, qrow) + 16 * t + 4 * g);
    }
  }
  f32x4 o[ND];
#pragma unroll
  for (int n = 0; n < ND; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;                       // l: this lane's keys only, summed over the groups at the end

  f32x4 st_[NST];
#pragma unroll
  for (int j = 0; j < NST; ++j) {
    st_[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (sval[j] && srow[j] < kend) st_[j] = src.stage(b, sisv[j], srow[j], sgcol[j]);
  }
  [[maybe_unused]] float kp_ = 0.f;                   // MASKED, tid < ATTN_KT: 1 where key k0 + tid is kept
  if constexpr (MASKED) {
    if (tid < ATTN_KT && tid < kend) kp_ = mask_kept(mk[tid]) ? 1.f : 0.f;
  }
  for (int k0 = 0; k0 < kend; k0 += ATTN_KT) {        // the same trip count for every wave of the block
    __syncthreads();                                  // the previous tile has been read
#pragma unroll
    for (int j = 0; j < NST; ++j)
      if (sval[j]) *(f32x4*)(smem + sloff[j]) = st_[j];
    if constexpr (MASKED) {
      if (tid < ATTN_KT) smem[TILES + tid] = kp_;
    }
    __syncthreads();
    if constexpr (MASKED) {
      if (tid < ATTN_KT) {
        const int r = k0 + ATTN_KT + tid;
        kp_ = r < kend && mask_kept(mk[r < kend ? r : 0]) ? 1.f : 0.f;
      }
    }
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
    if constexpr (MASKED) {
      if (!wkeep) continue;                           // all 16 queries are padding: zeros are stored after the loop
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
    for (int u = 0; u < ATTN_KT / 16; ++u) {
      [[maybe_unused]] f32x4 kf4 = f32x4{1.f, 1.f, 1.f, 1.f};
      if constexpr (MASKED) kf4 = *(const f32x4*)(smem + TILES + 16 * u + 4 * g);   // the flags of this lane's keys
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        bool masked = k0 + 16 * u + 4 * g + i >= Tk;
        if constexpr (CAUSAL) masked = masked || k0 + 16 * u + 4 * g + i > qtok;    // before the maximum is taken
        if constexpr (MASKED) masked = masked || kf4[i] == 0.f;
        if (masked) s[u][i] = -INFINITY;
        mx = fmaxf(mx, s[u][i]);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));               // finite: key k0 is in every tile (MASKED: unless it is padding)
    const float mn = fmaxf(m, mx);
    float me = mn;                                    // what the exponents are taken against
    if constexpr (CAUSAL || MASKED) {
      // a query that has seen no key yet and sees none in this tile (causal: none with today's tiles, a processed
      // tile holds key q0 <= qtok; padding mask: every tile before the first kept key): exp(-inf - 0) = 0 for
      // alpha and every p, never exp(-inf - -inf)
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
  float inv = 1.f / l;
  if constexpr (MASKED) {
    if (l == 0.f) inv = 0.f;
    if (!qkeep) {                                     // a padded query: zeros, whatever the arithmetic carried
      inv = 0.f;
#pragma unroll
      for (int n = 0; n < ND; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
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
template <typename T, typename Src, bool CAUSAL = false, bool MASKED = false>
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
  if constexpr (MASKED) {
    // the padding mask: a body of its own, so that the one below stays the text, and the instructions, it was
    static_assert(!CAUSAL, "a padding mask together with the causal mask is not built");
    const float* mk = src.key_mask(b);                // the group's mask row
    int ke = 0;
    for (int k = lane; k < Tk; k += 64)
      if (mask_kept(mk[k])) ke = k + 1;
#pragma unroll
    for (int o_ = 32; o_ > 0; o_ >>= 1) ke = max(ke, __shfl_xor(ke, o_));
    Tk = ke;                                          // the last kept key + 1: nothing beyond it is read
    T* orow = out + src.out_row(b, q) * ld_out;
    if (Tk == 0 || !mask_kept(mk[q])) {               // wave-uniform: a padded query, or no key kept: a row of zeros
      for (int cc = lane; cc < dv; cc += 64) st(orow + h * dv + cc, 0.f);
    } else {
      float mx = -INFINITY;
      for (int k = lane; k < Tk; k += 64)
        if (mask_kept(mk[k])) mx = fmaxf(mx, dot(qp, src.k(b, k), d));
      mx = wave_max(mx);
      for (int c0 = 0; c0 < dv; c0 += 64) {
        const int cc = c0 + lane;
        float acc = 0.f, ls = 0.f;
        for (int kb = 0; kb < Tk; kb += 64) {
          const int k = kb + lane;
          const bool kin = k < Tk && mask_kept(mk[k < Tk ? k : 0]);
          const float p = kin ? expf(dot(qp, src.k(b, k), d) - mx) : 0.f;     // a masked key's K row is not read
          ls += p;
          const unsigned long long km = __ballot(kin);                          // which of the 64 keys are kept
          const int nk = min(64, Tk - kb);
          for (int kk = 0; kk < nk; ++kk) {
            if (!((km >> kk) & 1)) continue;          // wave-uniform: a masked key's V row is not read
            const float pk = __shfl(p, kk);
            if (cc < dv) acc += pk * ld(src.v(b, kb + kk) + cc);
          }
        }
        const float l = wave_sum(ls);                 // > 0: the kept query is itself a kept key
        if (cc < dv) st(orow + h * dv + cc, acc / l);
      }
    }
    if (h == heads - 1)
      for (int cc = heads * dv + lane; cc < ld_out; cc += 64) st(orow + cc, 0.f);
    return;
  }
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
// instantiations (the caller has checked nq() == nk()), MASKED those under the padding mask of src.key_mask; the
// default is the kernels as they were.
template <typename T, typename Src, bool CAUSAL = false, bool MASKED = false>
hipError_t attention_core_launch(const Src& src, T* out, int ld_out, int groups, bool mfma, hipStream_t s) {
  if (mfma) {
    const int qtiles = (src.nq() + ATTN_QT - 1) / ATTN_QT;
    const dim3 grid(groups * src.heads * qtiles), block(256);
    const int dm = src.d > src.dv() ? src.d : src.dv();
    if (dm <= 32)
      hipLaunchKernelGGL((attention_mfma_kernel<T, 32, Src, CAUSAL, MASKED>), grid, block, 0, s, src, out, ld_out, qtiles);
    else if (dm <= 64)
      hipLaunchKernelGGL((attention_mfma_kernel<T, 64, Src, CAUSAL, MASKED>), grid, block, 0, s, src, out, ld_out, qtiles);
    else
      hipLaunchKernelGGL((attention_mfma_kernel<T, 128, Src, CAUSAL, MASKED>), grid, block, 0, s, src, out, ld_out, qtiles);
  } else {
    const int rows = groups * src.heads * src.nq();
    hipLaunchKernelGGL((attention_plain_kernel<T, Src, CAUSAL, MASKED>), dim3((rows + 3) / 4), dim3(256), 0, s, src, out, ld_out,
                       rows);
  }
  return hipGetLastError();
}

}  // namespace attn
}  // namespace adapt
