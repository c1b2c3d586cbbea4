// Incremental decoding: the key / value cache kernels and the decode attention kernel, fp32 and bf16, gfx950.
// attention_decode.hip instantiates them and keeps the argument checks and the entry points.
//
// Cache layout.  K is [B][hkv][Tmax][d] and V [B][hkv][Tmax][dv] in the activation type: the key stream of one
// (sequence, kv head) is contiguous and rows are unpadded.  `pos` is int32 [B] on the device: sequence b holds
// pos[b] tokens before a step, so a captured graph replays with advancing, per-sequence lengths.
//
// kv_append_kernel: B * Tn projection rows [Q: hq d | K: hkv d | V: hkv dv] at row stride ld; token j of
// sequence b has position pos[b] + j.  ROPE: Q and K are rotated at that position by the rotate-half convention
// with the cos / sin of the fp32 table [2][Ttab][d/2] (the formulas of layers.hip's rope kernel), Q goes to the
// q_out row (hq d channels, the rest of its ld_q zeros), K and V into the caches.  !ROPE (prefill: the plan's rope
// step has rotated already): K and V are copied, no Q.  A position outside [0, Tmax), or at or beyond Ttab,
// writes nothing: a kernel cannot raise, the host checks the bounds.  VEC = 16 bytes per thread where the head
// sizes, strides and bases allow, else 1.
//
// attention_decode_kernel<T, DMAX, VV>: one query per sequence against the keys 0 .. pos[b] of its cache, all
// query heads.  Math is fp32 whatever T (bf16 is widened on load, the output rounded once).
//
//   * Grid (S, hkv, B).  A block of 4 waves owns the contiguous key range [s KS, (s + 1) KS) of one (sequence, kv
//     head) for all g = hq / hkv query heads of that kv head at once: the g query rows, zero-padded to 16, are the
//     16-wide free dimension of v_mfma_f32_16x16x4_f32, so K and V of a kv head are read once per group, not g
//     times.  Q (16 x d, mostly zeros) is loaded once per block into registers.
//   * Swapped products, the form attention_core.h documents.  S^T = K Q^T has a 16-key fragment as the A operand:
//     lane (c = lane & 15, q = lane >> 4) loads key c's channels 4 VK q' .. in 16-byte vectors (VK = 4 fp32 / 8
//     bf16 elements; chunk t covers channels 4 VK t + VK q + e, and Q is held in the same order), and the result
//     register i holds for query c the key 4 q + i.  That register is the B operand of O^T = V^T P^T; its A
//     operand is V read in the same key order: lane (c, q) loads for key 4 q + i the VV channels VV c .. of a
//     16 VV-channel block, element e of the vector feeding the MFMA whose row c stands for channel VV c + e.  The
//     lane then holds for query c the 4 VV consecutive channels 4 VV q + VV j + e.  P never leaves registers.
//     VV = 4 (16-byte fp32 / 8-byte bf16 loads); bf16 at DMAX 128 takes VV = 8, where the 16 lanes of a 16-byte
//     load cover the head (at smaller heads half of its MFMA rows would be padding).
//   * No LDS staging of K or V: every cache element is used by exactly one wave exactly once.  Wave w takes the
//     16-key fragments w, w + 4, ... of the block's range straight from global memory, and the next fragment's
//     loads are issued before the current fragment's MFMAs.
//   * Per-wave online softmax (running maximum, running sum, O^T accumulators, exact expf).  A key beyond pos[b]
//     is never loaded (its K and V vectors are zeros) and scores -inf before the maximum is taken; where the
//     running and the fragment maximum are both -inf the exponent is taken against 0; a fragment with no visible
//     key is not visited.
//   * Merges, deterministic and without atomics.  The 4 waves' (m, l, O) of the g real rows meet in LDS and are
//     combined in wave order by the log-sum-exp rule.  S == 1: the block normalises and stores hq dv channels per
//     sequence (the block of the last kv head writes the rest of the row as zeros).  Else it writes (m, l,
//     unnormalised O) of its g rows to the fp32 workspace [B][hkv][S][g][dv + 2], and
//     attention_decode_combine_kernel merges the S partials in split order.  A split whose range starts beyond
//     pos[b] writes m = -inf, l = 0 and leaves; the combine kernel skips it (weight exactly 0, its O never read).
//   * S and KS depend on (B, hkv, Tmax) and the CU count alone (decode_plan), never on the lengths.
//
// The 1/sqrt(d) scale is already in Q.  Index math: element offsets inside one tensor are 32-bit, the entry points
// refuse what does not fit.
#pragma once
#include "attention_core.h"

namespace adapt {
namespace attn {

constexpr int DEC_FRAG = 16;   // keys per fragment (one MFMA tile)
constexpr int DEC_KSQ = 64;    // KS is a multiple of this: one fragment per wave

// S splits of KS keys: about `2 cus` blocks where Tmax allows
inline void decode_plan(int B, int hkv, int Tmax, int cus, int* S, int* KS) {
  long long want = (2ll * cus) / ((long long)B * hkv);
  if (want < 1) want = 1;
  long long ks = ((Tmax + want - 1) / want + DEC_KSQ - 1) / DEC_KSQ * DEC_KSQ;
  *KS = (int)ks;
  *S = (int)((Tmax + ks - 1) / ks);
}

template <typename T, int N>
struct DecVec {
  float f[N];
};

// N elements at p, widened; N * sizeof(T) bytes in one load
template <typename T, int N>
__device__ __forceinline__ DecVec<T, N> dec_ld(const T* p) {
  DecVec<T, N> r;
  if constexpr (N == 1) {
    r.f[0] = ld(p);
  } else if constexpr (sizeof(T) == 4) {
    static_assert(N == 4, "fp32 vectors are 16 bytes");
    const f32x4 q = *(const f32x4*)p;
    r.f[0] = q.x; r.f[1] = q.y; r.f[2] = q.z; r.f[3] = q.w;
  } else if constexpr (N == 4) {
    const f32x4 q = ld4(p);
    r.f[0] = q.x; r.f[1] = q.y; r.f[2] = q.z; r.f[3] = q.w;
  } else {
    static_assert(N == 8, "bf16 vectors are 8 or 16 bytes");
    V8 q;
    q.u = *(const u32x4*)p;
#pragma unroll
    for (int e = 0; e < 8; ++e) r.f[e] = bf2f(q.e[e]);
  }
  return r;
}

template <typename T, int N>
__device__ __forceinline__ void dec_st(T* p, const DecVec<T, N>& r) {
  if constexpr (N == 1) {
    st(p, r.f[0]);
  } else if constexpr (sizeof(T) == 4) {
    *(f32x4*)p = f32x4{r.f[0], r.f[1], r.f[2], r.f[3]};
  } else {
    V8 q;
#pragma unroll
    for (int e = 0; e < 8; ++e) q.e[e] = f2bf(r.f[e]);
    *(u32x4*)p = q.u;
  }
}

// bit copy of N elements
template <typename T, int N>
__device__ __forceinline__ void dec_cp(T* dst, const T* src) {
  if constexpr (N == 1) *dst = *src;
  else *(u32x4*)dst = *(const u32x4*)src;
}

struct KvAppendArgs {
  int Tn, Tmax, Ttab, hq, hkv, d, dv, ld, ld_q;
  int nq, nk, nv, nz;                                 // units per row: Q, K, V, zeros of the q_out row
  int total;
};

template <typename T, int VEC, bool ROPE>
__global__ __launch_bounds__(256) void kv_append_kernel(const T* __restrict__ x, const float* __restrict__ table,
                                                         const int* __restrict__ pos, T* __restrict__ kc,
                                                         T* __restrict__ vc, T* __restrict__ q_out, KvAppendArgs a) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= a.total) return;
  const int per = a.nq + a.nk + a.nv + a.nz;
  const int row = idx / per;
  int u = idx % per;
  const int b = row / a.Tn;
  const int p = pos[b] + row % a.Tn;
  if (p < 0 || p >= a.Tmax || (ROPE && p >= a.Ttab)) return;
  const T* xr = x + row * a.ld;
  const int half = a.d / 2;
  if (u < a.nq + a.nk) {
    if constexpr (ROPE) {
      // one vector of a head's first half and its partner at + d/2; heads 0 .. hq - 1 are Q, the rest K
      const int hv = half / VEC;
      const int head = u / hv, i = (u % hv) * VEC;
      const T* src = xr + head * a.d + i;
      T* dst = head < a.hq ? q_out + row * a.ld_q + head * a.d + i
                           : kc + ((b * a.hkv + head - a.hq) * a.Tmax + p) * a.d + i;
      const float* cs = table + p * half + i;         // cos; sin lies Ttab * half further on
      const float* sn = cs + a.Ttab * half;
      const DecVec<T, VEC> xa = dec_ld<T, VEC>(src), xb = dec_ld<T, VEC>(src + half);
      DecVec<T, VEC> oa, ob;
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        const float c = cs[e], s = sn[e];
        oa.f[e] = xa.f[e] * c - xb.f[e] * s;
        ob.f[e] = xb.f[e] * c + xa.f[e] * s;
      }
      dec_st<T, VEC>(dst, oa);
      dec_st<T, VEC>(dst + half, ob);
    } else {
      // nq = 0: K is copied as it stands
      const int col = u * VEC, head = col / a.d, i = col % a.d;
      dec_cp<T, VEC>(kc + ((b * a.hkv + head) * a.Tmax + p) * a.d + i, xr + a.hq * a.d + col);
    }
    return;
  }
  u -= a.nq + a.nk;
  if (u < a.nv) {
    const int col = u * VEC, head = col / a.dv, i = col % a.dv;
    dec_cp<T, VEC>(vc + ((b * a.hkv + head) * a.Tmax + p) * a.dv + i, xr + (a.hq + a.hkv) * a.d + col);
    return;
  }
  if constexpr (ROPE) {
    DecVec<T, VEC> z;
#pragma unroll
    for (int e = 0; e < VEC; ++e) z.f[e] = 0.f;
    dec_st<T, VEC>(q_out + row * a.ld_q + a.hq * a.d + (u - a.nv) * VEC, z);
  }
}

__global__ void advance_positions_kernel(int* __restrict__ pos, int B, int n) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) pos[b] += n;
}

struct DecodeArgs {
  int Tmax, hq, hkv, d, dv, ld_q, ld_out, S, KS;
};

// The keys of one fragment as this lane holds them: its K row's channel vectors and the V vectors of its 4 keys
template <int DMAX, int VK, int VV>
struct DecFrag {
  static constexpr int NCH = (DMAX + 4 * VK - 1) / (4 * VK);     // K chunks of 4 VK channels
  static constexpr int NVB = (DMAX + 16 * VV - 1) / (16 * VV);   // V blocks of 16 VV channels
  float k[NCH][VK];
  float v[4][NVB][VV];
};

// Fragment at key0 of the stream kb / vb; a key at or beyond L, and a channel at or beyond d / dv, loads zeros
template <typename T, int DMAX, int VK, int VV>
__device__ __forceinline__ void dec_load(DecFrag<DMAX, VK, VV>& f, const T* __restrict__ kb, const T* __restrict__ vb,
                                         int key0, int L, int d, int dv, int c, int q) {
  using F = DecFrag<DMAX, VK, VV>;
  const bool kin = key0 + c < L;
#pragma unroll
  for (int t = 0; t < F::NCH; ++t) {
    const int ch = 4 * VK * t + VK * q;
    DecVec<T, VK> r;
#pragma unroll
    for (int e = 0; e < VK; ++e) r.f[e] = 0.f;
    if (kin && ch < d) r = dec_ld<T, VK>(kb + (key0 + c) * d + ch);
#pragma unroll
    for (int e = 0; e < VK; ++e) f.k[t][e] = r.f[e];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int key = key0 + 4 * q + i;
#pragma unroll
    for (int n = 0; n < F::NVB; ++n) {
      const int ch = 16 * VV * n + VV * c;
      DecVec<T, VV> r;
#pragma unroll
      for (int e = 0; e < VV; ++e) r.f[e] = 0.f;
      if (key < L && ch < dv) r = dec_ld<T, VV>(vb + key * dv + ch);
#pragma unroll
      for (int e = 0; e < VV; ++e) f.v[i][n][e] = r.f[e];
    }
  }
}

template <typename T, int DMAX, int VV>
__global__ __launch_bounds__(256) void attention_decode_kernel(const T* __restrict__ qbuf, const T* __restrict__ kc,
                                                                const T* __restrict__ vc, const int* __restrict__ pos,
                                                                T* __restrict__ out, float* __restrict__ ws,
                                                                DecodeArgs a) {
  constexpr int VK = 16 / sizeof(T);
  using F = DecFrag<DMAX, VK, VV>;
  constexpr int NCH = F::NCH, NVB = F::NVB;
  constexpr int LROW = DMAX + 2;                      // LDS row of a (wave, query): O, m, l
  __shared__ float smem[4 * 16 * LROW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, q = lane >> 4;
  const int split = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
  const int d = a.d, dv = a.dv, G = a.hq / a.hkv;
  int L = pos[b] + 1;                                 // keys 0 .. pos[b]; never beyond the cache
  L = L < 0 ? 0 : L > a.Tmax ? a.Tmax : L;
  const int k_begin = split * a.KS;
  const int k_end = min(k_begin + a.KS, L);
  float* wrow = ws + (((size_t)(b * a.hkv + kvh) * a.S + split) * G) * (dv + 2);
  if (a.S > 1 && k_begin >= L) {                      // an empty split (block-uniform): m = -inf, l = 0, O unwritten
    if (tid < G) {
      wrow[tid * (dv + 2)] = -INFINITY;
      wrow[tid * (dv + 2) + 1] = 0.f;
    }
    return;
  }
  const T* kb = kc + (size_t)(b * a.hkv + kvh) * a.Tmax * d;
  const T* vb = vc + (size_t)(b * a.hkv + kvh) * a.Tmax * dv;

  // Q of query head kvh G + c in the K chunk order; rows G .. 15 are zeros
  float qf[NCH][VK];
#pragma unroll
  for (int t = 0; t < NCH; ++t) {
    const int ch = 4 * VK * t + VK * q;
    DecVec<T, VK> r;
#pragma unroll
    for (int e = 0; e < VK; ++e) r.f[e] = 0.f;
    if (c < G && ch < d) r = dec_ld<T, VK>(qbuf + b * a.ld_q + (kvh * G + c) * d + ch);
#pragma unroll
    for (int e = 0; e < VK; ++e) qf[t][e] = r.f[e];
  }
  f32x4 o[NVB][VV];
#pragma unroll
  for (int n = 0; n < NVB; ++n)
#pragma unroll
    for (int e = 0; e < VV; ++e) o[n][e] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;                       // l: this lane's keys only, summed over the lane groups below

  // k_end bounds the loads: a fragment straddles L alone (KS is a multiple of the fragment), and a fragment at or
  // beyond k_end is all predicates off, so the prefetch behind the wave's last fragment loads nothing
  F cur, nxt;
  int key0 = k_begin + wave * DEC_FRAG;
  dec_load<T, DMAX, VK, VV>(cur, kb, vb, key0, k_end, d, dv, c, q);
  for (; key0 < k_end; key0 += 4 * DEC_FRAG) {        // a fragment with no visible key is not visited
    dec_load<T, DMAX, VK, VV>(nxt, kb, vb, key0 + 4 * DEC_FRAG, k_end, d, dv, c, q);
    // S^T = K Q^T: s[i] = score(key key0 + 4 q + i, query c)
    f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NCH; ++t)
#pragma unroll
      for (int e = 0; e < VK; ++e) s = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.k[t][e], qf[t][e], s, 0, 0, 0);
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (key0 + 4 * q + i >= L) s[i] = -INFINITY;    // before the maximum is taken
      mx = fmaxf(mx, s[i]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float mn = fmaxf(m, mx);
    const float me = mn == -INFINITY ? 0.f : mn;      // never exp(-inf - -inf)
    const float alpha = expf(m - me);
    m = mn;
    float ps = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      s[i] = expf(s[i] - me);
      ps += s[i];
    }
    l = l * alpha + ps;
    // O^T += V^T P^T: o[n][e][j] = O(query c, channel 16 VV n + VV (4 q + j) + e)
#pragma unroll
    for (int n = 0; n < NVB; ++n)
#pragma unroll
      for (int e = 0; e < VV; ++e) {
        o[n][e] *= alpha;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[n][e] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.v[i][n][e], s[i], o[n][e], 0, 0, 0);
      }
    cur = nxt;
  }
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);

  // the waves' states of the G real rows meet in LDS
  if (c < G) {
    float* r = smem + (wave * 16 + c) * LROW;
#pragma unroll
    for (int n = 0; n < NVB; ++n)
#pragma unroll
      for (int e = 0; e < VV; ++e)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int ch = 16 * VV * n + VV * (4 * q + j) + e;
          if (ch < dv) r[ch] = o[n][e][j];
        }
    if (q == 0) {
      r[DMAX] = m;
      r[DMAX + 1] = l;
    }
  }
  __syncthreads();
  // thread per (row, channel): the 4 states in wave order by the log-sum-exp rule
  for (int idx = tid; idx < G * dv; idx += 256) {
    const int row = idx / dv, ch = idx - row * dv;
    const float* r = smem + row * LROW;
    float M = -INFINITY;
#pragma unroll
    for (int w = 0; w < 4; ++w) M = fmaxf(M, r[w * 16 * LROW + DMAX]);
    const float Me = M == -INFINITY ? 0.f : M;
    float lsum = 0.f, acc = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float wgt = expf(r[w * 16 * LROW + DMAX] - Me);      // a wave that saw no key: exp(-inf) = 0, O and l are 0
      lsum += r[w * 16 * LROW + DMAX + 1] * wgt;
      acc += r[w * 16 * LROW + ch] * wgt;
    }
    if (a.S == 1) {
      st(out + b * a.ld_out + (kvh * G + row) * dv + ch, lsum > 0.f ? acc / lsum : 0.f);
    } else {
      float* wr = wrow + row * (dv + 2);
      wr[2 + ch] = acc;
      if (ch == 0) {
        wr[0] = M;
        wr[1] = lsum;
      }
    }
  }
  if (a.S == 1 && kvh == a.hkv - 1)                   // layout padding of the row: zeros
    for (int cc = a.hq * dv + tid; cc < a.ld_out; cc += 256) st(out + b * a.ld_out + cc, 0.f);
}

// Thread per element of out [B][ld_out]: the S partials of its (sequence, head) in split order
template <typename T>
__global__ __launch_bounds__(256) void attention_decode_combine_kernel(const float* __restrict__ ws, T* __restrict__ out,
                                                                        DecodeArgs a, int total) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int b = idx / a.ld_out, col = idx - b * a.ld_out;
  const int dv = a.dv, G = a.hq / a.hkv;
  if (col >= a.hq * dv) {
    st(out + idx, 0.f);
    return;
  }
  const int h = col / dv, ch = col - h * dv;
  const int kvh = h / G, row = h - kvh * G;
  const float* p = ws + ((size_t)(b * a.hkv + kvh) * a.S * G + row) * (dv + 2);
  const int stride = G * (dv + 2);
  float M = -INFINITY;
  for (int s = 0; s < a.S; ++s) M = fmaxf(M, p[s * stride]);
  float lsum = 0.f, acc = 0.f;
  for (int s = 0; s < a.S; ++s) {
    const float ms = p[s * stride];
    if (ms == -INFINITY) continue;                    // an empty split: weight exactly 0, its O is not read
    const float wgt = expf(ms - M);
    lsum += p[s * stride + 1] * wgt;
    acc += p[s * stride + 2 + ch] * wgt;
  }
  st(out + idx, lsum > 0.f ? acc / lsum : 0.f);
}

}  // namespace attn
}  // namespace adapt
