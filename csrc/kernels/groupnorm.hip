// GroupNormalization (Keras semantics) on an NHWC map, fp32 and bf16, gfx950.
//
//   x [B][P][Cs], P = H * W pixels, Cs = C (fp32) or C padded to a multiple of 8 (bf16: the padding channels are
//   layout, not data); G groups of Cg = C / G channels.  Per (image, group):
//   mu = mean over (P, Cg), var = the biased variance over the same set,
//   y = act((x - mu) * rsqrt(var + eps) * gamma[c] + beta[c]).
//
// One (image, group) is P * Cg values strided through the map (65 K to 1 M values in the Stable Diffusion VAE
// decoder), so the statistics are a cross-block reduction.  It is deterministic and cancellation-safe:
//
// * Statistics are (n, mean, M2) triples.  A thread owns one 16-byte channel column (4 fp32 / 8 bf16 channels) and
//   walks pixels; per channel it keeps the sums of d = x - K and d^2 with K the first value it saw, so d is the
//   size of the spread, not of the mean, and M2 = sum d^2 - (sum d)^2 / n loses no more than a digit (E[x^2] -
//   mu^2 on the raw values loses all of them at mean 100 / sigma 0.1).  Triples are merged with Chan's formula
//   in a fixed order: a tree over the block's pixel rows in LDS, then the group's channels, then the image's
//   slabs.  No float atomics anywhere, so two runs, and a sliced and an unsliced run, agree bit for bit.
// * Vector path (C % 4 == 0 in fp32, always in bf16; at most 256 vectors per pixel): a block of 512 threads is
//   TX x TY, TX the power of two >= vectors per pixel, so a wave reads whole contiguous pixel rows with 16-byte
//   loads.  A vector may straddle groups (Cg = 2 in fp32, Cg <= 4 in bf16): the statistics are kept per channel
//   until the rows are merged, and the epilogue looks the group up per channel.
//     - single launch: where an image fits the block's registers (at most GN_FUSED_ROWS vectors per thread) one
//       block per image reads x once, reduces on chip and writes y once; no workspace.
//     - split: a statistics launch over (slab of pixels, image) writes one triple per (image, slab, group) to
//       the workspace, a one-wave-per-many-groups finalize launch merges the slabs in order into (mu, rstd), and
//       the apply launch reads those.  x is read twice.
// * Scalar path (C % 4 != 0 in fp32, or more than 256 vectors per pixel): the same three launches with scalar
//   accesses, one block per (slab, group, image).
// * Epilogue: (x - mu) * (rstd * gamma) + beta (the subtraction first: x * scale + shift would cancel at
//   mean >> sigma), then the folded activation (common.h ActMode).
// * bf16 padding channels C..Cp-1 never enter the statistics or the arithmetic whatever they hold and are
//   written as zeros.
//
// The workspace is sized by groupnorm_workspace_floats() and owned by the caller (the executor allocates it once),
// so every launch is graph-capturable.  Index math is 32-bit: the launchers refuse B * P * Cs >= 2^31.
#include <algorithm>

#include "kernels.h"

namespace adapt {
namespace {

constexpr int GN_THREADS = 512;        // vector kernels: TX x TY
constexpr int GN_MAX_NVEC = 256;       // 16-byte vectors per pixel the vector path takes
constexpr int GN_FUSED_ROWS = 8;       // vectors a thread of the single launch holds in registers
constexpr int GN_MAX_SLABS = 128;      // slabs per image (the finalize launch merges them serially)
constexpr int GN_APPLY_ROWS = 16;      // pixels per thread of an apply block
constexpr int GN_SC_THREADS = 256;     // scalar kernels

struct Stat {
  float n, mean, m2;
};

// Chan's pairwise update; either side may be empty (n = 0, mean = m2 = 0)
__device__ __forceinline__ Stat gn_merge(Stat a, Stat b) {
  const float n = a.n + b.n;
  const float f = n > 0.f ? b.n / n : 0.f;
  const float d = b.mean - a.mean;
  return Stat{n, a.mean + d * f, a.m2 + b.m2 + d * d * a.n * f};
}

// sums of d = x - k and d^2 over n values -> (n, mean, M2)
__device__ __forceinline__ Stat gn_from_sums(float n, float k, float s1, float s2) {
  if (!(n > 0.f)) return Stat{0.f, 0.f, 0.f};
  return Stat{n, k + s1 / n, fmaxf(s2 - s1 * s1 / n, 0.f)};
}

template <typename T>
struct GnVec;
template <>
struct GnVec<float> {
  static constexpr int N = 4;
  using raw = f32x4;
  // channels >= nreal are not data: zeros
  static __device__ __forceinline__ void unpack(const raw& r, int nreal, float (&f)[4]) {
    f[0] = r.x, f[1] = r.y, f[2] = r.z, f[3] = r.w;
#pragma unroll
    for (int e = 0; e < 4; ++e) f[e] = e < nreal ? f[e] : 0.f;
  }
  static __device__ __forceinline__ raw pack(const float (&f)[4]) { return raw{f[0], f[1], f[2], f[3]}; }
  static __device__ __forceinline__ void load_affine(const float* p, int col, float (&f)[4]) {
    const f32x4 v = ((const f32x4*)p)[col];
    f[0] = v.x, f[1] = v.y, f[2] = v.z, f[3] = v.w;
  }
};
template <>
struct GnVec<bf16> {
  static constexpr int N = 8;
  using raw = u32x4;
  static __device__ __forceinline__ void unpack(const raw& r, int nreal, float (&f)[8]) {
    V8 t;
    t.u = r;
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = e < nreal ? bf2f(t.e[e]) : 0.f;     // pads never enter
  }
  static __device__ __forceinline__ raw pack(const float (&f)[8]) {
    V8 t;
#pragma unroll
    for (int e = 0; e < 8; ++e) t.e[e] = f2bf(f[e]);
    return t.u;
  }
  static __device__ __forceinline__ void load_affine(const float* p, int col, float (&f)[8]) {
    const f32x4 a = ((const f32x4*)p)[2 * col], b = ((const f32x4*)p)[2 * col + 1];
    f[0] = a.x, f[1] = a.y, f[2] = a.z, f[3] = a.w, f[4] = b.x, f[5] = b.y, f[6] = b.z, f[7] = b.w;
  }
};

// The statistics of pixels [p0, p1) of image b for every group (FUSED: the whole image, then the output).
// grid (slabs, B), block GN_THREADS = TX x TY with TX = 1 << txs >= nvec.
template <typename T, bool FUSED, bool GEN>
__global__ __launch_bounds__(GN_THREADS) void gn_vec_kernel(const T* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, T* __restrict__ y,
                                                            float* __restrict__ ws, int P, int nvec, int C, int G,
                                                            int PS, int txs, float eps, int act, float alpha) {
  using V = GnVec<T>;
  using raw = typename V::raw;
  constexpr int N = V::N;
  __shared__ float sm_mean[N * GN_THREADS];      // tree: [e][thread]; afterwards per channel [c]
  __shared__ float sm_m2[N * GN_THREADS];
  __shared__ float sm_n[GN_THREADS];
  const int t = threadIdx.x;
  const int TX = 1 << txs, TY = GN_THREADS >> txs;
  const int tx = t & (TX - 1), ty = t >> txs;
  const int b = blockIdx.y, S = gridDim.x;
  const int p0 = FUSED ? 0 : blockIdx.x * PS;
  const int p1 = FUSED ? P : min(P, p0 + PS);
  const bool col = tx < nvec;
  const int nreal = min(max(C - tx * N, 0), N);           // real channels of this thread's vector
  const int Cg = C / G;
  const raw* xb = (const raw*)x + (size_t)b * P * nvec;

  float k[N], s1[N], s2[N];
#pragma unroll
  for (int e = 0; e < N; ++e) k[e] = s1[e] = s2[e] = 0.f;
  float cnt = 0.f;
  raw v[FUSED ? GN_FUSED_ROWS : 1];
  if constexpr (FUSED) {
#pragma unroll
    for (int r = 0; r < GN_FUSED_ROWS; ++r) {
      const int p = ty + r * TY;
      v[r] = raw{0, 0, 0, 0};
      if (col && p < P) v[r] = xb[(size_t)p * nvec + tx];
    }
#pragma unroll
    for (int r = 0; r < GN_FUSED_ROWS; ++r) {
      const int p = ty + r * TY;
      if (col && p < P) {
        float f[N];
        V::unpack(v[r], nreal, f);
#pragma unroll
        for (int e = 0; e < N; ++e) {
          if (r == 0) k[e] = f[e];                         // ty < P here: row 0 is the thread's first pixel
          const float d = f[e] - k[e];
          s1[e] += d;
          s2[e] += d * d;
        }
        cnt += 1.f;
      }
    }
  } else {
    if (col && p0 + ty < p1) {
      float f[N];
      V::unpack(xb[(size_t)(p0 + ty) * nvec + tx], nreal, f);
#pragma unroll
      for (int e = 0; e < N; ++e) k[e] = f[e];
    }
    if (col) {
#pragma unroll 4
      for (int p = p0 + ty; p < p1; p += TY) {
        float f[N];
        V::unpack(xb[(size_t)p * nvec + tx], nreal, f);
#pragma unroll
        for (int e = 0; e < N; ++e) {
          const float d = f[e] - k[e];
          s1[e] += d;
          s2[e] += d * d;
        }
        cnt += 1.f;
      }
    }
  }
  Stat st[N];
#pragma unroll
  for (int e = 0; e < N; ++e) st[e] = gn_from_sums(cnt, k[e], s1[e], s2[e]);

  // merge the block's TY pixel rows, column by column, in a fixed tree
  for (int h = TY >> 1; h > 0; h >>= 1) {
    if (ty >= h && ty < 2 * h) {
#pragma unroll
      for (int e = 0; e < N; ++e) {
        sm_mean[e * GN_THREADS + t] = st[e].mean;
        sm_m2[e * GN_THREADS + t] = st[e].m2;
      }
      sm_n[t] = st[0].n;
    }
    __syncthreads();
    if (ty < h) {
      const int o = t + (h << txs);                        // (tx, ty + h): < GN_THREADS as ty + h < 2h <= TY
      const float on = sm_n[o];
#pragma unroll
      for (int e = 0; e < N; ++e)
        st[e] = gn_merge(st[e], Stat{on, sm_mean[e * GN_THREADS + o], sm_m2[e * GN_THREADS + o]});
    }
  }
  __syncthreads();                                         // the last round's reads, before the slots are reused
  if (ty == 0) {
#pragma unroll
    for (int e = 0; e < N; ++e) {                          // tx * N + e < TX * N <= GN_MAX_NVEC * N <= N * GN_THREADS
      sm_mean[tx * N + e] = st[e].mean;
      sm_m2[tx * N + e] = st[e].m2;
    }
  }
  __syncthreads();
  const float npix = (float)(p1 - p0);                     // every real channel saw each pixel of the slab once

  if constexpr (!FUSED) {
    for (int g = t; g < G; g += GN_THREADS) {
      Stat a{0.f, 0.f, 0.f};
      for (int c = g * Cg; c < (g + 1) * Cg; ++c) a = gn_merge(a, Stat{npix, sm_mean[c], sm_m2[c]});
      float* w = ws + ((size_t)(b * S + blockIdx.x) * G + g) * 3;
      w[0] = a.n, w[1] = a.mean, w[2] = a.m2;
    }
  } else {
    __shared__ float g_mu[N * GN_MAX_NVEC];
    __shared__ float g_rs[N * GN_MAX_NVEC];
    for (int g = t; g < G; g += GN_THREADS) {              // G <= C <= N * nvec <= N * GN_MAX_NVEC
      Stat a{0.f, 0.f, 0.f};
      for (int c = g * Cg; c < (g + 1) * Cg; ++c) a = gn_merge(a, Stat{npix, sm_mean[c], sm_m2[c]});
      g_mu[g] = a.mean;
      g_rs[g] = 1.f / sqrtf(a.m2 / a.n + eps);
    }
    __syncthreads();
    if (!col) return;
    float mu[N], sc[N], sh[N];
    V::load_affine(gamma, tx, sc);                         // tx < nvec: inside the Cs floats of gamma / beta
    V::load_affine(beta, tx, sh);
#pragma unroll
    for (int e = 0; e < N; ++e) {
      const int g = e < nreal ? (tx * N + e) / Cg : 0;
      mu[e] = g_mu[g];
      sc[e] *= g_rs[g];
    }
    raw* yb = (raw*)y + (size_t)b * P * nvec;
#pragma unroll
    for (int r = 0; r < GN_FUSED_ROWS; ++r) {
      const int p = ty + r * TY;
      if (p < P) {
        float f[N];
        V::unpack(v[r], nreal, f);
#pragma unroll
        for (int e = 0; e < N; ++e) f[e] = e < nreal ? actx<GEN>((f[e] - mu[e]) * sc[e] + sh[e], act, alpha) : 0.f;
        yb[(size_t)p * nvec + tx] = V::pack(f);
      }
    }
  }
}

// (mu, rstd) of every (image, group) from its S slab triples, merged in slab order.  fin [B * G][2].
__global__ __launch_bounds__(GN_SC_THREADS) void gn_finalize_kernel(const float* __restrict__ ws,
                                                                     float* __restrict__ fin, int S, int G, int BG,
                                                                     float eps) {
  const int i = blockIdx.x * GN_SC_THREADS + threadIdx.x;
  if (i >= BG) return;
  const int b = i / G, g = i - b * G;
  Stat a{0.f, 0.f, 0.f};
  for (int s = 0; s < S; ++s) {
    const float* w = ws + ((size_t)(b * S + s) * G + g) * 3;
    a = gn_merge(a, Stat{w[0], w[1], w[2]});
  }
  fin[2 * (size_t)i] = a.mean;
  fin[2 * (size_t)i + 1] = 1.f / sqrtf(a.m2 / a.n + eps);
}

// y from the finalised (mu, rstd).  grid (blocks of TY * GN_APPLY_ROWS pixels, B), block TX x TY.
template <typename T, bool GEN>
__global__ __launch_bounds__(GN_THREADS) void gn_vec_apply_kernel(const T* __restrict__ x,
                                                                  const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta,
                                                                  const float* __restrict__ fin, T* __restrict__ y,
                                                                  int P, int nvec, int C, int G, int txs, int act,
                                                                  float alpha) {
  using V = GnVec<T>;
  using raw = typename V::raw;
  constexpr int N = V::N;
  const int t = threadIdx.x;
  const int TX = 1 << txs, TY = GN_THREADS >> txs;
  const int tx = t & (TX - 1), ty = t >> txs;
  if (tx >= nvec) return;
  const int b = blockIdx.y;
  const int p0 = blockIdx.x * (TY * GN_APPLY_ROWS);
  const int p1 = min(P, p0 + TY * GN_APPLY_ROWS);
  const int nreal = min(max(C - tx * N, 0), N);
  const int Cg = C / G;
  float mu[N], sc[N], sh[N];
  V::load_affine(gamma, tx, sc);
  V::load_affine(beta, tx, sh);
#pragma unroll
  for (int e = 0; e < N; ++e) {
    const int g = e < nreal ? (tx * N + e) / Cg : 0;
    mu[e] = fin[2 * (size_t)(b * G + g)];
    sc[e] *= fin[2 * (size_t)(b * G + g) + 1];
  }
  const raw* xb = (const raw*)x + (size_t)b * P * nvec;
  raw* yb = (raw*)y + (size_t)b * P * nvec;
#pragma unroll 4
  for (int p = p0 + ty; p < p1; p += TY) {
    float f[N];
    V::unpack(xb[(size_t)p * nvec + tx], nreal, f);
#pragma unroll
    for (int e = 0; e < N; ++e) f[e] = e < nreal ? actx<GEN>((f[e] - mu[e]) * sc[e] + sh[e], act, alpha) : 0.f;
    yb[(size_t)p * nvec + tx] = V::pack(f);
  }
}

__device__ __forceinline__ float gn_ld(const float* p) { return *p; }
__device__ __forceinline__ float gn_ld(const bf16* p) { return bf2f(*p); }
__device__ __forceinline__ void gn_st(float* p, float v) { *p = v; }
__device__ __forceinline__ void gn_st(bf16* p, float v) { *p = f2bf(v); }

// Scalar statistics: grid (slabs, G, B); the block sweeps pixels [p0, p1) x the group's Cg channels.
template <typename T>
__global__ __launch_bounds__(GN_SC_THREADS) void gn_scalar_stats_kernel(const T* __restrict__ x,
                                                                        float* __restrict__ ws, int P, int Cs, int C,
                                                                        int G, int PS) {
  __shared__ float sm_n[GN_SC_THREADS], sm_mean[GN_SC_THREADS], sm_m2[GN_SC_THREADS];
  const int t = threadIdx.x;
  const int s = blockIdx.x, g = blockIdx.y, b = blockIdx.z, S = gridDim.x;
  const int Cg = C / G;
  const int p0 = s * PS, p1 = min(P, p0 + PS);
  const int tot = max(p1 - p0, 0) * Cg;                    // <= P * C < 2^31
  const T* xb = x + (size_t)b * P * Cs + (size_t)g * Cg;
  float k = 0.f, s1 = 0.f, s2 = 0.f, cnt = 0.f;
  if (t < tot) k = gn_ld(xb + (size_t)(p0 + t / Cg) * Cs + t % Cg);
  for (int i = t; i < tot; i += GN_SC_THREADS) {
    const int q = i / Cg;
    const float d = gn_ld(xb + (size_t)(p0 + q) * Cs + (i - q * Cg)) - k;
    s1 += d;
    s2 += d * d;
    cnt += 1.f;
  }
  Stat a = gn_from_sums(cnt, k, s1, s2);
  for (int h = GN_SC_THREADS >> 1; h > 0; h >>= 1) {
    if (t >= h && t < 2 * h) sm_n[t] = a.n, sm_mean[t] = a.mean, sm_m2[t] = a.m2;
    __syncthreads();
    if (t < h) a = gn_merge(a, Stat{sm_n[t + h], sm_mean[t + h], sm_m2[t + h]});
  }
  if (t == 0) {
    float* w = ws + ((size_t)(b * S + s) * G + g) * 3;
    w[0] = a.n, w[1] = a.mean, w[2] = a.m2;
  }
}

// Scalar apply: one element per thread over [B * P][Cs]; channels >= C are written as zeros and never read.
template <typename T, bool GEN>
__global__ __launch_bounds__(GN_SC_THREADS) void gn_scalar_apply_kernel(const T* __restrict__ x,
                                                                        const float* __restrict__ gamma,
                                                                        const float* __restrict__ beta,
                                                                        const float* __restrict__ fin,
                                                                        T* __restrict__ y, int total, int P, int Cs,
                                                                        int C, int G, int act, float alpha) {
  const unsigned i = blockIdx.x * (unsigned)GN_SC_THREADS + threadIdx.x;
  if (i >= (unsigned)total) return;
  const int row = i / Cs, c = i - row * Cs;
  if (c >= C) {
    gn_st(y + i, 0.f);
    return;
  }
  const size_t bg = (size_t)((row / P) * G + c / (C / G));
  gn_st(y + i, actx<GEN>((gn_ld(x + i) - fin[2 * bg]) * (fin[2 * bg + 1] * gamma[c]) + beta[c], act, alpha));
}

struct GnPlan {
  int path;      // 0 scalar, 1 vector split, 2 vector single launch; -1 refused
  int nvec;      // 16-byte vectors per pixel (vector paths)
  int txs;       // log2 TX
  int S;         // slabs per image
  int PS;        // pixels per slab
  size_t ws;     // workspace floats
};

GnPlan gn_plan(int B, int P, int C, int Cs, int G, bool bf) {
  GnPlan pl{-1, 0, 0, 0, 0, 0};
  if (B < 1 || P < 1 || C < 1 || G < 1 || C % G || Cs < C || (bf && Cs % 8)) return pl;
  if ((double)B * P * Cs >= 2147483648.0 || B > 65535 || G > 65535) return pl;
  const int N = bf ? 8 : 4;
  const int Cg = C / G;
  if (Cs % N == 0 && Cs / N <= GN_MAX_NVEC) {
    pl.nvec = Cs / N;
    while ((1 << pl.txs) < pl.nvec) ++pl.txs;
    const int TY = GN_THREADS >> pl.txs;
    const int rows = (P + TY - 1) / TY;
    if (rows <= GN_FUSED_ROWS) {
      pl.path = 2, pl.S = 1, pl.PS = P;
      return pl;
    }
    pl.path = 1;
    int S = std::min({GN_MAX_SLABS, (rows + GN_FUSED_ROWS - 1) / GN_FUSED_ROWS, std::max(1, 1024 / B)});
    pl.PS = ((P + S - 1) / S + TY - 1) / TY * TY;
    pl.S = (P + pl.PS - 1) / pl.PS;
  } else {
    pl.path = 0;
    const long per = (long)P * Cg;
    int S = (int)std::min<long>({(long)GN_MAX_SLABS, (per + 16 * GN_SC_THREADS - 1) / (16 * GN_SC_THREADS), (long)P});
    S = std::max(S, 1);
    pl.PS = (P + S - 1) / S;
    pl.S = (P + pl.PS - 1) / pl.PS;
  }
  pl.ws = (size_t)B * pl.S * G * 3 + (size_t)B * G * 2;
  return pl;
}

inline bool gn_aligned16(const void* a, const void* b, const void* c, const void* d) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

template <typename T>
hipError_t gn_launch(const T* x, const float* gamma, const float* beta, T* y, float* ws, size_t ws_floats, int B,
                     int P, int C, int Cs, int G, float eps, int act, float alpha, hipStream_t s) {
  constexpr bool bf = sizeof(T) == 2;
  const GnPlan pl = gn_plan(B, P, C, Cs, G, bf);
  if (pl.path < 0 || !x || !y || !gamma || !beta) return hipErrorInvalidValue;
  if (pl.ws && (!ws || ws_floats < pl.ws)) return hipErrorInvalidValue;
  // the vector kernels load x / y / gamma / beta as 16-byte vectors
  if (pl.path && !gn_aligned16(x, y, gamma, beta)) return hipErrorInvalidValue;
  const bool gen = act > ACT_RELU6;
  float* fin = ws ? ws + (size_t)B * pl.S * G * 3 : nullptr;
  if (pl.path == 2) {
    if (gen)
      hipLaunchKernelGGL((gn_vec_kernel<T, true, true>), dim3(1, B), dim3(GN_THREADS), 0, s, x, gamma, beta, y,
                         (float*)nullptr, P, pl.nvec, C, G, P, pl.txs, eps, act, alpha);
    else
      hipLaunchKernelGGL((gn_vec_kernel<T, true, false>), dim3(1, B), dim3(GN_THREADS), 0, s, x, gamma, beta, y,
                         (float*)nullptr, P, pl.nvec, C, G, P, pl.txs, eps, act, alpha);
    return hipGetLastError();
  }
  if (pl.path == 1)
    hipLaunchKernelGGL((gn_vec_kernel<T, false, false>), dim3(pl.S, B), dim3(GN_THREADS), 0, s, x, gamma, beta, y, ws,
                       P, pl.nvec, C, G, pl.PS, pl.txs, eps, act, alpha);
  else
    hipLaunchKernelGGL(gn_scalar_stats_kernel<T>, dim3(pl.S, G, B), dim3(GN_SC_THREADS), 0, s, x, ws, P, Cs, C, G,
                       pl.PS);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(gn_finalize_kernel, dim3((B * G + GN_SC_THREADS - 1) / GN_SC_THREADS), dim3(GN_SC_THREADS), 0, s,
                     ws, fin, pl.S, G, B * G, eps);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (pl.path == 1) {
    const int per = (GN_THREADS >> pl.txs) * GN_APPLY_ROWS;
    const dim3 grid((P + per - 1) / per, B);
    if (gen)
      hipLaunchKernelGGL((gn_vec_apply_kernel<T, true>), grid, dim3(GN_THREADS), 0, s, x, gamma, beta, fin, y, P,
                         pl.nvec, C, G, pl.txs, act, alpha);
    else
      hipLaunchKernelGGL((gn_vec_apply_kernel<T, false>), grid, dim3(GN_THREADS), 0, s, x, gamma, beta, fin, y, P,
                         pl.nvec, C, G, pl.txs, act, alpha);
  } else {
    const int total = B * P * Cs;
    const dim3 grid((total + GN_SC_THREADS - 1) / GN_SC_THREADS);
    if (gen)
      hipLaunchKernelGGL((gn_scalar_apply_kernel<T, true>), grid, dim3(GN_SC_THREADS), 0, s, x, gamma, beta, fin, y,
                         total, P, Cs, C, G, act, alpha);
    else
      hipLaunchKernelGGL((gn_scalar_apply_kernel<T, false>), grid, dim3(GN_SC_THREADS), 0, s, x, gamma, beta, fin, y,
                         total, P, Cs, C, G, act, alpha);
  }
  return hipGetLastError();
}

}  // namespace

// The path a shape takes: 0 scalar (three launches), 1 vector split (three launches), 2 vector single launch;
// -1: refused.  Cs is the stored channel count (C in fp32, C padded to 8 in bf16).
int groupnorm_path(int B, int P, int C, int Cs, int G, bool bf16_act) { return gn_plan(B, P, C, Cs, G, bf16_act).path; }

// Slabs per image of the statistics launch (1 for the single launch)
int groupnorm_slabs(int B, int P, int C, int Cs, int G, bool bf16_act) { return gn_plan(B, P, C, Cs, G, bf16_act).S; }

// Floats of workspace the launch needs (0 for the single launch)
size_t groupnorm_workspace_floats(int B, int P, int C, int Cs, int G, bool bf16_act) {
  return gn_plan(B, P, C, Cs, G, bf16_act).ws;
}

hipError_t groupnorm_f32(const float* x, const float* gamma, const float* beta, float* y, float* ws, size_t ws_floats,
                         int B, int P, int C, int G, float eps, int act, float alpha, hipStream_t s) {
  return gn_launch<float>(x, gamma, beta, y, ws, ws_floats, B, P, C, C, G, eps, act, alpha, s);
}

// gamma / beta: Cp floats (the vector kernels load whole vectors of them; their padding values are not used)
hipError_t groupnorm(const bf16* x, const float* gamma, const float* beta, bf16* y, float* ws, size_t ws_floats, int B,
                     int P, int Cp, int C, int G, float eps, int act, float alpha, hipStream_t s) {
  return gn_launch<bf16>(x, gamma, beta, y, ws, ws_floats, B, P, C, Cp, G, eps, act, alpha, s);
}

}  // namespace adapt
