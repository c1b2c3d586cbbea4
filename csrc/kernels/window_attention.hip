// Swin window attention core: softmax(Q K^T + B) V inside M x M windows of an (H, W) map, with the cyclic shift
// of the window grid and its mask, fp32 and bf16 activations, gfx950.
//
// qkv is the NHWC map [B * H * W][ld_in], one row per position holding [Q | K | V], head-major inside each part
// (heads x d each); the 1/sqrt(d) scale is already in Q (runtime/plan.py folds it into the projection).  out is
// [B * H * W][ld_out] with heads x d true channels; channels heads * d .. ld_out - 1 are layout padding and are
// written as zeros.  Padding channels of qkv are never read.
//
// Nothing is rolled or partitioned in memory.  Token t = (i, j) of window (wy, wx), counted in the frame rolled
// by (-s, -s), lives at the map row ((wy M + i + s) mod H) W + (wx M + j + s) mod W, and its context goes to the
// same row of out: the roll, the partition, the reverse and the roll back are this one address.  It is computed
// once per staged K / V vector of a key tile and once per query.
//
// bias is host-packed (ops/attention.py `window_bias`): [classes][heads][Tp][Tp] fp32, Tp = M^2 rounded up to the
// key tile, bias[c][h][q][k] = table[index(q, k)][h] + mask_c(q, k), zeros in the padding.  The shift mask only
// depends on whether the window is in the last window row and / or the last window column, so it is baked in as
// four classes, class = 2 (wy last) + (wx last); an unshifted layer has one.  The kernel adds one table and
// computes no regions.  A lane reads the four keys of its query as one 16-byte load, and the score accumulator
// starts from it.
//
// MFMA path (d a multiple of 16 up to 128): the scheme of attention_core.h in a copy of its own (on the core's
// template this kernel measured up to 0.7 % slower, BASELINE.md "Round 16").  A block of 4 waves owns one (image,
// window, head, tile of WA_QT = 64 queries); the keys of the window are walked WA_KT = 32 at a time, K and V staged
// through padded LDS rows and fetched one tile ahead; swapped score product S^T = K Q^T on
// v_mfma_f32_16x16x4_f32, P kept in registers as the B operand of O^T = V^T P^T, online softmax in the lane that
// uses it.  Rows at or beyond M^2 are staged as zeros and their scores set to -inf, queries at or beyond M^2 are
// carried and not stored (and read no bias).  A window of at most 64 tokens would fit in LDS whole; staging
// Swin's 49 tokens as one 64-key tile (no second pass) measured 2 - 11 % slower than this two-tile loop at d = 32
// (BASELINE.md "Round 13"): half of the loads then sit in front of the first MFMA with nothing to hide under.  So
// the two-tile loop serves every size.
//
// Every other head size, and any misaligned buffer, takes the plain kernel: one wave per (image, window, head,
// query), lanes over the keys, two passes, fp32, every access bounds-checked.
//
// Index math is 32-bit; the launchers refuse sizes whose element offsets would not fit.
#include "kernels.h"

namespace adapt {
namespace {

constexpr int WA_QT = 64;     // queries per block (4 waves x 16)
constexpr int WA_KT = 32;     // keys per LDS tile
constexpr int WA_PAD = 4;     // floats of padding per LDS row

__device__ __forceinline__ f32x4 wa_ld4(const float* p) { return *(const f32x4*)p; }
__device__ __forceinline__ f32x4 wa_ld4(const bf16* p) {
  union { uint2 u; bf16 e[4]; } t;
  t.u = *(const uint2*)p;
  return f32x4{bf2f(t.e[0]), bf2f(t.e[1]), bf2f(t.e[2]), bf2f(t.e[3])};
}
__device__ __forceinline__ void wa_st4(float* p, f32x4 v) { *(f32x4*)p = v; }
__device__ __forceinline__ void wa_st4(bf16* p, f32x4 v) {
  union { uint2 u; bf16 e[4]; } t;
  t.e[0] = f2bf(v.x); t.e[1] = f2bf(v.y); t.e[2] = f2bf(v.z); t.e[3] = f2bf(v.w);
  *(uint2*)p = t.u;
}
__device__ __forceinline__ float wa_ld(const float* p) { return *p; }
__device__ __forceinline__ float wa_ld(const bf16* p) { return bf2f(*p); }
__device__ __forceinline__ void wa_st(float* p, float v) { *p = v; }
__device__ __forceinline__ void wa_st(bf16* p, float v) { *p = f2bf(v); }

struct WinGeom {
  int H, W, M, shift;
  int nwx, nwin;     // windows per row of windows, windows per image
  int Tn, Tp;        // tokens per window (M^2), Tn rounded up to WA_KT (the packed bias' row length)
};

// map row (inside its image) of token t < Tn of window (wy, wx): y0 = wy M + shift, x0 = wx M + shift
__device__ __forceinline__ int wa_row(const WinGeom& g, int y0, int x0, int t) {
  const int i = t / g.M, j = t - i * g.M;
  int y = y0 + i, x = x0 + j;                         // below 2 H and 2 W: one wrap at the most
  if (y >= g.H) y -= g.H;
  if (x >= g.W) x -= g.W;
  return y * g.W + x;
}

// mask class of a window: 2 (last window row) + (last window column) under a shift, 0 without
__device__ __forceinline__ int wa_class(const WinGeom& g, int wy, int wx) {
  return g.shift ? 2 * (wy == g.nwin / g.nwx - 1) + (wx == g.nwx - 1) : 0;
}

// DMAX: the head sizes this instantiation holds in registers (d <= DMAX, a multiple of 16)
template <typename T, int DMAX>
__global__ __launch_bounds__(256) void window_attention_mfma_kernel(const T* __restrict__ qkv,
                                                                    const float* __restrict__ bias,
                                                                    T* __restrict__ out, WinGeom g, int heads, int d,
                                                                    int ld_in, int ld_out, int qtiles) {
  constexpr int ND = DMAX / 16;                       // 16-wide slices of d
  constexpr int NST = WA_KT * DMAX / 512;             // staged 4-element vectors per thread (K and V together)
  __shared__ __attribute__((aligned(16))) float smem[2 * WA_KT * (DMAX + WA_PAD)];
  float* sk = smem;
  float* sv = smem + WA_KT * (DMAX + WA_PAD);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, gq = lane >> 4;
  int bid = blockIdx.x;
  const int qt = bid % qtiles;
  bid /= qtiles;
  const int h = bid % heads;
  bid /= heads;
  const int win = bid % g.nwin, img = bid / g.nwin;
  const int wy = win / g.nwx, wx = win - wy * g.nwx;
  const int y0 = wy * g.M + g.shift, x0 = wx * g.M + g.shift;
  const int Tn = g.Tn;
  const int ldk = d + WA_PAD;
  const T* base = qkv + img * (g.H * g.W) * ld_in;    // this image's rows
  const int kcol = heads * d + h * d, vcol = 2 * heads * d + h * d;

  // what this thread stages of every key tile: vector `idx` of the tile's K rows, then of its V rows
  const int nkv = d >> 2;
  int srow[NST], sgcol[NST], sloff[NST];
  bool sval[NST];
#pragma unroll
  for (int j = 0; j < NST; ++j) {
    int idx = tid + j * 256;
    sval[j] = idx < 2 * WA_KT * nkv;
    srow[j] = sgcol[j] = sloff[j] = 0;
    if (idx < WA_KT * nkv) {
      srow[j] = idx / nkv;
      const int v = idx - srow[j] * nkv;
      sgcol[j] = kcol + 4 * v;
      sloff[j] = srow[j] * ldk + 4 * v;
    } else if (sval[j]) {
      idx -= WA_KT * nkv;
      srow[j] = idx / nkv;
      const int v = idx - srow[j] * nkv;
      sgcol[j] = vcol + 4 * v;
      sloff[j] = WA_KT * (DMAX + WA_PAD) + srow[j] * ldk + 4 * v;
    }
  }

  const int q0 = qt * WA_QT + wave * 16;
  const bool active = q0 < Tn;                        // wave-uniform
  const int qtok = q0 + c;
  const bool qok = qtok < Tn;
  const int qrow = qok ? wa_row(g, y0, x0, qtok) : 0; // the query's map row: its Q is read and its context written there
  f32x4 qf[ND];
#pragma unroll
  for (int t = 0; t < ND; ++t) {
    qf[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (qok && 16 * t < d) qf[t] = wa_ld4(base + qrow * ld_in + h * d + 16 * t + 4 * gq);
  }
  // this query's row of the packed bias (never formed for a query >= Tn: such a row may lie beyond Tp)
  const float* brow = bias + ((wa_class(g, wy, wx) * heads + h) * g.Tp + (qok ? qtok : 0)) * g.Tp + 4 * gq;
  f32x4 o[ND];
#pragma unroll
  for (int n = 0; n < ND; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;                       // l: this lane's keys only, summed over the groups at the end

  f32x4 st[NST];
#pragma unroll
  for (int j = 0; j < NST; ++j) {
    st[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (sval[j] && srow[j] < Tn) st[j] = wa_ld4(base + wa_row(g, y0, x0, srow[j]) * ld_in + sgcol[j]);
  }
  for (int k0 = 0; k0 < Tn; k0 += WA_KT) {
    __syncthreads();                                  // the previous tile has been read
#pragma unroll
    for (int j = 0; j < NST; ++j)
      if (sval[j]) *(f32x4*)(smem + sloff[j]) = st[j];
    __syncthreads();
    if (k0 + WA_KT < Tn) {
#pragma unroll
      for (int j = 0; j < NST; ++j) {
        st[j] = f32x4{0.f, 0.f, 0.f, 0.f};            // tokens >= M^2 are zeros, never loaded
        const int r = k0 + WA_KT + srow[j];
        if (sval[j] && r < Tn) st[j] = wa_ld4(base + wa_row(g, y0, x0, r) * ld_in + sgcol[j]);
      }
    }
    if (!active) continue;
    // S^T = K Q^T + B^T: s[u][i] = score(key k0 + 16 u + 4 gq + i, query c), started from the packed bias
    // (k0 + 16 u + 4 gq + 3 < Tp: the tile lies inside the padded row)
    f32x4 s[WA_KT / 16];
#pragma unroll
    for (int u = 0; u < WA_KT / 16; ++u) {
      s[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (qok) s[u] = *(const f32x4*)(brow + k0 + 16 * u);
    }
#pragma unroll
    for (int u = 0; u < WA_KT / 16; ++u) {
#pragma unroll
      for (int t = 0; t < ND; ++t) {
        if (16 * t < d) {
          const f32x4 kf = *(const f32x4*)(sk + (16 * u + c) * ldk + 16 * t + 4 * gq);
          s[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.x, qf[t].x, s[u], 0, 0, 0);
          s[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.y, qf[t].y, s[u], 0, 0, 0);
          s[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.z, qf[t].z, s[u], 0, 0, 0);
          s[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.w, qf[t].w, s[u], 0, 0, 0);
        }
      }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int u = 0; u < WA_KT / 16; ++u)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (k0 + 16 * u + 4 * gq + i >= Tn) s[u][i] = -INFINITY;
        mx = fmaxf(mx, s[u][i]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));               // finite: key k0 < Tn is in every tile, the mask is -100
    const float mn = fmaxf(m, mx);
    const float alpha = expf(m - mn);                 // 0 on the first tile (m = -inf)
    m = mn;
    float ps = 0.f;
#pragma unroll
    for (int u = 0; u < WA_KT / 16; ++u)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        s[u][i] = expf(s[u][i] - mn);                 // tokens >= M^2: exp(-inf) = 0
        ps += s[u][i];
      }
    l = l * alpha + ps;
#pragma unroll
    for (int n = 0; n < ND; ++n) o[n] *= alpha;
    // O^T += V^T P^T: o[n][j] = O(query c, channel 16 n + 4 gq + j)
#pragma unroll
    for (int u = 0; u < WA_KT / 16; ++u)
#pragma unroll
      for (int n = 0; n < ND; ++n) {
        if (16 * n < d) {
          const float* vp = sv + (16 * u + 4 * gq) * ldk + 16 * n + c;
          o[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[0], s[u].x, o[n], 0, 0, 0);
          o[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[ldk], s[u].y, o[n], 0, 0, 0);
          o[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[2 * ldk], s[u].z, o[n], 0, 0, 0);
          o[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[3 * ldk], s[u].w, o[n], 0, 0, 0);
        }
      }
  }
  if (!active) return;
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (!qok) return;
  const float inv = 1.f / l;
  T* orow = out + (img * (g.H * g.W) + qrow) * ld_out;
#pragma unroll
  for (int n = 0; n < ND; ++n)
    if (16 * n < d) wa_st4(orow + h * d + 16 * n + 4 * gq, o[n] * inv);
  if (h == heads - 1)                                 // layout padding of the row: zeros
    for (int cc = heads * d + gq; cc < ld_out; cc += 4) wa_st(orow + cc, 0.f);
}

__device__ __forceinline__ float wa_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float wa_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <typename T>
__device__ __forceinline__ float wa_dot(const T* __restrict__ a, const T* __restrict__ b, int n) {
  float s = 0.f;
  for (int i = 0; i < n; ++i) s += wa_ld(a + i) * wa_ld(b + i);
  return s;
}

// Any d, stride and alignment: one wave per (image, window, head, query).
template <typename T>
__global__ __launch_bounds__(256) void window_attention_plain_kernel(const T* __restrict__ qkv,
                                                                     const float* __restrict__ bias,
                                                                     T* __restrict__ out, WinGeom g, int rows,
                                                                     int heads, int d, int ld_in, int ld_out) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= rows) return;                              // the whole wave leaves together
  const int Tn = g.Tn;
  const int q = w % Tn;
  int r = w / Tn;
  const int h = r % heads;
  r /= heads;
  const int win = r % g.nwin, img = r / g.nwin;
  const int wy = win / g.nwx, wx = win - wy * g.nwx;
  const int y0 = wy * g.M + g.shift, x0 = wx * g.M + g.shift;
  const T* base = qkv + img * (g.H * g.W) * ld_in;
  const int qrow = wa_row(g, y0, x0, q);
  const T* qp = base + qrow * ld_in + h * d;
  const T* kp = base + heads * d + h * d;
  const T* vp = base + 2 * heads * d + h * d;
  const float* brow = bias + ((wa_class(g, wy, wx) * heads + h) * g.Tp + q) * g.Tp;
  float mx = -INFINITY;
  for (int k = lane; k < Tn; k += 64)
    mx = fmaxf(mx, wa_dot(qp, kp + wa_row(g, y0, x0, k) * ld_in, d) + brow[k]);
  mx = wa_wave_max(mx);
  T* orow = out + (img * (g.H * g.W) + qrow) * ld_out;
  for (int c0 = 0; c0 < d; c0 += 64) {                // 64 output channels at a time, one per lane
    const int cc = c0 + lane;
    float acc = 0.f, ls = 0.f;
    for (int kb = 0; kb < Tn; kb += 64) {
      const int k = kb + lane;
      const int krow = k < Tn ? wa_row(g, y0, x0, k) : 0;
      const float p = k < Tn ? expf(wa_dot(qp, kp + krow * ld_in, d) + brow[k] - mx) : 0.f;
      ls += p;
      const int nk = min(64, Tn - kb);
      for (int kk = 0; kk < nk; ++kk) {
        const float pk = __shfl(p, kk);
        const int vr = __shfl(krow, kk);
        if (cc < d) acc += pk * wa_ld(vp + vr * ld_in + cc);
      }
    }
    const float l = wa_wave_sum(ls);
    if (cc < d) wa_st(orow + h * d + cc, acc / l);
  }
  if (h == heads - 1)
    for (int cc = heads * d + lane; cc < ld_out; cc += 64) wa_st(orow + cc, 0.f);
}

template <typename T>
hipError_t window_attention_launch(const T* qkv, const float* bias, T* out, int B, int H, int W, int M, int shift,
                                   int heads, int d, int ld_in, int ld_out, hipStream_t s) {
  if (B < 1 || H < 1 || W < 1 || M < 1 || heads < 1 || d < 1 || shift < 0 || shift >= M || H % M || W % M || !bias)
    return hipErrorInvalidValue;
  const long long lim = 0x7fffffffll;
  if (3ll * heads * d > ld_in || (long long)heads * d > ld_out || (long long)M * M > lim) return hipErrorInvalidValue;
  WinGeom g;
  g.H = H; g.W = W; g.M = M; g.shift = shift;
  g.nwx = W / M; g.nwin = (H / M) * (W / M);
  g.Tn = M * M; g.Tp = (g.Tn + WA_KT - 1) / WA_KT * WA_KT;
  const int qtiles = (g.Tn + WA_QT - 1) / WA_QT;
  // 32-bit element offsets and grid sizes: refuse what does not fit
  if ((long long)B * H * W * ld_in > lim || (long long)B * H * W * ld_out > lim ||
      (long long)B * H * W * heads > lim || (long long)B * g.nwin * heads * qtiles > lim ||
      4ll * heads * g.Tp * g.Tp > lim)
    return hipErrorInvalidValue;
  const uintptr_t align = sizeof(T) * 4 - 1;          // the MFMA kernel moves 4 elements at a time
  const bool vec = ld_in % 4 == 0 && ld_out % 4 == 0 && (((uintptr_t)qkv | (uintptr_t)out) & align) == 0 &&
                   ((uintptr_t)bias & 15) == 0;
  if (window_attention_path(d) && vec) {
    const dim3 grid(B * g.nwin * heads * qtiles), block(256);
    if (d <= 32)
      hipLaunchKernelGGL((window_attention_mfma_kernel<T, 32>), grid, block, 0, s, qkv, bias, out, g, heads, d, ld_in,
                         ld_out, qtiles);
    else if (d <= 64)
      hipLaunchKernelGGL((window_attention_mfma_kernel<T, 64>), grid, block, 0, s, qkv, bias, out, g, heads, d, ld_in,
                         ld_out, qtiles);
    else
      hipLaunchKernelGGL((window_attention_mfma_kernel<T, 128>), grid, block, 0, s, qkv, bias, out, g, heads, d,
                         ld_in, ld_out, qtiles);
  } else {
    const int rows = B * H * W * heads;               // B x windows x heads x M^2 queries
    hipLaunchKernelGGL(window_attention_plain_kernel<T>, dim3((rows + 3) / 4), dim3(256), 0, s, qkv, bias, out, g,
                       rows, heads, d, ld_in, ld_out);
  }
  return hipGetLastError();
}

}  // namespace

int window_attention_query_tile() { return WA_QT; }
int window_attention_key_tile() { return WA_KT; }

// 1: the MFMA path, 0: the plain kernel (which a misaligned buffer or stride takes as well)
int window_attention_path(int d) { return d >= 16 && d <= 128 && d % 16 == 0; }

hipError_t window_attention_f32(const float* qkv, const float* bias, float* out, int B, int H, int W, int M, int shift,
                                int heads, int d, int ld_in, int ld_out, hipStream_t s) {
  return window_attention_launch<float>(qkv, bias, out, B, H, W, M, shift, heads, d, ld_in, ld_out, s);
}

hipError_t window_attention_bf16(const bf16* qkv, const float* bias, bf16* out, int B, int H, int W, int M, int shift,
                                 int heads, int d, int ld_in, int ld_out, hipStream_t s) {
  return window_attention_launch<bf16>(qkv, bias, out, B, H, W, M, shift, heads, d, ld_in, ld_out, s);
}

}  // namespace adapt
