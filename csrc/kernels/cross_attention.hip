// Attention core with separate query, key and value sources, softmax(Q K^T) V per (image, head), fp32 and bf16
// activations, gfx950.  What attention.hip does for one [Q | K | V] buffer with one token count, for three row
// pointers and two token counts: an encoder whose keys and values come from different tensors, a decoder whose
// queries attend to another tensor's tokens.
//
// q is [B * Tq][ldq], k [B * Tk][ldk], v [B * Tk][ldv]; each pointer is already offset to the first column of
// its part by the host (they may be column slices of one buffer), head h's columns are at h * d (Q, K) and h * dv
// (V), and the 1/sqrt(d) scale is already in Q (runtime/plan.py folds it into the projection).  out is
// [B * Tq][ld_out] with heads x dv true channels; channels heads * dv .. ld_out - 1 are layout padding and are
// written as zeros.  Columns of q / k / v outside the heads are never read.
//
// MFMA path (d and dv multiples of 16 up to 128, any Tq, Tk >= 1), the scheme of attention_core.h in a copy of its
// own (on the core's template this kernel measured up to 0.9 % slower, BASELINE.md "Round 16"): a block of 4
// waves owns XA_QT = 64 queries of one (image, head), each wave's 16 queries' Q in registers; the keys are walked
// XA_KT = 32 at a time up to Tk, K / V rows through padded LDS rows and fetched into registers one tile ahead;
// the score product is taken swapped on v_mfma_f32_16x16x4_f32 (S^T = K Q^T), so a lane's four scores are the B
// operand of the O^T = V^T P^T product and P never leaves the registers; the online softmax (running maximum,
// running sum, exact expf) lives in the lane that uses it.  bf16 is widened while staged, all math is fp32, the
// output is rounded once.
//
// Tails.  K / V rows at or beyond Tk are staged as zeros by predicated loads and their scores are set to -inf
// (0 x NaN from a poisoned row would be NaN); the image bases use Tq for Q / out and Tk for K / V, so a tile never
// reaches into a neighbouring image.  Queries >= Tq load zeros, are carried through the arithmetic and are not
// stored.  The key loop's trip count depends on Tk alone and both barriers of an iteration come before the
// `active` test, so a wave whose 16 queries are all >= Tq (three of the four at Tq = 1) still reaches every
// barrier: it only helps staging, and leaves after the loop.
//
// Every other head size, a pointer that is not aligned to 4 elements and a stride that is not a multiple of 4
// take the plain kernel: one wave per (image, head, query), lanes over the keys, two passes, every access
// bounds-checked.
//
// Index math is 32-bit; the launcher refuses, per tensor, sizes whose element offsets would not fit.
#include "kernels.h"

namespace adapt {
namespace {

constexpr int XA_QT = 64;     // queries per block (4 waves x 16)
constexpr int XA_KT = 32;     // keys per LDS tile
constexpr int XA_PAD = 4;     // floats of padding per LDS row

__device__ __forceinline__ f32x4 xa_ld4(const float* p) { return *(const f32x4*)p; }
__device__ __forceinline__ f32x4 xa_ld4(const bf16* p) {
  union { uint2 u; bf16 e[4]; } t;
  t.u = *(const uint2*)p;
  return f32x4{bf2f(t.e[0]), bf2f(t.e[1]), bf2f(t.e[2]), bf2f(t.e[3])};
}
__device__ __forceinline__ void xa_st4(float* p, f32x4 v) { *(f32x4*)p = v; }
__device__ __forceinline__ void xa_st4(bf16* p, f32x4 v) {
  union { uint2 u; bf16 e[4]; } t;
  t.e[0] = f2bf(v.x); t.e[1] = f2bf(v.y); t.e[2] = f2bf(v.z); t.e[3] = f2bf(v.w);
  *(uint2*)p = t.u;
}
__device__ __forceinline__ float xa_ld(const float* p) { return *p; }
__device__ __forceinline__ float xa_ld(const bf16* p) { return bf2f(*p); }
__device__ __forceinline__ void xa_st(float* p, float v) { *p = v; }
__device__ __forceinline__ void xa_st(bf16* p, float v) { *p = f2bf(v); }

// DMAX: the head sizes this instantiation holds in registers (d, dv <= DMAX, both multiples of 16)
template <typename T, int DMAX>
__global__ __launch_bounds__(256) void cross_attention_mfma_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                                   const T* __restrict__ v, T* __restrict__ out,
                                                                   int Tq, int Tk, int heads, int d, int dv, int ldq,
                                                                   int ldk, int ldv, int ld_out, int qtiles) {
  constexpr int ND = DMAX / 16;                       // 16-wide slices of d / dv
  constexpr int NST = XA_KT * DMAX / 512;             // staged 4-element vectors per thread (K and V together)
  __shared__ __attribute__((aligned(16))) float smem[2 * XA_KT * (DMAX + XA_PAD)];
  float* sk = smem;
  float* sv = smem + XA_KT * (DMAX + XA_PAD);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  int bid = blockIdx.x;
  const int qt = bid % qtiles;
  bid /= qtiles;
  const int h = bid % heads, img = bid / heads;
  const int lk = d + XA_PAD, lv = dv + XA_PAD;        // LDS row lengths
  const T* qbase = q + img * Tq * ldq + h * d;        // this (image, head)'s rows: Tq of Q, Tk of K and V
  const T* kbase = k + img * Tk * ldk + h * d;
  const T* vbase = v + img * Tk * ldv + h * dv;

  // what this thread stages of every key tile: vector `idx` of the tile's K rows, then of its V rows
  const int nkv = d >> 2, nvv = dv >> 2;
  int srow[NST], sgcol[NST], sloff[NST];
  bool sval[NST], sisv[NST];
#pragma unroll
  for (int j = 0; j < NST; ++j) {
    int idx = tid + j * 256;
    sval[j] = idx < XA_KT * (nkv + nvv);
    sisv[j] = false;
    srow[j] = sgcol[j] = sloff[j] = 0;
    if (idx < XA_KT * nkv) {
      srow[j] = idx / nkv;
      const int vi = idx - srow[j] * nkv;
      sgcol[j] = 4 * vi;
      sloff[j] = srow[j] * lk + 4 * vi;
    } else if (sval[j]) {
      idx -= XA_KT * nkv;
      sisv[j] = true;
      srow[j] = idx / nvv;
      const int vi = idx - srow[j] * nvv;
      sgcol[j] = 4 * vi;
      sloff[j] = XA_KT * (DMAX + XA_PAD) + srow[j] * lv + 4 * vi;
    }
  }

  const int q0 = qt * XA_QT + wave * 16;
  const bool active = q0 < Tq;                        // wave-uniform
  const int qrow = q0 + c;
  f32x4 qf[ND];
#pragma unroll
  for (int t = 0; t < ND; ++t) {
    qf[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (qrow < Tq && 16 * t < d) qf[t] = xa_ld4(qbase + qrow * ldq + 16 * t + 4 * g);
  }
  f32x4 o[ND];
#pragma unroll
  for (int n = 0; n < ND; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;                       // l: this lane's keys only, summed over the groups at the end

  f32x4 st[NST];
#pragma unroll
  for (int j = 0; j < NST; ++j) {
    st[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (sval[j] && srow[j] < Tk)
      st[j] = sisv[j] ? xa_ld4(vbase + srow[j] * ldv + sgcol[j]) : xa_ld4(kbase + srow[j] * ldk + sgcol[j]);
  }
  for (int k0 = 0; k0 < Tk; k0 += XA_KT) {            // the same trip count for every wave of the block
    __syncthreads();                                  // the previous tile has been read
#pragma unroll
    for (int j = 0; j < NST; ++j)
      if (sval[j]) *(f32x4*)(smem + sloff[j]) = st[j];
    __syncthreads();
    if (k0 + XA_KT < Tk) {
#pragma unroll
      for (int j = 0; j < NST; ++j) {
        st[j] = f32x4{0.f, 0.f, 0.f, 0.f};            // rows >= Tk are zeros, never loaded
        const int r = k0 + XA_KT + srow[j];
        if (sval[j] && r < Tk) st[j] = sisv[j] ? xa_ld4(vbase + r * ldv + sgcol[j]) : xa_ld4(kbase + r * ldk + sgcol[j]);
      }
    }
    if (!active) continue;                            // after both barriers: the wave only helps staging
    // S^T = K Q^T: s[u][i] = score(key k0 + 16 u + 4 g + i, query c)
    f32x4 s[XA_KT / 16];
#pragma unroll
    for (int u = 0; u < XA_KT / 16; ++u) {
      s[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < ND; ++t) {
        if (16 * t < d) {
          const f32x4 kf = *(const f32x4*)(sk + (16 * u + c) * lk + 16 * t + 4 * g);
          s[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.x, qf[t].x, s[u], 0, 0, 0);
          s[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.y, qf[t].y, s[u], 0, 0, 0);
          s[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.z, qf[t].z, s[u], 0, 0, 0);
          s[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf.w, qf[t].w, s[u], 0, 0, 0);
        }
      }
    }
    float mx = -INFINITY;
#pragma unroll
    for (int u = 0; u < XA_KT / 16; ++u)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (k0 + 16 * u + 4 * g + i >= Tk) s[u][i] = -INFINITY;
        mx = fmaxf(mx, s[u][i]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));               // finite: key k0 < Tk is in every tile
    const float mn = fmaxf(m, mx);
    const float alpha = expf(m - mn);                 // 0 on the first tile (m = -inf)
    m = mn;
    float ps = 0.f;
#pragma unroll
    for (int u = 0; u < XA_KT / 16; ++u)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        s[u][i] = expf(s[u][i] - mn);                 // masked keys: exp(-inf) = 0
        ps += s[u][i];
      }
    l = l * alpha + ps;
#pragma unroll
    for (int n = 0; n < ND; ++n) o[n] *= alpha;
    // O^T += V^T P^T: o[n][j] = O(query c, channel 16 n + 4 g + j)
#pragma unroll
    for (int u = 0; u < XA_KT / 16; ++u)
#pragma unroll
      for (int n = 0; n < ND; ++n) {
        if (16 * n < dv) {
          const float* vp = sv + (16 * u + 4 * g) * lv + 16 * n + c;
          o[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[0], s[u].x, o[n], 0, 0, 0);
          o[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[lv], s[u].y, o[n], 0, 0, 0);
          o[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[2 * lv], s[u].z, o[n], 0, 0, 0);
          o[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(vp[3 * lv], s[u].w, o[n], 0, 0, 0);
        }
      }
  }
  if (!active) return;                                // no barrier follows
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (qrow >= Tq) return;
  const float inv = 1.f / l;
  T* orow = out + (img * Tq + qrow) * ld_out;
#pragma unroll
  for (int n = 0; n < ND; ++n)
    if (16 * n < dv) xa_st4(orow + h * dv + 16 * n + 4 * g, o[n] * inv);
  if (h == heads - 1)                                 // layout padding of the row: zeros
    for (int cc = heads * dv + g; cc < ld_out; cc += 4) xa_st(orow + cc, 0.f);
}

__device__ __forceinline__ float xa_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float xa_wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <typename T>
__device__ __forceinline__ float xa_dot(const T* __restrict__ a, const T* __restrict__ b, int n) {
  float s = 0.f;
  for (int i = 0; i < n; ++i) s += xa_ld(a + i) * xa_ld(b + i);
  return s;
}

// Any d, dv, stride and alignment: one wave per (image, head, query).
template <typename T>
__global__ __launch_bounds__(256) void cross_attention_plain_kernel(const T* __restrict__ q, const T* __restrict__ k,
                                                                    const T* __restrict__ v, T* __restrict__ out,
                                                                    int rows, int Tq, int Tk, int heads, int d, int dv,
                                                                    int ldq, int ldk, int ldv, int ld_out) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= rows) return;                              // the whole wave leaves together; the kernel has no barrier
  const int qi = w % Tq, r = w / Tq;
  const int h = r % heads, img = r / heads;
  const T* qp = q + (img * Tq + qi) * ldq + h * d;
  const T* kp = k + img * Tk * ldk + h * d;
  const T* vp = v + img * Tk * ldv + h * dv;
  float mx = -INFINITY;
  for (int kk = lane; kk < Tk; kk += 64) mx = fmaxf(mx, xa_dot(qp, kp + kk * ldk, d));
  mx = xa_wave_max(mx);
  T* orow = out + (img * Tq + qi) * ld_out;
  for (int c0 = 0; c0 < dv; c0 += 64) {               // 64 output channels at a time, one per lane
    const int cc = c0 + lane;
    float acc = 0.f, ls = 0.f;
    for (int kb = 0; kb < Tk; kb += 64) {
      const int kk = kb + lane;
      const float p = kk < Tk ? expf(xa_dot(qp, kp + kk * ldk, d) - mx) : 0.f;
      ls += p;
      const int nk = min(64, Tk - kb);
      for (int j = 0; j < nk; ++j) {
        const float pk = __shfl(p, j);
        if (cc < dv) acc += pk * xa_ld(vp + (kb + j) * ldv + cc);
      }
    }
    const float l = xa_wave_sum(ls);
    if (cc < dv) xa_st(orow + h * dv + cc, acc / l);
  }
  if (h == heads - 1)
    for (int cc = heads * dv + lane; cc < ld_out; cc += 64) xa_st(orow + cc, 0.f);
}

template <typename T>
hipError_t cross_attention_launch(const T* q, const T* k, const T* v, T* out, int B, int Tq, int Tk, int heads, int d,
                                  int dv, int ldq, int ldk, int ldv, int ld_out, hipStream_t s) {
  if (B < 1 || Tq < 1 || Tk < 1 || heads < 1 || d < 1 || dv < 1 || !q || !k || !v || !out) return hipErrorInvalidValue;
  const long long lim = 0x7fffffffll;
  if ((long long)heads * d > ldq || (long long)heads * d > ldk || (long long)heads * dv > ldv ||
      (long long)heads * dv > ld_out)
    return hipErrorInvalidValue;
  // 32-bit element offsets and grid sizes: refuse, per tensor, what does not fit
  if ((long long)B * Tq * ldq > lim || (long long)B * Tk * ldk > lim || (long long)B * Tk * ldv > lim ||
      (long long)B * Tq * ld_out > lim || (long long)B * heads * Tq > lim)
    return hipErrorInvalidValue;
  if (cross_attention_path((uintptr_t)q, (uintptr_t)k, (uintptr_t)v, (uintptr_t)out, d, dv, ldq, ldk, ldv, ld_out,
                           (int)sizeof(T))) {
    const int qtiles = (Tq + XA_QT - 1) / XA_QT;
    const dim3 grid(B * heads * qtiles), block(256);
    const int dm = d > dv ? d : dv;
    if (dm <= 32)
      hipLaunchKernelGGL((cross_attention_mfma_kernel<T, 32>), grid, block, 0, s, q, k, v, out, Tq, Tk, heads, d, dv,
                         ldq, ldk, ldv, ld_out, qtiles);
    else if (dm <= 64)
      hipLaunchKernelGGL((cross_attention_mfma_kernel<T, 64>), grid, block, 0, s, q, k, v, out, Tq, Tk, heads, d, dv,
                         ldq, ldk, ldv, ld_out, qtiles);
    else
      hipLaunchKernelGGL((cross_attention_mfma_kernel<T, 128>), grid, block, 0, s, q, k, v, out, Tq, Tk, heads, d, dv,
                         ldq, ldk, ldv, ld_out, qtiles);
  } else {
    const int rows = B * heads * Tq;
    hipLaunchKernelGGL(cross_attention_plain_kernel<T>, dim3((rows + 3) / 4), dim3(256), 0, s, q, k, v, out, rows, Tq,
                       Tk, heads, d, dv, ldq, ldk, ldv, ld_out);
  }
  return hipGetLastError();
}

}  // namespace

int cross_attention_query_tile() { return XA_QT; }
int cross_attention_key_tile() { return XA_KT; }

// 1: the MFMA path, 0: the plain kernel.  The MFMA kernel moves 4 elements at a time: head sizes that are
// multiples of 16 up to 128, the four addresses aligned to 4 elements of `elem_size` bytes, strides multiples of 4.
int cross_attention_path(uintptr_t q, uintptr_t k, uintptr_t v, uintptr_t out, int d, int dv, int ldq, int ldk, int ldv,
                         int ld_out, int elem_size) {
  const uintptr_t align = (uintptr_t)elem_size * 4 - 1;
  const bool vec = ldq % 4 == 0 && ldk % 4 == 0 && ldv % 4 == 0 && ld_out % 4 == 0 && ((q | k | v | out) & align) == 0;
  return attention_path(d, dv) && vec;
}

hipError_t attention_qkv_f32(const float* q, const float* k, const float* v, float* out, int B, int Tq, int Tk,
                             int heads, int d, int dv, int ldq, int ldk, int ldv, int ld_out, hipStream_t s) {
  return cross_attention_launch<float>(q, k, v, out, B, Tq, Tk, heads, d, dv, ldq, ldk, ldv, ld_out, s);
}

hipError_t attention_qkv_bf16(const bf16* q, const bf16* k, const bf16* v, bf16* out, int B, int Tq, int Tk, int heads,
                              int d, int dv, int ldq, int ldk, int ldv, int ld_out, hipStream_t s) {
  return cross_attention_launch<bf16>(q, k, v, out, B, Tq, Tk, heads, d, dv, ldq, ldk, ldv, ld_out, s);
}

}  // namespace adapt
