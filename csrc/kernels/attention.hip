// Self-attention core, softmax(Q K^T) V per (image, head), fp32 and bf16 activations, gfx950.
//
// qkv is [B * T][ld_in] with one row per token holding [Q | K | V], head-major inside each part (Q and K:
// heads x d, V: heads x dv); the 1/sqrt(d) scale is already in Q (runtime/plan.py folds it into the projection).
// out is [B * T][ld_out] with heads x dv true channels; channels heads * dv .. ld_out - 1 are layout padding and
// are written as zeros.  Padding channels of qkv are never read.
//
// MFMA path (d and dv multiples of 16 up to 128, any T >= 1): flash-style on v_mfma_f32_16x16x4_f32, all math in
// fp32 whatever the activation type (bf16 is widened while staged and the output is rounded once).
//
//   * A block of 4 waves owns one (image, head, tile of AT_QT = 64 queries); a wave owns 16 of the queries and
//     keeps their Q in registers for the whole kernel.  The block walks the keys AT_KT = 32 at a time: the K and
//     V rows of a key tile are staged once through LDS (rows padded by 4 floats: the 16-byte K reads of 16 lanes
//     and the V reads of the 4 lane groups then spread over the banks), fetched into registers one tile ahead so
//     that the loads of tile t + 1 are in flight under the MFMAs of tile t.
//   * The score product is taken swapped, S^T = K Q^T: M = key, N = query, so a lane of the 16x16 result holds
//     for query `lane & 15` the four keys `4 * (lane >> 4) + i`.  That register i is exactly the B operand of
//     the O^T = V^T P^T product when its k-step i is taken to mean the keys {4g + i} (V rows are read in that
//     permuted order), so P never goes through LDS, and O^T has the query on `lane & 15` as well: the row
//     maximum, the row sum and the rescale factor of the online softmax all live in the lane that needs them.
//     A row reduction is the in-lane registers plus two `__shfl_xor` steps (16, 32) over the four lane groups.
//   * Online softmax: running maximum m and running sum l per query; per key tile alpha = exp(m - m'),
//     p = exp(s - m') with the exact expf, O and l rescaled by alpha.  The T x T scores never touch memory.
//
// Tails.  K / V rows at or beyond T are staged as zeros by predicated loads and their scores are set to -inf (a
// zero probability alone is not enough: 0 x NaN from a poisoned row is NaN); a tile never reads a row >= T, so it
// cannot reach into the next image either.  Queries >= T load zeros, are carried through the arithmetic and are
// not stored; a wave whose 16 queries are all >= T only helps staging.  The k-step order inside a 16-wide slice
// of d is likewise permuted (step (t, j) means dd = 16 t + 4 (lane >> 4) + j), so K and Q are read 16 bytes at a
// time.
//
// Every other head size, and any misaligned buffer, takes the plain kernel: one wave per (image, head, query),
// lanes over the keys, two passes (maximum, then exp / sum / P V with the probabilities broadcast by `__shfl`),
// fp32, every access bounds-checked.
//
// Index math is 32-bit; the launchers refuse sizes whose element offsets would not fit.
#include "kernels.h"

namespace adapt {
namespace {

constexpr int AT_QT = 64;     // queries per block (4 waves x 16)
constexpr int AT_KT = 32;     // keys per LDS tile
constexpr int AT_PAD = 4;     // floats of padding per LDS row

__device__ __forceinline__ f32x4 at_ld4(const float* p) { return *(const f32x4*)p; }
__device__ __forceinline__ f32x4 at_ld4(const bf16* p) {
  union { uint2 u; bf16 e[4]; } t;
  t.u = *(const uint2*)p;
  return f32x4{bf2f(t.e[0]), bf2f(t.e[1]), bf2f(t.e[2]), bf2f(t.e[3])};
}
__device__ __forceinline__ void at_st4(float* p, f32x4 v) { *(f32x4*)p = v; }
__device__ __forceinline__ void at_st4(bf16* p, f32x4 v) {
  union { uint2 u; bf16 e[4]; } t;
  t.e[0] = f2bf(v.x); t.e[1] = f2bf(v.y); t.e[2] = f2bf(v.z); t.e[3] = f2bf(v.w);
  *(uint2*)p = t.u;
}
__device__ __forceinline__ float at_ld(const float* p) { return *p; }
__device__ __forceinline__ float at_ld(const bf16* p) { return bf2f(*p); }
__device__ __forceinline__ void at_st(float* p, float v) { *p = v; }
__device__ __forceinline__ void at_st(bf16* p, float v) { *p = f2bf(v); }

// DMAX: the head sizes this instantiation holds in registers (d, dv <= DMAX, both multiples of 16)
template <typename T, int DMAX>
__global__ __launch_bounds__(256) void attention_mfma_kernel(const T* __restrict__ qkv, T* __restrict__ out, int Tn,
                                                             int heads, int d, int dv, int ld_in, int ld_out,
                                                             int qtiles) {
  constexpr int ND = DMAX / 16;                       // 16-wide slices of d / dv
  constexpr int NST = AT_KT * DMAX / 512;             // staged 4-element vectors per thread (K and V together)
  __shared__ __attribute__((aligned(16))) float smem[2 * AT_KT * (DMAX + AT_PAD)];
  float* sk = smem;
  float* sv = smem + AT_KT * (DMAX + AT_PAD);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  int bid = blockIdx.x;
  const int qt = bid % qtiles;
  bid /= qtiles;
  const int h = bid % heads, img = bid / heads;
  const int ldk = d + AT_PAD, ldv = dv + AT_PAD;
  const T* base = qkv + img * Tn * ld_in;             // this image's rows
  const int kcol = heads * d + h * d, vcol = 2 * heads * d + h * dv;

  // what this thread stages of every key tile: vector `idx` of the tile's K rows, then of its V rows
  const int nkv = d >> 2, nvv = dv >> 2;
  int srow[NST], sgcol[NST], sloff[NST];
  bool sval[NST];
#pragma unroll
  for (int j = 0; j < NST; ++j) {
    int idx = tid + j * 256;
    sval[j] = idx < AT_KT * (nkv + nvv);
    srow[j] = sgcol[j] = sloff[j] = 0;
    if (idx < AT_KT * nkv) {
      srow[j] = idx / nkv;
      const int v = idx - srow[j] * nkv;
      sgcol[j] = kcol + 4 * v;
      sloff[j] = srow[j] * ldk + 4 * v;
    } else if (sval[j]) {
      idx -= AT_KT * nkv;
      srow[j] = idx / nvv;
      const int v = idx - srow[j] * nvv;
      sgcol[j] = vcol + 4 * v;
      sloff[j] = AT_KT * (DMAX + AT_PAD) + srow[j] * ldv + 4 * v;
    }
  }

  const int q0 = qt * AT_QT + wave * 16;
  const bool active = q0 < Tn;                        // wave-uniform
  const int qrow = q0 + c;
  f32x4 qf[ND];
#pragma unroll
  for (int t = 0; t < ND; ++t) {
    qf[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (qrow < Tn && 16 * t < d) qf[t] = at_ld4(base + qrow * ld_in + h * d + 16 * t + 4 * g);
  }
  f32x4 o[ND];
#pragma unroll
  for (int n = 0; n < ND; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;                       // l: this lane's keys only, summed over the groups at the end

  f32x4 st[NST];
#pragma unroll
  for (int j = 0; j < NST; ++j) {
    st[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (sval[j] && srow[j] < Tn) st[j] = at_ld4(base + srow[j] * ld_in + sgcol[j]);
  }
  for (int k0 = 0; k0 < Tn; k0 += AT_KT) {
    __syncthreads();                                  // the previous tile has been read
#pragma unroll
    for (int j = 0; j < NST; ++j)
      if (sval[j]) *(f32x4*)(smem + sloff[j]) = st[j];
    __syncthreads();
    if (k0 + AT_KT < Tn) {
#pragma unroll
      for (int j = 0; j < NST; ++j) {
        st[j] = f32x4{0.f, 0.f, 0.f, 0.f};            // rows >= T are zeros, never loaded
        const int r = k0 + AT_KT + srow[j];
        if (sval[j] && r < Tn) st[j] = at_ld4(base + r * ld_in + sgcol[j]);
      }
    }
    if (!active) continue;
    // S^T = K Q^T: s[u][i] = score(key k0 + 16 u + 4 g + i, query c)
    f32x4 s[AT_KT / 16];
#pragma unroll
    for (int u = 0; u < AT_KT / 16; ++u) {
      s[u] = f32x4{0.f, 0.f, 0.f, 0.f};
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
    for (int u = 0; u < AT_KT / 16; ++u)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (k0 + 16 * u + 4 * g + i >= Tn) s[u][i] = -INFINITY;
        mx = fmaxf(mx, s[u][i]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));               // finite: key k0 < T is in every tile
    const float mn = fmaxf(m, mx);
    const float alpha = expf(m - mn);                 // 0 on the first tile (m = -inf)
    m = mn;
    float ps = 0.f;
#pragma unroll
    for (int u = 0; u < AT_KT / 16; ++u)
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
    for (int u = 0; u < AT_KT / 16; ++u)
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
  if (!active) return;
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (qrow >= Tn) return;
  const float inv = 1.f / l;
  T* orow = out + (img * Tn + qrow) * ld_out;
#pragma unroll
  for (int n = 0; n < ND; ++n)
    if (16 * n < dv) at_st4(orow + h * dv + 16 * n + 4 * g, o[n] * inv);
  if (h == heads - 1)                                 // layout padding of the row: zeros
    for (int cc = heads * dv + g; cc < ld_out; cc += 4) at_st(orow + cc, 0.f);
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
__device__ __forceinline__ float at_dot(const T* __restrict__ a, const T* __restrict__ b, int n) {
  float s = 0.f;
  for (int i = 0; i < n; ++i) s += at_ld(a + i) * at_ld(b + i);
  return s;
}

// Any d, dv, stride and alignment: one wave per (image, head, query).
template <typename T>
__global__ __launch_bounds__(256) void attention_plain_kernel(const T* __restrict__ qkv, T* __restrict__ out, int rows,
                                                              int Tn, int heads, int d, int dv, int ld_in,
                                                              int ld_out) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= rows) return;                              // the whole wave leaves together
  const int q = w % Tn, r = w / Tn;
  const int h = r % heads, img = r / heads;
  const T* base = qkv + img * Tn * ld_in;
  const T* qp = base + q * ld_in + h * d;
  const T* kp = base + heads * d + h * d;
  const T* vp = base + 2 * heads * d + h * dv;
  float mx = -INFINITY;
  for (int k = lane; k < Tn; k += 64) mx = fmaxf(mx, at_dot(qp, kp + k * ld_in, d));
  mx = wave_max(mx);
  T* orow = out + (img * Tn + q) * ld_out;
  for (int c0 = 0; c0 < dv; c0 += 64) {               // 64 output channels at a time, one per lane
    const int cc = c0 + lane;
    float acc = 0.f, ls = 0.f;
    for (int kb = 0; kb < Tn; kb += 64) {
      const int k = kb + lane;
      const float p = k < Tn ? expf(at_dot(qp, kp + k * ld_in, d) - mx) : 0.f;
      ls += p;
      const int nk = min(64, Tn - kb);
      for (int kk = 0; kk < nk; ++kk) {
        const float pk = __shfl(p, kk);
        if (cc < dv) acc += pk * at_ld(vp + (kb + kk) * ld_in + cc);
      }
    }
    const float l = wave_sum(ls);
    if (cc < dv) at_st(orow + h * dv + cc, acc / l);
  }
  if (h == heads - 1)
    for (int cc = heads * dv + lane; cc < ld_out; cc += 64) at_st(orow + cc, 0.f);
}

template <typename T>
hipError_t attention_launch(const T* qkv, T* out, int B, int Tn, int heads, int d, int dv, int ld_in, int ld_out,
                            hipStream_t s) {
  if (B < 1 || Tn < 1 || heads < 1 || d < 1 || dv < 1) return hipErrorInvalidValue;
  const long long lim = 0x7fffffffll;
  if ((long long)heads * (2ll * d + dv) > ld_in || (long long)heads * dv > ld_out) return hipErrorInvalidValue;
  // 32-bit element offsets and grid sizes: refuse what does not fit
  if ((long long)B * Tn * ld_in > lim || (long long)B * Tn * ld_out > lim || (long long)B * heads * Tn > lim)
    return hipErrorInvalidValue;
  const uintptr_t align = sizeof(T) * 4 - 1;          // the MFMA kernel moves 4 elements at a time
  const bool vec = ld_in % 4 == 0 && ld_out % 4 == 0 && (((uintptr_t)qkv | (uintptr_t)out) & align) == 0;
  if (attention_path(d, dv) && vec) {
    const int qtiles = (Tn + AT_QT - 1) / AT_QT;
    const dim3 grid(B * heads * qtiles), block(256);
    const int dm = d > dv ? d : dv;
    if (dm <= 32)
      hipLaunchKernelGGL((attention_mfma_kernel<T, 32>), grid, block, 0, s, qkv, out, Tn, heads, d, dv, ld_in, ld_out,
                         qtiles);
    else if (dm <= 64)
      hipLaunchKernelGGL((attention_mfma_kernel<T, 64>), grid, block, 0, s, qkv, out, Tn, heads, d, dv, ld_in, ld_out,
                         qtiles);
    else
      hipLaunchKernelGGL((attention_mfma_kernel<T, 128>), grid, block, 0, s, qkv, out, Tn, heads, d, dv, ld_in,
                         ld_out, qtiles);
  } else {
    const int rows = B * heads * Tn;
    hipLaunchKernelGGL(attention_plain_kernel<T>, dim3((rows + 3) / 4), dim3(256), 0, s, qkv, out, rows, Tn, heads, d,
                       dv, ld_in, ld_out);
  }
  return hipGetLastError();
}

}  // namespace

int attention_query_tile() { return AT_QT; }
int attention_key_tile() { return AT_KT; }

// 1: the MFMA path, 0: the plain kernel (which a misaligned buffer or stride takes as well)
int attention_path(int d, int dv) { return d >= 16 && dv >= 16 && d <= 128 && dv <= 128 && d % 16 == 0 && dv % 16 == 0; }

hipError_t attention_f32(const float* qkv, float* out, int B, int T, int heads, int d, int dv, int ld_in, int ld_out,
                         hipStream_t s) {
  return attention_launch<float>(qkv, out, B, T, heads, d, dv, ld_in, ld_out, s);
}

hipError_t attention_bf16(const bf16* qkv, bf16* out, int B, int T, int heads, int d, int dv, int ld_in, int ld_out,
                          hipStream_t s) {
  return attention_launch<bf16>(qkv, out, B, T, heads, d, dv, ld_in, ld_out, s);
}

}  // namespace adapt
