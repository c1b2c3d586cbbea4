// Layers beyond the ResNet set, for the other Keras model families the
// DEFER API can be handed (models/zoo.py: MobileNetV2's DepthwiseConv2D,
// DenseNet's Concatenate + AveragePooling2D).  All three are memory-bound
// streams over bf16 NHWC activations whose channel dim is padded to Cp (a
// multiple of 8, the runtime's 16-byte vector layout): one thread per
// 8-channel chunk of one output pixel, 16-byte loads and stores, fp32 math.
#include "kernels.h"

namespace adapt {

namespace {
__device__ __forceinline__ size_t gstride() { return (size_t)gridDim.x * blockDim.x; }
__device__ __forceinline__ size_t gtid() { return blockIdx.x * (size_t)blockDim.x + threadIdx.x; }
inline unsigned grid_of(size_t n) {
  size_t g = (n + 255) / 256;
  return (unsigned)(g < 8192 ? (g ? g : 1) : 8192);
}
}  // namespace

// Depthwise KHxKW conv (depth multiplier 1): y[b,oh,ow,c] = act(sum_taps x * w[kh][kw][c] + bias[c]),
// BN folded into w/bias on the host; zero padding is implicit (pad_t / pad_l, Keras 'same' or a folded
// ZeroPadding2D).  w: fp32 [KH][KW][Cp].
template <bool GEN>
__global__ __launch_bounds__(256) void dwconv_kernel(const bf16* __restrict__ x, const float* __restrict__ w,
                                                     const float* __restrict__ bias, bf16* __restrict__ y, int B,
                                                     int H, int W, int Cp, int OH, int OW, int KH, int KW,
                                                     int stride, int pad_t, int pad_l, int act) {
  const int cpr = Cp / 8;
  const size_t total = (size_t)B * OH * OW * cpr;
  for (size_t i = gtid(); i < total; i += gstride()) {
    const int c0 = (int)(i % cpr) * 8;
    size_t pix = i / cpr;
    const int ow = (int)(pix % OW);
    pix /= OW;
    const int oh = (int)(pix % OH);
    const int b = (int)(pix / OH);
    float acc[8];
    const f32x4 b0 = *(const f32x4*)(bias + c0), b1 = *(const f32x4*)(bias + c0 + 4);
    acc[0] = b0[0]; acc[1] = b0[1]; acc[2] = b0[2]; acc[3] = b0[3];
    acc[4] = b1[0]; acc[5] = b1[1]; acc[6] = b1[2]; acc[7] = b1[3];
    const int ih0 = oh * stride - pad_t, iw0 = ow * stride - pad_l;
    for (int kh = 0; kh < KH; ++kh) {
      const int ih = ih0 + kh;
      if ((unsigned)ih >= (unsigned)H) continue;
      for (int kw = 0; kw < KW; ++kw) {
        const int iw = iw0 + kw;
        if ((unsigned)iw >= (unsigned)W) continue;
        V8 v;
        v.u = *(const u32x4*)(x + (((size_t)b * H + ih) * W + iw) * Cp + c0);
        const float* wt = w + ((size_t)kh * KW + kw) * Cp + c0;
        const f32x4 w0 = *(const f32x4*)wt, w1 = *(const f32x4*)(wt + 4);
        float xf[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) xf[t] = bf2f(v.e[t]);
        acc[0] += xf[0] * w0[0]; acc[1] += xf[1] * w0[1];
        acc[2] += xf[2] * w0[2]; acc[3] += xf[3] * w0[3];
        acc[4] += xf[4] * w1[0]; acc[5] += xf[5] * w1[1];
        acc[6] += xf[6] * w1[2]; acc[7] += xf[7] * w1[3];
      }
    }
    V8 o;
#pragma unroll
    for (int t = 0; t < 8; ++t) o.e[t] = f2bf(actx<GEN>(acc[t], act));
    *(u32x4*)(y + i * 8) = o.u;
  }
}

// 3x3 specialisation: a thread owns OWG consecutive output pixels of one row and one 8-channel chunk, so
// each input column of the (OWG-1)*S+3 it touches is loaded once per filter row (6 loads per row instead of
// 12 at stride 1, 9 instead of 12 at stride 2) and the row's three weight vectors stay in registers.
template <int S, int OWG, bool GEN>
__global__ __launch_bounds__(256) void dwconv3_kernel(const bf16* __restrict__ x, const float* __restrict__ w,
                                                      const float* __restrict__ bias, bf16* __restrict__ y, int B,
                                                      int H, int W, int Cp, int OH, int OW, int pad_t, int pad_l,
                                                      int act) {
  constexpr int COLS = (OWG - 1) * S + 3;
  const int cpr = Cp / 8;
  const int owg = (OW + OWG - 1) / OWG;
  const size_t total = (size_t)B * OH * owg * cpr;
  for (size_t i = gtid(); i < total; i += gstride()) {
    const int c0 = (int)(i % cpr) * 8;
    size_t pix = i / cpr;
    const int ow0 = (int)(pix % owg) * OWG;
    pix /= owg;
    const int oh = (int)(pix % OH);
    const int b = (int)(pix / OH);
    float acc[OWG][8];
    {
      const f32x4 b0 = *(const f32x4*)(bias + c0), b1 = *(const f32x4*)(bias + c0 + 4);
#pragma unroll
      for (int j = 0; j < OWG; ++j) {
        acc[j][0] = b0[0]; acc[j][1] = b0[1]; acc[j][2] = b0[2]; acc[j][3] = b0[3];
        acc[j][4] = b1[0]; acc[j][5] = b1[1]; acc[j][6] = b1[2]; acc[j][7] = b1[3];
      }
    }
    const int iw0 = ow0 * S - pad_l;
#pragma unroll
    for (int kh = 0; kh < 3; ++kh) {
      const int ih = oh * S - pad_t + kh;
      if ((unsigned)ih >= (unsigned)H) continue;
      float wk[3][8];
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) {
        const float* wt = w + ((size_t)kh * 3 + kw) * Cp + c0;
        const f32x4 w0 = *(const f32x4*)wt, w1 = *(const f32x4*)(wt + 4);
        wk[kw][0] = w0[0]; wk[kw][1] = w0[1]; wk[kw][2] = w0[2]; wk[kw][3] = w0[3];
        wk[kw][4] = w1[0]; wk[kw][5] = w1[1]; wk[kw][6] = w1[2]; wk[kw][7] = w1[3];
      }
      const bf16* row = x + ((size_t)b * H + ih) * W * Cp + c0;
#pragma unroll
      for (int c = 0; c < COLS; ++c) {
        const int iw = iw0 + c;
        if ((unsigned)iw >= (unsigned)W) continue;
        V8 v;
        v.u = *(const u32x4*)(row + (size_t)iw * Cp);
        float xf[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) xf[t] = bf2f(v.e[t]);
#pragma unroll
        for (int j = 0; j < OWG; ++j) {
          const int kw = c - j * S;
          if (kw < 0 || kw > 2) continue;      // compile-time after unrolling
#pragma unroll
          for (int t = 0; t < 8; ++t) acc[j][t] += xf[t] * wk[kw][t];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < OWG; ++j) {
      if (ow0 + j >= OW) break;
      V8 o;
#pragma unroll
      for (int t = 0; t < 8; ++t) o.e[t] = f2bf(actx<GEN>(acc[j][t], act));
      *(u32x4*)(y + (((size_t)b * OH + oh) * OW + ow0 + j) * Cp + c0) = o.u;
    }
  }
}

// Average pool; padded positions are excluded from the count (TF/Keras 'same'), 'valid' has none.
__global__ __launch_bounds__(256) void avgpool_kernel(const bf16* __restrict__ x, bf16* __restrict__ y, int B, int H,
                                                      int W, int Cp, int OH, int OW, int KH, int KW, int S,
                                                      int pad_t, int pad_l) {
  const int cpr = Cp / 8;
  const size_t total = (size_t)B * OH * OW * cpr;
  for (size_t i = gtid(); i < total; i += gstride()) {
    const int c0 = (int)(i % cpr) * 8;
    size_t pix = i / cpr;
    const int ow = (int)(pix % OW);
    pix /= OW;
    const int oh = (int)(pix % OH);
    const int b = (int)(pix / OH);
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int n = 0;
    for (int kh = 0; kh < KH; ++kh) {
      const int ih = oh * S - pad_t + kh;
      if ((unsigned)ih >= (unsigned)H) continue;
      for (int kw = 0; kw < KW; ++kw) {
        const int iw = ow * S - pad_l + kw;
        if ((unsigned)iw >= (unsigned)W) continue;
        V8 v;
        v.u = *(const u32x4*)(x + (((size_t)b * H + ih) * W + iw) * Cp + c0);
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[t] += bf2f(v.e[t]);
        ++n;
      }
    }
    const float inv = n ? 1.f / (float)n : 0.f;
    V8 o;
#pragma unroll
    for (int t = 0; t < 8; ++t) o.e[t] = f2bf(acc[t] * inv);
    *(u32x4*)(y + i * 8) = o.u;
  }
}

// One input of a channel concat: y[p][off + c] = x[p][c] for c < Cx; channels [zero_from, Cpy) of y are
// zeroed (the padding of the last input).  Aligned inputs (off, Cx, Cpx multiples of 8) move 16-byte chunks.
__global__ __launch_bounds__(256) void concat_vec_kernel(const bf16* __restrict__ x, int Cpx, bf16* __restrict__ y,
                                                         int Cpy, int off, int nchunk, size_t pixels) {
  const size_t total = pixels * nchunk;
  for (size_t i = gtid(); i < total; i += gstride()) {
    const size_t p = i / nchunk;
    const int c = (int)(i % nchunk) * 8;
    *(u32x4*)(y + p * Cpy + off + c) = *(const u32x4*)(x + p * Cpx + c);
  }
}

__global__ __launch_bounds__(256) void concat_scalar_kernel(const bf16* __restrict__ x, int Cx, int Cpx,
                                                            bf16* __restrict__ y, int Cpy, int off, int zero_from,
                                                            size_t pixels) {
  const int span = Cx + (zero_from < Cpy ? Cpy - zero_from : 0);
  const size_t total = pixels * span;
  for (size_t i = gtid(); i < total; i += gstride()) {
    const size_t p = i / span;
    const int c = (int)(i % span);
    if (c < Cx) y[p * Cpy + off + c] = x[p * Cpx + c];
    else y[p * Cpy + zero_from + (c - Cx)] = f2bf(0.f);
  }
}

// Standalone activation (any ActMode, LeakyReLU slope alpha) over bf16 chunks.
template <bool GEN>
__global__ __launch_bounds__(256) void act_kernel(const bf16* __restrict__ x, bf16* __restrict__ y, size_t chunks,
                                                  int mode, float alpha) {
  for (size_t i = gtid(); i < chunks; i += gstride()) {
    V8 v, o;
    v.u = ((const u32x4*)x)[i];
#pragma unroll
    for (int t = 0; t < 8; ++t) o.e[t] = f2bf(actx<GEN>(bf2f(v.e[t]), mode, alpha));
    ((u32x4*)y)[i] = o.u;
  }
}

// Element-wise binary op (Keras Multiply / Subtract / Maximum / Minimum / Average / Add) of a [P][Cp] tensor
// with b, where b is either the same shape or one [Cp] row per image (bcast_hw = H*W pixels share it: the
// squeeze-excite Multiply of EfficientNet, x * se[b, 1, 1, c]).
enum BinOp { BIN_ADD = 0, BIN_SUB, BIN_MUL, BIN_MAX, BIN_MIN, BIN_AVG };
template <bool GEN>
__global__ __launch_bounds__(256) void binary_kernel(const bf16* __restrict__ a, const bf16* __restrict__ b,
                                                     bf16* __restrict__ y, size_t chunks, int cpr, int bcast_hw,
                                                     int op, int act) {
  for (size_t i = gtid(); i < chunks; i += gstride()) {
    size_t bi = i;
    if (bcast_hw) {
      const size_t pix = i / cpr;
      bi = (pix / bcast_hw) * cpr + (i % cpr);
    }
    V8 va, vb, o;
    va.u = ((const u32x4*)a)[i];
    vb.u = ((const u32x4*)b)[bi];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const float p = bf2f(va.e[t]), q = bf2f(vb.e[t]);
      float r;
      switch (op) {
        case BIN_SUB: r = p - q; break;
        case BIN_MUL: r = p * q; break;
        case BIN_MAX: r = fmaxf(p, q); break;
        case BIN_MIN: r = fminf(p, q); break;
        case BIN_AVG: r = 0.5f * (p + q); break;
        default: r = p + q;
      }
      o.e[t] = f2bf(actx<GEN>(r, act));
    }
    ((u32x4*)y)[i] = o.u;
  }
}

// Global max pool: block (image, 64 chunks), 4 pixel groups, LDS combine (as head.hip's GAP).
__global__ __launch_bounds__(256) void gmp_kernel(const bf16* __restrict__ x, bf16* __restrict__ y, int HW, int Cp) {
  __shared__ float part[4][64][9];
  const int b = blockIdx.y;
  const int ch = threadIdx.x & 63, grp = threadIdx.x >> 6;
  const int cc = blockIdx.x * 64 + ch;
  const bool ok = cc * 8 < Cp;
  float m[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) m[t] = -INFINITY;
  if (ok) {
    const bf16* base = x + (size_t)b * HW * Cp + cc * 8;
    for (int i = grp; i < HW; i += 4) {
      V8 v;
      v.u = *(const u32x4*)(base + (size_t)i * Cp);
#pragma unroll
      for (int t = 0; t < 8; ++t) m[t] = fmaxf(m[t], bf2f(v.e[t]));
    }
  }
#pragma unroll
  for (int t = 0; t < 8; ++t) part[grp][ch][t] = m[t];
  __syncthreads();
  if (grp != 0 || !ok) return;
  V8 o;
#pragma unroll
  for (int t = 0; t < 8; ++t)
    o.e[t] = f2bf(fmaxf(fmaxf(part[0][ch][t], part[1][ch][t]), fmaxf(part[2][ch][t], part[3][ch][t])));
  *(u32x4*)(y + (size_t)b * Cp + cc * 8) = o.u;
}

// Global average pool over LARGE maps (EfficientNet's squeeze-excite at 112x112 .. 28x28), where head.hip's
// one-block-per-image GAP leaves most of the chip idle.  Pass 1: grid (S pixel slices, B); a block sums its
// slice for a group of up to 256 channel chunks (lane = chunk, the remaining threads stride the pixels) and
// reduces in LDS to one fp32 partial per channel.  Pass 2: sum of the S partials / HW -> bf16.
__global__ __launch_bounds__(256) void gap_part_kernel(const bf16* __restrict__ x, float* __restrict__ part,
                                                       int HW, int Cp, int S) {
  __shared__ float red[256][9];
  const int b = blockIdx.y, sl = blockIdx.x;
  const int cpr = Cp / 8;
  const int p0 = (int)((long long)HW * sl / S), p1 = (int)((long long)HW * (sl + 1) / S);
  for (int cg = 0; cg < cpr; cg += 256) {
    const int nc = min(256, cpr - cg);
    const int lanes = 256 / nc;                      // pixel lanes per chunk
    const int ch = threadIdx.x % nc, pl = threadIdx.x / nc;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (pl < lanes) {
      const bf16* base = x + (size_t)b * HW * Cp + (size_t)(cg + ch) * 8;
      for (int p = p0 + pl; p < p1; p += lanes) {
        V8 v;
        v.u = *(const u32x4*)(base + (size_t)p * Cp);
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[t] += bf2f(v.e[t]);
      }
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) red[threadIdx.x][t] = acc[t];
    __syncthreads();
    if (threadIdx.x < nc) {
      float sum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int l = 0; l < lanes; ++l)
#pragma unroll
        for (int t = 0; t < 8; ++t) sum[t] += red[l * nc + threadIdx.x][t];
      float* d = part + ((size_t)b * S + sl) * Cp + (size_t)(cg + threadIdx.x) * 8;
#pragma unroll
      for (int t = 0; t < 8; ++t) d[t] = sum[t];
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void gap_finish_kernel(const float* __restrict__ part, bf16* __restrict__ y,
                                                         float* __restrict__ y32, int B, int HW, int Cp, int S) {
  const size_t total = (size_t)B * Cp;
  const float inv = 1.f / (float)HW;
  for (size_t i = gtid(); i < total; i += gstride()) {
    const size_t b = i / Cp, c = i % Cp;
    float sum = 0.f;
    for (int sl = 0; sl < S; ++sl) sum += part[(b * S + sl) * Cp + c];
    if (y) y[i] = f2bf(sum * inv);
    if (y32) y32[i] = sum * inv;
  }
}

int gap_large_slices(int B, int HW) {
  int s = (512 + B - 1) / B;                       // ~2 blocks per CU in all
  const int cap = HW / 64 > 0 ? HW / 64 : 1;       // >= 64 pixels per slice
  return s < 1 ? 1 : (s > cap ? cap : s);
}

hipError_t gap_large(const bf16* x, bf16* y, float* y32, float* part, int B, int HW, int Cp, hipStream_t s) {
  if (Cp % 8) return hipErrorInvalidValue;
  const int S = gap_large_slices(B, HW);
  hipLaunchKernelGGL(gap_part_kernel, dim3(S, B), dim3(256), 0, s, x, part, HW, Cp, S);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(gap_finish_kernel, dim3(grid_of((size_t)B * Cp)), dim3(256), 0, s, part, y, y32, B, HW, Cp, S);
  return hipGetLastError();
}

hipError_t act(const bf16* x, bf16* y, size_t elems, int mode, float alpha, hipStream_t s) {
  if (elems % 8) return hipErrorInvalidValue;
  if (mode > ACT_RELU6) hipLaunchKernelGGL(act_kernel<true>, dim3(grid_of(elems / 8)), dim3(256), 0, s, x, y, elems / 8, mode, alpha);
  else hipLaunchKernelGGL(act_kernel<false>, dim3(grid_of(elems / 8)), dim3(256), 0, s, x, y, elems / 8, mode, alpha);
  return hipGetLastError();
}

hipError_t binary(const bf16* a, const bf16* b, bf16* y, size_t elems, int Cp, int bcast_hw, int op, int act_mode,
                  hipStream_t s) {
  if (elems % 8 || Cp % 8) return hipErrorInvalidValue;
  if (act_mode > ACT_RELU6)
    hipLaunchKernelGGL(binary_kernel<true>, dim3(grid_of(elems / 8)), dim3(256), 0, s, a, b, y, elems / 8, Cp / 8,
                       bcast_hw, op, act_mode);
  else
    hipLaunchKernelGGL(binary_kernel<false>, dim3(grid_of(elems / 8)), dim3(256), 0, s, a, b, y, elems / 8, Cp / 8,
                       bcast_hw, op, act_mode);
  return hipGetLastError();
}

hipError_t gmp(const bf16* x, bf16* y, int B, int HW, int Cp, hipStream_t s) {
  if (Cp % 8) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gmp_kernel, dim3((Cp / 8 + 63) / 64, B), dim3(256), 0, s, x, y, HW, Cp);
  return hipGetLastError();
}

hipError_t dwconv(const bf16* x, const float* w, const float* bias, bf16* y, int B, int H, int W, int Cp, int OH,
                  int OW, int KH, int KW, int stride, int pad_t, int pad_l, int act, hipStream_t s) {
  if (Cp % 8) return hipErrorInvalidValue;
  // The register-blocked 3x3 kernel pays off at stride 1 on large maps; measured on MobileNetV2 bs=32
  // (profiles/mbv2_bs32_steps_v*.json) it lost at stride 2 and on grids under ~512 blocks, where the
  // thread-per-pixel kernel keeps 4x more loads in flight.
  constexpr int OWG = 4;
  const size_t t3 = (size_t)B * OH * ((OW + OWG - 1) / OWG) * (Cp / 8);
  if (KH == 3 && KW == 3 && stride == 1 && t3 >= 512 * 256) {
    if (act > ACT_RELU6)
      hipLaunchKernelGGL((dwconv3_kernel<1, OWG, true>), dim3(grid_of(t3)), dim3(256), 0, s, x, w, bias, y, B, H, W, Cp,
                         OH, OW, pad_t, pad_l, act);
    else
      hipLaunchKernelGGL((dwconv3_kernel<1, OWG, false>), dim3(grid_of(t3)), dim3(256), 0, s, x, w, bias, y, B, H, W, Cp,
                         OH, OW, pad_t, pad_l, act);
    return hipGetLastError();
  }
  const size_t total = (size_t)B * OH * OW * (Cp / 8);
  if (act > ACT_RELU6)
    hipLaunchKernelGGL(dwconv_kernel<true>, dim3(grid_of(total)), dim3(256), 0, s, x, w, bias, y, B, H, W, Cp, OH, OW,
                       KH, KW, stride, pad_t, pad_l, act);
  else
    hipLaunchKernelGGL(dwconv_kernel<false>, dim3(grid_of(total)), dim3(256), 0, s, x, w, bias, y, B, H, W, Cp, OH, OW,
                       KH, KW, stride, pad_t, pad_l, act);
  return hipGetLastError();
}

hipError_t avgpool(const bf16* x, bf16* y, int B, int H, int W, int Cp, int OH, int OW, int KH, int KW, int S,
                   int pad_t, int pad_l, hipStream_t s) {
  if (Cp % 8) return hipErrorInvalidValue;
  const size_t total = (size_t)B * OH * OW * (Cp / 8);
  hipLaunchKernelGGL(avgpool_kernel, dim3(grid_of(total)), dim3(256), 0, s, x, y, B, H, W, Cp, OH, OW, KH, KW, S,
                     pad_t, pad_l);
  return hipGetLastError();
}

hipError_t concat_into(const bf16* x, int Cx, int Cpx, bf16* y, int Cpy, int off, int zero_from, size_t pixels,
                       hipStream_t s) {
  if (off + Cx > Cpy || Cx > Cpx || zero_from > Cpy) return hipErrorInvalidValue;
  if (off % 8 == 0 && Cx % 8 == 0 && Cpx % 8 == 0 && Cpy % 8 == 0 && zero_from >= Cpy) {
    const int nchunk = Cx / 8;
    hipLaunchKernelGGL(concat_vec_kernel, dim3(grid_of(pixels * nchunk)), dim3(256), 0, s, x, Cpx, y, Cpy, off,
                       nchunk, pixels);
  } else {
    const size_t span = (size_t)Cx + (zero_from < Cpy ? Cpy - zero_from : 0);
    hipLaunchKernelGGL(concat_scalar_kernel, dim3(grid_of(pixels * span)), dim3(256), 0, s, x, Cx, Cpx, y, Cpy,
                       off, zero_from, pixels);
  }
  return hipGetLastError();
}

// ViT class token + learned position embedding: y[b][0] = cls + pos[0] (with a class token, ct = 1),
// y[b][ct + t] = x[b][t] + pos[ct + t].  x is [B][T][ld], y [B][T + ct][ld] (fp32 rows of C channels, or bf16
// rows padded to ld with channels C..ld-1 written as zeros whatever x holds there); cls [C] and pos [T + ct][C]
// are fp32.  VEC = 16 bytes of activations per thread where ld and the bases allow, else 1.
namespace {
template <typename T, int VEC>
__global__ __launch_bounds__(256) void posembed_kernel(const T* __restrict__ x, const float* __restrict__ cls,
                                                        const float* __restrict__ pos, T* __restrict__ y, int Tn,
                                                        int C, int ld, int ct, size_t total) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int nv = ld / VEC;
  const int v = (int)(idx % nv);
  const size_t row = idx / nv;
  const int t = (int)(row % (Tn + ct));
  const size_t b = row / (Tn + ct);
  const bool tok = t >= ct;                           // a token row; otherwise the class token's
  const T* xr = x + (tok ? (b * Tn + (t - ct)) * ld + (size_t)v * VEC : 0);
  float f[VEC];
  if constexpr (VEC == 1) {
    f[0] = (tok && v < C) ? (float)xr[0] : 0.f;
  } else if constexpr (sizeof(T) == 4) {
    f32x4 q = f32x4{0.f, 0.f, 0.f, 0.f};
    if (tok) q = *(const f32x4*)xr;
    f[0] = q.x; f[1] = q.y; f[2] = q.z; f[3] = q.w;
  } else {
    V8 q;
    q.u = u32x4{0u, 0u, 0u, 0u};
    if (tok) q.u = *(const u32x4*)xr;
#pragma unroll
    for (int e = 0; e < VEC; ++e) f[e] = (float)q.e[e];
  }
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    const int c = v * VEC + e;
    f[e] = c < C ? (tok ? f[e] : cls[c]) + pos[(size_t)t * C + c] : 0.f;      // padding never enters
  }
  T* yr = y + row * ld + (size_t)v * VEC;
  if constexpr (VEC == 1) {
    yr[0] = (T)f[0];
  } else if constexpr (sizeof(T) == 4) {
    *(f32x4*)yr = f32x4{f[0], f[1], f[2], f[3]};
  } else {
    V8 q;
#pragma unroll
    for (int e = 0; e < VEC; ++e) q.e[e] = f2bf(f[e]);
    *(u32x4*)yr = q.u;
  }
}

template <typename T>
hipError_t posembed_launch(const T* x, const float* cls, const float* pos, T* y, int B, int Tn, int C, int ld, int ct,
                           hipStream_t s) {
  constexpr int VEC = 16 / sizeof(T);
  if (B < 1 || Tn < 1 || C < 1 || ld < C || ct < 0 || ct > 1 || (ct && !cls)) return hipErrorInvalidValue;
  const size_t rows = (size_t)B * (Tn + ct);
  if (ld % VEC == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0) {
    const size_t total = rows * (ld / VEC);
    hipLaunchKernelGGL((posembed_kernel<T, VEC>), dim3(grid_of(total)), dim3(256), 0, s, x, cls, pos, y, Tn, C, ld, ct,
                       total);
  } else {
    const size_t total = rows * ld;
    hipLaunchKernelGGL((posembed_kernel<T, 1>), dim3(grid_of(total)), dim3(256), 0, s, x, cls, pos, y, Tn, C, ld, ct,
                       total);
  }
  return hipGetLastError();
}
}  // namespace

hipError_t posembed_f32(const float* x, const float* cls, const float* pos, float* y, int B, int T, int C, int ct,
                        hipStream_t s) {
  return posembed_launch<float>(x, cls, pos, y, B, T, C, C, ct, s);
}

hipError_t posembed_bf16(const bf16* x, const float* cls, const float* pos, bf16* y, int B, int T, int Cp, int C,
                         int ct, hipStream_t s) {
  return posembed_launch<bf16>(x, cls, pos, y, B, T, C, Cp, ct, s);
}

// Learned queries: y[b][t][c] = emb[t][c] for every image b, a broadcast copy like posembed's.  emb [N][C] is fp32,
// y [B][N][ld] (fp32 rows of C channels, or bf16 rows padded to ld with channels C..ld-1 written as zeros).
// VEC = 16 bytes of y per thread where ld, C and the bases allow (every vector then lies wholly inside or wholly
// outside the C channels, and emb is read 16 bytes at a time), else 1.
namespace {
template <typename T, int VEC>
__global__ __launch_bounds__(256) void queries_kernel(const float* __restrict__ emb, T* __restrict__ y, int N, int C,
                                                      int ld, size_t total) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int nv = ld / VEC;
  const int v = (int)(idx % nv);
  const size_t row = idx / nv;
  const int t = (int)(row % N);
  const float* er = emb + (size_t)t * C + (size_t)v * VEC;
  T* yr = y + row * ld + (size_t)v * VEC;
  if constexpr (VEC == 1) {
    yr[0] = (T)(v < C ? er[0] : 0.f);
  } else if constexpr (sizeof(T) == 4) {
    *(f32x4*)yr = *(const f32x4*)er;                  // fp32 rows are not padded: ld == C
  } else {
    f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f}, b = a;
    if (v * VEC < C) {                                // C % 8 == 0 here: the vector is all channels or all padding
      a = *(const f32x4*)er;
      b = *(const f32x4*)(er + 4);
    }
    V8 q;
    q.e[0] = f2bf(a.x); q.e[1] = f2bf(a.y); q.e[2] = f2bf(a.z); q.e[3] = f2bf(a.w);
    q.e[4] = f2bf(b.x); q.e[5] = f2bf(b.y); q.e[6] = f2bf(b.z); q.e[7] = f2bf(b.w);
    *(u32x4*)yr = q.u;
  }
}

template <typename T>
hipError_t queries_launch(const float* emb, T* y, int B, int N, int C, int ld, hipStream_t s) {
  constexpr int VEC = 16 / sizeof(T);
  if (B < 1 || N < 1 || C < 1 || ld < C || !emb || !y) return hipErrorInvalidValue;
  if (sizeof(T) == 4 && ld != C) return hipErrorInvalidValue;
  const size_t rows = (size_t)B * N;
  if (ld % VEC == 0 && C % VEC == 0 && (((uintptr_t)emb | (uintptr_t)y) & 15) == 0) {
    const size_t total = rows * (ld / VEC);
    hipLaunchKernelGGL((queries_kernel<T, VEC>), dim3(grid_of(total)), dim3(256), 0, s, emb, y, N, C, ld, total);
  } else {
    const size_t total = rows * ld;
    hipLaunchKernelGGL((queries_kernel<T, 1>), dim3(grid_of(total)), dim3(256), 0, s, emb, y, N, C, ld, total);
  }
  return hipGetLastError();
}
}  // namespace

hipError_t queries_f32(const float* emb, float* y, int B, int N, int C, hipStream_t s) {
  return queries_launch<float>(emb, y, B, N, C, C, s);
}

hipError_t queries_bf16(const float* emb, bf16* y, int B, int N, int Cp, int C, hipStream_t s) {
  return queries_launch<bf16>(emb, y, B, N, C, Cp, s);
}

// Embedding: y[r] = table[(int)ids[r]], a row gather like the two copies above.  The token ids arrive as fp32 and
// are truncated toward zero (Keras casts a float input to int32); an id outside [0, V), an infinity or a NaN
// yields a zero row (TensorFlow's GPU gather), and its table row is never addressed.  table [V][ld] and y [rows][ld]
// are both in the activation type with rows of ld elements, so a row is copied as it stands, the bf16 layout's
// padding (prepared as zeros) included.  VEC = 16 bytes per thread where ld and the bases allow, else 1.  Offsets
// are 32-bit: the launcher refuses a table or an output of 2^31 elements or more, and V above 2^24, beyond
// which an fp32 id is no longer exact.
namespace {
template <typename T, int VEC>
__global__ __launch_bounds__(256) void embedding_kernel(const float* __restrict__ ids, const T* __restrict__ table,
                                                         T* __restrict__ y, int V, int ld, int total) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int nv = ld / VEC;
  const int v = idx % nv, row = idx / nv;
  const float f = ids[row];
  const bool ok = f > -1.f && f < (float)V;           // false for a NaN; (int)f then lies in [0, V)
  const int id = ok ? (int)f : 0;
  const T* tr = table + id * ld + v * VEC;
  T* yr = y + row * ld + v * VEC;
  if constexpr (VEC == 1) {
    yr[0] = ok ? tr[0] : (T)0.f;
  } else {
    u32x4 q = u32x4{0u, 0u, 0u, 0u};
    if (ok) q = *(const u32x4*)tr;
    *(u32x4*)yr = q;
  }
}

template <typename T>
hipError_t embedding_launch(const float* ids, const T* table, T* y, int rows, int V, int ld, hipStream_t s) {
  constexpr int VEC = 16 / sizeof(T);
  if (rows < 1 || V < 1 || V > (1 << 24) || ld < 1 || !ids || !table || !y) return hipErrorInvalidValue;
  if ((long long)V * ld > 0x7fffffffll || (long long)rows * ld > 0x7fffffffll) return hipErrorInvalidValue;
  if (ld % VEC == 0 && (((uintptr_t)table | (uintptr_t)y) & 15) == 0) {
    const int total = rows * (ld / VEC);
    hipLaunchKernelGGL((embedding_kernel<T, VEC>), dim3(grid_of(total)), dim3(256), 0, s, ids, table, y, V, ld, total);
  } else {
    const int total = rows * ld;
    hipLaunchKernelGGL((embedding_kernel<T, 1>), dim3(grid_of(total)), dim3(256), 0, s, ids, table, y, V, ld, total);
  }
  return hipGetLastError();
}
}  // namespace

hipError_t embedding_f32(const float* ids, const float* table, float* y, int rows, int V, int ld, hipStream_t s) {
  return embedding_launch<float>(ids, table, y, rows, V, ld, s);
}

hipError_t embedding_bf16(const float* ids, const bf16* table, bf16* y, int rows, int V, int ld, hipStream_t s) {
  return embedding_launch<bf16>(ids, table, y, rows, V, ld, s);
}

// Rotary position embedding (the rotate-half convention of Hugging Face Llama and keras_hub RotaryEmbedding) on
// the attention layer's projection buffer, out of place: x and y are [rows][ld] rows of [Q | K | V | padding], Q
// hq heads of d, K hkv heads of d, V hkv heads of dv.  For a Q or K head vector at position t = row % T (a batch
// restarts at 0 per image) and i in [0, d/2):
//
//   y[i] = x[i] cos(t, i) - x[i + d/2] sin(t, i),   y[i + d/2] = x[i + d/2] cos(t, i) + x[i] sin(t, i)
//
// cos and sin come from the fp32 table [2][T][d/2] that the host computed in float64 (ops/attention.py
// rope_table): the kernel evaluates no sinf / cosf, whose fp32 argument t * freq is already off by 5e-4 rad at
// t = 8192.  A thread owns one 16-byte vector of a head's first half, its partner vector at + d/2 and the matching
// cos and sin vectors, and writes both halves; the threads behind the rotated columns copy the V columns and
// write the columns from the true width to ld as zeros, so one launch writes every element of y.  Math is fp32,
// one rounding on a bf16 store.  VEC = 16 bytes per thread where d/2 and ld are multiples of it and the bases are
// aligned, else 1: every other even d.  Offsets are 32-bit: the launcher refuses what does not fit.
namespace {
template <typename T, int VEC>
struct RopeVec {
  float f[VEC];
};

template <typename T, int VEC>
__device__ __forceinline__ RopeVec<T, VEC> rope_ld(const T* p) {
  RopeVec<T, VEC> r;
  if constexpr (VEC == 1) {
    r.f[0] = (float)p[0];
  } else if constexpr (sizeof(T) == 4) {
    const f32x4 q = *(const f32x4*)p;
    r.f[0] = q.x; r.f[1] = q.y; r.f[2] = q.z; r.f[3] = q.w;
  } else {
    V8 q;
    q.u = *(const u32x4*)p;
#pragma unroll
    for (int e = 0; e < 8; ++e) r.f[e] = bf2f(q.e[e]);
  }
  return r;
}

template <typename T, int VEC>
__device__ __forceinline__ void rope_st(T* p, const RopeVec<T, VEC>& r) {
  if constexpr (VEC == 1) {
    p[0] = (T)r.f[0];
  } else if constexpr (sizeof(T) == 4) {
    *(f32x4*)p = f32x4{r.f[0], r.f[1], r.f[2], r.f[3]};
  } else {
    V8 q;
#pragma unroll
    for (int e = 0; e < 8; ++e) q.e[e] = f2bf(r.f[e]);
    *(u32x4*)p = q.u;
  }
}

// nrot: rotating threads per row ((hq + hkv) * half / VEC), ncopy: copying threads per row ((ld - rotw) / VEC);
// rotw = (hq + hkv) d, the first V column; W the true row width
template <typename T, int VEC>
__global__ __launch_bounds__(256) void rope_kernel(const T* __restrict__ x, const float* __restrict__ table,
                                                    T* __restrict__ y, int Tn, int half, int ld, int rotw, int W,
                                                    int nrot, int ncopy, int total) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int per = nrot + ncopy;
  const int row = idx / per, u = idx % per;
  const T* xr = x + row * ld;
  T* yr = y + row * ld;
  if (u < nrot) {
    const int hv = half / VEC;                        // vectors per half head
    const int head = u / hv, i = (u % hv) * VEC;
    const int col = head * 2 * half + i;
    const float* cs = table + (row % Tn) * half + i;  // cos; sin lies Tn * half further on
    const float* sn = cs + Tn * half;
    const RopeVec<T, VEC> a = rope_ld<T, VEC>(xr + col), b = rope_ld<T, VEC>(xr + col + half);
    RopeVec<T, VEC> oa, ob;
    if constexpr (VEC == 1) {
      const float c = cs[0], s = sn[0];
      oa.f[0] = a.f[0] * c - b.f[0] * s;
      ob.f[0] = b.f[0] * c + a.f[0] * s;
    } else {
#pragma unroll
      for (int v4 = 0; v4 < VEC / 4; ++v4) {
        const f32x4 c = ((const f32x4*)cs)[v4], s = ((const f32x4*)sn)[v4];
        const float cc[4] = {c.x, c.y, c.z, c.w}, ss[4] = {s.x, s.y, s.z, s.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          oa.f[4 * v4 + e] = a.f[4 * v4 + e] * cc[e] - b.f[4 * v4 + e] * ss[e];
          ob.f[4 * v4 + e] = b.f[4 * v4 + e] * cc[e] + a.f[4 * v4 + e] * ss[e];
        }
      }
    }
    rope_st<T, VEC>(yr + col, oa);
    rope_st<T, VEC>(yr + col + half, ob);
  } else {
    // V is copied as it stands (no arithmetic: bit-exact); the columns from W on are zeros, whatever x holds there
    const int col = rotw + (u - nrot) * VEC;
    if constexpr (VEC == 1) {
      yr[col] = col < W ? xr[col] : (T)0.f;
    } else {
      union { u32x4 u; T e[VEC]; } q;
      q.u = u32x4{0u, 0u, 0u, 0u};
      if (col < W) q.u = *(const u32x4*)(xr + col);
      if (col + VEC > W) {
#pragma unroll
        for (int e = 0; e < VEC; ++e)
          if (col + e >= W) q.e[e] = (T)0.f;
      }
      *(u32x4*)(yr + col) = q.u;
    }
  }
}

template <typename T>
hipError_t rope_launch(const T* x, const float* table, T* y, int rows, int Tn, int hq, int hkv, int d, int dv, int ld,
                       hipStream_t s) {
  constexpr int VEC = 16 / sizeof(T);
  if (rows < 1 || Tn < 1 || rows % Tn || hq < 1 || hkv < 1 || d < 2 || d % 2 || dv < 1 || !x || !table || !y || x == y)
    return hipErrorInvalidValue;
  const long long lim = 0x7fffffffll;
  const long long rotw = ((long long)hq + hkv) * d, W = rotw + (long long)hkv * dv;
  if (W > ld || (long long)rows * ld > lim || (long long)Tn * d > lim) return hipErrorInvalidValue;
  const int half = d / 2;
  const bool vec = half % VEC == 0 && ld % VEC == 0 &&
                   ((((uintptr_t)x | (uintptr_t)y) & 15) == 0) && (((uintptr_t)table & 15) == 0);
  const int v = vec ? VEC : 1;
  const int nrot = (int)(rotw / 2 / v), ncopy = (int)((ld - rotw) / v);
  if ((long long)rows * (nrot + ncopy) > lim) return hipErrorInvalidValue;
  const int total = rows * (nrot + ncopy);
  const dim3 grid((total + 255) / 256), block(256);
  if (vec)
    hipLaunchKernelGGL((rope_kernel<T, VEC>), grid, block, 0, s, x, table, y, Tn, half, ld, (int)rotw, (int)W, nrot,
                       ncopy, total);
  else
    hipLaunchKernelGGL((rope_kernel<T, 1>), grid, block, 0, s, x, table, y, Tn, half, ld, (int)rotw, (int)W, nrot,
                       ncopy, total);
  return hipGetLastError();
}
}  // namespace

hipError_t rope_f32(const float* x, const float* table, float* y, int rows, int T, int hq, int hkv, int d, int dv,
                    int ld, hipStream_t s) {
  return rope_launch<float>(x, table, y, rows, T, hq, hkv, d, dv, ld, s);
}

hipError_t rope_bf16(const bf16* x, const float* table, bf16* y, int rows, int T, int hq, int hkv, int d, int dv,
                     int ld, hipStream_t s) {
  return rope_launch<bf16>(x, table, y, rows, T, hq, hkv, d, dv, ld, s);
}

}  // namespace adapt
