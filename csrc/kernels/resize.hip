// UpSampling2D (nearest / bilinear), Cropping2D and Swin's space-to-depth (described at its kernel below), NHWC,
// fp32 and bf16, for gfx950.
//
//   nearest   y[b][oy][ox][c] = x[b][oy / SH][ox / SW][c]                                    (a bit-exact copy)
//   bilinear  tf.image.resize with half-pixel centres: fy = max((oy + 0.5) / SH - 0.5, 0), y0 = floor(fy),
//             y1 = min(y0 + 1, H - 1), weight fy - y0, the x axis alike; the row and column weights are
//             computed in fp32 from the output row / column, the four taps blended in fp32
//   crop      y[b][oy][ox][c] = x[b][oy + T][ox + L][c]                                     (a bit-exact copy)
//
// Memory-bound copies: one thread moves one 16-byte vector (4 fp32 or 8 bf16 channels of one output pixel)
// when the row width allows it, C % 4 == 0 for fp32 and always for bf16, whose rows are Cp = C padded to 8;
// every other fp32 width, or a base that is not 16-byte aligned, takes the scalar kernel, one thread per
// element.  Index math is 32-bit: the launchers refuse a tensor of 2^31 or more elements.  A source index is
// always derived from an in-range output index and clamped to the map, so nothing outside x is read.
// bf16 padding channels C..Cp-1 never enter the arithmetic and are written as zeros.  No workspace, no host
// sync: one launch on the caller's stream (graph-capturable).
#include "kernels.h"

namespace adapt {

namespace {

constexpr int RS_NT = 256;

struct ResizeGeom {
  int B, H, W, OH, OW;
  int SH, SW;        // upsample factors (mode 0 / 1)
  int T, L;          // crop offsets (mode 2)
  int mode;          // 0 nearest, 1 bilinear, 2 crop
};

struct Taps {
  int i0, i1;
  float w;
};

__device__ __forceinline__ Taps bilinear_taps(int o, int s, int size) {
  const float f = fmaxf(((float)o + 0.5f) / (float)s - 0.5f, 0.f);
  Taps t;
  t.i0 = min((int)f, size - 1);
  t.i1 = min(t.i0 + 1, size - 1);
  t.w = f - (float)t.i0;
  return t;
}

__device__ __forceinline__ float blend(float a, float b, float c, float d, float wx, float wy) {
  const float top = a + (b - a) * wx, bot = c + (d - c) * wx;
  return top + (bot - top) * wy;
}

// source pixel of a copy mode (nearest / crop)
__device__ __forceinline__ int src_pixel(const ResizeGeom& g, int img, int oy, int ox) {
  const int iy = g.mode == 2 ? oy + g.T : oy / g.SH, ix = g.mode == 2 ? ox + g.L : ox / g.SW;
  return (img * g.H + iy) * g.W + ix;
}

// VEC = true: one thread per 4-channel vector (C % 4 == 0); false: one thread per element
template <bool VEC>
__global__ __launch_bounds__(RS_NT) void resize_f32_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                          ResizeGeom g, int C, int total) {
  const int idx = blockIdx.x * RS_NT + threadIdx.x;
  if (idx >= total) return;
  const int per = VEC ? C >> 2 : C;
  const int cv = idx % per;
  int pix = idx / per;
  const int ox = pix % g.OW;
  pix /= g.OW;
  const int oy = pix % g.OH, img = pix / g.OH;
  if (g.mode != 1) {
    const int sp = src_pixel(g, img, oy, ox);
    if (VEC) ((f32x4*)y)[idx] = ((const f32x4*)x)[sp * per + cv];
    else y[idx] = x[sp * per + cv];
    return;
  }
  const Taps ty = bilinear_taps(oy, g.SH, g.H), tx = bilinear_taps(ox, g.SW, g.W);
  const int r0 = (img * g.H + ty.i0) * g.W, r1 = (img * g.H + ty.i1) * g.W;
  const int a = (r0 + tx.i0) * per + cv, b = (r0 + tx.i1) * per + cv, c = (r1 + tx.i0) * per + cv,
            d = (r1 + tx.i1) * per + cv;
  if (VEC) {
    const f32x4 va = ((const f32x4*)x)[a], vb = ((const f32x4*)x)[b], vc = ((const f32x4*)x)[c],
                vd = ((const f32x4*)x)[d];
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = blend(va[e], vb[e], vc[e], vd[e], tx.w, ty.w);
    ((f32x4*)y)[idx] = o;
  } else {
    y[idx] = blend(x[a], x[b], x[c], x[d], tx.w, ty.w);
  }
}

// one thread per 8-channel vector of a Cp-wide row; channels >= C are written as zeros
__global__ __launch_bounds__(RS_NT) void resize_bf16_kernel(const bf16* __restrict__ x, bf16* __restrict__ y,
                                                           ResizeGeom g, int Cp, int C, int total) {
  const int idx = blockIdx.x * RS_NT + threadIdx.x;
  if (idx >= total) return;
  const int per = Cp >> 3;
  const int cv = idx % per;
  int pix = idx / per;
  const int ox = pix % g.OW;
  pix /= g.OW;
  const int oy = pix % g.OH, img = pix / g.OH;
  V8 o;
  if (g.mode != 1) {
    o.u = ((const u32x4*)x)[src_pixel(g, img, oy, ox) * per + cv];
  } else {
    const Taps ty = bilinear_taps(oy, g.SH, g.H), tx = bilinear_taps(ox, g.SW, g.W);
    const int r0 = (img * g.H + ty.i0) * g.W, r1 = (img * g.H + ty.i1) * g.W;
    V8 va, vb, vc, vd;
    va.u = ((const u32x4*)x)[(r0 + tx.i0) * per + cv];
    vb.u = ((const u32x4*)x)[(r0 + tx.i1) * per + cv];
    vc.u = ((const u32x4*)x)[(r1 + tx.i0) * per + cv];
    vd.u = ((const u32x4*)x)[(r1 + tx.i1) * per + cv];
#pragma unroll
    for (int e = 0; e < 8; ++e)
      o.e[e] = f2bf(blend(bf2f(va.e[e]), bf2f(vb.e[e]), bf2f(vc.e[e]), bf2f(vd.e[e]), tx.w, ty.w));
  }
#pragma unroll
  for (int e = 0; e < 8; ++e)
    if (cv * 8 + e >= C) o.e[e] = f2bf(0.f);
  ((u32x4*)y)[idx] = o.u;
}

bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

// mode 0 / 1: OH = H * SH, OW = W * SW; mode 2: the window (T, L) + (OH, OW) lies inside (H, W)
bool geom_ok(const ResizeGeom& g, int rowc) {
  if (g.B < 1 || g.H < 1 || g.W < 1 || g.OH < 1 || g.OW < 1 || rowc < 1) return false;
  if (g.mode == 2) {
    if (g.T < 0 || g.L < 0 || g.T + g.OH > g.H || g.L + g.OW > g.W) return false;
  } else if (g.SH < 1 || g.SW < 1 || (long)g.H * g.SH != g.OH || (long)g.W * g.SW != g.OW) {
    return false;
  }
  return (double)g.B * g.OH * g.OW * rowc < 2147483648.0 && (double)g.B * g.H * g.W * rowc < 2147483648.0;
}

hipError_t resize_f32(const float* x, float* y, const ResizeGeom& g, int C, hipStream_t s) {
  if (!geom_ok(g, C)) return hipErrorInvalidValue;
  const bool vec = C % 4 == 0 && aligned16(x) && aligned16(y);
  const int total = g.B * g.OH * g.OW * (vec ? C / 4 : C);
  const dim3 grid((unsigned)((total + RS_NT - 1) / RS_NT));
  if (vec) hipLaunchKernelGGL(resize_f32_kernel<true>, grid, dim3(RS_NT), 0, s, x, y, g, C, total);
  else hipLaunchKernelGGL(resize_f32_kernel<false>, grid, dim3(RS_NT), 0, s, x, y, g, C, total);
  return hipGetLastError();
}

hipError_t resize_bf16(const bf16* x, bf16* y, const ResizeGeom& g, int Cp, int C, hipStream_t s) {
  if (!geom_ok(g, Cp) || Cp % 8 || C < 1 || C > Cp || !aligned16(x) || !aligned16(y)) return hipErrorInvalidValue;
  const int total = g.B * g.OH * g.OW * (Cp / 8);
  const dim3 grid((unsigned)((total + RS_NT - 1) / RS_NT));
  hipLaunchKernelGGL(resize_bf16_kernel, grid, dim3(RS_NT), 0, s, x, y, g, Cp, C, total);
  return hipGetLastError();
}

// Swin patch merging's rearrangement: y[b][oy][ox][(2 dx + dy) C + c] = x[b][2 oy + dy][2 ox + dx][c], a bit-exact
// copy.  x rows are ldx wide with C true channels, y rows ldy wide with 4 C true channels, contiguous; the rest
// of a y row is written as zeros and the padding of x is never read.  VEC: one thread per 16-byte vector (C a
// multiple of the vector, so a vector never straddles two source pixels and there is no padding); otherwise one
// thread per element of y.
template <typename T, bool VEC>
__global__ __launch_bounds__(RS_NT) void space_to_depth_kernel(const T* __restrict__ x, T* __restrict__ y, int H,
                                                               int W, int C, int ldx, int ldy, int total) {
  constexpr int N = VEC ? 16 / (int)sizeof(T) : 1;
  const int idx = blockIdx.x * RS_NT + threadIdx.x;
  if (idx >= total) return;
  const int per = ldy / N;
  const int c0 = (idx % per) * N;
  int pix = idx / per;
  const int OW = W >> 1, OH = H >> 1;
  const int ox = pix % OW;
  pix /= OW;
  const int oy = pix % OH, img = pix / OH;
  if (c0 >= 4 * C) {                                  // layout padding of the output row (scalar path only)
    y[idx] = T(0.f);
    return;
  }
  const int blk = c0 / C, c = c0 - blk * C;
  const int src = ((img * H + 2 * oy + (blk & 1)) * W + 2 * ox + (blk >> 1)) * ldx + c;
  if (VEC) ((u32x4*)y)[idx] = *(const u32x4*)(x + src);
  else y[idx] = x[src];
}

template <typename T>
hipError_t space_to_depth_launch(const T* x, T* y, int B, int H, int W, int C, int ldx, int ldy, hipStream_t s) {
  constexpr int N = 16 / (int)sizeof(T);
  if (B < 1 || H < 2 || W < 2 || H % 2 || W % 2 || C < 1 || ldx < C || (long)ldy < 4l * C) return hipErrorInvalidValue;
  if ((double)B * H * W * ldx >= 2147483648.0 || (double)B * (H / 2) * (W / 2) * ldy >= 2147483648.0)
    return hipErrorInvalidValue;
  const bool vec = C % N == 0 && ldx == C && ldy == 4 * C && aligned16(x) && aligned16(y);
  const int total = B * (H / 2) * (W / 2) * (vec ? ldy / N : ldy);
  const dim3 grid((unsigned)((total + RS_NT - 1) / RS_NT));
  if (vec) hipLaunchKernelGGL((space_to_depth_kernel<T, true>), grid, dim3(RS_NT), 0, s, x, y, H, W, C, ldx, ldy, total);
  else hipLaunchKernelGGL((space_to_depth_kernel<T, false>), grid, dim3(RS_NT), 0, s, x, y, H, W, C, ldx, ldy, total);
  return hipGetLastError();
}

}  // namespace

hipError_t space_to_depth_f32(const float* x, float* y, int B, int H, int W, int C, hipStream_t s) {
  return space_to_depth_launch<float>(x, y, B, H, W, C, C, 4 * C, s);
}

hipError_t space_to_depth_bf16(const bf16* x, bf16* y, int B, int H, int W, int Cpx, int Cpy, int C, hipStream_t s) {
  return space_to_depth_launch<bf16>(x, y, B, H, W, C, Cpx, Cpy, s);
}

hipError_t upsample_f32(const float* x, float* y, int B, int H, int W, int C, int SH, int SW, int bilinear,
                        hipStream_t s) {
  if (SH < 1 || SW < 1 || (long)H * SH > 0x7fffffff || (long)W * SW > 0x7fffffff) return hipErrorInvalidValue;
  return resize_f32(x, y, ResizeGeom{B, H, W, H * SH, W * SW, SH, SW, 0, 0, bilinear ? 1 : 0}, C, s);
}

hipError_t upsample_bf16(const bf16* x, bf16* y, int B, int H, int W, int Cp, int C, int SH, int SW, int bilinear,
                         hipStream_t s) {
  if (SH < 1 || SW < 1 || (long)H * SH > 0x7fffffff || (long)W * SW > 0x7fffffff) return hipErrorInvalidValue;
  return resize_bf16(x, y, ResizeGeom{B, H, W, H * SH, W * SW, SH, SW, 0, 0, bilinear ? 1 : 0}, Cp, C, s);
}

hipError_t crop_f32(const float* x, float* y, int B, int H, int W, int C, int OH, int OW, int T, int L, hipStream_t s) {
  return resize_f32(x, y, ResizeGeom{B, H, W, OH, OW, 1, 1, T, L, 2}, C, s);
}

hipError_t crop_bf16(const bf16* x, bf16* y, int B, int H, int W, int Cp, int C, int OH, int OW, int T, int L,
                     hipStream_t s) {
  return resize_bf16(x, y, ResizeGeom{B, H, W, OH, OW, 1, 1, T, L, 2}, Cp, C, s);
}

}  // namespace adapt
