// LayerNormalization over the last axis (Keras semantics), fp32 and bf16, gfx950.
//
//   mu = mean_c(x), var = mean_c((x - mu)^2) (biased), y = (x - mu) * rsqrt(var + eps) * gamma[c] + beta[c]
//
// x is [rows][C] fp32 or [rows][Cp] bf16 (Cp = C padded to a multiple of 8; the padding channels are layout,
// not data).  Memory-bound: the register path reads a row once with 16-byte loads (float4, or 8 bf16 per lane:
// cdna_hip_programming.md Guideline 13), keeps it in registers through both statistics and writes it once with
// 16-byte stores.  The statistics are two-pass in fp32 (the mean, then the centred sum of squares; never
// E[x^2] - mu^2, which loses every digit on a row such as mean 100 / sigma 0.1).  Cross-lane sums are
// `__shfl_xor` butterflies inside the wave: no LDS, no barrier, no atomics, no workspace, so the launch is
// graph-capturable like every other step.
//
// Rows per wave.  A row is spread over LPR lanes (a power of two) and a wave covers 64 / LPR rows; lane l of a
// row's group holds the 16-byte vectors l, l + LPR, ... (VPL of them), so every load instruction of the group
// is one contiguous run.  With nvec = C / 4 (fp32) or Cp / 8 (bf16) vectors per row the split is
//
//     nvec <=  16: LPR  8, VPL 2   (8 rows per wave)          nvec <= 128: LPR 64, VPL 2   (1 row per wave)
//     nvec <=  32: LPR 16, VPL 2   (4 rows per wave)          nvec <= 256: LPR 64, VPL 4
//     nvec <=  64: LPR 32, VPL 2   (2 rows per wave)          nvec <= 512: LPR 64, VPL 8
//
// i.e. the fewest lanes per row that keep a lane at two vectors: ConvNeXt's C = 96 map (24 fp32 vectors) runs 4
// rows per wave with 24 of 32 vector slots used (8 rows per wave in bf16, 12 of 16 slots), where one row per wave
// would leave 40 of 64 lanes idle and pay a 6-step butterfly instead of a 4- or 3-step one; two independent
// loads per lane are in flight before the first use.  Measured on the 100352 x 96 bf16 map, 8 lanes x 2 vectors
// and 16 lanes x 1 vector are within 3 % of each other (9.99 against 10.28 us), so the one rule is kept for all
// widths.  From C = 384 fp32 / Cp = 768 bf16 on a row fills the wave and VPL grows instead, up to 32 (fp32)
// or 64 (bf16) data registers per lane.  A block is 4 waves; rows past `rows` in the last block are masked
// lane by lane (the lanes still take part in the butterflies).
//
// Every other shape takes the looped path, one wave per row with scalar accesses and three sweeps over the row
// (mean, centred squares, output; the second and third come from L2): C % 4 != 0 or a base that is not 16-byte
// aligned (fp32), and nvec > 512, i.e. C > 2048 fp32 / Cp > 4096 bf16, where the row no longer fits registers.
//
// bf16 padding channels C..Cp-1 are excluded from both statistics (the divisor is C), never enter the
// arithmetic whatever they hold (NaN / inf in the pads cannot reach a real channel), and are written as zeros.
#include "kernels.h"

namespace adapt {
namespace {

constexpr int LN_WAVES = 4;          // waves per block
constexpr int LN_MAX_NVEC = 512;     // 16-byte vectors per row the register path holds (LPR 64 x VPL 8)

template <int W>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = W / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <int LPR, int VPL>
__global__ __launch_bounds__(64 * LN_WAVES) void layernorm_f32_kernel(const float* __restrict__ x,
                                                                       const float* __restrict__ gamma,
                                                                       const float* __restrict__ beta,
                                                                       float* __restrict__ y, int rows, int C,
                                                                       float eps) {
  constexpr int RPW = 64 / LPR;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane & (LPR - 1);
  const long row = ((long)blockIdx.x * LN_WAVES + wave) * RPW + lane / LPR;
  const int nvec = C >> 2;
  const bool live = row < rows;
  const f32x4* xr = (const f32x4*)(x + (size_t)(live ? row : 0) * C);
  f32x4 v[VPL];
  bool has[VPL];
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int j = sub + i * LPR;
    has[i] = live && j < nvec;
    v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (has[i]) v[i] = xr[j];
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
  const float mu = group_sum<LPR>(s) / (float)C;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    v[i] -= mu;                                   // lanes without a vector hold -mu: masked out below
    const float d = (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
    q += has[i] ? d : 0.f;
  }
  const float rstd = 1.f / sqrtf(group_sum<LPR>(q) / (float)C + eps);
  f32x4* yr = (f32x4*)(y + (size_t)(live ? row : 0) * C);
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int j = sub + i * LPR;
    if (has[i]) yr[j] = v[i] * rstd * ((const f32x4*)gamma)[j] + ((const f32x4*)beta)[j];
  }
}

template <int LPR, int VPL>
__global__ __launch_bounds__(64 * LN_WAVES) void layernorm_bf16_kernel(const bf16* __restrict__ x,
                                                                        const float* __restrict__ gamma,
                                                                        const float* __restrict__ beta,
                                                                        bf16* __restrict__ y, int rows, int Cp, int C,
                                                                        float eps) {
  constexpr int RPW = 64 / LPR;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane & (LPR - 1);
  const long row = ((long)blockIdx.x * LN_WAVES + wave) * RPW + lane / LPR;
  const int nvec = Cp >> 3;
  const bool live = row < rows;
  const u32x4* xr = (const u32x4*)(x + (size_t)(live ? row : 0) * Cp);
  float f[VPL][8];
  bool has[VPL];
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int j = sub + i * LPR;
    has[i] = live && j < nvec;
    V8 t;
    t.u = u32x4{0u, 0u, 0u, 0u};
    if (has[i]) t.u = xr[j];
#pragma unroll
    for (int e = 0; e < 8; ++e) f[i][e] = (has[i] && j * 8 + e < C) ? bf2f(t.e[e]) : 0.f;    // pads never enter
  }
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i)
    s += ((f[i][0] + f[i][1]) + (f[i][2] + f[i][3])) + ((f[i][4] + f[i][5]) + (f[i][6] + f[i][7]));
  const float mu = group_sum<LPR>(s) / (float)C;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int j = sub + i * LPR;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      f[i][e] -= mu;
      q += (has[i] && j * 8 + e < C) ? f[i][e] * f[i][e] : 0.f;
    }
  }
  const float rstd = 1.f / sqrtf(group_sum<LPR>(q) / (float)C + eps);
  u32x4* yr = (u32x4*)(y + (size_t)(live ? row : 0) * Cp);
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int j = sub + i * LPR;
    if (!has[i]) continue;
    const f32x4 g0 = ((const f32x4*)gamma)[2 * j], g1 = ((const f32x4*)gamma)[2 * j + 1];
    const f32x4 b0 = ((const f32x4*)beta)[2 * j], b1 = ((const f32x4*)beta)[2 * j + 1];
    const float g[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
    const float b[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
    V8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o.e[e] = f2bf(j * 8 + e < C ? f[i][e] * rstd * g[e] + b[e] : 0.f);
    yr[j] = o.u;
  }
}

__device__ __forceinline__ float ln_ld(const float* p) { return *p; }
__device__ __forceinline__ float ln_ld(const bf16* p) { return bf2f(*p); }
__device__ __forceinline__ void ln_st(float* p, float v) { *p = v; }
__device__ __forceinline__ void ln_st(bf16* p, float v) { *p = f2bf(v); }

// Any C, any alignment: one wave per row, scalar accesses, the row swept three times.  gamma / beta hold C values
// at least; channels C..Cp-1 of the output are written as zeros and never read.
template <typename T>
__global__ __launch_bounds__(64 * LN_WAVES) void layernorm_loop_kernel(const T* __restrict__ x,
                                                                        const float* __restrict__ gamma,
                                                                        const float* __restrict__ beta,
                                                                        T* __restrict__ y, int rows, int Cp, int C,
                                                                        float eps) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * LN_WAVES + (threadIdx.x >> 6);
  if (row >= rows) return;                        // the whole wave leaves together
  const T* xr = x + (size_t)row * Cp;
  T* yr = y + (size_t)row * Cp;
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += ln_ld(xr + c);
  const float mu = group_sum<64>(s) / (float)C;
  float q = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float d = ln_ld(xr + c) - mu;
    q += d * d;
  }
  const float rstd = 1.f / sqrtf(group_sum<64>(q) / (float)C + eps);
  for (int c = lane; c < C; c += 64) ln_st(yr + c, (ln_ld(xr + c) - mu) * rstd * gamma[c] + beta[c]);
  for (int c = C + lane; c < Cp; c += 64) ln_st(yr + c, 0.f);
}

inline bool aligned16(const void* a, const void* b, const void* c, const void* d) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

inline int blocks_for(int rows, int rows_per_block) { return (rows + rows_per_block - 1) / rows_per_block; }

}  // namespace

// lanes per row the register path uses for a row of `nvec` 16-byte vectors; 0: the looped path
int layernorm_lanes(int nvec) {
  if (nvec < 1 || nvec > LN_MAX_NVEC) return 0;
  return nvec <= 16 ? 8 : nvec <= 32 ? 16 : nvec <= 64 ? 32 : 64;
}

#define LN_LAUNCH(KERNEL, LPR, VPL, ...)                                                                \
  hipLaunchKernelGGL((KERNEL<LPR, VPL>), dim3(blocks_for(rows, LN_WAVES * (64 / LPR))), dim3(64 * LN_WAVES), 0, s, \
                     __VA_ARGS__)

#define LN_DISPATCH(KERNEL, nvec, ...)                        \
  do {                                                        \
    if (nvec <= 16) LN_LAUNCH(KERNEL, 8, 2, __VA_ARGS__);     \
    else if (nvec <= 32) LN_LAUNCH(KERNEL, 16, 2, __VA_ARGS__); \
    else if (nvec <= 64) LN_LAUNCH(KERNEL, 32, 2, __VA_ARGS__); \
    else if (nvec <= 128) LN_LAUNCH(KERNEL, 64, 2, __VA_ARGS__); \
    else if (nvec <= 256) LN_LAUNCH(KERNEL, 64, 4, __VA_ARGS__); \
    else LN_LAUNCH(KERNEL, 64, 8, __VA_ARGS__);               \
  } while (0)

hipError_t layernorm_f32(const float* x, const float* gamma, const float* beta, float* y, int rows, int C, float eps,
                         hipStream_t s) {
  if (rows < 1 || C < 1) return hipErrorInvalidValue;
  if (C % 4 == 0 && C / 4 <= LN_MAX_NVEC && aligned16(x, gamma, beta, y)) {
    const int nvec = C / 4;
    LN_DISPATCH(layernorm_f32_kernel, nvec, x, gamma, beta, y, rows, C, eps);
  } else {
    hipLaunchKernelGGL(layernorm_loop_kernel<float>, dim3(blocks_for(rows, LN_WAVES)), dim3(64 * LN_WAVES), 0, s, x,
                       gamma, beta, y, rows, C, C, eps);
  }
  return hipGetLastError();
}

// gamma / beta: Cp floats (the register path loads whole vectors of them; their padding values are not used)
hipError_t layernorm(const bf16* x, const float* gamma, const float* beta, bf16* y, int rows, int Cp, int C, float eps,
                     hipStream_t s) {
  if (rows < 1 || C < 1 || Cp < C || Cp % 8) return hipErrorInvalidValue;
  if (Cp / 8 <= LN_MAX_NVEC && aligned16(x, gamma, beta, y)) {
    const int nvec = Cp / 8;
    LN_DISPATCH(layernorm_bf16_kernel, nvec, x, gamma, beta, y, rows, Cp, C, eps);
  } else {
    hipLaunchKernelGGL(layernorm_loop_kernel<bf16>, dim3(blocks_for(rows, LN_WAVES)), dim3(64 * LN_WAVES), 0, s, x,
                       gamma, beta, y, rows, Cp, C, eps);
  }
  return hipGetLastError();
}

// RMSNormalization over the last axis (Keras 3 semantics; the norm of every Llama-family model):
//
//   y = x * rsqrt(mean_c(x^2) + eps) * scale[c]
//
// The scheme above with kernels of their own, so the layernorm kernels stay the instructions they are: the same
// rows-per-wave split, a row read once with 16-byte loads, kept in registers and written once, `__shfl_xor` sums
// only.  There is no mean to subtract, so one pass of statistics (the sum of squares, in fp32) is all there is:
// the cancellation that forces layernorm's second pass cannot arise in a sum of non-negative terms.  The looped
// path (fp32 C % 4 != 0, a misaligned base, more than 512 vectors per row) sweeps the row twice.  bf16 padding
// channels stay out of the sum (the divisor is C) and are written as zeros.
namespace {

template <int LPR, int VPL>
__global__ __launch_bounds__(64 * LN_WAVES) void rmsnorm_f32_kernel(const float* __restrict__ x,
                                                                     const float* __restrict__ scale,
                                                                     float* __restrict__ y, int rows, int C,
                                                                     float eps) {
  constexpr int RPW = 64 / LPR;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane & (LPR - 1);
  const long row = ((long)blockIdx.x * LN_WAVES + wave) * RPW + lane / LPR;
  const int nvec = C >> 2;
  const bool live = row < rows;
  const f32x4* xr = (const f32x4*)(x + (size_t)(live ? row : 0) * C);
  f32x4 v[VPL];
  bool has[VPL];
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int j = sub + i * LPR;
    has[i] = live && j < nvec;
    v[i] = f32x4{0.f, 0.f, 0.f, 0.f};                 // lanes without a vector add zeros
    if (has[i]) v[i] = xr[j];
  }
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) q += (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
  const float rstd = 1.f / sqrtf(group_sum<LPR>(q) / (float)C + eps);
  f32x4* yr = (f32x4*)(y + (size_t)(live ? row : 0) * C);
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int j = sub + i * LPR;
    if (has[i]) yr[j] = v[i] * rstd * ((const f32x4*)scale)[j];
  }
}

template <int LPR, int VPL>
__global__ __launch_bounds__(64 * LN_WAVES) void rmsnorm_bf16_kernel(const bf16* __restrict__ x,
                                                                      const float* __restrict__ scale,
                                                                      bf16* __restrict__ y, int rows, int Cp, int C,
                                                                      float eps) {
  constexpr int RPW = 64 / LPR;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane & (LPR - 1);
  const long row = ((long)blockIdx.x * LN_WAVES + wave) * RPW + lane / LPR;
  const int nvec = Cp >> 3;
  const bool live = row < rows;
  const u32x4* xr = (const u32x4*)(x + (size_t)(live ? row : 0) * Cp);
  float f[VPL][8];
  bool has[VPL];
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int j = sub + i * LPR;
    has[i] = live && j < nvec;
    V8 t;
    t.u = u32x4{0u, 0u, 0u, 0u};
    if (has[i]) t.u = xr[j];
#pragma unroll
    for (int e = 0; e < 8; ++e) f[i][e] = (has[i] && j * 8 + e < C) ? bf2f(t.e[e]) : 0.f;    // pads never enter
  }
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i)
    q += ((f[i][0] * f[i][0] + f[i][1] * f[i][1]) + (f[i][2] * f[i][2] + f[i][3] * f[i][3])) +
         ((f[i][4] * f[i][4] + f[i][5] * f[i][5]) + (f[i][6] * f[i][6] + f[i][7] * f[i][7]));
  const float rstd = 1.f / sqrtf(group_sum<LPR>(q) / (float)C + eps);
  u32x4* yr = (u32x4*)(y + (size_t)(live ? row : 0) * Cp);
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int j = sub + i * LPR;
    if (!has[i]) continue;
    const f32x4 g0 = ((const f32x4*)scale)[2 * j], g1 = ((const f32x4*)scale)[2 * j + 1];
    const float g[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
    V8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o.e[e] = f2bf(j * 8 + e < C ? f[i][e] * rstd * g[e] : 0.f);
    yr[j] = o.u;
  }
}

// Any C, any alignment: one wave per row, scalar accesses, the row swept twice.  scale holds C values at least;
// channels C..Cp-1 of the output are written as zeros and never read.
template <typename T>
__global__ __launch_bounds__(64 * LN_WAVES) void rmsnorm_loop_kernel(const T* __restrict__ x,
                                                                      const float* __restrict__ scale,
                                                                      T* __restrict__ y, int rows, int Cp, int C,
                                                                      float eps) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * LN_WAVES + (threadIdx.x >> 6);
  if (row >= rows) return;                        // the whole wave leaves together
  const T* xr = x + (size_t)row * Cp;
  T* yr = y + (size_t)row * Cp;
  float q = 0.f;
  for (int c = lane; c < C; c += 64) {
    const float v = ln_ld(xr + c);
    q += v * v;
  }
  const float rstd = 1.f / sqrtf(group_sum<64>(q) / (float)C + eps);
  for (int c = lane; c < C; c += 64) ln_st(yr + c, ln_ld(xr + c) * rstd * scale[c]);
  for (int c = C + lane; c < Cp; c += 64) ln_st(yr + c, 0.f);
}

}  // namespace

hipError_t rmsnorm_f32(const float* x, const float* scale, float* y, int rows, int C, float eps, hipStream_t s) {
  if (rows < 1 || C < 1) return hipErrorInvalidValue;
  if (C % 4 == 0 && C / 4 <= LN_MAX_NVEC && aligned16(x, scale, scale, y)) {
    const int nvec = C / 4;
    LN_DISPATCH(rmsnorm_f32_kernel, nvec, x, scale, y, rows, C, eps);
  } else {
    hipLaunchKernelGGL(rmsnorm_loop_kernel<float>, dim3(blocks_for(rows, LN_WAVES)), dim3(64 * LN_WAVES), 0, s, x,
                       scale, y, rows, C, C, eps);
  }
  return hipGetLastError();
}

// scale: Cp floats (the register path loads whole vectors of it; its padding values are not used)
hipError_t rmsnorm_bf16(const bf16* x, const float* scale, bf16* y, int rows, int Cp, int C, float eps,
                        hipStream_t s) {
  if (rows < 1 || C < 1 || Cp < C || Cp % 8) return hipErrorInvalidValue;
  if (Cp / 8 <= LN_MAX_NVEC && aligned16(x, scale, scale, y)) {
    const int nvec = Cp / 8;
    LN_DISPATCH(rmsnorm_bf16_kernel, nvec, x, scale, y, rows, Cp, C, eps);
  } else {
    hipLaunchKernelGGL(rmsnorm_loop_kernel<bf16>, dim3(blocks_for(rows, LN_WAVES)), dim3(64 * LN_WAVES), 0, s, x,
                       scale, y, rows, Cp, C, eps);
  }
  return hipGetLastError();
}

}  // namespace adapt
