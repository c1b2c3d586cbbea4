// Instantiations and launch checks of the skinny GEMM (gemm_skinny.h): F in 1 / 2 / 4 channel fragments per
// block, one or two row fragments (M <= 16 / M <= 32), fp32 and bf16.
#include "gemm_skinny.h"
#include "kernels.h"

namespace adapt {

namespace {

template <typename T, int F, int MF>
hipError_t sk_launch(const SkinnyParams<T>& p, int KS, hipStream_t s) {
  hipLaunchKernelGGL((gemm_skinny_kernel<T, F, MF>), dim3((p.N + 16 * F - 1) / (16 * F), KS), dim3(256), 0, s, p);
  return hipGetLastError();
}

template <typename T, int F>
hipError_t sk_rows(const SkinnyParams<T>& p, int KS, hipStream_t s) {
  return p.M > 16 ? sk_launch<T, F, 2>(p, KS, s) : sk_launch<T, F, 1>(p, KS, s);
}

template <typename T>
hipError_t sk_forward(const SkinnyParams<T>& p, int Npad, int F, int KS, hipStream_t s) {
  constexpr int VEC = SkinnyType<T>::VEC;
  if (p.M < 1 || p.M > 32 || p.N < 1 || p.K < 1 || p.K % VEC || p.N % VEC || p.Kpad % VEC || p.Kpad < p.K ||
      (F != 1 && F != 2 && F != 4) || p.act < 0 || p.act > 2)
    return hipErrorInvalidValue;
  if (Npad < (p.N + 16 * F - 1) / (16 * F) * (16 * F)) return hipErrorInvalidValue;     // whole fragments are read
  if (KS < 1 || KS > gemm_skinny_chunks(p.Kpad, (int)sizeof(T))) return hipErrorInvalidValue;    // no empty split
  if (KS > 1 && (!p.ws || !p.counters || (long long)KS * p.M * p.N * 4 > 0x7fffffffLL)) return hipErrorInvalidValue;
  const uintptr_t al = (uintptr_t)p.x | (uintptr_t)p.w | (uintptr_t)p.bias | (uintptr_t)p.ws;
  if (al % 16 || ((uintptr_t)p.res | (uintptr_t)p.out) % (4 * sizeof(T))) return hipErrorInvalidValue;
  switch (F) {
    case 1: return sk_rows<T, 1>(p, KS, s);
    case 2: return sk_rows<T, 2>(p, KS, s);
    default: return sk_rows<T, 4>(p, KS, s);
  }
}

}  // namespace

int gemm_skinny_chunks(int Kpad, int elem_size) {
  const int kc = 256 / elem_size;
  return (Kpad + kc - 1) / kc;
}

hipError_t gemm_skinny_f32(const float* x, const float* w, const float* bias, const float* res, float* out,
                           float* ws, int* counters, int M, int N, int K, int Kpad, int Npad, int act, int F,
                           int KS, hipStream_t s) {
  return sk_forward(SkinnyParams<float>{x, w, bias, res, out, ws, counters, M, N, K, Kpad, act}, Npad, F, KS, s);
}

hipError_t gemm_skinny_bf16(const bf16* x, const bf16* w, const float* bias, const bf16* res, bf16* out, float* ws,
                            int* counters, int M, int N, int K, int Kpad, int Npad, int act, int F, int KS,
                            hipStream_t s) {
  return sk_forward(SkinnyParams<bf16>{x, w, bias, res, out, ws, counters, M, N, K, Kpad, act}, Npad, F, KS, s);
}

}  // namespace adapt
