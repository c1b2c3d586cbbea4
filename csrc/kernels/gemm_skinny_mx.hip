// Instantiations and launch checks of the MXFP4 skinny GEMM (gemm_skinny_mx.h): F in 1 / 2 / 4 / 8 channel
// fragments per block, one or two row fragments (M <= 16 / M <= 32).
#include "gemm_skinny_mx.h"
#include "kernels.h"

namespace adapt {

namespace {

template <int F, int MF>
hipError_t mx_launch(const SkinnyMxParams& p, int KS, hipStream_t s) {
  hipLaunchKernelGGL((gemm_skinny_mx_kernel<F, MF>), dim3((p.N + 16 * F - 1) / (16 * F), KS), dim3(256), 0, s, p);
  return hipGetLastError();
}

template <int F>
hipError_t mx_rows(const SkinnyMxParams& p, int KS, hipStream_t s) {
  return p.M > 16 ? mx_launch<F, 2>(p, KS, s) : mx_launch<F, 1>(p, KS, s);
}

}  // namespace

int gemm_skinny_mx_chunks(int Kpad) { return (Kpad + MX_KC - 1) / MX_KC; }

hipError_t gemm_skinny_mx(const bf16* x, const uint32_t* codes, const uint32_t* scales, const float* bias,
                          const bf16* res, bf16* out, float* ws, int* counters, int M, int N, int K, int Kpad,
                          int Npad, int act, int F, int KS, hipStream_t s) {
  const SkinnyMxParams p{x, codes, scales, bias, res, out, ws, counters, M, N, K, Kpad, act};
  if (M < 1 || M > 32 || N < 1 || K < 1 || K % 8 || N % 8 || Kpad % MX_KC || Kpad < K ||
      (F != 1 && F != 2 && F != 4 && F != 8) || act < 0 || act > 2)
    return hipErrorInvalidValue;
  if (Npad < (N + 16 * F - 1) / (16 * F) * (16 * F)) return hipErrorInvalidValue;       // whole fragments are read
  if (KS < 1 || KS > gemm_skinny_mx_chunks(Kpad)) return hipErrorInvalidValue;          // no empty split
  if (KS > 1 && (!ws || !counters || (long long)KS * M * N * 4 > 0x7fffffffLL)) return hipErrorInvalidValue;
  if (!x || !codes || !scales || !bias || !out) return hipErrorInvalidValue;
  const uintptr_t al = (uintptr_t)x | (uintptr_t)codes | (uintptr_t)bias | (uintptr_t)ws;
  if (al % 16 || (uintptr_t)scales % 4 || ((uintptr_t)res | (uintptr_t)out) % 8) return hipErrorInvalidValue;
  switch (F) {
    case 1: return mx_rows<1>(p, KS, s);
    case 2: return mx_rows<2>(p, KS, s);
    case 4: return mx_rows<4>(p, KS, s);
    default: return mx_rows<8>(p, KS, s);
  }
}

}  // namespace adapt
