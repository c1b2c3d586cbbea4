// Instantiations and launch checks of the MXFP4 tile GEMM (gemm_tile_mx.h): (F, MT) = (4, 8), (2, 4), (1, 4), that
// is 256 x 128, 128 x 64 and 64 x 64 channels x rows a block (ops/conv.py MX_TILES).
#include "gemm_tile_mx.h"
#include "kernels.h"

namespace adapt {

namespace {

template <int F, int MT>
hipError_t mxt_launch(const SkinnyMxParams& p, int KS, hipStream_t s) {
  const long long tiles = (long long)((p.M + 16 * MT - 1) / (16 * MT)) * ((p.N + 64 * F - 1) / (64 * F));
  if (tiles > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL((gemm_tile_mx_kernel<F, MT>), dim3((unsigned)tiles, 1, KS), dim3(256), 0, s, p);
  return hipGetLastError();
}

}  // namespace

hipError_t gemm_tile_mx(const bf16* x, const uint32_t* codes, const uint32_t* scales, const float* bias,
                        const bf16* res, bf16* out, float* ws, int* counters, int M, int N, int K, int Kpad, int Npad,
                        int act, int F, int MT, int KS, hipStream_t s) {
  const SkinnyMxParams p{x, codes, scales, bias, res, out, ws, counters, M, N, K, Kpad, act};
  if (M < 1 || N < 1 || K < 1 || K % 8 || N % 8 || Kpad % MX_KC || Kpad < K || act < 0 || act > 2)
    return hipErrorInvalidValue;
  if (Npad < (N + 15) / 16 * 16) return hipErrorInvalidValue;                            // whole fragments are read
  if ((long long)M * N > 0x7fffffffLL || (long long)M * K > 0x7fffffffLL) return hipErrorInvalidValue;
  if (KS < 1 || KS > Kpad / MX_KC || KS > 65535) return hipErrorInvalidValue;            // no empty split
  if (KS > 1 && (!ws || !counters || (long long)M * N * 4 > 0x7fffffffLL)) return hipErrorInvalidValue;
  if (!x || !codes || !scales || !bias || !out) return hipErrorInvalidValue;
  const uintptr_t al = (uintptr_t)x | (uintptr_t)codes | (uintptr_t)bias | (uintptr_t)ws;
  if (al % 16 || (uintptr_t)scales % 4 || ((uintptr_t)res | (uintptr_t)out) % 8) return hipErrorInvalidValue;
  if (F == 4 && MT == 8) return mxt_launch<4, 8>(p, KS, s);
  if (F == 2 && MT == 4) return mxt_launch<2, 4>(p, KS, s);
  if (F == 1 && MT == 4) return mxt_launch<1, 4>(p, KS, s);
  return hipErrorInvalidValue;
}

}  // namespace adapt
