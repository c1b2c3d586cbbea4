// Entry points of incremental decoding (attention_decode.h holds the scheme): the key / value cache append, the
// decode attention with its split combine, and the position advance, fp32 and bf16, gfx950.
#include <atomic>

#include "attention_decode.h"

namespace adapt {
namespace {

constexpr long long LIM = 0x7fffffffll;

// The CU count the split plan is made for: the current device's (the wrapper makes the tensors' device current),
// asked once per device; an MI355X's 256 where there is no device (the plan is then only reported, never launched)
int decode_cus() {
  constexpr int MAXDEV = 64;
  static std::atomic<int> cached[MAXDEV];             // 0: not asked yet
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    (void)hipGetLastError();
    return 256;
  }
  if (dev >= 0 && dev < MAXDEV && (cus = cached[dev].load(std::memory_order_relaxed)) > 0) return cus;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) {
    (void)hipGetLastError();
    return 256;
  }
  if (dev >= 0 && dev < MAXDEV) cached[dev].store(cus, std::memory_order_relaxed);
  return cus;
}

bool decode_shape(int B, int Tmax, int hq, int hkv, int d, int dv) {
  if (B < 1 || Tmax < 1 || hq < 1 || hkv < 1 || hq % hkv || d < 1 || dv < 1) return false;
  return (long long)B * hkv * Tmax * (d > dv ? d : dv) <= LIM;
}

template <typename T>
hipError_t kv_append_launch(const T* x, const float* table, const int* pos, T* kc, T* vc, T* q_out, int B, int Tn,
                            int Tmax, int Ttab, int hq, int hkv, int d, int dv, int ld, int ld_q, hipStream_t s) {
  constexpr int VEC = 16 / sizeof(T);
  if (!decode_shape(B, Tmax, hq, hkv, d, dv) || Tn < 1 || !x || !pos || !kc || !vc) return hipErrorInvalidValue;
  const bool rope = table != nullptr;
  if (rope && (!q_out || d % 2 || Ttab < 1 || ld_q < hq * d || (long long)B * Tn * ld_q > LIM ||
               (long long)Ttab * d > LIM))
    return hipErrorInvalidValue;
  if ((long long)(hq + hkv) * d + (long long)hkv * dv > ld || (long long)B * Tn * ld > LIM) return hipErrorInvalidValue;
  uintptr_t ptrs = (uintptr_t)x | (uintptr_t)kc | (uintptr_t)vc;
  int sizes = d | dv | ld;
  if (rope) {
    ptrs |= (uintptr_t)q_out | (uintptr_t)table;
    sizes |= (d / 2) | ld_q;
  }
  const int v = (ptrs & 15) == 0 && sizes % VEC == 0 ? VEC : 1;
  attn::KvAppendArgs a{Tn, Tmax, Ttab, hq, hkv, d, dv, ld, ld_q, 0, 0, 0, 0, 0};
  a.nq = rope ? hq * (d / 2) / v : 0;
  a.nk = rope ? hkv * (d / 2) / v : hkv * d / v;
  a.nv = hkv * dv / v;
  a.nz = rope ? (ld_q - hq * d) / v : 0;
  const long long total = (long long)B * Tn * (a.nq + a.nk + a.nv + a.nz);
  if (total > LIM) return hipErrorInvalidValue;
  a.total = (int)total;
  const dim3 grid((a.total + 255) / 256), block(256);
  if (rope && v > 1)
    hipLaunchKernelGGL((attn::kv_append_kernel<T, VEC, true>), grid, block, 0, s, x, table, pos, kc, vc, q_out, a);
  else if (rope)
    hipLaunchKernelGGL((attn::kv_append_kernel<T, 1, true>), grid, block, 0, s, x, table, pos, kc, vc, q_out, a);
  else if (v > 1)
    hipLaunchKernelGGL((attn::kv_append_kernel<T, VEC, false>), grid, block, 0, s, x, table, pos, kc, vc, q_out, a);
  else
    hipLaunchKernelGGL((attn::kv_append_kernel<T, 1, false>), grid, block, 0, s, x, table, pos, kc, vc, q_out, a);
  return hipGetLastError();
}

template <typename T>
hipError_t attention_decode_launch(const T* q, const T* kc, const T* vc, const int* pos, T* out, float* ws, int B,
                                   int Tmax, int hq, int hkv, int d, int dv, int ld_q, int ld_out, hipStream_t s) {
  constexpr int VEC = 16 / sizeof(T);
  if (!decode_shape(B, Tmax, hq, hkv, d, dv) || !q || !kc || !vc || !pos || !out) return hipErrorInvalidValue;
  if (!attention_decode_path(d, dv, hq / hkv)) return hipErrorInvalidValue;
  if ((((uintptr_t)q | (uintptr_t)kc | (uintptr_t)vc) & 15) || ld_q % VEC || ld_q < hq * d || ld_out < hq * dv ||
      (long long)B * ld_q > LIM || (long long)B * ld_out > LIM || hkv > 65535 || B > 65535)
    return hipErrorInvalidValue;
  attn::DecodeArgs a{Tmax, hq, hkv, d, dv, ld_q, ld_out, 0, 0};
  attn::decode_plan(B, hkv, Tmax, decode_cus(), &a.S, &a.KS);
  if (a.S > 1 && !ws) return hipErrorInvalidValue;
  const dim3 grid(a.S, hkv, B), block(256);
  const int dm = d > dv ? d : dv;
  if (dm <= 32)
    hipLaunchKernelGGL((attn::attention_decode_kernel<T, 32, 4>), grid, block, 0, s, q, kc, vc, pos, out, ws, a);
  else if (dm <= 64)
    hipLaunchKernelGGL((attn::attention_decode_kernel<T, 64, 4>), grid, block, 0, s, q, kc, vc, pos, out, ws, a);
  else
    hipLaunchKernelGGL((attn::attention_decode_kernel<T, 128, VEC>), grid, block, 0, s, q, kc, vc, pos, out, ws, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || a.S == 1) return e;
  const int total = B * ld_out;
  hipLaunchKernelGGL((attn::attention_decode_combine_kernel<T>), dim3((total + 255) / 256), dim3(256), 0, s, ws, out, a,
                     total);
  return hipGetLastError();
}

}  // namespace

// 1: the decode kernel serves heads of (d, dv) shared by g query heads per key / value head
int attention_decode_path(int d, int dv, int g) { return attention_path(d, dv) && g >= 1 && g <= 16; }

// splits, keys per split and workspace floats ([B][hkv][S][g][dv + 2]; 0 when S == 1) of a decode launch
void attention_decode_plan(int B, int hkv, int Tmax, int* S, int* KS) {
  attn::decode_plan(B, hkv, Tmax, decode_cus(), S, KS);
}

hipError_t kv_append_f32(const float* x, const float* table, const int* pos, float* kc, float* vc, float* q_out, int B,
                         int Tn, int Tmax, int Ttab, int hq, int hkv, int d, int dv, int ld, int ld_q, hipStream_t s) {
  return kv_append_launch<float>(x, table, pos, kc, vc, q_out, B, Tn, Tmax, Ttab, hq, hkv, d, dv, ld, ld_q, s);
}

hipError_t kv_append_bf16(const bf16* x, const float* table, const int* pos, bf16* kc, bf16* vc, bf16* q_out, int B,
                          int Tn, int Tmax, int Ttab, int hq, int hkv, int d, int dv, int ld, int ld_q, hipStream_t s) {
  return kv_append_launch<bf16>(x, table, pos, kc, vc, q_out, B, Tn, Tmax, Ttab, hq, hkv, d, dv, ld, ld_q, s);
}

hipError_t attention_decode_f32(const float* q, const float* kc, const float* vc, const int* pos, float* out, float* ws,
                                int B, int Tmax, int hq, int hkv, int d, int dv, int ld_q, int ld_out, hipStream_t s) {
  return attention_decode_launch<float>(q, kc, vc, pos, out, ws, B, Tmax, hq, hkv, d, dv, ld_q, ld_out, s);
}

hipError_t attention_decode_bf16(const bf16* q, const bf16* kc, const bf16* vc, const int* pos, bf16* out, float* ws,
                                 int B, int Tmax, int hq, int hkv, int d, int dv, int ld_q, int ld_out, hipStream_t s) {
  return attention_decode_launch<bf16>(q, kc, vc, pos, out, ws, B, Tmax, hq, hkv, d, dv, ld_q, ld_out, s);
}

hipError_t advance_positions(int* pos, int B, int n, hipStream_t s) {
  if (!pos || B < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(attn::advance_positions_kernel, dim3((B + 255) / 256), dim3(256), 0, s, pos, B, n);
  return hipGetLastError();
}

}  // namespace adapt
