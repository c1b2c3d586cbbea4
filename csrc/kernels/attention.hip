// Self-attention front-end of the attention core (attention_core.h holds the scheme): softmax(Q K^T) V per
// (image, head) over one buffer, fp32 and bf16 activations, gfx950.
//
// qkv is [B * T][ld_in] with one row per token holding [Q | K | V], head-major inside each part (Q and K:
// heads x d, V: heads x dv).  out is [B * T][ld_out].  A group is an image; every address is the image's base
// plus a row and a column offset: head h's Q at column h d, its K at heads d + h d, its V at 2 heads d + h dv.  The
// staging table carries the K or V column of each vector, so a staged load needs no select.  The causal entry
// points run the core's CAUSAL instantiations on the same layout, the masked entry points its MASKED ones with a
// [B][T] fp32 padding mask (token j of an image is padding iff -1 < mask[j] < 1).
//
// Grouped-query attention (the gqa entry points): `heads` query heads share hkv < heads key / value heads, g =
// heads / hkv of them each, and a row is [Q: heads x d | K: hkv x d | V: hkv x dv].  That is a source policy derived
// from SelfSrc, GqaSrc, on the same templates: head h's K at column heads d + (h / g) d, its V at
// heads d + hkv d + (h / g) dv, everything else as SelfSrc.  Per (image, head) the arithmetic is that of a plain
// launch on rows in which each K / V head stands g times, so the two agree bit for bit.  SelfSrc and the templates
// are untouched.
#include "attention_core.h"

namespace adapt {
namespace {

template <typename T>
struct SelfSrc {
  const T* qkv;
  int Tn, heads, d, dv_, ld_in;
  struct Block {
    const T* base;                                    // this image's rows
    int img, qcol, kcol, vcol;
  };
  __host__ __device__ int dv() const { return dv_; }
  __host__ __device__ int nq() const { return Tn; }
  __host__ __device__ int nk() const { return Tn; }
  __device__ Block block(int img, int h) const {
    return Block{qkv + img * Tn * ld_in, img, h * d, heads * d + h * d, 2 * heads * d + h * dv_};
  }
  __device__ int stage_col(const Block& b, bool isv, int c) const { return (isv ? b.vcol : b.kcol) + c; }
  __device__ f32x4 stage(const Block& b, bool, int row, int col) const {
    return attn::ld4(b.base + row * ld_in + col);
  }
  __device__ const T* q(const Block& b, int row) const { return b.base + row * ld_in + b.qcol; }
  __device__ const T* k(const Block& b, int row) const { return b.base + b.kcol + row * ld_in; }
  __device__ const T* v(const Block& b, int row) const { return b.base + b.vcol + row * ld_in; }
  __device__ int out_row(const Block& b, int row) const { return b.img * Tn + row; }
};

// The same layout with a padding mask: image img's T mask values start at mask + img * T
template <typename T>
struct MaskedSelfSrc : SelfSrc<T> {
  const float* mask;
  __device__ const float* key_mask(const typename SelfSrc<T>::Block& b) const { return mask + b.img * this->Tn; }
};

// Grouped-query rows: hkv key / value heads, each read by g = heads / hkv consecutive query heads.  SelfSrc with
// the K and V columns of a block taken from its key / value head
template <typename T>
struct GqaSrc : SelfSrc<T> {
  int hkv, g;
  __device__ typename SelfSrc<T>::Block block(int img, int h) const {
    const int kv = h / g;
    return typename SelfSrc<T>::Block{this->qkv + img * this->Tn * this->ld_in, img, h * this->d,
                                      this->heads * this->d + kv * this->d,
                                      this->heads * this->d + hkv * this->d + kv * this->dv_};
  }
};

template <typename T, bool CAUSAL>
hipError_t attention_gqa_launch(const T* qkv, T* out, int B, int Tn, int heads, int hkv, int d, int dv, int ld_in,
                                int ld_out, hipStream_t s) {
  if (B < 1 || Tn < 1 || heads < 1 || hkv < 1 || heads % hkv || d < 1 || dv < 1 || !qkv || !out)
    return hipErrorInvalidValue;
  const long long lim = 0x7fffffffll;
  // the GQA row width: heads Q heads, hkv K and hkv V heads
  if ((long long)heads * d + (long long)hkv * ((long long)d + dv) > ld_in || (long long)heads * dv > ld_out)
    return hipErrorInvalidValue;
  if ((long long)B * Tn * ld_in > lim || (long long)B * Tn * ld_out > lim || (long long)B * heads * Tn > lim)
    return hipErrorInvalidValue;
  const bool mfma = attention_path(d, dv) &&
                    attn::attention_vec4((uintptr_t)qkv | (uintptr_t)out, ld_in | ld_out, (int)sizeof(T));
  GqaSrc<T> src;
  src.qkv = qkv; src.Tn = Tn; src.heads = heads; src.d = d; src.dv_ = dv; src.ld_in = ld_in;
  src.hkv = hkv; src.g = heads / hkv;
  return attn::attention_core_launch<T, GqaSrc<T>, CAUSAL>(src, out, ld_out, B, mfma, s);
}

template <typename T, bool CAUSAL>
hipError_t attention_launch(const T* qkv, T* out, int B, int Tn, int heads, int d, int dv, int ld_in, int ld_out,
                            hipStream_t s, const float* mask = nullptr) {
  if (B < 1 || Tn < 1 || heads < 1 || d < 1 || dv < 1) return hipErrorInvalidValue;
  const long long lim = 0x7fffffffll;
  if ((long long)heads * (2ll * d + dv) > ld_in || (long long)heads * dv > ld_out) return hipErrorInvalidValue;
  // 32-bit element offsets and grid sizes: refuse what does not fit
  if ((long long)B * Tn * ld_in > lim || (long long)B * Tn * ld_out > lim || (long long)B * heads * Tn > lim)
    return hipErrorInvalidValue;
  const bool mfma = attention_path(d, dv) &&
                    attn::attention_vec4((uintptr_t)qkv | (uintptr_t)out, ld_in | ld_out, (int)sizeof(T));
  if (mask) {
    if constexpr (!CAUSAL) {
      MaskedSelfSrc<T> src;
      src.qkv = qkv; src.Tn = Tn; src.heads = heads; src.d = d; src.dv_ = dv; src.ld_in = ld_in;
      src.mask = mask;
      return attn::attention_core_launch<T, MaskedSelfSrc<T>, false, true>(src, out, ld_out, B, mfma, s);
    }
    return hipErrorInvalidValue;                      // a padding mask together with the causal mask is not built
  }
  return attn::attention_core_launch<T, SelfSrc<T>, CAUSAL>(SelfSrc<T>{qkv, Tn, heads, d, dv, ld_in}, out, ld_out, B,
                                                            mfma, s);
}

}  // namespace

int attention_query_tile() { return attn::ATTN_QT; }
int attention_key_tile() { return attn::ATTN_KT; }

// 1: the MFMA path, 0: the plain kernel (which a misaligned buffer or stride takes as well)
int attention_path(int d, int dv) { return d >= 16 && dv >= 16 && d <= 128 && dv <= 128 && d % 16 == 0 && dv % 16 == 0; }

hipError_t attention_f32(const float* qkv, float* out, int B, int T, int heads, int d, int dv, int ld_in, int ld_out,
                         hipStream_t s) {
  return attention_launch<float, false>(qkv, out, B, T, heads, d, dv, ld_in, ld_out, s);
}

hipError_t attention_bf16(const bf16* qkv, bf16* out, int B, int T, int heads, int d, int dv, int ld_in, int ld_out,
                          hipStream_t s) {
  return attention_launch<bf16, false>(qkv, out, B, T, heads, d, dv, ld_in, ld_out, s);
}

// The causal instantiations: query i attends keys j <= i; same arguments and paths
hipError_t attention_causal_f32(const float* qkv, float* out, int B, int T, int heads, int d, int dv, int ld_in,
                                int ld_out, hipStream_t s) {
  return attention_launch<float, true>(qkv, out, B, T, heads, d, dv, ld_in, ld_out, s);
}

hipError_t attention_causal_bf16(const bf16* qkv, bf16* out, int B, int T, int heads, int d, int dv, int ld_in,
                                 int ld_out, hipStream_t s) {
  return attention_launch<bf16, true>(qkv, out, B, T, heads, d, dv, ld_in, ld_out, s);
}

// The padding-mask instantiations: mask [B][T] fp32, token j of an image is padding iff -1 < mask[j] < 1.  A padded
// key is not attended, a padded query's row (and every row of an image with no kept key) is zeros; key tiles past
// an image's last kept key are not loaded.  Same arguments and paths otherwise
hipError_t attention_masked_f32(const float* qkv, const float* mask, float* out, int B, int T, int heads, int d, int dv,
                                int ld_in, int ld_out, hipStream_t s) {
  if (!mask) return hipErrorInvalidValue;
  return attention_launch<float, false>(qkv, out, B, T, heads, d, dv, ld_in, ld_out, s, mask);
}

hipError_t attention_masked_bf16(const bf16* qkv, const float* mask, bf16* out, int B, int T, int heads, int d, int dv,
                                 int ld_in, int ld_out, hipStream_t s) {
  if (!mask) return hipErrorInvalidValue;
  return attention_launch<bf16, false>(qkv, out, B, T, heads, d, dv, ld_in, ld_out, s, mask);
}

// Grouped-query attention: `heads` query heads over kv_heads key / value heads (heads % kv_heads == 0), rows of
// [Q: heads x d | K: kv_heads x d | V: kv_heads x dv]; plain and causal, same paths
hipError_t attention_gqa_f32(const float* qkv, float* out, int B, int T, int heads, int kv_heads, int d, int dv,
                             int ld_in, int ld_out, hipStream_t s) {
  return attention_gqa_launch<float, false>(qkv, out, B, T, heads, kv_heads, d, dv, ld_in, ld_out, s);
}

hipError_t attention_gqa_bf16(const bf16* qkv, bf16* out, int B, int T, int heads, int kv_heads, int d, int dv,
                              int ld_in, int ld_out, hipStream_t s) {
  return attention_gqa_launch<bf16, false>(qkv, out, B, T, heads, kv_heads, d, dv, ld_in, ld_out, s);
}

hipError_t attention_gqa_causal_f32(const float* qkv, float* out, int B, int T, int heads, int kv_heads, int d, int dv,
                                    int ld_in, int ld_out, hipStream_t s) {
  return attention_gqa_launch<float, true>(qkv, out, B, T, heads, kv_heads, d, dv, ld_in, ld_out, s);
}

hipError_t attention_gqa_causal_bf16(const bf16* qkv, bf16* out, int B, int T, int heads, int kv_heads, int d, int dv,
                                     int ld_in, int ld_out, hipStream_t s) {
  return attention_gqa_launch<bf16, true>(qkv, out, B, T, heads, kv_heads, d, dv, ld_in, ld_out, s);
}

}  // namespace adapt
