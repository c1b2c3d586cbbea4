// Native CPU execution path (pybind11 module `_cpu`): the ops of a compiled
// fp32 launch plan (runtime/plan.py, `target="cpu"`) on NHWC float32 tensors,
// parallelised with OpenMP and vectorised over channels.
//
// The reference's single-chunk baseline runs ResNet-50 through TF's CPU
// kernels (`/root/reference/test/local_infer.py:18-28`, `model.predict` in
// float32) and its workers run whatever TF device they have
// (`/root/reference/src/node.py:177`).  Here a CPU stage executes the same
// fused steps as a GPU slice -- conv with BN folded into the weights at load,
// bias + residual + activation in the conv's own epilogue, pools with TF
// padding semantics, GAP, dense + softmax -- so PyTorch stays the test oracle
// only (ops/reference.py).
//
// Conv is a direct NHWC convolution blocked for registers: a task owns one
// output row segment of PIX pixels and a COB-wide slice of output channels,
// accumulates PIX x COB fp32 sums over (kh, kw, cin) with the filter row
// HWIO-contiguous in cout (one vector load feeds PIX FMAs), then applies the
// epilogue and stores.  1x1 convs and Dense are the same loop with kh = kw = 1.
// Each hot function is compiled for AVX-512, AVX2+FMA and baseline x86-64
// (`target_clones`); the loader picks the widest one the host CPU has, so the
// library runs on any x86-64 box.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <omp.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <vector>

namespace py = pybind11;

namespace {

#if defined(__x86_64__) && defined(__GNUC__) && !defined(__clang__)
#define ADAPT_CLONES __attribute__((target_clones("avx512f", "arch=haswell", "default")))
#else
#define ADAPT_CLONES
#endif

// Activations of the plan (graph/ir.py ACT_MODE; same formulas as
// csrc/kernels/common.h `act_f`, Keras 2 definitions).
enum Act { LINEAR = 0, RELU, RELU6, SWISH, SIGMOID, TANH, HARD_SIGMOID, HARD_SWISH, GELU, ELU, SELU, SOFTPLUS,
           LEAKY_RELU, GELU_TANH };

inline float act_f(float v, int mode, float alpha) {
  switch (mode) {
    case LINEAR: return v;
    case RELU: return v > 0.f ? v : 0.f;
    case RELU6: return std::min(std::max(v, 0.f), 6.f);
    case SWISH: return v / (1.f + std::exp(-v));
    case SIGMOID: return 1.f / (1.f + std::exp(-v));
    case TANH: return std::tanh(v);
    case HARD_SIGMOID: return std::min(std::max(0.2f * v + 0.5f, 0.f), 1.f);
    case HARD_SWISH: return v * std::min(std::max(v + 3.f, 0.f), 6.f) * (1.f / 6.f);
    case GELU: return 0.5f * v * (1.f + std::erf(v * 0.70710678f));
    case ELU: return v > 0.f ? v : std::exp(v) - 1.f;
    case SELU: return 1.0507009873554805f * (v > 0.f ? v : 1.6732632423543772f * (std::exp(v) - 1.f));
    case SOFTPLUS: return v > 20.f ? v : std::log1p(std::exp(v));
    case LEAKY_RELU: return v > 0.f ? v : alpha * v;
    case GELU_TANH: return 0.5f * v * (1.f + std::tanh(0.7978845608f * (v + 0.044715f * v * v * v)));
    default: throw std::invalid_argument("cpu_ops: unknown activation mode");
  }
}

template <typename T>
using Arr = py::array_t<T, py::array::c_style | py::array::forcecast>;

const float* cptr(const Arr<float>& a) { return a.data(); }
float* mptr(Arr<float>& a) { return a.mutable_data(); }

void need(bool ok, const char* what) {
  if (!ok) throw std::invalid_argument(std::string("cpu_ops: ") + what);
}

// ------------------------------------------------------------------ conv
constexpr int COB = 64;   // output channels per task (4 zmm / 8 ymm)
constexpr int PIX = 4;    // output pixels per task

struct ConvGeom {
  int N, H, W, C, OH, OW, CO, COP, KH, KW, S, PT, PL, act;
  float alpha;
};

// One task: pixels [ow0, ow0 + np) of output row (n, oh), channels [co0, co0 + COB).
// w is HWIO with cout padded to COP (a multiple of COB, zero filters).
ADAPT_CLONES
void conv_task(const ConvGeom& g, const float* __restrict x, const float* __restrict w, const float* __restrict bias,
               const float* __restrict res, float* __restrict y, int n, int oh, int ow0, int np, int co0) {
  float acc[PIX][COB];
  for (int p = 0; p < PIX; ++p)
    for (int j = 0; j < COB; ++j) acc[p][j] = 0.f;
  for (int kh = 0; kh < g.KH; ++kh) {
    const int ih = oh * g.S - g.PT + kh;
    if (ih < 0 || ih >= g.H) continue;
    for (int kw = 0; kw < g.KW; ++kw) {
      const float* xp[PIX];
      for (int p = 0; p < PIX; ++p) {
        const int iw = (ow0 + p) * g.S - g.PL + kw;
        xp[p] = (p < np && iw >= 0 && iw < g.W) ? x + (((size_t)n * g.H + ih) * g.W + iw) * g.C : nullptr;
      }
      const float* wr = w + ((size_t)(kh * g.KW + kw) * g.C) * g.COP + co0;
      if (xp[0] && xp[1] && xp[2] && xp[3]) {          // interior: no per-pixel checks in the K loop
        for (int c = 0; c < g.C; ++c) {
          const float* wv = wr + (size_t)c * g.COP;
          const float x0 = xp[0][c], x1 = xp[1][c], x2 = xp[2][c], x3 = xp[3][c];
#pragma omp simd
          for (int j = 0; j < COB; ++j) {
            const float wj = wv[j];
            acc[0][j] += x0 * wj;
            acc[1][j] += x1 * wj;
            acc[2][j] += x2 * wj;
            acc[3][j] += x3 * wj;
          }
        }
      } else {
        for (int c = 0; c < g.C; ++c) {
          const float* wv = wr + (size_t)c * g.COP;
          float xv[PIX];
          for (int p = 0; p < PIX; ++p) xv[p] = xp[p] ? xp[p][c] : 0.f;
#pragma omp simd
          for (int j = 0; j < COB; ++j) {
            const float wj = wv[j];
            acc[0][j] += xv[0] * wj;
            acc[1][j] += xv[1] * wj;
            acc[2][j] += xv[2] * wj;
            acc[3][j] += xv[3] * wj;
          }
        }
      }
    }
  }
  const int nco = std::min(COB, g.CO - co0);
  for (int p = 0; p < np; ++p) {
    const size_t o = (((size_t)n * g.OH + oh) * g.OW + ow0 + p) * g.CO + co0;
    float* yo = y + o;
    const float* ro = res ? res + o : nullptr;
    for (int j = 0; j < nco; ++j) {
      float v = acc[p][j] + bias[co0 + j];
      if (ro) v += ro[j];
      yo[j] = g.act == RELU ? (v > 0.f ? v : 0.f) : act_f(v, g.act, g.alpha);
    }
  }
}

// x [N,H,W,C]; w [KH,KW,C,COP] (cout padded to COP); bias [CO]; y [N,OH,OW,CO];
// residual (optional) [N,OH,OW,CO] added before the activation.
void conv2d(const Arr<float>& x, const Arr<float>& w, const Arr<float>& bias, Arr<float>& y, int stride, int pad_t,
            int pad_l, int act, float alpha, py::object residual) {
  need(x.ndim() == 4 && w.ndim() == 4 && y.ndim() == 4 && bias.ndim() == 1, "conv2d ranks");
  ConvGeom g{(int)x.shape(0), (int)x.shape(1), (int)x.shape(2), (int)x.shape(3), (int)y.shape(1), (int)y.shape(2),
             (int)y.shape(3), (int)w.shape(3), (int)w.shape(0), (int)w.shape(1), stride, pad_t, pad_l, act, alpha};
  need(w.shape(2) == g.C && g.COP % COB == 0 && g.COP >= g.CO && y.shape(0) == g.N && bias.shape(0) >= g.CO,
       "conv2d shapes");
  Arr<float> r;
  const float* rp = nullptr;
  if (!residual.is_none()) {
    r = residual.cast<Arr<float>>();
    need(r.size() == y.size(), "conv2d residual shape");
    rp = r.data();
  }
  const float *xp = cptr(x), *wp = cptr(w), *bp = cptr(bias);
  float* yp = mptr(y);
  const int segs = (g.OW + PIX - 1) / PIX, cob = g.COP / COB;
  const long tasks = (long)g.N * g.OH * segs * cob;
  py::gil_scoped_release nogil;
#pragma omp parallel for schedule(static)
  for (long t = 0; t < tasks; ++t) {
    // channel slice innermost: the tasks of one thread share their input row segment
    const int cb = (int)(t % cob);
    long r2 = t / cob;
    const int sg = (int)(r2 % segs);
    r2 /= segs;
    const int oh = (int)(r2 % g.OH), n = (int)(r2 / g.OH);
    const int ow0 = sg * PIX;
    conv_task(g, xp, wp, bp, rp, yp, n, oh, ow0, std::min(PIX, g.OW - ow0), cb * COB);
  }
}

// ------------------------------------------------------------------ grouped conv
// Keras Conv2D(groups = G): output channel o reads the C / G input channels of
// group o / (CO / G).  A task owns one output row of one group and accumulates
// CO / G sums per pixel over (kh, kw, ci) with the filter row contiguous in cout.
// x [N,H,W,C]; w [KH,KW,C/G,CO]; bias [CO]; y [N,OH,OW,CO]
ADAPT_CLONES
void gconv_row(const float* __restrict x, const float* __restrict w, const float* __restrict b, float* __restrict y,
               int n, int oh, int g, int H, int W, int C, int OH, int OW, int CO, int G, int KH, int KW, int S, int PT,
               int PL, int act, float alpha) {
  const int cgi = C / G, cgo = CO / G;
  std::vector<float> accv(cgo);
  float* a = accv.data();
  const float* bg = b + g * cgo;
  for (int ow = 0; ow < OW; ++ow) {
    std::copy(bg, bg + cgo, a);
    for (int kh = 0; kh < KH; ++kh) {
      const int ih = oh * S - PT + kh;
      if (ih < 0 || ih >= H) continue;
      for (int kw = 0; kw < KW; ++kw) {
        const int iw = ow * S - PL + kw;
        if (iw < 0 || iw >= W) continue;
        const float* xv = x + (((size_t)n * H + ih) * W + iw) * C + (size_t)g * cgi;
        const float* wr = w + ((size_t)(kh * KW + kw) * cgi) * CO + (size_t)g * cgo;
        for (int ci = 0; ci < cgi; ++ci) {
          const float xc = xv[ci];
          const float* wv = wr + (size_t)ci * CO;
#pragma omp simd
          for (int j = 0; j < cgo; ++j) a[j] += xc * wv[j];
        }
      }
    }
    float* yo = y + (((size_t)n * OH + oh) * OW + ow) * CO + (size_t)g * cgo;
    for (int j = 0; j < cgo; ++j) yo[j] = act_f(a[j], act, alpha);
  }
}

void gconv2d(const Arr<float>& x, const Arr<float>& w, const Arr<float>& bias, Arr<float>& y, int stride, int pad_t,
             int pad_l, int groups, int act, float alpha) {
  need(x.ndim() == 4 && w.ndim() == 4 && y.ndim() == 4 && bias.ndim() == 1, "gconv2d ranks");
  const int N = x.shape(0), H = x.shape(1), W = x.shape(2), C = x.shape(3), OH = y.shape(1), OW = y.shape(2),
            CO = y.shape(3), KH = w.shape(0), KW = w.shape(1);
  need(groups >= 1 && C % groups == 0 && CO % groups == 0 && w.shape(2) == C / groups && w.shape(3) == CO &&
           y.shape(0) == N && bias.shape(0) == CO && stride >= 1,
       "gconv2d shapes");
  const float *xp = cptr(x), *wp = cptr(w), *bp = cptr(bias);
  float* yp = mptr(y);
  py::gil_scoped_release nogil;
#pragma omp parallel for collapse(3) schedule(static)
  for (int n = 0; n < N; ++n)
    for (int oh = 0; oh < OH; ++oh)
      for (int g = 0; g < groups; ++g)
        gconv_row(xp, wp, bp, yp, n, oh, g, H, W, C, OH, OW, CO, groups, KH, KW, stride, pad_t, pad_l, act, alpha);
}

// ------------------------------------------------------------------ transposed conv
// Keras Conv2DTranspose in gather form: output (oy, ox) sits at f = o + pad in the
// full scatter frame F[i * S + t] += x[i] * w[t]; its taps are the t == f (mod S)
// with i = (f - t) / S inside the map.  Every output element is written once; one
// with no tap (KH < S) is act(bias).  A task owns one output row.
// x [N,H,W,C]; w [KH,KW,C,CO] (output channels last); bias [CO]; y [N,OH,OW,CO]
ADAPT_CLONES
void deconv_row(const float* __restrict x, const float* __restrict w, const float* __restrict b, float* __restrict y,
                int n, int oy, int H, int W, int C, int OH, int OW, int CO, int KH, int KW, int S, int PT, int PL,
                int act, float alpha) {
  std::vector<float> accv(CO);
  float* a = accv.data();
  const int fy = oy + PT;
  for (int ox = 0; ox < OW; ++ox) {
    std::copy(b, b + CO, a);
    const int fx = ox + PL;
    for (int ty = fy % S; ty < KH; ty += S) {
      const int iy = (fy - ty) / S;
      if (fy < ty || iy >= H) continue;
      for (int tx = fx % S; tx < KW; tx += S) {
        const int ix = (fx - tx) / S;
        if (fx < tx || ix >= W) continue;
        const float* xv = x + (((size_t)n * H + iy) * W + ix) * C;
        const float* wr = w + (size_t)(ty * KW + tx) * C * CO;
        for (int ci = 0; ci < C; ++ci) {
          const float xc = xv[ci];
          const float* wv = wr + (size_t)ci * CO;
#pragma omp simd
          for (int j = 0; j < CO; ++j) a[j] += xc * wv[j];
        }
      }
    }
    float* yo = y + (((size_t)n * OH + oy) * OW + ox) * CO;
    for (int j = 0; j < CO; ++j) yo[j] = act_f(a[j], act, alpha);
  }
}

void deconv2d(const Arr<float>& x, const Arr<float>& w, const Arr<float>& bias, Arr<float>& y, int stride, int pad_t,
              int pad_l, int act, float alpha) {
  need(x.ndim() == 4 && w.ndim() == 4 && y.ndim() == 4 && bias.ndim() == 1, "deconv2d ranks");
  const int N = x.shape(0), H = x.shape(1), W = x.shape(2), C = x.shape(3), OH = y.shape(1), OW = y.shape(2),
            CO = y.shape(3), KH = w.shape(0), KW = w.shape(1);
  need(w.shape(2) == C && w.shape(3) == CO && y.shape(0) == N && bias.shape(0) == CO && stride >= 1 && pad_t >= 0 &&
           pad_l >= 0 && N >= 1 && H >= 1 && W >= 1 && OH >= 1 && OW >= 1,
       "deconv2d shapes");
  const float *xp = cptr(x), *wp = cptr(w), *bp = cptr(bias);
  float* yp = mptr(y);
  py::gil_scoped_release nogil;
#pragma omp parallel for collapse(2) schedule(static)
  for (int n = 0; n < N; ++n)
    for (int oy = 0; oy < OH; ++oy)
      deconv_row(xp, wp, bp, yp, n, oy, H, W, C, OH, OW, CO, KH, KW, stride, pad_t, pad_l, act, alpha);
}

// ------------------------------------------------------------------ upsample / crop
// Keras UpSampling2D: y [N,H*SH,W*SW,C].  Nearest repeats pixels; bilinear is
// tf.image.resize with half-pixel centres: f = max((o + 0.5) / s - 0.5, 0),
// i0 = floor(f), i1 = min(i0 + 1, size - 1), weight f - i0.
void upsample2d(const Arr<float>& x, Arr<float>& y, int sh, int sw, bool bilinear) {
  need(x.ndim() == 4 && y.ndim() == 4 && sh >= 1 && sw >= 1, "upsample2d ranks");
  const int N = x.shape(0), H = x.shape(1), W = x.shape(2), C = x.shape(3);
  const int OH = H * sh, OW = W * sw;
  need(y.shape(0) == N && y.shape(1) == OH && y.shape(2) == OW && y.shape(3) == C, "upsample2d shapes");
  const float* xp = cptr(x);
  float* yp = mptr(y);
  py::gil_scoped_release nogil;
#pragma omp parallel for collapse(2) schedule(static)
  for (int n = 0; n < N; ++n)
    for (int oy = 0; oy < OH; ++oy) {
      float* yr = yp + ((size_t)n * OH + oy) * OW * C;
      if (!bilinear) {
        const float* xr = xp + ((size_t)n * H + oy / sh) * W * C;
        for (int ox = 0; ox < OW; ++ox) std::memcpy(yr + (size_t)ox * C, xr + (size_t)(ox / sw) * C, sizeof(float) * C);
        continue;
      }
      const float fy = std::max((oy + 0.5f) / sh - 0.5f, 0.f);
      const int y0 = (int)fy, y1 = std::min(y0 + 1, H - 1);
      const float wy = fy - y0;
      const float* r0 = xp + ((size_t)n * H + y0) * W * C;
      const float* r1 = xp + ((size_t)n * H + y1) * W * C;
      for (int ox = 0; ox < OW; ++ox) {
        const float fx = std::max((ox + 0.5f) / sw - 0.5f, 0.f);
        const int x0 = (int)fx, x1 = std::min(x0 + 1, W - 1);
        const float wx = fx - x0;
        const float *a = r0 + (size_t)x0 * C, *b = r0 + (size_t)x1 * C, *c = r1 + (size_t)x0 * C,
                    *d = r1 + (size_t)x1 * C;
        float* yo = yr + (size_t)ox * C;
#pragma omp simd
        for (int j = 0; j < C; ++j) {
          const float top = a[j] + (b[j] - a[j]) * wx, bot = c[j] + (d[j] - c[j]) * wx;
          yo[j] = top + (bot - top) * wy;
        }
      }
    }
}

// Keras Cropping2D: y [N,H-t-b,W-l-r,C] = x[:, t:H-b, l:W-r, :]
void crop2d(const Arr<float>& x, Arr<float>& y, int t, int l) {
  need(x.ndim() == 4 && y.ndim() == 4 && t >= 0 && l >= 0, "crop2d ranks");
  const int N = x.shape(0), H = x.shape(1), W = x.shape(2), C = x.shape(3), OH = y.shape(1), OW = y.shape(2);
  need(y.shape(0) == N && y.shape(3) == C && OH >= 1 && OW >= 1 && t + OH <= H && l + OW <= W, "crop2d shapes");
  const float* xp = cptr(x);
  float* yp = mptr(y);
  py::gil_scoped_release nogil;
#pragma omp parallel for collapse(2) schedule(static)
  for (int n = 0; n < N; ++n)
    for (int h = 0; h < OH; ++h)
      std::memcpy(yp + ((size_t)n * OH + h) * OW * C, xp + (((size_t)n * H + h + t) * W + l) * C,
                  sizeof(float) * OW * C);
}

// Swin patch merging's rearrangement: y [N,H/2,W/2,4C], y[n, i, j, (2 dx + dy) C + c] = x[n, 2i + dy, 2j + dx, c]
void space_to_depth(const Arr<float>& x, Arr<float>& y) {
  need(x.ndim() == 4 && y.ndim() == 4, "space_to_depth ranks");
  const int N = x.shape(0), H = x.shape(1), W = x.shape(2), C = x.shape(3);
  need(H % 2 == 0 && W % 2 == 0 && y.shape(0) == N && y.shape(1) == H / 2 && y.shape(2) == W / 2 &&
           y.shape(3) == 4 * C, "space_to_depth shapes");
  const float* xp = cptr(x);
  float* yp = mptr(y);
  py::gil_scoped_release nogil;
#pragma omp parallel for collapse(2) schedule(static)
  for (int n = 0; n < N; ++n)
    for (int i = 0; i < H / 2; ++i)
      for (int j = 0; j < W / 2; ++j)
        for (int dx = 0; dx < 2; ++dx)
          for (int dy = 0; dy < 2; ++dy)
            std::memcpy(yp + ((((size_t)n * (H / 2) + i) * (W / 2) + j) * 4 + 2 * dx + dy) * C,
                        xp + (((size_t)n * H + 2 * i + dy) * W + 2 * j + dx) * C, sizeof(float) * C);
}

// Swin window attention core on the NHWC map, nothing rolled or partitioned in memory: the argument layout of the
// GPU op (csrc/kernels/window_attention.hip) except that the bias is the raw table [(2M-1)^2][heads].  Token
// (i, j) of window (wy, wx) is the map row ((wy M + i + s) mod H) W + (wx M + j + s) mod W; its score against
// token (k, l) gets table[(i-k+M-1)(2M-1) + (j-l+M-1)][head], and -100 when s > 0 and the two lie in different
// regions of the rolled frame (rows [0, H-M), [H-M, H-s), [H-s, H), columns alike).
void window_attention(const Arr<float>& qkv, const Arr<float>& table, Arr<float>& out, int B, int H, int W, int M,
                      int s, int heads, int d) {
  need(qkv.ndim() >= 2 && out.ndim() >= 2 && B >= 1 && H >= 1 && W >= 1 && M >= 1 && heads >= 1 && d >= 1 &&
           s >= 0 && s < M && H % M == 0 && W % M == 0, "window_attention args");
  const long ld_in = qkv.shape(qkv.ndim() - 1), ld_out = out.shape(out.ndim() - 1);
  need(qkv.size() == (long)B * H * W * ld_in && out.size() == (long)B * H * W * ld_out &&
           ld_in >= 3l * heads * d && ld_out >= (long)heads * d, "window_attention shapes");
  need(table.ndim() == 2 && table.shape(0) == (long)(2 * M - 1) * (2 * M - 1) && table.shape(1) == heads,
       "window_attention table");
  const float *xp = cptr(qkv), *tp = cptr(table);
  float* yp = mptr(out);
  const int T = M * M, nwy = H / M, nwx = W / M;
  py::gil_scoped_release nogil;
#pragma omp parallel
  {
    std::vector<float> p(T);
    std::vector<long> row(T);
    std::vector<int> reg(T);
#pragma omp for collapse(3) schedule(static)
    for (int b = 0; b < B; ++b)
      for (int wy = 0; wy < nwy; ++wy)
        for (int wx = 0; wx < nwx; ++wx) {
          for (int t = 0; t < T; ++t) {
            const int ry = wy * M + t / M, rx = wx * M + t % M;      // rolled frame
            row[t] = ((long)b * H + (ry + s) % H) * W + (rx + s) % W;
            reg[t] = 3 * (ry < H - M ? 0 : ry < H - s ? 1 : 2) + (rx < W - M ? 0 : rx < W - s ? 1 : 2);
          }
          for (int h = 0; h < heads; ++h)
            for (int q = 0; q < T; ++q) {
              const float* qr = xp + row[q] * ld_in + h * d;
              float mx = -INFINITY;
              for (int k = 0; k < T; ++k) {
                const float* kr = xp + row[k] * ld_in + heads * d + h * d;
                float sc = 0.f;
                for (int i = 0; i < d; ++i) sc += qr[i] * kr[i];
                sc += tp[(long)((q / M - k / M + M - 1) * (2 * M - 1) + (q % M - k % M + M - 1)) * heads + h];
                if (s > 0 && reg[q] != reg[k]) sc += -100.f;
                p[k] = sc;
                mx = std::max(mx, sc);
              }
              float l = 0.f;
              for (int k = 0; k < T; ++k) {
                p[k] = std::exp(p[k] - mx);
                l += p[k];
              }
              float* orow = yp + row[q] * ld_out + h * d;
              for (int c = 0; c < d; ++c) orow[c] = 0.f;
              for (int k = 0; k < T; ++k) {
                const float* vr = xp + row[k] * ld_in + 2 * heads * d + h * d;
                const float pk = p[k];
                for (int c = 0; c < d; ++c) orow[c] += pk * vr[c];
              }
              const float inv = 1.f / l;
              for (int c = 0; c < d; ++c) orow[c] *= inv;
              if (h == heads - 1)
                for (long c = (long)heads * d; c < ld_out; ++c) yp[row[q] * ld_out + c] = 0.f;
            }
        }
  }
}

// Self-attention core, softmax(Q K^T) V per (image, head): qkv [B*T][ld_in] rows of [Q | K | V] (head-major, Q
// already scaled by 1/sqrt(d)), out [B*T][ld_out] with heads * dv channels (the rest of a row becomes zero): the
// argument layout of the GPU op (csrc/kernels/attention.hip).  fp32, the row maximum subtracted before the exponent.
// causal: query q attends keys k <= q (Keras' use_causal_mask).  key_mask (None, or B * T floats; never with
// causal): token j of an image is padding iff -1 < key_mask[j] < 1 (a NaN is kept); a padded key is not attended
// (its K and V rows are not read), a padded query's row and every row of an image with no kept key are zeros.
// kv_heads (0: heads): grouped-query attention, head h reads K / V head h / (heads / kv_heads) of a row
// [Q: heads x d | K: kv_heads x d | V: kv_heads x dv]; never with key_mask.
void attention(const Arr<float>& qkv, Arr<float>& out, int B, int T, int heads, int d, int dv, bool causal,
               const py::object& key_mask, int kv_heads) {
  const bool masked = !key_mask.is_none();
  const int hkv = kv_heads > 0 ? kv_heads : heads;
  need(kv_heads >= 0 && heads >= 1 && heads % hkv == 0, "attention kv_heads must divide heads");
  need(hkv == heads || !masked, "attention kv_heads never with key_mask");
  const int grp = heads / hkv;
  Arr<float> mask_arr;
  if (masked) {
    need(py::isinstance<Arr<float>>(key_mask), "attention key_mask must be a float32 array");
    mask_arr = key_mask.cast<Arr<float>>();
    need(!causal && mask_arr.size() == (long)B * T, "attention key_mask holds B * T values, and never with causal");
  }
  const float* mk = masked ? cptr(mask_arr) : nullptr;
  need(qkv.ndim() >= 2 && out.ndim() >= 2 && B >= 1 && T >= 1 && heads >= 1 && d >= 1 && dv >= 1, "attention args");
  const long ld_in = qkv.shape(qkv.ndim() - 1), ld_out = out.shape(out.ndim() - 1);
  need(qkv.size() == (long)B * T * ld_in && out.size() == (long)B * T * ld_out &&
           ld_in >= (long)heads * d + (long)hkv * (d + dv) && ld_out >= (long)heads * dv, "attention shapes");
  const float* xp = cptr(qkv);
  float* yp = mptr(out);
  py::gil_scoped_release nogil;
#pragma omp parallel
  {
    std::vector<float> p(T);
#pragma omp for collapse(2) schedule(static)
    for (int b = 0; b < B; ++b)
      for (int h = 0; h < heads; ++h) {
        const float* base = xp + (size_t)b * T * ld_in;
        const float* kb = base + heads * d + (h / grp) * d;
        const float* vb = base + heads * d + hkv * d + (h / grp) * dv;
        for (int q = 0; q < T; ++q) {
          const float* qr = base + (size_t)q * ld_in + h * d;
          const int nk = causal ? q + 1 : T;           // the keys this query attends
          const float* mrow = masked ? mk + (size_t)b * T : nullptr;
          auto kept = [&](int t) { return !mrow || !(mrow[t] > -1.f && mrow[t] < 1.f); };
          float* orow = yp + ((size_t)b * T + q) * ld_out + h * dv;
          float mx = -INFINITY;
          if (kept(q))                                 // a padded query attends nothing: l stays 0
            for (int k = 0; k < nk; ++k) {
              if (!kept(k)) continue;
              const float* kr = kb + (size_t)k * ld_in;
              float sc = 0.f;
              for (int i = 0; i < d; ++i) sc += qr[i] * kr[i];
              p[k] = sc;
              mx = std::max(mx, sc);
            }
          float l = 0.f;
          for (int c = 0; c < dv; ++c) orow[c] = 0.f;
          if (mx != -INFINITY || !masked) {
            for (int k = 0; k < nk; ++k) {
              if (!kept(k)) continue;
              p[k] = std::exp(p[k] - mx);
              l += p[k];
            }
            for (int k = 0; k < nk; ++k) {
              if (!kept(k)) continue;
              const float* vr = vb + (size_t)k * ld_in;
              const float pk = p[k];
              for (int c = 0; c < dv; ++c) orow[c] += pk * vr[c];
            }
          }
          const float inv = l == 0.f && masked ? 0.f : 1.f / l;
          for (int c = 0; c < dv; ++c) orow[c] *= inv;
          if (h == heads - 1)
            for (long c = (long)heads * dv; c < ld_out; ++c) yp[((size_t)b * T + q) * ld_out + c] = 0.f;
        }
      }
  }
}

// Attention core with separate sources, softmax(Q K^T) V per (image, head): q [B*Tq][ldq], k [B*Tk][ldk],
// v [B*Tk][ldv], each starting at its part's first column (head h at h*d for Q and K, h*dv for V; Q already scaled),
// out [B*Tq][ld_out] with heads * dv channels (the rest of a row becomes zero): the argument layout of the GPU op
// (csrc/kernels/cross_attention.hip), the strides being the arrays' last dimensions.  A column slice of a wider
// array arrives as a dense copy.
void cross_attention(const Arr<float>& q, const Arr<float>& k, const Arr<float>& v, Arr<float>& out, int B, int Tq,
                     int Tk, int heads, int d, int dv) {
  need(q.ndim() >= 2 && k.ndim() >= 2 && v.ndim() >= 2 && out.ndim() >= 2 && B >= 1 && Tq >= 1 && Tk >= 1 &&
           heads >= 1 && d >= 1 && dv >= 1, "cross_attention args");
  const long ldq = q.shape(q.ndim() - 1), ldk = k.shape(k.ndim() - 1), ldv = v.shape(v.ndim() - 1),
             ld_out = out.shape(out.ndim() - 1);
  need(q.size() == (long)B * Tq * ldq && k.size() == (long)B * Tk * ldk && v.size() == (long)B * Tk * ldv &&
           out.size() == (long)B * Tq * ld_out && ldq >= (long)heads * d && ldk >= (long)heads * d &&
           ldv >= (long)heads * dv && ld_out >= (long)heads * dv, "cross_attention shapes");
  const float *qp = cptr(q), *kp = cptr(k), *vp = cptr(v);
  float* yp = mptr(out);
  py::gil_scoped_release nogil;
#pragma omp parallel
  {
    std::vector<float> p(Tk);
#pragma omp for collapse(2) schedule(static)
    for (int b = 0; b < B; ++b)
      for (int h = 0; h < heads; ++h) {
        const float* kb = kp + (size_t)b * Tk * ldk + h * d;
        const float* vb = vp + (size_t)b * Tk * ldv + h * dv;
        for (int qi = 0; qi < Tq; ++qi) {
          const float* qr = qp + ((size_t)b * Tq + qi) * ldq + h * d;
          float mx = -INFINITY;
          for (int kk = 0; kk < Tk; ++kk) {
            const float* kr = kb + (size_t)kk * ldk;
            float sc = 0.f;
            for (int i = 0; i < d; ++i) sc += qr[i] * kr[i];
            p[kk] = sc;
            mx = std::max(mx, sc);
          }
          float l = 0.f;
          for (int kk = 0; kk < Tk; ++kk) {
            p[kk] = std::exp(p[kk] - mx);
            l += p[kk];
          }
          float* orow = yp + ((size_t)b * Tq + qi) * ld_out + h * dv;
          for (int c = 0; c < dv; ++c) orow[c] = 0.f;
          for (int kk = 0; kk < Tk; ++kk) {
            const float* vr = vb + (size_t)kk * ldv;
            const float pk = p[kk];
            for (int c = 0; c < dv; ++c) orow[c] += pk * vr[c];
          }
          const float inv = 1.f / l;
          for (int c = 0; c < dv; ++c) orow[c] *= inv;
          if (h == heads - 1)
            for (long c = (long)heads * dv; c < ld_out; ++c) yp[((size_t)b * Tq + qi) * ld_out + c] = 0.f;
        }
      }
  }
}

// Embedding: out[r] = table[(int)ids[r]], the ids carried as fp32 and truncated toward zero; an id outside [0, V)
// (or not a number) yields a zero row, as the GPU op (csrc/kernels/layers.hip).  table [V][C], out [rows...][C]
void embedding(const Arr<float>& ids, const Arr<float>& table, Arr<float>& out) {
  need(table.ndim() == 2 && ids.size() >= 1 && table.shape(0) >= 1 && table.shape(0) <= (1l << 24) &&
           out.size() == ids.size() * table.shape(1), "embedding shapes");
  const long V = table.shape(0), C = table.shape(1);
  const float *ip = cptr(ids), *tp = cptr(table);
  float* yp = mptr(out);
  for (long r = 0; r < (long)ids.size(); ++r) {
    const float f = ip[r];
    if (f > -1.f && f < (float)V)
      std::memcpy(yp + (size_t)r * C, tp + (size_t)(long)f * C, C * sizeof(float));
    else
      std::memset(yp + (size_t)r * C, 0, C * sizeof(float));
  }
}

// Learned queries: out[b][t] = emb[t] for every image, emb [N][C], out [B][...][N][C]
void queries(const Arr<float>& emb, Arr<float>& out, int B) {
  need(emb.ndim() == 2 && B >= 1 && out.size() == (long)B * emb.size(), "queries shapes");
  const float* ep = cptr(emb);
  float* yp = mptr(out);
  const size_t n = (size_t)emb.size();
  for (int b = 0; b < B; ++b) std::memcpy(yp + (size_t)b * n, ep, n * sizeof(float));
}

// ------------------------------------------------------------------ depthwise
// x [N,H,W,C]; w [KH,KW,C]; bias [C]; y [N,OH,OW,C]
ADAPT_CLONES
void dw_row(const float* __restrict x, const float* __restrict w, const float* __restrict b, float* __restrict y,
            int n, int oh, int H, int W, int C, int OW, int KH, int KW, int S, int PT, int PL, int act, float alpha,
            int OH) {
  std::vector<float> acc(C);
  for (int ow = 0; ow < OW; ++ow) {
    std::copy(b, b + C, acc.begin());
    for (int kh = 0; kh < KH; ++kh) {
      const int ih = oh * S - PT + kh;
      if (ih < 0 || ih >= H) continue;
      for (int kw = 0; kw < KW; ++kw) {
        const int iw = ow * S - PL + kw;
        if (iw < 0 || iw >= W) continue;
        const float* xv = x + (((size_t)n * H + ih) * W + iw) * C;
        const float* wv = w + (size_t)(kh * KW + kw) * C;
        float* a = acc.data();
#pragma omp simd
        for (int c = 0; c < C; ++c) a[c] += xv[c] * wv[c];
      }
    }
    float* yo = y + (((size_t)n * OH + oh) * OW + ow) * C;
    for (int c = 0; c < C; ++c) yo[c] = act_f(acc[c], act, alpha);
  }
}

void dwconv2d(const Arr<float>& x, const Arr<float>& w, const Arr<float>& bias, Arr<float>& y, int stride, int pad_t,
              int pad_l, int act, float alpha) {
  need(x.ndim() == 4 && w.ndim() == 3 && y.ndim() == 4, "dwconv ranks");
  const int N = x.shape(0), H = x.shape(1), W = x.shape(2), C = x.shape(3), OH = y.shape(1), OW = y.shape(2);
  need(w.shape(2) == C && y.shape(3) == C && bias.shape(0) == C, "dwconv shapes");
  const float *xp = cptr(x), *wp = cptr(w), *bp = cptr(bias);
  float* yp = mptr(y);
  const int KH = w.shape(0), KW = w.shape(1);
  py::gil_scoped_release nogil;
#pragma omp parallel for collapse(2) schedule(static)
  for (int n = 0; n < N; ++n)
    for (int oh = 0; oh < OH; ++oh) dw_row(xp, wp, bp, yp, n, oh, H, W, C, OW, KH, KW, stride, pad_t, pad_l, act, alpha, OH);
}

// ------------------------------------------------------------------ pools
// kind 0 max, 1 avg.  pad_zero (max): padded positions take part as zeros (a
// folded ZeroPadding2D); otherwise they are excluded (Keras 'same').  avg
// always excludes them (TF).
void pool2d(const Arr<float>& x, Arr<float>& y, int kind, int kh_, int kw_, int stride, int pad_t, int pad_l,
            bool pad_zero) {
  need(x.ndim() == 4 && y.ndim() == 4, "pool ranks");
  const int N = x.shape(0), H = x.shape(1), W = x.shape(2), C = x.shape(3), OH = y.shape(1), OW = y.shape(2);
  need(y.shape(3) == C, "pool channels");
  const float* xp = cptr(x);
  float* yp = mptr(y);
  py::gil_scoped_release nogil;
#pragma omp parallel for collapse(2) schedule(static)
  for (int n = 0; n < N; ++n)
    for (int oh = 0; oh < OH; ++oh) {
      std::vector<float> acc(C);
      for (int ow = 0; ow < OW; ++ow) {
        std::fill(acc.begin(), acc.end(), kind == 0 ? -INFINITY : 0.f);
        int cnt = 0;
        bool padded = false;
        for (int i = 0; i < kh_; ++i) {
          const int ih = oh * stride - pad_t + i;
          for (int j = 0; j < kw_; ++j) {
            const int iw = ow * stride - pad_l + j;
            if (ih < 0 || ih >= H || iw < 0 || iw >= W) {
              padded = true;
              continue;
            }
            ++cnt;
            const float* xv = xp + (((size_t)n * H + ih) * W + iw) * C;
            float* a = acc.data();
            if (kind == 0) {
#pragma omp simd
              for (int c = 0; c < C; ++c) a[c] = std::max(a[c], xv[c]);
            } else {
#pragma omp simd
              for (int c = 0; c < C; ++c) a[c] += xv[c];
            }
          }
        }
        float* yo = yp + (((size_t)n * OH + oh) * OW + ow) * C;
        if (kind == 0) {
          for (int c = 0; c < C; ++c) yo[c] = (padded && pad_zero) ? std::max(acc[c], 0.f) : acc[c];
        } else {
          const float inv = cnt ? 1.f / cnt : 0.f;
          for (int c = 0; c < C; ++c) yo[c] = acc[c] * inv;
        }
      }
    }
}

// global average / max pool: x [N, P, C] -> y [N, C]
void global_pool(const Arr<float>& x, Arr<float>& y, int kind) {
  const int N = x.shape(0), C = x.shape(x.ndim() - 1);
  const long P = x.size() / ((long)N * C);
  need(y.size() == (long)N * C, "global pool shape");
  const float* xp = cptr(x);
  float* yp = mptr(y);
  py::gil_scoped_release nogil;
#pragma omp parallel for schedule(static)
  for (int n = 0; n < N; ++n) {
    std::vector<double> acc(C, kind == 0 ? 0.0 : -INFINITY);
    for (long p = 0; p < P; ++p) {
      const float* xv = xp + ((size_t)n * P + p) * C;
      if (kind == 0)
        for (int c = 0; c < C; ++c) acc[c] += xv[c];
      else
        for (int c = 0; c < C; ++c) acc[c] = std::max(acc[c], (double)xv[c]);
    }
    for (int c = 0; c < C; ++c) yp[(size_t)n * C + c] = kind == 0 ? (float)(acc[c] / P) : (float)acc[c];
  }
}

// ------------------------------------------------------------------ eltwise
// y = act(x * scale[c] + shift[c])   (standalone BN, Rescaling, Normalization)
void affine(const Arr<float>& x, const Arr<float>& scale, const Arr<float>& shift, Arr<float>& y, int act,
            float alpha) {
  const int C = x.shape(x.ndim() - 1);
  const long rows = x.size() / C;
  need(scale.size() == C && shift.size() == C && y.size() == x.size(), "affine shapes");
  const float *xp = cptr(x), *sp = cptr(scale), *hp = cptr(shift);
  float* yp = mptr(y);
  py::gil_scoped_release nogil;
#pragma omp parallel for schedule(static)
  for (long r = 0; r < rows; ++r)
    for (int c = 0; c < C; ++c) yp[r * C + c] = act_f(xp[r * C + c] * sp[c] + hp[c], act, alpha);
}

// Keras LayerNormalization over the last axis: y = (x - mu) * rsqrt(var + eps) * gamma[c] + beta[c], with the
// row's mean and its biased variance from the centred values (two passes, never E[x^2] - mu^2)
void layernorm(const Arr<float>& x, const Arr<float>& gamma, const Arr<float>& beta, Arr<float>& y, float eps) {
  const int C = x.shape(x.ndim() - 1);
  const long rows = x.size() / C;
  need(gamma.size() == C && beta.size() == C && y.size() == x.size(), "layernorm shapes");
  const float *xp = cptr(x), *gp = cptr(gamma), *bp = cptr(beta);
  float* yp = mptr(y);
  py::gil_scoped_release nogil;
#pragma omp parallel for schedule(static)
  for (long r = 0; r < rows; ++r) {
    const float* xr = xp + r * C;
    float* yr = yp + r * C;
    double s = 0.0;
    for (int c = 0; c < C; ++c) s += xr[c];
    const double mu = s / C;
    double q = 0.0;
    for (int c = 0; c < C; ++c) {
      const double d = xr[c] - mu;
      q += d * d;
    }
    const double rstd = 1.0 / std::sqrt(q / C + (double)eps);
    for (int c = 0; c < C; ++c) yr[c] = (float)((xr[c] - mu) * rstd) * gp[c] + bp[c];
  }
}

// Keras 3 RMSNormalization over the last axis: y = x * rsqrt(mean(x^2) + eps) * scale[c], the sum of squares in
// double
void rmsnorm(const Arr<float>& x, const Arr<float>& scale, Arr<float>& y, float eps) {
  const int C = x.shape(x.ndim() - 1);
  const long rows = x.size() / C;
  need(scale.size() == C && y.size() == x.size(), "rmsnorm shapes");
  const float *xp = cptr(x), *gp = cptr(scale);
  float* yp = mptr(y);
  py::gil_scoped_release nogil;
#pragma omp parallel for schedule(static)
  for (long r = 0; r < rows; ++r) {
    const float* xr = xp + r * C;
    float* yr = yp + r * C;
    double q = 0.0;
    for (int c = 0; c < C; ++c) q += (double)xr[c] * xr[c];
    const double rstd = 1.0 / std::sqrt(q / C + (double)eps);
    for (int c = 0; c < C; ++c) yr[c] = (float)(xr[c] * rstd) * gp[c];
  }
}

// Rotary position embedding, rotate-half convention (the GPU op's arguments, csrc/kernels/layers.hip): x / y
// [rows][ld] rows of [Q: hq x d | K: hkv x d | V: hkv x dv | rest], the position of a row is row % T, table
// [2][T][d / 2] holds cos then sin.  Q and K heads are rotated in fp32, V is copied, the rest of a row becomes zero.
void rope(const Arr<float>& x, const Arr<float>& table, Arr<float>& y, int T, int hq, int hkv, int d, int dv) {
  need(x.ndim() >= 2 && T >= 1 && hq >= 1 && hkv >= 1 && d >= 2 && d % 2 == 0 && dv >= 1, "rope args (d is even)");
  const long ld = x.shape(x.ndim() - 1), rows = x.size() / ld;
  const long rotw = (long)(hq + hkv) * d, W = rotw + (long)hkv * dv;
  const int half = d / 2;
  need(y.size() == x.size() && y.shape(y.ndim() - 1) == ld && W <= ld && rows % T == 0 &&
           table.size() == 2l * T * half, "rope shapes");
  const float *xp = cptr(x), *tp = cptr(table);
  float* yp = mptr(y);
  need(xp != yp, "rope is out of place");
  py::gil_scoped_release nogil;
#pragma omp parallel for schedule(static)
  for (long r = 0; r < rows; ++r) {
    const float* xr = xp + r * ld;
    float* yr = yp + r * ld;
    const float* cs = tp + (r % T) * half;
    const float* sn = cs + (long)T * half;
    for (int h = 0; h < hq + hkv; ++h)
      for (int i = 0; i < half; ++i) {
        const float a = xr[h * d + i], b = xr[h * d + i + half];
        yr[h * d + i] = a * cs[i] - b * sn[i];
        yr[h * d + i + half] = b * cs[i] + a * sn[i];
      }
    for (long c = rotw; c < W; ++c) yr[c] = xr[c];
    for (long c = W; c < ld; ++c) yr[c] = 0.f;
  }
}

// Keras GroupNormalization on an NHWC map: per (image, group) the mean and the biased variance over (H, W, C / G)
// from the centred values (two passes in double, never E[x^2] - mu^2), then
// y = act((x - mu) * rsqrt(var + eps) * gamma[c] + beta[c])
void groupnorm(const Arr<float>& x, const Arr<float>& gamma, const Arr<float>& beta, Arr<float>& y, int groups,
               float eps, int act, float alpha) {
  need(x.ndim() == 4 && y.ndim() == 4, "groupnorm ranks");
  const int N = x.shape(0), C = x.shape(3);
  const long P = (long)x.shape(1) * x.shape(2);
  need(N >= 1 && P >= 1 && C >= 1 && groups >= 1 && C % groups == 0, "groupnorm groups");
  need(y.shape(0) == N && y.shape(1) == x.shape(1) && y.shape(2) == x.shape(2) && y.shape(3) == C &&
           gamma.size() == C && beta.size() == C, "groupnorm shapes");
  const int Cg = C / groups;
  const float *xp = cptr(x), *gp = cptr(gamma), *bp = cptr(beta);
  float* yp = mptr(y);
  py::gil_scoped_release nogil;
#pragma omp parallel for collapse(2) schedule(static)
  for (int n = 0; n < N; ++n)
    for (int g = 0; g < groups; ++g) {
      const float* xb = xp + (long)n * P * C + (long)g * Cg;
      float* yb = yp + (long)n * P * C + (long)g * Cg;
      double s = 0.0;
      for (long p = 0; p < P; ++p)
        for (int c = 0; c < Cg; ++c) s += xb[p * C + c];
      const double mu = s / ((double)P * Cg);
      double q = 0.0;
      for (long p = 0; p < P; ++p)
        for (int c = 0; c < Cg; ++c) {
          const double d = xb[p * C + c] - mu;
          q += d * d;
        }
      const double rstd = 1.0 / std::sqrt(q / ((double)P * Cg) + (double)eps);
      for (long p = 0; p < P; ++p)
        for (int c = 0; c < Cg; ++c)
          yb[p * C + c] = act_f((float)((xb[p * C + c] - mu) * rstd) * gp[g * Cg + c] + bp[g * Cg + c], act, alpha);
    }
}

// y = act(x)
void activation(const Arr<float>& x, Arr<float>& y, int act, float alpha) {
  need(y.size() == x.size(), "act shapes");
  const float* xp = cptr(x);
  float* yp = mptr(y);
  const long n = x.size();
  py::gil_scoped_release nogil;
#pragma omp parallel for schedule(static)
  for (long i = 0; i < n; ++i) yp[i] = act_f(xp[i], act, alpha);
}

// y = act(a (op) b); b is either a's shape or one channel row per image
// ([N, C] broadcast over a's pixels).  op: 0 add, 1 mul, 2 sub, 3 max, 4 min, 5 avg
void binary(const Arr<float>& a, const Arr<float>& b, Arr<float>& y, int op, int act, float alpha) {
  need(y.size() == a.size(), "binary shapes");
  const int N = a.shape(0), C = a.shape(a.ndim() - 1);
  const long per = a.size() / N;
  const bool bcast = b.size() != a.size();
  need(!bcast || b.size() == (long)N * C, "binary broadcast shape");
  const float *ap = cptr(a), *bp = cptr(b);
  float* yp = mptr(y);
  const long n = a.size();
  py::gil_scoped_release nogil;
#pragma omp parallel for schedule(static)
  for (long i = 0; i < n; ++i) {
    const float u = ap[i];
    const float v = bcast ? bp[(i / per) * C + i % C] : bp[i];
    float r;
    switch (op) {
      case 0: r = u + v; break;
      case 1: r = u * v; break;
      case 2: r = u - v; break;
      case 3: r = std::max(u, v); break;
      case 4: r = std::min(u, v); break;
      default: r = 0.5f * (u + v); break;
    }
    yp[i] = act_f(r, act, alpha);
  }
}

// row softmax over the last axis (in place allowed)
void softmax(const Arr<float>& x, Arr<float>& y) {
  const int C = x.shape(x.ndim() - 1);
  const long rows = x.size() / C;
  need(y.size() == x.size(), "softmax shapes");
  const float* xp = cptr(x);
  float* yp = mptr(y);
  py::gil_scoped_release nogil;
#pragma omp parallel for schedule(static)
  for (long r = 0; r < rows; ++r) {
    const float* xr = xp + r * C;
    float* yr = yp + r * C;
    float m = -INFINITY;
    for (int c = 0; c < C; ++c) m = std::max(m, xr[c]);
    double s = 0.0;
    for (int c = 0; c < C; ++c) {
      const float e = std::exp(xr[c] - m);
      yr[c] = e;
      s += e;
    }
    const float inv = (float)(1.0 / s);
    for (int c = 0; c < C; ++c) yr[c] *= inv;
  }
}

// copy x [N,H,W,C] into y [N,H+t+b,W+l+r,C] at (t, l), zeros around
void zero_pad(const Arr<float>& x, Arr<float>& y, int t, int l) {
  const int N = x.shape(0), H = x.shape(1), W = x.shape(2), C = x.shape(3), OH = y.shape(1), OW = y.shape(2);
  const float* xp = cptr(x);
  float* yp = mptr(y);
  py::gil_scoped_release nogil;
  std::memset(yp, 0, sizeof(float) * y.size());
#pragma omp parallel for collapse(2) schedule(static)
  for (int n = 0; n < N; ++n)
    for (int h = 0; h < H; ++h)
      std::memcpy(yp + (((size_t)n * OH + h + t) * OW + l) * C, xp + (((size_t)n * H + h) * W) * C,
                  sizeof(float) * W * C);
}

// channel concat of equal-pixel tensors: y [..., sum C_i]
void concat(const py::list& xs, Arr<float>& y) {
  const int CT = y.shape(y.ndim() - 1);
  const long rows = y.size() / CT;
  std::vector<Arr<float>> ins;
  for (auto h : xs) ins.push_back(h.cast<Arr<float>>());
  float* yp = mptr(y);
  int off = 0;
  for (auto& a : ins) {
    const int C = a.shape(a.ndim() - 1);
    need(a.size() == rows * C, "concat shapes");
    const float* ap = a.data();
#pragma omp parallel for schedule(static)
    for (long r = 0; r < rows; ++r) std::memcpy(yp + r * CT + off, ap + r * C, sizeof(float) * C);
    off += C;
  }
  need(off == CT, "concat channel total");
}

int threads() { return omp_get_max_threads(); }
void set_threads(int n) { omp_set_num_threads(n); }

}  // namespace

PYBIND11_MODULE(_cpu, m) {
  m.doc() = "ADAPT native CPU ops (OpenMP, NHWC fp32): the CPU stage / local_infer execution path";
  m.attr("COB") = COB;
  m.def("conv2d", &conv2d, py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("y"), py::arg("stride"),
        py::arg("pad_t"), py::arg("pad_l"), py::arg("act") = 0, py::arg("alpha") = 0.3f,
        py::arg("residual") = py::none());
  m.def("gconv2d", &gconv2d, py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("y"), py::arg("stride"),
        py::arg("pad_t"), py::arg("pad_l"), py::arg("groups"), py::arg("act") = 0, py::arg("alpha") = 0.3f);
  m.def("deconv2d", &deconv2d, py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("y"), py::arg("stride"),
        py::arg("pad_t"), py::arg("pad_l"), py::arg("act") = 0, py::arg("alpha") = 0.3f);
  m.def("upsample2d", &upsample2d, py::arg("x"), py::arg("y"), py::arg("sh"), py::arg("sw"), py::arg("bilinear"));
  m.def("crop2d", &crop2d, py::arg("x"), py::arg("y"), py::arg("t"), py::arg("l"));
  m.def("dwconv2d", &dwconv2d, py::arg("x"), py::arg("w"), py::arg("bias"), py::arg("y"), py::arg("stride"),
        py::arg("pad_t"), py::arg("pad_l"), py::arg("act") = 0, py::arg("alpha") = 0.3f);
  m.def("pool2d", &pool2d, py::arg("x"), py::arg("y"), py::arg("kind"), py::arg("kh"), py::arg("kw"),
        py::arg("stride"), py::arg("pad_t"), py::arg("pad_l"), py::arg("pad_zero"));
  m.def("global_pool", &global_pool, py::arg("x"), py::arg("y"), py::arg("kind") = 0);
  m.def("affine", &affine, py::arg("x"), py::arg("scale"), py::arg("shift"), py::arg("y"), py::arg("act") = 0,
        py::arg("alpha") = 0.3f);
  m.def("attention", &attention, py::arg("qkv"), py::arg("out"), py::arg("B"), py::arg("T"), py::arg("heads"),
        py::arg("key_dim"), py::arg("value_dim"), py::arg("causal") = false, py::arg("key_mask") = py::none(),
        py::arg("kv_heads") = 0);
  m.def("embedding", &embedding, py::arg("ids"), py::arg("table"), py::arg("out"));
  m.def("window_attention", &window_attention, py::arg("qkv"), py::arg("table"), py::arg("out"), py::arg("B"),
        py::arg("H"), py::arg("W"), py::arg("window"), py::arg("shift"), py::arg("heads"), py::arg("key_dim"));
  m.def("space_to_depth", &space_to_depth, py::arg("x"), py::arg("y"));
  m.def("cross_attention", &cross_attention, py::arg("q"), py::arg("k"), py::arg("v"), py::arg("out"), py::arg("B"),
        py::arg("Tq"), py::arg("Tk"), py::arg("heads"), py::arg("d"), py::arg("dv"));
  m.def("queries", &queries, py::arg("emb"), py::arg("out"), py::arg("B"));
  m.def("layernorm", &layernorm, py::arg("x"), py::arg("gamma"), py::arg("beta"), py::arg("y"), py::arg("eps"));
  m.def("rmsnorm", &rmsnorm, py::arg("x"), py::arg("scale"), py::arg("y"), py::arg("eps"));
  m.def("rope", &rope, py::arg("x"), py::arg("table"), py::arg("y"), py::arg("T"), py::arg("hq"), py::arg("hkv"),
        py::arg("key_dim"), py::arg("value_dim"));
  m.def("groupnorm", &groupnorm, py::arg("x"), py::arg("gamma"), py::arg("beta"), py::arg("y"), py::arg("groups"),
        py::arg("eps"), py::arg("act") = 0, py::arg("alpha") = 0.3f);
  m.def("activation", &activation, py::arg("x"), py::arg("y"), py::arg("act"), py::arg("alpha") = 0.3f);
  m.def("binary", &binary, py::arg("a"), py::arg("b"), py::arg("y"), py::arg("op"), py::arg("act") = 0,
        py::arg("alpha") = 0.3f);
  m.def("softmax", &softmax, py::arg("x"), py::arg("y"));
  m.def("zero_pad", &zero_pad, py::arg("x"), py::arg("y"), py::arg("t"), py::arg("l"));
  m.def("concat", &concat, py::arg("xs"), py::arg("y"));
  m.def("threads", &threads);
  m.def("set_threads", &set_threads, py::arg("n"));
}
