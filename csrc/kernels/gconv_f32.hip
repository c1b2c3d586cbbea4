// Grouped convolution (Keras Conv2D(groups = G > 1)), fp32 NHWC, for gfx950:
//   out[b][oh][ow][n] = act(sum_{kh,kw,ci in group(n)} x[b][ih][iw][ci] * w[kh][kw][ci - c0(n)][n] + bias[n])
// with BN folded into w / bias, any kh x kw, stride 1 or 2, explicit top / left
// pads (bottom / right follow from OH / OW), activation modes 0-2 (linear, ReLU,
// ReLU6).  No workspace, no host sync: one launch on the caller's stream
// (graph-capturable).
//
// A grouped filter is block-diagonal: output channel n reads only the
// Cin / G input channels of its group, so none of the dense implicit-GEMM,
// Winograd or pointwise kernels can express it without multiplying G-1 of
// every G weights by zero.  ResNeXt's 32 x 4d blocks have 4 .. 32 channels per
// group; there the layer is bound by its activation traffic, not by the
// matrix cores.
//
// Two paths behind gconv_f32_forward (the caller names the path; ops/conv.py
// `gconv_path` holds the shape rule and the launcher re-checks it):
//
// * MFMA path (v_mfma_f32_16x16x4_f32): Cin / G == Cout / G == CG in
//   {4, 8, 16, 32}, Cout % 16 == 0.  An N tile is 16 consecutive output
//   channels; its K range is taps x the 16 (CG <= 16) or 32 (CG = 32)
//   contiguous input channels of the group(s) it covers.  The host packs the
//   tile's weights as a dense [tap][chunk of 16 channels][16] block in fragment
//   order, with zeros off the group diagonal for CG 4 / 8 (4x / 2x wasted
//   MFMA work, at widths where the activations are the bound).
//
//   Structure built: a block of 4 waves owns a TR x TW tile of output pixels
//   (at most 128) of one image and 64 consecutive channels; wave w owns N tile
//   w of them.  The block stages the input halo of its pixel tile for those 64
//   channels in LDS once (zero outside the image; every global read is
//   predicated on its address, so pad rows, partial tiles and partial channel
//   blocks never leave the buffer), laid out [16-channel slab][halo pixel][16]
//   so that one ds_read_b128 per lane feeds the four k-steps of a 16-channel
//   chunk: lane (fr, fq) reads channels 4fq .. 4fq+3 of pixel fr, and k-step s
//   pairs channel 4fq+s with the weight the host put in the same slot.
//   GEMM transposed as in pw_f32.hip (A = weights, B = activations,
//   D = [channel][pixel]): a lane ends with 4 consecutive channels of one
//   pixel and stores them as one 16-byte vector, no LDS staging of the output.
//
//   The issue text suggested keeping a wave's packed weights in VGPRs for
//   the whole launch (conv3x3_rr.hip).  That fixes the tap count at compile
//   time (36 / 72 registers for a 3x3, 100 / 200 for a 5x5); here the weights
//   of one tap (one 16-byte load per lane and chunk, the next tap's prefetched
//   under the current tap's MFMAs, L2-resident: 9 .. 18 KB per N tile) are
//   read per tap, so one kernel takes every kh x kw and a wave keeps all 8
//   pixel fragments' accumulators and activations in registers.
//
// * Generic path: everything else (Cin / G != Cout / G, CG = 1, 2, 12, ...,
//   Cout % 16 != 0).  One thread per output element, weights in Keras layout
//   [kh][kw][Cin / G][Cout], plain bounds-checked loops, no MFMA.  It exists so
//   that no legal Keras `groups` is refused.
#include "kernels.h"

namespace adapt {

namespace {

constexpr int GC_NT = 256;          // threads per block (4 waves)
constexpr int GC_BN = 64;           // channels per block (one 16-channel N tile per wave)
constexpr int GC_MAXPX = 128;       // output pixels per tile (8 fragments of 16)
constexpr int GC_MAXHP = 256;       // halo pixels per tile: 256 B each -> 64 KB of LDS, two blocks per CU

struct GconvTile {
  int TR, TW;        // output rows / columns per tile
  int HR, HC;        // halo rows / columns: (T - 1) * S + K
  int nth, ntw;      // tiles per image, vertically / horizontally
};

// Tile shape: fewest (halo pixels staged + pixel slots multiplied + a fixed
// per-tile cost for the weight stream) over the whole map, within the pixel
// and LDS limits.  A 1 x 1 tile always fits when the filter itself does.
bool gconv_pick_tile(const GconvF32Params& p, GconvTile* best) {
  double best_cost = -1.0;
  const int taps = p.KH * p.KW;
  for (int tr = 1; tr <= p.OH && tr <= GC_MAXPX; ++tr) {
    for (int parts = 1; parts <= p.OW; ++parts) {
      const int tw = (p.OW + parts - 1) / parts;
      if (parts > 1 && tw == (p.OW + parts - 2) / (parts - 1)) continue;    // same width as the last one
      if (tr * tw > GC_MAXPX) continue;
      const int hr = (tr - 1) * p.S + p.KH, hc = (tw - 1) * p.S + p.KW;
      if (hr * hc > GC_MAXHP) continue;
      const int nth = (p.OH + tr - 1) / tr, ntw = (p.OW + tw - 1) / tw;
      const int pf = (tr * tw + 15) / 16;
      const double cost = (double)nth * ntw * (hr * hc + pf * 16.0 + 4.0 * taps);
      if (best_cost < 0.0 || cost < best_cost) {
        best_cost = cost;
        *best = GconvTile{tr, tw, hr, hc, nth, ntw};
      }
    }
  }
  return best_cost >= 0.0;
}

// NJ: 16-channel chunks of an N tile's K range (1: CG <= 16, 2: CG = 32);
// PF: 16-pixel fragments of the tile, compile-time so that the accumulators and
// the activation fragments are plain registers and the tap body is straight-line
template <int NJ, int PF>
__global__ __launch_bounds__(GC_NT, 2) void gconv_mfma_kernel(GconvF32Params p, GconvTile t) {
  extern __shared__ __attribute__((aligned(16))) char gc_lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int HP = t.HR * t.HC;
  int tile = blockIdx.x;
  const int tx = tile % t.ntw;
  tile /= t.ntw;
  const int ty = tile % t.nth, img = tile / t.nth;
  const int oh0 = ty * t.TR, ow0 = tx * t.TW;
  const int n0 = blockIdx.y * GC_BN;
  const int ih0 = oh0 * p.S - p.PT, iw0 = ow0 * p.S - p.PL;

  // halo of this pixel tile, channels n0 .. n0+63 -> LDS [slab of 16 channels][halo pixel][16];
  // four 16-byte loads in flight per thread, each predicated on its own address
  const int items = HP * 16;
  for (int i0 = tid; i0 < items; i0 += 4 * GC_NT) {
    f32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + u * GC_NT;
      const int hp = i >> 4, c = n0 + (i & 15) * 4;
      const int hr = hp / t.HC, hc = hp - hr * t.HC;
      const int ih = ih0 + hr, iw = iw0 + hc;
      v[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
      if (i < items && c < p.Cin && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W)
        v[u] = *(const f32x4*)(p.x + (((size_t)img * p.H + ih) * p.W + iw) * p.Cin + c);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + u * GC_NT;
      const int hp = i >> 4, ch = i & 15;
      if (i < items) *(f32x4*)(gc_lds + ((((ch >> 2) * HP + hp) << 6) | ((ch & 3) << 4))) = v[u];
    }
  }
  __syncthreads();

  const int nw = n0 + wave * 16;                 // this wave's N tile
  if (nw >= p.Cout) return;                      // partial channel block (wave-uniform; no barrier follows)
  const int npx = t.TR * t.TW;
  const int taps = p.KH * p.KW;
  // byte offset, inside a slab, of each pixel fragment's top-left tap (+ this lane's 4 channels)
  int hb[PF];
#pragma unroll
  for (int f = 0; f < PF; ++f) {
    const int px = min(f * 16 + fr, npx - 1);
    const int r = px / t.TW, c = px - r * t.TW;
    hb[f] = ((r * p.S * t.HC + c * p.S) << 6) + (fq << 4);
  }
  const int slab0 = NJ == 1 ? wave : (wave & ~1);
  const f32x4* wp = (const f32x4*)p.w + (size_t)(nw >> 4) * taps * NJ * 64 + lane;
  f32x4 wc[NJ], wn[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) wc[j] = wn[j] = wp[j * 64];
  f32x4 acc[PF];
#pragma unroll
  for (int f = 0; f < PF; ++f) acc[f] = (f32x4){0.f, 0.f, 0.f, 0.f};
  int kh = 0, kw = 0;
  for (int tap = 0; tap < taps; ++tap) {
    if (tap + 1 < taps) {
#pragma unroll
      for (int j = 0; j < NJ; ++j) wn[j] = wp[((tap + 1) * NJ + j) * 64];
    }
    const int toff = (kh * t.HC + kw) << 6;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const char* base = gc_lds + (((slab0 + j) * HP) << 6) + toff;
      f32x4 xf[PF];
#pragma unroll
      for (int f = 0; f < PF; ++f) xf[f] = *(const f32x4*)(base + hb[f]);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int f = 0; f < PF; ++f)
          acc[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[j][s], xf[f][s], acc[f], 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) wc[j] = wn[j];
    if (++kw == p.KW) {
      kw = 0;
      ++kh;
    }
  }
  // D fragment: channel nw + 4fq + e, pixel 16f + fr
  const f32x4 bias = *(const f32x4*)(p.bias + nw + fq * 4);
#pragma unroll
  for (int f = 0; f < PF; ++f) {
    const int px = f * 16 + fr;
    if (px < npx) {
      const int r = px / t.TW, c = px - r * t.TW;
      const int oh = oh0 + r, ow = ow0 + c;
      if (oh < p.OH && ow < p.OW) {
        f32x4 y;
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = act_relu(acc[f][e] + bias[e], p.act);
        *(f32x4*)(p.out + (((size_t)img * p.OH + oh) * p.OW + ow) * p.Cout + nw + fq * 4) = y;
      }
    }
  }
}

// one thread per output element; w is [KH][KW][Cin/G][Cout] (Keras layout)
__global__ __launch_bounds__(GC_NT) void gconv_generic_kernel(GconvF32Params p, size_t total) {
  const size_t idx = (size_t)blockIdx.x * GC_NT + threadIdx.x;
  if (idx >= total) return;
  const int n = (int)(idx % p.Cout);
  size_t pix = idx / p.Cout;
  const int ow = (int)(pix % p.OW);
  pix /= p.OW;
  const int oh = (int)(pix % p.OH), img = (int)(pix / p.OH);
  const int cgi = p.Cin / p.G, cgo = p.Cout / p.G;
  const int ci0 = (n / cgo) * cgi;
  float acc = 0.f;
  for (int kh = 0; kh < p.KH; ++kh) {
    const int ih = oh * p.S - p.PT + kh;
    if ((unsigned)ih >= (unsigned)p.H) continue;
    for (int kw = 0; kw < p.KW; ++kw) {
      const int iw = ow * p.S - p.PL + kw;
      if ((unsigned)iw >= (unsigned)p.W) continue;
      const float* xp = p.x + (((size_t)img * p.H + ih) * p.W + iw) * p.Cin + ci0;
      const float* wq = p.w + (size_t)(kh * p.KW + kw) * cgi * p.Cout + n;
      for (int ci = 0; ci < cgi; ++ci) acc = fmaf(xp[ci], wq[(size_t)ci * p.Cout], acc);
    }
  }
  p.out[idx] = act_relu(acc + p.bias[n], p.act);
}

bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

template <int NJ>
void gconv_mfma_launch(const GconvF32Params& p, const GconvTile& t, dim3 grid, size_t lds, hipStream_t s) {
  switch ((t.TR * t.TW + 15) / 16) {
#define GC_CASE(PF) \
  case PF: hipLaunchKernelGGL((gconv_mfma_kernel<NJ, PF>), grid, dim3(GC_NT), lds, s, p, t); break;
    GC_CASE(1) GC_CASE(2) GC_CASE(3) GC_CASE(4) GC_CASE(5) GC_CASE(6) GC_CASE(7) GC_CASE(8)
#undef GC_CASE
  }
}

}  // namespace

bool gconv_f32_mfma_ok(int Cin, int Cout, int G) {
  if (G < 1 || Cin % G || Cout % G || Cin != Cout || Cout % 16) return false;
  const int cg = Cin / G;
  return cg == 4 || cg == 8 || cg == 16 || cg == 32;
}

hipError_t gconv_f32_forward(const GconvF32Params& p, bool mfma, hipStream_t s) {
  if (p.B < 1 || p.H < 1 || p.W < 1 || p.OH < 1 || p.OW < 1 || p.G < 1 || p.Cin % p.G || p.Cout % p.G ||
      p.KH < 1 || p.KW < 1 || (p.S != 1 && p.S != 2) || p.PT < 0 || p.PL < 0 || p.act < 0 || p.act > ACT_RELU6)
    return hipErrorInvalidValue;
  // the last window must start inside the padded map: rows / columns past H / W read as zero
  if ((p.OH - 1) * p.S - p.PT >= p.H || (p.OW - 1) * p.S - p.PL >= p.W) return hipErrorInvalidValue;
  if (mfma) {
    GconvTile t;
    if (!gconv_f32_mfma_ok(p.Cin, p.Cout, p.G) || !aligned16(p.x) ||
        !aligned16(p.w) || !aligned16(p.bias) || !aligned16(p.out) || !gconv_pick_tile(p, &t))
      return hipErrorInvalidValue;
    const size_t tiles = (size_t)p.B * t.nth * t.ntw;
    if (tiles > 0x7fffffffu) return hipErrorInvalidValue;
    const dim3 grid((unsigned)tiles, (unsigned)((p.Cout + GC_BN - 1) / GC_BN));
    const size_t lds = (size_t)t.HR * t.HC * 256;
    if (p.Cin / p.G == 32) gconv_mfma_launch<2>(p, t, grid, lds, s);
    else gconv_mfma_launch<1>(p, t, grid, lds, s);
    return hipGetLastError();
  }
  const size_t total = (size_t)p.B * p.OH * p.OW * p.Cout;
  const size_t blocks = (total + GC_NT - 1) / GC_NT;
  if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gconv_generic_kernel, dim3((unsigned)blocks), dim3(GC_NT), 0, s, p, total);
  return hipGetLastError();
}

}  // namespace adapt
