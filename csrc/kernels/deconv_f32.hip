// Transposed convolution (Keras Conv2DTranspose, no output_padding, no dilation), NHWC, for gfx950:
//   F[b][i*S + t][j*S + u][n] += x[b][i][j][c] * w[t][u][c][n]          (full scatter frame, no kernel flip)
//   out[b][oy][ox][n] = act(F[b][oy + PT][ox + PL][n] + bias[n])         (zero where the frame ends: KH < S)
// with BN folded into w / bias, any kh x kw and stride, activation modes 0-2 (linear, ReLU, ReLU6).  No
// workspace, no atomics, no zero-stuffed input, no host sync: one launch on the caller's stream
// (graph-capturable); every output element is written exactly once, so the result is deterministic.
//
// Gather (output-stationary) form.  An output position with frame coordinate f = o + P belongs to phase
// f mod S on each axis; its taps are the t == f (mod S), and tap t = p + S a reads input i = m - a with
// m = (f - p) / S.  So each of the S x S phases is a stride-1 correlation of x with the ceil((K - p) / S)
// taps of its residue class, over the output pixels of that class: an implicit GEMM with M = the phase's
// pixels over the batch, K = the phase's taps x Cin, N = Cout.  A phase without taps (KH < S) is
// act(bias).  The MACs are the true H * W * KH * KW * Cin * Cout: none of the S^2 - 1 of every S^2
// products that a zero-stuffed input would multiply by zero.
//
// Two paths behind deconv_f32_forward (the caller names the path; ops/conv.py `deconv_path` holds the
// shape rule and the launcher re-checks it):
//
// * MFMA path (v_mfma_f32_16x16x4_f32): Cin % 16 == 0 and Cout % 16 == 0, every kernel, stride and
//   padding.  The host packs the weights once, per phase, N tile of 16 output channels, tap slot and
//   16-channel K chunk, in fragment order: [S*S][Cout/16][TA*TB][Cin/16][64 lanes][4], TA = ceil(KH / S),
//   TB = ceil(KW / S); tap slot (a, b) of phase (py, px) is tap (py + S a, px + S b), slots past the
//   kernel are zero and never read.  GEMM transposed as in gconv_f32.hip (A = weights, B = activations,
//   D = [channel][pixel]): a lane ends with 4 consecutive channels of one pixel and stores them as one
//   16-byte vector.
//
//   A block of 4 waves owns a TR x TW tile (at most 128 pixels, 8 fragments of 16) of one phase's pixel
//   grid in one image and 64 N columns; wave w owns N tile w of them, so all 16 pixels of an MFMA tile
//   and all of a wave's work belong to one phase and the tap set is wave-uniform.  Per 64-channel K
//   chunk the block stages the input halo of its tile ((TR + taps_y - 1) x (TW + taps_x - 1) input
//   pixels, zero outside the image; every global read is predicated on its address) in LDS once with
//   16-byte accesses, laid out [16-channel slab][halo pixel][16] so that one ds_read_b128 per lane feeds
//   four k-steps; the weights of a tap come from L2, one 16-byte load per lane and 16-channel chunk.
//
//   K == S (U-Net's 2x2 stride 2): every phase is a 1x1 with the same A operand, input pixel (i, j).
//   The launch is then one GEMM over the input pixels with N = S*S*Cout: the 64 N columns of a block run
//   through the phases (a wave's 16 columns lie in one phase), the staged x tile is shared by all of
//   them, and the epilogue scatters each wave's column block to its sub-pixel (S i + py, S j + px):
//   depth-to-space.  The N tiles of a pixel tile are adjacent in launch order, so that the other N tiles'
//   re-reads of the x tile can come from L2 (intended; not measured).
//
// * Generic path: every other shape.  One thread per output element, weights [KH][KW][Cin][Cout], plain
//   bounds-checked loops over the taps of the element's phase.  It is also the bf16 kernel (bf16 in and
//   out, fp32 weights and accumulate, rows of Cp = channels padded to 8: padding channels are never read
//   and are written as zeros).
#include "kernels.h"

namespace adapt {

namespace {

constexpr int DC_NT = 256;          // threads per block (4 waves)
constexpr int DC_BN = 64;           // N columns per block (one 16-column tile per wave)
constexpr int DC_CK = 64;           // input channels staged per K chunk
constexpr int DC_MAXPX = 128;       // output pixels per tile (8 fragments of 16)
constexpr int DC_MAXHP = 256;       // halo pixels per tile: 256 B each per chunk -> 64 KB of LDS, two blocks per CU

struct DeconvTile {
  int TR, TW;        // phase-grid rows / columns per tile
  int nth, ntw;      // tiles per image over the largest phase grid
  int ntn;           // N tiles of 64 per pixel tile
  int fused;         // K == S: one GEMM with N = S*S*Cout
};

// One axis of a phase: first output coordinate, count of outputs, taps, and m of the first output
struct PhaseAxis {
  int o0, n, taps, m0;
};

__host__ __device__ inline PhaseAxis phase_axis(int p, int S, int K, int P, int O) {
  PhaseAxis a;
  a.o0 = ((p - P) % S + S) % S;
  a.n = a.o0 < O ? (O - a.o0 + S - 1) / S : 0;
  a.taps = p < K ? (K - p + S - 1) / S : 0;
  a.m0 = (a.o0 + P - p) / S;
  return a;
}

// Tile shape: fewest (halo pixels staged + pixel slots multiplied) over the largest phase grid, within
// the pixel and LDS limits, the halo sized for the phase with the most taps.  A 1 x 1 tile fits whenever
// TA * TB <= DC_MAXHP.
bool deconv_pick_tile(const DeconvF32Params& p, DeconvTile* best) {
  const int ta = (p.KH + p.S - 1) / p.S, tb = (p.KW + p.S - 1) / p.S;
  const int gy = (p.OH + p.S - 1) / p.S, gx = (p.OW + p.S - 1) / p.S;
  double best_cost = -1.0;
  for (int tr = 1; tr <= gy && tr <= DC_MAXPX; ++tr) {
    for (int parts = 1; parts <= gx; ++parts) {
      const int tw = (gx + parts - 1) / parts;
      if (parts > 1 && tw == (gx + parts - 2) / (parts - 1)) continue;    // same width as the last one
      if (tr * tw > DC_MAXPX) continue;
      const int hr = tr + ta - 1, hc = tw + tb - 1;
      if (hr * hc > DC_MAXHP) continue;
      const int nth = (gy + tr - 1) / tr, ntw = (gx + tw - 1) / tw;
      const int pf = (tr * tw + 15) / 16;
      const double cost = (double)nth * ntw * (hr * hc + pf * 16.0 + 4.0 * ta * tb);
      if (best_cost < 0.0 || cost < best_cost) {
        best_cost = cost;
        best->TR = tr, best->TW = tw, best->nth = nth, best->ntw = ntw;
      }
    }
  }
  return best_cost >= 0.0;
}

// PF: 16-pixel fragments of the tile, compile-time so that the accumulators and the activation
// fragments are plain registers
template <int PF>
__global__ __launch_bounds__(DC_NT, 2) void deconv_mfma_kernel(DeconvF32Params p, DeconvTile t) {
  extern __shared__ __attribute__((aligned(16))) char dc_lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fq = lane >> 4;
  const int SS = p.S * p.S;
  int blk = blockIdx.x;
  const int nt = blk % t.ntn;               // N tiles fastest: the blocks that share an x tile run together
  blk /= t.ntn;
  const int tx = blk % t.ntw;
  blk /= t.ntw;
  const int ty = blk % t.nth, img = blk / t.nth;

  // the block's phase (geometry and halo) and this wave's N columns
  int bph, ncol;                            // ncol: first of the wave's 16 columns, in [0, Cout) of its phase
  int wph;
  if (t.fused) {
    const int n = nt * DC_BN + wave * 16;   // column of the N = S*S*Cout GEMM
    wph = n / p.Cout;
    ncol = n - wph * p.Cout;
    bph = 0;                                // K == S: every phase has the same grid (the input pixels), one tap
  } else {
    const int nb = (p.Cout + DC_BN - 1) / DC_BN;
    bph = nt / nb;
    wph = bph;
    ncol = (nt - bph * nb) * DC_BN + wave * 16;
  }
  const PhaseAxis by = phase_axis(bph / p.S, p.S, p.KH, p.PT, p.OH);
  const PhaseAxis bx = phase_axis(bph % p.S, p.S, p.KW, p.PL, p.OW);
  const int jy0 = ty * t.TR, jx0 = tx * t.TW;
  if (jy0 >= by.n || jx0 >= bx.n) return;   // a smaller phase grid has fewer tiles (block-uniform, before any barrier)
  const bool live = wph < SS && ncol < p.Cout;       // wave-uniform: a partial N block
  const int taps = by.taps * bx.taps;
  const int HC = t.TW + max(bx.taps, 1) - 1, HR = t.TR + max(by.taps, 1) - 1;
  const int HP = HR * HC;
  const int ih0 = by.m0 + jy0 - (max(by.taps, 1) - 1), iw0 = bx.m0 + jx0 - (max(bx.taps, 1) - 1);
  const int npx = t.TR * t.TW;

  // byte offset, inside a slab, of each pixel fragment's tap (0, 0) (+ this lane's 4 channels)
  int hb[PF];
#pragma unroll
  for (int f = 0; f < PF; ++f) {
    const int px = min(f * 16 + fr, npx - 1);
    const int r = px / t.TW, c = px - r * t.TW;
    hb[f] = (((r + HR - t.TR) * HC + (c + HC - t.TW)) << 6) + (fq << 4);
  }
  const int TS = ((p.KH + p.S - 1) / p.S) * ((p.KW + p.S - 1) / p.S), TBs = (p.KW + p.S - 1) / p.S;
  const int kc16 = p.Cin >> 4;
  const f32x4* wp = (const f32x4*)p.w + ((size_t)(live ? wph : 0) * (p.Cout >> 4) + (live ? ncol >> 4 : 0)) * TS * kc16 * 64 + lane;
  f32x4 acc[PF];
#pragma unroll
  for (int f = 0; f < PF; ++f) acc[f] = (f32x4){0.f, 0.f, 0.f, 0.f};

  if (taps > 0) {
    for (int c0 = 0; c0 < p.Cin; c0 += DC_CK) {
      const int nsub = min(DC_CK, p.Cin - c0) >> 4;       // 16-channel slabs of this chunk (Cin % 16 == 0)
      if (c0) __syncthreads();                            // the last chunk's reads are done
      // halo of this pixel tile, channels c0 .. c0+63 -> LDS [slab of 16 channels][halo pixel][16];
      // four 16-byte loads in flight per thread, each predicated on its own address
      const int items = HP * 16;
      for (int i0 = tid; i0 < items; i0 += 4 * DC_NT) {
        f32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = i0 + u * DC_NT;
          const int hp = i >> 4, c = c0 + (i & 15) * 4;
          const int hr = hp / HC, hc = hp - hr * HC;
          const int ih = ih0 + hr, iw = iw0 + hc;
          v[u] = (f32x4){0.f, 0.f, 0.f, 0.f};
          if (i < items && c < p.Cin && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W)
            v[u] = *(const f32x4*)(p.x + (((size_t)img * p.H + ih) * p.W + iw) * p.Cin + c);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int i = i0 + u * DC_NT;
          const int hp = i >> 4, ch = i & 15;
          if (i < items) *(f32x4*)(dc_lds + ((((ch >> 2) * HP + hp) << 6) | ((ch & 3) << 4))) = v[u];
        }
      }
      __syncthreads();
      if (live) {
        for (int a = 0; a < by.taps; ++a) {
          for (int b = 0; b < bx.taps; ++b) {
            const int toff = (a * HC + b) << 6;           // tap (a, b) reads input (m - a, m' - b)
            const f32x4* wt = wp + ((size_t)(a * TBs + b) * kc16 + (c0 >> 4)) * 64;
            for (int j = 0; j < nsub; ++j) {
              const f32x4 wc = wt[j * 64];
              const int off = ((j * HP) << 6) - toff;     // hb[f] - toff >= 0: hb starts taps - 1 rows / columns in
              f32x4 xf[PF];
#pragma unroll
              for (int f = 0; f < PF; ++f) xf[f] = *(const f32x4*)(dc_lds + (off + hb[f]));
#pragma unroll
              for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int f = 0; f < PF; ++f)
                  acc[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(wc[s], xf[f][s], acc[f], 0, 0, 0);
            }
          }
        }
      }
    }
  }
  if (!live) return;
  // D fragment: channel ncol + 4fq + e, pixel 16f + fr of the tile; the wave's own phase places it
  const PhaseAxis wy = phase_axis(wph / p.S, p.S, p.KH, p.PT, p.OH);
  const PhaseAxis wx = phase_axis(wph % p.S, p.S, p.KW, p.PL, p.OW);
  const f32x4 bias = *(const f32x4*)(p.bias + ncol + fq * 4);
#pragma unroll
  for (int f = 0; f < PF; ++f) {
    const int px = f * 16 + fr;
    if (px < npx) {
      const int r = px / t.TW, c = px - r * t.TW;
      const int jy = jy0 + r, jx = jx0 + c;
      if (jy < wy.n && jx < wx.n) {
        const int oy = wy.o0 + jy * p.S, ox = wx.o0 + jx * p.S;
        f32x4 y;
#pragma unroll
        for (int e = 0; e < 4; ++e) y[e] = act_relu(acc[f][e] + bias[e], p.act);
        *(f32x4*)(p.out + (((size_t)img * p.OH + oy) * p.OW + ox) * p.Cout + ncol + fq * 4) = y;
      }
    }
  }
}

__device__ __forceinline__ float dc_ld(const float* q) { return *q; }
__device__ __forceinline__ float dc_ld(const bf16* q) { return bf2f(*q); }
__device__ __forceinline__ void dc_st(float* q, float v) { *q = v; }
__device__ __forceinline__ void dc_st(bf16* q, float v) { *q = f2bf(v); }

// One thread per output element of rows Cop wide (Cop == Cout for fp32; bf16 rows are padded to 8);
// x rows are Cip wide.  w is [KH][KW][Cin][Cout] fp32, bias [Cout] fp32.
template <typename T>
__global__ __launch_bounds__(DC_NT) void deconv_generic_kernel(const T* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ bias, T* __restrict__ out,
                                                              DeconvF32Params p, int Cip, int Cop, size_t total) {
  const size_t idx = (size_t)blockIdx.x * DC_NT + threadIdx.x;
  if (idx >= total) return;
  const int n = (int)(idx % Cop);
  size_t pix = idx / Cop;
  const int ox = (int)(pix % p.OW);
  pix /= p.OW;
  const int oy = (int)(pix % p.OH), img = (int)(pix / p.OH);
  if (n >= p.Cout) {                        // a padding channel of the bf16 layout
    dc_st(out + idx, 0.f);
    return;
  }
  const int fy = oy + p.PT, fx = ox + p.PL;
  float acc = 0.f;
  for (int ty = fy % p.S; ty < p.KH; ty += p.S) {
    const int iy = (fy - ty) / p.S;
    if (fy < ty || iy >= p.H) continue;
    for (int tx = fx % p.S; tx < p.KW; tx += p.S) {
      const int ix = (fx - tx) / p.S;
      if (fx < tx || ix >= p.W) continue;
      const T* xp = x + (((size_t)img * p.H + iy) * p.W + ix) * Cip;
      const float* wq = w + (size_t)(ty * p.KW + tx) * p.Cin * p.Cout + n;
      for (int ci = 0; ci < p.Cin; ++ci) acc = fmaf(dc_ld(xp + ci), wq[(size_t)ci * p.Cout], acc);
    }
  }
  dc_st(out + idx, act_relu(acc + bias[n], p.act));
}

bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

bool deconv_params_ok(const DeconvF32Params& p) {
  if (p.B < 1 || p.H < 1 || p.W < 1 || p.Cin < 1 || p.Cout < 1 || p.OH < 1 || p.OW < 1 || p.KH < 1 || p.KW < 1 ||
      p.S < 1 || p.PT < 0 || p.PL < 0 || p.act < 0 || p.act > ACT_RELU6)
    return false;
  // the output window lies inside the frame extended to whole strides: rows past (H - 1) S + KH are bias only
  return p.PT + p.OH <= p.H * p.S + p.KH && p.PL + p.OW <= p.W * p.S + p.KW &&
         (double)p.B * p.OH * p.OW * max(p.Cout, 8) < 9.0e18;
}

}  // namespace

bool deconv_f32_mfma_ok(int Cin, int Cout, int KH, int KW, int S) {
  if (Cin < 16 || Cout < 16 || Cin % 16 || Cout % 16 || S < 1 || KH < 1 || KW < 1) return false;
  return (long)((KH + S - 1) / S) * ((KW + S - 1) / S) <= DC_MAXHP;
}

hipError_t deconv_f32_forward(const DeconvF32Params& p, bool mfma, hipStream_t s) {
  if (!deconv_params_ok(p)) return hipErrorInvalidValue;
  if (mfma) {
    DeconvTile t;
    if (!deconv_f32_mfma_ok(p.Cin, p.Cout, p.KH, p.KW, p.S) || !aligned16(p.x) || !aligned16(p.w) ||
        !aligned16(p.bias) || !aligned16(p.out) || !deconv_pick_tile(p, &t))
      return hipErrorInvalidValue;
    t.fused = p.KH == p.S && p.KW == p.S && p.PT == 0 && p.PL == 0;
    const int SS = p.S * p.S;
    t.ntn = t.fused ? (SS * p.Cout + DC_BN - 1) / DC_BN : SS * ((p.Cout + DC_BN - 1) / DC_BN);
    const size_t blocks = (size_t)p.B * t.nth * t.ntw * t.ntn;
    if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
    const int ta = (p.KH + p.S - 1) / p.S, tb = (p.KW + p.S - 1) / p.S;
    const size_t lds = (size_t)(t.TR + ta - 1) * (t.TW + tb - 1) * 256;
    const dim3 grid((unsigned)blocks);
    switch ((t.TR * t.TW + 15) / 16) {
#define DC_CASE(PF) \
  case PF: hipLaunchKernelGGL((deconv_mfma_kernel<PF>), grid, dim3(DC_NT), lds, s, p, t); break;
      DC_CASE(1) DC_CASE(2) DC_CASE(3) DC_CASE(4) DC_CASE(5) DC_CASE(6) DC_CASE(7) DC_CASE(8)
#undef DC_CASE
      default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
  }
  const size_t total = (size_t)p.B * p.OH * p.OW * p.Cout;
  const size_t blocks = (total + DC_NT - 1) / DC_NT;
  if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
  hipLaunchKernelGGL(deconv_generic_kernel<float>, dim3((unsigned)blocks), dim3(DC_NT), 0, s, p.x, p.w, p.bias, p.out,
                     p, p.Cin, p.Cout, total);
  return hipGetLastError();
}

hipError_t deconv_bf16_forward(const bf16* x, const float* w, const float* bias, bf16* out, const DeconvF32Params& p,
                               int Cip, int Cop, hipStream_t s) {
  if (!deconv_params_ok(p) || Cip < p.Cin || Cop < p.Cout) return hipErrorInvalidValue;
  const size_t total = (size_t)p.B * p.OH * p.OW * Cop;
  const size_t blocks = (total + DC_NT - 1) / DC_NT;
  if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
  hipLaunchKernelGGL(deconv_generic_kernel<bf16>, dim3((unsigned)blocks), dim3(DC_NT), 0, s, x, w, bias, out, p, Cip,
                     Cop, total);
  return hipGetLastError();
}

}  // namespace adapt
