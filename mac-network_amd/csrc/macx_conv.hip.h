// macx_conv.hip.h -- general 2-D convolution (any kernel size k >= 1, any stride s >= 1, TF "SAME" padding) as an
// implicit GEMM on exact-fp32 MFMA: the generic stem's layers (ops.cnn, ops.py:380-411, for every --stemKernelSize(s) /
// --stemStrideSizes / --stemNumLayers the reference accepts; the fused 2-layer 3x3 stem keeps its own kernels).
//
// Layouts: activations NHWC [B][H][W][C], kernels HWIO [k][k][Cin][Cout] (the reference's variable layout, so a kernel is
// a row-major [k*k*Cin][Cout] matrix whose row index is (tap, channel)).  Cin and Cout are multiples of 4 (16-byte rows).
//
// SAME padding (TF's conv2d):  Ho = ceil(H / s),  pad_total = max((Ho - 1) s + k - H, 0),  pad_top = pad_total / 2 (an odd
// total puts the extra row at the bottom), and the same along W.  Input row of output row oy under tap ky:
// iy = oy s - pad_top + ky; taps outside [0, H) read zeros.
//
// Three roles share one tiling (a 128 x 128 output tile per workgroup of 4 waves, each wave 64 x 64 = 2 x 2 MFMA tiles of
// v_mfma_f32_32x32x2_f32, 16-deep reduction slices staged through LDS, the next slice's global loads in flight while the
// current one is multiplied):
//   FWD   y [B*Ho*Wo][Cout]  = gather(x) [B*Ho*Wo][k*k*Cin] . W [k*k*Cin][Cout]  (+ bias)
//   BWD   dx [B*H*W][Cin]    = gather(dy) [B*H*W][k*k*Cout] . W^T                 tap (ky, kx) reaches input pixel iy only
//                            where iy + pad_top - ky is a multiple of s and (iy + pad_top - ky) / s lies in [0, Ho)
//   WGRAD dw [k*k*Cin][Cout] = gather(x)^T . dy, contracted over the B*Ho*Wo output pixels in split-K slabs; the slabs are
//                            summed by a second kernel in slab order (no float atomics: two identical calls give the same bits)
// No im2col buffer: the gathered operand is read from the image on the fly (16 bytes = 4 channels per load), zero outside it.
#pragma once
#include "macx_common.hip.h"

namespace macx {

constexpr int CV_BM = 128, CV_BN = 128, CV_BK = 16, CV_LD = CV_BM + 4, CV_THREADS = 256;
constexpr int CV_SLAB_TARGET = 512;       // workgroups the weight gradient aims for before it splits the pixel axis
constexpr int CV_MAX_SPLIT = 16;

enum : int { CV_FWD = 0, CV_BWD = 1, CV_WGRAD = 2 };

struct ConvGeom {
  int B, H, W, Cin, Cout, k, s, Ho, Wo, pt, pl;
};

__host__ __device__ inline int conv_out_dim(int n, int s) { return (n + s - 1) / s; }
__host__ __device__ inline int conv_pad_before(int n, int k, int s) {
  const int tot = (conv_out_dim(n, s) - 1) * s + k - n;
  return tot > 0 ? tot / 2 : 0;
}

struct ConvArgs {
  ConvGeom g;
  const float* a;      // FWD, WGRAD: x;  BWD: dy
  const float* b;      // FWD, BWD: W;    WGRAD: dy
  const float* bias;   // FWD only (may be null)
  float* out;
  int M, N, K;         // GEMM: out [M][N] = sum over K
  int kspan;           // reduction range of one blockIdx.z (multiple of CV_BK)
  size_t slab;         // floats between consecutive split-K slabs of `out` (0: one slab)
};

// one 16-byte piece of the gathered A operand: 4 consecutive reduction indices kk..kk+3 of GEMM row m (FWD, BWD), or
// 4 consecutive rows r..r+3 at reduction index p (WGRAD); zeros outside the image / the problem
template <int ROLE>
__device__ __forceinline__ f32x4 conv_gather(const ConvArgs& p, int b, int oy, int ox, bool row_ok, int kk, int kend) {
  const ConvGeom& g = p.g;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (!row_ok || kk >= kend) return v;
  if (ROLE == CV_FWD) {
    const int tap = kk / g.Cin, c = kk - tap * g.Cin;
    const int ky = tap / g.k, kx = tap - ky * g.k;
    const int iy = oy * g.s - g.pt + ky, ix = ox * g.s - g.pl + kx;
    if (iy < 0 || iy >= g.H || ix < 0 || ix >= g.W) return v;
    return *reinterpret_cast<const f32x4*>(p.a + (((size_t)b * g.H + iy) * g.W + ix) * g.Cin + c);
  } else {   // CV_BWD: (b, oy, ox) hold the INPUT pixel (b, iy, ix)
    const int tap = kk / g.Cout, c = kk - tap * g.Cout;
    const int ky = tap / g.k, kx = tap - ky * g.k;
    const int ty = oy + g.pt - ky, tx = ox + g.pl - kx;
    if (ty < 0 || tx < 0 || ty % g.s || tx % g.s) return v;
    const int y = ty / g.s, x = tx / g.s;
    if (y >= g.Ho || x >= g.Wo) return v;
    return *reinterpret_cast<const f32x4*>(p.a + (((size_t)b * g.Ho + y) * g.Wo + x) * g.Cout + c);
  }
}

template <int ROLE>
__global__ void __launch_bounds__(CV_THREADS) conv_gemm_kernel(ConvArgs p) {
  __shared__ float As[CV_BK * CV_LD];   // [k][m]
  __shared__ float Bs[CV_BK * CV_LD];   // [k][n]
  const ConvGeom& g = p.g;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * CV_BM, n0 = blockIdx.y * CV_BN;
  const int kbeg = blockIdx.z * p.kspan;
  const int kend = min(p.K, kbeg + p.kspan);

  // ---- per-thread loader state, fixed over the K loop
  // A (FWD, BWD): pieces (row = tid/4 + 64 i, k quad = tid%4);  A (WGRAD): pieces (rows 4 (tid%32) .., k = tid/32 + 8 i)
  // B (FWD, WGRAD): pieces (k = tid/32 + 8 i, cols 4 (tid%32) ..);  B (BWD): pieces (col = tid%128, k quad = tid/128 + 2 i)
  int ab[2], ay[2], ax[2];
  bool aok[2];
  int wtap = 0, wc = 0, wky = 0, wkx = 0;
  bool wrow_ok = false;
  if (ROLE != CV_WGRAD) {
    const int HW = ROLE == CV_FWD ? g.Ho * g.Wo : g.H * g.W, WW = ROLE == CV_FWD ? g.Wo : g.W;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int m = m0 + (tid >> 2) + 64 * i;
      aok[i] = m < p.M;
      const int mm = aok[i] ? m : 0;
      ab[i] = mm / HW;
      const int r = mm - ab[i] * HW;
      ay[i] = r / WW;
      ax[i] = r - ay[i] * WW;
    }
  } else {
    const int r = m0 + 4 * (tid & 31);
    wrow_ok = r < p.M;
    wtap = r / g.Cin;
    wc = r - wtap * g.Cin;
    wky = wtap / g.k;
    wkx = wtap - wky * g.k;
  }

  f32x4 ra[2], rb[2];
  auto load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (ROLE != CV_WGRAD) {
        ra[i] = conv_gather<ROLE>(p, ab[i], ay[i], ax[i], aok[i], k0 + 4 * (tid & 3), kend);
      } else {
        const int pix = k0 + (tid >> 5) + 8 * i;      // output pixel (b, oy, ox)
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (wrow_ok && pix < kend) {
          const int HWo = g.Ho * g.Wo;
          const int b = pix / HWo, r = pix - b * HWo, oy = r / g.Wo, ox = r - oy * g.Wo;
          const int iy = oy * g.s - g.pt + wky, ix = ox * g.s - g.pl + wkx;
          if (iy >= 0 && iy < g.H && ix >= 0 && ix < g.W)
            v = *reinterpret_cast<const f32x4*>(p.a + (((size_t)b * g.H + iy) * g.W + ix) * g.Cin + wc);
        }
        ra[i] = v;
      }
      if (ROLE != CV_BWD) {
        const int kk = k0 + (tid >> 5) + 8 * i, n = n0 + 4 * (tid & 31);
        rb[i] = (kk < kend && n < p.N) ? *reinterpret_cast<const f32x4*>(p.b + (size_t)kk * p.N + n) : f32x4{0.f, 0.f, 0.f, 0.f};
      } else {   // W^T: row (tap, co) of the GEMM, column ci  ->  W[tap][ci][co], contiguous along co
        const int kk = k0 + 4 * ((tid >> 7) + 2 * i), n = n0 + (tid & 127);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (kk < kend && n < p.N) {
          const int tap = kk / g.Cout, co = kk - tap * g.Cout;
          v = *reinterpret_cast<const f32x4*>(p.b + ((size_t)tap * g.Cin + n) * g.Cout + co);
        }
        rb[i] = v;
      }
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (ROLE != CV_WGRAD) {
        const int row = (tid >> 2) + 64 * i, kq = 4 * (tid & 3);
#pragma unroll
        for (int e = 0; e < 4; ++e) As[(kq + e) * CV_LD + row] = ra[i][e];
      } else {
        *reinterpret_cast<f32x4*>(As + ((tid >> 5) + 8 * i) * CV_LD + 4 * (tid & 31)) = ra[i];
      }
      if (ROLE != CV_BWD) {
        *reinterpret_cast<f32x4*>(Bs + ((tid >> 5) + 8 * i) * CV_LD + 4 * (tid & 31)) = rb[i];
      } else {
        const int col = tid & 127, kq = 4 * ((tid >> 7) + 2 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) Bs[(kq + e) * CV_LD + col] = rb[i][e];
      }
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][c][r] = 0.f;

  const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
  const int li = lane & 31, lk = lane >> 5;
  if (kbeg < kend) load(kbeg);
  for (int k0 = kbeg; k0 < kend; k0 += CV_BK) {
    __syncthreads();           // the previous slice's MFMAs are done with As / Bs
    stage();
    __syncthreads();
    if (k0 + CV_BK < kend) load(k0 + CV_BK);     // next slice in flight under this slice's MFMAs
#pragma unroll
    for (int ks = 0; ks < CV_BK; ks += 2) {
      const float* a_row = As + (ks + lk) * CV_LD + wm + li;
      const float* b_row = Bs + (ks + lk) * CV_LD + wn + li;
      const float a0 = a_row[0], a1 = a_row[32], b0 = b_row[0], b1 = b_row[32];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
  }

  // ---- epilogue: C/D map of the 32x32 MFMA -- column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  float* out = p.out + (size_t)blockIdx.z * p.slab;
#pragma unroll
  for (int tn = 0; tn < 2; ++tn) {
    const int n = n0 + wn + 32 * tn + li;
    if (n >= p.N) continue;
    const float bn = (ROLE == CV_FWD && p.bias) ? p.bias[n] : 0.f;
#pragma unroll
    for (int tm = 0; tm < 2; ++tm) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm + 32 * tm + (r & 3) + 8 * (r >> 2) + 4 * lk;
        if (m < p.M) out[(size_t)m * p.N + n] = acc[tm][tn][r] + bn;
      }
    }
  }
}

// dw[i] = sum over slabs z = 0, 1, .. of ws[z][i], in that order
__global__ void __launch_bounds__(256) conv_slab_sum_kernel(const float* __restrict__ ws, size_t n, int slabs, float* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float s = ws[i];
  for (int z = 1; z < slabs; ++z) s += ws[(size_t)z * n + i];
  out[i] = s;
}

inline ConvGeom conv_geom(int B, int H, int W, int Cin, int Cout, int k, int s) {
  ConvGeom g;
  g.B = B; g.H = H; g.W = W; g.Cin = Cin; g.Cout = Cout; g.k = k; g.s = s;
  g.Ho = conv_out_dim(H, s);
  g.Wo = conv_out_dim(W, s);
  g.pt = conv_pad_before(H, k, s);
  g.pl = conv_pad_before(W, k, s);
  return g;
}

// split-K slabs of the weight gradient: a pure function of the shapes (never of the device), so the summation order -- and
// with it every bit of dw -- is the same on every run
inline void conv_wgrad_split(const ConvGeom& g, int* slabs, int* span) {
  const long long P = (long long)g.B * g.Ho * g.Wo;
  const long long tiles = (long long)((g.k * g.k * g.Cin + CV_BM - 1) / CV_BM) * ((g.Cout + CV_BN - 1) / CV_BN);
  long long z = (CV_SLAB_TARGET + tiles - 1) / tiles;
  const long long zmax = P / (8 * CV_BK);      // at least 8 slices per slab
  if (z > zmax) z = zmax;
  if (z > CV_MAX_SPLIT) z = CV_MAX_SPLIT;
  if (z < 1) z = 1;
  long long sp = (P + z - 1) / z;
  sp = (sp + CV_BK - 1) / CV_BK * CV_BK;
  *span = (int)sp;
  *slabs = (int)((P + sp - 1) / sp);
}

template <int ROLE>
inline hipError_t conv_launch(const ConvArgs& a, int zdim, hipStream_t st) {
  dim3 grid((a.M + CV_BM - 1) / CV_BM, (a.N + CV_BN - 1) / CV_BN, zdim);
  hipLaunchKernelGGL(conv_gemm_kernel<ROLE>, grid, dim3(CV_THREADS), 0, st, a);
  return hipGetLastError();
}

}  // namespace macx
