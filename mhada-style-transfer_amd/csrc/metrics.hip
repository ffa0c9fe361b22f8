// Image-quality metrics of eval.py on u8 frames already in device memory (the output of
// mhada_frame_emit / mhada_conv3x3_out3_u8): the SSIM of SSIMMetric (eval.py:167-223) and the
// histograms that kl_loss, nth_order_moment, uniformity and average_entropy (eval.py:38-67,
// 111-164) are finalised from on the host.  Frames are [B][H][W][3] u8 with rows of `row_bytes`
// (>= 3W, padded rows allowed), as in ingest.hip; no byte at or past 3W of a row is read.
//
// ---- SSIM -------------------------------------------------------------------------------------
// Definition (eval.py:180-223): per channel, the five window moments
//   E[x] E[y] E[x^2] E[y^2] E[xy] = sum over the 11 x 11 window of w[i][j] * (...),
// zero padding 5 (the padded zeros are window members), w = the fp32 outer product of the fp32
// Gaussian (sigma 1.5) the reference builds — passed in by the caller, who builds it with the
// reference's own fp32 operations — then
//   ssim = (2 E[x]E[y] + C1)(2 cov + C2) / ((E[x]^2 + E[y]^2 + C1)(var_x + var_y + C2)),
// C1 = 0.01^2, C2 = 0.03^2 ON [0, 255] VALUES, mean over H x W, then over the 3 channels.
//
// Why fp64, and why the window is not separated: with constants that small the variance terms
// decide the value wherever the image is smooth, and there E[x^2] - E[x]^2 cancels to ~1e-8 of its
// operands (it is v^2 * S(1 - S) for a flat value v, S = sum(w) = 1 - 6.8e-8).  In fp32 that is
// rounding noise several times C2 (the reference's own result is off by ~1 on a flat-vs-step pair);
// and the value depends on the weights to better than 1e-9, so the weights have to be the
// reference's 121 fp32-ROUNDED products: a horizontal-then-vertical pass would use the unrounded
// products g[i] * g[j], whose sum differs by ~1e-8, which moves the flat-vs-step SSIM by 2e-3.
// So: the 121-tap sum, weights widened exactly to fp64, u8 values and their products exact in fp64,
// every moment an fp64 FMA chain in a fixed order (j outer, i inner).  The xy chain is the x^2
// chain when y == x, and the map value is formed without contraction, so ssim(x, x) == 1 exactly
// and ssim(a, b) == ssim(b, a) bit for bit.
//
// Layout: grid (W/32, H/32, 3B); a workgroup computes a 32 x 32 tile of one channel.  The 42 x 42
// input patch of both images goes to LDS as fp64 (28 KB); thread (tx, strip) owns the 4 output
// rows 4 strip .. 4 strip + 3 of column tx, so each patch value it loads (and its three products)
// feeds up to 4 outputs.  The tile's map values are summed in a fixed order (thread, wave shuffle,
// 4 waves) into one fp64 partial; ssim_finalize sums an image's partials in a fixed order, divides
// by 3HW and rounds to fp32 once.  No atomics: repeated calls return the same bits.
//
// ---- histograms -------------------------------------------------------------------------------
// hist [B][4][256] uint32: planes 0..2 = np.bincount of the three stored channels, plane 3 = of
// the gray image cv2.cvtColor(BGR2GRAY) as OpenCV 4 computes it for u8,
//   (R * 9798 + G * 19235 + B * 3735 + (1 << 14)) >> 15,
// `bgr` telling which stored byte is R.  cv2 itself is not installed here, so bit parity with cv2
// is PARITY UNPINNED: the tests hold the kernel to this integer formula.
// Per-workgroup LDS bins (4 x 256 full 32-bit counters, integer LDS atomics), flushed with integer
// global atomics into the output the entry point has zeroed: integer addition is order-independent,
// so the counts are exact and the same from run to run.
#include <algorithm>

#include "common.h"

namespace mhada {

constexpr int kSsimWin = 11, kSsimPad = 5, kSsimTile = 32;
constexpr int kSsimPatch = kSsimTile + 2 * kSsimPad;  // 42
constexpr int kSsimRows = 4;                          // output rows per thread
constexpr int kSsimIn = kSsimRows + kSsimWin - 1;     // 14 patch rows per thread

struct SsimWindow {
  float w[kSsimWin * kSsimWin];
};

MHADA_DEV double ssim_value(double m1, double m2, double exx, double eyy, double exy) {
#pragma clang fp contract(off)
  const double c1 = 0.01 * 0.01, c2 = 0.03 * 0.03;
  const double p11 = m1 * m1, p22 = m2 * m2, p12 = m1 * m2;
  const double s1 = exx - p11, s2 = eyy - p22, s12 = exy - p12;
  const double num = (2.0 * p12 + c1) * (2.0 * s12 + c2);
  const double den = ((p11 + p22) + c1) * ((s1 + s2) + c2);
  return num / den;
}

__global__ void __launch_bounds__(256) ssim_tile_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                         double* __restrict__ part, int H, int W, long long rba,
                                                         long long rbb, const SsimWindow win) {
  __shared__ double sx[kSsimPatch * kSsimPatch], sy[kSsimPatch * kSsimPatch];
  __shared__ double sw[kSsimWin * kSsimWin];
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const int img = blockIdx.z / 3, ch = blockIdx.z - 3 * img;
  const int x0 = blockIdx.x * kSsimTile, y0 = blockIdx.y * kSsimTile;
  const uint8_t* fa = a + (long long)img * H * rba;
  const uint8_t* fb = b + (long long)img * H * rbb;
  for (int i = tid; i < kSsimWin * kSsimWin; i += 256) sw[i] = (double)win.w[i];
  for (int i = tid; i < kSsimPatch * kSsimPatch; i += 256) {
    const int r = i / kSsimPatch, c = i - r * kSsimPatch;
    const int gy = y0 + r - kSsimPad, gx = x0 + c - kSsimPad;
    double vx = 0.0, vy = 0.0;  // the zero padding, and nothing else, outside the image
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
      vx = (double)fa[(long long)gy * rba + 3LL * gx + ch];
      vy = (double)fb[(long long)gy * rbb + 3LL * gx + ch];
    }
    sx[i] = vx;
    sy[i] = vy;
  }
  __syncthreads();

  const int tx = tid & 31, strip = tid >> 5;
  double acc[kSsimRows][5];
#pragma unroll
  for (int o = 0; o < kSsimRows; ++o)
#pragma unroll
    for (int m = 0; m < 5; ++m) acc[o][m] = 0.0;
  const double* px = sx + (kSsimRows * strip) * kSsimPatch + tx;
  const double* py = sy + (kSsimRows * strip) * kSsimPatch + tx;
  for (int j = 0; j < kSsimWin; ++j) {
    double wj[kSsimWin];
#pragma unroll
    for (int i = 0; i < kSsimWin; ++i) wj[i] = sw[i * kSsimWin + j];
#pragma unroll
    for (int q = 0; q < kSsimIn; ++q) {
      const double x = px[q * kSsimPatch + j], y = py[q * kSsimPatch + j];
      const double xx = x * x, yy = y * y, xy = x * y;  // exact: integers below 2^16
#pragma unroll
      for (int o = 0; o < kSsimRows; ++o) {
        const int i = q - o;  // window row of patch row q for output row o
        if (i >= 0 && i < kSsimWin) {
          acc[o][0] = fma(wj[i], x, acc[o][0]);
          acc[o][1] = fma(wj[i], y, acc[o][1]);
          acc[o][2] = fma(wj[i], xx, acc[o][2]);
          acc[o][3] = fma(wj[i], yy, acc[o][3]);
          acc[o][4] = fma(wj[i], xy, acc[o][4]);
        }
      }
    }
  }
  double s = 0.0;
#pragma unroll
  for (int o = 0; o < kSsimRows; ++o) {
    const int gy = y0 + kSsimRows * strip + o, gx = x0 + tx;
    if (gy < H && gx < W) s += ssim_value(acc[o][0], acc[o][1], acc[o][2], acc[o][3], acc[o][4]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  if (tid == 0)
    part[((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] =
        ((red[0] + red[1]) + red[2]) + red[3];
}

// out[b] = (float)(sum of image b's nparts partials / n), the partials summed in a fixed order
__global__ void __launch_bounds__(256) ssim_finalize(const double* __restrict__ part, float* __restrict__ out,
                                                      int nparts, double n) {
  __shared__ double red[4];
  const int b = blockIdx.x;
  double acc = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) acc += part[(long long)b * nparts + i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) out[b] = (float)((((red[0] + red[1]) + red[2]) + red[3]) / n);
}

constexpr int kHistPix = 4096;  // pixels per workgroup pass: 16 per thread

__global__ void __launch_bounds__(256) hist_u8_kernel(const uint8_t* __restrict__ in, uint32_t* __restrict__ hist, int H,
                                                       int W, long long row_bytes, int bgr) {
  __shared__ uint32_t bins[4 * 256];
  for (int i = threadIdx.x; i < 4 * 256; i += 256) bins[i] = 0u;
  __syncthreads();
  const int b = blockIdx.y;
  const uint8_t* frame = in + (long long)b * H * row_bytes;
  const long long HW = (long long)H * W;
  for (long long base = (long long)blockIdx.x * kHistPix; base < HW; base += (long long)gridDim.x * kHistPix) {
    const long long end = min(base + kHistPix, HW);
    for (long long pix = base + threadIdx.x; pix < end; pix += 256) {
      const int y = (int)(pix / W), x = (int)(pix - (long long)y * W);
      const uint8_t* p = frame + (long long)y * row_bytes + 3LL * x;
      const uint32_t c0 = p[0], c1 = p[1], c2 = p[2];
      const uint32_t r = bgr ? c2 : c0, bl = bgr ? c0 : c2;
      const uint32_t gray = (r * 9798u + c1 * 19235u + bl * 3735u + (1u << 14)) >> 15;  // <= 255
      atomicAdd(&bins[c0], 1u);
      atomicAdd(&bins[256 + c1], 1u);
      atomicAdd(&bins[512 + c2], 1u);
      atomicAdd(&bins[768 + gray], 1u);
    }
  }
  __syncthreads();
  uint32_t* out = hist + (long long)b * 4 * 256;
  for (int i = threadIdx.x; i < 4 * 256; i += 256)
    if (bins[i]) atomicAdd(out + i, bins[i]);
}

static long long ssim_tiles(int H, int W) {
  return 3LL * ((H + kSsimTile - 1) / kSsimTile) * ((W + kSsimTile - 1) / kSsimTile);
}

}  // namespace mhada

using namespace mhada;

extern "C" long long mhada_ssim_u8_work(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return (long long)B * ssim_tiles(H, W);
}

extern "C" int mhada_ssim_u8(const void* a, long long row_bytes_a, const void* b, long long row_bytes_b, int B, int H,
                             int W, const float* window, double* work, long long work_doubles, float* out,
                             mhada_stream_t s_) {
  if (!a || !b || !window || !work || !out || B <= 0 || H <= 0 || W <= 0) return fail("mhada_ssim_u8: bad args");
  if (row_bytes_a < 3LL * W || row_bytes_b < 3LL * W) return fail("mhada_ssim_u8: row_bytes < 3*W");
  const int tx = (W + kSsimTile - 1) / kSsimTile, ty = (H + kSsimTile - 1) / kSsimTile;
  if (ty > 65535 || 3LL * B > 65535) return fail("mhada_ssim_u8: too many tile rows or frames");
  if (B * ssim_tiles(H, W) >= (1LL << 31)) return fail("mhada_ssim_u8: too many tiles");
  if (work_doubles < mhada_ssim_u8_work(B, H, W)) return fail("mhada_ssim_u8: workspace too small (mhada_ssim_u8_work)");
  SsimWindow win;
  for (int i = 0; i < kSsimWin * kSsimWin; ++i) win.w[i] = window[i];
  const hipStream_t s = (hipStream_t)s_;
  hipLaunchKernelGGL(ssim_tile_kernel, dim3(tx, ty, 3 * B), dim3(256), 0, s, (const uint8_t*)a, (const uint8_t*)b, work,
                     H, W, row_bytes_a, row_bytes_b, win);
  if (int rc = check_launch("mhada_ssim_u8/tiles")) return rc;
  hipLaunchKernelGGL(ssim_finalize, dim3(B), dim3(256), 0, s, (const double*)work, out, (int)ssim_tiles(H, W),
                     3.0 * (double)H * (double)W);
  return check_launch("mhada_ssim_u8/finalize");
}

extern "C" int mhada_hist_u8(const void* frames, int B, int H, int W, long long row_bytes, int bgr, unsigned int* hist,
                             mhada_stream_t s_) {
  if (!frames || !hist || B <= 0 || H <= 0 || W <= 0) return fail("mhada_hist_u8: bad args");
  if (row_bytes < 3LL * W) return fail("mhada_hist_u8: row_bytes < 3*W");
  if (B > 65535) return fail("mhada_hist_u8: too many frames");
  const long long HW = (long long)H * W;
  if (HW > 0xFFFFFFFFLL) return fail("mhada_hist_u8: more pixels than a 32-bit counter holds");
  const hipStream_t s = (hipStream_t)s_;
  if (hipMemsetAsync(hist, 0, (size_t)B * 4 * 256 * sizeof(uint32_t), s) != hipSuccess)
    return check_launch("mhada_hist_u8/zero");
  const unsigned nblk = (unsigned)std::min<long long>((HW + kHistPix - 1) / kHistPix, 2048);
  hipLaunchKernelGGL(hist_u8_kernel, dim3(nblk, B), dim3(256), 0, s, (const uint8_t*)frames, hist, H, W, row_bytes,
                     bgr != 0);
  return check_launch("mhada_hist_u8");
}
