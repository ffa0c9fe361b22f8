// The convolutions and pools of the InceptionV3 trunk of SIFID (SIFID/inception.py:60-103, torchvision's
// BasicConv2d = Conv2d(bias=False) -> BatchNorm2d(eps=0.001) in eval mode -> ReLU), fp32 NHWC.
//
// mhada_conv2d: implicit GEMM on the fp32 MFMA (v_mfma_f32_32x32x2_f32, exact fp32 products, fp32 FMA
// chain), y[m][n] = act(scale[n] * sum_k A[m][k] W[n][k] + shift[n]) with m = (b, oh, ow), n the output
// channel and k = (kh, kw, c): x is [B][H][W][Cin], w is [Cout][KH][KW][Cin] (the OIHW filter
// permuted once on the host), so both operands are contiguous along c inside one tap.
//
// K walk.  One step is 16 channels of ONE tap: a step never reaches across a tap boundary, so the
// gather of a step is one 64-byte run per row whatever the geometry, and the zero padding is a
// per-row predicate.  Cin % 4 == 0, so a float4 is wholly inside or wholly past Cin; the channels
// past Cin of the last step of a tap (Cin = 48, 80, 160, 288, 448 ...) are staged as zeros in BOTH
// operands and add exactly 0.0.  Inside a step MFMA j takes the channel pair (j, j + 8), so a lane's
// eight A (and W) values of a step are two ds_read_b128 of one staged row (row stride 20 floats).
//
// Tiles.  A wave owns 32 rows x 64 columns (two 32 x 32 accumulators); a workgroup is WM waves stacked
// along M over one staged 64-column W tile:
//   WM = 4, 128 x 64, 256 threads  the stem and block 1 / 2 at useful image sizes (M in the thousands):
//                                  each staged W row serves four waves;
//   WM = 1,  32 x 64,  64 threads  the deep end (M = 196 rows at 512^2 in block 3, 900 in block 2),
//                                  where 128-row tiles would leave most CUs idle and most of a tile's
//                                  rows past M.
// The form is chosen by the number of 128 x 64 tiles against the CU count.  Both walk K in the same
// order with the same per-element FMA chain, so an output's bits do not depend on the form.
// The global loads of step i + 1 are issued before the MFMAs of step i (register staging).
//
// Output: y[m * ldc + c_off + n], so each branch of a Mixed block writes its slice of the block's
// concat buffer; there is no concat kernel.
#include "common.h"

namespace mhada {

constexpr int kCvBK = 16;          // channels per K step
constexpr int kCvRow = kCvBK + 4;  // floats per staged row (16-byte aligned, rows 80 B apart)

struct Conv2dP {
  const float *x, *w, *scale, *shift;
  float* y;
  int H, W, Cin, Cout, KH, KW, stride, ph, pw, Ho, Wo;
  long long M, ldc;
  int c_off, relu, ntn;
};

template <int WM>
__global__ void __launch_bounds__(64 * WM) conv2d_kernel(const Conv2dP p) {
  constexpr int BM = 32 * WM, NT = 64 * WM, WL = 256 / NT;
  __shared__ __attribute__((aligned(16))) float As[BM * kCvRow];
  __shared__ __attribute__((aligned(16))) float Ws[64 * kCvRow];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int tn = blockIdx.x % p.ntn;
  const long long m0 = (long long)(blockIdx.x / p.ntn) * BM;
  const int n0 = tn * 64;

  // the two A rows this thread gathers (float4 q of row idx >> 2), fixed for the whole K walk
  const float* abase[2];
  int ih0[2], iw0[2];
  bool aval[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const long long m = m0 + ((t + i * NT) >> 2);
    aval[i] = m < p.M;
    const long long mm = aval[i] ? m : 0;
    const int ow = (int)(mm % p.Wo);
    const long long r = mm / p.Wo;
    const int oh = (int)(r % p.Ho);
    abase[i] = p.x + (r / p.Ho) * ((long long)p.H * p.W * p.Cin);
    ih0[i] = oh * p.stride - p.ph;
    iw0[i] = ow * p.stride - p.pw;
  }
  const int q4 = 4 * (t & 3);  // NT % 4 == 0: the same float4 column for every i
  const int nc = (p.Cin + kCvBK - 1) / kCvBK, taps = p.KH * p.KW, nsteps = taps * nc;

  f32x4 ra[2], rw[WL];
  auto gather = [&](int step) {
    const int tap = step / nc, c = (step - tap * nc) * kCvBK + q4;
    const int kh = tap / p.KW, kw = tap - kh * p.KW;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int ih = ih0[i] + kh, iw = iw0[i] + kw;
      const bool ok = aval[i] && c < p.Cin && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
      ra[i] = ok ? ld4(abase[i] + ((long long)ih * p.W + iw) * p.Cin + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int i = 0; i < WL; ++i) {
      const int n = n0 + ((t + i * NT) >> 2);
      const bool ok = n < p.Cout && c < p.Cin;
      rw[i] = ok ? ld4(p.w + ((long long)n * taps + tap) * p.Cin + c) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };

  f32x16 acc[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  const int r32 = lane & 31, h = lane >> 5;
  gather(0);
  for (int step = 0; step < nsteps; ++step) {
#pragma unroll
    for (int i = 0; i < 2; ++i) st4(&As[((t + i * NT) >> 2) * kCvRow + q4], ra[i]);
#pragma unroll
    for (int i = 0; i < WL; ++i) st4(&Ws[((t + i * NT) >> 2) * kCvRow + q4], rw[i]);
    __syncthreads();
    if (step + 1 < nsteps) gather(step + 1);
    const float* ap = &As[(32 * wv + r32) * kCvRow + 8 * h];
    const f32x4 a0 = ld4(ap), a1 = ld4(ap + 4);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const float* wp = &Ws[(32 * j + r32) * kCvRow + 8 * h];
      const f32x4 b0 = ld4(wp), b1 = ld4(wp + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[e], b0[e], acc[j], 0, 0, 0);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[e], b1[e], acc[j], 0, 0, 0);
    }
    __syncthreads();
  }

  // conv, then the affine, then ReLU: the reference's order, the scale is not folded into the weights
#pragma unroll
  for (int j = 0; j < 2; ++j) {
#pragma clang fp contract(off)
    const int n = n0 + 32 * j + r32;
    if (n >= p.Cout) continue;
    const float sc = p.scale[n], sh = p.shift[n];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long long m = m0 + 32 * wv + acc_row(r, h);
      if (m >= p.M) continue;
      float v = acc[j][r] * sc + sh;
      if (p.relu && v < 0.f) v = 0.f;  // a NaN stays a NaN, as aten's relu
      p.y[m * p.ldc + p.c_off + n] = v;
    }
  }
}

// ---- pools (fp32 NHWC, C % 4 == 0, one thread per float4 of the output) ------------------------------
// max_pool2d(3, 2): no padding, floor (inception.py:75,84 and Mixed_6a / Mixed_7a's pool branch)
__global__ void __launch_bounds__(256) maxpool3s2_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W,
                                                          int C, int Ho, int Wo, long long ldc, int c_off,
                                                          long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c4 = C / 4, c = (int)(i % c4) * 4;
  const long long px = i / c4;
  const int ow = (int)(px % Wo);
  const long long r = px / Wo;
  const int oh = (int)(r % Ho);
  const float* src = x + (((r / Ho) * H + 2 * oh) * W + 2 * ow) * C + c;
  f32x4 m = ld4(src);
#pragma unroll
  for (int kh = 0; kh < 3; ++kh)
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const f32x4 v = ld4(src + ((long long)kh * W + kw) * C);
#pragma unroll
      for (int e = 0; e < 4; ++e) m[e] = (v[e] > m[e] || v[e] != v[e]) ? v[e] : m[e];  // NaN propagates, as aten's
    }
  st4(y + px * ldc + c_off + c, m);
}

// avg_pool2d(3, 1, 1), count_include_pad=True: the in-range taps added in row-major order, then / 9
__global__ void __launch_bounds__(256) avgpool3_kernel(const float* __restrict__ x, float* __restrict__ y, int H, int W,
                                                        int C, long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c4 = C / 4, c = (int)(i % c4) * 4;
  const long long px = i / c4;
  const int ow = (int)(px % W);
  const long long r = px / W;
  const int oh = (int)(r % H);
  const float* img = x + (r / H) * ((long long)H * W * C) + c;
  f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kh = -1; kh <= 1; ++kh)
#pragma unroll
    for (int kw = -1; kw <= 1; ++kw) {
      const int ih = oh + kh, iw = ow + kw;
      if ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W) s += ld4(img + ((long long)ih * W + iw) * C);
    }
  st4(y + px * C + c, s / 9.0f);
}

// NCHW fp32 [B][3][H][W] -> NHWC with the channels padded to 4 (the fourth is 0), optionally 2 x - 1
// (inception.py:137-138; 2 x is exact, so the result is torch's `2 * x - 1` bit for bit)
__global__ void __launch_bounds__(256) inception_input_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                               long long HW, long long total, int normalize) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long long b = i / HW, px = i - b * HW;
  const float* src = x + b * 3 * HW + px;
  f32x4 v = f32x4{src[0], src[HW], src[2 * HW], 0.f};
  if (normalize) {
#pragma unroll
    for (int e = 0; e < 3; ++e) v[e] = 2.0f * v[e] - 1.0f;
  }
  st4(y + 4 * i, v);
}

// ---- the stem: a direct 3-channel conv evaluated in fp64 ------------------------------------------------
// The reference feeds the trunk 2 (v / 255 / 255) - 1, within 0.008 of the constant -1 ("SIFID"):
// the first conv's output is -sum(w) plus 0.4 % of image content, and its BatchNorm subtracts the constant
// again.  An fp32 FMA chain (aten's as much as the MFMA's) leaves rounding noise of 2^-24 of the CONSTANT on
// the content, about 5e-5 of every feature that follows and far more of d^2, which is itself a difference.
// With 27 terms per output the layer costs nothing, so it is evaluated exactly where that is free: 2 x - 1,
// the products of the fp32 operands, their sum and the affine all in fp64 (scale and shift arrive as fp64,
// folded from the fp32 BatchNorm tensors), one rounding to fp32 at the store.  x is the caller's NCHW image
// [B][3][H][W] (no padded copy), w the packed filter [Cout][KH][KW][4] whose fourth channel is not read.
// One thread per output element, channel fastest: 32 consecutive lanes share a pixel's 27 inputs.
struct StemP {
  const float *x, *w;
  const double *scale, *shift;
  float* y;
  int H, W, Cout, KH, KW, stride, ph, pw, Ho, Wo;
  long long total, ldc;
  int c_off, relu, normalize;
};

__global__ void __launch_bounds__(256) conv2d_stem_kernel(const StemP p) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= p.total) return;
  const int n = (int)(i % p.Cout);
  const long long m = i / p.Cout;
  const int ow = (int)(m % p.Wo);
  const long long r = m / p.Wo;
  const int oh = (int)(r % p.Ho);
  const long long HW = (long long)p.H * p.W;
  const float* img = p.x + (r / p.Ho) * 3 * HW;
  const float* wn = p.w + (long long)n * p.KH * p.KW * 4;
  double acc = 0.0;
  for (int kh = 0; kh < p.KH; ++kh) {
    const int ih = oh * p.stride - p.ph + kh;
    if ((unsigned)ih >= (unsigned)p.H) continue;
    for (int kw = 0; kw < p.KW; ++kw) {
      const int iw = ow * p.stride - p.pw + kw;
      if ((unsigned)iw >= (unsigned)p.W) continue;
      const float* px = img + (long long)ih * p.W + iw;
      const float* wt = wn + (kh * p.KW + kw) * 4;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        double v = (double)px[c * HW];
        if (p.normalize) v = 2.0 * v - 1.0;  // exact in fp64 for every fp32 v in [0, 1]
        acc = fma((double)wt[c], v, acc);
      }
    }
  }
  double v = fma(acc, p.scale[n], p.shift[n]);
  if (p.relu && v < 0.0) v = 0.0;
  p.y[m * p.ldc + p.c_off + n] = (float)v;
}

static bool conv2d_geometry_ok(int KH, int KW) {
  const int g[7][2] = {{1, 1}, {3, 3}, {5, 5}, {1, 7}, {7, 1}, {1, 3}, {3, 1}};
  for (auto& k : g)
    if (k[0] == KH && k[1] == KW) return true;
  return false;
}

}  // namespace mhada

using namespace mhada;

extern "C" int mhada_conv2d(const float* x, const float* w, const float* scale, const float* shift, float* y, int B,
                            int H, int W, int Cin, int Cout, int KH, int KW, int stride, int ph, int pw,
                            long long ldc, int c_off, int relu, mhada_stream_t s_) {
  if (!x || !w || !scale || !shift || !y) return fail("mhada_conv2d: null pointer");
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return fail("mhada_conv2d: sizes must be positive");
  if (!conv2d_geometry_ok(KH, KW)) return fail("mhada_conv2d: kernel must be 1x1, 3x3, 5x5, 1x7, 7x1, 1x3 or 3x1");
  if (stride != 1 && stride != 2) return fail("mhada_conv2d: stride must be 1 or 2");
  if (ph < 0 || pw < 0 || ph >= KH || pw >= KW) return fail("mhada_conv2d: padding must be in [0, kernel) per axis");
  if (Cin % 4) return fail("mhada_conv2d: Cin must be a multiple of 4 (pad a 3-channel image with mhada_inception_input)");
  if (H + 2 * ph < KH || W + 2 * pw < KW) return fail("mhada_conv2d: the padded input is smaller than the kernel");
  if (c_off < 0 || ldc < (long long)c_off + Cout) return fail("mhada_conv2d: ldc must be >= c_off + Cout, c_off >= 0");
  if (relu != 0 && relu != 1) return fail("mhada_conv2d: relu must be 0 or 1");
  if (!aligned16(x) || !aligned16(w)) return fail("mhada_conv2d: x and w must be 16-byte aligned");
  const int Ho = (H + 2 * ph - KH) / stride + 1, Wo = (W + 2 * pw - KW) / stride + 1;
  const long long M = (long long)B * Ho * Wo;
  if (M >= (1LL << 31) || (long long)B * H * W >= (1LL << 31)) return fail("mhada_conv2d: 2^31 pixels or more");
  const int ntn = (Cout + 63) / 64;
  const long long big = ((M + 127) / 128) * ntn, small = ((M + 31) / 32) * ntn;
  if (small >= (1LL << 31)) return fail("mhada_conv2d: too many tiles");
  Conv2dP p{x, w, scale, shift, y, H, W, Cin, Cout, KH, KW, stride, ph, pw, Ho, Wo, M, ldc, c_off, relu, ntn};
  const hipStream_t s = (hipStream_t)s_;
  if (big >= num_cus())
    hipLaunchKernelGGL(conv2d_kernel<4>, dim3((unsigned)big), dim3(256), 0, s, p);
  else
    hipLaunchKernelGGL(conv2d_kernel<1>, dim3((unsigned)small), dim3(64), 0, s, p);
  return check_launch("mhada_conv2d");
}

extern "C" int mhada_conv2d_stem(const float* x, const float* w, const double* scale, const double* shift, float* y,
                                 int B, int H, int W, int Cout, int KH, int KW, int stride, int ph, int pw,
                                 long long ldc, int c_off, int relu, int normalize, mhada_stream_t s_) {
  if (!x || !w || !scale || !shift || !y) return fail("mhada_conv2d_stem: null pointer");
  if (B <= 0 || H <= 0 || W <= 0 || Cout <= 0) return fail("mhada_conv2d_stem: sizes must be positive");
  if (!conv2d_geometry_ok(KH, KW)) return fail("mhada_conv2d_stem: kernel must be 1x1, 3x3, 5x5, 1x7, 7x1, 1x3 or 3x1");
  if (stride != 1 && stride != 2) return fail("mhada_conv2d_stem: stride must be 1 or 2");
  if (ph < 0 || pw < 0 || ph >= KH || pw >= KW) return fail("mhada_conv2d_stem: padding must be in [0, kernel) per axis");
  if (H + 2 * ph < KH || W + 2 * pw < KW) return fail("mhada_conv2d_stem: the padded input is smaller than the kernel");
  if (c_off < 0 || ldc < (long long)c_off + Cout) return fail("mhada_conv2d_stem: ldc must be >= c_off + Cout, c_off >= 0");
  if ((relu != 0 && relu != 1) || (normalize != 0 && normalize != 1)) return fail("mhada_conv2d_stem: relu and normalize must be 0 or 1");
  if (((uintptr_t)scale | (uintptr_t)shift) & 7) return fail("mhada_conv2d_stem: scale and shift must be 8-byte aligned");
  const int Ho = (H + 2 * ph - KH) / stride + 1, Wo = (W + 2 * pw - KW) / stride + 1;
  const long long M = (long long)B * Ho * Wo, total = M * Cout;
  if (M >= (1LL << 31) || (long long)B * H * W >= (1LL << 31) || (total + 255) / 256 >= (1LL << 31))
    return fail("mhada_conv2d_stem: 2^31 pixels or more, or too many outputs");
  StemP p{x, w, scale, shift, y, H, W, Cout, KH, KW, stride, ph, pw, Ho, Wo, total, ldc, c_off, relu, normalize};
  hipLaunchKernelGGL(conv2d_stem_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)s_, p);
  return check_launch("mhada_conv2d_stem");
}

static int pool_args(const char* what, const float* x, float* y, int B, int H, int W, int C) {
  if (!x || !y) return fail(std::string(what) + ": null pointer");
  if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4) return fail(std::string(what) + ": sizes must be positive, C % 4 == 0");
  if (!aligned16(x) || !aligned16(y)) return fail(std::string(what) + ": pointers must be 16-byte aligned");
  if ((long long)B * H * W >= (1LL << 31)) return fail(std::string(what) + ": 2^31 pixels or more");
  return MHADA_OK;
}

extern "C" int mhada_maxpool3s2(const float* x, float* y, int B, int H, int W, int C, long long ldc, int c_off,
                                mhada_stream_t s_) {
  if (int rc = pool_args("mhada_maxpool3s2", x, y, B, H, W, C)) return rc;
  if (H < 3 || W < 3) return fail("mhada_maxpool3s2: the image is smaller than the 3x3 window");
  if (c_off < 0 || c_off % 4 || ldc % 4 || ldc < (long long)c_off + C)
    return fail("mhada_maxpool3s2: ldc >= c_off + C, both multiples of 4");
  const int Ho = (H - 3) / 2 + 1, Wo = (W - 3) / 2 + 1;
  const long long total = (long long)B * Ho * Wo * (C / 4);
  if ((total + 255) / 256 >= (1LL << 31)) return fail("mhada_maxpool3s2: too many elements");
  hipLaunchKernelGGL(maxpool3s2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)s_, x, y, H, W, C,
                     Ho, Wo, ldc, c_off, total);
  return check_launch("mhada_maxpool3s2");
}

extern "C" int mhada_avgpool3(const float* x, float* y, int B, int H, int W, int C, mhada_stream_t s_) {
  if (int rc = pool_args("mhada_avgpool3", x, y, B, H, W, C)) return rc;
  const long long total = (long long)B * H * W * (C / 4);
  if ((total + 255) / 256 >= (1LL << 31)) return fail("mhada_avgpool3: too many elements");
  hipLaunchKernelGGL(avgpool3_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)s_, x, y, H, W, C,
                     total);
  return check_launch("mhada_avgpool3");
}

extern "C" int mhada_inception_input(const float* x, float* y, int B, int H, int W, int normalize, mhada_stream_t s_) {
  if (!x || !y) return fail("mhada_inception_input: null pointer");
  if (B <= 0 || H <= 0 || W <= 0) return fail("mhada_inception_input: sizes must be positive");
  if (!aligned16(y)) return fail("mhada_inception_input: y must be 16-byte aligned");
  const long long total = (long long)B * H * W;
  if (total >= (1LL << 31)) return fail("mhada_inception_input: 2^31 pixels or more");
  hipLaunchKernelGGL(inception_input_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)s_, x, y,
                     (long long)H * W, total, normalize != 0);
  return check_launch("mhada_inception_input");
}
