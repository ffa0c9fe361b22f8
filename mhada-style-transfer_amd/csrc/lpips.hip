// The distance head of LPIPS (lpips/__init__.py:13-15, lpips/lpips.py:139-147) on two fp32 feature
// maps held NHWC, [B][P][C] with P = H * W: per image
//   na = sqrt(sum_c a_c^2),  a^_c = a_c / (na + 1e-10)   (and the same for b)
//   v_p = sum_c w_c (a^_c - b^_c)^2,                      out = (sum_p v_p) / P.
// As aten ops this is about ten elementwise and reduction kernels per layer, each reading or writing
// whole feature maps; here each map is read once and only per-workgroup scalars are written.
//
// Arithmetic.  Per pixel fp32, as the reference's: the two norms are fma chains over a lane's
// channels followed by a shuffle tree, 1 / (na + 1e-10f) is one correctly rounded division per
// pixel, a^_c = a_c * that (one rounding more than the reference's a_c / (na + eps), inside the
// bound of tests/lpips_ref.py), the difference a^_c - b^_c is formed DIRECTLY and without
// contraction (an fma(a, ra, -b * rb) would leave the rounding error of b * rb behind when the two
// maps are bit-identical): a == b gives exactly 0, an all-zero vector gives a^ = 0 * 1e10 = 0 with no
// special case, and (a, b) -> (b, a) changes no bit.  The sum over the pixels is fp64: each group's
// v_p is widened and added to an fp64 register, the registers of a wave's groups, the 4 waves of
// a workgroup and, in lpips_finalize, an image's workgroup partials are added in a fixed order.
// No atomics: repeated calls return the same bits.
//
// Layout.  A pixel's C floats are contiguous, C / 4 float4s.  G lanes share one pixel, G the largest
// power of two <= 64 dividing C / 4, each lane holding N = C / (4 G) float4s of each map (and of w,
// loaded once): C = 64 -> (G 16, N 1), 128 -> (32, 1), 192 -> (16, 3), 256 -> (64, 1), 320 -> (16, 5),
// 384 -> (32, 3), 448 -> (16, 7), 512 -> (64, 2).  So every load is a full-width dwordx4 and a wave
// load instruction covers 1 KB of 64 / G consecutive pixels, whatever C.  Groups whose pixel is past
// P load nothing (their vectors are zero and contribute exactly 0.0).  grid (nblk, B): workgroup k of
// an image walks pixels (4 k + wave) * 64 / G + group, stepping by nblk * 256 / G.
#include <algorithm>

#include "common.h"

namespace mhada {

constexpr int kLpipsMaxBlocks = 2048;  // per image
constexpr int kLpipsPasses = 4;        // pixel passes per wave before another workgroup is worth its launch

MHADA_DEV float dot4(f32x4 x, f32x4 y, float acc) {
  acc = fmaf(x[0], y[0], acc);
  acc = fmaf(x[1], y[1], acc);
  acc = fmaf(x[2], y[2], acc);
  return fmaf(x[3], y[3], acc);
}

template <int G> MHADA_DEV float group_sum(float v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// v_p of the pixel shared by this lane's group (the same value in its G lanes)
template <int G, int N> MHADA_DEV float lpips_pixel(const f32x4 (&a)[N], const f32x4 (&b)[N], const f32x4 (&w)[N]) {
#pragma clang fp contract(off)
  float sa = 0.f, sb = 0.f;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    sa = dot4(a[j], a[j], sa);
    sb = dot4(b[j], b[j], sb);
  }
  const float ra = 1.0f / (sqrtf(group_sum<G>(sa)) + 1e-10f);
  const float rb = 1.0f / (sqrtf(group_sum<G>(sb)) + 1e-10f);
  float v = 0.f;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const f32x4 ta = a[j] * ra, tb = b[j] * rb;
    const f32x4 d = ta - tb;
    v = dot4(w[j], d * d, v);
  }
  return group_sum<G>(v);
}

template <int G, int N>
__global__ void __launch_bounds__(256) lpips_layer_kernel(const float* __restrict__ fa, const float* __restrict__ fb,
                                                           const float* __restrict__ w, double* __restrict__ part,
                                                           long long P) {
  constexpr int C = 4 * G * N, kPix = 64 / G;  // pixels per wave pass
  __shared__ double red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sub = lane % G, grp = lane / G;
  const float* A = fa + (long long)blockIdx.y * P * C + 4 * sub;
  const float* Bm = fb + (long long)blockIdx.y * P * C + 4 * sub;
  f32x4 wv[N];
#pragma unroll
  for (int j = 0; j < N; ++j) wv[j] = *reinterpret_cast<const f32x4*>(w + 4 * (sub + G * j));
  double acc = 0.0;
  const long long step = (long long)gridDim.x * 4 * kPix;
  for (long long p0 = ((long long)blockIdx.x * 4 + wave) * kPix; p0 < P; p0 += step) {  // wave-uniform
    const long long p = p0 + grp;
    f32x4 a[N], b[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
      a[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      b[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (p < P) {
        a[j] = *reinterpret_cast<const f32x4*>(A + p * C + 4 * G * j);
        b[j] = *reinterpret_cast<const f32x4*>(Bm + p * C + 4 * G * j);
      }
    }
    acc += (double)lpips_pixel<G, N>(a, b, wv);
  }
#pragma unroll
  for (int o = 32; o >= G; o >>= 1) acc += __shfl_xor(acc, o, 64);  // across the wave's groups
  if (lane == 0) red[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0)
    part[(long long)blockIdx.y * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// out[b] = (sum of image b's nparts partials) / n, the partials summed in a fixed order
__global__ void __launch_bounds__(256) lpips_finalize(const double* __restrict__ part, double* __restrict__ out,
                                                       int nparts, double n) {
  __shared__ double red[4];
  const int b = blockIdx.x;
  double acc = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) acc += part[(long long)b * nparts + i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) out[b] = (((red[0] + red[1]) + red[2]) + red[3]) / n;
}

static int lpips_group(int C) {  // lanes per pixel: the largest power of two <= 64 dividing C / 4
  int g = 16;                    // C % 64 == 0
  while (g < 64 && (C / 4) % (2 * g) == 0) g *= 2;
  return g;
}

static long long lpips_blocks(long long P, int C) {
  const long long per_block = 4LL * (64 / lpips_group(C)) * kLpipsPasses;
  return std::min<long long>(std::max<long long>((P + per_block - 1) / per_block, 1), kLpipsMaxBlocks);
}

static bool lpips_c_ok(int C) { return C >= 64 && C <= 512 && C % 64 == 0; }

}  // namespace mhada

using namespace mhada;

extern "C" long long mhada_lpips_layer_work(int B, long long P, int C) {
  if (B <= 0 || P <= 0 || !lpips_c_ok(C)) return 0;
  return (long long)B * lpips_blocks(P, C);
}

extern "C" int mhada_lpips_layer(const float* fa, const float* fb, const float* w, int B, long long P, int C,
                                 double* work, long long work_doubles, double* out, mhada_stream_t s_) {
  if (!fa || !fb || !w || !work || !out || B <= 0 || P <= 0) return fail("mhada_lpips_layer: bad args");
  if (!lpips_c_ok(C)) return fail("mhada_lpips_layer: C must be a multiple of 64 and at most 512");
  if (B > 65535) return fail("mhada_lpips_layer: too many images");
  if (P >= (1LL << 31)) return fail("mhada_lpips_layer: 2^31 pixels or more per image");
  if (((uintptr_t)fa | (uintptr_t)fb | (uintptr_t)w) & 15) return fail("mhada_lpips_layer: pointers must be 16-byte aligned");
  if (work_doubles < mhada_lpips_layer_work(B, P, C))
    return fail("mhada_lpips_layer: workspace too small (mhada_lpips_layer_work)");
  const hipStream_t s = (hipStream_t)s_;
  const int nblk = (int)lpips_blocks(P, C);
  const dim3 grid(nblk, B), block(256);
#define MHADA_LPIPS_CASE(c, g, n)                                                                    \
  case c:                                                                                            \
    hipLaunchKernelGGL((lpips_layer_kernel<g, n>), grid, block, 0, s, fa, fb, w, work, P);            \
    break;
  switch (C) {
    MHADA_LPIPS_CASE(64, 16, 1)
    MHADA_LPIPS_CASE(128, 32, 1)
    MHADA_LPIPS_CASE(192, 16, 3)
    MHADA_LPIPS_CASE(256, 64, 1)
    MHADA_LPIPS_CASE(320, 16, 5)
    MHADA_LPIPS_CASE(384, 32, 3)
    MHADA_LPIPS_CASE(448, 16, 7)
    MHADA_LPIPS_CASE(512, 64, 2)
  }
#undef MHADA_LPIPS_CASE
  if (int rc = check_launch("mhada_lpips_layer/pixels")) return rc;
  hipLaunchKernelGGL(lpips_finalize, dim3(B), dim3(256), 0, s, (const double*)work, out, nblk, (double)P);
  return check_launch("mhada_lpips_layer/finalize");
}
