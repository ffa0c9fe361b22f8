// The moments of SIFID (SIFID/sifid_score.py:185-205: mu = np.mean(act, axis=0), sigma = np.cov(act,
// rowvar=False)) of fp32 feature rows x [n][C] (the NHWC feature map of ONE image), accumulated in fp64.
// Every sum has a fixed order and there are no floating-point atomics: repeated calls return the same
// bits.  Plain fp64 FMAs over LDS tiles; the largest case (dims 2048 at 512^2: 196 x 196 x 2048, or dims
// 64: 64 x 64 x 64009) is far below 1 GFMA.
//
//   mhada_sifid_stats  mean[c] = sum_i x[i][c] / n and ssq[c] = sum_i (x[i][c] - mean[c])^2, two-pass
//                      (tr S = sum_c ssq[c] / (n - 1));
//   mhada_sifid_cross  G[i][j] = sum_c (x1[i][c] - mu1[c]) (x2[j][c] - mu2[c]), [n1][n2]: the rank-deficient
//                      case min(n1, n2) < C, whose singular values give the trace term;
//   mhada_sifid_cov    S[a][b] = sum_i (x[i][a] - mu[a]) (x[i][b] - mu[b]), [C][C], not divided by n - 1.
#include "common.h"

namespace mhada {

constexpr int kStatGroups = 16;  // row groups per 64-channel workgroup

// grid (ceil(C / 64)), block 1024 = 64 channels x 16 row groups.  Row group g adds rows g, g + 16, ...
// in order; the 16 partial sums of a channel are then added in the order 0..15.
__global__ void __launch_bounds__(64 * kStatGroups) sifid_stats_kernel(const float* __restrict__ x, long long n, int C,
                                                                       double* __restrict__ mean,
                                                                       double* __restrict__ ssq) {
  __shared__ double part[kStatGroups][64];
  __shared__ double mu[64];
  const int cl = threadIdx.x & 63, g = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
  const bool ok = c < C;
  double s = 0.0;
  if (ok)
    for (long long i = g; i < n; i += kStatGroups) s += (double)x[i * C + c];
  part[g][cl] = s;
  __syncthreads();
  if (g == 0) {
    double t = 0.0;
    for (int k = 0; k < kStatGroups; ++k) t += part[k][cl];
    mu[cl] = t / (double)n;
    if (ok) mean[c] = mu[cl];
  }
  __syncthreads();
  const double m = mu[cl];
  s = 0.0;
  if (ok)
    for (long long i = g; i < n; i += kStatGroups) {
      const double d = (double)x[i * C + c] - m;
      s = fma(d, d, s);
    }
  __syncthreads();
  part[g][cl] = s;
  __syncthreads();
  if (g == 0 && ok) {
    double t = 0.0;
    for (int k = 0; k < kStatGroups; ++k) t += part[k][cl];
    ssq[c] = t;
  }
}

// out[i][j] = sum_c (a[i][c] - ma[c]) (b[j][c] - mb[c]); 16 x 16 outputs per workgroup of 256, C walked
// in chunks of 32 staged centred in LDS; each output is one fma chain over c = 0 .. C - 1.
__global__ void __launch_bounds__(256) sifid_cross_kernel(const float* __restrict__ a, const double* __restrict__ ma,
                                                           long long na, const float* __restrict__ b,
                                                           const double* __restrict__ mb, long long nb, int C,
                                                           double* __restrict__ out) {
  __shared__ double As[16][33], Bs[16][33];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const long long i0 = (long long)blockIdx.y * 16, j0 = (long long)blockIdx.x * 16;
  double acc = 0.0;
  for (int c0 = 0; c0 < C; c0 += 32) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int e = threadIdx.x + 256 * k, r = e >> 5, cc = e & 31, c = c0 + cc;
      const long long i = i0 + r, j = j0 + r;
      As[r][cc] = (i < na && c < C) ? (double)a[i * C + c] - ma[c] : 0.0;
      Bs[r][cc] = (j < nb && c < C) ? (double)b[j * C + c] - mb[c] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int cc = 0; cc < 32; ++cc) acc = fma(As[ty][cc], Bs[tx][cc], acc);
    __syncthreads();
  }
  if (i0 + ty < na && j0 + tx < nb) out[(i0 + ty) * nb + j0 + tx] = acc;
}

// out[p][q] = sum_i (x[i][p] - m[p]) (x[i][q] - m[q]); 16 x 16 outputs per workgroup, the rows walked in
// chunks of 32; each output is one fma chain over i = 0 .. n - 1.
__global__ void __launch_bounds__(256) sifid_cov_kernel(const float* __restrict__ x, const double* __restrict__ m,
                                                         long long n, int C, double* __restrict__ out) {
  __shared__ double Ps[32][17], Qs[32][17];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int p0 = blockIdx.y * 16, q0 = blockIdx.x * 16;
  double acc = 0.0;
  for (long long r0 = 0; r0 < n; r0 += 32) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int e = threadIdx.x + 256 * k, r = e >> 4, cc = e & 15;
      const long long i = r0 + r;
      const int p = p0 + cc, q = q0 + cc;
      Ps[r][cc] = (i < n && p < C) ? (double)x[i * C + p] - m[p] : 0.0;
      Qs[r][cc] = (i < n && q < C) ? (double)x[i * C + q] - m[q] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 32; ++r) acc = fma(Ps[r][ty], Qs[r][tx], acc);
    __syncthreads();
  }
  if (p0 + ty < C && q0 + tx < C) out[(long long)(p0 + ty) * C + q0 + tx] = acc;
}

}  // namespace mhada

using namespace mhada;

extern "C" int mhada_sifid_stats(const float* x, long long n, int C, double* mean, double* ssq, mhada_stream_t s_) {
  if (!x || !mean || !ssq) return fail("mhada_sifid_stats: null pointer");
  if (n <= 0 || C <= 0) return fail("mhada_sifid_stats: n and C must be positive");
  if (n >= (1LL << 31) || C > (1 << 20)) return fail("mhada_sifid_stats: 2^31 rows or more, or more than 2^20 channels");
  hipLaunchKernelGGL(sifid_stats_kernel, dim3((C + 63) / 64), dim3(64 * kStatGroups), 0, (hipStream_t)s_, x, n, C, mean, ssq);
  return check_launch("mhada_sifid_stats");
}

extern "C" int mhada_sifid_cross(const float* x1, const double* mean1, long long n1, const float* x2,
                                 const double* mean2, long long n2, int C, double* out, mhada_stream_t s_) {
  if (!x1 || !mean1 || !x2 || !mean2 || !out) return fail("mhada_sifid_cross: null pointer");
  if (n1 <= 0 || n2 <= 0 || C <= 0) return fail("mhada_sifid_cross: n1, n2 and C must be positive");
  if ((n1 + 15) / 16 > 65535 || (n2 + 15) / 16 >= (1LL << 31) || C > (1 << 20))
    return fail("mhada_sifid_cross: n1 above 16 * 65535, or sizes of 2^31 or more");
  hipLaunchKernelGGL(sifid_cross_kernel, dim3((unsigned)((n2 + 15) / 16), (unsigned)((n1 + 15) / 16)), dim3(256), 0,
                     (hipStream_t)s_, x1, mean1, n1, x2, mean2, n2, C, out);
  return check_launch("mhada_sifid_cross");
}

extern "C" int mhada_sifid_cov(const float* x, const double* mean, long long n, int C, double* out, mhada_stream_t s_) {
  if (!x || !mean || !out) return fail("mhada_sifid_cov: null pointer");
  if (n <= 0 || C <= 0) return fail("mhada_sifid_cov: n and C must be positive");
  if (n >= (1LL << 31) || C > 16 * 65535) return fail("mhada_sifid_cov: 2^31 rows or more, or C above 16 * 65535");
  hipLaunchKernelGGL(sifid_cov_kernel, dim3((C + 15) / 16, (C + 15) / 16), dim3(256), 0, (hipStream_t)s_, x, mean, n, C, out);
  return check_launch("mhada_sifid_cov");
}
