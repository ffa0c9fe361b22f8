// The temporal losses of train_video.py (lossfn.py:50-86) as HBM-bound streaming kernels with no
// host synchronisation: the reference ends each loss in torch.nonzero(m).shape[0], a device-to-host
// copy; here the count of m != 0 is reduced on the device beside the sum.
//
//   loss = sum_{b,c,y,x} m[b,y,x] * (x2 - warp(x1, flow) - t[b,y,x])^2 / (C * #{m != 0})
//
// temporal_loss_fwd: fp64 partial sum and integer count per workgroup in a fixed order, then one
// finalize workgroup in a fixed order (no atomics: the scalar is bit-identical from run to run).
// temporal_loss_bwd: recomputes the residual, writes dx2 = r = 2 m (x2 - warp(x1) - t) g / (C count)
// and scatters -r to the four taps of dx1 with fp32 atomics, as warp_bwd_kernel does.
// flow_mask_resize: the feature-level prologue (lossfn.py:71-80), F.interpolate(bilinear) of the
// flow (scaled to the feature grid) and of the mask (> 0).
//
// x1 / x2 carry explicit element strides.  Two thread mappings, picked from the channel stride:
//   PIX  one lane per pixel, a loop over a group of channels: coalesced when x is the unit
//        stride (contiguous NCHW: c1/c2/cs1/cs2);
//   CH   one wave per pixel, lanes over channels: coalesced when c is the unit stride (the
//        channels_last views of token-major storage: ada_fcs1/2).  The forward reads 16 B per lane
//        where alignment and strides allow (V = 4); the backward keeps one channel per lane, so
//        that each of its atomic wave-instructions covers 256 contiguous bytes.
// The warp's arithmetic is warp_tap.h's, shared with warp.hip.
#include <limits.h>

#include <algorithm>

#include "common.h"
#include "warp_tap.h"

namespace mhada {

constexpr int kTlMaxBlocks = MHADA_TEMPORAL_MAX_BLOCKS;
constexpr int kTlCpg = 16;  // PIX: channels per work item

struct Strides { long long b, c, y, x; };

struct TlArgs {
  const float *x1, *x2, *flow, *m, *c1, *c2;  // c1 == nullptr: no luminance target
  Strides s1, s2;
  int B, C, H, W;
};

// What every channel of one pixel shares.
struct TlPix {
  Tap tap;
  float m, t;
  int b, py, px;
  long long o1, o2;  // element offsets of x1's pixel (0, 0) of image b / of x2's pixel, channel 0
};

MHADA_DEV TlPix tl_pixel(const TlArgs& a, long long gp) {
  const long long HW = (long long)a.H * a.W;
  const int b = (int)(gp / HW);
  const long long pix = gp - (long long)b * HW;
  const int py = (int)(pix / a.W), px = (int)(pix - (long long)py * a.W);
  TlPix p;
  p.b = b;
  p.py = py;
  p.px = px;
  p.m = a.m[gp];
  p.t = 0.f;
  p.o1 = (long long)b * a.s1.b;
  p.o2 = (long long)b * a.s2.b + (long long)py * a.s2.y + (long long)px * a.s2.x;
  const float* fl = a.flow + (long long)b * 2 * HW;
  p.tap = warp_tap(px, py, fl[pix], fl[HW + pix], a.H, a.W, 0);
  if (a.c1) {
    // lossfn.py:52-53: 0.2126 r + 0.7152 g + 0.0722 b of c2 - warp(c1), one rounding per tensor op
    const float* w = a.c1 + (long long)b * 3 * HW;
    const float* o = a.c2 + (long long)b * 3 * HW;
    const float i0 = o[pix] - sample(w, p.tap, a.W);
    const float i1 = o[HW + pix] - sample(w + HW, p.tap, a.W);
    const float i2 = o[2 * HW + pix] - sample(w + 2 * HW, p.tap, a.W);
    p.t = __fadd_rn(__fadd_rn(__fmul_rn(0.2126f, i0), __fmul_rn(0.7152f, i1)), __fmul_rn(0.0722f, i2));
  }
  return p;
}

// (x2 - warp(x1)) - t of channel c
MHADA_DEV float tl_resid(const TlArgs& a, const TlPix& p, int c) {
  const float w = sample(a.x1 + p.o1 + (long long)c * a.s1.c, p.tap, a.s1.y, a.s1.x);
  return __fsub_rn(__fsub_rn(a.x2[p.o2 + (long long)c * a.s2.c], w), p.t);
}

MHADA_DEV double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
MHADA_DEV long long wave_sum_i64(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One partial sum and count per workgroup, the four waves added in a fixed order.
MHADA_DEV void tl_block_out(double acc, long long n, double* part, long long* cnt) {
  __shared__ double red[4];
  __shared__ long long redn[4];
  acc = wave_sum_f64(acc);
  n = wave_sum_i64(n);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = acc;
    redn[threadIdx.x >> 6] = n;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
    cnt[blockIdx.x] = ((redn[0] + redn[1]) + redn[2]) + redn[3];
  }
}

// PIX: work item = (block of 256 pixels of the flattened [B][H][W], group of kTlCpg channels).
__global__ void __launch_bounds__(256) temporal_fwd_pix_kernel(TlArgs a, int ncg, long long nitems, double* part,
                                                               long long* cnt) {
  const long long NP = (long long)a.B * a.H * a.W;
  double acc = 0.0;
  long long n = 0;
  for (long long it = blockIdx.x; it < nitems; it += gridDim.x) {
    const long long pb = it / ncg;
    const int cg = (int)(it - pb * ncg);
    const long long gp = pb * 256 + threadIdx.x;
    if (gp >= NP) continue;
    const float m = a.m[gp];
    if (m == 0.f) continue;
    if (cg == 0) ++n;
    const TlPix p = tl_pixel(a, gp);
    const int c1 = min(a.C, (cg + 1) * kTlCpg);
    for (int c = cg * kTlCpg; c < c1; ++c) {
      const float d = tl_resid(a, p, c);
      acc += (double)__fmul_rn(m, __fmul_rn(d, d));
    }
  }
  tl_block_out(acc, n, part, cnt);
}

// CH: work item = four pixels, one per wave; lane l takes channels V l .. V l + V - 1, then 64 V further on.
template <int V>
__global__ void __launch_bounds__(256) temporal_fwd_ch_kernel(TlArgs a, long long nitems, double* part, long long* cnt) {
  const long long NP = (long long)a.B * a.H * a.W;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double acc = 0.0;
  long long n = 0;
  for (long long it = blockIdx.x; it < nitems; it += gridDim.x) {
    const long long gp = it * 4 + wave;
    if (gp >= NP) continue;
    const float m = a.m[gp];
    if (m == 0.f) continue;
    if (lane == 0) ++n;
    const TlPix p = tl_pixel(a, gp);
    if constexpr (V == 4) {
      const Tap& t = p.tap;
      const float* q = a.x1 + p.o1 + (long long)t.y0 * a.s1.y + (long long)t.x0 * a.s1.x;
      for (int c = lane * 4; c < a.C; c += 256) {
        const f32x4 v2 = ld4(a.x2 + p.o2 + c);
        f32x4 w = {0.f, 0.f, 0.f, 0.f};
        if (t.inw) w += ld4(q + c) * t.wnw;
        if (t.ine) w += ld4(q + a.s1.x + c) * t.wne;
        if (t.isw) w += ld4(q + a.s1.y + c) * t.wsw;
        if (t.ise) w += ld4(q + a.s1.y + a.s1.x + c) * t.wse;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float d = __fsub_rn(__fsub_rn(v2[j], w[j]), p.t);
          acc += (double)__fmul_rn(m, __fmul_rn(d, d));
        }
      }
    } else {
      for (int c = lane; c < a.C; c += 64) {
        const float d = tl_resid(a, p, c);
        acc += (double)__fmul_rn(m, __fmul_rn(d, d));
      }
    }
  }
  tl_block_out(acc, n, part, cnt);
}

// work[0] = count, out = sum / (C * count): the partials of the nb workgroups in a fixed order.
__global__ void __launch_bounds__(256) temporal_finalize_kernel(const double* __restrict__ part,
                                                                const long long* __restrict__ cnt, int nb, int C,
                                                                long long* __restrict__ count, float* __restrict__ out) {
  __shared__ double red[4];
  __shared__ long long redn[4];
  double acc = 0.0;
  long long n = 0;
  for (int i = threadIdx.x; i < nb; i += 256) {
    acc += part[i];
    n += cnt[i];
  }
  acc = wave_sum_f64(acc);
  n = wave_sum_i64(n);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = acc;
    redn[threadIdx.x >> 6] = n;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const long long total = ((redn[0] + redn[1]) + redn[2]) + redn[3];
    count[0] = total;
    // an all-zero mask: 0 / 0 = NaN (the reference raises ZeroDivisionError, which needs the host)
    out[0] = (float)((((red[0] + red[1]) + red[2]) + red[3]) / ((double)C * (double)total));
  }
}

struct TlGrad {
  float *dx1, *dx2;  // either may be nullptr
  Strides sd1, sd2;
  const long long* count;
  const float* g;
};

// g / (C count) as the reference forms it: the upstream gradient times the fp32 value of 1 / N
MHADA_DEV float tl_scale(const TlGrad& gr, int C) {
  return __fmul_rn(gr.g[0], (float)(1.0 / ((double)C * (double)gr.count[0])));
}

// one (pixel, channel) of the backward: dx2 = r, dx1[taps] -= w r
MHADA_DEV void tl_bwd_elem(const TlArgs& a, const TlGrad& gr, const TlPix& p, float ms, int c) {
  // mse_loss_backward: 2 (input - target) grad, grad = m * (g / N); a masked pixel needs no residual
  const float r = p.m == 0.f ? ms : __fmul_rn(__fmul_rn(2.f, tl_resid(a, p, c)), ms);
  if (gr.dx2)
    gr.dx2[(long long)p.b * gr.sd2.b + (long long)c * gr.sd2.c + (long long)p.py * gr.sd2.y + (long long)p.px * gr.sd2.x] = r;
  if (!gr.dx1 || r == 0.f) return;
  const Tap& t = p.tap;
  float* q = gr.dx1 + (long long)p.b * gr.sd1.b + (long long)c * gr.sd1.c + (long long)t.y0 * gr.sd1.y +
             (long long)t.x0 * gr.sd1.x;
  if (t.inw) unsafeAtomicAdd(q, t.wnw * -r);
  if (t.ine) unsafeAtomicAdd(q + gr.sd1.x, t.wne * -r);
  if (t.isw) unsafeAtomicAdd(q + gr.sd1.y, t.wsw * -r);
  if (t.ise) unsafeAtomicAdd(q + gr.sd1.y + gr.sd1.x, t.wse * -r);
}

__global__ void __launch_bounds__(256) temporal_bwd_pix_kernel(TlArgs a, TlGrad gr, int ncg, long long nitems) {
  const long long NP = (long long)a.B * a.H * a.W;
  const float s = tl_scale(gr, a.C);
  for (long long it = blockIdx.x; it < nitems; it += gridDim.x) {
    const long long pb = it / ncg;
    const int cg = (int)(it - pb * ncg);
    const long long gp = pb * 256 + threadIdx.x;
    if (gp >= NP) continue;
    const TlPix p = tl_pixel(a, gp);
    const float ms = __fmul_rn(p.m, s);
    const int c1 = min(a.C, (cg + 1) * kTlCpg);
    for (int c = cg * kTlCpg; c < c1; ++c) tl_bwd_elem(a, gr, p, ms, c);
  }
}

__global__ void __launch_bounds__(256) temporal_bwd_ch_kernel(TlArgs a, TlGrad gr, long long nitems) {
  const long long NP = (long long)a.B * a.H * a.W;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const float s = tl_scale(gr, a.C);
  for (long long it = blockIdx.x; it < nitems; it += gridDim.x) {
    const long long gp = it * 4 + wave;
    if (gp >= NP) continue;
    const TlPix p = tl_pixel(a, gp);
    const float ms = __fmul_rn(p.m, s);
    for (int c = lane; c < a.C; c += 64) tl_bwd_elem(a, gr, p, ms, c);
  }
}

// lossfn.py:71-80 on the device: aten's upsample_bilinear2d (align_corners=False, no antialias; the
// source index clamped at 0) of the flow, channel 0 scaled by sx = Wf / W and channel 1 by sy = Hf / H,
// and of the mask followed by > 0.  One lane per feature-grid pixel.
__global__ void __launch_bounds__(256) flow_mask_resize_kernel(const float* __restrict__ flow, const float* __restrict__ mask,
                                                               float* __restrict__ fflow, float* __restrict__ fmask, int H,
                                                               int W, int Hf, int Wf, float rh, float rw, float sx,
                                                               float sy) {
  const int b = blockIdx.y;
  const long long HWf = (long long)Hf * Wf, HW = (long long)H * W;
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  if (o >= HWf) return;
  const int oy = (int)(o / Wf), ox = (int)(o - (long long)oy * Wf);
  // area_pixel_compute_source_index
  const float fy = fmaxf(rh * ((float)oy + 0.5f) - 0.5f, 0.f);
  const float fx = fmaxf(rw * ((float)ox + 0.5f) - 0.5f, 0.f);
  const int y0 = (int)fy, x0 = (int)fx;
  const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
  const float ly1 = fy - (float)y0, lx1 = fx - (float)x0;
  const float ly0 = 1.f - ly1, lx0 = 1.f - lx1;
  const long long o00 = (long long)y0 * W + x0, o01 = (long long)y0 * W + x1;
  const long long o10 = (long long)y1 * W + x0, o11 = (long long)y1 * W + x1;
  auto at = [&](const float* p) { return bilerp(ly0, ly1, lx0, lx1, p[o00], p[o01], p[o10], p[o11]); };
  const float* f = flow + (long long)b * 2 * HW;
  fflow[(long long)b * 2 * HWf + o] = at(f) * sx;
  fflow[(long long)b * 2 * HWf + HWf + o] = at(f + HW) * sy;
  fmask[(long long)b * HWf + o] = at(mask + (long long)b * HW) > 0.f ? 1.f : 0.f;
}

static bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

// Arguments common to the forward and the backward; the message names what is wrong.
static const char* tl_check(const float* x1, const long long* s1, const float* x2, const long long* s2, const float* flow,
                            const float* m, const float* c1, const float* c2, const void* work, int B, int C, int H,
                            int W) {
  if (!x1 || !s1 || !x2 || !s2 || !flow || !m || !work || B <= 0 || C <= 0 || H <= 0 || W <= 0) return "bad args";
  if ((c1 == nullptr) != (c2 == nullptr)) return "bad args (c1 and c2 go together)";
  if (!aligned4(x1) || !aligned4(x2) || !aligned4(flow) || !aligned4(m) || !aligned4(c1) || !aligned4(c2) ||
      ((uintptr_t)work & 7))
    return "misaligned pointer (fp32 tensors 4 bytes, the workspace 8)";
  for (int i = 0; i < 4; ++i)
    if (s1[i] < 0 || s2[i] < 0) return "bad args (negative stride)";
  if ((long long)B * H * W > (long long)INT_MAX - 256) return "bad args (B*H*W past 2^31)";
  return nullptr;
}

static Strides strides_of(const long long* s) { return Strides{s[0], s[1], s[2], s[3]}; }

// lanes over channels when both tensors have the channel as their unit stride
static bool tl_ch_form(const TlArgs& a) { return a.C > 1 && a.s1.c == 1 && a.s2.c == 1; }

static bool tl_vec4(const TlArgs& a) {
  auto ok = [](const Strides& s) { return s.b % 4 == 0 && s.y % 4 == 0 && s.x % 4 == 0; };
  return a.C % 4 == 0 && ok(a.s1) && ok(a.s2) && aligned16(a.x1) && aligned16(a.x2);
}

}  // namespace mhada

using namespace mhada;

extern "C" int mhada_temporal_loss_fwd(const float* x1, const long long* sx1, const float* x2, const long long* sx2,
                                       const float* flow, const float* m, const float* c1, const float* c2,
                                       void* work, float* out, int B, int C, int H, int W, mhada_stream_t s_) {
  const char* bad = tl_check(x1, sx1, x2, sx2, flow, m, c1, c2, work, B, C, H, W);
  if (!bad && !out) bad = "bad args";
  if (!bad && !aligned4(out)) bad = "misaligned pointer (fp32 tensors 4 bytes, the workspace 8)";
  if (bad) return fail(std::string("mhada_temporal_loss_fwd: ") + bad);
  const TlArgs a{x1, x2, flow, m, c1, c2, strides_of(sx1), strides_of(sx2), B, C, H, W};
  const long long NP = (long long)B * H * W;
  long long* w = static_cast<long long*>(work);
  double* part = reinterpret_cast<double*>(w + 1);
  long long* cnt = w + 1 + kTlMaxBlocks;
  hipStream_t s = (hipStream_t)s_;
  int nb;
  if (tl_ch_form(a)) {
    const long long nitems = (NP + 3) / 4;
    nb = (int)std::min<long long>(nitems, kTlMaxBlocks);
    if (tl_vec4(a))
      hipLaunchKernelGGL(temporal_fwd_ch_kernel<4>, dim3(nb), dim3(256), 0, s, a, nitems, part, cnt);
    else
      hipLaunchKernelGGL(temporal_fwd_ch_kernel<1>, dim3(nb), dim3(256), 0, s, a, nitems, part, cnt);
  } else {
    const int ncg = (C + kTlCpg - 1) / kTlCpg;
    const long long nitems = (NP + 255) / 256 * ncg;
    nb = (int)std::min<long long>(nitems, kTlMaxBlocks);
    hipLaunchKernelGGL(temporal_fwd_pix_kernel, dim3(nb), dim3(256), 0, s, a, ncg, nitems, part, cnt);
  }
  hipLaunchKernelGGL(temporal_finalize_kernel, dim3(1), dim3(256), 0, s, (const double*)part, (const long long*)cnt, nb,
                     C, w, out);
  return check_launch("mhada_temporal_loss_fwd");
}

extern "C" int mhada_temporal_loss_bwd(const float* x1, const long long* sx1, const float* x2, const long long* sx2,
                                       const float* flow, const float* m, const float* c1, const float* c2,
                                       const void* work, const float* gout, float* dx1, const long long* sdx1,
                                       float* dx2, const long long* sdx2, int B, int C, int H, int W,
                                       mhada_stream_t s_) {
  const char* bad = tl_check(x1, sx1, x2, sx2, flow, m, c1, c2, work, B, C, H, W);
  if (!bad && (!gout || (dx1 && !sdx1) || (dx2 && !sdx2))) bad = "bad args";
  if (!bad && (!aligned4(gout) || !aligned4(dx1) || !aligned4(dx2)))
    bad = "misaligned pointer (fp32 tensors 4 bytes, the workspace 8)";
  if (!bad)
    for (int i = 0; i < 4; ++i)
      if ((dx1 && sdx1[i] < 0) || (dx2 && sdx2[i] < 0)) bad = "bad args (negative stride)";
  if (bad) return fail(std::string("mhada_temporal_loss_bwd: ") + bad);
  if (!dx1 && !dx2) return MHADA_OK;
  const TlArgs a{x1, x2, flow, m, c1, c2, strides_of(sx1), strides_of(sx2), B, C, H, W};
  const Strides z{0, 0, 0, 0};
  const TlGrad gr{dx1, dx2, dx1 ? strides_of(sdx1) : z, dx2 ? strides_of(sdx2) : z,
                  static_cast<const long long*>(work), gout};
  const long long NP = (long long)B * H * W;
  hipStream_t s = (hipStream_t)s_;
  if (tl_ch_form(a)) {
    const long long nitems = (NP + 3) / 4;
    const int nb = (int)std::min<long long>(nitems, kTlMaxBlocks);
    hipLaunchKernelGGL(temporal_bwd_ch_kernel, dim3(nb), dim3(256), 0, s, a, gr, nitems);
  } else {
    const int ncg = (C + kTlCpg - 1) / kTlCpg;
    const long long nitems = (NP + 255) / 256 * ncg;
    const int nb = (int)std::min<long long>(nitems, kTlMaxBlocks);
    hipLaunchKernelGGL(temporal_bwd_pix_kernel, dim3(nb), dim3(256), 0, s, a, gr, ncg, nitems);
  }
  return check_launch("mhada_temporal_loss_bwd");
}

extern "C" int mhada_flow_mask_resize(const float* flow, const float* mask, float* fflow, float* fmask, int B, int H,
                                      int W, int Hf, int Wf, mhada_stream_t s_) {
  if (!flow || !mask || !fflow || !fmask || B <= 0 || H <= 0 || W <= 0 || Hf <= 0 || Wf <= 0 || B > 65535)
    return fail("mhada_flow_mask_resize: bad args");
  if (!aligned4(flow) || !aligned4(mask) || !aligned4(fflow) || !aligned4(fmask))
    return fail("mhada_flow_mask_resize: misaligned pointer (fp32 tensors 4 bytes)");
  const long long HWf = (long long)Hf * Wf;
  if (HWf > (long long)INT_MAX - 256) return fail("mhada_flow_mask_resize: bad args (Hf*Wf past 2^31)");
  // aten: the scale as fp32 in / out; lossfn.py:72-73: the flow factors as Python floats, applied in fp32
  hipLaunchKernelGGL(flow_mask_resize_kernel, dim3((unsigned)((HWf + 255) / 256), B), dim3(256), 0, (hipStream_t)s_, flow,
                     mask, fflow, fmask, H, W, Hf, Wf, (float)H / (float)Hf, (float)W / (float)Wf,
                     (float)((double)Wf / (double)W), (float)((double)Hf / (double)H));
  return check_launch("mhada_flow_mask_resize");
}
