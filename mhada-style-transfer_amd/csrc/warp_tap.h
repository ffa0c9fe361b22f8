// The bilinear tap of utilities.warp (utilities.py:100-118), shared by every kernel that warps
// (warp.hip, temporal.hip): vgrid = grid + flow normalised with (W-1) / (H-1), then
// F.grid_sample(bilinear, align_corners=False), with the fp32 operation order of the reference's
// tensor ops and ATen's grid_sampler (unnormalise, floor, the four corner weights, taps
// accumulated nw, ne, sw, se; zero padding skips out-of-range taps, border padding clamps the
// coordinate first).
#pragma once
#include "common.h"

namespace mhada {

struct Tap {
  int x0, y0;
  float wnw, wne, wsw, wse;
  bool inw, ine, isw, ise;
};

// Sample position of output pixel (x, y) displaced by (fx, fy); padding 0 zeros, 1 border.
MHADA_DEV Tap warp_tap(int x, int y, float fx, float fy, int H, int W, int padding) {
  const float dx = (float)(W - 1 > 1 ? W - 1 : 1), dy = (float)(H - 1 > 1 ? H - 1 : 1);
  // vgrid normalisation (utilities.py:112-113), one rounding per tensor op
  float gx = 2.0f * ((float)x + fx);
  gx = gx / dx;
  gx = gx - 1.0f;
  float gy = 2.0f * ((float)y + fy);
  gy = gy / dy;
  gy = gy - 1.0f;
  // grid_sampler_unnormalize, align_corners=False
  float ix = ((gx + 1.f) * (float)W - 1.f) / 2.f;
  float iy = ((gy + 1.f) * (float)H - 1.f) / 2.f;
  if (padding == 1) {  // border: clip_coordinates
    ix = fminf(fmaxf(ix, 0.f), (float)(W - 1));
    iy = fminf(fmaxf(iy, 0.f), (float)(H - 1));
  }
  const float fx0 = floorf(ix), fy0 = floorf(iy);
  Tap t;
  t.x0 = (int)fx0;
  t.y0 = (int)fy0;
  const float ix_se = fx0 + 1.f, iy_se = fy0 + 1.f;
  t.wnw = (ix_se - ix) * (iy_se - iy);
  t.wne = (ix - fx0) * (iy_se - iy);
  t.wsw = (ix_se - ix) * (iy - fy0);
  t.wse = (ix - fx0) * (iy - fy0);
  const bool x0in = t.x0 >= 0 && t.x0 < W, x1in = t.x0 + 1 >= 0 && t.x0 + 1 < W;
  const bool y0in = t.y0 >= 0 && t.y0 < H, y1in = t.y0 + 1 >= 0 && t.y0 + 1 < H;
  t.inw = x0in && y0in;
  t.ine = x1in && y0in;
  t.isw = x0in && y1in;
  t.ise = x1in && y1in;
  return t;
}

// The warped value of one contiguous [H][W] plane.
MHADA_DEV float sample(const float* plane, const Tap& t, int W) {
  float acc = 0.f;
  const long long o = (long long)t.y0 * W + t.x0;
  if (t.inw) acc += plane[o] * t.wnw;
  if (t.ine) acc += plane[o + 1] * t.wne;
  if (t.isw) acc += plane[o + W] * t.wsw;
  if (t.ise) acc += plane[o + W + 1] * t.wse;
  return acc;
}

// The same of a plane whose rows are sy and whose pixels are sx elements apart; p points at the
// plane's pixel (0, 0).
MHADA_DEV float sample(const float* p, const Tap& t, long long sy, long long sx) {
  float acc = 0.f;
  const long long o = (long long)t.y0 * sy + (long long)t.x0 * sx;
  if (t.inw) acc += p[o] * t.wnw;
  if (t.ine) acc += p[o + sx] * t.wne;
  if (t.isw) acc += p[o + sy] * t.wsw;
  if (t.ise) acc += p[o + sy + sx] * t.wse;
  return acc;
}

}  // namespace mhada
