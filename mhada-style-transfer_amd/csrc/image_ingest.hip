// Image ingest: the input preparation of every image entry point of the reference (infer_image.py:69,76,
// exps_image.py, exps_image_all.py, visual_*.py, and the style image of infer_video.py:58),
//   Image.open(p).convert("RGB").resize((W, H), Image.BILINEAR)  ->  toTensor255   (utilities.py:11-16)
// on a u8 HWC image already in device memory, bit for bit as PIL computes it.
//
// PIL's BILINEAR resize of 8-bit channels (Resample.c) is a separable resample with a triangle filter that
// is widened by the scale factor when shrinking (an antialiased resample, not F.interpolate), in 22-bit
// fixed point.  Per axis, for n_in -> n_out, output index i owns `count` taps starting at source index
// `xmin` with integer coefficients k[0..count) (sum ~ 2^22); one pass along the axis is, per channel,
//   out = clamp((2^21 + sum_t in[xmin + t] * k[t]) >> 22, 0, 255)   in 32-bit integers (< 2^31).
// The horizontal pass runs first (only if Wo != W) and ROUNDS TO u8; the vertical pass (only if Ho != H)
// runs on that u8 image.  The same size on both axes is a copy.  Then ToTensor's x / 255 and toTensor255's
// * 255, two correctly rounded fp32 operations, exactly as frame_ingest_kernel ends.
//
// The coefficients are an INPUT: int32 [n_out][ksize] and int32 [n_out][2] = (xmin, count) per axis, built
// on the host in float64 (ops.pil_bilinear_tables).  Nothing here recomputes a weight: an FMA contraction of
// the triangle changes its last bit and, rarely, a coefficient.  There is no floating point before the
// final toTensor255.
//
// Structure: two launches of one kernel template.  The horizontal pass writes a packed u8 workspace
// [B][H][Wo][3] (the caller's, mhada_image_resize_work bytes), the vertical pass reads it: the source leaves
// HBM once.  A pass that is the last one writes the outputs itself (u8 HWC and / or fp32 planar), so a
// one-axis resize and the copy are one launch and need no workspace.
//
// A workgroup is 64 lanes along x by 4 waves along y.  Horizontal: neighbouring lanes own neighbouring
// output pixels of one source row, so their footprints (3 * scale bytes apart) overlap in L1/L2; a lane
// carries kResizeRows rows of its column, which share the lane's coefficients (its coefficient row is
// strided against its neighbours': one table load then feeds 3 * kResizeRows products).  Vertical: a
// wave owns 64 pixels of one output row, every tap is a contiguous 192-byte row read and the coefficient
// is the same in all lanes.
#include "common.h"

namespace mhada {

constexpr int kResizeX = 64;     // lanes along x (one wave)
constexpr int kResizeY = 4;      // waves along y
constexpr int kResizeRows = 4;   // rows per lane in the horizontal pass

enum { kAlongX = 0, kAlongY = 1, kCopy = 2 };

// (xmin, count) of output index i, clipped to the table row and the axis: a table that does not belong to
// these sizes reads wrong pixels, never out of bounds
MHADA_DEV void resize_bounds(const int* __restrict__ bounds, int i, int n_in, int ksize, int& xmin, int& count) {
  xmin = min(max(bounds[2 * i], 0), n_in);
  count = max(min(min(bounds[2 * i + 1], ksize), n_in - xmin), 0);
}

MHADA_DEV int resize_round(int ss) { return min(max(ss >> 22, 0), 255); }

// One pass.  AXIS kAlongX: out (oy, ox) from in (oy, xmin .. xmin + count), R rows per lane; kAlongY: from in
// (ymin .. ymin + count, ox); kCopy: in (oy, ox).  Ho x Wo is the size this pass writes; n_in the length of
// the resampled axis of `in`.  in: u8 rows of in_row bytes, images in_img bytes apart.  out_u8 (nullable):
// rows of out_row bytes, images out_img apart, padding never written; out_f32 (nullable): [B][3][Ho][Wo].
// bgr swaps channels 0 and 2 (set on the last pass only: the swap commutes with the per-channel filter).
template <int AXIS, int R>
__global__ void __launch_bounds__(kResizeX* kResizeY)
    image_resize_pass(const uint8_t* __restrict__ in, long long in_row, long long in_img, int n_in,
                      const int* __restrict__ coef, const int* __restrict__ bounds, int ksize, int Ho, int Wo,
                      uint8_t* __restrict__ out_u8, long long out_row, long long out_img, float* __restrict__ out_f32,
                      int bgr) {
  const int lane = threadIdx.x;
  const int ox = blockIdx.x * kResizeX + lane;
  const int oy0 = (blockIdx.y * kResizeY + threadIdx.y) * R;  // the same in every lane of a wave
  const int b = blockIdx.z;
  if (oy0 >= Ho) return;  // whole waves only: every lane of a live wave reaches the stores' shuffle
  const int oxc = min(ox, Wo - 1);  // lanes past the row compute in bounds, store nothing
  const uint8_t* img = in + (long long)b * in_img;
  int acc[R][3];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r][0] = acc[r][1] = acc[r][2] = 1 << 21;

  if constexpr (AXIS == kAlongX) {
    int xmin, count;
    resize_bounds(bounds, oxc, n_in, ksize, xmin, count);
    const int* k = coef + (long long)oxc * ksize;
    const uint8_t* p[R];
#pragma unroll
    for (int r = 0; r < R; ++r) p[r] = img + (long long)min(oy0 + r, Ho - 1) * in_row + 3LL * xmin;
    for (int t = 0; t < count; ++t) {
      const int kt = k[t];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        acc[r][0] += (int)p[r][3 * t] * kt;
        acc[r][1] += (int)p[r][3 * t + 1] * kt;
        acc[r][2] += (int)p[r][3 * t + 2] * kt;
      }
    }
  } else if constexpr (AXIS == kAlongY) {
    static_assert(R == 1, "the vertical pass carries one row per lane");
    const int oy = __builtin_amdgcn_readfirstlane(oy0);
    int ymin, count;
    resize_bounds(bounds, oy, n_in, ksize, ymin, count);
    const int* k = coef + (long long)oy * ksize;
    const uint8_t* p = img + (long long)ymin * in_row + 3LL * oxc;
    for (int t = 0; t < count; ++t, p += in_row) {
      const int kt = k[t];
      acc[0][0] += (int)p[0] * kt;
      acc[0][1] += (int)p[1] * kt;
      acc[0][2] += (int)p[2] * kt;
    }
  } else {
    static_assert(R == 1, "the copy carries one row per lane");
    const uint8_t* p = img + (long long)oy0 * in_row + 3LL * oxc;
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[0][c] = (int)p[c] << 22;
  }

  const long long plane = (long long)Ho * Wo;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int oy = oy0 + r;
    const bool row = oy < Ho;  // the same in every lane of a wave
    const int v0 = resize_round(acc[r][bgr ? 2 : 0]), v1 = resize_round(acc[r][1]),
              v2 = resize_round(acc[r][bgr ? 0 : 2]);
    if (out_u8) {
      uint8_t* q = out_u8 + (long long)b * out_img + (long long)min(oy, Ho - 1) * out_row + 3LL * oxc;
      // lanes ox & 3 = 0..3 hold four consecutive pixels of the row when the last of them exists
      emit_store_px(q, (uint32_t)v0 | ((uint32_t)v1 << 8) | ((uint32_t)v2 << 16), lane & 3, row && ox < Wo,
                    row && (ox | 3) < Wo);
    }
    if (out_f32 && row && ox < Wo) {
      float* o = out_f32 + (long long)b * 3 * plane + (long long)oy * Wo + ox;
      // ToTensor (/255) then .mul(255): two fp32 roundings, as the reference's tensor ops
      o[0] = ((float)v0 / 255.0f) * 255.0f;
      o[plane] = ((float)v1 / 255.0f) * 255.0f;
      o[2 * plane] = ((float)v2 / 255.0f) * 255.0f;
    }
  }
}

static long long resize_work_bytes(int B, int H, int W, int Ho, int Wo) {
  return (Wo != W && Ho != H) ? 3LL * B * H * Wo : 0;
}

struct ResizeOut {
  uint8_t* u8;
  long long row, img;
  float* f32;
  int bgr;
};

template <int AXIS, int R>
static int resize_launch(const char* what, const uint8_t* in, long long in_row, long long in_img, int n_in,
                         const int* coef, const int* bounds, int ksize, int B, int Ho, int Wo, const ResizeOut& o,
                         hipStream_t s) {
  const dim3 grid((unsigned)((Wo + kResizeX - 1) / kResizeX),
                  (unsigned)((Ho + kResizeY * R - 1) / (kResizeY * R)), (unsigned)B);
  hipLaunchKernelGGL((image_resize_pass<AXIS, R>), grid, dim3(kResizeX, kResizeY), 0, s, in, in_row, in_img, n_in, coef,
                     bounds, ksize, Ho, Wo, o.u8, o.row, o.img, o.f32, o.bgr);
  return check_launch(what);
}

}  // namespace mhada

using namespace mhada;

extern "C" long long mhada_image_resize_work(int B, int H, int W, int Ho, int Wo) {
  if (B <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0) return 0;
  return resize_work_bytes(B, H, W, Ho, Wo);
}

extern "C" int mhada_image_resize(const void* frames, int B, int H, int W, long long row_bytes, int bgr,
                                  const int* coef_x, const int* bounds_x, int ksize_x, const int* coef_y,
                                  const int* bounds_y, int ksize_y, void* out_u8, long long out_row_bytes,
                                  float* out_f32, int Ho, int Wo, void* work, long long work_bytes,
                                  mhada_stream_t s_) {
  if (!frames || B <= 0 || H <= 0 || W <= 0 || Ho <= 0 || Wo <= 0) return fail("mhada_image_resize: bad args");
  if (!out_u8 && !out_f32) return fail("mhada_image_resize: both outputs are null");
  if (row_bytes < 3LL * W) return fail("mhada_image_resize: row_bytes < 3*W");
  if (out_u8 && out_row_bytes < 3LL * Wo) return fail("mhada_image_resize: out_row_bytes < 3*Wo");
  if ((uintptr_t)out_f32 & 3) return fail("mhada_image_resize: out_f32 is not 4-byte aligned");
  const bool px = Wo != W, py = Ho != H;
  if (px && (!coef_x || !bounds_x || ksize_x <= 0 || (((uintptr_t)coef_x | (uintptr_t)bounds_x) & 3)))
    return fail("mhada_image_resize: the x tables are null, misaligned or empty");
  if (py && (!coef_y || !bounds_y || ksize_y <= 0 || (((uintptr_t)coef_y | (uintptr_t)bounds_y) & 3)))
    return fail("mhada_image_resize: the y tables are null, misaligned or empty");
  // 3 * x in an int; the grid's y and z extents (the horizontal pass covers the H source rows)
  const int kMaxW = 0x7FFFFFFF / 3;
  if (W > kMaxW || Wo > kMaxW) return fail("mhada_image_resize: more than (2^31 - 1) / 3 pixels in a row");
  if (B > 65535) return fail("mhada_image_resize: too many images");
  if ((px ? (H + kResizeY * kResizeRows - 1) / (kResizeY * kResizeRows) : 0) > 65535 ||
      (Ho + kResizeY - 1) / kResizeY > 65535)
    return fail("mhada_image_resize: too many rows");
  const long long need = resize_work_bytes(B, H, W, Ho, Wo);
  if (need && (!work || work_bytes < need))
    return fail("mhada_image_resize: workspace null or too small (mhada_image_resize_work)");

  const hipStream_t s = (hipStream_t)s_;
  const uint8_t* src = (const uint8_t*)frames;
  const ResizeOut last{(uint8_t*)out_u8, out_row_bytes, (long long)Ho * out_row_bytes, out_f32, bgr != 0};
  if (px && py) {
    const ResizeOut mid{(uint8_t*)work, 3LL * Wo, 3LL * H * Wo, nullptr, 0};
    if (int rc = resize_launch<kAlongX, kResizeRows>("mhada_image_resize/horizontal", src, row_bytes, H * row_bytes, W,
                                                     coef_x, bounds_x, ksize_x, B, H, Wo, mid, s))
      return rc;
    return resize_launch<kAlongY, 1>("mhada_image_resize/vertical", mid.u8, mid.row, mid.img, H, coef_y, bounds_y,
                                     ksize_y, B, Ho, Wo, last, s);
  }
  if (px)
    return resize_launch<kAlongX, kResizeRows>("mhada_image_resize/horizontal", src, row_bytes, H * row_bytes, W, coef_x,
                                               bounds_x, ksize_x, B, Ho, Wo, last, s);
  if (py)
    return resize_launch<kAlongY, 1>("mhada_image_resize/vertical", src, row_bytes, H * row_bytes, H, coef_y, bounds_y,
                                     ksize_y, B, Ho, Wo, last, s);
  return resize_launch<kCopy, 1>("mhada_image_resize/copy", src, row_bytes, H * row_bytes, 0, nullptr, nullptr, 0, B,
                                 Ho, Wo, last, s);
}
