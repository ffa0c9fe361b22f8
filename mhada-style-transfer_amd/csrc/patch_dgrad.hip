// Input gradient of the ViT's patch embedding (vit.py:105-117: Conv2d(3, C, 8, stride 8)) with
// respect to the image, fp32 — the last link of a feature inversion's backward (visual_vit.py:88-112,
// visual_mhada.py:111-127 optimise the image through the frozen ViT):
//
//   dimg[b][c][8 py + ky][8 px + kx] = sum_n dy[b][py w + px][n] W[n][64 c + 8 ky + kx]
//
// dy [B][N][C] token rows (N = (H/8)(W/8)), W the conv weight (C, 3, 8, 8) as [C][192] (the k order
// of MHADA_A_PATCH8), dimg NCHW.  A GEMM with M = B N tokens, 192 columns, contraction over C whose
// results land as 8-float patch rows; patches do not overlap, so every pixel has one writer (no
// atomics) and the summation order over C is fixed: repeated calls return the same bits.
//
// Workgroup (4 waves) = a strip of kTok = 16 consecutive tokens of one patch row (b, py): 512^2 B1
// gives 256 workgroups.  dy and W are streamed through LDS in chunks of kKC channels, double
// buffered, the next chunk in flight in registers while this one's MFMAs run.  The products run on
// v_mfma_f32_16x16x4_f32 with the output columns on the accumulator rows and the tokens on the
// lanes: wave v owns columns 48 v .. 48 v + 47 (three independent accumulators), and a lane's four
// accumulator registers are four consecutive kx of one (c, ky) — one 16-byte piece of an image row.
// The accumulators go back through LDS as a [(c, ky)][8 tokens' pixels] tile, so the global stores
// are contiguous image-row segments (512 B per (c, ky) for a full strip).  The workgroups of the
// last patch row also write the zeros of the H % 8 rows below it (the forward ignores those rows).
#include "common.h"

namespace mhada {
namespace {

constexpr int kTok = 16;    // tokens per workgroup
constexpr int kKC = 32;     // channels per LDS chunk
constexpr int kLDW = 196;   // W chunk row (192 floats): 4 rows apart = 16 banks apart (ds_read_b32: 32 banks)
constexpr int kLDD = 36;    // dy chunk row (32 floats), 16-byte aligned, rows on distinct 16-byte slots
constexpr int kLDO = 132;   // output tile row (16 tokens x 8 floats)
constexpr int kWF4 = kKC * 192 / 4 / 256;  // W float4 per thread and chunk

static_assert(kKC * 192 / 4 == kWF4 * 256, "W chunk must divide over the workgroup");
static_assert(kKC * kTok / 4 <= 256, "dy chunk: at most one float4 per thread");
static_assert(24 * kLDO <= 2 * kKC * kLDW, "the output tile reuses the W buffers");

__global__ void __launch_bounds__(256) patch_embed_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                                float* __restrict__ dimg, int C, int H, int W, int hp,
                                                                int wp, int strips) {
  __shared__ __attribute__((aligned(16))) float sW[2][kKC * kLDW];
  __shared__ __attribute__((aligned(16))) float sD[2][kTok * kLDD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bid = blockIdx.x, strip = bid % strips, py = (bid / strips) % hp, b = bid / (strips * hp);
  const int px0 = strip * kTok, ntok = min(kTok, wp - px0);
  // 32-bit element offsets (the host checks B N C and B 3 H W against 2^31)
  const float* dyr = dy + ((b * hp + py) * wp + px0) * C;

  // global -> registers: the W chunk is one contiguous kKC x 192 block; dy rows of tokens >= ntok read 0
  const int dtok = tid >> 3, dk4 = (tid & 7) * 4;
  const bool dlive = tid < kKC * kTok / 4 && dtok < ntok;
  f32x4 rw[kWF4], rd;
  auto fetch = [&](int kc) {
#pragma unroll
    for (int i = 0; i < kWF4; ++i) rw[i] = ld4(w + kc * 192 + 4 * (tid + 256 * i));
    rd = f32x4{0.f, 0.f, 0.f, 0.f};
    if (dlive) rd = ld4(dyr + dtok * C + kc + dk4);
  };
  auto commit = [&](int buf) {
#pragma unroll
    for (int i = 0; i < kWF4; ++i) {
      const int f = tid + 256 * i, row = f / 48, c4 = f - row * 48;
      st4(&sW[buf][row * kLDW + 4 * c4], rw[i]);
    }
    if (tid < kKC * kTok / 4) st4(&sD[buf][dtok * kLDD + dk4], rd);
  };

  // MFMA 16x16x4 f32: lane l gives A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; register r of
  // lane l is D[4 (l >> 4) + r][l & 15].  A = W^T (i: output column), B = dy^T (j: token).  Within a
  // block of 16 channels, lane group g = l >> 4 holds channels 4 g .. 4 g + 3 (one ds_read_b128 of
  // dy) and step e multiplies channel 4 g + e of both operands: a fixed permutation of the k order.
  const int li = lane & 15, g = lane >> 4;
  f32x4 acc[3] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  const int nck = C / kKC;
  fetch(0);
  commit(0);
  __syncthreads();
  for (int ck = 0; ck < nck; ++ck) {
    const int buf = ck & 1;
    if (ck + 1 < nck) fetch((ck + 1) * kKC);
    const float* cw = &sW[buf][4 * g * kLDW + 48 * wave + li];
    const float* cd = &sD[buf][li * kLDD + 4 * g];
#pragma unroll
    for (int kb = 0; kb < kKC; kb += 16) {
      const f32x4 d4 = ld4(cd + kb);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int j = 0; j < 3; ++j)
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(cw[(kb + e) * kLDW + 16 * j], d4[e], acc[j], 0, 0, 0);
    }
    if (ck + 1 < nck) commit(buf ^ 1);
    __syncthreads();
  }

  // accumulators -> LDS tile [(c, ky) = column / 8][8 token + kx]; the loop's last barrier has
  // retired every read of the W buffers
  float* sO = &sW[0][0];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int col = 48 * wave + 16 * j + 4 * g;  // the lane's four columns: col .. col + 3
    st4(&sO[(col >> 3) * kLDO + 8 * li + (col & 7)], acc[j]);
  }
  __syncthreads();
  // 24 image-row segments of 8 ntok floats; the last patch row adds the 3 (H % 8) zero rows below it
  const int rem = py == hp - 1 ? H - 8 * hp : 0;
  const int nf4 = (24 + 3 * rem) * 32;
  for (int f = tid; f < nf4; f += 256) {
    const int r = f >> 5, x4 = f & 31;
    if (x4 >= 2 * ntok) continue;
    int c, y;
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (r < 24) {
      c = r >> 3;
      y = 8 * py + (r & 7);
      v = ld4(&sO[r * kLDO + 4 * x4]);
    } else {
      c = (r - 24) / rem;
      y = 8 * hp + (r - 24) - c * rem;
    }
    st4(dimg + ((b * 3 + c) * H + y) * W + 8 * px0 + 4 * x4, v);
  }
}

}  // namespace
}  // namespace mhada

using namespace mhada;

extern "C" int mhada_patch_embed_dgrad(const float* dy, const float* w, float* dimg, int B, int C, int Ci, int H, int W,
                                       mhada_stream_t s_) {
  if (!dy || !w || !dimg || B <= 0) return fail("mhada_patch_embed_dgrad: bad args");
  if (Ci != 3) return fail("mhada_patch_embed_dgrad: Ci must be 3 (an RGB image)");
  if (C <= 0 || C % 64) return fail("mhada_patch_embed_dgrad: C must be a positive multiple of 64");
  if (H < 8 || W < 8 || W % 8) return fail("mhada_patch_embed_dgrad: H >= 8 and W a positive multiple of 8");
  if (!aligned16(dy) || !aligned16(w) || !aligned16(dimg)) return fail("mhada_patch_embed_dgrad: dy / w / dimg must be 16-byte aligned");
  const int hp = H / 8, wp = W / 8, strips = (wp + kTok - 1) / kTok;
  // 32-bit element offsets in the kernel
  if ((long long)B * hp * wp * C >= (1LL << 31) || (long long)B * 3 * H * W >= (1LL << 31))
    return fail("mhada_patch_embed_dgrad: dy or dimg has 2^31 elements or more");
  const long long nb = (long long)B * hp * strips;
  hipLaunchKernelGGL(patch_embed_dgrad_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)s_, dy, w, dimg, C, H, W,
                     hp, wp, strips);
  return check_launch("mhada_patch_embed_dgrad");
}
