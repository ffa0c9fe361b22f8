// Shared definitions for the MHAda HIP kernels (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

#include "../../include/mhada_hip.h"

typedef __bf16 bf16;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

#define MHADA_DEV __device__ __forceinline__

namespace mhada {

// ---- error reporting (thread-local message, see mhada_last_error) -----------------------
void set_error(const std::string& msg);
int fail(const std::string& msg);  // sets message, returns MHADA_ERR_ARG
int check_launch(const char* what);  // hipGetLastError -> MHADA_ERR_LAUNCH

// ---- kernel-variant selection -------------------------------------------------------------
// The defaults are the measured winners.  The non-default variants exist for A/B measurements
// and for tests that force a rare path (e.g. the online-max bf16 attention).  The values are
// read ONCE, at the first launch, from MHADA_* environment variables, and can be changed only
// through mhada_set_tuning() (include/mhada_hip.h) — never per launch from the environment.
struct Tuning {
  int attn_fixed_shift = 1;  // bf16 softmax attention: fixed-shift kernel (0: online-max kernel)
  int attn_waves = 0;        // attention waves per workgroup: 4 | 8 as set; 0 = 8, or 4 when the 8-wave grid is smaller than the CU count
  int attn_tk = 128;         // bf16 attention keys per tile (64 | 128)
  int attn_prio = 1;         // fixed-shift kernel: s_setprio(1) for the younger wave half
  int vit_attn_vec = 1;      // bf16 batch-axis attention: vectorised form
  int out3_mfma = 1;         // bf16 last decoder layer: MFMA tile kernel (0: per-pixel VALU)
  int out3_tile = 1;         // fp32 last decoder layer: LDS-tiled kernel (0: per-pixel)
  int gemm_pp = 1;           // ping-pong GEMM kernels
  int gemm_persist = 1;      // persistent form of the ping-pong GEMM
  int gemm_pp128 = 1;        // 256x128 persistent ping-pong form for 65..128 columns
  int gemm_ldsepi = 1;       // ping-pong epilogue staged through LDS
  int gemm_n64 = 128;        // N <= 64 tile rows (128 | 256)
  int conv_c64 = 1;          // bf16 64->64 3x3 conv (+ fused upsample): direct tile kernel
  int conv_dir = 1;          // bf16 128->64 / 128->128 / 256->128 3x3 conv: direct tile kernel with a streamed weight ring (round 5)
  int gemm_rinit = 1;        // persistent ping-pong GEMM: residual + bias loaded into the accumulators
  int tn_skinny_lds = 1;     // M <= 4 conv weight gradient: LDS-tiled kernel (0: the gather kernel)
  int wino4 = 1;             // fp32 Winograd conv: 4-wave kernel (round 5; 0: the 8-wave kernel, also the fallback for inputs >= 2 GiB)
  int wino_split3 = 1;       // fp32 Winograd conv, Cin % 16 == 0, with the filters' plane image: SPLIT3 products on the bf16 MFMA (0: wino4 / the 8-wave kernel)
  int wino_s3_rows = 1;      // SPLIT3 Winograd conv: one Winograd row per wave, U from registers, wave-private V (0: wino_s3_kernel; bit-identical)
  int gemm_s3_order = 1;     // SPLIT3 GEMM: terms ordered so each operand plane is staged once per K chunk, separate A / W rings (0: six K-tiles per chunk, both operands staged for each)
  int train_dkv_dma = 1;     // training dK/dV' with the dS spill: LDS-DMA kernel, one wave per SIMD, software-pipelined (0: round 3's)
  int upsample_quad = 1;     // bf16 bilinear x2: 2 x 2-output-block kernel (0: the 16-B per-pixel kernel)
  int xknob = 0;             // scratch knob for one-off A/B builds; no shipped kernel or dispatch reads it
};
const Tuning& tuning();

// conv_tile.hip: bf16 3x3 conv, Cin = Cout = 64, reflect pad, optional fused bilinear x2
// upsample of the input; H, W = output size.  Dispatched from mhada_gemm.
int conv3x3_c64(const void* x, const void* w, const float* bias, void* y, int B, int H, int W, bool up, int relu,
                hipStream_t s);
// conv_tile.hip: bf16 3x3 conv, (Cin, Cout) in {(128, 64), (128, 128), (256, 128)}, reflect pad, no upsample.
int conv3x3_dir(const void* x, const void* w, const float* bias, void* y, int B, int H, int W, int cin, int cout,
                int relu, hipStream_t s);

// attn_hd.hip: the ViT's batch-axis attention at head_dim 32 / 128 (one kernel templated on the width, any
// L).  Dispatched from mhada_vit_batch_attn.
int vit_batch_attn_hd(const void* qkv, void* out, int dtype, int L, int ntok, int heads, int head_dim, hipStream_t s);

// ---- scalar conversions -----------------------------------------------------------------
template <typename T> MHADA_DEV float to_f32(T x);
template <> MHADA_DEV float to_f32<float>(float x) { return x; }
template <> MHADA_DEV float to_f32<bf16>(bf16 x) { return (float)x; }

template <typename T> MHADA_DEV T from_f32(float x);
template <> MHADA_DEV float from_f32<float>(float x) { return x; }
template <> MHADA_DEV bf16 from_f32<bf16>(float x) { return (bf16)x; }

// an fp16 plane value of the HALF2 operands (ops._half2_planes' arithmetic, shared by every plane writer):
// round to nearest, a subnormal result flushed to zero (the HALF2 GEMM does not rely on the MFMA keeping
// fp16 subnormals)
MHADA_DEV _Float16 half2_plane(float v) {
  const _Float16 q = (_Float16)v;
  return fabsf((float)q) < 6.103515625e-05f ? (_Float16)0.0f : q;
}

// the three bf16 planes of the SPLIT3 operands, x = a + b + c (ops.split3_weight's arithmetic, shared by
// every plane writer): a = bf16(x), b = bf16(x - a), c = bf16(x - a - b), each round to nearest.  This is
// THE split: every SPLIT3 product assumes that every writer of planes rounds exactly this way.
struct Bf3 { bf16 a, b, c; };
MHADA_DEV Bf3 split3(float x) {
  const bf16 a = (bf16)x;
  const float r = x - (float)a;
  const bf16 b = (bf16)r;
  return Bf3{a, b, (bf16)(r - (float)b)};
}
// element e of three plane vectors
template <typename V>
MHADA_DEV void split3_into(float x, V& a, V& b, V& c, int e) {
  const Bf3 s = split3(x);
  a[e] = s.a;
  b[e] = s.b;
  c[e] = s.c;
}

// 16-byte vector of T: 4 f32 or 8 bf16
template <typename T> struct Vec16;
template <> struct Vec16<float> { typedef f32x4 type; static constexpr int N = 4; };
template <> struct Vec16<bf16> { typedef bf16x8 type; static constexpr int N = 8; };

// Bilinear blend in PyTorch's order, h0 * (w0 * x00 + w1 * x01) + h1 * (w0 * x10 + w1 * x11), with the
// fp32 contraction pinned (explicit fmaf), so every kernel that upsamples — the standalone
// upsample kernels, the conv tile kernel's fused halo and the implicit GEMM's UP2 gather —
// produces the same bits.
MHADA_DEV float bilerp(float ly0, float ly1, float lx0, float lx1, float x00, float x01, float x10, float x11) {
  return fmaf(ly1, fmaf(lx0, x10, lx1 * x11), ly0 * fmaf(lx0, x00, lx1 * x01));
}

// ---- u8 frame output (mhada_frame_emit and the u8 form of the last decoder layer) ---------
// clamp(0, 255) then numpy's astype(uint8) (truncation toward zero); NaN -> 0 (fmaxf returns the
// non-NaN operand).
MHADA_DEV uint32_t emit_u8(float v) { return (uint32_t)fminf(fmaxf(v, 0.f), 255.f); }

// the three bytes of one pixel in memory order (byte 0 lowest): B,G,R for bgr, else R,G,B
MHADA_DEV uint32_t emit_pack(float r, float g, float b, int bgr) {
  const uint32_t c0 = emit_u8(bgr ? b : r), c1 = emit_u8(g), c2 = emit_u8(bgr ? r : b);
  return c0 | (c1 << 8) | (c2 << 16);
}

// Store one packed pixel per lane.  Called by every lane of the wave, `valid` or not.  `q` = the lane's
// position in its group of four consecutive lanes, which hold four consecutive pixels of one row
// when `quad` is set (the same value in all four lanes; implies valid): the 12 bytes then leave as
// three dword stores from lanes q = 0..2 if the group's first byte is 4-byte aligned.  Everything
// else (row ends, groups that straddle two rows, misaligned rows) is three byte stores per pixel.
MHADA_DEV void emit_store_px(uint8_t* p, uint32_t px, int q, bool valid, bool quad) {
  const uint32_t nx = (uint32_t)__shfl_down((int)px, 1, 64);
  if (quad && ((uintptr_t)(p - 3 * q) & 3) == 0) {
    // dword q of the group: bytes 4q .. 4q+3 = the upper 3 - q bytes of this pixel, then the next one's
    if (q < 3) *reinterpret_cast<uint32_t*>(p + q) = q == 0 ? (px | (nx << 24)) : ((px >> (8 * q)) | (nx << (24 - 8 * q)));
  } else if (valid) {
    p[0] = (uint8_t)px;
    p[1] = (uint8_t)(px >> 8);
    p[2] = (uint8_t)(px >> 16);
  }
}

MHADA_DEV float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
MHADA_DEV float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// ---- MFMA, LDS and addressing helpers -----------------------------------------------------
// Row of register r (0..15) of a 32x32 MFMA accumulator in lane half h (lane >> 5); the column is lane & 31.
MHADA_DEV int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

MHADA_DEV f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
MHADA_DEV void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// Workgroup barrier for an LDS hand-off only: __syncthreads() also acts as a release fence that drains
// every outstanding global store (vmcnt counts stores on CDNA4), which would serialise a kernel's
// stores with its next tile.
MHADA_DEV void lds_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

// LDS-DMA (global_load_lds), 16 B per lane: lane l's 16 bytes at src land at lds + 16 l
MHADA_DEV void glds16(const void* src, void* lds) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                   (__attribute__((address_space(3))) void*)lds, 16, 0, 0);
}

// reflect padding of index i into [0, n): one fold (|overhang| < n), and the same clamped for tile halos
// that reach further out than one fold covers
MHADA_DEV int reflect1(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }
MHADA_DEV int reflect_clamp(int v, int n) {
  v = v < 0 ? -v : (v >= n ? 2 * n - 2 - v : v);
  return min(max(v, 0), n - 1);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// compute units of the current device (abi.hip): queried once per process, 256 if the query fails
int num_cus();

// Form routing for chunked calls (abi.hip, mhada_set_route): the dispatch rules that choose a kernel form from
// the rows or the batch of a call (the fp32 GEMM's tile-fill rule, the attention's waves per block) evaluate
// routed(x) = x * mul / div, so that a chunk of div frames takes the forms a whole clip of mul frames takes
// and a frame's bits do not depend on the chunking.  Off (mul = div = 0, the default): routed(x) = x.
long long routed(long long x);

// Bijective XCD-aware block remap (cdna_hip_programming.md §5 "XCD swizzle must be
// bijective"): blocks b, b+8, b+16 ... are dealt to one XCD; give each XCD a contiguous
// range of logical ids so neighbouring tiles (which share operands) share its L2.
MHADA_DEV int xcd_remap(int bid, int nblk) {
  const int q = nblk / 8, r = nblk % 8;
  const int xcd = bid % 8, k = bid / 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + k;
}

}  // namespace mhada
