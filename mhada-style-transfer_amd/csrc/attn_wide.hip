// Single-head AdaAttN attention at head width 512 (AdaAttN / AdaAttnTransformer, MHAdaSTr/network/
// adaDecoder.py:85-131, 209-232) on v_mfma_f32_32x32x16_bf16: mhada_attn_wide.
//
//   A = softmax(Q K^T), M = A V', E2 = A V'^2,
//   out = sqrt(max(E2 - M^2, 1e-6)) * (fcs - mu) * rstd + M + v_mu            (A never in HBM)
//
// attn.hip / attn_hd.hip keep one query's whole M | E2 row (2 D fp32) in one wave's accumulators; at
// D = 512 that is 1024 registers.  This kernel keeps loss_attn.hip's answer to that shape: the waves of a
// workgroup split the WORK of one query tile, not its queries.  Workgroup = 8 waves = 64 queries of one
// image: wave = (qg, ws), qg = query half of 32 (lane & 31 = query, lane >> 5 = h selects the reduction
// half), ws = one of 4 slices of 128 channels.  Per 32-key tile:
//   * Q K^T split over d: wave (qg, ws) forms the partial S^T (keys x queries) over d in [128 ws, 128 ws +
//     128) — 8 MFMAs, its Q slice 8 bf16x8 registers, the K operand 16-B reads along the key rows of
//     sK[32][520] (rows padded by 16 B: conflict-free) — and writes it to sS[qg][ws] (fp32);
//   * barrier; every wave sums the 4 partials of its query half in the fixed order ws = 0, 1, 2, 3, so the
//     4 waves of a query half hold the identical score tile and take the identical online-softmax step
//     (fp32, log2 units: Q carries log2 e; lazy rescale kWideRescaleThr as attn.hip / loss_attn.hip);
//   * P V' split over d_v: wave (qg, ws) owns columns [128 ws, 128 ws + 128) of M and of E2 (8 f32x16
//     accumulators = 128 registers), P^T is the score accumulator itself rounded to bf16 (the B operand,
//     no lane movement), the A operand one 16-B read of sVt[512][40] = V'^T, and V'^2 the fp32 square of
//     that fragment rounded once in the register: 16 MFMAs.
// K and V' tiles are staged once per workgroup: 16-B global loads issued one tile ahead into registers, K
// committed row-major, V' transposed on its way into LDS with the keys of each group of 16 at position
// pos(n) = n with bits 2 and 3 swapped (attn_hd.hip's layout: the 8 keys 16 s + 8 (j >> 2) + 4 h + (j & 3)
// of one lane half's B slots are one 16-B read at 16 s + 8 h).  Single-buffered sK / sVt / sS, two barriers
// per tile (loss_attn_lds_kernel's schedule).  LDS: 33 280 (sK) + 40 960 (sVt) + 32 768 (sS) = 107 008 B,
// one workgroup per CU.  Keys past Ns are staged as zeros and their scores masked to -inf; queries past Nc
// read row Nc - 1 and store nothing.  No atomics, fixed summation order: bit-identical from run to run.
#include "common.h"

namespace mhada {
namespace wide {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr int D = 512;                  // the head width (= channels)
constexpr int TK = 32;                  // keys per tile
constexpr int LK = D + 8;               // sK row, bf16
constexpr int LV = TK + 8;              // sVt row, bf16
constexpr int NT = 512;                 // threads
constexpr int kMaxNs = 1 << 20;         // a tile's buffer resource spans (Ns - key0) * 1024 B as a 32-bit size
constexpr float kWideRescaleThr = 32.0f;  // log2 units, as attn.hip

struct WideP {
  const bf16* q;    // [B][Nc][512], log2 units
  const bf16* k;    // [B][Ns][512]
  const bf16* v;    // [B][Ns][512]  V' (centred, no bias)
  const float* fcs; // [B][Nc][512]
  const float* fcs_mu;
  const float* fcs_rstd;
  const float* v_mu;
  float* out;       // [B][Nc][512]
  bf16* out16;      // optional bf16 copy
  int Nc, Ns, nqb;
};

__global__ void __launch_bounds__(NT) attn_wide_kernel(const WideP p) {
  __shared__ __attribute__((aligned(16))) bf16 sK[TK * LK];
  __shared__ __attribute__((aligned(16))) bf16 sVt[D * LV];
  __shared__ __attribute__((aligned(16))) float sS[2][4][16][64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qg = wave >> 2, ws = wave & 3;
  const int h = lane >> 5, r32 = lane & 31;
  const int t0 = xcd_remap(blockIdx.x, gridDim.x);
  const int b = t0 / p.nqb, qb = t0 - b * p.nqb;
  const int q = qb * 64 + qg * 32 + r32;
  const int qc = min(q, p.Nc - 1);

  // Q^T operand of this wave's d slice: k-step s takes d = 128 ws + 16 s + 8 h + j
  bf16x8 qf[8];
  {
    const bf16* qp = p.q + ((long long)b * p.Nc + qc) * D + 128 * ws + 8 * h;
#pragma unroll
    for (int s = 0; s < 8; ++s) qf[s] = *reinterpret_cast<const bf16x8*>(qp + 16 * s);
  }
  const bf16* kb = p.k + (long long)b * p.Ns * D;
  const bf16* vb = p.v + (long long)b * p.Ns * D;

  // tile staging: K = 32 rows x 64 16-B chunks (4 per thread, coalesced along the rows); V' = 16 key
  // pairs x 64 chunks of 8 dv (2 units per thread, each the same 8 dv of two adjacent keys)
  // Loads through buffer resources built per tile over the key rows key0 .. Ns - 1 (scalar work): every
  // lane's byte offset is a loop constant and rows past Ns read 0 with no branch (their scores are masked).
  bf16x8 rk[4], rv[2][2];
  const int kvo = ((tid >> 6) * D + (tid & 63) * 8) * 2;          // chunk tid + NT i: 8 rows further
  const int vvo = (2 * (tid & 15) * D + (tid >> 4) * 8) * 2;      // unit tid + NT i: 256 columns further
  auto issue = [&](int key0) {  // key0 < Ns
    const int bytes = (p.Ns - key0) * D * 2;  // Ns <= kMaxNs: fits
    const __amdgpu_buffer_rsrc_t kr =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(kb + (long long)key0 * D), 0, bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t vr =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(vb + (long long)key0 * D), 0, bytes, 0x00020000);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      rk[i] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(kr, kvo + i * 8 * D * 2, 0, 0));
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      rv[i][0] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(vr, vvo + i * 512, 0, 0));
      rv[i][1] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(vr, vvo + i * 512 + D * 2, 0, 0));
    }
  };
  auto commit_k = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = tid + NT * i;
      *reinterpret_cast<bf16x8*>(sK + (c >> 6) * LK + (c & 63) * 8) = rk[i];
    }
  };
  auto commit_v = [&]() {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int u = tid + NT * i, n = 2 * (u & 15), col = (u >> 4) * 8;
      const int pos = (n & ~12) | ((n & 4) << 1) | ((n & 8) >> 1);  // bits 2 and 3 swapped
#pragma unroll
      for (int e = 0; e < 8; ++e)
        *reinterpret_cast<bf16x2*>(sVt + (col + e) * LV + pos) = bf16x2{rv[i][0][e], rv[i][1][e]};
    }
  };

  f32x16 O[8];  // O[j]: sum p v' for dv = 128 ws + 32 j + (r & 3) + 8 (r >> 2) + 4 h; O[4 + j]: sum p v'^2
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) O[i][e] = 0.f;
  float m2 = -INFINITY, l = 0.f;

  const int ntile = (p.Ns + TK - 1) / TK;
  issue(0);
  commit_k();
  __syncthreads();
  for (int tt = 0; tt < ntile; ++tt) {
    const int key0 = tt * TK;
    commit_v();  // V'(tt): sVt's readers (P V' of tile tt - 1) passed the last barrier
    issue(min(tt + 1, ntile - 1) * TK);
    // ---- partial S^T[key][q] over this wave's d slice
    f32x16 S;
#pragma unroll
    for (int e = 0; e < 16; ++e) S[e] = 0.f;
    {
      const bf16* krow = sK + r32 * LK + 128 * ws + 8 * h;
#pragma unroll
      for (int s = 0; s < 8; ++s)
        S = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(krow + 16 * s), qf[s], S, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) sS[qg][ws][r][lane] = S[r];
    __syncthreads();
    // ---- full scores: fixed-order sum of the 4 partials (identical in the 4 waves of a query half)
    // (four registers at a time: the 64 reads hoisted together would cost 64 registers the wave lacks)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma unroll
      for (int r = 4 * g; r < 4 * g + 4; ++r)
        S[r] = ((sS[qg][0][r][lane] + sS[qg][1][r][lane]) + sS[qg][2][r][lane]) + sS[qg][3][r][lane];
      __builtin_amdgcn_sched_barrier(0);
    }
    // keys past Ns: -inf.  Unconditional (one compare and select per score against constants): a branch for
    // the tail tile makes a second copy of the loop body, and that copy does not fit the register file
    const int nvalid = p.Ns - key0 - 4 * h;
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      S[r] = acc_row(r, 0) < nvalid ? S[r] : -INFINITY;
      mx = fmaxf(mx, S[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    // per-lane (query) decision, O columns are per query; the first tile always takes it (m2 = -inf and
    // mx is finite: tile 0 holds at least one key)
    if (mx > m2 + kWideRescaleThr) {
      const float mn = fmaxf(m2, mx);
      const float alpha = m2 == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m2 - mn);
      l *= alpha;
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) O[i][e] *= alpha;
      m2 = mn;
    }
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      S[r] = __builtin_amdgcn_exp2f(S[r] - m2);
      sum += S[r];
    }
    l += sum;
    // ---- O^T[dv][q] += V'^T P^T and (V'^2)^T P^T over the 32 keys
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      // B = P^T: element j <-> key 16 s + 8 (j >> 2) + 4 h + (j & 3) (accumulator regs 8 s .. 8 s + 7),
      // stored contiguously at key position 16 s + 8 h of the V'^T rows
      bf16x8 pf;
#pragma unroll
      for (int j = 0; j < 8; ++j) pf[j] = (bf16)S[8 * s + j];
      const bf16* vcol = sVt + (128 * ws + r32) * LV + 16 * s + 8 * h;
      // one fragment read ahead of the MFMAs, pinned: every fragment hoisted at once would cost 64 registers
      bf16x8 vn = *reinterpret_cast<const bf16x8*>(vcol);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bf16x8 vf = vn;
        if (j < 3) vn = *reinterpret_cast<const bf16x8*>(vcol + 32 * (j + 1) * LV);
        __builtin_amdgcn_sched_barrier(0);
        bf16x8 v2;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float f = (float)vf[e];
          v2[e] = (bf16)(f * f);
        }
        O[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, O[j], 0, 0, 0);
        O[4 + j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v2, pf, O[4 + j], 0, 0, 0);
      }
    }
    commit_k();  // K(tt + 1): every wave's S^T reads of sK ended before the barrier above
    __syncthreads();
  }

  // ---- epilogue: out[q][dv] = sqrt(max(E2 - M^2, 1e-6)) * (fcs - mu) * rstd + M + v_mu
  const float lt = l + __shfl_xor(l, 32, 64);
  if (q >= p.Nc) return;
  const float inv = 1.0f / lt;
  const int dvb = 128 * ws;
  const long long row = ((long long)b * p.Nc + q) * D + dvb;
  const float* fr = p.fcs + row;
  const float* mu = p.fcs_mu + (long long)b * D + dvb;
  const float* rs = p.fcs_rstd + (long long)b * D + dvb;
  const float* vm = p.v_mu + (long long)b * D + dvb;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int dv = 32 * j + 8 * g + 4 * h;
      const f32x4 f = *reinterpret_cast<const f32x4*>(fr + dv);
      const f32x4 m4 = *reinterpret_cast<const f32x4*>(mu + dv);
      const f32x4 r4 = *reinterpret_cast<const f32x4*>(rs + dv);
      const f32x4 v4 = *reinterpret_cast<const f32x4*>(vm + dv);
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float m1 = O[j][4 * g + e] * inv;
        const float e2 = O[4 + j][4 * g + e] * inv;
        o[e] = sqrtf(fmaxf(e2 - m1 * m1, 1e-6f)) * ((f[e] - m4[e]) * r4[e]) + (m1 + v4[e]);
      }
      *reinterpret_cast<f32x4*>(p.out + row + dv) = o;
      if (p.out16) *reinterpret_cast<bf16x4*>(p.out16 + row + dv) = bf16x4{(bf16)o[0], (bf16)o[1], (bf16)o[2], (bf16)o[3]};
    }
}

}  // namespace wide
}  // namespace mhada

using namespace mhada;

extern "C" int mhada_attn_wide(const void* q, const void* k, const void* v, const float* fcs, const float* fcs_mu,
                               const float* fcs_rstd, const float* v_mu, float* out, void* out16, int dtype, int B,
                               int Nc, int Ns, int D, mhada_stream_t s_) {
  if (!q || !k || !v || !fcs || !fcs_mu || !fcs_rstd || !v_mu || !out) return fail("mhada_attn_wide: null pointer");
  if (B <= 0 || Nc <= 0 || Ns <= 0) return fail("mhada_attn_wide: B, Nc, Ns must be positive");
  if (Ns > wide::kMaxNs) return fail("mhada_attn_wide: Ns must be at most 2^20 (32-bit buffer offsets)");
  if (D != wide::D) return fail("mhada_attn_wide: the head width must be 512");
  if (dtype != MHADA_BF16) return fail("mhada_attn_wide: q, k, v must be MHADA_BF16");
  for (const void* ptr : {q, k, v, (const void*)fcs, (const void*)fcs_mu, (const void*)fcs_rstd, (const void*)v_mu,
                          (const void*)out, (const void*)out16})
    if ((uintptr_t)ptr & 15) return fail("mhada_attn_wide: pointers must be 16-byte aligned");
  wide::WideP p;
  p.q = (const bf16*)q; p.k = (const bf16*)k; p.v = (const bf16*)v;
  p.fcs = fcs; p.fcs_mu = fcs_mu; p.fcs_rstd = fcs_rstd; p.v_mu = v_mu;
  p.out = out; p.out16 = (bf16*)out16;
  p.Nc = Nc; p.Ns = Ns;
  p.nqb = (Nc + 63) / 64;
  const long long nblk = (long long)B * p.nqb;
  if (nblk >= (1LL << 31)) return fail("mhada_attn_wide: grid too large");
  hipLaunchKernelGGL(wide::attn_wide_kernel, dim3((unsigned)nblk), dim3(wide::NT), 0, (hipStream_t)s_, p);
  return check_launch("mhada_attn_wide");
}
