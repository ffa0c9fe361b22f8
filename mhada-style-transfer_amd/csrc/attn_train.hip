// MHAda attention for the training path at head widths D = 32 | 64 | 128 (16-, 8- and 4-head models
// at 512 channels): forward that keeps the softmax statistics, and the backward (dual accumulator
// M / E2), one kernel family templated on D, fp32 on v_mfma_f32_32x32x2_f32.
//
// Reference: AdaAttnMultiHead.forward (MHAdaSTr/network/adaDecoder.py:186-198) under
// train_image.py:93-144 autograd.  Per (batch, head), with Q [Nc][D], K [Ns][D], V' [Ns][D]
// (V' = V - mean_tokens(V), centred by the caller under autograd: the variance is
// shift-invariant and d(out)/dV = d(out)/dV' exactly, since the rows of A sum to one) and
// X = InstanceNorm(fcs) [Nc][D]:
//   A = softmax(Q K^T)   M' = A V'   E2' = A V'^2   var = E2' - M'^2
//   out' = sqrt(max(var, 1e-6)) * X + M'            (the caller adds mean(V) back)
// (no 1/sqrt(d) factor).  The forward writes out', mo = [M' | E2'] ([Nc][2D]) and the log2 row
// normaliser lse2 = max + log2(sum).
// The caller turns d(out') into dmo = [dM' | dE2'] and D_row = dM'.M' + dE2'.E2' (elementwise,
// O(Nc*D): mhada_attn_train_bwd_prep / _hd); then with P = A (recomputed from lse2) and
// dA = dM'.V'^T + dE2'.(V'^2)^T:
//   dS = P * (dA - D_row)        (gradient of the natural-unit logits)
//   dQ = dS K       dK = dS^T Q       dV' = P^T dM' + 2 V' * (P^T dE2')
// as two deterministic kernels (no atomics): key-stationary dK/dV', query-stationary dQ, each
// recomputing P — the Nc x Ns matrices never reach HBM (the reference autograd keeps A, the
// softmax output, and their gradients: 4 B x Nc x Ns per head each).
//
// The kernels stage 32-row LDS tiles through registers (two buffers, one barrier per tile).  At
// 64 only, the dK/dV' kernel can also spill dS (dQ = dS K then runs as a GEMM), in this form or in
// the LDS-DMA form below (the training default); the SPLIT3 and vt forwards (attn_split3.hip,
// attn.hip) exist at 64 only too.
//
// MFMA 32x32x2 f32 layout (cdna_hip_programming.md §3): lane l gives A[l%32][l/32] and
// B[l/32][l%32]; accumulator register r of lane l is D[acc_row(r, l/32)][l%32].  Every
// product is arranged so that one operand is an accumulator of the previous product
// (accumulator-as-operand), so no score or probability ever moves between lanes.  A product over
// D k-indices is D/2 instructions: lane half h supplies the indices (D/2) h + s.
//
// Registers and LDS per workgroup of 4 waves (128 queries or keys); DESIGN.md §3b has the
// compiler's figures:
//   D = 32:  two waves per SIMD everywhere (accumulators: fwd 2 blocks, dQ 1, dK/dV' 3).
//   D = 64:  fwd and dQ two waves per SIMD; dK/dV' one: 288 registers, no spills (two waves per
//            SIMD at 256 registers spilled 18 and measured the same, tools/train_attn_bench.py).
//   D = 128: one wave per SIMD.  fwd: 8 accumulator blocks (128 registers) + the query row (64);
//            dQ: Q, dM', dE2' rows (192) + 4 blocks; dK/dV': K, V' rows (128; V'^2 is squared at
//            the operand, not kept) + dK, P^T dM', P^T dE2' (12 blocks, 192 registers); its Q
//            (16.5 KiB) and dmo (32.5 KiB) tiles double-buffered take 98 KiB of LDS.
#include "common.h"

#include <type_traits>

#include <stdlib.h>

namespace mhada {
namespace {

constexpr float kLog2e = 1.4426950408889634f;
constexpr int TT = 32;    // keys (fwd, dQ) or queries (dK/dV') staged per LDS tile
constexpr int kNT = 256;  // threads per workgroup: 4 waves of 32 lane columns, so
constexpr int kRowsWG = 128;  // queries (fwd, dQ) or keys (dK/dV') per workgroup

// The per-width decisions.  Minimum waves per SIMD handed to the register allocator (the second
// launch bound; 0 = none given, the 64-wide forward and dQ):
enum Kind { FWD, DQ, DKV };
constexpr int min_waves(int D, Kind kind) { return D == 32 ? 2 : D == 128 ? 1 : kind == DKV ? 1 : 0; }
// dK/dV': V'^2 of the wave's keys kept in registers, or (the budget at 128) squared at the operand
constexpr bool keep_v2(int D) { return D <= 64; }

MHADA_DEV f32x16 mfma(float a, float b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

struct TrainP {
  const float* q;    // [BH][Nc][D]
  const float* k;    // [BH][Ns][D]
  const float* v;    // [BH][Ns][D] centred V'
  const float* x;    // [BH][Nc][D] InstanceNorm(fcs)
  float* out;        // [BH][Nc][D]
  float* mo;         // [BH][Nc][2D]  M' | E2'
  float* lse;        // [BH][Nc]      log2 units
  const float* dmo;  // [BH][Nc][2D]  dM' | dE2'
  const float* dd;   // [BH][Nc]      D_row
  float* dq;         // [BH][Nc][D]
  float* dk;         // [BH][Ns][D]
  float* dv;         // [BH][Ns][D]
  float* ds;         // [BH][Nc][Ns] dS spill (dQ = dS K as a GEMM; D = 64), or null
  int Nc, Ns, nb, nblk;  // nb = row blocks per (b, h)
};

// In-kernel clock of the dK/dV' kernel, diagnostic builds only (-DATTN_CLOCK, tools/attn_clock.py
// dkv): thread 0 of each workgroup stamps the shader clock and the 100 MHz counter around the
// query loop into a buffer of its own (MI355X_MICROARCH.md, DVFS give-back item 6).
#ifdef ATTN_CLOCK
constexpr int kTrainClockBlocks = 65536;
__device__ unsigned long long g_train_clock[4 * kTrainClockBlocks];
#define TRAIN_STAMP(slot)                                                                    \
  do {                                                                                       \
    if (threadIdx.x == 0 && blockIdx.x < kTrainClockBlocks) {                                \
      const unsigned long long c_ = __builtin_amdgcn_s_memtime();                           \
      const unsigned long long r_ = __builtin_amdgcn_s_memrealtime();                       \
      g_train_clock[4 * blockIdx.x + 2 * (slot)] = c_;                                       \
      g_train_clock[4 * blockIdx.x + 2 * (slot) + 1] = r_;                                   \
    }                                                                                        \
  } while (0)
#else
#define TRAIN_STAMP(slot) \
  do {                    \
  } while (0)
#endif

// Register-staged copy of rows [r0, r0+TT) of a [n][W] matrix (zero rows past n; with CLAMP, r0
// may lie past n) into an LDS tile of rows padded to W + 4 floats (row reads by ds_read_b128 and
// column reads by ds_read_b32 are both conflict-free: W + 4 = 4 mod 32): load() issues the global
// reads one tile ahead, store() writes them after the current tile's math (one barrier per tile,
// two LDS buffers).  Row offsets are 64-bit.
template <int W, bool CLAMP = false>
struct Stager {
  static constexpr int NT = kNT;
  static constexpr int CPR = W / 4;        // 16-B chunks per row
  static constexpr int N = TT * CPR / NT;  // chunks per thread
  static constexpr int LD = W + 4;
  static_assert(N * NT == TT * CPR, "tile must divide evenly");
  f32x4 r[N];
  MHADA_DEV void load(const float* g, int r0, int n, int tid) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int c = tid + NT * i, row = c / CPR, col = (c % CPR) * 4, gr = r0 + row;
      if constexpr (CLAMP) {
        // unconditional load of a clamped row, zeroed afterwards: a branch around the load makes
        // the wait-count pass drain every outstanding store before the tile's LDS write
        const f32x4 x = ld4(g + (long long)min(gr, n - 1) * W + col);
        r[i] = gr < n ? x : f32x4{0.f, 0.f, 0.f, 0.f};
      } else {
        r[i] = gr < n ? ld4(g + (long long)gr * W + col) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
  }
  MHADA_DEV void store(float* s, int tid) const {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int c = tid + NT * i, row = c / CPR, col = (c % CPR) * 4;
      st4(s + row * LD + col, r[i]);
    }
  }
};

// The lane's half of a row of D = 2 HD floats: reg[s] = g[row][HD h + s] * scale (zeros if !valid).
template <int HD>
MHADA_DEV void load_half_row(float (&reg)[HD], const float* g, int row, bool valid, int h, float scale) {
  const float* p = g + (long long)(valid ? row : 0) * (2 * HD) + HD * h;
#pragma unroll
  for (int i = 0; i < HD / 4; ++i) {
    const f32x4 t = ld4(p + 4 * i);
#pragma unroll
    for (int e = 0; e < 4; ++e) reg[4 * i + e] = valid ? t[e] * scale : 0.f;
  }
}

// S^T (keys x queries) in log2 units from the staged K tile and the lane's query row
// (qr pre-scaled by log2 e); keys past Ns masked to -inf.
template <int HD>
MHADA_DEV f32x16 scores_t(const float* sK, const float (&qr)[HD], int k0, int Ns, int h, int r32) {
  f32x16 S = {};
  const float* kr = sK + r32 * (2 * HD + 4) + HD * h;
#pragma unroll
  for (int i = 0; i < HD / 4; ++i) {
    const f32x4 kk = ld4(kr + 4 * i);
#pragma unroll
    for (int e = 0; e < 4; ++e) S = mfma(kk[e], qr[4 * i + e], S);
  }
  if (k0 + TT > Ns) {
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (k0 + acc_row(r, h) >= Ns) S[r] = -INFINITY;
  }
  return S;
}

// accumulator blocks b = 0 .. DB-1 of a lane hold columns 32 b + 8 g + 4 h + e in register 4 g + e
template <int DB>
MHADA_DEV void store_blocks(float* row, const f32x16 (&A)[DB], int h) {
#pragma unroll
  for (int b = 0; b < DB; ++b)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      st4(row + 32 * b + 8 * g + 4 * h, f32x4{A[b][4 * g], A[b][4 * g + 1], A[b][4 * g + 2], A[b][4 * g + 3]});
}

// dK/dV' epilogue of the lane's key row (vg, dvr, dkr: its rows of V', dV', dK):
// dV' = G1 + 2 V' G2 with G1 = P^T dM', G2 = P^T dE2'.
template <int DB>
MHADA_DEV void store_dkv(const float* vg, float* dvr, float* dkr, int h, const f32x16 (&G1)[DB],
                         const f32x16 (&G2)[DB], const f32x16 (&dK)[DB]) {
#pragma unroll
  for (int cb = 0; cb < DB; ++cb)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int c0 = 32 * cb + 8 * g + 4 * h;
      const f32x4 vv = ld4(vg + c0);
      f32x4 a, b;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        a[e] = G1[cb][4 * g + e] + 2.0f * vv[e] * G2[cb][4 * g + e];
        b[e] = dK[cb][4 * g + e];
      }
      st4(dvr + c0, a);
      st4(dkr + c0, b);
    }
}

// ---------------------------------------------------------------------------------------
// forward: wave = 32 queries (one per lane column), online softmax over 32-key tiles
// ---------------------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(kNT, min_waves(D, FWD)) attn_train_fwd_kernel(const TrainP p) {
  constexpr int DB = D / 32, LD = D + 4;
  __shared__ __attribute__((aligned(16))) float sK[2][TT * LD];
  __shared__ __attribute__((aligned(16))) float sV[2][TT * LD];
  const int t0 = xcd_remap(blockIdx.x, p.nblk);
  const long long bh = t0 / p.nb;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, r32 = lane & 31;
  const int q = (t0 % p.nb) * kRowsWG + wave * 32 + r32;
  const bool qv = q < p.Nc;
  float qr[D / 2];
  load_half_row(qr, p.q + bh * p.Nc * D, q, qv, h, kLog2e);
  const float* kb = p.k + bh * p.Ns * D;
  const float* vb = p.v + bh * p.Ns * D;

  f32x16 O[2 * DB];  // blocks 0 .. DB-1: sum p v', DB .. 2 DB-1: sum p v'^2
#pragma unroll
  for (int i = 0; i < 2 * DB; ++i) O[i] = f32x16{};
  float m = -INFINITY, l = 0.f;
  Stager<D> gk, gv;
  gk.load(kb, 0, p.Ns, tid);
  gv.load(vb, 0, p.Ns, tid);
  gk.store(sK[0], tid);
  gv.store(sV[0], tid);
  __syncthreads();
  const int nt = (p.Ns + TT - 1) / TT;
  for (int t = 0; t < nt; ++t) {
    const int k0 = t * TT, cb = t & 1;
    const bool nxt = t + 1 < nt;
    if (nxt) {
      gk.load(kb, k0 + TT, p.Ns, tid);
      gv.load(vb, k0 + TT, p.Ns, tid);
    }
    f32x16 S = scores_t(sK[cb], qr, k0, p.Ns, h, r32);
    float mx = S[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, S[r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    if (__any(mx > m)) {  // exact online softmax: rescale whenever the running max moves
      const float mn = fmaxf(m, mx);
      const float alpha = __builtin_amdgcn_exp2f(m - mn);
      l *= alpha;
#pragma unroll
      for (int i = 0; i < 2 * DB; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) O[i][e] *= alpha;
      m = mn;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      S[r] = __builtin_amdgcn_exp2f(S[r] - m);
      l += S[r];
    }
    // O^T (c x queries) += V'^T (c x keys) . P^T (keys x queries); the upper blocks take V'^2
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float* vr = sV[cb] + acc_row(r, h) * LD + r32;
#pragma unroll
      for (int b = 0; b < DB; ++b) {
        const float vv = vr[32 * b];
        O[b] = mfma(vv, S[r], O[b]);
        O[DB + b] = mfma(vv * vv, S[r], O[DB + b]);
      }
    }
    if (nxt) {
      gk.store(sK[cb ^ 1], tid);
      gv.store(sV[cb ^ 1], tid);
    }
    __syncthreads();
  }
  l += __shfl_xor(l, 32, 64);
  if (!qv) return;
  const float inv = 1.0f / l;
  const long long row = bh * p.Nc + q;
  const float* xr = p.x + row * D;
  float* orow = p.out + row * D;
  float* mrow = p.mo + row * 2 * D;
#pragma unroll
  for (int b = 0; b < DB; ++b)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int c0 = 32 * b + 8 * g + 4 * h;
      const f32x4 xx = ld4(xr + c0);
      f32x4 o, mm, ee;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float m1 = O[b][4 * g + e] * inv;
        const float e2 = O[DB + b][4 * g + e] * inv;
        o[e] = sqrtf(fmaxf(e2 - m1 * m1, 1e-6f)) * xx[e] + m1;
        mm[e] = m1;
        ee[e] = e2;
      }
      st4(orow + c0, o);
      st4(mrow + c0, mm);
      st4(mrow + D + c0, ee);
    }
  if (h == 0) p.lse[row] = m + __log2f(l);
}

// ---------------------------------------------------------------------------------------
// dQ: wave = 32 queries; streams 32-key tiles of K, V'
// ---------------------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(kNT, min_waves(D, DQ)) attn_train_dq_kernel(const TrainP p) {
  constexpr int DB = D / 32, HD = D / 2, LD = D + 4;
  __shared__ __attribute__((aligned(16))) float sK[2][TT * LD];
  __shared__ __attribute__((aligned(16))) float sV[2][TT * LD];
  const int t0 = xcd_remap(blockIdx.x, p.nblk);
  const long long bh = t0 / p.nb;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, r32 = lane & 31;
  const int q = (t0 % p.nb) * kRowsWG + wave * 32 + r32;
  const bool qv = q < p.Nc;
  const long long row = bh * p.Nc + (qv ? q : 0);
  float qr[HD], dm[HD], de[HD];
  load_half_row(qr, p.q + bh * p.Nc * D, q, qv, h, kLog2e);
  load_half_row(dm, p.dmo + bh * p.Nc * 2 * D, 2 * q, qv, h, 1.0f);      // row q of [Nc][2D], first half
  load_half_row(de, p.dmo + bh * p.Nc * 2 * D + D, 2 * q, qv, h, 1.0f);  // second half
  const float L = qv ? p.lse[row] : INFINITY;  // invalid query: P = 0
  const float Dr = qv ? p.dd[row] : 0.f;
  const float* kb = p.k + bh * p.Ns * D;
  const float* vb = p.v + bh * p.Ns * D;
  f32x16 dQ[DB];
#pragma unroll
  for (int i = 0; i < DB; ++i) dQ[i] = f32x16{};
  Stager<D> gk, gv;
  gk.load(kb, 0, p.Ns, tid);
  gv.load(vb, 0, p.Ns, tid);
  gk.store(sK[0], tid);
  gv.store(sV[0], tid);
  __syncthreads();
  const int nt = (p.Ns + TT - 1) / TT;
  for (int t = 0; t < nt; ++t) {
    const int k0 = t * TT, cb = t & 1;
    const bool nxt = t + 1 < nt;
    if (nxt) {
      gk.load(kb, k0 + TT, p.Ns, tid);
      gv.load(vb, k0 + TT, p.Ns, tid);
    }
    const f32x16 S = scores_t(sK[cb], qr, k0, p.Ns, h, r32);
    // dA^T (keys x queries) = [V' | V'^2] (keys x 2D) . [dM' | dE2']^T
    f32x16 dA = {};
    const float* vr = sV[cb] + r32 * LD + HD * h;
#pragma unroll
    for (int i = 0; i < HD / 4; ++i) {
      const f32x4 vv = ld4(vr + 4 * i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        dA = mfma(vv[e], dm[4 * i + e], dA);
        dA = mfma(vv[e] * vv[e], de[4 * i + e], dA);
      }
    }
    f32x16 dS;
#pragma unroll
    for (int r = 0; r < 16; ++r) dS[r] = __builtin_amdgcn_exp2f(S[r] - L) * (dA[r] - Dr);
    // dQ^T (d x queries) += K^T (d x keys) . dS^T (keys x queries)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float* kr = sK[cb] + acc_row(r, h) * LD + r32;
#pragma unroll
      for (int b = 0; b < DB; ++b) dQ[b] = mfma(kr[32 * b], dS[r], dQ[b]);
    }
    if (nxt) {
      gk.store(sK[cb ^ 1], tid);
      gv.store(sV[cb ^ 1], tid);
    }
    __syncthreads();
  }
  if (!qv) return;
  store_blocks(p.dq + row * D, dQ, h);
}

// ---------------------------------------------------------------------------------------
// dK, dV': wave = 32 keys (one per lane column); streams 32-query tiles of Q, dmo, lse2, D_row.
// SPILL (D = 64): also writes dS [Nc][Ns] for dQ = dS K as a GEMM.
// ---------------------------------------------------------------------------------------
template <int D, bool SPILL>
__global__ void __launch_bounds__(kNT, min_waves(D, DKV)) attn_train_dkv_kernel(const TrainP p) {
  static_assert(!SPILL || D == 64, "the dS spill exists at 64 only");
  constexpr int DB = D / 32, HD = D / 2, LD = D + 4, LDO = 2 * D + 4;
  constexpr bool V2 = keep_v2(D);
  __shared__ __attribute__((aligned(16))) float sQ[2][TT * LD];
  __shared__ __attribute__((aligned(16))) float sO[2][TT * LDO];
  __shared__ float sL[2][TT], sD[2][TT];
  const int t0 = xcd_remap(blockIdx.x, p.nblk);
  const long long bh = t0 / p.nb;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, r32 = lane & 31;
  const int key = (t0 % p.nb) * kRowsWG + wave * 32 + r32;
  const bool kv = key < p.Ns;
  float kr[HD], vr[HD], vr2[V2 ? HD : 1];
  load_half_row(kr, p.k + bh * p.Ns * D, key, kv, h, kLog2e);
  load_half_row(vr, p.v + bh * p.Ns * D, key, kv, h, 1.0f);
  if constexpr (V2) {
#pragma unroll
    for (int s = 0; s < HD; ++s) vr2[s] = vr[s] * vr[s];  // V'^2 once (the wave's keys are fixed)
  }
  auto v2 = [&](int s) {
    if constexpr (V2) return vr2[s];
    else return vr[s] * vr[s];
  };
  const float* qb = p.q + bh * p.Nc * D;
  const float* ob = p.dmo + bh * p.Nc * 2 * D;
  const float* lb = p.lse + bh * p.Nc;
  const float* db = p.dd + bh * p.Nc;
  f32x16 G1[DB], G2[DB], dK[DB];
#pragma unroll
  for (int i = 0; i < DB; ++i) G1[i] = G2[i] = dK[i] = f32x16{};
  Stager<D, SPILL> gq;
  Stager<2 * D, SPILL> go;
  float gl = INFINITY, gd = 0.f;
  // With SPILL the loop body is branch-free around global memory (clamped loads, the tile after
  // the last one loaded and discarded, range-checked buffer stores for dS): the wait before the
  // LDS write then counts only the tile loads, and the dS stores stay in flight across tiles
  // (a branch around any of them made the wait-count pass drain every store: 8.69 -> 8.32 ms per
  // 512^2 B8 block backward).  Without stores the plain branches are cheaper.
  auto load = [&](int q0) {
    gq.load(qb, q0, p.Nc, tid);
    go.load(ob, q0, p.Nc, tid);
    const int qi = q0 + (SPILL ? tid & (TT - 1) : tid);  // SPILL: every thread loads (no branch)
    if constexpr (SPILL) {
      const float l0 = lb[min(qi, p.Nc - 1)], d0 = db[min(qi, p.Nc - 1)];
      gl = qi < p.Nc ? l0 : INFINITY;  // padded query: P = 0
      gd = qi < p.Nc ? d0 : 0.f;
    } else if (tid < TT && qi < p.Nc) {
      gl = lb[qi];
      gd = db[qi];
    } else {
      gl = INFINITY;
      gd = 0.f;
    }
  };
  auto store = [&](int buf) {
    gq.store(sQ[buf], tid);
    go.store(sO[buf], tid);
    if (tid < TT) {
      sL[buf][tid] = gl;
      sD[buf][tid] = gd;
    }
  };
  // dS rows of this (b, h): offsets past num_records (rows >= Nc, or a key >= Ns, whose lanes
  // add (Nc + 32) rows) are dropped; unsigned offsets < 2 (Nc + 32) Ns * 4 < 2^32 (entry check)
  const unsigned dkey = kv ? key * 4u : (unsigned)(p.Nc + TT) * p.Ns * 4;
  const __amdgpu_buffer_rsrc_t dsr =
      __builtin_amdgcn_make_buffer_rsrc(SPILL ? p.ds + bh * p.Nc * p.Ns : nullptr, 0,
                                        SPILL ? p.Nc * p.Ns * 4 : 0, 0x00020000);
  load(0);
  store(0);
  __syncthreads();
  TRAIN_STAMP(0);
  const int nt = (p.Nc + TT - 1) / TT;
  for (int t = 0; t < nt; ++t) {
    const int cb = t & 1;
    const bool nxt = t + 1 < nt;
    if (SPILL || nxt) load((t + 1) * TT);
    // S (queries x keys) = Q . K^T, dA (queries x keys) = [dM' | dE2'] . [V' | V'^2]^T
    f32x16 S = {}, dA = {};
    const float* qrow = sQ[cb] + r32 * LD + HD * h;
    const float* orow = sO[cb] + r32 * LDO + HD * h;
#pragma unroll
    for (int i = 0; i < HD / 4; ++i) {
      const f32x4 qq = ld4(qrow + 4 * i), o1 = ld4(orow + 4 * i), o2 = ld4(orow + D + 4 * i);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int s = 4 * i + e;
        S = mfma(qq[e], kr[s], S);
        dA = mfma(o1[e], vr[s], dA);
        dA = mfma(o2[e], v2(s), dA);
      }
    }
    f32x16 P, dS;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qi = acc_row(r, h);
      P[r] = __builtin_amdgcn_exp2f(S[r] - sL[cb][qi]);
      dS[r] = P[r] * (dA[r] - sD[cb][qi]);
    }
    if constexpr (SPILL) {  // dS [q][key]: for each register the 32 lanes of a half write 128 B
      const unsigned base = (unsigned)(t * TT + 4 * h) * p.Ns * 4 + dkey;
#pragma unroll
      for (int r = 0; r < 16; ++r)
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(dS[r]), dsr,
                                              (int)(base + acc_row(r, 0) * p.Ns * 4u), 0, 0);
    }
    // G1^T, G2^T (c x keys) += [dM' | dE2']^T (c x queries) . P;  dK^T += Q^T . dS
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float* o = sO[cb] + acc_row(r, h) * LDO + r32;
      const float* qq = sQ[cb] + acc_row(r, h) * LD + r32;
#pragma unroll
      for (int b = 0; b < DB; ++b) {
        G1[b] = mfma(o[32 * b], P[r], G1[b]);
        G2[b] = mfma(o[D + 32 * b], P[r], G2[b]);
        dK[b] = mfma(qq[32 * b], dS[r], dK[b]);
      }
    }
    if (nxt) store(cb ^ 1);
    lds_barrier();
  }
  TRAIN_STAMP(1);
  if (!kv) return;
  const long long row = bh * p.Ns + key;
  store_dkv(p.v + row * D, p.dv + row * D, p.dk + row * D, h, G1, G2, dK);
}

// ---------------------------------------------------------------------------------------
// dK, dV' with the dS spill, LDS-DMA + software-pipelined form (round 4; the training default):
// the same products in the same order as attn_train_dkv_kernel<.., SPILL> (bit-identical dK / dV'
// / dS).  That kernel runs one wave per SIMD (288 registers) and measured 0.76 of the
// clock-adjusted fp32 peak at 2.39 GHz (profiles/r04_train_dkv_clock.log): each tile's MFMA
// stream stops for its softmax VALU (S -> P, dA -> dS), its dS stores, its staging writes and the
// barrier.  Here:
//   * iteration t runs tile t+1's first phase (S, dA = 96 MFMAs) while tile t's softmax VALU and
//     dS stores fill the MFMA gaps, then tile t's second phase (G1, G2, dK = 96 MFMAs): the matrix
//     pipe always has independent work (two S / dA register sets, one wave per SIMD);
//   * the Q / dO / lse / D tiles arrive by LDS-DMA (global_load_lds) into a 3-slot ring — no
//     staging registers or LDS write pass, one counted vmcnt that never waits on the dS stores;
//     rows are XOR-swizzled on the source address (16-B chunk c of row r at slot c ^ (r & 15) of
//     its 256-B bank row): the phase-1 ds_read_b128 (32 rows, one chunk) and the phase-2
//     ds_read_b32 (one row, 32 consecutive floats) are conflict-free;
//   * query rows past Nc load clamped rows with lse = +inf, D = 0 (P = 0).
// 2 waves per SIMD (256 registers) was tried: 40+ spilled registers.
// ---------------------------------------------------------------------------------------
MHADA_DEV void train_glds(const float* src, float* lds, int bytes) {
  if (bytes == 16)
    glds16(src, lds);
  else
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)lds, 4, 0, 0);
}

// padding rows of the lse | D tile (query >= Nc): P = exp2(S - inf) = 0, D = 0
__device__ float g_train_pad[2] = {INFINITY, 0.f};

__global__ void __launch_bounds__(256, 1) attn_train_dkv_dma_kernel(const TrainP p) {
  constexpr int NW = 4, NS = 3;
  constexpr int QF = TT * 64, OF = TT * 128, SLOT = QF + OF + 2 * TT;  // floats per ring slot (24.8 KiB)
  __shared__ __attribute__((aligned(16))) float smem[NS * SLOT];      // 74.5 KiB
  const int t0 = xcd_remap(blockIdx.x, p.nblk);
  const long long bh = t0 / p.nb;
  const int tid = threadIdx.x, lane = tid & 63, h = lane >> 5, r32 = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int key = (t0 % p.nb) * 32 * NW + wave * 32 + r32;
  const bool kv = key < p.Ns;
  float kr[32], vr[32], vr2[32];
  load_half_row(kr, p.k + bh * p.Ns * 64, key, kv, h, kLog2e);
  load_half_row(vr, p.v + bh * p.Ns * 64, key, kv, h, 1.0f);
#pragma unroll
  for (int s2 = 0; s2 < 32; ++s2) vr2[s2] = vr[s2] * vr[s2];
  const float* qb = p.q + bh * p.Nc * 64;
  const float* ob = p.dmo + bh * p.Nc * 128;
  const float* lb = p.lse + bh * p.Nc;
  const float* db = p.dd + bh * p.Nc;
  // DMA pieces (1 KiB = 64 lanes x 16 B) of this wave: Q rows 4 per piece (pieces 2w, 2w+1), dO
  // rows 2 per piece (pieces 4w .. 4w+3); each lane fetches the global chunk its LDS slot holds.
  // Q and dO go through buffer resources built per tile (scalar work) over the rows q0 .. Nc - 1,
  // so each lane's offset is a constant and a piece costs no vector address arithmetic (an fp32
  // MFMA holds the SIMD's vector issue for its whole 64 cycles, profiles/r05_f32mfma_fill.log:
  // every VALU instruction adds to the loop).  Rows past Nc read 0 (out of range); with their
  // lse = +inf (padding piece below) P = 0 there, as with the clamped rows of the other kernel.
  typedef __attribute__((address_space(3))) void* LdsP;
  int qvo[2], ovo[4];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int row = 4 * (2 * wave + i) + (lane >> 4);
    qvo[i] = (row * 64 + 4 * ((lane & 15) ^ (row & 15))) * 4;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = 2 * (4 * wave + i) + (lane >> 5);
    ovo[i] = (row * 128 + 4 * (((lane >> 4) & 1) * 16 + ((lane & 15) ^ (row & 15)))) * 4;
  }
  auto stage = [&](int q0, int sl) {  // tile q0 .. q0+31 into ring slot sl
    float* d = smem + sl * SLOT;
    const int left = max(p.Nc - q0, 0);
    const __amdgpu_buffer_rsrc_t qrs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(qb + (long long)min(q0, p.Nc) * 64), 0, left * 64 * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t ors = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(ob + (long long)min(q0, p.Nc) * 128), 0, left * 128 * 4, 0x00020000);
#pragma unroll
    for (int i = 0; i < 2; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(qrs, (LdsP)(d + (2 * wave + i) * 256), 16, qvo[i], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ors, (LdsP)(d + QF + (4 * wave + i) * 256), 16, ovo[i], 0, 0, 0);
    // lse | D: lanes 0-31 / 32-63; padding queries read +inf / 0 (every wave issues the same
    // piece, so every wave's wait counts are equal)
    const int qi = q0 + r32;
    train_glds(qi < p.Nc ? (h ? db : lb) + qi : g_train_pad + h, d + QF + OF, 4);
  };
  // phase-2 reads of row R = rowb(r) + 4h: logical float r32 (chunk r32 / 4) sits at physical
  // 16-B slot (r32 / 4) ^ (R & 15) = 8 ((r >> 2) & 1) + ((r32 / 4) ^ ((r & 3) | 4h)); float 32 + r32
  // at slot 8 (1 ^ ((r >> 2) & 1)) + the same low bits.  Per lane only (r & 3) varies: 4 offsets
  // per operand (O and Q rows differ in length), the rest folds into the ds_read immediate.
  int xo[4], xq[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int lo = 4 * ((r32 >> 2) ^ (j | (4 * h))) + (r32 & 3);
    xo[j] = (QF + 4 * h * 128 + lo) & 0xffff;  // the O rows' base QF folded in: immediates stay < 64 KiB
    xq[j] = (4 * h * 64 + lo) & 0xffff;
  }
  const int sw1 = r32 & 15;
  f32x16 G1[2] = {f32x16{}, f32x16{}}, G2[2] = {f32x16{}, f32x16{}}, dK[2] = {f32x16{}, f32x16{}};
  // dS spill offsets of the lane's 16 accumulator rows relative to the tile's first row (past the
  // resource for keys >= Ns)
  unsigned dvo[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) dvo[r] = kv ? (unsigned)acc_row(r, h) * p.Ns * 4 + key * 4u : 0x7ff00000u;
  // phase 1 of the tile in ring slot sl: S (queries x keys) = Q . K^T, dA = [dM' | dE2'] . [V' | V'^2]^T
  // Every LDS address below is a per-lane register plus an immediate: the ring slot is a
  // compile-time constant in each unrolled step (the loop runs six steps per iteration, two
  // register sets x three slots), and the per-lane parts are masked so their sign bit is known
  // zero (hipcc folds constants into a ds_read immediate only then).
  int qoff[8], ooff[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int c = 4 * ((8 * h + i) ^ sw1);
    qoff[i] = (r32 * 64 + c) & 0xffff;
    ooff[i] = (QF + r32 * 128 + c) & 0xffff;
  }
  auto phase1 = [&](int sl, f32x16& S, f32x16& dA) {
    const float* sQ = smem + sl * SLOT;
    S = f32x16{};
    dA = f32x16{};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const f32x4 qq = ld4(sQ + qoff[i]), o1 = ld4(sQ + ooff[i]), o2 = ld4(sQ + ooff[i] + 64);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int s2 = 4 * i + e;
        S = mfma(qq[e], kr[s2], S);
        dA = mfma(o1[e], vr[s2], dA);
        dA = mfma(o2[e], vr2[s2], dA);
      }
    }
  };
  // S -> P, dA -> dS in place (tile of ring slot sl, first query q0), and dS's spill stores
  auto softmax = [&](int sl, int q0, f32x16& S, f32x16& dA) {
    const float* sLD = smem + sl * SLOT + QF + OF;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qi = acc_row(r, h);
      S[r] = __builtin_amdgcn_exp2f(S[r] - sLD[qi]);
      dA[r] = S[r] * (dA[r] - sLD[TT + qi]);
    }
    // dS [q][key]: 32 lanes write 128 B, through a resource over rows q0 .. Nc - 1 (rows past Nc
    // and keys past Ns are out of range: dropped) and per-lane offsets precomputed for the 16 rows
    const __amdgpu_buffer_rsrc_t dsr = __builtin_amdgcn_make_buffer_rsrc(
        p.ds + bh * p.Nc * p.Ns + (long long)min(q0, p.Nc) * p.Ns, 0, max(p.Nc - q0, 0) * p.Ns * 4, 0x00020000);
#pragma unroll
    for (int r = 0; r < 16; ++r)
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(dA[r]), dsr, (int)dvo[r], 0, 0);
  };
  // phase 2: G1^T, G2^T (c x keys) += [dM' | dE2']^T (c x queries) . P;  dK^T += Q^T . dS
  auto phase2 = [&](int sl, const f32x16& P, const f32x16& dS) {
    const float* sQ = smem + sl * SLOT;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = r & 3, rowb = acc_row(r, 0), b3 = (r >> 2) & 1;
      const float* o = sQ + xo[j] + rowb * 128;
      const float* qq = sQ + xq[j] + rowb * 64;
      G1[0] = mfma(o[32 * b3], P[r], G1[0]);
      G1[1] = mfma(o[32 * (1 - b3)], P[r], G1[1]);
      G2[0] = mfma(o[64 + 32 * b3], P[r], G2[0]);
      G2[1] = mfma(o[64 + 32 * (1 - b3)], P[r], G2[1]);
      dK[0] = mfma(qq[32 * b3], dS[r], dK[0]);
      dK[1] = mfma(qq[32 * (1 - b3)], dS[r], dK[1]);
    }
  };

  const int nt = (p.Nc + TT - 1) / TT;
  stage(0, 0);
  stage(TT, 1);
  asm volatile("s_waitcnt vmcnt(7)" ::: "memory");  // tile 0 (7 pieces per tile and wave)
  lds_barrier();
  TRAIN_STAMP(0);
  f32x16 Sa, dAa, Sb, dAb;
  phase1(0, Sa, dAa);
  // iteration t: publish tile t + 1; DMA tile t + 2 into the slot tile t - 1 used; tile t + 1's
  // phase 1 beside tile t's softmax and stores; tile t's phase 2.  Two register sets, A / B,
  // alternate and the ring slot cycles 0, 1, 2: six steps per loop iteration, each with its slot
  // a compile-time constant.
  auto step = [&](int t, auto slc, f32x16& S, f32x16& dA, f32x16& Sn, f32x16& dAn) __attribute__((always_inline)) {
    constexpr int SL = decltype(slc)::value, SN = (SL + 1) % 3, S2 = (SL + 2) % 3;
    // tile t + 1 landed (younger: tile t's dS stores... issued after it in iteration t - 1: 16)
    if (t == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    lds_barrier();
    stage((t + 2) * TT, S2);  // past the end: rows read 0, never used
    softmax(SL, t * TT, S, dA);
    phase1(SN, Sn, dAn);  // tile t + 1 (past the end: result unused)
    phase2(SL, S, dA);
  };
  typedef std::integral_constant<int, 0> L0;
  typedef std::integral_constant<int, 1> L1;
  typedef std::integral_constant<int, 2> L2;
  int t = 0;
  for (; t + 5 < nt; t += 6) {
    step(t, L0(), Sa, dAa, Sb, dAb);
    step(t + 1, L1(), Sb, dAb, Sa, dAa);
    step(t + 2, L2(), Sa, dAa, Sb, dAb);
    step(t + 3, L0(), Sb, dAb, Sa, dAa);
    step(t + 4, L1(), Sa, dAa, Sb, dAb);
    step(t + 5, L2(), Sb, dAb, Sa, dAa);
  }
  if (t < nt) step(t, L0(), Sa, dAa, Sb, dAb);
  if (t + 1 < nt) step(t + 1, L1(), Sb, dAb, Sa, dAa);
  if (t + 2 < nt) step(t + 2, L2(), Sa, dAa, Sb, dAb);
  if (t + 3 < nt) step(t + 3, L0(), Sb, dAb, Sa, dAa);
  if (t + 4 < nt) step(t + 4, L1(), Sa, dAa, Sb, dAb);
  TRAIN_STAMP(1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the clamped DMA past the end has landed
  if (!kv) return;
  const long long row = bh * p.Ns + key;
  store_dkv(p.v + row * 64, p.dv + row * 64, p.dk + row * 64, h, G1, G2, dK);
}

// per-(b, h) dS slice addressed by 32-bit buffer offsets, with 0x7ffffff0 free as the drop offset
constexpr long long kMaxSpillRows = (0x7fff0000LL / 4);
// rows and tiles are indexed in int (row offsets are 64-bit): n + kRowsWG must not wrap
constexpr int kMaxRows = 1 << 30;

typedef void (*TrainKernel)(TrainP);

// One kernel over the n rows (queries or keys) of each of BH (batch, head) pairs.
int launch(const char* fn, TrainKernel kern, TrainP& p, long long BH, int n, mhada_stream_t s) {
  p.nb = (n + kRowsWG - 1) / kRowsWG;
  const long long nblk = BH * p.nb;
  if (nblk > (1LL << 31) - 1) return fail(std::string(fn) + ": grid too large");
  p.nblk = (int)nblk;
  hipLaunchKernelGGL(kern, dim3(p.nblk), dim3(kNT), 0, (hipStream_t)s, p);
  return check_launch(fn);
}

// The launchers take what their entry points (fn) checked: D is 32, 64 or 128.
int launch_fwd(const char* fn, const float* q, const float* k, const float* v, const float* x, float* out, float* mo,
               float* lse, int BH, int D, int Nc, int Ns, mhada_stream_t s) {
  TrainP p = {};
  p.q = q; p.k = k; p.v = v; p.x = x; p.out = out; p.mo = mo; p.lse = lse; p.Nc = Nc; p.Ns = Ns;
  return launch(fn, D == 32 ? attn_train_fwd_kernel<32> : D == 64 ? attn_train_fwd_kernel<64> : attn_train_fwd_kernel<128>,
                p, BH, Nc, s);
}

int launch_dq(const char* fn, const float* q, const float* k, const float* v, const float* lse, const float* dmo,
              const float* dd, float* dq, int BH, int D, int Nc, int Ns, mhada_stream_t s) {
  TrainP p = {};
  p.q = q; p.k = k; p.v = v; p.lse = const_cast<float*>(lse); p.dmo = dmo; p.dd = dd; p.dq = dq; p.Nc = Nc; p.Ns = Ns;
  return launch(fn, D == 32 ? attn_train_dq_kernel<32> : D == 64 ? attn_train_dq_kernel<64> : attn_train_dq_kernel<128>,
                p, BH, Nc, s);
}

// ds (D = 64 only): the dS spill, by the LDS-DMA kernel (tuning train_dkv_dma, the default) or the
// register-staged one; null: no spill.  Nc == 0 is fine: no query tile, dK = dV' = 0.
int launch_dkv(const char* fn, const float* q, const float* k, const float* v, const float* lse, const float* dmo,
               const float* dd, float* dk, float* dv, float* ds, int BH, int D, int Nc, int Ns, mhada_stream_t s) {
  TrainP p = {};
  p.q = q; p.k = k; p.v = v; p.lse = const_cast<float*>(lse); p.dmo = dmo; p.dd = dd; p.dk = dk; p.dv = dv; p.ds = ds;
  p.Nc = Nc; p.Ns = Ns;
  const TrainKernel kern = ds ? (tuning().train_dkv_dma ? attn_train_dkv_dma_kernel : attn_train_dkv_kernel<64, true>)
                           : D == 32 ? attn_train_dkv_kernel<32, false>
                           : D == 64 ? attn_train_dkv_kernel<64, false>
                                     : attn_train_dkv_kernel<128, false>;
  return launch(fn, kern, p, BH, Ns, s);
}

// The width and row checks of the _hd entries (fn ends in "_hd").
int check_hd(const std::string& fn, int D, int Nc, int Ns) {
  if (D != 32 && D != 128) return fail(fn + ": D must be 32 or 128 (64: " + fn.substr(0, fn.size() - 3) + ")");
  if (Nc > kMaxRows || Ns > kMaxRows) return fail(fn + ": Nc, Ns above 2^30");
  return MHADA_OK;
}

}  // namespace
}  // namespace mhada

using namespace mhada;

extern "C" int mhada_attn_train_fwd(const float* q, const float* k, const float* v, const float* x, float* out,
                                    float* mo, float* lse, int BH, int Nc, int Ns, mhada_stream_t s) {
  if (!q || !k || !v || !x || !out || !mo || !lse || BH <= 0 || Nc <= 0 || Ns <= 0)
    return fail("mhada_attn_train_fwd: bad args");
  return launch_fwd("mhada_attn_train_fwd", q, k, v, x, out, mo, lse, BH, 64, Nc, Ns, s);
}

extern "C" int mhada_attn_train_bwd(const float* q, const float* k, const float* v, const float* lse,
                                    const float* dmo, const float* dd, float* dq, float* dk, float* dv, int BH,
                                    int Nc, int Ns, mhada_stream_t s) {
  if (!q || !k || !v || !lse || !dmo || !dd || !dq || !dk || !dv || BH <= 0 || Nc <= 0 || Ns <= 0)
    return fail("mhada_attn_train_bwd: bad args");
  if (int rc = launch_dq("mhada_attn_train_bwd", q, k, v, lse, dmo, dd, dq, BH, 64, Nc, Ns, s)) return rc;
  return launch_dkv("mhada_attn_train_bwd", q, k, v, lse, dmo, dd, dk, dv, nullptr, BH, 64, Nc, Ns, s);
}

extern "C" int mhada_attn_train_dq(const float* q, const float* k, const float* v, const float* lse, const float* dmo,
                                   const float* dd, float* dq, int BH, int Nc, int Ns, mhada_stream_t s) {
  if (!q || !k || !v || !lse || !dmo || !dd || !dq || BH <= 0 || Nc <= 0 || Ns <= 0)
    return fail("mhada_attn_train_dq: bad args");
  return launch_dq("mhada_attn_train_dq", q, k, v, lse, dmo, dd, dq, BH, 64, Nc, Ns, s);
}

extern "C" int mhada_attn_train_dkv(const float* q, const float* k, const float* v, const float* lse,
                                    const float* dmo, const float* dd, float* dk, float* dv, float* ds, int BH,
                                    int Nc, int Ns, mhada_stream_t s) {
  if (!q || !k || !v || !lse || !dmo || !dd || !dk || !dv || !ds || BH <= 0 || Nc <= 0 || Ns <= 0)
    return fail("mhada_attn_train_dkv: bad args");
  if ((long long)(Nc + TT) * Ns > kMaxSpillRows)
    return fail("mhada_attn_train_dkv: (Nc + 32) * Ns above 2^29 - 2^14 (32-bit dS offsets)");
  return launch_dkv("mhada_attn_train_dkv", q, k, v, lse, dmo, dd, dk, dv, ds, BH, 64, Nc, Ns, s);
}

extern "C" int mhada_attn_train_fwd_hd(const float* q, const float* k, const float* v, const float* x, float* out,
                                       float* mo, float* lse, int BH, int D, int Nc, int Ns, mhada_stream_t s) {
  if (!q || !k || !v || !x || !out || !mo || !lse || BH <= 0 || Nc < 0 || Ns <= 0)
    return fail("mhada_attn_train_fwd_hd: bad args");
  if (int rc = check_hd("mhada_attn_train_fwd_hd", D, Nc, Ns)) return rc;
  if (Nc == 0) return MHADA_OK;
  return launch_fwd("mhada_attn_train_fwd_hd", q, k, v, x, out, mo, lse, BH, D, Nc, Ns, s);
}

extern "C" int mhada_attn_train_bwd_hd(const float* q, const float* k, const float* v, const float* lse,
                                       const float* dmo, const float* dd, float* dq, float* dk, float* dv, int BH,
                                       int D, int Nc, int Ns, mhada_stream_t s) {
  if (!q || !k || !v || !lse || !dmo || !dd || !dq || !dk || !dv || BH <= 0 || Nc < 0 || Ns <= 0)
    return fail("mhada_attn_train_bwd_hd: bad args");
  if (int rc = check_hd("mhada_attn_train_bwd_hd", D, Nc, Ns)) return rc;
  if (Nc > 0)
    if (int rc = launch_dq("mhada_attn_train_bwd_hd", q, k, v, lse, dmo, dd, dq, BH, D, Nc, Ns, s)) return rc;
  return launch_dkv("mhada_attn_train_bwd_hd", q, k, v, lse, dmo, dd, dk, dv, nullptr, BH, D, Nc, Ns, s);
}

extern "C" int mhada_attn_train_dq_hd(const float* q, const float* k, const float* v, const float* lse,
                                      const float* dmo, const float* dd, float* dq, int BH, int D, int Nc, int Ns,
                                      mhada_stream_t s) {
  if (!q || !k || !v || !lse || !dmo || !dd || !dq || BH <= 0 || Nc < 0 || Ns <= 0)
    return fail("mhada_attn_train_dq_hd: bad args");
  if (int rc = check_hd("mhada_attn_train_dq_hd", D, Nc, Ns)) return rc;
  if (Nc == 0) return MHADA_OK;
  return launch_dq("mhada_attn_train_dq_hd", q, k, v, lse, dmo, dd, dq, BH, D, Nc, Ns, s);
}

#ifdef ATTN_CLOCK
// Diagnostic builds: the first n stamps (4 per workgroup) of the last dK/dV' launch.
extern "C" int mhada_dbg_train_clock(unsigned long long* host, int n) {
  if (!host || n <= 0 || n > 4 * kTrainClockBlocks) return fail("mhada_dbg_train_clock: bad args");
  if (hipMemcpyFromSymbol(host, HIP_SYMBOL(g_train_clock), sizeof(unsigned long long) * n) != hipSuccess)
    return fail("mhada_dbg_train_clock: copy failed");
  return MHADA_OK;
}
#endif
