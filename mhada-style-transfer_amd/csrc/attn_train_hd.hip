// MHAda attention for the training path at head widths D = 32 | 128 (16- and 4-head models at 512
// channels): the forward that keeps the softmax statistics and the two-kernel backward of
// attn_train.hip, one kernel family templated on D, fp32 on v_mfma_f32_32x32x2_f32.
//
// Reference: AdaAttnMultiHead.forward (MHAdaSTr/network/adaDecoder.py:186-198) under
// train_image.py:93-144 autograd.  The maths is attn_train.hip:1-23 with rows of D floats: per
// (batch, head), Q, X [Nc][D], K, V' [Ns][D] (V' centred by the caller),
//   A = softmax(Q K^T)   M' = A V'   E2' = A V'^2   out' = sqrt(max(E2' - M'^2, 1e-6)) X + M'
// (no 1/sqrt(d) factor).  The forward writes out', mo = [M' | E2'] ([Nc][2D]) and the log2 row
// normaliser lse2.  From dmo = [dM' | dE2'] and D_row (mhada_attn_train_bwd_prep_hd), with P = A
// recomputed from lse2 and dA = dM'.V'^T + dE2'.(V'^2)^T:
//   dS = P (dA - D_row)   dQ = dS K   dK = dS^T Q   dV' = P^T dM' + 2 V' (P^T dE2')
// as two deterministic kernels (no atomics): key-stationary dK / dV', query-stationary dQ.  The
// Nc x Ns matrices never reach memory.
//
// These are the simplest forms of the 64-wide family (attn_train_fwd_kernel, attn_train_dq_kernel,
// attn_train_dkv_kernel<.., SPILL = false>): register-staged 32-row LDS tiles (two buffers, one
// barrier per tile), every product arranged so that one operand is the accumulator of the previous
// one.  The dS spill and its GEMM, the LDS-DMA dK/dV' kernel, the SPLIT3 forward / dQ and the vt
// forward exist at 64 only.
//
// MFMA 32x32x2 f32 layout (cdna_hip_programming.md §3): lane l gives A[l%32][l/32] and
// B[l/32][l%32]; accumulator register r of lane l is D[acc_row(r, l/32)][l%32].  A product over
// D k-indices is D/2 instructions: lane half h supplies the indices (D/2) h + s.
//
// Registers and LDS per workgroup of 4 waves (128 queries or keys); DESIGN.md §3b has the
// compiler's figures:
//   D = 32:  two waves per SIMD everywhere (accumulators: fwd 2 blocks, dQ 1, dK/dV' 3).
//   D = 128: one wave per SIMD.  fwd: 8 accumulator blocks (128 registers) + the query row (64);
//            dQ: Q, dM', dE2' rows (192) + 4 blocks; dK/dV': K, V' rows (128; V'^2 is squared at
//            the operand, not kept) + dK, P^T dM', P^T dE2' (12 blocks, 192 registers); its Q
//            (16.5 KiB) and dmo (32.5 KiB) tiles double-buffered take 98 KiB of LDS.
#include "common.h"

namespace mhada {
namespace {

constexpr float kLog2e = 1.4426950408889634f;
constexpr int TT = 32;  // keys (fwd, dQ) or queries (dK/dV') staged per LDS tile
constexpr int kNW = 4;  // waves per workgroup: 128 queries (fwd, dQ) or keys (dK/dV')

MHADA_DEV int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
MHADA_DEV f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
MHADA_DEV void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
MHADA_DEV f32x16 mfma(float a, float b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

struct TrainHdP {
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
  int Nc, Ns, nb, nblk;  // nb = row blocks per (b, h)
};

// LDS hand-off barrier (attn_train.hip): waits for the LDS operations only.
MHADA_DEV void lds_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

// Register-staged copy of rows [r0, r0+TT) of a [n][W] matrix (rows past n zero) into an LDS tile
// of rows padded to W + 4 floats (row reads by ds_read_b128 and column reads by ds_read_b32 are
// both conflict-free: W + 4 = 4 mod 32): load() issues the global reads one tile ahead, store()
// writes them after the current tile's math.  Row offsets are 64-bit.
template <int W>
struct Stager {
  static constexpr int NT = 64 * kNW;
  static constexpr int CPR = W / 4;        // 16-B chunks per row
  static constexpr int N = TT * CPR / NT;  // chunks per thread
  static constexpr int LD = W + 4;
  static_assert(N * NT == TT * CPR, "tile must divide evenly");
  f32x4 r[N];
  MHADA_DEV void load(const float* g, int r0, int n, int tid) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int c = tid + NT * i, row = c / CPR, col = (c % CPR) * 4, gr = r0 + row;
      r[i] = gr < n ? ld4(g + (long long)gr * W + col) : f32x4{0.f, 0.f, 0.f, 0.f};
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

// The lane's half of a row of D floats: reg[s] = g[row][(D/2) h + s] * scale (zeros if !valid).
template <int D>
MHADA_DEV void load_half_row(float (&reg)[D / 2], const float* g, int row, bool valid, int h, float scale) {
  const float* p = g + (long long)(valid ? row : 0) * D + (D / 2) * h;
#pragma unroll
  for (int i = 0; i < D / 8; ++i) {
    const f32x4 t = ld4(p + 4 * i);
#pragma unroll
    for (int e = 0; e < 4; ++e) reg[4 * i + e] = valid ? t[e] * scale : 0.f;
  }
}

// S^T (keys x queries) in log2 units from the staged K tile and the lane's query row (qr
// pre-scaled by log2 e); keys past Ns masked to -inf.
template <int D>
MHADA_DEV f32x16 scores_t(const float* sK, const float (&qr)[D / 2], int k0, int Ns, int h, int r32) {
  f32x16 S = {};
  const float* kr = sK + r32 * (D + 4) + (D / 2) * h;
#pragma unroll
  for (int i = 0; i < D / 8; ++i) {
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

// accumulator blocks b = 0 .. D/32-1 of a lane hold columns 32 b + 8 g + 4 h + e in register 4 g + e
template <int D>
MHADA_DEV void store_blocks(float* row, const f32x16 (&A)[D / 32], int h) {
#pragma unroll
  for (int b = 0; b < D / 32; ++b)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      st4(row + 32 * b + 8 * g + 4 * h, f32x4{A[b][4 * g], A[b][4 * g + 1], A[b][4 * g + 2], A[b][4 * g + 3]});
}

// ---------------------------------------------------------------------------------------
// forward: wave = 32 queries (one per lane column), online softmax over 32-key tiles
// ---------------------------------------------------------------------------------------
template <int D, int OCC>
__global__ void __launch_bounds__(64 * kNW, OCC) attn_train_fwd_hd_kernel(const TrainHdP p) {
  constexpr int DB = D / 32, LD = D + 4;
  __shared__ __attribute__((aligned(16))) float sK[2][TT * LD];
  __shared__ __attribute__((aligned(16))) float sV[2][TT * LD];
  const int t0 = xcd_remap(blockIdx.x, p.nblk);
  const long long bh = t0 / p.nb;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, r32 = lane & 31;
  const int q = (t0 % p.nb) * 32 * kNW + wave * 32 + r32;
  const bool qv = q < p.Nc;
  float qr[D / 2];
  load_half_row<D>(qr, p.q + bh * p.Nc * D, q, qv, h, kLog2e);
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
    f32x16 S = scores_t<D>(sK[cb], qr, k0, p.Ns, h, r32);
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
template <int D, int OCC>
__global__ void __launch_bounds__(64 * kNW, OCC) attn_train_dq_hd_kernel(const TrainHdP p) {
  constexpr int DB = D / 32, HD = D / 2, LD = D + 4;
  __shared__ __attribute__((aligned(16))) float sK[2][TT * LD];
  __shared__ __attribute__((aligned(16))) float sV[2][TT * LD];
  const int t0 = xcd_remap(blockIdx.x, p.nblk);
  const long long bh = t0 / p.nb;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, r32 = lane & 31;
  const int q = (t0 % p.nb) * 32 * kNW + wave * 32 + r32;
  const bool qv = q < p.Nc;
  const long long row = bh * p.Nc + (qv ? q : 0);
  float qr[HD], dm[HD], de[HD];
  load_half_row<D>(qr, p.q + bh * p.Nc * D, q, qv, h, kLog2e);
  load_half_row<D>(dm, p.dmo + bh * p.Nc * 2 * D, 2 * q, qv, h, 1.0f);          // row q of [Nc][2D], first half
  load_half_row<D>(de, p.dmo + bh * p.Nc * 2 * D + D, 2 * q, qv, h, 1.0f);      // second half
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
    const f32x16 S = scores_t<D>(sK[cb], qr, k0, p.Ns, h, r32);
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
  store_blocks<D>(p.dq + row * D, dQ, h);
}

// ---------------------------------------------------------------------------------------
// dK, dV': wave = 32 keys (one per lane column); streams 32-query tiles of Q, dmo, lse2, D_row
// ---------------------------------------------------------------------------------------
template <int D, int OCC>
__global__ void __launch_bounds__(64 * kNW, OCC) attn_train_dkv_hd_kernel(const TrainHdP p) {
  constexpr int DB = D / 32, HD = D / 2, LD = D + 4, LDO = 2 * D + 4;
  __shared__ __attribute__((aligned(16))) float sQ[2][TT * LD];
  __shared__ __attribute__((aligned(16))) float sO[2][TT * LDO];
  __shared__ float sL[2][TT], sD[2][TT];
  const int t0 = xcd_remap(blockIdx.x, p.nblk);
  const long long bh = t0 / p.nb;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, r32 = lane & 31;
  const int key = (t0 % p.nb) * 32 * kNW + wave * 32 + r32;
  const bool kv = key < p.Ns;
  float kr[HD], vr[HD];
  load_half_row<D>(kr, p.k + bh * p.Ns * D, key, kv, h, kLog2e);
  load_half_row<D>(vr, p.v + bh * p.Ns * D, key, kv, h, 1.0f);
  const float* qb = p.q + bh * p.Nc * D;
  const float* ob = p.dmo + bh * p.Nc * 2 * D;
  const float* lb = p.lse + bh * p.Nc;
  const float* db = p.dd + bh * p.Nc;
  f32x16 G1[DB], G2[DB], dK[DB];
#pragma unroll
  for (int i = 0; i < DB; ++i) G1[i] = G2[i] = dK[i] = f32x16{};
  Stager<D> gq;
  Stager<2 * D> go;
  float gl = INFINITY, gd = 0.f;
  auto load = [&](int q0) {
    gq.load(qb, q0, p.Nc, tid);
    go.load(ob, q0, p.Nc, tid);
    const int qi = q0 + tid;
    if (tid < TT && qi < p.Nc) {
      gl = lb[qi];
      gd = db[qi];
    } else {
      gl = INFINITY;  // padded query: P = 0
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
  load(0);
  store(0);
  __syncthreads();
  const int nt = (p.Nc + TT - 1) / TT;
  for (int t = 0; t < nt; ++t) {
    const int cb = t & 1;
    const bool nxt = t + 1 < nt;
    if (nxt) load((t + 1) * TT);
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
        dA = mfma(o2[e], vr[s] * vr[s], dA);
      }
    }
    f32x16 P, dS;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qi = acc_row(r, h);
      P[r] = __builtin_amdgcn_exp2f(S[r] - sL[cb][qi]);
      dS[r] = P[r] * (dA[r] - sD[cb][qi]);
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
  if (!kv) return;
  const long long row = bh * p.Ns + key;
  const float* vg = p.v + row * D;
#pragma unroll
  for (int b = 0; b < DB; ++b)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 vv = ld4(vg + 32 * b + 8 * g + 4 * h);
#pragma unroll
      for (int e = 0; e < 4; ++e) G1[b][4 * g + e] += 2.0f * vv[e] * G2[b][4 * g + e];
    }
  store_blocks<D>(p.dv + row * D, G1, h);
  store_blocks<D>(p.dk + row * D, dK, h);
}

bool hd_width(int D) { return D == 32 || D == 128; }

// rows and tiles are indexed in int (row offsets are 64-bit): n + 32 * kNW must not wrap
constexpr int kMaxRows = 1 << 30;

bool set_grid(TrainHdP& p, long long BH, int n) {
  p.nb = (n + 32 * kNW - 1) / (32 * kNW);
  const long long nblk = BH * p.nb;
  if (nblk > (1LL << 31) - 1) return false;
  p.nblk = (int)nblk;
  return true;
}

}  // namespace
}  // namespace mhada

using namespace mhada;

extern "C" int mhada_attn_train_fwd_hd(const float* q, const float* k, const float* v, const float* x, float* out,
                                       float* mo, float* lse, int BH, int D, int Nc, int Ns, mhada_stream_t s_) {
  if (!q || !k || !v || !x || !out || !mo || !lse || BH <= 0 || Nc < 0 || Ns <= 0)
    return fail("mhada_attn_train_fwd_hd: bad args");
  if (!hd_width(D)) return fail("mhada_attn_train_fwd_hd: D must be 32 or 128 (64: mhada_attn_train_fwd)");
  if (Nc > kMaxRows || Ns > kMaxRows) return fail("mhada_attn_train_fwd_hd: Nc, Ns above 2^30");
  if (Nc == 0) return MHADA_OK;
  TrainHdP p = {};
  p.q = q; p.k = k; p.v = v; p.x = x; p.out = out; p.mo = mo; p.lse = lse; p.Nc = Nc; p.Ns = Ns;
  if (!set_grid(p, BH, Nc)) return fail("mhada_attn_train_fwd_hd: grid too large");
  const hipStream_t s = (hipStream_t)s_;
  if (D == 32) hipLaunchKernelGGL((attn_train_fwd_hd_kernel<32, 2>), dim3(p.nblk), dim3(64 * kNW), 0, s, p);
  else hipLaunchKernelGGL((attn_train_fwd_hd_kernel<128, 1>), dim3(p.nblk), dim3(64 * kNW), 0, s, p);
  return check_launch("mhada_attn_train_fwd_hd");
}

extern "C" int mhada_attn_train_bwd_hd(const float* q, const float* k, const float* v, const float* lse,
                                       const float* dmo, const float* dd, float* dq, float* dk, float* dv, int BH,
                                       int D, int Nc, int Ns, mhada_stream_t s_) {
  if (!q || !k || !v || !lse || !dmo || !dd || !dq || !dk || !dv || BH <= 0 || Nc < 0 || Ns <= 0)
    return fail("mhada_attn_train_bwd_hd: bad args");
  if (!hd_width(D)) return fail("mhada_attn_train_bwd_hd: D must be 32 or 128 (64: mhada_attn_train_bwd)");
  if (Nc > kMaxRows || Ns > kMaxRows) return fail("mhada_attn_train_bwd_hd: Nc, Ns above 2^30");
  const hipStream_t s = (hipStream_t)s_;
  TrainHdP p = {};
  p.q = q; p.k = k; p.v = v; p.lse = const_cast<float*>(lse); p.dmo = dmo; p.dd = dd; p.dq = dq; p.dk = dk; p.dv = dv;
  p.Nc = Nc; p.Ns = Ns;
  if (Nc > 0) {
    if (!set_grid(p, BH, Nc)) return fail("mhada_attn_train_bwd_hd: grid too large");
    if (D == 32) hipLaunchKernelGGL((attn_train_dq_hd_kernel<32, 2>), dim3(p.nblk), dim3(64 * kNW), 0, s, p);
    else hipLaunchKernelGGL((attn_train_dq_hd_kernel<128, 1>), dim3(p.nblk), dim3(64 * kNW), 0, s, p);
  }
  // Nc == 0: no query tile, dK = dV' = 0
  if (!set_grid(p, BH, Ns)) return fail("mhada_attn_train_bwd_hd: grid too large");
  if (D == 32) hipLaunchKernelGGL((attn_train_dkv_hd_kernel<32, 2>), dim3(p.nblk), dim3(64 * kNW), 0, s, p);
  else hipLaunchKernelGGL((attn_train_dkv_hd_kernel<128, 1>), dim3(p.nblk), dim3(64 * kNW), 0, s, p);
  return check_launch("mhada_attn_train_bwd_hd");
}

extern "C" int mhada_attn_train_dq_hd(const float* q, const float* k, const float* v, const float* lse,
                                      const float* dmo, const float* dd, float* dq, int BH, int D, int Nc, int Ns,
                                      mhada_stream_t s_) {
  if (!q || !k || !v || !lse || !dmo || !dd || !dq || BH <= 0 || Nc < 0 || Ns <= 0)
    return fail("mhada_attn_train_dq_hd: bad args");
  if (!hd_width(D)) return fail("mhada_attn_train_dq_hd: D must be 32 or 128 (64: mhada_attn_train_dq)");
  if (Nc > kMaxRows || Ns > kMaxRows) return fail("mhada_attn_train_dq_hd: Nc, Ns above 2^30");
  if (Nc == 0) return MHADA_OK;
  TrainHdP p = {};
  p.q = q; p.k = k; p.v = v; p.lse = const_cast<float*>(lse); p.dmo = dmo; p.dd = dd; p.dq = dq;
  p.Nc = Nc; p.Ns = Ns;
  if (!set_grid(p, BH, Nc)) return fail("mhada_attn_train_dq_hd: grid too large");
  const hipStream_t s = (hipStream_t)s_;
  if (D == 32) hipLaunchKernelGGL((attn_train_dq_hd_kernel<32, 2>), dim3(p.nblk), dim3(64 * kNW), 0, s, p);
  else hipLaunchKernelGGL((attn_train_dq_hd_kernel<128, 1>), dim3(p.nblk), dim3(64 * kNW), 0, s, p);
  return check_launch("mhada_attn_train_dq_hd");
}
