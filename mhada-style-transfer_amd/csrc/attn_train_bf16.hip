// MHAda attention for the training path at head width 64 with the three attention products on the
// bf16 MFMA (v_mfma_f32_32x32x16_bf16, fp32 accumulation): the opt-in mixed-precision mode of
// autograd_path.MHAdaAttnBf16Fn.  Inputs, outputs and gradients are fp32 tensors.
//
// Reference: AdaAttnMultiHead.forward (MHAdaSTr/network/adaDecoder.py:186-198) under
// train_image.py:93-144 autograd inside torch.autocast(bfloat16): bmm in bf16, softmax in fp32.
// The maths is attn_train.hip:1-21 at D = 64: per (batch, head), Q, X [Nc][64],
// K, V' [Ns][64] (V' centred by the caller),
//   A = softmax(Q K^T)   M' = A V'   E2' = A V'^2   out' = sqrt(max(E2' - M'^2, 1e-6)) X + M'
//   dA = dM'.V'^T + dE2'.(V'^2)^T   dS = P (dA - D_row)   dQ = dS K   dK = dS^T Q
//   dV' = P^T dM' + 2 V' (P^T dE2')
// The structure is that of attn_train.hip's plain kernels: a forward that keeps lse2, a query-stationary dQ kernel and
// a key-stationary dK / dV' kernel, both deterministic (no atomics); the Nc x Ns matrices never
// reach memory and nothing is spilled (the backward recomputes S and dA).
//
// Precision.  bf16 (round to nearest even) operands: Q, K, V'_b = bf16(V'), P, dM', dE2', dS, and
// V'_b^2 as an exact hi + lo pair of bf16 planes (the square of the ROUNDED V': 16 significant
// bits), so that E2' - M'^2 is the variance of V'_b under the weights P to fp32 accuracy.  With
// bf16(V'^2) beside bf16(V') (the inference image's form) the variance of a nearly one-hot row
// carried 2^-9 V'^2 of rounding noise against a true value near 0, d out'/d Var = x / (2 sqrt(Var))
// turned it into a large wrong dE2', and dV' was up to 17x further from fp64 than the reference under
// bf16 autocast.  The backward differentiates that forward: dA and dV' use V'_b and the same exact
// V'_b^2, and the two terms of dV' = P^T dM' + 2 V'_b (P^T dE2'), which cancel on peaked rows, take
// dM' and dE2' as hi + lo planes.  fp32: S, the online softmax in log2 units, the row sum (of the
// unrounded P), lse2, D_row, dA - D_row and every accumulator.  S = (bf16 Q . bf16 K) * log2(e): the factor multiplies the fp32 sum AFTER the product in
// all three kernels, so the backward's P = exp2(S - lse2) is the forward's P (rows sum to 1).
// D_row is formed by the pre-pass as sum_c bf16(dmo) mo, from the ROUNDED dmo that dA is formed from:
// dS = P (dA - D_row) cancels where the softmax is peaked, and D_row of the unrounded dmo
// (mhada_attn_train_bwd_prep's dd) leaves bf16-eps |dA| there, many times the true dS.
//
// Operand conversion: a pre-pass (cvt_bf16_kernel) writes each fp32 operand once per call as a bf16
// row image [n][W] and / or a transposed image [W][ceil64(n)] into a caller-provided workspace;
// every query block re-reads K and V' (Nc / 128 times), so converting in the stager would repeat
// the rounding that many times and stage twice the bytes.  The transposed images exist because
// each product that consumes an accumulator tile as its bf16 operand (P, dS: cdna_hip_programming.md
// §3, "an accumulator tile as the next MFMA's operand") sums over the accumulator's ROW index, so
// its other operand must be contiguous along that index; inside each group of 32 rows the
// transposed image stores row 16 s + 8 (j >> 2) + 4 h + (j & 3) at position 16 s + 8 h + j — the k
// order of the packed accumulator — so one 16-byte read is the fragment (as attn.hip's vt image).
//
// MFMA 32x32x16 bf16 layout: lane l (r = l % 32, h = l / 32) gives A[r][8 h + j] and B[8 h + j][r],
// j = 0..7; accumulator register i of lane l is D[acc_row(i, h)][r].
#include "common.h"

namespace mhada {
namespace {

constexpr float kLog2e = 1.4426950408889634f;
constexpr int kNW = 4;        // waves per workgroup: 128 queries (fwd, dQ) or keys (dK/dV')
constexpr int NT = 64 * kNW;  // threads per workgroup

MHADA_DEV bf16x8 ld8(const bf16* p) { return *reinterpret_cast<const bf16x8*>(p); }
MHADA_DEV f32x16 mfma(bf16x8 a, bf16x8 b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
// registers 8 s .. 8 s + 7 of an accumulator tile as the bf16 fragment of k-step s
MHADA_DEV bf16x8 pack8(const f32x16& x, int s) {
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (bf16)x[8 * s + j];
  return r;
}

struct TrainBfP {
  const bf16* qb;    // [BH][Nc][64]
  const bf16* qt;    // [BH][64][NcP]   (backward)
  const bf16* kb;    // [BH][Ns][64]
  const bf16* kt;    // [BH][64][NsP]   (backward)
  const bf16* vb;    // [BH][Ns][64]    V'_b = bf16(V')                  (backward)
  const bf16* wb;    // [BH][Ns][64]    hi plane of V'_b^2               (backward)
  const bf16* wl;    // [BH][Ns][64]    lo plane: hi + lo = V'_b^2 exactly (backward)
  const bf16* vt;    // [BH][64][NsP]   V'_b           (forward)
  const bf16* wt;    // [BH][64][NsP]   V'_b^2, hi     (forward)
  const bf16* wtl;   // [BH][64][NsP]   V'_b^2, lo     (forward)
  const bf16* ob;    // [BH][Nc][128]   dM' | dE2', bf16 (hi plane)
  const bf16* ot;    // [BH][128][NcP]  its transpose
  const bf16* otl;   // [BH][128][NcP]  transposed lo plane bf16(dmo - bf16(dmo))
  const float* v;    // [BH][Ns][64] fp32 V' (rounded again for the 2 V'_b factor of dV')
  const float* x;    // [BH][Nc][64] InstanceNorm(fcs)
  float* out;        // [BH][Nc][64]
  float* mo;         // [BH][Nc][128]  M' | E2'
  float* lse;        // [BH][Nc]       log2 units
  const float* dd;   // [BH][Nc]       D_row = sum_c bf16(dmo) mo (the pre-pass)
  float* dq;         // [BH][Nc][64]
  float* dk;         // [BH][Ns][64]
  float* dv;         // [BH][Ns][64]
  int Nc, Ns, NcP, NsP, nb, nblk;  // NxP = ceil64(Nx); nb = row blocks per (b, h)
};

// Register-staged copy of the ROWS x COLS bf16 tile at (r0, c0) of a [nrows][ld] matrix (rows past
// nrows zero; the columns must exist) into an LDS tile of rows padded to COLS + 8 elements (16-byte
// aligned rows, 4 dwords mod 32 apart): load() issues the global reads one tile ahead, store()
// writes them after the current tile's math.  Row offsets are 64-bit.
template <int ROWS, int COLS>
struct Tile {
  static constexpr int CPR = COLS / 8;         // 16-B chunks per row
  static constexpr int N = ROWS * CPR / NT;    // chunks per thread
  static constexpr int LD = COLS + 8;
  static_assert(N * NT == ROWS * CPR, "tile must divide evenly");
  bf16x8 r[N];
  MHADA_DEV void load(const bf16* g, long long ld, int r0, int nrows, int c0, int tid) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int c = tid + NT * i, row = c / CPR, col = (c % CPR) * 8, gr = r0 + row;
      if (gr < nrows) {
        r[i] = ld8(g + (long long)gr * ld + c0 + col);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) r[i][e] = (bf16)0.0f;
      }
    }
  }
  MHADA_DEV void store(bf16* s, int tid) const {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int c = tid + NT * i, row = c / CPR, col = (c % CPR) * 8;
      *reinterpret_cast<bf16x8*>(s + row * LD + col) = r[i];
    }
  }
};

// The lane's four fragments of row `row` of a bf16 [n][ld] matrix, columns c0 .. c0 + 63:
// f[s] = g[row][c0 + 16 s + 8 h ..] (zeros if !valid).
MHADA_DEV void load_frags(bf16x8 (&f)[4], const bf16* g, long long ld, int row, bool valid, int c0, int h) {
  const bf16* p = g + (long long)(valid ? row : 0) * ld + c0 + 8 * h;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const bf16x8 t = ld8(p + 16 * s);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[s][e] = valid ? t[e] : (bf16)0.0f;
  }
}

// rows (32 x 64 block at row r0 of an LDS row image, stride LD) x the lane's fragments
MHADA_DEV f32x16 rows_dot(const bf16* s, int LD, int r0, int c0, const bf16x8 (&f)[4], f32x16 acc, int h, int r32) {
  const bf16* row = s + (r0 + r32) * LD + c0 + 8 * h;
#pragma unroll
  for (int i = 0; i < 4; ++i) acc = mfma(ld8(row + 16 * i), f[i], acc);
  return acc;
}

// accumulator blocks b = 0, 1 of a lane hold columns 32 b + 8 g + 4 h + e in register 4 g + e
MHADA_DEV void store_blocks(float* row, const f32x16 (&A)[2], int h) {
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      st4(row + 32 * b + 8 * g + 4 * h, f32x4{A[b][4 * g], A[b][4 * g + 1], A[b][4 * g + 2], A[b][4 * g + 3]});
}

// ---------------------------------------------------------------------------------------
// pre-pass: fp32 [BH][n][W] -> bf16 images in the workspace, any subset of
//   rows [BH][n][W]: x_b = bf16(x);  cols [BH][W][nP]: its transpose (nP = ceil64(n), padding zero,
//   32-row groups in the packed-accumulator order);  cols_lo: bf16(x - x_b), the low plane of a
//   hi / lo pair;  rows_sq / rows_sq_lo, cols_sq / cols_sq_lo: the hi / lo pair of x_b^2, which is
//   EXACT (x_b has 8 significant bits, x_b^2 16: hi = bf16(x_b^2), lo = x_b^2 - hi);
//   dd [BH][n] = sum_c x_b[row][c] mo[row][c].
// One workgroup per group of 32 rows.
// ---------------------------------------------------------------------------------------
struct CvtP {
  const float* src;
  bf16 *rows, *cols, *cols_lo, *rows_sq, *rows_sq_lo, *cols_sq, *cols_sq_lo;
  const float* mo;
  float* dd;
  int n, nP;
};

struct Planes {
  bf16 b, lo, sq, sq_lo;
};
MHADA_DEV Planes planes(float t) {
  Planes r;
  r.b = (bf16)t;
  const float tb = (float)r.b, q = tb * tb;
  r.lo = (bf16)(t - tb);
  r.sq = (bf16)q;
  r.sq_lo = (bf16)(q - (float)r.sq);
  return r;
}

template <int W>
__global__ void __launch_bounds__(NT) cvt_bf16_kernel(const CvtP p) {
  __shared__ float sT[32][W + 1];
  const int n = p.n, nP = p.nP, ngrp = nP / 32;
  const long long bh = blockIdx.x / ngrp;
  const int g0 = (blockIdx.x % ngrp) * 32, tid = threadIdx.x;
  const float* sb = p.src + bh * n * W;
  for (int i = tid; i < 32 * W / 4; i += NT) {
    const int row = i / (W / 4), c4 = (i % (W / 4)) * 4, gr = g0 + row;
    const f32x4 t = gr < n ? ld4(sb + (long long)gr * W + c4) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) sT[row][c4 + e] = t[e];
  }
  __syncthreads();
  if (p.rows || p.rows_sq) {
    for (int i = tid; i < 32 * W / 8; i += NT) {
      const int row = i / (W / 8), c8 = (i % (W / 8)) * 8, gr = g0 + row;
      if (gr >= n) continue;
      bf16x8 a, b, bl;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const Planes t = planes(sT[row][c8 + e]);
        a[e] = t.b;
        b[e] = t.sq;
        bl[e] = t.sq_lo;
      }
      const long long o = (bh * n + gr) * W + c8;
      if (p.rows) *reinterpret_cast<bf16x8*>(p.rows + o) = a;
      if (p.rows_sq) *reinterpret_cast<bf16x8*>(p.rows_sq + o) = b;
      if (p.rows_sq_lo) *reinterpret_cast<bf16x8*>(p.rows_sq_lo + o) = bl;
    }
  }
  if (p.dd) {  // D_row = sum_c bf16(src[row][c]) * mo[row][c]: 8 threads per row, W / 8 columns each
    const int row = tid >> 3, c0 = (tid & 7) * (W / 8), gr = g0 + row;
    float acc = 0.f;
    if (gr < n) {
      const float* mr = p.mo + (bh * n + gr) * W + c0;
#pragma unroll
      for (int i = 0; i < W / 32; ++i) {
        const f32x4 m4 = ld4(mr + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = fmaf((float)(bf16)sT[row][c0 + 4 * i + e], m4[e], acc);
      }
    }
    acc += __shfl_xor(acc, 1, 64);
    acc += __shfl_xor(acc, 2, 64);
    acc += __shfl_xor(acc, 4, 64);
    if ((tid & 7) == 0 && gr < n) p.dd[bh * n + gr] = acc;
  }
  if (p.cols || p.cols_sq) {
    for (int i = tid; i < W * 4; i += NT) {
      const int c = i / 4, ch = i % 4, s = ch >> 1, hh = ch & 1;
      bf16x8 a, al, b, bl;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const Planes t = planes(sT[16 * s + 8 * (j >> 2) + 4 * hh + (j & 3)][c]);
        a[j] = t.b;
        al[j] = t.lo;
        b[j] = t.sq;
        bl[j] = t.sq_lo;
      }
      const long long o = (bh * W + c) * nP + g0 + 8 * ch;
      if (p.cols) *reinterpret_cast<bf16x8*>(p.cols + o) = a;
      if (p.cols_lo) *reinterpret_cast<bf16x8*>(p.cols_lo + o) = al;
      if (p.cols_sq) *reinterpret_cast<bf16x8*>(p.cols_sq + o) = b;
      if (p.cols_sq_lo) *reinterpret_cast<bf16x8*>(p.cols_sq_lo + o) = bl;
    }
  }
}

// S^T (keys x queries) in log2 units of key block kb of the staged K tile; keys past Ns -inf
template <int LD>
MHADA_DEV f32x16 scores_t(const bf16* sK, int kb, const bf16x8 (&qf)[4], int k0, int Ns, int h, int r32) {
  f32x16 S = rows_dot(sK, LD, 32 * kb, 0, qf, f32x16{}, h, r32);
#pragma unroll
  for (int r = 0; r < 16; ++r) S[r] = __fmul_rn(S[r], kLog2e);  // never contracted into the subtraction
  if (k0 + 32 * kb + 32 > Ns) {
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (k0 + 32 * kb + acc_row(r, h) >= Ns) S[r] = -INFINITY;
  }
  return S;
}

// ---------------------------------------------------------------------------------------
// forward: wave = 32 queries (one per lane column), online softmax over TT-key tiles
// ---------------------------------------------------------------------------------------
template <int TT>
__global__ void __launch_bounds__(NT, 2) attn_train_fwd_bf16_kernel(const TrainBfP p) {
  constexpr int KB = TT / 32;
  using TK = Tile<TT, 64>;
  using TV = Tile<64, TT>;
  __shared__ __attribute__((aligned(16))) bf16 sK[2][TT * TK::LD];
  __shared__ __attribute__((aligned(16))) bf16 sV[2][64 * TV::LD];
  __shared__ __attribute__((aligned(16))) bf16 sW[2][64 * TV::LD];
  __shared__ __attribute__((aligned(16))) bf16 sX[2][64 * TV::LD];  // lo plane of V'_b^2
  const int t0 = xcd_remap(blockIdx.x, p.nblk);
  const long long bh = t0 / p.nb;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, r32 = lane & 31;
  const int q = (t0 % p.nb) * 32 * kNW + wave * 32 + r32;
  const bool qv = q < p.Nc;
  bf16x8 qf[4];
  load_frags(qf, p.qb + bh * p.Nc * 64, 64, q, qv, 0, h);
  const bf16* kb_ = p.kb + bh * p.Ns * 64;
  const bf16* vt = p.vt + bh * 64 * p.NsP;
  const bf16* wt = p.wt + bh * 64 * p.NsP;
  const bf16* wtl = p.wtl + bh * 64 * p.NsP;

  f32x16 O[4];  // blocks 0, 1: sum p v'_b (channels 0-31, 32-63); 2, 3: sum p v'_b^2 (hi + lo planes: exact squares)
#pragma unroll
  for (int i = 0; i < 4; ++i) O[i] = f32x16{};
  float m = -INFINITY, l = 0.f;
  TK gk;
  TV gv, gw, gx;
  gk.load(kb_, 64, 0, p.Ns, 0, tid);
  gv.load(vt, p.NsP, 0, 64, 0, tid);
  gw.load(wt, p.NsP, 0, 64, 0, tid);
  gx.load(wtl, p.NsP, 0, 64, 0, tid);
  gk.store(sK[0], tid);
  gv.store(sV[0], tid);
  gw.store(sW[0], tid);
  gx.store(sX[0], tid);
  __syncthreads();
  const int nt = (p.Ns + TT - 1) / TT;
  for (int t = 0; t < nt; ++t) {
    const int k0 = t * TT, cb = t & 1;
    const bool nxt = t + 1 < nt;
    if (nxt) {
      gk.load(kb_, 64, k0 + TT, p.Ns, 0, tid);
      gv.load(vt, p.NsP, 0, 64, k0 + TT, tid);
      gw.load(wt, p.NsP, 0, 64, k0 + TT, tid);
      gx.load(wtl, p.NsP, 0, 64, k0 + TT, tid);
    }
    f32x16 S[KB];
    float mx = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      S[kb] = scores_t<TK::LD>(sK[cb], kb, qf, k0, p.Ns, h, r32);
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, S[kb][r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    if (__any(mx > m)) {  // exact online softmax: rescale whenever the running max moves
      const float mn = fmaxf(m, mx);
      const float alpha = __builtin_amdgcn_exp2f(m - mn);
      l *= alpha;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) O[i][e] *= alpha;
      m = mn;
    }
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        S[kb][r] = __builtin_amdgcn_exp2f(S[kb][r] - m);
        l += S[kb][r];
      }
      // O^T (c x queries) += V'^T (c x keys) . P^T (keys x queries); blocks 2, 3 take V'^2
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf16x8 pf = pack8(S[kb], s);
        const int o = r32 * TV::LD + 32 * kb + 16 * s + 8 * h;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          O[b] = mfma(ld8(sV[cb] + o + 32 * b * TV::LD), pf, O[b]);
          O[2 + b] = mfma(ld8(sW[cb] + o + 32 * b * TV::LD), pf, O[2 + b]);
          O[2 + b] = mfma(ld8(sX[cb] + o + 32 * b * TV::LD), pf, O[2 + b]);
        }
      }
    }
    if (nxt) {
      gk.store(sK[cb ^ 1], tid);
      gv.store(sV[cb ^ 1], tid);
      gw.store(sW[cb ^ 1], tid);
      gx.store(sX[cb ^ 1], tid);
    }
    __syncthreads();
  }
  l += __shfl_xor(l, 32, 64);
  if (!qv) return;
  const float inv = 1.0f / l;
  const long long row = bh * p.Nc + q;
  const float* xr = p.x + row * 64;
  float* orow = p.out + row * 64;
  float* mrow = p.mo + row * 128;
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int c0 = 32 * b + 8 * g + 4 * h;
      const f32x4 xx = ld4(xr + c0);
      f32x4 o, mm, ee;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float m1 = O[b][4 * g + e] * inv;
        const float e2 = O[2 + b][4 * g + e] * inv;
        o[e] = sqrtf(fmaxf(e2 - m1 * m1, 1e-6f)) * xx[e] + m1;
        mm[e] = m1;
        ee[e] = e2;
      }
      st4(orow + c0, o);
      st4(mrow + c0, mm);
      st4(mrow + 64 + c0, ee);
    }
  if (h == 0) p.lse[row] = m + __log2f(l);
}

// ---------------------------------------------------------------------------------------
// dQ: wave = 32 queries; streams TT-key tiles of K, K^T, V', V'^2
// ---------------------------------------------------------------------------------------
template <int TT>
__global__ void __launch_bounds__(NT, 2) attn_train_dq_bf16_kernel(const TrainBfP p) {
  constexpr int KB = TT / 32;
  using TK = Tile<TT, 64>;
  using TKt = Tile<64, TT>;
  __shared__ __attribute__((aligned(16))) bf16 sK[2][TT * TK::LD];
  __shared__ __attribute__((aligned(16))) bf16 sV[2][TT * TK::LD];
  __shared__ __attribute__((aligned(16))) bf16 sW[2][TT * TK::LD];
  __shared__ __attribute__((aligned(16))) bf16 sX[2][TT * TK::LD];  // lo plane of V'_b^2
  __shared__ __attribute__((aligned(16))) bf16 sKt[2][64 * TKt::LD];
  const int t0 = xcd_remap(blockIdx.x, p.nblk);
  const long long bh = t0 / p.nb;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, r32 = lane & 31;
  const int q = (t0 % p.nb) * 32 * kNW + wave * 32 + r32;
  const bool qv = q < p.Nc;
  const long long row = bh * p.Nc + (qv ? q : 0);
  bf16x8 qf[4], dm[4], de[4];
  load_frags(qf, p.qb + bh * p.Nc * 64, 64, q, qv, 0, h);
  load_frags(dm, p.ob + bh * p.Nc * 128, 128, q, qv, 0, h);
  load_frags(de, p.ob + bh * p.Nc * 128, 128, q, qv, 64, h);
  const float L = qv ? p.lse[row] : INFINITY;  // invalid query: P = 0
  const float Dr = qv ? p.dd[row] : 0.f;
  const bf16* kb_ = p.kb + bh * p.Ns * 64;
  const bf16* vb = p.vb + bh * p.Ns * 64;
  const bf16* wb = p.wb + bh * p.Ns * 64;
  const bf16* wl = p.wl + bh * p.Ns * 64;
  const bf16* kt = p.kt + bh * 64 * p.NsP;
  f32x16 dQ[2] = {f32x16{}, f32x16{}};
  TK gk, gv, gw, gx;
  TKt gt;
  auto load = [&](int k0) {
    gk.load(kb_, 64, k0, p.Ns, 0, tid);
    gv.load(vb, 64, k0, p.Ns, 0, tid);
    gw.load(wb, 64, k0, p.Ns, 0, tid);
    gx.load(wl, 64, k0, p.Ns, 0, tid);
    gt.load(kt, p.NsP, 0, 64, k0, tid);
  };
  auto store = [&](int buf) {
    gk.store(sK[buf], tid);
    gv.store(sV[buf], tid);
    gw.store(sW[buf], tid);
    gx.store(sX[buf], tid);
    gt.store(sKt[buf], tid);
  };
  load(0);
  store(0);
  __syncthreads();
  const int nt = (p.Ns + TT - 1) / TT;
  for (int t = 0; t < nt; ++t) {
    const int k0 = t * TT, cb = t & 1;
    const bool nxt = t + 1 < nt;
    if (nxt) load(k0 + TT);
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      const f32x16 S = scores_t<TK::LD>(sK[cb], kb, qf, k0, p.Ns, h, r32);
      // dA^T (keys x queries) = [V'_b | V'_b^2] (keys x 128) . [dM' | dE2']^T, the squares as hi + lo
      f32x16 dA = rows_dot(sV[cb], TK::LD, 32 * kb, 0, dm, f32x16{}, h, r32);
      dA = rows_dot(sW[cb], TK::LD, 32 * kb, 0, de, dA, h, r32);
      dA = rows_dot(sX[cb], TK::LD, 32 * kb, 0, de, dA, h, r32);
      f32x16 dS;
#pragma unroll
      for (int r = 0; r < 16; ++r) dS[r] = __builtin_amdgcn_exp2f(S[r] - L) * (dA[r] - Dr);
      // dQ^T (d x queries) += K^T (d x keys) . dS^T (keys x queries)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf16x8 sf = pack8(dS, s);
        const int o = r32 * TKt::LD + 32 * kb + 16 * s + 8 * h;
#pragma unroll
        for (int b = 0; b < 2; ++b) dQ[b] = mfma(ld8(sKt[cb] + o + 32 * b * TKt::LD), sf, dQ[b]);
      }
    }
    if (nxt) store(cb ^ 1);
    __syncthreads();
  }
  if (!qv) return;
  store_blocks(p.dq + row * 64, dQ, h);
}

// ---------------------------------------------------------------------------------------
// dK, dV': wave = 32 keys (one per lane column); streams TT-query tiles of Q, Q^T, dmo, dmo^T,
// lse2, D_row
// ---------------------------------------------------------------------------------------
template <int TT>
__global__ void __launch_bounds__(NT, 1) attn_train_dkv_bf16_kernel(const TrainBfP p) {
  constexpr int QB = TT / 32;
  using TQ = Tile<TT, 64>;
  using TQt = Tile<64, TT>;
  using TO = Tile<TT, 128>;
  using TOt = Tile<128, TT>;
  __shared__ __attribute__((aligned(16))) bf16 sQ[2][TT * TQ::LD];
  __shared__ __attribute__((aligned(16))) bf16 sQt[2][64 * TQt::LD];
  __shared__ __attribute__((aligned(16))) bf16 sO[2][TT * TO::LD];
  __shared__ __attribute__((aligned(16))) bf16 sOt[2][128 * TOt::LD];
  __shared__ __attribute__((aligned(16))) bf16 sOl[2][128 * TOt::LD];  // lo plane of dmo^T
  __shared__ float sL[2][TT], sD[2][TT];
  const int t0 = xcd_remap(blockIdx.x, p.nblk);
  const long long bh = t0 / p.nb;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, r32 = lane & 31;
  const int key = (t0 % p.nb) * 32 * kNW + wave * 32 + r32;
  const bool kv = key < p.Ns;
  bf16x8 kf[4], vf[4], wf[4], xf[4];
  load_frags(kf, p.kb + bh * p.Ns * 64, 64, key, kv, 0, h);
  load_frags(vf, p.vb + bh * p.Ns * 64, 64, key, kv, 0, h);
  load_frags(wf, p.wb + bh * p.Ns * 64, 64, key, kv, 0, h);
  load_frags(xf, p.wl + bh * p.Ns * 64, 64, key, kv, 0, h);
  const bf16* qb_ = p.qb + bh * p.Nc * 64;
  const bf16* qt = p.qt + bh * 64 * p.NcP;
  const bf16* ob = p.ob + bh * p.Nc * 128;
  const bf16* ot = p.ot + bh * 128 * p.NcP;
  const bf16* otl = p.otl + bh * 128 * p.NcP;
  const float* lb = p.lse + bh * p.Nc;
  const float* db = p.dd + bh * p.Nc;
  f32x16 G1[2], G2[2], dK[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) G1[i] = G2[i] = dK[i] = f32x16{};
  TQ gq;
  TQt gqt;
  TO go;
  TOt got, gol;
  float gl = INFINITY, gd = 0.f;
  auto load = [&](int q0) {
    gq.load(qb_, 64, q0, p.Nc, 0, tid);
    gqt.load(qt, p.NcP, 0, 64, q0, tid);
    go.load(ob, 128, q0, p.Nc, 0, tid);
    got.load(ot, p.NcP, 0, 128, q0, tid);
    gol.load(otl, p.NcP, 0, 128, q0, tid);
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
    gqt.store(sQt[buf], tid);
    go.store(sO[buf], tid);
    got.store(sOt[buf], tid);
    gol.store(sOl[buf], tid);
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
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
      // S (queries x keys) = Q . K^T, dA (queries x keys) = [dM' | dE2'] . [V' | V'^2]^T
      const f32x16 S = rows_dot(sQ[cb], TQ::LD, 32 * qb, 0, kf, f32x16{}, h, r32);
      f32x16 dA = rows_dot(sO[cb], TO::LD, 32 * qb, 0, vf, f32x16{}, h, r32);
      dA = rows_dot(sO[cb], TO::LD, 32 * qb, 64, wf, dA, h, r32);
      dA = rows_dot(sO[cb], TO::LD, 32 * qb, 64, xf, dA, h, r32);
      f32x16 P, dS;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qi = 32 * qb + acc_row(r, h);
        P[r] = __builtin_amdgcn_exp2f(__fmul_rn(S[r], kLog2e) - sL[cb][qi]);
        dS[r] = P[r] * (dA[r] - sD[cb][qi]);
      }
      // G1^T, G2^T (c x keys) += [dM' | dE2']^T (c x queries) . P with dmo as hi + lo planes: in
      // dV' = G1 + 2 V'_b G2 the two terms cancel on peaked rows (dM' = dout - 2 M' dVar against
      // 2 V'_b dVar with V'_b ~ M'), so their operands carry 16 bits;  dK^T (d x keys) += Q^T . dS
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf16x8 pf = pack8(P, s), sf = pack8(dS, s);
        const int c0 = 32 * qb + 16 * s + 8 * h;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          G1[b] = mfma(ld8(sOt[cb] + (32 * b + r32) * TOt::LD + c0), pf, G1[b]);
          G1[b] = mfma(ld8(sOl[cb] + (32 * b + r32) * TOt::LD + c0), pf, G1[b]);
          G2[b] = mfma(ld8(sOt[cb] + (64 + 32 * b + r32) * TOt::LD + c0), pf, G2[b]);
          G2[b] = mfma(ld8(sOl[cb] + (64 + 32 * b + r32) * TOt::LD + c0), pf, G2[b]);
          dK[b] = mfma(ld8(sQt[cb] + (32 * b + r32) * TQt::LD + c0), sf, dK[b]);
        }
      }
    }
    if (nxt) store(cb ^ 1);
    lds_barrier();
  }
  if (!kv) return;
  const long long row = bh * p.Ns + key;
  const float* vg = p.v + row * 64;
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 vv = ld4(vg + 32 * b + 8 * g + 4 * h);
#pragma unroll
      for (int e = 0; e < 4; ++e) G1[b][4 * g + e] += 2.0f * (float)(bf16)vv[e] * G2[b][4 * g + e];  // d(V'_b^2) = 2 V'_b
    }
  store_blocks(p.dv + row * 64, G1, h);
  store_blocks(p.dk + row * 64, dK, h);
}

constexpr int kTTFwd = 64, kTTDq = 32, kTTDkv = 32;

// rows and tiles are indexed in int (row offsets are 64-bit): n + 32 * kNW must not wrap
constexpr int kMaxRows = 1 << 30;

long long ceil64(long long n) { return (n + 63) / 64 * 64; }
long long seg(long long elems) { return (elems * 2 + 255) / 256 * 256; }  // bytes of a bf16 image, 256-B aligned

bool set_grid(TrainBfP& p, long long BH, int n) {
  p.nb = (n + 32 * kNW - 1) / (32 * kNW);
  const long long nblk = BH * p.nb;
  if (nblk > (1LL << 31) - 1) return false;
  p.nblk = (int)nblk;
  return true;
}

// one pre-pass launch; false if the grid does not fit
bool cvt(CvtP c, long long BH, int n, int W, hipStream_t s) {
  if (n == 0) return true;
  c.n = n;
  c.nP = (int)ceil64(n);
  const long long nblk = BH * (c.nP / 32);
  if (nblk > (1LL << 31) - 1) return false;
  if (W == 64) hipLaunchKernelGGL((cvt_bf16_kernel<64>), dim3((unsigned)nblk), dim3(NT), 0, s, c);
  else hipLaunchKernelGGL((cvt_bf16_kernel<128>), dim3((unsigned)nblk), dim3(NT), 0, s, c);
  return true;
}

long long ws_bytes(long long BH, long long Nc, long long Ns, bool backward) {
  const long long qb = seg(BH * Nc * 64), kb = seg(BH * Ns * 64), kt = seg(BH * 64 * ceil64(Ns));
  if (!backward) return qb + kb + 3 * kt;  // Q | K | V'^T | V'^2^T hi | V'^2^T lo
  const long long qt = seg(BH * 64 * ceil64(Nc)), ot = seg(BH * 128 * ceil64(Nc));
  // Q Q^T K K^T V' V'^2 hi, lo dmo dmo^T hi, lo D_row (fp32: two bf16 slots per element)
  return qb + qt + kb + kt + 3 * kb + seg(BH * Nc * 128) + 2 * ot + seg(BH * Nc * 2);
}

}  // namespace
}  // namespace mhada

using namespace mhada;

extern "C" long long mhada_attn_train_bf16_workspace(int BH, int Nc, int Ns, int backward) {
  if (BH <= 0 || Nc < 0 || Ns <= 0 || Nc > kMaxRows || Ns > kMaxRows) {
    fail("mhada_attn_train_bf16_workspace: bad args");
    return -1;
  }
  return ws_bytes(BH, Nc, Ns, backward != 0);
}

extern "C" int mhada_attn_train_fwd_bf16(const float* q, const float* k, const float* v, const float* x, float* out,
                                         float* mo, float* lse, void* ws, long long ws_size, int BH, int Nc, int Ns,
                                         mhada_stream_t s_) {
  if (!q || !k || !v || !x || !out || !mo || !lse || !ws || BH <= 0 || Nc < 0 || Ns <= 0)
    return fail("mhada_attn_train_fwd_bf16: bad args");
  if (Nc > kMaxRows || Ns > kMaxRows) return fail("mhada_attn_train_fwd_bf16: Nc, Ns above 2^30");
  if ((uintptr_t)ws % 16 || ws_size < ws_bytes(BH, Nc, Ns, false))
    return fail("mhada_attn_train_fwd_bf16: workspace unaligned or smaller than mhada_attn_train_bf16_workspace");
  if (Nc == 0) return MHADA_OK;
  const hipStream_t s = (hipStream_t)s_;
  TrainBfP p = {};
  char* w = static_cast<char*>(ws);
  bf16* qb = reinterpret_cast<bf16*>(w);  w += seg((long long)BH * Nc * 64);
  bf16* kb = reinterpret_cast<bf16*>(w);  w += seg((long long)BH * Ns * 64);
  bf16* vt = reinterpret_cast<bf16*>(w);  w += seg((long long)BH * 64 * ceil64(Ns));
  bf16* wt = reinterpret_cast<bf16*>(w);  w += seg((long long)BH * 64 * ceil64(Ns));
  bf16* wtl = reinterpret_cast<bf16*>(w);
  p.qb = qb; p.kb = kb; p.vt = vt; p.wt = wt; p.wtl = wtl; p.x = x; p.out = out; p.mo = mo; p.lse = lse;
  p.Nc = Nc; p.Ns = Ns; p.NcP = (int)ceil64(Nc); p.NsP = (int)ceil64(Ns);
  CvtP cq = {}, ck = {}, cv = {};
  cq.src = q; cq.rows = qb;
  ck.src = k; ck.rows = kb;
  cv.src = v; cv.cols = vt; cv.cols_sq = wt; cv.cols_sq_lo = wtl;
  if (!set_grid(p, BH, Nc) || !cvt(cq, BH, Nc, 64, s) || !cvt(ck, BH, Ns, 64, s) || !cvt(cv, BH, Ns, 64, s))
    return fail("mhada_attn_train_fwd_bf16: grid too large");
  hipLaunchKernelGGL((attn_train_fwd_bf16_kernel<kTTFwd>), dim3(p.nblk), dim3(NT), 0, s, p);
  return check_launch("mhada_attn_train_fwd_bf16");
}

extern "C" int mhada_attn_train_bwd_bf16(const float* q, const float* k, const float* v, const float* lse,
                                         const float* dmo, const float* mo, float* dq, float* dk, float* dv, void* ws,
                                         long long ws_size, int BH, int Nc, int Ns, int phases, mhada_stream_t s_) {
  const bool pre = phases & 1, run = phases & 2;  // 1: the pre-pass into ws, 2: the kernels on a filled ws
  if (phases < 1 || phases > 3) return fail("mhada_attn_train_bwd_bf16: bad args (phases must be 1, 2 or 3)");
  if (!q || !k || !v || !ws || BH <= 0 || Nc < 0 || Ns <= 0 || (pre && (!dmo || !mo)) ||
      (run && (!lse || !dq || !dk || !dv)))
    return fail("mhada_attn_train_bwd_bf16: bad args");
  if (Nc > kMaxRows || Ns > kMaxRows) return fail("mhada_attn_train_bwd_bf16: Nc, Ns above 2^30");
  if ((uintptr_t)ws % 16 || ws_size < ws_bytes(BH, Nc, Ns, true))
    return fail("mhada_attn_train_bwd_bf16: workspace unaligned or smaller than mhada_attn_train_bf16_workspace");
  const hipStream_t s = (hipStream_t)s_;
  if (Nc == 0) {  // no query: dK = dV' = 0
    if (!run) return MHADA_OK;
    const size_t n = (size_t)BH * Ns * 64 * sizeof(float);
    if (hipMemsetAsync(dk, 0, n, s) != hipSuccess || hipMemsetAsync(dv, 0, n, s) != hipSuccess)
      return check_launch("mhada_attn_train_bwd_bf16");
    return MHADA_OK;
  }
  TrainBfP p = {};
  char* w = static_cast<char*>(ws);
  bf16* qb = reinterpret_cast<bf16*>(w);  w += seg((long long)BH * Nc * 64);
  bf16* qt = reinterpret_cast<bf16*>(w);  w += seg((long long)BH * 64 * ceil64(Nc));
  bf16* kb = reinterpret_cast<bf16*>(w);  w += seg((long long)BH * Ns * 64);
  bf16* kt = reinterpret_cast<bf16*>(w);  w += seg((long long)BH * 64 * ceil64(Ns));
  bf16* vb = reinterpret_cast<bf16*>(w);  w += seg((long long)BH * Ns * 64);
  bf16* wb = reinterpret_cast<bf16*>(w);  w += seg((long long)BH * Ns * 64);
  bf16* wl = reinterpret_cast<bf16*>(w);  w += seg((long long)BH * Ns * 64);
  bf16* ob = reinterpret_cast<bf16*>(w);  w += seg((long long)BH * Nc * 128);
  bf16* ot = reinterpret_cast<bf16*>(w);  w += seg((long long)BH * 128 * ceil64(Nc));
  bf16* otl = reinterpret_cast<bf16*>(w);  w += seg((long long)BH * 128 * ceil64(Nc));
  float* dd = reinterpret_cast<float*>(w);
  p.qb = qb; p.qt = qt; p.kb = kb; p.kt = kt; p.vb = vb; p.wb = wb; p.wl = wl; p.ob = ob; p.ot = ot; p.otl = otl;
  p.v = v; p.lse = const_cast<float*>(lse); p.dd = dd; p.dq = dq; p.dk = dk; p.dv = dv;
  p.Nc = Nc; p.Ns = Ns; p.NcP = (int)ceil64(Nc); p.NsP = (int)ceil64(Ns);
  CvtP cq = {}, ck = {}, cv = {}, co = {};
  cq.src = q; cq.rows = qb; cq.cols = qt;
  ck.src = k; ck.rows = kb; ck.cols = kt;
  cv.src = v; cv.rows = vb; cv.rows_sq = wb; cv.rows_sq_lo = wl;
  co.src = dmo; co.rows = ob; co.cols = ot; co.cols_lo = otl; co.mo = mo; co.dd = dd;
  if (pre && (!cvt(cq, BH, Nc, 64, s) || !cvt(ck, BH, Ns, 64, s) || !cvt(cv, BH, Ns, 64, s) ||
              !cvt(co, BH, Nc, 128, s)))
    return fail("mhada_attn_train_bwd_bf16: grid too large");
  if (!run) return check_launch("mhada_attn_train_bwd_bf16");
  if (!set_grid(p, BH, Nc)) return fail("mhada_attn_train_bwd_bf16: grid too large");
  hipLaunchKernelGGL((attn_train_dq_bf16_kernel<kTTDq>), dim3(p.nblk), dim3(NT), 0, s, p);
  if (!set_grid(p, BH, Ns)) return fail("mhada_attn_train_bwd_bf16: grid too large");
  hipLaunchKernelGGL((attn_train_dkv_bf16_kernel<kTTDkv>), dim3(p.nblk), dim3(NT), 0, s, p);
  return check_launch("mhada_attn_train_bwd_bf16");
}
