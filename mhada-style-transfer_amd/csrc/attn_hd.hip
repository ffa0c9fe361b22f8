// MHAda inference at head widths D = 32 and D = 128 (16 and 4 heads at 512 channels): the fused
// attention, the weight fold, the cosine row normalisation and the ViT's batch-axis attention.
// The D = 64 kernels (attn.hip, attn_split3.hip, cosine.hip, small_ops.hip) are untouched; this
// file serves only the other two widths.
//
// mhada_attn_hd: mhada_attn's contract and output formula (adaDecoder.py:186-198) with 64 -> D,
// modelled on the general kernels attn_f32_kernel / attn_bf16_kernel of attn.hip:
//   * swapped products: S^T (keys x queries) = K . Q^T with the query on the MFMA lane (row max /
//     sum lane-local plus one cross-half shuffle), O^T (dv x queries) = V'^T . P^T with the S^T
//     accumulator itself as the B operand;
//   * online max with the deferred rescale (kRescaleThr), a wave-uniform branch inside one loop;
//   * only the last, partial key tile runs the masking code;
//   * the blocks of one (b, h) are remapped onto one XCD (decode_block).
// Block = 4 waves = 128 queries of one (b, h), each wave 32 queries (lane & 31 = query, lane >> 5
// = h selects the reduction half).  Both dtypes read kv [B][H][Ns][2D] (K | V') directly; there is
// no transposed image and nothing to cache beside kv.
// mhada_attn_hd_shared (clips: B frames against ONE style): the same kernels with kAttnShared
// (attn_common.h) in the ACT parameter, ACTF = ACT | kAttnShared: kv [H][Ns][2D] and v_mu [D H] are
// read at head hh for every frame b; everything else, the launch geometry included, is unchanged.
//
// fp32 (v_mfma_f32_32x32x2_f32, exact fp32): key tiles of TK = 64 (D = 32) / 32 (D = 128) whole kv
//   rows, register-staged into a double-buffered LDS image sKV[2][TK][2D + 4] (rows padded by 16 B:
//   conflict-free 16-B reads down a key column).  QK step s takes d = (D/2) h + s: the Q^T operand
//   is D/2 registers per lane, the K operand 16-B reads along a key row.  PV step r of key block kb
//   takes key 32 kb + (r & 3) + 8 (r >> 2) + 4 h (the accumulator row of P^T): V' is one 4-B read
//   sKV[key][D + 32 blk + lane & 31] per dv block, V'^2 its square formed in the register.
// bf16 (v_mfma_f32_32x32x16_bf16, fp32 accumulation and softmax): key tiles of TK = 128 (D = 32) /
//   64 (D = 128).  K rows go to sK[2][TK][D + 8]; V' is transposed on its way into LDS,
//   sV[2][2D][TK + 8] = V'^T (rows 0 .. D-1) | V'^2^T (rows D .. 2D-1, squared in fp32 and rounded
//   once, as mhada_transpose_v does), with the keys of each group of 16 stored at position
//   pos(n) = n with bits 2 and 3 swapped, so the 8 keys 16 s + 8 (j >> 2) + 4 h + (j & 3) of one
//   lane half's B slots are one 16-B read at 16 s + 8 h.  A thread stages the same 8 dv of two
//   adjacent keys and writes them as 4-B pairs (pos(n + 1) = pos(n) + 1 for even n).
// Accumulators: O[blk], blk < D/32: sum p v' for dv = (r & 3) + 8 (r >> 2) + 4 h + 32 blk;
//   O[D/32 + blk]: sum p v'^2.  D = 128: 128 accumulator registers per lane, one wave per SIMD on
//   the unified register file (__launch_bounds__(256, 1)); D = 32: two workgroups per CU.
// Results are bit-identical from run to run (no atomics, fixed reduction order).
#include "attn_common.h"

namespace mhada {
namespace hd {

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

static bool hd_width(int D) { return D == 32 || D == 128; }

// out = sqrt(max(E2 - M^2, 1e-6)) * IN(fcs) + M + v_mu for the wave's 32 queries.
// SHARED (mhada_attn_hd_shared): v_mu is one style's [C] for every frame b, as attn_epilogue's.
template <typename T, int D, bool SHARED = false>
MHADA_DEV void epilogue(const AttnP& p, const f32x16 (&O)[D / 16], float l, int b, int hh, int q, int h) {
  constexpr int NB = D / 32;
  const int C = p.H * D;
  const float lt = l + __shfl_xor(l, 32, 64);
  if (q >= p.Nc) return;
  const float inv = 1.0f / lt;
  const float* fr = p.fcs + ((long long)b * p.Nc + q) * C + hh * D;
  const float* mu = p.fcs_mu + (long long)b * C + hh * D;
  const float* rs = p.fcs_rstd + (long long)b * C + hh * D;
  const float* vm = p.v_mu + (SHARED ? 0LL : (long long)b * C) + hh * D;
  T* orow = reinterpret_cast<T*>(p.out) + ((long long)b * p.Nc + q) * C + hh * D;
#pragma unroll
  for (int blk = 0; blk < NB; ++blk) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {  // 4 contiguous dv per group
      const int dv0 = 8 * g + 4 * h + 32 * blk;
      const f32x4 f = *reinterpret_cast<const f32x4*>(fr + dv0);
      const f32x4 m4 = *reinterpret_cast<const f32x4*>(mu + dv0);
      const f32x4 r4 = *reinterpret_cast<const f32x4*>(rs + dv0);
      const f32x4 v4 = *reinterpret_cast<const f32x4*>(vm + dv0);
      float res[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float m1 = O[blk][4 * g + e] * inv;
        const float e2 = O[blk + NB][4 * g + e] * inv;
        const float sd = sqrtf(fmaxf(e2 - m1 * m1, 1e-6f));
        res[e] = sd * ((f[e] - m4[e]) * r4[e]) + (m1 + v4[e]);
      }
      if constexpr (sizeof(T) == 4) {
        *reinterpret_cast<f32x4*>(orow + dv0) = f32x4{res[0], res[1], res[2], res[3]};
      } else {
        *reinterpret_cast<bf16x4*>(orow + dv0) = bf16x4{(bf16)res[0], (bf16)res[1], (bf16)res[2], (bf16)res[3]};
      }
    }
  }
}

// ======================================================================================
// fp32
// ======================================================================================
template <int D, int ACTF>
__global__ void __launch_bounds__(256, D == 32 ? 2 : 1) attn_hd_f32_kernel(const AttnP p) {
  constexpr int ACT = ACTF & ~kAttnShared;
  constexpr bool SHARED = (ACTF & kAttnShared) != 0;
  constexpr int NT = 256, NB = D / 32, TK = D == 32 ? 64 : 32, NKB = TK / 32;
  constexpr int LR = 2 * D + 4;           // padded kv row (floats)
  constexpr int CPR = 2 * D / 4;          // 16-B chunks per kv row
  constexpr int CH = TK * CPR / NT;       // chunks per thread per tile
  static_assert(CH >= 1 && TK * CPR % NT == 0, "tile config");
  __shared__ __attribute__((aligned(16))) float sKV[2][TK * LR];
  int b, hh, qb;
  decode_block(p, b, hh, qb);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, r32 = lane & 31;
  const int q = qb * 128 + wave * 32 + r32;
  const long long bh = (long long)b * p.H + hh;

  // Q^T operand: MFMA step s takes d = (D/2) h + s
  float qreg[D / 2];
  {
    const float* qp = reinterpret_cast<const float*>(p.q) + (bh * p.Nc + (q < p.Nc ? q : 0)) * D + (D / 2) * h;
#pragma unroll
    for (int i = 0; i < D / 8; ++i) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(qp + 4 * i);
#pragma unroll
      for (int e = 0; e < 4; ++e) qreg[4 * i + e] = (q < p.Nc) ? t[e] : 0.f;
    }
  }
  const long long sbh = SHARED ? hh : bh;  // the style operands' problem index
  const float* kvb = reinterpret_cast<const float*>(p.kv) + sbh * p.Ns * (2 * D);

  f32x4 st[CH];
  auto issue = [&](int key0) {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = tid + NT * i, row = c / CPR, col = (c % CPR) * 4;
      const int key = key0 + row;
      st[i] = key < p.Ns ? *reinterpret_cast<const f32x4*>(kvb + (long long)key * (2 * D) + col)
                         : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  auto commit = [&](int buf) {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = tid + NT * i, row = c / CPR, col = (c % CPR) * 4;
      *reinterpret_cast<f32x4*>(&sKV[buf][row * LR + col]) = st[i];
    }
  };

  f32x16 O[2 * NB];
#pragma unroll
  for (int i = 0; i < 2 * NB; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) O[i][e] = 0.f;
  float m2 = -INFINITY, l = 0.f;

  auto qk = [&](const float* cur, f32x16 (&S)[NKB]) {
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
#pragma unroll
      for (int e = 0; e < 16; ++e) S[kb][e] = 0.f;
      const float* krow = cur + (kb * 32 + r32) * LR + (D / 2) * h;
#pragma unroll
      for (int i = 0; i < D / 8; ++i) {
        const f32x4 kk = *reinterpret_cast<const f32x4*>(krow + 4 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e)
          S[kb] = __builtin_amdgcn_mfma_f32_32x32x2f32(kk[e], qreg[4 * i + e], S[kb], 0, 0, 0);
      }
    }
  };
  auto pv = [&](const float* cur, const f32x16 (&P)[NKB]) {
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float* vr = cur + (kb * 32 + acc_row(r, h)) * LR + D + r32;
        const float pr = P[kb][r];
#pragma unroll
        for (int blk = 0; blk < NB; ++blk) {
          const float v = vr[32 * blk];
          O[blk] = __builtin_amdgcn_mfma_f32_32x32x2f32(v, pr, O[blk], 0, 0, 0);
          O[NB + blk] = __builtin_amdgcn_mfma_f32_32x32x2f32(v * v, pr, O[NB + blk], 0, 0, 0);
        }
      }
    }
  };

  const int NTILE = (p.Ns + TK - 1) / TK, NFULL = p.Ns / TK;
  issue(0);
  commit(0);
  __syncthreads();
  for (int t = 0; t < NFULL; ++t) {
    const int cb = t & 1;
    const bool nxt = t + 1 < NTILE;
    if (nxt) issue((t + 1) * TK);
    f32x16 S[NKB];
    qk(sKV[cb], S);
    softmax_step<ACT, NKB, 2 * NB>(S, O, m2, l);
    pv(sKV[cb], S);
    if (nxt) commit(cb ^ 1);
    __syncthreads();
  }
  if (NFULL < NTILE) {  // ragged last tile: masked
    const int cb = NFULL & 1;
    f32x16 S[NKB];
    qk(sKV[cb], S);
    mask_tile<ACT, NKB>(S, NFULL * TK, p.Ns, h);
    softmax_step<ACT, NKB, 2 * NB>(S, O, m2, l);
    pv(sKV[cb], S);
  }
  epilogue<float, D, SHARED>(p, O, l, b, hh, q, h);
}

// ======================================================================================
// bf16
// ======================================================================================
template <int D, int ACTF>
__global__ void __launch_bounds__(256, D == 32 ? 2 : 1) attn_hd_bf16_kernel(const AttnP p) {
  constexpr int ACT = ACTF & ~kAttnShared;
  constexpr bool SHARED = (ACTF & kAttnShared) != 0;
  constexpr int NT = 256, NB = D / 32, TK = D == 32 ? 128 : 64, NKB = TK / 32, KS = D / 16;
  constexpr int LK = D + 8;    // K rows: D + 8 bf16 (80 / 272 B): conflict-free 16-B row reads
  constexpr int LV = TK + 8;   // V'^T rows: TK keys + 8 (272 / 144 B): conflict-free
  constexpr int CPR = D / 8;                  // 16-B chunks per K (or V') row
  constexpr int KCH = TK * CPR / NT;          // K chunks per thread per tile
  constexpr int VU = (TK / 2) * CPR / NT;     // V' units (2 keys x 8 dv) per thread per tile
  static_assert(KCH >= 1 && VU >= 1 && TK * CPR % NT == 0 && (TK / 2) * CPR % NT == 0, "tile config");
  __shared__ __attribute__((aligned(16))) bf16 sK[2][TK * LK];
  __shared__ __attribute__((aligned(16))) bf16 sV[2][2 * D * LV];
  int b, hh, qb;
  decode_block(p, b, hh, qb);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, r32 = lane & 31;
  const int q = qb * 128 + wave * 32 + r32;
  const long long bh = (long long)b * p.H + hh;

  // Q^T operand: k-step s takes d = 16s + 8h + j
  bf16x8 qf[KS];
  {
    const bf16* qp = reinterpret_cast<const bf16*>(p.q) + (bh * p.Nc + (q < p.Nc ? q : 0)) * D + 8 * h;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      qf[s] = *reinterpret_cast<const bf16x8*>(qp + 16 * s);
      if (q >= p.Nc) {
#pragma unroll
        for (int e = 0; e < 8; ++e) qf[s][e] = (bf16)0.0f;
      }
    }
  }
  const long long sbh = SHARED ? hh : bh;  // the style operands' problem index
  const bf16* kvb = reinterpret_cast<const bf16*>(p.kv) + sbh * p.Ns * (2 * D);

  bf16x8 sk[KCH], sv[VU][2];
  auto load8 = [&](int key, int col) {
    bf16x8 v;
    if (key < p.Ns) {
      v = *reinterpret_cast<const bf16x8*>(kvb + (long long)key * (2 * D) + col);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (bf16)0.0f;
    }
    return v;
  };
  auto issue = [&](int key0) {
#pragma unroll
    for (int i = 0; i < KCH; ++i) {
      const int c = tid + NT * i;
      sk[i] = load8(key0 + c / CPR, (c % CPR) * 8);
    }
#pragma unroll
    for (int i = 0; i < VU; ++i) {
      const int u = tid + NT * i, kp = u % (TK / 2), col = (u / (TK / 2)) * 8;
      sv[i][0] = load8(key0 + 2 * kp, D + col);
      sv[i][1] = load8(key0 + 2 * kp + 1, D + col);
    }
  };
  auto commit = [&](bf16* dk, bf16* dv) {
#pragma unroll
    for (int i = 0; i < KCH; ++i) {
      const int c = tid + NT * i, row = c / CPR, col = (c % CPR) * 8;
      *reinterpret_cast<bf16x8*>(dk + row * LK + col) = sk[i];
    }
#pragma unroll
    for (int i = 0; i < VU; ++i) {
      const int u = tid + NT * i, n = 2 * (u % (TK / 2)), col = (u / (TK / 2)) * 8;
      const int pos = (n & ~12) | ((n & 4) << 1) | ((n & 8) >> 1);  // bits 2 and 3 swapped
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const bf16 v0 = sv[i][0][e], v1 = sv[i][1][e];
        const float f0 = (float)v0, f1 = (float)v1;
        *reinterpret_cast<bf16x2*>(dv + (col + e) * LV + pos) = bf16x2{v0, v1};
        *reinterpret_cast<bf16x2*>(dv + (D + col + e) * LV + pos) = bf16x2{(bf16)(f0 * f0), (bf16)(f1 * f1)};
      }
    }
  };

  f32x16 O[2 * NB];
#pragma unroll
  for (int i = 0; i < 2 * NB; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) O[i][e] = 0.f;
  float m2 = -INFINITY, l = 0.f;

  auto qk = [&](const bf16* ck, f32x16 (&S)[NKB]) {
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
#pragma unroll
      for (int e = 0; e < 16; ++e) S[kb][e] = 0.f;
      const bf16* krow = ck + (kb * 32 + r32) * LK + 8 * h;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const bf16x8 kk = *reinterpret_cast<const bf16x8*>(krow + 16 * s);
        S[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kk, qf[s], S[kb], 0, 0, 0);
      }
    }
  };
  auto pv = [&](const bf16* cv, const f32x16 (&P)[NKB]) {
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        // B = P^T: element j <-> key kb*32 + 16s + 8(j>>2) + 4h + (j&3) (accumulator regs 8s..8s+7),
        // stored contiguously at key position 16s + 8h of the V'^T rows
        bf16x8 pf;
#pragma unroll
        for (int j = 0; j < 8; ++j) pf[j] = (bf16)P[kb][8 * s + j];
        const bf16* vcol = cv + r32 * LV + kb * 32 + 16 * s + 8 * h;
#pragma unroll
        for (int blk = 0; blk < 2 * NB; ++blk) {  // rows 32 blk: V'^T for blk < NB, V'^2^T above
          const bf16x8 vf = *reinterpret_cast<const bf16x8*>(vcol + 32 * blk * LV);
          O[blk] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf, O[blk], 0, 0, 0);
        }
      }
    }
  };

  const int NTILE = (p.Ns + TK - 1) / TK, NFULL = p.Ns / TK;
  issue(0);
  commit(sK[0], sV[0]);
  __syncthreads();
  for (int t = 0; t < NFULL; ++t) {
    const int cb = t & 1;
    const bool nxt = t + 1 < NTILE;
    if (nxt) issue((t + 1) * TK);
    f32x16 S[NKB];
    qk(sK[cb], S);
    softmax_step<ACT, NKB, 2 * NB>(S, O, m2, l);
    pv(sV[cb], S);
    if (nxt) commit(sK[cb ^ 1], sV[cb ^ 1]);
    __syncthreads();
  }
  if (NFULL < NTILE) {  // ragged last tile: masked
    const int cb = NFULL & 1;
    f32x16 S[NKB];
    qk(sK[cb], S);
    mask_tile<ACT, NKB>(S, NFULL * TK, p.Ns, h);
    softmax_step<ACT, NKB, 2 * NB>(S, O, m2, l);
    pv(sV[cb], S);
  }
  epilogue<bf16, D, SHARED>(p, O, l, b, hh, q, h);
}

// SHARED: the shared-style forms (mhada_attn_hd_shared), the same kernel and grid with kAttnShared in ACTF.
template <int D, bool SHARED = false>
static void launch_attn_hd(const AttnP& p, int dtype, int activation, hipStream_t s) {
  const dim3 grid(p.nblk), blk(256);
  if constexpr (SHARED) {
    constexpr int SM = MHADA_ACT_SOFTMAX | kAttnShared, CS = MHADA_ACT_COSINE | kAttnShared;
    if (dtype == MHADA_F32) {
      if (activation == MHADA_ACT_SOFTMAX) hipLaunchKernelGGL((attn_hd_f32_kernel<D, SM>), grid, blk, 0, s, p);
      else hipLaunchKernelGGL((attn_hd_f32_kernel<D, CS>), grid, blk, 0, s, p);
    } else {
      if (activation == MHADA_ACT_SOFTMAX) hipLaunchKernelGGL((attn_hd_bf16_kernel<D, SM>), grid, blk, 0, s, p);
      else hipLaunchKernelGGL((attn_hd_bf16_kernel<D, CS>), grid, blk, 0, s, p);
    }
  } else if (dtype == MHADA_F32) {
    if (activation == MHADA_ACT_SOFTMAX) hipLaunchKernelGGL((attn_hd_f32_kernel<D, MHADA_ACT_SOFTMAX>), grid, blk, 0, s, p);
    else hipLaunchKernelGGL((attn_hd_f32_kernel<D, MHADA_ACT_COSINE>), grid, blk, 0, s, p);
  } else {
    if (activation == MHADA_ACT_SOFTMAX) hipLaunchKernelGGL((attn_hd_bf16_kernel<D, MHADA_ACT_SOFTMAX>), grid, blk, 0, s, p);
    else hipLaunchKernelGGL((attn_hd_bf16_kernel<D, MHADA_ACT_COSINE>), grid, blk, 0, s, p);
  }
}

// ---------------------------------------------------------------------------------------
// Weight fold (fold_kernel of small_ops.hip with a runtime head width), grid B*H.
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(256) fold_hd_kernel(const float* __restrict__ wf, const float* __restrict__ wg,
                                                      const float* __restrict__ wh, const float* __restrict__ bg,
                                                      const float* __restrict__ bh, const float* __restrict__ rstd_c,
                                                      const float* __restrict__ mu_s, const float* __restrict__ rstd_s,
                                                      T* __restrict__ wq, T* __restrict__ wkv, float* __restrict__ bkv,
                                                      float* __restrict__ v_mu, float kscale, int H, int D) {
  const int b = blockIdx.x / H, hh = blockIdx.x - b * H;
  const int C = H * D;
  const float* rc = rstd_c + (long long)b * C + hh * D;
  const float* rs = rstd_s + (long long)b * C + hh * D;
  const float* ms = mu_s + (long long)b * C + hh * D;
  const float* Wf = wf + (long long)hh * D * D;
  const float* Wg = wg + (long long)hh * D * D;
  const float* Wh = wh + (long long)hh * D * D;
  T* oq = wq + (long long)blockIdx.x * D * D;
  T* okv = wkv + (long long)blockIdx.x * 2 * D * D;
  for (int i = threadIdx.x; i < D * D; i += 256) {
    const int c = i & (D - 1);
    oq[i] = from_f32<T>(Wf[i] * rc[c]);
    okv[i] = from_f32<T>(Wg[i] * rs[c] * kscale);
    okv[D * D + i] = from_f32<T>(Wh[i]);
  }
  if (threadIdx.x < D) {
    const int o = threadIdx.x;
    float acc = bh[hh * D + o];
    for (int c = 0; c < D; ++c) acc += Wh[o * D + c] * ms[c];
    v_mu[(long long)b * C + hh * D + o] = acc;
    if (b == 0) {
      bkv[hh * 2 * D + o] = bg[hh * D + o] * kscale;
      bkv[hh * 2 * D + D + o] = 0.f;
    }
  }
}

// ---------------------------------------------------------------------------------------
// L2-normalise D-wide rows in place (adaDecoder.py:30-32): LP lanes per row, D / LP elements each.
// ---------------------------------------------------------------------------------------
template <typename T, int D>
__global__ void __launch_bounds__(256) rownorm_hd_kernel(T* __restrict__ x, long long rows, int ld) {
  constexpr int LP = D == 32 ? 32 : 64, E = D / LP;
  const long long row = (long long)blockIdx.x * (256 / LP) + threadIdx.x / LP;
  const bool valid = row < rows;  // a 32-lane row shares its wave: no early exit before the shuffles
  T* r = x + (valid ? row : 0) * ld + (threadIdx.x % LP) * E;
  float v[E], ss = 0.f;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    v[e] = to_f32<T>(r[e]);
    ss += v[e] * v[e];
  }
#pragma unroll
  for (int o = LP / 2; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
  const float n = sqrtf(ss);
  if (valid) {
#pragma unroll
    for (int e = 0; e < E; ++e) r[e] = from_f32<T>(v[e] / n);
  }
}

template <typename T>
static void launch_rownorm_hd(T* x, long long rows, int ld, int D, hipStream_t s) {
  if (D == 32) hipLaunchKernelGGL((rownorm_hd_kernel<T, 32>), dim3((unsigned)((rows + 7) / 8)), dim3(256), 0, s, x, rows, ld);
  else hipLaunchKernelGGL((rownorm_hd_kernel<T, 128>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, x, rows, ld);
}

// ---------------------------------------------------------------------------------------
// Batch-axis attention of the ViT (vit.py:48,59) at head_dim D: LP lanes own one (token, head),
// D / LP features each; online softmax over the L keys (any L), scale 1/sqrt(D).
// ---------------------------------------------------------------------------------------
template <typename T, int D>
__global__ void __launch_bounds__(256) vit_batch_attn_hd_kernel(const T* __restrict__ qkv, T* __restrict__ out, int L,
                                                                int ntok, int heads) {
  constexpr int LP = D == 32 ? 32 : 64, E = D / LP;
  constexpr float scale = D == 32 ? 0.17677669529663687f : 0.08838834764831845f;  // 1/sqrt(D)
  const long long pair = (long long)blockIdx.x * (256 / LP) + threadIdx.x / LP;
  const bool valid = pair < (long long)ntok * heads;
  const long long pp = valid ? pair : 0;
  const int C = heads * D;
  const int n = (int)(pp / heads), hh = (int)(pp - (long long)n * heads);
  const long long row_stride = (long long)ntok * 3 * C;  // between sequence (= batch) positions
  const int off = hh * D + (threadIdx.x % LP) * E;
  const T* base = qkv + (long long)n * 3 * C + off;
  for (int i = 0; i < L; ++i) {
    float qi[E], o[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      qi[e] = to_f32<T>(base[i * row_stride + e]) * scale;
      o[e] = 0.f;
    }
    float m = -INFINITY, l = 0.f;
    for (int j = 0; j < L; ++j) {
      float sj = 0.f;
#pragma unroll
      for (int e = 0; e < E; ++e) sj = fmaf(qi[e], to_f32<T>(base[j * row_stride + C + e]), sj);
#pragma unroll
      for (int s = LP / 2; s > 0; s >>= 1) sj += __shfl_xor(sj, s, 64);
      const float mn = fmaxf(m, sj);
      const float a = __expf(m - mn), pj = __expf(sj - mn);
      l = l * a + pj;
#pragma unroll
      for (int e = 0; e < E; ++e) o[e] = o[e] * a + pj * to_f32<T>(base[j * row_stride + 2 * C + e]);
      m = mn;
    }
    if (valid) {
#pragma unroll
      for (int e = 0; e < E; ++e) out[((long long)i * ntok + n) * C + off + e] = from_f32<T>(o[e] / l);
    }
  }
}

}  // namespace hd

int vit_batch_attn_hd(const void* qkv, void* out, int dtype, int L, int ntok, int heads, int head_dim, hipStream_t s) {
  using namespace hd;
  if (!hd_width(head_dim)) return fail("mhada_vit_batch_attn: head_dim must be 32, 64 or 128");
  const long long pairs = (long long)ntok * heads;
  const int ppb = head_dim == 32 ? 8 : 4;
  const dim3 grid((unsigned)((pairs + ppb - 1) / ppb)), blk(256);
  if (head_dim == 32) {
    if (dtype == MHADA_F32)
      hipLaunchKernelGGL((vit_batch_attn_hd_kernel<float, 32>), grid, blk, 0, s, (const float*)qkv, (float*)out, L, ntok, heads);
    else
      hipLaunchKernelGGL((vit_batch_attn_hd_kernel<bf16, 32>), grid, blk, 0, s, (const bf16*)qkv, (bf16*)out, L, ntok, heads);
  } else {
    if (dtype == MHADA_F32)
      hipLaunchKernelGGL((vit_batch_attn_hd_kernel<float, 128>), grid, blk, 0, s, (const float*)qkv, (float*)out, L, ntok, heads);
    else
      hipLaunchKernelGGL((vit_batch_attn_hd_kernel<bf16, 128>), grid, blk, 0, s, (const bf16*)qkv, (bf16*)out, L, ntok, heads);
  }
  return check_launch("mhada_vit_batch_attn");
}

}  // namespace mhada

using namespace mhada;

// mhada_attn_hd (SHARED = false) and mhada_attn_hd_shared: the same checks, kernel and grid; SHARED reads kv and
// v_mu of one style for every frame.
template <bool SHARED>
static int attn_hd_entry(const char* name_, const void* q, const void* kv, const float* fcs, const float* fcs_mu,
                         const float* fcs_rstd, const float* v_mu, void* out, int dtype, int B, int H, int D, int Nc,
                         int Ns, int activation, mhada_stream_t s_) {
  const std::string name(name_);
  hipStream_t s = (hipStream_t)s_;
  if (!q || !kv || !fcs || !fcs_mu || !fcs_rstd || !v_mu || !out || B <= 0 || H <= 0 || Nc <= 0 || Ns <= 0)
    return fail(name + ": bad args");
  if (!hd::hd_width(D)) return fail(name + ": D must be 32 or 128 (64: mhada_attn)");
  if (dtype != MHADA_F32 && dtype != MHADA_BF16) return fail(name + ": bad dtype");
  if (activation != MHADA_ACT_SOFTMAX && activation != MHADA_ACT_COSINE) return fail(name + ": bad activation");
  if (!aligned16(q) || !aligned16(kv) || !aligned16(fcs) || !aligned16(fcs_mu) ||
      !aligned16(fcs_rstd) || !aligned16(v_mu) || !aligned16(out))
    return fail(name + ": pointers must be 16-byte aligned");
  AttnP p = {};
  p.q = q; p.kv = kv; p.fcs = fcs; p.fcs_mu = fcs_mu; p.fcs_rstd = fcs_rstd; p.v_mu = v_mu;
  p.out = out; p.B = B; p.H = H; p.Nc = Nc; p.Ns = Ns;
  p.nqb = (Nc + 127) / 128;
  const long long nblk = (long long)B * H * p.nqb;
  if (nblk > (1LL << 31) - 1) return fail(name + ": grid too large");
  p.nblk = (int)nblk;
  if (D == 32) hd::launch_attn_hd<32, SHARED>(p, dtype, activation, s);
  else hd::launch_attn_hd<128, SHARED>(p, dtype, activation, s);
  return check_launch(name_);
}

extern "C" int mhada_attn_hd(const void* q, const void* kv, const float* fcs, const float* fcs_mu,
                             const float* fcs_rstd, const float* v_mu, void* out, int dtype, int B, int H, int D,
                             int Nc, int Ns, int activation, mhada_stream_t s_) {
  return attn_hd_entry<false>("mhada_attn_hd", q, kv, fcs, fcs_mu, fcs_rstd, v_mu, out, dtype, B, H, D, Nc, Ns,
                              activation, s_);
}

extern "C" int mhada_attn_hd_shared(const void* q, const void* kv, const float* fcs, const float* fcs_mu,
                                    const float* fcs_rstd, const float* v_mu, void* out, int dtype, int B, int H, int D,
                                    int Nc, int Ns, int activation, mhada_stream_t s_) {
  return attn_hd_entry<true>("mhada_attn_hd_shared", q, kv, fcs, fcs_mu, fcs_rstd, v_mu, out, dtype, B, H, D, Nc, Ns,
                             activation, s_);
}

extern "C" int mhada_fold_block_hd(const float* wf, const float* wg, const float* wh, const float* bg, const float* bh,
                                   const float* rstd_c, const float* mu_s, const float* rstd_s, void* wq, void* wkv,
                                   float* bkv, float* v_mu, float kscale, int dtype, int B, int H, int D,
                                   mhada_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  if (!wf || !wg || !wh || !bg || !bh || !rstd_c || !mu_s || !rstd_s || !wq || !wkv || !bkv || !v_mu || B <= 0 ||
      H <= 0)
    return fail("mhada_fold_block_hd: bad args");
  if (!hd::hd_width(D)) return fail("mhada_fold_block_hd: D must be 32 or 128 (64: mhada_fold_block)");
  if (dtype != MHADA_F32 && dtype != MHADA_BF16) return fail("mhada_fold_block_hd: bad dtype");
  if (dtype == MHADA_F32)
    hipLaunchKernelGGL((hd::fold_hd_kernel<float>), dim3(B * H), dim3(256), 0, s, wf, wg, wh, bg, bh, rstd_c, mu_s,
                       rstd_s, (float*)wq, (float*)wkv, bkv, v_mu, kscale, H, D);
  else
    hipLaunchKernelGGL((hd::fold_hd_kernel<bf16>), dim3(B * H), dim3(256), 0, s, wf, wg, wh, bg, bh, rstd_c, mu_s,
                       rstd_s, (bf16*)wq, (bf16*)wkv, bkv, v_mu, kscale, H, D);
  return check_launch("mhada_fold_block_hd");
}

extern "C" int mhada_cosine_prep_hd(void* q, void* kv, int dtype, int B, int H, int D, int Nc, int Ns,
                                    mhada_stream_t s_) {
  hipStream_t s = (hipStream_t)s_;
  if (B <= 0 || H <= 0 || Nc < 0 || Ns < 0 || (Nc == 0 && Ns == 0) || (Nc > 0 && !q) || (Ns > 0 && !kv))
    return fail("mhada_cosine_prep_hd: bad args");
  if (!hd::hd_width(D)) return fail("mhada_cosine_prep_hd: D must be 32 or 128 (64: mhada_cosine_prep)");
  if (dtype != MHADA_F32 && dtype != MHADA_BF16) return fail("mhada_cosine_prep_hd: bad dtype");
  const long long rq = (long long)B * H * Nc, rk = (long long)B * H * Ns;
  if (rq / 4 > (1LL << 31) - 2 || rk / 4 > (1LL << 31) - 2) return fail("mhada_cosine_prep_hd: too many rows");
  if (rq > 0) {
    if (dtype == MHADA_F32) hd::launch_rownorm_hd((float*)q, rq, D, D, s);
    else hd::launch_rownorm_hd((bf16*)q, rq, D, D, s);
  }
  if (rk > 0) {
    if (dtype == MHADA_F32) hd::launch_rownorm_hd((float*)kv, rk, 2 * D, D, s);
    else hd::launch_rownorm_hd((bf16*)kv, rk, 2 * D, D, s);
  }
  return check_launch("mhada_cosine_prep_hd");
}
