// mhada_gemm_half2 / mhada_gemm_half2_planes: argument checks and launch of the HALF2 GEMM
// (gemm_h2_kernel, gemm_impl.h) — an fp32 product of a range-bounded activation and a
// prepared weight as three fp16 products.
#include "gemm_impl.h"

using namespace mhada;

// out_scale: the mhada_gemm_half2_planes form (c2 = fp16 planes of out_scale[n] x); null: mhada_gemm_half2
static int gemm_half2(const mhada_gemm_args* a, const float* col_scale, const float* out_scale, hipStream_t stream) {
  if (a->M < 0 || a->N <= 0 || a->K <= 0) return fail("mhada_gemm_half2: bad sizes");
  if (a->nb1 != 1 || a->nb2 != 1) return fail("mhada_gemm_half2: one problem only (nb1 = nb2 = 1)");
  if (a->K % 64) return fail("mhada_gemm_half2: K0 must be a multiple of 64");
  if (a->a_mode != MHADA_A_ROWS || a->a_mu || a->vt) return fail("mhada_gemm_half2: ROWS mode, no centring / vt");
  if (a->c_dtype != MHADA_F32 && a->c_dtype != MHADA_BF16) return fail("mhada_gemm_half2: bad c_dtype");
  if (a->r && a->r_dtype != a->c_dtype) return fail("mhada_gemm_half2: residual dtype must equal output dtype");
  if (a->relu < 0 || a->relu > 1) return fail("mhada_gemm_half2: relu must be 0 or 1");
  if (!a->a || !a->w || !col_scale || (!a->c && !a->c2_planes && !out_scale)) return fail("mhada_gemm_half2: null operand");
  if (out_scale && (!a->c2 || a->c_dtype != MHADA_F32 || a->N % 4 || !tuning().gemm_ldsepi || !aligned16(out_scale) ||
                    a->ldc2 < a->N))
    return fail("mhada_gemm_half2_planes: needs a c2 buffer with ldc2 >= N, c_dtype fp32, N % 4 == 0, a 16-byte "
                "aligned out_scale and the LDS epilogue");
  if (a->M == 0) return MHADA_OK;
  if (!aligned16(a->a) || a->lda % 8 || a->lda < a->K)
    return fail("mhada_gemm_half2: A must be 16-byte aligned with lda a multiple of 8 and >= K0");
  if (!aligned16(a->w) || a->ldw % 8 || a->ldw < 2 * (long long)a->K)
    return fail("mhada_gemm_half2: W must be 16-byte aligned with ldw a multiple of 8 and >= 2 K0");
  if (!aligned16(col_scale)) return fail("mhada_gemm_half2: col_scale must be 16-byte aligned");
  if (((uintptr_t)a->c & 7) || a->ldc % 4) return fail("mhada_gemm_half2: C must be 8-byte aligned with ldc % 4 == 0");
  if (a->r && (((uintptr_t)a->r & 7) || a->ldr % 4))
    return fail("mhada_gemm_half2: R must be 8-byte aligned with ldr % 4 == 0");
  if (a->bias && !aligned16(a->bias)) return fail("mhada_gemm_half2: bias must be 16-byte aligned");
  if (a->c2 && (a->c_dtype != MHADA_F32 || ((uintptr_t)a->c2 & 7) || a->ldc2 % 4))
    return fail("mhada_gemm_half2: c2 needs fp32 C, 8-byte alignment and ldc2 % 4 == 0");
  if (!out_scale && a->c2_planes && (!a->c2 || a->N % 4 || !tuning().gemm_ldsepi))
    return fail("mhada_gemm_half2: c2_planes needs a c2 buffer, N % 4 == 0 and the LDS epilogue");
  if ((((long long)a->M + 255) / 256) * (((long long)a->N + 255) / 256) >= (1LL << 31))
    return fail("mhada_gemm_half2: more than 2^31 tiles");
  // 32-bit element offsets inside one operand plane (the staging addresses)
  if ((long long)(a->M - 1) * a->lda + a->K >= (1LL << 31) || (long long)(a->N - 1) * a->ldw + 2LL * a->K >= (1LL << 31))
    return fail("mhada_gemm_half2: operand spans need 32-bit element offsets");
  GemmP p{};
  p.M = a->M; p.N = a->N; p.K = a->K; p.nb2 = 1;
  p.a = a->a; p.lda = a->lda;
  p.spl = (long long)a->M * a->lda;
  p.w = a->w; p.ldw = a->ldw;
  p.bias = a->bias;
  p.r = a->r; p.ldr = a->ldr;
  p.c = a->c; p.ldc = a->ldc;
  p.relu = a->relu;
  p.c2 = a->c2; p.ldc2 = a->ldc2;
  p.c2planes = !out_scale && a->c2_planes ? 1 : 0;
  if (out_scale) return launch_gemm_h2_f16(p, col_scale, out_scale, stream);
  if (a->c_dtype == MHADA_F32) return launch_gemm_h2<float>(p, col_scale, stream);
  return launch_gemm_h2<bf16>(p, col_scale, stream);
}

extern "C" int mhada_gemm_half2(const mhada_gemm_args* a, const float* col_scale, mhada_stream_t stream) {
  if (!a) return fail("mhada_gemm_half2: null args");
  return gemm_half2(a, col_scale, nullptr, (hipStream_t)stream);
}

extern "C" int mhada_gemm_half2_planes(const mhada_gemm_args* a, const float* col_scale, const float* out_scale,
                                       mhada_stream_t stream) {
  if (!a || !out_scale) return fail("mhada_gemm_half2_planes: null args");
  return gemm_half2(a, col_scale, out_scale, (hipStream_t)stream);
}
