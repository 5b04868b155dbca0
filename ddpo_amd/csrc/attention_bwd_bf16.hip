// Attention backward on the 16-bit MFMA datapath.  Same algorithm as attention_bwd.hip (recompute P from the saved log2-LSE, two sweeps, no
// atomics) and the same operand-chaining trick as attention_bf16.hip: the 32x32 accumulator fragment of the score product (row =
// lane-half-dependent, col = lane&31) is converted in registers into the B operand of the next product, whose 8 reduction slots per lane
// half h in MFMA step u are rows 16u + 4h + {0,1,2,3, 8,9,10,11}.
//   dkdv kernel: workgroup = 4 waves x 32 keys (K, V fragments in registers); sweeps 64-query tiles held in LDS both
//       row-major (A of S = Q K^T and dP = dO V^T) and transposed (A of dV^T += dO^T P and dK^T += Q^T dS)
//   dq kernel:   workgroup = 4 waves x 32 queries (Q, dO fragments in registers); sweeps 64-key tiles: K row-major +
//       transposed, V row-major:  S^T = K Q^T, dP^T = V dO^T, dS^T = P^T (dP^T - D), dQ^T += K^T dS^T
// Q is pre-scaled by scale*log2(e) wherever it feeds the scores (so dK picks up ln 2 at the end).
//
// ONE body per kernel for both datapaths (template flag F16P, as in the forward).  What differs is arithmetic policy only, and it lives in
// AttnBwdArith<F16P>: the operand KIND of every image and fragment (below), the scale constants, the clamp and the exponential.  An operand
// is a Split<V> (hi + lo terms) or a single term (a bare vector); mma() issues the passes a pair of kinds needs, in a fixed order.
//   F16P == false, `bf16x3` (f16p == 0 of the entry point): EVERY operand bf16 hi + lo, three passes per product, no scaling — the round-1..3
//       kernels, kept as the reference-accuracy variant (84 + 60 MFMAs per 64 x 32 block pair).
//   F16P == true, `f16mx` (round 4).  Both kernels were matrix-pipe bound at three bf16 passes per product
//       (profiles/r03_final_train_kernel_stats.md).  Only the SCORES keep the three-pass bf16 split (they are exponentiated).  Every other
//       product has one operand that is a single f16 term (11 significant bits, round to nearest even) against the f16 hi + lo split of the
//       other (2 passes of v_mfma_f32_32x32x16_f16):
//         dP  = dO' V^T      dO' single,  V hi + lo          dV = P'^T dO'     P' single,  dO' hi + lo
//         dK  = dS'^T Q      dS' single,  Q hi + lo          dQ = dS' K        dS' single, K hi + lo
//       62 + 46 MFMAs instead of 84 + 60.  Ranges: P' = exp2(S - L + 14) in (0, 2^14] (as in the forward); dO' = dO * 2^-e with e the exponent
//       of max |dO| over the (batch, head) slab — found by the dvec pre-pass (one atomic max per slab) — so |dO'| < 1 whatever the loss scale
//       of the micro-batch (PPO gradients differ by 1e4 between timesteps; f16 keeps 14 binades below the slab maximum normal);
//       dS' = 16 P (dP' - D'), clamped to the f16 range.  The powers of two come out exactly in the output stage.
#include "attention_x16.h"
#include "attention_dvec.h"
#include <type_traits>

#define BWD_F16_MAX 60000.0f

// ---- operand kinds: Split<V> = hi + lo terms; a bare bf16x8 / f16x8 = a single term
template <typename V> struct Split { V hi, lo; };
template <typename T> struct OpKind { using V = T; static constexpr bool SPLIT = false; };
template <typename U> struct OpKind<Split<U>> { using V = U; static constexpr bool SPLIT = true; };
template <typename T> constexpr bool op_is_f16 = std::is_same_v<typename OpKind<T>::V, f16x8>;

__device__ __forceinline__ f32x16 mfma(bf16x8 a, bf16x8 b, f32x16 c) { return MFMA32(a, b, c); }
__device__ __forceinline__ f32x16 mfma(f16x8 a, f16x8 b, f32x16 c) { return MFMA32H(a, b, c); }
// acc += A B, small terms first.  The ONE place that fixes the pass order of every product of both kernels.
template <typename V> __device__ __forceinline__ void mma(f32x16& c, const Split<V>& a, const Split<V>& b) {
  c = mfma(a.lo, b.hi, c); c = mfma(a.hi, b.lo, c); c = mfma(a.hi, b.hi, c);
}
template <typename V> __device__ __forceinline__ void mma(f32x16& c, const Split<V>& a, const V& b) { c = mfma(a.lo, b, c); c = mfma(a.hi, b, c); }
template <typename V> __device__ __forceinline__ void mma(f32x16& c, const V& a, const Split<V>& b) { c = mfma(a, b.lo, c); c = mfma(a, b.hi, c); }

// 8 floats (held as 8 accumulator registers) -> one operand fragment of the kind of `f`
__device__ __forceinline__ void frag(const float* v, Split<bf16x8>& f) { frag8(v, f.hi, f.lo); }
__device__ __forceinline__ void frag(const float* v, Split<f16x8>& f) { frag8h2(v, f.hi, f.lo, BWD_F16_MAX); }
__device__ __forceinline__ void frag(const float* v, f16x8& f) { f = frag8h(v); }
// B-operand fragments (registers) of one token's feature vector: lane (token = li, half h) holds features 16s + 8h .. +8
template <int D, int NKS, typename T>
__device__ __forceinline__ void load_frags(const float* p, float mul, int h, T* f) {
#pragma unroll
  for (int s = 0; s < NKS; ++s) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = 16 * s + 8 * h + e;
      v[e] = c < D ? p[c] * mul : 0.f;
    }
    frag(v, f[s]);
  }
}

// ---- LDS.  An image = the hi plane at p and, for a Split kind, the lo plane `lo` bytes behind it; `ld` elements per row.
struct Img { char* p; int lo, ld; };
// Both kernels sweep 64-token tiles held as row-major images [token][feature] and transposed images [feature][token].  The kernels take their
// images and zero-fill counts from here and the launcher its byte counts: no size is written twice.
template <int DKP, int DVP, bool F16P>
struct AttnBwdLds {
  static constexpr int T = 64, LDR = DKP + 8, LDT = T + 4;          // tokens per tile; elements per row-major / transposed row
  static constexpr int RM = T * LDR * 2, TR = DVP * LDT * 2;        // bytes per plane
  // dK/dV kernel: Q' (score operand: bf16 hi / lo) and dO' (F16P: ONE f16 plane; else bf16 hi / lo) row-major, both transposed hi / lo, and
  // the tile's 64 LSE and 64 D values; the images (everything in front of A_ROWS) are zero-filled once
  static constexpr int A_Q = 0, A_O = A_Q + 2 * RM, A_QT = A_O + (F16P ? 1 : 2) * RM, A_OT = A_QT + 2 * TR, A_ROWS = A_OT + 2 * TR;
  static constexpr int A_BYTES = A_ROWS + 2 * T * (int)sizeof(float);
  // dQ kernel: K (score operand) and V row-major hi / lo, K transposed hi / lo; all of it zero-filled once
  static constexpr int B_K = 0, B_V = B_K + 2 * RM, B_KT = B_V + 2 * RM, B_BYTES = B_KT + 2 * TR;
  static_assert(A_ROWS % 16 == 0 && B_BYTES % 16 == 0, "zero-filled in 16-byte chunks");
  __device__ static Img rm(char* smem, int off) { return Img{smem + off, RM, LDR}; }
  __device__ static Img tr(char* smem, int off) { return Img{smem + off, TR, LDT}; }
};
__device__ __forceinline__ void lds_zero(char* smem, int bytes, int t) {
  for (int i = t; i < bytes / 16; i += 256) reinterpret_cast<uint4*>(smem)[i] = make_uint4(0u, 0u, 0u, 0u);
}
// row-major fragment: 8 consecutive features at (row, col0)
template <typename V> __device__ __forceinline__ void load_rm(Split<V>& f, const Img m, int row, int col0) {
  f.hi = ld_rm<V>(m.p, m.ld, row, col0); f.lo = ld_rm<V>(m.p + m.lo, m.ld, row, col0);
}
__device__ __forceinline__ void load_rm(f16x8& f, const Img m, int row, int col0) { f = ld_rm<f16x8>(m.p, m.ld, row, col0); }
// transposed fragment: tokens {s0..s0+3, s0+8..s0+11} of feature `row`
template <typename V> __device__ __forceinline__ void load_tr(Split<V>& f, const Img m, int row, int s0) {
  f.hi = ld_tr<V>(m.p, m.ld, row, s0); f.lo = ld_tr<V>(m.p + m.lo, m.ld, row, s0);
}
// Stage one float4 (features f0 .. f0 + 3 of token `tok`) as kind R into the row-major image rm and as the Split kind T into the transposed
// image tr (T = void: no transposed image).  R and T of one element type share one split.
struct Pk4 { uint32_t h0, h1, l0, l1; };                            // packed hi / lo pairs of features (f0, f0 + 1) and (f0 + 2, f0 + 3)
template <typename T> __device__ __forceinline__ Pk4 split4_as(const float4 v) {
  Pk4 r;
  if constexpr (op_is_f16<T>) { split2h(v.x, v.y, r.h0, r.l0, BWD_F16_MAX); split2h(v.z, v.w, r.h1, r.l1, BWD_F16_MAX); }
  else { split2(v.x, v.y, r.h0, r.l0); split2(v.z, v.w, r.h1, r.l1); }
  return r;
}
template <typename R, typename T>
__device__ __forceinline__ void stage4(const float4 v, const Img rm, const Img tr, int tok, int f0) {
  const Pk4 r = split4_as<R>(v);
  *reinterpret_cast<uint2*>(rm.p + (tok * rm.ld + f0) * 2) = make_uint2(r.h0, r.h1);
  if constexpr (OpKind<R>::SPLIT) *reinterpret_cast<uint2*>(rm.p + rm.lo + (tok * rm.ld + f0) * 2) = make_uint2(r.l0, r.l1);
  if constexpr (!std::is_void_v<T>) {
    static_assert(OpKind<T>::SPLIT, "transposed images hold hi + lo");
    const Pk4 t = split4_as<T>(v);
    scatter_tr(tr.p, tr.p + tr.lo, tr.ld, tok, f0, t.h0, t.h1, t.l0, t.l1);
  }
}

// ---- arithmetic policy.  Score operands are Split<bf16x8> in both; Narrow = the kind of dO', P' and dS', Wide = the kind of their partners
// (V, dO'^T, Q'^T, K^T).  With the scale constants at 1 and the shift at 0 the scaling arithmetic of the body folds away exactly.
template <bool F16P> struct AttnBwdArith;
template <> struct AttnBwdArith<false> {
  using Narrow = Split<bf16x8>;
  using Wide = Split<bf16x8>;
  static constexpr float P_SHIFT = 0.f, P_SCALE = 1.f, DS_SCALE = 1.f, omul = 1.f, oinv = 1.f;
  __device__ __forceinline__ AttnBwdArith(const uint32_t*, int) {}
  __device__ static __forceinline__ float exp2(float x) { return exp2f(x); }
  __device__ static __forceinline__ float clamp(float x) { return x; }
};
template <> struct AttnBwdArith<true> {
  using Narrow = f16x8;
  using Wide = Split<f16x8>;
  static constexpr float P_SHIFT = 14.f, P_SCALE = 16384.f;         // P' = 2^14 P
  static constexpr float DS_SCALE = 16.f;                           // dS' = 16 P (dP' - D')
  float omul, oinv;                                                 // dO' = dO * omul, oinv = 1 / omul
  // omul = 2^-e for the slab maximum amax[bh] (float bits of max |dO|, >= 0): max |dO| * omul lies in [0.5, 1).  amax == 0 -> 1.
  __device__ __forceinline__ AttnBwdArith(const uint32_t* amax, int bh) {
    uint32_t e = amax[bh] >> 23;
    if (e == 0u) { omul = 1.f; oinv = 1.f; return; }
    e = e > 250u ? 250u : e;
    omul = __uint_as_float((253u - e) << 23);
    oinv = __uint_as_float((e + 1u) << 23);
  }
  __device__ static __forceinline__ float exp2(float x) { return __builtin_amdgcn_exp2f(x); }
  __device__ static __forceinline__ float clamp(float x) { return fminf(fmaxf(x, -BWD_F16_MAX), BWD_F16_MAX); }
};

// ---------------------------------------------------------------------------------------------- dK, dV
template <int D, int DKP, int DVP, bool F16P>
__global__ void __launch_bounds__(256) attn_bwd_dkdv_x16_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ k,
                                                                int ldk, const float* __restrict__ v, int ldv,
                                                                const float* __restrict__ d_o, const float* __restrict__ lse,
                                                                const float* __restrict__ dvec, const uint32_t* __restrict__ amax,
                                                                float* __restrict__ dk, float* __restrict__ dv, int heads, int Nq, int Nk,
                                                                float scale_log2e) {
  using A = AttnBwdArith<F16P>;
  using L = AttnBwdLds<DKP, DVP, F16P>;
  using Score = Split<bf16x8>;
  using Narrow = typename A::Narrow;
  using Wide = typename A::Wide;
  constexpr int QT = L::T, NKS = DKP / 16, NDT = DVP / 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const Img Qs = L::rm(smem, L::A_Q), Os = L::rm(smem, L::A_O), QTs = L::tr(smem, L::A_QT), OTs = L::tr(smem, L::A_OT);
  float* Ls = reinterpret_cast<float*>(smem + L::A_ROWS);
  float* Dv = Ls + QT;
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6, li = lane & 31, h = lane >> 5;
  const int bh = blockIdx.y, b = bh / heads, hd = bh - b * heads, C = heads * D;
  const int key0 = blockIdx.x * 128 + wid * 32;
  const int krow = min(key0 + li, Nk - 1);
  const A ar(amax, bh);
  Score kr[NKS];
  Wide vr[NKS];
  load_frags<D, NKS>(k + ((int64_t)b * Nk + krow) * ldk + hd * D, 1.0f, h, kr);
  load_frags<D, NKS>(v + ((int64_t)b * Nk + krow) * ldv + hd * D, 1.0f, h, vr);
  lds_zero(smem, L::A_ROWS, t);

  f32x16 dvt[NDT], dkt[NDT];
#pragma unroll
  for (int n = 0; n < NDT; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) { dvt[n][r] = 0.f; dkt[n][r] = 0.f; }

  const float c1 = A::DS_SCALE / A::P_SCALE;                   // dS' = P' * (dP' - D') * c1
  const float* qb = q + (int64_t)b * Nq * ldq + hd * D;
  const float* ob = d_o + (int64_t)b * Nq * C + hd * D;
  for (int q0 = 0; q0 < Nq; q0 += QT) {
    __syncthreads();
    for (int i = t; i < QT * (D / 4); i += 256) {
      const int tok = i / (D / 4), c4 = i - tok * (D / 4);
      float4 qv = make_float4(0.f, 0.f, 0.f, 0.f), ov = qv;
      if (q0 + tok < Nq) {
        qv = *reinterpret_cast<const float4*>(qb + (int64_t)(q0 + tok) * ldq + c4 * 4);
        ov = *reinterpret_cast<const float4*>(ob + (int64_t)(q0 + tok) * C + c4 * 4);
        qv.x *= scale_log2e; qv.y *= scale_log2e; qv.z *= scale_log2e; qv.w *= scale_log2e;
        ov.x *= ar.omul; ov.y *= ar.omul; ov.z *= ar.omul; ov.w *= ar.omul;
      }
      stage4<Score, Wide>(qv, Qs, QTs, tok, c4 * 4);
      stage4<Narrow, Wide>(ov, Os, OTs, tok, c4 * 4);
    }
    if (t < QT) {
      const bool ok = q0 + t < Nq;
      Ls[t] = ok ? lse[(int64_t)bh * Nq + q0 + t] - A::P_SHIFT : INFINITY;       // padded queries: P' = exp2(S - inf) = 0
      Dv[t] = ok ? dvec[(int64_t)bh * Nq + q0 + t] * ar.omul * c1 : 0.f;
    }
    __syncthreads();
#pragma unroll 1
    for (int sub = 0; sub < 2; ++sub) {
      f32x16 sacc, dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) { sacc[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
      for (int s = 0; s < NKS; ++s) {
        Score qa;
        load_rm(qa, Qs, 32 * sub + li, 16 * s + 8 * h);
        mma(sacc, qa, kr[s]);
        Narrow oa;
        load_rm(oa, Os, 32 * sub + li, 16 * s + 8 * h);
        mma(dp, oa, vr[s]);
      }
      float p[16], ds[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int qq = 32 * sub + (r & 3) + 8 * (r >> 2) + 4 * h;       // accumulator row = query
        p[r] = A::exp2(sacc[r] - Ls[qq]);
        ds[r] = A::clamp(p[r] * (dp[r] * c1 - Dv[qq]));
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        Narrow pf, sf;
        frag(p + 8 * u, pf);
        frag(ds + 8 * u, sf);
        const int s0 = 32 * sub + 16 * u + 4 * h;
#pragma unroll
        for (int n = 0; n < NDT; ++n) {
          Wide ot, qt;
          load_tr(ot, OTs, 32 * n + li, s0);
          mma(dvt[n], ot, pf);
          load_tr(qt, QTs, 32 * n + li, s0);
          mma(dkt[n], qt, sf);
        }
      }
    }
  }
  if (key0 + li < Nk) {
    const float fk = 0.6931471805599453f * ar.oinv / A::DS_SCALE, fv = ar.oinv / A::P_SCALE;
    float* pk = dk + ((int64_t)b * Nk + key0 + li) * C + hd * D;
    float* pv = dv + ((int64_t)b * Nk + key0 + li) * C + hd * D;
#pragma unroll
    for (int n = 0; n < NDT; ++n)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int dc = 32 * n + 8 * g + 4 * h;
        if (dc < D) {
          *reinterpret_cast<float4*>(pk + dc) = make_float4(dkt[n][4 * g] * fk, dkt[n][4 * g + 1] * fk, dkt[n][4 * g + 2] * fk, dkt[n][4 * g + 3] * fk);
          *reinterpret_cast<float4*>(pv + dc) = make_float4(dvt[n][4 * g] * fv, dvt[n][4 * g + 1] * fv, dvt[n][4 * g + 2] * fv, dvt[n][4 * g + 3] * fv);
        }
      }
  }
}

// ---------------------------------------------------------------------------------------------- dQ
template <int D, int DKP, int DVP, bool F16P>
__global__ void __launch_bounds__(256) attn_bwd_dq_x16_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ k,
                                                              int ldk, const float* __restrict__ v, int ldv,
                                                              const float* __restrict__ d_o, const float* __restrict__ lse,
                                                              const float* __restrict__ dvec, const uint32_t* __restrict__ amax,
                                                              float* __restrict__ dq, int heads, int Nq, int Nk, float scale, float scale_log2e) {
  using A = AttnBwdArith<F16P>;
  using L = AttnBwdLds<DKP, DVP, F16P>;
  using Score = Split<bf16x8>;
  using Narrow = typename A::Narrow;
  using Wide = typename A::Wide;
  constexpr int KT = L::T, NKS = DKP / 16, NDT = DVP / 32;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const Img Ks = L::rm(smem, L::B_K), Vs = L::rm(smem, L::B_V), KTs = L::tr(smem, L::B_KT);
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6, li = lane & 31, h = lane >> 5;
  const int bh = blockIdx.y, b = bh / heads, hd = bh - b * heads, C = heads * D;
  const int q0 = blockIdx.x * 128 + wid * 32;
  const int qrow = min(q0 + li, Nq - 1);
  const A ar(amax, bh);
  Score qr[NKS];
  Narrow orr[NKS];
  load_frags<D, NKS>(q + ((int64_t)b * Nq + qrow) * ldq + hd * D, scale_log2e, h, qr);
  load_frags<D, NKS>(d_o + ((int64_t)b * Nq + qrow) * C + hd * D, ar.omul, h, orr);
  const float c1 = A::DS_SCALE / A::P_SCALE;
  const float Lq = lse[(int64_t)bh * Nq + qrow] - A::P_SHIFT, Dq = dvec[(int64_t)bh * Nq + qrow] * ar.omul * c1;
  lds_zero(smem, L::B_BYTES, t);

  f32x16 dqt[NDT];
#pragma unroll
  for (int n = 0; n < NDT; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) dqt[n][r] = 0.f;
  const float* kb = k + (int64_t)b * Nk * ldk + hd * D;
  const float* vb = v + (int64_t)b * Nk * ldv + hd * D;
  for (int kt0 = 0; kt0 < Nk; kt0 += KT) {
    __syncthreads();
    for (int i = t; i < KT * (D / 4); i += 256) {
      const int tok = i / (D / 4), c4 = i - tok * (D / 4);
      float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
      if (kt0 + tok < Nk) {
        kv = *reinterpret_cast<const float4*>(kb + (int64_t)(kt0 + tok) * ldk + c4 * 4);
        vv = *reinterpret_cast<const float4*>(vb + (int64_t)(kt0 + tok) * ldv + c4 * 4);
      }
      stage4<Score, Wide>(kv, Ks, KTs, tok, c4 * 4);
      stage4<Wide, void>(vv, Vs, Img{}, tok, c4 * 4);
    }
    __syncthreads();
#pragma unroll 1
    for (int j = 0; j < 2; ++j) {
      f32x16 sacc, dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) { sacc[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
      for (int s = 0; s < NKS; ++s) {
        Score ka;
        load_rm(ka, Ks, 32 * j + li, 16 * s + 8 * h);
        mma(sacc, ka, qr[s]);
        Wide va;
        load_rm(va, Vs, 32 * j + li, 16 * s + 8 * h);
        mma(dp, va, orr[s]);
      }
      float ds[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const bool ok = kt0 + 32 * j + (r & 3) + 8 * (r >> 2) + 4 * h < Nk;   // accumulator row = key
        const float p = ok ? A::exp2(sacc[r] - Lq) : 0.f;
        ds[r] = A::clamp(p * (dp[r] * c1 - Dq));
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        Narrow sf;
        frag(ds + 8 * u, sf);
        const int s0 = 32 * j + 16 * u + 4 * h;
#pragma unroll
        for (int n = 0; n < NDT; ++n) {
          Wide kt;
          load_tr(kt, KTs, 32 * n + li, s0);
          mma(dqt[n], kt, sf);
        }
      }
    }
  }
  if (q0 + li < Nq) {
    const float fq = scale * ar.oinv / A::DS_SCALE;
    float* pq = dq + ((int64_t)b * Nq + q0 + li) * C + hd * D;
#pragma unroll
    for (int n = 0; n < NDT; ++n)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int dc = 32 * n + 8 * g + 4 * h;
        if (dc < D)
          *reinterpret_cast<float4*>(pq + dc) = make_float4(dqt[n][4 * g] * fq, dqt[n][4 * g + 1] * fq, dqt[n][4 * g + 2] * fq, dqt[n][4 * g + 3] * fq);
      }
  }
}

template <int D, int DKP, int DVP, bool F16P>
static int launch_bwd_x16(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* o, const float* d_o,
                          const float* lse, float* dvec, float* dq, float* dk, float* dv, int B, int heads, int Nq, int Nk,
                          float scale, hipStream_t st) {
  using L = AttnBwdLds<DKP, DVP, F16P>;
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_bwd_dkdv_x16_kernel<D, DKP, DVP, F16P>), hipFuncAttributeMaxDynamicSharedMemorySize, L::A_BYTES);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_bwd_dq_x16_kernel<D, DKP, DVP, F16P>), hipFuncAttributeMaxDynamicSharedMemorySize, L::B_BYTES);
    attr = true;
  }
  const float sl2 = scale * 1.4426950408889634f;
  // F16P: the slab maxima live behind the B * heads * Nq floats of `dvec` (the caller allocates B * heads * (Nq + 1) floats, include/ddpo_hip.h)
  uint32_t* amax = F16P ? reinterpret_cast<uint32_t*>(dvec + (size_t)B * heads * Nq) : nullptr;
  if (F16P && hipMemsetAsync(amax, 0, (size_t)B * heads * sizeof(uint32_t), st) != hipSuccess) return DDPO_ELAUNCH;
  launch_attn_dvec<F16P>(o, d_o, dvec, amax, B, heads, Nq, D, st);
  DDPO_LAUNCH_CHECK();
  hipLaunchKernelGGL((attn_bwd_dkdv_x16_kernel<D, DKP, DVP, F16P>), dim3((Nk + 127) / 128, B * heads), dim3(256), L::A_BYTES, st, q, ldq, k,
                     ldk, v, ldv, d_o, lse, dvec, amax, dk, dv, heads, Nq, Nk, sl2);
  DDPO_LAUNCH_CHECK();
  hipLaunchKernelGGL((attn_bwd_dq_x16_kernel<D, DKP, DVP, F16P>), dim3((Nq + 127) / 128, B * heads), dim3(256), L::B_BYTES, st, q, ldq, k,
                     ldk, v, ldv, d_o, lse, dvec, amax, dq, heads, Nq, Nk, scale, sl2);
  DDPO_LAUNCH_CHECK();
  return DDPO_OK;
}

template <bool F16P>
static int attention_bwd_impl(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* o, const float* d_o,
                              const float* lse, float* dvec, float* dq, float* dk, float* dv, int B, int heads, int Nq, int Nk, int d,
                              float scale, hipStream_t st) {
#define BWDB(DD, DK, DV) return launch_bwd_x16<DD, DK, DV, F16P>(q, ldq, k, ldk, v, ldv, o, d_o, lse, dvec, dq, dk, dv, B, heads, Nq, Nk, scale, st)
  switch (d) {
    case 8: BWDB(8, 16, 32);
    case 16: BWDB(16, 16, 32);
    case 40: BWDB(40, 48, 64);
    case 64: BWDB(64, 64, 64);
    case 80: BWDB(80, 80, 96);
    default: return DDPO_EINVAL;
  }
#undef BWDB
}

/* f16p == 0: the bf16x3 datapath's backward; else the f16mx datapath's (see the head of this file), whose dvec is B * heads * (Nq + 1) floats. */
extern "C" int ddpo_attention_bwd_x16(int f16p, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* o,
                                      const float* d_o, const float* lse, float* dvec, float* dq, float* dk, float* dv, int B,
                                      int heads, int Nq, int Nk, int d, float scale, void* stream) {
  if (!q || !k || !v || !o || !d_o || !lse || !dvec || !dq || !dk || !dv) return DDPO_EINVAL;
  if (B <= 0 || heads <= 0 || Nq <= 0 || Nk <= 0 || (ldq & 3) || (ldk & 3) || (ldv & 3) || (long)B * heads > 65535) return DDPO_EINVAL;
  hipStream_t st = as_stream(stream);
  return !f16p ? attention_bwd_impl<false>(q, ldq, k, ldk, v, ldv, o, d_o, lse, dvec, dq, dk, dv, B, heads, Nq, Nk, d, scale, st)
               : attention_bwd_impl<true>(q, ldq, k, ldk, v, ldv, o, d_o, lse, dvec, dq, dk, dv, B, heads, Nq, Nk, d, scale, st);
}
