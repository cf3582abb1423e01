// Grouped-query attention (GQA) over a layer's compressed cache: G = Hq / Hkv query heads share one KV head
// (transformers' repeat_kv: query head h reads KV head h / G).  The MHA kernels build query-premultiplied codebook
// tables per query head; run per query head, that would repeat every look-up G times.  Here each packed word of a
// KV head is loaded and decoded ONCE and feeds the G query heads from registers:
//
//  q.K^T (gqa_score_kernel): one lane per token.  Per rotation pair (k_lo, k_hi = k_lo + 64) the lane looks the two
//    codes up in the raw per-channel codebook (LDS), forms the rotated key pair once,
//      r_lo = c*K[k_lo] - s*K[k_hi],  r_hi = s*K[k_lo] + c*K[k_hi]      ((c, s) of the pair's angle at the token)
//    and adds q_g[k_lo]*r_lo + q_g[k_hi]*r_hi for the G query heads -- the sum the MHA tables form (kvq_ktab.h).  The
//    query values are wave-uniform: they come from a permuted copy through the scalar cache.  The (c, s) of a token are
//    computed once per role and shared by the workgroup's KV heads.  K outlier entries come from the token-contiguous
//    mirror and are added to every query head of their KV head.  The first softmax pass (per-wave max and sum of
//    exp of the scaled scores) is fused, so kvq_softmax_finish runs over the Hq rows unchanged.
//  p.V (gqa_mix_kernel): a lane owns 8 channels of a KV head and 4 consecutive tokens per 64-token step; a code is
//    looked up once in the token's codebook row and multiplied into G accumulators.  V outlier entries of the
//    workgroup's KV head are summed into LDS in 32.32 fixed point (exact, order independent), per-chunk slabs are
//    reduced in a fixed order: deterministic, no float atomics.
#include "kvq_common.h"
#include "kvq_host.h"
#include "kvq_ktab.h"

namespace kvq {

constexpr int kGqaMaxG = 8;       // query heads per KV head
constexpr int kGqaMaxHpw = 4;     // KV heads per score workgroup (their codebooks live in LDS)
constexpr int kGqaPT = 64;        // tokens per softmax partial (one wave)
constexpr int kGqaMixBT = 256;    // p.V: tokens staged per block

// query heads per KV head, rounded up to the register layout the kernels are compiled for
static inline int gqa_bucket(int G) { return G <= 1 ? 1 : (G <= 2 ? 2 : (G <= 4 ? 4 : 8)); }

static inline bool gqa_shape_ok(int Hq, int Hkv, int hd) {
  if (Hq <= 0 || Hkv <= 0 || hd != kHeadDim || Hq % Hkv) return false;
  const int G = Hq / Hkv;
  return G >= 1 && G <= kGqaMaxG && (int64_t)Hkv * kHeadDim <= 8192;
}

// score workspace: [q32: Hq*128 f32][qp: Hkv*2*32*2*GB f32]
static inline size_t gqa_q32_bytes(int Hq) { return ((size_t)Hq * kHeadDim * 4 + 255) & ~(size_t)255; }
static inline size_t gqa_score_ws(int Hq, int Hkv) {
  return gqa_q32_bytes(Hq) + (size_t)Hkv * kHeadDim * gqa_bucket(Hq / Hkv) * 4;
}

// q32 = q as fp32; qp[kv][j][half][g] = q[kv*G + g][j + 64*half] (j = 0..63: role j/32, pair j%32), 0 for g >= G
template <int GB>
__global__ __launch_bounds__(256) void gqa_qprep_kernel(const void *__restrict__ q, int q_is_half, float *__restrict__ q32,
                                                        float *__restrict__ qp, int Hq, int Hkv, int G) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < Hq * kHeadDim) q32[i] = ld_act(q, i, q_is_half);
  if (i >= Hkv * kHeadDim * GB) return;
  const int g = i % GB, r = i / GB;
  const int half = r & 1, j = (r >> 1) & 63, kv = r >> 7;
  qp[i] = g < G ? ld_act(q, (int64_t)(kv * G + g) * kHeadDim + j + 64 * half, q_is_half) : 0.f;
}

__device__ __forceinline__ float gqa_wave_max(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d));
  return v;
}
__device__ __forceinline__ float gqa_wave_sum(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// grid (token tiles of blockDim tokens, KV-head groups of hpw); dynamic LDS: hpw codebooks [128][2^BITS] f32
// RT (scaled RoPE, kvq.h: kvq_rope): frequencies from rt_freq [64] instead of powf(rope_theta, ..), and the attention
// factor rt_af scales the lane's (cos, sin) once (and the sin / cos of each outlier entry); gqa_score_kernel_rt below
template <int BITS, int GB, bool RT>
__device__ __forceinline__ void gqa_score_body(
    const uint32_t *__restrict__ mat, const float *__restrict__ lut, const float *__restrict__ qp,
    const float *__restrict__ q32, const float *__restrict__ out_t, const int32_t *__restrict__ idx_t,
    float *__restrict__ mul, float *__restrict__ parts, int64_t L, int64_t max_len, int Hkv, int G, int hpw, int n_out,
    int pos_offset, float rope_theta, float inv, int n_parts, const float *__restrict__ rt_freq, float rt_af) {
  constexpr int N = 1 << BITS;
  constexpr int WPH = kHeadDim / 32 * BITS;
  extern __shared__ float tab[];
  const int h0 = blockIdx.y * hpw;
  const int nh = (Hkv - h0 < hpw) ? Hkv - h0 : hpw;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t wt0 = (int64_t)blockIdx.x * blockDim.x + wave * 64;    // first token of this wave
  const int64_t t = wt0 + lane;
  const bool valid = t < L;
  const int64_t tc = valid ? t : L - 1;
  for (int e = threadIdx.x; e < nh * kHeadDim * N; e += blockDim.x) tab[e] = lut[(int64_t)h0 * kHeadDim * N + e];
  __syncthreads();
  if (wt0 >= L) return;   // (no barrier below)

  const float th_reg = RT ? rt_freq[lane] : rope_freq(rope_theta, lane);   // theta_j in lane j
  const float posf = (float)((int)tc + pos_offset);
  // (every index into acc is a compile-time constant: static_for, so that the array lives in registers)
  float acc[kGqaMaxHpw * GB];
  static_for<0, kGqaMaxHpw * GB>([&](auto I) __attribute__((always_inline)) { acc[decltype(I)::value] = 0.f; });

  static_for<0, 2>([&](auto R) __attribute__((always_inline)) {
    constexpr int role = decltype(R)::value;    // pairs k_lo = 32*role + i, i < 32
    float cv[32], sv[32];
    static_for<0, 32>([&](auto I) __attribute__((always_inline)) {
      constexpr int i = decltype(I)::value;
      sincos_rev(__shfl(th_reg, role * 32 + i) * posf, sv[i], cv[i]);
      if constexpr (RT) {
        sv[i] *= rt_af;
        cv[i] *= rt_af;
      }
    });
    static_for<0, kGqaMaxHpw>([&](auto HH) __attribute__((always_inline)) {
      constexpr int hh = decltype(HH)::value;
      if (hh < nh) {
        const uint32_t *hb = mat + (int64_t)(h0 + hh) * WPH * max_len + tc;
        uint32_t wlo[BITS], whi[BITS];
#pragma unroll
        for (int w = 0; w < BITS; w++) {
          wlo[w] = hb[(int64_t)(role * BITS + w) * max_len];
          whi[w] = hb[(int64_t)((role + 2) * BITS + w) * max_len];
        }
        const float *tl = tab + hh * kHeadDim * N;
        const float *qh = qp + ((int64_t)(h0 + hh) * 64 + role * 32) * 2 * GB;
        static_for<0, 32>([&](auto I) __attribute__((always_inline)) {
          constexpr int i = decltype(I)::value;
          constexpr int klo = role * 32 + i, khi = klo + 64;
          const float Klo = tl[klo * N + code_of<BITS, i>(wlo)];
          const float Khi = tl[khi * N + code_of<BITS, i>(whi)];
          const float rlo = fmaf(cv[i], Klo, -(sv[i] * Khi));
          const float rhi = fmaf(sv[i], Klo, cv[i] * Khi);
          static_for<0, GB>([&](auto Gi) __attribute__((always_inline)) {
            constexpr int g = decltype(Gi)::value;
            acc[hh * GB + g] = fmaf(qh[i * 2 * GB + g], rlo, fmaf(qh[i * 2 * GB + GB + g], rhi, acc[hh * GB + g]));
          });
        });
      }
    });
  });

  // K outlier entries of this lane's token (mirror [n_out][max_len]) that belong to the group's KV heads
  if (idx_t != nullptr) {
    for (int s2 = 0; s2 < n_out; s2++) {
      const int col = idx_t[(int64_t)s2 * max_len + tc];
      const float val = out_t[(int64_t)s2 * max_len + tc];
      const int ch = col & (kHeadDim - 1);
      const float th = __shfl(th_reg, ch & 63);   // (all lanes active)
      const int hk = (col >> 7) - h0;
      if (valid && val != 0.f && (unsigned)hk < (unsigned)nh) {
        float sn, c;
        sincos_rev(th * posf, sn, c);
        if constexpr (RT) {
          sn *= rt_af;
          c *= rt_af;
        }
        const float sg = ch < 64 ? sn : -sn;
        const float *qk = q32 + (int64_t)(h0 + hk) * G * kHeadDim;
        static_for<0, GB>([&](auto Gi) __attribute__((always_inline)) {
          constexpr int g = decltype(Gi)::value;
          const float x = g < G ? val * fmaf(c, qk[g * kHeadDim + ch], sg * qk[g * kHeadDim + (ch ^ 64)]) : 0.f;
          static_for<0, kGqaMaxHpw>([&](auto HH) __attribute__((always_inline)) {
            constexpr int hh = decltype(HH)::value;
            acc[hh * GB + g] += hk == hh ? x : 0.f;   // (a select, not a branch: acc stays in registers)
          });
        });
      }
    }
  }

  // raw scores [Hq][L] and the first softmax pass per (query head, 64-token wave)
  const int64_t chunk = wt0 / kGqaPT;
  static_for<0, kGqaMaxHpw>([&](auto HH) __attribute__((always_inline)) {
    constexpr int hh = decltype(HH)::value;
    if (hh < nh) {
      static_for<0, GB>([&](auto Gi) __attribute__((always_inline)) {
        constexpr int g = decltype(Gi)::value;
        if (g < G) {
          const int64_t hq = (int64_t)(h0 + hh) * G + g;
          if (valid) mul[hq * L + t] = acc[hh * GB + g];
          if (parts != nullptr && chunk < n_parts) {
            const float x = valid ? scaled(acc[hh * GB + g], inv) : -INFINITY;
            const float m = gqa_wave_max(x);
            const float e = valid ? __builtin_amdgcn_exp2f((x - m) * 1.4426950408889634f) : 0.f;
            const float s = gqa_wave_sum(e);
            if (lane == 0) {
              parts[(hq * n_parts + chunk) * 2] = m;
              parts[(hq * n_parts + chunk) * 2 + 1] = s;
            }
          }
        }
      });
    }
  });
}

template <int BITS, int GB>
__global__ __launch_bounds__(256) void gqa_score_kernel(
    const uint32_t *__restrict__ mat, const float *__restrict__ lut, const float *__restrict__ qp,
    const float *__restrict__ q32, const float *__restrict__ out_t, const int32_t *__restrict__ idx_t,
    float *__restrict__ mul, float *__restrict__ parts, int64_t L, int64_t max_len, int Hkv, int G, int hpw, int n_out,
    int pos_offset, float rope_theta, float inv, int n_parts) {
  gqa_score_body<BITS, GB, false>(mat, lut, qp, q32, out_t, idx_t, mul, parts, L, max_len, Hkv, G, hpw, n_out, pos_offset,
                                  rope_theta, inv, n_parts, nullptr, 1.f);
}

template <int BITS, int GB>
__global__ __launch_bounds__(256) void gqa_score_kernel_rt(
    const uint32_t *__restrict__ mat, const float *__restrict__ lut, const float *__restrict__ qp,
    const float *__restrict__ q32, const float *__restrict__ out_t, const int32_t *__restrict__ idx_t,
    float *__restrict__ mul, float *__restrict__ parts, int64_t L, int64_t max_len, int Hkv, int G, int hpw, int n_out,
    int pos_offset, float inv, int n_parts, const float *__restrict__ rt_freq, float rt_af) {
  gqa_score_body<BITS, GB, true>(mat, lut, qp, q32, out_t, idx_t, mul, parts, L, max_len, Hkv, G, hpw, n_out, pos_offset,
                                 0.f, inv, n_parts, rt_freq, rt_af);
}

// grid (token chunks, Hkv), 256 lanes: wave w, lane l -> channel octet o = 4w + l/16 (channels 8o .. 8o+7), token quad
// l%16 of each 64-token step.  dst: out (one chunk) or the chunk's slab [Hq][128].
template <int BITS, int GB>
__global__ __launch_bounds__(256) void gqa_mix_kernel(const float *__restrict__ p, const uint32_t *__restrict__ mat,
                                                      const float *__restrict__ lut_rows, const float *__restrict__ vout,
                                                      const int32_t *__restrict__ vidx, float *__restrict__ dst,
                                                      int64_t L, int64_t max_len, int64_t ct, int Hq, int G, int n_out,
                                                      int accumulate, int n_chunks) {
  constexpr int N = 1 << BITS;
  constexpr int WPH = kHeadDim / 32 * BITS;
  // (row stride N + 1: the 16 lanes of an octet read rows 4 tokens apart, which a stride of N would put in ONE bank)
  constexpr int RS = N + 1;
  __shared__ float lrow[kGqaMixBT * RS];
  __shared__ float pl[GB * kGqaMixBT];
  __shared__ unsigned long long sacc[GB * kHeadDim];
  const int kv = blockIdx.y, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int oct = wave * 4 + (lane >> 4), quad = lane & 15;
  const int64_t t0 = (int64_t)blockIdx.x * ct;
  const int64_t t1 = (t0 + ct < L) ? t0 + ct : L;
  for (int i = tid; i < GB * kHeadDim; i += 256) sacc[i] = 0ull;
  // the packed rows this lane reads and where its 8 codes sit in them
  int row0, shift;
  bool two;
  if constexpr (BITS == 4) {
    row0 = oct; shift = 0; two = false;
  } else if constexpr (BITS == 2) {
    row0 = oct >> 1; shift = (oct & 1) * 16; two = false;
  } else {
    const int sub = oct & 3;   // 24 bits at bit 24*sub of the group's 96-bit word triple
    row0 = (oct >> 2) * 3 + ((sub * 24) >> 5);
    shift = (sub * 24) & 31;
    two = shift + 24 > 32;
  }
  const uint32_t *mrow = mat + ((int64_t)kv * WPH + row0) * max_len;
  float acc[GB * 8];
  static_for<0, GB * 8>([&](auto I) __attribute__((always_inline)) { acc[decltype(I)::value] = 0.f; });
  const float *prow = p + (int64_t)kv * G * L;

  for (int64_t tb = t0; tb < t1; tb += kGqaMixBT) {
    const int nt = (t1 - tb < kGqaMixBT) ? (int)(t1 - tb) : kGqaMixBT;
    __syncthreads();   // the previous block's stage is consumed
    for (int e = tid; e < kGqaMixBT * N; e += 256) lrow[(e / N) * RS + e % N] = (e / N < nt) ? lut_rows[tb * N + e] : 0.f;
    for (int e = tid; e < GB * kGqaMixBT; e += 256) {
      const int g = e / kGqaMixBT, tok = e % kGqaMixBT;
      pl[e] = (g < G && tok < nt) ? prow[(int64_t)g * L + tb + tok] : 0.f;
    }
    __syncthreads();
    for (int st = 0; st * 64 < nt; st++) {
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int tok = st * 64 + quad * 4 + u;
        if (tok < nt) {
          const int64_t tt = tb + tok;
          uint32_t x = mrow[tt] >> shift;
          if (BITS == 3 && two) x |= mrow[tt + max_len] << (32 - shift);
          float pv[GB];
          static_for<0, GB>([&](auto Gi) __attribute__((always_inline)) { pv[decltype(Gi)::value] = pl[decltype(Gi)::value * kGqaMixBT + tok]; });
          static_for<0, 8>([&](auto K) __attribute__((always_inline)) {
            constexpr int k = decltype(K)::value;
            const float vv = lrow[tok * RS + ((x >> (BITS * k)) & (N - 1))];
            static_for<0, GB>([&](auto Gi) __attribute__((always_inline)) {
              constexpr int g = decltype(Gi)::value;
              acc[g * 8 + k] = fmaf(vv, pv[g], acc[g * 8 + k]);
            });
          });
        }
      }
    }
    // V outlier entries of the block's tokens that belong to this KV head: 32.32 fixed point into LDS
    if (vidx != nullptr) {
      const int nent = nt * n_out;
      const int64_t e0 = tb * n_out;
      for (int e = tid; e < nent; e += 256) {
        const int col = vidx[e0 + e];
        const float val = vout[e0 + e];
        if (val != 0.f && (col >> 7) == kv) {
          const int tok = e / n_out, c = col & (kHeadDim - 1);
#pragma unroll
          for (int g = 0; g < GB; g++) {
            if (g < G) {
              const float xv = val * pl[g * kGqaMixBT + tok];
              const float fl = floorf(xv);
              const unsigned lo = (unsigned)((xv - fl) * 4294967296.0f);
              const unsigned long long fx = ((unsigned long long)(unsigned)(int)fl << 32) | lo;
              atomicAdd(&sacc[g * kHeadDim + c], fx);
            }
          }
        }
      }
    }
  }
  // the 16 token quads of an octet -> one sum per channel (fixed shuffle order)
  static_for<0, GB * 8>([&](auto I) __attribute__((always_inline)) {
    constexpr int i = decltype(I)::value;
    float v = acc[i];
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 8);
    acc[i] = v;
  });
  __syncthreads();   // outlier sums complete
  if (quad == 0) {
    static_for<0, GB>([&](auto Gi) __attribute__((always_inline)) {
      constexpr int g = decltype(Gi)::value;
      if (g < G) {
        const int hq = kv * G + g;
        float *o = n_chunks == 1 ? dst + (int64_t)hq * kHeadDim : dst + ((int64_t)blockIdx.x * Hq + hq) * kHeadDim;
        static_for<0, 8>([&](auto K) __attribute__((always_inline)) {
          constexpr int k = decltype(K)::value;
          const int c = oct * 8 + k;
          float r = acc[g * 8 + k] + (float)((double)(long long)sacc[g * kHeadDim + c] * 0x1p-32);
          if (n_chunks == 1 && accumulate) r += o[c];
          o[c] = r;
        });
      }
    });
  }
}

// out[i] (+)= sum over the chunks' slabs, in chunk order
__global__ __launch_bounds__(256) void gqa_mix_reduce_kernel(const float *__restrict__ slabs, float *__restrict__ out,
                                                             int n, int n_chunks, int accumulate) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int c = 0; c < n_chunks; c++) s += slabs[(int64_t)c * n + i];
  out[i] = accumulate ? out[i] + s : s;
}

// launch plan of the score kernel: KV heads per workgroup (shares the (cos, sin) of a token) and waves per workgroup
static void gqa_score_plan(int Hkv, int64_t L, int &hpw, int &nw) {
  const int64_t waves = (L + 63) / 64;
  hpw = Hkv < kGqaMaxHpw ? Hkv : kGqaMaxHpw;
  while (hpw > 1 && waves * ((Hkv + hpw - 1) / hpw) < 2048) hpw >>= 1;   // >= 8 waves per CU before sharing
  const int64_t groups = (Hkv + hpw - 1) / hpw;
  nw = 4;
  while (nw > 1 && ((waves + nw - 1) / nw) * groups < 512) nw >>= 1;     // >= 2 workgroups per CU on 256 CUs
}

// p.V: token chunks per KV head (about 1024 workgroups; a chunk is a multiple of 64 tokens)
static void gqa_mix_plan(int Hkv, int64_t L, int &n_chunks, int64_t &ct) {
  const int64_t blocks = (L + 63) / 64;
  int64_t n = (1024 + Hkv - 1) / Hkv;
  if (n > blocks) n = blocks;
  if (n < 1) n = 1;
  ct = ((L + n - 1) / n + 63) / 64 * 64;
  n_chunks = (int)((L + ct - 1) / ct);
}

// the G buckets the kernels are instantiated for (gqa_bucket)
template <class F>
static void with_gb(int GB, F &&f) {
  with_int<8, 4, 2, 1>(GB, f);
}

}  // namespace kvq

using namespace kvq;

extern "C" {

int kvq_gqa_supported(int Hq, int Hkv, int hd) { return gqa_shape_ok(Hq, Hkv, hd) ? 1 : 0; }

size_t kvq_score_k_gqa_workspace_bytes(int bits, int Hq, int Hkv) {
  if (bits < 2 || bits > 4 || !gqa_shape_ok(Hq, Hkv, kHeadDim)) return 0;
  return gqa_score_ws(Hq, Hkv);
}

int kvq_score_k_gqa_parts(int64_t L) { return L > 0 ? (int)((L + kGqaPT - 1) / kGqaPT) : 0; }

int kvq_score_k_gqa(int bits, const void *q, int q_is_half, const int32_t *mat, float *mul, const float *lut, int Hq,
                    int Hkv, int hd, int64_t L, int64_t max_len, float rope_theta, int pos_offset, const float *outliers_t,
                    const int32_t *outlier_idx_t, int n_out, float inv_sqrt_hd, float *softmax_parts, int n_parts,
                    void *workspace, size_t workspace_bytes, void *stream) {
  return kvq_score_k_gqa_rope(bits, q, q_is_half, mat, mul, lut, Hq, Hkv, hd, L, max_len, rope_theta, pos_offset,
                              outliers_t, outlier_idx_t, n_out, inv_sqrt_hd, softmax_parts, n_parts, workspace,
                              workspace_bytes, nullptr, stream);
}

int kvq_score_k_gqa_rope(int bits, const void *q, int q_is_half, const int32_t *mat, float *mul, const float *lut, int Hq,
                         int Hkv, int hd, int64_t L, int64_t max_len, float rope_theta, int pos_offset,
                         const float *outliers_t, const int32_t *outlier_idx_t, int n_out, float inv_sqrt_hd,
                         float *softmax_parts, int n_parts, void *workspace, size_t workspace_bytes, const kvq_rope *rope,
                         void *stream) {
  if (bits < 2 || bits > 4 || !gqa_shape_ok(Hq, Hkv, hd) || !q || !mat || !mul || !lut || !rope_ok(rope))
    return KVQ_EINVAL;
  if (L <= 0 || L > max_len || max_len >= (1ll << 31) || pos_offset < 0) return KVQ_EINVAL;
  // token-contiguous mirror with values (the compact format is not taken), or no outliers at all
  if ((outliers_t == nullptr) != (outlier_idx_t == nullptr) || (outlier_idx_t && n_out <= 0) || n_out < 0) return KVQ_EINVAL;
  if (softmax_parts && n_parts != kvq_score_k_gqa_parts(L)) return KVQ_EINVAL;
  if (!workspace || workspace_bytes < gqa_score_ws(Hq, Hkv) || reinterpret_cast<uintptr_t>(workspace) % 16)
    return KVQ_EWORKSPACE;
  const int G = Hq / Hkv, GB = gqa_bucket(G);
  hipStream_t st = (hipStream_t)stream;
  float *q32 = reinterpret_cast<float *>(workspace);
  float *qp = reinterpret_cast<float *>(reinterpret_cast<unsigned char *>(workspace) + gqa_q32_bytes(Hq));
  const int nprep = Hkv * kHeadDim * GB;
  with_gb(GB, [&](auto B) {
    gqa_qprep_kernel<decltype(B)::value><<<(nprep + 255) / 256, 256, 0, st>>>(q, q_is_half, q32, qp, Hq, Hkv, G);
  });
  int rc = check_launch();
  if (rc) return rc;
  int hpw, nw;
  gqa_score_plan(Hkv, L, hpw, nw);
  const int64_t tiles = (L + nw * 64 - 1) / (nw * 64);
  dim3 grid((unsigned)tiles, (unsigned)((Hkv + hpw - 1) / hpw)), block(nw * 64);
  const size_t lds = (size_t)hpw * kHeadDim * (1u << bits) * 4;
  const uint32_t *m = reinterpret_cast<const uint32_t *>(mat);
  const int np = softmax_parts ? n_parts : 0;
  with_bits(bits, [&](auto BITS) {
    with_gb(GB, [&](auto B) {
      constexpr int bt = decltype(BITS)::value, gb = decltype(B)::value;
      if (rope)
        gqa_score_kernel_rt<bt, gb><<<grid, block, lds, st>>>(m, lut, qp, q32, outliers_t, outlier_idx_t, mul, softmax_parts,
                                                              L, max_len, Hkv, G, hpw, n_out, pos_offset, inv_sqrt_hd, np,
                                                              rope->inv_freq, rope->attention_factor);
      else
        gqa_score_kernel<bt, gb><<<grid, block, lds, st>>>(m, lut, qp, q32, outliers_t, outlier_idx_t, mul, softmax_parts, L,
                                                           max_len, Hkv, G, hpw, n_out, pos_offset, rope_theta, inv_sqrt_hd,
                                                           np);
    });
  });
  return check_launch();
}

size_t kvq_mix_v_gqa_workspace_bytes(int bits, int Hq, int Hkv, int hd, int64_t L) {
  if (bits < 2 || bits > 4 || !gqa_shape_ok(Hq, Hkv, hd) || L <= 0) return 0;
  int n_chunks;
  int64_t ct;
  gqa_mix_plan(Hkv, L, n_chunks, ct);
  return n_chunks > 1 ? (size_t)n_chunks * Hq * kHeadDim * 4 : 16;
}

int kvq_mix_v_gqa(int bits, const float *p, const int32_t *mat, float *mul, const float *lut_rows, int Hq, int Hkv, int hd,
                  int64_t L, int64_t max_len, const float *outliers, const int32_t *outlier_idx, int n_out, int accumulate,
                  void *workspace, size_t workspace_bytes, void *stream) {
  if (bits < 2 || bits > 4 || !gqa_shape_ok(Hq, Hkv, hd) || !p || !mat || !mul || !lut_rows) return KVQ_EINVAL;
  if (L <= 0 || L > max_len) return KVQ_EINVAL;
  if ((outliers == nullptr) != (outlier_idx == nullptr) || (outlier_idx && n_out <= 0) || n_out < 0) return KVQ_EINVAL;
  if (outlier_idx && L * n_out >= (1ll << 31)) return KVQ_EINVAL;
  int n_chunks;
  int64_t ct;
  gqa_mix_plan(Hkv, L, n_chunks, ct);
  if (!workspace || workspace_bytes < kvq_mix_v_gqa_workspace_bytes(bits, Hq, Hkv, hd, L)) return KVQ_EWORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int G = Hq / Hkv, GB = gqa_bucket(G);
  float *dst = n_chunks == 1 ? mul : reinterpret_cast<float *>(workspace);
  dim3 grid((unsigned)n_chunks, (unsigned)Hkv);
  const uint32_t *m = reinterpret_cast<const uint32_t *>(mat);
  with_bits(bits, [&](auto BITS) {
    with_gb(GB, [&](auto B) {
      gqa_mix_kernel<decltype(BITS)::value, decltype(B)::value><<<grid, 256, 0, st>>>(
          p, m, lut_rows, outliers, outlier_idx, dst, L, max_len, ct, Hq, G, n_out, accumulate, n_chunks);
    });
  });
  const int rc = check_launch();
  if (rc || n_chunks == 1) return rc;
  const int n = Hq * kHeadDim;
  gqa_mix_reduce_kernel<<<(n + 255) / 256, 256, 0, st>>>(dst, mul, n, n_chunks, accumulate);
  return check_launch();
}

}  // extern "C"
