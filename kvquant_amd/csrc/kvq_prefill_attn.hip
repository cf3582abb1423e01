// Causal self-attention of the prompt (prefill) on the matrix cores: the one true dense contraction of the
// hot path (BASELINE config 4).  The reference calls flash-attn here (ML:1861-1874 -> 2013-2070, third party);
// this is a flash-style kernel written for gfx950: fp16 inputs, fp32 accumulation on
// v_mfma_f32_32x32x16_f16, online softmax, no S x S matrix in memory.
//
// Decomposition: workgroup = 8 waves = 256 query rows of one head; wave = 32 query rows; keys / values arrive in
// 64-key tiles shared by the waves through LDS (double buffered, one barrier per tile) in the layouts of the tile step
// (kvq_flash_tile.h: the transposed products, the online softmax).
// Causal mask only on the tiles that cross the diagonal; heavy (late) query blocks are scheduled first.
#include "kvq_common.h"
#include "kvq_flash_tile.h"
#include "kvq_host.h"

namespace kvq {

using namespace flash;

#ifndef KVQ_ATTN_WAVES
#define KVQ_ATTN_WAVES 8
#endif
constexpr int kAW = KVQ_ATTN_WAVES;           // waves per workgroup
constexpr int kQW = kQB * kAW;   // query rows per workgroup
constexpr int kKTile = kKV * kKRow;      // 16384
constexpr int kVTile = kD * kVRow;       // 17408
constexpr int kStage = kKTile + kVTile;  // 33792

struct AttnArgs {
  const f16 *q, *k, *v;   // element [h][s][d] at h * stride_h + s * stride_s + d
  f16 *o;
  int64_t qsh, qss, ksh, kss, vsh, vss, osh, oss;
  int S, H;
  float scale_log2e;      // softmax scale * log2(e)
  int G;                  // GQA: query heads per KV head (the GQA instantiation reads K / V of head h / G)
};

template <bool GQA>
__global__ __launch_bounds__(kAW * 64, 2) void prefill_attn_kernel(AttnArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * kStage];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hi = lane >> 5, ql = lane & 31;
  // heavy (late, long-row) query blocks of ALL heads first: the grid is walked in dispatch order
  const int nqb = (a.S + kQW - 1) / kQW;
  const int h = (int)blockIdx.x % a.H;
  const int qb = nqb - 1 - (int)blockIdx.x / a.H;
  const int q0w = qb * kQW;                            // first query row of the workgroup
  const int q0 = q0w + wave * kQB;                     // ... of this wave
  const int qrow = q0 + ql;                            // this lane's query row
  const int qrc = qrow < a.S ? qrow : a.S - 1;
  const int hk = GQA ? h / a.G : h;                    // KV head of this query head
  const f16 *kh = a.k + (int64_t)hk * a.ksh;
  const f16 *vh = a.v + (int64_t)hk * a.vsh;

  f16x8 qf[8];
  load_q(a.q + (int64_t)h * a.qsh + (int64_t)qrc * a.qss, hi, qf);
  f32x16 oacc[4];
  float m_run, l_run;
  reset(oacc, m_run, l_run);

  const int kv_end = (q0w + kQW < a.S ? q0w + kQW : a.S);     // keys [0, kv_end) matter to this workgroup
  const int n_tiles = (kv_end + kKV - 1) / kKV;

  // ---- staging: thread -> (key = tid & 63, 16-byte chunks c = (tid >> 6) + kAW j, j < 16 / kAW) of K and V
  constexpr int NCH = 16 / kAW;
  const int skey = tid & 63, sc0 = tid >> 6;
  u32x4 kreg[NCH], vreg[NCH];
  auto load_tile = [&](int t) __attribute__((always_inline)) {
    int key = t * kKV + skey;
    if (key >= a.S) key = a.S - 1;
    const f16 *kp = kh + (int64_t)key * a.kss;
    const f16 *vp = vh + (int64_t)key * a.vss;
#pragma unroll
    for (int j = 0; j < NCH; j++) {
      kreg[j] = *reinterpret_cast<const u32x4 *>(kp + (sc0 + kAW * j) * 8);
      vreg[j] = *reinterpret_cast<const u32x4 *>(vp + (sc0 + kAW * j) * 8);
    }
  };
  auto store_tile = [&](int stage) __attribute__((always_inline)) {
    unsigned char *ks = smem + stage * kStage;
    unsigned char *vs = ks + kKTile;
#pragma unroll
    for (int j = 0; j < NCH; j++) {
      const int c = sc0 + kAW * j;                                      // 16-byte chunk (8 d values)
      *reinterpret_cast<u32x4 *>(ks + skey * kKRow + ((c ^ (skey & 15)) << 4)) = kreg[j];
      // (the eight halves cut out of the four words: no pointer into the staging registers)
      const uint32_t wv[4] = {vreg[j].x, vreg[j].y, vreg[j].z, vreg[j].w};
#pragma unroll
      for (int i = 0; i < 8; i++)
        *reinterpret_cast<unsigned short *>(vs + (c * 8 + i) * kVRow + skey * 2) = (unsigned short)(wv[i >> 1] >> (16 * (i & 1)));
    }
  };

  load_tile(0);
  store_tile(0);
  __syncthreads();

  for (int t = 0; t < n_tiles; t++) {
    const int stage = t & 1;
    if (t + 1 < n_tiles) load_tile(t + 1);               // in flight during the math
    const int key0 = t * kKV;
    // a wave whose rows all lie before this tile has nothing to add (causal); it still takes part in the staging
    if (key0 <= q0 + kQB - 1) {
      const unsigned char *ks = smem + stage * kStage;
      const bool diag = key0 + kKV - 1 > q0 || key0 + kKV > a.S;       // tile crosses the diagonal / the end
      tile_step(ks, ks + kKTile, qf, oacc, m_run, l_run, a.scale_log2e, diag, hi, ql,
                [&](int kb, int r) __attribute__((always_inline)) {
                  const int key = key0 + kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                  return key <= qrow && key < a.S;
                });
    }
    if (t + 1 < n_tiles) store_tile(1 - stage);     // the other stage: free since the barrier of the previous tile
    __syncthreads();
  }

  // ---- normalise and write O[q][d] (fp16): accumulator reg r of block db is d = db*32 + (r&3) + 8(r>>2) + 4hi
  if (qrow < a.S) {
    const float inv = l_run > 0.f ? 1.0f / l_run : 0.f;
    f16 *op = a.o + (int64_t)h * a.osh + (int64_t)qrow * a.oss;
#pragma unroll
    for (int db = 0; db < 4; db++)
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const int d = db * 32 + 8 * g + 4 * hi;
        uint2 w;
        w.x = pack_f16(oacc[db][4 * g] * inv, oacc[db][4 * g + 1] * inv);
        w.y = pack_f16(oacc[db][4 * g + 2] * inv, oacc[db][4 * g + 3] * inv);
        *reinterpret_cast<uint2 *>(op + d) = w;
      }
  }
}

static int prefill_launch(bool gqa, const void *q, const void *k, const void *v, void *out, int H, int G, int S, int hd,
                          int64_t q_stride_h, int64_t q_stride_s, int64_t k_stride_h, int64_t k_stride_s,
                          int64_t v_stride_h, int64_t v_stride_s, int64_t o_stride_h, int64_t o_stride_s,
                          float softmax_scale, void *stream) {
  if (!q || !k || !v || !out || H <= 0 || S <= 0 || hd != kD) return KVQ_EINVAL;
  // 16-byte row segments are loaded / stored as vectors
  if ((q_stride_h | q_stride_s | k_stride_h | k_stride_s | v_stride_h | v_stride_s) % 8 || (o_stride_h | o_stride_s) % 4 ||
      (reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v)) % 16 ||
      reinterpret_cast<uintptr_t>(out) % 8)
    return KVQ_EINVAL;
  AttnArgs a;
  a.q = reinterpret_cast<const f16 *>(q);
  a.k = reinterpret_cast<const f16 *>(k);
  a.v = reinterpret_cast<const f16 *>(v);
  a.o = reinterpret_cast<f16 *>(out);
  a.qsh = q_stride_h; a.qss = q_stride_s; a.ksh = k_stride_h; a.kss = k_stride_s;
  a.vsh = v_stride_h; a.vss = v_stride_s; a.osh = o_stride_h; a.oss = o_stride_s;
  a.S = S;
  a.H = H;
  a.G = G;
  a.scale_log2e = softmax_scale * 1.4426950408889634f;
  dim3 grid((unsigned)((S + kQW - 1) / kQW) * (unsigned)H), block(kAW * 64);
  if (gqa) prefill_attn_kernel<true><<<grid, block, 0, (hipStream_t)stream>>>(a);
  else prefill_attn_kernel<false><<<grid, block, 0, (hipStream_t)stream>>>(a);
  return check_launch();
}

}  // namespace kvq

using namespace kvq;

extern "C" {

int kvq_prefill_attention(const void *q, const void *k, const void *v, void *out, int H, int S, int hd,
                          int64_t q_stride_h, int64_t q_stride_s, int64_t k_stride_h, int64_t k_stride_s,
                          int64_t v_stride_h, int64_t v_stride_s, int64_t o_stride_h, int64_t o_stride_s,
                          float softmax_scale, void *stream) {
  return prefill_launch(false, q, k, v, out, H, 1, S, hd, q_stride_h, q_stride_s, k_stride_h, k_stride_s, v_stride_h,
                        v_stride_s, o_stride_h, o_stride_s, softmax_scale, stream);
}

int kvq_prefill_attention_gqa(const void *q, const void *k, const void *v, void *out, int Hq, int Hkv, int S, int hd,
                              int64_t q_stride_h, int64_t q_stride_s, int64_t k_stride_h, int64_t k_stride_s,
                              int64_t v_stride_h, int64_t v_stride_s, int64_t o_stride_h, int64_t o_stride_s,
                              float softmax_scale, void *stream) {
  if (Hq <= 0 || Hkv <= 0 || Hq % Hkv || Hq / Hkv > 8) return KVQ_EINVAL;
  return prefill_launch(true, q, k, v, out, Hq, Hq / Hkv, S, hd, q_stride_h, q_stride_s, k_stride_h, k_stride_s, v_stride_h,
                        v_stride_s, o_stride_h, o_stride_s, softmax_scale, stream);
}

}  // extern "C"
