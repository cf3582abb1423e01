// Attention of a chunk of S new tokens over the COMPRESSED cache on the matrix cores (ABI 404): multi-turn follow-up
// prompts, draft verification and chunked fills after the first chunk.  The chunk has already been packed into columns
// c0 .. c0+S-1 by the fused packs; query i (RoPE'd at position sinks + c0 + i) attends to the fp16 sink tokens and to the
// compressed columns [0, c0 + i].
//
// Structure of kvq_prefill_attn.hip (fp16 operands on v_mfma_f32_32x32x16_f16, fp32 accumulation, online softmax, no
// S x L matrix in memory, both products computed transposed so that a lane owns one query row); what differs is where the
// K / V tiles come from.  Per 64-column tile the workgroup (8 waves = 256 query rows of one query head) decodes the tile
// itself, once for its 256 rows:
//   P0  the tile's V codebook rows -> LDS; every thread loads the packed words of its (column, 32-channel group)
//       (token-contiguous rows: a wave reads 64 consecutive columns of one word row -- coalesced);
//   P1  waves 0-3: K codes -> the head's per-channel codebook (LDS) -> fp32 K stage; waves 4-7: V codes -> the column's
//       own codebook row -> fp32 V stage;
//   P2  outlier residuals of this KV head added into the stages (K: token-contiguous mirror [n_out][max_len], V: reference
//       rows [max_len][n_out]; ids are global channels);
//   P3  waves 0-3: RoPE of each (k, k+64) pair at the column's position (sincos_rev, the angle rule of the decode
//       kernels) -> fp16 K tile in the XOR-swizzled layout of the prefill kernel; waves 4-7: fp16 V^T tile;
//   then the tile step both kernels share (kvq_flash_tile.h): S^T = K.Q^T, mask, online softmax, O^T += V^T.P^T.
// The fp16 sink tokens (post-RoPE K [Hkv][128][n_sink], V [Hkv][n_sink][128]) are one prefix tile without decode.
// The causal mask is evaluated only on tiles that reach past the wave's first row (c0 + q0) or past the last column.
//
// Parallelism: (query head x 256-row block) is 64 workgroups at Hq = 32, S = 512, so the column range is also split
// across workgroups; each split writes (max, sum, unnormalised O) partials and chunk_attn_merge_kernel merges the splits
// of a row in a fixed order (deterministic).  GQA: query head h reads KV head h / G (the tile is decoded per query head).
//
// Grouped variant (GR, kvq_chunk_attention_grouped: G >= 2, S <= 32 -- draft verification): a workgroup belongs to one KV
// head and one split; wave w < G owns the S rows of query head hk * G + w (one 32-row MFMA block, rows >= S clamped
// duplicates that are never written), waves >= G own no rows but decode with the others.  The tile is then decoded ONCE
// for the G heads of the group instead of once per query head; partials and merge are unchanged.
//
// Tree variant (TR, kvq_chunk_attention_tree: the grouped geometry, 1 <= G <= 8, 2 <= S <= 32 -- verification of a draft
// TREE): the chunk's rows are the nodes of a tree in topological order (row 0 the root).  Row i sees every column < c0
// and column c0 + j iff node j is i itself or one of its ancestors (bit j of anc[i]); column c0 + j rotates at the
// position of its DEPTH, pos_offset + c0 + depth[j], so siblings share a position.  anc / depth ride in the kernel
// arguments (Args::tree).  A chain (parent[i] = i - 1) is the grouped kernel, bit for bit.
//
// Window variant (WN, kvq_chunk_attention_window[_grouped]: sliding-window attention over a RING of C = max_len columns,
// per-head and grouped geometries): compressed token n lives in column n mod C, the chunk's tokens n0 .. n0+S-1 are
// already packed, N = n0 + S.  The resident columns are c < min(N, C); column c holds token
// n(c) = c + C * floor((N - 1 - c) / C) = c + base - (c > r ? C : 0), base = C * ((N - 1) / C), r = (N - 1) % C (host),
// and rotates at pos_offset + n(c).  Row i sees the sinks and column c iff n0 + i - W < n(c) <= n0 + i.  A ring tile may
// be masked in part anywhere: a wave takes the mask on every tile that is not visible in full to all of its rows and
// skips one that none of them sees (a masked tile that is not skipped adds exact zeros to the running sums); every
// workgroup decodes all resident tiles of its split.  The split plan counts the resident tiles, partials and merge are
// unchanged.  With N <= C and W >= N the statements reduce to the plain kernel's, bit for bit.
//
// kvq_keep_columns (end of the file): after a tree round the accepted root-to-leaf path moves into contiguous columns
// -- a copy of packed words, codebook rows and outlier rows; the keys are stored pre-RoPE, nothing is re-rotated.
#include "kvq_common.h"
#include "kvq_flash_tile.h"
#include "kvq_host.h"

namespace kvq {
namespace chunk {

using namespace flash;

constexpr int kAW = 8;             // waves per workgroup
constexpr int kThreads = kAW * 64;
constexpr int kQW = kQB * kAW;     // query rows per workgroup
constexpr int kSR = kD + 4;        // floats per column of the fp32 stages
constexpr int kMaxSink = 64;       // the sink tokens fit one tile
constexpr int kTargetWorkgroups = 512;
constexpr int kMinTilesPerSplit = 4;
constexpr int kMaxSplits = 64;
constexpr int kMaxS = 65536;
constexpr size_t kMaxWorkspace = size_t(1) << 30;

// TR: the tree of a chunk of S <= 32 rows
struct Tree {
  uint32_t anc[kQB];                 // bit j of anc[i]: node j is i or an ancestor of i
  uint8_t depth[kQB];                // edges from the root (row 0)
};

struct Args {
  const int32_t *kmat, *vmat;
  const float *klut;                 // [Hkv][128][2^bits]: the table the scores dequantise with
  const float *kout_t;               // K outlier mirror [n_out][max_len]
  const int32_t *kidx_t;
  const float *vrows;                // [max_len][2^bits]: the rows p.V dequantises with
  const float *vout;                 // V outlier rows [max_len][n_out]
  const int32_t *vidx;
  const f16 *q;                      // [Hq][S][128] at h * qsh + s * qss
  int64_t qsh, qss;
  const f16 *k_sink, *v_sink;        // [Hkv][128][n_sink], [Hkv][n_sink][128]
  float *part_o, *part_ml;           // [Hq][nsplit][S][128], [Hq][nsplit][S][2]
  int64_t max_len, c0;
  int Hq, G, S, n_sink, n_out, pos_offset, nqb, nsplit, tps;
  float rope_theta, scale_log2e;
  const float *rt_freq;              // RT (scaled RoPE, kvq.h: kvq_rope): the K tiles rotate with the frequencies rt_freq
  float rt_af;                       // [64] and (cos, sin) scaled by rt_af (before the fp16 rounding of the tile)
  Tree tree;                         // TR only (kernel arguments a variant does not read are never loaded)
  // WN only (c0 is then n0, the chunk's first TOKEN): the window, the ring's capacity, its resident columns
  // min(N, C), and the column -> token map n(c) = c + wn_base - (c > wn_r ? wn_cap : 0); all below 2^31
  int wn_window, wn_cap, wn_res, wn_r, wn_base;
};

// One kernel for the per-head (GR = TR = false), grouped (GR) and tree (GR and TR) geometries.  TR: tree mask and per-node
// positions from LDS copies of a.tree (the barriers in front of the first use order them).  WN: the window / ring variant
// of the per-head and grouped geometries.
template <int BITS, bool RT, bool GR, bool TR, bool WN = false>
__global__ __launch_bounds__(kThreads, 1) void chunk_attn_kernel(Args a) {
  static_assert(!TR || GR, "the tree variant runs in the grouped geometry");
  static_assert(!(TR && WN), "no draft trees on a ring");
  constexpr int N = 1 << BITS;
  constexpr int WPH = kD / 32 * BITS;
  __shared__ float klut[kD * N];
  __shared__ float theta[64];
  __shared__ float vrow[kKV * (N + 1)];
  __shared__ __attribute__((aligned(16))) float kst[kKV * kSR];
  __shared__ __attribute__((aligned(16))) float vst[kKV * kSR];
  __shared__ __attribute__((aligned(16))) unsigned char k16[kKV * kKRow];
  __shared__ __attribute__((aligned(16))) unsigned char vt16[kD * kVRow];
  __shared__ uint32_t tanc[kQB];                       // TR only (unused LDS is not allocated)
  __shared__ int tdepth[kQB];
  if constexpr (TR) {
    if (threadIdx.x < kQB) {
      tanc[threadIdx.x] = a.tree.anc[threadIdx.x];
      tdepth[threadIdx.x] = a.tree.depth[threadIdx.x];
    }
  }

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hi = lane >> 5, ql = lane & 31;
  const int split = (int)blockIdx.x % a.nsplit;
  const int rest = (int)blockIdx.x / a.nsplit;
  int h, qb, hk;
  if constexpr (GR) {                                  // rest = KV head; the wave's query head (waves >= G: rowless)
    const int w = __builtin_amdgcn_readfirstlane(wave);
    hk = rest;
    h = hk * a.G + (w < a.G ? w : a.G - 1);
    qb = 0;
  } else {
    h = rest % a.Hq;
    qb = a.nqb - 1 - rest / a.Hq;                      // late (long-row) query blocks first
    hk = h / a.G;
  }
  const bool has_rows = !GR || __builtin_amdgcn_readfirstlane(wave) < a.G;
  const int q0w = qb * kQW;
  const int q0 = GR ? 0 : q0w + wave * kQB;
  const int qrow = q0 + ql;
  const int qrc = qrow < a.S ? qrow : a.S - 1;
  const int64_t ml = a.max_len;
  const int64_t Lc = WN ? (int64_t)a.wn_res : a.c0 + a.S;   // compressed columns after the append (WN: resident ones)
  const int rows_end = (q0w + kQW < a.S) ? q0w + kQW : a.S;
  const int64_t kend = WN ? Lc : a.c0 + rows_end;      // columns [0, kend) matter to this workgroup
  const int n_tiles = (int)((kend + kKV - 1) / kKV);
  const int t_beg = split * a.tps;
  const int t_end = (t_beg + a.tps < n_tiles) ? t_beg + a.tps : n_tiles;
  const bool with_sinks = split == 0 && a.n_sink > 0;

  for (int e = tid; e < kD * N; e += kThreads) klut[e] = a.klut[(int64_t)hk * kD * N + e];
  if (tid < 64) theta[tid] = RT ? a.rt_freq[tid] : rope_freq(a.rope_theta, tid);

  f16x8 qf[8];
  load_q(a.q + (int64_t)h * a.qsh + (int64_t)qrc * a.qss, hi, qf);
  f32x16 oacc[4];
  float m_run, l_run;
  reset(oacc, m_run, l_run);

  // ---- S^T, mask, online softmax, O^T of one staged tile.  sink: key j of the tile is sink token j (no causal mask);
  // else key j is compressed column t0 + j, visible to row q iff t0 + j <= c0 + q (and < Lc); TR: iff t0 + j < c0 or
  // node t0 + j - c0 is in the row's ancestor set (which has no bit at or above S); WN: iff the column's token n(c) is
  // in (c0 + q - W, c0 + q]
  auto attend_tile = [&](bool sink, int64_t t0) __attribute__((always_inline)) {
    if (!(has_rows && q0 < a.S && (sink || WN || t0 <= a.c0 + q0 + kQB - 1))) return;
    bool diag = sink ? a.n_sink < kKV
                : TR ? t0 + kKV > a.c0
                     : (t0 + kKV - 1 > a.c0 + q0 || t0 + kKV > Lc);
    if constexpr (WN) {
      if (!sink) {
        // the tile's tokens are contiguous unless it holds the ring's newest column wn_r: then the wave skips a tile
        // none of its rows sees and takes one all of them see in full without the mask, as the plain kernel does
        const int c_lo = (int)t0, c_hi = (int)t0 + kKV - 1;
        const int q_lo = (int)a.c0 + q0, q_hi = (int)a.c0 + (q0 + kQB - 1 < a.S ? q0 + kQB - 1 : a.S - 1);
        diag = true;
        if (c_hi <= a.wn_r || c_lo > a.wn_r) {
          const int off = c_lo > a.wn_r ? a.wn_base - a.wn_cap : a.wn_base;
          const int t_lo = c_lo + off, t_hi = c_hi + off;
          if (t_lo > q_hi || t_hi <= q_lo - a.wn_window) return;
          diag = !(t_hi <= q_lo && t_lo > q_hi - a.wn_window && c_hi < a.wn_res);
        }
      }
    }
    // TR: bit j of vism[kb] = key kb * 32 + 4 * hi + j of the tile is visible to this lane's row (rows >= S: no node)
    uint32_t vism[2] = {0u, 0u};
    if constexpr (TR) {
      if (diag && !sink) {
        const int rel = (int)(t0 - a.c0);              // node of the tile's first key; > -64 (diag), <= S - 1
        const uint64_t an = tanc[ql];
        const uint64_t m = rel >= 0 ? an >> rel : (an << -rel) | ((uint64_t(1) << -rel) - 1);
        vism[0] = (uint32_t)m >> (4 * hi);
        vism[1] = (uint32_t)(m >> 32) >> (4 * hi);
      }
    }
    tile_step(k16, vt16, qf, oacc, m_run, l_run, a.scale_log2e, diag, hi, ql,
              [&](int kb, int r) __attribute__((always_inline)) -> bool {
                const int j = kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                if (sink) return j < a.n_sink;
                if constexpr (TR) {
                  return (vism[kb] >> ((r & 3) + 8 * (r >> 2))) & 1u;
                } else if constexpr (WN) {
                  const int c = (int)t0 + j;
                  const int tok = c + (c > a.wn_r ? a.wn_base - a.wn_cap : a.wn_base);
                  const int qt = (int)a.c0 + qrc;      // (rows >= S are clamped duplicates that are never written)
                  return tok <= qt && tok > qt - a.wn_window && c < a.wn_res;
                } else {
                  return t0 + j <= a.c0 + qrow && t0 + j < Lc;
                }
              });
  };

  // ---- the sink tokens: one prefix tile, fp16 as stored (keys past n_sink are zero and masked)
  if (with_sinks) {
    for (int i = tid; i < kKV * kD; i += kThreads) {
      const int j = i & 63, d = i >> 6;
      f16 kv = (f16)0.f, vv = (f16)0.f;
      if (j < a.n_sink) {
        kv = a.k_sink[((int64_t)hk * kD + d) * a.n_sink + j];
        vv = a.v_sink[((int64_t)hk * a.n_sink + j) * kD + d];
      }
      *reinterpret_cast<f16 *>(k16 + j * kKRow + (((d >> 3) ^ (j & 15)) << 4) + (d & 7) * 2) = kv;
      *reinterpret_cast<f16 *>(vt16 + d * kVRow + j * 2) = vv;
    }
    __syncthreads();
    attend_tile(true, 0);
  }

  // ---- staging roles: column skey of the tile, waves 0-3 K channel group g, waves 4-7 V channel group g
  const int skey = tid & 63;
  const bool is_k = wave < 4;
  const int g = wave & 3;
  const int32_t *mat = is_k ? a.kmat : a.vmat;
  for (int t = t_beg; t < t_end; t++) {
    const int64_t t0 = (int64_t)t * kKV;
    const int64_t col = t0 + skey;
    const bool valid = col < Lc;
    const int64_t colc = valid ? col : Lc - 1;
    // P0: the tile's V codebook rows -> LDS; this thread's packed words -> registers
    for (int i = tid; i < kKV * N; i += kThreads) {
      const int kk = i / N, c = i % N;
      const int64_t cc = (t0 + kk < Lc) ? t0 + kk : Lc - 1;
      vrow[kk * (N + 1) + c] = a.vrows[cc * N + c];
    }
    uint32_t w[BITS];
#pragma unroll
    for (int i = 0; i < BITS; i++) w[i] = (uint32_t)mat[((int64_t)hk * WPH + g * BITS + i) * ml + colc];
    __syncthreads();
    // P1: codes -> fp32 stage (K: the head's per-channel codebook; V: the column's own row)
    {
      float *st = (is_k ? kst : vst) + skey * kSR + g * 32;
      const float *tab = is_k ? klut + g * 32 * N : vrow + skey * (N + 1);
      const int cstride = is_k ? N : 0;
      float x[32];
      static_for<0, 32>([&](auto I) __attribute__((always_inline)) {
        constexpr int i = decltype(I)::value;
        x[i] = tab[i * cstride + (int)code_of<BITS, i>(w)];
      });
#pragma unroll
      for (int i = 0; i < 8; i++)
        *reinterpret_cast<f32x4 *>(st + 4 * i) = f32x4{x[4 * i], x[4 * i + 1], x[4 * i + 2], x[4 * i + 3]};
    }
    __syncthreads();
    // P2: this KV head's outlier residuals (slots g, g + 4, ... of the column)
    if (valid) {
      const int base = hk * kD;
      if (is_k) {
        for (int s = g; s < a.n_out; s += 4) {
          const int ch = a.kidx_t[(int64_t)s * ml + col] - base;
          const float val = a.kout_t[(int64_t)s * ml + col];
          if ((unsigned)ch < (unsigned)kD && val != 0.f) atomicAdd(&kst[skey * kSR + ch], val);
        }
      } else {
        for (int s = g; s < a.n_out; s += 4) {
          const int ch = a.vidx[col * a.n_out + s] - base;
          const float val = a.vout[col * a.n_out + s];
          if ((unsigned)ch < (unsigned)kD && val != 0.f) atomicAdd(&vst[skey * kSR + ch], val);
        }
      }
    }
    __syncthreads();
    // P3: K: RoPE of pairs (j, j + 64), j = 16g .. 16g+15, at position pos_offset + column (TR: a column of the chunk
    //     at pos_offset + c0 + its node's depth) -> fp16 K tile;  V: channels 32g .. 32g+31 -> fp16 V^T tile
    if (is_k) {
      int pos = (int)colc;
      if constexpr (TR) {
        const int node = (int)(colc - a.c0);           // <= S - 1 (colc < Lc)
        if (node >= 0) pos = (int)a.c0 + tdepth[node];
      }
      if constexpr (WN) pos += pos > a.wn_r ? a.wn_base - a.wn_cap : a.wn_base;      // the token the column holds
      const float posf = (float)(pos + a.pos_offset);
      const float *kr = kst + skey * kSR;
      float lo[16], hv[16];
#pragma unroll
      for (int i = 0; i < 16; i++) {
        const int j = 16 * g + i;
        float sn, cs;
        sincos_rev(theta[j] * posf, sn, cs);
        if constexpr (RT) {
          sn *= a.rt_af;
          cs *= a.rt_af;
        }
        const float klo = kr[j], khi = kr[j + 64];
        lo[i] = fmaf(cs, klo, -(sn * khi));
        hv[i] = fmaf(sn, klo, cs * khi);
      }
#pragma unroll
      for (int c = 0; c < 2; c++) {
        const u32x4 wl = {pack_f16(lo[8 * c], lo[8 * c + 1]), pack_f16(lo[8 * c + 2], lo[8 * c + 3]),
                          pack_f16(lo[8 * c + 4], lo[8 * c + 5]), pack_f16(lo[8 * c + 6], lo[8 * c + 7])};
        const u32x4 wh = {pack_f16(hv[8 * c], hv[8 * c + 1]), pack_f16(hv[8 * c + 2], hv[8 * c + 3]),
                          pack_f16(hv[8 * c + 4], hv[8 * c + 5]), pack_f16(hv[8 * c + 6], hv[8 * c + 7])};
        const int clo = 2 * g + c, chi = 8 + 2 * g + c;
        *reinterpret_cast<u32x4 *>(k16 + skey * kKRow + ((clo ^ (skey & 15)) << 4)) = wl;
        *reinterpret_cast<u32x4 *>(k16 + skey * kKRow + ((chi ^ (skey & 15)) << 4)) = wh;
      }
    } else {
      const float *vr = vst + skey * kSR + g * 32;
#pragma unroll
      for (int i = 0; i < 32; i++)
        *reinterpret_cast<f16 *>(vt16 + (g * 32 + i) * kVRow + skey * 2) = (f16)vr[i];
    }
    __syncthreads();
    attend_tile(false, t0);
  }

  // ---- partials of this split: unnormalised O^T rows, (max in raw score units, sum)
  if (has_rows && qrow < a.S) {
    const int64_t prow = ((int64_t)h * a.nsplit + split) * a.S + qrow;
    float *op = a.part_o + prow * kD;
#pragma unroll
    for (int db = 0; db < 4; db++)
#pragma unroll
      for (int gg = 0; gg < 4; gg++) {
        const int d = db * 32 + 8 * gg + 4 * hi;
        *reinterpret_cast<f32x4 *>(op + d) =
            f32x4{oacc[db][4 * gg], oacc[db][4 * gg + 1], oacc[db][4 * gg + 2], oacc[db][4 * gg + 3]};
      }
    if (hi == 0) {
      a.part_ml[prow * 2] = m_run;
      a.part_ml[prow * 2 + 1] = l_run;
    }
  }
}

// out[s][h][:] = sum_split w * O_split / sum_split w * l_split, w = 2^((m_split - M) * c), splits in index order
__global__ __launch_bounds__(kD) void chunk_attn_merge_kernel(const float *__restrict__ part_o,
                                                              const float *__restrict__ part_ml, float *__restrict__ out,
                                                              int Hq, int S, int nsplit, float scale_log2e) {
  const int row = blockIdx.x;              // s * Hq + h
  const int s = row / Hq, h = row % Hq, d = threadIdx.x;
  const int64_t base = (int64_t)h * nsplit * S + s;
  float M = -INFINITY;
  for (int i = 0; i < nsplit; i++) M = fmaxf(M, part_ml[(base + (int64_t)i * S) * 2]);
  float l = 0.f, o = 0.f;
  for (int i = 0; i < nsplit; i++) {
    const int64_t pr = base + (int64_t)i * S;
    const float m = part_ml[pr * 2];
    if (m == -INFINITY) continue;
    const float w = __builtin_amdgcn_exp2f((m - M) * scale_log2e);
    l = fmaf(w, part_ml[pr * 2 + 1], l);
    o = fmaf(w, part_o[pr * kD + d], o);
  }
  out[(int64_t)row * kD + d] = l > 0.f ? o / l : 0.f;
}

struct Plan {
  int nqb, nsplit, tps;
  size_t o_bytes, ml_bytes;
};

static size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

// grouped: the plan of the grouped kernel (G >= 2, S <= 32): Hkv workgroup rows in place of Hq x nqb
// tree (with grouped): the tree variant also takes G = 1, and a tree has at least one draft node (S >= 2)
// cols >= 0 (the window variant): the tiles are counted over cols resident columns instead of c0 + S
static bool plan(int Hq, int Hkv, int S, int64_t c0, Plan &p, bool grouped = false, bool tree = false,
                 int64_t cols = -1) {
  if (Hq <= 0 || Hkv <= 0 || Hq % Hkv || Hq / Hkv > 8 || (int64_t)Hkv * kD > 8192 || S <= 0 || S > kMaxS || c0 < 0 ||
      c0 + S >= (int64_t(1) << 31))
    return false;
  if (grouped && ((Hq / Hkv < 2 && !tree) || S > kQB)) return false;
  if (tree && S < 2) return false;
  p.nqb = (S + kQW - 1) / kQW;
  const int64_t tiles = ((cols >= 0 ? cols : c0 + S) + kKV - 1) / kKV;
  const int64_t base = grouped ? (int64_t)Hkv : (int64_t)Hq * p.nqb;
  int64_t ns = (kTargetWorkgroups + base - 1) / base;
  const int64_t cap = tiles / kMinTilesPerSplit > 1 ? tiles / kMinTilesPerSplit : 1;
  if (ns > cap) ns = cap;
  if (ns > kMaxSplits) ns = kMaxSplits;
  if (ns < 1) ns = 1;
  auto bytes = [&](int64_t n) { return align256((size_t)Hq * n * S * kD * 4) + align256((size_t)Hq * n * S * 8); };
  while (ns > 1 && bytes(ns) > kMaxWorkspace) ns--;
  p.tps = (int)((tiles + ns - 1) / ns);
  p.nsplit = (int)((tiles + p.tps - 1) / p.tps);
  p.o_bytes = align256((size_t)Hq * p.nsplit * S * kD * 4);
  p.ml_bytes = align256((size_t)Hq * p.nsplit * S * 8);
  return true;
}

// the window variant's plan over a ring of max_len columns (kvq.h: kvq_chunk_attention_window): false for what the plain
// plan refuses and for window < 1, window + S - 1 > max_len, max_len % 64 != 0
static bool plan_window(int Hq, int Hkv, int S, int64_t n0, int64_t window, int64_t max_len, Plan &p, bool grouped) {
  if (window < 1 || max_len <= 0 || max_len % kKV || max_len >= (int64_t(1) << 31) || S <= 0 || n0 < 0 ||
      window + S - 1 > max_len)
    return false;
  const int64_t N = n0 + S;
  return plan(Hq, Hkv, S, n0, p, grouped, false, N < max_len ? N : max_len);
}

}  // namespace chunk
}  // namespace kvq

using namespace kvq;

// depth and ancestor sets of a tree of S rows from its parent array (HOST memory; parent[0] is ignored): false unless
// 2 <= S <= 32 and parent[i] < i for every draft node
static bool tree_of(const uint8_t *parent, int S, chunk::Tree &t) {
  if (!parent || S < 2 || S > chunk::kQB) return false;
  for (int i = 0; i < chunk::kQB; i++) {
    t.anc[i] = 0;
    t.depth[i] = 0;
  }
  t.anc[0] = 1u;
  for (int i = 1; i < S; i++) {
    const int p = parent[i];
    if (p >= i) return false;
    t.depth[i] = (uint8_t)(t.depth[p] + 1);
    t.anc[i] = t.anc[p] | (1u << i);
  }
  return true;
}

// grouped: the grouped kernel (one workgroup per KV head and split), which plan() takes for G >= 2 and S <= 32 only
// parent (with grouped; HOST array of S entries): the tree variant, G >= 1 and 2 <= S <= 32
// window >= 1 (no parent): the window / ring variant, c0 is then n0 (0: the plain kernels)
static int chunk_attention_launch(const kvq_layer *ly, int Hq, int S, int64_t c0, const void *q, int64_t q_stride_h,
                                  int64_t q_stride_s, const uint16_t *k_sink, const uint16_t *v_sink, int n_sink,
                                  float *out, void *workspace, size_t workspace_bytes, const kvq_rope *rope, void *stream,
                                  bool grouped, const uint8_t *parent = nullptr, int64_t window = 0) {
  if (!ly || !q || !out || !rope_ok(rope)) return KVQ_EINVAL;
  const bool ring = window != 0;
  if (ring && parent) return KVQ_EINVAL;
  chunk::Args a = {};
  if (parent && !(grouped && tree_of(parent, S, a.tree))) return KVQ_EINVAL;
  const int bits = ly->bits;
  if ((bits != 2 && bits != 3 && bits != 4) || ly->hd != chunk::kD || ly->thr_k <= 0) return KVQ_EINVAL;
  chunk::Plan p;
  if (ring ? !chunk::plan_window(Hq, ly->H, S, c0, window, ly->max_len, p, grouped)
           : !chunk::plan(Hq, ly->H, S, c0, p, grouped, parent != nullptr))
    return KVQ_EINVAL;
  if (ly->max_len <= 0 || ly->max_len >= (int64_t(1) << 31) || (!ring && c0 + S > ly->max_len) || ly->pos_offset < 0 ||
      c0 + S + ly->pos_offset >= (int64_t(1) << 31))
    return KVQ_EINVAL;
  const float *klut = ly->klut_score ? ly->klut_score : ly->klut;
  const float *vrows = ly->v_mix_rows ? ly->v_mix_rows : ly->vlut_rows;
  if (!ly->kmat || !ly->vmat || !klut || !vrows || !ly->koutliers_t || !ly->kidx_t || !ly->voutliers || !ly->vidx)
    return KVQ_EINVAL;
  if (n_sink < 0 || n_sink > chunk::kMaxSink || (n_sink > 0 && (!k_sink || !v_sink))) return KVQ_EINVAL;
  // q rows are read as 16-byte vectors, partials / output as 16-byte vectors
  if ((q_stride_h | q_stride_s) % 8 || q_stride_h < 0 || q_stride_s < 0 || reinterpret_cast<uintptr_t>(q) % 16 ||
      reinterpret_cast<uintptr_t>(out) % 16 || (k_sink && reinterpret_cast<uintptr_t>(k_sink) % 2) ||
      (v_sink && reinterpret_cast<uintptr_t>(v_sink) % 2))
    return KVQ_EINVAL;
  if (!workspace || reinterpret_cast<uintptr_t>(workspace) % 256 || workspace_bytes < p.o_bytes + p.ml_bytes)
    return KVQ_EWORKSPACE;
  a.kmat = ly->kmat;
  a.vmat = ly->vmat;
  a.klut = klut;
  a.kout_t = ly->koutliers_t;
  a.kidx_t = ly->kidx_t;
  a.vrows = vrows;
  a.vout = ly->voutliers;
  a.vidx = ly->vidx;
  a.q = reinterpret_cast<const chunk::f16 *>(q);
  a.qsh = q_stride_h;
  a.qss = q_stride_s;
  a.k_sink = reinterpret_cast<const chunk::f16 *>(k_sink);
  a.v_sink = reinterpret_cast<const chunk::f16 *>(v_sink);
  a.part_o = reinterpret_cast<float *>(workspace);
  a.part_ml = reinterpret_cast<float *>(reinterpret_cast<char *>(workspace) + p.o_bytes);
  a.max_len = ly->max_len;
  a.c0 = c0;
  a.Hq = Hq;
  a.G = Hq / ly->H;
  a.S = S;
  a.n_sink = n_sink;
  a.n_out = 2 * ly->thr_k;
  a.pos_offset = ly->pos_offset;
  a.nqb = p.nqb;
  a.nsplit = p.nsplit;
  a.tps = p.tps;
  a.rope_theta = ly->rope_theta;
  a.scale_log2e = (1.0f / sqrtf((float)chunk::kD)) * 1.4426950408889634f;
  a.rt_freq = rope ? rope->inv_freq : nullptr;
  a.rt_af = rope ? rope->attention_factor : 1.f;
  if (ring) {
    const int64_t C = ly->max_len, N = c0 + S;
    a.wn_window = (int)window;                         // (<= max_len < 2^31: plan_window)
    a.wn_cap = (int)C;
    a.wn_res = (int)(N < C ? N : C);
    a.wn_r = (int)((N - 1) % C);
    a.wn_base = (int)((N - 1) / C * C);
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((int64_t)(grouped ? ly->H : Hq * p.nqb) * p.nsplit)), block(chunk::kThreads);
  with_bits(bits, [&](auto B) {
    with_int<0, 1, 2, 3, 4>(ring ? (grouped ? 4 : 3) : parent ? 2 : grouped ? 1 : 0, [&](auto V) {
      with_bool(rope != nullptr, [&](auto RT) {
        constexpr int v = decltype(V)::value;          // per-head, grouped, tree, window per-head, window grouped
        chunk::chunk_attn_kernel<decltype(B)::value, decltype(RT)::value, v == 1 || v == 2 || v == 4, v == 2, v >= 3>
            <<<grid, block, 0, st>>>(a);
      });
    });
  });
  int rc = check_launch();
  if (rc) return rc;
  chunk::chunk_attn_merge_kernel<<<(unsigned)((int64_t)S * Hq), chunk::kD, 0, st>>>(a.part_o, a.part_ml, out, Hq, S,
                                                                                     p.nsplit, a.scale_log2e);
  return check_launch();
}

extern "C" {

size_t kvq_chunk_attention_workspace_bytes(int Hq, int Hkv, int S, int64_t c0) {
  chunk::Plan p;
  if (!chunk::plan(Hq, Hkv, S, c0, p)) return 0;
  return p.o_bytes + p.ml_bytes;
}

int kvq_chunk_attention(const kvq_layer *ly, int Hq, int S, int64_t c0, const void *q, int64_t q_stride_h,
                        int64_t q_stride_s, const uint16_t *k_sink, const uint16_t *v_sink, int n_sink, float *out,
                        void *workspace, size_t workspace_bytes, void *stream) {
  return kvq_chunk_attention_rope(ly, Hq, S, c0, q, q_stride_h, q_stride_s, k_sink, v_sink, n_sink, out, workspace,
                                  workspace_bytes, nullptr, stream);
}

int kvq_chunk_attention_rope(const kvq_layer *ly, int Hq, int S, int64_t c0, const void *q, int64_t q_stride_h,
                             int64_t q_stride_s, const uint16_t *k_sink, const uint16_t *v_sink, int n_sink, float *out,
                             void *workspace, size_t workspace_bytes, const kvq_rope *rope, void *stream) {
  return chunk_attention_launch(ly, Hq, S, c0, q, q_stride_h, q_stride_s, k_sink, v_sink, n_sink, out, workspace,
                                workspace_bytes, rope, stream, false);
}

size_t kvq_chunk_attention_grouped_workspace_bytes(int Hq, int Hkv, int S, int64_t c0) {
  chunk::Plan p;
  if (!chunk::plan(Hq, Hkv, S, c0, p, true)) return 0;
  return p.o_bytes + p.ml_bytes;
}

int kvq_chunk_attention_grouped(const kvq_layer *ly, int Hq, int S, int64_t c0, const void *q, int64_t q_stride_h,
                                int64_t q_stride_s, const uint16_t *k_sink, const uint16_t *v_sink, int n_sink, float *out,
                                void *workspace, size_t workspace_bytes, void *stream) {
  return chunk_attention_launch(ly, Hq, S, c0, q, q_stride_h, q_stride_s, k_sink, v_sink, n_sink, out, workspace,
                                workspace_bytes, nullptr, stream, true);
}

int kvq_chunk_attention_grouped_rope(const kvq_layer *ly, int Hq, int S, int64_t c0, const void *q, int64_t q_stride_h,
                                     int64_t q_stride_s, const uint16_t *k_sink, const uint16_t *v_sink, int n_sink,
                                     float *out, void *workspace, size_t workspace_bytes, const kvq_rope *rope,
                                     void *stream) {
  return chunk_attention_launch(ly, Hq, S, c0, q, q_stride_h, q_stride_s, k_sink, v_sink, n_sink, out, workspace,
                                workspace_bytes, rope, stream, true);
}

size_t kvq_chunk_attention_tree_workspace_bytes(int Hq, int Hkv, int S, int64_t c0) {
  chunk::Plan p;
  if (!chunk::plan(Hq, Hkv, S, c0, p, true, true)) return 0;
  return p.o_bytes + p.ml_bytes;
}

int kvq_chunk_attention_tree(const kvq_layer *ly, int Hq, int S, int64_t c0, const void *q, int64_t q_stride_h,
                             int64_t q_stride_s, const uint16_t *k_sink, const uint16_t *v_sink, int n_sink, float *out,
                             void *workspace, size_t workspace_bytes, const uint8_t *parent, void *stream) {
  if (!parent) return KVQ_EINVAL;
  return chunk_attention_launch(ly, Hq, S, c0, q, q_stride_h, q_stride_s, k_sink, v_sink, n_sink, out, workspace,
                                workspace_bytes, nullptr, stream, true, parent);
}

int kvq_chunk_attention_tree_rope(const kvq_layer *ly, int Hq, int S, int64_t c0, const void *q, int64_t q_stride_h,
                                  int64_t q_stride_s, const uint16_t *k_sink, const uint16_t *v_sink, int n_sink,
                                  float *out, void *workspace, size_t workspace_bytes, const uint8_t *parent,
                                  const kvq_rope *rope, void *stream) {
  if (!parent) return KVQ_EINVAL;
  return chunk_attention_launch(ly, Hq, S, c0, q, q_stride_h, q_stride_s, k_sink, v_sink, n_sink, out, workspace,
                                workspace_bytes, rope, stream, true, parent);
}

size_t kvq_chunk_attention_window_workspace_bytes(int Hq, int Hkv, int S, int64_t n0, int64_t window, int64_t max_len) {
  chunk::Plan p;
  if (!chunk::plan_window(Hq, Hkv, S, n0, window, max_len, p, false)) return 0;
  return p.o_bytes + p.ml_bytes;
}

int kvq_chunk_attention_window(const kvq_layer *ly, int Hq, int S, int64_t n0, int64_t window, const void *q,
                               int64_t q_stride_h, int64_t q_stride_s, const uint16_t *k_sink, const uint16_t *v_sink,
                               int n_sink, float *out, void *workspace, size_t workspace_bytes, const kvq_rope *rope,
                               void *stream) {
  if (window < 1) return KVQ_EINVAL;
  return chunk_attention_launch(ly, Hq, S, n0, q, q_stride_h, q_stride_s, k_sink, v_sink, n_sink, out, workspace,
                                workspace_bytes, rope, stream, false, nullptr, window);
}

size_t kvq_chunk_attention_window_grouped_workspace_bytes(int Hq, int Hkv, int S, int64_t n0, int64_t window,
                                                          int64_t max_len) {
  chunk::Plan p;
  if (!chunk::plan_window(Hq, Hkv, S, n0, window, max_len, p, true)) return 0;
  return p.o_bytes + p.ml_bytes;
}

int kvq_chunk_attention_window_grouped(const kvq_layer *ly, int Hq, int S, int64_t n0, int64_t window, const void *q,
                                       int64_t q_stride_h, int64_t q_stride_s, const uint16_t *k_sink,
                                       const uint16_t *v_sink, int n_sink, float *out, void *workspace,
                                       size_t workspace_bytes, const kvq_rope *rope, void *stream) {
  if (window < 1) return KVQ_EINVAL;
  return chunk_attention_launch(ly, Hq, S, n0, q, q_stride_h, q_stride_s, k_sink, v_sink, n_sink, out, workspace,
                                workspace_bytes, rope, stream, true, nullptr, window);
}

}  // extern "C"

// ---- kvq_keep_columns: the accepted path of a tree round moves into contiguous columns ---------------------------------
// Every array in which a column owns storage holds 4-byte elements, either as rows along the columns (packed words, the
// K outlier mirror: element (r, c) at r * max_len + c) or as token-major rows (codebook rows, outlier rows: element
// (c, e) at c * width + e).  A thread owns ONE storage position (a word row r, or an entry slot e) across the chunk's S
// columns: it loads its n_keep sources c0 + keep[j] into registers, then stores them to c0 + j and zeros to the columns
// behind -- keep[j] >= j makes a destination another element's source, but only ever within one thread's position, and
// every load of a thread precedes its first store.  One launch for all arrays of the layer (a few hundred threads).
namespace kvq {
namespace keep {

constexpr int kMaxS = 32;
constexpr int kMaxJobs = 10;
constexpr int kThreads = 256;

struct Jobs {
  uint32_t *base[kMaxJobs];
  int64_t pos_stride[kMaxJobs];      // elements between two storage positions
  int64_t col_stride[kMaxJobs];      // elements between two columns
  int first[kMaxJobs + 1];           // job i owns threads [first[i], first[i + 1])
  int n_jobs, S, n_keep;
  int64_t c0;
  uint8_t keep[kMaxS];
};

__global__ __launch_bounds__(kThreads) void keep_columns_kernel(Jobs jb) {
  const int gid = (int)(blockIdx.x * kThreads + threadIdx.x);
  uint32_t *p = nullptr;
  int64_t cs = 0;
#pragma unroll
  for (int i = 0; i < kMaxJobs; i++)
    if (i < jb.n_jobs && gid >= jb.first[i] && gid < jb.first[i + 1]) {
      p = jb.base[i] + (int64_t)(gid - jb.first[i]) * jb.pos_stride[i] + jb.c0 * jb.col_stride[i];
      cs = jb.col_stride[i];
    }
  if (!p) return;
  uint32_t v[kMaxS];
#pragma unroll
  for (int j = 0; j < kMaxS; j++) v[j] = j < jb.n_keep ? p[(int64_t)jb.keep[j] * cs] : 0u;
#pragma unroll
  for (int j = 0; j < kMaxS; j++)
    if (j < jb.S) p[(int64_t)j * cs] = v[j];
}

}  // namespace keep
}  // namespace kvq

extern "C" {

int kvq_keep_columns(const kvq_layer *ly, int64_t c0, int S, const uint8_t *keep_idx, int n_keep, void *stream) {
  if (!ly || !keep_idx) return KVQ_EINVAL;
  const int bits = ly->bits;
  if ((bits != 2 && bits != 3 && bits != 4) || ly->H <= 0 || ly->hd <= 0 || ly->hd % 32 || ly->thr_k < 0)
    return KVQ_EINVAL;
  if (S < 1 || S > keep::kMaxS || n_keep < 1 || n_keep > S || c0 < 0 || ly->max_len <= 0 || c0 + S > ly->max_len)
    return KVQ_EINVAL;
  if (keep_idx[0] != 0) return KVQ_EINVAL;
  for (int j = 1; j < n_keep; j++)
    if (keep_idx[j] <= keep_idx[j - 1] || keep_idx[j] >= S) return KVQ_EINVAL;
  if (!ly->kmat && !ly->vmat) return KVQ_EINVAL;
  const int64_t ml = ly->max_len;
  const int64_t words = (int64_t)ly->H * (ly->hd / 32) * bits;
  const int n_out = 2 * ly->thr_k, N = 1 << bits;
  if (words > (1 << 20) || n_out > (1 << 20)) return KVQ_EINVAL;
  keep::Jobs jb;
  int n = 0, total = 0;
  auto add = [&](void *base, int positions, int64_t pos_stride, int64_t col_stride) {
    jb.base[n] = reinterpret_cast<uint32_t *>(base);
    jb.pos_stride[n] = pos_stride;
    jb.col_stride[n] = col_stride;
    jb.first[n] = total;
    total += positions;
    n++;
  };
  if (ly->kmat) {
    // the reference outlier format: rows and mirror, values and indices (a compact cache keeps no value arrays)
    if (n_out > 0 && (!ly->koutliers || !ly->kidx || !ly->koutliers_t || !ly->kidx_t)) return KVQ_EINVAL;
    add(ly->kmat, (int)words, ml, 1);
    if (n_out > 0) {
      add(ly->koutliers_t, n_out, ml, 1);
      add(ly->kidx_t, n_out, ml, 1);
      add(ly->koutliers, n_out, 1, n_out);
      add(ly->kidx, n_out, 1, n_out);
    }
  }
  if (ly->vmat) {
    if (!ly->vlut_rows || (n_out > 0 && (!ly->voutliers || !ly->vidx))) return KVQ_EINVAL;
    add(ly->vmat, (int)words, ml, 1);
    add(ly->vlut_rows, N, 1, N);
    if (ly->vnorm && ly->vnorm->lut_rows2) add(ly->vnorm->lut_rows2, N, 1, N);
    if (n_out > 0) {
      add(ly->voutliers, n_out, 1, n_out);
      add(ly->vidx, n_out, 1, n_out);
    }
  }
  for (int i = n; i < keep::kMaxJobs; i++) {
    jb.base[i] = nullptr;
    jb.pos_stride[i] = jb.col_stride[i] = 0;
  }
  for (int i = n; i <= keep::kMaxJobs; i++) jb.first[i] = total;
  jb.n_jobs = n;
  jb.S = S;
  jb.n_keep = n_keep;
  jb.c0 = c0;
  for (int j = 0; j < keep::kMaxS; j++) jb.keep[j] = j < n_keep ? keep_idx[j] : 0;
  const unsigned blocks = (unsigned)((total + keep::kThreads - 1) / keep::kThreads);
  keep::keep_columns_kernel<<<blocks, keep::kThreads, 0, (hipStream_t)stream>>>(jb);
  return check_launch();
}

}  // extern "C"
