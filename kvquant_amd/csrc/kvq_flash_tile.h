// The flash-attention tile step of the matrix-core attention kernels (kvq_prefill_attn.hip, kvq_chunk_attn.hip): a wave
// owns 32 query rows (its Q fragments live in registers for the whole kernel) and folds one 64-key tile, staged in LDS
// as fp16, into its running softmax: fp16 operands on v_mfma_f32_32x32x16_f16, fp32 accumulation, no score matrix in
// memory.  Both products are computed TRANSPOSED so that a lane owns ONE query row end to end (column = lane & 31 of
// every accumulator):
//   S^T[key][q] = K[key][:] . Q[q][:]      A = K tile (LDS, 16-byte row chunks XOR-swizzled by the key: conflict
//                                          free ds_read_b128), B = Q (registers)
//   O^T[d][q]  += V^T[d][key] . P^T[key][q]  A = V^T tile (LDS, transposed while staging, row stride 136 B:
//                                          conflict free ds_read_b64), B = P packed to fp16 IN PLACE: the MFMA
//                                          summation index is just a label, so the keys are fed in the order the
//                                          S^T accumulator holds them (rows (r&3) + 8(r>>2) + 4(lane>>5)) and the
//                                          V^T fragment is read in the same order -- no cross-lane exchange.
// Row max / sum: in-lane over the lane's 32 scores of the tile + one exchange with lane ^ 32.
// What differs between the kernels is where the tiles come from and which keys a row may see (the functor of
// tile_step); the arithmetic and its order are the same statements for both.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kvq {
namespace flash {

typedef _Float16 f16;
typedef f16 f16x8 __attribute__((ext_vector_type(8)));
typedef f16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));   // (a native vector: HIP's uint4 class ends up on the stack)

constexpr int kD = 128;          // head_dim
constexpr int kQB = 32;          // query rows per wave
constexpr int kKV = 64;          // keys per tile
constexpr int kKRow = kD * 2;    // bytes of a K row in LDS
constexpr int kVRow = 136;       // bytes of a V^T row in LDS (64 keys x 2 B + 8 pad)

// two floats -> packed fp16, ROUND TO NEAREST (gfx950's v_cvt_pk_f16_f32; cvt_pkrtz truncates, which biases P -- and
// with it every output -- down by 2^-12 .. 2^-11 relative to the unrounded row sum it is normalised with)
__device__ __forceinline__ uint32_t pack_f16(float a, float b) {
  uint32_t r;
  asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// Q fragments (B operand of S^T) of the lane's query row `q` [128]: lane (q, hi) holds Q[q][ks*16 + hi*8 .. +7], ks = 0..7
__device__ __forceinline__ void load_q(const f16 *q, int hi, f16x8 (&qf)[8]) {
#pragma unroll
  for (int ks = 0; ks < 8; ks++) qf[ks] = *reinterpret_cast<const f16x8 *>(q + hi * 8 + ks * 16);
}

__device__ __forceinline__ void reset(f32x16 (&oacc)[4], float &m_run, float &l_run) {
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int r = 0; r < 16; r++) oacc[i][r] = 0.f;
  m_run = -INFINITY;
  l_run = 0.f;
}

// One staged tile (ks: K tile, vs: V^T tile) into (oacc, m_run, l_run) of the lane's row; hi = lane >> 5, ql = lane & 31.
// Accumulator reg r of block kb holds key kb*32 + (r&3) + 8(r>>2) + 4hi of the tile; under diag (a tile that some row of
// the wave sees only in part) that key counts iff vis(kb, r), else every key of the tile does and vis is not consulted.
template <class Vis>
__device__ __forceinline__ void tile_step(const unsigned char *ks, const unsigned char *vs, const f16x8 (&qf)[8],
                                          f32x16 (&oacc)[4], float &m_run, float &l_run, float scale_log2e, bool diag,
                                          int hi, int ql, Vis vis) {
  // ---- S^T = K . Q^T: two 32-key blocks
  f32x16 sacc[2];
#pragma unroll
  for (int kb = 0; kb < 2; kb++) {
#pragma unroll
    for (int r = 0; r < 16; r++) sacc[kb][r] = 0.f;
    const int key = kb * 32 + ql;                      // A operand row of this lane
#pragma unroll
    for (int kk = 0; kk < 8; kk++) {
      const int c = kk * 2 + hi;                       // 16-byte chunk: d = kk*16 + hi*8 .. +7
      const f16x8 kf = *reinterpret_cast<const f16x8 *>(ks + key * kKRow + ((c ^ (key & 15)) << 4));
      sacc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[kk], sacc[kb], 0, 0, 0);
    }
  }
  // ---- mask + scale + online softmax
  // (running max m_run is kept in RAW score units; the softmax scale (> 0) and log2(e) are folded into one FMA
  //  per exponential: p = 2^(s*c - m*c))
  float mx = -INFINITY;
#pragma unroll
  for (int kb = 0; kb < 2; kb++)
#pragma unroll
    for (int r = 0; r < 16; r++) {
      float s = sacc[kb][r];
      if (diag) {
        if (!vis(kb, r)) s = -INFINITY;
        sacc[kb][r] = s;
      }
      mx = fmaxf(mx, s);
    }
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  const float m_new = fmaxf(m_run, mx);
  const float m_use = m_new == -INFINITY ? 0.f : m_new;            // (a fully masked row so far)
  const float mc = -m_use * scale_log2e;
  float ps = 0.f;
  uint32_t pp[2][8];                                                // P^T packed: regs (2i, 2i+1)
#pragma unroll
  for (int kb = 0; kb < 2; kb++)
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
      const float p0 = __builtin_amdgcn_exp2f(fmaf(sacc[kb][r], scale_log2e, mc));
      const float p1 = __builtin_amdgcn_exp2f(fmaf(sacc[kb][r + 1], scale_log2e, mc));
      ps += p0 + p1;
      pp[kb][r >> 1] = pack_f16(p0, p1);
    }
  ps += __shfl_xor(ps, 32);
  // the running sums only need rescaling when some row's maximum moved (wave-uniform test: rare after the first
  // tiles on real data); 2^-inf = 0 on the first tile
  if (__any(m_new != m_run)) {
    const float alpha = __builtin_amdgcn_exp2f((m_run - m_use) * scale_log2e);
    l_run *= alpha;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int r = 0; r < 16; r++) oacc[i][r] *= alpha;
  }
  l_run += ps;
  m_run = m_new;
  // ---- O^T += V^T . P^T.  k index (hi*8 + i) of step (kb, ks2) stands for key kb*32 + ks2*16 + (i>>2)*8 + 4hi + (i&3)
#pragma unroll
  for (int kb = 0; kb < 2; kb++)
#pragma unroll
    for (int ks2 = 0; ks2 < 2; ks2++) {
      const u32x4 pw = {pp[kb][ks2 * 4], pp[kb][ks2 * 4 + 1], pp[kb][ks2 * 4 + 2], pp[kb][ks2 * 4 + 3]};
      const f16x8 pf = __builtin_bit_cast(f16x8, pw);
      const int kofs = (kb * 32 + ks2 * 16 + 4 * hi) * 2;          // byte offset of the first 4 keys in a V^T row
#pragma unroll
      for (int db = 0; db < 4; db++) {
        const unsigned char *row = vs + (db * 32 + ql) * kVRow + kofs;
        const f16x4 v0 = *reinterpret_cast<const f16x4 *>(row);
        const f16x4 v1 = *reinterpret_cast<const f16x4 *>(row + 16);
        const f16x8 vf = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
        oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, oacc[db], 0, 0, 0);
      }
    }
}

}  // namespace flash
}  // namespace kvq
