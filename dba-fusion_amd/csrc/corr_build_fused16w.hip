// Maps 65..128 wide in the linear pixel order on SIXTEEN waves (round 6, last session): 28 x 107 is the KITTI-360 shape of
// BASELINE's configs.  One strip per workgroup like corr_build_fused_kernel<4, false> -- a 128-column tile (136 KB) leaves no LDS for
// a walk's second operand buffer and no registers for resident target fragments -- but a target row is shared by two waves: wave
// (r, hf) owns the columns 64 hf .. 64 hf + 63 of row ty0 + r (2 x 2 accumulator tiles, 64 registers, instead of 2 x 4), so four
// waves per SIMD instead of two wait for the row's target fragments, which come out of L2 in every strip (32 KB per row: the
// matrix phase of the eight-wave form is mostly that wait).  Same arithmetic in the same order: bit-identical.  The conventions of
// corr_build_fused16g_kernel: the tile's wrap columns are the second wave's own products, no masked tile writes, no wrap columns
// in the pooled region (which takes the dead tile's place, as in the eight-wave form), level-0 lines split between a row's waves.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "corr_build_tile.h"

namespace dba {

__global__ __launch_bounds__(1024) void corr_build_fused16w_kernel(const _Float16 *__restrict__ A, const _Float16 *__restrict__ Bm,
                                                                   FusedLevels L, int C, int h1, int w1, int h2, int w2, int HW1p,
                                                                   float inv_w1, const int *__restrict__ oslots) {
  constexpr int W2P = 128;
  typedef TileGeom<W2P> G;
  constexpr int RP = G::RP, PITCH = G::PITCH, RP1 = G::RP1;
  extern __shared__ __attribute__((aligned(16))) _Float16 smem[];
  _Float16 *T = smem;                          // [64][PITCH]   level 0 of the strip, rounded; before that: the strip's source operand
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r = wave & 7, hf = wave >> 3;      // this wave's target row of the tile, its half of the row's columns
  const int strip = blockIdx.x, ty0 = blockIdx.y * FT_ROWS, e = blockIdx.z;
  const int HW1 = h1 * w1, HW2 = h2 * w2;
  const int l31 = lane & 31, kh = (lane >> 5) * 8;
  const int p0 = strip * 64;
  const SrcMap map{HW1, w1, inv_w1, false};
  const EdgePlanes planes{L, oslots ? oslots[e] : e, h2, w2, HW1p};
  const unsigned plane_bytes = planes.plane_bytes();
  const int ksteps = C >> 4;

  // ---- the strip's source operand into the (still unused) tile: [k-step][32-pixel block][q][k-half][pixel][4 halves] ----------
  {
    const _Float16 *Ae = A + (size_t)e * HW1 * C;
    for (int idx = tid; idx < ksteps * 128; idx += 1024) {  // 16-byte pieces: [k-block][pixel][half of the 16 channels]
      const int kbk = idx >> 7, rem = idx & 127, px = rem >> 1, hk = rem & 1;
      const half8 v = *reinterpret_cast<const half8 *>(Ae + ((size_t)kbk * HW1 + min(p0 + px, HW1 - 1)) * 16 + hk * 8);
      const int fa = ((((kbk * 2 + (px >> 5)) * 2 + 0) * 2 + hk) * 32 + (px & 31)) * 4;
      half4 lo, hi;
#pragma unroll
      for (int c = 0; c < 4; c++) lo[c] = v[c], hi[c] = v[4 + c];
      *reinterpret_cast<half4 *>(T + fa) = lo;
      *reinterpret_cast<half4 *>(T + fa + 2 * 32 * 4) = hi;
    }
  }
  // ---- this wave's target fragments: streamed per k-step, two steps ahead (rows past the map: a valid row, never stored; the
  // columns w2 .. w2 + 3: targets 0..3 of the row -- the tile's wrap columns; columns behind them: never read) -------------------
  const _Float16 *bp[2];
  {
    const int ty = min(ty0 + r, h2 - 1);
#pragma unroll
    for (int j = 0; j < 2; j++) {
      int txl = 64 * hf + 32 * j + l31;
      txl -= (txl >= w2 && txl < w2 + 4) ? w2 : 0;
      bp[j] = Bm + (size_t)e * HW2 * C + (size_t)min(ty * w2 + txl, HW2 - 1) * 16 + kh;
    }
  }
  const size_t kb = (size_t)HW2;
  half8 b0[2], b1[2], b2[2];
#pragma unroll
  for (int j = 0; j < 2; j++) {
    b0[j] = *reinterpret_cast<const half8 *>(bp[j]);
    b1[j] = *reinterpret_cast<const half8 *>(bp[j] + (size_t)min(1, ksteps - 1) * 16 * kb);
  }
  __syncthreads();

  // ---- products: acc[i][j] = 32 x 32 tile (sources 32 i .., targets 64 hf + 32 j ..) of target row ty0 + r ------------------------
  float16v acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int k = 0; k < 16; k++) acc[i][j][k] = 0.f;
  for (int ks = 0; ks < ksteps; ks++) {
    const int kn = min(ks + 2, ksteps - 1);  // (the last steps re-request a fragment: no branch in the loop)
#pragma unroll
    for (int j = 0; j < 2; j++) b2[j] = *reinterpret_cast<const half8 *>(bp[j] + (size_t)kn * 16 * kb);
    half8 a[2];
#pragma unroll
    for (int t = 0; t < 2; t++) {
      const _Float16 *fp = T + ((((ks * 2 + t) * 2 + 0) * 2 + (lane >> 5)) * 32 + l31) * 4;
      const half4 lo = *reinterpret_cast<const half4 *>(fp), hi = *reinterpret_cast<const half4 *>(fp + 2 * 32 * 4);
#pragma unroll
      for (int c = 0; c < 4; c++) a[t][c] = lo[c], a[t][4 + c] = hi[c];
    }
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 2; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(b0[j], a[i], acc[i][j], 0, 0, 0);  // targets x sources
#pragma unroll
    for (int j = 0; j < 2; j++) {
      b0[j] = b1[j];
      b1[j] = b2[j];
    }
  }
  lds_barrier();  // every wave is done with the source operand: the tile takes its place
  // D layout: col = lane & 31 (source within the 32-block), row = (k & 3) + 8 (k >> 2) + 4 (lane >> 5) (target)
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int rq = 0; rq < 4; rq++) {
        half4 v;
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = (_Float16)acc[i][j][4 * rq + k];
        *reinterpret_cast<half4 *>(T + (i * 32 + l31) * PITCH + r * RP + 64 * hf + 32 * j + 8 * rq + 4 * (lane >> 5)) = v;
      }
  // (maps 125..128 wide: the wrap columns from 128 on are outside the second wave's half -- the first wave's own values go there)
  if (w2 + 3 >= W2P && hf == 0 && lane < 32) {
#pragma unroll
    for (int i = 0; i < 2; i++) {
      _Float16 *wr = T + (i * 32 + l31) * PITCH + r * RP + w2;
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (w2 + k >= W2P) wr[k] = (_Float16)acc[i][0][k];
    }
  }
  lds_barrier();

  const int q4 = (lane & 15) * 4, g = lane >> 4;     // the lane's quad of pixels and its line of a batch of four
  const int nb = (w2 + 3) >> 2, nb0 = ((nb + 1) >> 1) - 1;   // batches of four level-0 lines: [0, nb0) to the row's first wave (it has the
  const int b_begin = hf ? nb0 : 0, b_end = hf ? nb : nb0;   // larger share of the pooling's reads in front of it), the rest to its partner
  const Quads quad = classify_quads(map, p0, q4, g);
  // ---- level 0: Vs0[(ty - y1) mod h2][dx][pixel] = T[pixel][ty][(x1 + dx) mod w2], this wave's target row and share of the dx ----
  {
    const int ty = ty0 + r;
    if (ty < h2) {  // (wave-uniform)
      const __amdgpu_buffer_rsrc_t r0 = planes.rsrc(0);
      if (quad.regular) {
        int t = quad.qx0 + g + 4 * b_begin;
        t -= (t >= w2) ? w2 : 0;
        t -= (t >= w2) ? w2 : 0;
        int dy = ty - quad.qy0;
        dy += (dy < 0) ? h2 : 0;
        unsigned voff = ((unsigned)dy * (unsigned)w2 + (unsigned)(g + 4 * b_begin)) * plane_bytes + 2u * (unsigned)(p0 + q4);
        const _Float16 *lb = T + q4 * PITCH + r * RP;
        for (int b0_ = b_begin; b0_ < b_end; b0_ += 4) {  // four batches at a time: their 16 LDS reads are in flight together
          unsigned short a[4][4];
#pragma unroll
          for (int b = 0; b < 4; b++) {
            const _Float16 *pp = lb + t;
#pragma unroll
            for (int u = 0; u < 4; u++) a[b][u] = __builtin_bit_cast(unsigned short, pp[u * (PITCH + 1)]);
            t += 4;
            t -= (t >= w2) ? w2 : 0;
          }
#pragma unroll
          for (int b = 0; b < 4; b++) {
              u2v d;
            d.x = (unsigned)a[b][0] | ((unsigned)a[b][1] << 16);
            d.y = (unsigned)a[b][2] | ((unsigned)a[b][3] << 16);
            __builtin_amdgcn_raw_buffer_store_b64(d, r0, (b0_ + b < b_end && 4 * (b0_ + b) + g < w2) ? voff : OOR, 0, 0);
            voff += 4u * plane_bytes;
          }
        }
      }
      irregular_store<0, PITCH, 16>(planes, map, quad.irregular, T + r * RP, ty, p0, lane, 64 * hf, min(w2, 64 * hf + 64));
    }
  }
  // ---- levels 1..3: every thread pools one 8 x 8 block (from the ROUNDED level below each time) in registers; behind a barrier (the
  // tile is dead: its level-0 stores have read it) the values take its place, behind a second one the sheared store loops read them
  _Float16 *P1 = T, *P2 = P1 + G::P2_OFF, *P3 = P1 + G::P3_OFF;   // the pooled region (TileGeom), no wrap columns
  {
    const int src = tid >> 4, cb = tid & 15;
    _Float16 q1[4][4], q2[2][2], q3;
    pool_block<RP>(T + src * PITCH + 8 * cb, q1, q2, q3);
    lds_barrier();  // every read of the level-0 tile is done (its sheared store above included)
#pragma unroll
    for (int rw = 0; rw < 4; rw++) {
      half4 v;
#pragma unroll
      for (int c = 0; c < 4; c++) v[c] = q1[rw][c];
      *reinterpret_cast<half4 *>(P1 + (src * 4 + rw) * RP1 + 4 * cb) = v;
    }
#pragma unroll
    for (int rw = 0; rw < 2; rw++) {
      half2v v;
      v.x = q2[rw][0], v.y = q2[rw][1];
      *reinterpret_cast<half2v *>(P2 + (src * 2 + rw) * (W2P / 4) + 2 * cb) = v;
    }
    P3[src * (W2P / 8) + cb] = q3;
  }
  lds_barrier();
  {  // level 1: wave w takes pooled row w & 3 (floor sizes of avg_pool2d: the last partial row of the level below is dropped)
    const int tyl = wave & 3, grp = wave >> 2, tyg = (ty0 >> 1) + tyl;
    if (tyg < (h2 >> 1)) {
      if (quad.regular) level1_regular_store<RP1>(planes, quad, P1, tyl, tyg, grp, g, q4, p0);
      // (the four waves of a pooled row take every fourth group of 16 offsets)
      irregular_store<1, 4 * RP1, 64>(planes, map, quad.irregular, P1 + tyl * RP1, tyg, p0, lane, 16 * grp, w2 >> 1);
    }
  }
  levels23_store<16, W2P>(planes, map, P1, wave, lane, ty0, p0);
}

// LDS: the tile; the source operand (at most 64 x 512 halves) before it and the pooled region after it live inside it
constexpr size_t FUSED16W_LDS_BYTES = sizeof(_Float16) * (size_t)TileGeom<128>::TILE;
static_assert(FUSED16W_LDS_BYTES <= LDS_MAX_BYTES && 64 * 512 <= TileGeom<128>::TILE, "LDS of a CU");

int corr_build_fused16w_launch(const BuildArgs &a, hipStream_t s) {
  static DeviceOnce attr_once;
  if (attr_once.needed()) {
    DBA_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&corr_build_fused16w_kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)FUSED16W_LDS_BYTES));
    attr_once.done();
  }
  const dim3 grid(a.HW1p / 64, (a.h2 + FT_ROWS - 1) / FT_ROWS, a.n);
  hipLaunchKernelGGL(corr_build_fused16w_kernel, grid, dim3(1024), FUSED16W_LDS_BYTES, s, a.A, a.Bm, a.L, a.C, a.h1, a.w1, a.h2, a.w2,
                     a.HW1p, a.inv_w1, a.oslots);
  return DBA_OK;
}

}  // namespace dba
