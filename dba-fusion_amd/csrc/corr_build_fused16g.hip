// The sixteen-wave strip walk for the maps whose planes keep the LINEAR pixel order (round 6, last session): 32 < w2 <= 64,
// C = 128, any h2 -- 55 x 55 is what the reference's TUM-VI demo runs on (512 x 512 resized to 440 x 440,
// demo_vio_tumvi.py:55-60).  Same work split as corr_build_fused16_kernel (a target row shared by two waves, four waves per SIMD,
// tile + two operand buffers + pooled region in LDS), same arithmetic in the same order as the eight-wave walk
// (corr_build_fused_kernel<2, true>): bit-identical to it.  What differs from the tiled form: a strip is 64 consecutive pixels of
// the flattened map and may span a row end (quads that do are stored by the whole wave, sixteen offsets per instruction), the map
// width is not a power of two (wraps by compare-and-subtract; the tile's wrap columns sit behind column w2 - 1 and are the second
// wave's own products: its fragments for those columns are targets 0..3 of the row, so no write of the tile is masked; the pooled
// region has no wrap columns, the level-1 loop wraps its offsets itself), the last row tile may be partial, and the operands are
// the k-block-major copies (16-byte pieces of the caller's maps are not aligned at these widths).  The two waves of a row split the
// offsets dx of the level-0 lines (batches of four lines; the wave that also pools takes one batch less).
// W2C > 0: the map width as a compile-time constant (w1 == w2 == W2C: the wraps, the splits of the lines between the waves and the
// divisions by the width fold into constants and the store loops unroll); 0: any width at run time.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "corr_build_tile.h"

namespace dba {

template <int W2C>
__global__ __launch_bounds__(1024) void corr_build_fused16g_kernel(const _Float16 *__restrict__ A, const _Float16 *__restrict__ Bm,
                                                                   FusedLevels L, int h1, int w1_, int h2, int w2_, int HW1p,
                                                                   float inv_w1_, int strips_per_wg, const int *__restrict__ oslots) {
  constexpr int C = 128, W2P = 64, KSL = 8;
  const int w2 = W2C > 0 ? W2C : w2_, w1 = W2C > 0 ? W2C : w1_;
  const float inv_w1 = W2C > 0 ? 1.0f / (float)W2C : inv_w1_;
  typedef TileGeom<W2P> G;
  constexpr int RP = G::RP, PITCH = G::PITCH, RP1 = G::RP1;
  extern __shared__ __attribute__((aligned(16))) _Float16 smem[];
  _Float16 *T = smem;                          // [64][PITCH]   level 0 of the current strip, rounded
  _Float16 *Ab0 = smem + G::TILE;              // two source-operand buffers of 16 KB
  _Float16 *P1 = Ab0 + 2 * OPERAND_HALVES;     // the pooled levels of the current strip (TileGeom), no wrap columns
  _Float16 *P2 = P1 + G::P2_OFF, *P3 = P1 + G::P3_OFF;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r = wave & 7, hf = wave >> 3;      // this wave's target row of the tile, its half of the row's targets
  const int ty0 = blockIdx.y * FT_ROWS, e = blockIdx.z;
  const int HW1 = h1 * w1, HW2 = h2 * w2;
  const int l31 = lane & 31, kh = (lane >> 5) * 8;
  const int nstrips = HW1p >> 6;
  const int s_begin = blockIdx.x * strips_per_wg, s_end = min(nstrips, s_begin + strips_per_wg);
  if (s_begin >= s_end) return;   // (workgroup-uniform)
  const SrcMap map{HW1, w1, inv_w1, false};
  const EdgePlanes planes{L, oslots ? oslots[e] : e, h2, w2, HW1p};
  const unsigned plane_bytes = planes.plane_bytes();

  // ---- source operand of a strip: 1024 pieces of 16 bytes ([k-block][pixel][half of the 16 channels]), one per thread ----------
  half8 apre;
  const int a_kbk = tid >> 7, a_px = (tid & 127) >> 1, a_hf = tid & 1;
  auto request_a = [&](int strip) {
    apre = *reinterpret_cast<const half8 *>(A + (size_t)e * HW1 * C + ((size_t)a_kbk * HW1 + min(strip * 64 + a_px, HW1 - 1)) * 16 + a_hf * 8);
  };
  auto stage_a = [&](_Float16 *dst) {   // -> LDS, fragment layout [k-step][32-pixel block][q][k-half][pixel][4 halves]
    const int fa = ((((a_kbk * 2 + (a_px >> 5)) * 2 + 0) * 2 + a_hf) * 32 + (a_px & 31)) * 4;
    half4 lo, hi;
#pragma unroll
    for (int c = 0; c < 4; c++) lo[c] = apre[c], hi[c] = apre[4 + c];
    *reinterpret_cast<half4 *>(dst + fa) = lo;
    *reinterpret_cast<half4 *>(dst + fa + 2 * 32 * 4) = hi;
  };
  request_a(s_begin);
  // ---- this wave's target fragments, resident for the whole walk: 32 targets x 128 channels (rows past the map: a valid row,
  // never stored; targets past the row's end: the next row's, never stored) ----------------------------------------------------
  half8 bres[KSL];
  {
    const int ty = min(ty0 + r, h2 - 1);
    // The tile wants columns 0..3 of a row once more behind column w2 - 1 (the level-0 loop's diagonal reads).  Those columns lie
    // in the second wave's half (w2 > 32): its fragments for them are targets 0..3 of the row, so the products land there by
    // themselves -- same operands, same order of accumulation, the same bits as in columns 0..3 -- and the tile write needs no mask
    int txl = 32 * hf + l31;
    txl -= (txl >= w2 && txl < w2 + 4) ? w2 : 0;
    const _Float16 *bpt = Bm + (size_t)e * HW2 * C + (size_t)min(ty * w2 + txl, HW2 - 1) * 16 + kh;
#pragma unroll
    for (int ks = 0; ks < KSL; ks++) bres[ks] = *reinterpret_cast<const half8 *>(bpt + (size_t)ks * 16 * HW2);
#pragma unroll
    for (int ks = 0; ks < KSL; ks++) asm volatile("" : "+v"(bres[ks]));   // (pinned: not re-read per strip)
  }
  stage_a(Ab0);

  const int q4 = (lane & 15) * 4, g = lane >> 4;     // the lane's quad of pixels and its line of a batch of four
  // batches of four level-0 lines: [0, nb0) to the row's first wave, the rest to its partner -- one batch moved from the first wave,
  // which also pools (none or two moved: measured, slower, see profiles/r06_build_g16.txt)
  const int nb = (w2 + 3) >> 2, nb0 = ((nb + 1) >> 1) - 1;
  const int b_begin = hf ? nb0 : 0, b_end = hf ? nb : nb0;

  for (int strip = s_begin; strip < s_end; strip++) {
    const int p0 = strip * 64;
    _Float16 *Ab = Ab0 + ((strip - s_begin) & 1) * OPERAND_HALVES;
    if (strip + 1 < s_end) request_a(strip + 1);   // consumed behind the tile write, BEFORE this strip's stores are issued
    lds_barrier();

    // ---- products: acc[i] = 32 x 32 tile (targets 32 hf .., sources 32 i ..) of target row ty0 + r -----------------------------
    float16v acc[2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int k = 0; k < 16; k++) acc[i][k] = 0.f;
#pragma unroll
    for (int ks = 0; ks < KSL; ks++) {
      half8 a[2];
#pragma unroll
      for (int t = 0; t < 2; t++) {
        const _Float16 *fp = Ab + ((((ks * 2 + t) * 2 + 0) * 2 + (lane >> 5)) * 32 + l31) * 4;
        const half4 lo = *reinterpret_cast<const half4 *>(fp), hi = *reinterpret_cast<const half4 *>(fp + 2 * 32 * 4);
#pragma unroll
        for (int c = 0; c < 4; c++) a[t][c] = lo[c], a[t][4 + c] = hi[c];
      }
#pragma unroll
      for (int i = 0; i < 2; i++) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bres[ks], a[i], acc[i], 0, 0, 0);  // targets x sources
    }
    lds_barrier();  // every wave is done with the source operand and with the previous strip's tile
    // D layout: col = lane & 31 (source within the 32-block), row = (k & 3) + 8 (k >> 2) + 4 (lane >> 5) (target).  Columns
    // w2 .. w2 + 3 hold columns 0..3 once more (the second wave's products, see its fragments); the ones behind them are never read.
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int rq = 0; rq < 4; rq++) {
        half4 v;
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = (_Float16)acc[i][4 * rq + k];
        *reinterpret_cast<half4 *>(T + (i * 32 + l31) * PITCH + r * RP + 32 * hf + 8 * rq + 4 * (lane >> 5)) = v;
      }
    // (maps 61..63 wide: the wrap columns from 64 on are outside the second wave's half -- the first wave's own values go there)
    if (w2 + 3 >= W2P && hf == 0 && lane < 32) {
#pragma unroll
      for (int i = 0; i < 2; i++) {
        _Float16 *wr = T + (i * 32 + l31) * PITCH + r * RP + w2;
#pragma unroll
        for (int k = 0; k < 4; k++)
          if (w2 + k >= W2P) wr[k] = (_Float16)acc[i][k];
      }
    }
    lds_barrier();
    if (strip + 1 < s_end) stage_a(Ab0 + ((strip + 1 - s_begin) & 1) * OPERAND_HALVES);

    // ---- the lane's quad of pixels (levels 0, 1) and the strip's irregular quads -----------------------------------------------
    const Quads quad = classify_quads(map, p0, q4, g);
    // ---- level 0: Vs0[(ty - y1) mod h2][dx][pixel] = T[pixel][ty][(x1 + dx) mod w2], this wave's target row and half of the dx ----
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
          // (a line dx = 4 b + g is this lane's to store iff b < b_end and dx < w2: ONE compare against the lane's limit; the column
          // counter wraps as an unsigned minimum: t + 4 - w2 is huge while t + 4 < w2)
          const unsigned dx_lim = (unsigned)min(w2, 4 * b_end + g);
          unsigned dxu = (unsigned)(4 * b_begin + g), tu = (unsigned)t;
          for (int b0 = b_begin; b0 < b_end; b0 += 4) {  // four batches at a time: their 16 LDS reads are in flight together
            unsigned short a[4][4];
#pragma unroll
            for (int b = 0; b < 4; b++) {
              const _Float16 *pp = lb + tu;
#pragma unroll
              for (int u = 0; u < 4; u++) a[b][u] = __builtin_bit_cast(unsigned short, pp[u * (PITCH + 1)]);
              tu = min(tu + 4u, tu + 4u - (unsigned)w2);
            }
#pragma unroll
            for (int b = 0; b < 4; b++) {
              u2v d;
              d.x = (unsigned)a[b][0] | ((unsigned)a[b][1] << 16);
              d.y = (unsigned)a[b][2] | ((unsigned)a[b][3] << 16);
              __builtin_amdgcn_raw_buffer_store_b64(d, r0, (dxu < dx_lim) ? voff : OOR, 0, 0);
              voff += 4u * plane_bytes;
              dxu += 4u;
            }
          }
        }
        irregular_store<0, PITCH, 16>(planes, map, quad.irregular, T + r * RP, ty, p0, lane, 32 * hf, min(w2, 32 * hf + 32));
      }
    }
    // ---- levels 1..3: threads 0..511 pool one 8 x 8 block each (from the ROUNDED level below each time) into the pooled region
    if (tid < 512) {
      const int src = tid >> 3, cb = tid & 7;
      _Float16 q1[4][4], q2[2][2], q3;
      pool_block<RP>(T + src * PITCH + 8 * cb, q1, q2, q3);
      // (no wrap columns in the pooled region: with a run-time width they would be 2-byte writes at an odd offset and the row's
      // last block a masked write -- the level-1 loop wraps its three offset columns itself)
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
    // The level-1 loop of regular quads and the level-2/3 loop below are this kernel's own copies of level1_regular_store and
    // level23_store (corr_build_tile.h, which fused16w uses): on the shared functions the 55-wide instantiation, which sits on the
    // 128-register ceiling of 1024 threads, spills to scratch.
    {  // level 1: 4 rows x w2l offsets, four lines per store instruction; wave w takes pooled row w & 3 and the groups of four
       // offsets (w >> 2) + 4 k.  The quad's columns (x >> 1) - (x0 >> 1) are 0, 0|1, 1, 1|2
      const int w2l = w2 >> 1, h2l = h2 >> 1;
      const __amdgpu_buffer_rsrc_t rl = planes.rsrc(1);
      const int tyl = wave & 3, grp = wave >> 2, tyg = (ty0 >> 1) + tyl;
      if (tyg < h2l) {  // floor sizes of avg_pool2d: the last partial row of the level below is dropped
        if (quad.regular) {
          const int xh = quad.qx0 >> 1;
          const int o1 = ((quad.qx0 + 1) >> 1) - xh, o2 = ((quad.qx0 + 2) >> 1) - xh, o3 = ((quad.qx0 + 3) >> 1) - xh;
          int t = xh + 4 * grp + g;
          t -= (t >= w2l) ? w2l : 0;
          t -= (t >= w2l) ? w2l : 0;
          int dy = tyg - (quad.qy0 >> 1);
          dy += (dy < 0) ? h2l : 0;
          unsigned voff = ((unsigned)dy * (unsigned)w2l + (unsigned)(4 * grp + g)) * plane_bytes + 2u * (unsigned)(p0 + q4);
          const _Float16 *lb = P1 + (q4 * 4 + tyl) * RP1;
          for (int dx0 = 4 * grp; dx0 < w2l; dx0 += 16) {
            int c1 = t + o1, c2 = t + o2, c3 = t + o3;   // (t < w2l; the offsets are 0..2)
            c1 -= (c1 >= w2l) ? w2l : 0;
            c2 -= (c2 >= w2l) ? w2l : 0;
            c3 -= (c3 >= w2l) ? w2l : 0;
            const unsigned short a0 = __builtin_bit_cast(unsigned short, lb[t]), a1 = __builtin_bit_cast(unsigned short, lb[4 * RP1 + c1]);
            const unsigned short a2 = __builtin_bit_cast(unsigned short, lb[8 * RP1 + c2]), a3 = __builtin_bit_cast(unsigned short, lb[12 * RP1 + c3]);
            u2v d;
            d.x = (unsigned)a0 | ((unsigned)a1 << 16);
            d.y = (unsigned)a2 | ((unsigned)a3 << 16);
            __builtin_amdgcn_raw_buffer_store_b64(d, rl, (dx0 + g < w2l) ? voff : OOR, 0, 0);
            voff += 16u * plane_bytes;
            t += 16;
            t -= (t >= w2l) ? w2l : 0;
            t -= (t >= w2l) ? w2l : 0;
          }
        }
        irregular_store<1, 4 * RP1, 64>(planes, map, quad.irregular, P1 + tyl * RP1, tyg, p0, lane, 16 * grp, w2l);
      }
    }
    {  // levels 2 and 3: a lane is one source pixel, (ty_l, dx) segments are dealt to the waves
      const int p = p0 + lane;
      const bool active = p < HW1;
      int x1, y1;
      map.xy(p, x1, y1);
      auto store_level = [&](int lvl, const _Float16 *Pl, int rows, int pitch_cols) {
        const int h2l = h2 >> lvl, w2l = w2 >> lvl;
        const __amdgpu_buffer_rsrc_t rl = planes.rsrc(lvl);
        const int x1l = x1 >> lvl, y1l = y1 >> lvl;
        for (int seg = wave; seg < rows * w2l; seg += 16) {  // (wave-uniform)
          const int tyl = seg / w2l, dx = seg - tyl * w2l;
          const int tyg = (ty0 >> lvl) + tyl;
          if (tyg >= h2l) continue;
          int dy = tyg - y1l;
          dy += (dy < 0) ? h2l : 0;
          int tx = x1l + dx;
          tx -= (tx >= w2l) ? w2l : 0;
          const _Float16 v = Pl[(lane * rows + tyl) * pitch_cols + tx];
          const unsigned voff = active ? ((unsigned)dy * (unsigned)w2l + (unsigned)dx) * plane_bytes + 2u * (unsigned)p : OOR;
          __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, v), rl, voff, 0, 0);
        }
      };
      store_level(2, P1 + G::P2_OFF, 2, W2P / 4);
      store_level(3, P1 + G::P3_OFF, 1, W2P / 8);
    }
  }
}

// LDS: the tile, two operand buffers, the pooled region
constexpr size_t FUSED16G_LDS_BYTES = sizeof(_Float16) * (size_t)(TileGeom<64>::TILE + 2 * OPERAND_HALVES + TileGeom<64>::POOLED);
static_assert(FUSED16G_LDS_BYTES <= LDS_MAX_BYTES, "LDS of a CU");

template <int W2C>
static int fused16g_launch(const BuildArgs &a, hipStream_t s) {
  static DeviceOnce attr_once;
  if (attr_once.needed()) {
    DBA_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&corr_build_fused16g_kernel<W2C>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)FUSED16G_LDS_BYTES));
    attr_once.done();
  }
  const dim3 grid((a.HW1p / 64 + a.spw - 1) / a.spw, (a.h2 + FT_ROWS - 1) / FT_ROWS, a.n);
  hipLaunchKernelGGL(corr_build_fused16g_kernel<W2C>, grid, dim3(1024), FUSED16G_LDS_BYTES, s, a.A, a.Bm, a.L, a.h1, a.w1, a.h2, a.w2,
                     a.HW1p, a.inv_w1, a.spw, a.oslots);
  return DBA_OK;
}

int corr_build_fused16g_launch(int route, const BuildArgs &a, hipStream_t s) {
  // 55 x 55 (the reference's TUM-VI demo) has its own instantiation
  return route == DBA_CORR_ROUTE_FUSED16G_55 ? fused16g_launch<55>(a, s) : fused16g_launch<0>(a, s);
}

}  // namespace dba
