// What the four fused correlation-build kernels share (corr_build_walk8.hip, corr_build_fused16.hip, corr_build_fused16g.hip,
// corr_build_fused16w.hip; the overview is at the top of corr_build_fused.hip): the LDS geometry of a strip's tile, the XCD mapping,
// an edge's buffer resources, the 8 x 8 block pooling (all four kernels), the whole-wave stores of irregular quads and the quad classification
// (fused16g, fused16w).  level1_regular_store and level23_store are the text fused16g and
// fused16w had in common; only fused16w calls them: on them fused16g<55>, at the 128-register ceiling of 1024 threads, spills, and the
// eight-wave kernels (wrap columns, classification over four pixels; on the shared stores 24 x 30 measured slower) and fused16
// (constant width) keep their own text there, as every kernel keeps its own
// writes of the pooled region (one shared function for them cost registers in four instantiations).  Callers differ by compile-time
// constants only; nothing here branches at run time on which kernel called it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"

namespace dba {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef float float16v __attribute__((ext_vector_type(16)));
typedef unsigned u2v __attribute__((ext_vector_type(2)));

struct FusedLevels {
  _Float16 *vs[4];
};

constexpr int FT_ROWS = 8;               // target rows per tile
constexpr unsigned OOR = 0x80000000u;    // a store offset beyond every buffer range: the store is dropped
constexpr size_t LDS_MAX_BYTES = 160 * 1024;

// LDS geometry of a strip (64 source pixels) with W2P tile columns, in halves
template <int W2P>
struct TileGeom {
  static constexpr int RP = W2P + 4;                 // tile row: the columns, then columns 0..3 once more (level-0 loops)
  static constexpr int PITCH = FT_ROWS * RP + 4;     // per source pixel
  static constexpr int RP1 = W2P / 2 + 4;            // level-1 row of the pooled region
  static constexpr int TILE = 64 * PITCH;
  static constexpr int P2_OFF = 64 * 4 * RP1;        // pooled region: P1 [64][4][RP1], P2 [64][2][W2P / 4], P3 [64][W2P / 8]
  static constexpr int P3_OFF = P2_OFF + 64 * 2 * (W2P / 4);
  static constexpr int POOLED = P3_OFF + 64 * (W2P / 8);
  static_assert(POOLED <= TILE, "the pooled region takes the dead tile's place in the one-strip kernels");
};
constexpr int OPERAND_HALVES = 64 * 128;   // a strip's source operand at C = 128 (the strip walks keep two)

// What a launch function is handed (corr_build_fused.hip fills it in; h1, w1: the source GRID where the planes are tiled)
struct BuildArgs {
  const _Float16 *A, *Bm;   // the operands the route reads: the caller's maps or their k-block-major copies
  FusedLevels L;
  int n, C, h1, w1, h2, w2, HW1p;
  float inv_w1;
  int spw;                  // strips per workgroup (strip walks)
  const int *oslots;
  int tiled;
};
int corr_build_walk8_launch(int route, const BuildArgs &a, hipStream_t s);   // the five eight-wave instantiations
int corr_build_fused16_launch(const BuildArgs &a, hipStream_t s);
int corr_build_fused16g_launch(int route, const BuildArgs &a, hipStream_t s);   // <55> or <0>
int corr_build_fused16w_launch(const BuildArgs &a, hipStream_t s);

__device__ __forceinline__ _Float16 pool4(_Float16 a, _Float16 b, _Float16 c, _Float16 d) {
  // ATen avg_pool2d on half: float accumulate, one rounding
  return (_Float16)(((float)a + (float)b + (float)c + (float)d) / 4.0f);
}

// workgroup barrier that orders LDS traffic only (global stores stay in flight)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Tiled planes: the row tiles ty0 and ty0 + 8 of one source tile write complementary pieces of the same lines, so all row tiles
// of a (strip group, edge) go to ONE XCD -- consecutive dispatch ids round-robin over the 8 XCDs, each XCD takes a contiguous
// eighth of the logical ids, row tile fastest -- and run side by side: the pieces meet in that XCD's L2 and leave it as whole
// lines.  (Without the mapping: measured, slower, see profiles/LOOKUP_NOTES.md.)
__device__ __forceinline__ void xcd_remap(int &bx, int &by, int &bz) {
  const int total = (int)(gridDim.x * gridDim.y * gridDim.z);
  const int lin = bx + (int)gridDim.x * (by + (int)gridDim.y * bz);
  const int q8 = total >> 3, r8 = total & 7, xk = lin & 7;
  const int logical = xk * q8 + min(xk, r8) + (lin >> 3);
  by = logical % (int)gridDim.y;
  const int rest = logical / (int)gridDim.y;
  bx = rest % (int)gridDim.x;
  bz = rest / (int)gridDim.x;
}

// plane index -> source pixel (common.h: linear or 4 x 16 tiles); indices past the map read the last pixel
struct SrcMap {
  int HW1, w1;
  float inv_w1;
  bool tiled;
  __device__ __forceinline__ void xy(int pix, int &x, int &y) const { sh_pixel_yx(min(pix, HW1 - 1), w1, inv_w1, tiled, y, x); }
};

// The planes of one edge.  Level l: [h2 >> l][w2 >> l][HW1p] halves, addressed through a buffer resource (an edge-level is
// < 2 GB); eo: the slot the edge is written into (the slot-addressed CorrBlock builds new edges straight into free slots)
struct EdgePlanes {
  const FusedLevels &L;
  int eo, h2, w2, HW1p;
  __device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc(int lvl) const {
    const size_t elems = (size_t)(h2 >> lvl) * (w2 >> lvl) * HW1p;
    return __builtin_amdgcn_make_buffer_rsrc((void *)(L.vs[lvl] + (size_t)eo * elems), 0, (int)(2 * elems), 0x00020000);
  }
  __device__ __forceinline__ unsigned plane_bytes() const { return 2u * (unsigned)HW1p; }
};

// Levels 0 and 1: a lane owns the QUAD of pixels p0 + q4 .. + 3 (q4 = 4 (lane & 15)) on one of four lines (g = lane >> 4) and
// stores 8 bytes.  A quad whose pixels do not share a source row (a strip that spans a row end, the last pixels of the map) is
// not regular: the whole wave stores it afterwards (irregular_store).  irregular: bit = quad index, wave-uniform.
struct Quads {
  int qx0, qy0;
  bool regular;
  unsigned long long irregular;
};
__device__ __forceinline__ Quads classify_quads(const SrcMap &map, int p0, int q4, int g) {
  Quads q;
  int qx3, qy3;
  map.xy(p0 + q4, q.qx0, q.qy0);
  map.xy(p0 + q4 + 3, qx3, qy3);
  q.regular = (p0 + q4 + 3 < map.HW1) && (q.qy0 == qy3);
  q.irregular = __ballot(!q.regular && g == 0 && (p0 + q4 < map.HW1));
  return q;
}

// Irregular quads of level LVL (0 or 1) of one target row: the quad's four pixels sit on four different lines, so the WHOLE wave
// takes them, lane = (pixel lane & 3 of the quad, offset lane >> 2), sixteen offsets per 2-byte store instruction.  (Left to the
// quad's own four lanes they cost 4 x w2 / 4 instructions issued by a wave with 4 of 64 lanes alive: strips with a row end took
// 2.5-3x as long.)  rows: the row's values of the strip's first pixel, PIX_PITCH halves per pixel; tyg: the row at this level;
// the wave takes the groups of sixteen offsets dx_begin, dx_begin + STRIDE, .. below dx_end.
template <int LVL, int PIX_PITCH, int STRIDE>
__device__ __forceinline__ void irregular_store(const EdgePlanes &pl, const SrcMap &map, unsigned long long mask,
                                                const _Float16 *rows, int tyg, int p0, int lane, int dx_begin, int dx_end) {
  const int w2l = pl.w2 >> LVL, h2l = pl.h2 >> LVL;
  const unsigned plane_bytes = pl.plane_bytes();
  const __amdgpu_buffer_rsrc_t rl = pl.rsrc(LVL);
  const int ipx = lane & 3, idx16 = lane >> 2;
  for (unsigned long long m = mask; m; m &= m - 1) {
    const int pix = 4 * (int)__builtin_ctzll(m) + ipx;  // this lane's pixel of the quad, within the strip
    int xi, yi;
    map.xy(p0 + pix, xi, yi);
    const bool pok = p0 + pix < map.HW1;
    int dy = tyg - (yi >> LVL);
    dy += (dy < 0) ? h2l : 0;
    const _Float16 *row = rows + pix * PIX_PITCH;
    const unsigned vbase = (unsigned)dy * (unsigned)w2l * plane_bytes + 2u * (unsigned)(p0 + pix);
    for (int dx0 = dx_begin; dx0 < dx_end; dx0 += STRIDE) {
      const int dx = dx0 + idx16;
      int tx = (xi >> LVL) + dx;
      tx -= (tx >= w2l) ? w2l : 0;
      tx = min(tx, w2l - 1);  // (dx beyond the map in the last group: read something valid, store nothing)
      const _Float16 v = row[tx];
      __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, v), rl,
                                            (pok && dx < w2l) ? vbase + (unsigned)dx * plane_bytes : OOR, 0, 0);
    }
  }
}

// One 8 x 8 block of one source pixel's rounded tile (tb: its first element, RP halves per row) -> its 4 x 4 level-1, 2 x 2
// level-2 and 1 level-3 values, each from the ROUNDED level below (== F.avg_pool2d on half, floor sizes), in registers
template <int RP>
__device__ __forceinline__ void pool_block(const _Float16 *tb, _Float16 (&q1)[4][4], _Float16 (&q2)[2][2], _Float16 &q3) {
  _Float16 t8[8][8];
#pragma unroll
  for (int r = 0; r < 8; r++) {
    const half4 lo = *reinterpret_cast<const half4 *>(tb + r * RP), hi = *reinterpret_cast<const half4 *>(tb + r * RP + 4);
#pragma unroll
    for (int c = 0; c < 4; c++) t8[r][c] = lo[c], t8[r][4 + c] = hi[c];
  }
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int c = 0; c < 4; c++) q1[r][c] = pool4(t8[2 * r][2 * c], t8[2 * r][2 * c + 1], t8[2 * r + 1][2 * c], t8[2 * r + 1][2 * c + 1]);
#pragma unroll
  for (int r = 0; r < 2; r++)
#pragma unroll
    for (int c = 0; c < 2; c++) q2[r][c] = pool4(q1[2 * r][2 * c], q1[2 * r][2 * c + 1], q1[2 * r + 1][2 * c], q1[2 * r + 1][2 * c + 1]);
  q3 = pool4(q2[0][0], q2[0][1], q2[1][0], q2[1][1]);
}

// Level 1, regular quads, pooled region WITHOUT wrap columns (the linear sixteen-wave kernels): 4 pooled rows x w2l offsets, four
// lines per store instruction; wave w takes pooled row tyl = w & 3 and the groups of four offsets grp + 4 k (grp = w >> 2).  The
// quad's columns (x >> 1) - (x0 >> 1) are 0, 0|1, 1, 1|2.  tyg: the pooled row in the map.
template <int RP1>
__device__ __forceinline__ void level1_regular_store(const EdgePlanes &pl, const Quads &q, const _Float16 *P1, int tyl, int tyg,
                                                     int grp, int g, int q4, int p0) {
  const int w2l = pl.w2 >> 1, h2l = pl.h2 >> 1;
  const unsigned plane_bytes = pl.plane_bytes();
  const __amdgpu_buffer_rsrc_t rl = pl.rsrc(1);
  const int xh = q.qx0 >> 1;
  const int o1 = ((q.qx0 + 1) >> 1) - xh, o2 = ((q.qx0 + 2) >> 1) - xh, o3 = ((q.qx0 + 3) >> 1) - xh;
  int t = xh + 4 * grp + g;
  t -= (t >= w2l) ? w2l : 0;
  t -= (t >= w2l) ? w2l : 0;
  int dy = tyg - (q.qy0 >> 1);
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

// Levels 2 and 3 of a strip from the pooled region: a lane is one source pixel (x1, y1) = plane index p, the (ty_l, dx) segments
// are dealt to the workgroup's NWAVES waves.  Pl: [64][rows][pitch_cols]
template <int NWAVES, int LVL>
__device__ __forceinline__ void level23_store(const EdgePlanes &pl, const _Float16 *Pl, int rows, int pitch_cols, int wave, int lane,
                                              int ty0, int x1, int y1, int p, bool active) {
  const int h2l = pl.h2 >> LVL, w2l = pl.w2 >> LVL;
  const unsigned plane_bytes = pl.plane_bytes();
  const __amdgpu_buffer_rsrc_t rl = pl.rsrc(LVL);
  const int x1l = x1 >> LVL, y1l = y1 >> LVL;
  for (int seg = wave; seg < rows * w2l; seg += NWAVES) {  // (wave-uniform)
    const int tyl = seg / w2l, dx = seg - tyl * w2l;
    const int tyg = (ty0 >> LVL) + tyl;
    if (tyg >= h2l) continue;
    int dy = tyg - y1l;
    dy += (dy < 0) ? h2l : 0;
    int tx = x1l + dx;
    tx -= (tx >= w2l) ? w2l : 0;
    const _Float16 v = Pl[(lane * rows + tyl) * pitch_cols + tx];
    const unsigned voff = active ? ((unsigned)dy * (unsigned)w2l + (unsigned)dx) * plane_bytes + 2u * (unsigned)p : OOR;
    __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, v), rl, voff, 0, 0);
  }
}
template <int NWAVES, int W2P>
__device__ __forceinline__ void levels23_store(const EdgePlanes &pl, const SrcMap &map, const _Float16 *P, int wave, int lane, int ty0,
                                               int p0) {
  typedef TileGeom<W2P> G;
  const int p = p0 + lane;
  int x1, y1;
  map.xy(p, x1, y1);
  level23_store<NWAVES, 2>(pl, P + G::P2_OFF, 2, W2P / 4, wave, lane, ty0, x1, y1, p, p < map.HW1);
  level23_store<NWAVES, 3>(pl, P + G::P3_OFF, 1, W2P / 8, wave, lane, ty0, x1, y1, p, p < map.HW1);
}

}  // namespace dba
