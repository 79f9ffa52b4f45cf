// The eight-wave kernels of the fused correlation build (overview: corr_build_fused.hip; shared phases: corr_build_tile.h): one
// template, five instantiations -- one strip per workgroup on 64 or 128 tile columns (<2, false>, <4, false>) and the strip walk on
// the k-block-major copies (<2, true>), on the caller's own maps (<2, true, true>) or on the target map only (<2, true, false, true>).
// A wave owns one whole target row of the tile.  corr_build_walk8_launch picks the instantiation by route.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "corr_build_tile.h"

namespace dba {

// LOOP (64-wide tiles, C = 128): the workgroup walks `strips_per_wg` consecutive strips of its target-row tile.  The
// wave's target fragments (16 KB: every k-step of its row) then live in 64 registers for the whole walk - no fragment
// load sits between the matrix products any more -, and the next strip's source operand is requested at the top of a
// strip and put into LDS (double-buffered) right after the strip's tile write, BEFORE the strip's stores are issued: a
// wave's loads and stores complete in order, so consumed after those stores the operand would wait for all of them to
// reach HBM; consumed before them it only waits for the previous strip's, which have had a whole multiplication to drain.
// The stores then drain while the next strip is multiplied.  One workgroup per CU (103 KB of LDS, up to 256 registers
// per lane).
// NATIVE / NATIVE_B (LOOP form only): A / Bm are the caller's feature maps as they lie, [n][C][h][w] -- no k-block-major copies
// are made first (a launch and 2 x the map's bytes of traffic less per map and build).  The source operand's 16 KB per strip
// are read as 16-byte pieces (8 consecutive pixels of one channel, which both pixel orders of the planes keep adjacent), 4
// channels per thread (threads 0..255), scaled (/ 4: corr.py:67-68) and transposed in registers into the LDS fragment layout's
// [pixel][4 channels] units; the wave's target fragments -- read once per walk -- go through 2 KB of LDS per wave
// ([pixel][16 channels], written by halves, read back as fragments).
template <int NT, bool LOOP, bool NATIVE = false, bool NATIVE_B = NATIVE>
__global__ __launch_bounds__(512, LOOP ? 2 : ((NT <= 2) ? 4 : 2)) void corr_build_fused_kernel(
    const _Float16 *__restrict__ A, const _Float16 *__restrict__ Bm, FusedLevels L, int C, int h1, int w1, int h2, int w2,
    int HW1p, float inv_w1, int strips_per_wg, const int *__restrict__ oslots, int tiled) {
  constexpr int W2P = 32 * NT;               // tile columns (targets beyond w2 are computed and never read)
  typedef TileGeom<W2P> G;
  constexpr int RP = G::RP, PITCH = G::PITCH;
  extern __shared__ __attribute__((aligned(16))) _Float16 smem[];
  _Float16 *T = smem;                              // [64][PITCH]  level 0, rounded; before that: the strip's A operand
  _Float16 *Ab0 = LOOP ? smem + G::TILE : smem;     // the strip's source operand (LOOP: two 16 KB buffers behind the tile)
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  // Workgroup -> (strip group, target-row tile, edge).  Tiled planes: the row tiles ty0 and ty0 + 8 of one source tile write
  // complementary pieces of the same lines (see the level-0 stores), so all row tiles of a (strip group, edge) go to ONE
  // XCD -- consecutive dispatch ids round-robin over the 8 XCDs, each XCD takes a contiguous eighth of the logical ids,
  // row tile fastest -- and run side by side: the pieces then meet in that XCD's L2 and leave it as whole lines.
  int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  if (tiled) xcd_remap(bx, by, bz);
  const int ty0 = by * FT_ROWS;                    // first target row of the tile
  const int e = bz;
  const int HW1 = h1 * w1, HW2 = h2 * w2;
  const int l31 = lane & 31, kh = (lane >> 5) * 8;
  const int nstrips = HW1p >> 6;
  const int s_begin = LOOP ? bx * strips_per_wg : bx;
  const int s_end = LOOP ? min(nstrips, s_begin + strips_per_wg) : s_begin + 1;
  constexpr int KSL = 8;                           // k-steps of the LOOP form (C = 128)
  half8 bres[LOOP ? KSL : 1][NT];                  // LOOP: the wave's target fragments, resident
  half8 apre[2];                                   // LOOP: this thread's two 16-byte pieces of the next source operand
  half8 anat[4];                                   // NATIVE: 8 pixels x 4 channels of the next source operand (threads 0..255)
  auto request_a = [&](int strip) {
    const _Float16 *Ae = A + (size_t)e * HW1 * C;
    if constexpr (NATIVE) {   // thread = (channel group of 4, pixel group of 8: half a tile row, or 8 pixels of the linear order)
      if (tid < 256) {
        const int kg = tid >> 3, pg = tid & 7;
        int yy, xx;
        sh_pixel_yx(min(strip * 64 + 8 * pg, HW1 - 8), w1, inv_w1, tiled != 0, yy, xx);
        const _Float16 *src = Ae + (size_t)(4 * kg) * HW1 + yy * w1 + xx;
#pragma unroll
        for (int c = 0; c < 4; c++) anat[c] = *reinterpret_cast<const half8 *>(src + (size_t)c * HW1);
      }
      return;
    }
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const int idx = tid + 512 * u, kbk = idx >> 7, r = idx & 127, px = r >> 1, hf = r & 1;
      apre[u] = *reinterpret_cast<const half8 *>(Ae + ((size_t)kbk * HW1 + min(strip * 64 + px, HW1 - 1)) * 16 + hf * 8);
    }
  };
  auto stage_a = [&](_Float16 *dst) {  // this thread's pieces -> LDS, fragment layout (see the non-LOOP staging below)
    if constexpr (NATIVE) {
      if (tid < 256) {
        const int kg = tid >> 3, pg = tid & 7, kbk = kg >> 2, qq = kg & 1, hf = (kg >> 1) & 1, px = 8 * pg;
        _Float16 *d = dst + (((((kbk * 2 + (px >> 5)) * 2 + qq) * 2 + hf) * 32 + (px & 31)) * 4);
#pragma unroll
        for (int j = 0; j < 8; j++) {   // pixel j: its four channels
          half4 o;
#pragma unroll
          for (int c = 0; c < 4; c++) o[c] = anat[c][j];
          *reinterpret_cast<half4 *>(d + 4 * j) = o * (_Float16)0.25f;   // (corr.py:67-68: both maps / 4, one rounding to half)
        }
      }
      return;
    }
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const int idx = tid + 512 * u, kbk = idx >> 7, r = idx & 127, px = r >> 1, hf = r & 1;
      const int fa = ((((kbk * 2 + (px >> 5)) * 2 + 0) * 2 + hf) * 32 + (px & 31)) * 4;
      half4 lo, hi;
#pragma unroll
      for (int c = 0; c < 4; c++) lo[c] = apre[u][c], hi[c] = apre[u][4 + c];
      *reinterpret_cast<half4 *>(dst + fa) = lo;
      *reinterpret_cast<half4 *>(dst + fa + 2 * 32 * 4) = hi;
    }
  };
  if constexpr (LOOP) {
    const int ty = min(ty0 + wave, h2 - 1);
    if constexpr (NATIVE_B) {
      // k-step ks: 16 channels x 64 targets of row ty = 128 pieces of 8 targets x 1 channel, two per lane
      const _Float16 *Be = Bm + (size_t)e * HW2 * C + (size_t)ty * w2;
      const int kq = lane >> 3, tx0 = min(8 * (lane & 7), w2 - 8);
      half8 raw[KSL][2];
#pragma unroll
      for (int ks = 0; ks < KSL; ks++)
#pragma unroll
        for (int u = 0; u < 2; u++)
          raw[ks][u] = *reinterpret_cast<const half8 *>(Be + (size_t)(16 * ks + kq + 8 * u) * HW2 + tx0);
      _Float16 *scr = T + wave * (64 * 16);   // (the tile's LDS: nothing lives there before the first strip)
#pragma unroll
      for (int ks = 0; ks < KSL; ks++) {
#pragma unroll
        for (int u = 0; u < 2; u++)
#pragma unroll
          for (int j = 0; j < 8; j++) scr[(8 * (lane & 7) + j) * 16 + kq + 8 * u] = raw[ks][u][j] * (_Float16)0.25f;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int t = 0; t < NT; t++) bres[ks][t] = *reinterpret_cast<const half8 *>(scr + (t * 32 + l31) * 16 + kh);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      }
    } else {
#pragma unroll
    for (int t = 0; t < NT; t++) {
      const _Float16 *bpt = Bm + (size_t)e * HW2 * C + (size_t)min(ty * w2 + t * 32 + l31, HW2 - 1) * 16 + kh;
#pragma unroll
      for (int ks = 0; ks < KSL; ks++) bres[ks][t] = *reinterpret_cast<const half8 *>(bpt + (size_t)ks * 16 * HW2);
    }
    }
    // (pinned: left to itself the compiler sinks these loads into the strip loop and re-reads the fragments per strip)
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
      for (int ks = 0; ks < KSL; ks++) asm volatile("" : "+v"(bres[ks][t]));
    request_a(s_begin);
    stage_a(Ab0);
  }
  for (int strip = s_begin; strip < s_end; strip++) {
  const int p0 = strip * 64;                       // first source pixel of the strip
  _Float16 *Ab = LOOP ? Ab0 + ((strip - s_begin) & 1) * OPERAND_HALVES : Ab0;
  // LOOP: the next strip's operand is requested now and consumed after this strip's tile write, i.e. BEFORE this strip's
  // stores are issued: the wait for it (loads and stores of a wave complete in order) then only covers the previous
  // strip's stores, which have had this strip's whole multiplication to drain
  if constexpr (LOOP) {
    if (strip + 1 < s_end) request_a(strip + 1);
  }

  // ---- the strip's source operand, shared by the 8 waves: [C/16][64 pixels][16] halves into the (still unused) tile ----
  // (k-block-major like the global map, so a k-step's fragment is 32 lanes x 32 B contiguous: conflict-free b128 reads)
  if constexpr (!LOOP) {
    const _Float16 *Ae = A + (size_t)e * HW1 * C;
    const int kblocks = C >> 4;
    for (int idx = tid; idx < kblocks * 128; idx += 512) {  // 16-byte pieces: [kblock][pixel][half of the 16 channels]
      const int kbk = idx >> 7, r = idx & 127, px = r >> 1, hf = r & 1;
      const half8 v = *reinterpret_cast<const half8 *>(Ae + ((size_t)kbk * HW1 + min(p0 + px, HW1 - 1)) * 16 + hf * 8);
      // LDS layout [k-step][32-pixel block][q][k-half][pixel][4 halves] (q inside the block since round 6: a lane's two halves
      // pair up into one two-address read whose registers are the fragment): a wave's fragment read is TWO ds_read_b64 of
      // 512 consecutive bytes each (3.4 cycles of the LDS pipe per instruction; the one ds_read_b128 at a 32-byte pitch
      // this replaces takes 32: scratch/lds_rates.hip)
      const int fa = ((((kbk * 2 + (px >> 5)) * 2 + 0) * 2 + hf) * 32 + (px & 31)) * 4;
      half4 lo, hi;
#pragma unroll
      for (int c = 0; c < 4; c++) lo[c] = v[c], hi[c] = v[4 + c];
      *reinterpret_cast<half4 *>(T + fa) = lo;
      *reinterpret_cast<half4 *>(T + fa + 2 * 32 * 4) = hi;
    }
  }
  if constexpr (LOOP) lds_barrier();  // (a __syncthreads would wait for the previous strip's stores)
  else __syncthreads();

  // ---- MFMA: acc[i][j] = 32x32 tile (sources 32 i .. , targets 32 j ..) of target row ty0 + wave ------------------
  float16v acc[2][NT];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < NT; j++)
#pragma unroll
      for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;
  auto read_a = [&](int ks, half8 (&a)[2]) {
#pragma unroll
    for (int t = 0; t < 2; t++) {
      const _Float16 *fp = Ab + ((((ks * 2 + t) * 2 + 0) * 2 + (lane >> 5)) * 32 + l31) * 4;
      const half4 lo = *reinterpret_cast<const half4 *>(fp), hi = *reinterpret_cast<const half4 *>(fp + 2 * 32 * 4);
#pragma unroll
      for (int c = 0; c < 4; c++) a[t][c] = lo[c], a[t][4 + c] = hi[c];
    }
  };
  if constexpr (LOOP) {
#pragma unroll
    for (int ks = 0; ks < KSL; ks++) {
      half8 a[2];
      read_a(ks, a);
#pragma unroll
      for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < NT; j++)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(bres[ks][j], a[i], acc[i][j], 0, 0, 0);  // targets x sources
    }
  } else {
    const int ty = min(ty0 + wave, h2 - 1);  // rows past the map are computed on a valid row and never stored
    const _Float16 *bp[NT];  // k-block-major map: element (k, pixel) at ((k >> 4) * HW + pixel) * 16 + (k & 15)
#pragma unroll
    for (int t = 0; t < NT; t++) bp[t] = Bm + (size_t)e * HW2 * C + (size_t)min(ty * w2 + t * 32 + l31, HW2 - 1) * 16 + kh;
    const size_t kb = (size_t)HW2;  // elements between consecutive k-blocks / 16
    // target fragments two k-steps ahead of their use (L2 latency), source fragments from LDS right before it
    half8 b0[NT], b1[NT], b2[NT];
    const int ksteps = C >> 4;
#pragma unroll
    for (int t = 0; t < NT; t++) {
      b0[t] = *reinterpret_cast<const half8 *>(bp[t]);
      b1[t] = *reinterpret_cast<const half8 *>(bp[t] + (size_t)min(1, ksteps - 1) * 16 * kb);
    }
    for (int ks = 0; ks < ksteps; ks++) {
      const int kn = min(ks + 2, ksteps - 1);  // (the last steps re-request a fragment: no branch in the loop)
#pragma unroll
      for (int t = 0; t < NT; t++) b2[t] = *reinterpret_cast<const half8 *>(bp[t] + (size_t)kn * 16 * kb);
      half8 a[2];
      read_a(ks, a);
#pragma unroll
      for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < NT; j++)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(b0[j], a[i], acc[i][j], 0, 0, 0);  // targets x sources
#pragma unroll
      for (int t = 0; t < NT; t++) {
        b0[t] = b1[t];
        b1[t] = b2[t];
      }
    }
  }
  lds_barrier();  // every wave is done with the source operand: the tile takes its place
  // D layout: col = lane & 31 (source within the 32-block), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) (target tx):
  // four consecutive targets of one source per register quad -> one 8-byte LDS write
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < NT; j++)
#pragma unroll
      for (int rq = 0; rq < 4; rq++) {
        const int src = i * 32 + l31;
        const int tx = j * 32 + 8 * rq + 4 * (lane >> 5);
        half4 v;
#pragma unroll
        for (int q = 0; q < 4; q++) v[q] = (_Float16)acc[i][j][4 * rq + q];
        *reinterpret_cast<half4 *>(T + src * PITCH + wave * RP + tx) = v;
      }
  // columns 0..3 once more behind column w2 - 1 (after the row's own writes: for w2 < W2P those put unused targets
  // there): a store lane's four diagonal reads then never wrap inside a quad
  if (lane < 32) {
#pragma unroll
    for (int i = 0; i < 2; i++) {
      _Float16 *wr = T + (i * 32 + l31) * PITCH + wave * RP + w2;
#pragma unroll
      for (int q = 0; q < 4; q++) wr[q] = (_Float16)acc[i][0][q];
    }
  }
  lds_barrier();  // the last barrier: everything below reads the tile only
  if constexpr (LOOP) {
    if (strip + 1 < s_end) stage_a(Ab0 + ((strip + 1 - s_begin) & 1) * OPERAND_HALVES);  // ahead of this strip's stores
  }

  // ---- this lane's source pixel (levels 2, 3: a lane is one pixel) and its QUAD of pixels (levels 0, 1) ------------------
  const SrcMap map{HW1, w1, inv_w1, tiled != 0};   // (corr_build_tile.h)
  const int p = p0 + lane;
  const bool active = p < HW1;
  int x1, y1;
  map.xy(p, x1, y1);
  const EdgePlanes planes{L, oslots ? oslots[e] : e, h2, w2, HW1p};
  const unsigned plane_bytes = planes.plane_bytes();

  // Levels 0 and 1 carry 94 % of the bytes.  A 2-byte-per-lane store instruction costs the vector memory pipe as much as
  // an 8-byte one (~13 cycles per wave instruction: 10 B/clk/CU, which capped the store phases), so there a lane owns
  // FOUR consecutive pixels (q = lane & 15) of one of four lines (g = lane >> 4) and stores 8 bytes: one instruction is
  // four full 128-byte lines.  A quad whose pixels do not share a source row (a strip that spans a row end, or the last
  // pixels of the map) is not stored by its lanes but by the whole wave afterwards (`irregular`).
  const int q4 = (lane & 15) * 4, g = lane >> 4;
  int qx[4], qy[4];
#pragma unroll
  for (int i = 0; i < 4; i++) map.xy(p0 + q4 + i, qx[i], qy[i]);
  const bool quad_regular = (p0 + q4 + 3 < HW1) && (qy[0] == qy[3]);
  // Quads that are not regular are rare (one per row end inside the strip, one at the end of the map) but their four
  // pixels sit on four different lines: the WHOLE wave takes them, lane = (pixel lane & 3 of the quad, offset lane >> 2),
  // sixteen offsets per 2-byte store instruction -- w2 / 16 instructions per such quad.  (Left to the quad's own four
  // lanes, as until round 3, they cost 4 x w2 / 4 instructions issued by a wave with 4 of 64 lanes alive: strips with a
  // row end took 2.5-3x as long, which is most of what 28x107 and 55x55 lost against 64x64.)
  const unsigned long long irregular = __ballot(!quad_regular && g == 0 && (p0 + q4 < HW1));  // bit = quad index (wave-uniform)
  const int ipx = lane & 3, idx16 = lane >> 2;
  // ---- level 0: Vs0[(ty - y1) mod h2][dx][pixel] = T[pixel][ty][(x1 + dx) mod w2], this wave's own target row.  A lane's
  // quad of pixels reads the tile along a diagonal (pixel + 1, column + 1); with columns 0..3 replicated behind the row
  // only the first column wraps, once per line, and the store offset just advances by four planes: ~10 VALU
  // instructions per 8-byte store where the general form needs ~70 ----
  // Tiled pixel order (common.h): the strip is a 4 x 16 tile of the map, its quads sit on four source rows, and a line of
  // the planes holds all four at ONE dy = ty - y1.  So that a store instruction still writes whole lines, the quads of tile
  // row rr take the target row (wave + rr) mod 8 of the workgroup's tile instead of the wave's own: dy is then the same for
  // every lane of waves 0..4 (four full lines per instruction), and two values, 8 apart, in waves 5..7.  (With the wave's
  // own row for every quad each instruction wrote sixteen 32-byte pieces: 16.7 against 14.7 us per edge.)
  const int rr = tiled ? ((lane & 15) >> 2) : 0;
  {
    const int wrow = (wave + rr) & (FT_ROWS - 1);
    const int ty = ty0 + wave, tyq = ty0 + wrow;
    if (tiled || ty < h2) {  // (wave-uniform)
      const __amdgpu_buffer_rsrc_t r0 = planes.rsrc(0);
      if (quad_regular && tyq < h2) {
        int t = qx[0] + g;
        t -= (t >= w2) ? w2 : 0;
        int dy = tyq - qy[0];
        dy += (dy < 0) ? h2 : 0;
        unsigned voff = ((unsigned)dy * (unsigned)w2 + (unsigned)g) * plane_bytes + 2u * (unsigned)(p0 + q4);
        const _Float16 *lb = T + q4 * PITCH + wrow * RP;
        for (int dx0 = 0; dx0 < w2; dx0 += 16) {  // four lines per batch: their 16 LDS reads are in flight together
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
            __builtin_amdgcn_raw_buffer_store_b64(d, r0, (dx0 + 4 * b + g < w2) ? voff : OOR, 0, 0);
            voff += 4u * plane_bytes;
          }
        }
      }
      // (this kernel's own text of irregular_store, corr_build_tile.h: on the shared one the walk at 24 x 30 measured slower)
      for (unsigned long long m = (ty < h2) ? irregular : 0ull; m; m &= m - 1) {
        const int pl = 4 * (int)__builtin_ctzll(m) + ipx;  // this lane's pixel of the quad, within the strip
        int xi, yi;
        map.xy(p0 + pl, xi, yi);
        const bool pok = p0 + pl < HW1;
        int dy = ty - yi;
        dy += (dy < 0) ? h2 : 0;
        const _Float16 *row = T + pl * PITCH + wave * RP;
        const unsigned vbase = (unsigned)dy * (unsigned)w2 * plane_bytes + 2u * (unsigned)(p0 + pl);
        for (int dx0 = 0; dx0 < w2; dx0 += 16) {
          const int dx = dx0 + idx16;
          int tx = xi + dx;
          tx -= (tx >= w2) ? w2 : 0;
          tx = min(tx, w2 - 1);  // (dx beyond the map in the last group: read something valid, store nothing)
          const _Float16 v = row[tx];
          __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, v), r0,
                                                (pok && dx < w2) ? vbase + (unsigned)dx * plane_bytes : OOR, 0, 0);
        }
      }
    }
  }
  // ---- levels 1..3.  Each thread pools ONE 8 x 8 block of one source pixel's tile into its 4 x 4 level-1, 2 x 2 level-2
  // and 1 level-3 values (from the ROUNDED level below each time), all in registers; after one barrier (every read of
  // the tile, the level-0 stores included, is done) the values take the tile's place in LDS, after a second one the
  // three sheared store loops read them.  (Pooling every element in the lane that stores it needs no barrier at all
  // but 2.4x the arithmetic -- the kernel is bound by VALU issue, 1935 instructions per wave before, see the header.)
  constexpr int RP1 = G::RP1;                      // level-1 row: w2 >> 1 columns, then columns 0..3 once more
  _Float16 *P1 = T, *P2 = P1 + G::P2_OFF, *P3 = P1 + G::P3_OFF;   // the pooled region (TileGeom)
  constexpr int NBLK = W2P / 8;                    // 8-column blocks per pixel
  constexpr int PER = 64 * NBLK / 512;             // blocks per thread (1 for 64-wide tiles, 2 for 128-wide)
  _Float16 q1[PER][4][4], q2[PER][2][2], q3[PER];
#pragma unroll
  for (int u = 0; u < PER; u++) {
    const int blk = tid + 512 * u, src = blk / NBLK, cb = blk - src * NBLK;
    pool_block<RP>(T + src * PITCH + 8 * cb, q1[u], q2[u], q3[u]);
  }
  lds_barrier();  // every read of the level-0 tile is done (its sheared store above included)
#pragma unroll
  for (int u = 0; u < PER; u++) {
    const int blk = tid + 512 * u, src = blk / NBLK, cb = blk - src * NBLK;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      half4 v;
#pragma unroll
      for (int c = 0; c < 4; c++) v[c] = q1[u][r][c];
      _Float16 *row1 = P1 + (src * 4 + r) * RP1;
      if (4 * cb + 4 <= (w2 >> 1)) {
        *reinterpret_cast<half4 *>(row1 + 4 * cb) = v;
      } else {  // the block that holds column (w2 >> 1) - 1: the columns behind it belong to the copy of block 0
#pragma unroll
        for (int c = 0; c < 4; c++)
          if (4 * cb + c < (w2 >> 1)) row1[4 * cb + c] = q1[u][r][c];
      }
      if (cb == 0) {
#pragma unroll
        for (int c = 0; c < 4; c++) row1[(w2 >> 1) + c] = q1[u][r][c];
      }
    }
#pragma unroll
    for (int r = 0; r < 2; r++) {
      half2v v;
      v.x = q2[u][r][0], v.y = q2[u][r][1];
      *reinterpret_cast<half2v *>(P2 + (src * 2 + r) * (W2P / 4) + 2 * cb) = v;
    }
    P3[src * (W2P / 8) + cb] = q3[u];
  }
  lds_barrier();
  {  // level 1: 4 rows x (w2 >> 1) offsets, four lines per store instruction; wave w takes row w & 3 and every other
     // group of four offsets.  The quad's columns (x >> 1) - (x0 >> 1) are 0, 0|1, 1, 1|2: lane constants
    const int w2l = w2 >> 1, h2l = h2 >> 1;
    const __amdgpu_buffer_rsrc_t rl = planes.rsrc(1);
    const int tyl = wave & 3, tyg = (ty0 >> 1) + tyl;
    // (tiled: the quads of tile rows 2, 3 -- level-1 source row + 1 -- take the next pooled row, see level 0)
    const int tylq = (tyl + (rr >> 1)) & 3, tygq = (ty0 >> 1) + tylq;
    if (tiled || tyg < h2l) {  // floor sizes of avg_pool2d: the last partial row of the level below is dropped
      if (quad_regular && tygq < h2l) {
        const int xh = qx[0] >> 1;
        const int o1 = (qx[1] >> 1) - xh, o2 = (qx[2] >> 1) - xh, o3 = (qx[3] >> 1) - xh;
        int t = xh + 4 * (wave >> 2) + g;
        t -= (t >= w2l) ? w2l : 0;
        t -= (t >= w2l) ? w2l : 0;  // (maps down to 8 columns: twice)
        int dy = tygq - (qy[0] >> 1);
        dy += (dy < 0) ? h2l : 0;
        unsigned voff = ((unsigned)dy * (unsigned)w2l + (unsigned)(4 * (wave >> 2) + g)) * plane_bytes + 2u * (unsigned)(p0 + q4);
        const _Float16 *lb = P1 + (q4 * 4 + tylq) * RP1;
        for (int dx0 = 4 * (wave >> 2); dx0 < w2l; dx0 += 8) {
          const _Float16 *pp = lb + t;
          const unsigned short a0 = __builtin_bit_cast(unsigned short, pp[0]), a1 = __builtin_bit_cast(unsigned short, pp[4 * RP1 + o1]);
          const unsigned short a2 = __builtin_bit_cast(unsigned short, pp[8 * RP1 + o2]), a3 = __builtin_bit_cast(unsigned short, pp[12 * RP1 + o3]);
          u2v d;
          d.x = (unsigned)a0 | ((unsigned)a1 << 16);
          d.y = (unsigned)a2 | ((unsigned)a3 << 16);
          __builtin_amdgcn_raw_buffer_store_b64(d, rl, (dx0 + g < w2l) ? voff : OOR, 0, 0);
          voff += 8u * plane_bytes;
          t += 8;
          t -= (t >= w2l) ? w2l : 0;
          t -= (t >= w2l) ? w2l : 0;
        }
      }
      for (unsigned long long m = (tyg < h2l) ? irregular : 0ull; m; m &= m - 1) {  // (the two waves of a row take alternate groups of 16 offsets)
        const int pl = 4 * (int)__builtin_ctzll(m) + ipx;
        int xi, yi;
        map.xy(p0 + pl, xi, yi);
        const bool pok = p0 + pl < HW1;
        int dy = tyg - (yi >> 1);
        dy += (dy < 0) ? h2l : 0;
        const _Float16 *row = P1 + (pl * 4 + tyl) * RP1;
        const unsigned vbase = (unsigned)dy * (unsigned)w2l * plane_bytes + 2u * (unsigned)(p0 + pl);
        for (int dx0 = 16 * (wave >> 2); dx0 < w2l; dx0 += 32) {
          const int dx = dx0 + idx16;
          int tx = (xi >> 1) + dx;
          tx -= (tx >= w2l) ? w2l : 0;
          tx = min(tx, w2l - 1);
          const _Float16 v = row[tx];
          __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, v), rl,
                                                (pok && dx < w2l) ? vbase + (unsigned)dx * plane_bytes : OOR, 0, 0);
        }
      }
    }
  }
  // levels 2 and 3: a lane is one source pixel, (ty_l, dx) segments are dealt to the waves
  auto store_level = [&](int lvl, const _Float16 *Pl, int rows, int pitch_cols) {
    const int h2l = h2 >> lvl, w2l = w2 >> lvl;
    const __amdgpu_buffer_rsrc_t rl = planes.rsrc(lvl);
    const int x1l = x1 >> lvl, y1l = y1 >> lvl;
    for (int seg = wave; seg < rows * w2l; seg += 8) {  // (wave-uniform)
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
  store_level(2, P2, 2, W2P / 4);
  store_level(3, P3, 1, W2P / 8);
  }  // strips of this workgroup
}

// LDS: the tile (the pooled region and, in the one-strip form, the source operand -- at most 64 x 512 halves -- live inside it);
// the walk keeps two operand buffers behind it
template <int NT, bool LOOP>
constexpr size_t walk8_lds_bytes() {
  return sizeof(_Float16) * (size_t)(TileGeom<32 * NT>::TILE + (LOOP ? 2 * OPERAND_HALVES : 0));
}
static_assert(walk8_lds_bytes<2, true>() <= LDS_MAX_BYTES && walk8_lds_bytes<4, false>() <= LDS_MAX_BYTES, "LDS of a CU");
static_assert(64 * 512 <= TileGeom<64>::TILE, "the one-strip form stages 64 pixels x C <= 512 channels inside the tile");

template <int NT, bool LOOP, bool NATIVE = false, bool NATIVE_B = NATIVE>
static int walk8_launch(const BuildArgs &a, hipStream_t s) {
  constexpr size_t lds = walk8_lds_bytes<NT, LOOP>();
  static DeviceOnce attr_once;
  if (attr_once.needed()) {
    DBA_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&corr_build_fused_kernel<NT, LOOP, NATIVE, NATIVE_B>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr_once.done();
  }
  const int nstrips = a.HW1p / 64, spw = LOOP ? a.spw : 1;
  const dim3 grid((nstrips + spw - 1) / spw, (a.h2 + FT_ROWS - 1) / FT_ROWS, a.n);
  hipLaunchKernelGGL((corr_build_fused_kernel<NT, LOOP, NATIVE, NATIVE_B>), grid, dim3(512), lds, s, a.A, a.Bm, a.L, a.C, a.h1, a.w1,
                     a.h2, a.w2, a.HW1p, a.inv_w1, spw, a.oslots, a.tiled);
  return DBA_OK;
}

int corr_build_walk8_launch(int route, const BuildArgs &a, hipStream_t s) {
  switch (route) {
    case DBA_CORR_ROUTE_WALK_NATIVE: return walk8_launch<2, true, true>(a, s);
    case DBA_CORR_ROUTE_WALK_NATIVE_B: return walk8_launch<2, true, false, true>(a, s);
    case DBA_CORR_ROUTE_WALK_COPY: return walk8_launch<2, true>(a, s);
    case DBA_CORR_ROUTE_STRIP_64: return walk8_launch<2, false>(a, s);
    case DBA_CORR_ROUTE_STRIP_128: return walk8_launch<4, false>(a, s);
    default: return DBA_ERR_ARG;
  }
}

}  // namespace dba
