// Fused all-pairs correlation + 4-level pyramid + flow-aligned ("sheared") store, gfx950 MFMA, any map size.
//
// One pass replaces CorrBlock.corr (torch.matmul), the three avg_pool2d passes of CorrBlock.__init__
// (/root/reference/dbaf/modules/corr.py:24-38, :63-71) and the re-layout into the sheared volume
// (corr_sheared.hip): the reference materialises level 0 (33.5 MB/edge at 64x64), reads it back three times for the
// pooling, and this repo's unfused path then reads and rewrites every level once more for the shear.
// Here every output byte is written exactly once (44.6 MB/edge) and the inputs (2 x 1 MB/edge) stay in L2.
//
// Workgroup = 8 waves; tile = one STRIP of 64 consecutive source pixels of the flattened (y1, x1) index (the unit the
// lookup reads, see corr_sheared.hip) x 8 target rows ty0..ty0+7 x all w2 target columns (w2 <= 128):
//   * wave w owns target row ty0 + w: 64 sources x (32 NT) targets = 2 x NT v_mfma_f32_32x32x16_f16 tiles computed as
//     targets x sources, so that a register quad is four consecutive targets of one source (one 8-byte LDS write);
//     16-byte fragment loads straight from the k-block-major feature maps [C/16][HW][16] (corr_build.hip; L2-resident,
//     8 full lines per load instruction), the next k-step's fragments are requested before the current one is
//     multiplied;
//   * accumulators -> f16 (the single rounding of the reference's half GEMM) -> LDS tile T[source][ty][tx];
//   * stores: every element goes from the tile to Vs_l[(ty_l - (y1 >> l)) mod h2l][dx][pixel] with PER-PIXEL offsets, so
//     any map width works (a strip may span a row end).  Levels 0 and 1 (94 % of the bytes): a lane owns four
//     consecutive pixels of one of four (dy, dx) lines and stores 8 bytes (a quad that spans a row end is stored by the
//     whole wave, 2 bytes per lane, sixteen offsets per instruction); levels 2, 3: a lane is one pixel.  The barriers synchronise LDS only (`s_waitcnt lgkmcnt(0); s_barrier`): a
//     `__syncthreads()` would drain every outstanding store first;
//   * levels 1..3: 2x2 averages of the ROUNDED level below (== F.avg_pool2d on half, floor sizes): each thread pools one
//     8 x 8 block of the tile down to its 4 x 4 + 2 x 2 + 1 values in registers, which then take the dead tile's place in
//     LDS (two barriers) for the sheared store loops;
//   * the strip's source operand (16 KB at C = 128) is staged ONCE per workgroup in the LDS the tile will take, and the
//     target fragments are requested two k-steps ahead.
// Where the time goes, one-strip form (in-kernel timestamps, 64x64, 32 edges; a workgroup lives 47 k cycles,
// two per CU): source operand 9 %, MFMA phase 43 % (the 32 MFMAs per wave need a third of it; the rest is the target
// fragments, 16 KB per wave out of L2 at ~20 B/clk/CU), tile write 6 %, level-0 stores 25 %, pooled levels 13 %, drain
// 3 %: 517 us per 32 edges = 16.2 us per edge, 0.36 of the HBM peak on the kernel alone (round 1: 23.3 us; before the
// store loops below were cut from ~70 to ~10 VALU instructions per 8-byte store: 20.1 us, 1935 VALU instructions per
// wave, VALU busy 64 %).  The strip-walking form (LOOP, see the kernel's comment) takes 413-439 us = 12.9-13.7 us per
// edge, 0.43-0.45: ~21 k cycles per strip and wave, of which level-0 stores + pooling 7.1 k, pooled stores 4.5 k, 3.3-4.4 k
// at the top of a strip (the next operand's loads wait behind the previous strip's stores), products 2.4 k, tile write 1.9 k.
// What was measured and did not help (scratch/cu_rates.hip, scratch/lds_rates.hip, scratch/corr_build_pipe_experiment.hip):
//   * one CU alone stores 28 B/clk, the whole chip 5.4-5.6 TB/s = 9 B/clk/CU: in the store phases, which all
//     workgroups enter together, the chip is at HBM's write ceiling, in the MFMA phases HBM idles.  A persistent,
//     wave-specialised form (8 compute + 8 store waves, tile double-buffered in LDS, stores of tile i - 1 issued while
//     tile i is multiplied) was built and is bit-exact, but runs at 20.5-21.5 us/edge: its waves wait 63 % of their
//     cycles at the three barriers that couple the roles (VALU busy 28 %, LDS busy 17 %);
//   * target map in blocks of 8 channels (a half wave's fragment load = 512 contiguous bytes): no change;
//   * staggered start of the two co-resident workgroups, 4-deep fragment prefetch: no change.
// Halving the fragment traffic needs a 128-pixel tile (132 KB of LDS, one workgroup per CU).
// Operands (round 5): where 16-byte pieces of the maps are aligned (map width a multiple of 8) the strip-walking form reads
// the caller's [n][C][h][w] maps as they lie (NATIVE below) -- the two fmap_pixel_major_kernel launches (20 us each per 32
// edges at 64x64) and their scratch traffic are gone; the kernel itself pays ~1 % for the 32-byte pieces a tiled strip's
// channel slice consists of (16.9 against 17.6 us per edge end to end; DBA_BUILD_OPERANDS=copy|bnative for the A/B run).
// Shapes: w2 <= 128, C % 16 == 0, 4 levels, h2 >> 3 >= 1, w2 >> 3 >= 1; anything else takes the unfused path of
// corr_build.hip + corr_shear_kernel.
// The kernels, one file each, each with its launch function (declared in corr_build_tile.h, which also holds every phase they share):
//   corr_build_walk8.hip     corr_build_fused_kernel<NT, LOOP, NATIVE, NATIVE_B> -- the eight-wave forms described above (maps up to 32
//                            wide, tiled planes that miss the sixteen-wave form's conditions, widths that are multiples of 8 on linear
//                            planes, 128-wide tiled planes)
//   corr_build_fused16.hip   corr_build_fused16_kernel -- the strip walk on sixteen waves, tiled planes, 64 columns (the headline shapes)
//   corr_build_fused16g.hip  corr_build_fused16g_kernel<W2C> -- the same walk on linear planes, 33..63 columns whose 16-byte pieces are
//                            not aligned (55 x 55)
//   corr_build_fused16w.hip  corr_build_fused16w_kernel -- one strip per workgroup on sixteen waves, linear planes, 65..128 columns
// This file decides: corr_build_route picks the kernel, strips_per_wg the length of a walk, the entry point copies the operands the
// route needs and switches on it.  DBA_BUILD_WAVES=8 / DBA_BUILD_KERNEL / DBA_BUILD_OPERANDS force the older forms (tests, A/B runs).
// Forms that were measured and are not kept (commit 18ba9af is the last that carries their text and the two in-kernel phase
// timers the profiles cite):
//   * cache policy bits on the level stores (sc0 / nt / sc1): measured, slower, see profiles/r06_late_experiments.txt, item 4
//   * row tiles dealt to the XCDs as dispatched, without xcd_remap: measured, slower, see profiles/LOOKUP_NOTES.md
//   * fused16: pooled stores deferred into the next strip's product phase: measured, slower, see profiles/r06_build16.txt
//   * fused16: a row's level-0 stores split between its two waves in time: measured, slower, see profiles/r06_build16.txt
//   * fused16g: none or two batches of level-0 lines moved to the row's second wave: measured, slower, see profiles/r06_build_g16.txt
//   * walks longer than 16 strips outside fused16g, and the rule that aimed at 256 workgroups: measured, slower, see
//     profiles/r06_build_wg.txt and profiles/r06_build_g16.txt
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>

#include "corr_build_tile.h"

namespace dba {

// defined in corr_build.hip
__global__ void fmap_pixel_major_kernel(const _Float16 *in, _Float16 *out, int C, int HW, int kb, int w_tiled, int HWo, int w_grid);
__global__ void fmap_pixel_major_pair_kernel(const _Float16 *in1, _Float16 *out1, int w_tiled1, const _Float16 *in2, _Float16 *out2,
                                             int C, int HW, int kb, int n, int HWo1, int w_grid1);

}  // namespace dba

using namespace dba;

namespace {

// The environment switches of the build, each read once per process (A/B runs and the tests of the older forms)
struct BuildEnv {
  int force;        // DBA_BUILD_KERNEL=classic|loop forces one form where both apply: 0 automatic, 1 classic, 2 loop
  int native_mode;  // DBA_BUILD_OPERANDS=copy|bnative: 0 copies of both maps, 1 both maps as they lie, 2 the target map only
  bool waves16;     // DBA_BUILD_WAVES=8 keeps the eight-wave forms
};
const BuildEnv &build_env() {
  static const BuildEnv env = [] {
    BuildEnv v;
    const char *e = getenv("DBA_BUILD_KERNEL");
    v.force = !e ? 0 : (e[0] == 'c' ? 1 : (e[0] == 'l' ? 2 : 0));
    e = getenv("DBA_BUILD_OPERANDS");
    v.native_mode = !e ? 1 : (e[0] == 'c' ? 0 : (e[0] == 'b' ? 2 : 1));
    e = getenv("DBA_BUILD_WAVES");
    v.waves16 = !(e && atoi(e) == 8);
    return v;
  }();
  return env;
}

// Which kernel a SUPPORTED shape gets: the one place the launch conditions live (dba_corr_volume_build_route reports it, the
// launcher switches on it).  tiled / padded: the planes' pixel order (shear_grid) and whether the grid is larger than the map.
int corr_build_route(int C, int h1, int w1, int h2, int w2, bool tiled, bool padded, const BuildEnv &env) {
  const int HW1 = h1 * w1, HW2 = h2 * w2;
  // the strip walk for every map up to 64 wide at C = 128 (since the row-end quads are stored by the whole wave it also
  // wins where strips span row ends: 55x55 13.3 against 14.3 us/edge)
  const bool loop_form = (w2 <= 64 && C == 128 && env.force != 1);
  // sixteen waves per workgroup on planes in the linear pixel order: the general form, on the k-block-major copies
  // (where 16-byte pieces of the maps are aligned -- widths that are multiples of 8 -- the eight-wave walk on the caller's own maps
  // is as fast or faster: 40 x 56 6.1 against 6.2 us per edge, 30 x 40 2.6 against 2.8; profiles/r06_build_g16.txt)
  const bool general16 = loop_form && env.waves16 && !tiled && w2 > 32 && h1 == h2 && w1 == w2 && ((w2 % 8) != 0 || (HW2 % 8) != 0);
  // ... and, where 8-byte pieces of the maps are aligned, straight from the caller's [n][C][h][w] maps
  const bool native_b = loop_form && !general16 && !padded && env.native_mode != 0 && (w2 % 8 == 0) && (HW2 % 8 == 0);
  const bool native = native_b && env.native_mode == 1 && (HW1 % 8 == 0) && (w1 % 8 == 0);
  if (loop_form) {
    // 55 x 55 (the reference's TUM-VI demo, demo_vio_tumvi.py:55-60) has its own instantiation
    if (general16) return (w2 == 55) ? DBA_CORR_ROUTE_FUSED16G_55 : DBA_CORR_ROUTE_FUSED16G;
    if (native && tiled && w2 == 64 && (h2 % 8) == 0 && env.waves16) return DBA_CORR_ROUTE_FUSED16;   // the shapes the headline runs on
    if (native) return DBA_CORR_ROUTE_WALK_NATIVE;
    if (native_b) return DBA_CORR_ROUTE_WALK_NATIVE_B;
    return DBA_CORR_ROUTE_WALK_COPY;
  }
  if (w2 <= 64) return DBA_CORR_ROUTE_STRIP_64;
  // sixteen waves per workgroup where the planes keep the linear pixel order
  if (env.waves16 && !tiled && h1 == h2 && w1 == w2 && (C % 16) == 0 && C <= 512) return DBA_CORR_ROUTE_FUSED16W;
  return DBA_CORR_ROUTE_STRIP_128;
}

// Strips per workgroup of a strip walk.  One workgroup per CU (LDS), so the launch runs in ceil(workgroups / 256) rounds, each as
// long as a walk: spw strips + the prologue (the waves' target fragments, 128 KB per workgroup: ~1.5 strips' worth).  Pick the spw
// that minimises rounds x (spw + 1.5), at most 16 -- the general sixteen-wave walk may take a whole row of strips (36 edges at
// 55 x 55, the TUM-VI window, are 252 rows, one round of one walk each: 10.5 against 10.8 us per edge with the cap of 16; the other
// forms were measured with the cap).  rows: target-row tiles x edges.  forced_loop (DBA_BUILD_KERNEL=loop): at least two strips.
int strips_per_wg(int nstrips, long long rows, bool general16, bool forced_loop) {
  int spw = 1;
  double best = 1e300;
  const int cap = general16 ? nstrips : 16;
  for (int c = 1; c <= cap && c <= nstrips; c++) {
    const long long wgs = (long long)((nstrips + c - 1) / c) * rows;
    // (a last round that is partly empty is cheaper than a full one -- the walk is half chain, half memory traffic --: the
    // mean of whole and fractional rounds matches the measured picks, profiles/r06_build16.txt item 7)
    const double rounds = 0.5 * (double)((wgs + 255) / 256) + 0.5 * ((double)wgs / 256.0 < 1.0 ? 1.0 : (double)wgs / 256.0);
    const double cost = rounds * ((double)c + 1.5);
    if (cost <= best) best = cost, spw = c;   // (ties: the longer walk -- fewer prologues in total)
  }
  return (forced_loop && spw < 2) ? 2 : spw;
}

}  // namespace

extern "C" {

int dba_corr_volume_build_sheared_supported(int C, int h1, int w1, int h2, int w2, int num_levels) {
  if (C <= 0 || (C % 16) != 0 || num_levels != 4 || h1 <= 0 || w1 <= 0) return 0;
  if (w2 > 128 || (h2 >> 3) < 1 || (w2 >> 3) < 1) return 0;
  if (C > 512) return 0;  // the strip's source operand (64 x C halves) is staged inside the level-0 tile
  // dy = ty - (y1 >> l) and tx = (x1 >> l) + dx take ONE conditional wrap in every kernel: a source map more than one row or
  // column larger than the target map would be stored at wrapped offsets ("Correlation build: the statement")
  if (h1 > h2 + 1 || w1 > w2 + 1) return 0;
  const size_t elems0 = (size_t)h2 * w2 * (size_t)dba_corr_sheared_plane_elems(h1, w1);
  return (2 * elems0 < ((size_t)1 << 31)) ? 1 : 0;  // one edge-level is addressed through a 31-bit buffer range
}

int dba_corr_volume_build_route(int C, int h1, int w1, int h2, int w2, int num_levels) {
  if (!dba_corr_volume_build_sheared_supported(C, h1, w1, h2, w2, num_levels)) return DBA_CORR_ROUTE_UNFUSED;
  int h1g, w1g;
  const bool tiled = shear_grid(h1, w1, &h1g, &w1g);
  return corr_build_route(C, h1, w1, h2, w2, tiled, tiled && (h1g != h1 || w1g != w1), build_env());
}

int dba_corr_volume_build_sheared(const void *fmap1, const void *fmap2, void *const *sheared_levels, int n, int C,
                                  int h1, int w1, int h2, int w2, int num_levels, void *scratch,
                                  size_t scratch_bytes, dba_stream_t stream) {
  return dba_corr_volume_build_sheared_slots(fmap1, fmap2, sheared_levels, nullptr, n, C, h1, w1, h2, w2, num_levels, scratch,
                                             scratch_bytes, stream);
}

int dba_corr_volume_build_sheared_slots(const void *fmap1, const void *fmap2, void *const *sheared_levels,
                                        const int *out_slots, int n, int C, int h1, int w1, int h2, int w2, int num_levels,
                                        void *scratch, size_t scratch_bytes, dba_stream_t stream) {
  if (!dba_corr_volume_build_sheared_supported(C, h1, w1, h2, w2, num_levels)) return DBA_ERR_UNSUPPORTED;
  if (n < 0) return DBA_ERR_ARG;
  if (n == 0) return DBA_OK;
  if (!fmap1 || !fmap2 || !sheared_levels || !scratch) return DBA_ERR_ARG;
  if (scratch_bytes < dba_corr_volume_scratch_bytes(n, C, h1, w1, h2, w2)) return DBA_ERR_WORKSPACE;
  const int HW1 = h1 * w1, HW2 = h2 * w2;
  const int HW1p = dba_corr_sheared_plane_elems(h1, w1);
  hipStream_t s = (hipStream_t)stream;
  _Float16 *A = static_cast<_Float16 *>(scratch);
  _Float16 *Bm = reinterpret_cast<_Float16 *>(static_cast<char *>(scratch) + align_up((size_t)n * C * HW1p * 2, 256));
  // the source pixels in 4 x 16 tiles of the grid (h1g, w1g) >= the map: the planes' pixel order (common.h).  On a padded grid the
  // kernels below are handed the GRID as their source map -- a strip is a tile of it, the operand copy has a row per grid pixel,
  // and what the pad pixels' rows hold only ever reaches their own entries of the planes, which nobody reads
  int h1g, w1g;
  const int tiled = shear_grid(h1, w1, &h1g, &w1g) ? 1 : 0;
  const bool padded = tiled && (h1g != h1 || w1g != w1);
  const int h1k = tiled ? h1g : h1, w1k = tiled ? w1g : w1;
  const BuildEnv &env = build_env();
  const int route = corr_build_route(C, h1, w1, h2, w2, tiled != 0, padded, env);
  // what the route says about the operands and the walk (corr_build_route)
  const bool general16 = route == DBA_CORR_ROUTE_FUSED16G || route == DBA_CORR_ROUTE_FUSED16G_55;
  const bool native = route == DBA_CORR_ROUTE_FUSED16 || route == DBA_CORR_ROUTE_WALK_NATIVE;
  const bool native_b = native || route == DBA_CORR_ROUTE_WALK_NATIVE_B;
  const bool loop_form = general16 || native_b || route == DBA_CORR_ROUTE_WALK_COPY;
  const int HW1o = tiled ? HW1p : HW1;   // pixels per map of the source operand's copy
  if (!native && !native_b && HW1 == HW2 && 2 * (long long)n <= 65535)   // both copies in one launch
    hipLaunchKernelGGL(fmap_pixel_major_pair_kernel, dim3((HW1 + 63) / 64, (C + 63) / 64, 2 * n), dim3(256), 0, s,
                       static_cast<const _Float16 *>(fmap1), A, tiled ? w1 : 0, static_cast<const _Float16 *>(fmap2), Bm, C, HW1, 16, n,
                       HW1o, w1g);
  else {
    if (!native)
      hipLaunchKernelGGL(fmap_pixel_major_kernel, dim3((HW1 + 63) / 64, (C + 63) / 64, n), dim3(256), 0, s,
                         static_cast<const _Float16 *>(fmap1), A, C, HW1, 16, tiled ? w1 : 0, HW1o, w1g);
    if (!native_b)
      hipLaunchKernelGGL(fmap_pixel_major_kernel, dim3((HW2 + 63) / 64, (C + 63) / 64, n), dim3(256), 0, s,
                         static_cast<const _Float16 *>(fmap2), Bm, C, HW2, 16, 0, HW2, 0);
  }
  BuildArgs a;
  a.A = native ? static_cast<const _Float16 *>(fmap1) : A;
  a.Bm = native_b ? static_cast<const _Float16 *>(fmap2) : Bm;
  for (int l = 0; l < 4; l++) a.L.vs[l] = static_cast<_Float16 *>(sheared_levels[l]);
  a.n = n, a.C = C, a.h1 = h1k, a.w1 = w1k, a.h2 = h2, a.w2 = w2, a.HW1p = HW1p;
  a.inv_w1 = 1.0f / (float)w1k;
  a.spw = loop_form ? strips_per_wg(HW1p / 64, (long long)((h2 + FT_ROWS - 1) / FT_ROWS) * n, general16, env.force == 2) : 1;
  a.oslots = out_slots;
  a.tiled = tiled;
  int rc;
  switch (route) {
    case DBA_CORR_ROUTE_FUSED16: rc = corr_build_fused16_launch(a, s); break;
    case DBA_CORR_ROUTE_FUSED16G:
    case DBA_CORR_ROUTE_FUSED16G_55: rc = corr_build_fused16g_launch(route, a, s); break;
    case DBA_CORR_ROUTE_FUSED16W: rc = corr_build_fused16w_launch(a, s); break;
    default: rc = corr_build_walk8_launch(route, a, s); break;
  }
  if (rc != DBA_OK) return rc;
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

}  // extern "C"
