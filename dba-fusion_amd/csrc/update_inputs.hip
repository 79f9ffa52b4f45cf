// The statements of CovisibleGraph.update() between the update operator and video.ba (dbaf/covisible_graph.py:229-230,
// :242-247, :311-333, use_inactive=True), gfx950, two launches:
//   edge pass     one workgroup of 1024 lanes, no atomics.  t0 = max(1, min(ii) + 1) (:230); the inactive edges inside
//                 the window compacted in list order (flag_slot, edge_lists.h, :243) and the active list appended
//                 (:244-245); min / max of the concatenated lists (:327-328 and depth_video.py:327-348); torch.unique of
//                 the concatenated ii through a presence table in LDS (:330); one byte of flags per output edge: bit 0
//                 short baseline (:317-321), bit 1 ii == max(ii) (:327), bit 2 jj == max(jj) (:328); a result block of
//                 int32 words for the host and for the second launch.
//   payload pass  grid over (output edge, pixel chunk) and (damping row, pixel chunk).  Reads the edge's row of target /
//                 weight from the inactive or the active tensor ([n, ht, wd, 2], pixel-interleaved), applies the four
//                 weight rules (:311-328) and writes the planar [N, 2, ht, wd] rows of :332-333; damping rows
//                 0.2 * damping[kx[r]] + EP (:330).  It compares the counts the edge pass left with the counts its
//                 outputs were sized for: on a mismatch it writes zeros and raises a pinned host word.
//                 A second instantiation (dba_update_inputs_payload_op) takes the active rows from the update operator's
//                 outputs instead: target = coords1 + delta.float(), weight = weight.float() (:235-236), written out
//                 pixel-interleaved as the new graph.target / graph.weight and carried on in registers.
// Arithmetic.  torch on the device divides a tensor by a host scalar as a multiplication with the scalar's float32
// reciprocal (measured on the MI355X), one rounding per statement; `.2 * d + EP` is two kernels, two
// roundings.  Every float operation here goes through an intrinsic the compiler neither contracts nor re-associates.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "common.h"
#include "edge_lists.h"
#include "size_guard.h"

namespace dba {

constexpr int UI_THREADS = 1024;
constexpr int UI_WAVES = UI_THREADS / WAVE;
constexpr int UI_PAY_THREADS = 256;
constexpr int UI_FLAG_SHORT = 1, UI_FLAG_NEWEST_I = 2, UI_FLAG_NEWEST_J = 4;
constexpr int UI_INDEX_CLAMP = 1 << 30;

__device__ __forceinline__ float ui_mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float ui_add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float ui_sub(float a, float b) { return __fsub_rn(a, b); }

// lietorch shim, _cross / _qrot: each product and each difference is a torch kernel of its own
__device__ __forceinline__ void ui_cross(const float *a, const float *b, float *c) {
  c[0] = ui_sub(ui_mul(a[1], b[2]), ui_mul(a[2], b[1]));
  c[1] = ui_sub(ui_mul(a[2], b[0]), ui_mul(a[0], b[2]));
  c[2] = ui_sub(ui_mul(a[0], b[1]), ui_mul(a[1], b[0]));
}

// v + w * uv + cross(qv, uv), uv = 2 * cross(qv, v)
__device__ __forceinline__ void ui_qrot(const float *q, const float *v, float *out) {
  float uv[3], c[3];
  ui_cross(q, v, uv);
#pragma unroll
  for (int k = 0; k < 3; k++) uv[k] = ui_mul(2.0f, uv[k]);
  ui_cross(q, uv, c);
#pragma unroll
  for (int k = 0; k < 3; k++) out[k] = ui_add(ui_add(v[k], ui_mul(q[3], uv[k])), c[k]);
}

// || (T_i * T_j^-1).t ||: inv = (-qrot(qinv(q_j), t_j), qinv(q_j)), mul = qrot(q_i, t_B) + t_i.  The three squares are
// summed as torch.norm's device reduction sums a row of three: (x^2 + z^2) + y^2.
__device__ __forceinline__ float ui_baseline(const float *Pi, const float *Pj) {
  const float qinv[4] = {-Pj[3], -Pj[4], -Pj[5], Pj[6]};
  float r[3], t[3];
  ui_qrot(qinv, Pj, r);
#pragma unroll
  for (int k = 0; k < 3; k++) r[k] = -r[k];
  ui_qrot(Pi + 3, r, t);
#pragma unroll
  for (int k = 0; k < 3; k++) t[k] = ui_add(t[k], Pi[k]);
  return __fsqrt_rn(ui_add(ui_add(ui_mul(t[0], t[0]), ui_mul(t[2], t[2])), ui_mul(t[1], t[1])));
}

template <bool IS_MIN>
__device__ __forceinline__ int ui_block_minmax(int x, int *sh) {
  x = wave_minmax<IS_MIN>(x);
  if ((threadIdx.x & (WAVE - 1)) == 0) sh[threadIdx.x >> 6] = x;
  __syncthreads();
  int r = sh[0];
#pragma unroll
  for (int w = 1; w < UI_WAVES; w++) r = IS_MIN ? min(r, sh[w]) : max(r, sh[w]);
  __syncthreads();
  return r;
}

__device__ __forceinline__ int ui_clamp_index(int64_t v) {
  return (int)(v > UI_INDEX_CLAMP ? UI_INDEX_CLAMP : (v < -UI_INDEX_CLAMP ? -UI_INDEX_CLAMP : v));
}

// Capacities (the host allocates them): sel [n_inac]; ii_out, jj_out, flags [n_inac + n_act]; kx [min(B, n_inac + n_act)];
// res [DBA_UI_RES_WORDS].
__global__ __launch_bounds__(UI_THREADS) void update_inputs_edge_kernel(
    const int64_t *__restrict__ ii_inac, const int64_t *__restrict__ jj_inac, int n_inac,
    const int64_t *__restrict__ ii_act, const int64_t *__restrict__ jj_act, int n_act, const float *__restrict__ poses,
    int B, int has_t0, int64_t t0_arg, int64_t inac_range, float mask_threshold, int baseline_rule,
    int *__restrict__ sel, int64_t *ii_out, int64_t *jj_out, unsigned char *__restrict__ flags,
    int64_t *__restrict__ kx, int *__restrict__ res) {
  __shared__ int wcount[UI_WAVES];
  __shared__ int red[UI_WAVES];
  __shared__ unsigned char present[DBA_UI_MAX_FRAMES];
  const int tid = threadIdx.x;
  present[tid] = 0;  // (DBA_UI_MAX_FRAMES == UI_THREADS)

  // :230, over the ACTIVE list alone
  int64_t t0 = t0_arg;
  if (!has_t0) {
    int m = UI_INDEX_CLAMP;
    for (int p = tid; p < n_act; p += UI_THREADS) m = min(m, ui_clamp_index(ii_act[p]));
    m = ui_block_minmax<true>(m, red);
    t0 = m + 1 > 1 ? m + 1 : 1;
  } else {
    __syncthreads();
  }
  const int64_t oldest = t0 - inac_range;

  int lo_i = UI_INDEX_CLAMP, lo_j = UI_INDEX_CLAMP, hi_i = -UI_INDEX_CLAMP, hi_j = -UI_INDEX_CLAMP, bad = 0;
  // :243-245, the inactive edges inside the window, in list order
  int kept = 0;  // in the tiles before this one
  for (int start = 0; start < n_inac; start += UI_THREADS) {
    const int p = start + tid;
    int64_t i = 0, j = 0;
    bool k = false;
    if (p < n_inac) {
      i = ii_inac[p];
      j = jj_inac[p];
      k = i >= oldest && j >= oldest;
    }
    int total;
    const int q = kept + flag_slot<UI_THREADS>(k, wcount, &total);
    if (k) {
      sel[q] = p;
      ii_out[q] = i;
      jj_out[q] = j;
      const int ci = ui_clamp_index(i), cj = ui_clamp_index(j);
      lo_i = min(lo_i, ci), hi_i = max(hi_i, ci), lo_j = min(lo_j, cj), hi_j = max(hi_j, cj);
      if (i >= 0 && i < B) present[i] = 1;
      if (i < 0 || i >= B || j < 0 || j >= B) bad = 1;
    }
    kept += total;
  }
  const int n_sel = kept, N = n_sel + n_act;
  for (int p = tid; p < n_act; p += UI_THREADS) {
    const int64_t i = ii_act[p], j = jj_act[p];
    ii_out[n_sel + p] = i;
    jj_out[n_sel + p] = j;
    const int ci = ui_clamp_index(i), cj = ui_clamp_index(j);
    lo_i = min(lo_i, ci), hi_i = max(hi_i, ci), lo_j = min(lo_j, cj), hi_j = max(hi_j, cj);
    if (i >= 0 && i < B) present[i] = 1;
    if (i < 0 || i >= B || j < 0 || j >= B) bad = 1;
  }
  // (the barriers inside also order the writes of ii_out / jj_out / present before the reads below)
  lo_i = ui_block_minmax<true>(lo_i, red);
  lo_j = ui_block_minmax<true>(lo_j, red);
  hi_i = ui_block_minmax<false>(hi_i, red);
  hi_j = ui_block_minmax<false>(hi_j, red);
  bad = ui_block_minmax<false>(bad, red);

  // :330, torch.unique(ii): the frames present, ascending
  int n_kx;
  const bool seen = present[tid] != 0;
  const int q_kx = flag_slot<UI_THREADS>(seen, wcount, &n_kx);
  if (seen) kx[q_kx] = tid;

  // :317-321, :327-328
  for (int e = tid; e < N; e += UI_THREADS) {
    const int64_t i = ii_out[e], j = jj_out[e];
    int f = 0;
    if (baseline_rule && i >= 0 && i < B && j >= 0 && j < B) {
      float Pi[7], Pj[7];
#pragma unroll
      for (int k = 0; k < 7; k++) { Pi[k] = poses[7 * i + k]; Pj[k] = poses[7 * j + k]; }
      if (ui_baseline(Pi, Pj) < mask_threshold) f |= UI_FLAG_SHORT;
    }
    if (ui_clamp_index(i) == hi_i) f |= UI_FLAG_NEWEST_I;
    if (ui_clamp_index(j) == hi_j) f |= UI_FLAG_NEWEST_J;
    flags[e] = (unsigned char)f;
  }
  if (tid == 0) {
    res[0] = (int)(t0 > UI_INDEX_CLAMP ? UI_INDEX_CLAMP : (t0 < -UI_INDEX_CLAMP ? -UI_INDEX_CLAMP : t0));
    res[1] = n_sel;
    res[2] = N;
    res[3] = n_kx;
    res[4] = lo_i;
    res[5] = hi_i;
    res[6] = lo_j;
    res[7] = hi_j;
    res[8] = bad;  // an index outside [0, B): the host raises
  }
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// where the active rows come from: the graph's target / weight tensors, or the update operator's outputs in float32 / float16
constexpr int UI_SRC_GRAPH = 0, UI_SRC_OP_F32 = 1, UI_SRC_OP_F16 = 2;

struct PayloadArgs {
  const float *target_inac, *weight_inac, *target_act, *weight_act, *disps, *damping;
  // UI_SRC_OP_*: coords1 [n_act, ht, wd, 2] f32, delta and weight_op likewise in the operator's dtype; target_new, weight_new
  // [n_act, ht, wd, 2] f32 out; act_tail0: the first active row that no output row [exp_n_sel, exp_N) covers
  const float *coords1;
  const void *delta, *weight_op;
  float *target_new, *weight_new;
  int act_tail0;
  const int *sel, *res;
  const int64_t *ii_out, *kx;
  const unsigned char *flags;
  float *target_out, *weight_out, *damping_out;
  int *status;  // pinned host words
  int n_inac, n_act, B, HW, chunks, exp_n_sel, exp_N, exp_n_kx, far_rule;
  float far_threshold, ep;
};

constexpr float UI_INV_1000 = 1.0f / 1000.0f, UI_INV_10 = 1.0f / 10.0f, UI_INV_4 = 1.0f / 4.0f, UI_FIFTH = 0.2f;

__device__ __forceinline__ float ui_weight(float w, bool far_px, int f) {
  if (far_px) w = ui_mul(w, UI_INV_1000);                 // :314
  if (f & UI_FLAG_SHORT) w = ui_mul(w, UI_INV_1000);      // :322
  if (f & UI_FLAG_NEWEST_I) w = ui_mul(w, UI_INV_10);     // :327
  if (f & UI_FLAG_NEWEST_J) w = ui_mul(w, UI_INV_4);      // :328
  return w;
}

// 2 * PIX consecutive values of an operator output as float32 (a float16 widens exactly)
template <int SRC>
__device__ __forceinline__ void ui_op_load4(const void *base, long long at, f32x4 &lo, f32x4 &hi) {
  if (SRC == UI_SRC_OP_F16) {
    const f16x8 v = *(const f16x8 *)((const _Float16 *)base + at);
#pragma unroll
    for (int k = 0; k < 4; k++) lo[k] = (float)v[k], hi[k] = (float)v[4 + k];
  } else {
    lo = *(const f32x4 *)((const float *)base + at), hi = *(const f32x4 *)((const float *)base + at + 4);
  }
}

template <int SRC>
__device__ __forceinline__ f32x2 ui_op_load1(const void *base, long long at) {
  if (SRC == UI_SRC_OP_F16) {
    const f16x2 v = *(const f16x2 *)((const _Float16 *)base + at);
    return f32x2{(float)v[0], (float)v[1]};
  }
  return *(const f32x2 *)((const float *)base + at);
}

// :235-236 for PIX pixels of active row ea: target = coords1 + delta.float() (one rounding), weight = weight.float(); both
// stored pixel-interleaved into the new tensors and handed back for the planar rows
template <int PIX, int SRC>
__device__ __forceinline__ void ui_op_row(const PayloadArgs &a, int ea, int p0, f32x4 &t0, f32x4 &t1, f32x4 &w0, f32x4 &w1) {
  const long long at = (long long)ea * 2 * a.HW + 2 * p0;
  if (PIX == 4) {
    const f32x4 c0 = *(const f32x4 *)(a.coords1 + at), c1 = *(const f32x4 *)(a.coords1 + at + 4);
    f32x4 d0, d1;
    ui_op_load4<SRC>(a.delta, at, d0, d1);
    ui_op_load4<SRC>(a.weight_op, at, w0, w1);
#pragma unroll
    for (int k = 0; k < 4; k++) t0[k] = ui_add(c0[k], d0[k]), t1[k] = ui_add(c1[k], d1[k]);
    *(f32x4 *)(a.target_new + at) = t0, *(f32x4 *)(a.target_new + at + 4) = t1;
    *(f32x4 *)(a.weight_new + at) = w0, *(f32x4 *)(a.weight_new + at + 4) = w1;
  } else {   // one pixel: its pair travels in the first two entries
    const f32x2 c = *(const f32x2 *)(a.coords1 + at);
    const f32x2 d = ui_op_load1<SRC>(a.delta, at), w = ui_op_load1<SRC>(a.weight_op, at);
    const f32x2 t = {ui_add(c[0], d[0]), ui_add(c[1], d[1])};
    *(f32x2 *)(a.target_new + at) = t, *(f32x2 *)(a.weight_new + at) = w;
    t0[0] = t[0], t0[1] = t[1], w0[0] = w[0], w0[1] = w[1];
  }
}

// PIX pixels per lane: 4 where ht * wd is a multiple of 4 (16-byte loads and stores throughout), else 1 (an odd map
// leaves every other edge row 8-byte aligned only).  SRC: where the active rows come from (UI_SRC_*)
template <int PIX, int SRC>
__global__ __launch_bounds__(UI_PAY_THREADS) void update_inputs_payload_kernel(PayloadArgs a) {
  const int HW = a.HW;
  const bool ok = a.res[1] == a.exp_n_sel && a.res[2] == a.exp_N && a.res[3] == a.exp_n_kx && a.res[8] == 0;
  if (!ok && blockIdx.x == 0 && threadIdx.x == 0)
    guard_report<3>(a.status, {a.res[1], a.res[2], a.res[3]}, {a.exp_n_sel, a.exp_N, a.exp_n_kx});
  const unsigned bid = blockIdx.x;
  const unsigned row = bid / (unsigned)a.chunks, chunk = bid - row * (unsigned)a.chunks;
  const int p0 = ((int)chunk * UI_PAY_THREADS + (int)threadIdx.x) * PIX;
  if (p0 >= HW) return;
  if (SRC != UI_SRC_GRAPH && (int)row >= a.exp_N + a.exp_n_kx) {
    // the new target / weight depend on no count: the active rows that outputs sized for other counts leave out
    const int ea = a.act_tail0 + ((int)row - a.exp_N - a.exp_n_kx);
    f32x4 t0, t1, w0, w1;
    if (ea < a.n_act) ui_op_row<PIX, SRC>(a, ea, p0, t0, t1, w0, w1);
    return;
  }
  if ((int)row >= a.exp_N) {  // a damping row
    const int r = (int)row - a.exp_N;
    if (r >= a.exp_n_kx) return;
    float *dst = a.damping_out + (long long)r * HW + p0;
    const int64_t fr = ok ? a.kx[r] : -1;
    if (PIX == 4) {
      f32x4 d = {a.ep, a.ep, a.ep, a.ep};
      if (fr >= 0 && fr < a.B) {
        d = *(const f32x4 *)(a.damping + fr * HW + p0);
#pragma unroll
        for (int k = 0; k < 4; k++) d[k] = ui_add(ui_mul(UI_FIFTH, d[k]), a.ep);
      }
      *(f32x4 *)dst = d;
    } else {
      *dst = (fr >= 0 && fr < a.B) ? ui_add(ui_mul(UI_FIFTH, a.damping[fr * HW + p0]), a.ep) : a.ep;
    }
    return;
  }
  const int e = (int)row;
  float *tx = a.target_out + (long long)e * 2 * HW + p0, *ty = tx + HW;
  float *wx = a.weight_out + (long long)e * 2 * HW + p0, *wy = wx + HW;
  // the edge's source row: inactive row sel[e] or active row e - n_sel
  const float *ts = nullptr, *ws = nullptr;
  // an active row of the operator's outputs: made and stored whatever the guard says, then kept in registers
  const bool op_row = SRC != UI_SRC_GRAPH && e >= a.exp_n_sel && e - a.exp_n_sel < a.n_act;
  f32x4 t0, t1, w0, w1;
  if (op_row) ui_op_row<PIX, SRC>(a, e - a.exp_n_sel, p0, t0, t1, w0, w1);
  if (ok) {
    if (e < a.exp_n_sel) {
      const int s = a.sel[e];
      if (s >= 0 && s < a.n_inac) ts = a.target_inac + (long long)s * 2 * HW, ws = a.weight_inac + (long long)s * 2 * HW;
    } else if (SRC == UI_SRC_GRAPH && e - a.exp_n_sel < a.n_act) {
      ts = a.target_act + (long long)(e - a.exp_n_sel) * 2 * HW, ws = a.weight_act + (long long)(e - a.exp_n_sel) * 2 * HW;
    }
  }
  if (!ts && !(ok && op_row)) {  // the guard: zero weights leave ba's state as it is
    if (PIX == 4) {
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      *(f32x4 *)tx = z, *(f32x4 *)ty = z, *(f32x4 *)wx = z, *(f32x4 *)wy = z;
    } else {
      *tx = 0.f, *ty = 0.f, *wx = 0.f, *wy = 0.f;
    }
    return;
  }
  const int f = a.flags[e];
  const int64_t i = a.ii_out[e];
  const bool far_on = a.far_rule && i >= 0 && i < a.B;
  if (PIX == 4) {
    if (!op_row) {
      t0 = *(const f32x4 *)(ts + 2 * p0), t1 = *(const f32x4 *)(ts + 2 * p0 + 4);
      w0 = *(const f32x4 *)(ws + 2 * p0), w1 = *(const f32x4 *)(ws + 2 * p0 + 4);
    }
    f32x4 d = {0.f, 0.f, 0.f, 0.f};
    if (far_on) d = *(const f32x4 *)(a.disps + i * HW + p0);
    const bool fp0 = far_on && d[0] < a.far_threshold, fp1 = far_on && d[1] < a.far_threshold;
    const bool fp2 = far_on && d[2] < a.far_threshold, fp3 = far_on && d[3] < a.far_threshold;
    const f32x4 ox = {t0[0], t0[2], t1[0], t1[2]}, oy = {t0[1], t0[3], t1[1], t1[3]};
    const f32x4 vx = {ui_weight(w0[0], fp0, f), ui_weight(w0[2], fp1, f), ui_weight(w1[0], fp2, f), ui_weight(w1[2], fp3, f)};
    const f32x4 vy = {ui_weight(w0[1], fp0, f), ui_weight(w0[3], fp1, f), ui_weight(w1[1], fp2, f), ui_weight(w1[3], fp3, f)};
    *(f32x4 *)tx = ox, *(f32x4 *)ty = oy, *(f32x4 *)wx = vx, *(f32x4 *)wy = vy;
  } else {
    f32x2 t, w;
    if (op_row) t = f32x2{t0[0], t0[1]}, w = f32x2{w0[0], w0[1]};
    else t = *(const f32x2 *)(ts + 2 * p0), w = *(const f32x2 *)(ws + 2 * p0);
    const bool fp = far_on && a.disps[i * HW + p0] < a.far_threshold;
    *tx = t[0], *ty = t[1];
    *wx = ui_weight(w[0], fp, f), *wy = ui_weight(w[1], fp, f);
  }
}

// a mismatch is reported through its words (size_guard.h): [1..3] the counts of the edge pass, [4..6] the counts the
// outputs were sized for
static SizeGuard ui_guard;

}  // namespace dba

using namespace dba;

extern "C" {

int dba_update_inputs_edges(const int64_t *ii_inac, const int64_t *jj_inac, int n_inac, const int64_t *ii_act,
                            const int64_t *jj_act, int n_act, const float *poses, int n_frames, int has_t0, int64_t t0,
                            int64_t inac_range, float mask_threshold, int baseline_rule, int *sel, int64_t *ii_out,
                            int64_t *jj_out, unsigned char *flags, int64_t *kx, int *res, dba_stream_t stream) {
  if (n_inac < 0 || n_act <= 0 || n_frames <= 0 || !ii_act || !jj_act || !ii_out || !jj_out || !flags || !kx || !res)
    return DBA_ERR_ARG;
  if (n_inac > 0 && (!ii_inac || !jj_inac || !sel)) return DBA_ERR_ARG;
  if (baseline_rule && !poses) return DBA_ERR_ARG;
  if (n_inac > DBA_SEL_MAX_EDGES || n_act > DBA_SEL_MAX_EDGES || n_frames > DBA_UI_MAX_FRAMES) return DBA_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(update_inputs_edge_kernel, dim3(1), dim3(UI_THREADS), 0, (hipStream_t)stream, ii_inac, jj_inac,
                     n_inac, ii_act, jj_act, n_act, poses, n_frames, has_t0 ? 1 : 0, t0, inac_range, mask_threshold,
                     baseline_rule ? 1 : 0, sel, ii_out, jj_out, flags, kx, res);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

// both payload entry points: src = UI_SRC_GRAPH reads (target_act, weight_act), UI_SRC_OP_* reads (coords1, delta, weight_op)
// and writes (target_new, weight_new)
static int payload_launch(int src, const float *target_inac, const float *weight_inac, int n_inac, const float *target_act,
                          const float *weight_act, const float *coords1, const void *delta, const void *weight_op, int n_act,
                          const float *disps, const float *damping, int n_frames, int ht, int wd, float far_threshold,
                          int far_rule, float ep, const int *sel, const int64_t *ii_out, const unsigned char *flags,
                          const int64_t *kx, const int *res, int exp_n_sel, int exp_N, int exp_n_kx, float *target_out,
                          float *weight_out, float *damping_out, float *target_new, float *weight_new, dba_stream_t stream) {
  if (n_inac < 0 || n_act <= 0 || n_frames <= 0 || ht <= 0 || wd <= 0 || (int64_t)ht * wd > (1 << 24)) return DBA_ERR_ARG;
  if (exp_n_sel < 0 || exp_n_sel > n_inac || exp_N < 0 || exp_N > n_inac + n_act || exp_n_kx < 0 ||
      exp_n_kx > n_frames || exp_n_kx > n_inac + n_act)
    return DBA_ERR_ARG;  // the edge pass's buffers hold n_inac + n_act edges and min(n_frames, that) frames
  const bool op = src != UI_SRC_GRAPH;
  if (op ? (!coords1 || !delta || !weight_op || !target_new || !weight_new) : (!target_act || !weight_act)) return DBA_ERR_ARG;
  if (!damping || !ii_out || !flags || !kx || !res) return DBA_ERR_ARG;
  if (n_inac > 0 && (!target_inac || !weight_inac || !sel)) return DBA_ERR_ARG;
  if (far_rule && !disps) return DBA_ERR_ARG;
  if ((exp_N > 0 && (!target_out || !weight_out)) || (exp_n_kx > 0 && !damping_out)) return DBA_ERR_ARG;
  if (n_inac > DBA_SEL_MAX_EDGES || n_act > DBA_SEL_MAX_EDGES || n_frames > DBA_UI_MAX_FRAMES) return DBA_ERR_UNSUPPORTED;
  PayloadArgs a{};
  if (const int rc = ui_guard.words(&a.status)) return rc;
  a.target_inac = target_inac, a.weight_inac = weight_inac, a.target_act = target_act, a.weight_act = weight_act;
  a.coords1 = coords1, a.delta = delta, a.weight_op = weight_op, a.target_new = target_new, a.weight_new = weight_new;
  a.disps = disps, a.damping = damping, a.sel = sel, a.res = res, a.ii_out = ii_out, a.kx = kx, a.flags = flags;
  a.target_out = target_out, a.weight_out = weight_out, a.damping_out = damping_out;
  a.n_inac = n_inac, a.n_act = n_act, a.B = n_frames, a.HW = ht * wd;
  a.exp_n_sel = exp_n_sel, a.exp_N = exp_N, a.exp_n_kx = exp_n_kx, a.far_rule = far_rule ? 1 : 0;
  a.far_threshold = far_threshold, a.ep = ep;
  // (operator source) the active rows behind the output rows [exp_n_sel, exp_N): none when the counts are the edge pass's
  a.act_tail0 = op ? (exp_N > exp_n_sel ? (exp_N - exp_n_sel < n_act ? exp_N - exp_n_sel : n_act) : 0) : n_act;
  const uint64_t rows = (uint64_t)exp_N + (uint64_t)exp_n_kx + (uint64_t)(n_act - a.act_tail0);
  if (rows == 0) return DBA_OK;
  const uintptr_t align = (uintptr_t)target_inac | (uintptr_t)weight_inac | (uintptr_t)target_act | (uintptr_t)weight_act |
                          (uintptr_t)disps | (uintptr_t)damping | (uintptr_t)target_out | (uintptr_t)weight_out |
                          (uintptr_t)damping_out | (uintptr_t)coords1 | (uintptr_t)target_new | (uintptr_t)weight_new;
  const uintptr_t align_op = (uintptr_t)delta | (uintptr_t)weight_op;   // a pixel's pair: 4 bytes in float16, 8 in float32
  if (align % 8 || align_op % (src == UI_SRC_OP_F16 ? 4 : 8)) return DBA_ERR_ARG;
  const bool wide = a.HW % 4 == 0 && align % 16 == 0 && align_op % 16 == 0;
  const int per_wg = UI_PAY_THREADS * (wide ? 4 : 1);
  a.chunks = (a.HW + per_wg - 1) / per_wg;
  const uint64_t wgs = rows * (uint64_t)a.chunks;
  if (wgs > (uint64_t)INT32_MAX) return DBA_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)wgs), block(UI_PAY_THREADS);
#define UI_LAUNCH(PIX, SRC) hipLaunchKernelGGL((update_inputs_payload_kernel<PIX, SRC>), grid, block, 0, (hipStream_t)stream, a)
  if (src == UI_SRC_GRAPH) {
    if (wide) UI_LAUNCH(4, UI_SRC_GRAPH); else UI_LAUNCH(1, UI_SRC_GRAPH);
  } else if (src == UI_SRC_OP_F32) {
    if (wide) UI_LAUNCH(4, UI_SRC_OP_F32); else UI_LAUNCH(1, UI_SRC_OP_F32);
  } else {
    if (wide) UI_LAUNCH(4, UI_SRC_OP_F16); else UI_LAUNCH(1, UI_SRC_OP_F16);
  }
#undef UI_LAUNCH
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

int dba_update_inputs_payload(const float *target_inac, const float *weight_inac, int n_inac, const float *target_act,
                              const float *weight_act, int n_act, const float *disps, const float *damping,
                              int n_frames, int ht, int wd, float far_threshold, int far_rule, float ep, const int *sel,
                              const int64_t *ii_out, const unsigned char *flags, const int64_t *kx, const int *res,
                              int exp_n_sel, int exp_N, int exp_n_kx, float *target_out, float *weight_out,
                              float *damping_out, dba_stream_t stream) {
  return payload_launch(UI_SRC_GRAPH, target_inac, weight_inac, n_inac, target_act, weight_act, nullptr, nullptr, nullptr, n_act,
                        disps, damping, n_frames, ht, wd, far_threshold, far_rule, ep, sel, ii_out, flags, kx, res, exp_n_sel,
                        exp_N, exp_n_kx, target_out, weight_out, damping_out, nullptr, nullptr, stream);
}

int dba_update_inputs_payload_op(const float *target_inac, const float *weight_inac, int n_inac, const float *coords1,
                                 const void *delta, const void *weight_op, int op_dtype, int n_act, const float *disps,
                                 const float *damping, int n_frames, int ht, int wd, float far_threshold, int far_rule,
                                 float ep, const int *sel, const int64_t *ii_out, const unsigned char *flags,
                                 const int64_t *kx, const int *res, int exp_n_sel, int exp_N, int exp_n_kx,
                                 float *target_out, float *weight_out, float *damping_out, float *target_new,
                                 float *weight_new, dba_stream_t stream) {
  if (op_dtype != DBA_F32 && op_dtype != DBA_F16) return DBA_ERR_UNSUPPORTED;
  return payload_launch(op_dtype == DBA_F16 ? UI_SRC_OP_F16 : UI_SRC_OP_F32, target_inac, weight_inac, n_inac, nullptr, nullptr,
                        coords1, delta, weight_op, n_act, disps, damping, n_frames, ht, wd, far_threshold, far_rule, ep, sel,
                        ii_out, flags, kx, res, exp_n_sel, exp_N, exp_n_kx, target_out, weight_out, damping_out, target_new,
                        weight_new, stream);
}

int dba_update_inputs_poll(int *counts6) { return ui_guard.poll(counts6, 6); }

}  // extern "C"
