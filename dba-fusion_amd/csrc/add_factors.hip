// Adding edges on the device (CovisibleGraph.add_factors, dbaf/covisible_graph.py:102-149), gfx950:
//   dba_add_factors_plan     <- __filter_repeated_edges (:61-72, :112), the eviction mask `argsort(age) >= max_factors -
//                               n_new` with the index statements of rm_factors(store=True) (:118-122, :157-165), the
//                               torch.cat of ii, jj, age (:141-143) and the index arithmetic of the gathers (:124-134)
//   dba_add_factors_payload  <- every payload statement of the call: the kept rows of net, inp, target, weight and the
//                               appended inactive store (rm_factors, :159-160, :170-176), the gathers nets[ii], inps[ii],
//                               fmaps[ii,0], fmaps[jj,c] (:124-134), video.reproject(ii, jj) (:138), zeros_like (:139)
//                               and the torch.cat that follow (:135, :146-149), in one launch
// The plan is one workgroup of 1024 lanes (the filter and the compaction are edge_lists.h's):
//   - filter: a lane holds up to 8 proposals in registers and strikes those in the active or the inactive list; the
//     survivors are numbered in order (duplicates inside the proposal stay);
//   - eviction: edge e's stable rank r(e) = #{f: age[f] < age[e]} + #{f < e: age[f] == age[e]} is argsort's inverse
//     (ties to the lower position), so position r(e) of the mask is `e >= limit`; the mask goes to LDS and is compacted
//     as dba_select_edges compacts its mask: both sides in the input's order;
//   - every kept proposal is range-checked against the video's rows BEFORE anything dereferences it: the verdict is in
//     the block the host reads, and a gather position that failed the check is written as -1, which the payload launch
//     skips.
// The payload launch is the row mover's grid (row_jobs.h) over up to 16 copy / gather / zero jobs, followed by the
// workgroups of one reprojection job, whose pixels go through reproj.h exactly as reproject_kernel's do (same bits).
// No atomics, no inter-workgroup communication, nothing synchronises the host.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "common.h"
#include "edge_lists.h"
#include "reproj.h"
#include "row_jobs.h"

namespace dba {

constexpr int AF_THREADS = 1024;
constexpr int AF_PER = DBA_SEL_MAX_EDGES / AF_THREADS;  // list entries per lane

__global__ __launch_bounds__(AF_THREADS) void add_factors_plan_kernel(
    const int64_t *__restrict__ ii, const int64_t *__restrict__ jj, const int64_t *__restrict__ age, int n,
    const int64_t *__restrict__ ii_inac, const int64_t *__restrict__ jj_inac, int m, const int64_t *__restrict__ pii,
    const int64_t *__restrict__ pjj, int p, int max_factors, int may_evict, int n_frames, int cams,
    int64_t *__restrict__ lists, int64_t *__restrict__ inac, int *__restrict__ info) {
  __shared__ int64_t sx[2][AF_THREADS];
  __shared__ unsigned char dflag[DBA_SEL_MAX_EDGES];
  __shared__ int wcount[AF_THREADS / WAVE];
  __shared__ int s_bad;
  const int tid = threadIdx.x;
  if (tid == 0) s_bad = 0;

  // ---- :61-72: the proposals that are in neither list --------------------------------------------------------------
  const int p_tiles = (p + AF_THREADS - 1) / AF_THREADS;
  int64_t a[AF_PER], b[AF_PER];
  bool fresh[AF_PER];
#pragma unroll
  for (int t = 0; t < AF_PER; t++) {
    const int k = t * AF_THREADS + tid;
    fresh[t] = k < p;
    a[t] = fresh[t] ? pii[k] : 0;
    b[t] = fresh[t] ? pjj[k] : 0;
  }
  strike_listed<AF_THREADS>(ii, jj, n, a, b, fresh, p_tiles, sx);
  strike_listed<AF_THREADS>(ii_inac, jj_inac, m, a, b, fresh, p_tiles, sx);
  int q_new[AF_PER];
  int n_new = 0;
#pragma unroll
  for (int t = 0; t < AF_PER; t++) {
    q_new[t] = 0;
    if (t >= p_tiles) continue;
    int tot;
    q_new[t] = n_new + flag_slot<AF_THREADS>(fresh[t], wcount, &tot);
    n_new += tot;
  }

  // ---- :118-122 with :157-165: the eviction mask over positions and both sides of it ----------------------------------
  const int cap = n + p;
  int64_t *out_ii = lists, *out_jj = lists + cap, *out_age = lists + 2 * (int64_t)cap;
  int *keep_pos = info + DBA_AF_INFO_WORDS, *drop_pos = keep_pos + n;
  const bool evict = n_new > 0 && may_evict && max_factors > 0 && (int64_t)n + n_new > max_factors;
  const int n_tiles = (n + AF_THREADS - 1) / AF_THREADS;
  int n_drop = 0;
  if (evict) {
    const int64_t limit = (int64_t)max_factors - n_new;  // may be negative: everything goes
    int64_t g[AF_PER];
    int rank[AF_PER];
#pragma unroll
    for (int t = 0; t < AF_PER; t++) {
      const int e = t * AF_THREADS + tid;
      g[t] = e < n ? age[e] : 0;
      rank[t] = 0;
    }
    for (int f0 = 0; f0 < n; f0 += AF_THREADS) {
      const int nf = min(n - f0, AF_THREADS);
      __syncthreads();
      if (tid < nf) sx[0][tid] = age[f0 + tid];
      __syncthreads();
#pragma unroll
      for (int t = 0; t < AF_PER; t++) {
        if (t >= n_tiles) break;
        const int e = t * AF_THREADS + tid;
        if (e < n)
          for (int f = 0; f < nf; f++) {
            const int64_t gf = sx[0][f];
            rank[t] += (gf < g[t] || (gf == g[t] && f0 + f < e)) ? 1 : 0;
          }
      }
    }
#pragma unroll
    for (int t = 0; t < AF_PER; t++) {
      const int e = t * AF_THREADS + tid;
      if (e < n) dflag[rank[t]] = (int64_t)e >= limit;  // the ranks are a permutation of [0, n): every slot once
    }
    for (int k = tid; k < m; k += AF_THREADS) { inac[k] = ii_inac[k]; inac[(int64_t)(m + n) + k] = jj_inac[k]; }
    __syncthreads();
    int64_t *d_ii = inac + m, *d_jj = inac + (int64_t)(m + n) + m;
    for (int t = 0; t < n_tiles; t++) {
      const int k = t * AF_THREADS + tid;
      const bool in = k < n;
      const bool d = in && dflag[k] != 0;
      int tot;
      const int qd = n_drop + flag_slot<AF_THREADS>(d, wcount, &tot);
      if (in) {
        const int64_t i = ii[k], j = jj[k];
        if (d) {
          d_ii[qd] = i;
          d_jj[qd] = j;
          drop_pos[qd] = k;
        } else {
          const int q = k - qd;
          out_ii[q] = i;
          out_jj[q] = j;
          out_age[q] = age[k];
          keep_pos[q] = k;
        }
      }
      n_drop += tot;
    }
  } else {
    for (int k = tid; k < n; k += AF_THREADS) {
      out_ii[k] = ii[k];
      out_jj[k] = jj[k];
      out_age[k] = age[k];
      keep_pos[k] = k;
    }
  }
  const int n_keep = n - n_drop;

  // ---- :141-143 and the source rows of :124-134, range-checked --------------------------------------------------------
  int *row_net = drop_pos + n, *row_f1 = row_net + p, *row_f2 = row_f1 + p;
#pragma unroll
  for (int t = 0; t < AF_PER; t++) {
    if (t >= p_tiles) break;
    if (!fresh[t]) continue;
    const int q = q_new[t];
    const int64_t i = a[t], j = b[t];
    out_ii[n_keep + q] = i;
    out_jj[n_keep + q] = j;
    out_age[n_keep + q] = 0;
    const bool in_range = i >= 0 && i < n_frames && j >= 0 && j < n_frames;
    const bool ok = in_range && (i != j || cams >= 2);  // fmaps[jj, 1] needs the second camera's map
    row_net[q] = ok ? (int)i : -1;
    row_f1[q] = ok ? (int)i * cams : -1;
    row_f2[q] = ok ? (int)j * cams + (i == j ? 1 : 0) : -1;
    if (!in_range) s_bad = DBA_AF_BAD_RANGE;  // (lanes that write store one of two non-zero verdicts)
    else if (!ok) s_bad = DBA_AF_BAD_STEREO;
  }
  __syncthreads();
  if (tid == 0) {
    info[0] = n_new;
    info[1] = n_keep;
    info[2] = n_drop;
    info[3] = s_bad;
    info[4] = evict ? 1 : 0;
  }
}

struct ReprojJob {
  const float *poses, *disps, *intr;
  const int64_t *ii, *jj;
  float2 *coords;
  int count, HW, wd, n_frames;
  unsigned wg_start, chunks;  // first workgroup of the job; workgroups per edge
};

__global__ __launch_bounds__(MOVE_THREADS) void add_factors_payload_kernel(RowTable<DBA_AF_MAX_JOBS> t, ReprojJob rp) {
  if (blockIdx.x < rp.wg_start) {
    run_row_jobs<DBA_AF_MAX_JOBS, true>(t);
    return;
  }
  const unsigned local = blockIdx.x - rp.wg_start;
  const int e = (int)(local / rp.chunks);
  const int k = (int)(local - (unsigned)e * rp.chunks) * MOVE_THREADS + (int)threadIdx.x;
  if (e >= rp.count || k >= rp.HW) return;
  const int64_t i64 = rp.ii[e], j64 = rp.jj[e];
  if (i64 < 0 || i64 >= rp.n_frames || j64 < 0 || j64 >= rp.n_frames) return;  // (the host raised on the plan's verdict)
  const int ix = (int)i64, jx = (int)j64;
  const EdgeGeom G = edge_geom(rp.poses, rp.intr, ix, jx);
  const float u = (float)(k % rp.wd), v = (float)(k / rp.wd);
  float ok;
  rp.coords[(size_t)e * rp.HW + k] = reproject_pixel(G, u, v, rp.disps[(size_t)ix * rp.HW + k], ok);
}

}  // namespace dba

using namespace dba;

extern "C" {

int dba_add_factors_plan(const int64_t *ii, const int64_t *jj, const int64_t *age, int n, const int64_t *ii_inac,
                         const int64_t *jj_inac, int n_inac, const int64_t *prop_ii, const int64_t *prop_jj, int n_prop,
                         int max_factors, int may_evict, int n_frames, int cams, int64_t *lists, int64_t *inac,
                         int *info, dba_stream_t stream) {
  if (n < 0 || n_inac < 0 || n_prop < 0 || n_frames < 0 || cams < 1 || !info) return DBA_ERR_ARG;
  if (n > DBA_SEL_MAX_EDGES || n_inac > DBA_SEL_MAX_EDGES || n_prop > DBA_SEL_MAX_EDGES) return DBA_ERR_UNSUPPORTED;
  if ((int64_t)n_frames * cams > INT32_MAX) return DBA_ERR_UNSUPPORTED;
  if (n > 0 && (!ii || !jj || !age)) return DBA_ERR_ARG;
  if (n_inac > 0 && (!ii_inac || !jj_inac)) return DBA_ERR_ARG;
  if (n_prop > 0 && (!prop_ii || !prop_jj)) return DBA_ERR_ARG;
  if (n + n_prop > 0 && !lists) return DBA_ERR_ARG;
  if (may_evict && n_inac + n > 0 && !inac) return DBA_ERR_ARG;
  hipLaunchKernelGGL(add_factors_plan_kernel, dim3(1), dim3(AF_THREADS), 0, (hipStream_t)stream, ii, jj, age, n,
                     ii_inac, jj_inac, n_inac, prop_ii, prop_jj, n_prop, max_factors, may_evict ? 1 : 0, n_frames, cams,
                     lists, inac, info);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

int dba_add_factors_payload(const dba_af_job *jobs, int n_jobs, const dba_af_geometry *geom, dba_stream_t stream) {
  if (n_jobs < 0 || n_jobs > DBA_AF_MAX_JOBS + 1 || (n_jobs > 0 && !jobs)) return DBA_ERR_ARG;
  RowTable<DBA_AF_MAX_JOBS> t{};
  ReprojJob rp{};
  uint64_t wgs = 0;
  const dba_af_job *reproject = nullptr;
  for (int k = 0; k < n_jobs; k++) {
    const dba_af_job &a = jobs[k];
    const dba_row_job &j = a.rows;
    if (a.kind < DBA_AF_COPY || a.kind > DBA_AF_REPROJECT) return DBA_ERR_ARG;
    if (a.kind == DBA_AF_REPROJECT) {
      if (!row_range_ok(j) || reproject) return DBA_ERR_ARG;  // one per call
      reproject = &a;
      continue;
    }
    const bool reads = a.kind != DBA_AF_ZERO;
    const int live = check_row_job(j, reads, a.kind == DBA_AF_COPY ? POS_FORBIDDEN : POS_REQUIRED);
    if (live < 0) return live;
    if (!live) continue;
    if (t.n == DBA_AF_MAX_JOBS) return DBA_ERR_ARG;
    if (!push_job(t, wgs, reads ? (const char *)j.src : nullptr, (char *)j.dst, a.kind == DBA_AF_GATHER ? j.pos : nullptr,
                  j.row_bytes, j.count, j.dst_row0, j.src_rows))
      return DBA_ERR_UNSUPPORTED;
  }
  rp.wg_start = (unsigned)wgs;
  rp.chunks = 1;
  if (reproject && reproject->rows.count > 0) {
    const dba_row_job &j = reproject->rows;
    if (!geom || !geom->poses || !geom->disps || !geom->intrinsics_b4 || !geom->ii || !geom->jj || !j.dst)
      return DBA_ERR_ARG;
    if (geom->ht <= 0 || geom->wd <= 0 || geom->n_frames <= 0 || (int64_t)geom->ht * geom->wd > INT32_MAX / 8)
      return DBA_ERR_ARG;
    const int HW = geom->ht * geom->wd;
    if (j.row_bytes != (int64_t)HW * 8 || ((uintptr_t)j.dst & 7u)) return DBA_ERR_ARG;  // rows of [ht, wd, 2] float32
    rp.poses = geom->poses;
    rp.disps = geom->disps;
    rp.intr = geom->intrinsics_b4;
    rp.ii = geom->ii;
    rp.jj = geom->jj;
    rp.coords = reinterpret_cast<float2 *>(j.dst) + (int64_t)j.dst_row0 * HW;
    rp.count = j.count;
    rp.HW = HW;
    rp.wd = geom->wd;
    rp.n_frames = geom->n_frames;
    rp.chunks = (unsigned)((HW + MOVE_THREADS - 1) / MOVE_THREADS);
    wgs += (uint64_t)rp.chunks * (uint64_t)j.count;
    if (wgs > (uint64_t)INT32_MAX) return DBA_ERR_UNSUPPORTED;
  }
  if (wgs == 0) return DBA_OK;
  hipLaunchKernelGGL(add_factors_payload_kernel, dim3((unsigned)wgs), dim3(MOVE_THREADS), 0, (hipStream_t)stream, t, rp);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

}  // extern "C"
