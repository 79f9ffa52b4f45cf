// Retiring edges and dropping a keyframe on the device (dbaf/covisible_graph.py, dbaf/dbaf_frontend.py), gfx950:
//   dba_select_edges  <- the masks of CovisibleGraph.rm_factors (covisible_graph.py:152-176), rm_keyframe (:197-199,
//                        :207-210), the frontend's retirement rule (dbaf_frontend.py:235-239) and __rollup's edge
//                        statements (dbaf_frontend.py:106-118), with the compaction of ii, jj, age that follows them
//   dba_move_rows     <- every x[mask] / x[:, ~mask] / torch.cat of a payload (target, weight, net, inp and the inactive
//                        store) that one such call performs, in one launch
//   dba_shift_rows    <- rm_keyframe's buf[ix] = buf[ix+1] over the video buffers (covisible_graph.py:185-195)
// The reference runs these as boolean-index statements, each a nonzero with a host synchronisation of its own.  Here:
//   - selection: one workgroup of 1024 lanes walks the edge list a tile at a time.  Each wave ballots its drop flags;
//     a lane's slot among the dropped is the dropped count of the tiles before, of the waves before (LDS) and of the
//     lanes before (popcount of the ballot below the lane); its slot among the kept is its position minus that.  Both
//     sides therefore come out in the input's order, which is the order boolean indexing gives.  No atomics.
//   - row mover: a job table passed by value in the kernel arguments; the grid is the concatenation of every job's
//     (row, chunk) pairs, a chunk being 1024 elements of the job's vector width (16 KB at 16 bytes), four loads in
//     flight per lane before the first store.  Pure streaming: no LDS, plain vector stores.  (The table and the
//     copy body are in row_jobs.h, which add_factors.hip shares.)
//   - row shift: the same body over a table of one-row jobs.
// Nothing synchronises the host; the selection leaves its counts and position lists in one small buffer.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "common.h"
#include "row_jobs.h"

namespace dba {

constexpr int SEL_THREADS = 1024;

__global__ __launch_bounds__(SEL_THREADS) void select_edges_kernel(
    const int64_t *__restrict__ ii, const int64_t *__restrict__ jj, const int64_t *__restrict__ age, int n, int mode,
    const unsigned char *__restrict__ mask, int64_t a, int64_t b, const int64_t *__restrict__ pre_ii,
    const int64_t *__restrict__ pre_jj, int n_pre, int64_t *__restrict__ keep, int64_t *__restrict__ drop,
    int *__restrict__ sel) {
  __shared__ int wdrop[SEL_THREADS / WAVE];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid >> 6;
  int64_t *kii = keep, *kjj = keep + n, *kage = keep + 2 * (int64_t)n;
  int64_t *dii = drop, *djj = drop + (n_pre + n);
  int *keep_pos = sel + 2, *drop_pos = sel + 2 + n;
  for (int p = tid; p < n_pre; p += SEL_THREADS) { dii[p] = pre_ii[p]; djj[p] = pre_jj[p]; }
  int dropped = 0;  // in the tiles before this one
  for (int start = 0; start < n; start += SEL_THREADS) {
    const int p = start + tid;
    const bool in = p < n;
    int64_t i = 0, j = 0, g = 0;
    bool d = false;
    if (in) {
      i = ii[p];
      j = jj[p];
      if (age) g = age[p];
      switch (mode) {
        case DBA_SEL_MASK: d = mask[p] != 0; break;
        case DBA_SEL_RULE_OR: d = (g > a) || (i < b || j < b); break;
        case DBA_SEL_RULE_AND: d = (g > a) && (i < b || j < b); break;
        case DBA_SEL_KEYFRAME:
          d = i == a || j == a;
          if (i >= a) i -= 1;
          if (j >= a) j -= 1;
          break;
        case DBA_SEL_ROLL:
          i -= a;
          j -= a;
          d = i < 0 || j < 0;
          break;
        default:  // DBA_SEL_SHIFT
          i -= a;
          j -= a;
          break;
      }
    }
    const uint64_t m = __ballot(d);
    if (lane == 0) wdrop[wv] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < SEL_THREADS / WAVE; w++) {
      const int s = wdrop[w];
      if (w < wv) before += s;
      total += s;
    }
    __syncthreads();
    const int q_drop = dropped + before + __popcll(m & ((1ull << lane) - 1ull));
    if (in) {
      if (d) {
        dii[n_pre + q_drop] = i;
        djj[n_pre + q_drop] = j;
        drop_pos[q_drop] = p;
      } else {
        const int q = p - q_drop;
        kii[q] = i;
        kjj[q] = j;
        if (age) kage[q] = g;
        keep_pos[q] = p;
      }
    }
    dropped += total;
  }
  if (tid == 0) {
    sel[0] = n - dropped;
    sel[1] = dropped;
  }
}

__global__ __launch_bounds__(MOVE_THREADS) void row_mover_kernel(RowTable<DBA_MAX_ROW_JOBS> t) { run_row_jobs(t); }

__global__ __launch_bounds__(MOVE_THREADS) void row_shift_kernel(RowTable<DBA_MAX_SHIFT_BUFS> t) { run_row_jobs(t); }

}  // namespace dba

using namespace dba;

extern "C" {

int dba_select_edges(const int64_t *ii, const int64_t *jj, const int64_t *age, int n, int mode,
                     const unsigned char *mask, int64_t a, int64_t b, const int64_t *pre_ii, const int64_t *pre_jj,
                     int n_pre, int64_t *keep, int64_t *drop, int *sel, dba_stream_t stream) {
  if (n < 0 || n_pre < 0 || mode < DBA_SEL_MASK || mode > DBA_SEL_SHIFT || !sel) return DBA_ERR_ARG;
  if (n > DBA_SEL_MAX_EDGES) return DBA_ERR_UNSUPPORTED;
  if (n > 0 && (!ii || !jj || !keep || !drop)) return DBA_ERR_ARG;
  if (n > 0 && mode == DBA_SEL_MASK && !mask) return DBA_ERR_ARG;
  if (n > 0 && (mode == DBA_SEL_RULE_OR || mode == DBA_SEL_RULE_AND) && !age) return DBA_ERR_ARG;
  if (n_pre > 0 && (!pre_ii || !pre_jj || !drop)) return DBA_ERR_ARG;
  hipLaunchKernelGGL(select_edges_kernel, dim3(1), dim3(SEL_THREADS), 0, (hipStream_t)stream, ii, jj, age, n, mode,
                     mask, a, b, pre_ii, pre_jj, n_pre, keep, drop, sel);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

int dba_move_rows(const dba_row_job *jobs, int n_jobs, dba_stream_t stream) {
  if (n_jobs < 0 || n_jobs > DBA_MAX_ROW_JOBS || (n_jobs > 0 && !jobs)) return DBA_ERR_ARG;
  RowTable<DBA_MAX_ROW_JOBS> t{};
  uint64_t wgs = 0;
  for (int k = 0; k < n_jobs; k++) {
    const dba_row_job &j = jobs[k];
    if (j.count < 0 || j.row_bytes < 0 || j.dst_row0 < 0 || j.src_rows < 0 || j.dst_rows < 0) return DBA_ERR_ARG;
    if ((int64_t)j.dst_row0 + j.count > j.dst_rows) return DBA_ERR_ARG;
    if (!j.pos && j.count > j.src_rows) return DBA_ERR_ARG;
    if (j.count == 0 || j.row_bytes == 0) continue;
    if (!j.src || !j.dst) return DBA_ERR_ARG;
    const char *s0 = (const char *)j.src, *s1 = s0 + (int64_t)j.src_rows * j.row_bytes;
    const char *d0 = (const char *)j.dst + (int64_t)j.dst_row0 * j.row_bytes, *d1 = d0 + (int64_t)j.count * j.row_bytes;
    if (s0 < d1 && d0 < s1) return DBA_ERR_ARG;  // the rows read and the rows written overlap
    if (!push_job(t, wgs, s0, (char *)j.dst, j.pos, j.row_bytes, j.count, j.dst_row0, j.src_rows))
      return DBA_ERR_UNSUPPORTED;
  }
  if (t.n == 0) return DBA_OK;
  hipLaunchKernelGGL(row_mover_kernel, dim3((unsigned)wgs), dim3(MOVE_THREADS), 0, (hipStream_t)stream, t);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

int dba_shift_rows(void *const *bases, const int64_t *row_bytes, const int64_t *rows, int n_bufs, int64_t ix,
                   dba_stream_t stream) {
  if (n_bufs < 0 || n_bufs > DBA_MAX_SHIFT_BUFS || (n_bufs > 0 && (!bases || !row_bytes || !rows))) return DBA_ERR_ARG;
  RowTable<DBA_MAX_SHIFT_BUFS> t{};
  uint64_t wgs = 0;
  for (int k = 0; k < n_bufs; k++) {
    if (row_bytes[k] < 0 || ix < 0 || ix + 1 >= rows[k]) return DBA_ERR_ARG;
    if (row_bytes[k] == 0) continue;
    if (!bases[k]) return DBA_ERR_ARG;
    char *d = (char *)bases[k] + ix * row_bytes[k];
    if (!push_job(t, wgs, d + row_bytes[k], d, nullptr, row_bytes[k], 1, 0, 1)) return DBA_ERR_UNSUPPORTED;
  }
  if (t.n == 0) return DBA_OK;
  hipLaunchKernelGGL(row_shift_kernel, dim3((unsigned)wgs), dim3(MOVE_THREADS), 0, (hipStream_t)stream, t);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

}  // extern "C"
