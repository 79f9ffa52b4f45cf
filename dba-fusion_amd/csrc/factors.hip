// Retiring edges and dropping a keyframe on the device (dbaf/covisible_graph.py, dbaf/dbaf_frontend.py), gfx950:
//   dba_select_edges  <- the masks of CovisibleGraph.rm_factors (covisible_graph.py:152-176), rm_keyframe (:197-199,
//                        :207-210), the frontend's retirement rule (dbaf_frontend.py:235-239) and __rollup's edge
//                        statements (dbaf_frontend.py:106-118), with the compaction of ii, jj, age that follows them
//   dba_move_rows     <- every x[mask] / x[:, ~mask] / torch.cat of a payload (target, weight, net, inp and the inactive
//                        store) that one such call performs, in one launch
//   dba_shift_rows    <- rm_keyframe's buf[ix] = buf[ix+1] over the video buffers (covisible_graph.py:185-195)
// The reference runs these as boolean-index statements, each a nonzero with a host synchronisation of its own.  Here:
//   - selection: one workgroup of 1024 lanes walks the edge list a tile at a time.  A lane's slot among the dropped is
//     the dropped count of the tiles before plus its slot in the tile (flag_slot, edge_lists.h); its slot among the kept
//     is its position minus that.  Both sides therefore come out in the input's order, which is the order boolean
//     indexing gives.  No atomics.
//   - row mover: a job table passed by value in the kernel arguments; the grid is the concatenation of every job's
//     (row, chunk) pairs, a chunk being 1024 elements of the job's vector width (16 KB at 16 bytes), four loads in
//     flight per lane before the first store.  Pure streaming: no LDS, plain vector stores.  (The table, the
//     copy body and the check of a job are in row_jobs.h, which add_factors.hip shares.)
//   - row shift: the same body over a table of one-row jobs.
// Nothing synchronises the host; the selection leaves its counts and position lists in one small buffer.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "common.h"
#include "edge_lists.h"
#include "row_jobs.h"

namespace dba {

constexpr int SEL_THREADS = 1024;

__global__ __launch_bounds__(SEL_THREADS) void select_edges_kernel(
    const int64_t *__restrict__ ii, const int64_t *__restrict__ jj, const int64_t *__restrict__ age, int n, int mode,
    const unsigned char *__restrict__ mask, int64_t a, int64_t b, const int64_t *__restrict__ pre_ii,
    const int64_t *__restrict__ pre_jj, int n_pre, int64_t *__restrict__ keep, int64_t *__restrict__ drop,
    int *__restrict__ sel) {
  __shared__ int wdrop[SEL_THREADS / WAVE];
  const int tid = threadIdx.x;
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
    int total;
    const int q_drop = dropped + flag_slot<SEL_THREADS>(d, wdrop, &total);
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
    const int live = check_row_job(j, true, POS_OPTIONAL);
    if (live < 0) return live;
    if (!live) continue;
    if (!push_job(t, wgs, (const char *)j.src, (char *)j.dst, j.pos, j.row_bytes, j.count, j.dst_row0, j.src_rows))
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
