// Edge management of the covisibility graph on the device (dbaf/covisible_graph.py, dbaf/depth_video.py), gfx950:
//   dba_frame_distance_bidir   <- DepthVideo.distance, bidirectional (depth_video.py:240-270): two frame_distance
//                                 calls, (ii,jj) and (jj,ii), and .5 * (d1 + d2), in one launch
//   dba_proximity_edges        <- CovisibleGraph.add_proximity_factors (covisible_graph.py:357-441): the edge list it
//                                 hands to add_factors, in the same order
//   dba_filter_repeated_edges  <- CovisibleGraph.__filter_repeated_edges (covisible_graph.py:61-72)
// The reference runs these as Python loops over device tensors: one launch per element write and one host sync per
// candidate.  Here:
//   - distances: one workgroup of 512 lanes per pair; lanes 0-255 compute (i,j), lanes 256-511 (j,i), each with the
//     per-pair body of frame_distance_kernel (frame_distance.h), so the result is bit-identical to two
//     dba_frame_distance calls averaged in float;
//   - selection: one workgroup of 1024 lanes.  The candidate distances sit in LDS; the suppression of steps 3-4 writes
//     +inf there in parallel (every write stores the same value, so their order does not matter); the candidates that
//     can ever be taken (not > thresh: d <= thresh or NaN) are compacted in index order and bitonic-sorted by
//     (distance, index), which is torch.argsort's order with ties broken by the lower index.  Wave 0 then walks the
//     sorted list 64 candidates at a time: a ballot finds the first one whose CURRENT distance is still takeable, it is
//     appended and its neighbourhood suppressed, and the walk resumes after it;
//   - the repeated-edge filter: one workgroup, one proposal per lane a tile at a time, through the filter and the
//     order-preserving compaction of edge_lists.h.
// No atomics anywhere: every result is bit-identical run to run.  Nothing synchronises the host; each call writes its
// edge count to a caller-provided device word.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>
#include <stdint.h>

#include "common.h"
#include "edge_lists.h"
#include "frame_distance.h"

namespace dba {

constexpr int PROX_MAX_CAND = 8192;  // (t-t0)(t-t1) + skip extras; the reference's --buffer 80 at t0 = t1 = 0 is 6400
constexpr int PROX_MAX_SKIP = 16;
constexpr int PROX_THREADS = 1024;
constexpr unsigned short PROX_PAD = 0xffff;

// the candidate list of add_proximity_factors: meshgrid(arange(t0,t), arange(t1,t)) row-major (:361-366), then the
// skip extras (t-1, t0+s) for the s of skip_edge with t0+s > 0 (:371-377)
struct ProxGrid {
  int t, t0, t1, cc, n_extra;
  int extra_jj[PROX_MAX_SKIP];
};

__device__ __forceinline__ void prox_pair(const ProxGrid &g, int k, int &i, int &j) {
  const int W = g.t - g.t1;
  if (k < g.cc) {
    i = g.t0 + k / W;
    j = g.t1 + k % W;
  } else {
    i = g.t - 1;
    j = g.extra_jj[k - g.cc];
  }
}

// .5 * (frame_distance(i,j) + frame_distance(j,i)) by a 512-lane workgroup; NaN for a pair outside [0, n_frames)
__device__ __forceinline__ float bidir_distance(const float *poses, const float *disps, const float *intr, int64_t i,
                                                int64_t j, int n_frames, int HW, int wd, float beta) {
  __shared__ float red[2][3][4];
  const int dir = threadIdx.x >> 8, tid = threadIdx.x & 255;
  const bool ok = i >= 0 && i < n_frames && j >= 0 && j < n_frames;  // uniform over the workgroup
  if (ok) frame_distance_partials(poses, disps, intr, dir ? (int)j : (int)i, dir ? (int)i : (int)j, HW, wd, beta, tid,
                                  256, red[dir]);
  __syncthreads();
  if (!ok) return __int_as_float(0x7fc00000);
  const float d1 = frame_distance_finish(red[0]), d2 = frame_distance_finish(red[1]);
  return 0.5f * (d1 + d2);  // depth_video.py:261, float32
}

__global__ __launch_bounds__(512) void frame_distance_bidir_kernel(const float *__restrict__ poses,
                                                                   const float *__restrict__ disps,
                                                                   const float *__restrict__ intr,
                                                                   const int64_t *__restrict__ ii,
                                                                   const int64_t *__restrict__ jj, int n_frames, int HW,
                                                                   int wd, float beta, float *__restrict__ dist) {
  const int n = blockIdx.x;
  const float d = bidir_distance(poses, disps, intr, ii[n], jj[n], n_frames, HW, wd, beta);
  if (threadIdx.x == 0) dist[n] = d;
}

// the candidates' distances with step 2 applied (:380-381): inf where ii - rad < jj (not computed), inf where d > 100
__global__ __launch_bounds__(512) void proximity_distance_kernel(const float *__restrict__ poses,
                                                                 const float *__restrict__ disps,
                                                                 const float *__restrict__ intr, ProxGrid g, int rad,
                                                                 int HW, int wd, float beta, float *__restrict__ dist) {
  const int k = blockIdx.x;
  int i, j;
  prox_pair(g, k, i, j);
  float d = INFINITY;
  if (!(i - rad < j)) {
    d = bidir_distance(poses, disps, intr, i, j, g.t, HW, wd, beta);
    if (d > 100.f) d = INFINITY;
  }
  if (threadIdx.x == 0) dist[k] = d;
}

// :386-393 / :425-432: +inf on the flat index of every (i+di, j+dj) inside the grid with |di|+|dj| <= r,
// r = max(min(|i-j|-2, nms), 0), di, dj in [-nms, nms] (an empty range when nms < 0).  Lanes `lane`, `lane + lanes`,
// ... of the caller take the cells.
__device__ __forceinline__ void suppress(float *dw, int64_t i, int64_t j, int nms, int t0, int t1, int t, int lane,
                                         int lanes) {
  if (nms < 0) return;
  const int64_t dij = i > j ? i - j : j - i;
  const int r = (int)max(min(dij - 2, (int64_t)nms), (int64_t)0);
  const int side = 2 * r + 1, W = t - t1;
  for (int c = lane; c < side * side; c += lanes) {
    const int di = c / side - r, dj = c % side - r;
    if (abs(di) + abs(dj) > r) continue;
    const int64_t i1 = i + di, j1 = j + dj;
    if (t0 <= i1 && i1 < t && t1 <= j1 && j1 < t) dw[(int)(i1 - t0) * W + (int)(j1 - t1)] = INFINITY;
  }
}

// exclusive prefix sum of v over the workgroup (all lanes call it); *total = the sum
__device__ __forceinline__ int block_exclusive_scan(int v, int *wsum, int *total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
  int x = v;
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) wsum[wv] = x;
  __syncthreads();
  int base = 0, tot = 0;
  for (int w = 0; w < nw; w++) {
    const int s = wsum[w];
    if (w < wv) base += s;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return base + x - v;
}

// torch.argsort's ascending order as a total order: -0 == +0, NaN after +inf, ties by the lower index
__device__ __forceinline__ uint64_t sort_key(const float *dw, unsigned short k) {
  if (k == PROX_PAD) return ~0ull;
  const float v = dw[k];
  uint32_t b = __float_as_uint(v == 0.f ? 0.f : v);
  if (v != v) b = 0xffffffffu;
  else b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return ((uint64_t)b << 32) | k;
}

__global__ __launch_bounds__(PROX_THREADS) void proximity_select_kernel(
    const float *__restrict__ dist, ProxGrid g, int rad, int nms, double thresh, int max_factors, int stereo,
    const int64_t *__restrict__ ex_ii, const int64_t *__restrict__ ex_jj, int n_ex, int64_t *__restrict__ out_ii,
    int64_t *__restrict__ out_jj, int capacity, int *__restrict__ count) {
  __shared__ float dw[PROX_MAX_CAND];
  __shared__ unsigned short order[PROX_MAX_CAND];
  __shared__ int wsum[PROX_THREADS / 64];
  __shared__ int s_len, s_err;
  const int tid = threadIdx.x;
  const int t = g.t, t0 = g.t0, t1 = g.t1, W = t - t1, R = t - t0, cc = g.cc, L = cc + g.n_extra;
  for (int k = tid; k < L; k += PROX_THREADS) dw[k] = dist[k];
  if (tid == 0) {
    // step 4's edge list (:395-405), in the reference's order: (i,i) when stereo, then (i,j), (j,i) for each j
    int len = 0, err = 0;
    for (int i = t0; i < t; i++) {
      const int jlo = max(i - rad - 1, 0);
      const int n_i = (stereo ? 1 : 0) + 2 * max(i - jlo, 0);
      if (len + n_i > capacity) { err = 1; break; }
      if (stereo) { out_ii[len] = i; out_jj[len] = i; len++; }
      for (int j = jlo; j < i; j++) {
        out_ii[len] = i; out_jj[len] = j;
        out_ii[len + 1] = j; out_jj[len + 1] = i;
        len += 2;
      }
    }
    s_len = len;
    s_err = err;
  }
  __syncthreads();
  // step 3 (:383-393): around the active, bad and inactive edges
  for (int e = tid; e < n_ex; e += PROX_THREADS) suppress(dw, ex_ii[e], ex_jj[e], nms, t0, t1, t, 0, 1);
  // step 4's writes (:399, :404-405): the stereo index is a Python index (negative counts from the end of d); the
  // neighbour index is written whenever it is >= 0, even for j < t1, where it lands in the previous row
  for (int r = tid; r < R; r += PROX_THREADS) {
    const int i = t0 + r;
    if (stereo) {
      int idx = r * W + (i - t1);
      if (idx < 0) idx += L;
      if (idx < 0) s_err = 2;  // the reference raises IndexError here
      else dw[idx] = INFINITY;
    }
    for (int j = max(i - rad - 1, 0); j < i; j++) {
      const int idx = r * W + (j - t1);
      if (idx >= 0) dw[idx] = INFINITY;
    }
  }
  __syncthreads();
  // compaction, in index order, of the grid candidates not > thresh (the only ones the greedy pass can take: a
  // candidate's current value is its value here or +inf)
  const int per = (cc + PROX_THREADS - 1) / PROX_THREADS;
  const int k0 = min(tid * per, cc), k1 = min(k0 + per, cc);
  int mine = 0;
  for (int k = k0; k < k1; k++) mine += !((double)dw[k] > thresh);
  int n_take;
  int pos = block_exclusive_scan(mine, wsum, &n_take);
  for (int k = k0; k < k1; k++)
    if (!((double)dw[k] > thresh)) order[pos++] = (unsigned short)k;
  int P = 1;
  while (P < n_take) P <<= 1;
  for (int p = n_take + tid; p < P; p += PROX_THREADS) order[p] = PROX_PAD;
  __syncthreads();
  // bitonic sort of order[0, P) by sort_key
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int p = tid; p < (P >> 1); p += PROX_THREADS) {
        const int a = 2 * p - (p & (stride - 1)), b = a + stride;
        const bool up = (a & size) == 0;
        const unsigned short oa = order[a], ob = order[b];
        if ((sort_key(dw, oa) > sort_key(dw, ob)) == up) { order[a] = ob; order[b] = oa; }
      }
      __syncthreads();
    }
  }
  if (tid >= 64) return;
  // step 5 (:407-432), wave 0
  const int lane = tid;
  int len = s_len;
  bool err = s_err != 0;
  int at = 0;
  while (!err && at < n_take) {
    const int p = at + lane;
    bool ok = false;
    if (p < n_take) ok = !((double)dw[order[p]] > thresh);
    const uint64_t m = __ballot(ok);
    if (m == 0ull) { at += 64; continue; }
    const int f = __ffsll((unsigned long long)m) - 1;
    if (len > max_factors) break;  // :415
    if (len + 2 > capacity) { err = true; break; }
    const int k = order[at + f];
    int i, j;
    prox_pair(g, k, i, j);
    if (lane == 0) {
      out_ii[len] = i; out_jj[len] = j;
      out_ii[len + 1] = j; out_jj[len + 1] = i;
    }
    len += 2;
    suppress(dw, i, j, nms, t0, t1, t, lane, 64);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // the wave's LDS writes before its next reads
    __builtin_amdgcn_wave_barrier();
    at += f + 1;
  }
  if (lane != 0) return;
  // step 6 (:434-438): the extra with the smallest d (lowest index on ties), taken if 0 < d < thresh (float32 compare)
  if (!err && g.n_extra > 0) {
    int best = cc;
    for (int k = cc + 1; k < L; k++)
      if (sort_key(dw, (unsigned short)k) < sort_key(dw, (unsigned short)best)) best = k;
    const float v = dw[best];
    if (v < (float)thresh && v > 0.f) {
      if (len + 2 > capacity) {
        err = true;
      } else {
        int i, j;
        prox_pair(g, best, i, j);
        out_ii[len] = i; out_jj[len] = j;
        out_ii[len + 1] = j; out_jj[len + 1] = i;
        len += 2;
      }
    }
  }
  *count = err ? (s_err == 2 ? -2 : -1) : len;
}

// covisible_graph.py:61-72: keep, in order, every proposal not in the existing list
__global__ __launch_bounds__(PROX_THREADS) void filter_repeated_edges_kernel(
    const int64_t *__restrict__ ii, const int64_t *__restrict__ jj, int n, const int64_t *__restrict__ ex_ii,
    const int64_t *__restrict__ ex_jj, int n_ex, int64_t *__restrict__ out_ii, int64_t *__restrict__ out_jj,
    int *__restrict__ count) {
  __shared__ int wsum[PROX_THREADS / 64];
  __shared__ int64_t sx[2][PROX_THREADS];
  int base = 0;
  for (int start = 0; start < n; start += PROX_THREADS) {
    const int p = start + threadIdx.x;
    int64_t a[1] = {0}, b[1] = {0};
    bool keep[1] = {p < n};
    if (keep[0]) { a[0] = ii[p]; b[0] = jj[p]; }
    strike_listed<PROX_THREADS>(ex_ii, ex_jj, n_ex, a, b, keep, 1, sx);
    int tot;
    const int off = flag_slot<PROX_THREADS>(keep[0], wsum, &tot);
    if (keep[0]) { out_ii[base + off] = a[0]; out_jj[base + off] = b[0]; }
    base += tot;
  }
  if (threadIdx.x == 0) *count = base;
}

}  // namespace dba

using namespace dba;

namespace {

// the number of edges step 4 appends (:395-405)
int64_t neighbour_edges(int t, int t0, int rad, int stereo) {
  int64_t n = 0;
  for (int i = t0; i < t; i++) n += (stereo ? 1 : 0) + 2 * (int64_t)std::max(i - std::max(i - rad - 1, 0), 0);
  return n;
}

}  // namespace

extern "C" {

int dba_frame_distance_bidir(const float *poses, const float *disps, const float *intrinsics, const int64_t *ii,
                             const int64_t *jj, int N, int n_frames, int ht, int wd, float beta, float *dist,
                             dba_stream_t stream) {
  if (N < 0 || n_frames < 0 || ht <= 0 || wd <= 0 || (int64_t)ht * wd > INT32_MAX) return DBA_ERR_ARG;
  if (N == 0) return DBA_OK;
  if (!poses || !disps || !intrinsics || !ii || !jj || !dist) return DBA_ERR_ARG;
  hipLaunchKernelGGL(frame_distance_bidir_kernel, dim3(N), dim3(512), 0, (hipStream_t)stream, poses, disps,
                     intrinsics, ii, jj, n_frames, ht * wd, wd, beta, dist);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

int dba_proximity_edges_capacity(int t, int t0, int rad, int stereo, int max_factors) {
  if (t0 < 0 || t0 >= t) return DBA_ERR_ARG;
  const int64_t cap = neighbour_edges(t, t0, rad, stereo) + std::max(max_factors, 0) + 4;
  return cap > INT32_MAX ? DBA_ERR_UNSUPPORTED : (int)cap;
}

int dba_proximity_edges(const float *poses, const float *disps, const float *intrinsics, int ht, int wd, int t,
                        int t0, int t1, int rad, int nms, float beta, double thresh, int max_factors, int stereo,
                        const int *skip_edge_host, int n_skip, int frontend_window, const int64_t *ex_ii,
                        const int64_t *ex_jj, int n_ex, float *dist, int64_t *edges, int capacity, int *count,
                        dba_stream_t stream) {
  if (ht <= 0 || wd <= 0 || (int64_t)ht * wd > INT32_MAX) return DBA_ERR_ARG;
  if (t0 < 0 || t1 < 0 || t0 >= t || t1 >= t || n_skip < 0 || n_ex < 0) return DBA_ERR_ARG;
  if (!poses || !disps || !intrinsics || !dist || !edges || !count || (n_ex > 0 && (!ex_ii || !ex_jj)) ||
      (n_skip > 0 && !skip_edge_host))
    return DBA_ERR_ARG;
  const int64_t cc = (int64_t)(t - t0) * (t - t1);
  if (n_skip > PROX_MAX_SKIP || cc + n_skip > PROX_MAX_CAND) return DBA_ERR_UNSUPPORTED;
  if (capacity < dba_proximity_edges_capacity(t, t0, rad, stereo, max_factors)) return DBA_ERR_WORKSPACE;
  ProxGrid g{};
  g.t = t; g.t0 = t0; g.t1 = t1; g.cc = (int)cc; g.n_extra = 0;
  // :371-377: max(ii) - min(ii) == frontend_window - 1 with max(ii) = t-1, min(ii) = t0
  if (n_skip > 0 && (t - 1) - t0 == frontend_window - 1)
    for (int s = 0; s < n_skip; s++)
      if ((int64_t)t0 + skip_edge_host[s] > 0) g.extra_jj[g.n_extra++] = t0 + skip_edge_host[s];
  const hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(proximity_distance_kernel, dim3(g.cc + g.n_extra), dim3(512), 0, s, poses, disps, intrinsics, g,
                     rad, ht * wd, wd, beta, dist);
  DBA_LAUNCH_CHECK();
  hipLaunchKernelGGL(proximity_select_kernel, dim3(1), dim3(PROX_THREADS), 0, s, dist, g, rad, nms, thresh,
                     max_factors, stereo, ex_ii, ex_jj, n_ex, edges, edges + capacity, capacity, count);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

int dba_filter_repeated_edges(const int64_t *ii, const int64_t *jj, int n, const int64_t *ex_ii, const int64_t *ex_jj,
                              int n_ex, int64_t *out_ii, int64_t *out_jj, int *count, dba_stream_t stream) {
  if (n < 0 || n_ex < 0 || !count) return DBA_ERR_ARG;
  if ((n > 0 && (!ii || !jj || !out_ii || !out_jj)) || (n_ex > 0 && (!ex_ii || !ex_jj))) return DBA_ERR_ARG;
  hipLaunchKernelGGL(filter_repeated_edges_kernel, dim3(1), dim3(PROX_THREADS), 0, (hipStream_t)stream, ii, jj, n,
                     ex_ii, ex_jj, n_ex, out_ii, out_jj, count);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

}  // extern "C"
