// The elementwise body of the update operator's ConvGRU (include/dba_hip.h "ConvGRU glue"), around the seven
// convolutions that stay with PyTorch / MIOpen:
//
//   dba_gru_pack     <- inp = torch.cat(inputs, 1); net_inp = torch.cat([net, inp], 1)        (dbaf/modules/gru.py:20-21)
//   dba_gru_pack_relu   the same with torch.relu on chosen sources: the encoders' last ReLUs  (dbaf/droid_net.py:83, :89)
//   dba_gru_context  <- glo = (sigmoid(w(net)) * net).view(b, c, h*w).mean(-1)                (:24-25)
//   dba_gru_reset    <- r = sigmoid(convr(net_inp) + convr_glo(glo)); cat([r*net, inp], 1)    (:28-29)
//   dba_gru_blend    <- z = sigmoid(..), q = tanh(..), net = (1-z) * net + z * q              (:27, :29, :31)
//
// Four streaming launches.  Every statement of the reference produces a tensor of the input dtype, so a kernel rounds to
// that dtype (rnd<T>) exactly where a statement ends and computes in float32 in between; this file is built with
// -ffp-contract=off.  expf, tanhf and the division are the correctly rounded / few-ulp library forms: the fast
// v_exp_f32 path loses log2(e) x |x| rounding units in the argument, far more than the tests' band allows.
//
// Layout.  Tensors are [n, c, hw]; an edge's c * hw elements are contiguous, and the packed buffer keeps C = sum c_k
// channels per edge.  The elementwise kernels walk an edge's c * hw elements in 16-byte vectors when c * hw * itemsize
// and C * hw * itemsize are multiples of 16 and the bases are aligned (a vector may then straddle planes: the lane
// follows the plane index through its vector and reloads the per-plane gate term where it changes); otherwise element
// by element.  The context kernel owns one plane per workgroup and takes vectors when hw * itemsize is a multiple of 16.
// No atomics, no host read; LDS only for the four wave partials of the context sum, added in wave order.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "common.h"
#include "gru_gates.h"
#include "row_jobs.h"

namespace dba {

constexpr int GRU_THREADS = 256;
constexpr int GRU_UNROLL = 2;  // vectors in flight per lane and input tensor

template <typename T, int W>
struct alignas(sizeof(T) * W) GruVec {
  T e[W];
};

// rnd<T>, sigmoid_f32 and the gate statements: gru_gates.h (shared with the convolution epilogues of conv3x3.hip)

// ---- pack -------------------------------------------------------------------------------------------------------------
struct PackTable {
  const char *src[DBA_GRU_MAX_SOURCES];
  long long run[DBA_GRU_MAX_SOURCES];        // bytes of the source per edge, c_k * hw * itemsize
  long long off[DBA_GRU_MAX_SOURCES];        // where the run starts in an edge's row of dst, in bytes
  unsigned chunk_start[DBA_GRU_MAX_SOURCES]; // first chunk of the source among an edge's chunks
  int n_src, width;
  long long row_bytes;
  unsigned chunks;  // per edge, all sources
};

__global__ __launch_bounds__(MOVE_THREADS) void gru_pack_kernel(char *dst, PackTable t) {
  const unsigned e = blockIdx.x / t.chunks, local = blockIdx.x - e * t.chunks;
  // the workgroup's source: constant indices and selects keep the table in scalar registers (row_jobs.h)
  const char *src = t.src[0];
  long long run = t.run[0], off = t.off[0];
  unsigned start = 0;
#pragma unroll
  for (int k = 1; k < DBA_GRU_MAX_SOURCES; k++)
    if (k < t.n_src && local >= t.chunk_start[k]) {
      src = t.src[k];
      run = t.run[k];
      off = t.off[k];
      start = t.chunk_start[k];
    }
  const char *s = src + (long long)e * run;
  char *d = dst + (long long)e * t.row_bytes + off;
  const unsigned chunk = local - start;
  switch (t.width) {
    case 16: copy_chunk<u32x4>(s, d, run / 16, chunk); break;
    case 8: copy_chunk<uint64_t>(s, d, run / 8, chunk); break;
    case 4: copy_chunk<uint32_t>(s, d, run / 4, chunk); break;
    default: copy_chunk<uint16_t>(s, d, run / 2, chunk); break;
  }
}

// pack with torch.relu on the marked sources: the same walk as gru_pack_kernel, in a kernel of its own so that the plain
// copy keeps its registers.  The ReLU is taken on the bits (no conversion): an element is kept when its sign bit is clear
// or it is a NaN, and becomes +0 otherwise, which is torch.relu byte for byte (NaN payloads go through, -0 -> +0).
template <typename U>   // U: the unsigned integer of the element's size
__device__ __forceinline__ U relu_bits(U u) {
  constexpr U SIGN = (U)1 << (8 * sizeof(U) - 1);
  constexpr U EXP = sizeof(U) == 2 ? (U)0x7c00 : (U)0x7f800000;
  return (!(u & SIGN) || (U)(u & ~SIGN) > EXP) ? u : (U)0;
}

template <typename V, typename U>
__device__ __forceinline__ void copy_chunk_relu(const char *s, char *d, long long n, unsigned chunk, bool relu) {
  constexpr int PER = sizeof(V) / sizeof(U);
  union Item {
    V v;
    U u[PER];
  };
  const V *sp = (const V *)s;
  V *dp = (V *)d;
  const long long e0 = (long long)chunk * MOVE_CHUNK + threadIdx.x;
  Item it[MOVE_UNROLL];
#pragma unroll
  for (int u = 0; u < MOVE_UNROLL; u++)
    if (e0 + u * MOVE_THREADS < n) it[u].v = sp[e0 + u * MOVE_THREADS];
  if (relu) {
#pragma unroll
    for (int u = 0; u < MOVE_UNROLL; u++) {
#pragma unroll
      for (int j = 0; j < PER; j++) it[u].u[j] = relu_bits<U>(it[u].u[j]);
    }
  }
#pragma unroll
  for (int u = 0; u < MOVE_UNROLL; u++)
    if (e0 + u * MOVE_THREADS < n) dp[e0 + u * MOVE_THREADS] = it[u].v;
}

template <typename U>
__global__ __launch_bounds__(MOVE_THREADS) void gru_pack_relu_kernel(char *dst, PackTable t, unsigned relu_mask) {
  const unsigned e = blockIdx.x / t.chunks, local = blockIdx.x - e * t.chunks;
  const char *src = t.src[0];
  long long run = t.run[0], off = t.off[0];
  unsigned start = 0;
  bool relu = relu_mask & 1u;
#pragma unroll
  for (int k = 1; k < DBA_GRU_MAX_SOURCES; k++)
    if (k < t.n_src && local >= t.chunk_start[k]) {
      src = t.src[k];
      run = t.run[k];
      off = t.off[k];
      start = t.chunk_start[k];
      relu = (relu_mask >> k) & 1u;
    }
  const char *s = src + (long long)e * run;
  char *d = dst + (long long)e * t.row_bytes + off;
  const unsigned chunk = local - start;
  if constexpr (sizeof(U) == 2) {
    switch (t.width) {
      case 16: copy_chunk_relu<u32x4, U>(s, d, run / 16, chunk, relu); break;
      case 8: copy_chunk_relu<uint64_t, U>(s, d, run / 8, chunk, relu); break;
      case 4: copy_chunk_relu<uint32_t, U>(s, d, run / 4, chunk, relu); break;
      default: copy_chunk_relu<uint16_t, U>(s, d, run / 2, chunk, relu); break;
    }
  } else {
    switch (t.width) {   // float elements: every run starts and ends on 4 bytes
      case 16: copy_chunk_relu<u32x4, U>(s, d, run / 16, chunk, relu); break;
      case 8: copy_chunk_relu<uint64_t, U>(s, d, run / 8, chunk, relu); break;
      default: copy_chunk_relu<uint32_t, U>(s, d, run / 4, chunk, relu); break;
    }
  }
}

// ---- context ------------------------------------------------------------------------------------------------------------
// glo[plane] = rnd( (sum over the plane of rnd(rnd(sigmoid(a)) * net)) * inv_hw ): a lane adds its elements in index
// order (vector v = tid, tid + 256, ...; within a vector front to back), the 64 lanes fold on the DPP network, the four
// wave totals are added in wave order.  One fixed order: the same bits run to run.
template <typename T, int W>
__global__ __launch_bounds__(GRU_THREADS) void gru_context_kernel(const T *__restrict__ a, const T *__restrict__ net,
                                                                  T *__restrict__ glo, int hw, float inv_hw) {
  using VT = GruVec<T, W>;
  __shared__ float part[GRU_THREADS / WAVE];
  const long long base = (long long)blockIdx.x * hw;
  const VT *av = (const VT *)(a + base), *nv = (const VT *)(net + base);
  const int n_vec = hw / W;  // W == 1 or hw % W == 0
  float acc = 0.0f;
  for (int v0 = threadIdx.x; v0 < n_vec; v0 += GRU_THREADS * GRU_UNROLL) {
    VT x[GRU_UNROLL], y[GRU_UNROLL];
#pragma unroll
    for (int u = 0; u < GRU_UNROLL; u++)
      if (v0 + u * GRU_THREADS < n_vec) {
        x[u] = av[v0 + u * GRU_THREADS];
        y[u] = nv[v0 + u * GRU_THREADS];
      }
#pragma unroll
    for (int u = 0; u < GRU_UNROLL; u++)
      if (v0 + u * GRU_THREADS < n_vec) {
#pragma unroll
        for (int j = 0; j < W; j++) acc += rnd<T>(rnd<T>(sigmoid_f32((float)x[u].e[j])) * (float)y[u].e[j]);
      }
  }
  acc = wave_sum_to_lane63(acc);
  if (lane_id() == WAVE - 1) part[threadIdx.x / WAVE] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = part[0];
#pragma unroll
    for (int w = 1; w < GRU_THREADS / WAVE; w++) s += part[w];
    glo[blockIdx.x] = (T)(s * inv_hw);
  }
}

// ---- reset gate and blend -------------------------------------------------------------------------------------------------
// A lane's vector starts at element i of its edge's c * hw: plane i / hw, then on through the vector.
struct PlaneWalk {
  int plane, r, hw;
  __device__ __forceinline__ PlaneWalk(int i, int hw_) : plane(i / hw_), r(i - (i / hw_) * hw_), hw(hw_) {}
  // true when the NEXT element lies in another plane
  __device__ __forceinline__ bool step() {
    if (++r < hw) return false;
    r = 0;
    plane++;
    return true;
  }
};

// buf[e, 0:c] = rnd( rnd(sigmoid(rnd(cr + gr))) * net ); buf rows are row_stride elements apart, the others c * hw
template <typename T, int W>
__global__ __launch_bounds__(GRU_THREADS) void gru_reset_kernel(T *__restrict__ buf, const T *__restrict__ cr,
                                                                const T *__restrict__ gr, const T *__restrict__ net, int c,
                                                                int hw, long long row_stride, unsigned chunks) {
  using VT = GruVec<T, W>;
  const unsigned e = blockIdx.x / chunks, chunk = blockIdx.x - e * chunks;
  const long long row = (long long)c * hw;  // < 2^31 (host)
  const T *cr_e = cr + (long long)e * row, *net_e = net + (long long)e * row, *gr_e = gr + (long long)e * c;
  T *dst = buf + (long long)e * row_stride;
  long long i[GRU_UNROLL];
  VT x[GRU_UNROLL], y[GRU_UNROLL];
#pragma unroll
  for (int u = 0; u < GRU_UNROLL; u++) {
    i[u] = (((long long)chunk * GRU_UNROLL + u) * GRU_THREADS + threadIdx.x) * W;
    if (i[u] < row) {
      x[u] = *(const VT *)(cr_e + i[u]);
      y[u] = *(const VT *)(net_e + i[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < GRU_UNROLL; u++) {
    if (i[u] >= row) continue;
    PlaneWalk w((int)i[u], hw);
    float g = (float)gr_e[w.plane];
    VT o;
#pragma unroll
    for (int j = 0; j < W; j++) {
      o.e[j] = gru_reset_value<T>((float)x[u].e[j], g, (float)y[u].e[j]);
      if (j + 1 < W && w.step()) g = (float)gr_e[w.plane];
    }
    *(VT *)(dst + i[u]) = o;
  }
}

// out = rnd( rnd(rnd(1 - z) * net) + rnd(z * q) ), z = rnd(sigmoid(rnd(cz + gz))), q = rnd(tanh(rnd(cq + gq))).  out may be
// net: a lane reads its own elements of net before it writes them, and no other lane touches them (no __restrict__ there).
template <typename T, int W>
__global__ __launch_bounds__(GRU_THREADS) void gru_blend_kernel(const T *__restrict__ cz, const T *__restrict__ gz,
                                                                const T *__restrict__ cq, const T *__restrict__ gq,
                                                                const T *net, T *out, int c, int hw, unsigned chunks) {
  using VT = GruVec<T, W>;
  const unsigned e = blockIdx.x / chunks, chunk = blockIdx.x - e * chunks;
  const long long row = (long long)c * hw, e0 = (long long)e * row;
  const T *gz_e = gz + (long long)e * c, *gq_e = gq + (long long)e * c;
  long long i[GRU_UNROLL];
  VT xz[GRU_UNROLL], xq[GRU_UNROLL], y[GRU_UNROLL];
#pragma unroll
  for (int u = 0; u < GRU_UNROLL; u++) {
    i[u] = (((long long)chunk * GRU_UNROLL + u) * GRU_THREADS + threadIdx.x) * W;
    if (i[u] < row) {
      xz[u] = *(const VT *)(cz + e0 + i[u]);
      xq[u] = *(const VT *)(cq + e0 + i[u]);
      y[u] = *(const VT *)(net + e0 + i[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < GRU_UNROLL; u++) {
    if (i[u] >= row) continue;
    PlaneWalk w((int)i[u], hw);
    float bz = (float)gz_e[w.plane], bq = (float)gq_e[w.plane];
    VT o;
#pragma unroll
    for (int j = 0; j < W; j++) {
      o.e[j] = gru_blend_value<T>(gru_gate<T>((float)xz[u].e[j], bz), (float)xq[u].e[j], bq, (float)y[u].e[j]);
      if (j + 1 < W && w.step()) {
        bz = (float)gz_e[w.plane];
        bq = (float)gq_e[w.plane];
      }
    }
    *(VT *)(out + e0 + i[u]) = o;
  }
}

}  // namespace dba

using namespace dba;

namespace {

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

int item_size(int dtype) { return dtype == DBA_F16 ? 2 : dtype == DBA_F32 ? 4 : 0; }

// the grid of an elementwise kernel over n edges of `row` elements in vectors of W: chunks per edge, 0 when it does not fit
unsigned edge_chunks(int n, long long row, int W) {
  const long long per = (long long)GRU_THREADS * GRU_UNROLL * W;
  const long long chunks = (row + per - 1) / per;
  if (chunks * (long long)n > (long long)INT32_MAX) return 0;
  return (unsigned)chunks;
}

template <typename T>
int launch_context(const void *a, const void *net, void *glo, int planes, int hw, hipStream_t s) {
  constexpr int W = 16 / sizeof(T);
  const float inv_hw = 1.0f / (float)hw;
  if (hw % W == 0 && aligned16(a) && aligned16(net))
    hipLaunchKernelGGL((gru_context_kernel<T, W>), dim3(planes), dim3(GRU_THREADS), 0, s, (const T *)a, (const T *)net,
                       (T *)glo, hw, inv_hw);
  else
    hipLaunchKernelGGL((gru_context_kernel<T, 1>), dim3(planes), dim3(GRU_THREADS), 0, s, (const T *)a, (const T *)net,
                       (T *)glo, hw, inv_hw);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

template <typename T>
int launch_reset(void *buf, long long row_stride, const void *cr, const void *gr, const void *net, int n, int c, int hw,
                 hipStream_t s) {
  constexpr int W = 16 / sizeof(T);
  const long long row = (long long)c * hw;
  const bool vec = row % W == 0 && row_stride % W == 0 && aligned16(buf) && aligned16(cr) && aligned16(net);
  const unsigned chunks = edge_chunks(n, row, vec ? W : 1);
  if (!chunks) return DBA_ERR_ARG;
  if (vec)
    hipLaunchKernelGGL((gru_reset_kernel<T, W>), dim3(chunks * (unsigned)n), dim3(GRU_THREADS), 0, s, (T *)buf, (const T *)cr,
                       (const T *)gr, (const T *)net, c, hw, row_stride, chunks);
  else
    hipLaunchKernelGGL((gru_reset_kernel<T, 1>), dim3(chunks * (unsigned)n), dim3(GRU_THREADS), 0, s, (T *)buf, (const T *)cr,
                       (const T *)gr, (const T *)net, c, hw, row_stride, chunks);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

template <typename T>
int launch_blend(const void *cz, const void *gz, const void *cq, const void *gq, const void *net, void *out, int n, int c,
                 int hw, hipStream_t s) {
  constexpr int W = 16 / sizeof(T);
  const long long row = (long long)c * hw;
  const bool vec = row % W == 0 && aligned16(cz) && aligned16(cq) && aligned16(net) && aligned16(out);
  const unsigned chunks = edge_chunks(n, row, vec ? W : 1);
  if (!chunks) return DBA_ERR_ARG;
  if (vec)
    hipLaunchKernelGGL((gru_blend_kernel<T, W>), dim3(chunks * (unsigned)n), dim3(GRU_THREADS), 0, s, (const T *)cz,
                       (const T *)gz, (const T *)cq, (const T *)gq, (const T *)net, (T *)out, c, hw, chunks);
  else
    hipLaunchKernelGGL((gru_blend_kernel<T, 1>), dim3(chunks * (unsigned)n), dim3(GRU_THREADS), 0, s, (const T *)cz,
                       (const T *)gz, (const T *)cq, (const T *)gq, (const T *)net, (T *)out, c, hw, chunks);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

// extents every entry point shares: positive, an edge's c * hw elements below 2^31, n * c planes within the grid limit
bool extents_ok(int n, int c, int hw) {
  if (n <= 0 || c <= 0 || hw <= 0) return false;
  if ((long long)c * hw > (long long)INT32_MAX) return false;
  return (long long)n * c <= (long long)INT32_MAX;
}

}  // namespace

extern "C" {

// the checks and the table of a pack; with_relu: the kernel that applies the mask, else the plain copy
static int pack_impl(const void *const *srcs, const int *channels, int n_src, int n, int hw, int dtype, void *dst, int with_relu,
                     unsigned relu_mask, dba_stream_t stream) {
  const int isz = item_size(dtype);
  if (!isz) return DBA_ERR_UNSUPPORTED;
  if (!srcs || !channels || !dst || n_src < 1 || n_src > DBA_GRU_MAX_SOURCES || n <= 0 || hw <= 0) return DBA_ERR_ARG;
  long long c_total = 0;
  for (int k = 0; k < n_src; k++) {
    if (!srcs[k] || channels[k] <= 0 || ((uintptr_t)srcs[k] % isz)) return DBA_ERR_ARG;
    c_total += channels[k];
  }
  if ((uintptr_t)dst % isz || c_total > INT32_MAX || !extents_ok(n, (int)c_total, hw)) return DBA_ERR_ARG;
  PackTable t{};
  t.n_src = n_src;
  t.row_bytes = c_total * hw * isz;
  uintptr_t bits = (uintptr_t)dst | (uintptr_t)t.row_bytes;
  for (int k = 0; k < n_src; k++) {
    t.src[k] = (const char *)srcs[k];
    t.run[k] = (long long)channels[k] * hw * isz;
    t.off[k] = k ? t.off[k - 1] + t.run[k - 1] : 0;
    if (ranges_overlap(dst, t.row_bytes * n, srcs[k], t.run[k] * n)) return DBA_ERR_ARG;
    bits |= (uintptr_t)srcs[k] | (uintptr_t)t.run[k];
  }
  t.width = (bits & 15) == 0 ? 16 : (bits & 7) == 0 ? 8 : (bits & 3) == 0 ? 4 : 2;  // every run starts and ends on it
  unsigned long long chunks = 0;
  for (int k = 0; k < n_src; k++) {
    t.chunk_start[k] = (unsigned)chunks;
    chunks += (unsigned long long)((t.run[k] / t.width + MOVE_CHUNK - 1) / MOVE_CHUNK);
    if (chunks * (unsigned long long)n > (unsigned long long)INT32_MAX) return DBA_ERR_ARG;
  }
  t.chunks = (unsigned)chunks;
  const dim3 grid(t.chunks * (unsigned)n);
  if (!with_relu)
    hipLaunchKernelGGL(gru_pack_kernel, grid, dim3(MOVE_THREADS), 0, (hipStream_t)stream, (char *)dst, t);
  else if (isz == 2)
    hipLaunchKernelGGL(gru_pack_relu_kernel<uint16_t>, grid, dim3(MOVE_THREADS), 0, (hipStream_t)stream, (char *)dst, t, relu_mask);
  else
    hipLaunchKernelGGL(gru_pack_relu_kernel<uint32_t>, grid, dim3(MOVE_THREADS), 0, (hipStream_t)stream, (char *)dst, t, relu_mask);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

int dba_gru_pack(const void *const *srcs, const int *channels, int n_src, int n, int hw, int dtype, void *dst,
                 dba_stream_t stream) {
  return pack_impl(srcs, channels, n_src, n, hw, dtype, dst, 0, 0u, stream);
}

int dba_gru_pack_relu(const void *const *srcs, const int *channels, int n_src, int n, int hw, int dtype, void *dst,
                      unsigned relu_mask, dba_stream_t stream) {
  if (n_src >= 1 && n_src <= DBA_GRU_MAX_SOURCES && (relu_mask >> n_src)) return DBA_ERR_ARG;   // a bit without a source
  return pack_impl(srcs, channels, n_src, n, hw, dtype, dst, 1, relu_mask, stream);
}

int dba_gru_context(const void *a, const void *net, int n, int c, int hw, int dtype, void *glo, dba_stream_t stream) {
  const int isz = item_size(dtype);
  if (!isz) return DBA_ERR_UNSUPPORTED;
  if (!a || !net || !glo || !extents_ok(n, c, hw)) return DBA_ERR_ARG;
  if (((uintptr_t)a | (uintptr_t)net | (uintptr_t)glo) % isz) return DBA_ERR_ARG;
  const long long bytes = (long long)n * c * hw * isz, gbytes = (long long)n * c * isz;
  if (ranges_overlap(glo, gbytes, a, bytes) || ranges_overlap(glo, gbytes, net, bytes)) return DBA_ERR_ARG;
  return dtype == DBA_F16 ? launch_context<_Float16>(a, net, glo, n * c, hw, (hipStream_t)stream)
                          : launch_context<float>(a, net, glo, n * c, hw, (hipStream_t)stream);
}

int dba_gru_reset(void *buf, int c_total, const void *cr, const void *gr, const void *net, int n, int c, int hw, int dtype,
                  dba_stream_t stream) {
  const int isz = item_size(dtype);
  if (!isz) return DBA_ERR_UNSUPPORTED;
  if (!buf || !cr || !gr || !net || !extents_ok(n, c, hw) || c_total < c || !extents_ok(n, c_total, hw)) return DBA_ERR_ARG;
  if (((uintptr_t)buf | (uintptr_t)cr | (uintptr_t)gr | (uintptr_t)net) % isz) return DBA_ERR_ARG;
  const long long bytes = (long long)n * c * hw * isz, gbytes = (long long)n * c * isz;
  const long long bbytes = (long long)n * c_total * hw * isz;
  if (ranges_overlap(buf, bbytes, cr, bytes) || ranges_overlap(buf, bbytes, gr, gbytes) || ranges_overlap(buf, bbytes, net, bytes))
    return DBA_ERR_ARG;
  const long long stride = (long long)c_total * hw;
  return dtype == DBA_F16 ? launch_reset<_Float16>(buf, stride, cr, gr, net, n, c, hw, (hipStream_t)stream)
                          : launch_reset<float>(buf, stride, cr, gr, net, n, c, hw, (hipStream_t)stream);
}

int dba_gru_blend(const void *cz, const void *gz, const void *cq, const void *gq, const void *net, int n, int c, int hw,
                  int dtype, void *out, dba_stream_t stream) {
  const int isz = item_size(dtype);
  if (!isz) return DBA_ERR_UNSUPPORTED;
  if (!cz || !gz || !cq || !gq || !net || !out || !extents_ok(n, c, hw)) return DBA_ERR_ARG;
  if (((uintptr_t)cz | (uintptr_t)gz | (uintptr_t)cq | (uintptr_t)gq | (uintptr_t)net | (uintptr_t)out) % isz) return DBA_ERR_ARG;
  const long long bytes = (long long)n * c * hw * isz, gbytes = (long long)n * c * isz;
  if (ranges_overlap(out, bytes, cz, bytes) || ranges_overlap(out, bytes, cq, bytes) || ranges_overlap(out, bytes, gz, gbytes) ||
      ranges_overlap(out, bytes, gq, gbytes))
    return DBA_ERR_ARG;
  if (out != net && ranges_overlap(out, bytes, net, bytes)) return DBA_ERR_ARG;
  return dtype == DBA_F16 ? launch_blend<_Float16>(cz, gz, cq, gq, net, out, n, c, hw, (hipStream_t)stream)
                          : launch_blend<float>(cz, gz, cq, gq, net, out, n, c, hw, (hipStream_t)stream);
}

}  // extern "C"
