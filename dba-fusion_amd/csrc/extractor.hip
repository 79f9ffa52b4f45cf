// The glue of the feature and context encoders (include/dba_hip.h "Encoder glue"), around the convolutions that stay with
// PyTorch / MIOpen (dbaf/modules/extractor.py:47-55, :183-198; dbaf/motion_filter.py:29-30, :35-36, :64-65):
//
//   dba_enc_norm           <- relu(InstanceNorm2d(x)), or the norm alone
//   dba_enc_norm_skip      <- relu(skip + relu(norm2(x))), skip as it is or norm3(d) of the 1x1 downsample branch
//   dba_enc_relu_skip      <- relu(skip + relu(x)), the same tail with norm_fn='none'
//   dba_enc_image          <- image[:, [2,1,0]] / 255.0, .sub_(MEAN), .div_(STDV)
//   dba_enc_context_split  <- net, inp = cnet(image).split(..); net.tanh(), inp.relu()
//
// Every statement of the reference yields a tensor of the input dtype, so a kernel rounds to that dtype (rnd<T>) exactly
// where a statement ends and computes in float32 in between; this file is built with -ffp-contract=off.
//
// The norm kernels.  One workgroup owns one plane (the two-norm tail: one plane of x and the plane of d that goes with
// it) and HOLDS it in registers: at most 64 elements per lane at 1024 lanes, hence the cap of 65536 elements.  The plane
// is cut into items, 16-byte vectors when hw * itemsize is a multiple of 16 and every base is aligned, else elements;
// lane t holds items t, t + lanes, t + 2 lanes, ...  enc_geometry() picks the lane count (a power of two, 64 .. 1024)
// and the items per lane (a power of two) from the item count, so a 5 x 7 plane is one wave.
// The summation order is fixed: a lane adds its elements in index order, the 64 lanes of a wave fold on the DPP network,
// the wave totals are added in wave order by every lane alike.  mean = sum / hw; var = (sum of (x - mean)^2 over the held
// values) / hw; r = 1 / sqrt(var + eps), all float32 and correctly rounded.  The same bits run to run; (mean, r) as
// multiplied with go to `stats` when it is given.  No atomics, no host read; LDS only for the wave totals.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "common.h"

namespace dba {

constexpr int ENC_MAX_THREADS = 1024;
constexpr int ENC_MAX_WAVES = ENC_MAX_THREADS / WAVE;
constexpr int ENC_MAX_PER_LANE = 64;                                  // elements a lane holds of one plane
constexpr int ENC_MAX_PLANE = ENC_MAX_THREADS * ENC_MAX_PER_LANE;     // 65536
constexpr int ENC_THREADS = 256;                                      // the elementwise kernels
constexpr int ENC_UNROLL = 2;

template <typename T, int W>
struct alignas(sizeof(T) * W) EncVec {
  T e[W];
};

template <typename T>
__device__ __forceinline__ float enc_rnd(float x) { return (float)(T)x; }  // the end of a statement

// A float32 product that is rounded to half next: keeps its float32 rounding.  Without it the backend rounds the exact
// product to half in ONE step (v_fma_mixlo_f16), which differs from the statement's two roundings where the float32
// result is a tie of half.
__device__ __forceinline__ float enc_f32(float x) {
  asm("" : "+v"(x));
  return x;
}

// torch.relu: NaN goes through (fmaxf would drop it)
__device__ __forceinline__ float enc_relu(float x) { return x > 0.0f ? x : (x != x ? x : 0.0f); }

// the sum over the workgroup, the same value in every lane: DPP fold, then the wave totals in wave order
__device__ __forceinline__ float enc_block_sum(float v, float *part, int waves) {
  v = wave_sum_to_lane63(v);
  if (lane_id() == WAVE - 1) part[threadIdx.x / WAVE] = v;
  __syncthreads();
  float s = part[0];
  for (int w = 1; w < waves; w++) s += part[w];
  return s;
}

// which of a lane's items t + k lanes exist: rounds k < full for every lane (a scalar test, no per-item lane mask), round
// k == full for the lanes below the remainder
struct EncValid {
  int full;
  bool tail;
  __device__ __forceinline__ EncValid(int n_items) : full(n_items / (int)blockDim.x), tail((int)threadIdx.x < n_items - full * (int)blockDim.x) {}
  __device__ __forceinline__ bool operator()(int k) const { return k < full || (k == full && tail); }
};

// a plane in registers: V items of W elements per lane
template <typename T, int V, int W>
struct EncHeld {
  EncVec<T, W> v[V];

  __device__ __forceinline__ void load(const T *plane, int n_items) {
    const EncVec<T, W> *p = (const EncVec<T, W> *)plane;
    const EncValid ok(n_items);
#pragma unroll
    for (int k = 0; k < V; k++)
      if (ok(k)) v[k] = p[threadIdx.x + k * blockDim.x];
  }
  // (mean, r) of the held plane; part: two rows of ENC_MAX_WAVES floats
  __device__ __forceinline__ void stats(int n_items, int hw, float eps, float (*part)[ENC_MAX_WAVES], float &mean, float &r) const {
    const int waves = blockDim.x / WAVE;
    const EncValid ok(n_items);
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < V; k++)
      if (ok(k)) {
#pragma unroll
        for (int j = 0; j < W; j++) acc += (float)v[k].e[j];
      }
    mean = enc_block_sum(acc, part[0], waves) / (float)hw;
    acc = 0.0f;
#pragma unroll
    for (int k = 0; k < V; k++)
      if (ok(k)) {
#pragma unroll
        for (int j = 0; j < W; j++) {
          const float d = (float)v[k].e[j] - mean;
          acc += d * d;
        }
      }
    const float var = enc_block_sum(acc, part[1], waves) / (float)hw;
    r = 1.0f / sqrtf(var + eps);
  }
};

// out = rnd(relu?((x - mean) * r)).  out may be x: the workgroup holds its plane before it writes (no __restrict__).
template <typename T, int V, int W>
__global__ __launch_bounds__(ENC_MAX_THREADS) void enc_norm_kernel(const T *x, T *out, float *__restrict__ stats, int hw,
                                                                   float eps, int relu) {
  __shared__ float part[2][ENC_MAX_WAVES];
  const long long base = (long long)blockIdx.x * hw;
  const int n_items = hw / W;  // W == 1 or hw % W == 0
  EncHeld<T, V, W> h;
  h.load(x + base, n_items);
  float mean, r;
  h.stats(n_items, hw, eps, part, mean, r);
  if (stats && threadIdx.x == 0) {
    stats[2 * (long long)blockIdx.x] = mean;
    stats[2 * (long long)blockIdx.x + 1] = r;
  }
  EncVec<T, W> *o = (EncVec<T, W> *)(out + base);
  const EncValid ok(n_items);
#pragma unroll
  for (int k = 0; k < V; k++) {
    const int item = threadIdx.x + k * blockDim.x;
    if (ok(k)) {
      EncVec<T, W> y;
#pragma unroll
      for (int j = 0; j < W; j++) {
        const float t = enc_f32(((float)h.v[k].e[j] - mean) * r);
        y.e[j] = (T)(relu ? enc_relu(t) : t);
      }
      o[item] = y;
    }
  }
}

// out = rnd(relu(rnd(s + y))), y = rnd(relu(norm(x))), s = side (MODE 0: the skip as it is) or rnd(norm(side)) (the
// downsample branch; MODE 1: its plane is held next to x's, MODE 2: both planes together are beyond the register budget,
// so d's plane is read a second time, from L2, where it is written).  out may be x.
template <typename T, int V, int W, int MODE>
__global__ __launch_bounds__(ENC_MAX_THREADS) void enc_norm_skip_kernel(const T *x, const T *__restrict__ side, T *out,
                                                                        float *__restrict__ stats, float *__restrict__ stats_d,
                                                                        int hw, float eps) {
  __shared__ float part[4][ENC_MAX_WAVES];
  const long long base = (long long)blockIdx.x * hw;
  const int n_items = hw / W;
  const EncVec<T, W> *sv = (const EncVec<T, W> *)(side + base);
  float mean, r, mean_d = 0.0f, r_d = 1.0f;
  EncHeld<T, (MODE == 1 ? V : 1), W> hd;
  if constexpr (MODE == 1) {
    hd.load(side + base, n_items);
    hd.stats(n_items, hw, eps, part + 2, mean_d, r_d);
  } else if constexpr (MODE == 2) {
    EncHeld<T, V, W> tmp;  // gone before x's plane is loaded
    tmp.load(side + base, n_items);
    tmp.stats(n_items, hw, eps, part + 2, mean_d, r_d);
  }
  EncHeld<T, V, W> h;
  h.load(x + base, n_items);
  h.stats(n_items, hw, eps, part, mean, r);
  if (threadIdx.x == 0) {
    if (stats) {
      stats[2 * (long long)blockIdx.x] = mean;
      stats[2 * (long long)blockIdx.x + 1] = r;
    }
    if (MODE != 0 && stats_d) {
      stats_d[2 * (long long)blockIdx.x] = mean_d;
      stats_d[2 * (long long)blockIdx.x + 1] = r_d;
    }
  }
  EncVec<T, W> *o = (EncVec<T, W> *)(out + base);
  const EncValid ok(n_items);
#pragma unroll
  for (int k = 0; k < V; k++) {
    const int item = threadIdx.x + k * blockDim.x;
    if (ok(k)) {
      EncVec<T, W> s, y;
      if constexpr (MODE == 1) s = hd.v[k];
      else s = sv[item];
#pragma unroll
      for (int j = 0; j < W; j++) {
        const float yy = enc_rnd<T>(enc_relu(enc_f32(((float)h.v[k].e[j] - mean) * r)));
        float ss = (float)s.e[j];
        if (MODE != 0) ss = enc_rnd<T>(enc_f32((ss - mean_d) * r_d));
        y.e[j] = (T)enc_relu(enc_rnd<T>(ss + yy));
      }
      o[item] = y;
    }
  }
}

// ---- elementwise ----------------------------------------------------------------------------------------------------------
// out = rnd(relu(rnd(skip + relu(x)))); out may be x: a lane reads its own elements before it writes them
template <typename T, int W>
__global__ __launch_bounds__(ENC_THREADS) void enc_relu_skip_kernel(const T *x, const T *__restrict__ skip, T *out,
                                                                    long long count) {
  using VT = EncVec<T, W>;
  long long i[ENC_UNROLL];
  VT a[ENC_UNROLL], b[ENC_UNROLL];
#pragma unroll
  for (int u = 0; u < ENC_UNROLL; u++) {
    i[u] = (((long long)blockIdx.x * ENC_UNROLL + u) * ENC_THREADS + threadIdx.x) * W;
    if (i[u] < count) {
      a[u] = *(const VT *)(x + i[u]);
      b[u] = *(const VT *)(skip + i[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < ENC_UNROLL; u++) {
    if (i[u] >= count) continue;
    VT o;
#pragma unroll
    for (int j = 0; j < W; j++) o.e[j] = (T)enc_relu(enc_rnd<T>((float)b[u].e[j] + enc_relu((float)a[u].e[j])));
    *(VT *)(out + i[u]) = o;
  }
}

// out[p, c] = ((img[p, 2 - c] * (1 / 255)) - mean_c) / std_c: the product with the float32 reciprocal is what torch's
// `/ 255.0` (a division by a host scalar) runs on the device; the division by std is a division.  One rounding to half.
struct ImageConsts {
  float mean[3], stdv[3];
};

template <typename S, typename D, int W>
__global__ __launch_bounds__(ENC_THREADS) void enc_image_kernel(const S *__restrict__ img, D *__restrict__ out, int hw,
                                                                unsigned chunks, ImageConsts k) {
  const unsigned plane = blockIdx.x / chunks, chunk = blockIdx.x - plane * chunks;
  const unsigned frame = plane / 3, c = plane - frame * 3;
  const int i = (chunk * ENC_THREADS + threadIdx.x) * W;
  if (i >= hw) return;
  const float mean = c == 0 ? k.mean[0] : c == 1 ? k.mean[1] : k.mean[2];
  const float stdv = c == 0 ? k.stdv[0] : c == 1 ? k.stdv[1] : k.stdv[2];
  const EncVec<S, W> v = *(const EncVec<S, W> *)(img + ((long long)frame * 3 + (2 - c)) * hw + i);
  EncVec<D, W> o;
  const float inv = 1.0f / 255.0f;
#pragma unroll
  for (int j = 0; j < W; j++) o.e[j] = (D)((((float)v.e[j] * inv) - mean) / stdv);
  *(EncVec<D, W> *)(out + (long long)plane * hw + i) = o;
}

// x [n, (c_net + c_inp) hw]: the first run of a row -> net = rnd(tanh(x)), the second -> inp = rnd(relu(x)).  A vector
// lies in one run (the host takes vectors only when both runs are whole vectors).
template <typename T, int W>
__global__ __launch_bounds__(ENC_THREADS) void enc_context_split_kernel(const T *__restrict__ x, T *__restrict__ net,
                                                                        T *__restrict__ inp, long long run_net,
                                                                        long long run_inp, unsigned chunks) {
  using VT = EncVec<T, W>;
  const unsigned e = blockIdx.x / chunks, chunk = blockIdx.x - e * chunks;
  const long long row = run_net + run_inp;
#pragma unroll
  for (int u = 0; u < ENC_UNROLL; u++) {
    const long long i = (((long long)chunk * ENC_UNROLL + u) * ENC_THREADS + threadIdx.x) * W;
    if (i >= row) continue;
    const VT v = *(const VT *)(x + (long long)e * row + i);
    VT o;
    if (i < run_net) {
#pragma unroll
      for (int j = 0; j < W; j++) o.e[j] = (T)tanhf((float)v.e[j]);
      *(VT *)(net + (long long)e * run_net + i) = o;
    } else {
#pragma unroll
      for (int j = 0; j < W; j++) o.e[j] = (T)enc_relu((float)v.e[j]);
      *(VT *)(inp + (long long)e * run_inp + (i - run_net)) = o;
    }
  }
}

}  // namespace dba

using namespace dba;

namespace {

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

int item_size(int dtype) { return dtype == DBA_F16 ? 2 : dtype == DBA_F32 ? 4 : 0; }

int pow2_ceil(int x) {
  int p = 1;
  while (p < x) p *= 2;
  return p;
}

// lanes and items per lane of a plane of n_items items of W elements (see the head of the file and include/dba_hip.h):
// vectors: lanes = pow2 >= n_items / 2 in [64, 1024], per lane the pow2 >= n_items / lanes;
// elements: lanes = pow2 >= n_items / 4 in [64, 1024], per lane the smallest of 1, 4, 16, 64 >= n_items / lanes
void enc_geometry(int n_items, bool vec, int *lanes, int *per_lane) {
  int l = pow2_ceil((n_items + (vec ? 1 : 3)) / (vec ? 2 : 4));
  l = l < WAVE ? WAVE : l > ENC_MAX_THREADS ? ENC_MAX_THREADS : l;
  const int need = (n_items + l - 1) / l;
  int v = pow2_ceil(need);
  if (!vec) v = v <= 1 ? 1 : v <= 4 ? 4 : v <= 16 ? 16 : 64;
  *lanes = l;
  *per_lane = v;
}

template <typename T, int V, int W>
int launch_norm_v(const void *x, void *out, float *stats, int planes, int hw, float eps, int relu, int lanes, hipStream_t s) {
  hipLaunchKernelGGL((enc_norm_kernel<T, V, W>), dim3(planes), dim3(lanes), 0, s, (const T *)x, (T *)out, stats, hw, eps, relu);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

template <typename T>
int launch_norm(const void *x, void *out, float *stats, int planes, int hw, float eps, int relu, hipStream_t s) {
  constexpr int W = 16 / sizeof(T);
  const bool vec = hw % W == 0 && aligned16(x) && aligned16(out);
  int lanes, v;
  enc_geometry(vec ? hw / W : hw, vec, &lanes, &v);
#define ENC_NORM_CASE(V_, W_) \
  case V_: return launch_norm_v<T, V_, W_>(x, out, stats, planes, hw, eps, relu, lanes, s)
  if (vec) {
    switch (v) {
      ENC_NORM_CASE(1, W);
      ENC_NORM_CASE(2, W);
      ENC_NORM_CASE(4, W);
      ENC_NORM_CASE(8, W);
      case 16:
        if constexpr (W == 4) return launch_norm_v<T, 16, W>(x, out, stats, planes, hw, eps, relu, lanes, s);
    }
  } else {
    switch (v) {
      ENC_NORM_CASE(1, 1);
      ENC_NORM_CASE(4, 1);
      ENC_NORM_CASE(16, 1);
      ENC_NORM_CASE(64, 1);
    }
  }
#undef ENC_NORM_CASE
  return DBA_ERR_ARG;
}

template <typename T, int V, int W>
int launch_skip_v(const void *x, const void *side, bool down, void *out, float *stats, float *stats_d, int planes, int hw,
                  float eps, int lanes, hipStream_t s) {
  constexpr int DOWN_MODE = V * W == ENC_MAX_PER_LANE ? 2 : 1;  // two full planes per lane do not fit the register file
  if (!down)
    hipLaunchKernelGGL((enc_norm_skip_kernel<T, V, W, 0>), dim3(planes), dim3(lanes), 0, s, (const T *)x, (const T *)side,
                       (T *)out, stats, stats_d, hw, eps);
  else
    hipLaunchKernelGGL((enc_norm_skip_kernel<T, V, W, DOWN_MODE>), dim3(planes), dim3(lanes), 0, s, (const T *)x,
                       (const T *)side, (T *)out, stats, stats_d, hw, eps);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

template <typename T>
int launch_skip(const void *x, const void *side, bool down, void *out, float *stats, float *stats_d, int planes, int hw,
                float eps, hipStream_t s) {
  constexpr int W = 16 / sizeof(T);
  const bool vec = hw % W == 0 && aligned16(x) && aligned16(side) && aligned16(out);
  int lanes, v;
  enc_geometry(vec ? hw / W : hw, vec, &lanes, &v);
#define ENC_SKIP_CASE(V_, W_) \
  case V_: return launch_skip_v<T, V_, W_>(x, side, down, out, stats, stats_d, planes, hw, eps, lanes, s)
  if (vec) {
    switch (v) {
      ENC_SKIP_CASE(1, W);
      ENC_SKIP_CASE(2, W);
      ENC_SKIP_CASE(4, W);
      ENC_SKIP_CASE(8, W);
      case 16:
        if constexpr (W == 4) return launch_skip_v<T, 16, W>(x, side, down, out, stats, stats_d, planes, hw, eps, lanes, s);
    }
  } else {
    switch (v) {
      ENC_SKIP_CASE(1, 1);
      ENC_SKIP_CASE(4, 1);
      ENC_SKIP_CASE(16, 1);
      ENC_SKIP_CASE(64, 1);
    }
  }
#undef ENC_SKIP_CASE
  return DBA_ERR_ARG;
}

template <typename T>
int launch_relu_skip(const void *x, const void *skip, void *out, long long count, hipStream_t s) {
  constexpr int W = 16 / sizeof(T);
  const bool vec = count % W == 0 && aligned16(x) && aligned16(skip) && aligned16(out);
  const long long per = (long long)ENC_THREADS * ENC_UNROLL * (vec ? W : 1);
  const long long blocks = (count + per - 1) / per;
  if (blocks > (long long)INT32_MAX) return DBA_ERR_ARG;
  if (vec)
    hipLaunchKernelGGL((enc_relu_skip_kernel<T, W>), dim3((unsigned)blocks), dim3(ENC_THREADS), 0, s, (const T *)x,
                       (const T *)skip, (T *)out, count);
  else
    hipLaunchKernelGGL((enc_relu_skip_kernel<T, 1>), dim3((unsigned)blocks), dim3(ENC_THREADS), 0, s, (const T *)x,
                       (const T *)skip, (T *)out, count);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

template <typename S, typename D>
int launch_image(const void *img, void *out, int n, int hw, hipStream_t s) {
  // the constants of motion_filter.py:29-30 as torch.as_tensor makes them: the float32 nearest to the decimal
  const ImageConsts k = {{0.485f, 0.456f, 0.406f}, {0.229f, 0.224f, 0.225f}};
  const bool vec = hw % 4 == 0 && ((uintptr_t)img % (4 * sizeof(S))) == 0 && ((uintptr_t)out % (4 * sizeof(D))) == 0;
  const long long per = (long long)ENC_THREADS * (vec ? 4 : 1);
  const long long chunks = (hw + per - 1) / per;
  if (chunks * 3 * (long long)n > (long long)INT32_MAX) return DBA_ERR_ARG;
  const dim3 grid((unsigned)(chunks * 3 * n));
  if (vec)
    hipLaunchKernelGGL((enc_image_kernel<S, D, 4>), grid, dim3(ENC_THREADS), 0, s, (const S *)img, (D *)out, hw, (unsigned)chunks, k);
  else
    hipLaunchKernelGGL((enc_image_kernel<S, D, 1>), grid, dim3(ENC_THREADS), 0, s, (const S *)img, (D *)out, hw, (unsigned)chunks, k);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

template <typename T>
int launch_context_split(const void *x, void *net, void *inp, int n, long long run_net, long long run_inp, hipStream_t s) {
  constexpr int W = 16 / sizeof(T);
  const bool vec = run_net % W == 0 && run_inp % W == 0 && aligned16(x) && aligned16(net) && aligned16(inp);
  const long long per = (long long)ENC_THREADS * ENC_UNROLL * (vec ? W : 1);
  const long long chunks = (run_net + run_inp + per - 1) / per;
  if (chunks * (long long)n > (long long)INT32_MAX) return DBA_ERR_ARG;
  const dim3 grid((unsigned)(chunks * n));
  if (vec)
    hipLaunchKernelGGL((enc_context_split_kernel<T, W>), grid, dim3(ENC_THREADS), 0, s, (const T *)x, (T *)net, (T *)inp,
                       run_net, run_inp, (unsigned)chunks);
  else
    hipLaunchKernelGGL((enc_context_split_kernel<T, 1>), grid, dim3(ENC_THREADS), 0, s, (const T *)x, (T *)net, (T *)inp,
                       run_net, run_inp, (unsigned)chunks);
  DBA_LAUNCH_CHECK();
  return DBA_OK;
}

// a grid of 256-lane workgroups over `rows` rows of `row` elements, at best `per_lane` elements per lane, is beyond 2^31 - 1:
// asked before the overlap tests, whose byte ranges mean nothing at such extents; the launchers repeat it for their route
bool grid_beyond(long long rows, long long row, int per_lane) {
  const long long per = (long long)ENC_THREADS * per_lane;
  return (row + per - 1) / per > (long long)INT32_MAX / rows;
}

bool plane_extents_ok(int planes, int hw) { return planes > 0 && hw > 0 && hw <= ENC_MAX_PLANE; }

}  // namespace

extern "C" {

int dba_enc_norm(const void *x, int planes, int hw, float eps, int relu, int dtype, void *out, float *stats,
                 dba_stream_t stream) {
  const int isz = item_size(dtype);
  if (!isz) return DBA_ERR_UNSUPPORTED;
  if (!x || !out || !plane_extents_ok(planes, hw) || !(eps >= 0.0f)) return DBA_ERR_ARG;
  if (((uintptr_t)x | (uintptr_t)out) % isz || (stats && (uintptr_t)stats % 4)) return DBA_ERR_ARG;
  const long long bytes = (long long)planes * hw * isz, sbytes = (long long)planes * 8;
  if (out != x && ranges_overlap(out, bytes, x, bytes)) return DBA_ERR_ARG;
  if (stats && (ranges_overlap(stats, sbytes, x, bytes) || ranges_overlap(stats, sbytes, out, bytes))) return DBA_ERR_ARG;
  return dtype == DBA_F16 ? launch_norm<_Float16>(x, out, stats, planes, hw, eps, relu != 0, (hipStream_t)stream)
                          : launch_norm<float>(x, out, stats, planes, hw, eps, relu != 0, (hipStream_t)stream);
}

int dba_enc_norm_skip(const void *x, const void *skip, const void *d, int planes, int hw, float eps, int dtype, void *out,
                      float *stats, float *stats_d, dba_stream_t stream) {
  const int isz = item_size(dtype);
  if (!isz) return DBA_ERR_UNSUPPORTED;
  if (!x || !out || (skip == nullptr) == (d == nullptr) || !plane_extents_ok(planes, hw) || !(eps >= 0.0f)) return DBA_ERR_ARG;
  const void *side = skip ? skip : d;
  if (((uintptr_t)x | (uintptr_t)out | (uintptr_t)side) % isz) return DBA_ERR_ARG;
  if ((stats && (uintptr_t)stats % 4) || (stats_d && (uintptr_t)stats_d % 4)) return DBA_ERR_ARG;
  if (stats_d && !d) return DBA_ERR_ARG;
  const long long bytes = (long long)planes * hw * isz, sbytes = (long long)planes * 8;
  if (out != x && ranges_overlap(out, bytes, x, bytes)) return DBA_ERR_ARG;
  if (ranges_overlap(out, bytes, side, bytes)) return DBA_ERR_ARG;
  for (float *st : {stats, stats_d})
    if (st && (ranges_overlap(st, sbytes, x, bytes) || ranges_overlap(st, sbytes, out, bytes) || ranges_overlap(st, sbytes, side, bytes)))
      return DBA_ERR_ARG;
  if (stats && stats_d && ranges_overlap(stats, sbytes, stats_d, sbytes)) return DBA_ERR_ARG;
  return dtype == DBA_F16
             ? launch_skip<_Float16>(x, side, d != nullptr, out, stats, stats_d, planes, hw, eps, (hipStream_t)stream)
             : launch_skip<float>(x, side, d != nullptr, out, stats, stats_d, planes, hw, eps, (hipStream_t)stream);
}

int dba_enc_relu_skip(const void *x, const void *skip, long long count, int dtype, void *out, dba_stream_t stream) {
  const int isz = item_size(dtype);
  if (!isz) return DBA_ERR_UNSUPPORTED;
  if (!x || !skip || !out || count <= 0 || grid_beyond(1, count, ENC_UNROLL * (16 / isz))) return DBA_ERR_ARG;
  if (((uintptr_t)x | (uintptr_t)skip | (uintptr_t)out) % isz) return DBA_ERR_ARG;
  const long long bytes = count * isz;
  if (out != x && ranges_overlap(out, bytes, x, bytes)) return DBA_ERR_ARG;
  if (ranges_overlap(out, bytes, skip, bytes)) return DBA_ERR_ARG;
  return dtype == DBA_F16 ? launch_relu_skip<_Float16>(x, skip, out, count, (hipStream_t)stream)
                          : launch_relu_skip<float>(x, skip, out, count, (hipStream_t)stream);
}

int dba_enc_image(const void *img, int n, int H, int W, int src_dtype, int dtype, void *out, dba_stream_t stream) {
  const int isz = item_size(dtype);
  if (!isz || (src_dtype != DBA_U8 && src_dtype != DBA_F32)) return DBA_ERR_UNSUPPORTED;
  if (!img || !out || n <= 0 || H <= 0 || W <= 0 || (long long)H * W > (long long)INT32_MAX / 4) return DBA_ERR_ARG;
  const int ssz = src_dtype == DBA_U8 ? 1 : 4;
  if ((uintptr_t)img % ssz || (uintptr_t)out % isz) return DBA_ERR_ARG;
  const int hw = H * W;
  if (grid_beyond(3LL * n, hw, 4)) return DBA_ERR_ARG;
  if (ranges_overlap(out, 3LL * n * hw * isz, img, 3LL * n * hw * ssz)) return DBA_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  if (src_dtype == DBA_U8)
    return dtype == DBA_F16 ? launch_image<uint8_t, _Float16>(img, out, n, hw, s) : launch_image<uint8_t, float>(img, out, n, hw, s);
  return dtype == DBA_F16 ? launch_image<float, _Float16>(img, out, n, hw, s) : launch_image<float, float>(img, out, n, hw, s);
}

int dba_enc_context_split(const void *x, int n, int c_net, int c_inp, int hw, int dtype, void *net, void *inp,
                          dba_stream_t stream) {
  const int isz = item_size(dtype);
  if (!isz) return DBA_ERR_UNSUPPORTED;
  if (!x || !net || !inp || n <= 0 || c_net <= 0 || c_inp <= 0 || hw <= 0) return DBA_ERR_ARG;
  const long long run_net = (long long)c_net * hw, run_inp = (long long)c_inp * hw;
  if (run_net + run_inp > (long long)INT32_MAX || grid_beyond(n, run_net + run_inp, ENC_UNROLL * (16 / isz))) return DBA_ERR_ARG;
  if (((uintptr_t)x | (uintptr_t)net | (uintptr_t)inp) % isz) return DBA_ERR_ARG;
  const long long nb = run_net * n * isz, ib = run_inp * n * isz;
  if (ranges_overlap(net, nb, x, nb + ib) || ranges_overlap(inp, ib, x, nb + ib) || ranges_overlap(net, nb, inp, ib)) return DBA_ERR_ARG;
  return dtype == DBA_F16 ? launch_context_split<_Float16>(x, net, inp, n, run_net, run_inp, (hipStream_t)stream)
                          : launch_context_split<float>(x, net, inp, n, run_net, run_inp, (hipStream_t)stream);
}

}  // extern "C"
