// The ConvGRU's gate arithmetic, stated once for the streaming kernels of gru.hip and the convolution epilogues of
// conv3x3.hip.  Every statement of the reference (dbaf/modules/gru.py:27-31) yields a tensor of the input dtype T: rnd<T>
// rounds where a statement ends, everything between two roundings is float32.  Files that include this are built with
// -ffp-contract=off.  expf, tanhf and the division are the library forms (gru.hip's header says why).
#pragma once
#include <hip/hip_runtime.h>

namespace dba {

template <typename T>
__device__ __forceinline__ float rnd(float x) { return (float)(T)x; }  // the end of a statement: round to the tensor dtype

__device__ __forceinline__ float sigmoid_f32(float x) { return 1.0f / (1.0f + expf(-x)); }

// rnd(sigmoid(rnd(c + g))): the gate z or r from a convolution output c and its per-plane term g
template <typename T>
__device__ __forceinline__ float gru_gate(float c, float g) { return rnd<T>(sigmoid_f32(rnd<T>(c + g))); }

// rnd(r * net), r = gru_gate(cr, gr): an element of r * net
template <typename T>
__device__ __forceinline__ T gru_reset_value(float cr, float gr, float net) { return (T)(gru_gate<T>(cr, gr) * net); }

// rnd(rnd(rnd(1 - z) * net) + rnd(z * q)), q = rnd(tanh(rnd(cq + gq))): an element of the new hidden state from the gate z
template <typename T>
__device__ __forceinline__ T gru_blend_value(float z, float cq, float gq, float net) {
  const float q = rnd<T>(tanhf(rnd<T>(cq + gq)));
  const float keep = rnd<T>(rnd<T>(1.0f - z) * net);
  return (T)(keep + rnd<T>(z * q));
}

}  // namespace dba
