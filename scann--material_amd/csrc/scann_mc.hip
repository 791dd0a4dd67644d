// Monte Carlo dropout (scann_predict_mc): the per-atom structure table the MC instantiations key their masks with, and the reduction of
// the [T, n] sample matrices to a mean and an unbiased standard deviation per column.
#include "scann_internal.h"

namespace scann {

namespace {

// one thread per atom: its structure by binary search over the offsets (atoms of a structure are contiguous)
__global__ __launch_bounds__(256) void mc_rows_kernel(const int32_t* __restrict__ mol_offset, const int32_t* __restrict__ edge_offset,
                                                      const unsigned long long* __restrict__ keys, int n_struct, int n_atom, McRow* __restrict__ rows) {
  const int a = blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= n_atom) return;
  int lo = 0, hi = n_struct - 1;  // largest s with mol_offset[s] <= a
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (mol_offset[mid] <= a) lo = mid;
    else hi = mid - 1;
  }
  const int a0 = mol_offset[lo];
  rows[a] = McRow{a0, edge_offset[a0], keys ? keys[lo] : 0ull};
}

// one thread per column: samples summed in order 0..T-1 in fp64, then the squared deviations from the mean, divided by T - 1
__global__ __launch_bounds__(256) void mc_reduce_kernel(const float* __restrict__ x, int T, int n, float* __restrict__ mean,
                                                        float* __restrict__ std_out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  double s = 0.0;
  for (int t = 0; t < T; ++t) s += (double)x[(size_t)t * n + j];
  const double m = s / T;
  double v = 0.0;
  for (int t = 0; t < T; ++t) {
    const double d = (double)x[(size_t)t * n + j] - m;
    v = fma(d, d, v);
  }
  mean[j] = (float)m;
  std_out[j] = (float)sqrt(v / (T - 1));
}

}  // namespace

void launch_mc_rows(const int32_t* mol_offset, const int32_t* edge_offset, const unsigned long long* keys, int n_struct, int n_atom, McRow* rows,
                    hipStream_t s) {
  if (n_atom <= 0 || n_struct <= 0) return;
  hipLaunchKernelGGL(mc_rows_kernel, dim3((n_atom + 255) / 256), dim3(256), 0, s, mol_offset, edge_offset, keys, n_struct, n_atom, rows);
}

void launch_mc_reduce(const float* samples, int T, int n, float* mean, float* std_out, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(mc_reduce_kernel, dim3((n + 255) / 256), dim3(256), 0, s, samples, T, n, mean, std_out);
}

}  // namespace scann
