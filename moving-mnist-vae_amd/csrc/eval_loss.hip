// Held-out evaluation kernels: the per-image terms of the ELBO and the importance-weighted bound.  Every output is f64 [rows],
// WRITTEN (not accumulated) by one 256-thread block per image: each thread adds its strided elements into an f64 register in a
// fixed order, the four wave sums (a fixed shuffle tree) meet in LDS and thread 0 adds them in wave order.  No atomics: the bits
// depend on the inputs (and, for the Gaussian term, on the rows' alignment) only.  The per-element arithmetic is that of the
// batch sums in latent_loss.hip, so an image's term is what it contributes to VAE.loss.
#include "kernels.hpp"

namespace mmvae {

// Sum over the block; the total is returned in thread 0 (other threads: unspecified).  Ends with no barrier: call it once per kernel,
// or put a __syncthreads() between two calls.
__device__ __forceinline__ double image_sum(double v) {
  __shared__ double sred[4];
  v = wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sred[0] + sred[1]) + (sred[2] + sred[3]);
}
__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// ---------------------------------------------------------------- Gaussian NLL per image (model.py:403)
// Rows start at r + n * per with `per` odd in general (S = 9: 81), so a row is 4-byte aligned and no more.  16-byte loads run from
// the row's first 16-byte boundary on, and only when target's row sits at the same offset from one (same_phase, checked per row);
// the <= 3 elements in front and the <= 3 behind the last whole float4 are read one by one.  Otherwise the whole row is.
__global__ __launch_bounds__(256) void gauss_nll_image_kernel(const float* __restrict__ r, const float* __restrict__ t, long per, float inv2var,
                                                              float cst, double* __restrict__ out) {
  const float* rp = r + (long)blockIdx.x * per;
  const float* tp = t + (long)blockIdx.x * per;
  const uintptr_t ra = reinterpret_cast<uintptr_t>(rp), ta = reinterpret_cast<uintptr_t>(tp);
  const bool same_phase = (ra & 15) == (ta & 15);
  long head = same_phase ? (long)(((16 - (ra & 15)) & 15) >> 2) : per;      // (float pointers: ra is a multiple of 4)
  if (head > per) head = per;
  const long n4 = (per - head) >> 2;
  const long tail = head + (n4 << 2);
  double acc = 0.0;
  const float4* r4 = reinterpret_cast<const float4*>(rp + head);
  const float4* t4 = reinterpret_cast<const float4*>(tp + head);
  for (long i = threadIdx.x; i < n4; i += 256) {
    const float4 a = r4[i], b = t4[i];
    const float d0 = b.x - a.x, d1 = b.y - a.y, d2 = b.z - a.z, d3 = b.w - a.w;
    acc += ((double)(d0 * d0) + (double)(d1 * d1)) + ((double)(d2 * d2) + (double)(d3 * d3));
  }
  for (long i = threadIdx.x; i < head; i += 256) { const float d = tp[i] - rp[i]; acc += (double)(d * d); }
  for (long i = tail + threadIdx.x; i < per; i += 256) { const float d = tp[i] - rp[i]; acc += (double)(d * d); }
  const double s = image_sum(acc);
  if (threadIdx.x == 0) out[blockIdx.x] = s * (double)inv2var + (double)cst * (double)per;
}
int launch_gauss_nll_per_image(const float* r, const float* t, int N, long per, float sigma, double* out, hipStream_t s) {
  const float var = sigma * sigma;
  const float cst = logf(sigma) + (float)log(sqrt(2.0 * 3.14159265358979323846));      // as launch_gauss_nll_fwd
  hipLaunchKernelGGL(gauss_nll_image_kernel, dim3(N), dim3(256), 0, s, r, t, per, 1.0f / (2.0f * var), cst, out);
  return check_launch("gauss_nll_per_image");
}

// ---------------------------------------------------------------- weighted cross entropy per image (model.py:400-401)
// ce_kernel's pixel arithmetic (max-subtracted log-sum-exp); a thread's pixels are HW-strided planes apart, consecutive threads read
// consecutive pixels.
__global__ __launch_bounds__(256) void ce_image_kernel(const float* __restrict__ r, const long long* __restrict__ t, const float* __restrict__ w,
                                                       int Q, int HW, double* __restrict__ out) {
  const float* rn = r + (long)blockIdx.x * Q * HW;
  const long long* tn = t + (long)blockIdx.x * HW;
  double acc = 0.0;
  for (int p = threadIdx.x; p < HW; p += 256) {
    const float* rp = rn + p;
    const int tg = (int)tn[p];
    float mx = rp[0];
    for (int q = 1; q < Q; ++q) mx = fmaxf(mx, rp[(long)q * HW]);
    float se = 0.f;
    for (int q = 0; q < Q; ++q) se += expf(rp[(long)q * HW] - mx);
    const float lse = logf(se);
    const float wt = w ? w[tg] : 1.f;
    acc += (double)(wt * (lse - (rp[(long)tg * HW] - mx)));
  }
  const double s = image_sum(acc);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}
int launch_ce_per_image(const float* r, const long long* t, const float* w, int N, int Q, int HW, double* out, hipStream_t s) {
  hipLaunchKernelGGL(ce_image_kernel, dim3(N), dim3(256), 0, s, r, t, w, Q, HW, out);
  return check_launch("ce_per_image");
}

// ---------------------------------------------------------------- KL per image (model.py:364-365)
__global__ __launch_bounds__(256) void kl_image_kernel(const float* __restrict__ mu, const float* __restrict__ lv, int d, double* __restrict__ out) {
  const long base = (long)blockIdx.x * d;
  double acc = 0.0;
  for (int i = threadIdx.x; i < d; i += 256) {
    const float l = lv[base + i], m = mu[base + i];
    acc += (double)(l - expf(l) - m * m + 1.0f);       // kl_fwd_kernel's term
  }
  const double s = image_sum(acc);
  if (threadIdx.x == 0) out[blockIdx.x] = -0.5 * s;
}
int launch_kl_per_image(const float* mu, const float* lv, int N, int d, double* out, hipStream_t s) {
  hipLaunchKernelGGL(kl_image_kernel, dim3(N), dim3(256), 0, s, mu, lv, d, out);
  return check_launch("kl_per_image");
}

// ---------------------------------------------------------------- log p(z) - log q(z|x) per image
// With z = mu + exp(lv/2) eps: log q = sum -0.5 (eps^2 + lv + log 2pi), log p = sum -0.5 (z^2 + log 2pi); the constants cancel.
// z is rsample_fwd_kernel's f32 expression (the code the decoder is fed); from there on the term is formed in f64.
__global__ __launch_bounds__(256) void latent_logratio_kernel(const float* __restrict__ mu, const float* __restrict__ lv, const float* __restrict__ eps,
                                                              int d, double* __restrict__ out) {
  const long base = (long)blockIdx.x * d;
  double acc = 0.0;
  for (int k = threadIdx.x; k < d; k += 256) {
    const long i = base + k;
    const float z = mu[i] + eps[i] * expf(lv[i] * 0.5f);
    const double zd = (double)z, ed = (double)eps[i];
    acc += (zd * zd - ed * ed) - (double)lv[i];
  }
  const double s = image_sum(acc);
  if (threadIdx.x == 0) out[blockIdx.x] = -0.5 * s;
}
int launch_latent_logratio(const float* mu, const float* lv, const float* eps, int N, int d, double* out, hipStream_t s) {
  hipLaunchKernelGGL(latent_logratio_kernel, dim3(N), dim3(256), 0, s, mu, lv, eps, d, out);
  return check_launch("latent_logratio");
}

// ---------------------------------------------------------------- importance-weighted bound
// out[n] = log (1/K) sum_k exp(w_k), w_k = logratio[k][n] - nll[k][n], all in f64.  The block's maximum is subtracted before any
// exponential (one sample hundreds of nats ahead of the others leaves the rest at exp(-800) = 0, not the leader at inf); K = 1:
// exp(0) = 1, log 1 = 0 and log K = 0, so the row itself comes back to the last bit.  A maximum of +-inf is returned as it is.
__global__ __launch_bounds__(256) void iw_bound_kernel(const double* __restrict__ nll, const double* __restrict__ lr, int K, int N,
                                                       double* __restrict__ out) {
  __shared__ double smax[4];
  const int n = blockIdx.x;
  double mx = -INFINITY;
  for (int k = threadIdx.x; k < K; k += 256) mx = fmax(mx, lr[(long)k * N + n] - nll[(long)k * N + n]);
  mx = wave_max_d(mx);
  if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = mx;
  __syncthreads();
  mx = fmax(fmax(smax[0], smax[1]), fmax(smax[2], smax[3]));
  double acc = 0.0;
  if (!isinf(mx))
    for (int k = threadIdx.x; k < K; k += 256) acc += exp((lr[(long)k * N + n] - nll[(long)k * N + n]) - mx);
  const double s = image_sum(acc);
  if (threadIdx.x == 0) out[n] = isinf(mx) ? mx : (mx + log(s)) - log((double)K);
}
int launch_iw_bound(const double* nll, const double* logratio, int K, int N, double* out, hipStream_t s) {
  hipLaunchKernelGGL(iw_bound_kernel, dim3(N), dim3(256), 0, s, nll, logratio, K, N, out);
  return check_launch("iw_bound");
}

}  // namespace mmvae
