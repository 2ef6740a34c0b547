// crf_band.hip — DCNF's CRF on fine superpixel grids (include/a3d_crf_band.h, NON-REFERENCE, --superpixel 20 / 10): the
// negative log-likelihood L = e^T A e - 1/2 log det A + (nsp / 2) log pi, e = y - A^-1 z, its gradients wrt z and the pair
// weights r, and the MAP depths A^-1 z, for up to 768 superpixels per image.  A = I + D - R of a row-major grid graph is
// banded, half bandwidth `band` = the grid's columns.  One workgroup per image; the dense A is never formed.
//
// Band storage.  S[c][d], c < nsp, 0 <= d <= band, holds the lower triangle by columns: S[c][d] = A[c + d][c].  The
// factorisation A = L D L^T (no pivoting) runs in place: step k reads column k and subtracts l_i a_j from S[k + j][i - j],
// 1 <= j <= i <= band, so the storage holds a = L D until one parallel pass divides every column by its pivot.  The
// forward solve L u = z rides along in the same steps.  mu comes from the column sweep of L^T mu = D^-1 u.  With dr the
// Takahashi recurrence then overwrites the factor, last row first, with the entries of Z = A^-1 inside the band,
// S[i][d] = Z[i][i + d]:  Z[i][j] = -sum_m L[i + m][i] Z[i + m][j] (j > i),  Z[i][i] = 1 / D_i - sum_m L[i + m][i] Z[i][i + m].
// e^T A e = sum_i D_i ((L^T e)_i)^2 is taken from the factor before that: A itself is gone by then.
//
// Row stride.  The lanes walk S along a row (S[c][d], d the lane: dwords 1 apart) and along an anti-diagonal
// (S[k - d][d] in the backward sweep, S[i + d][m - d] in the recurrence: dwords stride - 1 apart); nothing on the serial
// chain walks a column.  So the stride is the even number band + 1 or band + 2, which makes stride - 1 odd: both walks
// touch 32 different banks of the 64.  (crf.hip's tiles are walked by row and by column and have odd strides for the
// same reason.)  Only the set-up pass that adds the row sums of R walks columns, two lanes to a bank, once.
//
// Threads.  kThreads = 256: four wavefronts.  Steps k and k + 1 of all three sweeps depend on each other, so every step ends
// in a barrier, and a one-wavefront workgroup's barrier is free; but a step of the factorisation is up to 528 multiply-adds
// whose LDS round trips one wavefront takes 16 deep and four take 4 deep, and that outweighs s_barrier: measured at batch
// 16, 24 x 32, the launch without dr takes 0.94 ms with 64 threads and 0.42 ms with 256 (DESIGN.md §3.5 has both tables).
// The code is written for any multiple of 64 (-DA3DB_THREADS=64 builds the other one).
//
// LDS (dynamic, sized from the call's nsp and band): nsp x stride floats of S and two vectors of nsp floats (z / u / mu and
// y / e); static: 1056 bytes in the nll kernel (the recurrence's partial sums, the wavefronts' sums, two flags), 16 in the
// map kernel.  Dynamic bytes:
//   6 x 8   (band 8,  stride 10):  48 x 10 x 4 +  384 =   2 304 bytes
//   12 x 16 (band 16, stride 18): 192 x 18 x 4 + 1536 =  15 360 bytes
//   24 x 32 (band 32, stride 34): 768 x 34 x 4 + 6144 = 110 592 bytes      (the maxima; 160 KiB per CU: one workgroup)
// crf_band_posterior_kernel (include/a3d_posterior.h) adds a third vector (the observed flags): 2 496, 16 128 and 113 664
// bytes, 1 040 static.
// Compiler's resource report for gfx950 (-Rpass-analysis=kernel-resource-usage): crf_band_kernel<false> (nll) 48 VGPRs,
// crf_band_kernel<true> (map) 28 VGPRs, crf_band_posterior_kernel 40 VGPRs, mean_kernel (crf_common.h) 7 VGPRs; scratch
// 0 bytes, no spills in all four.
//
// Every loop bound is a function of nsp, band, npairs and the thread alone; no trip count, branch or index depends on a
// value of z, y or r.  A bad pivot turns values into NaN or inf and nothing else.  Indices into S: a column c < nsp with an
// offset d <= band (c = k + j <= k + w, w = min(band, nsp - 1 - k); c = k - d >= 0 is tested); a pair's cell only after
// both of its indices were checked against [0, nsp) and their distance against band.  No spin waits, nothing between
// workgroups, no float atomics: the only atomics are an integer max in LDS that finds the last writer of a cell and, in the
// posterior kernel, an integer add in LDS that counts the observed superpixels (whose flags select values, never an index).
#include "a3d_internal.h"
#include "a3d_crf_band.h"
#include "a3d_posterior.h"
#include "crf_common.h"

#ifndef A3DB_THREADS
#define A3DB_THREADS 256
#endif

namespace a3d {
namespace {

constexpr int kThreads = A3DB_THREADS;
constexpr int kWaves = kThreads / 64;
static_assert(kThreads % 64 == 0 && kThreads >= 64 && kThreads <= 1024, "whole wavefronts");

__host__ __device__ constexpr int band_stride(int band) { return (band + 2) & ~1; }

// the sum over the workgroup in a fixed order: xor butterfly inside a wavefront, then the wavefronts in turn
__device__ __forceinline__ float band_block_sum(float v, float* red) {
  v = wave_sum_f(v);
  if (kWaves == 1) return v;
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = red[0];
  for (int i = 1; i < kWaves; ++i) s += red[i];
  __syncthreads();
  return s;
}

// ---- the sweeps, written once: crf_band_kernel<false> (nll), crf_band_kernel<true> (map) and crf_band_posterior_kernel
// call them in this order.  All are entered and left by the whole workgroup; each says which barrier it ends with.

// a pair's cell S[lo][d], or false where the pair cannot be used (an index outside [0, n), farther apart than band)
__device__ __forceinline__ bool band_pair_cell(int l, int rr, int n, int band, int& lo, int& d) {
  lo = min(l, rr), d = max(l, rr) - lo;
  return !(l < 0 || l >= n || rr < 0 || rr >= n || d > band);
}

// Si[cell] = the last writer of every cell, the largest pair number, -1 where no pair is; flags[0 .. 2) = 0, then flags[0] = 1
// if a pair cannot be used (skipped, never indexed with).  Ends with a barrier.
__device__ __forceinline__ void band_scatter(int* Si, int* flags, const int* __restrict__ left, const int* __restrict__ right,
                                             int n, int stride, int band, int npairs, int t) {
  for (int c = t; c < n * stride; c += kThreads) Si[c] = -1;
  if (t < 2) flags[t] = 0;
  __syncthreads();
  for (int q = t; q < npairs; q += kThreads) {
    int lo, d;
    if (!band_pair_cell(left[q], right[q], n, band, lo, d)) flags[0] = 1;
    else if (d > 0) atomicMax(&Si[lo * stride + d], q);
  }
  __syncthreads();
}

// -R below the diagonal (0 - r as crf.hip), +0 where no pair is; r is the image's row.  Ends with a barrier.
__device__ __forceinline__ void band_fill(float* S, const int* Si, const float* __restrict__ r, int n, int stride, int t) {
  for (int c = t; c < n * stride; c += kThreads) {
    const int q = Si[c];
    S[c] = q >= 0 ? 0.f - r[q] : 0.f;
  }
  __syncthreads();
}

// A[i][i] = 1 + the row sum of R over every stored cell, columns in ascending order.  No barrier: the caller loads its
// vectors first.
__device__ __forceinline__ void band_diagonal(float* S, int n, int stride, int band, int i) {
  float rs = 0.f;
  for (int j = max(0, i - band); j < i; ++j) rs += S[j * stride + (i - j)];
  const int w = min(band, n - 1 - i);
  for (int d = 1; d <= w; ++d) rs += S[i * stride + d];
  S[i * stride] = 1.f - rs;                      // rs = -(row sum): 1 + the row sum, bit for bit
}

// L D L^T and L u = z.  Thread (i, g): row offset i = 1 .. 32, column offsets j = 1 + g, 1 + g + G, ... <= i.  A barrier
// after every step.
__device__ __forceinline__ void band_factor_solve(float* S, float* zv, int n, int stride, int band, int t) {
  const int i = (t & 31) + 1, g = t >> 5;
  constexpr int G = kThreads / 32;
  for (int k = 0; k < n; ++k) {
    const int w = min(band, n - 1 - k);
    const float* col = S + k * stride;
    if (i <= w) {
      const float li = col[i] / col[0];
      for (int j = 1 + g; j <= i; j += G) S[(k + j) * stride + (i - j)] -= li * col[j];
      if (g == 0) zv[k + i] -= li * zv[k];
    }
    __syncthreads();
  }
}

// the pivots: flags[1] = 1 unless all are finite and > 0; L = a / D; D^-1 u; with kLogDet the sum of their logs.  Ends with
// a barrier.
template <bool kLogDet>
__device__ __forceinline__ float band_pivots(float* S, float* zv, int* flags, float* red, int n, int stride, int band, int t) {
  float ld = 0.f;
  bool ok = true;
  for (int i = t; i < n; i += kThreads) {
    const float p = S[i * stride];
    ok = ok && p > 0.f && p < INFINITY;
    if (kLogDet) ld += logf(p);
    zv[i] = zv[i] / p;
  }
  for (int c = t; c < n * stride; c += kThreads) {
    const int row = c / stride, d = c - row * stride;
    if (d >= 1 && d <= band) S[c] = S[c] / S[row * stride];
  }
  if (!ok) flags[1] = 1;
  if (kLogDet) ld = band_block_sum(ld, red);
  __syncthreads();
  return ld;
}

// L^T mu = D^-1 u, column sweep: once mu_k stands, the rows above take their share.  A barrier after every step.
__device__ __forceinline__ void band_column_sweep(const float* S, float* zv, int n, int stride, int band, int t) {
  for (int k = n - 1; k > 0; --k) {
    const int d = t + 1;
    if (d <= band && k - d >= 0) zv[k - d] -= S[(k - d) * stride + d] * zv[k];
    __syncthreads();
  }
}

// flags[1] = 1 if a component of zv is not finite.  Ends with a barrier.
__device__ __forceinline__ void band_check_finite(const float* zv, int* flags, int n, int t) {
  bool fin = true;
  for (int i = t; i < n; i += kThreads) fin = fin && isfinite(zv[i]);
  if (!fin) flags[1] = 1;
  __syncthreads();
}

// Takahashi: row i of Z over the slot of column i of L.  Thread (d, g): the terms m = 1 + g, 1 + g + G, ... of the entry
// Z[i][i + d]; the G partial sums meet in LDS (part [kThreads]) and the first 32 threads add them in the order of g.
// Entered after a barrier; a barrier after every row.
__device__ __forceinline__ void band_takahashi(float* S, float* part, int n, int stride, int band, int t) {
  for (int i = n - 1; i >= 0; --i) {
    constexpr int G = kThreads / 32;
    const int w = min(band, n - 1 - i), d = (t & 31) + 1, g = t >> 5;
    const float* col = S + i * stride;
    float acc = 0.f;
    if (d <= w)
      for (int m = 1 + g; m <= w; m += G) {
        const float zz = m <= d ? S[(i + m) * stride + (d - m)] : S[(i + d) * stride + (m - d)];
        acc += col[m] * zz;
      }
    part[t] = acc;
    const float ld_ = (g == 0 && d <= w) ? col[d] : 0.f, dinv = 1.f / col[0];
    __syncthreads();                             // column i of L has been read, the partial sums stand
    if (g == 0) {                                // one half of the first wavefront; the other half adds zeros
      float sum = part[t];
      for (int k = 1; k < G; ++k) sum += part[k * 32 + t];
      const float zij = 0.f - sum;
      float s = ld_ * zij;
#pragma unroll
      for (int off = 16; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
      if (d <= w) S[i * stride + d] = zij;
      if (t == 0) S[i * stride] = dinv - s;
    }
    __syncthreads();
  }
}

// kMap: mu and status alone (y, loss_img, dz, dr are not touched).
template <bool kMap>
__global__ __launch_bounds__(kThreads) void crf_band_kernel(const float* __restrict__ z, const float* __restrict__ y,
                                                            const float* __restrict__ r, const int* __restrict__ left,
                                                            const int* __restrict__ right, float* __restrict__ loss_img,
                                                            float* __restrict__ dz, float* dr, float* __restrict__ mu,
                                                            int* __restrict__ status, int n, int band, int npairs,
                                                            float inv_batch) {
  extern __shared__ __attribute__((aligned(16))) float band_smem[];
  __shared__ float red[kWaves > 1 ? kWaves : 1];
  __shared__ float part[kThreads];               // the recurrence's partial sums, [kThreads / 32][32]
  __shared__ int flags[2];                       // [0]: a pair that cannot be used; [1]: a pivot or a value that is not accepted
  const int stride = band_stride(band);
  float* S = band_smem;                          // [n][stride]
  int* Si = reinterpret_cast<int*>(band_smem);
  float* zv = S + n * stride;                    // z, then u (L u = z), then D^-1 u, then mu
  float* ev = zv + n;                            // y, then e = y - mu
  const int b = blockIdx.x, t = threadIdx.x;
  const float nanf_ = __builtin_nanf("");
  const bool want_dr = !kMap && dr != nullptr;

  band_scatter(Si, flags, left, right, n, stride, band, npairs, t);
  const bool bad = flags[0] != 0;                // the index lists are the batch's: every image ends as NaN
  if (want_dr) {                                 // park "this pair owns its cell" in dr; each thread reads back its own
    for (int q = t; q < npairs; q += kThreads) {
      int lo, d;
      const bool usable = band_pair_cell(left[q], right[q], n, band, lo, d) && d > 0;
      dr[(size_t)b * npairs + q] = (usable && Si[lo * stride + d] == q) ? 1.f : 0.f;
    }
    __syncthreads();
  }
  band_fill(S, Si, r + (size_t)b * npairs, n, stride, t);
  for (int i = t; i < n; i += kThreads) {
    band_diagonal(S, n, stride, band, i);
    zv[i] = z[(size_t)b * n + i];
    if (!kMap) ev[i] = y[(size_t)b * n + i];
  }
  __syncthreads();

  band_factor_solve(S, zv, n, stride, band, t);
  const float ld = band_pivots<true>(S, zv, flags, red, n, stride, band, t);
  band_column_sweep(S, zv, n, stride, band, t);
  if (kMap) {
    band_check_finite(zv, flags, n, t);
    const bool nan_row = bad || flags[1] != 0;
    for (int i = t; i < n; i += kThreads) mu[(size_t)b * n + i] = nan_row ? nanf_ : zv[i];
    if (t == 0) status[b] = nan_row ? 1 : 0;
    return;
  }
  for (int i = t; i < n; i += kThreads) ev[i] = ev[i] - zv[i];
  __syncthreads();
  float qf = 0.f;                                // e^T A e = sum_i D_i ((L^T e)_i)^2
  for (int i = t; i < n; i += kThreads) {
    const int w = min(band, n - 1 - i);
    float s = ev[i];
    for (int d = 1; d <= w; ++d) s += S[i * stride + d] * ev[i + d];
    qf += S[i * stride] * (s * s);
  }
  qf = band_block_sum(qf, red);
  const float loss = (qf - 0.5f * ld) + (float)n * kHalfLogPi;
  const bool nan_row = bad || flags[1] != 0 || !isfinite(loss);
  if (t == 0) {
    loss_img[b] = nan_row ? nanf_ : loss;
    status[b] = nan_row ? 1 : 0;
  }
  for (int i = t; i < n; i += kThreads) {
    dz[(size_t)b * n + i] = nan_row ? nanf_ : (-2.f * ev[i]) * inv_batch;
    if (mu) mu[(size_t)b * n + i] = nan_row ? nanf_ : zv[i];
  }
  if (!want_dr) return;
  __syncthreads();
  band_takahashi(S, part, n, stride, band, t);
  for (int q = t; q < npairs; q += kThreads) {
    const size_t o = (size_t)b * npairs + q;
    const bool own = dr[o] != 0.f;
    float v = nanf_;
    if (!nan_row) {                              // not bad: an owner's l and rr are inside [0, n), 0 < |l - rr| <= band
      v = 0.f;
      if (own) {
        const int l = left[q], rr = right[q];
        const int lo = min(l, rr), d = max(l, rr) - lo;
        const float zlr = S[lo * stride + d];
        const float s_a = ((S[l * stride] + S[rr * stride]) - zlr) - zlr;
        const float vq = ev[l] - ev[rr], vm = zv[l] - zv[rr];
        v = (((2.f * vq) * vm + vq * vq) - 0.5f * s_a) * inv_batch;
      }
    }
    dr[o] = v;
  }
}

// The field's posterior given the superpixels whose y is finite (include/a3d_posterior.h): the same sweeps on A', which is
// A with every observed row and column replaced by the identity's.  The scatter, the -R cells and the diagonal are the map
// kernel's, over every stored cell; only then one pass builds the right-hand side (z_i + sum over observed neighbours of
// r_ij y_j on a missing i, 0 on an observed one) and a second drops the cells with an observed end and sets the observed
// diagonals to 1.  With nothing observed both passes change no bit and the solution is crf_band_kernel<true>'s.  A' has A's
// band and is positive definite where A is; its inverse on the missing superpixels is that of A_MM, so the recurrence's
// diagonal is twice the conditional variance.  The mask is data, but it only selects between values: no trip count, branch
// target or index depends on it.  LDS: S and three vectors of n (rhs / solution, y, the observed flags).
__global__ __launch_bounds__(kThreads) void crf_band_posterior_kernel(const float* __restrict__ z, const float* __restrict__ y,
                                                                      const float* __restrict__ r,
                                                                      const int* __restrict__ left,
                                                                      const int* __restrict__ right, float* __restrict__ mean,
                                                                      float* __restrict__ var, int* __restrict__ nobs,
                                                                      int* __restrict__ status, int n, int band, int npairs) {
  extern __shared__ __attribute__((aligned(16))) float band_smem[];
  __shared__ float red[kWaves > 1 ? kWaves : 1];
  __shared__ float part[kThreads];
  __shared__ int flags[2];                       // as crf_band_kernel's
  __shared__ int seen;                           // the number of observed superpixels
  const int stride = band_stride(band);
  float* S = band_smem;
  int* Si = reinterpret_cast<int*>(band_smem);
  float* zv = S + n * stride;                    // z, then the right-hand side of A', then its solution
  float* yv = zv + n;                            // y (NaN without y)
  int* ov = reinterpret_cast<int*>(yv + n);      // 1 where the superpixel is observed
  const int b = blockIdx.x, t = threadIdx.x;
  const float nanf_ = __builtin_nanf("");

  if (t == 0) seen = 0;
  band_scatter(Si, flags, left, right, n, stride, band, npairs, t);
  const bool bad = flags[0] != 0;
  band_fill(S, Si, r + (size_t)b * npairs, n, stride, t);
  int mine = 0;
  for (int i = t; i < n; i += kThreads) {
    band_diagonal(S, n, stride, band, i);
    zv[i] = z[(size_t)b * n + i];
    const float yi = y ? y[(size_t)b * n + i] : nanf_;
    const int o = isfinite(yi) ? 1 : 0;
    yv[i] = yi;
    ov[i] = o;
    mine += o;
  }
  if (mine) atomicAdd(&seen, mine);              // an integer sum: any order gives the same count
  __syncthreads();
  for (int i = t; i < n; i += kThreads) {        // the right-hand side: the cells -r of the observed neighbours, columns ascending
    float acc = zv[i];
    for (int j = max(0, i - band); j < i; ++j) {
      const float c = S[j * stride + (i - j)], yj = yv[j];
      acc -= ov[j] ? c * yj : 0.f;
    }
    const int w = min(band, n - 1 - i);
    for (int d = 1; d <= w; ++d) {
      const float c = S[i * stride + d], yj = yv[i + d];
      acc -= ov[i + d] ? c * yj : 0.f;
    }
    zv[i] = ov[i] ? 0.f : acc;
  }
  __syncthreads();
  for (int c = t; c < n * stride; c += kThreads) {      // A -> A'
    const int row = c / stride, d = c - row * stride;
    if (d == 0) {
      if (ov[row]) S[c] = 1.f;
    } else if (d <= band && row + d < n) {
      if (ov[row] | ov[row + d]) S[c] = 0.f;
    }
  }
  __syncthreads();

  band_factor_solve(S, zv, n, stride, band, t);
  band_pivots<false>(S, zv, flags, red, n, stride, band, t);
  band_column_sweep(S, zv, n, stride, band, t);
  band_check_finite(zv, flags, n, t);
  if (var) {
    band_takahashi(S, part, n, stride, band, t);
    bool ok = true;
    for (int i = t; i < n; i += kThreads) {
      const float v = 0.5f * S[i * stride];
      ok = ok && (ov[i] || (v > 0.f && v < INFINITY));
    }
    if (!ok) flags[1] = 1;
    __syncthreads();
  }
  const bool nan_row = bad || flags[1] != 0;
  for (int i = t; i < n; i += kThreads) {
    const bool o = ov[i] != 0;
    mean[(size_t)b * n + i] = nan_row ? nanf_ : (o ? yv[i] : zv[i]);
    if (var) var[(size_t)b * n + i] = nan_row ? nanf_ : (o ? 0.f : 0.5f * S[i * stride]);
  }
  if (t == 0) {
    nobs[b] = seen;
    status[b] = nan_row ? 1 : 0;
  }
}

// dynamic LDS: the band storage and `vectors` vectors of nsp floats (two in crf_band_kernel, three in the posterior's)
constexpr size_t band_lds_bytes(int nsp, int band, int vectors) {
  return ((size_t)nsp * band_stride(band) + (size_t)vectors * nsp) * sizeof(float);
}
static_assert(band_lds_bytes(A3DB_MAX_SP, A3DB_MAX_BAND, 3) == 113664 &&
                  band_lds_bytes(A3DB_MAX_SP, A3DB_MAX_BAND, 3) + 2048 <= 160 * 1024,
              "the maxima fit one CU's LDS");

// above 64 KiB of dynamic LDS: the attribute is per device and cheap, set on every call that needs it
template <typename Kernel>
bool band_allow_lds(Kernel kernel, size_t lds, int vectors) {
  return lds <= 64 * 1024 ||
         hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)band_lds_bytes(A3DB_MAX_SP, A3DB_MAX_BAND, vectors)) == hipSuccess;
}

template <bool kMap>
int band_launch(int n, int nsp, int band, const float* z, const float* y, const float* r, const int32_t* left,
                const int32_t* right, int npairs, float* loss_per_image, float* dz, float* dr, float* mu, int32_t* status,
                hipStream_t st, const char* what) {
  const size_t lds = band_lds_bytes(nsp, band, 2);
  if (!band_allow_lds(&crf_band_kernel<kMap>, lds, 2)) return set_error(A3D_ELAUNCH, "%s: hipFuncSetAttribute failed", what);
  clear_stale_error();
  hipLaunchKernelGGL(crf_band_kernel<kMap>, dim3(n), dim3(kThreads), lds, st, z, y, r, left, right, loss_per_image, dz, dr,
                     mu, status, nsp, band, npairs, 1.0f / (float)n);
  return check_launch(what);
}

}  // namespace
}  // namespace a3d

using namespace a3d;

extern "C" {

int a3db_crf_band_nll(int n, int nsp, int band, const float* z, const float* y, const float* r, const int32_t* left,
                      const int32_t* right, int npairs, float* loss_per_image, float* loss_mean, float* dz, float* dr,
                      float* mu, int32_t* status, void* stream) {
  A3D_CHECK_ARG(n > 0 && nsp >= 1 && nsp <= A3DB_MAX_SP && band >= 1 && band <= A3DB_MAX_BAND && npairs > 0 && z && y && r &&
                    left && right && loss_per_image && loss_mean && dz && status,
                "crf_band_nll: bad arguments (1 .. %d superpixels, band 1 .. %d)", A3DB_MAX_SP, A3DB_MAX_BAND);
  hipStream_t st = static_cast<hipStream_t>(stream);
  int rc = band_launch<false>(n, nsp, band, z, y, r, left, right, npairs, loss_per_image, dz, dr, mu, status, st,
                              "crf_band_nll");
  if (rc != A3D_OK) return rc;
  clear_stale_error();
  hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(64), 0, st, loss_per_image, n, loss_mean);
  return check_launch("crf_band_nll_mean");
}

int a3db_crf_band_map(int n, int nsp, int band, const float* z, const float* r, const int32_t* left, const int32_t* right,
                      int npairs, float* mu, int32_t* status, void* stream) {
  A3D_CHECK_ARG(n > 0 && nsp >= 1 && nsp <= A3DB_MAX_SP && band >= 1 && band <= A3DB_MAX_BAND && npairs > 0 && z && r && left &&
                    right && mu && status,
                "crf_band_map: bad arguments (1 .. %d superpixels, band 1 .. %d)", A3DB_MAX_SP, A3DB_MAX_BAND);
  return band_launch<true>(n, nsp, band, z, nullptr, r, left, right, npairs, nullptr, nullptr, nullptr, mu, status,
                           static_cast<hipStream_t>(stream), "crf_band_map");
}

int a3dc_crf_band_posterior(int n, int nsp, int band, const float* z, const float* y, const float* r, const int32_t* left,
                            const int32_t* right, int npairs, float* mean, float* var, int32_t* nobs, int32_t* status,
                            void* stream) {
  A3D_CHECK_ARG(n > 0 && nsp >= 1 && nsp <= A3DB_MAX_SP && band >= 1 && band <= A3DB_MAX_BAND && npairs > 0 && z && r && left &&
                    right && mean && nobs && status,
                "crf_band_posterior: bad arguments (1 .. %d superpixels, band 1 .. %d)", A3DB_MAX_SP, A3DB_MAX_BAND);
  const size_t lds = band_lds_bytes(nsp, band, 3);
  if (!band_allow_lds(&crf_band_posterior_kernel, lds, 3))
    return set_error(A3D_ELAUNCH, "crf_band_posterior: hipFuncSetAttribute failed");
  clear_stale_error();
  hipLaunchKernelGGL(crf_band_posterior_kernel, dim3(n), dim3(kThreads), lds, static_cast<hipStream_t>(stream), z, y, r, left,
                     right, mean, var, nobs, status, nsp, band, npairs);
  return check_launch("crf_band_posterior");
}

}  // extern "C"
