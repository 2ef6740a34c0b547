// crf.hip — the pairwise part and the CRF negative log-likelihood of ann3depth's DCNF model
// (src/models.py:20-48,91-177): 40x40 "superpixel" statistics, pair similarities, the 48x48 system A = I + D - R per
// image (LU with partial pivoting in LDS, one wavefront per image), the loss and its gradient wrt the unary output z;
// and, for evaluation, the field's MAP depths A^-1 z (crf_map_kernel), which the reference never forms.
// A is a constant for the gradient: TF 1.3 registers no gradient for scatter_nd_update (oracle/dcnf.py states the
// assumption).  All of it is tiny next to the unary conv stack; the kernels are written for clarity, not speed.
// The three one-wavefront kernels over the system (loss, MAP, observed likelihood) share their steps, the device functions
// in front of crf_loss_kernel; crf_common.h holds what crf_band.hip uses as well.
// NON-REFERENCE (include/a3d_pairwise.h, --train-pairwise): the same loss kernel can also carry the identity through its
// LU and write d loss / d r, the gradient TF 1.3 lacks; pair_dense_bwd_kernel takes it to the pairwise dense layer and
// sgd_floor_kernel keeps that layer's weights >= 0 (Liu et al. 2015, eq. 9-14).  include/a3d_texture.h
// (--pairwise-texture) adds the paper's third similarity, texture disparity over local-binary-pattern histograms.
// include/a3d_crf_valid.h (--model dcnf on depth maps with holes): the superpixel mean over the measured pixels and the
// likelihood of the observed superpixels alone, the others integrated out (crf_observed_kernel).
#include <algorithm>

#include "a3d_internal.h"
#include "a3d_crf_valid.h"
#include "a3d_pairwise.h"
#include "a3d_texture.h"
#include "crf_common.h"
#include "optim_rules.h"

namespace a3d {

__device__ __forceinline__ float block_sum_256(float v, float* red) {
  v = wave_sum_f(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const float s = red[0] + red[1] + red[2] + red[3];
  __syncthreads();
  return s;
}

// mean over each sp x sp block: x [n,h,w,c] -> out [n, (h/sp)*(w/sp), c]          (reduce_mean(superpixels, axis=2))
__global__ __launch_bounds__(256) void superpixel_mean_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                              int h, int w, int c, int sp) {
  __shared__ float red[4];
  const int cols = w / sp, rows = h / sp;
  const int p = blockIdx.x % (rows * cols), b = blockIdx.x / (rows * cols);
  const int pr = p / cols, pc = p % cols;
  for (int ch = 0; ch < c; ++ch) {
    float s = 0.f;
    for (int i = threadIdx.x; i < sp * sp; i += 256) {
      const int yy = pr * sp + i / sp, xx = pc * sp + i % sp;
      s += x[(((size_t)b * h + yy) * w + xx) * c + ch];
    }
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) out[((size_t)b * rows * cols + p) * c + ch] = s / (float)(sp * sp);
  }
}

// color_histogram (src/models.py:95-100): 256 bins of r*2^24 + g*2^16 + b*2^8 over [0, 2^24)
__global__ __launch_bounds__(256) void superpixel_hist_kernel(const float* __restrict__ x, float* __restrict__ hist,
                                                              int h, int w, int sp) {
  __shared__ int bins[256];
  const int cols = w / sp, rows = h / sp;
  const int p = blockIdx.x % (rows * cols), b = blockIdx.x / (rows * cols);
  const int pr = p / cols, pc = p % cols;
  bins[threadIdx.x] = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < sp * sp; i += 256) {
    const int yy = pr * sp + i / sp, xx = pc * sp + i % sp;
    atomicAdd(&bins[colour_bin(x + (((size_t)b * h + yy) * w + xx) * 3)], 1);
  }
  __syncthreads();
  hist[((size_t)b * rows * cols + p) * 256 + threadIdx.x] = (float)bins[threadIdx.x];
}

// NON-REFERENCE (include/a3d_texture.h, --pairwise-texture): local-binary-pattern histogram of every superpixel, the
// texture observation of Liu et al. 2015.  One block per (image, superpixel).  The (sp + 2)^2 grey values of the block
// and its one-pixel halo are staged in LDS once: the halo comes from the IMAGE (the neighbouring superpixels) and is
// clamped at the image border, where a clamped neighbour can be the pixel itself.  Bit k of a pixel's code is set iff
// neighbour k >= centre (false with a NaN on either side, true for -0 >= +0); the code is the bin.  Integer LDS
// atomics: the counts do not depend on the order.  Every global index is clamped into the image, every tile index is
// below (sp + 2)^2 <= kLbpTile.
constexpr int kMaxTextureSp = A3DT_MAX_SP;
constexpr int kLbpTile = (kMaxTextureSp + 2) * (kMaxTextureSp + 2);      // 3025 floats = 12100 bytes of LDS
__global__ __launch_bounds__(256) void superpixel_lbp_hist_kernel(const float* __restrict__ x, float* __restrict__ hist,
                                                                  int h, int w, int sp) {
  __shared__ float tile[kLbpTile];
  __shared__ int bins[256];
  const int cols = w / sp, rows = h / sp;
  const int p = blockIdx.x % (rows * cols), b = blockIdx.x / (rows * cols);
  const int y0 = (p / cols) * sp - 1, x0 = (p % cols) * sp - 1;      // the tile's corner in the image, halo included
  const int tw = sp + 2;
  bins[threadIdx.x] = 0;
  for (int i = threadIdx.x; i < tw * tw; i += 256) {
    const int yy = min(max(y0 + i / tw, 0), h - 1), xx = min(max(x0 + i % tw, 0), w - 1);
    const float* px = x + (((size_t)b * h + yy) * w + xx) * 3;
    tile[i] = (px[0] + px[1] + px[2]) / 3.f;                          // pair_similarity_kernel's grey value
  }
  __syncthreads();
  for (int i = threadIdx.x; i < sp * sp; i += 256) {
    const float* c = tile + (i / sp + 1) * tw + i % sp + 1;
    const float g = c[0];
    const int code = (c[-tw - 1] >= g ? 1 : 0) | (c[-tw] >= g ? 2 : 0) | (c[-tw + 1] >= g ? 4 : 0) | (c[1] >= g ? 8 : 0) |
                     (c[tw + 1] >= g ? 16 : 0) | (c[tw] >= g ? 32 : 0) | (c[tw - 1] >= g ? 64 : 0) | (c[-1] >= g ? 128 : 0);
    atomicAdd(&bins[code], 1);
  }
  __syncthreads();
  hist[((size_t)b * rows * cols + p) * 256 + threadIdx.x] = (float)bins[threadIdx.x];
}

// similarity() of the feature kinds for one (image, pair) + the pairwise dense layer (K -> 1).  K = 2: colour and
// colour histogram, the reference's (a3d_pair_similarity).  K = 3 (a3dt_pair_similarity3, NON-REFERENCE) adds the texture
// similarity from the LBP histograms `lbp`, the distance of the two frequency histograms; the first two similarities
// come from the same operations in the same order in both.  A pair with an index outside [0, nsp) gets NaN
// similarities and a NaN r in every image; the other pairs do not notice.
template <int K>
__global__ __launch_bounds__(256) void pair_similarity_kernel(const float* __restrict__ x, const float* __restrict__ hist,
                                                              const float* __restrict__ lbp,
                                                              const int* __restrict__ left, const int* __restrict__ right,
                                                              const float* __restrict__ dw, const float* __restrict__ db,
                                                              float* __restrict__ sims, float* __restrict__ r, int h,
                                                              int w, int sp, int npairs, float gamma) {
  static_assert(K == 2 || K == 3, "two or three similarities per pair");
  __shared__ float red[4];
  const int cols = w / sp, nsp = (h / sp) * cols;
  const int q = blockIdx.x % npairs, b = blockIdx.x / npairs;
  const int pl = left[q], pr = right[q];
  if (pl < 0 || pl >= nsp || pr < 0 || pr >= nsp) {       // the whole block: nothing is indexed with a bad superpixel
    if (threadIdx.x == 0) {
      const size_t o = (size_t)b * npairs + q;
      for (int j = 0; j < K; ++j) sims[K * o + j] = __builtin_nanf("");
      r[o] = __builtin_nanf("");
    }
    return;
  }
  float sc = 0.f;
  for (int i = threadIdx.x; i < sp * sp; i += 256) {
    const int dy = i / sp, dx = i % sp;
    const float* a = x + (((size_t)b * h + (pl / cols) * sp + dy) * w + (pl % cols) * sp + dx) * 3;
    const float* c = x + (((size_t)b * h + (pr / cols) * sp + dy) * w + (pr % cols) * sp + dx) * 3;
    const float ga = (a[0] + a[1] + a[2]) / 3.f, gc = (c[0] + c[1] + c[2]) / 3.f;     // reduce_mean over channels
    const float d = ga - gc;
    sc += d * d;
  }
  sc = block_sum_256(sc, red);
  const float* hl = hist + ((size_t)b * nsp + pl) * 256;
  const float* hr = hist + ((size_t)b * nsp + pr) * 256;
  const float dh = hl[threadIdx.x] - hr[threadIdx.x];
  const float sh = block_sum_256(dh * dh, red);
  float st = 0.f;
  if (K == 3) {                                           // integer counts, S_t < 2^24: exact in any order
    const float dt = lbp[((size_t)b * nsp + pl) * 256 + threadIdx.x] - lbp[((size_t)b * nsp + pr) * 256 + threadIdx.x];
    st = block_sum_256(dt * dt, red);
  }
  if (threadIdx.x == 0) {
    const float cdiff = expf(-gamma * sqrtf(sc)), hdiff = expf(-gamma * sqrtf(sh));
    const size_t o = (size_t)b * npairs + q;
    sims[K * o] = cdiff;
    sims[K * o + 1] = hdiff;
    if (K == 2) {
      r[o] = cdiff * dw[0] + hdiff * dw[1] + db[0];
    } else {
      const float tdiff = expf(-gamma * (sqrtf(st) / (float)(sp * sp)));
      sims[K * o + 2] = tdiff;
      r[o] = ((cdiff * dw[0] + hdiff * dw[1]) + tdiff * dw[2]) + db[0];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The dense CRF: one wavefront per image, the n x n system A = I + D - R (n <= kMaxSp) in LDS tiles of row width W.  The
// steps that crf_loss_kernel, crf_map_kernel and crf_observed_kernel share follow, each written once.  A tile that lanes
// walk both down a column, one row each, and along a row has an odd row stride, so the two walks hit different banks.
constexpr int kMaxSp = 64;

// v[q] (without v: q itself, as bits) into T[l][r] and T[r][l] in pair order: a later pair overwrites an earlier one, a self
// pair lands on the diagonal.  True, in every lane, iff a pair has an index outside [0, n): then nothing is scattered and
// nothing indexed with, for every output of every image is NaN whatever T holds.  The lanes look at all pairs first, so
// that lane 0's serial loop has no branch that waits for a load.  The caller's barrier comes before T is read.
template <int W>
__device__ bool scatter_pairs(float (*T)[W], const float* __restrict__ v, const int* __restrict__ left,
                              const int* __restrict__ right, int n, int npairs, int lane) {
  bool outside = false;
  for (int q = lane; q < npairs; q += 64) {
    const int l = left[q], rr = right[q];
    outside = outside || l < 0 || l >= n || rr < 0 || rr >= n;
  }
  if (__any(outside)) return true;
  if (lane == 0)
    for (int q = 0; q < npairs; ++q) {
      const int l = left[q], rr = right[q];
      const float val = v ? v[q] : __int_as_float(q);
      T[l][rr] = val;
      T[rr][l] = val;
    }
  return false;
}

// A = I + diag(row sums of R) - R in the n x n corner of T, R scattered from the image's pair weights r: the row sum over
// ascending columns, 1 + it on the diagonal, 0 - R beside it.  Lane i ends with row i; the caller's barrier comes before
// anyone reads another row.  Returns scatter_pairs' flag: the index lists are the batch's, so it is every image's.
template <int W>
__device__ bool pair_matrix(float (*T)[W], const float* __restrict__ r, const int* __restrict__ left,
                            const int* __restrict__ right, int n, int npairs, int lane) {
  for (int i = lane; i < n * n; i += 64) T[i / n][i % n] = 0.f;
  __syncthreads();
  const bool bad = scatter_pairs(T, r, left, right, n, npairs, lane);
  __syncthreads();
  if (lane < n) {
    float rs = 0.f;
    for (int j = 0; j < n; ++j) rs += T[lane][j];
    for (int j = 0; j < n; ++j) T[lane][j] = (j == lane ? 1.f + rs : 0.f) - T[lane][j];
  }
  return bad;
}

// Row `lane` of an nn x nn system in U gets its right-hand side in column nn and, with `inverse`, its row of the identity
// in the nn columns behind that: [. | rhs | I].
template <int W>
__device__ void augment(float (*U)[W], int nn, int lane, float rhs, bool inverse) {
  if (lane >= nn) return;
  U[lane][nn] = rhs;
  if (inverse)
    for (int j = 0; j < nn; ++j) U[lane][nn + 1 + j] = j == lane ? 1.f : 0.f;
}

// Step k's pivot: of rows k .. nn - 1 the one with the largest magnitude in column k, the lowest of equals, a NaN before all
// (np.argmax's rule, tests/crf_loss_ref.loss32).  It is exchanged with row k over columns 0 .. last; true iff rows moved.
// Every lane ends with the same row: lane k always offers a value >= 0, the lanes outside [k, nn) offer -1.
// Left as a NaN, a candidate would compare false with everything: its lane would keep its own row, the others would
// agree on a row without it, and the lanes would exchange different rows, each in its own columns.  crf_loss_kernel once
// did; the rule changes none of its results, because with a NaN in column k on or below the diagonal every output of the
// image was NaN then as it is now.  If it is U[k][k], lane k, which moves column k, keeps row k: the pivot is NaN, and so
// is det in every lane.  If it is U[i][k], i > k, no other lane can settle on row i, so it stays where it is, row i's
// multiplier is NaN, and row i is NaN over columns k .. last whatever was exchanged; that repeats at every later step
// until k = i, the first case.  A NaN det makes fac, Z, u, the loss and every dz NaN, and dr through nan_row.
template <int W>
__device__ bool pivot_exchange(float (*U)[W], int k, int nn, int last, int lane) {
  float best = -1.f;
  if (lane >= k && lane < nn) {
    best = fabsf(U[lane][k]);
    if (!(best == best)) best = INFINITY;
  }
  int arg = lane;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ob = __shfl_xor(best, off, 64);
    const int oa = __shfl_xor(arg, off, 64);
    if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
  }
  if (arg != k)
    for (int j = lane; j <= last; j += 64) { const float t = U[k][j]; U[k][j] = U[arg][j]; U[arg][j] = t; }
  __syncthreads();
  return arg != k;
}

// What an elimination says about its pivots.  The function is inlined: a caller pays for the fields it reads.
struct Pivots {
  float det;         // their product, its sign turned at every exchange (the exchange first, then the pivot)
  float logdet;      // the sum of their logarithms
  bool positive;     // every one, after its exchange, finite and > 0, and the number of exchanges even
};

// LU with partial pivoting of the nn x nn system in the leading columns of U, carried over the columns 0 .. last, one lane
// per row.  Nothing stops at a bad pivot: the values turn into NaN or inf, no index depends on them.  nn = 0: {1, 0, true}.
template <int W>
__device__ __forceinline__ Pivots eliminate(float (*U)[W], int nn, int last, int lane) {
  Pivots p = {1.f, 0.f, true};
  bool even = true;
  for (int k = 0; k < nn; ++k) {
    if (pivot_exchange(U, k, nn, last, lane)) {
      p.det = -p.det;
      even = !even;
    }
    const float piv = U[k][k];
    p.det *= piv;
    p.positive = p.positive && piv > 0.f && piv < INFINITY;
    p.logdet += logf(piv);
    if (lane > k && lane < nn) {
      const float f = U[lane][k] / piv;
      for (int j = k; j <= last; ++j) U[lane][j] -= f * U[k][j];
    }
    __syncthreads();
  }
  p.positive = p.positive && even;
  return p;
}

// Back substitution after eliminate: x = the solution of column nn (lane 0, serial: 48 x 48 is small), and with `inverse`
// the nn columns behind it in place, one lane per column.
template <int W>
__device__ void back_substitute(float (*U)[W], int nn, int lane, bool inverse, float* x) {
  if (lane == 0) {
    for (int i = nn - 1; i >= 0; --i) {
      float s = U[i][nn];
      for (int j = i + 1; j < nn; ++j) s -= U[i][j] * x[j];
      x[i] = s / U[i][i];
    }
  }
  if (inverse && lane < nn) {
    const int c = nn + 1 + lane;
    for (int i = nn - 1; i >= 0; --i) {
      float s = U[i][c];
      for (int j = i + 1; j < nn; ++j) s -= U[i][j] * U[j][c];
      U[i][c] = s / U[i][i];
    }
  }
  __syncthreads();
}

// S = Z[l][l] + Z[r][r] - Z[l][r] - Z[r][l] of the inverse Z that back_substitute left behind column nn, added left to right
template <int W>
__device__ float pair_spread(float (*U)[W], int nn, int l, int rr) {
  const int c = nn + 1;
  return ((U[l][c + l] + U[rr][c + rr]) - U[l][c + rr]) - U[rr][c + l];
}

// The reference's loss (src/models.py:129-177): det(A) = +-prod(pivots) and w = A^-1 z from the LU of [A | z]; then energy,
// partition function, loss, d loss / d z, with the reference's epsilons.  A pair index outside [0, n) turns every image's
// loss and dz into NaN.
//
// kPairGrad (a3dp_crf_loss_grad) also writes dr = d mean loss / d r [batch, npairs], A no longer a constant.  With
// dA / dr_q = (e_l - e_r)(e_l - e_r)^T:  dE_q = (y_l - y_r)^2,  dg_q = -(w_l - w_r)^2,  d det = det S_q with S_q =
// pair_spread of A^-1, hence dfac_q = -fac / (sqrt(det) + eps) (sqrt(det) / 2) S_q.  A^-1 comes from the same elimination:
// U is [A | z | I].  Every operation that feeds the loss and dz is the one the other instantiation performs, in its order:
// both write the same bits.  A pair whose two cells a later pair overwrote has no part in A: its dr is +0; once A has
// been read, the tile holds the last writer of every cell instead.
template <bool kPairGrad>
__global__ __launch_bounds__(64) void crf_loss_kernel(const float* __restrict__ z, const float* __restrict__ y,
                                                      const float* __restrict__ r, const int* __restrict__ left,
                                                      const int* __restrict__ right, float* __restrict__ loss_img,
                                                      float* __restrict__ dz, float* __restrict__ dr, int n, int npairs,
                                                      float eps, float fac0, float inv_batch) {
  __shared__ float A[kMaxSp][kMaxSp + 1];
  __shared__ float U[kMaxSp][kPairGrad ? 2 * kMaxSp + 3 : kMaxSp + 2];      // working copy: [A | z] or [A | z | I]
  __shared__ float wv[kMaxSp];
  const int b = blockIdx.x, lane = threadIdx.x;
  const float zi = lane < n ? z[(size_t)b * n + lane] : 0.f;      // on their way while the matrix is built
  const float yi = lane < n ? y[(size_t)b * n + lane] : 0.f;
  const bool bad = pair_matrix(A, r + (size_t)b * npairs, left, right, n, npairs, lane);
  if (lane < n)
    for (int j = 0; j < n; ++j) U[lane][j] = A[lane][j];
  augment(U, n, lane, zi, kPairGrad);
  __syncthreads();
  // energy = y^T A y - 2 z^T y + z^T z
  float ay = 0.f;
  if (lane < n)
    for (int j = 0; j < n; ++j) ay += A[lane][j] * y[(size_t)b * n + j];
  const float yAy = wave_sum_f(yi * ay), zy = wave_sum_f(zi * yi), zz = wave_sum_f(zi * zi), zsum = wave_sum_f(zi);
  const float energy = yAy - 2.f * zy + zz;
  if (kPairGrad) {                              // A has been read: the last writer of every cell takes its place
    __syncthreads();
    scatter_pairs(A, nullptr, left, right, n, npairs, lane);
    __syncthreads();
  }
  const float det = eliminate(U, n, kPairGrad ? 2 * n : n, lane).det;
  back_substitute(U, n, lane, kPairGrad, wv);   // wv = A^-1 z; A^-1 behind column n
  const float wi = lane < n ? wv[lane] : 0.f;
  // g = z^T (A^-1 + eps) z - z^T z ;  inverseA = inv(A) + eps adds eps to EVERY element (src/models.py:165)
  const float zw = wave_sum_f(zi * wi);
  const float g = zw + eps * zsum * zsum - zz;
  const float sd = sqrtf(det);
  const float fac = fac0 / (sd + eps);
  const float ex = expf(g);
  const float Z = fac * ex + eps;
  const float u = expf(-energy) / Z;
  const float loss = -logf(u + eps);
  if (lane == 0) loss_img[b] = bad ? __builtin_nanf("") : loss;
  if (lane < n) {
    const float dE = -2.f * yi + 2.f * zi;
    const float dg = 2.f * wi + 2.f * eps * zsum - 2.f * zi;
    const float du = u * (-dE) - (u / Z) * (fac * ex * dg);
    dz[(size_t)b * n + lane] = bad ? __builtin_nanf("") : (-du / (u + eps)) * inv_batch;
  }
  if (kPairGrad) {
    const bool nan_row = bad || !(loss == loss);              // a negative determinant among them: sd is NaN
    const float dfac_s = -(fac / (sd + eps) * (sd * 0.5f));   // dfac_q = dfac_s * S_q
    for (int q = lane; q < npairs; q += 64) {
      float v = __builtin_nanf("");
      if (!nan_row) {                                         // not bad: l and rr are inside [0, n)
        const int l = left[q], rr = right[q];
        v = 0.f;
        if (__float_as_int(A[l][rr]) == q) {                  // else a later pair overwrote both cells
          const float dy = y[(size_t)b * n + l] - y[(size_t)b * n + rr], dw = wv[l] - wv[rr];
          const float dE = dy * dy, dg = -(dw * dw), dfac = dfac_s * pair_spread(U, n, l, rr);
          const float du = u * (-dE) - (u / Z) * (dfac * ex + fac * ex * dg);
          v = (-du / (u + eps)) * inv_batch;
        }
      }
      dr[(size_t)b * npairs + q] = v;
    }
  }
}

// The pairwise dense layer's backward: dw[k] = sum_i dr[i] sims[i][k], db = sum_i dr[i] over the count = n * npairs pairs of
// the batch.  ONE block and no atomics: thread t adds pairs t, t + 256, ... in order, then block_sum_256 — the same
// bits on every run.  k is the number of similarities per pair (1 .. kMaxSims); a NaN in dr reaches every output.
constexpr int kMaxSims = 8;
__global__ __launch_bounds__(256) void pair_dense_bwd_kernel(const float* __restrict__ sims, const float* __restrict__ dr,
                                                             float* __restrict__ dw, float* __restrict__ db,
                                                             size_t count, int k) {
  __shared__ float red[4];
  float acc[kMaxSims], accb = 0.f;
#pragma unroll
  for (int j = 0; j < kMaxSims; ++j) acc[j] = 0.f;
  for (size_t i = threadIdx.x; i < count; i += 256) {
    const float d = dr[i];
    accb += d;
#pragma unroll
    for (int j = 0; j < kMaxSims; ++j)
      if (j < k) acc[j] += d * sims[i * k + j];
  }
#pragma unroll
  for (int j = 0; j < kMaxSims; ++j) {
    if (j < k) {                                // k is the block's: no divergent barrier
      const float s = block_sum_256(acc[j], red);
      if (threadIdx.x == 0) dw[j] = s;
    }
  }
  accb = block_sum_256(accb, red);
  if (threadIdx.x == 0) db[0] = accb;
}

// MAP depths of the same field: y = A^-1 z from [A | z] in one tile.  The shared pivot search and exchange; but a row is
// eliminated with one lane per column, and only the rows whose multiplier is not zero are visited: A is sparse (a
// superpixel has at most four neighbours, fill-in stays inside the band).
// Then a column sweep by the whole wavefront: lane j keeps the right-hand side of row j in a register, and once y[i]
// is known every lane above subtracts its U[j][i] * y[i] (zero coefficients skipped too: r = 0 returns z's bits).
// A pivot that is zero or not finite or a non-finite component of the solution turns the image's whole row of y into NaN
// and its status into 1; nothing traps, other images are not touched.  A pair index outside [0, n) does the same to
// every image.
__global__ __launch_bounds__(64) void crf_map_kernel(const float* __restrict__ z, const float* __restrict__ r,
                                                     const int* __restrict__ left, const int* __restrict__ right,
                                                     float* __restrict__ y, int* __restrict__ status, int n,
                                                     int npairs) {
  __shared__ float U[kMaxSp][kMaxSp + 1];       // column n holds the right-hand side
  const int b = blockIdx.x, lane = threadIdx.x;
  const float zi = lane < n ? z[(size_t)b * n + lane] : 0.f;      // on its way while the matrix is built
  bool bad = pair_matrix(U, r + (size_t)b * npairs, left, right, n, npairs, lane);
  augment(U, n, lane, zi, false);
  __syncthreads();
  for (int k = 0; k < n && !bad; ++k) {         // `bad` is the same in every lane: no divergent barrier
    pivot_exchange(U, k, n, n, lane);           // a NaN is taken as the pivot at once, and ends the image below
    const float piv = U[k][k];
    if (piv == 0.f || !isfinite(piv)) { bad = true; break; }
    const bool below = lane > k && lane < n;
    const float f = below ? U[lane][k] / piv : 0.f;       // lane i: the multiplier of row i
    const float prow = below ? U[k][lane] : 0.f;          // lane j: column j of the pivot row
    if (f != 0.f) U[lane][n] -= f * U[k][n];
    unsigned long long todo = __ballot(f != 0.f);         // only the rows that have something to eliminate
    while (todo) {
      const int i = __ffsll(todo) - 1;
      todo &= todo - 1;
      const float fi = __shfl(f, i, 64);
      if (below) U[i][lane] -= fi * prow;
    }
    __syncthreads();
  }
  float rhs = 0.f, yi = 0.f;
  if (!bad) {
    if (lane < n) rhs = U[lane][n];
    for (int i = n - 1; i >= 0; --i) {
      const float yv = __shfl(rhs, i, 64) / U[i][i];
      if (lane == i) yi = yv;
      if (lane < i) {
        const float u = U[lane][i];
        if (u != 0.f) rhs -= u * yv;
      }
    }
    bad = __any(lane < n && !isfinite(yi));
  }
  if (lane < n) y[(size_t)b * n + lane] = bad ? __builtin_nanf("") : yi;
  if (lane == 0 && status) status[b] = bad ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// NON-REFERENCE (include/a3d_crf_valid.h, --model dcnf with --min-depth / --max-depth): depth maps with holes.

// superpixel_mean_kernel over the finite pixels of a one-channel map: the same threads add the same pixels in the same
// order, a hole adds nothing; c counts the pixels that were added.
__global__ __launch_bounds__(256) void superpixel_mean_valid_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                                    int* __restrict__ count, int h, int w, int sp,
                                                                    int min_count) {
  __shared__ float red[4];
  __shared__ int redc[4];
  const int cols = w / sp, rows = h / sp;
  const int p = blockIdx.x % (rows * cols), b = blockIdx.x / (rows * cols);
  const int pr = p / cols, pc = p % cols;
  float s = 0.f;
  int c = 0;
  for (int i = threadIdx.x; i < sp * sp; i += 256) {
    const int yy = pr * sp + i / sp, xx = pc * sp + i % sp;
    const float v = x[((size_t)b * h + yy) * w + xx];
    if (isfinite(v)) { s += v; ++c; }
  }
  s = block_sum_256(s, red);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
  if ((threadIdx.x & 63) == 0) redc[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    c = redc[0] + redc[1] + redc[2] + redc[3];
    const size_t o = (size_t)b * rows * cols + p;
    out[o] = c >= max(1, min_count) ? s / (float)c : __builtin_nanf("");
    if (count) count[o] = c;
  }
}

// One wavefront per image: the negative log-likelihood of the superpixels whose target y is finite (O, m of them; M the
// others), L = q^T A q + (log det A_MM - log det A) / 2 + m log(pi) / 2 with q = yhat - A^-1 z, yhat = y on O and the
// conditional mean A_MM^-1 (z_M - A_MO y_O) on M; dz = -2 q / batch; kPairGrad: dr too (include/a3d_crf_valid.h has the
// derivation).  Two eliminations, one after the other in the same tile U: [A | z | I] and, the missing rows and columns
// of A moved together in their order, [A_MM | z_M - A_MO y_O | I] (the identity columns only under kPairGrad).  A stays in
// its own tile for the second system and for q^T A q, and holds the last writer of every cell after that.
// LDS: A 64 x 65 floats (16640 bytes), U 64 x 131 (33536; 64 x 67 = 17152 without dr), seven arrays of 64 words (1792):
// 51968 bytes under kPairGrad, 35584 without.
// y is read once, to tell finite from not; an entry that is not finite is never used again.  dr holds S_k(A^-1) of every
// pair between the two eliminations (each lane reads back only what it wrote itself).
// Every index into A, U and the arrays is a lane, a pair index checked against [0, n), a rank below the number of missing
// superpixels, or a column <= 2 n.
template <bool kPairGrad>
__global__ __launch_bounds__(64) void crf_observed_kernel(const float* __restrict__ z, const float* __restrict__ y,
                                                          const float* __restrict__ r, const int* __restrict__ left,
                                                          const int* __restrict__ right, float* __restrict__ loss_img,
                                                          float* __restrict__ dz, float* dr, int* __restrict__ nobs,
                                                          int* __restrict__ status, int n, int npairs, float inv_batch) {
  __shared__ float A[kMaxSp][kMaxSp + 1];
  __shared__ float U[kMaxSp][kPairGrad ? 2 * kMaxSp + 3 : kMaxSp + 3];
  __shared__ float zs[kMaxSp], yh[kMaxSp], mu[kMaxSp], xm[kMaxSp], qv[kMaxSp];
  __shared__ int mrank[kMaxSp], midx[kMaxSp];
  const int b = blockIdx.x, lane = threadIdx.x;
  const float nanf_ = __builtin_nanf("");
  const float zi = lane < n ? z[(size_t)b * n + lane] : 0.f;      // on their way while the matrix is built
  const float yraw = lane < n ? y[(size_t)b * n + lane] : 0.f;
  const bool bad = pair_matrix(A, r + (size_t)b * npairs, left, right, n, npairs, lane);
  const bool obs = lane < n && isfinite(yraw);
  const bool mis = lane < n && !obs;
  const float yi = obs ? yraw : 0.f;            // from here on an unobserved target is not looked at
  const unsigned long long mis_mask = __ballot(mis);
  const int m = __popcll(__ballot(obs)), km = __popcll(mis_mask);
  if (bad || m == 0) {                          // the whole wavefront: the index lists are the batch's, m is the image's
    const float v = bad ? nanf_ : 0.f;
    if (lane == 0) {
      loss_img[b] = v;
      nobs[b] = m;
      status[b] = bad ? 1 : 0;
    }
    if (lane < n) dz[(size_t)b * n + lane] = v;
    if (kPairGrad)
      for (int q = lane; q < npairs; q += 64) dr[(size_t)b * npairs + q] = v;
    return;
  }
  const int rank = __popcll(mis_mask & ((1ull << lane) - 1ull));
  if (lane < n) {
    zs[lane] = zi;
    yh[lane] = yi;
    mrank[lane] = mis ? rank : -1;
    if (mis) midx[rank] = lane;
    for (int j = 0; j < n; ++j) U[lane][j] = A[lane][j];
  }
  augment(U, n, lane, zi, kPairGrad);
  __syncthreads();
  const Pivots pa = eliminate(U, n, kPairGrad ? 2 * n : n, lane);
  back_substitute(U, n, lane, kPairGrad, mu);                           // mu = A^-1 z; A^-1 behind column n
  if (kPairGrad) {
    for (int q = lane; q < npairs; q += 64)                             // not bad: the pairs are inside [0, n)
      dr[(size_t)b * npairs + q] = pair_spread(U, n, left[q], right[q]);
    __syncthreads();                                                    // A^-1 has been read: U is free
  }
  float rhs_m = 0.f;
  if (lane < km) {                              // row `lane` of the second system: missing superpixel i = midx[lane]
    const int i = midx[lane];
    for (int c = 0; c < km; ++c) U[lane][c] = A[i][midx[c]];
    float s = 0.f;
    for (int j = 0; j < n; ++j) s += A[i][j] * yh[j];                   // yh = 0 on M: A_MO y_O
    rhs_m = zs[i] - s;
  }
  augment(U, km, lane, rhs_m, kPairGrad);
  __syncthreads();
  const Pivots pm = eliminate(U, km, kPairGrad ? 2 * km : km, lane);
  back_substitute(U, km, lane, kPairGrad, xm);                          // xm = yhat_M; A_MM^-1 behind column km
  float qi = 0.f;
  if (lane < n) {
    qi = (obs ? yi : xm[rank]) - mu[lane];
    qv[lane] = qi;
  }
  __syncthreads();
  float aq = 0.f;
  if (lane < n)
    for (int j = 0; j < n; ++j) aq += A[lane][j] * qv[j];
  const float qAq = wave_sum_f(qi * aq);
  const float loss = (qAq + 0.5f * (pm.logdet - pa.logdet)) + (float)m * kHalfLogPi;
  const bool nan_row = !(pa.positive && pm.positive && isfinite(loss));
  if (lane == 0) {
    loss_img[b] = nan_row ? nanf_ : loss;
    nobs[b] = m;
    status[b] = nan_row ? 1 : 0;
  }
  if (lane < n) dz[(size_t)b * n + lane] = nan_row ? nanf_ : (-2.f * qi) * inv_batch;
  if (kPairGrad) {
    __syncthreads();                            // A has been read: the last writer of every cell takes its place
    scatter_pairs(A, nullptr, left, right, n, npairs, lane);
    __syncthreads();
    for (int q = lane; q < npairs; q += 64) {
      float v = nanf_;
      if (!nan_row) {
        const int l = left[q], rr = right[q];
        v = 0.f;
        if (__float_as_int(A[l][rr]) == q) {                            // else a later pair overwrote both cells
          const float s_a = dr[(size_t)b * npairs + q];
          const int gl = mrank[l], gr = mrank[rr];
          float s_m = 0.f;                                              // S_k of A_MM^-1 padded with zeros
          if (gl >= 0 && gr >= 0)
            s_m = pair_spread(U, km, gl, gr);
          else if (gl >= 0)
            s_m = U[gl][km + 1 + gl];
          else if (gr >= 0)
            s_m = U[gr][km + 1 + gr];
          const float vq = qv[l] - qv[rr], vm = mu[l] - mu[rr];
          v = (((2.f * vq) * vm + vq * vq) - 0.5f * (s_a - s_m)) * inv_batch;
        }
      }
      dr[(size_t)b * npairs + q] = v;
    }
  }
}

// tf.train.GradientDescentOptimizer(lr) (src/models.py:198): var -= lr * g
// the two descents' walks: optim_rules.h, shared with the launches that scale lr by a gradient-norm control block (clip.hip)
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ var, const float* __restrict__ g, size_t count,
                                                  float lr) {
  sgd_body(var, g, count, lr);
}

// projected gradient descent: sgd_kernel's step, then no lower than `floor`.  The comparison keeps a NaN a NaN.
__global__ __launch_bounds__(256) void sgd_floor_kernel(float* __restrict__ var, const float* __restrict__ g, size_t count,
                                                        float lr, float floor) {
  sgd_floor_body(var, g, count, lr, floor);
}

}  // namespace a3d

using namespace a3d;

extern "C" {

int a3d_superpixel_mean(int n, int h, int w, int c, const float* x, int sp, float* out, void* stream) {
  A3D_CHECK_ARG(n > 0 && sp > 0 && h % sp == 0 && w % sp == 0 && c > 0 && x && out, "superpixel_mean: bad arguments");
  clear_stale_error();
  hipLaunchKernelGGL(superpixel_mean_kernel, dim3(n * (h / sp) * (w / sp)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), x, out, h, w, c, sp);
  return check_launch("superpixel_mean");
}

int a3d_superpixel_hist(int n, int h, int w, const float* x, int sp, float* hist, void* stream) {
  A3D_CHECK_ARG(n > 0 && sp > 0 && h % sp == 0 && w % sp == 0 && x && hist, "superpixel_hist: bad arguments");
  clear_stale_error();
  hipLaunchKernelGGL(superpixel_hist_kernel, dim3(n * (h / sp) * (w / sp)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), x, hist, h, w, sp);
  return check_launch("superpixel_hist");
}

int a3d_pair_similarity(int n, int h, int w, const float* x, int sp, const float* hist, const int32_t* left,
                        const int32_t* right, int npairs, const float* dense_w, const float* dense_b, float gamma,
                        float* sims, float* r, void* stream) {
  A3D_CHECK_ARG(n > 0 && sp > 0 && h % sp == 0 && w % sp == 0 && npairs > 0 && x && hist && left && right && dense_w &&
                    dense_b && sims && r, "pair_similarity: bad arguments");
  clear_stale_error();
  hipLaunchKernelGGL(pair_similarity_kernel<2>, dim3(n * npairs), dim3(256), 0, static_cast<hipStream_t>(stream), x, hist,
                     nullptr, left, right, dense_w, dense_b, sims, r, h, w, sp, npairs, gamma);
  return check_launch("pair_similarity");
}

int a3dt_superpixel_lbp_hist(int n, int h, int w, const float* x, int sp, float* hist, void* stream) {
  A3D_CHECK_ARG(n > 0 && h > 0 && w > 0 && sp > 0 && sp <= kMaxTextureSp && h % sp == 0 && w % sp == 0 && x && hist,
                "superpixel_lbp_hist: bad arguments (superpixel edge at most %d)", kMaxTextureSp);
  clear_stale_error();
  hipLaunchKernelGGL(superpixel_lbp_hist_kernel, dim3(n * (h / sp) * (w / sp)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), x, hist, h, w, sp);
  return check_launch("superpixel_lbp_hist");
}

int a3dt_pair_similarity3(int n, int h, int w, const float* x, int sp, const float* hist, const float* lbp_hist,
                          const int32_t* left, const int32_t* right, int npairs, const float* dense_w,
                          const float* dense_b, float gamma, float* sims, float* r, void* stream) {
  A3D_CHECK_ARG(n > 0 && h > 0 && w > 0 && sp > 0 && sp <= kMaxTextureSp && h % sp == 0 && w % sp == 0 && npairs > 0 &&
                    x && hist && lbp_hist && left && right && dense_w && dense_b && sims && r,
                "pair_similarity3: bad arguments (superpixel edge at most %d)", kMaxTextureSp);
  clear_stale_error();
  hipLaunchKernelGGL(pair_similarity_kernel<3>, dim3(n * npairs), dim3(256), 0, static_cast<hipStream_t>(stream), x, hist,
                     lbp_hist, left, right, dense_w, dense_b, sims, r, h, w, sp, npairs, gamma);
  return check_launch("pair_similarity3");
}

// a3d_crf_loss (dr == nullptr) and a3dp_crf_loss_grad: the same two launches, the first one in its other instantiation
static int crf_loss_launch(int n, int nsp, const float* z, const float* y, const float* r, const int32_t* left,
                           const int32_t* right, int npairs, float eps, float* loss_per_image, float* loss_mean,
                           float* dz, float* dr, void* stream) {
  hipStream_t st = static_cast<hipStream_t>(stream);
  const float fac0 = (float)pow(3.14159265358979323846, nsp / 2.0);
  clear_stale_error();
  hipLaunchKernelGGL(dr ? crf_loss_kernel<true> : crf_loss_kernel<false>, dim3(n), dim3(64), 0, st, z, y, r, left,
                     right, loss_per_image, dz, dr, nsp, npairs, eps, fac0, 1.0f / (float)n);
  int rc = check_launch("crf_loss");
  if (rc != A3D_OK) return rc;
  clear_stale_error();
  hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(64), 0, st, loss_per_image, n, loss_mean);
  return check_launch("crf_loss_mean");
}

int a3d_crf_loss(int n, int nsp, const float* z, const float* y, const float* r, const int32_t* left,
                 const int32_t* right, int npairs, float eps, float* loss_per_image, float* loss_mean, float* dz,
                 void* stream) {
  A3D_CHECK_ARG(n > 0 && nsp > 0 && nsp <= kMaxSp && npairs > 0 && z && y && r && left && right && loss_per_image &&
                    loss_mean && dz, "crf_loss: bad arguments (at most %d superpixels)", kMaxSp);
  return crf_loss_launch(n, nsp, z, y, r, left, right, npairs, eps, loss_per_image, loss_mean, dz, nullptr, stream);
}

int a3dp_crf_loss_grad(int n, int nsp, const float* z, const float* y, const float* r, const int32_t* left,
                       const int32_t* right, int npairs, float eps, float* loss_per_image, float* loss_mean, float* dz,
                       float* dr, void* stream) {
  A3D_CHECK_ARG(n > 0 && nsp > 0 && nsp <= kMaxSp && npairs > 0 && z && y && r && left && right && loss_per_image &&
                    loss_mean && dz && dr, "crf_loss_grad: bad arguments (at most %d superpixels)", kMaxSp);
  return crf_loss_launch(n, nsp, z, y, r, left, right, npairs, eps, loss_per_image, loss_mean, dz, dr, stream);
}

int a3dp_pair_dense_bwd(int n, int npairs, int k, const float* sims, const float* dr, float* dw, float* db,
                        void* stream) {
  A3D_CHECK_ARG(n > 0 && npairs > 0 && k >= 1 && k <= kMaxSims && sims && dr && dw && db,
                "pair_dense_bwd: bad arguments (1 .. %d similarities per pair)", kMaxSims);
  clear_stale_error();
  hipLaunchKernelGGL(pair_dense_bwd_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), sims, dr, dw, db,
                     (size_t)n * (size_t)npairs, k);
  return check_launch("pair_dense_bwd");
}

int a3d_crf_map(int n, int nsp, const float* z, const float* r, const int32_t* left, const int32_t* right, int npairs,
                float* y, int32_t* status, void* stream) {
  A3D_CHECK_ARG(n > 0 && nsp > 0 && nsp <= kMaxSp && npairs > 0 && z && r && left && right && y,
                "crf_map: bad arguments (at most %d superpixels)", kMaxSp);
  clear_stale_error();
  hipLaunchKernelGGL(crf_map_kernel, dim3(n), dim3(64), 0, static_cast<hipStream_t>(stream), z, r, left, right, y,
                     status, nsp, npairs);
  return check_launch("crf_map");
}

int a3dv_superpixel_mean_valid(int n, int h, int w, const float* x, int sp, int min_count, float* y, int32_t* count,
                               void* stream) {
  A3D_CHECK_ARG(n > 0 && sp > 0 && h > 0 && w > 0 && h % sp == 0 && w % sp == 0 && min_count >= 0 && x && y,
                "superpixel_mean_valid: bad arguments");
  clear_stale_error();
  hipLaunchKernelGGL(superpixel_mean_valid_kernel, dim3(n * (h / sp) * (w / sp)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), x, y, count, h, w, sp, min_count);
  return check_launch("superpixel_mean_valid");
}

int a3dv_crf_loss_observed(int n, int nsp, const float* z, const float* y, const float* r, const int32_t* left,
                           const int32_t* right, int npairs, float* loss_per_image, float* loss_mean, float* dz, float* dr,
                           int32_t* nobs, int32_t* status, void* stream) {
  A3D_CHECK_ARG(n > 0 && nsp > 0 && nsp <= kMaxSp && npairs > 0 && z && y && r && left && right && loss_per_image &&
                    loss_mean && dz && nobs && status, "crf_loss_observed: bad arguments (at most %d superpixels)", kMaxSp);
  hipStream_t st = static_cast<hipStream_t>(stream);
  clear_stale_error();
  hipLaunchKernelGGL(dr ? crf_observed_kernel<true> : crf_observed_kernel<false>, dim3(n), dim3(64), 0, st, z, y, r, left,
                     right, loss_per_image, dz, dr, nobs, status, nsp, npairs, 1.0f / (float)n);
  int rc = check_launch("crf_loss_observed");
  if (rc != A3D_OK) return rc;
  clear_stale_error();
  hipLaunchKernelGGL(mean_kernel, dim3(1), dim3(64), 0, st, loss_per_image, n, loss_mean);
  return check_launch("crf_loss_observed_mean");
}

int a3d_sgd_apply(size_t count, float* var, const float* g, float lr, void* stream) {
  A3D_CHECK_ARG(count > 0 && var && g, "sgd: bad arguments");
  clear_stale_error();
  hipLaunchKernelGGL(sgd_kernel, dim3(rule_grid_scalar(count)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), var, g, count, lr);
  return check_launch("sgd");
}

int a3dp_sgd_apply_floor(size_t count, float* var, const float* g, float lr, float floor, void* stream) {
  A3D_CHECK_ARG(count > 0 && var && g, "sgd_floor: bad arguments");
  clear_stale_error();
  hipLaunchKernelGGL(sgd_floor_kernel, dim3(rule_grid_scalar(count)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), var, g, count, lr, floor);
  return check_launch("sgd_floor");
}

}  // extern "C"
