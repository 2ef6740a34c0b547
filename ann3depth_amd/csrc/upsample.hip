// upsample.hip — joint bilateral upsampling of a coarse depth map under the full-resolution image
// (include/a3d_upsample.h; NON-REFERENCE, `predict` and `evaluate --upsample joint`).
//
// One block per 8 x 32 tile of output pixels, one pixel per lane.  The cells a tile's windows can reach stand in LDS as
// (d, I~r, I~g, I~b), one 16-byte read per cell and lane, mostly the same address across a wave (a broadcast); every lane
// then walks its window twice, a minimum pass and the sums.  The work is the exponentials and those LDS reads, not HBM: a
// pixel moves 16 bytes (12 of guide, 4 of output) against (2R + 1)^2 expf.  Built with -ffp-contract=off; the operations
// of the definition are spelled with the __f*_rn intrinsics all the same.
#include <math.h>

#include "a3d_internal.h"
#include "../../include/a3d_upsample.h"

namespace a3d {
namespace {

constexpr int kTileX = 32, kTileY = 8;      // output pixels per block: lanes along x, the guide's innermost pixel axis
constexpr int kCapCells = 1024;             // cells of a tile's range held in LDS (16 KiB)

struct UpsampleParams {
  const float* depth;
  const void* guide;
  const float *cy, *cx;
  const int32_t *ay, *ax;
  float* out;
  int gh, gw, H, W, R, tiles_x, tiles_y;
  float inv2ss, inv2sr;
};

__device__ inline bool finite(float v) { return fabsf(v) < INFINITY; }

template <bool U8>
__device__ inline void load_rgb(const void* guide, size_t pixel, float (&c)[3]) {
  if constexpr (U8) {
    const uint8_t* g = static_cast<const uint8_t*>(guide) + pixel * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = __fdiv_rn((float)g[k], 255.f);
  } else {
    const float* g = static_cast<const float*>(guide) + pixel * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = g[k];
  }
}

// Cell (i, j) of image b as the window loop wants it: x its depth, y z w its colour.  A cell whose anchor lies outside the
// image carries a NaN depth, which is how the loop skips it; the anchor is not used as an index then.
template <bool U8>
__device__ inline float4 fetch_cell(const UpsampleParams& p, int b, int i, int j) {
  const float d = p.depth[((size_t)b * p.gh + i) * p.gw + j];
  const int a_y = p.ay[i], a_x = p.ax[j];
  const bool inside = a_y >= 0 && a_y < p.H && a_x >= 0 && a_x < p.W;
  float c[3] = {0.f, 0.f, 0.f};
  if (inside) load_rgb<U8>(p.guide, ((size_t)b * p.H + a_y) * p.W + a_x, c);
  return make_float4(inside ? d : __builtin_nanf(""), c[0], c[1], c[2]);
}

// clamp(floor(c + 1/2), 0, last) as a float, then the integer: fmaxf takes a NaN to 0
__device__ inline int window_centre(float c, int last) {
  return (int)fminf(fmaxf(floorf(__fadd_rn(c, 0.5f)), 0.f), (float)last);
}

// The value of one output pixel.  STAGED: the cells [i0, ..] x [j0, j0 + nj) stand in s_cell; else they come from memory.
template <bool STAGED, bool U8>
__device__ inline float upsample_pixel(const UpsampleParams& p, const float4* s_cell, int i0, int j0, int nj, int b, int q0y,
                                       int q0x, float cyv, float cxv, const float (&g)[3]) {
  const int ilo = max(q0y - p.R, 0), ihi = min(q0y + p.R, p.gh - 1);
  const int jlo = max(q0x - p.R, 0), jhi = min(q0x + p.R, p.gw - 1);
  float e_min = INFINITY, d_min = INFINITY, d_max = -INFINITY, num = 0.f, den = 0.f;
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    for (int i = ilo; i <= ihi; ++i) {
      const float dy = __fsub_rn((float)i, cyv);
      const float dy2 = __fmul_rn(dy, dy);
      for (int j = jlo; j <= jhi; ++j) {
        const float4 c = STAGED ? s_cell[(i - i0) * nj + (j - j0)] : fetch_cell<U8>(p, b, i, j);
        const float dx = __fsub_rn((float)j, cxv);
        const float space = __fadd_rn(dy2, __fmul_rn(dx, dx));
        const float dr = __fsub_rn(g[0], c.y), dg = __fsub_rn(g[1], c.z), db = __fsub_rn(g[2], c.w);
        const float range = __fadd_rn(__fadd_rn(__fmul_rn(dr, dr), __fmul_rn(dg, dg)), __fmul_rn(db, db));
        const float e = __fadd_rn(__fmul_rn(space, p.inv2ss), __fmul_rn(range, p.inv2sr));
        const bool keep = finite(c.x) && finite(e);
        if (pass == 0) {
          e_min = keep ? fminf(e_min, e) : e_min;
          d_min = keep ? fminf(d_min, c.x) : d_min;
          d_max = keep ? fmaxf(d_max, c.x) : d_max;
        } else {
          // a skipped cell adds +0 to sums that started at +0: the bits of leaving it out
          const float w = keep ? expf(-__fsub_rn(e, e_min)) : 0.f;
          num = __fadd_rn(num, keep ? __fmul_rn(w, c.x) : 0.f);
          den = __fadd_rn(den, w);
        }
      }
    }
  }
  const float v = fminf(fmaxf(__fdiv_rn(num, den), d_min), d_max);
  return e_min < INFINITY ? v : __builtin_nanf("");
}

template <bool U8>
__global__ __launch_bounds__(kTileX* kTileY) void joint_bilateral_upsample_kernel(const UpsampleParams p) {
  __shared__ float4 s_cell[kCapCells];
  __shared__ int s_range[4];      // min and max window centre of the tile's rows, then of its columns
  const int tid = threadIdx.x, lx = tid % kTileX, ly = tid / kTileX;
  const int tile = blockIdx.x % (p.tiles_x * p.tiles_y), b = blockIdx.x / (p.tiles_x * p.tiles_y);
  const int x = (tile % p.tiles_x) * kTileX + lx, y = (tile / p.tiles_x) * kTileY + ly;
  const bool inside = x < p.W && y < p.H;
  const float cyv = y < p.H ? p.cy[y] : 0.f, cxv = x < p.W ? p.cx[x] : 0.f;
  const int q0y = window_centre(cyv, p.gh - 1), q0x = window_centre(cxv, p.gw - 1);
  if (tid == 0) s_range[0] = s_range[2] = 0x7fffffff, s_range[1] = s_range[3] = -1;
  __syncthreads();
  // integer LDS atomics: the same numbers in any order.  Lane column 0 of a tile is always inside the image, and row 0.
  if (lx == 0 && y < p.H) atomicMin(&s_range[0], q0y), atomicMax(&s_range[1], q0y);
  if (ly == 0 && x < p.W) atomicMin(&s_range[2], q0x), atomicMax(&s_range[3], q0x);
  __syncthreads();
  const int i0 = max(s_range[0] - p.R, 0), i1 = min(s_range[1] + p.R, p.gh - 1);
  const int j0 = max(s_range[2] - p.R, 0), j1 = min(s_range[3] + p.R, p.gw - 1);
  const int nj = j1 - j0 + 1;
  const bool staged = (long long)(i1 - i0 + 1) * nj <= kCapCells;      // the same in every lane of the block
  if (staged) {
    const int cells = (i1 - i0 + 1) * nj;
    for (int t = tid; t < cells; t += kTileX * kTileY) s_cell[t] = fetch_cell<U8>(p, b, i0 + t / nj, j0 + t % nj);
  }
  __syncthreads();
  if (!inside) return;
  const size_t pixel = ((size_t)b * p.H + y) * p.W + x;
  float g[3];
  load_rgb<U8>(p.guide, pixel, g);
  p.out[pixel] = staged ? upsample_pixel<true, U8>(p, s_cell, i0, j0, nj, b, q0y, q0x, cyv, cxv, g)
                        : upsample_pixel<false, U8>(p, s_cell, i0, j0, nj, b, q0y, q0x, cyv, cxv, g);
}

}  // namespace
}  // namespace a3d

using namespace a3d;

extern "C" {

int a3du_joint_bilateral_upsample(int n, int gh, int gw, const float* depth, int H, int W, const void* guide, int guide_u8,
                                  const float* cy, const float* cx, const int32_t* ay, const int32_t* ax, int radius,
                                  float inv2ss, float inv2sr, float* out, void* stream) {
  const char* who = "joint_bilateral_upsample";
  A3D_CHECK_ARG(depth && guide && cy && cx && ay && ax && out, "%s: NULL pointer", who);
  A3D_CHECK_ARG(n > 0 && gh > 0 && gw > 0 && H > 0 && W > 0, "%s: n, gh, gw, H, W must be positive", who);
  A3D_CHECK_ARG(radius >= 1 && radius <= A3DU_MAX_RADIUS, "%s: radius %d outside 1 .. %d", who, radius, A3DU_MAX_RADIUS);
  A3D_CHECK_ARG(inv2ss >= 0.f && inv2ss < INFINITY && inv2sr >= 0.f && inv2sr < INFINITY,
                "%s: inv2ss = %g, inv2sr = %g must be finite and >= 0", who, (double)inv2ss, (double)inv2sr);
  A3D_CHECK_ARG(gh <= (1 << 24) && gw <= (1 << 24), "%s: a grid of %d x %d cells, above 2^24 along an axis", who, gh, gw);
  const int tiles_x = (W + kTileX - 1) / kTileX, tiles_y = (H + kTileY - 1) / kTileY;
  A3D_CHECK_ARG((long long)n * H * W <= 0x7fffffffLL && (long long)n * tiles_x * tiles_y <= 0x7fffffffLL,
                "%s: more than 2^31 - 1 output pixels", who);
  const UpsampleParams p{depth, guide, cy, cx, ay, ax, out, gh, gw, H, W, radius, tiles_x, tiles_y, inv2ss, inv2sr};
  clear_stale_error();
  hipLaunchKernelGGL(guide_u8 ? joint_bilateral_upsample_kernel<true> : joint_bilateral_upsample_kernel<false>,
                     dim3((unsigned)(n * tiles_x * tiles_y)), dim3(kTileX * kTileY), 0, static_cast<hipStream_t>(stream), p);
  return check_launch(who);
}

}  // extern "C"
