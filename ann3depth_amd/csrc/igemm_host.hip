// igemm_host.hip — the conv2d / dense entry points of include/a3d.h: which kernel takes a call (the stencil, conv3 / conv3b, the
// bf16 image and window-run forms with their filter repacks, fewch / fewch16, the LDS-DMA kernel or the generic GEMM), the workspace
// that takes, and the kernel's parameters.  The plans: igemm_plan.cc; the launches: igemm_launch.hip.
#include <algorithm>
#include <cmath>

#include "../../include/a3d_wino.h"
#include "../../include/a3d_wino_grad.h"
#include "../../include/a3d_wino_bwd.h"
#include "../../include/a3d_wino1d.h"
#include "a3d_internal.h"
#include "igemm.h"
#include "igemm_cfgs.h"

namespace a3d {

int launch_igemm_multi_bwd_d(int avec, int bvec, IgemmMulti& ps, unsigned grid_x, unsigned count, hipStream_t st);
int launch_igemm_bf16_multi_bwd_d(int bn, IgemmMulti& ps, unsigned grid_x, unsigned count, hipStream_t st);

// The switches read here and in igemm_launch.hip (A3D_PLAN_LOG, A3D_DBG, A3D_FEWCH, ...) and the planner's (A3D_FORCE_*,
// A3D_BF16_BN, A3D_RING*) all go through tune_int() (igemm_plan.h, capi.cc): the environment is consulted on every launch ONLY
// in a process started with A3D_TUNING=1, as the sweep and fuzz tools do; otherwise nothing reads it, and plans are cached per
// problem (plan_gemm).

// ---- "window-run" form of few-channel VALID convolutions (Cin = 3: conv2d_0, fine/first) ----
// For an unpadded conv with densely packed pixels a filter row (s, c) is ONE contiguous run of S*Cin floats of the
// input, starting stride*Cin floats after the previous output pixel's run.  When those starts are 16- (or 8-) byte
// aligned the run is gathered with vector loads instead of float by float: the K axis becomes (r, q) with q padded
// to a multiple of the vector width, the padded filter rows are zero, and the generic kernel sees a conv with S' = 1
// and Cin' = padded run length.  The few floats read past a run belong to the next pixels of the same image row
// (guaranteed in-bounds by run_form_ok) and meet zero weights.
struct RunForm {
  int vec;      // 4 or 2
  int rl, rlp;  // run length S*Cin and its padded length
  int kp;       // R * rlp
  int np;       // forward: a row of the padded filter, the k filters padded to 16 bytes
  size_t bytes; // the padded filter (bwd-filter: its gradient) in the workspace
};
// bwd_filter: the filter-gradient GEMM may also take runs that start at any 4-byte address (DCNF's first conv: stride 1,
// runs 12 bytes apart) as 8-byte buffer loads — the hardware only asks a multi-dword buffer load for dword alignment —
// and runs whose padding reaches past the row's end: what a pad element multiplies ends up in a pad row of the padded
// gradient, which is never stored (past the tensor's end the descriptor returns zeros).
// x_off: x's address & 15 (a query: kOnGrid.x)
static bool run_form_ok(const a3d_conv_desc* d, unsigned x_off, RunForm* rf, bool bwd_filter = false) {
  if (d->pad_t || d->pad_l || d->ldx != d->c || d->c % 4 == 0 || d->c > 4) return false;
  const int step = d->stride * d->c, row = d->w * d->c;
  int vec = 0;
  bool anywhere = false;
  if (step % 4 == 0 && row % 4 == 0 && x_off == 0) vec = 4;
  else if (step % 2 == 0 && row % 2 == 0 && (x_off & 7) == 0) vec = 2;
  else if (bwd_filter && d->precision == A3D_PREC_F32 && !d->storage && (x_off & 3) == 0) {
    vec = 2;
    anywhere = true;
  }
  if (vec == 4 && d->precision == A3D_PREC_F32) {      // (the bf16 kernels take 16-byte operands only)
    // 8-byte runs pad less (conv2d_0: 33 -> 34 instead of 36 floats per filter row).  Worth the narrower loads when it
    // saves a whole 128-row tile of the bwd-filter GEMM (374 vs 396 rows: 3 tiles instead of 4; 172 -> 148 us, and the
    // forward loses a k-tile: 135 -> 129 us)
    const int rl = d->s * d->c;
    const int kp4 = d->r * ((rl + 3) / 4 * 4), kp2 = d->r * ((rl + 1) / 2 * 2);
    if ((kp2 + 127) / 128 < (kp4 + 127) / 128) vec = 2;
  }
  if (!vec) return false;
  rf->vec = vec;
  rf->rl = d->s * d->c;
  rf->rlp = (rf->rl + vec - 1) / vec * vec;
  rf->kp = d->r * rf->rlp;
  rf->np = (d->k + 3) / 4 * 4;
  rf->bytes = up256((size_t)rf->kp * rf->np * 4);
  // the padded run of the last output column stays inside its row; `anywhere`: the run itself does (no implicit padding
  // on the right / below: a SAME convolution with an even kernel has pad_t = pad_l = 0 and still pads), its padding may not
  if (anywhere) return (d->wo - 1) * step + rf->rl <= row && (d->ho - 1) * d->stride + d->r <= d->h;
  return (d->wo - 1) * step + rf->rlp <= row;
}

// filter [R*RL][N] <-> padded [R*RLP][N] (pad rows zero)
// (forward: the copy's rows are also padded to `np` >= n columns, zeros: fine/first's 63 filters become 16-byte rows)
__global__ __launch_bounds__(256) void pad_filter_kernel(const float* w, float* wp, int r, int rl, int rlp, int n, int np) {
  const int total = r * rlp * np;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int col = i % np, row = i / np;
    const int q = row % rlp, rr = row / rlp;
    wp[i] = (q < rl && col < n) ? w[(size_t)(rr * rl + q) * n + col] : 0.f;
  }
}
__global__ __launch_bounds__(256) void unpad_filter_kernel(const float* wp, float* w, int r, int rl, int rlp, int n) {
  const int total = r * rl * n;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int col = i % n, row = i / n;
    const int q = row % rl, rr = row / rl;
    w[i] = wp[(size_t)(rr * rlp + q) * n + col];
  }
}

// ---- what a candidate is told about a call's operands ----
// A call is served by one of a fixed list of candidates: the GEMM over the tensors as stored, the same on the LDS-DMA kernel, the
// window-run and bf16 image forms, conv3 / conv3b, fewch / fewch16, the stencil.  Each is written once, as a function of the
// descriptor and of what is known of the operands, and answers whether it takes the call, the GEMM it plans and the workspace it
// needs.  A launch asks the candidate it picks from its real pointers and checks ws_bytes against that answer; a *_ws_bytes query
// has the descriptor alone and takes the maximum over the list, asking with kOnGrid: every operand on the 16-byte grid, no fused
// pool, no prepared filter, a bias gradient wanted, and `known` false.  Where `known` is false the tests that need a pointer, a
// pixel stride or the epilogue count as passed, and the GEMM is planned from the descriptor's channel counts alone (no hint, no
// storage bit): every place that reads `o.known` is a query answer that a launch may exceed (tests/golden/plan_table.json pins them);
// an operand off the grid is not one of them (fit_workspace).
struct Operands {
  bool known = false;
  unsigned x = 0, w = 0, y = 0;      // address & 15 of the image-side tensor (x, dx), the filter (w, dw) and the output-side one (y, dz)
  unsigned aux = 0;                  // ... of the argmax rows (pooled forward) or the mask (bwd-data); 0 without one
  int act = A3D_ACT_NONE, pool = 0, ld_out = 0;
  bool argmax = false, prepared = false;
  bool db = true;                    // bwd-filter: the bias gradient is wanted
};
static const Operands kOnGrid{};
// ... of a launch: x / w / y as in Operands
static Operands launch_operands(const void* x, const void* w, const void* y, const void* aux) {
  auto off16 = [](const void* p) { return (unsigned)(reinterpret_cast<uintptr_t>(p) & 15); };
  Operands o;
  o.known = true;
  o.x = off16(x); o.w = off16(w); o.y = off16(y); o.aux = off16(aux);
  return o;
}

enum GemmForm { kAsStored, kLdsDma, kRunForm, kBf16Image };
struct Route {
  bool ok = false;
  RunForm rf{};           // kRunForm, kBf16Image
  GemmProblem g{};
  GemmPlan plan{};
  size_t repack = 0;      // the repacked filter at the workspace's start; the plan's slabs follow it
  size_t bytes = 0;       // all of it: repack + plan.ws_bytes + bias slabs or column-sum partials
};
static size_t upto(size_t need, const Route& r) { return r.ok ? std::max(need, r.bytes) : need; }
// A query plans with kOnGrid; an operand off the 16-byte grid plans another GEMM (scalar gathers: another tile, another split, no
// LDS-DMA twin), whose slabs may outgrow the query's answer.  include/a3d.h promises that the query's bytes are enough wherever
// the operands lie: such a launch plans its split within the bytes it was given (per_split: the bias gradient's row of a split).
static void fit_workspace(Route& r, const Operands& o, size_t ws_bytes, size_t per_split = 0) {
  if (r.bytes <= ws_bytes || !(o.x | o.w | o.y | o.aux) || r.repack > ws_bytes) return;
  r.plan = plan_within(r.g, r.plan, ws_bytes - r.repack, per_split);
  r.bytes = r.repack + r.plan.ws_bytes + (r.plan.splitk > 1 ? (size_t)r.plan.splitk * per_split : 0);
}
// `ws` is read and written in 16-byte pieces (the padded and packed filter copies at its start, the vectorised split-K reduction)
#define A3D_CHECK_WS(ws, who) A3D_CHECK_ARG(aligned16(ws), who ": ws must be 16-byte aligned")

static const int kAll16 = A3D_STORE_X_BF16 | A3D_STORE_W_BF16 | A3D_STORE_Y_BF16;
static bool stored16(const a3d_conv_desc* d, int bits) { return (d->storage & bits) == bits; }
// Forward / bwd-data: `both` operands bf16 tensors, whole 16-byte pieces inside one of at most 128 taps, the output (address & 15:
// out_off) on the grid: the LDS-DMA kernel may take the launch
static bool ring_ok(const a3d_conv_desc* d, const Operands& o, int both, unsigned out_off, int taps) {
  if (d->precision != A3D_PREC_BF16 || !stored16(d, both) || d->c % 8 || d->k % 8) return false;
  return !o.known || (d->ldx % 8 == 0 && d->ldy % 8 == 0 && taps <= 128 && !out_off);
}

// ---- descriptor checks / parameter assembly ----
static int ilog2_exact(int v) {
  for (int l = 0; l < 8; ++l)
    if ((1 << l) == v) return l;
  return -1;
}

static int check_desc(const a3d_conv_desc* d) {
  A3D_CHECK_ARG(d != nullptr, "conv: null descriptor");
  A3D_CHECK_ARG(d->n > 0 && d->h > 0 && d->w > 0 && d->c > 0 && d->k > 0 && d->r > 0 && d->s > 0, "conv: bad dims");
  A3D_CHECK_ARG(ilog2_exact(d->stride) >= 0 && d->stride <= 4, "conv: stride %d unsupported (1, 2 or 4)", d->stride);
  A3D_CHECK_ARG(d->pad_t >= 0 && d->pad_l >= 0 && d->pad_t < d->r && d->pad_l < d->s, "conv: bad padding");
  A3D_CHECK_ARG(d->ho > 0 && d->wo > 0, "conv: bad output size");
  A3D_CHECK_ARG((d->ho - 1) * d->stride - d->pad_t < d->h && (d->wo - 1) * d->stride - d->pad_l < d->w,
                "conv: output size inconsistent with input");
  A3D_CHECK_ARG(d->ldx >= d->c && d->ldy >= d->k, "conv: pixel strides smaller than channel counts");
  A3D_CHECK_ARG(d->precision >= A3D_PREC_F32 && d->precision <= A3D_PREC_F32_WINOGRAD, "conv: unknown precision %d", d->precision);
  const double lim = 2147483647.0;
  A3D_CHECK_ARG((double)d->n * d->h * d->w * d->ldx < lim && (double)d->n * d->ho * d->wo * d->ldy < lim &&
                    (double)d->r * d->s * d->c * d->k < lim,
                "conv: tensor too large for 31-bit indexing");
  // Those are ELEMENT counts: a tensor may hold up to 8 GiB.  The implicit-GEMM gathers address a tile's rows in BYTES from the
  // image of the tile's first row (igemm.h, igemm_bf16.h, igemm_ring.h: int row-table entries), so the images that a tile of up
  // to 256 rows can reach — one more than the rows cover — must lie within 2^31 bytes (4-byte elements assumed)
  auto tile_span_ok = [&](double rows_per_image, double image_elems) {
    const double images = std::min((double)d->n, std::floor(255.0 / rows_per_image) + 2.0);
    return images * image_elems * 4.0 < lim;
  };
  A3D_CHECK_ARG(tile_span_ok((double)d->ho * d->wo, (double)d->h * d->w * d->ldx) &&                                   // forward, bwd-filter: x
                    tile_span_ok(std::max(1.0, std::floor((double)d->h / d->stride) * std::floor((double)d->w / d->stride)),
                                 (double)d->ho * d->wo * d->ldy),                                                      // bwd-data: dz, per class
                "conv: single images too large for 31-bit byte offsets inside a tile");
  return A3D_OK;
}

// A3D_PREC_F32_WINOGRAD on a call the Winograd route (wino.hip) does not take runs exactly as A3D_PREC_F32 does: from this
// line on `d` is the descriptor with that value
#define A3D_AS_F32(d)                                          \
  a3d_conv_desc d##_f32;                                       \
  if ((d) && (d)->precision == A3D_PREC_F32_WINOGRAD) {        \
    d##_f32 = *(d);                                            \
    d##_f32.precision = A3D_PREC_F32;                          \
    (d) = &d##_f32;                                            \
  }

static GemmProblem fwd_problem(const a3d_conv_desc* d) {
  GemmProblem g;
  g.mode = MODE_FWD;
  g.M = d->n * d->ho * d->wo; g.N = d->k; g.K = d->r * d->s * d->c;
  g.avec = (d->c % 4 == 0 && d->ldx % 4 == 0) ? 4 : 1;
  g.bvec = (d->k % 4 == 0) ? 4 : 1;
  return g;
}
static GemmProblem bwd_d_problem(const a3d_conv_desc* d) {
  GemmProblem g;
  g.mode = MODE_BWD_D;
  g.M = d->n * d->h * d->w; g.N = d->c; g.K = d->r * d->s * d->k;
  g.avec = (d->k % 4 == 0 && d->ldy % 4 == 0) ? 4 : 1;
  g.bvec = (d->k % 4 == 0) ? 4 : 1;
  return g;
}
static GemmProblem bwd_f_problem(const a3d_conv_desc* d) {
  GemmProblem g;
  g.mode = MODE_BWD_F;
  g.M = d->r * d->s * d->c; g.N = d->k; g.K = d->n * d->ho * d->wo;
  g.avec = (d->c % 4 == 0 && d->ldx % 4 == 0) ? 4 : 1;
  g.bvec = (d->k % 4 == 0 && d->ldy % 4 == 0) ? 4 : 1;
  return g;
}

// the problem as planned for bf16 operands: gathered in 16-byte pieces, and a bf16 output is not the LDS-DMA fp32 kernels'
static void storage_vecs(GemmProblem& g, bool a16, bool b16, bool c16) {
  if (c16) g.no_glds = 1;
  if (a16) g.avec = 4;
  if (b16) g.bvec = 4;
}
// a3d_conv_desc.storage -> which GEMM operands are bf16, with the checks a 16-byte bf16 gather needs
// an / bn / cn: the operands' names in the entry point's argument list, for the message
static int apply_storage(IgemmParams& p, int precision, bool a16, bool b16, bool c16, int a_c, int a_ld, int b_c, int b_ld,
                         const void* a, const void* b, const void* c, const char* an, const char* bn, const char* cn) {
  if (!a16 && !b16 && !c16) return A3D_OK;
  // a bf16 OUTPUT alone is also served by the fp32 kernels (the 3-channel layers of config 5 keep fp32 arithmetic)
  A3D_CHECK_ARG(precision == A3D_PREC_BF16 || (precision == A3D_PREC_F32 && !a16 && !b16),
                "bf16 operands need precision A3D_PREC_BF16");
  A3D_CHECK_ARG(!a16 || (a_c % 8 == 0 && a_ld % 8 == 0 && aligned16(a)), "bf16 %s: channels / stride must be multiples of 8, base 16-byte aligned", an);
  // b_c < 0: a row-major [rows][b_ld] operand read in whole 16-byte chunks (its pad columns must be readable zeros)
  A3D_CHECK_ARG(!b16 || ((b_c < 0 || b_c % 8 == 0) && b_ld % 8 == 0 && aligned16(b)), "bf16 %s: channels / stride must be multiples of 8, base 16-byte aligned", bn);
  A3D_CHECK_ARG(!c16 || aligned16(c), "bf16 %s: base must be 16-byte aligned", cn);
  p.a16 = a16; p.b16 = b16; p.c16 = c16;
  return A3D_OK;
}

static void fill_common(IgemmParams& p, const GemmProblem& g) {
  p = IgemmParams{};
  p.M = g.M; p.N = g.N; p.K = g.K;
  p.mask_scale = 1.f;
  p.mask_act = EPI_RELU;
  p.sub_step = 1;
}

// Staging parameters of igemm_body (call after S, Cg, H, W, stride and the paddings are set): operand extents for the
// buffer descriptors, the wave-uniform tap decode for layers whose gathered channel count is a multiple of BK = 32, and
// whether the gather can leave the image at all.
static void fill_staging(IgemmParams& p, int mode, unsigned long long a_elems, unsigned long long b_elems, int taps_r,
                         int taps_s) {
  p.a_elems = a_elems;
  p.b_elems = b_elems;
  p.ntaps = std::max(1, taps_r * taps_s);
  p.cpt = std::max(1, p.Cg / 32);
  p.uni = (mode != MODE_BWD_F) && p.Cg % 32 == 0 && p.K == p.ntaps * p.Cg;
  p.kperm = p.uni && p.ntaps > 1 && p.cpt > 1;
  p.div_cpt = make_fastdiv(p.cpt);
  p.div_taps = make_fastdiv(p.ntaps);
  p.cpt64 = std::max(1, p.Cg / 64);
  p.uni64 = p.uni && p.Cg % 64 == 0;
  p.kperm64 = p.uni64 && p.ntaps > 1 && p.cpt64 > 1;
  p.div_cpt64 = make_fastdiv(p.cpt64);
}

// The gather's geometry for a launch that reads d's input image (pixel stride `ld`) through d's windows: filter rows of S
// taps over Cg gathered channels, the GEMM's pixel axis decoded over d's output grid.
static void fill_gather(IgemmParams& p, const a3d_conv_desc* d, int ld, int S, int Cg) {
  p.H = d->h; p.W = d->w; p.ld = ld; p.pHW = d->h * d->w;
  p.stride = d->stride; p.lstride = ilog2_exact(d->stride); p.pad_t = d->pad_t; p.pad_l = d->pad_l;
  p.S = S; p.Cg = Cg;
  p.div_phw = make_fastdiv(d->ho * d->wo); p.div_pw = make_fastdiv(d->wo);
  p.div_c = make_fastdiv(Cg); p.div_s = make_fastdiv(S);
  p.div_c_half = make_fastdiv(std::max(1, Cg / 2));
}
// ... with the 2x2 max pool in the epilogue: the pixel axis runs over pool windows of four, the output is the pooled map
static void fill_pool(IgemmParams& p, const a3d_conv_desc* d, uint8_t* argmax, int ld_out) {
  const int ph = d->ho / 2, pw = d->wo / 2;
  p.pool = 1;
  p.argmax = argmax;
  p.div_phw = make_fastdiv(ph * pw * 4); p.div_pw = make_fastdiv(pw);
  p.ldc = ld_out;
}

// GEMM rows of a forward: output pixels or, with the 2x2 max pool in the epilogue, pool windows x 4
static int fwd_rows(const a3d_conv_desc* d, int pool) {
  return pool ? d->n * (d->ho / 2) * (d->wo / 2) * 4 : d->n * d->ho * d->wo;
}

// ---- the few-channel kernels as the timing list sees them (a3d_timing_*); m: fwd_rows ----
// lds_dma 2: conv3_fwd_kernel (filter repack included in ms)
static a3d_timing_record conv3_record(const a3d_conv_desc* d, int m) {
  return timing_record(MODE_FWD, A3D_PREC_F32, 64, d->k > 64 ? 96 : 64, 1, 1, 8, 4, 4, 2, m, d->k, d->r * d->s * d->c);
}
// conv3b_fwd_kernel; k, flops: algorithmic, the image's three real channels
static a3d_timing_record conv3b_record(const a3d_conv_desc* d, int m) {
  return timing_record(MODE_FWD, A3D_PREC_BF16, 64, d->k > 64 ? 96 : 64, 1, 1, 16, 4, 4, 2, m, d->k, d->r * d->s * 3);
}
// lds_dma 4: fewch_bwdf_kernel, ms includes the slab reduction
static a3d_timing_record fewch_record(const a3d_conv_desc* d) {
  return timing_record(MODE_BWD_F, A3D_PREC_F32, 128, (d->k + 31) / 32 * 32, 4, 4, 2, 1, 1, 4, d->r * d->s * d->c, d->k, d->n * d->ho * d->wo);
}
// ... fewch16_bwdf_kernel
static a3d_timing_record fewch16_record(const a3d_conv_desc* d) {
  return timing_record(MODE_BWD_F, A3D_PREC_BF16, 128, (d->k + 31) / 32 * 32, 4, 4, 16, 1, 1, 4, d->r * d->s * d->c, d->k, d->n * d->ho * d->wo);
}

// ---- window-run form over a bf16 image of 8-byte pixels (4 channels; a3d_pad_channels_bf16) ----
// Seen through its float view a pixel is 2 floats, so at an even stride the runs of a filter row start 16 bytes apart and
// the bf16 kernel gathers them with its 16-byte loads: K = (r, run of s*4 bf16 padded to a multiple of 8), the filter
// [r][s][4][k] float32 is repacked per call as bf16 [r][run][k padded to 8] (pad rows / columns zero).  rf: in bf16 elements.
static bool bf16_image_form_ok(const a3d_conv_desc* d, const Operands& o, RunForm* rf) {
  rf->vec = 4;
  rf->rl = d->s * 4;
  rf->rlp = (d->s * 2 + 3) / 4 * 4 * 2;
  rf->kp = d->r * rf->rlp;
  rf->np = (d->k + 7) / 8 * 8;
  rf->bytes = up256((size_t)rf->kp * rf->np * 2);
  if (!(d->storage & A3D_STORE_X_BF16) || d->c != 4 || d->ldx != 4) return false;
  if (!o.known) return true;
  if ((d->storage & A3D_STORE_W_BF16) || d->precision != A3D_PREC_BF16) return false;
  if (d->pad_t || d->pad_l || d->stride % 2 || (d->w * 2) % 4 || o.x) return false;
  return (d->wo - 1) * d->stride * 2 + rf->rlp / 2 <= d->w * 2;      // (view floats) the last column's padded run stays inside its row
}
// filter [r][rl][n] float32 -> bf16 [r][rlp][np], pad rows / columns zero
__global__ __launch_bounds__(256) void pad_filter_bf16_kernel(const float* w, __bf16* wp, int r, int rl, int rlp, int n, int np) {
  const int total = r * rlp * np;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int col = i % np, row = i / np;
    const int q = row % rlp, rr = row / rlp;
    wp[i] = (__bf16)((q < rl && col < n) ? w[(size_t)(rr * rl + q) * n + col] : 0.f);
  }
}
// the filter padded for the window-run form (float32) or for the bf16 image form (bf16) into wp
static int pad_filter(const a3d_conv_desc* d, const RunForm& rf, bool bf16, const float* w, void* wp, hipStream_t st) {
  const dim3 grid((rf.kp * rf.np + 255) / 256), block(256);
  clear_stale_error();
  if (bf16)
    hipLaunchKernelGGL(pad_filter_bf16_kernel, grid, block, 0, st, w, static_cast<__bf16*>(wp), d->r, rf.rl, rf.rlp, d->k, rf.np);
  else
    hipLaunchKernelGGL(pad_filter_kernel, grid, block, 0, st, w, static_cast<float*>(wp), d->r, rf.rl, rf.rlp, d->k, rf.np);
  return check_launch(bf16 ? "pad_filter_bf16" : "pad_filter");
}

// Does this form take the forward?  (kLdsDma, pooled: the pooled map's pixel stride and the argmax rows in whole 16-byte pieces too)
static bool fwd_form_ok(const a3d_conv_desc* d, const Operands& o, GemmForm form, RunForm* rf) {
  if (form == kRunForm) return run_form_ok(d, o.x, rf);
  if (form == kBf16Image) return bf16_image_form_ok(d, o, rf);
  if (form == kAsStored || !ring_ok(d, o, A3D_STORE_X_BF16 | A3D_STORE_W_BF16, o.y, d->r * d->s)) return form == kAsStored;
  return !o.known || (o.act != A3D_ACT_SIGMOID && (!o.pool || ((d->storage & A3D_STORE_Y_BF16) && o.ld_out % 8 == 0 &&
                                                               (!o.argmax || (d->k % 16 == 0 && !o.aux)))));
}
// The forward as a GEMM: over the tensors as stored, the same offered to the LDS-DMA kernel, or in the window-run / bf16 image
// form (K = (r, padded run), the filter padded into the workspace)
static Route fwd_gemm(const a3d_conv_desc* d, const Operands& o, GemmForm form) {
  Route r;
  if (!(r.ok = fwd_form_ok(d, o, form, &r.rf))) return r;
  GemmProblem& g = r.g;
  g = fwd_problem(d);
  g.M = fwd_rows(d, o.pool); g.plain = o.pool ? 1 : 0;
  if (o.x) g.avec = 1;
  if (o.w) g.bvec = 1;
  if (form == kRunForm || form == kBf16Image) {
    g.K = r.rf.kp; g.avec = r.rf.vec;
    if (!o.prepared) r.repack = r.rf.bytes;      // (prepared: w already is the padded filter, a3d_conv2d_fwd_prepare_filter)
  }
  if (form == kBf16Image) { g.bvec = 4; g.no_glds = 1; }
  if (form == kLdsDma) { g.ring_ok = 1; g.avec = g.bvec = 4; }
  if (o.known) {
    if (d->hints & A3D_HINT_SHARE_CU) g.no_glds = 1;      // the register-staged kernels take the hint (launch_one)
    if (form == kRunForm) g.bvec = 4;                     // the padded copy starts the workspace (16-byte aligned: A3D_CHECK_WS), its rows are whole 16-byte pieces
    storage_vecs(g, d->storage & A3D_STORE_X_BF16, d->storage & A3D_STORE_W_BF16, d->storage & A3D_STORE_Y_BF16);
  }
  r.plan = plan_gemm(g, d->precision);
  r.bytes = r.repack + r.plan.ws_bytes;
  return r;
}

}  // namespace a3d

using namespace a3d;

// ---- what the Winograd routes share in the front end: a plane's product, the workspace queries, the filter's transform ----
// The surrogate descriptor of one plane's product: an r x 1 convolution (stride 1, vertical padding pad_t) of n images h x w of c
// channels onto ho x w pixels of k, every tensor densely packed.  F(2x2,3x3) is its r = 1 case over T one-pixel images.
static a3d_conv_desc plane_desc(int n, int h, int w, int ho, int c, int k, int r, int pad_t) {
  a3d_conv_desc e{};
  e.n = n; e.h = h; e.w = w; e.ho = ho; e.wo = w; e.c = c; e.k = k; e.r = r; e.s = 1; e.stride = 1; e.pad_t = pad_t; e.ldx = c; e.ldy = k;
  return e;
}
// One plane's product as the GEMM bodies take it.  MODE_FWD: C [pixels][k] = conv(A, B [r c][k]); MODE_BWD_F: C [r c][k] = the
// filter gradient from A (the image) and B (the gradient tensor), dbias its [splits][k] bias partials or null.
static IgemmParams plane_product(int mode, const a3d_conv_desc& e, const float* A, const float* B, float* C, float* dbias,
                                 unsigned long long a_elems, unsigned long long b_elems, int taps_r) {
  const bool filt = mode == MODE_BWD_F;
  const GemmProblem gp = filt ? bwd_f_problem(&e) : fwd_problem(&e);
  IgemmParams p;
  fill_common(p, gp);
  p.A = A; p.B = B; p.C = C; p.dbias = dbias;
  p.npix = filt ? gp.K : gp.M; p.nrsc = filt ? gp.M : gp.K;
  fill_gather(p, &e, e.c, 1, e.c);
  p.ldb = e.k; p.ldc = e.k;
  fill_staging(p, mode, a_elems, b_elems, taps_r, 1);
  return p;
}
// the bytes a layout (a3d_internal.h) takes: its carve from offset 0
template <typename Geom>
static size_t product_ws_bytes(const Geom& g, bool prepared) {
  Carve c{0};
  carve_product(c, g, prepared);
  return c.at;
}
template <typename Geom>
static size_t grad_ws_bytes(const Geom& g) {
  Carve c{0};
  carve_grad(c, g);
  return c.at;
}
// U: the prepared transform `w` (on the 16-byte grid), or `w` transformed by xform into the workspace's head
template <typename Xform>
static int transformed_filter(const char* who, bool prepared, const float* w, float* head, const float*& U, Xform&& xform) {
  A3D_CHECK_ARG(!prepared || aligned16(w), "%s: the prepared filter must be 16-byte aligned", who);
  U = prepared ? w : head;
  return prepared ? A3D_OK : xform(head);
}

extern "C" {

// ---- A3D_PREC_F32_WINOGRAD (wino.hip): workspace [U unless prepared][V][M] ----

static size_t wino_bytes(const a3d_conv_desc* d, bool bwd, bool prepared) { return product_ws_bytes(wino_geom(d, bwd), prepared); }
// one of the sixteen products: T rows of Kp gathered channels (a 1x1 conv over T one-pixel images) against U[xi] [Kp][Np]
static IgemmParams wino_product(const WinoGeom& g, const float* V, const float* U, float* M) {
  return plane_product(MODE_FWD, plane_desc((int)g.T, 1, 1, 1, g.Kp, g.Np, 1, 0), V, U, M, nullptr, (unsigned long long)g.T * g.Kp,
                       (unsigned long long)g.Kp * g.Np, 1);
}
// forward (dz = x, dx = y, bias + act) or bwd-data (mask) of a descriptor wino_applicable() accepted; `w`: the filter, or its
// transform when prepared
static int wino_conv(const a3d_conv_desc* d, bool bwd, const float* src, const float* w, float* out, const float* bias, const float* mask,
                     int act, bool prepared, void* ws, size_t ws_bytes, hipStream_t st) {
  const WinoGeom g = wino_geom(d, bwd);
  Carve c{reinterpret_cast<uintptr_t>(ws)};
  const ProductWs at = carve_product(c, g, prepared);
  const size_t need = c.at - reinterpret_cast<uintptr_t>(ws);
  if (!ws || need > ws_bytes) return set_error(A3D_EWORKSPACE, "conv2d (Winograd): need %zu workspace bytes", need);
  const float* U;
  int rc = transformed_filter("conv2d (Winograd)", prepared, w, at.U, U, [&](float* u) { return wino_filter(d, bwd, w, u, st); });
  if (rc != A3D_OK) return rc;
  rc = wino_input(d, bwd, src, at.V, st);
  if (rc != A3D_OK) return rc;
  IgemmParams p = wino_product(g, at.V, U, at.M);
  rc = timed_launch(wino_record(bwd ? MODE_BWD_D : MODE_FWD, g), st, [&] { return wino_gemm(p, g, st); });
  if (rc != A3D_OK) return rc;
  return wino_output(d, bwd, at.M, out, bias, mask, act, st);
}

size_t a3d_conv2d_fwd_ws_bytes(const a3d_conv_desc* d) {
  if (check_desc(d) != A3D_OK) return 0;
  const size_t wino = wino_applicable(d) ? wino_bytes(d, false, (d->hints & A3D_HINT_W_PREPARED) != 0) : 0;
  A3D_AS_F32(d);
  if (stencil1_applicable(d)) return 0;
  if (wino) return std::max(wino, a3d_conv2d_fwd_ws_bytes(d));      // (the _ex2 form with a second output runs direct)
  // (a maximum over the paths a launch may take: which one it is also depends on the operands' alignment)
  size_t need = 0;
  for (GemmForm form : {kAsStored, kLdsDma, kRunForm, kBf16Image}) need = upto(need, fwd_gemm(d, kOnGrid, form));
  RunForm rf;
  if (bf16_image_form_ok(d, kOnGrid, &rf)) need = std::max(need, conv3b_filter_bytes(d));
  if (conv3_applicable(d, kOnGrid.x)) need = std::max(need, conv3_ws_bytes(d));
  return need;
}

// conv2d forward; pool != 0: y is the 2x2 / stride-2 max pool of the activated conv output, [n, ho/2, wo/2, k] with
// pixel stride ld_out, and the conv output itself is never written
static int conv_fwd_impl(const a3d_conv_desc* d, const float* x, const float* w, const float* bias, float* y, int act,
                         int pool, int ld_out, uint8_t* argmax, void* ws, size_t ws_bytes, void* stream,
                         const a3d_second_output* out2 = nullptr) {
  int rc = check_desc(d);
  if (rc != A3D_OK) return rc;
  if (!ws) ws_bytes = 0;
  if (wino_applicable(d) && !pool && !(out2 && out2->ptr)) {
    A3D_CHECK_ARG(x && w && y, "conv2d_fwd: null tensor");
    A3D_CHECK_WS(ws, "conv2d_fwd");
    A3D_CHECK_ARG(act == A3D_ACT_NONE || act == A3D_ACT_RELU || act == A3D_ACT_SIGMOID, "conv2d_fwd: bad act");
    return wino_conv(d, false, x, w, y, bias, nullptr, act, (d->hints & A3D_HINT_W_PREPARED) != 0, ws, ws_bytes,
                     static_cast<hipStream_t>(stream));
  }
  // the prepared filter of an 'fp32w' descriptor is the Winograd transform: the direct forwards (fused pool, second output) cannot read it
  A3D_CHECK_ARG(!(wino_applicable(d) && (d->hints & A3D_HINT_W_PREPARED)),
                "conv2d_fwd: A3D_HINT_W_PREPARED with A3D_PREC_F32_WINOGRAD is for the plain forward only (no fused pool, no second output)");
  A3D_AS_F32(d);
  Operands o = launch_operands(x, w, y, argmax);
  o.act = act; o.pool = pool; o.ld_out = ld_out; o.argmax = argmax != nullptr;
  o.prepared = (d->hints & A3D_HINT_W_PREPARED) != 0;
  RunForm rf;
  const bool image = fwd_form_ok(d, o, kBf16Image, &rf);
  A3D_CHECK_ARG(!(out2 && out2->ptr) || (!pool && !stencil1_applicable(d) && !image && !conv3_applicable(d, o.x)),
                "conv2d_fwd_ex2: a second output on the implicit-GEMM forwards only (no fused pool, no few-channel / one-filter kernels)");
  A3D_CHECK_ARG(x && w && y, "conv2d_fwd: null tensor");
  A3D_CHECK_WS(ws, "conv2d_fwd");
  A3D_CHECK_ARG(act == A3D_ACT_NONE || act == A3D_ACT_RELU || act == A3D_ACT_SIGMOID, "conv2d_fwd: bad act");
  if (pool) {
    A3D_CHECK_ARG(d->precision == A3D_PREC_F32 || image ||
                      (d->precision == A3D_PREC_BF16 && (stored16(d, kAll16) || d->storage == A3D_STORE_Y_BF16)),
                  "conv2d_pool_fwd: fp32, the bf16 image form (4-channel bf16 image, a3d_pad_channels_bf16), or bf16 arithmetic on "
                  "bf16 x, w and y (LDS-DMA kernel)");
    A3D_CHECK_ARG(d->ho >= 2 && d->wo >= 2 && ld_out >= d->k, "conv2d_pool_fwd: output smaller than one pool window");
    A3D_CHECK_ARG(!stencil1_applicable(d), "conv2d_pool_fwd: single-output-channel convs are not supported");
  } else if (stencil1_applicable(d)) {
    A3D_CHECK_ARG(!d->storage, "conv2d_fwd: single-output-channel convs take float32 tensors");
    return stencil1_fwd(d, x, w, bias, y, act, static_cast<hipStream_t>(stream));
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (image && conv3b_applicable(d))             // straight from L2 on the bf16 matrix cores (conv3.hip, conv3b_fwd_kernel)
    return timed_launch(conv3b_record(d, fwd_rows(d, pool)), st,
                        [&] { return conv3b_fwd(d, x, w, bias, y, act, pool, ld_out, argmax, ws, ws_bytes, st, o.prepared); });
  if (!image && conv3_applicable(d, o.x))        // few-channel layers: operands straight from L2 (conv3.hip)
    return timed_launch(conv3_record(d, fwd_rows(d, pool)), st,
                        [&] { return conv3_fwd(d, x, w, bias, y, act, pool, ld_out, argmax, ws, ws_bytes, st, o.prepared); });
  // the window-run form if the workspace holds its padded filter; else the tensors as stored, on the LDS-DMA kernel where that may be
  const bool run = !image && fwd_form_ok(d, o, kRunForm, &rf) && (o.prepared || rf.bytes <= ws_bytes), padded = run || image;
  Route r = fwd_gemm(d, o, image ? kBf16Image : run ? kRunForm : fwd_form_ok(d, o, kLdsDma, &rf) ? kLdsDma : kAsStored);
  fit_workspace(r, o, ws_bytes);
  // (the prepared layout was chosen for a 16-byte aligned x — fwd_filter_form — and this launch reads it with THAT row padding)
  A3D_CHECK_ARG(!o.prepared || (padded && !o.w && !o.x),
                "conv2d_fwd: A3D_HINT_W_PREPARED on a launch that reads the filter as stored, or with x off the 16-byte grid");
  IgemmParams p;
  fill_common(p, r.g);
  const int sb = d->storage;
  if (image) {
    p.a16 = 1; p.b16 = 1; p.c16 = (sb & A3D_STORE_Y_BF16) ? 1 : 0;
  } else {
    A3D_CHECK_ARG(!sb || ((!pool || sb == A3D_STORE_Y_BF16 || (sb == kAll16 && d->precision == A3D_PREC_BF16)) &&
                          !(run && (sb & A3D_STORE_W_BF16))),
                  "conv2d_fwd: the fused pool takes float32 inputs (its output may be bf16) or bf16 x, w and y; 3-channel filters stay float32");
    rc = apply_storage(p, d->precision, sb & A3D_STORE_X_BF16, sb & A3D_STORE_W_BF16, sb & A3D_STORE_Y_BF16, d->c, d->ldx, d->k, d->k,
                       x, w, y, "x", "w", "y");
    if (rc != A3D_OK) return rc;
    A3D_CHECK_ARG(!(pool && (p.a16 || p.b16)) || r.plan.ring,
                  "conv2d_pool_fwd: on bf16 inputs the fused pool is the LDS-DMA kernel's (channels and strides in whole 16-byte pieces, k %% 16 == 0)");
  }
  if (r.bytes > ws_bytes) return set_error(A3D_EWORKSPACE, "conv2d_fwd: need %zu workspace bytes", r.bytes);
  A3D_CHECK_ARG(!image || (r.plan.prec == A3D_PREC_BF16 && !o.y), "conv2d_fwd: bf16 image form needs the bf16 kernel");
  A3D_CHECK_ARG(!(p.a16 || p.b16) || r.plan.prec == A3D_PREC_BF16, "conv2d_fwd: bf16 operands need vectorisable tensors");
  A3D_CHECK_ARG(!p.c16 || r.plan.prec == A3D_PREC_BF16 || !is_glds_cfg(r.plan.cfg), "conv2d_fwd: no bf16 output from the LDS-DMA kernels");
  const float* filter = w;
  if (padded && !o.prepared) {
    rc = pad_filter(d, r.rf, image, w, ws, st);
    if (rc != A3D_OK) return rc;
    filter = static_cast<const float*>(ws);
  }
  const int ldb = padded ? r.rf.np : d->k;
  p.A = x; p.B = filter; p.C = y; p.bias = bias; p.act = act;
  p.share = (d->hints & A3D_HINT_SHARE_CU) ? 1 : 0;
  p.npix = r.g.M; p.nrsc = r.g.K;
  fill_gather(p, d, d->ldx, padded ? 1 : d->s, padded ? r.rf.rlp : d->c);
  p.ldb = ldb; p.ldc = d->ldy;
  if (pool) fill_pool(p, d, argmax, ld_out);
  fill_staging(p, MODE_FWD, (unsigned long long)d->n * d->h * d->w * d->ldx, (unsigned long long)r.g.K * ldb, d->r, padded ? 1 : d->s);
  rc = take_second_output(p, out2);
  if (rc != A3D_OK) return rc;
  return launch_igemm(MODE_FWD, r.plan, r.g.avec, r.g.bvec, p, static_cast<char*>(ws) + r.repack, st);
}

int a3d_conv2d_fwd(const a3d_conv_desc* d, const float* x, const float* w, const float* bias, float* y, int act,
                   void* ws, size_t ws_bytes, void* stream) {
  return conv_fwd_impl(d, x, w, bias, y, act, 0, 0, nullptr, ws, ws_bytes, stream);
}

// Which per-call repack of the filter does this forward do?  0 none, 1 bf16 image form, 2 conv3's [K/4][N][4], 3 window-run padding
static int fwd_filter_form(const a3d_conv_desc* d, RunForm* rf) {
  if (check_desc(d) != A3D_OK || stencil1_applicable(d)) return 0;
  const Operands o = launch_operands(nullptr, nullptr, nullptr, nullptr);      // the layout a launch with every operand on the 16-byte grid reads
  if (bf16_image_form_ok(d, o, rf)) return 1;
  if (conv3_applicable(d, o.x)) return 2;
  if (run_form_ok(d, o.x, rf)) return 3;
  return 0;
}

size_t a3d_conv2d_fwd_prepared_filter_bytes(const a3d_conv_desc* d) {
  if (check_desc(d) == A3D_OK && wino_applicable(d)) return wino_geom(d, false).u_bytes;      // the transformed filter U
  A3D_AS_F32(d);
  RunForm rf{};
  switch (fwd_filter_form(d, &rf)) {
    case 1: return conv3b_applicable(d) ? conv3b_filter_bytes(d) : rf.bytes;
    case 2: return conv3_ws_bytes(d);
    case 3: return rf.bytes;
    default: return 0;
  }
}

int a3d_conv2d_fwd_prepare_filter(const a3d_conv_desc* d, const float* w, void* prepared, size_t prepared_bytes, void* stream) {
  int rc = check_desc(d);
  if (rc != A3D_OK) return rc;
  A3D_CHECK_ARG(w && prepared && aligned16(prepared), "conv2d_fwd_prepare_filter: null or misaligned buffer");
  const size_t need = a3d_conv2d_fwd_prepared_filter_bytes(d);
  A3D_CHECK_ARG(need > 0, "conv2d_fwd_prepare_filter: this forward reads the filter as stored");
  if (prepared_bytes < need) return set_error(A3D_EWORKSPACE, "conv2d_fwd_prepare_filter: need %zu bytes", need);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (wino_applicable(d)) return wino_filter(d, false, w, static_cast<float*>(prepared), st);
  A3D_AS_F32(d);
  RunForm rf{};
  switch (fwd_filter_form(d, &rf)) {
    case 1: return conv3b_applicable(d) ? conv3b_pack(d, w, prepared, st) : pad_filter(d, rf, true, w, prepared, st);
    case 2: return conv3_pack(d, w, static_cast<float*>(prepared), st);
    default: return pad_filter(d, rf, false, w, prepared, st);
  }
}

int a3d_conv2d_fwd_ex2(const a3d_conv_desc* d, const float* x, const float* w, const float* bias, float* y, int act,
                       const a3d_second_output* out2, void* ws, size_t ws_bytes, void* stream) {
  return conv_fwd_impl(d, x, w, bias, y, act, 0, 0, nullptr, ws, ws_bytes, stream, out2);
}

int a3d_conv2d_pool_fwd(const a3d_conv_desc* d, const float* x, const float* w, const float* bias, float* y_pooled,
                        int ld_pooled, uint8_t* argmax, int act, void* ws, size_t ws_bytes, void* stream) {
  return conv_fwd_impl(d, x, w, bias, y_pooled, act, 1, ld_pooled, argmax, ws, ws_bytes, stream);
}

// One parity class (ph, pw) of a strided bwd-data as a stride-1 problem; false if the class has no pixels.
struct BwdDClass {
  int ph, pw, hc, wc, r0, s0, rp, sp, off_y, off_x;
  GemmProblem g;
};
static bool bwd_d_class(const a3d_conv_desc* d, int ph, int pw, BwdDClass* c) {
  const int st = d->stride;
  c->ph = ph; c->pw = pw;
  c->hc = (d->h - ph + st - 1) / st;
  c->wc = (d->w - pw + st - 1) / st;
  if (c->hc <= 0 || c->wc <= 0) return false;
  c->r0 = (ph + d->pad_t) % st;
  c->s0 = (pw + d->pad_l) % st;
  c->rp = c->r0 < d->r ? (d->r - c->r0 + st - 1) / st : 0;
  c->sp = c->s0 < d->s ? (d->s - c->s0 + st - 1) / st : 0;
  c->off_y = (ph + d->pad_t - c->r0) / st;
  c->off_x = (pw + d->pad_l - c->s0) / st;
  c->g = bwd_d_problem(d);
  c->g.M = d->n * c->hc * c->wc;
  c->g.K = c->rp * c->sp * d->k;          // 0: no tap reaches this class, the launch only writes zeros
  return true;
}
// the classes that have pixels (a stride-1 conv is its one class); returns their number
static int bwd_d_classes(const a3d_conv_desc* d, BwdDClass (&cls)[16]) {
  int n = 0;
  for (int ph = 0; ph < d->stride; ++ph)
    for (int pw = 0; pw < d->stride; ++pw)
      if (bwd_d_class(d, ph, pw, &cls[n])) ++n;
  return n;
}

// One class as a GEMM over the tensors as stored, or (stride 1, the mask on the 16-byte grid too) the same offered to the LDS-DMA
// kernel; tiles: the plan is this one, nothing is searched
static Route bwd_d_gemm(const a3d_conv_desc* d, const BwdDClass& c, const Operands& o, GemmForm form, const GemmPlan* tiles = nullptr) {
  Route r;
  r.ok = form == kAsStored || (d->stride == 1 && !o.aux && ring_ok(d, o, A3D_STORE_Y_BF16 | A3D_STORE_W_BF16, o.x, c.rp * c.sp));
  if (!r.ok) return r;
  r.g = c.g;
  if (o.y) r.g.avec = 1;
  if (o.w) r.g.bvec = 1;
  if (form == kLdsDma) { r.g.ring_ok = 1; r.g.avec = r.g.bvec = 4; }
  if (o.known) storage_vecs(r.g, d->storage & A3D_STORE_Y_BF16, d->storage & A3D_STORE_W_BF16, d->storage & A3D_STORE_X_BF16);
  r.plan = tiles ? *tiles : plan_gemm(r.g, d->precision);
  r.bytes = r.plan.ws_bytes;
  return r;
}

size_t a3d_conv2d_bwd_data_ws_bytes(const a3d_conv_desc* d) {
  if (check_desc(d) != A3D_OK) return 0;
  if (wino_applicable(d)) return wino_bytes(d, true, (d->hints & A3D_HINT_W_PREPARED) != 0);
  A3D_AS_F32(d);
  BwdDClass cls[16];
  const int ncls = bwd_d_classes(d, cls);
  size_t need = 0;
  for (int i = 0; i < ncls; ++i)
    for (GemmForm form : {kAsStored, kLdsDma}) need = upto(need, bwd_d_gemm(d, cls[i], kOnGrid, form));
  return need;
}

// The parameters of one class's launch: the class is a stride-1 problem over dz
static void fill_bwd_d_class(IgemmParams& p, const a3d_conv_desc* d, const BwdDClass& c, const float* dz, const float* w, float* dx,
                             const float* relu_mask) {
  p.A = dz; p.B = w; p.C = dx; p.mask = relu_mask;
  p.npix = p.M; p.nrsc = p.K;
  p.H = d->ho; p.W = d->wo; p.ld = d->ldy; p.pHW = d->ho * d->wo;
  p.stride = 1; p.lstride = 0; p.pad_t = c.off_y; p.pad_l = c.off_x;
  p.S = std::max(c.sp, 1); p.Cg = d->k; p.Cn = d->c;
  p.div_phw = make_fastdiv(c.hc * c.wc); p.div_pw = make_fastdiv(c.wc);
  p.div_c = make_fastdiv(d->k); p.div_s = make_fastdiv(std::max(c.sp, 1));
  p.div_c_half = make_fastdiv(std::max(1, d->k / 2));
  p.ldb = 0; p.ldc = d->ldx;
  p.sub_step = d->stride; p.sub_ph = c.ph; p.sub_pw = c.pw; p.tap_r0 = c.r0; p.tap_s0 = c.s0; p.S_full = d->s;
  p.outW = d->w; p.outHW = d->h * d->w;
  fill_staging(p, MODE_BWD_D, (unsigned long long)d->n * d->ho * d->wo * d->ldy, (unsigned long long)d->r * d->s * d->c * d->k, c.rp,
               c.sp);
}

int a3d_conv2d_bwd_data(const a3d_conv_desc* d, const float* dz, const float* w, float* dx, const float* relu_mask,
                        void* ws, size_t ws_bytes, void* stream) {
  int rc = check_desc(d);
  if (rc != A3D_OK) return rc;
  A3D_CHECK_ARG(dz && w && dx, "conv2d_bwd_data: null tensor");
  A3D_CHECK_WS(ws, "conv2d_bwd_data");
  if (!ws) ws_bytes = 0;
  if (wino_applicable(d))
    return wino_conv(d, true, dz, w, dx, nullptr, relu_mask, A3D_ACT_NONE, (d->hints & A3D_HINT_W_PREPARED) != 0, ws, ws_bytes,
                     static_cast<hipStream_t>(stream));
  A3D_AS_F32(d);
  const Operands o = launch_operands(dx, w, dz, relu_mask);
  hipStream_t st = static_cast<hipStream_t>(stream);
  BwdDClass cls[16];
  const int ncls = bwd_d_classes(d, cls);
  // stride 2, fp32: the (up to) four classes as ONE launch of 64x64 tiles when that alone fills the chip; under 256 tiles that
  // is too little work without split-K: one launch per class
  long tiles64 = 0;
  for (int i = 0; i < ncls; ++i) tiles64 += (long)((cls[i].g.M + 63) / 64) * ((cls[i].g.N + 63) / 64);
  const bool multi32 = d->stride == 2 && d->precision == A3D_PREC_F32 && !d->storage && tune_int("A3D_FORCE_CFG", -1) < 0 && tiles64 >= 256;
  // ... and on bf16-stored tensors (BASELINE config 5's conv2d_4): one launch of the bf16 kernel's 128-row tiles
  const bool multi16 = d->stride == 2 && d->precision == A3D_PREC_BF16 && stored16(d, kAll16) && !o.y && !o.w &&
                       tune_int("A3D_FORCE_SPLITK", 0) <= 0;
  IgemmMulti multi;
  int avec = 4, bvec = 4, multi16_bn = 0;
  unsigned multi_grid = 0;
  double multi_flops = 0;                    // the classes' own, summed: a class runs only the taps that reach it
  for (int i = 0; i < ncls; ++i) {
    const BwdDClass& c = cls[i];
    GemmPlan tiles64{};                      // multi32: 64x64 tiles, no split-K, no workspace
    tiles64.cfg = 4; tiles64.splitk = 1; tiles64.ktiles_per_split = std::max(1, (c.g.K + 31) / 32);
    tiles64.tiles_m = (c.g.M + 63) / 64; tiles64.tiles_n = (c.g.N + 63) / 64;
    Route r = bwd_d_gemm(d, c, o, kLdsDma);
    if (!r.ok) r = bwd_d_gemm(d, c, o, kAsStored, multi32 ? &tiles64 : nullptr);
    IgemmParams p;
    fill_common(p, r.g);
    rc = apply_storage(p, d->precision, d->storage & A3D_STORE_Y_BF16, d->storage & A3D_STORE_W_BF16, d->storage & A3D_STORE_X_BF16,
                       d->k, d->ldy, d->k, d->k, dz, w, dx, "dz", "w", "dx");
    if (rc != A3D_OK) return rc;
    A3D_CHECK_ARG(!p.c16 || !o.aux, "conv2d_bwd_data: bf16 mask must be 16-byte aligned");
    A3D_CHECK_ARG(!d->storage || r.plan.prec == A3D_PREC_BF16, "conv2d_bwd_data: bf16 storage needs vectorisable operands");
    if (multi16) {                           // the bf16 kernel's tiles, no split-K, no workspace
      multi16_bn = r.plan.bf16_bn;
      r.plan.splitk = 1; r.plan.ktiles_per_split = std::max(1, (r.g.K + 63) / 64);
    } else if (!multi32) {
      fit_workspace(r, o, ws_bytes);
      if (r.bytes > ws_bytes) return set_error(A3D_EWORKSPACE, "conv2d_bwd_data: need %zu workspace bytes", r.bytes);
    }
    fill_bwd_d_class(p, d, c, dz, w, dx, relu_mask);
    if (!multi32 && !multi16) {
      rc = launch_igemm(MODE_BWD_D, r.plan, r.g.avec, r.g.bvec, p, ws, st);
      if (rc != A3D_OK) return rc;
      continue;
    }
    p.splitk = 1; p.ktiles_per_split = r.plan.ktiles_per_split; p.tiles_m = r.plan.tiles_m; p.tiles_n = r.plan.tiles_n;
    p.slab = (size_t)p.M * p.N;
    multi.p[i] = p;
    avec = std::min(avec, r.g.avec); bvec = std::min(bvec, r.g.bvec);
    multi_grid = std::max(multi_grid, (unsigned)((long)r.plan.tiles_m * r.plan.tiles_n));
    multi_flops += 2.0 * p.M * p.N * p.K;
  }
  if (!multi32 && !multi16) return A3D_OK;
  a3d_timing_record rec = multi16 ? timing_record(MODE_BWD_D, A3D_PREC_BF16, 128, multi16_bn, 4, 8, 64, 4, 4, 0, d->n * d->h * d->w, d->c,
                                                  d->r * d->s * d->k)
                                  : timing_record(MODE_BWD_D, A3D_PREC_F32, 64, 64, 2, 4, 32, avec, bvec, 0, d->n * d->h * d->w, d->c,
                                                  d->r * d->s * d->k);
  rec.flops = multi_flops;
  return timed_launch(rec, st, [&] {
    return multi16 ? launch_igemm_bf16_multi_bwd_d(multi16_bn, multi, multi_grid, (unsigned)ncls, st)
                   : launch_igemm_multi_bwd_d(avec, bvec, multi, multi_grid, (unsigned)ncls, st);
  });
}

size_t a3dw_conv2d_bwd_data_prepared_filter_bytes(const a3d_conv_desc* d) {
  return check_desc(d) == A3D_OK && wino_applicable(d) ? wino_geom(d, true).u_bytes : 0;
}

int a3dw_conv2d_bwd_data_prepare_filter(const a3d_conv_desc* d, const float* w, void* prepared, size_t prepared_bytes, void* stream) {
  int rc = check_desc(d);
  if (rc != A3D_OK) return rc;
  A3D_CHECK_ARG(w && prepared && aligned16(prepared), "conv2d_bwd_data_prepare_filter: null or misaligned buffer");
  const size_t need = a3dw_conv2d_bwd_data_prepared_filter_bytes(d);
  A3D_CHECK_ARG(need > 0, "conv2d_bwd_data_prepare_filter: this bwd-data reads the filter as stored");
  if (prepared_bytes < need) return set_error(A3D_EWORKSPACE, "conv2d_bwd_data_prepare_filter: need %zu bytes", need);
  return wino_filter(d, true, w, static_cast<float*>(prepared), static_cast<hipStream_t>(stream));
}

// bf16 x and bf16 dz, whole 16-byte pieces inside one filter tap, 31-bit byte offsets into x AND into dz (the kernel addresses
// both from the tensor's first byte: a piece at 2^31 or beyond would read as zeros): the LDS-DMA kernel may take the filter
// gradient (BiasAddGrad then comes from colsum_bf16)
static bool bwd_f_ring_ok(const a3d_conv_desc* d, const Operands& o) {
  return d->precision == A3D_PREC_BF16 && stored16(d, A3D_STORE_X_BF16 | A3D_STORE_Y_BF16) && d->c % 8 == 0 && d->ldx % 8 == 0 &&
         d->k % 8 == 0 && d->ldy % 8 == 0 && (double)d->n * d->h * d->w * d->ldx * 2.0 < 2147483647.0 &&
         (double)d->n * d->ho * d->wo * d->ldy * 2.0 < 2147483647.0 && colsum_bf16_ok(d->k) && d->ldy == d->k && !o.w;
}
// The filter gradient as a GEMM: over the tensors as stored, the same offered to the LDS-DMA kernel, or in the window-run form
// (the gradient of the PADDED filter into the workspace, unpadded afterwards)
static Route bwd_f_gemm(const a3d_conv_desc* d, const Operands& o, GemmForm form) {
  Route r;
  r.ok = form == kRunForm ? run_form_ok(d, o.x, &r.rf, true) : form == kLdsDma ? bwd_f_ring_ok(d, o) : true;
  if (!r.ok) return r;
  GemmProblem& g = r.g;
  g = bwd_f_problem(d);
  if (o.x) g.avec = 1;
  if (o.y) g.bvec = 1;
  if (form == kRunForm) {
    g.M = r.rf.kp; g.avec = r.rf.vec;
    r.repack = r.rf.bytes;
  }
  if (o.known) storage_vecs(g, d->storage & A3D_STORE_X_BF16, d->storage & A3D_STORE_Y_BF16, false);
  g.ring_ok = form == kLdsDma;
  r.plan = plan_gemm(g, d->precision);
  // BiasAddGrad: column sums of dz fused into the GEMM, one slab row per split; beside the LDS-DMA kernel, colsum_bf16's partials
  if (r.plan.ring) r.bytes = r.plan.ws_bytes + (o.db ? colsum_bf16_ws_bytes(d->k) : 0);
  else r.bytes = r.repack + r.plan.ws_bytes + (r.plan.splitk > 1 && o.db ? (size_t)r.plan.splitk * g.N * 4 : 0);
  return r;
}

int a3d_conv2d_bwd_both_supported(const a3d_conv_desc* d) {
  A3D_AS_F32(d);
  return check_desc(d) == A3D_OK && !d->storage && stencil1_bwd_both_applicable(d);
}

size_t a3d_conv2d_bwd_both_ws_bytes(const a3d_conv_desc* d) {
  return a3d_conv2d_bwd_both_supported(d) ? stencil1_bwd_both_ws_bytes(d) : 0;
}

int a3d_conv2d_bwd_both(const a3d_conv_desc* d, const float* x, const float* dz, const float* w, float* dw, float* db,
                        void* dx, int lddx, int dx_bf16, int relu_mask, uint32_t* state, void* ws, size_t ws_bytes,
                        void* stream) {
  A3D_AS_F32(d);
  int rc = check_desc(d);
  if (rc != A3D_OK) return rc;
  A3D_CHECK_ARG(x && dz && w && dw && dx && state, "conv2d_bwd_both: null tensor");
  A3D_CHECK_ARG(a3d_conv2d_bwd_both_supported(d),
                "conv2d_bwd_both: one output channel, 5x5, stride 1, an even channel count <= 64, float32 tensors, x below 1 GiB");
  A3D_CHECK_ARG(lddx >= d->c && lddx % 2 == 0, "conv2d_bwd_both: lddx must be even and >= c");
  A3D_CHECK_ARG((reinterpret_cast<uintptr_t>(x) & 7) == 0 && (reinterpret_cast<uintptr_t>(w) & 7) == 0 &&
                    (reinterpret_cast<uintptr_t>(dx) & (dx_bf16 ? 3 : 7)) == 0 && (reinterpret_cast<uintptr_t>(ws) & 3) == 0,
                "conv2d_bwd_both: x, w and dx must be aligned to a channel pair");
  if (stencil1_bwd_both_ws_bytes(d) > ws_bytes) return set_error(A3D_EWORKSPACE, "conv2d_bwd_both: workspace too small");
  return stencil1_bwd_both(d, x, dz, w, dw, db, dx, lddx, dx_bf16, relu_mask, state, ws, static_cast<hipStream_t>(stream));
}

// the few-channel layers' filter gradient from LDS-staged input rows (fewch.hip); A3D_FEWCH=0 (tuning processes) keeps the
// window-run form of the generic kernel for A/B runs
static bool fewch_wanted(const a3d_conv_desc* d, bool pooled) {
  return !d->storage && fewch_bwdf_applicable(d, pooled) && tune_int("A3D_FEWCH", 1) != 0;
}

static int fewch_timed(const a3d_conv_desc* d, const float* x, int src, const void* dz, int ldz, const void* pooled_act,
                       const uint8_t* argmax, int ld_arg, float* dw, float* db, void* ws, hipStream_t st) {
  return timed_launch(fewch_record(d), st, [&] { return fewch_bwd_filter(d, x, src, dz, ldz, pooled_act, argmax, ld_arg, dw, db, ws, st); });
}

// config 5: bf16 arithmetic on the fp32 image and bf16 pooled tensors (fewch16.hip); A3D_FEWCH16=0 (tuning processes): refused
static bool fewch16_wanted(const a3d_conv_desc* d, bool pooled) {
  return !d->storage && fewch16_bwdf_applicable(d, pooled) && tune_int("A3D_FEWCH16", 1) != 0;
}

// the pooled filter gradient in fp32 arithmetic (float32 or bf16 pooled tensors)
static bool fewch_pooled_ok(const a3d_conv_desc* d) { return !d->storage && fewch_bwdf_applicable(d, true); }

size_t a3d_conv2d_bwd_filter_pooled_ws_bytes(const a3d_conv_desc* d) {
  A3D_AS_F32(d);
  if (check_desc(d) != A3D_OK) return 0;
  if (fewch16_wanted(d, true)) return fewch16_bwdf_ws_bytes(d, true);
  return fewch_pooled_ok(d) ? fewch_bwdf_ws_bytes(d, true) : 0;
}

int a3d_conv2d_bwd_filter_pooled(const a3d_conv_desc* d, const float* x, const void* dpool, int ld_dpool, const void* pooled,
                                 const uint8_t* argmax, int ld_argmax, int pooled_bf16, float* dw, float* db, void* ws,
                                 size_t ws_bytes, void* stream) {
  A3D_AS_F32(d);
  int rc = check_desc(d);
  if (rc != A3D_OK) return rc;
  A3D_CHECK_ARG(x && dpool && argmax && dw, "conv2d_bwd_filter_pooled: null tensor");
  A3D_CHECK_WS(ws, "conv2d_bwd_filter_pooled");
  if (fewch16_wanted(d, true)) {                    // bf16 arithmetic: float32 image, bf16 pooled tensors
    A3D_CHECK_ARG(pooled_bf16 && ld_dpool >= d->k && ld_argmax >= d->k && ld_dpool % 4 == 0 &&
                      (reinterpret_cast<uintptr_t>(dpool) & 7) == 0 && (reinterpret_cast<uintptr_t>(pooled) & 7) == 0 &&
                      (reinterpret_cast<uintptr_t>(x) & 15) == 0,
                  "conv2d_bwd_filter_pooled: bf16 arithmetic takes bf16 pooled tensors in whole aligned 4-channel groups");
    A3D_CHECK_ARG(fewch_extents_ok(d, true, ld_dpool, 2, ld_argmax), "conv2d_bwd_filter_pooled: pooled tensors of 2 GiB or more");
    if (fewch16_bwdf_ws_bytes(d, true) > ws_bytes) return set_error(A3D_EWORKSPACE, "conv2d_bwd_filter_pooled: workspace too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
    return timed_launch(fewch16_record(d), st,
                        [&] { return fewch16_bwd_filter(d, x, true, dpool, ld_dpool, pooled, argmax, ld_argmax, dw, db, ws, st); });
  }
  A3D_CHECK_ARG(fewch_pooled_ok(d),
                "conv2d_bwd_filter_pooled: an unpadded conv of <= 4 densely packed float32 input channels and 33..96 filters (fp32 "
                "arithmetic; or bf16 arithmetic with bf16 pooled tensors)");
  A3D_CHECK_ARG(ld_dpool >= d->k && ld_argmax >= d->k, "conv2d_bwd_filter_pooled: pixel strides below the filter count");
  A3D_CHECK_ARG(ld_dpool % 4 == 0 && aligned16(x) && (reinterpret_cast<uintptr_t>(dpool) & (pooled_bf16 ? 7 : 15)) == 0 &&
                    (reinterpret_cast<uintptr_t>(pooled) & (pooled_bf16 ? 7 : 15)) == 0,
                "conv2d_bwd_filter_pooled: x, dpool and pooled in whole aligned 4-channel groups (ld_dpool % 4 == 0)");
  A3D_CHECK_ARG(fewch_extents_ok(d, true, ld_dpool, pooled_bf16 ? 2 : 4, ld_argmax), "conv2d_bwd_filter_pooled: pooled tensors of 2 GiB or more");
  if (fewch_bwdf_ws_bytes(d, true) > ws_bytes) return set_error(A3D_EWORKSPACE, "conv2d_bwd_filter_pooled: workspace too small");
  return fewch_timed(d, x, pooled_bf16 ? 2 : 1, dpool, ld_dpool, pooled, argmax, ld_argmax, dw, db, ws,
                     static_cast<hipStream_t>(stream));
}

size_t a3d_conv2d_bwd_filter_ws_bytes(const a3d_conv_desc* d) {
  A3D_AS_F32(d);
  if (check_desc(d) != A3D_OK) return 0;
  if (stencil1_applicable(d)) return stencil1_bwdf_ws_bytes(d);
  size_t need = fewch_wanted(d, false) ? fewch_bwdf_ws_bytes(d, false) : 0;      // (an unaligned x falls back to the plans below)
  // kAsStored: the plan without the LDS-DMA kernel, a launch may fall back to it (a dw off the 16-byte grid: ADVICE r4)
  for (GemmForm form : {kAsStored, kLdsDma, kRunForm}) need = upto(need, bwd_f_gemm(d, kOnGrid, form));
  return need;
}

int a3d_conv2d_bwd_filter(const a3d_conv_desc* d, const float* x, const float* dz, float* dw, float* db, void* ws,
                          size_t ws_bytes, void* stream) {
  A3D_AS_F32(d);
  int rc = check_desc(d);
  if (rc != A3D_OK) return rc;
  A3D_CHECK_ARG(x && dz && dw, "conv2d_bwd_filter: null tensor");
  A3D_CHECK_WS(ws, "conv2d_bwd_filter");
  if (!ws) ws_bytes = 0;
  if (stencil1_applicable(d)) {
    A3D_CHECK_ARG(!d->storage, "conv2d_bwd_filter: single-output-channel convs take float32 tensors");
    if (stencil1_bwdf_ws_bytes(d) > ws_bytes) return set_error(A3D_EWORKSPACE, "conv2d_bwd_filter: workspace too small");
    return stencil1_bwd_filter(d, x, dz, dw, db, ws, static_cast<hipStream_t>(stream));
  }
  if (fewch_wanted(d, false) && aligned16(x) && fewch_extents_ok(d, false, d->ldy, 4, 0)) {
    if (fewch_bwdf_ws_bytes(d, false) > ws_bytes) return set_error(A3D_EWORKSPACE, "conv2d_bwd_filter: workspace too small");
    return fewch_timed(d, x, 0, dz, d->ldy, nullptr, nullptr, 0, dw, db, ws, static_cast<hipStream_t>(stream));
  }
  Operands o = launch_operands(x, dw, dz, nullptr);
  o.db = db != nullptr;
  // the window-run form if the workspace holds the padded gradient; else the tensors as stored, on the LDS-DMA kernel where that may be
  RunForm rf;
  const bool run = run_form_ok(d, o.x, &rf, true) && rf.bytes <= ws_bytes;
  Route r = bwd_f_gemm(d, o, run ? kRunForm : bwd_f_ring_ok(d, o) ? kLdsDma : kAsStored);
  fit_workspace(r, o, ws_bytes, o.db ? (size_t)r.g.N * 4 : 0);
  const GemmPlan& plan = r.plan;
  float* out = run ? static_cast<float*>(ws) : dw;
  IgemmParams p;
  fill_common(p, r.g);
  rc = apply_storage(p, d->precision, d->storage & A3D_STORE_X_BF16, d->storage & A3D_STORE_Y_BF16, false, d->c, d->ldx, -1, d->ldy,
                     x, dz, dw, "x", "dz", "dw");
  if (rc != A3D_OK) return rc;
  A3D_CHECK_ARG(!d->storage || plan.prec == A3D_PREC_BF16, "conv2d_bwd_filter: bf16 storage needs vectorisable operands");
  if (r.bytes > ws_bytes) return set_error(A3D_EWORKSPACE, "conv2d_bwd_filter: need %zu workspace bytes", r.bytes);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (plan.ring && db) {                           // the LDS-DMA kernel never holds dz in registers: BiasAddGrad on the side
    // a split launch ends in a reduction kernel anyway: that one adds the partial sums (one launch fewer per layer)
    float* parts = reinterpret_cast<float*>(static_cast<char*>(ws) + plan.ws_bytes);
    int nparts = 0;
    rc = colsum_bf16(dz, r.g.K, d->k, d->ldy, plan.splitk > 1 ? nullptr : db, parts, &nparts, st);
    if (rc != A3D_OK) return rc;
    if (plan.splitk > 1) { p.dbias_parts = parts; p.dbias_parts_out = db; p.dbias_parts_n = nparts; }
    db = nullptr;
  }
  p.A = x; p.B = dz; p.C = out; p.dbias = db;     // BiasAddGrad = column sums of dz, fused into the same kernel
  p.npix = r.g.K; p.nrsc = r.g.M;
  fill_gather(p, d, d->ldx, run ? 1 : d->s, run ? rf.rlp : d->c);
  p.ldb = d->ldy; p.ldc = d->k;
  fill_staging(p, MODE_BWD_F, (unsigned long long)d->n * d->h * d->w * d->ldx, (unsigned long long)d->n * d->ho * d->wo * d->ldy, d->r,
               run ? 1 : d->s);
  if (run) { p.unpad_dst = dw; p.unpad_rl = rf.rl; p.unpad_rlp = rf.rlp; }
  rc = launch_igemm(MODE_BWD_F, plan, r.g.avec, r.g.bvec, p, static_cast<char*>(ws) + r.repack, st);
  if (rc != A3D_OK || !run || p.unpad_done) return rc;       // the split-K reduction stored the unpadded filter itself
  clear_stale_error();
  hipLaunchKernelGGL(unpad_filter_kernel, dim3((d->r * rf.rl * d->k + 255) / 256), dim3(256), 0, st, out, dw, d->r,
                     rf.rl, rf.rlp, d->k);
  return check_launch("unpad_filter");
}

// ---- include/a3d_wino_grad.h: the filter gradient through Winograd F(2x2,3x3); workspace [V][Z][slabs][bias partials] ----
static bool wino_grad_takes(const a3d_conv_desc* d) { return check_desc(d) == A3D_OK && wino_grad_applicable(d); }

// one of the sixteen sums over tiles: the filter gradient of a 1x1 conv over T one-pixel images of Cp channels, Kp filters
static IgemmParams wino_grad_product(const WinoGradGeom& g, const float* V, const float* Z, float* slabs, float* bparts) {
  return plane_product(MODE_BWD_F, plane_desc((int)g.T, 1, 1, 1, g.Cp, g.Kp, 1, 0), V, Z, slabs, bparts, (unsigned long long)g.T * g.Cp,
                       (unsigned long long)g.T * g.Kp, 1);
}

size_t a3dwg_conv2d_bwd_filter_ws_bytes(const a3d_conv_desc* d) {
  if (!wino_grad_takes(d)) return a3d_conv2d_bwd_filter_ws_bytes(d);
  return grad_ws_bytes(wino_grad_geom(d));
}

int a3dwg_conv2d_bwd_filter(const a3d_conv_desc* d, const float* x, const float* dz, float* dw, float* db, void* ws,
                            size_t ws_bytes, void* stream) {
  if (!wino_grad_takes(d)) return a3d_conv2d_bwd_filter(d, x, dz, dw, db, ws, ws_bytes, stream);
  A3D_CHECK_ARG(x && dz && dw, "conv2d_bwd_filter (Winograd): null tensor");
  A3D_CHECK_WS(ws, "conv2d_bwd_filter (Winograd)");
  const WinoGradGeom g = wino_grad_geom(d);
  Carve c{reinterpret_cast<uintptr_t>(ws)};
  const GradWs at = carve_grad(c, g);
  const size_t need = c.at - reinterpret_cast<uintptr_t>(ws);
  if (!ws || need > ws_bytes) return set_error(A3D_EWORKSPACE, "conv2d_bwd_filter (Winograd): need %zu workspace bytes", need);
  hipStream_t st = static_cast<hipStream_t>(stream);
  int rc = wino_input(d, false, x, at.V, st);
  if (rc != A3D_OK) return rc;
  rc = wino_dz(d, dz, at.Z, st);
  if (rc != A3D_OK) return rc;
  IgemmParams p = wino_grad_product(g, at.V, at.Z, at.slabs, db ? at.bparts : nullptr);
  rc = timed_launch(wino_grad_record(d, g), st, [&] { return wino_grad_gemm(p, g, st); });
  if (rc != A3D_OK) return rc;
  return wino_dw(d, g, at.slabs, at.bparts, dw, db, st);
}

// ---- include/a3d_wino_bwd.h: both gradients as one chain; workspace [U unless prepared][V_dz][M][V_x][Z][slabs][bias partials] ----
// Both routes take the descriptor, and the filter gradient's tile grid (over ho x wo) lies inside bwd-data's (over h x w), whose
// items write Z
static bool wino_bwd_takes(const a3d_conv_desc* d) {
  if (!wino_grad_takes(d)) return false;
  const WinoGeom gx = wino_geom(d, false), gd = wino_geom(d, true);
  return gx.th <= gd.th && gx.tw <= gd.tw;
}
static a3d_conv_desc as_winograd(const a3d_conv_desc* d) {
  a3d_conv_desc e = *d;
  e.precision = A3D_PREC_F32_WINOGRAD;
  return e;
}

size_t a3dwb_sizeof_pool(void) { return sizeof(a3dwb_pool); }

size_t a3dwb_conv2d_bwd_ws_bytes(const a3d_conv_desc* d, int w_prepared, int pooled) {
  (void)pooled;      // the pooled-size dx has no buffer
  if (!wino_bwd_takes(d)) return std::max(a3dwg_conv2d_bwd_filter_ws_bytes(d), a3d_conv2d_bwd_data_ws_bytes(d));
  const a3d_conv_desc e = as_winograd(d);
  Carve c{0};
  carve_product(c, wino_geom(&e, true), w_prepared != 0);
  carve_grad(c, wino_grad_geom(&e));
  return c.at;
}

int a3dwb_conv2d_bwd(const a3d_conv_desc* d, const float* x, const float* dz, const float* w_or_U, float* dw, float* db, float* dx,
                     const float* relu_mask, const a3dwb_pool* pool, void* ws, size_t ws_bytes, void* stream) {
  static_assert(sizeof(WinoBwdPool) == sizeof(a3dwb_pool), "WinoBwdPool mirrors a3dwb_pool");
  if (!wino_bwd_takes(d)) {
    A3D_CHECK_ARG(!pool, "conv2d_bwd (Winograd): a pool only where the Winograd routes take the descriptor");
    const int rc = a3dwg_conv2d_bwd_filter(d, x, dz, dw, db, ws, ws_bytes, stream);
    return rc != A3D_OK ? rc : a3d_conv2d_bwd_data(d, dz, w_or_U, dx, relu_mask, ws, ws_bytes, stream);
  }
  A3D_CHECK_ARG(x && dz && w_or_U && dw && dx, "conv2d_bwd (Winograd): null tensor");
  A3D_CHECK_WS(ws, "conv2d_bwd (Winograd)");
  A3D_CHECK_ARG(!(pool && relu_mask), "conv2d_bwd (Winograd): relu_mask and pool exclude each other");
  A3D_CHECK_ARG(!pool || (pool->argmax && pool->y && pool->ldy >= d->c && pool->h2 >= 2 && pool->w2 >= 2 && pool->h2 / 2 == d->h &&
                          pool->w2 / 2 == d->w),
                "conv2d_bwd (Winograd): the pool's halved extents must be the layer's input's");
  const a3d_conv_desc e = as_winograd(d);
  const bool prepared = (d->hints & A3D_HINT_W_PREPARED) != 0;
  const WinoGeom g = wino_geom(&e, true);
  const WinoGradGeom gg = wino_grad_geom(&e);
  Carve c{reinterpret_cast<uintptr_t>(ws)};
  const ProductWs ad = carve_product(c, g, prepared);      // bwd-data's
  const GradWs af = carve_grad(c, gg);                     // the filter gradient's
  const size_t need = c.at - reinterpret_cast<uintptr_t>(ws);
  if (!ws || need > ws_bytes) return set_error(A3D_EWORKSPACE, "conv2d_bwd (Winograd): need %zu workspace bytes", need);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const float* U;
  int rc = transformed_filter("conv2d_bwd (Winograd)", prepared, w_or_U, ad.U, U, [&](float* u) { return wino_filter(&e, true, w_or_U, u, st); });
  if (rc != A3D_OK) return rc;
  rc = wino_bwd_transforms(&e, x, dz, af.V, ad.V, af.Z, st);
  if (rc != A3D_OK) return rc;
  IgemmParams pf = wino_grad_product(gg, af.V, af.Z, af.slabs, db ? af.bparts : nullptr);
  IgemmParams pd = wino_product(g, ad.V, U, ad.M);
  // a bracket measures one kernel: when either product's record is wanted the two run as the launches those records describe
  const a3d_timing_record rf = wino_grad_record(&e, gg), rd = wino_record(MODE_BWD_D, g);
  if (timing_wanted(rf) || timing_wanted(rd) || tune_int("A3D_WINO_BWD_PAIR", 1) == 0) {      // (A3D_TUNING=1: the A/B of the pairing)
    rc = timed_launch(rf, st, [&] { return wino_grad_gemm(pf, gg, st); });
    if (rc != A3D_OK) return rc;
    rc = timed_launch(rd, st, [&] { return wino_gemm(pd, g, st); });
  } else {
    rc = wino_bwd_gemm(pf, gg, pd, g, st);
  }
  if (rc != A3D_OK) return rc;
  WinoBwdPool wp{};
  if (pool) wp = WinoBwdPool{pool->argmax, pool->y, pool->ldy, pool->h2, pool->w2};
  return wino_bwd_finish(&e, gg, af.slabs, af.bparts, dw, db, ad.M, dx, relu_mask, pool ? &wp : nullptr, st);
}

// ---- include/a3d_wino1d.h: the gradients of a stride-1 convolution 5 wide through 1-D Winograd F(4,5) (wino1d.hip) ----
static bool wino1d_takes(const a3d_conv_desc* d) { return check_desc(d) == A3D_OK && wino1d_applicable(d); }

// one of bwd-data's eight products: the forward of an r x 1 convolution over a plane of V [n][ho][tw][Kp] with vertical padding
// r - 1 - pad_t, onto dx's rows x tiles, against U[xi] [r Kp][Np]
static IgemmParams wino1d_product(const a3d_conv_desc* d, const Wino1dGeom& g, const float* V, const float* U, float* M) {
  return plane_product(MODE_FWD, plane_desc(d->n, d->ho, g.tw, d->h, g.Kp, g.Np, g.R, g.R - 1 - d->pad_t), V, U, M, nullptr,
                       (unsigned long long)g.Pv * g.Kp, (unsigned long long)g.R * g.Kp * g.Np, g.R);
}
// one of the filter gradient's eight sums: the filter gradient of an r x 1 convolution from a plane of V [n][h][tw][Cp] and a
// plane of Z [n][ho][tw][Kp]
static IgemmParams wino1d_grad_product(const a3d_conv_desc* d, const Wino1dGradGeom& g, const float* V, const float* Z, float* slabs,
                                       float* bparts) {
  return plane_product(MODE_BWD_F, plane_desc(d->n, d->h, g.tw, d->ho, g.Cp, g.Kp, g.R, d->pad_t), V, Z, slabs, bparts,
                       (unsigned long long)g.Px * g.Cp, (unsigned long long)g.Pz * g.Kp, g.R);
}

size_t a3dl_conv2d_bwd_data_ws_bytes(const a3d_conv_desc* d) {
  if (!wino1d_takes(d)) return a3d_conv2d_bwd_data_ws_bytes(d);
  return product_ws_bytes(wino1d_geom(d), (d->hints & A3D_HINT_W_PREPARED) != 0);
}

int a3dl_conv2d_bwd_data(const a3d_conv_desc* d, const float* dz, const float* w, float* dx, const float* relu_mask, void* ws,
                         size_t ws_bytes, void* stream) {
  if (!wino1d_takes(d)) return a3d_conv2d_bwd_data(d, dz, w, dx, relu_mask, ws, ws_bytes, stream);
  A3D_CHECK_ARG(dz && w && dx, "conv2d_bwd_data (Winograd 1-D): null tensor");
  A3D_CHECK_WS(ws, "conv2d_bwd_data (Winograd 1-D)");
  const bool prepared = (d->hints & A3D_HINT_W_PREPARED) != 0;
  const Wino1dGeom g = wino1d_geom(d);
  Carve c{reinterpret_cast<uintptr_t>(ws)};
  const ProductWs at = carve_product(c, g, prepared);
  const size_t need = c.at - reinterpret_cast<uintptr_t>(ws);
  if (!ws || need > ws_bytes) return set_error(A3D_EWORKSPACE, "conv2d_bwd_data (Winograd 1-D): need %zu workspace bytes", need);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const float* U;
  int rc = transformed_filter("conv2d_bwd_data (Winograd 1-D)", prepared, w, at.U, U, [&](float* u) { return wino1d_filter(d, w, u, st); });
  if (rc != A3D_OK) return rc;
  rc = wino1d_input(dz, at.V, (size_t)d->n * d->ho, d->wo, d->k, d->ldy, g.off, g.tw, g.Kp, st);
  if (rc != A3D_OK) return rc;
  IgemmParams p = wino1d_product(d, g, at.V, U, at.M);
  rc = timed_launch(wino1d_record(g), st, [&] { return wino1d_gemm(p, g, at.sk, st); });
  if (rc != A3D_OK) return rc;
  return wino1d_output(d, g, at.M, dx, relu_mask, st);
}

size_t a3dl_conv2d_bwd_filter_ws_bytes(const a3d_conv_desc* d) {
  if (!wino1d_takes(d)) return a3d_conv2d_bwd_filter_ws_bytes(d);
  return grad_ws_bytes(wino1d_grad_geom(d));
}

int a3dl_conv2d_bwd_filter(const a3d_conv_desc* d, const float* x, const float* dz, float* dw, float* db, void* ws, size_t ws_bytes,
                           void* stream) {
  if (!wino1d_takes(d)) return a3d_conv2d_bwd_filter(d, x, dz, dw, db, ws, ws_bytes, stream);
  A3D_CHECK_ARG(x && dz && dw, "conv2d_bwd_filter (Winograd 1-D): null tensor");
  A3D_CHECK_WS(ws, "conv2d_bwd_filter (Winograd 1-D)");
  const Wino1dGradGeom g = wino1d_grad_geom(d);
  Carve c{reinterpret_cast<uintptr_t>(ws)};
  const GradWs at = carve_grad(c, g);
  const size_t need = c.at - reinterpret_cast<uintptr_t>(ws);
  if (!ws || need > ws_bytes) return set_error(A3D_EWORKSPACE, "conv2d_bwd_filter (Winograd 1-D): need %zu workspace bytes", need);
  hipStream_t st = static_cast<hipStream_t>(stream);
  int rc = wino1d_input(x, at.V, (size_t)d->n * d->h, d->w, d->c, d->ldx, d->pad_l, g.tw, g.Cp, st);
  if (rc != A3D_OK) return rc;
  rc = wino1d_dz(d, g, dz, at.Z, st);
  if (rc != A3D_OK) return rc;
  IgemmParams p = wino1d_grad_product(d, g, at.V, at.Z, at.slabs, db ? at.bparts : nullptr);
  rc = timed_launch(wino1d_grad_record(d, g), st, [&] { return wino1d_grad_gemm(p, g, st); });
  if (rc != A3D_OK) return rc;
  return wino1d_dw(d, g, at.slabs, at.bparts, dw, db, st);
}

size_t a3dl_conv2d_bwd_data_prepared_filter_bytes(const a3d_conv_desc* d) { return wino1d_takes(d) ? wino1d_geom(d).u_bytes : 0; }

int a3dl_conv2d_bwd_data_prepare_filter(const a3d_conv_desc* d, const float* w, void* prepared, size_t prepared_bytes, void* stream) {
  int rc = check_desc(d);
  if (rc != A3D_OK) return rc;
  A3D_CHECK_ARG(w && prepared && aligned16(prepared), "conv2d_bwd_data_prepare_filter (Winograd 1-D): null or misaligned buffer");
  const size_t need = a3dl_conv2d_bwd_data_prepared_filter_bytes(d);
  A3D_CHECK_ARG(need > 0, "conv2d_bwd_data_prepare_filter (Winograd 1-D): the route does not take this descriptor");
  if (prepared_bytes < need) return set_error(A3D_EWORKSPACE, "conv2d_bwd_data_prepare_filter (Winograd 1-D): need %zu bytes", need);
  return wino1d_filter(d, w, static_cast<float*>(prepared), static_cast<hipStream_t>(stream));
}

// ---- dense = 1x1 conv over a 1x1 image ----
static a3d_conv_desc dense_desc(int m, int k, int n) {
  a3d_conv_desc d{};
  d.n = m; d.h = 1; d.w = 1; d.c = k; d.k = n; d.r = 1; d.s = 1; d.stride = 1; d.ho = 1; d.wo = 1;
  d.ldx = k; d.ldy = n;
  return d;
}

size_t a3d_dense_fwd_ws_bytes(int m, int k, int n) {
  a3d_conv_desc d = dense_desc(m, k, n);
  if (check_desc(&d) != A3D_OK) return 0;
  // the GEMM a3d_dense_fwd plans (never the few-channel convolution paths: a dense layer of <= 4 inputs is still a GEMM)
  return std::max(plan_gemm(fwd_problem(&d), A3D_PREC_F32).ws_bytes, dense_stream_ws_bytes(m, k, n));
}

int a3d_dense_fwd(int m, int k, int n, const float* x, const float* w, const float* bias, float* y, int act,
                  const uint8_t* drop_keep, void* ws, size_t ws_bytes, void* stream) {
  return a3d_dense_fwd_ex(m, k, n, x, w, bias, y, act, drop_keep, A3D_PREC_F32, 0, ws, ws_bytes, stream);
}

int a3d_dense_fwd_ex(int m, int k, int n, const float* x, const float* w, const float* bias, float* y, int act,
                     const uint8_t* drop_keep, int precision, int storage, void* ws, size_t ws_bytes, void* stream) {
  return a3d_dense_fwd_ex2(m, k, n, x, w, bias, y, n, n, act, drop_keep, precision, storage, nullptr, ws, ws_bytes, stream);
}

int a3d_dense_fwd_ex2(int m, int k, int n, const float* x, const float* w, const float* bias, float* y, int ldy, int ncols_y, int act,
                      const uint8_t* drop_keep, int precision, int storage, const a3d_second_output* out2, void* ws,
                      size_t ws_bytes, void* stream) {
  A3D_CHECK_ARG(m > 0 && k > 0 && n > 0, "dense_fwd: bad dims");
  A3D_CHECK_ARG(ncols_y > 0 && ncols_y <= n && ldy >= ncols_y, "dense_fwd: y rows of %d columns at pitch %d from a GEMM of %d", ncols_y, ldy, n);
  A3D_CHECK_ARG((storage & ~(A3D_STORE_W_BF16 | A3D_STORE_X_BF16)) == 0, "dense_fwd: the weights and x may be bf16, y is float32");
  if (precision == A3D_PREC_F32_WINOGRAD) precision = A3D_PREC_F32;      // no 3x3 window in a dense layer: runs as A3D_PREC_F32
  a3d_conv_desc d = dense_desc(m, k, n);
  d.precision = precision;
  int rc = check_desc(&d);
  if (rc != A3D_OK) return rc;
  A3D_CHECK_ARG(x && w && y, "dense_fwd: null tensor");
  A3D_CHECK_WS(ws, "dense_fwd");
  if (precision == A3D_PREC_F32 && !storage && dense_stream_applicable(m, k, n) && aligned16(x) && !out2 && ldy == n && ncols_y == n &&
      !tune_int("A3D_NO_DENSE_KERNELS", 0))
    return dense_fwd_stream(m, k, n, x, w, bias, y, act, drop_keep, 2.f, ws, ws_bytes, static_cast<hipStream_t>(stream));
  GemmProblem g = fwd_problem(&d);
  if (!aligned16(x)) g.avec = 1;
  if (!aligned16(w)) g.bvec = 1;
  IgemmParams p;
  fill_common(p, g);
  rc = apply_storage(p, precision, storage & A3D_STORE_X_BF16, storage & A3D_STORE_W_BF16, false, k, k, n, n, x, w, y, "x", "w", "y");
  if (rc != A3D_OK) return rc;
  A3D_CHECK_ARG(!p.a16 || aligned16(y), "dense_fwd: beside a bf16 x, y must be 16-byte aligned (the LDS-DMA kernel alone reads a bf16 x)");
  storage_vecs(g, p.a16, p.b16, p.c16);
  g.ring_ok = p.a16 && p.b16 && precision == A3D_PREC_BF16 && k % 8 == 0 && n % 8 == 0 && aligned16(y) && act != A3D_ACT_SIGMOID;
  g.need_reduce = ncols_y != n;                  // rows narrower than the GEMM are stored by the split-K reduction: plan one
  GemmPlan plan = plan_gemm(g, precision);
  if (!aligned16(x) || !aligned16(w) || !aligned16(y)) plan = plan_within(g, plan, ws ? ws_bytes : 0, 0);      // (fit_workspace)
  A3D_CHECK_ARG(!storage || plan.prec == A3D_PREC_BF16, "dense_fwd: bf16 weights need vectorisable operands");
  A3D_CHECK_ARG(!p.a16 || plan.ring, "dense_fwd: a bf16 x is taken by the LDS-DMA kernel only (bf16 weights, k and n multiples of 8)");
  if (plan.ws_bytes > ws_bytes) return set_error(A3D_EWORKSPACE, "dense_fwd: need %zu workspace bytes", plan.ws_bytes);
  p.A = x; p.B = w; p.C = y; p.bias = bias; p.act = act; p.keep = drop_keep; p.mask_scale = 2.f;
  p.npix = m; p.nrsc = k;
  fill_gather(p, &d, k, 1, k);                   // one tap over the k inputs of a row
  p.ldb = n; p.ldc = ldy; p.c_cols = ncols_y == n ? 0 : ncols_y;
  rc = take_second_output(p, out2);
  if (rc != A3D_OK) return rc;
  fill_staging(p, MODE_FWD, (unsigned long long)m * k, (unsigned long long)k * n, 1, 1);
  return launch_igemm(MODE_FWD, plan, g.avec, g.bvec, p, ws, static_cast<hipStream_t>(stream));
}

size_t a3d_dense_bwd_data_ws_bytes(int m, int k, int n) {
  a3d_conv_desc d = dense_desc(m, k, n);
  return a3d_conv2d_bwd_data_ws_bytes(&d);
}

int a3d_dense_bwd_data(int m, int k, int n, const float* dz, const float* w, float* dx, const float* mask,
                       int mask_act, float scale, void* ws, size_t ws_bytes, void* stream) {
  return a3d_dense_bwd_data_ex(m, k, n, dz, w, dx, mask, mask_act, scale, A3D_PREC_F32, 0, ws, ws_bytes, stream);
}

int a3d_dense_bwd_data_ex(int m, int k, int n, const float* dz, const float* w, float* dx, const float* mask, int mask_act,
                          float scale, int precision, int storage, void* ws, size_t ws_bytes, void* stream) {
  return a3d_dense_bwd_data_ex2(m, k, n, dz, w, dx, mask, mask_act, scale, precision, storage, nullptr, ws, ws_bytes, stream);
}

int a3d_dense_bwd_data_ex2(int m, int k, int n, const float* dz, const float* w, float* dx, const float* mask, int mask_act,
                           float scale, int precision, int storage, const a3d_second_output* out2, void* ws, size_t ws_bytes,
                           void* stream) {
  A3D_CHECK_ARG(m > 0 && k > 0 && n > 0, "dense_bwd_data: bad dims");
  // storage bits as a3d_conv2d_bwd_data's: Y = dz, W = w, X = dx and the mask
  if (precision == A3D_PREC_F32_WINOGRAD) precision = A3D_PREC_F32;      // as a3d_dense_fwd_ex2
  A3D_CHECK_ARG(precision >= A3D_PREC_F32 && precision <= A3D_PREC_BF16, "dense_bwd_data: unknown precision %d", precision);
  A3D_CHECK_ARG(!mask || mask_act == A3D_ACT_RELU || mask_act == A3D_ACT_SIGMOID, "dense_bwd_data: bad mask_act");
  a3d_conv_desc d = dense_desc(m, k, n);
  int rc = check_desc(&d);
  if (rc != A3D_OK) return rc;
  A3D_CHECK_ARG(dz && w && dx, "dense_bwd_data: null tensor");
  A3D_CHECK_WS(ws, "dense_bwd_data");
  GemmProblem g = bwd_d_problem(&d);
  if (!aligned16(dz)) g.avec = 1;
  if (!aligned16(w)) g.bvec = 1;
  IgemmParams p;
  fill_common(p, g);
  rc = apply_storage(p, precision, storage & A3D_STORE_Y_BF16, storage & A3D_STORE_W_BF16, storage & A3D_STORE_X_BF16, n, n, n, n, dz, w,
                     dx, "dz", "w", "dx");
  if (rc != A3D_OK) return rc;
  A3D_CHECK_ARG(!p.c16 || aligned16(mask), "dense_bwd_data: bf16 mask must be 16-byte aligned");
  storage_vecs(g, p.a16, p.b16, p.c16);
  g.ring_ok = p.a16 && p.b16 && precision == A3D_PREC_BF16 && k % 8 == 0 && n % 8 == 0 && aligned16(dx) &&
              (!mask || (aligned16(mask) && mask_act == A3D_ACT_RELU));
  GemmPlan plan = plan_gemm(g, precision);
  if (!aligned16(dz) || !aligned16(w) || !aligned16(dx) || !aligned16(mask)) plan = plan_within(g, plan, ws ? ws_bytes : 0, 0);      // (fit_workspace)
  A3D_CHECK_ARG(!storage || plan.prec == A3D_PREC_BF16, "dense_bwd_data: bf16 weights need vectorisable operands");
  A3D_CHECK_ARG(!(p.a16 || p.c16) || plan.ring, "dense_bwd_data: bf16 dz / dx are taken by the LDS-DMA kernel only (bf16 weights, k and n multiples of 8, ReLU mask)");
  if (plan.ws_bytes > ws_bytes) return set_error(A3D_EWORKSPACE, "dense_bwd_data: need %zu workspace bytes", plan.ws_bytes);
  p.A = dz; p.B = w; p.C = dx; p.mask = mask; p.mask_scale = scale; p.mask_act = mask_act;
  p.npix = m; p.nrsc = n;
  fill_gather(p, &d, n, 1, n);                   // one tap over the n gradients of a row
  p.Cn = k;
  p.ldc = k;
  p.S_full = 1;
  rc = take_second_output(p, out2);
  if (rc != A3D_OK) return rc;
  fill_staging(p, MODE_BWD_D, (unsigned long long)m * n, (unsigned long long)k * n, 1, 1);
  return launch_igemm(MODE_BWD_D, plan, g.avec, g.bvec, p, ws, static_cast<hipStream_t>(stream));
}

size_t a3d_dense_bwd_filter_ws_bytes(int m, int k, int n) {
  a3d_conv_desc d = dense_desc(m, k, n);
  return a3d_conv2d_bwd_filter_ws_bytes(&d);
}

int a3d_dense_bwd_filter(int m, int k, int n, const float* x, const float* dz, float* dw, float* db, void* ws,
                         size_t ws_bytes, void* stream) {
  A3D_CHECK_ARG(m > 0 && k > 0 && n > 0, "dense_bwd_filter: bad dims");
  A3D_CHECK_WS(ws, "dense_bwd_filter");
  if (dense_dw_applicable(m, k, n) && (long)k * n >= (1L << 16) && !tune_int("A3D_NO_DENSE_KERNELS", 0)) {      // small batch: stream dw once (dense.hip)
    A3D_CHECK_ARG(x && dz && dw, "dense_bwd_filter: null tensor");
    return dense_dw_launch(m, k, n, x, dz, dw, db, static_cast<hipStream_t>(stream));
  }
  a3d_conv_desc d = dense_desc(m, k, n);
  return a3d_conv2d_bwd_filter(&d, x, dz, dw, db, ws, ws_bytes, stream);
}

}  // extern "C"
