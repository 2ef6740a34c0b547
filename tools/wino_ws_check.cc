// wino_ws_check — the workspace layouts of the Winograd routes (csrc/a3d_internal.h: Carve, carve_product, carve_grad) on the host,
// under AddressSanitizer and UBSan, without a GPU and without Python:  make -C ann3depth_amd/csrc ws_check
// Over the descriptors of tests/wino_ref.py (which wino_grad_ref.py shares) and tests/wino1d_ref.py, with the filter prepared and
// not: every segment starts on a 256-byte boundary, the segments follow each other in the layout's order without a gap or an
// overlap (each is filled with its own byte in an allocation of exactly the queried size, then read back), and the end offset is
// the byte count that the Python restatements of the routes give (restated here in plain integers).
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../ann3depth_amd/csrc/a3d_internal.h"

namespace a3d {      // what wino.hip and wino1d.hip want from the rest of the library
int set_error(int code, const char*, ...) { return code; }
a3d_timing_record timing_record(int, int, int, int, int, int, int, int, int, int, int, int, int) { return a3d_timing_record{}; }
int tune_int(const char*, int dflt) { return dflt; }
}  // namespace a3d

using namespace a3d;

static int failures = 0;
#define EXPECT(cond, ...)                     \
  do {                                        \
    if (!(cond)) {                            \
      ++failures;                             \
      printf("FAIL %s: ", #cond);             \
      printf(__VA_ARGS__);                    \
      printf("\n");                           \
    }                                         \
  } while (0)

static long cdiv(long a, long b) { return (a + b - 1) / b; }
static long pad4(long c) { return cdiv(c, 4) * 4; }
static size_t up(size_t b) { return (b + 255) / 256 * 256; }

struct Case {
  int n, h, w, c, k, r, s;
  bool same;
};
static a3d_conv_desc desc_of(const Case& q, int precision) {
  a3d_conv_desc d{};
  d.n = q.n; d.h = q.h; d.w = q.w; d.c = q.c; d.k = q.k; d.r = q.r; d.s = q.s; d.stride = 1;
  d.pad_t = q.same ? (q.r - 1) / 2 : 0;
  d.pad_l = q.same ? (q.s - 1) / 2 : 0;
  d.ho = q.same ? q.h : q.h - q.r + 1;
  d.wo = q.same ? q.w : q.w - q.s + 1;
  d.ldx = q.c; d.ldy = q.k; d.precision = precision;
  return d;
}

// tests/wino_grad_ref.py: splits(); tests/wino1d_ref.py: grad_splits()
static long ref_splits(long planes, long m, long n, long pixels, bool larger_on_tie) {
  const long blocks1 = planes * cdiv(m, 128) * cdiv(n, 128), nk = cdiv(pixels, 32);
  const long smax = std::max(1L, std::min(512 / blocks1, nk / 5));
  long s = 1;
  for (long t = 2; t <= smax; ++t) {      // work on the busiest CU: ceil(blocks1 t / 256) / t
    const long lt = cdiv(blocks1 * t, 256) * s, ls = cdiv(blocks1 * s, 256) * t;
    if (lt < ls || (larger_on_tie && lt == ls)) s = t;
  }
  return cdiv(nk, cdiv(nk, s));
}

// carves `layout` from an allocation of exactly `bytes`, fills every segment with its index and reads them back
template <typename Layout>
static void walk(const char* what, size_t bytes, const std::vector<size_t>& sizes, Layout&& layout) {
  unsigned char* base = static_cast<unsigned char*>(aligned_alloc(256, std::max<size_t>(bytes, 256)));
  Carve c{reinterpret_cast<uintptr_t>(base)};
  const std::vector<float*> segs = layout(c);
  EXPECT(c.at - reinterpret_cast<uintptr_t>(base) == bytes, "%s: the launch's carve ends at %zu, the query's at %zu", what,
         (size_t)(c.at - reinterpret_cast<uintptr_t>(base)), bytes);
  EXPECT(segs.size() == sizes.size(), "%s: %zu segments", what, segs.size());
  size_t at = 0;
  for (size_t i = 0; i < segs.size(); ++i) {
    unsigned char* p = reinterpret_cast<unsigned char*>(segs[i]);
    EXPECT(p == base + at, "%s: segment %zu at offset %td, after its predecessors %zu", what, i, p - base, at);
    EXPECT((reinterpret_cast<uintptr_t>(p) & 255) == 0 && sizes[i] % 256 == 0, "%s: segment %zu off the 256-byte grid", what, i);
    memset(p, (int)(i + 1), sizes[i]);
    at += sizes[i];
  }
  EXPECT(at == bytes, "%s: the segments hold %zu bytes of %zu", what, at, bytes);
  for (size_t i = 0, o = 0; i < segs.size(); o += sizes[i], ++i)
    for (size_t b = 0; b < sizes[i]; b += 64) EXPECT(base[o + b] == i + 1, "%s: segment %zu overwritten at %zu", what, i, b);
  free(base);
}

template <typename Geom>
static std::vector<size_t> product_sizes(const Geom& g, bool prepared) {
  std::vector<size_t> v;
  if (!prepared) v.push_back(g.u_bytes);
  v.insert(v.end(), {g.v_bytes, g.m_bytes, g.sk_bytes});
  return v;
}
template <typename Geom>
static std::vector<float*> product_segs(Carve& c, const Geom& g, bool prepared) {
  const ProductWs w = carve_product(c, g, prepared);
  std::vector<float*> v;
  if (!prepared) v.push_back(w.U);
  v.insert(v.end(), {w.V, w.M, w.sk});
  return v;
}
template <typename Geom>
static std::vector<float*> grad_segs(Carve& c, const Geom& g) {
  const GradWs w = carve_grad(c, g);
  return {w.V, w.Z, w.slabs, w.bparts};
}
template <typename Geom>
static size_t product_bytes(const Geom& g, bool prepared) {
  Carve c{0};
  carve_product(c, g, prepared);
  return c.at;
}
template <typename Geom>
static size_t grad_bytes(const Geom& g) {
  Carve c{0};
  carve_grad(c, g);
  return c.at;
}

static void check_2d(const Case& q) {
  char what[96];
  const a3d_conv_desc d = desc_of(q, A3D_PREC_F32_WINOGRAD);
  EXPECT(wino_applicable(&d) && wino_grad_applicable(&d), "%dx%dx%dx%dx%d: not taken", q.n, q.h, q.w, q.c, q.k);
  const WinoGradGeom gg = wino_grad_geom(&d);
  const size_t cp = pad4(q.c), kp = pad4(q.k), tx = (size_t)q.n * cdiv(d.ho, 2) * cdiv(d.wo, 2);
  const size_t s = ref_splits(16, q.c, q.k, tx, false);
  const size_t grad_ref = up(16 * tx * cp * 4) + up(16 * tx * kp * 4) + up(16 * s * cp * kp * 4) + up(s * kp * 4);
  const std::vector<size_t> gsizes = {gg.v_bytes, gg.z_bytes, gg.slab_bytes, gg.bias_bytes};
  snprintf(what, sizeof what, "2d %dx%dx%dx%dx%d %s grad", q.n, q.h, q.w, q.c, q.k, q.same ? "SAME" : "VALID");
  EXPECT(gg.splits == (int)s && grad_bytes(gg) == grad_ref, "%s: %zu bytes at %d splits, the reference %zu at %zu", what, grad_bytes(gg),
         gg.splits, grad_ref, s);
  walk(what, grad_bytes(gg), gsizes, [&](Carve& c) { return grad_segs(c, gg); });
  for (int bwd = 0; bwd < 2; ++bwd)
    for (int prepared = 0; prepared < 2; ++prepared) {
      const WinoGeom g = wino_geom(&d, bwd != 0);
      const size_t t = bwd ? (size_t)q.n * cdiv(q.h, 2) * cdiv(q.w, 2) : tx, K = bwd ? kp : cp, N = bwd ? cp : kp;
      const size_t ref = (prepared ? 0 : up(16 * K * N * 4)) + up(16 * t * K * 4) + up(16 * t * N * 4);
      snprintf(what, sizeof what, "2d %dx%dx%dx%dx%d %s bwd %d prepared %d", q.n, q.h, q.w, q.c, q.k, q.same ? "SAME" : "VALID", bwd, prepared);
      EXPECT(product_bytes(g, prepared) == ref, "%s: %zu bytes, the reference %zu", what, product_bytes(g, prepared), ref);
      walk(what, ref, product_sizes(g, prepared), [&](Carve& c) { return product_segs(c, g, prepared); });
      if (!bwd) continue;
      std::vector<size_t> sizes = product_sizes(g, prepared);      // the chain: bwd-data's layout, then the filter gradient's
      sizes.insert(sizes.end(), gsizes.begin(), gsizes.end());
      walk(what, ref + grad_ref, sizes, [&](Carve& c) {
        std::vector<float*> v = product_segs(c, g, prepared), f = grad_segs(c, gg);
        v.insert(v.end(), f.begin(), f.end());
        return v;
      });
    }
}

// tests/wino1d_ref.py: bwd_data_ws_bytes, bwd_filter_ws_bytes
static void check_1d(const Case& q) {
  char what[96];
  const a3d_conv_desc d = desc_of(q, A3D_PREC_F32);
  EXPECT(wino1d_applicable(&d), "%dx%dx%dx%dx%dx%d: not taken", q.n, q.h, q.w, q.c, q.k, q.r);
  const size_t cp = pad4(q.c), kp = pad4(q.k), R = q.r;
  {
    const size_t tw = cdiv(q.w, 4), pv = (size_t)q.n * d.ho * tw, pm = (size_t)q.n * q.h * tw, bn = cp <= 96 ? 96 : 128;
    const long tiles = cdiv(pm, 128) * cdiv(cp, bn), nk = cdiv(R * kp, 32);
    const size_t blocks = std::max(1L, std::min(512L / 8, tiles * nk / 4));
    const Wino1dGeom g = wino1d_geom(&d);
    for (int prepared = 0; prepared < 2; ++prepared) {
      const size_t ref = (prepared ? 0 : up(8 * R * kp * cp * 4)) + up(8 * pv * kp * 4) + up(8 * pm * cp * 4) + up(8 * 2 * blocks * 128 * bn * 4);
      snprintf(what, sizeof what, "1d %dx%dx%dx%dx%dx%d %s bwd-data prepared %d", q.n, q.h, q.w, q.c, q.k, q.r, q.same ? "SAME" : "VALID", prepared);
      EXPECT(product_bytes(g, prepared) == ref, "%s: %zu bytes, the reference %zu", what, product_bytes(g, prepared), ref);
      walk(what, ref, product_sizes(g, prepared), [&](Carve& c) { return product_segs(c, g, prepared); });
    }
  }
  const size_t tw = cdiv(d.wo, 4), px = (size_t)q.n * q.h * tw, pz = (size_t)q.n * d.ho * tw;
  const size_t s = ref_splits(8, R * cp, kp, pz, true);
  const size_t ref = up(8 * px * cp * 4) + up(8 * pz * kp * 4) + up(8 * s * R * cp * kp * 4) + up(s * kp * 4);
  const Wino1dGradGeom gg = wino1d_grad_geom(&d);
  snprintf(what, sizeof what, "1d %dx%dx%dx%dx%dx%d %s grad", q.n, q.h, q.w, q.c, q.k, q.r, q.same ? "SAME" : "VALID");
  EXPECT(gg.splits == (int)s && grad_bytes(gg) == ref, "%s: %zu bytes at %d splits, the reference %zu at %zu", what, grad_bytes(gg), gg.splits,
         ref, s);
  walk(what, ref, {gg.v_bytes, gg.z_bytes, gg.slab_bytes, gg.bias_bytes}, [&](Carve& c) { return grad_segs(c, gg); });
}

int main() {
  // tests/wino_ref.py CASES (n, h, w, c, k, padding), and the two layers at n = 13 of the gradient tests (five uneven splits)
  const Case two_d[] = {{3, 13, 18, 256, 384, 3, 3, true}, {3, 13, 18, 384, 256, 3, 3, true}, {1, 9, 9, 5, 7, 3, 3, true},
                        {2, 6, 8, 32, 200, 3, 3, false}, {1, 1, 1, 4, 4, 3, 3, true},        {1, 2, 3, 8, 8, 3, 3, true},
                        {3, 13, 18, 32, 200, 3, 3, true}, {13, 13, 18, 256, 384, 3, 3, true}, {13, 13, 18, 384, 256, 3, 3, true}};
  // tests/wino1d_ref.py CASES (n, h, w, c, k, r, padding)
  const Case one_d[] = {{1, 3, 5, 8, 12, 5, 5, true},    {2, 3, 6, 8, 12, 5, 5, true},     {3, 6, 7, 6, 5, 5, 5, true},   {2, 7, 8, 8, 12, 5, 5, false},
                        {1, 9, 9, 6, 5, 5, 5, false},    {2, 5, 9, 8, 12, 3, 5, true},     {2, 27, 37, 8, 12, 5, 5, true}, {1, 27, 37, 96, 256, 5, 5, true},
                        {3, 27, 37, 96, 256, 5, 5, true}, {2, 6, 9, 100, 64, 5, 5, true}};
  for (const Case& q : two_d) check_2d(q);
  for (const Case& q : one_d) check_1d(q);
  printf("%s: %zu + %zu descriptors, %d failures\n", failures ? "FAILED" : "ok", sizeof two_d / sizeof *two_d, sizeof one_d / sizeof *one_d, failures);
  return failures != 0;
}
