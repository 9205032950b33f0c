// EDVR's TSA fusion operators on channels-last (N, 1, H, W, C) views
// (EDVR_arch.py:257-323), fp32 arithmetic on fp32 / bf16 / fp16 storage, no
// atomics: every sum has a fixed order, so all of them are bitwise reproducible.
//   tsa_tatt:     per-pixel temporal attention (:284-294): the correlation of
//                 each frame's embedding with the centre frame's, its sigmoid,
//                 and the aligned features scaled by it into the frame's channel
//                 slice of the fusion conv's input.
//   pool3s2:      nn.MaxPool2d(3, 2, 1) and nn.AvgPool2d(3, 2, 1) of one input
//                 in one pass, stored [max | avg] (:267-268, 301-308).
//   tsa_modulate: fea * sigmoid(att) * 2 + att_add (:317-320).
// A lane moves one 16-byte chunk of the channel axis (cl_lane.h).  In the
// attention kernels the chunks of one pixel sit in L neighbouring lanes (L the
// power of two >= chunks per pixel, <= 64) and the channel sum is finished with
// an xor butterfly over those lanes, which leaves every lane the same bits.
#include <math.h>
#include "cl_lane.h"

namespace {

using namespace vsrk_cl;

__device__ __forceinline__ float sigmoidf(float v) { return 1.f / (1.f + expf(-v)); }

// sum over the L lanes (a power of two, aligned in the wave) that share a pixel
__device__ __forceinline__ float group_sum(float v, int L) {
  for (int o = L >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// group index -> (image, row, column); 32-bit divisions below 2^32 groups
__device__ __forceinline__ void pixel_of(int64_t g, int w, int h, int& n, int& y, int& x) {
  if ((g >> 32) == 0) {
    uint32_t i = (uint32_t)g, q = i / (uint32_t)w;
    x = (int)(i - q * w);
    i = q / (uint32_t)h;
    y = (int)(q - i * h);
    n = (int)i;
    return;
  }
  x = (int)(g % w);
  g /= w;
  y = (int)(g % h);
  n = (int)(g / h);
}

// ---- temporal attention ----
struct TattFwd {
  View emb, ref, al, out;
  float* prob;  // (B, N, H, W)
  int nframes, nc, lshift;
  int64_t groups;  // B * N * H * W
};

template <typename T, bool VEC> __global__ __launch_bounds__(256) void tatt_fwd_kernel(TattFwd a) {
  constexpr int E = Lane<T, VEC>::E;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int L = 1 << a.lshift, lane = (int)(tid & (L - 1));
  const int64_t grp = tid >> a.lshift;
  const bool live = grp < a.groups && lane < a.nc;
  int bi = 0, y = 0, x = 0;
  if (grp < a.groups) pixel_of(grp, a.emb.w, a.emb.h, bi, y, x);
  const int b = bi / a.nframes, i = bi - b * a.nframes, c0 = lane * E;
  float s = 0.f, v[E];
  if (live) {
    float e[E], r[E];
    Lane<T, VEC>::load(reinterpret_cast<const T*>(a.emb.ptr) + off(a.emb, bi, y, x, c0), e);
    Lane<T, VEC>::load(reinterpret_cast<const T*>(a.ref.ptr) + off(a.ref, b, y, x, c0), r);
#pragma unroll
    for (int k = 0; k < E; ++k) s += e[k] * r[k];
  }
  const float p = sigmoidf(group_sum(s, L));
  if (!live) return;
  Lane<T, VEC>::load(reinterpret_cast<const T*>(a.al.ptr) + off(a.al, bi, y, x, c0), v);
#pragma unroll
  for (int k = 0; k < E; ++k) v[k] *= p;
  Lane<T, VEC>::store(reinterpret_cast<T*>(a.out.ptr) + off(a.out, b, y, x, i * a.emb.c + c0), v);
  if (lane == 0) a.prob[grp] = p;
}

struct TattBwd {
  View emb, ref, al, gout, gemb, gref, gal;
  const float* prob;
  int nframes, nc, lshift;
  int64_t groups;  // B * H * W
};

// One group of lanes per (b, pixel) walks the frames in ascending order, so
// g_emb_ref's sum over the frames has a fixed order.
template <typename T, bool VEC> __global__ __launch_bounds__(256) void tatt_bwd_kernel(TattBwd a) {
  constexpr int E = Lane<T, VEC>::E;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int L = 1 << a.lshift, lane = (int)(tid & (L - 1));
  const int64_t grp = tid >> a.lshift;
  const bool live = grp < a.groups && lane < a.nc;
  int b = 0, y = 0, x = 0;
  if (grp < a.groups) pixel_of(grp, a.ref.w, a.ref.h, b, y, x);
  const int c0 = lane * E, C = a.ref.c;
  const int64_t hw = (int64_t)a.ref.h * a.ref.w, pix = (int64_t)y * a.ref.w + x;
  float r[E], acc[E];
#pragma unroll
  for (int k = 0; k < E; ++k) r[k] = acc[k] = 0.f;
  if (live) Lane<T, VEC>::load(reinterpret_cast<const T*>(a.ref.ptr) + off(a.ref, b, y, x, c0), r);
  for (int i = 0; i < a.nframes; ++i) {
    const int bi = b * a.nframes + i;
    float g[E], v[E], s = 0.f;
    if (live) {
      Lane<T, VEC>::load(reinterpret_cast<const T*>(a.gout.ptr) + off(a.gout, b, y, x, i * C + c0), g);
      Lane<T, VEC>::load(reinterpret_cast<const T*>(a.al.ptr) + off(a.al, bi, y, x, c0), v);
#pragma unroll
      for (int k = 0; k < E; ++k) s += g[k] * v[k];
    }
    s = group_sum(s, L);
    if (!live) continue;
    const float p = a.prob[(int64_t)bi * hw + pix], gcor = s * (p * (1.f - p));
    float e[E];
    Lane<T, VEC>::load(reinterpret_cast<const T*>(a.emb.ptr) + off(a.emb, bi, y, x, c0), e);
#pragma unroll
    for (int k = 0; k < E; ++k) {
      g[k] *= p;
      acc[k] += gcor * e[k];
      e[k] = gcor * r[k];
    }
    Lane<T, VEC>::store(reinterpret_cast<T*>(a.gal.ptr) + off(a.gal, bi, y, x, c0), g);
    Lane<T, VEC>::store(reinterpret_cast<T*>(a.gemb.ptr) + off(a.gemb, bi, y, x, c0), e);
  }
  if (live) Lane<T, VEC>::store(reinterpret_cast<T*>(a.gref.ptr) + off(a.gref, b, y, x, c0), acc);
}

// ---- the 3x3 stride-2 pad-1 max / avg pool pair ----
// window of output o on one axis: input 2 o - 1 .. 2 o + 1, clipped to the image
__device__ __forceinline__ void window(int o, int size, int& lo, int& hi) {
  lo = max(2 * o - 1, 0);
  hi = min(2 * o + 1, size - 1);
}

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void pool3s2_fwd_kernel(View x, View y, int nc, int64_t total) {
  constexpr int E = Lane<T, VEC>::E;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  int n, oy, ox, c0;
  decode(idx, nc, y.w, y.h, E, n, oy, ox, c0);
  int y0, y1, x0, x1;
  window(oy, x.h, y0, y1);
  window(ox, x.w, x0, x1);
  const T* xp = reinterpret_cast<const T*>(x.ptr);
  float best[E], sum[E], v[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    best[e] = -INFINITY;
    sum[e] = 0.f;
  }
  for (int iy = y0; iy <= y1; ++iy)
    for (int ix = x0; ix <= x1; ++ix) {
      Lane<T, VEC>::load(xp + off(x, n, iy, ix, c0), v);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        if (beats(v[e], best[e])) best[e] = v[e];
        sum[e] += v[e];
      }
    }
#pragma unroll
  for (int e = 0; e < E; ++e) sum[e] /= 9.f;  // count_include_pad
  T* yp = reinterpret_cast<T*>(y.ptr) + off(y, n, oy, ox, c0);
  Lane<T, VEC>::store(yp, best);
  Lane<T, VEC>::store(yp + x.c, sum);
}

// One lane per INPUT chunk gathers over the windows that cover it (one or two
// per axis), in row-major output order.  The max part recomputes each window's
// arg-max from the saved input; its sum is rounded to the storage type after
// every term, as torch's CPU kernel accumulates it.  The avg part is summed in
// fp32.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void pool3s2_bwd_kernel(View x, View gy, View gx, int nc, int64_t total) {
  constexpr int E = Lane<T, VEC>::E;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  int n, iy, ix, c0;
  decode(idx, nc, x.w, x.h, E, n, iy, ix, c0);
  const T* xp = reinterpret_cast<const T*>(x.ptr);
  const T* gp = reinterpret_cast<const T*>(gy.ptr);
  float route[E], avg[E];
#pragma unroll
  for (int e = 0; e < E; ++e) route[e] = avg[e] = 0.f;
  const int oy0 = iy >> 1, oy1 = min((iy + 1) >> 1, gy.h - 1), ox0 = ix >> 1, ox1 = min((ix + 1) >> 1, gy.w - 1);
  for (int oy = oy0; oy <= oy1; ++oy)
    for (int ox = ox0; ox <= ox1; ++ox) {
      int y0, y1, x0, x1;
      window(oy, x.h, y0, y1);
      window(ox, x.w, x0, x1);
      float best[E], v[E], g[E];
      bool mine[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        best[e] = -INFINITY;
        mine[e] = y0 == iy && x0 == ix;  // the first position holds until something beats it
      }
      for (int wy = y0; wy <= y1; ++wy)
        for (int wx = x0; wx <= x1; ++wx) {
          Lane<T, VEC>::load(xp + off(x, n, wy, wx, c0), v);
          const bool me = wy == iy && wx == ix;
#pragma unroll
          for (int e = 0; e < E; ++e)
            if (beats(v[e], best[e])) {
              best[e] = v[e];
              mine[e] = me;
            }
        }
      const T* gq = gp + off(gy, n, oy, ox, c0);
      Lane<T, VEC>::load(gq, g);
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (mine[e]) route[e] = to_f32<T>(from_f32<T>(route[e] + g[e]));
      Lane<T, VEC>::load(gq + x.c, g);
#pragma unroll
      for (int e = 0; e < E; ++e) avg[e] += g[e] / 9.f;
    }
#pragma unroll
  for (int e = 0; e < E; ++e) route[e] += avg[e];
  Lane<T, VEC>::store(reinterpret_cast<T*>(gx.ptr) + off(gx, n, iy, ix, c0), route);
}

// ---- sigmoid-gated merge ----
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void modulate_fwd_kernel(View fea, View att, View add, View out, int nc,
                                                           int64_t total) {
  constexpr int E = Lane<T, VEC>::E;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  int n, y, x, c0;
  decode(idx, nc, fea.w, fea.h, E, n, y, x, c0);
  float f[E], a[E], b[E];
  Lane<T, VEC>::load(reinterpret_cast<const T*>(fea.ptr) + off(fea, n, y, x, c0), f);
  Lane<T, VEC>::load(reinterpret_cast<const T*>(att.ptr) + off(att, n, y, x, c0), a);
  Lane<T, VEC>::load(reinterpret_cast<const T*>(add.ptr) + off(add, n, y, x, c0), b);
#pragma unroll
  for (int e = 0; e < E; ++e) f[e] = f[e] * sigmoidf(a[e]) * 2.f + b[e];
  Lane<T, VEC>::store(reinterpret_cast<T*>(out.ptr) + off(out, n, y, x, c0), f);
}

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void modulate_bwd_kernel(View fea, View att, View g, View gfea, View gatt, View gadd,
                                                           int has_gadd, int nc, int64_t total) {
  constexpr int E = Lane<T, VEC>::E;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  int n, y, x, c0;
  decode(idx, nc, fea.w, fea.h, E, n, y, x, c0);
  float f[E], a[E], d[E], gf[E], ga[E];
  Lane<T, VEC>::load(reinterpret_cast<const T*>(fea.ptr) + off(fea, n, y, x, c0), f);
  Lane<T, VEC>::load(reinterpret_cast<const T*>(att.ptr) + off(att, n, y, x, c0), a);
  Lane<T, VEC>::load(reinterpret_cast<const T*>(g.ptr) + off(g, n, y, x, c0), d);
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const float s = sigmoidf(a[e]);
    gf[e] = 2.f * s * d[e];
    ga[e] = 2.f * s * (1.f - s) * f[e] * d[e];
  }
  Lane<T, VEC>::store(reinterpret_cast<T*>(gfea.ptr) + off(gfea, n, y, x, c0), gf);
  Lane<T, VEC>::store(reinterpret_cast<T*>(gatt.ptr) + off(gatt, n, y, x, c0), ga);
  if (has_gadd) Lane<T, VEC>::store(reinterpret_cast<T*>(gadd.ptr) + off(gadd, n, y, x, c0), d);
}

// ---- argument checks ----
// `t` is a view of `like`'s dtype and (n, h, w) with c channels
int check_like(const char* name, const char* what, const vsrk_tensor5* t, const vsrk_tensor5* like, int n, int c) {
  return check_shape(name, what, t, like->dtype, n, like->h, like->w, c);
}

// lanes per pixel of the attention kernels: log2 of the power of two >= nc
int tatt_lshift(const char* name, int c, bool vec, int dtype, int& nc, int& lshift) {
  nc = chunks(dtype, vec, c);
  VSRK_CHECK(nc <= 64, "%s: %d channels%s need more than the 64 lanes of a wavefront", name, c,
             vec ? "" : " (views that do not allow 16-byte accesses)");
  lshift = 0;
  while ((1 << lshift) < nc) ++lshift;
  return VSRK_OK;
}

int check_tatt(const char* name, const vsrk_tensor5* emb, const vsrk_tensor5* ref, const vsrk_tensor5* al,
               const vsrk_tensor5* out, int& nframes) {
  VSRK_TRY(check_view(name, emb));
  VSRK_TRY(check_view(name, ref));
  VSRK_CHECK(emb->n % ref->n == 0, "%s: %d embeddings are no multiple of the %d reference embeddings", name, emb->n,
             ref->n);
  nframes = emb->n / ref->n;
  VSRK_TRY(check_like(name, "emb_ref", ref, emb, ref->n, emb->c));
  VSRK_TRY(check_like(name, "aligned", al, emb, emb->n, emb->c));
  VSRK_CHECK((int64_t)nframes * emb->c <= INT32_MAX, "%s: too many channels", name);
  VSRK_TRY(check_like(name, "out", out, emb, ref->n, nframes * emb->c));
  return VSRK_OK;
}

int check_pool(const char* name, const vsrk_tensor5* x, const vsrk_tensor5* y) {
  VSRK_TRY(check_view(name, x));
  VSRK_TRY(check_view(name, y));
  VSRK_CHECK(x->dtype == y->dtype, "%s: dtype mismatch (%d and %d)", name, x->dtype, y->dtype);
  VSRK_CHECK(y->n == x->n && y->h == (x->h - 1) / 2 + 1 && y->w == (x->w - 1) / 2 + 1 && y->c == 2 * x->c,
             "%s: input (%d, 1, %d, %d, %d) needs the [max | avg] view (%d, 1, %d, %d, %d), got (%d, 1, %d, %d, %d)",
             name, x->n, x->h, x->w, x->c, x->n, (x->h - 1) / 2 + 1, (x->w - 1) / 2 + 1, 2 * x->c, y->n, y->h, y->w,
             y->c);
  return VSRK_OK;
}

}  // namespace

extern "C" int vsrk_tsa_tatt_fwd(const vsrk_tensor5* emb, const vsrk_tensor5* emb_ref, const vsrk_tensor5* aligned,
                                 const vsrk_tensor5* out, float* prob, void* stream) {
  int nframes, nc, lshift;
  VSRK_TRY(check_tatt("tsa_tatt_fwd", emb, emb_ref, aligned, out, nframes));
  VSRK_CHECK(prob, "tsa_tatt_fwd: null argument");
  // out's channel slices start at multiples of c: 16-byte aligned when c is a multiple of the chunk
  const bool vec = vec_ok(emb) && vec_ok(emb_ref) && vec_ok(aligned) && vec_ok(out);
  VSRK_TRY(tatt_lshift("tsa_tatt_fwd", emb->c, vec, emb->dtype, nc, lshift));
  TattFwd a = {make_view(emb), make_view(emb_ref), make_view(aligned), make_view(out), prob, nframes, nc, lshift,
               (int64_t)emb->n * emb->h * emb->w};
  launch_lanes(emb->dtype, vec, a.groups << lshift, stream, [&](auto lane, dim3 grid, hipStream_t s) {
    using L = decltype(lane);
    tatt_fwd_kernel<typename L::Elem, L::Vec><<<grid, 256, 0, s>>>(a);
  });
  VSRK_LAUNCH_CHECK("tsa_tatt_fwd");
  return VSRK_OK;
}

extern "C" int vsrk_tsa_tatt_bwd(const vsrk_tensor5* emb, const vsrk_tensor5* emb_ref, const vsrk_tensor5* aligned,
                                 const float* prob, const vsrk_tensor5* gout, const vsrk_tensor5* g_emb,
                                 const vsrk_tensor5* g_emb_ref, const vsrk_tensor5* g_aligned, void* stream) {
  const char* name = "tsa_tatt_bwd";
  int nframes, nc, lshift;
  VSRK_TRY(check_tatt(name, emb, emb_ref, aligned, gout, nframes));
  VSRK_CHECK(prob, "tsa_tatt_bwd: null argument");
  VSRK_TRY(check_like(name, "g_emb", g_emb, emb, emb->n, emb->c));
  VSRK_TRY(check_like(name, "g_emb_ref", g_emb_ref, emb, emb_ref->n, emb->c));
  VSRK_TRY(check_like(name, "g_aligned", g_aligned, emb, emb->n, emb->c));
  const bool vec = vec_ok(emb) && vec_ok(emb_ref) && vec_ok(aligned) && vec_ok(gout) && vec_ok(g_emb) &&
                   vec_ok(g_emb_ref) && vec_ok(g_aligned);
  VSRK_TRY(tatt_lshift(name, emb->c, vec, emb->dtype, nc, lshift));
  TattBwd a = {make_view(emb), make_view(emb_ref), make_view(aligned), make_view(gout), make_view(g_emb),
               make_view(g_emb_ref), make_view(g_aligned), prob, nframes, nc, lshift,
               (int64_t)emb_ref->n * emb->h * emb->w};
  launch_lanes(emb->dtype, vec, a.groups << lshift, stream, [&](auto lane, dim3 grid, hipStream_t s) {
    using L = decltype(lane);
    tatt_bwd_kernel<typename L::Elem, L::Vec><<<grid, 256, 0, s>>>(a);
  });
  VSRK_LAUNCH_CHECK(name);
  return VSRK_OK;
}

extern "C" int vsrk_pool3s2_fwd(const vsrk_tensor5* x, const vsrk_tensor5* y, void* stream) {
  VSRK_TRY(check_pool("pool3s2_fwd", x, y));
  const bool vec = vec_ok(x) && vec_ok(y);
  const int nc = chunks(x->dtype, vec, x->c);
  const int64_t total = (int64_t)y->n * y->h * y->w * nc;
  launch_lanes(x->dtype, vec, total, stream, [&](auto lane, dim3 grid, hipStream_t s) {
    using L = decltype(lane);
    pool3s2_fwd_kernel<typename L::Elem, L::Vec><<<grid, 256, 0, s>>>(make_view(x), make_view(y), nc, total);
  });
  VSRK_LAUNCH_CHECK("pool3s2_fwd");
  return VSRK_OK;
}

extern "C" int vsrk_pool3s2_bwd(const vsrk_tensor5* x, const vsrk_tensor5* gy, const vsrk_tensor5* gx, void* stream) {
  VSRK_TRY(check_pool("pool3s2_bwd", x, gy));
  VSRK_TRY(check_like("pool3s2_bwd", "gx", gx, x, x->n, x->c));
  const bool vec = vec_ok(x) && vec_ok(gy) && vec_ok(gx);
  const int nc = chunks(x->dtype, vec, x->c);
  const int64_t total = (int64_t)x->n * x->h * x->w * nc;
  launch_lanes(x->dtype, vec, total, stream, [&](auto lane, dim3 grid, hipStream_t s) {
    using L = decltype(lane);
    pool3s2_bwd_kernel<typename L::Elem, L::Vec><<<grid, 256, 0, s>>>(make_view(x), make_view(gy), make_view(gx), nc,
                                                                      total);
  });
  VSRK_LAUNCH_CHECK("pool3s2_bwd");
  return VSRK_OK;
}

extern "C" int vsrk_tsa_modulate_fwd(const vsrk_tensor5* fea, const vsrk_tensor5* att, const vsrk_tensor5* att_add,
                                     const vsrk_tensor5* out, void* stream) {
  const char* name = "tsa_modulate_fwd";
  VSRK_TRY(check_view(name, fea));
  VSRK_TRY(check_like(name, "att", att, fea, fea->n, fea->c));
  VSRK_TRY(check_like(name, "att_add", att_add, fea, fea->n, fea->c));
  VSRK_TRY(check_like(name, "out", out, fea, fea->n, fea->c));
  const bool vec = vec_ok(fea) && vec_ok(att) && vec_ok(att_add) && vec_ok(out);
  const int nc = chunks(fea->dtype, vec, fea->c);
  const int64_t total = (int64_t)fea->n * fea->h * fea->w * nc;
  launch_lanes(fea->dtype, vec, total, stream, [&](auto lane, dim3 grid, hipStream_t s) {
    using L = decltype(lane);
    modulate_fwd_kernel<typename L::Elem, L::Vec><<<grid, 256, 0, s>>>(make_view(fea), make_view(att),
                                                                       make_view(att_add), make_view(out), nc, total);
  });
  VSRK_LAUNCH_CHECK(name);
  return VSRK_OK;
}

extern "C" int vsrk_tsa_modulate_bwd(const vsrk_tensor5* fea, const vsrk_tensor5* att, const vsrk_tensor5* g,
                                     const vsrk_tensor5* gfea, const vsrk_tensor5* gatt, const vsrk_tensor5* gatt_add,
                                     void* stream) {
  const char* name = "tsa_modulate_bwd";
  VSRK_TRY(check_view(name, fea));
  VSRK_TRY(check_like(name, "att", att, fea, fea->n, fea->c));
  VSRK_TRY(check_like(name, "g", g, fea, fea->n, fea->c));
  VSRK_TRY(check_like(name, "gfea", gfea, fea, fea->n, fea->c));
  VSRK_TRY(check_like(name, "gatt", gatt, fea, fea->n, fea->c));
  if (gatt_add) VSRK_TRY(check_like(name, "gatt_add", gatt_add, fea, fea->n, fea->c));
  const bool vec = vec_ok(fea) && vec_ok(att) && vec_ok(g) && vec_ok(gfea) && vec_ok(gatt) &&
                   (!gatt_add || vec_ok(gatt_add));
  const int nc = chunks(fea->dtype, vec, fea->c);
  const int64_t total = (int64_t)fea->n * fea->h * fea->w * nc;
  launch_lanes(fea->dtype, vec, total, stream, [&](auto lane, dim3 grid, hipStream_t s) {
    using L = decltype(lane);
    modulate_bwd_kernel<typename L::Elem, L::Vec><<<grid, 256, 0, s>>>(
        make_view(fea), make_view(att), make_view(g), make_view(gfea), make_view(gatt),
        make_view(gatt_add ? gatt_add : g), gatt_add ? 1 : 0, nc, total);
  });
  VSRK_LAUNCH_CHECK(name);
  return VSRK_OK;
}
