// Modulated deformable convolution (DCNv2) and deformable convolution (DCNv1)
// sampling kernels for gfx950: the EDVR alignment op of the reference
// (edvr_net/dcn/src/deform_conv_cuda_kernel.cu:189-766, deform_conv.py:97-330).
//
// Split as the reference splits it -- sample (im2col), contraction, and the
// two backward scatters -- but laid out channels-last so the contraction is
// the library's MFMA 1x1 conv (cols (N, Ho, Wo, K*C) x W' (Cout, K*C)) and
// every sampling lane moves a 16-byte chunk of the channel axis (cl_lane.h):
//   im2col:     cols[n,ho,wo,k*C+c] = m * bilinear(x[n,:,:,c], p_k + off)
//   col2im:     grad_x[n,y,x,c] += m * w_corner * gcols[n,ho,wo,k*C+c]
//               (float atomics, as the reference's col2im: the one
//               non-fixed-order sum of the library)
//   coord_grad: d/d off_{h,w} = m * sum_c gcols * d bilinear/d{h,w}
//               d/d m         =     sum_c gcols * bilinear
//               (one thread per (n,ho,wo,g,k), channels in order: deterministic)
// Sampling rule (dmcn_im2col_bilinear, .cu:467-498 / :600-625): position
// h = ho*sh - ph + i*dh + off_h (w likewise); sampled when -1 < h < H and
// -1 < w < W, corners outside the image read as zero.
//
// There is ONE family of three kernels, on channels-last views of fp32 / bf16 /
// fp16 with fp32 arithmetic.  Both sets of entry points launch it; they differ
// in the sample source, a template parameter that says where a sample's
// (off_h, off_w, m) is read and where its three gradients are written:
//   PlaneSrc  vsrk_dcn_*: offset (N, G*2*K, Ho, Wo) and mask (N, G*K, Ho, Wo;
//             NULL = DCNv1, m = 1) fp32 planes in the reference's NCHW layout;
//             x, cols, gcols are contiguous fp32 buffers, wrapped in views here.
//   OmSrc     vsrk_dcn_view_*: the raw fp32 output `om` of conv_offset_mask,
//             channels-last (N, 1, Ho, Wo, 3*G*K): the reference's chunk(3) /
//             cat(o1, o2) / sigmoid (deform_conv.py:261-300) are folded in --
//             offset (g, k) is om channels (g*K + k)*2 + {0: h, 1: w}, mask
//             (g, k) is sigmoid(om[2*G*K + g*K + k]) -- and the coordinate
//             gradient is the gradient of om itself, the sigmoid's m (1 - m)
//             included.
#include <math.h>
#include "cl_lane.h"
#include "../../include/vsrk_dcn.h"

namespace {

using namespace vsrk_cl;

struct DcnGeom {
  int n, h, w, c, ho, wo, kh, kw, sh, sw, ph, pw, dh, dw, groups;  // groups = deformable groups
};

// ---- sample sources: the offsets and modulation of sample gk = g*K + k at output pixel (n, oy, ox) ----
struct PlaneSrc {
  static constexpr bool FP32_ONLY = true;
  const float* off;
  const float* msk;  // NULL: m = 1
  float* goff;
  float* gmsk;  // may be NULL
  __device__ __forceinline__ void read(const DcnGeom& g, int n, int oy, int ox, int gk, float& oh, float& ow,
                                       float& m) const {
    const int K = g.kh * g.kw;
    const int64_t plane = (int64_t)g.ho * g.wo, pix = (int64_t)oy * g.wo + ox;
    const float* ob = off + ((int64_t)n * g.groups * 2 * K + (int64_t)gk * 2) * plane;
    oh = ob[pix];
    ow = ob[plane + pix];
    m = msk ? msk[((int64_t)n * g.groups * K + gk) * plane + pix] : 1.f;
  }
  // vh, vw, vm: the sums over the channels of gcols * d bilinear / d{h, w} and gcols * bilinear
  __device__ __forceinline__ void write_grad(const DcnGeom& g, int n, int oy, int ox, int gk, float vh, float vw,
                                             float vm, float m) const {
    const int K = g.kh * g.kw;
    const int64_t plane = (int64_t)g.ho * g.wo, pix = (int64_t)oy * g.wo + ox;
    float* ob = goff + ((int64_t)n * g.groups * 2 * K + (int64_t)gk * 2) * plane;
    ob[pix] = vh * m;
    ob[plane + pix] = vw * m;
    if (gmsk) gmsk[((int64_t)n * g.groups * K + gk) * plane + pix] = vm;
  }
};

struct OmSrc {
  static constexpr bool FP32_ONLY = false;
  View om, gom;
  __device__ __forceinline__ void read(const DcnGeom& g, int n, int oy, int ox, int gk, float& oh, float& ow,
                                       float& m) const {
    const float* p = reinterpret_cast<const float*>(om.ptr) + vsrk_cl::off(om, n, oy, ox, 0);
    oh = p[2 * gk];
    ow = p[2 * gk + 1];
    m = 1.f / (1.f + expf(-p[2 * g.groups * g.kh * g.kw + gk]));
  }
  __device__ __forceinline__ void write_grad(const DcnGeom& g, int n, int oy, int ox, int gk, float vh, float vw,
                                             float vm, float m) const {
    float* o = reinterpret_cast<float*>(gom.ptr) + vsrk_cl::off(gom, n, oy, ox, 0);
    o[2 * gk] = vh * m;
    o[2 * gk + 1] = vw * m;
    o[2 * g.groups * g.kh * g.kw + gk] = vm * (m * (1.f - m));
  }
};

struct Sample {
  float hs, ws;  // sampling position
  float m;       // modulation (1 without a mask)
  bool ok;
};

template <typename S>
__device__ __forceinline__ Sample sample(const DcnGeom& g, const S& src, int n, int oy, int ox, int grp, int k) {
  const int i = k / g.kw, j = k - i * g.kw;
  float oh, ow;
  Sample s;
  src.read(g, n, oy, ox, grp * g.kh * g.kw + k, oh, ow, s.m);
  s.hs = (float)(oy * g.sh - g.ph + i * g.dh) + oh;
  s.ws = (float)(ox * g.sw - g.pw + j * g.dw) + ow;
  s.ok = s.hs > -1.f && s.ws > -1.f && s.hs < (float)g.h && s.ws < (float)g.w;
  return s;
}

// bilinear corners: weights w[4] and in-image flags for (hl,wl),(hl,wh),(hh,wl),(hh,wh)
struct Corners {
  int hl, wl;
  float wt[4];
  bool in[4];
};

__device__ __forceinline__ Corners corners(float hs, float ws, int H, int W) {
  Corners c;
  c.hl = (int)floorf(hs);
  c.wl = (int)floorf(ws);
  const float lh = hs - c.hl, lw = ws - c.wl, hh = 1.f - lh, hw = 1.f - lw;
  c.wt[0] = hh * hw;
  c.wt[1] = hh * lw;
  c.wt[2] = lh * hw;
  c.wt[3] = lh * lw;
  c.in[0] = c.hl >= 0 && c.wl >= 0;
  c.in[1] = c.hl >= 0 && c.wl + 1 <= W - 1;
  c.in[2] = c.hl + 1 <= H - 1 && c.wl >= 0;
  c.in[3] = c.hl + 1 <= H - 1 && c.wl + 1 <= W - 1;
  return c;
}

// The sums of the kernels below are written op by op -- fmaf where a product is fused into its sum, mul_rn
// where it is rounded first -- and not left to the compiler's contraction: which products it fuses depends
// on how it vectorises the code around them, and that differed between the two sample sources by an ulp.
// With the ops fixed the plane and the view entry points agree bit for bit on the same samples
// (test_plane_and_view_entry_points_run_one_core).  The forms are the ones the view kernels compiled to
// before, so their results did not change.
// a * b rounded on its own, never contracted into a neighbouring add
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// idx -> (n, oy, ox, k, first channel) over (n, ho, wo, K, c / E); 32-bit divisions below 2^32 lanes
__device__ __forceinline__ void decode_col(int64_t idx, int nc, int K, int wo, int ho, int E, int& n, int& oy,
                                           int& ox, int& k, int& c0) {
  if ((idx >> 32) == 0) {
    uint32_t i = (uint32_t)idx, q = i / (uint32_t)nc;
    c0 = (int)(i - q * nc) * E;
    i = q / (uint32_t)K;
    k = (int)(q - i * K);
    q = i / (uint32_t)wo;
    ox = (int)(i - q * wo);
    i = q / (uint32_t)ho;
    oy = (int)(q - i * ho);
    n = (int)i;
    return;
  }
  c0 = (int)(idx % nc) * E;
  idx /= nc;
  k = (int)(idx % K);
  idx /= K;
  ox = (int)(idx % wo);
  idx /= wo;
  oy = (int)(idx % ho);
  n = (int)(idx / ho);
}

// one lane per (n, ho, wo, k, channel chunk)
template <typename S, typename T, bool VEC>
__global__ __launch_bounds__(256) void dcn_view_im2col_kernel(DcnGeom g, View x, S src, View cols, int nc,
                                                              int64_t total) {
  using L = Lane<T, VEC>;
  constexpr int E = L::E;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  int n, oy, ox, k, c0;
  decode_col(idx, nc, g.kh * g.kw, g.wo, g.ho, E, n, oy, ox, k, c0);
  const Sample s = sample(g, src, n, oy, ox, c0 / (g.c / g.groups), k);
  float v[E];
#pragma unroll
  for (int e = 0; e < E; ++e) v[e] = 0.f;
  if (s.ok) {
    const Corners q = corners(s.hs, s.ws, g.h, g.w);
    const T* xb = reinterpret_cast<const T*>(x.ptr);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (!q.in[t]) continue;
      float u[E];
      L::load(xb + vsrk_cl::off(x, n, q.hl + (t >> 1), q.wl + (t & 1), c0), u);
#pragma unroll
      for (int e = 0; e < E; ++e) v[e] = fmaf(q.wt[t], u[e], v[e]);
    }
  }
#pragma unroll
  for (int e = 0; e < E; ++e) v[e] *= s.m;
  L::store(reinterpret_cast<T*>(cols.ptr) + vsrk_cl::off(cols, n, oy, ox, k * g.c + c0), v);
}

// gx is a zeroed fp32 (N, H, W, C) buffer: float atomics; one lane per (n, ho, wo, k, channel chunk), the
// chunk's channels added one after the other
template <typename S, typename T, bool VEC>
__global__ __launch_bounds__(256) void dcn_view_col2im_kernel(DcnGeom g, View gcols, S src, float* __restrict__ gx,
                                                              int nc, int64_t total) {
  using L = Lane<T, VEC>;
  constexpr int E = L::E;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  int n, oy, ox, k, c0;
  decode_col(idx, nc, g.kh * g.kw, g.wo, g.ho, E, n, oy, ox, k, c0);
  const Sample s = sample(g, src, n, oy, ox, c0 / (g.c / g.groups), k);
  if (!s.ok) return;
  float gv[E];
  L::load(reinterpret_cast<const T*>(gcols.ptr) + vsrk_cl::off(gcols, n, oy, ox, k * g.c + c0), gv);
  const Corners q = corners(s.hs, s.ws, g.h, g.w);
  float* xb = gx + (int64_t)n * g.h * g.w * g.c + c0;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (!q.in[t]) continue;
    const float f = q.wt[t] * s.m;
    float* p = xb + ((int64_t)(q.hl + (t >> 1)) * g.w + (q.wl + (t & 1))) * g.c;
#pragma unroll
    for (int e = 0; e < E; ++e) atomicAdd(p + e, f * gv[e]);
  }
}

// one thread per (n, ho, wo, group, k), channels in order: the three gradients of one sample
template <typename S, typename T, bool VEC>
__global__ __launch_bounds__(256) void dcn_view_coord_grad_kernel(DcnGeom g, View x, View gcols, S src,
                                                                  int64_t total) {
  using L = Lane<T, VEC>;
  constexpr int E = L::E;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  int n, oy, ox, grp, k;
  decode_col(idx, g.kh * g.kw, g.groups, g.wo, g.ho, 1, n, oy, ox, grp, k);
  const int cpg = g.c / g.groups;
  const Sample s = sample(g, src, n, oy, ox, grp, k);
  float vh = 0.f, vw = 0.f, vm = 0.f;
  if (s.ok) {
    const Corners q = corners(s.hs, s.ws, g.h, g.w);
    const float lh = s.hs - q.hl, lw = s.ws - q.wl;
    // d w_t / d h and d w_t / d w for the four corners (dmcn_get_coordinate_weight)
    const float dwh[4] = {-(1.f - lw), -lw, 1.f - lw, lw};
    const float dww[4] = {-(1.f - lh), 1.f - lh, -lh, lh};
    const T* xb = reinterpret_cast<const T*>(x.ptr);
    const T* gb = reinterpret_cast<const T*>(gcols.ptr) + vsrk_cl::off(gcols, n, oy, ox, k * g.c);
    for (int c = grp * cpg; c < (grp + 1) * cpg; c += E) {
      float gv[E], bil[E], dh[E], dw[E];
      L::load(gb + c, gv);
#pragma unroll
      for (int e = 0; e < E; ++e) bil[e] = dh[e] = dw[e] = 0.f;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (!q.in[t]) continue;
        float u[E];
        L::load(xb + vsrk_cl::off(x, n, q.hl + (t >> 1), q.wl + (t & 1), c), u);
#pragma unroll
        for (int e = 0; e < E; ++e) {
          bil[e] = fmaf(q.wt[t], u[e], bil[e]);
          dh[e] = fmaf(dwh[t], u[e], dh[e]);
          dw[e] = fmaf(dww[t], u[e], dw[e]);
        }
      }
#pragma unroll
      for (int e = 0; e < E; ++e) {
        // (a chunk's mask products are rounded before they are added, a single element's is fused)
        vm = VEC ? vm + mul_rn(gv[e], bil[e]) : fmaf(gv[e], bil[e], vm);
        vh = fmaf(gv[e], dh[e], vh);
        vw = fmaf(gv[e], dw[e], vw);
      }
    }
  }
  src.write_grad(g, n, oy, ox, grp * g.kh * g.kw + k, vh, vw, vm, s.m);
}

// ---- host side ----
// the geometry of every entry point
int check_geometry(const char* name, const int32_t* shp, DcnGeom& g) {
  VSRK_CHECK(shp, "%s: null argument", name);
  g = DcnGeom{shp[0], shp[1], shp[2], shp[3], shp[4], shp[5], shp[6], shp[7], shp[8], shp[9],
              shp[10], shp[11], shp[12], shp[13], shp[14]};
  VSRK_CHECK(g.n > 0 && g.h > 0 && g.w > 0 && g.c > 0 && g.ho > 0 && g.wo > 0 && g.kh > 0 && g.kw > 0 &&
                 g.sh > 0 && g.sw > 0 && g.ph >= 0 && g.pw >= 0 && g.dh > 0 && g.dw > 0 && g.groups > 0,
             "%s: bad geometry", name);
  VSRK_CHECK(g.c % g.groups == 0, "%s: %d channels do not divide into %d deformable groups", name, g.c, g.groups);
  VSRK_CHECK(g.ho == (g.h + 2 * g.ph - (g.dh * (g.kh - 1) + 1)) / g.sh + 1 &&
                 g.wo == (g.w + 2 * g.pw - (g.dw * (g.kw - 1) + 1)) / g.sw + 1,
             "%s: output %d x %d does not follow from the input %d x %d", name, g.ho, g.wo, g.h, g.w);
  const int64_t K = (int64_t)g.kh * g.kw;
  VSRK_CHECK(K * g.c <= INT32_MAX / 4 && 3 * K * g.groups <= INT32_MAX / 4, "%s: too many channels", name);
  // one lane per column chunk in 256-thread workgroups: the grid is a 32-bit count
  VSRK_CHECK((int64_t)g.n * g.ho * g.wo * K * g.c <= ((int64_t)1 << 39) &&
                 (int64_t)g.n * g.h * g.w * g.c <= ((int64_t)1 << 39),
             "%s: tensor too large", name);
  return VSRK_OK;
}

// geometry and the views every *_view entry point takes: om, the columns, and x where it is read
int view_geom(const char* name, const int32_t* shp, const vsrk_tensor5* x, const vsrk_tensor5* cols,
              const vsrk_tensor5* om, DcnGeom& g) {
  VSRK_CHECK(cols && om, "%s: null argument", name);
  VSRK_TRY(check_geometry(name, shp, g));
  const int K = g.kh * g.kw;
  VSRK_TRY(check_shape(name, "cols", cols, cols->dtype, g.n, g.ho, g.wo, K * g.c, false));
  VSRK_TRY(check_shape(name, "om", om, VSRK_F32, g.n, g.ho, g.wo, 3 * K * g.groups, false));
  if (x) VSRK_TRY(check_shape(name, "x", x, cols->dtype, g.n, g.h, g.w, g.c, false));
  return VSRK_OK;
}

// geometry of the plane entry points: their contract (vsrk_dcn.h) wants whole fp32 chunks in a deformable group
int plane_geometry(const char* name, const int32_t* shp, DcnGeom& g) {
  VSRK_TRY(check_geometry(name, shp, g));
  VSRK_CHECK((g.c / g.groups) % 4 == 0, "%s: channels per deformable group (%d / %d) must be a multiple of 4", name,
             g.c, g.groups);
  return VSRK_OK;
}

// a contiguous fp32 (n, h, w, c) buffer as a view
vsrk_tensor5 plane_view(const float* p, int n, int h, int w, int c) {
  const int64_t sh = (int64_t)w * c, sn = h * sh;
  return vsrk_tensor5{const_cast<float*>(p), n, 1, h, w, c, sn, sn, sh, c, 1, VSRK_F32};
}

// 16-byte chunks need the views to allow them and a chunk to stay inside one deformable group
bool view_vec(const DcnGeom& g, const vsrk_tensor5* cols, const vsrk_tensor5* x) {
  return (g.c / g.groups) % (16 / vsrk_esize(cols->dtype)) == 0 && vec_ok(cols) && (!x || vec_ok(x));
}

// launch_lanes for the source S: the plane entry points are fp32 only and get no 16-bit instantiations
template <typename S, typename Fn>
void launch_src(int dtype, bool vec, int64_t lanes, void* stream, Fn&& launch) {
  if constexpr (S::FP32_ONLY) launch_lanes_of<float>(vec, lanes, stream, launch);
  else launch_lanes(dtype, vec, lanes, stream, launch);
}

template <typename S>
void launch_im2col(const DcnGeom& g, const vsrk_tensor5* x, const S& src, const vsrk_tensor5* cols, void* stream) {
  const bool vec = view_vec(g, cols, x);
  const int nc = chunks(cols->dtype, vec, g.c);
  const int64_t total = (int64_t)g.n * g.ho * g.wo * g.kh * g.kw * nc;
  launch_src<S>(cols->dtype, vec, total, stream, [&](auto lane, dim3 grid, hipStream_t s) {
    using L = decltype(lane);
    dcn_view_im2col_kernel<S, typename L::Elem, L::Vec><<<grid, 256, 0, s>>>(g, make_view(x), src, make_view(cols), nc,
                                                                             total);
  });
}

template <typename S>
void launch_coord_grad(const DcnGeom& g, const vsrk_tensor5* x, const vsrk_tensor5* gcols, const S& src,
                       void* stream) {
  const int64_t total = (int64_t)g.n * g.ho * g.wo * g.groups * g.kh * g.kw;
  launch_src<S>(gcols->dtype, view_vec(g, gcols, x), total, stream, [&](auto lane, dim3 grid, hipStream_t s) {
    using L = decltype(lane);
    dcn_view_coord_grad_kernel<S, typename L::Elem, L::Vec><<<grid, 256, 0, s>>>(g, make_view(x), make_view(gcols), src,
                                                                                 total);
  });
}

}  // namespace

extern "C" int vsrk_dcn_im2col(const int32_t* geometry, const float* x, const float* offset, const float* mask,
                               float* cols, void* stream) {
  VSRK_CHECK(geometry && x && offset && cols, "dcn_im2col: null argument");
  DcnGeom g;
  VSRK_TRY(plane_geometry("dcn_im2col", geometry, g));
  const vsrk_tensor5 xt = plane_view(x, g.n, g.h, g.w, g.c);
  const vsrk_tensor5 ct = plane_view(cols, g.n, g.ho, g.wo, g.kh * g.kw * g.c);
  launch_im2col(g, &xt, PlaneSrc{offset, mask, nullptr, nullptr}, &ct, stream);
  VSRK_LAUNCH_CHECK("dcn_im2col");
  return VSRK_OK;
}

extern "C" int vsrk_dcn_col2im(const int32_t* geometry, const float* gcols, const float* offset, const float* mask,
                               float* grad_x, void* stream) {
  VSRK_CHECK(geometry && gcols && offset && grad_x, "dcn_col2im: null argument");
  DcnGeom g;
  VSRK_TRY(plane_geometry("dcn_col2im", geometry, g));
  const vsrk_tensor5 ct = plane_view(gcols, g.n, g.ho, g.wo, g.kh * g.kw * g.c);
  // four fp32 channels per lane (unlike vsrk_dcn_view_col2im below)
  const bool vec = view_vec(g, &ct, nullptr);
  const int nc = chunks(VSRK_F32, vec, g.c);
  const int64_t total = (int64_t)g.n * g.ho * g.wo * g.kh * g.kw * nc;
  const PlaneSrc src = {offset, mask, nullptr, nullptr};
  launch_lanes_of<float>(vec, total, stream, [&](auto lane, dim3 grid, hipStream_t s) {
    dcn_view_col2im_kernel<PlaneSrc, float, decltype(lane)::Vec><<<grid, 256, 0, s>>>(g, make_view(&ct), src, grad_x,
                                                                                      nc, total);
  });
  VSRK_LAUNCH_CHECK("dcn_col2im");
  return VSRK_OK;
}

extern "C" int vsrk_dcn_coord_grad(const int32_t* geometry, const float* x, const float* gcols, const float* offset,
                                   const float* mask, float* grad_offset, float* grad_mask, void* stream) {
  VSRK_CHECK(geometry && x && gcols && offset && grad_offset, "dcn_coord_grad: null argument");
  DcnGeom g;
  VSRK_TRY(plane_geometry("dcn_coord_grad", geometry, g));
  const vsrk_tensor5 xt = plane_view(x, g.n, g.h, g.w, g.c);
  const vsrk_tensor5 ct = plane_view(gcols, g.n, g.ho, g.wo, g.kh * g.kw * g.c);
  launch_coord_grad(g, &xt, &ct, PlaneSrc{offset, mask, grad_offset, grad_mask}, stream);
  VSRK_LAUNCH_CHECK("dcn_coord_grad");
  return VSRK_OK;
}

extern "C" int vsrk_dcn_view_im2col(const int32_t* geometry, const vsrk_tensor5* x, const vsrk_tensor5* om,
                                    const vsrk_tensor5* cols, void* stream) {
  VSRK_CHECK(x, "dcn_view_im2col: null argument");
  DcnGeom g;
  VSRK_TRY(view_geom("dcn_view_im2col", geometry, x, cols, om, g));
  launch_im2col(g, x, OmSrc{make_view(om), View{}}, cols, stream);
  VSRK_LAUNCH_CHECK("dcn_view_im2col");
  return VSRK_OK;
}

extern "C" int vsrk_dcn_view_col2im(const int32_t* geometry, const vsrk_tensor5* gcols, const vsrk_tensor5* om,
                                    float* grad_x, void* stream) {
  VSRK_CHECK(grad_x, "dcn_view_col2im: null argument");
  DcnGeom g;
  VSRK_TRY(view_geom("dcn_view_col2im", geometry, nullptr, gcols, om, g));
  // One channel per lane whatever the views allow: an atomic wave-instruction then adds to 64 consecutive
  // floats (256 contiguous bytes where C >= 64), the shape global float atomics run fastest at; with a chunk
  // per lane each instruction touches 4-byte pieces 16 or 32 bytes apart.
  const int64_t total = (int64_t)g.n * g.ho * g.wo * g.kh * g.kw * g.c;
  const dim3 grid((unsigned)ceil_div64(total, 256));
  const OmSrc src = {make_view(om), View{}};
  vsrk_dispatch_dtype(gcols->dtype, [&](auto tag) {
    dcn_view_col2im_kernel<OmSrc, decltype(tag), false><<<grid, 256, 0, (hipStream_t)stream>>>(
        g, make_view(gcols), src, grad_x, g.c, total);
  });
  VSRK_LAUNCH_CHECK("dcn_view_col2im");
  return VSRK_OK;
}

extern "C" int vsrk_dcn_view_coord_grad(const int32_t* geometry, const vsrk_tensor5* x, const vsrk_tensor5* gcols,
                                        const vsrk_tensor5* om, const vsrk_tensor5* gom, void* stream) {
  VSRK_CHECK(x, "dcn_view_coord_grad: null argument");
  DcnGeom g;
  VSRK_TRY(view_geom("dcn_view_coord_grad", geometry, x, gcols, om, g));
  VSRK_TRY(check_shape("dcn_view_coord_grad", "gom", gom, VSRK_F32, g.n, g.ho, g.wo, 3 * g.kh * g.kw * g.groups,
                       false));
  launch_coord_grad(g, x, gcols, OmSrc{make_view(om), make_view(gom)}, stream);
  VSRK_LAUNCH_CHECK("dcn_view_coord_grad");
  return VSRK_OK;
}
