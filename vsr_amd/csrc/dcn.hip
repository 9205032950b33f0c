// Modulated deformable convolution (DCNv2) and deformable convolution (DCNv1)
// sampling kernels for gfx950: the EDVR alignment op of the reference
// (edvr_net/dcn/src/deform_conv_cuda_kernel.cu:189-766, deform_conv.py:97-330).
//
// Split as the reference splits it -- sample (im2col), contraction, and the
// two backward scatters -- but laid out channels-last so the contraction is
// the library's MFMA 1x1 conv (cols (N, Ho, Wo, K*C) x W' (Cout, K*C)) and
// every sampling thread moves 16-byte channel vectors:
//   dcn_im2col:     cols[n,ho,wo,k*C+c] = m * bilinear(x[n,:,:,c], p_k + off)
//   dcn_col2im:     grad_x[n,y,x,c] += m * w_corner * gcols[n,ho,wo,k*C+c]
//                   (float atomics, as the reference's col2im: the one
//                   non-fixed-order sum of the library)
//   dcn_coord_grad: grad_off[n,(g*K+k)*2+{0,1},ho,wo] = sum_c gcols * m * d bilinear/d{h,w}
//                   grad_mask[n,g*K+k,ho,wo]        = sum_c gcols * bilinear
//                   (one thread per (n,ho,wo,g,k), channels in order: deterministic)
// Sampling rule (dmcn_im2col_bilinear, .cu:467-498 / :600-625): position
// h = ho*sh - ph + i*dh + off_h (w likewise); sampled when -1 < h < H and
// -1 < w < W, corners outside the image read as zero.  offset (N, G*2*K,
// Ho, Wo) and mask (N, G*K, Ho, Wo) keep the reference's NCHW layout; x,
// cols, grad_x, gcols are channels-last fp32.
//
// The *_view kernels below are the same three on channels-last VIEWS of fp32 /
// bf16 / fp16 (fp32 arithmetic, 16-byte chunks of the channel axis per lane:
// cl_lane.h; the atomic scatter takes one channel per lane).  They read the
// offsets and masks straight from the raw fp32 output `om` of
// conv_offset_mask, channels-last (N, 1, Ho, Wo, 3*G*K): the reference's
// chunk(3) / cat(o1, o2) / sigmoid (deform_conv.py:261-300) are folded in --
// offset (g, k) is om channels (g*K + k)*2 + {0: h, 1: w}, mask (g, k) is
// sigmoid(om[2*G*K + g*K + k]) -- and the coordinate gradient is the gradient
// of om itself, the sigmoid's m (1 - m) included.
#include <math.h>
#include "cl_lane.h"
#include "../../include/vsrk_dcn.h"

namespace {

struct DcnGeom {
  int n, h, w, c, ho, wo, kh, kw, sh, sw, ph, pw, dh, dw, groups;  // groups = deformable groups
};

struct Sample {
  float hs, ws;  // sampling position
  float m;       // modulation (1 without a mask)
  bool ok;
};

__device__ __forceinline__ Sample sample_at(const DcnGeom& g, const float* __restrict__ off,
                                            const float* __restrict__ msk, int n, int oy, int ox, int grp, int k) {
  const int K = g.kh * g.kw, i = k / g.kw, j = k - (k / g.kw) * g.kw;
  const int64_t plane = (int64_t)g.ho * g.wo, pix = (int64_t)oy * g.wo + ox;
  const float* ob = off + ((int64_t)n * g.groups * 2 * K + (int64_t)(grp * K + k) * 2) * plane;
  Sample s;
  s.hs = (float)(oy * g.sh - g.ph + i * g.dh) + ob[pix];
  s.ws = (float)(ox * g.sw - g.pw + j * g.dw) + ob[plane + pix];
  s.m = msk ? msk[((int64_t)n * g.groups * K + grp * K + k) * plane + pix] : 1.f;
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

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// one thread per (n, ho, wo, k, 4-channel vector)
__global__ __launch_bounds__(256) void dcn_im2col_kernel(DcnGeom g, const float* __restrict__ x,
                                                         const float* __restrict__ off, const float* __restrict__ msk,
                                                         float* __restrict__ cols, int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int C4 = g.c / 4, K = g.kh * g.kw;
  const int c4 = (int)(idx % C4);
  int64_t r = idx / C4;
  const int k = (int)(r % K);
  r /= K;
  const int ox = (int)(r % g.wo);
  r /= g.wo;
  const int oy = (int)(r % g.ho);
  const int n = (int)(r / g.ho);
  const int c = 4 * c4, grp = c / (g.c / g.groups);
  const Sample s = sample_at(g, off, msk, n, oy, ox, grp, k);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (s.ok) {
    const Corners q = corners(s.hs, s.ws, g.h, g.w);
    const float* xb = x + (int64_t)n * g.h * g.w * g.c + c;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (!q.in[t]) continue;
      const int yy = q.hl + (t >> 1), xx = q.wl + (t & 1);
      const float4 u = ld4(xb + ((int64_t)yy * g.w + xx) * g.c);
      v.x += q.wt[t] * u.x;
      v.y += q.wt[t] * u.y;
      v.z += q.wt[t] * u.z;
      v.w += q.wt[t] * u.w;
    }
  }
  v.x *= s.m;
  v.y *= s.m;
  v.z *= s.m;
  v.w *= s.m;
  *reinterpret_cast<float4*>(cols + ((((int64_t)n * g.ho + oy) * g.wo + ox) * K + k) * g.c + c) = v;
}

__global__ __launch_bounds__(256) void dcn_col2im_kernel(DcnGeom g, const float* __restrict__ gcols,
                                                         const float* __restrict__ off, const float* __restrict__ msk,
                                                         float* __restrict__ gx, int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int C4 = g.c / 4, K = g.kh * g.kw;
  const int c4 = (int)(idx % C4);
  int64_t r = idx / C4;
  const int k = (int)(r % K);
  r /= K;
  const int ox = (int)(r % g.wo);
  r /= g.wo;
  const int oy = (int)(r % g.ho);
  const int n = (int)(r / g.ho);
  const int c = 4 * c4, grp = c / (g.c / g.groups);
  const Sample s = sample_at(g, off, msk, n, oy, ox, grp, k);
  if (!s.ok) return;
  const float4 gv = ld4(gcols + ((((int64_t)n * g.ho + oy) * g.wo + ox) * K + k) * g.c + c);
  const Corners q = corners(s.hs, s.ws, g.h, g.w);
  float* xb = gx + (int64_t)n * g.h * g.w * g.c + c;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (!q.in[t]) continue;
    const int yy = q.hl + (t >> 1), xx = q.wl + (t & 1);
    const float f = q.wt[t] * s.m;
    float* p = xb + ((int64_t)yy * g.w + xx) * g.c;
    atomicAdd(p + 0, f * gv.x);
    atomicAdd(p + 1, f * gv.y);
    atomicAdd(p + 2, f * gv.z);
    atomicAdd(p + 3, f * gv.w);
  }
}

// one thread per (n, ho, wo, group, k): the offset and mask gradients of one sample
__global__ __launch_bounds__(256) void dcn_coord_grad_kernel(DcnGeom g, const float* __restrict__ x,
                                                             const float* __restrict__ gcols,
                                                             const float* __restrict__ off,
                                                             const float* __restrict__ msk,
                                                             float* __restrict__ goff, float* __restrict__ gmsk,
                                                             int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  const int K = g.kh * g.kw;
  const int k = (int)(idx % K);
  int64_t r = idx / K;
  const int grp = (int)(r % g.groups);
  r /= g.groups;
  const int ox = (int)(r % g.wo);
  r /= g.wo;
  const int oy = (int)(r % g.ho);
  const int n = (int)(r / g.ho);
  const int cpg = g.c / g.groups;
  const Sample s = sample_at(g, off, msk, n, oy, ox, grp, k);
  float vh = 0.f, vw = 0.f, vm = 0.f;
  if (s.ok) {
    const Corners q = corners(s.hs, s.ws, g.h, g.w);
    const float lh = s.hs - q.hl, lw = s.ws - q.wl;
    // d w_t / d h and d w_t / d w for the four corners (dmcn_get_coordinate_weight)
    const float dwh[4] = {-(1.f - lw), -lw, 1.f - lw, lw};
    const float dww[4] = {-(1.f - lh), 1.f - lh, -lh, lh};
    const float* xb = x + (int64_t)n * g.h * g.w * g.c + grp * cpg;
    const float* gb = gcols + ((((int64_t)n * g.ho + oy) * g.wo + ox) * K + k) * g.c + grp * cpg;
    for (int c = 0; c < cpg; c += 4) {
      const float4 gv = ld4(gb + c);
      float4 bil = make_float4(0.f, 0.f, 0.f, 0.f), dh4 = bil, dw4 = bil;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (!q.in[t]) continue;
        const int yy = q.hl + (t >> 1), xx = q.wl + (t & 1);
        const float4 u = ld4(xb + ((int64_t)yy * g.w + xx) * g.c + c);
        bil.x += q.wt[t] * u.x; bil.y += q.wt[t] * u.y; bil.z += q.wt[t] * u.z; bil.w += q.wt[t] * u.w;
        dh4.x += dwh[t] * u.x; dh4.y += dwh[t] * u.y; dh4.z += dwh[t] * u.z; dh4.w += dwh[t] * u.w;
        dw4.x += dww[t] * u.x; dw4.y += dww[t] * u.y; dw4.z += dww[t] * u.z; dw4.w += dww[t] * u.w;
      }
      vm += gv.x * bil.x + gv.y * bil.y + gv.z * bil.z + gv.w * bil.w;
      vh += gv.x * dh4.x + gv.y * dh4.y + gv.z * dh4.z + gv.w * dh4.w;
      vw += gv.x * dw4.x + gv.y * dw4.y + gv.z * dw4.z + gv.w * dw4.w;
    }
  }
  const int64_t plane = (int64_t)g.ho * g.wo, pix = (int64_t)oy * g.wo + ox;
  float* ob = goff + ((int64_t)n * g.groups * 2 * K + (int64_t)(grp * K + k) * 2) * plane;
  ob[pix] = vh * s.m;
  ob[plane + pix] = vw * s.m;
  if (gmsk) gmsk[((int64_t)n * g.groups * K + grp * K + k) * plane + pix] = vm;
}

// ---- the same kernels on views, offsets and masks decoded from om ----
__device__ __forceinline__ Sample sample_om(const DcnGeom& g, const View& omv, int n, int oy, int ox, int grp, int k) {
  const int K = g.kh * g.kw, i = k / g.kw, j = k - i * g.kw, gk = grp * K + k;
  const float* om = reinterpret_cast<const float*>(omv.ptr) + vsrk_cl::off(omv, n, oy, ox, 0);
  Sample s;
  s.hs = (float)(oy * g.sh - g.ph + i * g.dh) + om[2 * gk];
  s.ws = (float)(ox * g.sw - g.pw + j * g.dw) + om[2 * gk + 1];
  s.m = 1.f / (1.f + expf(-om[2 * g.groups * K + gk]));
  s.ok = s.hs > -1.f && s.ws > -1.f && s.hs < (float)g.h && s.ws < (float)g.w;
  return s;
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
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void dcn_view_im2col_kernel(DcnGeom g, View x, View om, View cols, int nc,
                                                              int64_t total) {
  using L = vsrk_cl::Lane<T, VEC>;
  constexpr int E = L::E;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  int n, oy, ox, k, c0;
  decode_col(idx, nc, g.kh * g.kw, g.wo, g.ho, E, n, oy, ox, k, c0);
  const Sample s = sample_om(g, om, n, oy, ox, c0 / (g.c / g.groups), k);
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
      for (int e = 0; e < E; ++e) v[e] += q.wt[t] * u[e];
    }
  }
#pragma unroll
  for (int e = 0; e < E; ++e) v[e] *= s.m;
  L::store(reinterpret_cast<T*>(cols.ptr) + vsrk_cl::off(cols, n, oy, ox, k * g.c + c0), v);
}

// gx is a zeroed fp32 (N, H, W, C) buffer: float atomics, as dcn_col2im_kernel; one lane per
// (n, ho, wo, k, channel)
template <typename T>
__global__ __launch_bounds__(256) void dcn_view_col2im_kernel(DcnGeom g, View gcols, View om, float* __restrict__ gx,
                                                              int64_t total) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  int n, oy, ox, k, c;
  decode_col(idx, g.c, g.kh * g.kw, g.wo, g.ho, 1, n, oy, ox, k, c);
  const Sample s = sample_om(g, om, n, oy, ox, c / (g.c / g.groups), k);
  if (!s.ok) return;
  const float gv = to_f32<T>(reinterpret_cast<const T*>(gcols.ptr)[vsrk_cl::off(gcols, n, oy, ox, k * g.c + c)]);
  const Corners q = corners(s.hs, s.ws, g.h, g.w);
  float* xb = gx + (int64_t)n * g.h * g.w * g.c + c;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (!q.in[t]) continue;
    atomicAdd(xb + ((int64_t)(q.hl + (t >> 1)) * g.w + (q.wl + (t & 1))) * g.c, q.wt[t] * s.m * gv);
  }
}

// one thread per (n, ho, wo, group, k), channels in order: the three om gradients of one sample
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void dcn_view_coord_grad_kernel(DcnGeom g, View x, View gcols, View om, View gom,
                                                                  int64_t total) {
  using L = vsrk_cl::Lane<T, VEC>;
  constexpr int E = L::E;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= total) return;
  int n, oy, ox, grp, k;
  decode_col(idx, g.kh * g.kw, g.groups, g.wo, g.ho, 1, n, oy, ox, grp, k);
  const int K = g.kh * g.kw, cpg = g.c / g.groups, gk = grp * K + k;
  const Sample s = sample_om(g, om, n, oy, ox, grp, k);
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
          bil[e] += q.wt[t] * u[e];
          dh[e] += dwh[t] * u[e];
          dw[e] += dww[t] * u[e];
        }
      }
#pragma unroll
      for (int e = 0; e < E; ++e) {
        vm += gv[e] * bil[e];
        vh += gv[e] * dh[e];
        vw += gv[e] * dw[e];
      }
    }
  }
  float* o = reinterpret_cast<float*>(gom.ptr) + vsrk_cl::off(gom, n, oy, ox, 0);
  o[2 * gk] = vh * s.m;
  o[2 * gk + 1] = vw * s.m;
  o[2 * g.groups * K + gk] = vm * (s.m * (1.f - s.m));
}

int geom(const int32_t* shp, DcnGeom& g) {
  g = DcnGeom{shp[0], shp[1], shp[2], shp[3], shp[4], shp[5], shp[6], shp[7], shp[8], shp[9],
              shp[10], shp[11], shp[12], shp[13], shp[14]};
  VSRK_CHECK(g.n > 0 && g.h > 0 && g.w > 0 && g.c > 0 && g.ho > 0 && g.wo > 0 && g.kh > 0 && g.kw > 0 &&
                 g.sh > 0 && g.sw > 0 && g.dh > 0 && g.dw > 0 && g.groups > 0,
             "dcn: bad geometry");
  VSRK_CHECK(g.c % g.groups == 0 && (g.c / g.groups) % 4 == 0,
             "dcn: channels per deformable group (%d / %d) must be a multiple of 4", g.c, g.groups);
  return VSRK_OK;
}

int64_t blocks_for(int64_t total) { return (total + 255) / 256; }

int check_t5(const char* name, const char* what, const vsrk_tensor5* t, int dtype, int n, int h, int w, int c) {
  VSRK_CHECK(t && t->ptr, "%s: null %s", name, what);
  VSRK_CHECK(t->shuffle <= 1 && t->d == 1, "%s: %s must be a plain (n, 1, h, w, c) view", name, what);
  VSRK_CHECK(t->dtype == dtype, "%s: %s has dtype %d, expected %d", name, what, t->dtype, dtype);
  VSRK_CHECK(t->n == n && t->h == h && t->w == w && t->c == c,
             "%s: %s is (%d, 1, %d, %d, %d), expected (%d, 1, %d, %d, %d)", name, what, t->n, t->h, t->w, t->c, n, h, w,
             c);
  return VSRK_OK;
}

// geometry and the views every *_view entry point takes: om, the columns, and x where it is read
int view_geom(const char* name, const int32_t* shp, const vsrk_tensor5* x, const vsrk_tensor5* cols,
              const vsrk_tensor5* om, DcnGeom& g) {
  VSRK_CHECK(shp && cols && om, "%s: null argument", name);
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
  VSRK_CHECK(cols->dtype == VSRK_F32 || cols->dtype == VSRK_BF16 || cols->dtype == VSRK_F16, "%s: unknown dtype %d",
             name, cols->dtype);
  // one lane per column chunk in 256-thread workgroups: the grid is a 32-bit count
  VSRK_CHECK((int64_t)g.n * g.ho * g.wo * K * g.c <= ((int64_t)1 << 39) &&
                 (int64_t)g.n * g.h * g.w * g.c <= ((int64_t)1 << 39),
             "%s: tensor too large", name);
  if (int rc = check_t5(name, "cols", cols, cols->dtype, g.n, g.ho, g.wo, (int)(K * g.c))) return rc;
  if (int rc = check_t5(name, "om", om, VSRK_F32, g.n, g.ho, g.wo, (int)(3 * K * g.groups))) return rc;
  if (x)
    if (int rc = check_t5(name, "x", x, cols->dtype, g.n, g.h, g.w, g.c)) return rc;
  return VSRK_OK;
}

// 16-byte chunks need the views to allow them and a chunk to stay inside one deformable group
bool view_vec(const DcnGeom& g, const vsrk_tensor5* cols, const vsrk_tensor5* x) {
  return (g.c / g.groups) % (16 / vsrk_esize(cols->dtype)) == 0 && vsrk_cl::vec_ok(cols) && (!x || vsrk_cl::vec_ok(x));
}

}  // namespace

extern "C" int vsrk_dcn_im2col(const int32_t* geometry, const float* x, const float* offset, const float* mask,
                               float* cols, void* stream) {
  VSRK_CHECK(geometry && x && offset && cols, "dcn_im2col: null argument");
  DcnGeom g;
  if (int rc = geom(geometry, g)) return rc;
  const int64_t total = (int64_t)g.n * g.ho * g.wo * g.kh * g.kw * (g.c / 4);
  dcn_im2col_kernel<<<blocks_for(total), 256, 0, (hipStream_t)stream>>>(g, x, offset, mask, cols, total);
  VSRK_LAUNCH_CHECK("dcn_im2col");
  return VSRK_OK;
}

extern "C" int vsrk_dcn_col2im(const int32_t* geometry, const float* gcols, const float* offset, const float* mask,
                               float* grad_x, void* stream) {
  VSRK_CHECK(geometry && gcols && offset && grad_x, "dcn_col2im: null argument");
  DcnGeom g;
  if (int rc = geom(geometry, g)) return rc;
  const int64_t total = (int64_t)g.n * g.ho * g.wo * g.kh * g.kw * (g.c / 4);
  dcn_col2im_kernel<<<blocks_for(total), 256, 0, (hipStream_t)stream>>>(g, gcols, offset, mask, grad_x, total);
  VSRK_LAUNCH_CHECK("dcn_col2im");
  return VSRK_OK;
}

extern "C" int vsrk_dcn_coord_grad(const int32_t* geometry, const float* x, const float* gcols, const float* offset,
                                   const float* mask, float* grad_offset, float* grad_mask, void* stream) {
  VSRK_CHECK(geometry && x && gcols && offset && grad_offset, "dcn_coord_grad: null argument");
  DcnGeom g;
  if (int rc = geom(geometry, g)) return rc;
  const int64_t total = (int64_t)g.n * g.ho * g.wo * g.groups * g.kh * g.kw;
  dcn_coord_grad_kernel<<<blocks_for(total), 256, 0, (hipStream_t)stream>>>(g, x, gcols, offset, mask, grad_offset,
                                                                            grad_mask, total);
  VSRK_LAUNCH_CHECK("dcn_coord_grad");
  return VSRK_OK;
}

extern "C" int vsrk_dcn_view_im2col(const int32_t* geometry, const vsrk_tensor5* x, const vsrk_tensor5* om,
                                    const vsrk_tensor5* cols, void* stream) {
  VSRK_CHECK(x, "dcn_view_im2col: null argument");
  DcnGeom g;
  if (int rc = view_geom("dcn_view_im2col", geometry, x, cols, om, g)) return rc;
  hipStream_t s = (hipStream_t)stream;
  VSRK_CL_LAUNCH(dcn_view_im2col_kernel, cols->dtype, view_vec(g, cols, x), (int64_t)g.n * g.ho * g.wo * g.kh * g.kw,
                 g.c, g, make_view(x), make_view(om), make_view(cols));
  VSRK_LAUNCH_CHECK("dcn_view_im2col");
  return VSRK_OK;
}

extern "C" int vsrk_dcn_view_col2im(const int32_t* geometry, const vsrk_tensor5* gcols, const vsrk_tensor5* om,
                                    float* grad_x, void* stream) {
  VSRK_CHECK(grad_x, "dcn_view_col2im: null argument");
  DcnGeom g;
  if (int rc = view_geom("dcn_view_col2im", geometry, nullptr, gcols, om, g)) return rc;
  hipStream_t s = (hipStream_t)stream;
  // One channel per lane whatever the views allow: an atomic wave-instruction then adds to 64 consecutive
  // floats (256 contiguous bytes where C >= 64), the shape global float atomics run fastest at; with a chunk
  // per lane each instruction touches 4-byte pieces 16 or 32 bytes apart.
  const int64_t total = (int64_t)g.n * g.ho * g.wo * g.kh * g.kw * g.c;
  const dim3 grid((unsigned)ceil_div64(total, 256));
  const View cv = make_view(gcols), ov = make_view(om);
  if (gcols->dtype == VSRK_BF16) dcn_view_col2im_kernel<bf16><<<grid, 256, 0, s>>>(g, cv, ov, grad_x, total);
  else if (gcols->dtype == VSRK_F16) dcn_view_col2im_kernel<f16><<<grid, 256, 0, s>>>(g, cv, ov, grad_x, total);
  else dcn_view_col2im_kernel<float><<<grid, 256, 0, s>>>(g, cv, ov, grad_x, total);
  VSRK_LAUNCH_CHECK("dcn_view_col2im");
  return VSRK_OK;
}

extern "C" int vsrk_dcn_view_coord_grad(const int32_t* geometry, const vsrk_tensor5* x, const vsrk_tensor5* gcols,
                                        const vsrk_tensor5* om, const vsrk_tensor5* gom, void* stream) {
  VSRK_CHECK(x, "dcn_view_coord_grad: null argument");
  DcnGeom g;
  if (int rc = view_geom("dcn_view_coord_grad", geometry, x, gcols, om, g)) return rc;
  if (int rc = check_t5("dcn_view_coord_grad", "gom", gom, VSRK_F32, g.n, g.ho, g.wo, 3 * g.kh * g.kw * g.groups))
    return rc;
  hipStream_t s = (hipStream_t)stream;
  const bool vec = view_vec(g, gcols, x);
  const int64_t total = (int64_t)g.n * g.ho * g.wo * g.groups * g.kh * g.kw;
  const dim3 grid((unsigned)ceil_div64(total, 256));
  const View xv = make_view(x), cv = make_view(gcols), ov = make_view(om), gv = make_view(gom);
  if (gcols->dtype == VSRK_BF16) {
    if (vec) dcn_view_coord_grad_kernel<bf16, true><<<grid, 256, 0, s>>>(g, xv, cv, ov, gv, total);
    else dcn_view_coord_grad_kernel<bf16, false><<<grid, 256, 0, s>>>(g, xv, cv, ov, gv, total);
  } else if (gcols->dtype == VSRK_F16) {
    if (vec) dcn_view_coord_grad_kernel<f16, true><<<grid, 256, 0, s>>>(g, xv, cv, ov, gv, total);
    else dcn_view_coord_grad_kernel<f16, false><<<grid, 256, 0, s>>>(g, xv, cv, ov, gv, total);
  } else {
    if (vec) dcn_view_coord_grad_kernel<float, true><<<grid, 256, 0, s>>>(g, xv, cv, ov, gv, total);
    else dcn_view_coord_grad_kernel<float, false><<<grid, 256, 0, s>>>(g, xv, cv, ov, gv, total);
  }
  VSRK_LAUNCH_CHECK("dcn_view_coord_grad");
  return VSRK_OK;
}
