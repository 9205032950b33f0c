// Pointwise (1x1x1) convolution for 16-bit channels-last activations, host
// side: eligibility, argument set-up, the weight-gradient plan, the C entry
// points and the two small reduce kernels.  The design notes and the kernels
// are in conv_pw_impl.h; the conv_pw_*.hip units instantiate them.
#include "conv_pw_impl.h"
#include "conv_wgrad.h"

namespace {
using namespace vsrk_conv;

// Channel c of a fused reduction: sum of the lane partials that hold its
// column, over (block, wave, lane) in a fixed order, in double.
__global__ __launch_bounds__(256) void pw_red_final_kernel(const float* __restrict__ ws, int nbx, int cop, int ocpr,
                                                           int rstep, int cout, float* __restrict__ o1,
                                                           float* __restrict__ o2) {
  const int c = blockIdx.x;
  if (c >= cout) return;
  const int yc = c / cop, cc = c - yc * cop, col = cc >> 3, e = cc & 7;
  const int nlane = rstep;            // lanes of column col: col + ocpr * k, k < rstep
  const int nitems = nbx * (PW_THR / 64) * nlane;
  double s1 = 0.0, s2 = 0.0;
  constexpr int U = 8;  // loads in flight per lane before the adds (the partials are latency-bound)
  for (int i0 = threadIdx.x; i0 < nitems; i0 += 256 * U) {
    float v1[U], v2[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = i0 + 256 * u;
      v1[u] = v2[u] = 0.f;
      if (i < nitems) {
        const int k = i % nlane, bw = i / nlane;  // bw = block * waves + wave
        const float* p = ws + (((int64_t)yc * nbx * (PW_THR / 64) + bw) * 64 + col + ocpr * k) * 16;
        v1[u] = p[e];
        v2[u] = p[8 + e];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      s1 += v1[u];
      s2 += v2[u];
    }
  }
  __shared__ double r1[256], r2[256];
  r1[threadIdx.x] = s1;
  r2[threadIdx.x] = s2;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (threadIdx.x < k) {
      r1[threadIdx.x] += r1[threadIdx.x + k];
      r2[threadIdx.x] += r2[threadIdx.x + k];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    o1[c] = (float)r1[0];
    o2[c] = (float)r2[0];
  }
}

// dw[co][ci] (torch layout of a 1x1x1 weight, fp32) [+]= scale * sum over
// splits of the slabs; then dbias.  A block = 32 consecutive outputs x 8 split
// groups; group g sums splits g, g+8, ... in order (4 loads in flight), the 8
// partials are added in a fixed order: deterministic.
__global__ __launch_bounds__(256) void pw_wgrad_reduce(const float* __restrict__ ws, float* __restrict__ dw,
                                                      float* __restrict__ db, int nsplit, int nchunks, int slab,
                                                      int cout, int cin, int cop, int cic, int ci_chunks,
                                                      float scale, int accumulate) {
  __shared__ float part[8][32];
  const int l = threadIdx.x & 31, grp = threadIdx.x >> 5;
  const int64_t idx = (int64_t)blockIdx.x * 32 + l;
  const int64_t nw = (int64_t)cout * cin;
  const int64_t total = nw + (db ? cout : 0);
  const float* p = nullptr;
  int co = 0;
  if (idx < nw) {
    co = (int)(idx / cin);
    const int ci = (int)(idx - (int64_t)co * cin);
    const int chunk = (co / cop) * ci_chunks + ci / cic;
    p = ws + (int64_t)chunk * slab + (int64_t)(co % cop) * cic + (ci % cic);
  } else if (idx < total) {
    co = (int)(idx - nw);
    const int chunk = (co / cop) * ci_chunks;
    p = ws + (int64_t)chunk * slab + (int64_t)cop * cic + (co % cop);
  }
  float s = 0.f;
  if (p) {
    const int64_t ss = (int64_t)nchunks * slab;
    int k = grp;
    for (; k + 24 < nsplit; k += 32) {
      const float a0 = p[k * ss], a1 = p[(k + 8) * ss], a2 = p[(k + 16) * ss], a3 = p[(k + 24) * ss];
      s += a0;
      s += a1;
      s += a2;
      s += a3;
    }
    for (; k < nsplit; k += 8) s += p[k * ss];
  }
  part[grp][l] = s;
  __syncthreads();
  if (grp != 0 || idx >= total) return;
  float t = part[0][l];
#pragma unroll
  for (int g = 1; g < 8; ++g) t += part[g][l];
  t *= scale;
  if (idx < nw) {
    float* d = dw + idx;
    *d = accumulate ? *d + t : t;
  } else {
    db[co] = accumulate ? db[co] + t : t;
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
bool dhw_dense(const vsrk_tensor5* t) {
  return t->shuffle <= 1 && t->sw >= t->c && (t->h == 1 || t->sh == (int64_t)t->w * t->sw) &&
         (t->d == 1 || t->sd == (int64_t)t->h * t->sh);
}

// An operand the kernels address like `ref`: its type and shape, dense rows
bool same_geo(const vsrk_tensor5* t, const vsrk_tensor5* ref) {
  return t->dtype == ref->dtype && t->n == ref->n && t->d == ref->d && t->h == ref->h && t->w == ref->w &&
         t->c == ref->c && dhw_dense(t);
}

// Lane offsets relative to the first sample of a span of `span` voxels stay below 2 GiB
bool pw_span_ok(const vsrk_tensor5* t, int dhw, int span) {
  const int64_t span_n = span / std::max(dhw, 1) + 2;
  return 2 * (span_n * t->sn + (int64_t)std::max(dhw, 1) * t->sw + t->c) < 0x7FFFFFF0ll;
}
constexpr int PW_FWD_SPAN = 32 * 4;  // the largest forward tile

int pw_grid(int64_t ntiles) {
  int grid = (int)std::min<int64_t>(vsrk_num_cus(), ceil_div64(ntiles, PW_THR / 64));
  if (vsrk_g_grid_cap > 0) grid = std::min(grid, vsrk_g_grid_cap);
  return std::max(grid, 1);
}

// VSRK_LAUNCH_CHECK for the entry points that return 1 / 0 / -status
#define PW_LAUNCH_CHECK(name)                                                \
  do {                                                                       \
    const hipError_t _e = hipGetLastError();                                 \
    if (_e != hipSuccess) {                                                  \
      vsrk_set_error("%s: launch failed: %s", name, hipGetErrorString(_e));  \
      return -(int)VSRK_ERR_LAUNCH;                                          \
    }                                                                        \
  } while (0)

// The forward / data-gradient arguments common to every pointwise launch;
// false when a lane offset could pass 2 GiB.
bool pw_fill_args(PwArgs& a, const vsrk_conv_desc* d, const vsrk_tensor5* x, const void* w_packed, const float* bias,
                  const float* pro_scale, const float* pro_shift, const vsrk_tensor5* mask, const vsrk_tensor5* y,
                  int cip) {
  a = PwArgs{};
  a.x = x->ptr;
  a.y = y->ptr;
  a.msk = mask ? mask->ptr : nullptr;
  a.w = w_packed;
  a.bias = bias;
  a.pro_scale = pro_scale;
  a.pro_shift = pro_shift;
  a.mask_slope = d->mask_slope;
  a.act_param = d->act_param;
  a.xsn = x->sn; a.xsw = x->sw;
  a.ysn = y->sn; a.ysw = y->sw;
  a.msn = mask ? mask->sn : 0;
  a.msw = mask ? mask->sw : 0;
  a.dhw = x->d * x->h * x->w;
  const int64_t nvox = (int64_t)x->n * a.dhw;
  if (nvox >= (1ll << 31) - 4096) return false;
  a.nvox = (int)nvox;
  a.fd = make_fastdiv(std::max(a.dhw, 1));
  for (const vsrk_tensor5* t : {x, y, mask})
    if (t && !pw_span_ok(t, a.dhw, PW_FWD_SPAN)) return false;
  a.cin = x->c;
  a.cout = y->c;
  a.ci_pad = cip;
  a.co_rows = round_up(y->c, 128);
  a.prologue = d->prologue;
  a.act = d->act;
  a.accumulate = d->accumulate;
  a.has_mask = mask != nullptr;
  a.out_scale = d->out_scale;
  return true;
}

struct PwPbwd {  // the PBWD form (see PwArgs::pbwd)
  int c_lo;
  const vsrk_slope_out* out;
};
}  // namespace

static int fwd_pw_impl(const vsrk_conv_desc* d, const vsrk_tensor5* x, const void* w_packed, const float* bias,
                       const float* pro_scale, const float* pro_shift, const vsrk_tensor5* residual,
                       const vsrk_tensor5* mask, const vsrk_tensor5* y, hipStream_t s, const PwPbwd* pb);

// 1 = launched, 0 = not eligible (caller uses the tile kernels), <0 = -status.
int vsrk_conv_fwd_pw(const vsrk_conv_desc* d, const vsrk_tensor5* x, const void* w_packed, const float* bias,
                     const float* pro_scale, const float* pro_shift, const vsrk_tensor5* residual,
                     const vsrk_tensor5* mask, const vsrk_tensor5* y, hipStream_t s) {
  return fwd_pw_impl(d, x, w_packed, bias, pro_scale, pro_shift, residual, mask, y, s, nullptr);
}

// The data gradient of a pointwise conv with its consumer's PReLU backward
// after the accumulate on output channels >= c_lo (mask = that PReLU's output,
// y's geometry): 1 = launched (*nparts slope partials in ws), 0 = not eligible.
int vsrk_conv_fwd_pw_pbwd(const vsrk_conv_desc* d, const vsrk_tensor5* x, const void* w_packed,
                          const vsrk_tensor5* mask, const vsrk_tensor5* y, int c_lo, const vsrk_slope_out* slope,
                          hipStream_t s) {
  if (!mask || !d->mask_slope || d->prologue || d->act != VSRK_ACT_NONE || d->out_scale != 1.f) return 0;
  if (c_lo < 0 || c_lo >= y->c || c_lo % 8) return 0;
  if (mask->shuffle > 1 || y->shuffle > 1) return 0;
  vsrk_conv_desc dd = *d;
  PwPbwd pb{c_lo, slope};
  return fwd_pw_impl(&dd, x, w_packed, nullptr, nullptr, nullptr, nullptr, mask, y, s, &pb);
}

// grid <= CUs, <= 2 output chunks, one partial per wave
size_t vsrk_pw_pbwd_ws_bytes() { return (size_t)vsrk_num_cus() * 2 * (PW_THR / 64) * sizeof(double); }

static int fwd_pw_impl(const vsrk_conv_desc* d, const vsrk_tensor5* x, const void* w_packed, const float* bias,
                       const float* pro_scale, const float* pro_shift, const vsrk_tensor5* residual,
                       const vsrk_tensor5* mask, const vsrk_tensor5* y, hipStream_t s, const PwPbwd* pb) {
  if (!vsrk_path_mode(VSRK_PATH_PW)) return 0;
  if (!vsrk_is16(x->dtype) || y->dtype != x->dtype) return 0;
  if (d->kd != 1 || d->kh != 1 || d->kw != 1 || d->pd || d->ph || d->pw) return 0;
  if (residual || d->bias_perm_r > 1) return 0;
  if (d->act == VSRK_ACT_PRELU && !d->act_param) return 0;
  if (d->act < VSRK_ACT_NONE || d->act > VSRK_ACT_PRELU) return 0;  // (PReLU of the sum: the tile kernel)
  if (x->n != y->n || x->d != y->d || x->h != y->h || x->w != y->w) return 0;
  if (!dhw_dense(x) || !dhw_dense(y) || (mask && !same_geo(mask, y))) return 0;
  if (x->c % 8 || y->c % 4 || !chunk_ok(x, 2)) return 0;
  if (((uintptr_t)y->ptr) % 8 || y->sn % 4 || y->sw % 4) return 0;
  if (mask && (((uintptr_t)mask->ptr) % 8 || mask->sn % 4 || mask->sw % 4)) return 0;
  const int cip = round_up(x->c, 32);
  const int ncb = cip / 32;  // square kernels: COP = CIP
  if (ncb < 2 || ncb > 8) return 0;
  const int cop_total = round_up(y->c, 32);
  // narrowing convs (DRF's 128..256 -> 64 projections, DUF's 256 -> 16
  // residual head) and the widening data gradients of DRF's 64 -> 128..256
  // projections: one output chunk of cop_total != cip channels (one pass
  // over x instead of cop_total / cip)
  const bool wide_ok = ncb == 2 && (cop_total == 128 || cop_total == 192 || cop_total == 256);
  const int narrow = (cop_total < cip || wide_ok) ? cop_total / 32 : 0;
  if (!narrow && cop_total % cip != 0) return 0;  // output handled in chunks of CIP channels
  const int nchunk = narrow ? 1 : cop_total / cip;
  PwArgs a;
  if (!pw_fill_args(a, d, x, w_packed, bias, pro_scale, pro_shift, mask, y, cip)) return 0;
  if (pb) {  // the mask operand is the PReLU output read after the accumulate
    a.has_mask = 0;
    a.pbwd = 1;
    a.pm_lo = pb->c_lo;
    a.slope_part = pb->out->part;
    *pb->out->nparts = 0;
  }
  if (a.nvox == 0) return 1;
  // the staged kernel of (nc output, nk input) blocks: the narrow / wide pair,
  // or square; 256 input channels in two 128-channel output chunks per 256
  // (x read twice, once per chunk, at the staged kernel's rate).  A form it
  // declines (cout % 8 == 4; a mask or accumulate with a prologue or an
  // activation; a prologue with PReLU) goes to conv_fast or the tile conv.
  int nc = narrow ? narrow : ncb, nchunks = nchunk;
  if (!narrow && ncb == 8) {
    if (pb) return 0;
    nc = 4;
    nchunks = 2 * nchunk;
  }
  a.ntiles = ceil_div(a.nvox, 32 * pw_tile_m(nc, ncb));
  const int grid = pw_grid(a.ntiles);
  if (pb) {  // the grid's slope partials must fit the workspace
    const size_t n = (size_t)grid * nchunks * (PW_THR / 64);
    if (n > pb->out->cap) return 0;
    *pb->out->nparts = (int)n;
  }
  const auto launch = !narrow ? (ncb <= 4 ? pw_fwd_square_lo : pw_fwd_square_hi) : (nc < ncb ? pw_fwd_narrow : pw_fwd_widen);
  if (!launch(nc, ncb, x->dtype, a, grid, nchunks, s)) {
    if (pb) *pb->out->nparts = 0;
    return 0;
  }
  PW_LAUNCH_CHECK("conv_fwd_pw");
  return 1;
}

extern "C" size_t vsrk_conv_fwd_reduce_workspace(const vsrk_conv_desc* d, const vsrk_tensor5* y) {
  const size_t pw = (size_t)vsrk_num_cus() * (PW_THR / 64) * 64 * 16 * sizeof(float);
  if (d && y && d->kd == 3) return std::max(pw, vsrk_roll_bnred_ws_floats(y) * sizeof(float));
  return pw;
}

// the sums of a launch with nothing to reduce
static int pw_zero_sums(float* out_a, float* out_b, int c, hipStream_t s) {
  hipError_t e = hipMemsetAsync(out_a, 0, sizeof(float) * c, s);
  if (e == hipSuccess) e = hipMemsetAsync(out_b, 0, sizeof(float) * c, s);
  if (e != hipSuccess) {
    vsrk_set_error("conv_fwd_reduce: clearing the sums failed: %s", hipGetErrorString(e));
    return VSRK_ERR_LAUNCH;
  }
  return VSRK_OK;
}

// q (with qx, xo): the BNB input form (vsrk_conv_fwd_reduce_bnb), x = q->dz
static int fwd_reduce_impl(const vsrk_conv_desc* d, const vsrk_tensor5* x, const void* w_packed, const float* bias,
                           const float* pro_scale, const float* pro_shift, const vsrk_tensor5* y, int32_t mode,
                           const vsrk_tensor5* bnx, const float* scale, const float* shift, const float* mean,
                           const float* invstd, float* out_a, float* out_b, void* workspace, size_t workspace_bytes,
                           void* stream, const vsrk_tensor5* qx, const vsrk_bn_contrib* q, const vsrk_tensor5* xo) {
  VSRK_CHECK(d && x && y && w_packed && out_a && out_b, "conv_fwd_reduce: null argument");
  VSRK_CHECK(mode == 1 || mode == 2, "conv_fwd_reduce: mode must be 1 (statistics) or 2 (BN+ReLU backward)");
  hipStream_t s = (hipStream_t)stream;
  if (mode == 2 && d->kd == 3 && !q) {
    // the data gradient of a dense unit's Conv3d 3x3x3 (conv2) feeding bn2's
    // backward: the rolling kernel's epilogue form (conv_roll.hip)
    VSRK_CHECK(bnx && scale && shift && mean && invstd, "conv_fwd_reduce: mode 2 needs bnx and the BN constants");
    VSRK_CHECK(workspace, "conv_fwd_reduce: null workspace");
    vsrk_roll_bnred r{bnx, scale, shift, mean, invstd, (float*)workspace, workspace_bytes / sizeof(float), 0, 0};
    const int rc = vsrk_conv_fwd_roll(d, x, w_packed, bias, nullptr, nullptr, nullptr, nullptr, y, s, nullptr, &r);
    if (rc == 0) return VSRK_ERR_UNSUPPORTED;
    if (rc < 0) return -rc;
    if (r.ntiles == 0) return pw_zero_sums(out_a, out_b, y->c, s);
    return vsrk_roll_bnred_final(r, y->c, out_a, out_b, s);
  }
  // eligible: a square pointwise conv on the staged kernel, no epilogue operands
  if (!vsrk_path_mode(VSRK_PATH_PW) || !vsrk_is16(x->dtype) || y->dtype != x->dtype) return VSRK_ERR_UNSUPPORTED;
  if (d->kd != 1 || d->kh != 1 || d->kw != 1 || d->pd || d->ph || d->pw || d->bias_perm_r > 1) return VSRK_ERR_UNSUPPORTED;
  if (d->act != VSRK_ACT_NONE || d->accumulate || d->out_scale != 1.f) return VSRK_ERR_UNSUPPORTED;
  if ((mode == 1) != (d->prologue != VSRK_PRO_NONE)) return VSRK_ERR_UNSUPPORTED;
  if (x->n != y->n || x->d != y->d || x->h != y->h || x->w != y->w || x->c != y->c) return VSRK_ERR_UNSUPPORTED;
  if (!dhw_dense(x) || !dhw_dense(y) || !chunk_ok(x, 2) || !chunk_ok(y, 2) || x->c % 32) return VSRK_ERR_UNSUPPORTED;
  const int ncb = x->c / 32;
  if (ncb < 2 || ncb > 7) return VSRK_ERR_UNSUPPORTED;
  // bnx, qx and xo: read or written in 16-byte chunks at x's geometry
  auto operand_ok = [&](const vsrk_tensor5* t) {
    return same_geo(t, x) && chunk_ok(t, 2) && pw_span_ok(t, x->d * x->h * x->w, PW_FWD_SPAN);
  };
  if (mode == 2) {
    VSRK_CHECK(bnx && scale && shift && mean && invstd, "conv_fwd_reduce: mode 2 needs bnx and the BN constants");
    if (!operand_ok(bnx)) return VSRK_ERR_UNSUPPORTED;
  }
  if (q) {
    if (mode != 2 || bias || d->prologue != VSRK_PRO_NONE || !operand_ok(qx) || !operand_ok(xo)) return VSRK_ERR_UNSUPPORTED;
    VSRK_CHECK(q->shift && q->mean && q->invstd && q->sum_dy && q->sum_dy_xhat && q->count > 0,
               "conv_fwd_reduce_bnb: missing BatchNorm operands");
  }
  PwArgs a;
  if (!pw_fill_args(a, d, x, w_packed, bias, pro_scale, pro_shift, nullptr, y, x->c)) return VSRK_ERR_UNSUPPORTED;
  if (q) {
    a.qx = qx->ptr;
    a.qsn = qx->sn;
    a.qsw = qx->sw;
    a.xo = xo->ptr;
    a.osn = xo->sn;
    a.osw = xo->sw;
    a.qsh = q->shift;
    a.qmu = q->mean;
    a.qis = q->invstd;
    a.qgm = q->gamma;
    a.qsdy = q->sum_dy;
    a.qsdyx = q->sum_dy_xhat;
    a.qinv_count = (float)(1.0 / q->count);
  }
  if (mode == 2) {
    a.bnx = bnx->ptr;
    a.bsn = bnx->sn;
    a.bsw = bnx->sw;
    a.bsc = scale;
    a.bsh = shift;
    a.bmu = mean;
    a.bis = invstd;
  }
  VSRK_CHECK(workspace && workspace_bytes >= vsrk_conv_fwd_reduce_workspace(d, y),
             "conv_fwd_reduce: workspace %zu < %zu bytes", workspace_bytes, vsrk_conv_fwd_reduce_workspace(d, y));
  a.red_ws = (float*)workspace;
  if (a.nvox == 0) return pw_zero_sums(out_a, out_b, y->c, s);
  a.ntiles = ceil_div(a.nvox, 32 * pw_tile_m(ncb, ncb));
  const int grid = std::min(pw_grid(a.ntiles), vsrk_num_cus());
  pw_fwd_reduce(ncb, x->dtype, mode, q != nullptr, a, grid, s);
  VSRK_LAUNCH_CHECK("conv_fwd_reduce");
  const int ocpr = ncb * 4;
  pw_red_final_kernel<<<y->c, 256, 0, s>>>(a.red_ws, grid, 32 * ncb, ocpr, 64 / ocpr, y->c, out_a, out_b);
  VSRK_LAUNCH_CHECK("conv_fwd_reduce_final");
  return VSRK_OK;
}

extern "C" int vsrk_conv_fwd_reduce(const vsrk_conv_desc* d, const vsrk_tensor5* x, const void* w_packed,
                                    const float* bias, const float* pro_scale, const float* pro_shift,
                                    const vsrk_tensor5* y, int32_t mode, const vsrk_tensor5* bnx, const float* scale,
                                    const float* shift, const float* mean, const float* invstd, float* out_a,
                                    float* out_b, void* workspace, size_t workspace_bytes, void* stream) {
  return fwd_reduce_impl(d, x, w_packed, bias, pro_scale, pro_shift, y, mode, bnx, scale, shift, mean, invstd, out_a,
                         out_b, workspace, workspace_bytes, stream, nullptr, nullptr, nullptr);
}

extern "C" int vsrk_conv_fwd_reduce_bnb(const vsrk_conv_desc* d, const vsrk_tensor5* bn_x, const vsrk_bn_contrib* pre,
                                        const vsrk_tensor5* x_out, const void* w_packed, const vsrk_tensor5* y,
                                        const vsrk_tensor5* bnx, const float* scale, const float* shift,
                                        const float* mean, const float* invstd, float* out_a, float* out_b,
                                        void* workspace, size_t workspace_bytes, void* stream) {
  VSRK_CHECK(bn_x && pre && x_out, "conv_fwd_reduce_bnb: null argument");
  return fwd_reduce_impl(d, &pre->dz, w_packed, nullptr, nullptr, nullptr, y, 2, bnx, scale, shift, mean, invstd,
                         out_a, out_b, workspace, workspace_bytes, stream, bn_x, pre, x_out);
}

namespace {
struct PwWPlan {
  bool ok;
  int nco, ncit, nw, ci_chunks, co_chunks, nchunks, nsplit, slab;
  int64_t vps;
  size_t ws_bytes;
};

PwWPlan pw_wgrad_plan(const vsrk_conv_desc* d, const vsrk_tensor5* x, const vsrk_tensor5* dy) {
  PwWPlan p{};
  p.ok = false;
  if (!vsrk_path_mode(VSRK_PATH_PW)) return p;
  if (!vsrk_is16(x->dtype) || dy->dtype != x->dtype) return p;
  if (d->kd != 1 || d->kh != 1 || d->kw != 1 || d->pd || d->ph || d->pw) return p;
  if (x->n != dy->n || x->d != dy->d || x->h != dy->h || x->w != dy->w) return p;
  if (!dhw_dense(x) || !dhw_dense(dy) || !chunk_ok(x, 2) || !chunk_ok(dy, 2)) return p;
  if (x->c % 8 || dy->c % 8) return p;
  const int cob = ceil_div(dy->c, 32), cib = ceil_div(x->c, 32);
  p.nco = std::min(cob, 8);
  p.co_chunks = ceil_div(cob, p.nco);
  // One X block per wave: up to 4 input blocks on 4 waves; 5..8 on 8 waves in
  // one chunk; more in balanced chunks of <= 8.  The reason, measured on the
  // 4-wave kernel (profiles/r4_pw_wgrad_ci8_ab.txt): split into chunks of <= 4
  // blocks, dY is read once per chunk -- twice from 160 channels on; one chunk
  // of up to 8 blocks, two per wave, read dY once and took DUF unit 5
  // (224 -> 224) 1568 -> 1071 us and the heads 256 -> 512 / 512 -> 400 /
  // 256 -> 256 910 / 1741 / 479 -> 657 / 1169 / 372 us, but with twice the
  // accumulators per wave it lost at 160 and 192 channels (1650 -> 1949,
  // 1374 -> 1583 us).  Eight waves keep the single pass over dY with one
  // block, and half those accumulators, per wave.
  p.nw = cib > 4 ? 8 : 4;
  p.ci_chunks = ceil_div(cib, p.nw);
  p.ncit = ceil_div(cib, p.ci_chunks);
  if (p.nco < 2) return p;
  p.nchunks = p.co_chunks * p.ci_chunks;
  const int64_t nvox = (int64_t)x->n * x->d * x->h * x->w;
  if (nvox >= (1ll << 31) - 4096) return p;
  for (const vsrk_tensor5* t : {x, dy})
    if (!pw_span_ok(t, x->d * x->h * x->w, PW_KP)) return p;
  const int64_t steps = std::max<int64_t>(1, ceil_div64(nvox, PW_KP));
  // two workgroups per CU where the double-buffered stage fits LDS twice
  const size_t lds = (size_t)2 * (p.nco + p.nw) * PW_KP * 64;
  int want = std::max(1, vsrk_num_cus() * (lds <= 80 * 1024 ? 2 : 1) / p.nchunks);
  if (vsrk_g_grid_cap > 0) want = std::max(1, vsrk_g_grid_cap / p.nchunks);
  want = (int)std::min<int64_t>(want, steps);
  p.vps = ceil_div64(steps, want) * PW_KP;
  p.nsplit = (int)std::max<int64_t>(1, ceil_div64(nvox, p.vps));
  p.slab = 32 * p.nco * 32 * p.ncit + 32 * p.nco;
  p.ws_bytes = (size_t)p.nsplit * p.nchunks * p.slab * sizeof(float);
  p.ok = true;
  return p;
}

}  // namespace

size_t vsrk_conv_wgrad_pw_workspace(const vsrk_conv_desc* d, const vsrk_tensor5* x, const vsrk_tensor5* dy) {
  const PwWPlan p = pw_wgrad_plan(d, x, dy);
  return p.ok ? p.ws_bytes : 0;
}

// 1 = launched (kernel + reduce), 0 = not eligible, <0 = -status.
int vsrk_conv_wgrad_pw(const vsrk_conv_desc* d, const vsrk_tensor5* x, const vsrk_tensor5* dy,
                       const float* pro_scale, const float* pro_shift, float dy_scale, int32_t perm_r, float* dw,
                       float* dbias, int32_t accumulate, void* workspace, size_t workspace_bytes, hipStream_t s) {
  if (perm_r > 1) return 0;
  const PwWPlan p = pw_wgrad_plan(d, x, dy);
  if (!p.ok) return 0;
  if (!workspace || workspace_bytes < p.ws_bytes) {
    vsrk_set_error("conv_wgrad: workspace %zu < %zu bytes", workspace_bytes, p.ws_bytes);
    return -VSRK_ERR_INVALID;
  }
  PwWArgs a;
  a.x = x->ptr;
  a.dy = dy->ptr;
  a.pro_scale = pro_scale;
  a.pro_shift = pro_shift;
  a.ws = (float*)workspace;
  a.xsn = x->sn; a.xsw = x->sw;
  a.dsn = dy->sn; a.dsw = dy->sw;
  a.nvox = x->n * x->d * x->h * x->w;
  a.vox_per_split = (int)p.vps;
  a.dhw = x->d * x->h * x->w;
  a.fd = make_fastdiv(std::max(a.dhw, 1));
  a.cin = x->c;
  a.cout = dy->c;
  a.prologue = d->prologue;
  a.ncit = p.ncit;
  a.ci_chunks = p.ci_chunks;
  a.nchunks = p.nchunks;
  a.slab = p.slab;
  a.want_bias = dbias != nullptr;
  // (no voxels: the gradient is zero, the reduce below sums nothing)
  if (a.nvox > 0) {
    if (!pw_wgrad(p.nco, p.nw, x->dtype, a, p.nsplit, s)) return 0;
    PW_LAUNCH_CHECK("conv_wgrad_pw");
  }
  const int64_t total = (int64_t)dy->c * x->c + (dbias ? dy->c : 0);
  pw_wgrad_reduce<<<(int)ceil_div64(total, 32), 256, 0, s>>>(
      (const float*)workspace, dw, dbias, a.nvox > 0 ? p.nsplit : 0, p.nchunks, p.slab, dy->c, x->c, 32 * p.nco,
      32 * p.ncit, p.ci_chunks, dy_scale, accumulate);
  PW_LAUNCH_CHECK("conv_wgrad_pw_reduce");
  return 1;
}
