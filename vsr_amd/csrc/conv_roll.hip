// Host entry of the rolling-depth conv with 16-row tiles (the kernel and its
// design notes are in conv_roll_impl.h): eligibility, argument set-up and
// dispatch of the Conv3d 3x3x3 and the 2-D 3x3 forms, the fused PReLU-backward
// entry point and the final kernel of the fused BN+ReLU backward reduce.
#include "conv_roll_impl.h"

namespace {

// Channel c of the fused BN+ReLU backward reduce: the (tile, wave) partials
// of the tiles whose output block holds c (tile order: block fastest), in a
// fixed order, in double.  A (tile, wave) record is [sum: 32 | sum xhat: 32]
// over the block's channels.
__global__ __launch_bounds__(256) void roll_bnred_final_kernel(const float* __restrict__ ws, int ntiles, int ntn,
                                                               int cout, const float* __restrict__ invstd,
                                                               float* __restrict__ o1, float* __restrict__ o2) {
  const int c = blockIdx.x;
  if (c >= cout) return;
  const int blk = c >> 5, cc = c & 31;
  const int nt = (ntiles - blk + ntn - 1) / ntn;  // tiles blk, blk + ntn, ...
  double s1 = 0.0, s2 = 0.0;
  constexpr int U = 8;  // loads in flight per lane before the adds (the partials are latency-bound)
  const int n = nt * RNW;
  for (int i0 = threadIdx.x; i0 < n; i0 += 256 * U) {
    float v1[U], v2[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = i0 + 256 * u;
      v1[u] = v2[u] = 0.f;
      if (i < n) {
        const int t = blk + ntn * (i / RNW), w = i % RNW;
        const float* p = ws + ((int64_t)t * RNW + w) * 64;
        v1[u] = p[cc];
        v2[u] = p[32 + cc];
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
    o2[c] = (float)(r2[0] * (double)invstd[c]);  // the partials are sums of dy' (x - mean)
  }
}

}  // namespace

size_t vsrk_roll_slope_ws_bytes() { return (size_t)vsrk_num_cus() * RNW * sizeof(double); }

// 1 = launched (2: on the wide row kernel), 0 = not eligible, < 0 = -(error status)
static int roll_fwd_one(const vsrk_conv_desc* d, const vsrk_tensor5* x, const void* w_packed, const float* bias,
                        const float* pro_scale, const float* pro_shift, const vsrk_tensor5* residual,
                        const vsrk_tensor5* mask, const vsrk_tensor5* y, hipStream_t s, const vsrk_slope_out* slope,
                        vsrk_roll_bnred* bnred);

// The rolling kernels address their views with 32-bit element offsets.  A
// batch whose views span more (DUF's 256-channel concat buffer at cfg 5:
// 128 windows x 7 x 128 x 128 x 256 = 3.8e9 elements) is launched in sample
// chunks that fit, for the forms without a cross-sample reduction (the BN
// reduce and the PReLU slope partials are per launch); before, such a
// batch fell back to conv_fast.
int vsrk_conv_fwd_roll(const vsrk_conv_desc* d, const vsrk_tensor5* x, const void* w_packed, const float* bias,
                       const float* pro_scale, const float* pro_shift, const vsrk_tensor5* residual,
                       const vsrk_tensor5* mask, const vsrk_tensor5* y, hipStream_t s, const vsrk_slope_out* slope,
                       vsrk_roll_bnred* bnred) {
  auto span = [](const vsrk_tensor5* t, int64_t n) -> int64_t {  // as roll_fwd_one's check, for n samples
    const int64_t r = t->shuffle > 1 ? t->shuffle : 1;
    return (n - 1) * t->sn + (int64_t)(t->d - 1) * t->sd + (int64_t)(r * (t->h + RFTH + 2) - 1) * t->sh +
           (int64_t)(r * (t->w + 2 * RHW) - 1) * t->sw + t->c;
  };
  const vsrk_tensor5* ts[4] = {x, y, residual, mask};
  auto fits = [&](int64_t n) {
    for (const vsrk_tensor5* t : ts)
      if (t && span(t, n) >= (1ll << 31)) return false;
    return true;
  };
  if (slope || bnred || x->n <= 1 || y->n != x->n || fits(x->n))
    return roll_fwd_one(d, x, w_packed, bias, pro_scale, pro_shift, residual, mask, y, s, slope, bnred);
  for (const vsrk_tensor5* t : ts)
    if (t && (t->n != x->n || t->sn < 0)) return 0;
  int nc = x->n;
  while (nc > 1 && !fits(nc)) nc = (nc + 1) / 2;
  if (!fits(nc)) return 0;
  for (int n0 = 0; n0 < x->n; n0 += nc) {
    vsrk_tensor5 c[4];
    for (int i = 0; i < 4; ++i) {
      if (!ts[i]) continue;
      c[i] = *ts[i];
      c[i].n = std::min(nc, x->n - n0);
      c[i].ptr = (char*)ts[i]->ptr + (int64_t)n0 * ts[i]->sn * vsrk_esize(ts[i]->dtype);
    }
    const int rc = roll_fwd_one(d, &c[0], w_packed, bias, pro_scale, pro_shift, residual ? &c[2] : nullptr,
                                mask ? &c[3] : nullptr, &c[1], s, nullptr, nullptr);
    if (rc == 0 && n0 == 0) return 0;  // not eligible: nothing launched
    if (rc == 0) return -VSRK_ERR_INVALID;  // (same shapes, fewer samples: cannot happen)
    if (rc < 0) return rc;
  }
  return 1;
}

static int roll_fwd_one(const vsrk_conv_desc* d, const vsrk_tensor5* x, const void* w_packed, const float* bias,
                        const float* pro_scale, const float* pro_shift, const vsrk_tensor5* residual,
                        const vsrk_tensor5* mask, const vsrk_tensor5* y, hipStream_t s, const vsrk_slope_out* slope,
                        vsrk_roll_bnred* bnred) {
  const int roll_mode = vsrk_path_mode(VSRK_PATH_ROLL);  // 0 off, 1 forced on, 2 automatic
  // resident weights (WR): 0 off, 1 where faster, 2 also with the prefetched
  // residual / mask epilogue (tests)
  const int wres_mode = vsrk_path_mode(VSRK_PATH_ROLL_WR);
  if (roll_mode == 0) return 0;
  if (!vsrk_is16(x->dtype) || y->dtype != x->dtype) return 0;
  if (d->kh != 3 || d->kw != 3) return 0;
  // the two forms: Conv3d 3x3x3 (32-channel output blocks) and 3x3 over
  // depth-1 slices with 64-channel output blocks (cout a multiple of 64)
  const bool k3 = d->kd == 3;
  if (!k3 && !(d->kd == 1 && d->pd == 0 && y->c % 64 == 0)) return 0;
  // PReLU-backward mask (slope): the mask has y's geometry and strides
  const bool pmask = slope != nullptr;
  if ((d->bias_perm_r > 1 && (y->shuffle != d->bias_perm_r || y->c % (d->bias_perm_r * d->bias_perm_r))) ||
      (d->mask_slope && !pmask))
    return 0;
  if (pmask) {
    if (!mask || !d->mask_slope || residual || d->kd != 1 || d->prologue) return 0;
    if (mask->dtype != y->dtype || mask->shuffle != y->shuffle || mask->n != y->n || mask->d != y->d ||
        mask->h != y->h || mask->w != y->w || mask->c != y->c || mask->sn != y->sn ||
        (y->d > 1 && mask->sd != y->sd) ||
        mask->sh != y->sh || mask->sw != y->sw)
      return 0;
  }
  if (d->act == VSRK_ACT_PRELU && (k3 || !d->act_param)) return 0;
  // PReLU of the sum (RBPN's block tail): the plain 2-D form with a residual
  // operand only; an unknown activation code is nobody's
  const bool sumact = d->act == VSRK_ACT_PRELU_SUM;
  if (d->act < VSRK_ACT_NONE || d->act > VSRK_ACT_PRELU_SUM) return 0;
  if (sumact && (k3 || !d->act_param || !residual || mask || d->accumulate || d->prologue || x->shuffle > 1 ||
                 y->shuffle > 1 || bnred))
    return 0;
  if (k3 && (residual || mask || d->accumulate)) return 0;
  // a single output depth from three slices (DUF's last unit): the depth-
  // folded 2-D form (conv_roll_fold.hip)
  if (k3 && y->d == 1 && x->d == 3 && d->pd == 0 && !bnred && !residual && !mask && !pmask &&
      vsrk_path_mode(VSRK_PATH_ROLL_FOLD) != 0) {
    if (const int rf = vsrk_conv_fwd_roll_fold(d, x, w_packed, bias, pro_scale, pro_shift, y, s)) return rf;
  }
  // automatic mode: a single output depth has no slice reuse to roll over;
  // the per-kd-stage kernel is faster there (DUF's last unit, 3 -> 1 slices
  // at F = 224: 817 vs 943 us, r3p microbench)
  if (roll_mode == 2 && k3 && y->d == 1 && !bnred && vsrk_g_roll_dz == 0) return 0;
  if (bnred) {
    const vsrk_tensor5* b = bnred->bnx;
    if (!k3 || d->prologue || d->act != VSRK_ACT_NONE || bias || d->out_scale != 1.f || !b || b->dtype != y->dtype ||
        b->shuffle > 1 ||
        b->n != y->n || b->d != y->d || b->h != y->h || b->w != y->w || b->c != y->c || b->sn != y->sn ||
        b->sd != y->sd || b->sh != y->sh || b->sw != y->sw)
      return 0;
  }
  // sub-pixel operands (2-D only, one of x / y): each 16-channel input chunk
  // (x) or 32-channel output block (y) must lie inside one phase
  const int sp = x->shuffle > 1 ? SP_X : (y->shuffle > 1 ? SP_Y : SP_NONE);
  if (x->shuffle > 1 && y->shuffle > 1) return 0;
  if (sp != SP_NONE) {
    if (k3 || d->prologue || residual || (mask && !pmask)) return 0;
    const vsrk_tensor5* t = sp == SP_X ? x : y;
    const int r = t->shuffle, cph = t->c / (r * r);
    if (cph * r * r != t->c || cph % (sp == SP_X ? RCH : 32) != 0) return 0;
    if (t->c / (sp == SP_X ? RCH : 32) > RMAXSUB) return 0;
  }
  if (x->c % RCH != 0 || !chunk_ok(x, 2)) return 0;
  if (d->pd < 0 || d->pd > 2 || d->ph < 0 || d->ph > 2 || d->pw < 0 || d->pw > 2) return 0;
  if (y->d != x->d + 2 * d->pd - (d->kd - 1) || y->h != x->h + 2 * d->ph - 2 || y->w != x->w + 2 * d->pw - 2) return 0;
  auto out_ok = [&](const vsrk_tensor5* t) {  // 8-byte epilogue accesses, the output's geometry
    return t->dtype == y->dtype && (t->shuffle <= 1 || (t == y && sp == SP_Y)) && t->n == y->n && t->d == y->d &&
           t->h == y->h && t->w == y->w &&
           t->c == y->c && ((uintptr_t)t->ptr) % 8 == 0 && t->sn % 4 == 0 && t->sd % 4 == 0 && t->sh % 4 == 0 &&
           t->sw % 4 == 0;
  };
  if (y->c % (k3 ? 8 : 4) != 0 || !out_ok(y)) return 0;
  if ((residual && !out_ok(residual)) || (mask && !pmask && !out_ok(mask))) return 0;
  for (const vsrk_tensor5* t : {x, y, residual, mask}) {  // every element offset fits in 32 bits
    if (!t) continue;
    const int64_t r = t->shuffle > 1 ? t->shuffle : 1;
    const int64_t span = (int64_t)(t->n - 1) * t->sn + (int64_t)(t->d - 1) * t->sd +
                         (int64_t)(r * (t->h + RFTH + 2) - 1) * t->sh + (int64_t)(r * (t->w + 2 * RHW) - 1) * t->sw +
                         t->c;
    if (span >= (1ll << 31) || t->sn < 0 || t->sd < 0 || t->sh < 0 || t->sw < 0) return 0;
  }
  // EDSR's 64 -> 64 body convs: the row-walking kernel (conv_row.hip) takes
  // the forms it covers.  An explicit roll_wr setting (0 or 2) asks for one
  // of the tile kernel's two forms: the row kernel stands aside.
  if (!k3 && sp == SP_NONE && !pmask && !bnred && wres_mode == 1) {
    if (const int rw = vsrk_conv_fwd_row(d, x, w_packed, bias, residual, mask, y, s)) return rw;
  }
  // EDSR's 64 -> 256 up-sampler convs through a shuffle-2 output view: the
  // wide row-walking kernel (conv_row_wide.hip); 2 = launched there (the
  // dispatch log tells it from the tile kernel)
  if (sp == SP_Y && !k3 && !pmask && !bnred) {
    if (const int rw = vsrk_conv_fwd_row_wide(d, x, w_packed, bias, residual, mask, y, s)) return rw > 0 ? 2 : rw;
  }
  // a shuffled view walks the low-res grid: its row / column strides are r
  // physical rows / columns (the phase lives in the channel offset table)
  auto rview = [](const vsrk_tensor5* t) {
    RView v;
    const int r = t->shuffle > 1 ? t->shuffle : 1;
    v.ptr = (char*)t->ptr;
    v.d = t->d; v.h = t->h; v.w = t->w;
    v.sn = (int)t->sn; v.sd = (int)t->sd; v.sh = (int)(r * t->sh); v.sw = (int)(r * t->sw);
    return v;
  };
  RollArgs a;
  a.x = rview(x);
  a.y = rview(y);
  a.res = rview(residual ? residual : y);
  a.msk = rview(mask ? mask : y);
  a.w = w_packed;
  a.bias = bias;
  a.bias_r = d->bias_perm_r > 1 ? d->bias_perm_r : 1;
  a.pro_scale = pro_scale;
  a.pro_shift = pro_shift;
  a.cin = x->c;
  a.cout = y->c;
  a.cin_pad = round_up(x->c, 32);
  a.cout_pad = round_up(y->c, 128);
  a.pd = d->pd;
  a.ph = d->ph;
  a.pw = d->pw;
  a.prologue = d->prologue;
  a.out_scale = d->out_scale;
  a.nchunk = x->c / RCH;
  a.act_param = d->act_param;
  a.prio = vsrk_g_roll_prio;
  if (sp != SP_NONE) {
    const vsrk_tensor5* t = sp == SP_X ? x : y;
    const int r = t->shuffle, cph = t->c / (r * r), step = sp == SP_X ? RCH : 32;
    for (int i = 0; i < t->c / step; ++i) {
      const int c = i * step, sub = c / cph, cc = c - sub * cph;
      a.spoff[i] = (int)((sub / r) * t->sh + (sub % r) * t->sw + cc);
      a.sptap[i] = subpixel_tapmask(d->subpixel, r, sub);
    }
  }
  const int nt = k3 ? 1 : 2;
  const int tiles_h = ceil_div(y->h, RFTH), tiles_w = ceil_div(y->w, TW), ntn = ceil_div(y->c, 32 * nt);
  const int64_t spatial = (int64_t)y->n * tiles_h * tiles_w * ntn;
  if (spatial == 0 || y->d == 0) return 1;
  // Depth run per tile: as long as possible (each input slice then serves
  // three output depths) while the grid still gets >= 2 tiles per CU.
  int dzc = y->d;
  if (vsrk_g_roll_dz > 0) {
    dzc = std::min(vsrk_g_roll_dz, y->d);
  } else if (k3) {
    const int64_t want = 2 * (int64_t)vsrk_num_cus();
    if (spatial < want) {
      const int64_t runs = std::min<int64_t>(ceil_div64(want, spatial), y->d);
      dzc = (int)ceil_div64(y->d, runs);
    }
  } else {
    dzc = 1;  // 2-D: a tile is one slice
  }
  a.dzc = dzc;
  const int nzc = ceil_div(y->d, dzc);
  a.ntn = make_rdiv(ntn);
  a.nzc = make_rdiv(nzc);
  a.tiles_w = make_rdiv(tiles_w);
  a.tiles_h = make_rdiv(tiles_h);
  const int64_t ntiles = spatial * nzc;
  VSRK_CHECK(ntiles < (1ll << 31), "conv_fwd(roll): too many tiles");
  a.ntiles = (int)ntiles;
  // resident weights (WR): plain views, no prologue, the weight image of an
  // output block <= 80 KB, and (2-D) one output block for the whole launch
  // -- EDSR's 64 -> 64 body convs -- or (3-D) whole-depth tiles, where a
  // reload per tile is amortised over nsl x nchunk stages (DUF's data
  // gradients 32 -> F).  VSRK_ROLL_WRES=0 turns it off (A/B).
  const size_t nb = k3 ? RollGeo<3, 1>::NB : RollGeo<1, 2>::NB;
  const size_t wbytes = (size_t)a.nchunk * nb * 1024;
  const size_t tables = (size_t)a.cout_pad * 4 + (d->prologue || bnred ? 2 * (size_t)a.cin_pad * 4 : 0) +
                        (bnred ? 4 * (size_t)a.cout_pad * 4 : 0);
  const size_t wslot = k3 ? RollGeo<3, 1, 1>::SLOT : RollGeo<1, 2, 1>::SLOT;
  // (2-D: not with a prefetched residual / mask operand unless forced (mode
  // 2): correct -- tests/test_roll_gpu.py compares the forced form bitwise
  // with the streamed one; round 4's wrong results came with the inline-asm
  // prefetch, whose registers the compiler could re-use before the data
  // landed, since removed -- but slower: EDSR res 129 -> 146 us, mask
  // 147 -> 163 us per launch (profiles/r5_roll_wr_prefetch_ab.txt))
  const bool pref2d =
      wres_mode != 2 && !k3 && ((residual != nullptr) != (mask != nullptr && !pmask)) && !d->accumulate;
  const bool wr = wres_mode && sp == SP_NONE && !d->prologue && wbytes <= 80 * 1024 && !pref2d &&
                  (k3 ? dzc == y->d : ntn == 1) && (size_t)RNSLOT * wslot + wbytes + tables <= 160 * 1024;
  const size_t slot = wr ? wslot : (k3 ? RollGeo<3, 1>::SLOT : RollGeo<1, 2>::SLOT);
  const size_t lds = (size_t)RNSLOT * slot + (wr ? wbytes : 0) + tables;
  if (bnred) {
    if (bnred->ws_floats < (size_t)ntiles * RNW * 64) return 0;
    a.bnx = (const char*)bnred->bnx->ptr;
    a.msk = rview(bnred->bnx);  // the epilogue operand prefetch reads the BN input through msk
    a.bn_sc = bnred->scale;
    a.bn_sh = bnred->shift;
    a.bn_mu = bnred->mean;
    a.bn_is = bnred->invstd;
    a.red_ws = bnred->ws;
    bnred->ntiles = (int)ntiles;
    bnred->ntn = ntn;
  }
  if (lds > 160 * 1024) return 0;
  const int grid = (int)vsrk_capped_grid(std::min<int64_t>(ntiles, vsrk_num_cus()));
  const bool relu = d->act == VSRK_ACT_RELU;
  const int em = (residual ? RE_RES : 0) | (mask ? (pmask ? RE_PMASK : RE_MASK) : 0) | (d->accumulate ? RE_ACC : 0) |
                 (relu ? RE_RELU : 0) | (d->act == VSRK_ACT_PRELU ? RE_PRELU : 0) | (sumact ? RE_SUMACT : 0);
  a.mask_slope = d->mask_slope;
  if (pmask) {
    if ((size_t)grid * RNW > slope->cap) return 0;
    a.slope_part = slope->part;
    *slope->nparts = grid * RNW;
  }
  int rc = vsrk_dispatch16(x->dtype, [&](auto tag) {
    using H = decltype(tag);
    if (k3) {
      if (bnred)
        return wr ? launch_roll<3, 1, 0, RE_BNRED, SP_NONE, H, 1>(a, lds, grid, s)
                  : launch_roll<3, 1, 0, RE_BNRED, SP_NONE, H>(a, lds, grid, s);
      if (d->prologue) return relu ? launch_roll<3, 1, 1, RE_RELU, SP_NONE, H>(a, lds, grid, s) : launch_roll<3, 1, 1, 0, SP_NONE, H>(a, lds, grid, s);
      if (wr)
        return relu ? launch_roll<3, 1, 0, RE_RELU, SP_NONE, H, 1>(a, lds, grid, s)
                    : launch_roll<3, 1, 0, 0, SP_NONE, H, 1>(a, lds, grid, s);
      return relu ? launch_roll<3, 1, 0, RE_RELU, SP_NONE, H>(a, lds, grid, s) : launch_roll<3, 1, 0, 0, SP_NONE, H>(a, lds, grid, s);
    }
    // 2-D forms of the EDSR body and its backward: plain, ReLU, residual,
    // ReLU mask, residual + accumulate; DUF's tail conv (1,3,3) 256 -> 256
    // with the BN+ReLU prologue (duf_net.py:116-118); DRF's sub-pixel
    // projections: plain, PReLU, accumulate over a shuffled input or output
    if (d->prologue) {
      if (sp != SP_NONE || em != 0) return (int)VSRK_ERR_UNSUPPORTED;
      return launch_roll<1, 2, 1, 0, SP_NONE, H>(a, lds, grid, s);
    }
    if (sp == SP_X) {
      switch (em) {
        case 0: return launch_roll<1, 2, 0, 0, SP_X, H>(a, lds, grid, s);
        case RE_PRELU: return launch_roll<1, 2, 0, RE_PRELU, SP_X, H>(a, lds, grid, s);
        case RE_ACC: return launch_roll<1, 2, 0, RE_ACC, SP_X, H>(a, lds, grid, s);
        case RE_PMASK: return launch_roll<1, 2, 0, RE_PMASK, SP_X, H>(a, lds, grid, s);
        case RE_PMASK | RE_ACC: return launch_roll<1, 2, 0, RE_PMASK | RE_ACC, SP_X, H>(a, lds, grid, s);
        default: return (int)VSRK_ERR_UNSUPPORTED;
      }
    }
    if (sp == SP_Y) {
      switch (em) {
        case 0: return launch_roll<1, 2, 0, 0, SP_Y, H>(a, lds, grid, s);
        case RE_PRELU: return launch_roll<1, 2, 0, RE_PRELU, SP_Y, H>(a, lds, grid, s);
        case RE_ACC: return launch_roll<1, 2, 0, RE_ACC, SP_Y, H>(a, lds, grid, s);
        case RE_PMASK: return launch_roll<1, 2, 0, RE_PMASK, SP_Y, H>(a, lds, grid, s);
        case RE_PMASK | RE_ACC: return launch_roll<1, 2, 0, RE_PMASK | RE_ACC, SP_Y, H>(a, lds, grid, s);
        default: return (int)VSRK_ERR_UNSUPPORTED;
      }
    }
    if (wr) {
      switch (em) {
        case 0: return launch_roll<1, 2, 0, 0, SP_NONE, H, 1>(a, lds, grid, s);
        case RE_RELU: return launch_roll<1, 2, 0, RE_RELU, SP_NONE, H, 1>(a, lds, grid, s);
        case RE_RES | RE_ACC: return launch_roll<1, 2, 0, RE_RES | RE_ACC, SP_NONE, H, 1>(a, lds, grid, s);
        case RE_PMASK: return launch_roll<1, 2, 0, RE_PMASK, SP_NONE, H, 1>(a, lds, grid, s);
        default: return (int)VSRK_ERR_UNSUPPORTED;
      }
    }
    switch (em) {
      case 0: return launch_roll<1, 2, 0, 0, SP_NONE, H>(a, lds, grid, s);
      case RE_RELU: return launch_roll<1, 2, 0, RE_RELU, SP_NONE, H>(a, lds, grid, s);
      case RE_RES: return launch_roll<1, 2, 0, RE_RES, SP_NONE, H>(a, lds, grid, s);
      case RE_RES | RE_SUMACT: return launch_roll<1, 2, 0, RE_RES | RE_SUMACT, SP_NONE, H>(a, lds, grid, s);
      case RE_MASK: return launch_roll<1, 2, 0, RE_MASK, SP_NONE, H>(a, lds, grid, s);
      case RE_RES | RE_ACC: return launch_roll<1, 2, 0, RE_RES | RE_ACC, SP_NONE, H>(a, lds, grid, s);
      case RE_PMASK: return launch_roll<1, 2, 0, RE_PMASK, SP_NONE, H>(a, lds, grid, s);
      default: return (int)VSRK_ERR_UNSUPPORTED;
    }
  });
  if (rc == VSRK_ERR_UNSUPPORTED) return 0;
  return rc == VSRK_OK ? 1 : -rc;
}

#ifdef ROLL_STAMP
extern "C" int vsrk_roll_stamps(unsigned* dst) {
  return hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_roll_stamp), sizeof(g_roll_stamp)) == hipSuccess ? 0 : 1;
}
#endif

extern "C" size_t vsrk_conv_prelu_bwd_workspace(void) {
  return std::max(vsrk_roll_slope_ws_bytes(), vsrk_pw_pbwd_ws_bytes());
}

extern "C" int vsrk_conv_fwd_prelu_bwd(const vsrk_conv_desc* d, const vsrk_tensor5* x, const void* w_packed,
                                       const float* bias, const vsrk_tensor5* y_fwd, const vsrk_tensor5* y,
                                       int32_t c_lo, float* da, int32_t accumulate_da, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  VSRK_CHECK(d && x && y && y_fwd && w_packed && d->mask_slope, "conv_fwd_prelu_bwd: null argument");
  VSRK_CHECK(workspace && workspace_bytes >= vsrk_conv_prelu_bwd_workspace(),
             "conv_fwd_prelu_bwd: workspace %zu < %zu bytes", workspace_bytes, vsrk_conv_prelu_bwd_workspace());
  VSRK_CHECK(((uintptr_t)workspace & 15) == 0, "conv_fwd_prelu_bwd: workspace must be 16-byte aligned");
  VSRK_CHECK(c_lo >= 0 && c_lo < y->c, "conv_fwd_prelu_bwd: c_lo %d outside [0, %d)", c_lo, y->c);
  hipStream_t s = (hipStream_t)stream;
  if ((int64_t)y->n * y->d * y->h * y->w == 0) {  // nothing to launch: no slope gradient
    if (da && !accumulate_da) {
      const hipError_t e = hipMemsetAsync(da, 0, sizeof(float), s);
      if (e != hipSuccess) {
        vsrk_set_error("conv_fwd_prelu_bwd: clearing the slope gradient failed: %s", hipGetErrorString(e));
        return VSRK_ERR_LAUNCH;
      }
    }
    return VSRK_OK;
  }
  int nparts = 0;
  const vsrk_slope_out so{(double*)workspace, workspace_bytes / sizeof(double), &nparts};
  int rc;
  if (d->kd == 1 && d->kh == 1 && d->kw == 1) {
    // pointwise: the staged kernel's post-accumulate form, any channel tail
    if (bias) return VSRK_ERR_UNSUPPORTED;
    rc = vsrk_conv_fwd_pw_pbwd(d, x, w_packed, y_fwd, y, c_lo, &so, s);
  } else {
    if (c_lo != 0) return VSRK_ERR_UNSUPPORTED;  // the rolling kernel masks every output channel
    rc = vsrk_conv_fwd_roll(d, x, w_packed, bias, nullptr, nullptr, nullptr, y_fwd, y, s, &so);
  }
  if (rc == 0) return VSRK_ERR_UNSUPPORTED;
  if (rc < 0) return -rc;
  if (da) {  // (da == NULL: the partials stay in the workspace slot, vsrk_slope_final_sum later)
    vsrk_slope_final((const double*)workspace, nparts, d->mask_slope, da, accumulate_da, 0, s);
    VSRK_LAUNCH_CHECK("conv_fwd_prelu_bwd_final");
  }
  return VSRK_OK;
}

int vsrk_roll_bnred_final(const vsrk_roll_bnred& r, int cout, float* sum_dy, float* sum_dy_xhat, hipStream_t s) {
  roll_bnred_final_kernel<<<cout, 256, 0, s>>>(r.ws, r.ntiles, r.ntn, cout, r.invstd, sum_dy, sum_dy_xhat);
  VSRK_LAUNCH_CHECK("conv_fwd_reduce(roll) final");
  return VSRK_OK;
}

size_t vsrk_roll_bnred_ws_floats(const vsrk_tensor5* y) {  // every depth its own tile run (an upper bound)
  return (size_t)y->n * ceil_div(y->h, RFTH) * ceil_div(y->w, TW) * ceil_div(y->c, 32) * std::max(y->d, 1) * RNW * 64;
}
