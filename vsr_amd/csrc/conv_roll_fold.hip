// The depth-folded rolling forward: conv_roll_impl.h's kernel built with
// 32-row tiles (8 waves x 4 rows) in the (kd, channel)-chunk form SP_FOLD, for
// a Conv3d 3x3x3 with one output depth from three input slices (DUF's last
// dense unit, duf_net.py:214), and its host entry.  A translation unit of its
// own: the tile height is a build constant of the rolling kernel, and the
// 3-D / 2-D forms (conv_roll.hip) keep 16 rows.
#define ROLL_RMS 4
#include "conv_roll_impl.h"

// DUF's last unit is Conv3d(224, 32, 3, padding
// (0, 1, 1)) over three input slices into one output depth (duf_net.py:214):
// a rolling walk finds one kd tap per staged slice, so its stage carried a
// third of the 3-D form's MFMAs beside the same 47 DMA pieces (and 27 B
// fragment reads) -- it ran on conv_fast at ~0.22 of peak.  Folded, it is a
// 3x3 conv over 3 x cin (kd, channel) chunks with one 32-channel output
// block: a stage stages 37 A pieces (34 x 34 halo voxels of 16 channels) and
// the 9 B pieces of its depth tap, and each wave runs 9 taps x 4 rows = 36
// MFMAs per stage (18 in the 3-D form's one-bank stages).
// 1 = launched, 0 = not eligible, < 0 = -(error status)
int vsrk_conv_fwd_roll_fold(const vsrk_conv_desc* d, const vsrk_tensor5* x, const void* w_packed, const float* bias,
                            const float* pro_scale, const float* pro_shift, const vsrk_tensor5* y, hipStream_t s) {
  if (d->kd != 3 || d->kh != 3 || d->kw != 3 || d->pd != 0 || x->d != 3 || y->d != 1) return 0;
  if (!vsrk_is16(x->dtype) || y->dtype != x->dtype || x->shuffle > 1 || y->shuffle > 1) return 0;
  if (d->act != VSRK_ACT_NONE && d->act != VSRK_ACT_RELU) return 0;
  if (d->accumulate || d->mask_slope || d->bias_perm_r > 1) return 0;
  if (x->c % RCH != 0 || 3 * (x->c / RCH) > RMAXSUB || !chunk_ok(x, 2)) return 0;
  if (y->c % 32 != 0 || ((uintptr_t)y->ptr) % 16 != 0 || y->sn % 8 || y->sh % 8 || y->sw % 8) return 0;
  if (d->ph < 0 || d->ph > 2 || d->pw < 0 || d->pw > 2) return 0;
  if (y->h != x->h + 2 * d->ph - 2 || y->w != x->w + 2 * d->pw - 2 || y->n != x->n) return 0;
  for (const vsrk_tensor5* t : {x, y}) {  // every element offset fits in 32 bits
    const int64_t span = (int64_t)(t->n - 1) * t->sn + (int64_t)(t->d - 1) * t->sd +
                         (int64_t)(t->h + RFTH + 2) * t->sh + (int64_t)(t->w + 2 * RHW) * t->sw + t->c;
    if (span >= (1ll << 31) || t->sn < 0 || t->sd < 0 || t->sh < 0 || t->sw < 0) return 0;
  }
  RollArgs a;
  a.x.ptr = (char*)x->ptr;
  a.x.d = 1; a.x.h = x->h; a.x.w = x->w;
  a.x.sn = (int)x->sn; a.x.sd = (int)x->sd; a.x.sh = (int)x->sh; a.x.sw = (int)x->sw;
  a.y.ptr = (char*)y->ptr;
  a.y.d = 1; a.y.h = y->h; a.y.w = y->w;
  a.y.sn = (int)y->sn; a.y.sd = (int)y->sd; a.y.sh = (int)y->sh; a.y.sw = (int)y->sw;
  a.res = a.y;
  a.msk = a.y;
  a.w = w_packed;
  a.bias = bias;
  a.bias_r = 1;
  a.pro_scale = pro_scale;
  a.pro_shift = pro_shift;
  a.cin = 3 * x->c;
  a.cout = y->c;
  a.cin_pad = round_up(x->c, 32);  // of the packed weights
  a.cout_pad = round_up(y->c, 128);
  a.pd = 0;
  a.ph = d->ph;
  a.pw = d->pw;
  a.prologue = d->prologue;
  a.out_scale = d->out_scale;
  const int nc = x->c / RCH;
  a.nchunk = 3 * nc;
  a.fold_nc = nc;
  a.fold_wstride = 9 * a.cout_pad * a.cin_pad;
  a.fold_tab = 3 * x->c;
  a.fold_cin = x->c;
  a.act_param = nullptr;
  a.prio = 0;
  a.mask_slope = nullptr;
  a.slope_part = nullptr;
  for (int i = 0; i < a.nchunk; ++i) {
    const int kd = i / nc;
    a.spoff[i] = (int)(kd * x->sd + (i - kd * nc) * RCH);
    a.sptap[i] = (uint16_t)kd;
  }
  const int tiles_h = ceil_div(y->h, RFTH), tiles_w = ceil_div(y->w, TW), ntn = ceil_div(y->c, 32);
  const int64_t ntiles = (int64_t)y->n * tiles_h * tiles_w * ntn;
  if (ntiles == 0) return 1;
  VSRK_CHECK(ntiles < (1ll << 31), "conv_fwd(roll fold): too many tiles");
  a.dzc = 1;
  a.ntn = make_rdiv(ntn);
  a.nzc = make_rdiv(1);
  a.tiles_w = make_rdiv(tiles_w);
  a.tiles_h = make_rdiv(tiles_h);
  a.ntiles = (int)ntiles;
  using G = RollGeo<1, 1>;
  const size_t tables = (size_t)a.cout_pad * 4 + (d->prologue ? 2 * (size_t)a.fold_tab * 4 : 0);
  const size_t lds = (size_t)RNSLOT * G::SLOT + tables;
  if (lds > 160 * 1024) return 0;
  const int grid = (int)vsrk_capped_grid(std::min<int64_t>(ntiles, vsrk_num_cus()));
  const bool relu = d->act == VSRK_ACT_RELU;
  int rc = vsrk_dispatch16(x->dtype, [&](auto tag) {
    using H = decltype(tag);
    if (d->prologue)
      return relu ? launch_roll<1, 1, 1, RE_RELU, SP_FOLD, H>(a, lds, grid, s) : launch_roll<1, 1, 1, 0, SP_FOLD, H>(a, lds, grid, s);
    return relu ? launch_roll<1, 1, 0, RE_RELU, SP_FOLD, H>(a, lds, grid, s) : launch_roll<1, 1, 0, 0, SP_FOLD, H>(a, lds, grid, s);
  });
  if (rc == VSRK_ERR_UNSUPPORTED) return 0;
  return rc == VSRK_OK ? 1 : -rc;
}
