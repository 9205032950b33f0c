// Implicit-GEMM convolution weight/bias gradient on CDNA4 MFMA (gfx950).
// Design notes: conv_fwd.hip (layout) and the comment block below.  This unit
// holds the generic kernel, its plan and the entry point, which routes between
// the family's candidates (conv_wgrad.h); the reduce is conv_wgrad_reduce.hip.
#include "conv_wgrad.h"

namespace {
using namespace vsrk_conv;

// ---------------------------------------------------------------------------
// weight gradient
// ---------------------------------------------------------------------------
// dW[tap][co][ci] = sum_m dY[m][co] * X[m + tap][ci]: the voxel index m is the
// MFMA k dimension.  A workgroup owns a (32*NCO output x 32*NCI input channel,
// kd tap) combo and a run of 8x32-voxel tiles (split-K over voxels).  Per tile
// it stages dY (NCO planes of 32 channels) and the input halo (NCI planes,
// prologue applied) into LDS once and its 8 waves = NCO x NCI channel blocks x
// NV voxel parts run all kh*kw taps; both operands are read transposed with
// ds_read_b64_tr_b16 (64-byte plane rows: conflict-free).  The next tile's
// loads are in flight during the current tile's MFMAs.  Wave partials are
// summed through LDS in a fixed order into one fp32 slab per (split, combo);
// combos at (ci chunk 0, kd = kd_bias) also produce dbias partials from the
// staged dY.  wgrad_reduce sums slabs in split order: deterministic.
template <typename T, int NCO, int NCI, int KK, bool VEC>
__global__ __attribute__((amdgpu_waves_per_eu(1, 1))) __launch_bounds__(GTHR) void conv_wgrad_kernel(WgradArgs a) {
  constexpr int E = Chunk<T>::E;
  constexpr int PB = 32 * (int)sizeof(T);  // plane row bytes: 32 channels
  constexpr int CPP = PB / 16;             // 16-byte chunks per plane row
  constexpr int NV = 4 / (NCO * NCI);      // voxel parts (waves sharing a channel block)
  constexpr int VOX = GTH * TW;
  constexpr int VPW = VOX / NV;            // voxels per wave
  constexpr int YCPV = NCO * CPP;          // dY chunks per voxel
  constexpr int XCPV = NCI * CPP;          // X chunks per slot
  constexpr int HWd = TW + KK - 1;
  constexpr int SLOTS = (GTH + KK - 1) * HWd;
  constexpr int TAPS = KK * KK;
  constexpr int MAXY = (VOX * YCPV) / GTHR;
  constexpr int MAXX = (SLOTS * XCPV + GTHR - 1) / GTHR;
  extern __shared__ __attribute__((aligned(16))) char lds[];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int cis = wave % NCI, cos_ = (wave / NCI) % NCO, vp = wave / (NCI * NCO);
  char* ldsY = lds;                          // [NCO][VOX][PB]
  char* ldsX = lds + NCO * VOX * PB;         // [NCI][SLOTS][PB]
  float* lsc = reinterpret_cast<float*>(ldsX + NCI * SLOTS * PB);
  float* lsh = lsc + a.cin_pad;

  const int L = xcd_remap(blockIdx.x, a.nblk);
  const int split = L / a.ncombos;
  int combo = L - split * a.ncombos;
  const int cot = combo % a.n_co_tiles;
  combo /= a.n_co_tiles;
  const int cic = combo % a.n_ci_chunks;
  const int kdi = combo / a.n_ci_chunks;
  const int co0 = cot * 32 * NCO, ci0 = cic * 32 * NCI;
  const bool do_bias = a.want_bias && cic == 0 && kdi == a.kd_bias;
  const bool relu_in = (a.prologue & VSRK_PRO_RELU) != 0;
  if (a.prologue) {
    stage_prologue(lsc, lsh, a.prologue, a.pro_scale, a.pro_shift, a.cin, a.cin_pad, tid, GTHR);
    __syncthreads();
  }

  // fixed per-thread chunk roles (GTHR is a multiple of YCPV and XCPV)
  const int yrem = tid % YCPV, xrem = tid % XCPV;
  const int yc = co0 + (yrem / CPP) * 32 + (yrem % CPP) * E;  // dY channel of every y chunk
  const int xc = ci0 + (xrem / CPP) * 32 + (xrem % CPP) * E;  // X channel of every x chunk
  const int ydst = (yrem / CPP) * VOX * PB + (yrem % CPP) * 16;
  const int xdst = (xrem / CPP) * SLOTS * PB + (xrem % CPP) * 16;
  const bool yc_ok = yc < a.cout, xc_ok = xc < a.cin;
  const int ycc = yc_ok ? yc : 0, xcc = xc_ok ? xc : 0;

  uint4 ry[MAXY], rx[MAXX];
  unsigned ymask = 0, xmask = 0;  // validity of the chunks in flight
  float bsum[E];
#pragma unroll
  for (int e = 0; e < E; ++e) bsum[e] = 0.f;

  auto tile_ok = [&](int t) __attribute__((always_inline)) {
    const int dz = (t / (a.tiles_w * a.tiles_h)) % a.dy.d;
    const int di = dz + kdi - a.pd;
    return di >= 0 && di < a.x.d;
  };
  auto issue = [&](int t) __attribute__((always_inline)) {
    int b = t;
    const int tw_i = b % a.tiles_w;
    b /= a.tiles_w;
    const int th_i = b % a.tiles_h;
    b /= a.tiles_h;
    const int dz = b % a.dy.d;
    const int nb = b / a.dy.d;
    const int di = dz + kdi - a.pd;
    const int h0 = th_i * GTH, w0 = tw_i * TW;
    ymask = 0;
    xmask = 0;
#pragma unroll
    for (int i = 0; i < MAXY; ++i) {
      const int vox = (tid + i * GTHR) / YCPV;
      const int ho = h0 + vox / TW, wo = w0 + (vox % TW);
      const bool ok = ho < a.dy.h && wo < a.dy.w && yc_ok;
      ymask |= (ok ? 1u : 0u) << i;
      if constexpr (VEC) {
        ry[i] = *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(a.dy.ptr) +
                                                view_off(a.dy, nb, dz, ok ? ho : 0, ok ? wo : 0, ycc));
      } else {
        ry[i] = ok ? load_raw<T>(a.dy, nb, dz, ho, wo, yc, a.cout, false) : make_uint4(0, 0, 0, 0);
      }
    }
#pragma unroll
    for (int i = 0; i < MAXX; ++i) {
      const int slot = (tid + i * GTHR) / XCPV;
      const int hh = slot / HWd, ww = slot - hh * HWd;
      const int hi = h0 + hh - a.ph, wi = w0 + ww - a.pw;
      const bool ok = slot < SLOTS && hi >= 0 && hi < a.x.h && wi >= 0 && wi < a.x.w && xc_ok;
      xmask |= (ok ? 1u : 0u) << i;
      if constexpr (VEC) {
        rx[i] = *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(a.x.ptr) +
                                                view_off(a.x, nb, di, ok ? hi : 0, ok ? wi : 0, xcc));
      } else {
        rx[i] = ok ? load_raw<T>(a.x, nb, di, hi, wi, xc, a.cin, false) : make_uint4(0, 0, 0, 0);
      }
    }
  };
  auto commit = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < MAXY; ++i) {
      const int vox = (tid + i * GTHR) / YCPV;
      const uint4 v = ((ymask >> i) & 1) ? ry[i] : make_uint4(0, 0, 0, 0);
      *reinterpret_cast<uint4*>(ldsY + ydst + vox * PB) = v;
      if (do_bias) {
        float f[E];
        Chunk<T>::unpack(v, f);
#pragma unroll
        for (int e = 0; e < E; ++e) bsum[e] += f[e];
      }
    }
#pragma unroll
    for (int i = 0; i < MAXX; ++i) {
      const int slot = (tid + i * GTHR) / XCPV;
      if (slot < SLOTS) {
        uint4 v = rx[i];
        if (a.prologue) v = prologue_lds<T>(v, xc, relu_in, lsc, lsh);
        if (!((xmask >> i) & 1)) v = make_uint4(0, 0, 0, 0);
        *reinterpret_cast<uint4*>(ldsX + xdst + slot * PB) = v;
      }
    }
  };

  f32x16 acc[TAPS];
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;

  const int t_begin = split * a.tiles_per_split;
  const int t_end = min(a.ntiles, t_begin + a.tiles_per_split);
  int t = t_begin;
  while (t < t_end && !tile_ok(t)) ++t;
  if (t < t_end) {
    issue(t);
    commit();
    __syncthreads();
  }
  const char* py = ldsY + cos_ * VOX * PB;
  const char* px = ldsX + cis * SLOTS * PB;
  while (t < t_end) {
    int tn = t + 1;
    while (tn < t_end && !tile_ok(tn)) ++tn;
    if (tn < t_end) issue(tn);
    if constexpr (sizeof(T) == 2) {
      // Group g = lane>>4 reads a 4-row x 16-column block; lane 4q+p
      // addresses row q, columns 4p..4p+3, and receives column lane&15.
      const int g = lane >> 4, i16 = lane & 15, q = i16 >> 2, p = i16 & 3;
      const int hfk = g >> 1, colb = ((g & 1) * 16 + 4 * p) * 2;
#pragma unroll
      for (int ks = 0; ks < VPW / 16; ++ks) {
        const int vb = vp * VPW + ks * 16;
        const int vrow = vb / TW, vcol0 = (vb % TW) + 8 * hfk;
        v4i16 y0 = ds_read_tr(py + (vrow * TW + vcol0 + q) * PB + colb);
        v4i16 y1 = ds_read_tr(py + (vrow * TW + vcol0 + 4 + q) * PB + colb);
        const uint4 af = __builtin_bit_cast(uint4, __builtin_shufflevector(y0, y1, 0, 1, 2, 3, 4, 5, 6, 7));
#pragma unroll
        for (int khi = 0; khi < KK; ++khi) {
#pragma unroll
          for (int kwi = 0; kwi < KK; ++kwi) {
            const char* xs = px + ((vrow + khi) * HWd + vcol0 + kwi + q) * PB + colb;
            v4i16 x0 = ds_read_tr(xs);
            v4i16 x1 = ds_read_tr(xs + 4 * PB);
            const uint4 bfr = __builtin_bit_cast(uint4, __builtin_shufflevector(x0, x1, 0, 1, 2, 3, 4, 5, 6, 7));
            mma<T>(acc[khi * KK + kwi], af, bfr);
          }
        }
      }
    } else {
      // fp32: 32x32x2, lane l: A[co=l&31][k=l>>5], B[k=l>>5][ci=l&31]
      const int r = lane & 31, hfk = lane >> 5;
      for (int kk = 0; kk < VPW; kk += 2) {
        const int vox = vp * VPW + kk + hfk;
        const int vrow = vox / TW, vcol = vox % TW;
        const float av = *reinterpret_cast<const float*>(py + vox * PB + r * 4);
#pragma unroll
        for (int khi = 0; khi < KK; ++khi) {
#pragma unroll
          for (int kwi = 0; kwi < KK; ++kwi) {
            const int sl = (vrow + khi) * HWd + vcol + kwi;
            const float bv = *reinterpret_cast<const float*>(px + sl * PB + r * 4);
            acc[khi * KK + kwi] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[khi * KK + kwi], 0, 0, 0);
          }
        }
      }
    }
    if (tn < t_end) {
      __syncthreads();
      commit();
      __syncthreads();
    }
    t = tn;
  }

  // slab layout: [tap][co (32*NCO)][ci (32*NCI)] then dbias[32*NCO]
  float* out = a.ws + (int64_t)L * a.slab;
  constexpr int NW = TAPS * 1024 * NCO * NCI;
  const int r = lane & 31, hfo = lane >> 5;
  if constexpr (NV == 1) {
#pragma unroll
    for (int tap = 0; tap < TAPS; ++tap) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int co = cos_ * 32 + (i & 3) + 8 * (i >> 2) + 4 * hfo;
        out[(tap * 32 * NCO + co) * (32 * NCI) + cis * 32 + r] = acc[tap][i];
      }
    }
  } else {
    // fixed-order sum of the NV voxel-part partials: red[cos][cis][tap][co][ci]
    __syncthreads();
    float* red = reinterpret_cast<float*>(lds);
    for (int v = 0; v < NV; ++v) {
      if (vp == v) {
#pragma unroll
        for (int tap = 0; tap < TAPS; ++tap) {
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int co = (i & 3) + 8 * (i >> 2) + 4 * hfo;
            float* dst = red + (((cos_ * NCI + cis) * TAPS + tap) * 32 + co) * 32 + r;
            *dst = (v == 0) ? acc[tap][i] : *dst + acc[tap][i];
          }
        }
      }
      __syncthreads();
    }
    for (int i = tid; i < NW; i += GTHR) {
      const int ci = i % (32 * NCI);
      const int t2 = i / (32 * NCI);
      const int co = t2 % (32 * NCO);
      const int tap = t2 / (32 * NCO);
      out[i] = red[((((co / 32) * NCI + ci / 32) * TAPS + tap) * 32 + (co % 32)) * 32 + (ci % 32)];
    }
  }
  if (do_bias) {
    __syncthreads();
    float* red = reinterpret_cast<float*>(lds);
#pragma unroll
    for (int e = 0; e < E; ++e) red[tid * E + e] = bsum[e];
    __syncthreads();
    if (tid < 32 * NCO) {
      const int plane = tid / 32, within = tid % 32;
      const int grp = plane * CPP + within / E, e = within % E;
      float sacc = 0.f;
      for (int kk = grp; kk < GTHR; kk += YCPV) sacc += red[kk * E + e];
      out[NW + tid] = sacc;
    }
  }
}

// VSRK_WGRAD_TARGET=<workgroups> (at least 64) overrides wgrad_plan's split rule (A/B, read at load); unset or 0: the rule
const int g_wgrad_target_env = vsrk_env_int("VSRK_WGRAD_TARGET", 0);
const int g_wgrad_target = g_wgrad_target_env ? std::max(64, g_wgrad_target_env) : 0;

template <typename T, int NCO, int NCI, int KK, bool VEC>
void launch_wgrad(const WgradArgs& a, hipStream_t s) {
  constexpr int PB = 32 * (int)sizeof(T);
  constexpr int SLOTS = (GTH + KK - 1) * (TW + KK - 1);
  const size_t stage = (size_t)(NCO * GTH * TW + NCI * SLOTS) * PB + (a.prologue ? 2 * a.cin_pad * 4 : 0);
  const size_t red = (4 / (NCO * NCI)) > 1 ? (size_t)NCO * NCI * KK * KK * 1024 * sizeof(float) : 0;
  const size_t bias = (size_t)GTHR * (16 / sizeof(T)) * sizeof(float);
  const size_t lds = std::max(stage, std::max(red, bias));
  auto kern = conv_wgrad_kernel<T, NCO, NCI, KK, VEC>;
  (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  kern<<<a.nblk, GTHR, lds, s>>>(a);
}

template <typename T, int NCO, int NCI>
void wgrad_k(const WgradArgs& a, bool vec, hipStream_t s) {
  if (a.kh == 1) {
    if (vec) launch_wgrad<T, NCO, NCI, 1, true>(a, s); else launch_wgrad<T, NCO, NCI, 1, false>(a, s);
  } else {
    if (vec) launch_wgrad<T, NCO, NCI, 3, true>(a, s); else launch_wgrad<T, NCO, NCI, 3, false>(a, s);
  }
}

// The generic plan: the thin, pipelined and generic kernels run on it.
struct WgradPlan {
  int nco, nci;  // channel blocks per workgroup (x32)
  int ncombos, ntiles, tps;
  WgradSlabs slabs;
};

WgradPlan wgrad_plan(const vsrk_conv_desc* d, const vsrk_tensor5* x, const vsrk_tensor5* dy) {
  WgradPlan p;
  WgradSlabs& sl = p.slabs;
  const bool f32 = x->dtype == VSRK_F32;
  p.nco = (!f32 && dy->c > 32) ? 2 : 1;
  p.nci = (!f32 && x->c > 32) ? 2 : 1;
  sl.nco_t = ceil_div(dy->c, 32 * p.nco);
  sl.nci_t = ceil_div(x->c, 32 * p.nci);
  p.ncombos = sl.nco_t * sl.nci_t * d->kd;
  p.ntiles = dy->n * dy->d * ceil_div(dy->h, GTH) * ceil_div(dy->w, TW);
  // Splits (workgroups per combo): about 512 workgroups (two resident per
  // CU), but no fewer than 16 tiles (of 8x32 voxels) per workgroup while that
  // still leaves one workgroup per CU: each workgroup writes a whole fp32 slab
  // and the reduce reads it back, which at 8 tiles per workgroup cost the
  // EDSR 64->64 wgrad 10 % (147 -> 133 us at 256 workgroups; DUF's 3x3x3,
  // at 24 tiles per workgroup, keeps its 512: 231 vs 324 us at 256).
  // VSRK_WGRAD_TARGET=<workgroups> overrides the rule (A/B only).
  const int target = g_wgrad_target;
  // 3-D (kd > 1): about 64 tiles per workgroup (at least one workgroup per
  // CU).  The pipelined kernel's sweep (profiles/r2_wgrad_pipe_ab.txt): DUF
  // 64->32 at 64 x 7 x 128 x 128 fastest at ~1024 workgroups (~84 tiles
  // each), 224->32 at ~4096 (~60 tiles each); the 2-D EDSR 64->64 is fastest
  // at 512.
  int want;
  if (target) want = ceil_div(target, p.ncombos);
  else if (d->kd > 1) want = std::max(ceil_div(p.ntiles, 64), ceil_div(256, p.ncombos));
  else want = std::min(ceil_div(512, p.ncombos), std::max(ceil_div(p.ntiles, 16), ceil_div(256, p.ncombos)));
  if (vsrk_g_grid_cap > 0) want = std::max(1, vsrk_g_grid_cap / p.ncombos);
  want = std::max(1, std::min(want, p.ntiles));
  p.tps = ceil_div(p.ntiles, want);
  // the kernels' slabs (the end of conv_wgrad_kernel): split-major, one per
  // (split, combo) of 32 * nco x 32 * nci channels and a kd tap
  sl.nsplit = ceil_div(p.ntiles, p.tps);
  sl.slab = d->kh * d->kw * 1024 * p.nco * p.nci + 32 * p.nco;
  sl.kd = d->kd; sl.kh = d->kh; sl.kw = d->kw;
  sl.cot_w = 32 * p.nco; sl.cit_w = 32 * p.nci;
  sl.kd_bias = std::min(d->pd, d->kd - 1);
  sl.rows_ok = true;
  return p;
}

// Launches the plan's slab kernel: thin, else pipelined, else generic.
int wgrad_generic(const vsrk_conv_desc* d, const vsrk_tensor5* x, const vsrk_tensor5* dy, const float* pro_scale,
                  const float* pro_shift, int perm_r, bool want_bias, float* ws, const WgradPlan& p, hipStream_t s) {
  const int es = vsrk_esize(x->dtype);
  WgradArgs a;
  a.x = make_view(x);
  a.dy = make_view(dy);
  a.pro_scale = pro_scale;
  a.pro_shift = pro_shift;
  a.ws = ws;
  a.cin = x->c;
  a.cout = dy->c;
  a.kd = d->kd; a.kh = d->kh; a.kw = d->kw;
  a.pd = d->pd; a.ph = d->ph; a.pw = d->pw;
  a.prologue = d->prologue;
  a.xvec = chunk_ok(x, es);
  a.dyvec = chunk_ok(dy, es);
  a.tiles_h = ceil_div(dy->h, GTH);
  a.tiles_w = ceil_div(dy->w, TW);
  a.ntiles = p.ntiles;
  a.tiles_per_split = p.tps;
  a.nsplit = p.slabs.nsplit;
  a.ncombos = p.ncombos;
  a.nblk = p.slabs.nsplit * p.ncombos;
  a.n_ci_chunks = p.slabs.nci_t;
  a.n_co_tiles = p.slabs.nco_t;
  a.kd_bias = p.slabs.kd_bias;
  a.slab = p.slabs.slab;
  a.want_bias = want_bias;
  a.cin_pad = round_up(x->c, 32 * p.nci);
  a.sp_by = 0;
  if (d->subpixel && d->kd == 1 && d->kh == 3 && d->kw == 3 && ((x->shuffle > 1) != (dy->shuffle > 1))) {
    const vsrk_tensor5* t = dy->shuffle > 1 ? dy : x;
    const int r = t->shuffle, cph = t->c / (r * r);
    if (cph % 32 == 0 && t->c / 32 <= 64) {
      a.sp_by = dy->shuffle > 1 ? 1 : 2;
      const int32_t code = d->subpixel & ~(1 << 25);  // gradients of the forward (unflipped) taps
      for (int b = 0; b < t->c / 32; ++b) a.sptap[b] = subpixel_tapmask(code, r, b * 32 / cph);
    }
  }
  const bool vec = a.xvec && a.dyvec;
  if (vsrk_is16(x->dtype) && vsrk_conv_wgrad_thin(a, p.nco, p.nci, perm_r, x->dtype, s)) {
    // thin-channel kernel (conv_thin.hip)
  } else if (vsrk_is16(x->dtype) && vsrk_conv_wgrad_pipe(a, p.nco, p.nci, x->dtype, s)) {
    // two-stage pipelined kernel (conv_wgrad_pipe.hip)
  } else if (vsrk_is16(x->dtype)) {
    vsrk_dispatch16(x->dtype, [&](auto tag) {
      using H = decltype(tag);
      if (p.nco == 2 && p.nci == 2) wgrad_k<H, 2, 2>(a, vec, s);
      else if (p.nco == 2) wgrad_k<H, 2, 1>(a, vec, s);
      else if (p.nci == 2) wgrad_k<H, 1, 2>(a, vec, s);
      else wgrad_k<H, 1, 1>(a, vec, s);
      return 0;
    });
  } else {
    wgrad_k<float, 1, 1>(a, vec, s);
  }
  VSRK_LAUNCH_CHECK("conv_wgrad");
  return VSRK_OK;
}

// Views spanning more than the rolling weight gradient's 32-bit element
// offsets (DUF's concat buffer at cfg 5) run in sample chunks that fit: the
// chunk's sample count, 0 when no split applies
int wgrad_roll_chunk(const vsrk_tensor5* x, const vsrk_tensor5* dy) {
  auto fits = [&](int64_t n) {
    for (const vsrk_tensor5* t : {x, dy})
      if (n * t->sn + (int64_t)t->d * t->sd + (int64_t)(t->h + 64) * t->sh + (int64_t)(t->w + 64) * t->sw + t->c >=
          (1ll << 31))
        return false;
    return true;
  };
  if (x->n <= 1 || x->n != dy->n || x->sn < 0 || dy->sn < 0 || fits(x->n)) return 0;
  int nc = x->n;
  while (nc > 1 && !fits(nc)) nc = (nc + 1) / 2;
  return fits(nc) ? nc : 0;
}

// The candidates, in routing order.  Each answers a request with "not
// eligible" or a plan; the answer never depends on the workspace.
enum WgradKind { WG_PW, WG_ROLL, WG_ROLL_CHUNKS, WG_ROW, WG_GENERIC, WG_COUNT };
struct WgradCand {
  size_t ws_bytes;
  int chunk_n;        // WG_ROLL_CHUNKS: samples per chunk
  VsrkRollPlan roll;  // WG_ROLL; WG_ROLL_CHUNKS: the plan of a full chunk
  VsrkRowPlan row;
  WgradPlan gen;
};

bool wgrad_candidate(int kind, const vsrk_conv_desc* d, const vsrk_tensor5* x, const vsrk_tensor5* dy, WgradCand* c) {
  switch (kind) {
    case WG_PW:  // (its own slabs and reduce: conv_pw.hip)
      c->ws_bytes = vsrk_conv_wgrad_pw_workspace(d, x, dy);
      return c->ws_bytes != 0;
    case WG_ROLL:
      if (!vsrk_wgrad_roll_plan(d, x, dy, &c->roll)) return false;
      c->ws_bytes = c->roll.slabs.ws_bytes();
      return true;
    case WG_ROLL_CHUNKS: {  // only views the whole-view form refuses
      vsrk_tensor5 xc = *x, gc = *dy;
      xc.n = gc.n = c->chunk_n = wgrad_roll_chunk(x, dy);
      if (!c->chunk_n || vsrk_wgrad_roll_plan(d, x, dy, &c->roll) || !vsrk_wgrad_roll_plan(d, &xc, &gc, &c->roll))
        return false;
      c->ws_bytes = c->roll.slabs.ws_bytes();
      return true;
    }
    case WG_ROW:
      if (!vsrk_wgrad_row_plan(d, x, dy, &c->row)) return false;
      c->ws_bytes = c->row.slabs.ws_bytes();
      return true;
    default:  // WG_GENERIC: always eligible
      c->gen = wgrad_plan(d, x, dy);
      c->ws_bytes = c->gen.slabs.ws_bytes();
      return true;
  }
}

}  // namespace

extern "C" size_t vsrk_conv_wgrad_workspace_size(const vsrk_conv_desc* d, const vsrk_tensor5* x,
                                                 const vsrk_tensor5* dy) {
  size_t need = 0;
  WgradCand c;
  for (int kind = 0; kind < WG_COUNT; ++kind)
    if (wgrad_candidate(kind, d, x, dy, &c)) need = std::max(need, c.ws_bytes);
  return need;
}

extern "C" int vsrk_conv_wgrad(const vsrk_conv_desc* d, const vsrk_tensor5* x, const vsrk_tensor5* dy,
                               const float* pro_scale, const float* pro_shift, float dy_scale, int32_t perm_r,
                               float* dw, float* dbias, int32_t accumulate, void* workspace,
                               size_t workspace_bytes, void* stream) {
  VSRK_CHECK(d && x && dy && dw, "conv_wgrad: null argument");
  VSRK_CHECK(x->dtype == dy->dtype, "conv_wgrad: x/dy dtype mismatch");
  if (!view_ok(x, "conv_wgrad x") || !view_ok(dy, "conv_wgrad dy")) return VSRK_ERR_INVALID;
  VSRK_CHECK(d->kh == d->kw && (d->kh == 1 || d->kh == 3), "conv_wgrad: kh = kw in {1, 3}");
  VSRK_CHECK(!(d->prologue & VSRK_PRO_AFFINE) || (pro_scale && pro_shift), "conv_wgrad: affine prologue needs scale/shift");
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)workspace;
  // The first eligible candidate runs.  The pointwise kernel has no output
  // permutation; the rolling kernels want voxels and a workspace (without:
  // the generic path's checks).
  const bool rolling = workspace && dy->n * dy->d * dy->h * dy->w > 0;
  WgradCand c;
  int kind = WG_PW;
  for (;; ++kind) {
    if (kind == WG_PW && perm_r > 1) continue;
    if ((kind == WG_ROLL || kind == WG_ROLL_CHUNKS || kind == WG_ROW) && !rolling) continue;
    if (wgrad_candidate(kind, d, x, dy, &c)) break;  // WG_GENERIC always is
  }
  VSRK_CHECK(workspace && workspace_bytes >= c.ws_bytes, "conv_wgrad: workspace %zu < %zu bytes", workspace_bytes,
             c.ws_bytes);
  auto roll = [&](const vsrk_tensor5* xv, const vsrk_tensor5* gv, const VsrkRollPlan& p, int32_t acc) -> int {
    vsrk_conv_wgrad_roll(d, xv, gv, pro_scale, pro_shift, dbias != nullptr, ws, p, s);
    VSRK_LAUNCH_CHECK("conv_wgrad(roll)");
    return wgrad_reduce(p.slabs, ws, dy->c, x->c, perm_r, dy_scale, acc, dw, dbias, s);
  };
  switch (kind) {
    case WG_PW: {
      const int pw = vsrk_conv_wgrad_pw(d, x, dy, pro_scale, pro_shift, dy_scale, perm_r, dw, dbias, accumulate,
                                        workspace, workspace_bytes, s);
      VSRK_CHECK(pw != 0, "conv_wgrad(pw): planned but not launched");
      return pw > 0 ? VSRK_OK : -pw;
    }
    case WG_ROLL:
      return roll(x, dy, c.roll, accumulate);
    case WG_ROLL_CHUNKS:  // each chunk reduced onto dw after the first (fixed chunk order: deterministic)
      for (int n0 = 0, es = vsrk_esize(x->dtype); n0 < x->n; n0 += c.chunk_n) {
        vsrk_tensor5 xc = *x, gc = *dy;
        xc.n = gc.n = std::min(c.chunk_n, x->n - n0);
        xc.ptr = (char*)x->ptr + (int64_t)n0 * x->sn * es;
        gc.ptr = (char*)dy->ptr + (int64_t)n0 * dy->sn * es;
        VsrkRollPlan p = c.roll;
        bool ok = true;
        if (xc.n != c.chunk_n) ok = vsrk_wgrad_roll_plan(d, &xc, &gc, &p);  // the short last chunk: its own plan
        VSRK_CHECK(ok && p.slabs.ws_bytes() <= workspace_bytes, "conv_wgrad(roll): a sample chunk was not eligible");
        const int st = roll(&xc, &gc, p, n0 == 0 ? accumulate : 1);
        if (st != VSRK_OK) return st;
      }
      return VSRK_OK;
    case WG_ROW:
      vsrk_conv_wgrad_row(d, x, dy, dbias != nullptr, ws, c.row, s);
      VSRK_LAUNCH_CHECK("conv_wgrad(row)");
      return wgrad_reduce(c.row.slabs, ws, dy->c, x->c, perm_r, dy_scale, accumulate, dw, dbias, s);
    default: {
      if (c.gen.ntiles == 0) return VSRK_OK;
      const int st = wgrad_generic(d, x, dy, pro_scale, pro_shift, perm_r, dbias != nullptr, ws, c.gen, s);
      return st != VSRK_OK ? st : wgrad_reduce(c.gen.slabs, ws, dy->c, x->c, perm_r, dy_scale, accumulate, dw, dbias, s);
    }
  }
}
