// Row-walking implicit-GEMM Conv 3x3 (kd = 1, padding 1, stride 1) 64 -> 64
// channels on MFMA for 16-bit channels-last views (gfx950): the forward of
// EDSR's body convs nn.Conv2d(64, 64, 3, padding=1) (edsr_net.py:41-53,
// 108-114) and, with a mode-1 packed weight, their input gradient
// (edsr_net.py:182-190, loss.backward()).
//
// Why not conv_roll's 2-D form: "rolling" there rolls over depth, and with
// kd = 1 nothing rolls -- it is a tiled conv of 16 x 32 voxels with an
// 18 x 34 halo (1.20x the tile staged), four 16-channel K stages per tile
// (each a barrier and 20 LDS-DMA pieces) and a burst epilogue of the whole
// tile; 2048 tiles per EDSR launch, each with a fill and a drain, at about
// twice the HBM floor.  Here, as conv_wgrad_row.hip does for the weight
// gradient, the walk is over image rows:
//  * A workgroup owns a segment of up to 128 output columns, all 64 input and
//    output channels and a band of consecutive rows of one slice.  Every
//    input row (all 64 channels) is brought into a four-slot LDS ring ONCE and
//    stays for the three output rows that meet it.  A stage is ONE output row
//    (K = 9 x 64 per stage and barrier) from the three resident input rows,
//    into one of two accumulator banks that alternate per stage; the bank of
//    the stage before is a finished output row and is stored during this
//    stage: its flush shares no register with the stage's MFMAs.  Loads, MFMAs
//    and stores run at one steady rate; no column halo (one zero or neighbour
//    voxel each side), 2 halo rows per band.
//  * Summation order of an output element: channel chunk, kw, kh -- the order
//    of conv_roll's 2-D form, the same MFMA on the same operands in the same
//    roles, so the output is BITWISE what that kernel stores (a train step
//    computes what it computed before; tests/test_conv_row_gpu.py).  Rolling
//    three banks over the input rows (kh outermost, one third of the
//    fragment reads) gives another fp32 order: measured about 5 % faster per
//    launch, but the step's outputs then differ from the tile kernel's (at
//    rounding level per layer; after 33 layers and Adam, up to 0.6 % on single
//    weights), which a change of kernel alone must not do.  The order is the
//    same at every row of the image, whatever the band split or the grid.
//  * 8 waves = 2 output halves (32 channels) x 4 voxel quarters (32 columns),
//    two per SIMD; v_mfma_f32_32x32x16, operands "weights x voxels".
//  * Weights in REGISTERS: a wave's 9 taps x 4 chunks x (32 co x 16 ci) = 36
//    fragments of 4 VGPRs (144), loaded once per workgroup straight from the
//    packed image (vsrk_conv_pack_weights, mode 0 or 1).  The alternative, the
//    72 KB image resident in LDS, costs one ds_read_b128 per MFMA: 4 SIMDs x
//    1 KB per 32-cycle MFMA is the whole LDS read rate (128 B / cycle), with
//    the voxel fragments and the staging writes on top; from registers the
//    LDS carries the voxel fragment reads alone, one per MFMA and wave.
//  * Register staging, two rows in flight, with ordinary (compiler-visible)
//    buffer loads: during the stage of output row o each wave loads 2 KB of
//    input row o + 3 (16 B per lane, coalesced; out-of-image rows and columns
//    read as zero through an out-of-range buffer offset: no branch) into one
//    of four register sets that rotate with the ring, and writes the set
//    loaded one stage earlier (row o + 2) to the ring at the end of the stage,
//    then one barrier.  No LDS-DMA: 17 pieces a row would cost 60-185
//    issue cycles each (MI355X_MICROARCH.md), and with DMA in flight the
//    compiler drains the counter at every ordinary load's use (the epilogue
//    operands).
//  * LDS image of a row: voxel lv = column - segment start + 1 (lv 0 and 129
//    are the halo columns) at lv * 128 B, its 16-byte piece p (channels
//    8 p .. 8 p + 7) in position p ^ ((lv >> 1) & 7).  Banks: a ds_read_b128 /
//    ds_write_b128 is served in groups of 16 lanes = 256 B = all 64 banks
//    once.  Fragment read: 16 lanes read piece p of 16 consecutive voxels
//    lv0 .. lv0 + 15 (any lv0: the kw taps shift it by 0..2): (lv >> 1) & 7
//    takes every value 0..7 twice, the two times on voxels of different
//    parity (the 128-byte half of the 256-byte bank line), so the 16
//    (half, position) pairs are distinct.  Staging write: 16 lanes fill the 8
//    pieces of 2 consecutive voxels: 2 halves x 8 distinct positions.
//  * The epilogue transposes a bank in registers (v_permlane32/16_swap, as
//    conv_roll's epilogue_sw): every global access is 16 contiguous bytes.
//    The operand rows (residual, mask, old output for accumulate) are loaded
//    into registers one stage ahead.  Rounds once, at the store.
#include "conv_row_common.h"

namespace {
using namespace vsrk_conv;

constexpr int CR_BIAS = CR_NSLOT * CR_SLOT;    // [64] bias * out_scale
constexpr int CR_LDS = CR_BIAS + 256;          // 66,816 B
enum { CE_RES = 1, CE_MASK = 2, CE_ACC = 4, CE_RELU = 8 };

using rawbuf::rsrc_at;

struct ConvRowArgs {
  CrView x, y, res, msk;
  const void* w;      // packed [9 taps][cout_pad][cin_pad]
  const float* bias;  // or null
  int cout_pad, cin_pad;
  float out_scale;
  int D, H, W;
  int nseg, nband, band_h, nitems;
};

template <int EM, bool HALO, typename H>
__global__ __launch_bounds__(CR_NW * 64, 1) void conv_row_kernel(ConvRowArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hf = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int coh = wave & 1, vq = wave >> 1;  // output half (32 channels), voxel quarter (32 columns)

  // ---- this wave's weights: fragment (tap, chunk c) = rows coh*32 + r,
  // input channels 16 c + 8 hf .. + 7 ----
  uint4 wf[9][4];
  {
    const H* wp = reinterpret_cast<const H*>(a.w);
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int c = 0; c < 4; ++c)
        wf[t][c] = *reinterpret_cast<const uint4*>(wp + ((int64_t)(t * a.cout_pad + coh * 32 + r) * a.cin_pad + c * 16 + 8 * hf));
  }
  // epilogue lanes (after the register transpose): the 8-channel chunk ecc of
  // the wave's output half, voxels (r & 15) + 16 q of its quarter
  const int ecc = 2 * (r >> 4) + hf;
  const int ech = coh * 32 + 8 * ecc;
  const float osc = a.out_scale;
  float* lbias = reinterpret_cast<float*>(lds + CR_BIAS);
  if (tid < 64) lbias[tid] = a.bias ? a.bias[tid] * osc : 0.f;
  if constexpr (!HALO) {
    // one segment: the halo columns (voxels 0 and 129 of every slot) are
    // outside the image, zero for the whole launch
    if (tid < CR_NSLOT * 16)
      *reinterpret_cast<uint4*>(lds + (tid >> 4) * CR_SLOT + ((tid >> 3) & 1) * (CR_SEG + 1) * 128 + (tid & 7) * 16) =
          make_uint4(0, 0, 0, 0);
  }

  // ---- LDS addresses ----
  // voxel fragment of tap column kw, chunk c: voxel lv = 32 vq + r + kw, piece 2 c + hf
  uint32_t fa[3], fh[3];
#pragma unroll
  for (int kw = 0; kw < 3; ++kw) {
    const int lv = vq * 32 + r + kw;
    fa[kw] = cr_frag_base(lv, hf);
    fh[kw] = cr_frag_swz(lv);
  }
  // staging roles: q = 0, 1: column 8 wave + lane / 8 + 64 q of the segment,
  // piece lane & 7 (64 voxels apart: the same swizzle, 8 KB apart in the
  // slot); with a halo, wave 0's lanes 0-15 also the two halo columns
  const int sp = lane & 7;
  constexpr int NSQ = HALO ? 3 : 2;
  const int scol = 8 * wave + (lane >> 3);
  const int hcol = (lane >> 3) == 0 ? -1 : CR_SEG;
  const uint32_t sdst = CR_STAGE_DST(scol, sp);
  const uint32_t hdst = CR_STAGE_DST(hcol, sp);
  const bool halo_lane = wave == 0 && lane < 16;

  f32x16 b0, b1;

  for (int item = blockIdx.x; item < a.nitems; item += gridDim.x) {
    // item = (image, segment, band), band fastest (neighbours share halo rows in L2)
    const int band = item % a.nband;
    const int t1 = item / a.nband;
    const int seg = t1 % a.nseg, img = t1 / a.nseg;
    const int in_ = img / a.D, id = img - in_ * a.D;
    const int c0 = seg * CR_SEG;
    const int r0 = band * a.band_h, r1 = min(r0 + a.band_h, a.H);
    const int nstage = r1 - r0 + 1;  // one per output row, and one for the last flush

    const CrRsrc rx = rsrc_at(reinterpret_cast<const H*>(a.x.ptr) + (in_ * a.x.sn + id * a.x.sd));
    const CrRsrc ry = rsrc_at(reinterpret_cast<const H*>(a.y.ptr) + (in_ * a.y.sn + id * a.y.sd));
    const CrRsrc rr = rsrc_at(reinterpret_cast<const H*>(a.res.ptr) + (in_ * a.res.sn + id * a.res.sd));
    const CrRsrc rm = rsrc_at(reinterpret_cast<const H*>(a.msk.ptr) + (in_ * a.msk.sn + id * a.msk.sd));

    // per-lane byte offsets inside a row (q = 0; the q-th group's columns go
    // into the uniform offset) and the validity of each group's column
    const uint32_t xcolb = 2u * (uint32_t)((c0 + scol) * a.x.sw + 8 * sp);
    const uint32_t hcolb = 2u * (uint32_t)((c0 + hcol) * a.x.sw + 8 * sp);
    bool xok[3];
    xok[0] = c0 + scol < a.W;
    xok[1] = c0 + scol + 64 < a.W;
    xok[2] = halo_lane && c0 + hcol >= 0 && c0 + hcol < a.W;
    const int ecol = c0 + vq * 32 + (r & 15);
    const uint32_t ycolb = 2u * (uint32_t)(ecol * a.y.sw + ech);
    const uint32_t rcolb = 2u * (uint32_t)(ecol * a.res.sw + ech);
    const uint32_t mcolb = 2u * (uint32_t)(ecol * a.msk.sw + ech);
    const bool yok[2] = {ecol < a.W, ecol + 16 < a.W};

    // input row `row` of the band's walk (zero outside the image or past the band's last halo row)
    // (four register sets in rotation with the ring: the set a stage loads is
    // written to LDS at the end of the NEXT stage, so two rows are in flight
    // and at most two sets are live)
    uint4 stq[CR_NSLOT][NSQ];
    const CrLoadRow<HALO, ConvRowArgs> load_row{a, r1, xok, xcolb, rx, hcolb};
    auto write_row = [&](int slot, const uint4 (&st)[NSQ]) __attribute__((always_inline)) {
      cr_write_row<HALO>(lds + slot * CR_SLOT, st, sdst, hdst, halo_lane);
    };

    // epilogue operands of output row `orow`, one stage ahead of its flush
    uint4 pr[2], pm[2], po[2];
    auto load_pre = [&](int orow) __attribute__((always_inline)) {
      const bool rv = orow >= r0 && orow < r1;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const bool ok = rv && yok[q];
        const int ro = rv ? orow : 0;
        if constexpr (EM & CE_RES) pr[q] = cr_load16(rr, ok ? rcolb : CR_OOB, 2u * (uint32_t)(ro * a.res.sh + 16 * q * a.res.sw));
        if constexpr (EM & CE_MASK) pm[q] = cr_load16(rm, ok ? mcolb : CR_OOB, 2u * (uint32_t)(ro * a.msk.sh + 16 * q * a.msk.sw));
        if constexpr (EM & CE_ACC) po[q] = cr_load16(ry, ok ? ycolb : CR_OOB, 2u * (uint32_t)(ro * a.y.sh + 16 * q * a.y.sw));
      }
    };

    // Flush of a finished bank = output row `orow` (a row outside the band
    // takes out-of-range offsets: nothing is stored), through cr_transpose:
    // the lane then holds chunk ecc of voxels (r & 15) + 16 q in v[8 q .. + 7].
    auto flush = [&](const f32x16& A, int orow) __attribute__((always_inline)) {
      const bool rv = orow >= r0 && orow < r1;
      float v[16];
      cr_transpose(A, v);
      float bsv[8];
      {
        const float4 c0 = *reinterpret_cast<const float4*>(lbias + ech);
        const float4 c1 = *reinterpret_cast<const float4*>(lbias + ech + 4);
        bsv[0] = c0.x; bsv[1] = c0.y; bsv[2] = c0.z; bsv[3] = c0.w;
        bsv[4] = c1.x; bsv[5] = c1.y; bsv[6] = c1.z; bsv[7] = c1.w;
      }
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        float t[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          t[e] = fmaf(v[8 * q + e], osc, bsv[e]);
          if constexpr (EM & CE_RELU) t[e] = fmaxf(t[e], 0.f);
        }
        if constexpr (EM & CE_MASK) {
          float m[8];
          Chunk<H>::unpack(pm[q], m);
#pragma unroll
          for (int e = 0; e < 8; ++e) t[e] = m[e] > 0.f ? t[e] : 0.f;
        }
        if constexpr (EM & CE_RES) {
          float rs[8];
          Chunk<H>::unpack(pr[q], rs);
#pragma unroll
          for (int e = 0; e < 8; ++e) t[e] += rs[e];
        }
        if constexpr (EM & CE_ACC) {
          float o[8];
          Chunk<H>::unpack(po[q], o);
#pragma unroll
          for (int e = 0; e < 8; ++e) t[e] += o[e];
        }
        const uint32_t yo = ycolb + 2u * (uint32_t)((rv ? orow : 0) * a.y.sh + 16 * q * a.y.sw);
        cr_store16(ry, (rv && yok[q]) ? yo : CR_OOB, Chunk<H>::pack(t));
      }
    };

    // ---- fill: input rows r0 - 1, r0, r0 + 1 into slots 0-2, row r0 + 2 in flight ----
    __syncthreads();  // the previous item's last stage is done with the ring
    load_row(r0 - 1, stq[0]);
    load_row(r0, stq[1]);
    load_row(r0 + 1, stq[2]);
    load_row(r0 + 2, stq[3]);  // in flight through stage 0, which writes it to slot 3
    write_row(0, stq[0]);
    write_row(1, stq[1]);
    write_row(2, stq[2]);
    load_pre(r0 - 1);  // (outside the band: zeros, keeps the first flush's operands defined)

    // Stage s (K = s % 4): output row o = r0 + s from the input rows o - 1,
    // o, o + 1 in slots K, K + 1, K + 2; the row the stage before loaded goes
    // to slot K + 3 at its end.  Pprev is the row finished one stage ago:
    // its flush has no register in common with this stage's MFMAs.  The last
    // stage (s = r1 - r0) only flushes; its MFMAs run on stale rows into a
    // bank nobody stores (no branch around them).
    int s = 0;
    auto step = [&](auto k_c, f32x16& Pcur, const f32x16& Pprev) __attribute__((always_inline)) -> bool {
      constexpr int K = decltype(k_c)::value;
      const int o = r0 + s;
      __syncthreads();  // slots K .. K + 2 are whole; every wave is past its reads of slot (K + 3) % 4
      load_row(o + 3, stq[K]);  // written to slot K at the end of the next stage
      flush(Pprev, o - 1);
      load_pre(o);
      // (the 12 fragment addresses are recomputed per stage, not kept in 12 VGPRs)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) asm volatile("" : "+v"(fh[kw]));
#pragma unroll
      for (int c = 0; c < 4; ++c) {
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const uint32_t fo = fa[kw] + (((uint32_t)c ^ fh[kw]) << 5);
#pragma unroll
          for (int kh = 0; kh < 3; ++kh) {
            const uint4 f = *reinterpret_cast<const uint4*>(lds + ((K + kh) % CR_NSLOT) * CR_SLOT + fo);
            if (c == 0 && kw == 0 && kh == 0) {
#pragma unroll
              for (int k = 0; k < 16; ++k) Pcur[k] = 0.f;
            }
            mma<H>(Pcur, wf[kh * 3 + kw][c], f);
          }
        }
      }
      write_row((K + 3) % CR_NSLOT, stq[(K + 3) % CR_NSLOT]);  // input row o + 2, loaded one stage ago
      return ++s < nstage;
    };
#pragma unroll
    for (int k = 0; k < 16; ++k) b0[k] = b1[k] = 0.f;
    while (step(std::integral_constant<int, 0>{}, b0, b1) && step(std::integral_constant<int, 1>{}, b1, b0) &&
           step(std::integral_constant<int, 2>{}, b0, b1) && step(std::integral_constant<int, 3>{}, b1, b0)) {
    }
  }
}

unsigned long long g_row_launches = 0;

template <int EM, typename H>
int launch_row(const ConvRowArgs& a, int grid, hipStream_t s) {
  // (one segment: the form without the halo-column loads)
  auto kern = a.nseg > 1 ? conv_row_kernel<EM, true, H> : conv_row_kernel<EM, false, H>;
  (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, CR_LDS);
  kern<<<grid, CR_NW * 64, CR_LDS, s>>>(a);
  ++g_row_launches;
  VSRK_LAUNCH_CHECK("conv_fwd(row)");
  return VSRK_OK;
}

// Forms routed to the row kernel by default (mode -1): those that measured
// faster than the tile kernel inside the EDSR step
constexpr bool cr_default_on(int em) {
  return em == 0 || em == CE_RELU || em == CE_RES || em == CE_MASK || em == (CE_RES | CE_ACC);
}

}  // namespace

// launches of the row kernel so far (tests: the routing, which the outputs do not show)
extern "C" unsigned long long vsrk_conv_row_launches(void) { return g_row_launches; }

// The caller (roll_fwd_one's 2-D branch) has checked: 16-bit x and y of one
// type, 3x3, kd = 1, plain views, geometry of y / residual / mask, 8-byte
// alignment of the output-shaped views, non-negative strides.
// 1 = launched, 0 = not eligible, < 0 = -(error status)
int vsrk_conv_fwd_row(const vsrk_conv_desc* d, const vsrk_tensor5* x, const void* w_packed, const float* bias,
                      const vsrk_tensor5* residual, const vsrk_tensor5* mask, const vsrk_tensor5* y, hipStream_t s) {
  const int mode = vsrk_path_mode(VSRK_PATH_ROW);  // -1: per-form default routing, 0 off, 1 every eligible form
  if (mode == 0) return 0;
  if (d->kd != 1 || d->kh != 3 || d->kw != 3 || d->pd != 0 || d->ph != 1 || d->pw != 1) return 0;
  if (x->c != 64 || y->c != 64 || x->shuffle > 1 || y->shuffle > 1) return 0;
  if (d->prologue || d->mask_slope || d->bias_perm_r > 1 || d->subpixel) return 0;
  if (d->act != VSRK_ACT_NONE && d->act != VSRK_ACT_RELU) return 0;
  if (x->n != y->n || x->d != y->d || x->h != y->h || x->w != y->w) return 0;
  const int em = (residual ? CE_RES : 0) | (mask ? CE_MASK : 0) | (d->accumulate ? CE_ACC : 0) |
                 (d->act == VSRK_ACT_RELU ? CE_RELU : 0);
  if (em != 0 && em != CE_RELU && em != CE_RES && em != CE_MASK && em != (CE_RES | CE_ACC)) return 0;
  if (mode < 0 && !cr_default_on(em)) return 0;
  if (!chunk_ok(x, 2)) return 0;
  for (const vsrk_tensor5* t : {x, y, residual, mask})
    if (t && !cr_view_fits(t, t->h, t->w)) return 0;
  const int64_t nimg = (int64_t)y->n * y->d;
  if (nimg == 0 || y->h == 0 || y->w == 0) return 1;
  CrPlan p;
  if (!cr_plan(nimg, y->h, y->w, p)) return 0;
  ConvRowArgs a;
  a.x = cr_view(x);
  a.y = cr_view(y);
  a.res = cr_view(residual ? residual : y);
  a.msk = cr_view(mask ? mask : y);
  a.w = w_packed;
  a.bias = bias;
  a.cin_pad = round_up(x->c, 32);
  a.cout_pad = round_up(y->c, 128);
  a.out_scale = d->out_scale;
  a.D = y->d; a.H = y->h; a.W = y->w;
  a.nseg = p.nseg; a.nband = p.nband; a.band_h = p.band_h; a.nitems = p.nitems;
  const int grid = p.grid;
  int rc = vsrk_dispatch16(x->dtype, [&](auto tag) {
    using H = decltype(tag);
    switch (em) {
      case 0: return launch_row<0, H>(a, grid, s);
      case CE_RELU: return launch_row<CE_RELU, H>(a, grid, s);
      case CE_RES: return launch_row<CE_RES, H>(a, grid, s);
      case CE_MASK: return launch_row<CE_MASK, H>(a, grid, s);
      default: return launch_row<CE_RES | CE_ACC, H>(a, grid, s);
    }
  });
  return rc == VSRK_OK ? 1 : -rc;
}
