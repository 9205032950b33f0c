// Row-walking Conv 3x3 (kd = 1, padding 1) 64 -> 256 channels on MFMA, the
// output written through a shuffle-2 view: the forward of EDSR's up-sampler
// convs nn.Conv2d(64, 256, 3, padding=1) + PixelShuffle(2) (edsr_net.py:117),
// bias and out_scale, no activation / residual / mask / accumulate.
//
// It is conv_row.hip's walk (read its header first: segments of 128 columns,
// bands of rows, the four-slot LDS ring that holds every input row once, the
// register staging with two rows in flight, conv_row_common.h) with other
// wave roles.  conv_roll's 2-D tile form ran these convs before: four
// 64-channel output blocks per 16 x 32 tile, so every input tile and its halo
// was staged four times, and the weights streamed through LDS per tile.
//  * The packed weight image (perm_r = 2: rows in view order, phase-major) is
//    256 rows x 9 taps x 64 ci x 2 B = 295 KB = 8 waves x 144 VGPRs: wave w
//    keeps packed rows 32 w .. 32 w + 31 in registers for the whole launch.
//    Those are channels 32 (w & 1) .. + 31 of phase w >> 1 (HR row 2 o +
//    (phase >> 1), HR column 2 col + (phase & 1)): conv_roll's spoff table.
//  * A stage is one low-res output row of the segment.  Every wave walks the
//    segment's four 32-voxel quarters: 36 MFMAs each into one of two banks
//    (quarter & 1); the bank of the quarter before is flushed beside them, the
//    last quarter's in the next stage.  144 MFMAs per wave for one barrier
//    and one staged row; the fragment reads are the LDS's only consumer.
//  * A quarter moves every fragment address by 32 voxels = 4096 B and leaves
//    the swizzle ((lv >> 1) & 7) alone: an immediate offset.
//  * Summation order per output element: channel chunk, kw, kh; the same
//    mma<H> on the same operands in the same roles and the same epilogue
//    arithmetic as conv_roll's SP_Y form, so the output is BITWISE what that
//    kernel stores (tests/test_conv_row_wide_gpu.py).
//  * The band's last stage only has the last quarter's flush to do; as in
//    conv_row_kernel its MFMAs run on stale rows into banks nobody stores (a
//    uniform branch around them doubles the flush code and the kernel then
//    spills: 184 B of scratch per lane against none).
#include "conv_row_common.h"

namespace {
using namespace vsrk_conv;

constexpr int CW_COUT = 256;
constexpr int CW_BIAS = CR_NSLOT * CR_SLOT;   // [256] bias * out_scale, packed-row order
constexpr int CW_LDS = CW_BIAS + CW_COUT * 4; // 67,584 B

using rawbuf::rsrc_at;

struct ConvRowWideArgs {
  CrView x;           // (images, H, W, 64)
  CrView y;           // the PHYSICAL (images, 2 H, 2 W, 64) image of the shuffle-2 view
  const void* w;      // packed [9 taps][256][cin_pad], rows in view order
  const float* bias;  // or null; torch pixel-shuffle order
  int cin_pad;
  float out_scale;
  int D, H, W;        // low-res
  int nseg, nband, band_h, nitems;
};

template <bool HALO, typename H>
__global__ __launch_bounds__(CR_NW * 64, 1) void conv_row_wide_kernel(ConvRowWideArgs a) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hf = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // ---- this wave's weights: fragment (tap, chunk c) = packed rows 32 wave + r,
  // input channels 16 c + 8 hf .. + 7 ----
  uint4 wf[9][4];
  {
    const H* wp = reinterpret_cast<const H*>(a.w);
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int c = 0; c < 4; ++c)
        wf[t][c] = *reinterpret_cast<const uint4*>(wp + ((int64_t)(t * CW_COUT + wave * 32 + r) * a.cin_pad + c * 16 + 8 * hf));
  }
  // epilogue lanes (after the register transpose): the 8-channel chunk ecc of
  // the wave's 32 packed rows, voxels (r & 15) + 16 q of the quarter
  const int ecc = 2 * (r >> 4) + hf;
  const int prow = wave * 32 + 8 * ecc;      // packed row: the bias table's index
  const int ych = (wave & 1) * 32 + 8 * ecc; // channel inside the phase
  const int phi = wave >> 2, phj = (wave >> 1) & 1;
  const float osc = a.out_scale;
  float* lbias = reinterpret_cast<float*>(lds + CW_BIAS);
  if (tid < CW_COUT) {  // view order (sub, c') -> torch order c' * 4 + sub
    float b = 0.f;
    if (a.bias) b = a.bias[(tid & 63) * 4 + (tid >> 6)];
    lbias[tid] = b * osc;
  }
  if constexpr (!HALO) {
    // one segment: the halo columns (voxels 0 and 129 of every slot) are
    // outside the image, zero for the whole launch
    if (tid < CR_NSLOT * 16)
      *reinterpret_cast<uint4*>(lds + (tid >> 4) * CR_SLOT + ((tid >> 3) & 1) * (CR_SEG + 1) * 128 + (tid & 7) * 16) =
          make_uint4(0, 0, 0, 0);
  }

  // ---- LDS addresses ----
  // voxel fragment of quarter vq, tap column kw, chunk c: voxel lv = 32 vq + r + kw, piece 2 c + hf
  uint32_t fa[3], fh[3];
#pragma unroll
  for (int kw = 0; kw < 3; ++kw) {
    fa[kw] = cr_frag_base(r + kw, hf);
    fh[kw] = cr_frag_swz(r + kw);
  }
  // staging roles, as conv_row_kernel's
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

    const uint32_t xcolb = 2u * (uint32_t)((c0 + scol) * a.x.sw + 8 * sp);
    const uint32_t hcolb = 2u * (uint32_t)((c0 + hcol) * a.x.sw + 8 * sp);
    bool xok[3];
    xok[0] = c0 + scol < a.W;
    xok[1] = c0 + scol + 64 < a.W;
    xok[2] = halo_lane && c0 + hcol >= 0 && c0 + hcol < a.W;
    // low-res column ecol + 32 vq + 16 q -> physical column 2 (..) + phj of physical row 2 o + phi
    const int ecol = c0 + (r & 15);
    const uint32_t ycolb = 2u * ((uint32_t)(2 * ecol + phj) * (uint32_t)a.y.sw + (uint32_t)phi * (uint32_t)a.y.sh + (uint32_t)ych);

    uint4 stq[CR_NSLOT][NSQ];
    const CrLoadRow<HALO, ConvRowWideArgs> load_row{a, r1, xok, xcolb, rx, hcolb};
    auto write_row = [&](int slot, const uint4 (&st)[NSQ]) __attribute__((always_inline)) {
      cr_write_row<HALO>(lds + slot * CR_SLOT, st, sdst, hdst, halo_lane);
    };

    // Flush of a finished bank = quarter vq of output row `orow` (a row
    // outside the band takes out-of-range offsets: nothing is stored)
    auto flush = [&](const f32x16& A, int orow, int vq) __attribute__((always_inline)) {
      const bool rv = orow >= r0 && orow < r1;
      float v[16];
      cr_transpose(A, v);
      float bsv[8];
      {
        const float4 c0 = *reinterpret_cast<const float4*>(lbias + prow);
        const float4 c1 = *reinterpret_cast<const float4*>(lbias + prow + 4);
        bsv[0] = c0.x; bsv[1] = c0.y; bsv[2] = c0.z; bsv[3] = c0.w;
        bsv[4] = c1.x; bsv[5] = c1.y; bsv[6] = c1.z; bsv[7] = c1.w;
      }
      const uint32_t yrow = 2u * (uint32_t)(2 * (rv ? orow : 0)) * (uint32_t)a.y.sh;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        float t[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) t[e] = fmaf(v[8 * q + e], osc, bsv[e]);
        const int dc = 32 * vq + 16 * q;
        const uint32_t yo = ycolb + yrow + 2u * (uint32_t)(2 * dc) * (uint32_t)a.y.sw;
        cr_store16(ry, (rv && ecol + dc < a.W) ? yo : CR_OOB, Chunk<H>::pack(t));
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

    // Stage s (K = s % 4): output row o = r0 + s from the input rows o - 1,
    // o, o + 1 in slots K, K + 1, K + 2; the row the stage before loaded goes
    // to slot K + 3 at its end.  Quarter vq goes into bank vq & 1 while the
    // other bank, the quarter before (quarter 3 of row o - 1 for vq = 0), is
    // flushed: the flush has no register in common with the quarter's MFMAs.
    int s = 0;
    auto step = [&](auto k_c) __attribute__((always_inline)) -> bool {
      constexpr int K = decltype(k_c)::value;
      const int o = r0 + s;
      __syncthreads();  // slots K .. K + 2 are whole; every wave is past its reads of slot (K + 3) % 4
      load_row(o + 3, stq[K]);  // written to slot K at the end of the next stage
      // (the fragment addresses are recomputed per stage, not kept in VGPRs)
#pragma unroll
      for (int kw = 0; kw < 3; ++kw) asm volatile("" : "+v"(fh[kw]));
#pragma unroll
      for (int vq = 0; vq < 4; ++vq) {
        f32x16& Pcur = (vq & 1) ? b1 : b0;
        const f32x16& Pprev = (vq & 1) ? b0 : b1;
        // (a quarter is scheduled on its own: with the four in one region the
        // fragment reads are hoisted across quarters and the kernel spills)
        __builtin_amdgcn_sched_barrier(0);
        flush(Pprev, vq == 0 ? o - 1 : o, (vq + 3) & 3);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
#pragma unroll
          for (int kw = 0; kw < 3; ++kw) {
            const uint32_t fo = fa[kw] + (((uint32_t)c ^ fh[kw]) << 5);
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
              const uint4 f = *reinterpret_cast<const uint4*>(lds + ((K + kh) % CR_NSLOT) * CR_SLOT + vq * 32 * 128 + fo);
              if (c == 0 && kw == 0 && kh == 0) {
#pragma unroll
                for (int k = 0; k < 16; ++k) Pcur[k] = 0.f;
              }
              mma<H>(Pcur, wf[kh * 3 + kw][c], f);
            }
          }
        }
      }
      write_row((K + 3) % CR_NSLOT, stq[(K + 3) % CR_NSLOT]);  // input row o + 2, loaded one stage ago
      return ++s < nstage;
    };
#pragma unroll
    for (int k = 0; k < 16; ++k) b0[k] = b1[k] = 0.f;
    while (step(std::integral_constant<int, 0>{}) && step(std::integral_constant<int, 1>{}) &&
           step(std::integral_constant<int, 2>{}) && step(std::integral_constant<int, 3>{})) {
    }
  }
}

unsigned long long g_row_wide_launches = 0;

template <typename H>
int launch_row_wide(const ConvRowWideArgs& a, int grid, hipStream_t s) {
  // (one segment: the form without the halo-column loads)
  auto kern = a.nseg > 1 ? conv_row_wide_kernel<true, H> : conv_row_wide_kernel<false, H>;
  (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, CW_LDS);
  kern<<<grid, CR_NW * 64, CW_LDS, s>>>(a);
  ++g_row_wide_launches;
  VSRK_LAUNCH_CHECK("conv_fwd(row_wide)");
  return VSRK_OK;
}

// Shapes routed to the wide kernel by default (mode -1): those that measured
// faster than the tile kernel.  Both shapes of
// the EDSR x4 step did, 64 images of 128 x 128 and of 256 x 256 low-res voxels
// (one and two segments, 32- and 128-row bands), by 26-29 % per launch, and
// nothing in the walk gets dearer at another size: every eligible shape.
constexpr bool cw_default_on(const vsrk_tensor5*) { return true; }

}  // namespace

// launches of the wide row kernel so far (tests: the routing, which the outputs do not show)
extern "C" unsigned long long vsrk_conv_row_wide_launches(void) { return g_row_wide_launches; }

// The caller (roll_fwd_one's SP_Y branch) has checked: 16-bit x and y of one
// type, 3x3, y's shuffle view (whole phases, 8-byte alignment), no prologue /
// residual / ReLU mask, the conv's output geometry, non-negative strides.
// 1 = launched, 0 = not eligible, < 0 = -(error status)
int vsrk_conv_fwd_row_wide(const vsrk_conv_desc* d, const vsrk_tensor5* x, const void* w_packed, const float* bias,
                           const vsrk_tensor5* residual, const vsrk_tensor5* mask, const vsrk_tensor5* y,
                           hipStream_t s) {
  const int mode = vsrk_g_row_wide_mode;  // -1: per-shape default routing, 0 off, 1 every eligible shape
  if (mode == 0) return 0;
  if (d->kd != 1 || d->kh != 3 || d->kw != 3 || d->pd != 0 || d->ph != 1 || d->pw != 1) return 0;
  if (x->c != 64 || y->c != CW_COUT || y->shuffle != 2 || x->shuffle > 1) return 0;
  if (d->subpixel || d->act != VSRK_ACT_NONE) return 0;
  if (residual || mask || d->accumulate || d->prologue || d->mask_slope) return 0;
  if (bias && d->bias_perm_r != 2) return 0;  // the bias table's order is the shuffle's
  if (x->n != y->n || x->d != y->d || x->h != y->h || x->w != y->w) return 0;
  if (mode < 0 && !cw_default_on(y)) return 0;
  if (!chunk_ok(x, 2)) return 0;
  if (!cr_view_fits(x, x->h, x->w) || !cr_view_fits(y, 2 * (int64_t)y->h, 2 * (int64_t)y->w)) return 0;
  const int64_t nimg = (int64_t)y->n * y->d;
  if (nimg == 0 || y->h == 0 || y->w == 0) return 1;
  CrPlan p;
  if (!cr_plan(nimg, y->h, y->w, p)) return 0;
  ConvRowWideArgs a;
  a.x = cr_view(x);
  a.y = cr_view(y);
  a.w = w_packed;
  a.bias = bias;
  a.cin_pad = round_up(x->c, 32);
  a.out_scale = d->out_scale;
  a.D = y->d; a.H = y->h; a.W = y->w;
  a.nseg = p.nseg; a.nband = p.nband; a.band_h = p.band_h; a.nitems = p.nitems;
  int rc = vsrk_dispatch16(x->dtype, [&](auto tag) { return launch_row_wide<decltype(tag)>(a, p.grid, s); });
  return rc == VSRK_OK ? 1 : -rc;
}
