// Pointwise (1x1x1) convolution on CDNA4 for 16-bit (bf16 / fp16) channels-last activations:
// forward / data-gradient (pw_fwd) and weight gradient (pw_wgrad).
//
// DUF's dense-unit bottlenecks (BN3d-ReLU-Conv1x1x1, duf_net.py:198-200,
// cin = cout = 64..224 at up to 7 x 128 x 128 voxels per sample) and its
// 256-channel heads (duf_net.py:40-49) move (cin + cout) * 2 bytes per voxel
// for 2 * cin * cout flops: <= 256 flop/B at cin = cout <= 256, under the
// MI355X ridge (2.5 PF / 8 TB/s ~ 312 flop/B).  They are HBM-bound, so the
// design goal is ONE pass over x and y at full HBM rate (the 3x3 tile kernels
// re-read x once per 128-channel output tile and stage it through LDS with a
// barrier per tile):
//
//  * pw_fwd: the weight chunk (<= 256 x 256 bf16 = 128 KiB) is staged into LDS
//    once per workgroup.  Each wave then streams its own 32*M-voxel tiles
//    from HBM with coalesced row loads through a wave-private LDS row buffer
//    (the MFMA B operand, x^T: lane l holds voxel l&31, 8 channels), applies
//    the BatchNorm+ReLU prologue in registers, runs all output-channel blocks
//    against the resident weights (A operand, one conflict-free ds_read_b128
//    per MFMA) and stores rows back the same way: no barrier after the weight
//    load, the next tile's loads in flight during the current tile's MFMAs
//    and stores (pw_fwd_staged_kernel below).
//  * pw_wgrad: dW = dY^T X reduces over voxels.  Each workgroup owns a
//    contiguous voxel range and a (cout chunk x cin chunk) of <= 256 x 256,
//    stages 64 voxels of dY and X per step (register-staged double buffer,
//    planar 64-byte rows read transposed with ds_read_b64_tr_b16), and writes
//    one fp32 partial slab; pw_wgrad_reduce sums the slabs in split order
//    (deterministic).  One pass over dY and X per cin/cout chunk.
//
// This header holds the device helpers, the kernel templates and their
// templated launchers; conv_pw.hip holds the host side (eligibility, argument
// set-up, plans, the C entry points and the two small reduce kernels) and each
// conv_pw_*.hip translation unit instantiates one family of kernels behind a
// plain function declared below, so the library builds in parallel.
#pragma once
#include <algorithm>
#include <type_traits>
#include "conv_common.h"

namespace vsrk_conv {

constexpr int PW_THR = 256;  // 4 waves, one per SIMD
enum { EIN_GEN = 1, EIN_ACC = 2, EIN_PB = 3, EIN_PBACC = 4 };  // staged kernel store-pass forms
constexpr int PW_KP = 64;    // wgrad voxels per stage
// cache policy of the staged kernel's output stores: non-temporal (DUF 75.8 -> 75.4 ms, profiles/r4_pw_nt_ab.txt)
constexpr int PW_NT = 2;

// Division by a launch constant d (dividends < 2^31), branch-free:
// q = (x * mul) >> p with p = 31 + ceil(log2 d), mul = ceil(2^p / d) < 2^32.
struct FastDiv {
  uint32_t d, mul, p;
};
inline FastDiv make_fastdiv(int d) {
  int l = 0;
  while ((1u << l) < (uint32_t)d) ++l;
  const uint32_t p = 31 + l;
  return FastDiv{(uint32_t)d, (uint32_t)(((1ull << p) + (uint64_t)d - 1) / (uint64_t)d), p};
}
__device__ __forceinline__ uint32_t fdiv(uint32_t x, const FastDiv& f) {
  return (uint32_t)(((uint64_t)x * f.mul) >> f.p);
}

struct PwArgs {  // 16-bit tensors of one type H (bf16 / fp16)
  const void* x;
  void* y;
  const void* msk;
  const void* w;  // packed [round_up(cout,128)][ci_pad] (vsrk_conv_pack_weight)
  const float* bias;
  const float* pro_scale;
  const float* pro_shift;
  const float* mask_slope;
  const float* act_param;                 // PReLU slope (device scalar)
  // fused per-channel reduction of the stored output (RED 1: BatchNorm
  // statistics sum y, sum y^2; RED 2: BatchNorm+ReLU backward sum dy',
  // sum dy' xhat with dy' = y * (bnx * scale + shift > 0), xhat =
  // (bnx - mean) * invstd): per-lane partials, slab [block][wave][lane][16]
  const void* bnx;
  int64_t bsn, bsw;
  const float *bsc, *bsh, *bmu, *bis;
  float* red_ws;
  // BNB: the conv input is a BatchNorm+ReLU backward applied on the fly
  // (x = dz, the BN's output gradient; qx = the BN's input): the applied
  // gradient feeds the MFMAs and is stored to xo (the weight gradient's dY)
  const void* qx;
  void* xo;
  int64_t qsn, qsw, osn, osw;
  const float *qsh, *qmu, *qis, *qgm, *qsdy, *qsdyx;
  float qinv_count;
  int64_t xsn, xsw, ysn, ysw, msn, msw;  // element strides
  int nvox, dhw;
  FastDiv fd;                             // division by dhw
  int cin, cout, ci_pad, co_rows;
  int prologue, act, accumulate, has_mask;
  // PBWD (EIN form): the PReLU backward of the output's consumer applied
  // after the accumulate, on output channels >= pm_lo (a consumer that
  // owns the tail slice of a concat gradient): dy' = (conv [+ dy]) *
  // (msk > 0 ? 1 : slope), msk = that PReLU's output; the slope gradient
  // sum_{msk<0} dy' msk as per-lane partials, slab [block y][block x][wave][lane]
  int pbwd, pm_lo;
  double* slope_part;  // [block y][block x][wave] partials of the slope gradient
  float out_scale;
  int ntiles;  // tiles of 32*M voxels
};

struct PwWArgs {
  const void* x;
  const void* dy;
  const float* pro_scale;
  const float* pro_shift;
  float* ws;
  int64_t xsn, xsw, dsn, dsw;  // element strides
  int nvox, vox_per_split, dhw;
  FastDiv fd;
  int cin, cout, prologue;
  int ncit;                  // ci blocks in this launch's chunks (<= NW, one per wave)
  int ci_chunks, nchunks;    // blockIdx.y = co_chunk * ci_chunks + ci_chunk
  int slab;                  // floats per (split, chunk): 32*NCO * 32*ncit + 32*NCO
  int want_bias;
};

// Tiles of 32*M voxels per wave step: M so that one step loads ~16 KiB of nkb
// input blocks, and at most 128 accumulators (M * ncb <= 8).
constexpr int pw_m(int nkb) { return nkb <= 2 ? 4 : (nkb <= 4 ? 2 : 1); }
constexpr int pw_tile_m(int ncb, int nkb) { return pw_m(nkb) * ncb <= 8 ? pw_m(nkb) : (8 / ncb > 0 ? 8 / ncb : 1); }

// f(std::integral_constant<int, N>{}) for the N of [LO, HI] equal to n, and
// its result; false when n is outside the range.
template <int LO, int HI, typename F>
bool pw_dispatch_ncb(int n, F&& f) {
  if constexpr (LO > HI) {
    return false;
  } else {
    if (n == LO) return f(std::integral_constant<int, LO>{});
    return pw_dispatch_ncb<LO + 1, HI>(n, f);
  }
}

// Per-family launchers, one translation unit each.  Forward / data gradient on
// the staged kernel of ncb output and nkb input blocks of 32 channels, with
// a.ntiles tiles of 32 * pw_tile_m(ncb, nkb) voxels; false: nothing launched
// (the staged kernel declines the form, or the unit does not hold the shape).
bool pw_fwd_square_lo(int ncb, int nkb, int dtype, const PwArgs& a, int grid, int nchunk, hipStream_t s);  // conv_pw_sq_lo.hip: ncb = nkb = 2..4
bool pw_fwd_square_hi(int ncb, int nkb, int dtype, const PwArgs& a, int grid, int nchunk, hipStream_t s);  // conv_pw_sq_hi.hip: 5..7 and (4, 8)
bool pw_fwd_narrow(int ncb, int nkb, int dtype, const PwArgs& a, int grid, int nchunk, hipStream_t s);     // conv_pw_narrow.hip: (1,8) (2,4) (2,6) (2,8)
bool pw_fwd_widen(int ncb, int nkb, int dtype, const PwArgs& a, int grid, int nchunk, hipStream_t s);      // conv_pw_widen.hip: (4,2) (6,2) (8,2)
// square ncb = 2..7 with the fused per-channel reduction RED (1 / 2), bnb: the BNB input form
bool pw_fwd_reduce(int ncb, int dtype, int red, bool bnb, const PwArgs& a, int grid, hipStream_t s);       // conv_pw_red.hip
// weight gradient: nco = 2..8 dY blocks per chunk, nw = 4 or 8 waves
bool pw_wgrad(int nco, int nw, int dtype, const PwWArgs& a, int nsplit, hipStream_t s);          // conv_pw_wgrad.hip

}  // namespace vsrk_conv

namespace {
using namespace vsrk_conv;
using namespace vsrk_conv::rawbuf;

// LDS access by 32-bit byte address (plain vector types: HIP's uint4 class has
// no address-space-qualified copy)
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint4 lds_ld16(uint32_t addr) {
  return __builtin_bit_cast(uint4, *(const __attribute__((address_space(3))) u32x4_t*)(size_t)addr);
}
__device__ __forceinline__ float4 lds_ldf4(uint32_t addr) {
  return __builtin_bit_cast(float4, *(const __attribute__((address_space(3))) f32x4_t*)(size_t)addr);
}
__device__ __forceinline__ void lds_st8(uint32_t addr, uint2 v) {
  *(__attribute__((address_space(3))) u32x2_t*)(size_t)addr = __builtin_bit_cast(u32x2_t, v);
}
template <typename H>
__device__ __forceinline__ uint4 h8_affine(uint4 v, const float4& s0, const float4& s1, const float4& h0,
                                          const float4& h1, bool relu) {
  float f[8];
  Chunk<H>::unpack(v, f);
  const float sc[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
  const float sh[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float t = fmaf(f[e], sc[e], sh[e]);
    f[e] = relu ? fmaxf(t, 0.f) : t;
  }
  return Chunk<H>::pack(f);
}

// Byte offsets of a tile's voxels relative to the sample that holds its first
// voxel: lane voxel v = v0 + k (k < 32*M) -> (n - n0) * sn + r * sw.
struct TileBase {
  int n0, r0;
};
__device__ __forceinline__ TileBase tile_base(int v0, const FastDiv& fd) {
  const int n0 = (int)fdiv((uint32_t)v0, fd);
  return {n0, v0 - n0 * (int)fd.d};
}
__device__ __forceinline__ uint32_t lane_off(const TileBase& tb, int k, int v, int nvox, const FastDiv& fd,
                                             int64_t sn, int64_t sw) {
  // the host guarantees these offsets fit 31 bits: 32-bit arithmetic
  const uint32_t rel = (uint32_t)(tb.r0 + k);
  const uint32_t dn = fdiv(rel, fd);
  const uint32_t r = rel - dn * fd.d;
  const uint32_t off = 2u * (dn * (uint32_t)sn + r * (uint32_t)sw);
  return v < nvox ? off : OOB;
}

// ---------------------------------------------------------------------------
// forward / data gradient: y[v][co] = epi(sum_ci W[co][ci] * pro(x[v][ci]))
// NCB output blocks of 32 channels per workgroup (blockIdx.y picks the chunk),
// KS = 2*NKB k-steps of 16 input channels, M tiles of 32 voxels per wave step.
// ---------------------------------------------------------------------------
// The staged kernel (NCB <= 8 output blocks, NKB <= 8 input blocks; NCB < NKB
// for the narrowing 1x1 convs, e.g. DRF's 256 -> 64): each wave owns an LDS
// tile buffer [32*M voxels][CIP + 8 pad] H.  The next tile is fetched with
// coalesced 16-byte loads (consecutive lanes -> consecutive bytes of a voxel
// row, then the next row) into registers while the current tile computes; the
// B fragments are read back from LDS (row pad: conflict-free ds_read_b128).
// The outputs take the same way back: H-packed accumulators to the buffer,
// then coalesced 16-byte row stores.  Wave-private buffer: no barriers.
// AL: every tile lies inside one sample (d*h*w % (32*M) == 0), so a voxel
// row's offset is row * sw from the tile's base -- the common, cheap case;
// otherwise rows are placed with a division per row.  ACT: VSRK_ACT_NONE /
// VSRK_ACT_RELU at compile time (the epilogue is most of the VALU work).
// EIN: the ReLU/PReLU mask and / or accumulate of a data gradient
// (dx = mask(conv) [+ dx]) applied on the 16-byte row chunks of the store
// pass, their operands loaded as coalesced rows like the output (the
// first-generation register-operand kernel, since removed, read them 8 bytes
// per lane across 32 voxel rows).  The buffered value is rounded to H before
// the accumulate: one extra rounding of the new term against the conv_fast
// and tile kernels, which accumulate in fp32.
// BNB (with RED 2, no PRO / bias): the input is the BN+ReLU backward of the
// previous BatchNorm, x' = k1 * (qx * k1 + sh > 0 ? x : 0) + k2 * qx + k3
// per channel (bn_relu_bwd_apply_kernel's arithmetic, so x' is bitwise the
// separate apply's; k1 = gamma * invstd is bn_finalize's scale, bn.hip:193),
// computed on the 16-byte row chunks between the coalesced loads and the LDS
// put, and stored once to xo for the weight gradient.
template <int NCB, int NKB, int M, bool PRO, bool AL, int ACT, int EIN, typename H, int RED = 0, bool BNB = false>
__global__ __launch_bounds__(PW_THR, 1) void pw_fwd_staged_kernel(PwArgs a) {
  const H* aX = reinterpret_cast<const H*>(a.x);
  H* aY = reinterpret_cast<H*>(a.y);
  const H* aW = reinterpret_cast<const H*>(a.w);
  constexpr int KS = 2 * NKB;
  constexpr int COP = 32 * NCB;
  constexpr int CIP = 16 * KS;
  constexpr int RS = 2 * (CIP > COP ? CIP : COP) + 16;  // buffer row stride (bytes): input or output row
  constexpr int CPR = CIP / 8;               // 16-byte chunks per row
  constexpr int ROWS = 32 * M;
  constexpr int NCK = ROWS * CPR / 64;       // chunks per lane per tile (= M*KS)
  constexpr int WBYTES = KS * 2 * COP * 16;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  char* lw = lds;                                         // [KS][2][COP] x 16 B
  float* lsc = reinterpret_cast<float*>(lds + WBYTES);    // [CIP]
  float* lsh = lsc + CIP;                                 // [CIP]
  static_assert(!BNB || (RED == 2 && !PRO && !EIN && ACT == 0), "BNB: the data-gradient reduce form only");
  constexpr int OFF_LB = WBYTES + (PRO ? 2 * CIP * 4 : 0);
  constexpr int OFF_Q = OFF_LB + (BNB ? 0 : COP * 4);    // BNB: no bias (a data gradient)
  constexpr int OFF_BUF = OFF_Q + (BNB ? 4 * CIP * 4 : 0);
  float* lb = reinterpret_cast<float*>(lds + OFF_LB);     // [COP]
  float* lq = reinterpret_cast<float*>(lds + OFF_Q);      // BNB: [4][CIP] sh, k1, k2, k3
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hf = lane >> 5, col = lane & 31;
  const int co0 = blockIdx.y * COP;
  char* buf = lds + OFF_BUF + wave * (ROWS * RS);

  for (int i = tid; i < KS * 2 * COP; i += PW_THR) {
    const int co = i % COP, t = i / COP, h = t & 1, s = t >> 1;
    const int ci = 16 * s + 8 * h;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (ci < a.ci_pad && co0 + co < a.co_rows)
      v = *reinterpret_cast<const uint4*>(aW + (int64_t)(co0 + co) * a.ci_pad + ci);
    *reinterpret_cast<uint4*>(lw + i * 16) = v;
  }
  if (PRO) stage_prologue(lsc, lsh, a.prologue, a.pro_scale, a.pro_shift, a.cin, CIP, tid, PW_THR);
  if constexpr (BNB) {
    for (int c = tid; c < CIP; c += PW_THR) {
      float sh = 0.f, k1 = 0.f, k2 = 0.f, k3 = 0.f;
      if (c < a.cin) {  // bn_relu_bwd_apply_kernel's constants, the same fp32 operations
        const float is = a.qis[c], gm = a.qgm ? a.qgm[c] : 1.f;
        const float aa = gm * is, bb = is * a.qsdyx[c] * a.qinv_count;
        sh = a.qsh[c];
        k1 = aa;
        k2 = -aa * bb;
        k3 = aa * (a.qmu[c] * bb - a.qsdy[c] * a.qinv_count);
      }
      lq[c] = sh;
      lq[CIP + c] = k1;
      lq[2 * CIP + c] = k2;
      lq[3 * CIP + c] = k3;
    }
  } else {
    for (int i = tid; i < COP; i += PW_THR) lb[i] = (a.bias && co0 + i < a.cout) ? a.bias[co0 + i] : 0.f;
  }
  __syncthreads();

  const bool relu_in = (a.prologue & VSRK_PRO_RELU) != 0;
  const int nwaves = gridDim.x * (PW_THR / 64);
  const int wv = __builtin_amdgcn_readfirstlane(wave);
  const float osc = a.out_scale;
  const float pslope = ACT == VSRK_ACT_PRELU ? *a.act_param : 0.f;
  float sacc = 0.f;  // PBWD: this lane's slope-gradient partial
  // fused reduction: this lane's fixed 8-channel column and its constants
  constexpr int ROCPR = COP / 8;
  constexpr int RSTEP = 64 / ROCPR > 0 ? 64 / ROCPR : 1;
  constexpr int RNIT = RED ? (ROWS + RSTEP - 1) / RSTEP : 1;
  const int rcol = lane % ROCPR, rrow0 = lane / ROCPR;
  const bool rch_ok = co0 + 8 * rcol < a.cout;
  float rs1[8], rs2[8], rsc[8], rsh[8], rmu[8], ris[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    rs1[e] = rs2[e] = 0.f;
    rsc[e] = rsh[e] = rmu[e] = ris[e] = 0.f;
    if constexpr (RED == 2) {
      const int c = min(co0 + 8 * rcol + e, a.cout - 1);
      rsc[e] = a.bsc[c];
      rsh[e] = a.bsh[c];
      rmu[e] = a.bmu[c];
      ris[e] = a.bis[c];
    }
  }

  // byte offset of tile row `row` (voxel v0 + row) from the tile's sample base
  auto row_off = [&](const TileBase& tb, int row, int v0, int64_t sn, int64_t sw) __attribute__((always_inline)) {
    if constexpr (AL) {
      return (uint32_t)(2 * (tb.r0 + row) * (uint32_t)sw);
    } else {
      return lane_off(tb, row, v0 + row, a.nvox, a.fd, sn, sw);
    }
  };

  // fixed chunk roles: chunk k of a lane = row (lane + 64k) / CPR, column % CPR.
  // `ln` = lane through an opaque copy per use site: the per-chunk offsets
  // derived from it are recomputed (a few VALU) instead of held in VGPRs.
  constexpr int NQK = BNB ? NCK : 1;
  auto load = [&](int tile, uint4 (&r)[NCK], uint4 (&rq)[NQK]) __attribute__((always_inline)) {
    int ln = lane;
    asm volatile("" : "+v"(ln));
    const int v0 = tile * ROWS;
    const TileBase tb = tile_base(v0, a.fd);
    const Rsrc rs = rsrc_at(aX + (int64_t)tb.n0 * a.xsn);
#pragma unroll
    for (int k = 0; k < NCK; ++k) {
      const int i = ln + 64 * k, row = i / CPR, c = 8 * (i % CPR);
      const uint32_t off = row_off(tb, row, v0, a.xsn, a.xsw);
      r[k] = bload16(rs, c < a.cin ? off + 2 * c : OOB);
    }
    if constexpr (BNB) {
      const Rsrc rq_ = rsrc_at(reinterpret_cast<const H*>(a.qx) + (int64_t)tb.n0 * a.qsn);
#pragma unroll
      for (int k = 0; k < NCK; ++k) {
        const int i = ln + 64 * k, row = i / CPR, c = 8 * (i % CPR);
        const uint32_t off = row_off(tb, row, v0, a.qsn, a.qsw);
        rq[k] = bload16(rq_, c < a.cin ? off + 2 * c : OOB);
      }
    }
  };
  auto put = [&](int tile, const uint4 (&r)[NCK], const uint4 (&rq)[NQK]) __attribute__((always_inline)) {
    int ln = lane;
    asm volatile("" : "+v"(ln));
    if constexpr (BNB) {
      const int v0 = tile * ROWS;
      const TileBase tb = tile_base(v0, a.fd);
      const Rsrc ro = rsrc_at(reinterpret_cast<H*>(a.xo) + (int64_t)tb.n0 * a.osn);
      const uint32_t qb = lds_addr(lq);
#pragma unroll
      for (int k = 0; k < NCK; ++k) {
        const int i = ln + 64 * k, row = i / CPR, c = i % CPR;
        float g[8], f[8], o[8], sh[8], k1[8], k2[8], k3[8];
        Chunk<H>::unpack(r[k], g);
        Chunk<H>::unpack(rq[k], f);
        const uint32_t qa = qb + c * 32;
        *reinterpret_cast<float4*>(sh) = lds_ldf4(qa);
        *reinterpret_cast<float4*>(sh + 4) = lds_ldf4(qa + 16);
        *reinterpret_cast<float4*>(k1) = lds_ldf4(qa + CIP * 4);
        *reinterpret_cast<float4*>(k1 + 4) = lds_ldf4(qa + CIP * 4 + 16);
        *reinterpret_cast<float4*>(k2) = lds_ldf4(qa + CIP * 8);
        *reinterpret_cast<float4*>(k2 + 4) = lds_ldf4(qa + CIP * 8 + 16);
        *reinterpret_cast<float4*>(k3) = lds_ldf4(qa + CIP * 12);
        *reinterpret_cast<float4*>(k3 + 4) = lds_ldf4(qa + CIP * 12 + 16);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float dy = fmaf(f[e], k1[e], sh[e]) > 0.f ? g[e] : 0.f;
          o[e] = fmaf(k1[e], dy, fmaf(k2[e], f[e], k3[e]));
        }
        const uint4 v = Chunk<H>::pack(o);
        *reinterpret_cast<uint4*>(buf + row * RS + c * 16) = v;
        const uint32_t off = row_off(tb, row, v0, a.osn, a.osw);
        bstore16<PW_NT>(ro, 8 * c < a.cin ? off + 16 * c : OOB, v);
      }
    } else {
#pragma unroll
      for (int k = 0; k < NCK; ++k) {
        const int i = ln + 64 * k, row = i / CPR, c = i % CPR;
        *reinterpret_cast<uint4*>(buf + row * RS + c * 16) = r[k];
      }
    }
  };

  constexpr int EIN_NOK = ROWS * (COP / 8) / 64;  // store-pass row chunks per lane
  // EIN forms: 1 = generic (runtime flags: mask, accumulate, PBWD on the
  // channels >= pm_lo); compile-time and branch-free: EIN_ACC (accumulate),
  // EIN_PB (PBWD), EIN_PBACC (both).  The generic store pass carried ~3.5 K
  // extra instructions per tile (divergent per-chunk branches): 2.2x the plain
  // kernel's time at DRF's 64 -> 256 data gradients.
  const bool f_mask = EIN == 1 ? a.has_mask != 0 : false;
  const bool f_acc = EIN == 1 ? a.accumulate != 0 : (EIN == EIN_ACC || EIN == EIN_PBACC);
  const bool f_pb = EIN == 1 ? a.pbwd != 0 : (EIN == EIN_PB || EIN == EIN_PBACC);
  // Store-pass chunk k of a lane: row-major (2 rows of every column per k),
  // or, in the compile-time forms with whole 64-channel column groups, 8 rows
  // x one 64-channel group per k -- so "is this chunk on the PReLU tail" is
  // the same for the whole wave and the tail work is a scalar branch
  constexpr int OCPR_ = COP / 8;
  constexpr bool BLK = EIN >= 2 && OCPR_ % 8 == 0;
  constexpr int NGRP = OCPR_ / 8;
  auto chunk_rc = [&](int ln, int k, int& row, int& c) __attribute__((always_inline)) {
    if constexpr (BLK) {
      row = 8 * (k / NGRP) + (ln >> 3);
      c = 8 * (8 * (k % NGRP) + (ln & 7));
    } else {
      const int i = ln + 64 * k;
      row = i / OCPR_;
      c = 8 * (i % OCPR_);
    }
  };
  auto on_tail = [&](int k, int c) __attribute__((always_inline)) {  // BLK: wave-uniform
    return BLK ? co0 + 64 * (k % NGRP) >= a.pm_lo : co0 + c >= a.pm_lo;
  };
  auto ein_load = [&](int tile, uint4 (&em)[EIN ? EIN_NOK : 1], uint4 (&ey)[EIN ? EIN_NOK : 1])
                      __attribute__((always_inline)) {
    if constexpr (EIN) {
      constexpr int OCPR = COP / 8;
      int ln = lane;
      asm volatile("" : "+v"(ln));
      const int v0 = tile * ROWS;
      const TileBase tb = tile_base(v0, a.fd);
      const Rsrc ry = rsrc_at(aY + (int64_t)tb.n0 * a.ysn);
      const Rsrc rm = rsrc_at(reinterpret_cast<const H*>(a.msk ? a.msk : a.y) + (int64_t)tb.n0 * a.msn);
#pragma unroll
      for (int k = 0; k < EIN_NOK; ++k) {
        int row, c;
        chunk_rc(ln, k, row, c);
        const bool ok = co0 + c < a.cout;
        if (EIN == 1) {
          if (f_mask || (f_pb && co0 + c >= a.pm_lo))
            em[k] = bload16(rm, ok ? row_off(tb, row, v0, a.msn, a.msw) + 2 * (co0 + c) : OOB);
        } else if (f_pb) {
          if (BLK) {
            if (on_tail(k, c)) em[k] = bload16(rm, ok ? row_off(tb, row, v0, a.msn, a.msw) + 2 * (co0 + c) : OOB);
          } else {  // branch-free: chunks below pm_lo read nothing (out-of-range offset) and see m = 0
            em[k] = bload16(rm, ok && on_tail(k, c) ? row_off(tb, row, v0, a.msn, a.msw) + 2 * (co0 + c) : OOB);
          }
        }
        if (f_acc) ey[k] = bload16(ry, ok ? row_off(tb, row, v0, a.ysn, a.ysw) + 2 * (co0 + c) : OOB);
      }
    }
  };
  uint4 rg[NCK], rgq[NQK];
  int t = blockIdx.x * (PW_THR / 64) + wv;
  if (t < a.ntiles) load(t, rg, rgq);
  while (t < a.ntiles) {
    const int tn = t + nwaves;
    put(t, rg, rgq);
    // RED 2: the BN input rows of this tile's reduce, issued before the next
    // tile's operands so the epilogue's wait on them leaves those in flight
    uint4 bx[RED == 2 ? RNIT : 1];
    const bool lane_ok = lane < ROCPR * RSTEP;
    auto load_bx = [&]() __attribute__((always_inline)) {
      const int v0 = t * ROWS;
      const TileBase tb = tile_base(v0, a.fd);
      const Rsrc rb = rsrc_at(reinterpret_cast<const H*>(a.bnx) + (int64_t)tb.n0 * a.bsn);
#pragma unroll
      for (int j = 0; j < RNIT; ++j) {
        const int row = rrow0 + RSTEP * j;
        const bool ok = lane_ok && row < ROWS && rch_ok;
        bx[j] = bload16(rb, ok ? row_off(tb, row, v0, a.bsn, a.bsw) + 2 * (co0 + 8 * rcol) : OOB);
      }
    };
    if constexpr (RED == 2) load_bx();
    if (tn < a.ntiles) load(tn, rg, rgq);  // in flight during this tile's MFMAs and stores
    // EIN: the store pass's mask / accumulate operands of this tile, issued
    // before its MFMAs so their latency hides under them; issued
    // at the store pass they made an accumulate data gradient 2.2x the plain one
    // (DRF 64 -> 256 at 512^2: 312 vs 143 us, r5 tools/diag/pw_pbwd_micro.py)
    uint4 em[EIN ? EIN_NOK : 1], ey[EIN ? EIN_NOK : 1];
    if constexpr (EIN) ein_load(t, em, ey);

    f32x16 acc[M][NCB];
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[m][cb][i] = 0.f;
    // k-step s+1's fragments (and prologue constants) are read while step s's MFMAs run
    struct Frag {
      uint4 a[NCB], b[M];
      float4 s0, s1, h0, h1;
    };
    // LDS byte addresses from opaque per-tile bases: the compiler would otherwise
    // hoist one VGPR per (k-step, block) address out of the tile loop (offsets
    // past the 64 KiB immediate range) and starve the fragment pipeline
    uint32_t abase = lds_addr(lw) + (hf * COP + col) * 16;
    uint32_t bbase = lds_addr(buf) + col * RS + hf * 16;
    asm volatile("" : "+v"(abase), "+v"(bbase));
    auto rd = [&](int s, Frag& f) __attribute__((always_inline)) {
#pragma unroll
      for (int m = 0; m < M; ++m) f.b[m] = lds_ld16(bbase + m * 32 * RS + 32 * s);
      const uint32_t as = abase + s * 2 * COP * 16;
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) f.a[cb] = lds_ld16(as + cb * 32 * 16);
      if (PRO) {
        const int c = 16 * s + 8 * hf;
        f.s0 = *reinterpret_cast<const float4*>(lsc + c);
        f.s1 = *reinterpret_cast<const float4*>(lsc + c + 4);
        f.h0 = *reinterpret_cast<const float4*>(lsh + c);
        f.h1 = *reinterpret_cast<const float4*>(lsh + c + 4);
      }
    };
    Frag fr[2];
    rd(0, fr[0]);
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      Frag& f = fr[s & 1];
      if (s + 1 < KS) rd(s + 1, fr[(s + 1) & 1]);
      if (PRO) {
#pragma unroll
        for (int m = 0; m < M; ++m) f.b[m] = h8_affine<H>(f.b[m], f.s0, f.s1, f.h0, f.h1, relu_in);
      }
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int m = 0; m < M; ++m) mma<H>(acc[m][cb], f.a[cb], f.b[m]);
    }

    // epilogue into the buffer (row = voxel, COP H channels), then row stores
    {
      uint32_t ebase = lds_addr(buf) + col * RS + hf * 8;
      uint32_t bias_b = lds_addr(lb) + hf * 16;
      asm volatile("" : "+v"(ebase), "+v"(bias_b));
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float4 bb = make_float4(0.f, 0.f, 0.f, 0.f);
          if constexpr (!BNB) bb = lds_ldf4(bias_b + (cb * 32 + 8 * j) * 4);
#pragma unroll
          for (int m = 0; m < M; ++m) {
            float o[4] = {acc[m][cb][4 * j] + bb.x, acc[m][cb][4 * j + 1] + bb.y, acc[m][cb][4 * j + 2] + bb.z,
                          acc[m][cb][4 * j + 3] + bb.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              o[e] *= osc;
              if constexpr (ACT == VSRK_ACT_RELU) o[e] = fmaxf(o[e], 0.f);
              if constexpr (ACT == VSRK_ACT_PRELU) o[e] = o[e] > 0.f ? o[e] : pslope * o[e];
            }
            lds_st8(ebase + m * 32 * RS + (cb * 32 + 8 * j) * 2, pack_pk<H, uint2>(o));
          }
        }
    }
    if constexpr (RED != 0) {
      // reduce form of the store pass: lane l keeps ONE 8-channel column
      // (l % OCPR) and walks rows l / OCPR + RSTEP j, so its partial sums
      // are per channel; the lanes past OCPR * RSTEP idle
      const int v0 = t * ROWS;
      const TileBase tb = tile_base(v0, a.fd);
      const Rsrc ry = rsrc_at(aY + (int64_t)tb.n0 * a.ysn);
#pragma unroll
      for (int j = 0; j < RNIT; ++j) {
        const int row = rrow0 + RSTEP * j;
        if (lane_ok && row < ROWS) {
          const uint4 v = *reinterpret_cast<const uint4*>(buf + row * RS + 16 * rcol);
          const uint32_t off = row_off(tb, row, v0, a.ysn, a.ysw);
          const bool vox_ok = AL || v0 + row < a.nvox;
          bstore16<PW_NT>(ry, rch_ok ? off + 2 * (co0 + 8 * rcol) : OOB, v);
          if (vox_ok && rch_ok) {
            float o[8];
            Chunk<H>::unpack(v, o);  // the stored (rounded) values, as the separate pass reads them
            if constexpr (RED == 1) {
#pragma unroll
              for (int e = 0; e < 8; ++e) {
                rs1[e] += o[e];
                rs2[e] = fmaf(o[e], o[e], rs2[e]);
              }
            } else {
              float xb[8];
              Chunk<H>::unpack(bx[j], xb);
#pragma unroll
              for (int e = 0; e < 8; ++e) {
                const float dy = fmaf(xb[e], rsc[e], rsh[e]) > 0.f ? o[e] : 0.f;
                rs1[e] += dy;
                rs2[e] = fmaf(dy, (xb[e] - rmu[e]) * ris[e], rs2[e]);
              }
            }
          }
        }
      }
    } else {
      const int v0 = t * ROWS;
      const TileBase tb = tile_base(v0, a.fd);
      const Rsrc ry = rsrc_at(aY + (int64_t)tb.n0 * a.ysn);
      constexpr int OCPR = COP / 8;
      constexpr int NOK = ROWS * OCPR / 64;
      static_assert(NOK >= 1 && ROWS * OCPR % 64 == 0, "whole row chunks per lane");
      int ln = lane;
      asm volatile("" : "+v"(ln));
      const float mslope = (EIN && a.mask_slope) ? *a.mask_slope : 0.f;
#pragma unroll
      for (int k = 0; k < NOK; ++k) {
        int row, c;
        chunk_rc(ln, k, row, c);
        uint4 v = *reinterpret_cast<const uint4*>(buf + row * RS + c * 2);
        if constexpr (EIN) {
          float o[8];
          Chunk<H>::unpack(v, o);
          if (f_mask) {
            float m[8];
            Chunk<H>::unpack(em[k], m);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = mask_apply(m[e], o[e], mslope);
          }
          if (f_acc) {
            float yo[8];
            Chunk<H>::unpack(ey[k], yo);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] += yo[e];
          }
          v = Chunk<H>::pack(o);
          if (EIN != 1 && f_pb && (!BLK || on_tail(k, c))) {
            const bool tail = BLK || on_tail(k, c);
            float m[8], tr[8];
            Chunk<H>::unpack(em[k], m);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (tail && !(m[e] > 0.f)) ? mslope * o[e] : o[e];
            v = Chunk<H>::pack(o);
            Chunk<H>::unpack(v, tr);  // the stored (rounded) values, as prelu_bwd reads them
#pragma unroll
            for (int e = 0; e < 8; ++e) sacc = fmaf(m[e] < 0.f ? tr[e] : 0.f, m[e], sacc);  // m = 0 off the tail
          } else if (f_pb && co0 + c >= a.pm_lo) {
            float m[8];
            Chunk<H>::unpack(em[k], m);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = m[e] > 0.f ? o[e] : mslope * o[e];
            v = Chunk<H>::pack(o);
            float tr[8];
            Chunk<H>::unpack(v, tr);  // the stored (rounded) values, as prelu_bwd reads them
            // (out-of-range rows load zeros: m = 0 adds nothing)
#pragma unroll
            for (int e = 0; e < 8; ++e)
              if (m[e] < 0.f) sacc = fmaf(tr[e], m[e], sacc);
          }
        }
        const uint32_t off = row_off(tb, row, v0, a.ysn, a.ysw);
        bstore16<PW_NT>(ry, co0 + c < a.cout ? off + 2 * (co0 + c) : OOB, v);
      }
    }
    t = tn;
  }
  if constexpr (EIN) {
    if (f_pb) {
      const double wsum = vsrk_wave_sum((double)sacc);
      if (lane == 0) a.slope_part[(blockIdx.y * gridDim.x + blockIdx.x) * (PW_THR / 64) + wave] = wsum;
      return;
    }
  }
  if constexpr (RED != 0) {
    float* o = a.red_ws + ((((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (PW_THR / 64) + wave) * 64 + lane) * 16;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      o[e] = rs1[e];
      o[8 + e] = rs2[e];
    }
  }
}

// NCO dY channel blocks per chunk; NW waves (4 or 8), wave w owns X block w
// of the chunk's <= NW.  NW = 8 takes the wide chunks (5-8 X blocks): one
// pass over dY at 160-256 channels with one block per wave (the plan's
// comment in conv_pw.hip has the measurements, profiles/r4_pw_wgrad_ci8_ab.txt).
// Two register-staged stages in flight (stage s in register set s & 1).  A
// stage is 64 voxels, a few microseconds of HBM latency against well under
// one of MFMA work at these channel counts, so with one stage in flight the
// workgroup waited on its loads (2.4-3 TB/s at 160-224 channels; the first
// two-stage trial is profiles/r2e_pw_wgrad_prefetch2_microbench.txt).
template <int NCO, typename H, int NW = 4>
__global__ __launch_bounds__(NW * 64, 1) void pw_wgrad_kernel(PwWArgs a) {
  const H* aX = reinterpret_cast<const H*>(a.x);
  const H* aD = reinterpret_cast<const H*>(a.dy);
  constexpr int THR = NW * 64;
  constexpr int DK = (PW_KP * 4 * NCO + THR - 1) / THR;     // dY pieces per thread
  constexpr int XK = (PW_KP * 4 * NW + THR - 1) / THR;  // X pieces per thread (max)
  constexpr int PLMAX = NCO + NW;       // 32-channel planes per stage (max)
  constexpr int PSZ = PW_KP * 64;       // bytes per plane: 64 voxel rows of 32 H
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int split = blockIdx.x, chunk = blockIdx.y;
  const int co_chunk = chunk / a.ci_chunks, ci_chunk = chunk - co_chunk * a.ci_chunks;
  const int co0 = co_chunk * 32 * NCO, ci0 = ci_chunk * 32 * a.ncit;
  const int vbeg = split * a.vox_per_split;
  const int vend = min(a.nvox, vbeg + a.vox_per_split);
  const int nst = vend > vbeg ? (vend - vbeg + PW_KP - 1) / PW_KP : 0;
  const bool relu_in = (a.prologue & VSRK_PRO_RELU) != 0;
  const bool aff = (a.prologue & VSRK_PRO_AFFINE) != 0;
  const bool do_bias = a.want_bias && ci_chunk == 0 && wave == 0;

  // Per-thread chunk roles, fixed for the whole loop: dY piece k (i < 256 NCO)
  // and X piece k (i < 256 ncit) are 16-byte pieces i = tid + THR k of the
  // stage's [voxel][plane][4 x 16 B] image; every load instruction reads one
  // tensor.  (Piece validity is wave-uniform: the bounds are multiples of 256.)
  int dvox[DK], dch[DK], dlds[DK];
#pragma unroll
  for (int k = 0; k < DK; ++k) {
    const int i = tid + k * THR;
    const int vox = i / (4 * NCO), within = i - vox * (4 * NCO);
    const int plane = within >> 2, q = within & 3;
    dvox[k] = vox;
    const int c = co0 + plane * 32 + q * 8;
    dch[k] = (i < PW_KP * 4 * NCO && c < a.cout) ? 2 * c : -1;
    dlds[k] = i < PW_KP * 4 * NCO ? plane * PSZ + vox * 64 + q * 16 : -1;
  }
  int xvox[XK], xch[XK], xlds[XK];
  const int nxc = 4 * a.ncit;
#pragma unroll
  for (int k = 0; k < XK; ++k) {
    const int i = tid + k * THR;
    const int vox = i / nxc, within = i - vox * nxc;
    const int plane = within >> 2, q = within & 3;
    xvox[k] = vox;
    const int c = ci0 + plane * 32 + q * 8;
    const bool ok = i < PW_KP * nxc;
    xch[k] = (ok && c < a.cin) ? 2 * c : -1;
    xlds[k] = ok ? (NCO + plane) * PSZ + vox * 64 + q * 16 : -1;
  }

  uint4 ry[2][DK], rx[2][XK];
  auto issue = [&](int st, auto S) __attribute__((always_inline)) {
    constexpr int R = decltype(S)::value;
    const int v0 = vbeg + st * PW_KP;
    const TileBase tb = tile_base(v0, a.fd);
    const Rsrc rdy = rsrc_at(aD + (int64_t)tb.n0 * a.dsn);
    const Rsrc rxx = rsrc_at(aX + (int64_t)tb.n0 * a.xsn);
#pragma unroll
    for (int k = 0; k < DK; ++k) {
      const uint32_t off = lane_off(tb, dvox[k], v0 + dvox[k], vend, a.fd, a.dsn, a.dsw);
      ry[R][k] = bload16(rdy, dch[k] >= 0 ? off + dch[k] : OOB);
    }
#pragma unroll
    for (int k = 0; k < XK; ++k) {
      if (xlds[k] >= 0) {
        const uint32_t off = lane_off(tb, xvox[k], v0 + xvox[k], vend, a.fd, a.xsn, a.xsw);
        rx[R][k] = bload16(rxx, xch[k] >= 0 ? off + xch[k] : OOB);
      }
    }
  };
  auto commit = [&](int buf, auto S) __attribute__((always_inline)) {
    constexpr int R = decltype(S)::value;
    char* base = lds + buf * (PLMAX * PSZ);
#pragma unroll
    for (int k = 0; k < DK; ++k)
      if (DK * THR == PW_KP * 4 * NCO || dlds[k] >= 0) *reinterpret_cast<uint4*>(base + dlds[k]) = ry[R][k];
#pragma unroll
    for (int k = 0; k < XK; ++k)
      if (xlds[k] >= 0) *reinterpret_cast<uint4*>(base + xlds[k]) = rx[R][k];
  };
  const std::integral_constant<int, 0> I0{};
  const std::integral_constant<int, 1> I1{};

  // prologue scale/shift of the lane's X channel in the wave's block
  // (kept as the one-trip loop it was when a wave could own several blocks:
  // as straight-line code the compiler places the two loads elsewhere and the
  // whole kernel is scheduled differently, 30-130 instructions apart)
  float psc, psh;
#pragma unroll
  for (int once = 0; once < 1; ++once) {
    const int c = ci0 + wave * 32 + (lane & 31);
    const bool ok = c < a.cin;
    psc = ok ? (aff ? a.pro_scale[c] : 1.f) : 0.f;
    psh = ok ? (aff ? a.pro_shift[c] : 0.f) : 0.f;
  }

  f32x16 acc[NCO];
#pragma unroll
  for (int i = 0; i < NCO; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
  float bsum[NCO];
#pragma unroll
  for (int i = 0; i < NCO; ++i) bsum[i] = 0.f;

  // ds_read_b64_tr_b16: group g = lane>>4 reads a 4-voxel x 16-channel block;
  // lane 4q+p addresses voxel row q, channels 4p..4p+3, and receives channel
  // lane&15 of the group's 16: lane l ends up with channel l&31 of the plane
  // for voxels 8*(l>>5) .. +7 of the k-step.
  const int g = lane >> 4, i16 = lane & 15, q = i16 >> 2, p = i16 & 3;
  const int colb = ((g & 1) * 16 + 4 * p) * 2;
  const int rowk = 8 * (g >> 1) + q;

  auto compute = [&](int buf) __attribute__((always_inline)) {
    const char* base = lds + buf * (PLMAX * PSZ);
#pragma unroll
    for (int kk = 0; kk < PW_KP / 16; ++kk) {
      const int row = kk * 16 + rowk;
      uint4 bfr;
      if (wave < a.ncit) {
        const char* px = base + (NCO + wave) * PSZ + row * 64 + colb;
        const v4i16 x0 = ds_read_tr(px), x1 = ds_read_tr(px + 4 * 64);
        uint4 xv = __builtin_bit_cast(uint4, __builtin_shufflevector(x0, x1, 0, 1, 2, 3, 4, 5, 6, 7));
        if (a.prologue) {
          float f[8];
          Chunk<H>::unpack(xv, f);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float tt = fmaf(f[e], psc, psh);
            f[e] = relu_in ? fmaxf(tt, 0.f) : tt;
          }
          xv = Chunk<H>::pack(f);
        }
        bfr = xv;
      }
#pragma unroll
      for (int cb = 0; cb < NCO; ++cb) {
        const char* py = base + cb * PSZ + row * 64 + colb;
        const v4i16 y0 = ds_read_tr(py), y1 = ds_read_tr(py + 4 * 64);
        const uint4 af = __builtin_bit_cast(uint4, __builtin_shufflevector(y0, y1, 0, 1, 2, 3, 4, 5, 6, 7));
        if (do_bias) {
          float fa[8];
          Chunk<H>::unpack(af, fa);
#pragma unroll
          for (int e = 0; e < 8; ++e) bsum[cb] += fa[e];
        }
        if (wave < a.ncit) mma<H>(acc[cb], af, bfr);
      }
    }
  };

  // stage s lives in register set s & 1 and LDS buffer s & 1.  Issues run
  // past the end unconditionally (every voxel out of range: zero loads, no
  // memory traffic), so the compiler's in-order vmcnt waits stay exact.
  if (nst > 0) {
    issue(0, I0);
    issue(1, I1);
    commit(0, I0);
    __syncthreads();
    issue(2, I0);
    for (int st = 0; st < nst; st += 2) {
      compute(0);
      commit(1, I1);  // stage st + 1
      __syncthreads();
      issue(st + 3, I1);
      if (st + 1 >= nst) break;
      compute(1);
      commit(0, I0);  // stage st + 2
      __syncthreads();
      issue(st + 4, I0);
    }
  }

  // slab: [co (32*NCO)][ci (32*ncit)] then dbias[32*NCO]
  const int cic = 32 * a.ncit;
  float* out = a.ws + ((int64_t)split * a.nchunks + chunk) * a.slab;
  const int hf = lane >> 5, col = lane & 31;
#pragma unroll
  for (int cb = 0; cb < NCO; ++cb)
    if (wave < a.ncit) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int co = cb * 32 + 8 * (e >> 2) + 4 * hf + (e & 3);
        out[co * cic + wave * 32 + col] = acc[cb][e];
      }
    }
  if (a.want_bias && ci_chunk == 0 && wave == 0) {
#pragma unroll
    for (int cb = 0; cb < NCO; ++cb) {
      const float tot = bsum[cb] + __shfl_xor(bsum[cb], 32);
      if (hf == 0) out[32 * NCO * cic + cb * 32 + col] = tot;
    }
  }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
// A form of the staged kernel, its AL variant chosen by the tile alignment
template <int NCB, int NKB, int M, bool PRO, int ACT, int EIN, typename H, int RED = 0, bool BNB = false>
auto pw_staged_al(bool al) -> void (*)(PwArgs) {
  return al ? pw_fwd_staged_kernel<NCB, NKB, M, PRO, true, ACT, EIN, H, RED, BNB>
            : pw_fwd_staged_kernel<NCB, NKB, M, PRO, false, ACT, EIN, H, RED, BNB>;
}

// Staged launch (LDS row buffers) of (NCB output blocks, NKB input blocks);
// false when the output is not 8-channel aligned or the kernel has no such form.
template <int NCB, int NKB, typename H>
bool launch_fwd_staged(const PwArgs& a, int grid, int nchunk, hipStream_t s) {
  constexpr int M = pw_tile_m(NCB, NKB);
  constexpr int KS = 2 * NKB, COP = 32 * NCB, CIP = 16 * KS;
  if (a.cout % 8 != 0) return false;
  const bool pro = a.prologue != VSRK_PRO_NONE;
  const bool ein = a.has_mask || a.accumulate || a.pbwd;
  if (ein && (pro || a.act != VSRK_ACT_NONE)) return false;  // data gradients: no prologue / activation
  if (pro && a.act == VSRK_ACT_PRELU) return false;
  constexpr int RW = CIP > COP ? CIP : COP;
  const size_t lds = (size_t)KS * 2 * COP * 16 + (pro ? 2 * CIP * 4 : 0) + COP * 4 + 4 * (32 * M) * (2 * RW + 16);
  const bool al = a.dhw % (32 * M) == 0;
  const bool relu = a.act == VSRK_ACT_RELU;
  void (*kern)(PwArgs);
  if (ein) {
    kern = pw_staged_al<NCB, NKB, M, false, 0, EIN_GEN, H>(al);
    if constexpr (NKB == 2) {  // DRF's 64-input-channel data gradients: the branch-free forms
      // (with whole 64-channel store groups (COP % 64 == 0) the PReLU tail is
      // decided per group, so it must start on a group boundary; any other
      // c_lo -- e.g. num_features 48: c_lo = 144 of 192 -- takes the generic
      // per-chunk form)
      constexpr bool GROUPED = (COP / 8) % 8 == 0;
      const bool tail_ok = !a.pbwd || !GROUPED || a.pm_lo % 64 == 0;
      if (!a.has_mask && (a.accumulate || a.pbwd) && tail_ok)
        kern = !a.pbwd        ? pw_staged_al<NCB, NKB, M, false, 0, EIN_ACC, H>(al)
               : a.accumulate ? pw_staged_al<NCB, NKB, M, false, 0, EIN_PBACC, H>(al)
                              : pw_staged_al<NCB, NKB, M, false, 0, EIN_PB, H>(al);
    }
  } else if (a.act == VSRK_ACT_PRELU) {
    kern = pw_staged_al<NCB, NKB, M, false, VSRK_ACT_PRELU, 0, H>(al);
  } else if (pro) {
    kern = relu ? pw_staged_al<NCB, NKB, M, true, 1, 0, H>(al) : pw_staged_al<NCB, NKB, M, true, 0, 0, H>(al);
  } else {
    kern = relu ? pw_staged_al<NCB, NKB, M, false, 1, 0, H>(al) : pw_staged_al<NCB, NKB, M, false, 0, 0, H>(al);
  }
  (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  kern<<<dim3(grid, nchunk), PW_THR, lds, s>>>(a);
  return true;
}
template <int NCB, int NKB>
bool launch_fwd_staged16(int dtype, const PwArgs& a, int grid, int nchunk, hipStream_t s) {
  return vsrk_dispatch16(dtype, [&](auto tag) { return launch_fwd_staged<NCB, NKB, decltype(tag)>(a, grid, nchunk, s); });
}

// Staged launch with the fused per-channel reduction (square f -> f convs,
// one output chunk): RED 1 with the BN prologue (a BatchNorm's input
// statistics, duf_net.py:198-201), RED 2 without (the data gradient that
// feeds a BN+ReLU backward, duf_net.py:198-200).
template <int NCB, int RED, typename H, bool BNB = false>
void launch_fwd_reduce(const PwArgs& a, int grid, hipStream_t s) {
  constexpr int M = pw_tile_m(NCB, NCB);
  constexpr int KS = 2 * NCB, COP = 32 * NCB, CIP = 16 * KS;
  const size_t lds = (size_t)KS * 2 * COP * 16 + (RED == 1 ? 2 * CIP * 4 : 0) + (BNB ? 4 * CIP * 4 : COP * 4) +
                     4 * (32 * M) * (2 * CIP + 16);
  auto kern = pw_staged_al<NCB, NCB, M, RED == 1, 0, 0, H, RED, BNB>(a.dhw % (32 * M) == 0);
  (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  kern<<<dim3(grid, 1), PW_THR, lds, s>>>(a);
}

template <int NCO, typename H, int NW>
void launch_wgrad_pw(const PwWArgs& a, int nsplit, hipStream_t s) {
  const size_t lds = (size_t)2 * (NCO + NW) * PW_KP * 64;
  auto kern = pw_wgrad_kernel<NCO, H, NW>;
  (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  kern<<<dim3(nsplit, a.nchunks), NW * 64, lds, s>>>(a);
}
}  // namespace
