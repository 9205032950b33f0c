// What the row-walking convs share (conv_row.hip: 64 -> 64; conv_row_wide.hip:
// 64 -> 256 through a shuffle-2 output view): the segment / ring geometry,
// the LDS image of an input row and its swizzle, the register staging of a
// row (two rows in flight), the register transpose of a finished accumulator
// bank, the view struct and the host's view checks and band / grid choice.
// conv_row.hip's header comment describes the walk.
#pragma once
#include "conv_common.h"

namespace vsrk_conv {

constexpr int CR_NW = 8;                       // waves
constexpr int CR_SEG = 128;                    // output columns per segment
constexpr int CR_SLOT = (CR_SEG + 2) * 128;    // 16,640 B: columns -1 .. 128 of one input row
constexpr int CR_NSLOT = 4;
constexpr int CR_MINBAND = 4;                  // rows: a band pays 2 halo rows and the weight load
constexpr uint32_t CR_OOB = 0x80000000u;       // buffer offset past the range: loads read zero, stores are dropped

typedef rawbuf::Rsrc CrRsrc;
typedef int cr_v4i __attribute__((ext_vector_type(4)));
// byte offset = voff (per lane; CR_OOB: out of range) + soff (wave-uniform,
// < 2^31: the row and the q-th voxel group, so a lane keeps one offset per view)
__device__ __forceinline__ uint4 cr_load16(CrRsrc r, uint32_t voff, uint32_t soff) {
  return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0));
}
// A store keeps its whole offset in the VGPR: with a register in the scalar
// offset field the compiler assumes that a 16-byte store has read its data by
// the time the next VALU instruction overwrites the data registers, and pads
// nothing -- on gfx950 the store can still be reading them (seen in some
// launches only: one dword of the 16 bytes, in the last four lanes of each
// 16-lane row, took the next voxel group's value).  Without a scalar offset
// the compiler inserts the wait states of that hazard itself.
__device__ __forceinline__ void cr_store16(CrRsrc r, uint32_t voff, uint4 v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(cr_v4i, v), r, (int)voff, 0, 0);
}

// a view of (images, H, W, channels): element strides (the host checks that
// every byte offset inside one image fits the buffer range)
struct CrView {
  const char* ptr;
  int64_t sn, sd;
  int sh, sw;
};

// ---- LDS image of a row: voxel lv at lv * 128 B, its 16-byte piece p in
// position p ^ ((lv >> 1) & 7) ----
// voxel fragment of chunk c (piece 2 c + hf) of voxel lv: byte offset
// cr_frag_base + ((c ^ cr_frag_swz) << 5) of the slot
__device__ __forceinline__ uint32_t cr_frag_base(int lv, int hf) {
  const int sz = (lv >> 1) & 7;
  return (uint32_t)(lv * 128 + ((hf ^ (sz & 1)) << 4));
}
__device__ __forceinline__ uint32_t cr_frag_swz(int lv) {
  const int sz = (lv >> 1) & 7;
  return (uint32_t)(sz >> 1);
}
// staging write of piece sp of segment column col (-1 and CR_SEG: the halo
// columns).  A macro on purpose: as a function the compiler simplifies the
// expression on its own before inlining it, and conv_row_kernel's schedule
// and register allocation come out different from the measured ones.
#define CR_STAGE_DST(col, sp) ((uint32_t)(((col) + 1) * 128 + (((sp) ^ ((((col) + 1) >> 1) & 7)) << 4)))

// Input row `row` into a register set: columns c0 + scol + 64 q (q = 0, 1;
// xcolb: the lane's byte offset at q = 0) and, with a halo, the lane's halo
// column (hcolb); zero outside the image (xok: the columns' validity), above
// it, below it or past the band's last halo row r1.  A closure over the
// kernel's arguments (x, H) and the item's values, what the lambda it
// replaces was (a plain function compiles conv_row_kernel differently).
template <bool HALO, typename Args>
struct CrLoadRow {
  const Args& a;
  const int& r1;
  const bool (&xok)[3];
  const uint32_t& xcolb;
  const CrRsrc& rx;
  const uint32_t& hcolb;
  __device__ __forceinline__ void operator()(int row, uint4 (&st)[HALO ? 3 : 2]) const {
    const bool rv = row >= 0 && row < a.H && row <= r1;
    const uint32_t rb = rv ? 2u * (uint32_t)(row * a.x.sh) : 0u;
#pragma unroll
    for (int q = 0; q < 2; ++q) st[q] = cr_load16(rx, (rv && xok[q]) ? xcolb : CR_OOB, rb + 2u * (uint32_t)(64 * q * a.x.sw));
    if constexpr (HALO) st[2] = cr_load16(rx, (rv && xok[2]) ? hcolb : CR_OOB, rb);
  }
};
// ... and from the register set into ring slot `sl`
template <bool HALO>
__device__ __forceinline__ void cr_write_row(char* sl, const uint4 (&st)[HALO ? 3 : 2], uint32_t sdst, uint32_t hdst,
                                             bool halo_lane) {
#pragma unroll
  for (int q = 0; q < 2; ++q) *reinterpret_cast<uint4*>(sl + sdst + q * 64 * 128) = st[q];
  if constexpr (HALO) {
    if (halo_lane) *reinterpret_cast<uint4*>(sl + hdst) = st[2];
  }
}

// Register transpose of a finished 32 x 32 bank.  Lane (r, hf) holds voxel r,
// channels 8 g + 4 hf + i in register 4 g + i; the swaps leave it chunk
// 2 (r >> 4) + hf of voxels (r & 15) + 16 q in registers 8 q .. + 7 (see
// conv_roll_impl.h, epilogue_sw).
__device__ __forceinline__ void cr_transpose(const f32x16& A, float (&v)[16]) {
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = A[i];
#pragma unroll
  for (int g = 0; g < 4; g += 2) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const auto sw = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(uint32_t, v[4 * g + i]),
                                                       __builtin_bit_cast(uint32_t, v[4 * g + 4 + i]), false, false);
      v[4 * g + i] = __builtin_bit_cast(float, (uint32_t)sw[0]);
      v[4 * g + 4 + i] = __builtin_bit_cast(float, (uint32_t)sw[1]);
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const auto sw = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(uint32_t, v[e]),
                                                     __builtin_bit_cast(uint32_t, v[8 + e]), false, false);
    v[e] = __builtin_bit_cast(float, (uint32_t)sw[0]);
    v[8 + e] = __builtin_bit_cast(float, (uint32_t)sw[1]);
  }
}

// ---- host side ----
static inline CrView cr_view(const vsrk_tensor5* t) {
  CrView v;
  v.ptr = (const char*)t->ptr;
  v.sn = t->sn; v.sd = t->sd; v.sh = (int)t->sh; v.sw = (int)t->sw;
  return v;
}
// every byte offset inside one image of ph x pw physical voxels of 64
// channels fits the buffer range (exact reads: no over-read margin)
static inline bool cr_view_fits(const vsrk_tensor5* t, int64_t ph, int64_t pw) {
  const int64_t span = (ph - 1) * t->sh + (pw - 1) * t->sw + 64;
  if (t->sn < 0 || t->sd < 0 || t->sh < 0 || t->sw < 0 || 2 * span >= 0x7FFFFFF0ll) return false;
  return t->sh < (1ll << 30) && t->sw < (1ll << 30);
}
// Items of a launch over nimg images of h x w output voxels: bands as many
// as it takes for the (capped) grid to cover the CUs.  false: too many items.
struct CrPlan {
  int nseg, nband, band_h, nitems, grid;
};
static inline bool cr_plan(int64_t nimg, int h, int w, CrPlan& p) {
  p.nseg = ceil_div(w, CR_SEG);
  const int64_t target = vsrk_capped_grid(vsrk_num_cus());
  const int64_t cols = nimg * p.nseg;
  const int64_t nb = std::max<int64_t>(1, std::min<int64_t>(ceil_div64(target, cols), h));
  p.band_h = (int)std::max<int64_t>(ceil_div64(h, nb), std::min(CR_MINBAND, h));
  p.nband = ceil_div(h, p.band_h);
  const int64_t nitems = cols * p.nband;
  if (nitems >= (1ll << 31)) return false;
  p.nitems = (int)nitems;
  p.grid = (int)vsrk_capped_grid(std::min<int64_t>(nitems, vsrk_num_cus()));
  return true;
}

}  // namespace vsrk_conv
