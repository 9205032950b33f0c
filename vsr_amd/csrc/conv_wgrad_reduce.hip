// The weight gradient's reduce: sums the fp32 slabs a slab kernel left in the
// workspace (WgradSlabs, conv_wgrad.h) into dw and dbias, in a fixed order.
#include "conv_wgrad.h"

namespace {

// dw[co][ci][kd][kh][kw] (torch, fp32) = scale * sum_split slab[split][combo][tap][co][ci]
// (+ dbias from the bias tails).  A block = 64 outputs x 4 split groups; each
// thread sums a strided quarter of the splits, then the 4 partials are added
// in a fixed order: deterministic.
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(
    const float* __restrict__ ws, float* __restrict__ dw, float* __restrict__ db, int nsplit, int ncombos,
    int slab, int cout, int cin, int kd, int kh, int kw, int nco_t, int nci_t, int cot_w, int cit_w, int kd_bias,
    int perm_r, float scale, int accumulate) {
  __shared__ float part[4][64];
  const int taps2 = kh * kw;
  const int64_t nw = (int64_t)cout * cin * kd * taps2;
  const int64_t idx = (int64_t)blockIdx.x * 64 + (threadIdx.x & 63);
  const int grp = threadIdx.x >> 6;
  const int64_t total = nw + (db ? cout : 0);
  const int64_t sstride = (int64_t)ncombos * slab;
  const float* p = nullptr;
  int co = 0, ci = 0, tap = 0, kdi = 0;
  if (idx < nw) {
    ci = idx % cin;
    int64_t t = idx / cin;
    co = t % cout;
    t /= cout;
    tap = t % taps2;
    kdi = t / taps2;
    const int combo = (kdi * nci_t + ci / cit_w) * nco_t + co / cot_w;
    p = ws + (int64_t)combo * slab + ((int64_t)tap * cot_w + (co % cot_w)) * cit_w + (ci % cit_w);
  } else if (idx < total) {
    co = (int)(idx - nw);
    const int combo = (kd_bias * nci_t + 0) * nco_t + co / cot_w;
    p = ws + (int64_t)combo * slab + (int64_t)taps2 * cot_w * cit_w + (co % cot_w);
  }
  float s = 0.f;
  if (p) {
    int k = grp;
    for (; k + 12 < nsplit; k += 16) {
      const float a0 = p[k * sstride], a1 = p[(k + 4) * sstride], a2 = p[(k + 8) * sstride],
                  a3 = p[(k + 12) * sstride];
      s += a0;
      s += a1;
      s += a2;
      s += a3;
    }
    for (; k < nsplit; k += 4) s += p[k * sstride];
  }
  part[grp][threadIdx.x & 63] = s;
  __syncthreads();
  if (grp != 0 || idx >= total) return;
  const int l = threadIdx.x;
  s = ((part[0][l] + part[1][l]) + part[2][l]) + part[3][l];
  int cot = co;
  if (perm_r > 1) {
    const int rr = perm_r * perm_r, cp = cout / rr;
    const int sub = co / cp, cc = co - sub * cp;
    cot = cc * rr + sub;
  }
  s *= scale;
  if (idx < nw) {
    const int khi = tap / kw, kwi = tap % kw;
    float* d = dw + ((((int64_t)cot * cin + ci) * kd + kdi) * kh + khi) * kw + kwi;
    *d = accumulate ? *d + s : s;
  } else {
    db[cot] = accumulate ? db[cot] + s : s;
  }
}

// The same sums as wgrad_reduce_kernel, in dw's memory order: a workgroup
// owns one (output channel, input block of cit_w channels, kd) and its
// cit_w x taps outputs, reads each split's [tap][ci] rows of the slab
// coalesced (8 splits of loads in flight per output), sums the splits in
// order 0, 1, 2, ... in fp32, and writes the (ci, tap) run of dw through LDS.
// Workgroups past the weights sum the dbias tails, one output channel per
// lane.  (wgrad_reduce_kernel writes dw with a 9-float stride per lane: the
// DRF sub-pixel weight gradients spent ~27 us per reduce in it.)
__global__ __launch_bounds__(256) void wgrad_reduce_rows_kernel(
    const float* __restrict__ ws, float* __restrict__ dw, float* __restrict__ db, int nsplit, int slab, int cout,
    int cin, int kd, int taps2, int nco_t, int nci_t, int cot_w, int cit_w, int kd_bias, int perm_r, float scale,
    int accumulate, int nblk_w) {
  constexpr int U = 8;
  __shared__ float out[64 * 9];
  const int64_t sstride = (int64_t)nco_t * nci_t * kd * slab;
  const int tid = threadIdx.x;
  auto sum_splits = [&](const float* p) __attribute__((always_inline)) {
    float s = 0.f;
    for (int k0 = 0; k0 < nsplit; k0 += U) {
      float v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = k0 + u < nsplit ? p[(int64_t)(k0 + u) * sstride] : 0.f;
#pragma unroll
      for (int u = 0; u < U; ++u) s += v[u];
    }
    return s;
  };
  auto torch_co = [&](int co) __attribute__((always_inline)) {
    if (perm_r > 1) {
      const int rr = perm_r * perm_r, cp = cout / rr;
      const int sub = co / cp;
      return (co - sub * cp) * rr + sub;
    }
    return co;
  };
  if ((int)blockIdx.x >= nblk_w) {  // dbias
    if (!db) return;
    const int co = ((int)blockIdx.x - nblk_w) * 256 + tid;
    if (co >= cout) return;
    const int combo = (kd_bias * nci_t + 0) * nco_t + co / cot_w;
    const float s = sum_splits(ws + (int64_t)combo * slab + (int64_t)taps2 * cot_w * cit_w + (co % cot_w)) * scale;
    const int cot = torch_co(co);
    db[cot] = accumulate ? db[cot] + s : s;
    return;
  }
  int b = blockIdx.x;
  const int kdi = b % kd;
  b /= kd;
  const int cic = b % nci_t;
  const int co = b / nci_t;
  const int ci0 = cic * cit_w;
  const int nci = min(cit_w, cin - ci0);
  const int nout = nci * taps2;
  const int combo = (kdi * nci_t + cic) * nco_t + co / cot_w;
  const float* base = ws + (int64_t)combo * slab + (int64_t)(co % cot_w) * cit_w;
  for (int j = tid; j < cit_w * taps2; j += 256) {  // read order: tap-major rows of cit_w input channels
    const int tap = j / cit_w, cil = j - tap * cit_w;
    if (cil < nci) out[cil * taps2 + tap] = sum_splits(base + (int64_t)tap * cot_w * cit_w + cil) * scale;
  }
  __syncthreads();
  float* d = dw + ((int64_t)torch_co(co) * cin + ci0) * kd * taps2 + (int64_t)kdi * taps2;
  for (int j = tid; j < nout; j += 256) {  // dw order: (ci, [kd,] tap)
    const int cil = j / taps2, tap = j - cil * taps2;
    float* q = d + (int64_t)cil * kd * taps2 + tap;
    *q = accumulate ? *q + out[j] : out[j];
  }
}

// A/B knob, read at load: 0 keeps the per-output reduce kernel
const int g_wgrad_reduce = vsrk_env_flag("VSRK_WGRAD_REDUCE", 1);

}  // namespace

int wgrad_reduce(const WgradSlabs& sl, const float* ws, int cout, int cin, int perm_r, float scale, int accumulate,
                 float* dw, float* db, hipStream_t s) {
  const int taps2 = sl.kh * sl.kw;
  const int nblk_w = cout * sl.nci_t * sl.kd;
  // The row-order kernel: one lane sums all splits of an output, so only for
  // few splits and enough workgroups (EDSR's 64 -> 64 has 256 splits over 64
  // such workgroups)
  if (sl.rows_ok && g_wgrad_reduce && sl.cit_w * taps2 <= 64 * 9 && sl.nsplit <= 32 && nblk_w >= 256) {
    const int nblk_b = db ? (int)ceil_div64(cout, 256) : 0;
    wgrad_reduce_rows_kernel<<<nblk_w + nblk_b, 256, 0, s>>>(ws, dw, db, sl.nsplit, sl.slab, cout, cin, sl.kd, taps2,
                                                              sl.nco_t, sl.nci_t, sl.cot_w, sl.cit_w, sl.kd_bias,
                                                              perm_r, scale, accumulate, nblk_w);
  } else {
    const int64_t total = (int64_t)cout * cin * sl.kd * taps2 + (db ? cout : 0);
    wgrad_reduce_kernel<<<(int)ceil_div64(total, 64), 256, 0, s>>>(
        ws, dw, db, sl.nsplit, sl.ncombos(), sl.slab, cout, cin, sl.kd, sl.kh, sl.kw, sl.nco_t,
        sl.nci_t, sl.cot_w, sl.cit_w, sl.kd_bias, perm_r, scale, accumulate);
  }
  VSRK_LAUNCH_CHECK("conv_wgrad_reduce");
  return VSRK_OK;
}
