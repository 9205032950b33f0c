/* vsrk deformable convolution (DCNv1 / DCNv2): the sampling and scatter
 * kernels of the reference's only native op (edvr_net/dcn/src/
 * deform_conv_cuda_kernel.cu:189-766, bound in deform_conv_cuda.cpp:681-695).
 * The contraction with the weights is the library's 1x1 conv (vsrk_conv_fwd /
 * vsrk_conv_wgrad in vsrk.h) over the sampled columns.
 *
 * geometry: int32[15] = {N, H, W, C, Ho, Wo, kh, kw, stride_h, stride_w,
 *   pad_h, pad_w, dil_h, dil_w, deformable_groups}; C / deformable_groups a
 *   multiple of 4.
 * x, grad_x: (N, H, W, C) fp32 channels-last.  cols, gcols: (N, Ho, Wo,
 *   kh*kw*C) fp32, column index k*C + c with k = i*kw + j.
 * offset, grad_offset: (N, G*2*kh*kw, Ho, Wo) fp32 (the reference's NCHW
 *   layout: channel (g*K + k)*2 + {0: h, 1: w}); mask, grad_mask: (N, G*kh*kw,
 *   Ho, Wo), mask NULL = DCNv1 (deform_conv), grad_mask may be NULL.
 *   vsrk_dcn_im2col:     cols = mask * bilinear(x, p + offset)
 *   vsrk_dcn_col2im:     grad_x += scatter of gcols (float atomics, as the
 *                        reference's col2im; grad_x must be zeroed first)
 *   vsrk_dcn_coord_grad: grad_offset, grad_mask (fixed-order per sample)
 * Same conventions as vsrk.h: int status, vsrk_last_error(), caller's stream. */
#ifndef VSRK_DCN_H
#define VSRK_DCN_H
#include <stdint.h>
#include "vsrk.h" /* vsrk_tensor5, for the view entry points */

#ifdef __cplusplus
extern "C" {
#endif

int vsrk_dcn_im2col(const int32_t* geometry, const float* x, const float* offset, const float* mask, float* cols,
                    void* stream);
int vsrk_dcn_col2im(const int32_t* geometry, const float* gcols, const float* offset, const float* mask,
                    float* grad_x, void* stream);
int vsrk_dcn_coord_grad(const int32_t* geometry, const float* x, const float* gcols, const float* offset,
                        const float* mask, float* grad_offset, float* grad_mask, void* stream);

/* The same three on channels-last VIEWS, for a net that keeps its activations
 * in views and in 16-bit storage (EDVR's PCD alignment):
 * x: (N, 1, H, W, C); cols, gcols: (N, 1, Ho, Wo, kh*kw*C), column k*C + c as
 *   above; vsrk_tensor5 views of VSRK_F32, VSRK_BF16 or VSRK_F16, one dtype per
 *   call.  Arithmetic is fp32; loads and stores are 16 bytes wide along the
 *   channel axis where C / deformable_groups, the base pointers and the strides
 *   allow, one element per lane otherwise (any C / deformable_groups).
 * om, gom: (N, 1, Ho, Wo, 3*G*K) fp32 views, the RAW output of the pack's
 *   conv_offset_mask and its gradient: the reference's chunk(3), cat(o1, o2)
 *   and sigmoid (deform_conv.py:261-300) are folded into the kernels.  The
 *   offset of (g, k) is channels (g*K + k)*2 + {0: h, 1: w} of the first 2*G*K,
 *   its mask sigmoid(om[2*G*K + g*K + k]).  Offsets, masks and their gradients
 *   stay fp32 in every compute precision.
 * geometry: as above, and Ho, Wo must follow from H, W.
 *   vsrk_dcn_view_im2col:     cols = mask * bilinear(x, p + offset)
 *   vsrk_dcn_view_coord_grad: gom, all 3*G*K channels, the sigmoid's m (1 - m)
 *                             included; one thread per (n, ho, wo, g, k),
 *                             channels in order: bitwise reproducible
 *   vsrk_dcn_view_col2im:     grad_x += scatter of gcols into an fp32
 *                             (N, H, W, C) contiguous buffer the caller has
 *                             zeroed (the caller casts afterwards).  Float
 *                             atomics, exactly as vsrk_dcn_col2im: with it the
 *                             library's one sum that is NOT in a fixed order.
 *                             One channel per lane, so that an atomic
 *                             instruction covers consecutive floats. */
int vsrk_dcn_view_im2col(const int32_t* geometry, const vsrk_tensor5* x, const vsrk_tensor5* om,
                         const vsrk_tensor5* cols, void* stream);
int vsrk_dcn_view_coord_grad(const int32_t* geometry, const vsrk_tensor5* x, const vsrk_tensor5* gcols,
                             const vsrk_tensor5* om, const vsrk_tensor5* gom, void* stream);
int vsrk_dcn_view_col2im(const int32_t* geometry, const vsrk_tensor5* gcols, const vsrk_tensor5* om, float* grad_x,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VSRK_DCN_H */
