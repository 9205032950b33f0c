"""What the flow-warp / pooling / channels-last resampling layer promises
without a device: the entry points exist and reject bad arguments on the
host (VSRK_ERR_INVALID with a vsrk_last_error text, nothing launched), the
custom ops have fake implementations, and swap_modules knows FRVSR's layers
(frvsr_net.py:84-86,127,196-226)."""
import ctypes as C
import inspect

import pytest
import torch
import torch.nn as nn

from vsr_amd import modules
from vsr_amd._native import Tensor5

INVALID = 1  # VSRK_ERR_INVALID
F32, BF16 = 0, 1
NEW = ["vsrk_flow_warp_fwd", "vsrk_flow_warp_bwd", "vsrk_max_pool2x2_fwd", "vsrk_max_pool2x2_bwd",
       "vsrk_upsample_cl_fwd", "vsrk_upsample_cl_bwd", "vsrk_tanh_fwd", "vsrk_tanh_bwd"]


def _t5(h, w, c, n=1, ptr=0x1000, dtype=F32, d=1, shuffle=1):
    return Tensor5(ptr, n, d, h, w, c, h * w * c, h * w * c, w * c, c, shuffle, dtype)


def _err(native, needle):
    text = native.vsrk_last_error()
    assert needle in text, text


def test_library_exports_the_new_entry_points(native):
    for name in NEW:
        assert hasattr(native, name), name


def test_flow_warp_rejects_bad_arguments(native):
    img, flow = _t5(4, 6, 2), C.c_void_p(0x2000)

    def fwd(i=img, f=flow, o=_t5(4, 6, 2), s2d=1, pad=1, ac=0, up=1):
        return native.vsrk_flow_warp_fwd(C.byref(i), f, up, C.byref(o), s2d, pad, ac, None)

    assert native.vsrk_flow_warp_fwd(None, flow, 1, C.byref(img), 1, 1, 0, None) == INVALID
    _err(native, b"null")
    assert fwd(f=None) == INVALID
    assert fwd(o=_t5(4, 5, 2)) == INVALID
    _err(native, b"shape mismatch")
    assert fwd(o=_t5(4, 6, 2, dtype=BF16)) == INVALID
    _err(native, b"dtype mismatch")
    assert fwd(o=_t5(2, 3, 2), s2d=2) == INVALID  # r*r*c = 8 channels wanted
    assert fwd(o=_t5(2, 2, 18), s2d=3) == INVALID
    _err(native, b"multiple of s2d")
    assert fwd(pad=2) == INVALID
    _err(native, b"padding_mode")
    assert fwd(ac=2) == INVALID
    assert fwd(s2d=0) == INVALID
    assert fwd(up=0) == INVALID
    assert fwd(up=4) == INVALID  # 6 columns
    _err(native, b"multiple of flow_up")
    assert fwd(i=_t5(4, 6, 2, d=2)) == INVALID
    assert fwd(i=_t5(4, 6, 2, shuffle=2)) == INVALID
    assert fwd(i=_t5(4, 6, 2, dtype=7), o=_t5(4, 6, 2, dtype=7)) == INVALID
    g = _t5(4, 6, 2)
    assert native.vsrk_flow_warp_bwd(C.byref(img), flow, 1, C.byref(g), 1, 1, 0, 0, None, None) == INVALID
    assert native.vsrk_flow_warp_bwd(C.byref(img), flow, 1, C.byref(g), 1, 1, 0, 2, C.c_void_p(0x3000),
                                     None) == INVALID
    _err(native, b"accumulate")


def test_pool_and_resample_reject_bad_arguments(native):
    x = _t5(4, 6, 8)
    assert native.vsrk_max_pool2x2_fwd(C.byref(x), C.byref(_t5(2, 2, 8)), None) == INVALID
    _err(native, b"factor 2")
    assert native.vsrk_max_pool2x2_fwd(C.byref(x), C.byref(_t5(2, 3, 4)), None) == INVALID
    assert native.vsrk_max_pool2x2_fwd(C.byref(x), None, None) == INVALID
    assert native.vsrk_max_pool2x2_fwd(C.byref(_t5(1, 6, 8)), C.byref(_t5(0, 3, 8)), None) == INVALID
    _err(native, b"empty")
    assert native.vsrk_max_pool2x2_bwd(C.byref(x), C.byref(_t5(2, 3, 8)), C.byref(_t5(4, 5, 8)), None) == INVALID
    assert native.vsrk_upsample_cl_fwd(C.byref(x), C.byref(_t5(8, 13, 8)), 2, 0, 0, None) == INVALID
    assert native.vsrk_upsample_cl_fwd(C.byref(x), C.byref(_t5(8, 12, 8)), 0, 0, 0, None) == INVALID
    _err(native, b"scale factor")
    assert native.vsrk_upsample_cl_fwd(C.byref(x), C.byref(_t5(8, 12, 8)), 2, 2, 0, None) == INVALID
    assert native.vsrk_upsample_cl_bwd(C.byref(_t5(8, 12, 8)), C.byref(x), 2, 0, 3, None) == INVALID
    assert native.vsrk_upsample_cl_bwd(C.byref(_t5(8, 12, 8, dtype=BF16)), C.byref(x), 2, 0, 0, None) == INVALID
    _err(native, b"dtype mismatch")
    assert native.vsrk_tanh_fwd(C.byref(x), C.byref(_t5(4, 6, 4)), None) == INVALID
    assert native.vsrk_tanh_bwd(C.byref(x), C.byref(x), None, None) == INVALID


def test_ops_have_fake_implementations():
    img = torch.empty((2, 3, 5, 7), device="meta", dtype=torch.bfloat16)
    u = torch.empty((2, 5, 7), device="meta")
    y = torch.ops.vsrk.flow_warp(img, u, u, "border", False)
    assert y.shape == img.shape and y.dtype == torch.bfloat16 and y.device.type == "meta"
    p = torch.ops.vsrk.max_pool2x2(img)
    assert p.shape == (2, 3, 2, 3) and p.dtype == torch.bfloat16


def test_stn_has_the_reference_signature():
    stn = modules.STN()
    assert (stn.mode, stn.padding_mode, stn.norm) == ("bilinear", "zeros", False)
    assert list(inspect.signature(stn.forward).parameters) == ["inputs", "u", "v"]
    assert list(stn.state_dict()) == []


def test_convert_takes_frvsr_layers():
    # the tail's deconvs: output_padding = s - k + 2p, and 0 as before
    assert type(modules._convert(nn.ConvTranspose2d(64, 64, 3, stride=2, padding=1, output_padding=1))) \
        is modules.HipConvTranspose2d
    assert type(modules._convert(nn.ConvTranspose2d(8, 8, 8, stride=4, padding=2))) is modules.HipConvTranspose2d
    assert type(modules._convert(nn.ConvTranspose2d(8, 8, 6, stride=2, padding=2))) is modules.HipConvTranspose2d
    # any other output_padding is not the sub-pixel form's size
    assert modules._convert(nn.ConvTranspose2d(8, 8, 8, stride=4, padding=2, output_padding=1)) is None
    assert modules._convert(nn.ConvTranspose2d(8, 8, 5, stride=3, padding=1, output_padding=1)) is None
    assert modules._convert(nn.ConvTranspose2d(8, 8, 5, stride=3, padding=1, output_padding=2)) is None
    # nn.MaxPool2d(2) and only that
    for ok in (nn.MaxPool2d(2), nn.MaxPool2d((2, 2), stride=2), nn.MaxPool2d(2, stride=(2, 2), padding=0)):
        assert type(modules._convert(ok)) is modules.HipMaxPool2d, ok
    for no in (nn.MaxPool2d(2, ceil_mode=True), nn.MaxPool2d(2, return_indices=True), nn.MaxPool2d(3),
               nn.MaxPool2d(2, stride=1), nn.MaxPool2d(2, padding=1), nn.MaxPool2d(2, dilation=2),
               nn.MaxPool2d((2, 1))):
        assert modules._convert(no) is None, no
    net = modules.swap_modules(nn.Sequential(nn.Conv2d(2, 32, 3, padding=1), nn.LeakyReLU(0.2), nn.MaxPool2d(2)))
    assert [type(m).__name__ for m in net] == ["HipConv2d", "LeakyReLU", "HipMaxPool2d"]
    assert net[2].kernel_size == 2 and net[2].stride == 2
