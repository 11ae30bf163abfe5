"""Reference for INT8 engines loaded in the "int8_general" mode (spvo_set_int8_general).  TEST INFRASTRUCTURE.

oracle/net_int8.py defines the INT8 arithmetic and raises NotImplementedError for a stand-alone max-pool.  `forward` here is that
module's op loop, built from its own helpers (fma32, quantize, quantize_weights, bn_affine, folds, is_quantized), plus the one op the
mode adds.  On a plan without a stand-alone pool it gives oracle.net_int8.forward's bits (tests/test_int8_general_cpu.py).

Stand-alone 2x2/2 max-pool from int8 tensor i (scale s_i) to int8 tensor o (scale s_o) -- csrc/conv_i8.hip.h, maxpool2_i8_kernel:

    inv = f32(1) / f32(s_o)                                      one fp32 division
    m   = f32(f32(s_i) * inv)                                    one fp32 multiply
    q_o = clip(rint(f32(max of the four q_i) * m), -127, 127)    one fp32 multiply per value, round-half-even

The four q_i are integers of magnitude at most 127, so f32() of their maximum is exact.  A pool between two fp32 tensors passes the
maximum through (no engine holds one: the loader refuses it).

A convolution whose cin is 16 more than a multiple of 32 needs nothing here: the weights are quantised over the op's real cin and the
accumulator is the exact integer sum, however the kernel pads its last chunk.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle.net_int8 import bn_affine, f32, fma32, folds, is_quantized, quantize, quantize_weights
from spvo import weights as W


def pool_multiplier(s_in, s_out):
    inv = f32(1.0) / f32(s_out)
    return f32(f32(s_in) * inv)


def pool_max(src):
    B, C, H, Wd = src.shape
    return src.reshape(B, C, H // 2, 2, Wd // 2, 2).max(axis=(3, 5))


def maxpool_i8(src, s_in, s_out):
    """(q_o int8, the window maxima int8)"""
    mx = pool_max(src)
    v = (mx.astype(f32) * pool_multiplier(s_in, s_out)).astype(f32)
    return np.clip(np.rint(v), -127, 127).astype(np.int8), mx


def forward(plan, x, return_all=False):
    """x: float32 [B,1,H,W].  Returns (det, desc) float32 NCHW; with return_all also {tensor id: int8 or float32 array}."""
    assert plan.precision == "INT8" and plan.act_scales is not None
    B, _, H, Wd = x.shape
    s = plan.act_scales.astype(f32)
    vals = {plan.input_tensor: x.astype(f32)}
    for op in plan.ops:
        src = vals[op.inp]
        if op.type in (W.OP_CONV, W.OP_DWCONV):
            dw = op.type == W.OP_DWCONV
            xin = src[:, op.in_c_off:op.in_c_off + op.cin]
            k, pad = op.ksize, op.ksize // 2
            fold = folds(plan, op)
            inv_out = f32(1.0) / f32(s[op.out])
            has_bn = bool(op.flags & W.FLAG_BN)
            if not is_quantized(plan, op.inp):
                assert op.cin == 1 and not dw and not (op.flags & (W.FLAG_POOL | W.FLAG_ADD))
                xp = np.pad(xin[:, 0], ((0, 0), (pad, pad), (pad, pad)))
                r = np.broadcast_to(op.bias.astype(f32)[None, :, None, None], (B, op.cout, H >> plan.tensors[op.inp][1], Wd >> plan.tensors[op.inp][1])).copy()
                hh, ww = r.shape[2], r.shape[3]
                for ky in range(k):
                    for kx in range(k):
                        r = fma32(op.weight[:, 0, ky, kx].astype(f32)[None, :, None, None], xp[:, None, ky:ky + hh, kx:kx + ww], r)
            else:
                wq, ws = quantize_weights(op.weight)
                acc = F.conv2d(torch.from_numpy(xin.astype(np.float64)), torch.from_numpy(wq.astype(np.float64)), None, stride=1, padding=pad,
                               groups=op.cin if dw else 1).numpy()
                assert np.abs(acc).max() < 2 ** 31
                m = (ws * s[op.inp]).astype(f32)
                bias = op.bias.astype(f32)
                if fold and not has_bn:
                    m, bias = (m * inv_out).astype(f32), (bias * inv_out).astype(f32)
                r = fma32(acc.astype(np.int32).astype(f32), m[None, :, None, None], bias[None, :, None, None])
            if op.flags & W.FLAG_RELU:
                r = np.maximum(r, f32(0))
            if has_bn:
                sc, sh = bn_affine(op)
                if fold:
                    sc, sh = (sc * inv_out).astype(f32), (sh * inv_out).astype(f32)
                r = np.maximum(fma32(r, sc[None, :, None, None], sh[None, :, None, None]), f32(0))
            if op.flags & W.FLAG_ADD:
                r = np.maximum(fma32(vals[op.residual].astype(f32), f32(s[op.residual]), r), f32(0))
            if op.flags & W.FLAG_POOL:
                r = r.reshape(B, op.cout, r.shape[2] // 2, 2, r.shape[3] // 2, 2).max(axis=(3, 5))
            out = quantize(r, s[op.out], fold) if is_quantized(plan, op.out) else r
            ch, lvl = plan.tensors[op.out]
            if op.out not in vals:
                vals[op.out] = np.zeros((B, ch, H >> lvl, Wd >> lvl), out.dtype)
            vals[op.out][:, op.out_c_off:op.out_c_off + op.cout] = out
        elif op.type == W.OP_MAXPOOL:
            qi, qo = is_quantized(plan, op.inp), is_quantized(plan, op.out)
            assert qi == qo, "a stand-alone max-pool between an int8 and an fp32 tensor"
            vals[op.out] = maxpool_i8(src, s[op.inp], s[op.out])[0] if qi else pool_max(src)
        elif op.type == W.OP_L2NORM:
            v = torch.from_numpy(src)
            vals[op.out] = (v / torch.sqrt((v * v).sum(dim=1, keepdim=True))).numpy()
        else:
            raise NotImplementedError("INT8 engines: op type %d" % op.type)
    det, desc = vals[plan.det_tensor], vals[plan.desc_tensor]
    return (det, desc, vals) if return_all else (det, desc)
