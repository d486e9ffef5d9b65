"""The reference's frame preprocessing, exactly: PIL's 8-bit BILINEAR resize, centre crop, ToTensor, Normalize.

The reference decodes a frame to a PIL image and applies torchvision's Resize / CenterCrop / ToTensor / Normalize
(vsc/baseline/inference_impl.py:39-69).  PIL's 8-bit resize (`ImagingResample`) is integer arithmetic on fixed-point
coefficients, so it can be reproduced bit for bit; the rule is written out in include/vscmi.h
(`vsc_frame_transform_u8`).  This module holds

  * `resize_plan`      resize target, window and output shape of an `InferenceTransforms` member for one source size;
  * `pil_coeffs`, `resize_levels`, `transform_host`   the numpy restatement of the rule: the CPU contract, which shares
                       no code with the library's table builder (csrc/frame_transform.hip);
  * `transform_device` the library's kernels on uint8 device tensors of different source sizes, fp32 NCHW or bf16 NHWC.

`inference_cli.run_inference_packed` (`--packed_batch`) is the user of both.
"""
import math
from typing import List, Sequence, Tuple

import numpy as np

from vsc2022_amd import _lib
from vsc2022_amd.vsc.baseline.inference import IMAGENET_MEAN, IMAGENET_STD
from vsc2022_amd.vsc.baseline.inference_cli import _short_edge_size

PRECISION_BITS = 22


def _transform_name(transform) -> str:
    return transform if isinstance(transform, str) else transform.name


def resize_plan(transform, h: int, w: int) -> Tuple[int, int, int, int, int, int]:
    """(th, tw, top, left, oh, ow): resize an h x w frame to (th, tw), keep [top, top + oh) x [left, left + ow).
    `device_transform`'s rules; `round` is Python's (half to even), as in torchvision's center_crop."""
    name = _transform_name(transform)
    if name == "RESIZE_224_SQUARE":
        return 224, 224, 0, 0, 224, 224
    if name == "RESIZE_288":
        th, tw = _short_edge_size(h, w, 288)
        return th, tw, 0, 0, th, tw
    if name == "RESIZE_320_CENTER":
        th, tw = _short_edge_size(h, w, 320)
        return th, tw, int(round((th - 320) / 2.0)), int(round((tw - 320) / 2.0)), 320, 320
    raise ValueError(f"unknown transform {transform!r}")


def check_limits(h: int, w: int, th: int, tw: int):
    """The limits of `vsc_frame_transform_u8`, as a ValueError that names the limit."""
    if not (1 <= h <= _lib.FRAME_MAX_SRC and 1 <= w <= _lib.FRAME_MAX_SRC):
        raise ValueError(f"frame of {h} x {w}: the frame transform takes source edges of 1..{_lib.FRAME_MAX_SRC} pixels")
    if not (1 <= th <= _lib.FRAME_MAX_DST and 1 <= tw <= _lib.FRAME_MAX_DST):
        raise ValueError(f"frame of {h} x {w} resizes to {th} x {tw}: the frame transform takes resized edges of "
                         f"1..{_lib.FRAME_MAX_DST} pixels")


def pil_coeffs(in_size: int, out_size: int):
    """(ksize, xmin [out], taps [out], K [out, ksize] int32) of PIL's precompute_coeffs + normalize_coeffs_8bpc for the
    triangle filter (ImagingResample, BILINEAR).  Python floats are C doubles; int() truncates toward zero."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = fs
    ksize = int(math.ceil(support)) * 2 + 1
    inv = 1.0 / fs
    xmins = np.zeros(out_size, np.int32)
    taps = np.zeros(out_size, np.int32)
    kk = np.zeros((out_size, ksize), np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * inv)) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            k = v / ww if ww != 0.0 else v
            kk[xx, x] = int(-0.5 + k * (1 << PRECISION_BITS)) if k < 0 else int(0.5 + k * (1 << PRECISION_BITS))
        xmins[xx], taps[xx] = xmin, n
    return ksize, xmins, taps, kk


def _resample_axis0(img: np.ndarray, out_size: int) -> np.ndarray:
    """One pass along axis 0 of a uint8 array; the result is uint8 again (rounded, clipped)."""
    _, xmins, taps, kk = pil_coeffs(img.shape[0], out_size)
    out = np.empty((out_size,) + img.shape[1:], np.uint8)
    src = img.astype(np.int32)
    for xx in range(out_size):
        a, n = int(xmins[xx]), int(taps[xx])
        acc = np.tensordot(kk[xx, :n], src[a : a + n], axes=(0, 0)).astype(np.int32) + (1 << (PRECISION_BITS - 1))
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


def resize_levels(img_u8_hwc: np.ndarray, th: int, tw: int) -> np.ndarray:
    """`np.asarray(PIL.Image.fromarray(img).resize((tw, th), BILINEAR))`: horizontal pass, then vertical, the image
    between them uint8; an axis that keeps its size is skipped."""
    img = np.ascontiguousarray(img_u8_hwc)
    assert img.dtype == np.uint8 and img.ndim == 3
    if img.shape[1] != tw:
        img = _resample_axis0(img.transpose(1, 0, 2), tw).transpose(1, 0, 2)
    if img.shape[0] != th:
        img = _resample_axis0(img, th)
    return np.ascontiguousarray(img)


def value_table(mean=IMAGENET_MEAN, std=IMAGENET_STD) -> np.ndarray:
    """[3, 256] fp32: ((float)level / 255 - mean[c]) / std[c], each step rounded to fp32 (ToTensor, then Normalize)."""
    level = np.arange(256, dtype=np.float32) / np.float32(255.0)
    m, s = np.asarray(mean, np.float32).reshape(3, 1), np.asarray(std, np.float32).reshape(3, 1)
    return ((level[None, :] - m) / s).astype(np.float32)


def transform_host(frames_u8: np.ndarray, transform) -> np.ndarray:
    """uint8 [n, H, W, 3] -> fp32 [n, 3, oh, ow], exactly what the reference's host preprocessing gives."""
    frames_u8 = np.asarray(frames_u8)
    if frames_u8.ndim == 3:
        frames_u8 = frames_u8[None]
    n, h, w, _ = frames_u8.shape
    th, tw, top, left, oh, ow = resize_plan(transform, h, w)
    lut = value_table()
    out = np.empty((n, 3, oh, ow), np.float32)
    chan = np.arange(3).reshape(3, 1, 1)
    for i in range(n):
        lv = resize_levels(frames_u8[i], th, tw)[top : top + oh, left : left + ow]
        out[i] = lut[chan, lv.transpose(2, 0, 1)]
    return out


def transform_device(frames: Sequence, transform, out: str = "f32", into=None):
    """uint8 device tensors [k_i, H_i, W_i, 3] (any mix of source sizes that share an output shape under `transform`)
    -> one tensor of logical shape [sum k_i, 3, oh, ow] in the order given: contiguous fp32 for out="f32", bf16 with
    channels_last strides for out="bf16" (what `FastTrunk` converts its input to).  One library call, on torch's current
    stream.  `into`: a contiguous tensor of the output's dtype and element count on the same device to write instead
    of a new one."""
    import torch

    if out not in ("f32", "bf16"):
        raise ValueError(f"out must be 'f32' or 'bf16', not {out!r}")
    frames = [f.unsqueeze(0) if f.ndim == 3 else f for f in frames]
    if not frames:
        raise ValueError("transform_device needs at least one tensor")
    device = frames[0].device
    plans: List[Tuple[int, int, int, int, int, int]] = []
    for f in frames:
        if f.dtype != torch.uint8 or f.ndim != 4 or f.shape[3] != 3 or not f.is_cuda or f.device != device:
            raise ValueError("transform_device takes uint8 [k, H, W, 3] tensors on one GPU")
        p = resize_plan(transform, int(f.shape[1]), int(f.shape[2]))
        check_limits(int(f.shape[1]), int(f.shape[2]), p[0], p[1])
        if plans and p[4:] != plans[0][4:]:
            raise ValueError(f"frames of one call must share an output shape: {p[4:]} and {plans[0][4:]}")
        plans.append(p)
    oh, ow = plans[0][4:]
    frames = [f.contiguous() for f in frames]
    # The library addresses every frame by its offset from one base pointer: views of one allocation are read in place,
    # anything else is stacked first.
    store = frames[0].untyped_storage().data_ptr()
    if all(f.untyped_storage().data_ptr() == store for f in frames):
        src, starts = frames[0], [f.data_ptr() for f in frames]
        base = min(starts)
        starts = [p - base for p in starts]
    else:
        src, starts, at = torch.cat([f.reshape(-1) for f in frames]), [], 0
        base = src.data_ptr()
        for f in frames:
            starts.append(at)
            at += f.numel()
    offs, cols = [], [[] for _ in range(6)]
    for f, start, (th, tw, top, left, _, _) in zip(frames, starts, plans):
        k, h, w = int(f.shape[0]), int(f.shape[1]), int(f.shape[2])
        offs.extend(start + i * h * w * 3 for i in range(k))
        for col, v in zip(cols, (h, w, th, tw, top, left)):
            col.extend([v] * k)
    n = len(offs)
    off = np.asarray(offs, np.int64)
    sh, sw, dh, dw, tp, lf = (np.asarray(c, np.int32) for c in cols)
    mean, std = np.asarray(IMAGENET_MEAN, np.float32), np.asarray(IMAGENET_STD, np.float32)
    with torch.cuda.device(device):
        shape, dtype, fmt = (((n, oh, ow, 3), torch.bfloat16, _lib.FRAME_OUT_BF16_NHWC) if out == "bf16" else
                             ((n, 3, oh, ow), torch.float32, _lib.FRAME_OUT_F32_NCHW))
        if into is None:
            res = torch.empty(shape, dtype=dtype, device=device)
        else:
            if into.dtype != dtype or into.device != device or not into.is_contiguous() or into.numel() != n * 3 * oh * ow:
                raise ValueError(f"into must be a contiguous {dtype} tensor of {n * 3 * oh * ow} elements on {device}")
            res = into.view(shape)
        _lib.check(_lib.lib().vsc_frame_transform_u8(
            base, off.ctypes.data, sh.ctypes.data, sw.ctypes.data, dh.ctypes.data, dw.ctypes.data, tp.ctypes.data,
            lf.ctypes.data, n, oh, ow, mean.ctypes.data, std.ctypes.data, fmt, res.data_ptr(),
            torch.cuda.current_stream(device).cuda_stream))
    return res.permute(0, 3, 1, 2) if out == "bf16" else res
