"""DnS L3-iMAC region descriptors (`--baseline dns`; the reference's docs/baseline_dns.md, first stage).

The reference runs a downloaded TorchScript file (`resnet50_l3imac.torchscript.pt`, `--transforms RESIZE_224_SQUARE
--store_fp16`) whose definition is not in its tree.  `L3iMACModel` restates it in eager fp32 PyTorch as recalled from
the public distill-and-select repository (`model/feature_extractor.py`, `model/layers.py:PCA`), which is not part of
this project: a torchvision ResNet-50 whose four stage outputs (256, 512, 1024, 2048 channels) are region-max-pooled
with windows (28, 14, 6, 3) and strides ceil(window / 2), L2-normalised over the channels, brought onto the last tap's
grid by an adaptive max-pool, normalised again, concatenated (3840 channels), laid out as [frames, regions, 3840] in
row-major grid order and normalised once more; an optional PCA whitening (`mean`, `DVt`) follows.  224 x 224 frames
give 3 x 3 = 9 regions and the adaptive pool is the identity.  `l3imac_from_module` therefore only accepts an export
that reproduces `L3iMACModel` on a random batch, so that a wrong recollection makes `--fast` refuse the model instead
of returning wrong descriptors.

`FastL3iMAC` is the same pass on the GPU: the folded bf16 NHWC trunk of `FastSSCD` (`inference.FastTrunk`), the region
pooling and channel normalisation of every tap as one launch of `vsc_region_pool_l2_bf16` on the bf16 activation as it
stands in memory, and `vsc_rows_l2norm_f32` over the assembled rows (csrc/region_pool.hip).
"""
import math
from typing import List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from vsc2022_amd.vsc.baseline.inference import RESNET50_STAGES, FastTrunk, fold_batchnorm, resnet50_stem_trunk

TAP_CHANNELS = tuple(4 * planes for planes, _, _ in RESNET50_STAGES)           # (256, 512, 1024, 2048)
TAP_BLOCKS = tuple(sum(b for _, b, _ in RESNET50_STAGES[: i + 1]) - 1 for i in range(4))  # last block of each stage
TAP_WINDOWS = (28, 14, 6, 3)
TAP_STRIDES = tuple(math.ceil(s / 2) for s in TAP_WINDOWS)                       # (14, 7, 3, 2)
L3IMAC_DIMS = sum(TAP_CHANNELS)                                                  # 3840
NORM_EPS = 1e-12                                                                 # F.normalize's default


def _grid(h: int, w: int, win: int, stride: int) -> Tuple[int, int]:
    """Output size of max_pool2d(win, stride) without padding (floor); ValueError when the window does not fit."""
    if h < win or w < win:
        raise ValueError(f"L3-iMAC: a {h} x {w} activation is smaller than its {win} x {win} region window "
                         "(the frame is too small)")
    return (h - win) // stride + 1, (w - win) // stride + 1


class Whitening(nn.Module):
    """PCA whitening of distill-and-select's `model/layers.py:PCA`: y = normalize((x - mean) @ DVt)."""

    def __init__(self, dims: int, in_dims: int = L3IMAC_DIMS):
        super().__init__()
        self.register_buffer("mean", torch.zeros(in_dims))
        self.register_buffer("DVt", torch.zeros(in_dims, dims))

    def forward(self, x):
        return F.normalize((x - self.mean) @ self.DVt, p=2, dim=-1)


class L3iMACModel(nn.Module):
    """[B, 3, H, W] normalised frames -> [B, R, 3840] fp32 region descriptors ([B, R, dims] with whitening); module
    docstring.  Tensors in torchvision's resnet50 order, then `pca.mean`, `pca.DVt`."""

    def __init__(self, dims: Optional[int] = None):
        super().__init__()
        self.stem, self.trunk = resnet50_stem_trunk()
        self.pca = Whitening(dims) if dims else None

    def taps(self, x) -> List[torch.Tensor]:
        out = []
        x = self.stem(x)
        for i, blk in enumerate(self.trunk):
            x = blk(x)
            if i in TAP_BLOCKS:
                out.append(x)
        return out

    @staticmethod
    def regions(taps: List[torch.Tensor]) -> torch.Tensor:
        pooled = []
        for x, win, stride in zip(taps, TAP_WINDOWS, TAP_STRIDES):
            _grid(x.shape[-2], x.shape[-1], win, stride)
            pooled.append(F.normalize(F.max_pool2d(x.float(), win, stride), p=2, dim=1))
        h, w = pooled[-1].shape[-2], pooled[-1].shape[-1]
        pooled = [F.normalize(F.adaptive_max_pool2d(r, (h, w)), p=2, dim=1) for r in pooled]
        x = torch.cat(pooled, dim=1)
        x = x.permute(0, 2, 3, 1).reshape(x.shape[0], h * w, L3IMAC_DIMS)
        return F.normalize(x, p=2, dim=-1)

    def forward(self, x):
        x = self.regions(self.taps(x))
        return x if self.pca is None else self.pca(x)


def build_l3imac_model(dims: Optional[int] = None, seed: int = 0, device="cpu") -> L3iMACModel:
    """A random-init L3-iMAC network for tests and benchmarks (like `build_sscd_model`).  With `dims`, whitening buffers
    of a plausible kind: DVt = V / sqrt(d) with V a seeded random orthonormal [3840, dims] and d geometric from 1 down to
    1/16 (PCA whitening divides by the root of the eigenvalues); mean with entries of the order of 1e-2."""
    torch.manual_seed(seed)
    model = L3iMACModel(dims).eval()
    if dims:
        g = torch.Generator().manual_seed(seed + 1)
        v, _ = torch.linalg.qr(torch.randn((L3IMAC_DIMS, dims), generator=g, dtype=torch.float64))
        d = torch.logspace(0.0, math.log2(1.0 / 16.0), dims, base=2.0, dtype=torch.float64)
        model.pca.DVt.copy_((v / d.sqrt()).float())
        model.pca.mean.copy_(1e-2 * torch.randn(L3IMAC_DIMS, generator=g))
    model = model.to(device)
    for p in model.parameters():
        p.requires_grad_(False)
    return model


def l3imac_from_module(module, check_tol: float = 1e-3) -> Optional[L3iMACModel]:
    """An `L3iMACModel` holding the weights of `module` (a TorchScript or eager L3-iMAC export), or None when it is not
    that architecture.  Same contract as `sscd_from_module`: tensors are matched by position and shape (names may carry
    any prefix): the ResNet-50 convolutions and BatchNorms in torchvision's order, then optionally the unused `fc` pair
    [1000, 2048], [1000] of a whole torchvision resnet50 (ignored), then optionally the whitening's mean [3840] and DVt
    [3840, dims]; both networks must agree on a random 2 x 3 x 128 x 128 batch (squared distance of every region vector
    <= check_tol) or None is returned."""
    try:
        src = [(k, v) for k, v in module.state_dict().items() if not k.endswith("num_batches_tracked")]
    except Exception:
        return None
    trunk = [(k, v) for k, v in L3iMACModel().state_dict().items() if not k.endswith("num_batches_tracked")]
    if len(src) < len(trunk) or any(a[1].shape != b[1].shape for a, b in zip(src, trunk)):
        return None
    rest = [v for _, v in src[len(trunk):]]
    if len(rest) >= 2 and tuple(rest[0].shape) == (1000, 2048) and tuple(rest[1].shape) == (1000,):
        rest = rest[2:]
    dims = None
    if rest:
        if len(rest) != 2 or tuple(rest[0].shape) != (L3IMAC_DIMS,) or rest[1].dim() != 2 or rest[1].shape[0] != L3IMAC_DIMS:
            return None
        dims = int(rest[1].shape[1])
    model = L3iMACModel(dims).eval()
    dst = [(k, v) for k, v in model.state_dict().items() if not k.endswith("num_batches_tracked")]
    with torch.no_grad():
        for a, (_, b) in zip([v for _, v in src[: len(trunk)]] + rest, dst):
            b.copy_(a.detach().to(device=b.device, dtype=b.dtype))
        dev = src[0][1].device
        model = model.to(dev)
        g = torch.Generator().manual_seed(0)
        x = torch.randn((2, 3, 128, 128), generator=g).to(dev)
        try:
            got, want = model(x).float(), module(x).float()
            if got.shape != want.shape:
                return None
            d = (want - got).pow(2).sum(dim=-1)
        except Exception:
            return None
    if not bool(torch.isfinite(d).all()) or float(d.max()) > check_tol:
        return None
    for p in model.parameters():
        p.requires_grad_(False)
    return model


# ------------------------------------------------------------------------------------------------ kernel wrappers
def _region_pool_l2(x: torch.Tensor, win: int, stride: int, out: Optional[torch.Tensor] = None, out_col: int = 0,
                    eps: float = NORM_EPS) -> torch.Tensor:
    """Region max-pool + channel L2 normalisation of a [B, C, H, W] bf16 tensor in channels-last memory:
    `vsc_region_pool_l2_bf16` (csrc/region_pool.hip).  Writes columns [out_col, out_col + C) of the rows of `out`
    [B, gh * gw, row] fp32 (a fresh [B, gh * gw, C] when None) and returns it."""
    from vsc2022_amd import _lib

    b, c, h, w = x.shape
    assert x.is_cuda and x.dtype == torch.bfloat16 and x.permute(0, 2, 3, 1).is_contiguous()
    gh, gw = _grid(h, w, win, stride)
    if out is None:
        out = torch.empty((b, gh * gw, c), dtype=torch.float32, device=x.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.dim() == 3 and out.device == x.device
    assert out.shape[0] == b and out.shape[1] == gh * gw
    _lib.check(_lib.lib().vsc_region_pool_l2_bf16(x.data_ptr(), out.data_ptr(), b, h, w, c, win, stride, out.shape[2], out_col,
                                                  float(eps), torch.cuda.current_stream(x.device).cuda_stream))
    return out


def _rows_l2norm(x: torch.Tensor, eps: float = NORM_EPS) -> torch.Tensor:
    """In place F.normalize over the last dimension of a contiguous fp32 device tensor: `vsc_rows_l2norm_f32`."""
    from vsc2022_amd import _lib

    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() >= 1
    cols = x.shape[-1]
    _lib.check(_lib.lib().vsc_rows_l2norm_f32(x.data_ptr(), x.numel() // max(cols, 1), cols, float(eps),
                                              torch.cuda.current_stream(x.device).cuda_stream))
    return x


class FastL3iMAC(FastTrunk):
    """`L3iMACModel` prepared for inference on the GPU the way `FastSSCD` prepares an `SSCDModel`: BatchNorms folded,
    stem and blocks in bf16 NHWC (`FastTrunk`).  The taps are the block outputs as they stand in memory.

    A tap whose grid equals the final grid (every tap at 224 x 224) is written by `vsc_region_pool_l2_bf16` straight into
    its column slice of the [B, R, 3840] fp32 block; the adaptive pool is the identity there, and the second
    normalisation of the already unit-norm vector is skipped.  That second division would divide by the fp32 norm of a
    vector normalised in fp32, which is 1 to within the rounding of a C-term sum: skipping it changes a value by at most
    about C * 2^-24 relative (1.2e-4 for the 2048-channel tap), far inside the bf16 trunk's own error.  A tap with another
    grid (frames that are not 224 x 224) is pooled by the kernel into [B, g * g, C]; the adaptive pool, the second
    normalisation and the copy into the slice are torch ops on that small tensor.  `vsc_rows_l2norm_f32` then normalises
    the 3840 columns, and the whitening, when present, is the eager model's own fp32 module.
    Takes the fp32 normalised frames [B, 3, H, W]; returns fp32 [B, R, 3840] (or [B, R, dims])."""

    def __init__(self, model: L3iMACModel):
        m = fold_batchnorm(model)
        super().__init__(m)
        self.pca = m.pca
        for p in self.parameters():
            p.requires_grad_(False)

    def taps(self, x) -> List[torch.Tensor]:
        """The four stage outputs, [B, C, H, W] bf16 in channels-last memory."""
        out = []
        x = self._stem(x)
        for i, blk in enumerate(self.blocks):
            x = blk(x)
            if i in TAP_BLOCKS:
                out.append(x)
        return out

    @staticmethod
    def regions(taps: List[torch.Tensor]) -> torch.Tensor:
        """`L3iMACModel.regions` on the bf16 taps through the two kernels: [B, R, 3840] fp32."""
        grids = [_grid(t.shape[-2], t.shape[-1], win, stride) for t, win, stride in zip(taps, TAP_WINDOWS, TAP_STRIDES)]
        b, (h, w) = taps[-1].shape[0], grids[-1]
        out = torch.empty((b, h * w, L3IMAC_DIMS), dtype=torch.float32, device=taps[-1].device)
        col = 0
        for t, grid, win, stride in zip(taps, grids, TAP_WINDOWS, TAP_STRIDES):
            c = t.shape[1]
            if grid == (h, w):
                _region_pool_l2(t, win, stride, out, col)
            else:
                r = _region_pool_l2(t, win, stride).view(b, grid[0], grid[1], c).permute(0, 3, 1, 2)
                r = F.normalize(F.adaptive_max_pool2d(r, (h, w)), p=2, dim=1)
                out[:, :, col : col + c] = r.permute(0, 2, 3, 1).reshape(b, h * w, c)
            col += c
        return _rows_l2norm(out)

    def _forward(self, x):
        with torch.no_grad():
            x = self.regions(self.taps(x))
            return x if self.pca is None else self.pca(x)
