"""DnS L3-iMAC region descriptors (`--baseline dns`, `inference_l3imac`) on the CPU: the eager restatement against the
definition written out with plain functional ops, the whitening, the recogniser, `CheckedFast` on [B, R, D] outputs,
the argument checks of the two kernels' entry points (no device needed) and the CLI.  The kernels and `FastL3iMAC` on
the GPU: tests/test_gpu_dns_inference.py."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F


def _frames(b, h, w, seed):
    return torch.randn((b, 3, h, w), generator=torch.Generator().manual_seed(seed))


def _restated(model, x):
    """The definition with forward hooks on the four stage ends and plain functional ops, in the model's order."""
    taps = []
    hooks = [model.trunk[i].register_forward_hook(lambda m, a, out: taps.append(out)) for i in (2, 6, 12, 15)]
    try:
        with torch.no_grad():
            model(x)
    finally:
        for h in hooks:
            h.remove()
    assert [t.shape[1] for t in taps] == [256, 512, 1024, 2048]
    pooled = []
    for t, s in zip(taps, (28, 14, 6, 3)):
        pooled.append(F.normalize(F.max_pool2d(t, s, stride=-(-s // 2)), p=2, dim=1))
    tap_grids = [tuple(r.shape[-2:]) for r in pooled]
    grid = tap_grids[-1]
    pooled = [F.normalize(F.adaptive_max_pool2d(r, grid), p=2, dim=1) for r in pooled]
    y = torch.cat(pooled, dim=1).permute(0, 2, 3, 1).reshape(x.shape[0], grid[0] * grid[1], 3840)
    return tap_grids, F.normalize(y, p=2, dim=-1)


@pytest.fixture(scope="module")
def plain_model():
    from vsc2022_amd.vsc.baseline.inference_l3imac import build_l3imac_model

    return build_l3imac_model(seed=3)


@pytest.mark.parametrize("h, w, grids", [(224, 224, [(3, 3)] * 4), (320, 320, [(4, 4), (4, 4), (5, 5), (4, 4)]),
                                         (224, 288, [(3, 4), (3, 4), (3, 5), (3, 4)])])
def test_l3imac_model_contract(plain_model, h, w, grids):
    """[B, R, 3840] with R the last tap's grid (9 at 224 x 224, 16 at 320 x 320 where the third tap's 5 x 5 grid goes
    through a real adaptive pool, 12 at 224 x 288), unit rows, equal to the restated definition to fp32 noise (same ops,
    same order)."""
    x = _frames(2, h, w, seed=h + w)
    with torch.no_grad():
        y = plain_model(x)
    tap_grids, want = _restated(plain_model, x)
    assert tap_grids == grids
    R = grids[-1][0] * grids[-1][1]
    assert y.shape == (2, R, 3840) and y.dtype == torch.float32 and torch.isfinite(y).all()
    assert float((y.norm(dim=-1) - 1).abs().max()) <= 1e-5
    assert torch.allclose(y, want, rtol=1e-5, atol=1e-6), float((y - want).abs().max())
    assert float((y[0] - y[1]).abs().max()) > 1e-4  # (different frames, different descriptors)


def test_l3imac_model_refuses_a_frame_smaller_than_a_window(plain_model):
    with pytest.raises(ValueError):
        plain_model(_frames(1, 96, 96, seed=1))


def test_l3imac_whitening(plain_model):
    """dims=512: [B, 9, 512] = normalize((x - mean) @ DVt) of the 3840-d output with the same trunk weights; the buffers
    are what `build_l3imac_model` documents."""
    from vsc2022_amd.vsc.baseline.inference_l3imac import build_l3imac_model

    white = build_l3imac_model(dims=512, seed=3)
    for (ka, a), (kb, b) in zip(plain_model.state_dict().items(), white.state_dict().items()):
        assert ka == kb and torch.equal(a, b)
    keys = list(white.state_dict())
    assert keys[-2:] == ["pca.mean", "pca.DVt"] and keys[0] == "stem.0.weight"
    mean, DVt = white.pca.mean, white.pca.DVt
    assert mean.shape == (3840,) and DVt.shape == (3840, 512)
    assert 1e-3 < float(mean.abs().mean()) < 1e-1
    col = DVt.double().norm(dim=0)  # orthonormal columns scaled by 1 / sqrt(d), d geometric 1 .. 1/16
    assert abs(float(col[0]) - 1.0) < 1e-5 and abs(float(col[-1]) - 4.0) < 1e-4 and bool((col[1:] > col[:-1]).all())
    vn = DVt.double() / col
    assert float((vn.T @ vn - torch.eye(512, dtype=torch.float64)).abs().max()) < 1e-5
    x = _frames(2, 224, 224, seed=9)
    with torch.no_grad():
        y, base = white(x), plain_model(x)
    assert y.shape == (2, 9, 512)
    want = F.normalize((base - mean) @ DVt, p=2, dim=-1)
    assert torch.allclose(y, want, rtol=1e-5, atol=1e-6)


class _Resnet(nn.Module):
    """torchvision-style names (conv1, bn1, layer1 .. layer4, downsample, fc) around the same tensors."""

    def __init__(self, model):
        super().__init__()
        self.conv1, self.bn1, self.relu, self.maxpool = model.stem[0], model.stem[1], model.stem[2], model.stem[3]
        blocks = list(model.trunk)
        self.layer1, self.layer2 = nn.Sequential(*blocks[:3]), nn.Sequential(*blocks[3:7])
        self.layer3, self.layer4 = nn.Sequential(*blocks[7:13]), nn.Sequential(*blocks[13:])
        self.fc = nn.Linear(2048, 1000)  # never used


class _Export(nn.Module):
    def __init__(self, model):
        super().__init__()
        self.cnn = _Resnet(model)
        self.regions = model.regions
        self.pca = model.pca

    def forward(self, x):
        c = self.cnn
        x = c.maxpool(c.relu(c.bn1(c.conv1(x))))
        taps = []
        for layer in (c.layer1, c.layer2, c.layer3, c.layer4):
            x = layer(x)
            taps.append(x)
        x = self.regions(taps)
        return x if self.pca is None else self.pca(x)


@pytest.mark.parametrize("dims", [None, 64])
def test_l3imac_weights_are_recovered_from_an_export(tmp_path, dims):
    """A traced export with torchvision's parameter names and an unused fc (and, with dims, whitening buffers) comes back
    as an `L3iMACModel` that agrees with the source; the other recognisers refuse it."""
    import warnings

    from vsc2022_amd.vsc.baseline.inference import sscd_from_module
    from vsc2022_amd.vsc.baseline.inference_l3imac import L3iMACModel, build_l3imac_model, l3imac_from_module
    from vsc2022_amd.vsc.baseline.inference_vit import dino_from_module

    model = build_l3imac_model(dims=dims, seed=5)
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():  # non-trivial BatchNorms: the order of the tensors matters
        for m in model.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.add_(0.1 * torch.randn(m.weight.shape, generator=g))
                m.bias.add_(0.1 * torch.randn(m.bias.shape, generator=g))
                m.running_mean.add_(0.1 * torch.randn(m.bias.shape, generator=g))
                m.running_var.mul_(1.0 + 0.2 * torch.rand(m.bias.shape, generator=g))
    export = _Export(model).eval()
    keys = list(export.state_dict())
    assert keys[0] == "cnn.conv1.weight" and "cnn.layer1.0.down.0.weight" in keys and "cnn.fc.weight" in keys
    path = str(tmp_path / "l3imac.torchscript.pt")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # (the tracer warns about the window check on Python ints)
        torch.jit.trace(export, torch.zeros(1, 3, 224, 224)).save(path)
    loaded = torch.jit.load(path)
    back = l3imac_from_module(loaded)
    assert isinstance(back, L3iMACModel) and (back.pca is None) == (dims is None)
    x = _frames(2, 224, 224, seed=7)
    with torch.no_grad():
        got, want = back(x), model(x)
    assert got.shape == (2, 9, dims or 3840)
    assert torch.allclose(got, want, rtol=1e-4, atol=1e-5), float((got - want).abs().max())
    assert l3imac_from_module(export) is not None  # an eager module as well
    assert sscd_from_module(loaded) is None and dino_from_module(loaded) is None


def test_l3imac_recogniser_refuses_other_models(tmp_path):
    """An SSCD export, a depth-2 DINO export, nn.Linear and an L3-iMAC-shaped module that computes another function all
    give None."""
    from vsc2022_amd.vsc.baseline.inference import build_sscd_model
    from vsc2022_amd.vsc.baseline.inference_l3imac import L3iMACModel, build_l3imac_model, l3imac_from_module
    from vsc2022_amd.vsc.baseline.inference_vit import build_dino_model

    sscd = build_sscd_model(dims=64, seed=5, device="cpu", channels_last=False)
    sscd_path = str(tmp_path / "sscd.torchscript.pt")
    torch.jit.trace(sscd, torch.zeros(1, 3, 64, 64)).save(sscd_path)
    assert l3imac_from_module(torch.jit.load(sscd_path)) is None
    dino_path = str(tmp_path / "dino.torchscript.pt")
    torch.jit.trace(build_dino_model(seed=1, depth=2), torch.zeros(1, 3, 224, 224)).save(dino_path)
    assert l3imac_from_module(torch.jit.load(dino_path)) is None
    assert l3imac_from_module(nn.Linear(16, 8)) is None
    assert l3imac_from_module(object()) is None

    class NoFinalNorm(L3iMACModel):  # same tensors, another function: refused by the check on a random batch
        def forward(self, x):
            return 2.0 * super().forward(x)

    other = NoFinalNorm().eval()
    other.load_state_dict(build_l3imac_model(seed=2).state_dict())
    assert l3imac_from_module(other) is None


def test_checked_fast_gates_every_region_of_every_frame():
    """`CheckedFast` on [B, R, D] outputs: one bad region of one frame drops the fast network; a uniformly good one keeps
    it, and `first_batch_cosine` is the minimum over frames and regions."""
    from vsc2022_amd.vsc.baseline.inference_cli import CheckedFast

    g = torch.Generator().manual_seed(0)
    ref = F.normalize(torch.randn((4, 9, 32), generator=g), dim=-1)
    noise = F.normalize(torch.randn((4, 9, 32), generator=g), dim=-1)

    class Fixed(nn.Module):
        def __init__(self, y):
            super().__init__()
            self.y = y

        def forward(self, x):
            return self.y

    good = ref + 1e-3 * noise
    good[2, 5] = ref[2, 5] + 2e-2 * noise[2, 5]  # the worst region, still above the gate
    cos = F.cosine_similarity(ref, good, dim=-1)
    assert int(cos.argmin()) == 2 * 9 + 5 and 0.999 < float(cos.min()) < 0.9999
    ok = CheckedFast(Fixed(good), Fixed(ref), 0.999)
    y = ok(torch.zeros(4, 3))
    assert ok.checked and ok.use_fast and torch.equal(y, good)
    assert ok.first_batch_cosine == pytest.approx(float(cos.min()), abs=1e-6)

    bad = good.clone()
    bad[1, 7] = ref[1, 7] + 0.06 * noise[1, 7]  # one region of one frame below the gate; the frame as a whole is not
    assert float(F.cosine_similarity(ref[1, 7], bad[1, 7], dim=0)) < 0.999
    assert float(F.cosine_similarity(ref.reshape(4, -1), bad.reshape(4, -1), dim=1).min()) > 0.999
    gate = CheckedFast(Fixed(bad), Fixed(ref), 0.999)
    y = gate(torch.zeros(4, 3))
    assert gate.checked and not gate.use_fast and gate.first_batch_cosine < 0.999 and torch.equal(y, ref)
    assert torch.equal(gate(torch.zeros(4, 3)), ref)


def test_region_kernel_entry_points_refuse_bad_arguments_without_a_device():
    """Both entry points return VSC_ERR_INVALID before any device call (the pointers are never dereferenced), and
    B = 0 / rows = 0 are no-ops."""
    from vsc2022_amd import _lib

    L = _lib.lib()
    x, out = 0x10000, 0x20000  # non-null, aligned, never touched

    def pool(B=1, H=7, W=7, C=2048, win=3, stride=2, out_row=3840, out_col=1792, eps=1e-12, xp=x, op=out):
        return L.vsc_region_pool_l2_bf16(xp, op, B, H, W, C, win, stride, out_row, out_col, eps, None)

    assert pool(C=12) == _lib.VSC_ERR_INVALID
    assert pool(C=4104, out_row=8192, out_col=0) == _lib.VSC_ERR_INVALID
    assert pool(C=0) == _lib.VSC_ERR_INVALID
    assert pool(H=2) == _lib.VSC_ERR_INVALID and pool(W=2) == _lib.VSC_ERR_INVALID
    assert pool(out_row=3839) == _lib.VSC_ERR_INVALID and pool(out_col=-8) == _lib.VSC_ERR_INVALID
    assert pool(win=0) == _lib.VSC_ERR_INVALID and pool(stride=0) == _lib.VSC_ERR_INVALID
    assert pool(xp=None) == _lib.VSC_ERR_INVALID and pool(op=None) == _lib.VSC_ERR_INVALID
    assert pool(B=-1) == _lib.VSC_ERR_INVALID
    assert b"vsc_region_pool_l2_bf16" in L.vsc_last_error()
    assert pool(B=0) == _lib.VSC_OK and pool(B=0, xp=None, op=None) == _lib.VSC_OK
    with pytest.raises(ValueError):
        _lib.check(pool(C=12))

    assert L.vsc_rows_l2norm_f32(None, 4, 3840, 1e-12, None) == _lib.VSC_ERR_INVALID
    assert L.vsc_rows_l2norm_f32(out, 4, 0, 1e-12, None) == _lib.VSC_ERR_INVALID
    assert L.vsc_rows_l2norm_f32(out, -1, 8, 1e-12, None) == _lib.VSC_ERR_INVALID
    assert L.vsc_rows_l2norm_f32(out, 4, 8, -1.0, None) == _lib.VSC_ERR_INVALID
    assert b"vsc_rows_l2norm_f32" in L.vsc_last_error()
    assert L.vsc_rows_l2norm_f32(out, 0, 8, 1e-12, None) == _lib.VSC_OK
    assert L.vsc_rows_l2norm_f32(None, 0, 8, 1e-12, None) == _lib.VSC_OK


def test_cli_runs_an_l3imac_torchscript_export_cpu(tmp_path):
    """The reference's DnS command (`--baseline dns --torchscript_path ... --transforms RESIZE_224_SQUARE --store_fp16`)
    on the CPU: float16 [n, 9, 3840] region descriptors per video, the export's own; they load back with `load_features`
    and `dns_index.index_videos` accepts them (stub fine-grained student)."""
    import warnings

    from vsc2022_amd.vsc.baseline import dns_index
    from vsc2022_amd.vsc.baseline import inference_cli as cli
    from vsc2022_amd.vsc.baseline.inference_l3imac import build_l3imac_model
    from vsc2022_amd.vsc.storage import load_features

    data = tmp_path / "videos"
    data.mkdir()
    rng = np.random.default_rng(3)
    lens = [3, 2, 4]
    for v, k in enumerate(lens):
        np.save(data / f"Q{v:06d}.npy", rng.integers(0, 256, (k, 72, 96, 3), dtype=np.uint8))
    model = build_l3imac_model(seed=1)
    path = str(tmp_path / "resnet50_l3imac.torchscript.pt")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.jit.trace(model, torch.zeros(2, 3, 224, 224)).save(path)
    args = ["--baseline", "dns", "--torchscript_path", path, "--transforms", "RESIZE_224_SQUARE", "--store_fp16",
            "--batch_size", "3", "--dataset_path", str(data), "--video_extensions", "npy", "--video_reader", "NPY",
            "--accelerator", "cpu", "--output_file", str(tmp_path / "q.npz")]
    cli.main(cli.build_parser().parse_args(args))
    vfs = load_features(str(tmp_path / "q.npz"))
    assert [v.video_id for v in vfs] == [f"Q{v:06d}" for v in range(len(lens))]
    for v, vf in enumerate(vfs):
        assert vf.feature.dtype == np.float16 and vf.feature.shape == (lens[v], 9, 3840) and len(vf) == lens[v]
        frames = torch.from_numpy(np.load(data / f"Q{v:06d}.npy")).permute(0, 3, 1, 2)
        with torch.no_grad():
            direct = model(cli.device_transform(frames, cli.InferenceTransforms.RESIZE_224_SQUARE)).numpy()
        assert np.abs(direct - vf.feature.astype(np.float32)).max() <= 2.0 ** -11  # one rounding to half of |x| <= 1

    class Student:
        student_type, fg_type = "fg", "att"

        @staticmethod
        def index_video(x):
            assert x.dtype == torch.float32 and x.dim() == 3 and tuple(x.shape[1:]) == (9, 3840)
            return x[:, :, :128]

    indexed = dns_index.index_videos(Student(), vfs, torch.device("cpu"))
    assert [v.video_id for v in indexed] == [v.video_id for v in vfs]
    assert all(v.feature.shape == (n, 9, 128) and v.feature.dtype == np.float16 for v, n in zip(indexed, lens))
