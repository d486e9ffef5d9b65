"""DnS matching baseline on the MI355X engine: coarse-descriptor search -> candidates -> Temporal-Network
localisation on a FINE-GRAINED similarity produced by a torch network.

Drop-in for `python -m vsc.baseline.dns_baseline` of the reference (same flags, same output files, same
module-level names `VCSLLocalizationDnS`, `search`, `localize_and_verify`, `match`, `main`;
/root/reference/vsc/baseline/dns_baseline.py:52-290).

`VCSLLocalizationDnS` (reference :108-163): the frame x frame matrix handed to the aligner comes from a
caller-supplied similarity network on FINE (region-level) descriptors, optionally symmetrised, mapped to
[0, 1] and combined with the coarse inner-product similarity (+ bias) by a geometric mean.  The reference gets
the network from a TorchScript file (`dns_fine_grained_student`); no weights exist in this environment, so the
network is whatever `torch.jit.load` / the caller supplies: any callable `sim_model(query [Lq, ...], ref [Lr, ...])
-> [Lq, Lr]` with an `fg_type` attribute.  The fine descriptors arrive as the reference's callers pass them --
`Dict[video_id, VideoFeature]` (`convert_to_dict`, reference :183-186, 260-264) -- or as a list.

Because `similarity()` is overridden, `localize_all` takes the reference's route of
`vsc2022_amd.vsc.baseline.localization.VCSLLocalization`: one matrix per pair (the coarse part computed on the
GPU by libvscmi), alignment of all of them in one `vsc_tn_forward_sim` call, MaxSim score per box.

`on_device=True` (opt-in; the default is the route above, unchanged) keeps every matrix in HBM: `_device_route` then
names `_launch_fine`, and the batch goes the base class's way from candidates to rows.  Stage 1 produces the
fine matrices F = sim / 2 + 0.5 of a batch in one device slab: an exact `ChamferSimilarity` instance -- the part of a
fine-grained student that has no weights -- runs in libvscmi on fine descriptors that went down once
(`vsc_tn_set_fine`, `vsc_tn_fine_similarity`: region Chamfer on the matrix cores); any other model runs as before, per
pair, on `torch_device` (a GPU), with its descriptors uploaded once per unique video of the batch.  Stage 2
(`vsc_tn_localize_fine`) blends the slab with the coarse similarity inside the Temporal-Network kernel, aligns and
scores; nothing is copied to the host before the box table.  The arithmetic is written down in include/vscmi.h ("DnS
localisation on the device"): with a torch model both routes see the same F bits and return equal matches; with
`ChamferSimilarity` the device route has the bits of the CPU restatement in tests/dns_fine_ref.py.

`fine_codec="bits"` (with on_device=True and `ChamferSimilarity("bin")` only) keeps the binary student's descriptors in
HBM as the bits they are, 1/32 of the default +-1 fp32 rows: each video is packed on the host
(`pack_fine_bits`), `vsc_tn_set_fine_bits` stores the rows and stage 1 runs on xor + popcount (fine_bits.hip).  The
results are the bits of the default store: include/vscmi.h writes down why.

`fine_codec="SQfp16"` (with on_device=True and `ChamferSimilarity` WITHOUT "bin" only) keeps the attention student's
descriptors in HBM as half floats -- what dns_index writes for it (`feature.half()`) -- at half the bytes of the default
fp32 rows.  float16 features go down as they are (`vsc_tn_set_fine_f16`, no fp32 copy on the host, half the transfer)
and give the default store's results bit for bit; other dtypes are rounded to half by the library (round to nearest
even), and the results are those of the default store on the rounded values.  A value a half cannot hold (NaN, inf,
beyond +-65504) is a ValueError.
"""
import argparse
import ctypes
import logging
import os
from typing import Dict, List, Mapping, Sequence, Tuple, Union

import numpy as np
import torch

from vsc2022_amd import _lib
from vsc2022_amd.vsc import metrics as M
from vsc2022_amd.vsc import storage
from vsc2022_amd.vsc.baseline.dns_index import Accelerator
from vsc2022_amd.vsc.baseline.localization import VCSLLocalizationMaxSim
from vsc2022_amd.vsc.candidates import CandidateGeneration, MaxScoreAggregation
from vsc2022_amd.vsc.index import VideoFeature
from vsc2022_amd.vsc.metrics import CandidatePair, Match

logger = logging.getLogger("dns_baseline.py")
logger.setLevel(logging.INFO)

FineFeatures = Union[Mapping[object, VideoFeature], Sequence[VideoFeature]]


def _by_id(features: FineFeatures) -> Dict[object, VideoFeature]:
    if isinstance(features, Mapping):
        return dict(features)
    return {v.video_id: v for v in features}


FINE_CODECS = ("bits", "SQfp16")


def pack_fine_bits(feature) -> np.ndarray:
    """Binary fine descriptors [..., D] (bool, or integers {0, 1}) -> [..., ceil(D / 8)] bytes, element d in bit d % 8 of
    byte d / 8: the packed input of `vsc_tn_set_fine_bits`."""
    return np.packbits(np.asarray(feature) > 0, axis=-1, bitorder="little")


def _check_fine_codec(fine_codec, on_device: bool, model):
    """What `fine_codec` can be asked for, judged before anything touches a device."""
    if fine_codec is None:
        return
    if fine_codec not in FINE_CODECS:
        raise ValueError(f"unknown fine_codec {fine_codec!r} (None or one of {FINE_CODECS})")
    if not on_device:
        raise ValueError(f"fine_codec={fine_codec!r} is a store of the device route: it needs on_device=True")
    binary = "bin" in getattr(model, "fg_type", "")
    if fine_codec == "SQfp16":
        if type(model) is not ChamferSimilarity:
            raise ValueError(f"fine_codec={fine_codec!r} keeps half-float descriptors for libvscmi's region Chamfer kernel: the "
                             "model must be exactly ChamferSimilarity (a torch model holds its own tensors)")
        if binary:
            raise ValueError(f"fine_codec={fine_codec!r} is the store of an attention student's descriptors: for a binary "
                             "student (\"bin\" in fg_type) the store to use is fine_codec=\"bits\"")
        return
    if type(model) is not ChamferSimilarity or not binary:
        raise ValueError(f"fine_codec={fine_codec!r} packs binary descriptors for libvscmi's region Chamfer kernel: the model "
                         "must be exactly ChamferSimilarity with \"bin\" in fg_type")


class ChamferSimilarity(torch.nn.Module):
    """The ViSiL / DnS frame-to-frame region Chamfer similarity, the part of a fine-grained student that has no weights:
    inner products of all region pairs of two frames, max over the second argument's regions, mean over the first's.
    `a` [La, R, D], `b` [Lb, R, D] -> [La, Lb].  `fg_type` as the reference reads it: "bin" descriptors arrive rescaled
    to {-1, +1} and their inner product is divided by the width.  A model like any other on the host route; with
    `VCSLLocalizationDnS(on_device=True)` an instance of exactly this class is computed by libvscmi (fine_sim.hip)."""

    def __init__(self, fg_type: str = "att"):
        super().__init__()
        self.fg_type = fg_type
        self.student_type = "fg"

    def forward(self, a, b):
        s = torch.einsum("ird,jsd->ijrs", a, b)
        if "bin" in self.fg_type:
            s = s / a.shape[-1]
        return s.max(dim=3).values.mean(dim=2)


class VCSLLocalizationDnS(VCSLLocalizationMaxSim):
    def __init__(self, model, queries_fine: FineFeatures, refs_fine: FineFeatures,
                 queries_coarse: List[VideoFeature], refs_coarse: List[VideoFeature], model_type, device,
                 symmetric: bool = True, geometric_mean: bool = True, on_device: bool = False, fine_codec=None, **kwargs):
        # the reference stores what it was given (a torch.device or the --accelerator string) and only ever hands it
        # to Tensor.to(); "cuda" is the ROCm device under PyTorch-ROCm
        torch_device = device if isinstance(device, torch.device) else torch.device(device)
        self._chamfer = type(model) is ChamferSimilarity
        _check_fine_codec(fine_codec, bool(on_device), model)
        self.fine_codec = fine_codec
        if on_device:  # (checked before the descriptors go anywhere)
            if model_type != "TN":
                raise ValueError(f"on_device=True aligns with the Temporal Network kernel: model_type {model_type!r} is not \"TN\"")
            if type(self).score is not VCSLLocalizationMaxSim.score or type(self).similarity is not VCSLLocalizationDnS.similarity:
                raise ValueError("on_device=True needs the stock MaxSim score and similarity: an override cannot run in the kernel")
            if not self._chamfer and torch_device.type != "cuda":
                raise ValueError(f"on_device=True runs a torch similarity model on a GPU device, not on {torch_device}")
        super().__init__(queries_coarse, refs_coarse, model_type, **kwargs)
        self.queries_fine = _by_id(queries_fine)
        self.refs_fine = _by_id(refs_fine)
        self.sim_model = model
        self.torch_device = torch_device
        self.symmetric = symmetric
        self.geometric_mean = geometric_mean
        self.on_device = bool(on_device)
        self._bound_stream = None
        if self.on_device:
            self._q_len = np.array([len(v) for v in self._q_videos], dtype=np.int64)
            self._r_len = np.array([len(v) for v in self._r_videos], dtype=np.int64)
            if self._chamfer:
                self._upload_fine()

    # -- on_device=True ----------------------------------------------------------------------------
    def _upload_fine(self):
        """The fine descriptors of both sides, in the order of the context's videos, down once (vsc_tn_set_fine; with
        fine_codec="bits" packed video by video first, so that the host staging copy is D / 8 bytes per region, and
        handed to vsc_tn_set_fine_bits; with fine_codec="SQfp16" handed to vsc_tn_set_fine_f16, as the halves they are
        when every video's descriptors are float16 -- no fp32 copy exists on the host -- and as fp32 otherwise)."""
        binary = "bin" in self.sim_model.fg_type
        bits = self.fine_codec == "bits"
        half = self.fine_codec == "SQfp16"
        sides = []
        for videos, table in ((self._q_videos, self.queries_fine), (self._r_videos, self.refs_fine)):
            parts = []
            for v in videos:
                x = np.asarray(table[v.video_id].feature)
                if x.ndim != 3 or len(x) != len(v):
                    raise ValueError(f"video {v.video_id!r}: fine descriptors of shape {x.shape} for {len(v)} frames ([L, R, D] expected)")
                parts.append((x.shape[1:], pack_fine_bits(x)) if bits else (x.shape[1:], x))
            sides.append(parts)
        shapes = {shape for parts in sides for shape, _ in parts}
        if len(shapes) > 1:
            raise ValueError(f"fine descriptors differ in regions x width: {sorted(shapes)}")
        if not shapes:
            return
        regions, width = shapes.pop()
        dtype = np.uint8 if binary else np.float32
        if half and all(x.dtype == np.float16 for parts in sides for _, x in parts):
            dtype = np.float16
        rows = [np.ascontiguousarray(np.concatenate([x for _, x in parts], axis=0), dtype=dtype) if parts else None for parts in sides]
        addr = [x.ctypes.data if x is not None and x.size else None for x in rows]
        if bits:
            _lib.check(_lib.lib().vsc_tn_set_fine_bits(self._ctx, addr[0], addr[1], int(regions), int(width), 1, _lib.MEM_HOST))
        elif half:
            _lib.check(_lib.lib().vsc_tn_set_fine_f16(self._ctx, addr[0], addr[1], int(regions), int(width),
                                                      int(dtype == np.float16), _lib.MEM_HOST))
        else:
            _lib.check(_lib.lib().vsc_tn_set_fine(self._ctx, addr[0], addr[1], int(regions), int(width),
                                                  _lib.FINE_BIN if binary else _lib.FINE_ATT, _lib.MEM_HOST))

    @property
    def fine_bytes(self) -> int:
        """Bytes of HBM the context holds for the fine descriptor rows (`ChamferSimilarity` with on_device=True)."""
        return int(_lib.lib().vsc_tn_fine_bytes(self._ctx))

    def _slab_device(self) -> torch.device:
        return torch.device("cuda", self.device)

    def _bind_stream(self):
        """The context's launches follow torch's on torch's current stream (as engine.bind_aux_stream does for the
        entry points without a handle): the slab torch wrote is read without a device-wide synchronisation."""
        tdev = self._slab_device()
        if os.environ.get("VSC_TORCH_STREAM", "1") == "0":
            torch.cuda.synchronize(tdev)
            return
        st = torch.cuda.current_stream(tdev).cuda_stream
        if self._bound_stream != st:
            _lib.check(_lib.lib().vsc_tn_set_stream(self._ctx, ctypes.c_void_p(st), 0))
            self._bound_stream = st

    @torch.no_grad()
    def _model_fine(self, q: torch.Tensor, r: torch.Tensor) -> torch.Tensor:
        """F of one pair by the torch model, on `torch_device`: for `similarity` and for the slab of the device route."""
        sim = self.sim_model(q, r)
        if self.symmetric:
            sim = (sim + self.sim_model(r, q).mT) / 2.0
        return sim / 2.0 + 0.5

    def _load_fine(self, table, video_id) -> torch.Tensor:
        """A video's fine descriptors as the model takes them: fp32 on `torch_device`, binaries rescaled."""
        t = torch.from_numpy(np.asarray(table[video_id].feature)).to(self.torch_device).float()
        return self._rescale_binaries(t)

    def _fine_tensor(self, table, video_id, cache) -> torch.Tensor:
        t = cache.get(video_id)
        if t is None:
            t = cache[video_id] = self._load_fine(table, video_id)
        return t

    def _fine_slab(self, candidates, pair_q: np.ndarray, pair_r: np.ndarray):
        """Stage 1: (slab, offsets) in HBM -- F of pair k, row-major, at slab[offsets[k]:]."""
        n = len(candidates)
        lq, lr = self._q_len[pair_q], self._r_len[pair_r]
        cells = lq * lr
        off = np.zeros(n, dtype=np.int64)
        np.cumsum(cells[:-1], out=off[1:])
        total = int(cells.sum())
        tdev = self._slab_device()
        slab = torch.empty(max(total, 1), dtype=torch.float32, device=tdev)
        d_off = torch.from_numpy(off).to(tdev)
        if self._chamfer:
            self._bind_stream()
            _lib.check(_lib.lib().vsc_tn_fine_similarity(
                self._ctx, pair_q.ctypes.data, pair_r.ctypes.data, n, _lib.MEM_HOST, int(bool(self.symmetric)),
                slab.data_ptr(), d_off.data_ptr(), total, _lib.MEM_DEVICE))
            return slab, d_off
        q_cache, r_cache = {}, {}  # one upload per unique video of the batch
        for k, c in enumerate(candidates):
            if cells[k] == 0:
                continue
            f = self._model_fine(self._fine_tensor(self.queries_fine, c.query_id, q_cache),
                                 self._fine_tensor(self.refs_fine, c.ref_id, r_cache))
            slab[int(off[k]) : int(off[k] + cells[k])].view(int(lq[k]), int(lr[k])).copy_(f)
        self._bind_stream()
        return slab, d_off

    def _device_route(self):
        """on_device=True: both stages in HBM (`_launch_fine`).  Otherwise the base class's choice: with `similarity`
        overridden here, the reference's route through it."""
        return self._launch_fine if self.on_device else super()._device_route()

    def _launch_fine(self, candidates, table):
        """Both stages of a batch: the fine slab, then blend, alignment and scores (libvscmi vsc_tn_localize_fine)."""
        slab, d_off = self._fine_slab(candidates, table.pair_q, table.pair_r)
        _lib.check(_lib.lib().vsc_tn_localize_fine(
            self._ctx, table.pair_q.ctypes.data, table.pair_r.ctypes.data, len(table.pair_q), _lib.MEM_HOST, slab.data_ptr(),
            d_off.data_ptr(), _lib.MEM_DEVICE, int(bool(self.geometric_mean)), ctypes.byref(self.model.params),
            float(self.similarity_bias), table.n_boxes.ctypes.data, table.boxes.ctypes.data, table.box_max.ctypes.data,
            _lib.MEM_HOST))

    def _device_similarity_fine(self, candidate: CandidatePair) -> np.ndarray:
        """S of one pair: stage 1 for it alone, blended by libvscmi (vsc_tn_similarity_fine)."""
        pair_q, pair_r = self._pair_ordinals([candidate])
        slab, _ = self._fine_slab([candidate], pair_q, pair_r)
        out = np.empty((int(self._q_len[pair_q[0]]), int(self._r_len[pair_r[0]])), dtype=np.float32)
        _lib.check(_lib.lib().vsc_tn_similarity_fine(
            self._ctx, int(pair_q[0]), int(pair_r[0]), float(self.similarity_bias), slab.data_ptr(), _lib.MEM_DEVICE,
            int(bool(self.geometric_mean)), out.ctypes.data, out.size, None, None))
        return out

    def _rescale_binaries(self, x):
        if "bin" in getattr(self.sim_model, "fg_type", ""):
            x = 2 * x - 1
        return x

    @torch.no_grad()
    def similarity(self, candidate: CandidatePair):
        if self.on_device:
            return self._device_similarity_fine(candidate)
        sim = self._model_fine(self._load_fine(self.queries_fine, candidate.query_id),
                               self._load_fine(self.refs_fine, candidate.ref_id)).cpu().numpy()
        if self.geometric_mean:
            coarse = self._device_similarity(candidate, self.similarity_bias)  # q @ r.T + bias, on the GPU
            sim = np.sqrt(sim.clip(1e-7) * coarse.clip(1e-7))
        return sim


def search(queries: List[VideoFeature], refs: List[VideoFeature], retrieve_per_query: float = 1200.0,
           candidates_per_query: float = 25.0) -> List[CandidatePair]:
    """Best `candidates_per_query * len(queries)` video pairs on the COARSE descriptors (reference :166-180)."""
    n_hits = int(retrieve_per_query * len(queries))
    n_keep = int(candidates_per_query * len(queries))
    pairs = CandidateGeneration(refs, MaxScoreAggregation()).query(queries, global_k=n_hits)[:n_keep]
    logger.info("Got %d candidates", len(pairs))
    return pairs


def localize_and_verify(model, queries_fine: FineFeatures, refs_fine: FineFeatures, queries_coarse: List[VideoFeature],
                        refs_coarse: List[VideoFeature], candidates: Sequence[CandidatePair],
                        localize_per_query: float = 5.0, device="cpu", on_device: bool = False, fine_codec=None) -> List[Match]:
    """Reference :183-227: the best `localize_per_query * len(queries_fine)` candidates, batches of 512 pairs.
    on_device: `VCSLLocalizationDnS(on_device=True)`, every matrix stays in HBM; fine_codec: its store of the fine rows
    (one of FINE_CODECS)."""
    todo = candidates[: int(len(queries_fine) * localize_per_query)]
    aligner = VCSLLocalizationDnS(model, queries_fine, refs_fine, queries_coarse, refs_coarse, model_type="TN",
                                  tn_max_step=5, min_length=4, concurrency=16, similarity_bias=0.5, device=device,
                                  on_device=on_device, fine_codec=fine_codec)
    found: List[Match] = []
    batch = 512
    for start in range(0, len(todo), batch):
        found += aligner.localize_all(todo[start : start + batch])
        logger.info("Aligned %d pairs of %d; %d predictions so far", min(start + batch, len(todo)), len(todo), len(found))
    return found


def match(model, queries_fine: FineFeatures, refs_fine: FineFeatures, queries_coarse: List[VideoFeature],
          refs_coarse: List[VideoFeature], output_path: str, device, on_device: bool = False,
          fine_codec=None) -> Tuple[str, str]:
    """Reference :230-258; returns the paths of candidates.csv and matches.csv."""
    pairs = search(queries_coarse, refs_coarse)
    os.makedirs(output_path, exist_ok=True)
    candidate_file = os.path.join(output_path, "candidates.csv")
    CandidatePair.write_csv(pairs, candidate_file)
    found = localize_and_verify(model, queries_fine, refs_fine, queries_coarse, refs_coarse, pairs, device=device,
                                on_device=on_device, fine_codec=fine_codec)
    matches_file = os.path.join(output_path, "matches.csv")
    Match.write_csv(found, matches_file)
    return candidate_file, matches_file


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="DnS matching baseline on MI355X")
    for flag, text in (("--torchscript_path", "Path to the fine-grained student model used for similarity calculation."),
                       ("--query_coarse_features", "Path to query coarse descriptors"),
                       ("--ref_coarse_features", "Path to reference coarse descriptors"),
                       ("--query_fine_features", "Path to query fine descriptors"),
                       ("--ref_fine_features", "Path to reference fine descriptors"),
                       ("--output_path", "The path to write match prediction.")):
        p.add_argument(flag, help=text, type=str, required=True)
    p.add_argument("--accelerator", help="Device used for the similarity calculation",
                   choices=[x.name.lower() for x in Accelerator], default="cpu", type=str)
    p.add_argument("--ground_truth", help="Path to the ground truth (labels) CSV file.", type=str)
    p.add_argument("--overwrite", help="Overwrite prediction files, if found.", action="store_true")
    p.add_argument("--on_device", help="Keep the similarity matrices of the localisation in HBM (needs a GPU accelerator).",
                   action="store_true")
    p.add_argument("--fine_codec", help="Store of the fine descriptors in HBM with --on_device: bits = 1 bit per value "
                   "(binary students through ChamferSimilarity only), SQfp16 = half floats (attention students through "
                   "ChamferSimilarity only).", choices=list(FINE_CODECS), default=None)
    return p


parser = build_parser()


def main(args):
    if getattr(args, "fine_codec", None) is not None and not args.on_device:
        raise ValueError("--fine_codec is a store of the device route: it needs --on_device")
    if os.path.exists(args.output_path) and not args.overwrite:
        raise Exception(f"Output path already exists: {args.output_path}. Do you want to --overwrite?")
    model = torch.jit.load(args.torchscript_path)
    if "fg" != model.student_type:
        raise Exception("Only fine-grained student are accepted for similarity calculation.")
    device = Accelerator[args.accelerator.upper()].get_device()
    model = model.eval().to(device)
    queries_fine = storage.convert_to_dict(storage.load_features(args.query_fine_features, M.Dataset.QUERIES))
    refs_fine = storage.convert_to_dict(storage.load_features(args.ref_fine_features, M.Dataset.REFS))
    queries_coarse = storage.load_features(args.query_coarse_features, M.Dataset.QUERIES)
    refs_coarse = storage.load_features(args.ref_coarse_features, M.Dataset.REFS)
    candidate_file, match_file = match(model, queries_fine, refs_fine, queries_coarse, refs_coarse, args.output_path,
                                       device, on_device=args.on_device, fine_codec=getattr(args, "fine_codec", None))
    if args.ground_truth:
        from vsc2022_amd.vsc.baseline.sscd_baseline import _report

        _report(args.output_path, args.ground_truth, candidate_file, match_file)


if __name__ == "__main__":
    logging.basicConfig(format="%(asctime)s %(levelname)-8s %(message)s", level=logging.INFO,
                        datefmt="%Y-%m-%d %H:%M:%S")
    main(parser.parse_args())
