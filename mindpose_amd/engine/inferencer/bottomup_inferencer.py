"""Bottom-up (associative-embedding) inference engine (reference: mindpose/engine/inferencer/bottomup_inferencer.py:18-250).

The network and the decoder run on the HIP path (``EvalNet(net, BottomUpHeatMapAEDecoder)``), and so does the grouping: one
``mp_bottomup_match_by_tag`` launch per batch (``match_by_tag_batch``), bit-equal to the host ``match_by_tag``, which serves arrays
that live on the CPU, extents outside the kernel's limits and ``MINDPOSE_MATCH_DEVICE=0``.  The back-projection is host numpy, as
in the reference.  Behind the device grouping the rest of ``_parse`` stays on the device too (``finish_people_batch``: the
per-person scores, the mean tags and the optional missing-joint refinement in the two launches of ``mp_bottomup_finish_people``,
then two downloads; ``MINDPOSE_FINISH_DEVICE=0``: the host-driven tail below).  Without it the optional missing-joint refinement
still runs on the device (``mp_bottomup_refine_missing``, one launch per batch): the full-resolution maps never travel to the
host - only the located tags of the grouped persons ([J_total, L]) come down and their mean tags ([P, L]) go up.  Maps that
already live on the CPU take the host function ``refine_missing_joint``.

Flip TTA (``hflip_tta``, the reference's ``_MultiRunNet``, :252-297): the backbone and head run on the image and its mirror, and the
decoder folds the mirrored run into its own first launch (``decode_flip_aggregated``); the two decodes the reference computes and
throws away (:270, :272) are skipped.
"""
from functools import partial
from typing import Any, Dict, Iterable, List, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from ... import _lib
from ...data.transform.utils import transform_keypoints
from ...models import EvalNet
from ...models.decoders import BottomUpHeatMapAEDecoder
from ...models.layers import flip_pair_batched
from ...register import register
from ...utils.match import finish_people_batch, host_match_of, match_by_tag, match_by_tag_batch, match_on_device_supported


# MINDPOSE_FINISH_DEVICE when the environment does not set it (DESIGN.md 4.13 holds the measurement that decided it)
FINISH_DEVICE_DEFAULT = True


class _MultiRunNet(nn.Module):
    """Running the inference twice with horizontal-flip TTA (bottomup_inferencer.py:252-297); what is computed, and where the
    reference's own expression cannot run, is in ``BottomUpHeatMapAEDecoder.decode_flip_aggregated``."""

    def __init__(self, net: EvalNet, decoder: BottomUpHeatMapAEDecoder, flip_index: np.ndarray) -> None:
        super().__init__()
        self.net = net
        self.decoder = decoder
        self.flip_index = decoder.check_flip_index(flip_index)

    @torch.no_grad()
    def forward(self, image: torch.Tensor, mask: torch.Tensor) -> Tuple[torch.Tensor, ...]:
        raw_net = self.net.net  # EvalNet.net: backbone + head
        # planned network under amp O2 / O3: both runs as ONE 2N-image forward, its halves handed to the decoder as views.  The fp16
        # kernels give the same bits whatever the tile shape; the tuner may pick another fp32 form for the 2N shapes, so fp32 keeps
        # the two forwards (as topdown_inferencer._MultiRunNet)
        if hasattr(raw_net, "forward_flip_pair") and getattr(raw_net, "amp_level", "O0") != "O0" and flip_pair_batched():
            n = image.shape[0]
            both = raw_net.forward_flip_pair(image)
            outputs, flipped = [o[:n] for o in both], [o[n:] for o in both]
        else:
            outputs = [o.clone() for o in raw_net(image)]  # the plan's output buffers are reused by the second run
            if hasattr(raw_net, "get_plan"):  # planned network: the mirror goes straight into its input buffer (mp_flip_width)
                flipped = raw_net(image, flip_width=True)
            else:
                flipped = raw_net(torch.flip(image, dims=[3]))
        return self.decoder.decode_flip_aggregated(outputs, flipped, self.flip_index, mask)


@register("inferencer", extra_name="bottomup_heatmap_ae")
class BottomUpHeatMapAEInferencer:
    """Runs the evaluation network over an iterable of batches and returns records ``{pred, score, image_path}``."""

    def __init__(self, net: EvalNet, config: Optional[Dict[str, Any]] = None, progress_bar: bool = False,
                 decoder: Optional[BottomUpHeatMapAEDecoder] = None) -> None:
        self.net = net
        self.config = config if config else dict()
        self._inference_cfg = self.load_inference_cfg()
        self.progress_bar = progress_bar
        self.decoder = decoder
        if self.decoder is None and self._inference_cfg["hflip_tta"]:
            raise ValueError("Decoder must be provided for flip TTA")
        if self._inference_cfg["hflip_tta"] and not self._inference_cfg["has_heatmap_output"]:
            raise ValueError("flip TTA need heatmap output.")
        if self._inference_cfg["hflip_tta"]:
            if not isinstance(self.decoder, BottomUpHeatMapAEDecoder):
                raise NotImplementedError("bottom-up flip TTA on the HIP path needs the HIP decoder (BottomUpHeatMapAEDecoder): "
                                          "its first launch is what folds the mirrored run in")
            self._multi_run_net = _MultiRunNet(self.net, self.decoder, self._inference_cfg["flip_index"])  # ValueError: bad flip_index
            self._multi_run_net.eval()
        else:
            self._multi_run_net = None

    def load_inference_cfg(self) -> Dict[str, Any]:
        """bottomup_inferencer.py:66-89."""
        c = self.config
        cfg = dict(has_heatmap_output=c["has_heatmap_output"], hflip_tta=c["hflip_tta"], joint_order=c["joint_order"],
                   vis_thr=float(c["vis_thr"]), ignore_too_much=c["ignore_too_much"], use_rounded_norm=c["use_rounded_norm"],
                   tag_thr=float(c["tag_thr"]), pixel_std=float(c["pixel_std"]), downsample_scale=c["downsample_scale"],
                   refine_missing_joint=c["refine_missing_joint"])
        flip_index = np.array(c["flip_pairs"])[:, ::-1].flatten()
        cfg["flip_index"] = np.insert(flip_index, 0, 0)
        return cfg

    def __call__(self, dataset: Iterable[Dict[str, Any]]) -> List[Dict[str, Any]]:
        return self.infer(dataset)

    @torch.no_grad()
    def infer(self, dataset: Iterable[Dict[str, Any]]) -> List[Dict[str, Any]]:
        """``dataset`` yields dicts with ``image, mask`` (CUDA tensors) and ``center, scale, image_shape, image_file``;
        returns one record ``{pred [P, K, 3 + L], score [P], image_path}`` per image (:91-187)."""
        outputs = []
        for data in dataset:
            if self._inference_cfg["hflip_tta"]:
                preds = self._multi_run_net(data["image"], data["mask"])
            elif self._inference_cfg["has_heatmap_output"]:
                preds, _ = self.net(data["image"], data["mask"])
            else:
                preds = self.net(data["image"], data["mask"])
            keypoints, scores = self._parse(*preds)
            center, scale, image_shape = (np.asarray(data[k].cpu() if torch.is_tensor(data[k]) else data[k])
                                          for k in ("center", "scale", "image_shape"))
            keypoints = transform_keypoints(keypoints, center, scale, image_shape / self._inference_cfg["downsample_scale"],
                                            pixel_std=self._inference_cfg["pixel_std"])
            paths = data.get("image_file", [None] * len(keypoints))
            for pred, score, path in zip(keypoints, scores, paths):
                outputs.append(dict(pred=pred, score=score, image_path=path.tolist() if hasattr(path, "tolist") else path))
        return outputs

    def _parse(self, val_k, tag_k, ind_k, heatmap, tagging_heatmap) -> Tuple[List[np.ndarray], List[List[float]]]:
        """Grouping, per-person score (mean joint value) and the optional missing-joint refinement (:120-150).  With maps on the
        device and everything ``_match`` asks of the device grouping, all three stay there (``MINDPOSE_FINISH_DEVICE=0``: never): the
        grouping launch, the two launches of ``mp_bottomup_finish_people`` and two downloads (``finish_people_batch``) - the same
        records."""
        if heatmap.is_cuda and tagging_heatmap.is_cuda and _lib.env_on("MINDPOSE_FINISH_DEVICE", default=FINISH_DEVICE_DEFAULT) \
                and self._match_on_device(val_k, tag_k, ind_k):
            kwargs = self._match_kwargs()
            people, counts, status = match_by_tag_batch(val_k, tag_k, ind_k, download=False, **kwargs)  # match_by_tag_device
            return finish_people_batch(people, counts, status, heatmap, tagging_heatmap, self._inference_cfg["refine_missing_joint"],
                                       host_match_of(val_k, tag_k, ind_k, **kwargs))
        keypoints = self._match(val_k, tag_k, ind_k)
        scores = [[person[:, 2].mean() for person in people] for people in keypoints]
        if self._inference_cfg["refine_missing_joint"]:
            if heatmap.is_cuda:
                self._refine_on_device(keypoints, heatmap, tagging_heatmap)
            else:
                heatmap = heatmap.numpy()
                tagging_heatmap = tagging_heatmap.numpy()
                if tagging_heatmap.shape[1] != heatmap.shape[1]:  # one tag map for all joints (tag_per_joint=False)
                    tagging_heatmap = np.broadcast_to(tagging_heatmap, heatmap.shape[:2] + tagging_heatmap.shape[2:])
                for i in range(len(keypoints)):
                    for j in range(len(keypoints[i])):
                        keypoints[i][j] = refine_missing_joint(heatmap[i], tagging_heatmap[i], keypoints[i][j])
        return keypoints, scores

    @staticmethod
    def _refine_on_device(keypoints: List[np.ndarray], heatmap: torch.Tensor, tagging_heatmap: torch.Tensor) -> None:
        """``refine_missing_joint`` for every person of the batch, in place: one indexed read of the located tags, the mean tag per
        person with the reference's own ``np.mean`` on the host, one ``mp_bottomup_refine_missing`` launch, the reference's rule
        ``found[j, 2] > 0 and keypoints[j, 2] == 0`` on the downloaded ``found`` [P, K, 3]."""
        n, k, h, w = heatmap.shape
        ktag, num_tags = tagging_heatmap.shape[1], tagging_heatmap.shape[4]
        persons, index, counts = [], [], []
        for i in range(len(keypoints)):
            for person in keypoints[i]:
                located = person[:, :2].astype(np.int32)
                joints = np.flatnonzero(person[:, 2] > 0)
                if joints.size == 0:  # (grouping builds a person from at least one detection)
                    continue
                persons.append((i, person))
                counts.append(joints.size)
                index.append(np.stack([np.full(joints.size, i), joints if ktag > 1 else np.zeros_like(joints),
                                       np.clip(located[joints, 1], 0, h - 1), np.clip(located[joints, 0], 0, w - 1)]))
        if not persons:
            return
        dev = heatmap.device
        heatmap = _lib.require_cuda_f32(heatmap, "heatmap")
        tagging_heatmap = _lib.require_cuda_f32(tagging_heatmap, "tagging_heatmap")
        img, ch, ys, xs = torch.from_numpy(np.concatenate(index, axis=1).astype(np.int64)).to(dev)
        tags = tagging_heatmap[img, ch, ys, xs].cpu().numpy()  # [J_total, L]
        starts = np.concatenate([[0], np.cumsum(counts)])
        mean_tag = np.stack([np.mean(tags[starts[p]:starts[p + 1]], axis=0) for p in range(len(persons))]).astype(np.float32)
        mean_dev = torch.from_numpy(np.ascontiguousarray(mean_tag)).to(dev)
        image_dev = torch.tensor([i for i, _ in persons], dtype=torch.int32, device=dev)
        found = torch.empty(len(persons), k, 3, device=dev, dtype=torch.float32)
        _lib.check(_lib.load().mp_bottomup_refine_missing(_lib.ptr(heatmap), _lib.ptr(tagging_heatmap), _lib.ptr(mean_dev),
                                                          _lib.ptr(image_dev), len(persons), n, k, h, w, int(ktag > 1 or k == 1),
                                                          num_tags, _lib.ptr(found), _lib.stream()), "mp_bottomup_refine_missing")
        found = found.cpu().numpy()
        for (_, person), rows in zip(persons, found):
            fill = (rows[:, 2] > 0) & (person[:, 2] == 0)
            person[fill, :3] = rows[fill]

    def _match_kwargs(self) -> Dict[str, Any]:
        cfg = self._inference_cfg
        return dict(joint_order=cfg["joint_order"], vis_thr=cfg["vis_thr"], tag_thr=cfg["tag_thr"],
                    ignore_too_much=cfg["ignore_too_much"], use_rounded_norm=cfg["use_rounded_norm"])

    @staticmethod
    def _match_on_device(val_k, tag_k, ind_k) -> bool:
        return val_k.is_cuda and tag_k.is_cuda and ind_k.is_cuda and _lib.env_on("MINDPOSE_MATCH_DEVICE") \
            and match_on_device_supported(val_k.shape[1], val_k.shape[2], tag_k.shape[3])

    def _match(self, val_k, tag_k, ind_k) -> List[np.ndarray]:
        """Grouping of the batch: one ``mp_bottomup_match_by_tag`` launch when the decoder's arrays live on the device and are inside
        the entry's limits (``MINDPOSE_MATCH_DEVICE=0``: never), else the host function image by image - the same arrays either way."""
        kwargs = self._match_kwargs()
        if self._match_on_device(val_k, tag_k, ind_k):
            return match_by_tag_batch(val_k, tag_k, ind_k, **kwargs)
        return list(map(partial(match_by_tag, **kwargs), val_k.cpu().numpy(), tag_k.cpu().numpy(), ind_k.cpu().numpy()))


def refine_missing_joint(heatmap: np.ndarray, tagging_heatmap: np.ndarray, keypoints: np.ndarray) -> np.ndarray:
    """Fill the joints of one person that grouping left empty (bottomup_inferencer.py:189-250).  heatmap [K, H, W],
    tagging_heatmap [K, H, W, L], keypoints [K, 3 + L] (updated in place and returned): per joint, the pixel maximising
    heat-map value minus the rounded L2 distance between its tag and the person's mean tag, at its centre (+0.5) shifted
    0.25 towards the larger horizontal / vertical neighbour; taken only where the person has no value and the pixel's is > 0."""
    k, h, w = heatmap.shape
    located = keypoints[:, :2].astype(np.int32)
    person_tags = [tagging_heatmap[j, located[j, 1], located[j, 0]] for j in range(k) if keypoints[j, 2] > 0]
    mean_tag = np.mean(person_tags, axis=0)

    dist = np.round(np.linalg.norm(tagging_heatmap - mean_tag[None, None, None, :], axis=3))
    best = np.argmax((heatmap - dist).reshape(k, -1), axis=1)
    ys_int, xs_int = np.unravel_index(best, (h, w))
    xs = xs_int.astype(np.float32) + 0.5
    ys = ys_int.astype(np.float32) + 0.5
    for j in range(k):
        x, y = xs_int[j], ys_int[j]
        xs[j] += 0.25 if heatmap[j, y, min(x + 1, w - 1)] > heatmap[j, y, max(x - 1, 0)] else -0.25
        ys[j] += 0.25 if heatmap[j, min(y + 1, h - 1), x] > heatmap[j, max(0, y - 1), x] else -0.25

    vals = heatmap[np.arange(k), ys_int, xs_int]
    found = np.stack((xs, ys, vals), axis=1)
    for j in range(k):
        if found[j, 2] > 0 and keypoints[j, 2] == 0:
            keypoints[j, :3] = found[j]
    return keypoints
