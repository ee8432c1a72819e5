"""HigherHRNet-W32 bottom-up inference timings on one GPU; prints ONE JSON line.

  python tools/bench_bottomup.py [--steps 20]

- forward: network plan (tuner on) at N = 1 and N = 32 for fp32 and amp O2, with the algorithmic GFLOP per image recomputed from the
  plan's recorded MACs (2 FLOP per MAC);
- decoder: BottomUpHeatMapAEDecoder (two launches) at the eval map size 256 x 416 (N = 1) and 256 x 256 (N = 32), microseconds per
  image and the fraction of 8 TB/s reached on its algorithmic bytes (reads: 17 full-resolution heat maps + 34 half-resolution
  channels; writes: heatmap_raw + tagging);
- match_by_tag: host milliseconds per image on the decoder's output of random maps;
- resize_pad_normalize: ``mp_resize_pad_normalize`` of one 640 x 480 source to 832 x 512 (the evaluation input), device microseconds and
  the fraction of 8 TB/s on its algorithmic bytes (read: the uint8 source; written: three fp32 planes + the mask);
- refine: the missing-joint refinement of P = 1, 10, 30 persons at the 256 x 416 map - the device path (tag gather, mean tags, one
  ``mp_bottomup_refine_missing`` launch, the download of ``found``) against the host path (``refine_missing_joint`` per person after
  the two ``.cpu()`` copies of the maps), wall milliseconds per batch, and the kernel alone in device microseconds;
- train_augment: the train-time augmentation of a batch, N = 32 sources of 640 x 480 to a 512 x 512 image and the 128 / 256 mask
  stages, half of the images flipped: the ONE ``mp_bottomup_train_augment`` launch on prepared arguments in device microseconds
  against the same work composed from what existed before it, in the same run - ``mp_warp_affine`` of the batch, ``mp_flip_width``
  of the flipped half (the other half copied), and the masks by torch indexing (fixed-point coordinates, gather, ``where``, mirror,
  pad) from matrices already inverted and uploaded; the two results are compared bit for bit first.  Fraction of 8 TB/s on the
  algorithmic bytes (read: the uint8 sources and masks; written: three fp32 planes and the padded uint8 mask stages).
- train_masks: the training masks of a batch, N = 32 images of 480 x 640 with two polygon regions each, radii [24, 12] (the recipe's
  sigma 2 on two levels): the two launches of ``mp_bottomup_train_masks`` on prepared, uploaded tables in device microseconds
  (alternated rounds, median and min - max), the whole ``bottomup_masks_batch`` call (packing, one upload, the launches) and the
  same batch through ``decode_mask_info`` on the host in wall milliseconds; both results are compared bit for bit first.  Fraction
  of 8 TB/s on the algorithmic bytes (written: the uint8 clearance plane and the S stage planes; read: the clearance plane once).
- flip_tta: the flip test.  The parse launch alone at the recipe shape (N = 1, stages 128 x 128 with 34 channels and 256 x 256 with 17,
  NMS 3, max_num 30): ``mp_bottomup_parse_nms_topk_flip`` beside the plain ``mp_bottomup_parse_nms_topk``, alternated in rounds of
  device-event timings (median and min - max over the rounds) with the algorithmic bytes of each (flip: both runs' stages read,
  ``tagging`` twice as wide, ``heatmap_raw`` once); and the wall milliseconds of one ``infer`` batch (N = 1, 512 x 512, amp O2,
  missing-joint refinement on) with ``MINDPOSE_FLIP_BATCHED`` 1 and 0, alternated the same way;
- match: the grouping at the recipe's K = 17, M = 30, L = 1, for N = 1 and N = 32 images whose detections are drawn around 5, 20 and
  500 person centres (tags a centre's integer plus normal noise of 0.25; values uniform, nine in ten above ``vis_thr``): the host
  ``match_by_tag`` map (with the three ``.cpu()`` copies the inferencer made) against ``match_by_tag_batch`` (one launch, its two
  downloads and the per-image copies), wall milliseconds per batch in alternated rounds (median and min - max), the persons found,
  and the ``mp_bottomup_match_by_tag`` launch alone on prepared buffers in device microseconds.  Both paths are compared bit for
  bit first.
- multi_scale: the multi-scale test at base 512 x 832, N = 1, scale factors (0.5, 1, 2), NMS 3, max_num 30, without and with the flip
  test.  The ONE ``mp_bottomup_parse_nms_topk_multi`` launch on prepared arguments against the same aggregation composed in the same
  run from what existed before it: one single-run parse launch per scale (each run's stage mean at its own map size), torch ops on
  their ``heatmap_raw`` (``F.interpolate`` of the other scales' maps to the base map, the sum, the division) and one more parse
  launch over the averaged map for the NMS and the per-tile top-k; alternated rounds of device-event timings (median, min - max).
  The composition resizes in two steps and with half-pixel centres, so its bits differ: it stands for the work, not the values.
  Fraction of 8 TB/s of the fused launch on its algorithmic bytes (every heat-map plane of every run read once, the base run's tag
  planes once, ``heatmap_raw`` and ``tagging`` written).  ``mp_resize_bilinear_nchw`` of the input to the two other scales in device
  microseconds.  Then one forward per scale 0.5 / 1 / 1.5 / 2 of both recipe sizes in fp32 and amp O2 (``MINDPOSE_AUTOTUNE`` as the
  environment sets it, reported); a scale whose plan cannot be recorded reports the plan's own error instead of a time.
- finish: the tail of a bottom-up batch behind the decoder - ``BottomUpHeatMapAEInferencer._parse`` (grouping, scores, missing-joint
  refinement on) - with ``MINDPOSE_FINISH_DEVICE`` 0 (the grouping launch, then the host-driven tail: four downloads, one upload and
  two Python loops over persons) and 1 (the grouping launch, ``mp_bottomup_finish_people``, two downloads): wall milliseconds per
  batch in alternated rounds in one process (median and min - max) at K = 17, M = 30, L = 1, the 256 x 256 map, N = 1 and N = 32,
  detections drawn around 5, 20 and 500 centres as in ``match``; the persons found and the share of their joints that grouping left
  empty (the refinement's work) are printed, and both settings are compared bit for bit first.  Then the entry's two launches in
  device microseconds (events around each call, the persons restored outside them; launch A alone is the call without refinement)
  and the bytes launch B reads ((1 + L) * H * W * 4 per missing joint), beside ``mp_bottomup_refine_missing`` for the same persons
  (every joint of every person).
- eval_batched: the evaluation chain dataset -> pipeline -> inferencer end to end on a synthetic folder of 96 JPEG files of COCO's
  usual sizes (64 of 640 x 480, 32 of 480 x 640, interleaved) with the synthetic weights, NMS 3, max_num 30, refinement on, no flip
  test, four codec workers and a prefetch of 2: ``create_pipeline(bucket_by_shape=False)`` (one image per batch, what the parent
  commit did) against ``bucket_by_shape=True`` at batch sizes 4, 8 and 16, in fp32 and amp O2.  Wall milliseconds per image over a
  whole epoch, alternated rounds in one process after one pass per setting that records its plans (median and min - max), the
  speed-up over the unbucketed median of the same run, the pipeline alone (every batch waited for, no network) and the persons
  per image.  The synthetic weights find far more persons per image than a trained network would: the share of grouping and
  finish is overstated.  ``MINDPOSE_AUTOTUNE`` is as the environment sets it and is reported.
Forward sizes are the recipe's eval images: 512 x 512 (N = 1 and 32) and 512 x 832 (N = 1).

``--only NAME`` runs one section in this process; without it every section runs in a child process of its own under a time limit
(``--section-timeout`` seconds), and a section that fails or overruns ends the run.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mindpose_amd as mp  # noqa: E402
from mindpose_amd import _lib  # noqa: E402
from mindpose_amd.data.transform._launch import norm255, source_batch  # noqa: E402
from mindpose_amd.data.transform.bottomup_transform import launch_resize_pad_normalize  # noqa: E402
from mindpose_amd.engine.inferencer.bottomup_inferencer import BottomUpHeatMapAEInferencer, refine_missing_joint  # noqa: E402
from mindpose_amd.utils.match import match_by_tag, match_by_tag_batch  # noqa: E402

DEV = torch.device("cuda:0")
HBM = 8e12
JOINT_ORDER = [0, 1, 2, 3, 4, 5, 6, 11, 12, 7, 8, 9, 10, 13, 14, 15, 16]


def _time(fn, steps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps  # ms


def forward(amp, n, h, w, steps):
    net = mp.init_synthetic(mp.create_network("hrnet_w32", "higher_hrnet_head"), seed=0).to(DEV).eval()
    if amp != "O0":
        mp.models.auto_mixed_precision(net, amp)
    image = net.input_buffer((n, 3, h, w), DEV)
    image.copy_(torch.randn(n, 3, h, w))
    ms = _time(lambda: net(image), steps)
    plan = net.get_plan((n, 3, h, w), DEV)
    return dict(amp=amp, n=n, h=h, w=w, ms=round(ms, 4), img_s=round(n * 1000 / ms, 1),
                gflop_per_image=round(2 * plan.total_macs / n / 1e9, 2))


def decoder(n, h, w, steps):
    g = torch.Generator().manual_seed(0)
    outs = [torch.rand(n, 34, h // 2, w // 2, generator=g).to(DEV), torch.rand(n, 17, h, w, generator=g).to(DEV)]
    mask = torch.ones(n, 2 * h, 2 * w, dtype=torch.bool, device=DEV)
    dec = mp.create_decoder("bottomup_heatmap_ae", use_nms=True, nms_kernel=3, max_num=30)
    ms = _time(lambda: dec(outs, mask), steps)
    nbytes = n * 4 * (17 * h * w + 34 * (h // 2) * (w // 2) + 2 * 17 * h * w)
    val, tag, ind, _, _ = dec(outs, mask)
    t0 = time.perf_counter()
    for i in range(n):
        match_by_tag(val[i].cpu().numpy(), tag[i].cpu().numpy(), ind[i].cpu().numpy(), JOINT_ORDER)
    match_ms = (time.perf_counter() - t0) * 1000 / n
    return dict(n=n, h=h, w=w, us_per_image=round(ms * 1000 / n, 2), hbm_fraction=round(nbytes / (ms * 1e-3) / HBM, 3),
                mb_per_image=round(nbytes / n / 1e6, 2), match_ms_per_image=round(match_ms, 3))


def resize_pad_normalize(steps):
    src_w, src_h, tw, th, pw, ph = 640, 480, 683, 512, 832, 512
    image = torch.randint(0, 256, (src_h, src_w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).to(DEV)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.255)
    ms = _time(lambda: launch_resize_pad_normalize([image], [(tw, th)], (pw, ph), mean, std), steps)  # (with the wrapper's two small uploads)
    # the kernel alone: the C entry on prepared arguments
    import ctypes
    lib = _lib.load()
    _, offs, hw, _ = source_batch([image])
    out, mask = torch.empty(1, 3, ph, pw, device=DEV), torch.empty(1, ph, pw, dtype=torch.uint8, device=DEV)
    twh = (ctypes.c_int * 2)(tw, th)
    m3, s3 = norm255(mean, std)
    kernel_ms = _time(lambda: lib.mp_resize_pad_normalize(_lib.ptr(image), _lib.ptr(offs), _lib.ptr(hw), twh, _lib.ptr(out), _lib.ptr(mask), 1,
                                                          ph, pw, m3, s3, _lib.stream()), steps)
    nbytes = src_h * src_w * 3 + ph * pw * (3 * 4 + 1)
    return dict(src=[src_w, src_h], target=[tw, th], padded=[pw, ph], kernel_us=round(kernel_ms * 1000, 2), call_us=round(ms * 1000, 2),
                mb=round(nbytes / 1e6, 2), hbm_fraction=round(nbytes / (kernel_ms * 1e-3) / HBM, 4))


def refine(persons, steps, h=256, w=416, k=17, num_tags=1):
    g = torch.Generator().manual_seed(persons)
    heat = torch.rand(1, k, h, w, generator=g).to(DEV)
    tagging = torch.rand(1, k, h, w, num_tags, generator=g).to(DEV)
    people = np.zeros((persons, k, 3 + num_tags), np.float32)  # every person: ten located joints, seven to refine
    rng = np.random.RandomState(persons)
    for p in range(persons):
        joints = rng.permutation(k)[:10]
        people[p, joints, 0], people[p, joints, 1], people[p, joints, 2] = rng.randint(0, w, 10), rng.randint(0, h, 10), 0.5

    def device():
        BottomUpHeatMapAEInferencer._refine_on_device([people.copy()], heat, tagging)

    def host():  # what the inferencer ran before: both maps to the host, then numpy per person
        hm, tg = heat.cpu().numpy(), tagging.cpu().numpy()
        for person in people.copy():
            refine_missing_joint(hm[0], tg[0], person)

    def wall(fn, reps):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1000 / reps

    lib = _lib.load()
    mean = torch.rand(persons, num_tags, generator=g).to(DEV)
    img = torch.zeros(persons, dtype=torch.int32, device=DEV)
    found = torch.empty(persons, k, 3, device=DEV)
    kernel_ms = _time(lambda: lib.mp_bottomup_refine_missing(_lib.ptr(heat), _lib.ptr(tagging), _lib.ptr(mean), _lib.ptr(img), persons, 1, k, h,
                                                             w, 1, num_tags, _lib.ptr(found), _lib.stream()), steps)
    nbytes = persons * k * h * w * 4 * (1 + num_tags)
    return dict(persons=persons, h=h, w=w, device_ms=round(wall(device, steps), 3), host_ms=round(wall(host, max(2, steps // 5)), 3),
                kernel_us=round(kernel_ms * 1000, 2), hbm_fraction=round(nbytes / (kernel_ms * 1e-3) / HBM, 4))


def train_augment(steps, n=32, src_w=640, src_h=480):
    import ctypes
    from mindpose_amd.data.transform.bottomup_transform import _invert_affine
    cfg = dict(image_size=[512, 512], max_image_size=[512, 512], heatmap_sizes=[[128, 128], [256, 256]], flip_pairs=[[1, 2]], pixel_std=200.0,
               tag_per_joint=True)
    affine = mp.BottomUpRandomAffine(config=cfg)
    g = torch.Generator().manual_seed(0)
    images = torch.randint(0, 256, (n, src_h, src_w, 3), dtype=torch.uint8, generator=g).to(DEV)
    masks = (torch.rand(n, src_h, src_w, generator=g) > 0.2).to(torch.uint8).to(DEV)
    np.random.seed(0)
    mats = np.stack([affine.matrices(affine.draw(src_w, src_h)) for _ in range(n)])  # [n, 3, 2, 3]: stages, then the image
    flags = [1] * (n // 2) + [0] * (n - n // 2)
    sizes, (out_w, out_h) = cfg["heatmap_sizes"], cfg["image_size"]
    s, wmax, hmax = len(sizes), 256, 256
    lib = _lib.load()
    _, offs, hw, _ = source_batch(list(images))
    _, moffs, _, _ = source_batch(list(masks), pixel=())
    trans = torch.from_numpy(np.ascontiguousarray(mats.reshape(n, s + 1, 6))).to(DEV)
    fl = torch.tensor(flags, dtype=torch.int32, device=DEV)
    out = torch.empty(n, 3, out_h, out_w, device=DEV)
    mask_out = torch.empty(n, s, hmax, wmax, dtype=torch.uint8, device=DEV)
    wh = (ctypes.c_int * (2 * s))(*[v for size in sizes for v in size])
    m3, s3 = norm255((0.485, 0.456, 0.406), (0.229, 0.224, 0.255))

    def fused():
        _lib.check(lib.mp_bottomup_train_augment(_lib.ptr(images), _lib.ptr(offs), _lib.ptr(hw), _lib.ptr(masks), _lib.ptr(moffs), _lib.ptr(trans),
                                                 _lib.ptr(fl), wh, _lib.ptr(out), _lib.ptr(mask_out), n, s, out_h, out_w, hmax, wmax, m3, s3,
                                                 _lib.stream()), "mp_bottomup_train_augment")

    # the composition: its constant operands are prepared outside the timed region
    trans_image = trans[:, s].contiguous()
    warped, composed = torch.empty_like(out), torch.empty_like(out)
    composed_mask = torch.zeros_like(mask_out)
    flagged = fl.bool()[:, None, None]
    stage_terms = []
    for j, (w, h) in enumerate(sizes):
        inv = torch.tensor([_invert_affine(mats[i, j]) for i in range(n)], dtype=torch.float64, device=DEV)  # [n, 6]: i00 i01 i02 i10 i11 i12
        stage_terms.append((inv, torch.arange(w, dtype=torch.float64, device=DEV), torch.arange(h, dtype=torch.float64, device=DEV)))
    flat_masks = masks.reshape(n, -1)

    def compose_image():
        _lib.check(lib.mp_warp_affine(_lib.ptr(images), _lib.ptr(offs), _lib.ptr(hw), None, _lib.ptr(trans_image), _lib.ptr(warped), n, out_h,
                                      out_w, 1, m3, s3, _lib.stream()), "mp_warp_affine")
        _lib.check(lib.mp_flip_width(_lib.ptr(warped), _lib.ptr(composed), n // 2, 3, out_h, out_w, _lib.stream()), "mp_flip_width")
        composed[n // 2:].copy_(warped[n // 2:])

    def compose_masks():
        for j, (inv, xs, ys) in enumerate(stage_terms):
            w, h = sizes[j]
            sx = ((torch.round((inv[:, 1, None] * ys + inv[:, 2, None]) * 1024.0).long() + 512)[:, :, None]
                  + torch.round(inv[:, 0, None] * xs * 1024.0).long()[:, None, :]) >> 10
            sy = ((torch.round((inv[:, 4, None] * ys + inv[:, 5, None]) * 1024.0).long() + 512)[:, :, None]
                  + torch.round(inv[:, 3, None] * xs * 1024.0).long()[:, None, :]) >> 10
            inside = (sx >= 0) & (sx < src_w) & (sy >= 0) & (sy < src_h)
            flat = (sy.clamp(0, src_h - 1) * src_w + sx.clamp(0, src_w - 1)).reshape(n, -1)
            plane = torch.where(inside, torch.gather(flat_masks, 1, flat).reshape(n, h, w), 0)
            composed_mask[:, j, :h, :w] = torch.where(flagged, plane.flip(2), plane)

    fused()
    compose_image()
    compose_masks()
    torch.cuda.synchronize()
    if not torch.equal(out.view(torch.int32), composed.view(torch.int32)) or not torch.equal(mask_out, composed_mask):
        raise RuntimeError("the fused launch and the composition disagree")
    fused_ms = _time(fused, steps)
    image_ms, masks_ms = _time(compose_image, steps), _time(compose_masks, steps)
    nbytes = n * (src_h * src_w * 4 + out_h * out_w * 12 + s * hmax * wmax)
    return dict(n=n, src=[src_w, src_h], image=[out_w, out_h], stages=sizes, flipped=n // 2, fused_us=round(fused_ms * 1000, 2),
                composed_us=round((image_ms + masks_ms) * 1000, 2), composed_image_us=round(image_ms * 1000, 2),
                composed_masks_us=round(masks_ms * 1000, 2), ratio=round((image_ms + masks_ms) / fused_ms, 2), mb=round(nbytes / 1e6, 2),
                hbm_fraction=round(nbytes / (fused_ms * 1e-3) / HBM, 4))


def train_masks(steps, rounds=5, n=32, h=480, w=640, radii=(24, 12)):
    from mindpose_amd.data.transform import bottomup_mask as bm
    rng = np.random.RandomState(0)
    infos = []
    for _ in range(n):
        x0, y0, x1, y1 = rng.randint(0, w // 2), rng.randint(0, h // 2), rng.randint(w // 2, w), rng.randint(h // 2, h)
        box = [x0, y0, x0 + (x1 - x0) // 3, y0, x0 + (x1 - x0) // 3, y0 + (y1 - y0) // 3, x0, y0 + (y1 - y0) // 3]
        blob = [float(v) for v in np.stack([rng.uniform(x0, x1, 3), rng.uniform(y0, y1, 3)], axis=1).reshape(-1)]
        infos.append(dict(regions=[bm.rle_from_polygon(box, h, w), bm.rle_from_polygon(blob, h, w)], shape=(len(radii), h, w), radii=list(radii)))
    t0 = time.perf_counter()
    want = [bm.decode_mask_info(info) for info in infos]
    host_ms = (time.perf_counter() - t0) * 1000
    got = mp.bottomup_masks_batch(infos, DEV)
    if any(not np.array_equal(g.cpu().numpy(), w_) for g, w_ in zip(got, want)):
        raise RuntimeError("the device masks and the host decode disagree")
    s, size = len(radii), len(radii) * h * w
    tabs = bm.pack_mask_tables(infos, [i * size for i in range(n)])
    tables = torch.from_numpy(tabs["blob"]).to(DEV)
    out = torch.empty(n * size, dtype=torch.uint8, device=DEV)
    ws = torch.empty(tabs["clear_bytes"], dtype=torch.uint8, device=DEV)
    base, starts = tables.data_ptr(), tabs["starts"]
    as_p = lambda a, c: a.ctypes.data_as(ctypes.POINTER(c))  # noqa: E731
    args = (as_p(tabs["prefix"], ctypes.c_uint32), as_p(tabs["region_ptr"], ctypes.c_int), as_p(tabs["image_tab"], ctypes.c_int),
            as_p(tabs["offsets"], ctypes.c_longlong), base + starts[3], base + starts[2], base + starts[1], base + starts[0],
            (ctypes.c_int * s)(*radii), as_p(tabs["half"], ctypes.c_uint8), out.data_ptr(), out.numel(), ws.data_ptr(), ws.numel(), n, s)
    lib = _lib.load()

    def launches():
        _lib.check(lib.mp_bottomup_train_masks(*args, _lib.stream()), "mp_bottomup_train_masks")

    def call():
        mp.bottomup_masks_batch(infos, DEV)

    def wall(fn, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1000 / reps

    launches()
    torch.cuda.synchronize()
    if any(not np.array_equal(out[i * size:(i + 1) * size].view(s, h, w).cpu().numpy(), want[i]) for i in range(n)):
        raise RuntimeError("the prepared launch and the host decode disagree")
    times, calls = [], []
    for _ in range(rounds):
        times.append(_time(launches, steps) * 1000)
        calls.append(wall(call, max(2, steps // 4)))
    nbytes = n * h * w * (s + 2)
    us = _spread(times)
    return dict(n=n, image=[w, h], regions=2, runs=[int(min(len(r) for i in infos for r in i["regions"])), int(max(len(r) for i in infos for r in i["regions"]))],
                radii=list(radii), launches_us=us, call_ms=_spread(calls), host_decode_ms=round(host_ms, 1),
                ratio_host_over_call=round(host_ms / _spread(calls)["median"], 1), mb=round(nbytes / 1e6, 2),
                hbm_fraction=round(nbytes / (us["median"] * 1e-6) / HBM, 4), valid_fraction=[round(float(np.mean([m[i].mean() for m in want])), 3) for i in range(s)])


def _spread(values):
    v = sorted(values)
    return dict(median=round(v[len(v) // 2], 3), min=round(v[0], 3), max=round(v[-1], 3))


def flip_tta(steps, rounds=7):
    lib = _lib.load()
    n, k, h, w, m = 1, 17, 256, 256, 30
    g = torch.Generator().manual_seed(0)
    runs = [[torch.rand(n, 2 * k, h // 2, w // 2, generator=g).to(DEV), torch.rand(n, k, h, w, generator=g).to(DEV)] for _ in range(2)]
    mask = torch.ones(n, 2 * h, 2 * w, dtype=torch.uint8, device=DEV)
    raw = torch.empty(n, k, h, w, device=DEV)
    tagging = torch.empty(n, k, h, w, 2, device=DEV)
    ws_bytes = lib.mp_bottomup_workspace_bytes(n, k, h, w, m)
    ws = torch.empty(ws_bytes // 8, device=DEV, dtype=torch.int64)
    descs = [(_lib.BottomUpStage * 2)(*[_lib.BottomUpStage(data=t.data_ptr(), c=t.shape[1], h=t.shape[2], w=t.shape[3], has_tags=int(i == 0))
                                        for i, t in enumerate(run)]) for run in runs]
    index = (ctypes.c_int32 * k)(0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15)
    tail = (2, _lib.ptr(mask), 2 * h, 2 * w, n, k, 1, 3, m, _lib.ptr(raw), _lib.ptr(tagging), _lib.ptr(ws), ws_bytes)

    def plain():
        _lib.check(lib.mp_bottomup_parse_nms_topk(descs[0], *tail, _lib.stream()), "mp_bottomup_parse_nms_topk")

    def flip():
        _lib.check(lib.mp_bottomup_parse_nms_topk_flip(descs[0], descs[1], index, *tail, _lib.stream()), "mp_bottomup_parse_nms_topk_flip")

    times = dict(plain=[], flip=[])
    for _ in range(rounds):  # alternated: a drift of the machine meets both alike
        times["plain"].append(_time(plain, steps) * 1000)
        times["flip"].append(_time(flip, steps) * 1000)
    stage_bytes = 4 * n * (2 * k * (h // 2) * (w // 2) + k * h * w)
    nbytes = dict(plain=stage_bytes + 4 * n * k * h * w * 2, flip=2 * stage_bytes + 4 * n * k * h * w * 3)
    res = dict(parse_launch_us={name: dict(_spread(t), mb=round(nbytes[name] / 1e6, 2)) for name, t in times.items()})
    res["parse_launch_ratio"] = round(res["parse_launch_us"]["flip"]["median"] / res["parse_launch_us"]["plain"]["median"], 3)

    net = mp.init_synthetic(mp.create_network("hrnet_w32", "higher_hrnet_head"), seed=0).to(DEV).eval()
    mp.models.auto_mixed_precision(net, "O2")
    dec = mp.create_decoder("bottomup_heatmap_ae", use_nms=True, nms_kernel=3, max_num=m)
    cfg = dict(has_heatmap_output=True, hflip_tta=True, joint_order=JOINT_ORDER, vis_thr=0.1, ignore_too_much=False, use_rounded_norm=True,
               tag_thr=1.0, pixel_std=200.0, downsample_scale=2, refine_missing_joint=True,
               flip_pairs=[[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]])
    inf = BottomUpHeatMapAEInferencer(mp.create_eval_network(net, dec), config=cfg, decoder=dec)
    batch = dict(image=torch.randn(1, 3, 512, 512, generator=g).to(DEV), mask=torch.ones(1, 512, 512, dtype=torch.bool, device=DEV),
                 center=np.array([[256.0, 256.0]], np.float32), scale=np.array([[2.56, 2.56]], np.float32),
                 image_shape=np.array([[512, 512]], np.float32))

    def wall(batched):
        os.environ["MINDPOSE_FLIP_BATCHED"] = batched
        inf.infer([batch])  # (the first call of a setting records its plan)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            records = inf.infer([batch])  # ends in the downloads of the decoded arrays: synchronised
        return (time.perf_counter() - t0) * 1000 / steps, len(records[0]["pred"])

    infer = {"1": [], "0": []}
    for _ in range(rounds):
        for batched in ("1", "0"):
            ms, persons = wall(batched)
            infer[batched].append(ms)
    res["infer_batch_ms"] = dict(batched=_spread(infer["1"]), two_forwards=_spread(infer["0"]), persons=persons)
    return res


def match(steps, rounds=5, k=17, m=30, num_tags=1):
    lib = _lib.load()
    out = []
    for n in (1, 32):
        for centres in (5, 20, 500):
            rng = np.random.RandomState(centres + n)
            tag = (rng.randint(0, centres, (n, k, m, 1)) + 0.25 * rng.randn(n, k, m, num_tags)).astype(np.float32)
            val, tag, ind = (torch.from_numpy(a).to(DEV) for a in (rng.rand(n, k, m).astype(np.float32), tag,
                                                                   rng.randint(0, 256, (n, k, m, 2)).astype(np.float32)))

            def host():
                return [match_by_tag(v, t, i, JOINT_ORDER) for v, t, i in zip(val.cpu().numpy(), tag.cpu().numpy(), ind.cpu().numpy())]

            def device():
                return match_by_tag_batch(val, tag, ind, JOINT_ORDER)

            want, got = host(), device()
            if any(g.shape != w.shape or not np.array_equal(g.view(np.uint32), w.view(np.uint32)) for g, w in zip(got, want)):
                raise RuntimeError("the device grouping and the host function disagree")

            def wall(fn, reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn()  # both end in downloads: synchronised
                return (time.perf_counter() - t0) * 1000 / reps

            times = dict(host=[], device=[])
            for _ in range(rounds):  # alternated: a drift of the machine meets both alike
                times["host"].append(wall(host, max(1, steps // (4 if n == 1 else 20))))
                times["device"].append(wall(device, steps))
            people = torch.empty(n, k * m, k, 3 + num_tags, device=DEV)
            meta = torch.empty(2, n, dtype=torch.int32, device=DEV)
            ws_bytes = lib.mp_bottomup_match_workspace_bytes(n, k, m, num_tags)
            ws = torch.empty(ws_bytes // 4, device=DEV)
            order = (ctypes.c_int * k)(*JOINT_ORDER)
            kernel_ms = _time(lambda: lib.mp_bottomup_match_by_tag(_lib.ptr(val), _lib.ptr(tag), _lib.ptr(ind), n, k, m, num_tags, order, 0.1, 1.0,
                                                                   0, 1, _lib.ptr(people), _lib.ptr(meta[0]), _lib.ptr(meta[1]), _lib.ptr(ws),
                                                                   ws_bytes, _lib.stream()), steps)
            host_ms, device_ms = _spread(times["host"]), _spread(times["device"])
            out.append(dict(n=n, centres=centres, persons=[int(min(len(w) for w in want)), int(max(len(w) for w in want))],
                            host_ms=host_ms, device_ms=device_ms, ratio=round(host_ms["median"] / device_ms["median"], 2),
                            kernel_us=round(kernel_ms * 1000, 2)))
    return out


def _time_each(prepare, fn, steps, warmup=2):
    """device milliseconds per call of ``fn``, ``prepare`` run before each call outside the timed events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    total = 0.0
    for i in range(warmup + steps):
        prepare()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            total += e0.elapsed_time(e1)
    return total / steps


def finish(steps, rounds=5, k=17, m=30, num_tags=1, h=256, w=256):
    from mindpose_amd.utils.match import match_by_tag_device
    lib = _lib.load()
    cfg = dict(has_heatmap_output=True, hflip_tta=False, joint_order=JOINT_ORDER, vis_thr=0.1, ignore_too_much=False, use_rounded_norm=True,
               tag_thr=1.0, pixel_std=200.0, downsample_scale=2, refine_missing_joint=True,
               flip_pairs=[[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]])
    inf = BottomUpHeatMapAEInferencer(None, config=cfg)
    out = []
    for n in (1, 32):
        g = torch.Generator().manual_seed(n)
        heat = torch.rand(n, k, h, w, generator=g).to(DEV)
        tagging = (torch.rand(n, k, h, w, num_tags, generator=g) * 8.0).to(DEV)
        for centres in (5, 20, 500):
            rng = np.random.RandomState(centres + n)
            tag = (rng.randint(0, centres, (n, k, m, 1)) + 0.25 * rng.randn(n, k, m, num_tags)).astype(np.float32)
            val, tag, ind = (torch.from_numpy(a).to(DEV) for a in (rng.rand(n, k, m).astype(np.float32), tag,
                                                                   rng.randint(0, 256, (n, k, m, 2)).astype(np.float32)))

            def parse(switch):
                os.environ["MINDPOSE_FINISH_DEVICE"] = switch
                return inf._parse(val, tag, ind, heat, tagging)

            (kp0, sc0), (kp1, sc1) = parse("0"), parse("1")
            if any(a.shape != b.shape or not np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(kp0, kp1)) or sc0 != sc1:
                raise RuntimeError("the device tail and the host-driven tail disagree")

            def wall(switch, reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    parse(switch)  # both end in downloads: synchronised
                return (time.perf_counter() - t0) * 1000 / reps

            reps = max(1, steps // (1 if n == 1 else 10))
            times = {"0": [], "1": []}
            for _ in range(rounds):  # alternated: a drift of the machine meets both alike
                for switch in ("0", "1"):
                    times[switch].append(wall(switch, reps))

            # the launches alone, on the grouping's own buffers; the grouped persons are kept aside and restored before every call
            people, counts, status = match_by_tag_device(val, tag, ind, JOINT_ORDER)
            pristine = people.clone()
            scores = torch.empty(n, k * m, device=DEV)
            ws_bytes = lib.mp_bottomup_finish_workspace_bytes(n, k, m, num_tags)
            ws = torch.empty(ws_bytes // 4, device=DEV)

            def entry(refine):
                return lambda: _lib.check(lib.mp_bottomup_finish_people(
                    _lib.ptr(people), _lib.ptr(counts), _lib.ptr(status), _lib.ptr(heat), _lib.ptr(tagging), n, k, m, h, w, 1, num_tags, refine,
                    _lib.ptr(scores), _lib.ptr(ws), ws_bytes, _lib.stream()), "mp_bottomup_finish_people")

            restore = lambda: people.copy_(pristine)  # noqa: E731
            a_us = _time_each(restore, entry(0), steps) * 1000
            ab_us = _time_each(restore, entry(1), steps) * 1000
            # mp_bottomup_refine_missing for the same persons with the mean tags launch A left in the workspace
            count_host = counts.cpu().numpy()
            persons = int(count_host.sum())
            img = torch.from_numpy(np.repeat(np.arange(n), count_host).astype(np.int32)).to(DEV)
            mean = torch.cat([ws[:n * k * m * num_tags].view(n, k * m, num_tags)[i, :count_host[i]] for i in range(n)]).contiguous()
            found = torch.empty(persons, k, 3, device=DEV)
            old_us = _time(lambda: lib.mp_bottomup_refine_missing(_lib.ptr(heat), _lib.ptr(tagging), _lib.ptr(mean), _lib.ptr(img), persons, n, k, h,
                                                                  w, 1, num_tags, _lib.ptr(found), _lib.stream()), steps) * 1000
            grouped = [p for p in match_by_tag_batch(val, tag, ind, JOINT_ORDER)]
            missing = int(sum((p[:, :, 2] == 0).sum() for p in grouped if p.size))
            plane_bytes = (1 + num_tags) * h * w * 4
            off_ms, on_ms = _spread(times["0"]), _spread(times["1"])
            out.append(dict(n=n, centres=centres, persons=[int(count_host.min()), int(count_host.max())],
                            missing_share=round(missing / max(1, persons * k), 3), switch0_ms=off_ms, switch1_ms=on_ms,
                            ratio=round(off_ms["median"] / on_ms["median"], 2), launch_a_us=round(a_us, 2),
                            launch_b_us=round(ab_us - a_us, 2), launch_b_mb=round(missing * plane_bytes / 1e6, 1),
                            refine_missing_us=round(old_us, 2), refine_missing_mb=round(persons * k * plane_bytes / 1e6, 1)))
    os.environ.pop("MINDPOSE_FINISH_DEVICE", None)
    return out


def multi_scale(steps, rounds=5):
    import torch.nn.functional as F
    from mindpose_amd.models.decoders import resize_bilinear
    lib = _lib.load()
    n, k, m, bh, bw, scales, base = 1, 17, 30, 512, 832, (0.5, 1.0, 2.0), 1
    h, w = bh // 2, bw // 2
    g = torch.Generator().manual_seed(0)

    def run_outputs(s):
        hs, ws_ = int(bh * s), int(bw * s)
        return [torch.rand(n, 2 * k, hs // 4, ws_ // 4, generator=g).to(DEV), torch.rand(n, k, hs // 2, ws_ // 2, generator=g).to(DEV)]

    def describe(run):
        return (_lib.BottomUpStage * 2)(*[_lib.BottomUpStage(data=t.data_ptr(), c=t.shape[1], h=t.shape[2], w=t.shape[3], has_tags=int(i == 0))
                                          for i, t in enumerate(run)])

    plain, mirrored = [run_outputs(s) for s in scales], [run_outputs(s) for s in scales]
    pd, md = [describe(r) for r in plain], [describe(r) for r in mirrored]
    index = (ctypes.c_int32 * k)(0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15)
    mask = torch.ones(n, bh, bw, dtype=torch.uint8, device=DEV)
    raw, tagging = torch.empty(n, k, h, w, device=DEV), torch.empty(n, k, h, w, 2, device=DEV)
    ws_bytes = lib.mp_bottomup_workspace_bytes(n, k, h, w, m)
    ws = torch.empty(ws_bytes // 8, device=DEV, dtype=torch.int64)
    # the composition's buffers: every run's own map, its own workspace and tags; the averaged map beside unused tag channels
    own = []
    for r, s in enumerate(scales):
        hs, ws_ = plain[r][1].shape[2:]
        nb = lib.mp_bottomup_workspace_bytes(n, k, hs, ws_, m)
        own.append(dict(raw=torch.empty(n, k, hs, ws_, device=DEV), tagging=torch.empty(n, k, hs, ws_, 2, device=DEV),
                        ws=torch.empty(nb // 8, device=DEV, dtype=torch.int64), ws_bytes=nb, h=hs, w=ws_))
    averaged = torch.zeros(n, 2 * k, h, w, device=DEV)
    averaged_desc = describe([averaged])

    def tail(raw_t, tagging_t, ws_t, nbytes, stages=2):
        return (stages, _lib.ptr(mask), bh, bw, n, k, 1, 3, m, _lib.ptr(raw_t), _lib.ptr(tagging_t), _lib.ptr(ws_t), nbytes, _lib.stream())

    def fused(flip):
        table = (_lib.BottomUpRun * len(scales))(*[_lib.BottomUpRun(stages=a, flipped=b if flip else None) for a, b in zip(pd, md)])
        args = (table, len(scales), base, index if flip else None) + tail(raw, tagging, ws, ws_bytes)
        return lambda: _lib.check(lib.mp_bottomup_parse_nms_topk_multi(*args), "mp_bottomup_parse_nms_topk_multi")

    def composed(flip):
        def fn():
            for r, o in enumerate(own):
                t = tail(o["raw"], o["tagging"], o["ws"], o["ws_bytes"])
                if flip:
                    _lib.check(lib.mp_bottomup_parse_nms_topk_flip(pd[r], md[r], index, *t), "mp_bottomup_parse_nms_topk_flip")
                else:
                    _lib.check(lib.mp_bottomup_parse_nms_topk(pd[r], *t), "mp_bottomup_parse_nms_topk")
            total = own[0]["raw"] if base == 0 else F.interpolate(own[0]["raw"], size=(h, w), mode="bilinear", align_corners=False)
            for r in range(1, len(own)):
                total = total + (own[r]["raw"] if r == base else F.interpolate(own[r]["raw"], size=(h, w), mode="bilinear", align_corners=False))
            averaged[:, :k] = total / len(own)
            _lib.check(lib.mp_bottomup_parse_nms_topk(averaged_desc, *tail(raw, own[base]["tagging"], ws, ws_bytes, stages=1)),
                       "mp_bottomup_parse_nms_topk")
        return fn

    res = dict(base=[bh, bw], scales=list(scales), map=[h, w], autotune=os.environ.get("MINDPOSE_AUTOTUNE", "1"), parse_launch_us={})
    heat = 4 * n * k * sum(t.shape[2] * t.shape[3] for r in plain for t in r)
    tags = 4 * n * k * plain[base][0].shape[2] * plain[base][0].shape[3]
    for flip in (False, True):
        f, c = fused(flip), composed(flip)
        times = dict(fused=[], composed=[])
        for _ in range(rounds):  # alternated: a drift of the machine meets both alike
            times["fused"].append(_time(f, steps) * 1000)
            times["composed"].append(_time(c, steps) * 1000)
        nbytes = (2 if flip else 1) * (heat + tags) + 4 * n * k * h * w * (3 if flip else 2)
        fu, co = _spread(times["fused"]), _spread(times["composed"])
        res["parse_launch_us"]["flip" if flip else "plain"] = dict(
            fused=fu, composed=co, ratio=round(co["median"] / fu["median"], 2), mb=round(nbytes / 1e6, 2),
            hbm_fraction=round(nbytes / (fu["median"] * 1e-6) / HBM, 4))

    image = torch.randn(n, 3, bh, bw, generator=g).to(DEV)
    res["resize_input_us"] = {}
    for s in scales:
        if s != 1.0:
            out = torch.empty(n, 3, int(bh * s), int(bw * s), device=DEV)
            res["resize_input_us"][str(s)] = round(_time(lambda: resize_bilinear(image, out.shape[2:], out=out), steps) * 1000, 2)

    res["forward"] = []
    for fh, fw in ((512, 512), (512, 832)):
        for amp in ("O0", "O2"):
            for s in (0.5, 1.0, 1.5, 2.0):
                try:
                    res["forward"].append(dict(forward(amp, n, int(fh * s), int(fw * s), max(3, steps // 4)), base=[fh, fw], scale=s))
                except Exception as e:  # the plan's own error is the answer for this scale; a failed launch or HIP call ends the run
                    if "hipError" in str(e) or "HIP error" in str(e):
                        raise
                    res["forward"].append(dict(amp=amp, n=n, h=int(fh * s), w=int(fw * s), base=[fh, fw], scale=s,
                                               error=f"{type(e).__name__}: {str(e)[:200]}"))
                torch.cuda.empty_cache()
    return res


def eval_batched(steps, rounds=5, landscape=64, portrait=32):
    """(``steps`` is not used: a pass is one epoch over the folder.)"""
    import shutil
    import tempfile
    from PIL import Image
    root = tempfile.mkdtemp(prefix="mindpose_eval_batched_")
    try:
        # COCO's usual sizes, both orientations interleaved 2 : 1; smooth content with mild noise, so that the JPEG codec has real work
        rng = np.random.RandomState(0)
        kinds = (["land", "land", "port"] * max(landscape, portrait))
        left = dict(land=landscape, port=portrait)
        count = 0
        for kind in kinds:
            if left[kind] == 0:
                continue
            left[kind] -= 1
            w, h = (640, 480) if kind == "land" else (480, 640)
            yy, xx = np.mgrid[0:h, 0:w]
            base = np.stack([(xx * 255 // w), (yy * 255 // h), ((xx + yy) * 255 // (w + h))], axis=2).astype(np.float32)
            pixels = np.clip(base + rng.normal(0, 6, (h, w, 3)), 0, 255).astype(np.uint8)
            Image.fromarray(pixels).save(os.path.join(root, f"{count:04d}_{kind}.jpg"), quality=90)
            count += 1
        cfg = dict(image_size=[512, 512], max_image_size=[832, 512], heatmap_sizes=[[128, 128], [256, 256]], pixel_std=200.0, tag_per_joint=True,
                   flip_pairs=[[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]])
        infer_cfg = dict(has_heatmap_output=True, hflip_tta=False, joint_order=JOINT_ORDER, vis_thr=0.1, ignore_too_much=False,
                         use_rounded_norm=True, tag_thr=1.0, pixel_std=200.0, downsample_scale=2, refine_missing_joint=True,
                         flip_pairs=cfg["flip_pairs"])
        ds = mp.create_dataset(root, None, dataset_format="imagefolder_bottomup", is_train=False)
        settings = [("unbucketed", dict(batch_size=1))] + [(f"bucketed_{n}", dict(batch_size=n, bucket_by_shape=True)) for n in (4, 8, 16)]
        res = dict(images=count, landscape=landscape, portrait=portrait, rounds=rounds, num_workers=4, prefetch=2,
                   autotune=os.environ.get("MINDPOSE_AUTOTUNE", "unset"), rows=[])
        for amp in ("O0", "O2"):
            net = mp.init_synthetic(mp.create_network("hrnet_w32", "higher_hrnet_head"), seed=0).to(DEV).eval()
            if amp != "O0":
                mp.models.auto_mixed_precision(net, amp)
            dec = mp.create_decoder("bottomup_heatmap_ae", use_nms=True, nms_kernel=3, max_num=30)
            inf = mp.create_inferencer(mp.create_eval_network(net, dec), "bottomup_heatmap_ae", config=infer_cfg, decoder=dec)
            pipes = {name: mp.create_pipeline(ds, ["bottomup_rescale", "bottomup_pad"], method="imagefolder_bottomup", is_train=False, config=cfg,
                                              num_workers=4, prefetch=2, **kw) for name, kw in settings}

            def chain(pipe):  # dataset -> pipeline -> inferencer: ends in the downloads of the last batch, synchronised
                t0 = time.perf_counter()
                records = inf(pipe)
                return (time.perf_counter() - t0) * 1000 / count, records

            def loader(pipe):  # the pipeline alone, every batch waited for
                t0 = time.perf_counter()
                for batch in pipe:
                    pass
                torch.cuda.synchronize()
                return (time.perf_counter() - t0) * 1000 / count

            try:
                persons = {}
                for name, pipe in pipes.items():  # the first pass records the plans of this setting's batch sizes
                    _, records = chain(pipe)
                    assert len(records) == count
                    persons[name] = round(sum(len(r["pred"]) for r in records) / count, 1)
                times = {name: [] for name in pipes}
                loads = {name: [] for name in pipes}
                for _ in range(rounds):  # alternated: a drift of the machine meets every setting alike
                    for name, pipe in pipes.items():
                        times[name].append(chain(pipe)[0])
                        loads[name].append(loader(pipe))
            finally:
                for pipe in pipes.values():
                    pipe.close()
            base = _spread(times["unbucketed"])["median"]
            for name in pipes:
                t = _spread(times[name])
                res["rows"].append(dict(amp=amp, setting=name, batches=len(pipes[name]), ms_per_image=t, pipeline_alone_ms_per_image=_spread(loads[name]),
                                        speedup_over_unbucketed=round(base / t["median"], 2), persons_per_image=persons[name]))
            del inf, net
            torch.cuda.empty_cache()
        return res
    finally:
        shutil.rmtree(root, ignore_errors=True)


SECTIONS = {
    "forward": lambda steps: [forward(a, n, h, w, steps) for a in ("O0", "O2") for n, h, w in ((1, 512, 512), (32, 512, 512), (1, 512, 832))],
    "decoder": lambda steps: [decoder(1, 256, 416, steps), decoder(32, 256, 256, steps)],
    "resize_pad_normalize": resize_pad_normalize,
    "refine": lambda steps: [refine(p, steps) for p in (1, 10, 30)],
    "train_augment": train_augment,
    "train_masks": train_masks,
    "flip_tta": flip_tta,
    "match": match,
    "finish": finish,
    "multi_scale": multi_scale,
    "eval_batched": eval_batched,
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--only", choices=sorted(SECTIONS), help="run this section in this process and print its JSON")
    ap.add_argument("--sections", default=",".join(SECTIONS), help="comma-separated sections to run (each in a child process)")
    ap.add_argument("--section-timeout", type=int, default=600, help="seconds per section")
    args = ap.parse_args()
    if args.only:
        print(json.dumps(SECTIONS[args.only](args.steps)))
        return
    res = dict(workload="higher_hrnet_w32_bottomup")
    for name in args.sections.split(","):
        # a fresh child per section, each under its own time limit; a section that fails or overruns ends the run
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--only", name, "--steps", str(args.steps)], stdout=subprocess.PIPE,
                             timeout=args.section_timeout, check=True)
        res[name] = json.loads(out.stdout.decode().strip().splitlines()[-1])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
