"""Batched bottom-up evaluation on the MI355X: ``create_pipeline(bucket_by_shape=True)`` batches images that share one network input
size.  The bucketed batches against the grouping's prediction and, row by row, against the unbucketed N = 1 pipeline (bit-equal);
the inferencer over them against hand-stacked batches of the N = 1 tensors (bit-equal records keyed by ``image_path``, equal
evaluator stats), with the flip test off and on in fp32 and on under amp O2; and ``infer`` on a three-image batch whose middle
image has no person and whose ``image_shape`` s differ, under the host and device forms of grouping and finish.

Records of an N = 3 batch are NOT compared with those of N = 1 batches: the library may pick another kernel form for another N."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mindpose_amd as mp  # noqa: E402
from mindpose_amd.data.data_factory import bucket_indices  # noqa: E402
from mindpose_amd.data.transform.utils import transform_keypoints  # noqa: E402

DEV = torch.device("cuda:0")
K = 17
FLIP_PAIRS = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]
# (192, 128): the smallest pair with two distinct stride-32 shapes and two map stages (32 x 48 and 64 x 96)
CFG = dict(image_size=[128, 128], max_image_size=[192, 128], heatmap_sizes=[[32, 32], [64, 64]], pixel_std=200.0, tag_per_joint=True,
           flip_pairs=FLIP_PAIRS)
INFER_CFG = dict(has_heatmap_output=True, hflip_tta=False, joint_order=[0, 1, 2, 3, 4, 5, 6, 11, 12, 7, 8, 9, 10, 13, 14, 15, 16], vis_thr=0.1,
                 ignore_too_much=False, use_rounded_norm=True, tag_thr=1.0, pixel_std=200.0, downsample_scale=2, refine_missing_joint=True,
                 flip_pairs=FLIP_PAIRS)
RECIPE = ["bottomup_rescale", "bottomup_pad"]
LAND, PORT = (3, 128, 192), (3, 192, 128)
# file order; (width, height) -> rescaled (w, h) by hand from BottomUpRescale._get_new_size with max (192, 128):
IMAGES = [("l0.png", 64, 48),     # 1.33 <= 1.5 -> h = 128, w = round(64 * 128 / 48) = 171: landscape
          ("p0.png", 48, 64),     # portrait, limits (128, 192): 0.75 > 0.667 -> w = 128, h = 171
          ("l1.png", 90, 40),     # 2.25 > 1.5 -> w = 192, h = round(40 * 192 / 90) = 85
          ("sq.png", 319, 320),   # PORTRAIT by one pixel: w = 128, h = round(320 * 128 / 319) = round(128.4) = 128 -> pads to landscape
          ("p1.png", 40, 70),     # 0.571 <= 0.667 -> h = 192, w = round(40 * 192 / 70) = 110
          ("l2.png", 80, 50),     # 1.6 > 1.5 -> w = 192, h = 120
          ("l3.png", 70, 52)]     # h = 128, w = round(70 * 128 / 52) = 172
BATCH = 3
# the walk: landscape fills at sq -> [l0, l1, sq]; then the partial lists, portrait (pending since p0) before the second landscape one
WANT = [(["l0.png", "l1.png", "sq.png"], LAND), (["p0.png", "p1.png"], PORT), (["l2.png", "l3.png"], LAND)]
COLUMNS = ["image", "mask", "center", "scale", "image_file", "image_shape"]


def _write_json(path, images, anns):
    with open(path, "w") as f:
        json.dump(dict(images=images, annotations=anns, categories=[dict(id=1, name="person")]), f)


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    from PIL import Image
    root = str(tmp_path_factory.mktemp("bucketed"))
    rng = np.random.RandomState(33)
    images, anns = [], []
    for image_id, (name, w, h) in enumerate(IMAGES, start=1):
        Image.fromarray(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).save(os.path.join(root, name))
        images.append(dict(id=image_id, file_name=name, width=w, height=h))
        kp = np.zeros((K, 3))
        kp[:, 0], kp[:, 1], kp[:, 2] = rng.uniform(0, w, K), rng.uniform(0, h, K), 2
        anns.append(dict(id=image_id, image_id=image_id, category_id=1, iscrowd=0, num_keypoints=K, keypoints=kp.reshape(-1).tolist(),
                         area=float(w * h) / 2, bbox=[0.0, 0.0, float(w), float(h)]))
    ann = os.path.join(root, "ann.json")
    _write_json(ann, images, anns)
    wrong = os.path.join(root, "wrong.json")  # l1's sizes swapped: it would be planned into the portrait bucket
    _write_json(wrong, [dict(im, width=40, height=90) if im["file_name"] == "l1.png" else im for im in images], anns)
    return root, ann, wrong


def _pipeline(folder, ann=None, **kwargs):
    root, default_ann, _ = folder
    ds = mp.create_dataset(root, ann or default_ann, dataset_format="coco_bottomup", is_train=False)
    return mp.create_pipeline(ds, RECIPE, method="bottomup", batch_size=BATCH, is_train=False, config=CFG, **kwargs)


def _epoch(pipe):
    return list(pipe.create_dict_iterator())


@pytest.fixture(scope="module")
def singles(folder):
    """file name -> the batch of the unbucketed pipeline (N = 1, today's behaviour) for that file."""
    pipe = _pipeline(folder, prefetch=0)
    assert pipe.batch_size == 1 and not pipe.bucket_by_shape and len(pipe) == len(IMAGES)
    batches = _epoch(pipe)
    assert [os.path.basename(b["image_file"][0]) for b in batches] == [name for name, _, _ in IMAGES]  # dataset order
    return {os.path.basename(b["image_file"][0]): b for b in batches}


@pytest.fixture(scope="module")
def bucketed(folder):
    pipe = _pipeline(folder, prefetch=0, bucket_by_shape=True)
    assert isinstance(pipe, mp.BottomUpPipeline) and pipe.bucket_by_shape and pipe.batch_size == BATCH and pipe.mode == "rescale_pad"
    assert len(pipe) == pipe.get_dataset_size() == len(WANT)
    return _epoch(pipe)


def _same_batches(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert list(x) == list(y) == COLUMNS
        assert torch.equal(x["image"], y["image"]) and torch.equal(x["mask"], y["mask"]) and x["image_file"] == y["image_file"]
        for key in ("center", "scale", "image_shape"):
            assert np.array_equal(x[key], y[key]) and x[key].dtype == y[key].dtype


def _stack(singles, names):
    """A batch stacked by hand from the N = 1 pipeline's tensors."""
    parts = [singles[name] for name in names]
    out = dict(image=torch.cat([p["image"] for p in parts]), mask=torch.cat([p["mask"] for p in parts]),
               image_file=[p["image_file"][0] for p in parts])
    for key in ("center", "scale", "image_shape"):
        out[key] = np.concatenate([p[key] for p in parts])
    return {k: out[k] for k in COLUMNS}


def test_bucketed_batches_are_what_the_grouping_predicts(folder, bucketed):
    root = folder[0]
    assert [([os.path.basename(f) for f in b["image_file"]], tuple(b["image"].shape[1:])) for b in bucketed] == WANT
    for b, (names, shape) in zip(bucketed, WANT):
        n = len(names)
        assert list(b) == COLUMNS and b["image_file"] == [os.path.join(root, name) for name in names]
        assert b["image"].shape == (n,) + shape and b["image"].is_cuda and b["image"].dtype == torch.float32
        assert b["mask"].shape == (n,) + shape[1:] and b["mask"].is_cuda and b["mask"].dtype == torch.uint8
        assert b["center"].shape == b["scale"].shape == b["image_shape"].shape == (n, 2)
    # the same lists from the grouping function over the declared sizes, keyed by the pipeline's own transforms
    pipe = _pipeline(folder, prefetch=0, bucket_by_shape=True)
    source = pipe.dataset.source
    assert pipe.input_size(319, 320) == (192, 128) and pipe.input_size(48, 64) == (128, 192)
    plan = list(bucket_indices(pipe.dataset.indices(), source.image_size, pipe.input_size, BATCH))
    assert plan == pipe.buckets() == [[0, 2, 3], [1, 4], [5, 6]]
    # images of one batch differ below the shared padded size
    assert bucketed[0]["image_shape"].tolist() == [[171, 128], [192, 85], [128, 128]]


def test_bucketed_rows_are_bit_equal_to_the_unbucketed_pipeline(bucketed, singles):
    _same_batches(bucketed, [_stack(singles, names) for names, _ in WANT])
    for b in bucketed:  # the mask is each image's own rescaled extent
        for row, (w, h) in zip(b["mask"], b["image_shape"].tolist()):
            assert bool(row[:h, :w].all()) and int(row.sum()) == w * h


@pytest.mark.parametrize("kwargs", [dict(prefetch=2), dict(prefetch=2, num_workers=2), dict(prefetch=0, num_workers=2)])
def test_bucketed_batches_under_prefetch_and_codec_workers(folder, bucketed, kwargs):
    pipe = _pipeline(folder, bucket_by_shape=True, **kwargs)
    try:
        _same_batches(bucketed, _epoch(pipe))
        assert len(pipe) == len(WANT)
        _same_batches(bucketed, _epoch(pipe))  # a second epoch (the codec workers, when there are any, live on)
        if kwargs.get("num_workers", 1) > 1:
            assert pipe._codec is not None and pipe._codec.batch == BATCH  # the regions hold the real batch size
    finally:
        pipe.close()
    assert pipe._codec is None


@pytest.mark.parametrize("kwargs", [dict(prefetch=0), dict(prefetch=2, num_workers=2)])
def test_a_wrong_declared_size_names_the_file(folder, kwargs):
    pipe = _pipeline(folder, ann=folder[2], bucket_by_shape=True, **kwargs)
    assert pipe.buckets() == [[1, 2, 4], [0, 3, 5], [6]]  # planned from the json: l1 among the portraits, whose list now fills first
    try:
        with pytest.raises(ValueError, match=r"l1\.png.*40 x 90.*90 x 40"):
            _epoch(pipe)
    finally:
        pipe.close()


# ---- the inferencer -------------------------------------------------------------------------------------------------------------
_NETS = {}


def _net(amp_level):
    if amp_level not in _NETS:  # one network (and its plans) per precision for the whole module
        net = mp.init_synthetic(mp.create_network("hrnet_w32", "higher_hrnet_head"), seed=0).to(DEV).eval()
        if amp_level != "O0":
            mp.models.auto_mixed_precision(net, amp_level)
        _NETS[amp_level] = net
    return _NETS[amp_level]


def _same_record(r, q):
    return r["image_path"] == q["image_path"] and np.array_equal(r["pred"], q["pred"]) and list(r["score"]) == list(q["score"])


@pytest.mark.parametrize("amp_level,flip", [("O0", False), ("O0", True), ("O2", True)])
def test_inferencer_over_bucketed_batches(folder, bucketed, singles, amp_level, flip, monkeypatch):
    monkeypatch.setenv("MINDPOSE_AUTOTUNE", "0")  # the library's own choice of kernel per layer: no candidate timing in this test
    root, ann, _ = folder
    net = _net(amp_level)
    dec = mp.create_decoder("bottomup_heatmap_ae", use_nms=True, nms_kernel=3, max_num=30)
    inf = mp.create_inferencer(mp.create_eval_network(net, dec), "bottomup_heatmap_ae", config=dict(INFER_CFG, hflip_tta=flip), decoder=dec)
    records = inf(bucketed)
    assert [r["image_path"] for r in records] == [f for b in bucketed for f in b["image_file"]]  # one per image, in BATCH order
    assert sorted(os.path.basename(r["image_path"]) for r in records) == sorted(name for name, _, _ in IMAGES)
    assert sum(len(r["pred"]) for r in records) > 0 and all(len(r["pred"]) == len(r["score"]) for r in records)
    assert all(r["pred"].shape[1:] == (K, 3 + (2 if flip else 1)) for r in records if len(r["pred"]))
    if amp_level == "O2" and flip:
        assert any(key[0] == (2 * BATCH,) + LAND for key in net._plans)  # the flip test ran as one 2N forward

    # the same batches stacked by hand from the N = 1 pipeline's tensors, fed in another order
    want = {r["image_path"]: r for r in inf([_stack(singles, names) for names, _ in reversed(WANT)])}
    assert len(want) == len(records) == len(IMAGES)
    for r in records:
        assert _same_record(r, want[r["image_path"]])

    ev = mp.create_evaluator(ann, name="bottomup", metric=["AP"], result_path=os.path.join(root, f"res_{amp_level}_{int(flip)}.json"),
                             config=dict(oks_thr=0.9, use_nms=True, soft_nms=False, sigmas=mp.utils.nms.COCO_SIGMAS.tolist()))
    stats = ev(records)
    assert stats == ev([want[r["image_path"]] for r in reversed(records)])  # keyed on image_path: the record order does not matter
    assert all(name in stats for name in ev.metrics)


def test_infer_on_a_batch_with_an_image_without_persons(monkeypatch):
    """N = 3 with differing ``image_shape`` s; the middle image's heat maps are zero (nothing passes ``vis_thr``).  ``infer`` gives
    one record per image - the empty one included, in place - each the back-projection of that image's own geometry, and the same
    records with the grouping and the finish on the host."""
    gen = torch.Generator().manual_seed(9)
    h, w = 64, 96
    low = torch.rand(3, 2 * K, h // 2, w // 2, generator=gen)
    low[:, K:] *= 8.0  # spread tags: grouping leaves persons with empty joints for the refinement
    high = torch.rand(3, K, h, w, generator=gen)
    low[1, :K] = 0.0
    high[1] = 0.0
    outs = [low.to(DEV), high.to(DEV)]
    shapes = np.array([[171, 128], [192, 85], [128, 128]])
    mask = torch.zeros(3, 2 * h, 2 * w, dtype=torch.uint8)
    for i, (sw, sh) in enumerate(shapes.tolist()):
        mask[i, :sh, :sw] = 1
    batch = dict(image=torch.zeros(3, 3, 2 * h, 2 * w, device=DEV), mask=mask.to(DEV), center=np.array([[32, 24], [45, 20], [160, 160]]),
                 scale=np.array([[0.32, 0.24], [0.45, 0.2], [1.595, 1.6]]), image_shape=shapes, image_file=["a.png", "b.png", "c.png"])
    dec = mp.create_decoder("bottomup_heatmap_ae", use_nms=True, nms_kernel=3, max_num=30)
    inf = mp.BottomUpHeatMapAEInferencer(lambda image, mask: (dec(outs, mask), outs), config=INFER_CFG)

    records = inf.infer([batch])
    assert [r["image_path"] for r in records] == ["a.png", "b.png", "c.png"]
    assert records[1]["pred"].size == 0 and list(records[1]["score"]) == []
    assert len(records[0]["pred"]) > 0 and len(records[2]["pred"]) > 0
    keypoints, scores = inf._parse(*dec(outs, batch["mask"]))
    for i in (0, 2):  # image i alone through the back-projection, with its own centre, scale and map extent
        alone = transform_keypoints([keypoints[i]], batch["center"][i:i + 1], batch["scale"][i:i + 1], shapes[i:i + 1] / 2, pixel_std=200.0)[0]
        assert np.array_equal(records[i]["pred"], alone) and list(records[i]["score"]) == list(scores[i])
        assert not np.array_equal(alone[..., :2], keypoints[i][..., :2])
    for name in ("MINDPOSE_FINISH_DEVICE", "MINDPOSE_MATCH_DEVICE"):
        monkeypatch.setenv(name, "0")  # first the host-driven tail behind the device grouping, then the host grouping as well
        host = inf.infer([batch])
        assert len(host) == 3 and all(_same_record(r, q) for r, q in zip(records, host))
