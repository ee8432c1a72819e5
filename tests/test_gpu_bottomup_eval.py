"""Bottom-up evaluation on the MI355X: the fused rescale + pad + Normalize kernel and the resize path of the pipeline against the
host transform chain (bit-equal: integer pixels, then the same IEEE expression), the device missing-joint refinement against the
host ``refine_missing_joint`` (bit-equal, dyadic and random-normal maps), the inferencer without map downloads, and dataset ->
pipeline -> HigherHRNet -> inferencer -> evaluator end to end."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mindpose_amd as mp  # noqa: E402
from mindpose_amd import _lib  # noqa: E402
from mindpose_amd.data.transform.bottomup_transform import launch_resize_pad_normalize  # noqa: E402
from mindpose_amd.engine.inferencer.bottomup_inferencer import refine_missing_joint  # noqa: E402
from oracle import loader as ol  # noqa: E402

DEV = torch.device("cuda:0")
K = 17
FLIP_PAIRS = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]
CFG = dict(image_size=[512, 512], max_image_size=[832, 512], heatmap_sizes=[[128, 128], [256, 256]], pixel_std=200.0, tag_per_joint=True,
           flip_pairs=FLIP_PAIRS)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.255)
MEAN255, STD255 = [m * 255.0 for m in MEAN], [s * 255.0 for s in STD]
INFER_CFG = dict(has_heatmap_output=True, hflip_tta=False, joint_order=[0, 1, 2, 3, 4, 5, 6, 11, 12, 7, 8, 9, 10, 13, 14, 15, 16], vis_thr=0.1,
                 ignore_too_much=False, use_rounded_norm=True, tag_thr=1.0, pixel_std=200.0, downsample_scale=2, refine_missing_joint=True,
                 flip_pairs=FLIP_PAIRS)


# ---- mp_resize_pad_normalize ---------------------------------------------------------------------------------------------------
def _host_chain(image, cfg):
    """rescale -> pad -> Normalize + HWC2CHW on the host: (image [3, PH, PW] fp32, mask [PH, PW] uint8, the rescale's state)."""
    state = dict(image=image)
    state.update(mp.BottomUpRescale(is_train=False, config=cfg).transform(state))
    state.update(mp.BottomUpPad(is_train=False, config=cfg).transform(state))
    return ol.normalize_chw(state["image"], MEAN255, STD255), state["mask"], state


# (source w, h) at max_image_size (832, 512); the last case has an odd padded width: the scalar-store form of the kernel
@pytest.mark.parametrize("w,h,max_size", [(640, 480, (832, 512)), (480, 640, (832, 512)), (500, 375, (832, 512)), (333, 500, (832, 512)),
                                          (64, 48, (832, 512)), (832, 512, (832, 512)), (80, 60, (101, 64))])
def test_resize_pad_normalize_bit_equal_to_host_chain(w, h, max_size):
    cfg = dict(CFG, max_image_size=list(max_size))
    image = np.random.RandomState(w + h).randint(0, 256, (h, w, 3)).astype(np.uint8)
    want_image, want_mask, state = _host_chain(image, cfg)
    padded = mp.BottomUpPad(is_train=False, config=cfg).padded_size(*state["image_shape"])
    assert (padded[1], padded[0]) == want_mask.shape
    got_image, got_mask = launch_resize_pad_normalize([torch.from_numpy(image).to(DEV)], [state["image_shape"]], padded, MEAN, STD)
    assert got_image.shape == (1, 3) + want_mask.shape and got_mask.dtype == torch.uint8
    assert torch.equal(got_mask[0].cpu(), torch.from_numpy(want_mask))
    assert torch.equal(got_image[0].cpu(), torch.from_numpy(want_image))


def test_resize_pad_normalize_batch_of_images():
    """Several sources of different sizes in one launch (packed views of one buffer, as the pipeline uploads them)."""
    rng = np.random.RandomState(3)
    images = [rng.randint(0, 256, s).astype(np.uint8) for s in ((480, 640, 3), (375, 500, 3), (100, 260, 3))]
    sizes = [(im.size + 255) & ~255 for im in images]
    packed = torch.zeros(sum(sizes), dtype=torch.uint8, device=DEV)
    views, off = [], 0
    for im, size in zip(images, sizes):
        packed[off:off + im.size] = torch.from_numpy(im.reshape(-1)).to(DEV)
        views.append(packed[off:off + im.size].view(im.shape))
        off += size
    want = [_host_chain(im, CFG) for im in images]
    got_image, got_mask = launch_resize_pad_normalize(views, [w[2]["image_shape"] for w in want], (832, 512), MEAN, STD)
    for i, (image, mask, _) in enumerate(want):
        assert torch.equal(got_image[i].cpu(), torch.from_numpy(image)) and torch.equal(got_mask[i].cpu(), torch.from_numpy(mask))


def test_resize_pad_normalize_error_codes():
    lib = _lib.load()
    src = torch.zeros(48 * 64 * 3, dtype=torch.uint8, device=DEV)
    offs = torch.zeros(1, dtype=torch.int64, device=DEV)
    hw = torch.tensor([[48, 64]], dtype=torch.int32, device=DEV)
    out = torch.empty(1, 3, 64, 96, device=DEV)
    mask = torch.empty(1, 64, 96, dtype=torch.uint8, device=DEV)
    m3, s3 = (ctypes.c_float * 3)(*MEAN255), (ctypes.c_float * 3)(*STD255)

    def call(twh=(85, 64), n=1, ph=64, pw=96, src_=src, out_=out, mask_=mask, std=s3, twh_null=False):
        t = None if twh_null else (ctypes.c_int * 2)(*twh)
        return lib.mp_resize_pad_normalize(_lib.ptr(src_), _lib.ptr(offs), _lib.ptr(hw), t, _lib.ptr(out_), _lib.ptr(mask_), n, ph, pw, m3,
                                           std, _lib.stream())

    assert call() == 0
    assert call(src_=None) == -1 and call(out_=None) == -1 and call(mask_=None) == -1 and call(twh_null=True) == -1 and call(std=None) == -1
    assert call(n=0) == -2 and call(ph=0) == -2 and call(pw=-1) == -2
    assert call(twh=(97, 64)) == -2 and call(twh=(85, 65)) == -2 and call(twh=(0, 64)) == -2  # tw > PW, th > PH, empty target
    assert call(std=(ctypes.c_float * 3)(1.0, 0.0, 1.0)) == -2
    torch.cuda.synchronize()
    with pytest.raises(_lib.MindposeHipError):
        launch_resize_pad_normalize([torch.zeros(4, 4, 3, dtype=torch.uint8)], [(4, 4)], (8, 8), MEAN, STD)  # a CPU source: no fallback


# ---- a synthetic COCO folder with .npy payloads ----------------------------------------------------------------------------------
def _write_folder(tmp_path):
    """Landscape, portrait and an image without annotations; the files hold .npy payloads, which the codec accepts."""
    rng = np.random.RandomState(21)
    images = [dict(id=7, file_name="land.jpg", width=640, height=480), dict(id=3, file_name="port.jpg", width=480, height=640),
              dict(id=9, file_name="none.jpg", width=500, height=375)]
    pixels = {}
    for im in images:
        pixels[im["file_name"]] = rng.randint(0, 256, (im["height"], im["width"], 3)).astype(np.uint8)
        with open(os.path.join(tmp_path, im["file_name"]), "wb") as f:
            np.save(f, pixels[im["file_name"]])
    anns = []
    for ann_id, (image_id, x0, y0) in enumerate(((7, 50, 60), (7, 300, 200), (3, 100, 300)), start=1):
        kp = np.zeros((K, 3))
        kp[:, 0], kp[:, 1], kp[:, 2] = x0 + rng.uniform(0, 120, K), y0 + rng.uniform(0, 120, K), 2
        anns.append(dict(id=ann_id, image_id=image_id, category_id=1, iscrowd=0, num_keypoints=K, keypoints=kp.reshape(-1).tolist(),
                         area=14400.0, bbox=[x0, y0, 120.0, 120.0]))
    ann = os.path.join(tmp_path, "ann.json")
    with open(ann, "w") as f:
        json.dump(dict(images=images, annotations=anns, categories=[dict(id=1, name="person")]), f)
    return ann, pixels


def _same_batches(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert list(x) == list(y) == ["image", "mask", "center", "scale", "image_file", "image_shape"]
        assert torch.equal(x["image"], y["image"]) and torch.equal(x["mask"], y["mask"]) and x["image_file"] == y["image_file"]
        for key in ("center", "scale", "image_shape"):
            assert np.array_equal(x[key], y[key])


def test_bottomup_resize_through_the_pipeline(tmp_path):
    ann, pixels = _write_folder(tmp_path)
    ds = mp.create_dataset(str(tmp_path), ann, dataset_format="coco_bottomup", is_train=False)
    pipe = mp.create_pipeline(ds, [{"bottomup_resize": dict(size=512, base_length=64)}], method="bottomup", batch_size=8, is_train=False,
                              config=CFG, prefetch=0)
    assert isinstance(pipe, mp.BottomUpPipeline) and pipe.batch_size == 1 and len(pipe) == 3 and pipe.mode == "resize"
    batches = list(pipe.create_dict_iterator())
    t = mp.BottomUpResize(is_train=False, config=CFG)
    for batch, name in zip(batches, ("land.jpg", "port.jpg", "none.jpg")):
        image = pixels[name]
        geo = t.geometry(image.shape[1], image.shape[0])
        tw, th = geo["image_shape"]
        want = ol.normalize_chw(ol.warp_affine(image, geo["_trans"], tw, th), MEAN255, STD255)
        assert batch["image"].shape == (1, 3, th, tw) and batch["image"].is_cuda and batch["image"].dtype == torch.float32
        assert torch.equal(batch["image"][0].cpu(), torch.from_numpy(want))
        assert batch["mask"].shape == (1, th, tw) and batch["mask"].dtype == torch.uint8 and batch["mask"].is_cuda and bool(batch["mask"].all())
        assert np.array_equal(batch["center"], geo["center"][None]) and np.array_equal(batch["scale"], geo["scale"][None])
        assert batch["image_shape"].tolist() == [[tw, th]] and batch["image_file"] == [os.path.join(str(tmp_path), name)]
        # the transform's own host path is the same arithmetic
        assert np.array_equal(t.transform(dict(image=image))["image"], ol.warp_affine(image, geo["_trans"], tw, th))


def test_pipeline_fallback_without_pad_uses_the_host_chain(tmp_path):
    ann, pixels = _write_folder(tmp_path)
    ds = mp.create_dataset(str(tmp_path), ann, dataset_format="coco_bottomup", is_train=False)
    pipe = mp.create_pipeline(ds, ["bottomup_rescale"], method="bottomup", is_train=False, config=CFG, prefetch=0)
    assert pipe.mode == "host"
    batch = next(iter(pipe))
    want = mp.BottomUpRescale(is_train=False, config=CFG).transform(dict(image=pixels["land.jpg"]))["image"]
    assert batch["image"].shape == (1, 3, 512, 683) and bool(batch["mask"].all()) and batch["mask"].shape == (1, 512, 683)
    assert np.allclose(batch["image"][0].cpu().numpy(), ol.normalize_chw(want, MEAN255, STD255), rtol=1e-6, atol=1e-6)


# ---- mp_bottomup_refine_missing ------------------------------------------------------------------------------------------------
def _dyadic(gen, *shape, lo=-1.0, hi=1.0):
    return (torch.randint(int(lo * 1024), int(hi * 1024), shape, generator=gen).float() / 1024.0)


def _people(gen, n, h, w, num_tags, persons_per_image, located_counts):
    """keypoints [P_i, K, 3 + L] per image: ``located_counts[p]`` located joints (value > 0, coordinates off the integer grid as the decoder's +-0.25 shift leaves them), the
    others empty (all zero) - the shape ``match_by_tag`` hands to the refinement."""
    out = []
    for i in range(n):
        people = np.zeros((persons_per_image, K, 3 + num_tags), np.float32)
        for p in range(persons_per_image):
            count = located_counts[(i * persons_per_image + p) % len(located_counts)]
            joints = torch.randperm(K, generator=gen)[:count].numpy()
            people[p, joints, 0] = torch.randint(0, w, (count,), generator=gen).numpy() + 0.25
            people[p, joints, 1] = torch.randint(0, h, (count,), generator=gen).numpy() + 0.75
            people[p, joints, 2] = 0.5
        out.append(people)
    return out


def _check_refine(heat, tagging, keypoints):
    """The device path on CUDA maps against the host function on the same maps, person by person: bit-equal key points."""
    want = [kp.copy() for kp in keypoints]
    heat_np, tag_np = heat.numpy(), tagging.numpy()
    if tag_np.shape[1] != heat_np.shape[1]:  # tag_per_joint=False: the reference broadcasts the single tag map to every joint
        tag_np = np.broadcast_to(tag_np, heat_np.shape[:2] + tag_np.shape[2:])
    for i in range(len(want)):
        for p in range(len(want[i])):
            want[i][p] = refine_missing_joint(heat_np[i], tag_np[i], want[i][p])
    got = [kp.copy() for kp in keypoints]
    mp.BottomUpHeatMapAEInferencer._refine_on_device(got, heat.to(DEV), tagging.to(DEV))
    for g, r in zip(got, want):
        assert np.array_equal(g, r)
    return got


@pytest.mark.parametrize("kind", ["dyadic", "normal"])
@pytest.mark.parametrize("num_tags,tag_per_joint,h,w", [(1, True, 24, 40), (2, True, 64, 104), (2, False, 24, 40), (1, False, 33, 17)])
def test_refine_missing_bit_equal_to_host(kind, num_tags, tag_per_joint, h, w):
    gen = torch.Generator().manual_seed(100 * num_tags + h + (kind == "normal"))
    n, ktag = 2, K if tag_per_joint else 1
    if kind == "dyadic":  # multiples of 1 / 1024: differences and the mean of a few tags stay short fractions
        heat, tagging = _dyadic(gen, n, K, h, w), _dyadic(gen, n, ktag, h, w, num_tags, lo=-4.0, hi=4.0)
    else:  # the mean comes from the host and sqrtf / rintf are exact operations: random-normal maps must be bit-equal as well
        heat, tagging = torch.randn(n, K, h, w, generator=gen), 2.0 * torch.randn(n, ktag, h, w, num_tags, generator=gen)
    keypoints = _people(gen, n, h, w, num_tags, 5, located_counts=(1, 3, 9, 16, 1))  # persons with ONE located joint included
    got = _check_refine(heat, tagging, keypoints)
    filled = sum(int(((g[..., 2] != 0) & (k[..., 2] == 0)).sum()) for g, k in zip(got, keypoints))
    assert filled > 0  # the case does refine something


def test_refine_missing_edges():
    gen = torch.Generator().manual_seed(7)
    h, w = 20, 36
    heat = _dyadic(gen, 1, K, h, w, lo=0.0, hi=0.5)
    tagging = torch.zeros(1, K, h, w, 1)
    # joint 1: every value <= 0 -> the winner's value is not > 0: the joint stays empty
    heat[0, 1] = -heat[0, 1]
    # joint 2: a constant plane - every pixel ties, flat index 0 wins; equal neighbours compare "not greater": both shifts are -0.25
    heat[0, 2] = 0.25
    # joint 3: the same maximum at two pixels: the lower flat index wins
    heat[0, 3, 5, 30] = heat[0, 3, 11, 2] = 0.75
    # joints 4-7: the winner in each corner, joints 8-9 on the left / bottom edge: the neighbours are clamped to the winner itself
    for joint, (y, x) in zip(range(4, 10), ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (9, 0), (h - 1, 17))):
        heat[0, joint, y, x] = 0.875
    person = np.zeros((1, K, 4), np.float32)
    person[0, 0] = (3.0, 4.0, 0.5, 0.0)  # one located joint; its tag (0) is the mean tag: the distance term is 0 everywhere
    got = _check_refine(heat, tagging, [person])[0][0]
    assert got[1, 2] == 0 and got[1, :2].tolist() == [0.0, 0.0]
    assert got[2, :3].tolist() == [0.25, 0.25, 0.25]
    assert got[3, 2] == 0.75 and int(got[3, 1]) == 5 and int(got[3, 0]) == 30
    assert [int(v) for v in got[4:10, 0]] == [0, w - 1, 0, w - 1, 0, 17] and [int(v) for v in got[4:10, 1]] == [0, 0, h - 1, h - 1, 9, h - 1]
    assert (got[4:10, 2] == 0.875).all()
    # the rounded tag distance moves the winner: far tags on the maximum of joint 10 push it to the runner-up
    tagging2 = tagging.clone()
    top = int(heat[0, 10].argmax())
    tagging2[0, 10, top // w, top % w, 0] = 3.0
    got2 = _check_refine(heat, tagging2, [person])[0][0]
    assert (int(got2[10, 1]), int(got2[10, 0])) != (top // w, top % w)


def test_refine_missing_no_persons_is_no_launch():
    lib = _lib.load()
    assert lib.mp_bottomup_refine_missing(None, None, None, None, 0, 1, K, 8, 8, 1, 1, None, _lib.stream()) == 0  # P = 0: nothing is read
    heat, tagging = torch.zeros(1, K, 8, 8, device=DEV), torch.zeros(1, K, 8, 8, 1, device=DEV)
    keypoints = [np.array([])]
    mp.BottomUpHeatMapAEInferencer._refine_on_device(keypoints, heat, tagging)  # an image without persons: no error
    assert keypoints[0].size == 0
    found = torch.empty(1, K, 3, device=DEV)
    img = torch.zeros(1, dtype=torch.int32, device=DEV)
    mean = torch.zeros(1, 1, device=DEV)
    args = (_lib.ptr(mean), _lib.ptr(img), 1, 1, K, 8, 8, 1)
    assert lib.mp_bottomup_refine_missing(None, _lib.ptr(tagging), *args, 1, _lib.ptr(found), _lib.stream()) == -1
    assert lib.mp_bottomup_refine_missing(_lib.ptr(heat), _lib.ptr(tagging), *args, 0, _lib.ptr(found), _lib.stream()) == -3  # L = 0
    assert lib.mp_bottomup_refine_missing(_lib.ptr(heat), _lib.ptr(tagging), _lib.ptr(mean), _lib.ptr(img), 1, 1, K, 0, 8, 1, 1,
                                          _lib.ptr(found), _lib.stream()) == -2


# ---- the inferencer ----------------------------------------------------------------------------------------------------------
def test_inferencer_refines_without_downloading_the_maps(monkeypatch):
    gen = torch.Generator().manual_seed(5)
    h, w = 128, 128
    low = torch.rand(1, 2 * K, h // 2, w // 2, generator=gen)
    low[:, K:] *= 8.0  # spread tags: grouping leaves persons with empty joints for the refinement
    outs = [low.to(DEV), torch.rand(1, K, h, w, generator=gen).to(DEV)]
    mask = torch.ones(1, 2 * h, 2 * w, dtype=torch.uint8, device=DEV)
    dec = mp.create_decoder("bottomup_heatmap_ae", use_nms=True, nms_kernel=3, max_num=30)
    batch = dict(image=torch.zeros(1, 3, 2 * h, 2 * w, device=DEV), mask=mask, center=np.array([[128, 128]]), scale=np.array([[1.28, 1.28]]),
                 image_shape=np.array([[256, 256]]), image_file=["a.jpg"])

    def on_device(image, mask):
        return dec(outs, mask), outs

    def maps_on_host(image, mask):
        val_k, tag_k, ind_k, raw, tagging = dec(outs, mask)
        return (val_k, tag_k, ind_k, raw.cpu(), tagging.cpu()), outs

    host = mp.BottomUpHeatMapAEInferencer(maps_on_host, config=INFER_CFG).infer([batch])
    plain = mp.BottomUpHeatMapAEInferencer(on_device, config=dict(INFER_CFG, refine_missing_joint=False)).infer([batch])
    large = []
    original = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: (large.append(t.numel()) if t.numel() >= K * h * w else None, original(t, *a, **k))[1])
    device = mp.BottomUpHeatMapAEInferencer(on_device, config=INFER_CFG).infer([batch])
    monkeypatch.undo()
    assert large == []  # neither heatmap_raw [1, 17, H, W] nor tagging came to the host
    assert len(device) == len(host) == 1 and device[0]["image_path"] == "a.jpg"
    assert np.array_equal(device[0]["pred"], host[0]["pred"]) and device[0]["score"] == host[0]["score"]
    assert len(device[0]["pred"]) > 0 and not np.array_equal(device[0]["pred"], plain[0]["pred"])  # the refinement filled joints


# ---- dataset -> pipeline -> network -> inferencer -> evaluator -------------------------------------------------------------------
def test_end_to_end_evaluation(tmp_path, monkeypatch):
    monkeypatch.setenv("MINDPOSE_AUTOTUNE", "0")  # the library's own choice of kernel per layer: no candidate timing in this test
    ann, pixels = _write_folder(tmp_path)
    ds = mp.create_dataset(str(tmp_path), ann, dataset_format="coco_bottomup", is_train=False)

    def batches(**kwargs):
        pipe = mp.create_pipeline(ds, ["bottomup_rescale", "bottomup_pad"], method="bottomup", batch_size=4, is_train=False, config=CFG, **kwargs)
        assert isinstance(pipe, mp.BottomUpPipeline) and pipe.mode == "rescale_pad" and pipe.get_dataset_size() == 3
        try:
            return list(pipe.create_dict_iterator())
        finally:
            pipe.close()

    sync = batches(prefetch=0)
    _same_batches(sync, batches(prefetch=2))
    _same_batches(sync, batches(prefetch=2, num_workers=2))  # the codec workers read the files themselves (lazy image paths)
    assert [tuple(b["image"].shape) for b in sync] == [(1, 3, 512, 832), (1, 3, 832, 512), (1, 3, 512, 832)]
    assert all(b["image"].is_cuda and b["image"].dtype == torch.float32 and b["mask"].is_cuda and b["mask"].dtype == torch.uint8 for b in sync)

    # the same batches from the host transform chain
    host = []
    for name in ("land.jpg", "port.jpg", "none.jpg"):
        image, mask, state = _host_chain(pixels[name], CFG)
        host.append(dict(image=torch.from_numpy(image)[None].to(DEV), mask=torch.from_numpy(mask)[None].to(DEV), center=state["center"][None],
                         scale=state["scale"][None], image_file=[os.path.join(str(tmp_path), name)],
                         image_shape=np.asarray(state["image_shape"])[None]))
    _same_batches(sync, [{k: b[k] for k in sync[0]} for b in host])

    net = mp.init_synthetic(mp.create_network("hrnet_w32", "higher_hrnet_head"), seed=0).to(DEV).eval()
    dec = mp.create_decoder("bottomup_heatmap_ae", use_nms=True, nms_kernel=3, max_num=30)
    inf = mp.create_inferencer(mp.create_eval_network(net, dec), "bottomup_heatmap_ae", config=INFER_CFG)
    records, want = inf(sync), inf(host)
    assert [r["image_path"] for r in records] == [b["image_file"][0] for b in sync]
    for r, q in zip(records, want):
        assert np.array_equal(r["pred"], q["pred"]) and r["score"] == q["score"] and r["image_path"] == q["image_path"]

    ev = mp.create_evaluator(ann, name="bottomup", metric=["AP"], result_path=os.path.join(str(tmp_path), "res.json"),
                             config=dict(oks_thr=0.9, use_nms=True, soft_nms=False, sigmas=mp.utils.nms.COCO_SIGMAS.tolist()))
    stats = ev(records)
    assert all(name in stats for name in ev.metrics) and -1.0 <= stats["AP"] <= 1.0
