"""``mp_bottomup_train_augment`` and ``bottomup_augment_batch`` on the GPU.  The oracle is the host chain, bit for bit:
``warp_affine_linear_u8`` + Normalize / HWC2CHW (as tests/test_gpu_loader.py normalises for ``mp_warp_affine``) for the image,
``warp_affine_nearest_u8`` into the stage's corner for the masks, then the column mirror.  The arithmetic is integer up to the one
IEEE expression of the normalise, so every comparison is exact; outputs are prefilled with NaN / 0xFF so an unwritten byte shows."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

import mindpose_amd as mp  # noqa: E402
from mindpose_amd import _lib  # noqa: E402
from mindpose_amd.data.transform.bottomup_transform import warp_affine_linear_u8, warp_affine_nearest_u8  # noqa: E402
from mindpose_amd.data.transform.topdown_transform import launch_warp_affine  # noqa: E402
from oracle import loader as ol  # noqa: E402

DEV = torch.device("cuda:0")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.255)
MEAN255, STD255 = [v * 255 for v in MEAN], [v * 255 for v in STD]
SOURCES = [(53, 37), (61, 80), (64, 64), (1, 1)]  # (h, w): different sizes in one batch, odd extents, a single pixel
CONFIGS = {"vector": dict(image_size=[64, 48], heatmap_sizes=[[16, 12], [32, 24]]),  # 16-byte / 4-byte stores, stage 0 padded
           "scalar": dict(image_size=[50, 38], heatmap_sizes=[[13, 9], [25, 19]])}   # odd widths: one pixel per thread
K = 5


def _cfg(name):
    return dict(CONFIGS[name], max_image_size=CONFIGS[name]["image_size"], flip_pairs=[[1, 2], [3, 4]], pixel_std=200.0, tag_per_joint=True)


def _sources(seed=0):
    rng = np.random.RandomState(seed)
    images = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in SOURCES]
    masks = [rng.randint(1, 256, (h, w)).astype(np.uint8) for h, w in SOURCES]  # no zero inside: a zero in the output is the border
    return images, masks


def _fixed_matrices(affine):
    """Rotation +30 / -30 and scale 0.75 / 1.5 (the ends of the recipe's ranges) with a translation, through the class's own
    ``matrices``: [N, S + 1, 2, 3]."""
    draws = [(30.0, 0.75, (0, 0)), (-30.0, 1.5, (5, -3)), (30.0, 1.5, (-7, 4)), (-30.0, 0.75, (0, 0))]
    mats = []
    for (h, w), (rot, scale, (dx, dy)) in zip(SOURCES, draws):
        img_scale = np.array([w, h], dtype=np.float32)
        img_scale *= scale
        mats.append(affine.matrices(dict(center=np.array((w / 2 + dx, h / 2 + dy)), img_scale=img_scale, rot=rot)))
    return np.stack(mats)


def _launch(images, masks, mats, flips, cfg, image_out=None, mask_out=None):
    """The C entry on prefilled outputs; returns (image, mask) tensors."""
    lib = _lib.load()
    n, sizes = len(images), np.asarray(cfg["heatmap_sizes"])
    s, (out_w, out_h) = len(sizes), cfg["image_size"]
    wmax, hmax = int(sizes[:, 0].max()), int(sizes[:, 1].max())
    base, mbase = min(t.data_ptr() for t in images), min(t.data_ptr() for t in masks)
    offs = torch.tensor([t.data_ptr() - base for t in images], dtype=torch.int64, device=DEV)
    moffs = torch.tensor([t.data_ptr() - mbase for t in masks], dtype=torch.int64, device=DEV)
    hw = torch.tensor([list(t.shape[:2]) for t in images], dtype=torch.int32, device=DEV)
    trans = torch.from_numpy(np.ascontiguousarray(mats, np.float64).reshape(n, s + 1, 6)).to(DEV)
    fl = None if flips is None else torch.tensor(flips, dtype=torch.int32, device=DEV)
    if image_out is None:
        image_out = torch.full((n, 3, out_h, out_w), float("nan"), device=DEV)
    if mask_out is None:
        mask_out = torch.full((n, s, hmax, wmax), 0xFF, dtype=torch.uint8, device=DEV)
    wh = (ctypes.c_int * (2 * s))(*[int(v) for v in sizes.reshape(-1)])
    m3 = (ctypes.c_float * 3)(*[float(np.float32(v * 255.0)) for v in MEAN])
    s3 = (ctypes.c_float * 3)(*[float(np.float32(v * 255.0)) for v in STD])
    _lib.check(lib.mp_bottomup_train_augment(base, _lib.ptr(offs), _lib.ptr(hw), mbase, _lib.ptr(moffs), _lib.ptr(trans), _lib.ptr(fl), wh,
                                             image_out.data_ptr(), mask_out.data_ptr(), n, s, out_h, out_w, hmax, wmax, m3, s3,
                                             _lib.stream()), "mp_bottomup_train_augment")
    torch.cuda.synchronize()
    return image_out, mask_out


def _host_chain(images, masks, mats, flips, cfg):
    sizes = cfg["heatmap_sizes"]
    out_w, out_h = cfg["image_size"]
    wmax, hmax = max(s[0] for s in sizes), max(s[1] for s in sizes)
    ref_image = np.zeros((len(images), 3, out_h, out_w), np.float32)
    ref_mask = np.zeros((len(images), len(sizes), hmax, wmax), np.uint8)
    for i, (img, msk) in enumerate(zip(images, masks)):
        planes = ol.normalize_chw(warp_affine_linear_u8(img, mats[i][-1], (out_w, out_h)), MEAN255, STD255)
        ref_image[i] = planes[:, :, ::-1] if flips is not None and flips[i] else planes
        for j, (w, h) in enumerate(sizes):
            warped = warp_affine_nearest_u8(msk, mats[i][j], (w, h))
            ref_mask[i, j, :h, :w] = warped[:, ::-1] if flips is not None and flips[i] else warped
    return ref_image, ref_mask


@pytest.fixture(scope="module")
def host_refs():
    """The unflipped host chain of both configurations, computed once: a flip is a mirror of these."""
    images, masks = _sources()
    refs = {}
    for name in CONFIGS:
        cfg = _cfg(name)
        mats = _fixed_matrices(mp.BottomUpRandomAffine(config=cfg))
        refs[name] = (cfg, mats) + _host_chain(images, masks, mats, None, cfg)
    dev = [torch.from_numpy(a).to(DEV) for a in images], [torch.from_numpy(a).to(DEV) for a in masks]
    return images, masks, dev, refs


def _mirrored(ref_image, ref_mask, flips, cfg):
    if flips is None:
        return ref_image, ref_mask
    image, mask = ref_image.copy(), ref_mask.copy()
    for i, f in enumerate(flips):
        if f:
            image[i] = ref_image[i][:, :, ::-1]
            for j, (w, h) in enumerate(cfg["heatmap_sizes"]):
                mask[i, j, :h, :w] = ref_mask[i, j, :h, :w][:, ::-1]
    return image, mask


@pytest.mark.parametrize("flips", [None, [1, 0, 0, 1], [0, 1, 1, 0]], ids=["noflip", "flip1001", "flip0110"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_kernel_bit_equal_to_the_host_chain(host_refs, name, flips):
    _, _, (dimages, dmasks), refs = host_refs
    cfg, mats, ref_image, ref_mask = refs[name]
    want_image, want_mask = _mirrored(ref_image, ref_mask, flips, cfg)
    image, mask = _launch(dimages, dmasks, mats, flips, cfg)
    got_image, got_mask = image.cpu().numpy(), mask.cpu().numpy()
    assert not np.isnan(got_image).any(), "an image element was left unwritten"
    assert np.array_equal(got_image.view(np.uint32), want_image.view(np.uint32)), np.abs(got_image - want_image).max()
    assert np.array_equal(got_mask, want_mask), int((got_mask != want_mask).sum())
    # what the cases are there for: part of the output lies outside the source (normalised zero, mask 0 INSIDE the corner, where no
    # source pixel is zero), and the padding beyond a smaller stage is zero
    pad = ol.normalize_chw(np.zeros((1, 1, 3), np.uint8), MEAN255, STD255).reshape(3)
    (w0, h0), (w1, h1) = cfg["heatmap_sizes"]
    for i in (1, 2):  # scale 1.5
        assert (got_image[i] == pad[:, None, None]).all(axis=0).any() and (got_mask[i, 1, :h1, :w1] == 0).any()
        assert (got_mask[i, 1, :h1, :w1] != 0).any()
    assert not got_mask[:, 0, h0:].any() and not got_mask[:, 0, :, w0:].any() and (got_mask[:, 0, :h0, :w0] != 0).any()


def test_flip_is_not_a_no_op_and_is_per_image(host_refs):
    _, _, _, refs = host_refs
    cfg, _, ref_image, ref_mask = refs["vector"]
    image, mask = _mirrored(ref_image, ref_mask, [1, 0, 0, 1], cfg)
    assert not np.array_equal(image[0], ref_image[0]) and np.array_equal(image[1], ref_image[1])
    assert not np.array_equal(mask[0], ref_mask[0]) and np.array_equal(mask[2], ref_mask[2])


@pytest.mark.parametrize("image_shift, mask_shift", [(1, 0), (0, 1), (1, 1)], ids=["image", "mask", "both"])
def test_unaligned_outputs_take_the_scalar_stores_with_the_same_result(host_refs, image_shift, mask_shift):
    """Widths that allow the wide stores, base addresses that do not: the entry falls back per output, the result is the same."""
    _, _, (dimages, dmasks), refs = host_refs
    cfg, mats, ref_image, ref_mask = refs["vector"]
    flips = [0, 1, 1, 0]
    want_image, want_mask = _mirrored(ref_image, ref_mask, flips, cfg)
    image_store = torch.full((ref_image.size + 4,), float("nan"), device=DEV)
    mask_store = torch.full((ref_mask.size + 4,), 0xFF, dtype=torch.uint8, device=DEV)
    image_out = image_store[image_shift:image_shift + ref_image.size].view(ref_image.shape)
    mask_out = mask_store[mask_shift:mask_shift + ref_mask.size].view(ref_mask.shape)
    assert (image_out.data_ptr() % 16 != 0) == bool(image_shift) and (mask_out.data_ptr() % 4 != 0) == bool(mask_shift)
    _launch(dimages, dmasks, mats, flips, cfg, image_out, mask_out)
    assert np.array_equal(image_out.cpu().numpy().view(np.uint32), want_image.view(np.uint32))
    assert np.array_equal(mask_out.cpu().numpy(), want_mask)
    # nothing outside the views was touched
    rest = torch.cat([image_store[:image_shift], image_store[image_shift + ref_image.size:]])
    assert torch.isnan(rest).all()
    assert (torch.cat([mask_store[:mask_shift], mask_store[mask_shift + ref_mask.size:]]) == 0xFF).all()


@pytest.mark.parametrize("name", list(CONFIGS))
def test_image_equals_the_launches_it_replaces(host_refs, name):
    """flip 0: ``mp_warp_affine`` with the image matrix; flip 1: ``mp_flip_width`` of that - to the bit."""
    _, _, (dimages, dmasks), refs = host_refs
    cfg, mats, _, _ = refs[name]
    out_w, out_h = cfg["image_size"]
    n = len(dimages)
    warped = launch_warp_affine(dimages, list(range(n)), mats[:, -1], (out_h, out_w), True, None, MEAN, STD)
    mirrored = torch.empty_like(warped)
    _lib.check(_lib.load().mp_flip_width(_lib.ptr(warped), _lib.ptr(mirrored), n, 3, out_h, out_w, _lib.stream()), "mp_flip_width")
    plain, _ = _launch(dimages, dmasks, mats, [0] * n, cfg)
    flipped, _ = _launch(dimages, dmasks, mats, [1] * n, cfg)
    assert torch.equal(plain.view(torch.int32), warped.view(torch.int32))
    assert torch.equal(flipped.view(torch.int32), mirrored.view(torch.int32))
    assert not torch.equal(plain, flipped)


def _samples(seed=4):
    rng = np.random.RandomState(seed)
    shapes = [(53, 37), (61, 80), (64, 64), (40, 56), (33, 47), (48, 64)]
    images = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in shapes]
    masks = [(rng.rand(h, w) > 0.25).astype(np.uint8) for h, w in shapes]
    persons = [2, 0, 3, 1, 2, 1]
    keypoints = [np.concatenate([rng.uniform(0, w, (m, K, 1)), rng.uniform(0, h, (m, K, 1)), rng.randint(0, 3, (m, K, 1))], axis=2).astype(np.float32)
                 for m, (h, w) in zip(persons, shapes)]
    return images, masks, keypoints


def _host_samples(affine, flip, images, masks, keypoints, seed):
    """The two host ``transform`` s sample by sample under ``seed``; returns the per-sample states and the generator's next draw."""
    s = len(affine._transform_cfg["heatmap_sizes"])
    np.random.seed(seed)
    states = []
    for img, msk, kp in zip(images, masks, keypoints):
        state = dict(image=img, mask=np.repeat(msk[None], s, axis=0), keypoints=np.repeat(kp[None], s, axis=0))
        state.update(affine.transform(state))
        before = state["image"]
        state.update(flip.transform(state))
        state["flipped"] = state["image"] is not before
        states.append(state)
    return states, np.random.rand()


@pytest.mark.parametrize("name", list(CONFIGS))
def test_augment_batch_equals_the_host_transforms_sample_by_sample(name):
    cfg = _cfg(name)
    affine, flip = mp.BottomUpRandomAffine(config=cfg), mp.BottomUpHorizontalRandomFlip(config=cfg, flip_prob=0.5)
    images, masks, keypoints = _samples()
    seed = 7
    states, next_draw = _host_samples(affine, flip, images, masks, keypoints, seed)
    flipped = [st["flipped"] for st in states]
    assert any(flipped) and not all(flipped)
    dimages, dmasks = [torch.from_numpy(a).to(DEV) for a in images], [torch.from_numpy(a).to(DEV) for a in masks]
    kp_before = [a.copy() for a in keypoints]
    np.random.seed(seed)
    out = mp.bottomup_augment_batch(affine, flip, dimages, dmasks, keypoints)
    assert np.random.rand() == next_draw  # the generator was consumed identically
    assert all(np.array_equal(a, b) for a, b in zip(keypoints, kp_before))  # the caller's arrays are not changed
    n, s, m = len(images), len(cfg["heatmap_sizes"]), 3
    assert out["keypoints"].shape == (n, s, m, K, 3) and out["keypoints"].dtype == torch.float32 and out["keypoints"].is_cuda
    assert out["num_persons"].tolist() == [2, 0, 3, 1, 2, 1]
    got_image, got_mask, got_kp = out["image"].cpu().numpy(), out["mask"].cpu().numpy(), out["keypoints"].cpu().numpy()
    assert got_mask.dtype == np.uint8 and got_image.dtype == np.float32
    for i, st in enumerate(states):
        want = ol.normalize_chw(st["image"], MEAN255, STD255)
        assert np.array_equal(got_image[i].view(np.uint32), want.view(np.uint32)), i
        assert np.array_equal(got_mask[i], st["mask"]), i
        count = st["keypoints"].shape[1]
        assert np.array_equal(got_kp[i, :, :count], st["keypoints"]), i
        assert not got_kp[i, :, count:].any()
    # the same seed again: bit-identical, also into a caller's buffer
    np.random.seed(seed)
    buf = torch.full_like(out["image"], float("nan"))
    again = mp.bottomup_augment_batch(affine, flip, dimages, dmasks, keypoints, out=buf)
    assert again["image"].data_ptr() == buf.data_ptr()
    for key in ("image", "mask", "keypoints"):
        assert torch.equal(again[key], out[key]), key
    # without the flip transform no flip number is drawn and nothing is mirrored
    np.random.seed(seed)
    plain = mp.bottomup_augment_batch(affine, None, dimages[:1], dmasks[:1], keypoints[:1])
    after_plain = np.random.rand()
    np.random.seed(seed)
    only_affine = affine.transform(dict(image=images[0], mask=np.repeat(masks[0][None], s, axis=0), keypoints=np.repeat(keypoints[0][None], s, axis=0)))
    assert np.random.rand() == after_plain
    assert np.array_equal(plain["mask"][0].cpu().numpy(), only_affine["mask"])
    assert np.array_equal(plain["image"][0].cpu().numpy(), ol.normalize_chw(only_affine["image"], MEAN255, STD255))


def test_end_of_the_chain_targets_and_loss():
    """bottomup_augment_batch -> generate_batch -> AEMultiLoss: targets and tag indices equal the host path's on the host-augmented
    samples (the key points are identical, so no tolerance), the uint8 mask goes into the loss as it is."""
    cfg = _cfg("vector")
    affine, flip = mp.BottomUpRandomAffine(config=cfg), mp.BottomUpHorizontalRandomFlip(config=cfg, flip_prob=0.5)
    target_gen = mp.BottomUpGenerateTarget(config=cfg, sigma=2.0, max_num=4)
    images, masks, keypoints = _samples()
    seed = 7
    states, _ = _host_samples(affine, flip, images, masks, keypoints, seed)
    np.random.seed(seed)
    out = mp.bottomup_augment_batch(affine, flip, [torch.from_numpy(a).to(DEV) for a in images], [torch.from_numpy(a).to(DEV) for a in masks],
                                    keypoints)
    target, tag_ind = target_gen.generate_batch(out["keypoints"], out["num_persons"])
    got_target, got_tag = target.cpu().numpy(), tag_ind.cpu().numpy()
    for i, st in enumerate(states):
        want = target_gen.transform(dict(keypoints=st["keypoints"]))
        assert np.array_equal(got_tag[i], want["tag_ind"]), i
        assert np.array_equal(got_target[i].view(np.uint32), want["target"].view(np.uint32)), (i, np.abs(got_target[i] - want["target"]).max())
    assert got_tag[..., 1].sum() > 0 and got_target.max() > 0.5
    n = len(images)
    (w0, h0), (w1, h1) = cfg["heatmap_sizes"]
    g = torch.Generator().manual_seed(0)
    preds = [torch.randn(n, 2 * K, h0, w0, generator=g).to(DEV).requires_grad_(), torch.randn(n, K, h1, w1, generator=g).to(DEV).requires_grad_()]
    loss_fn = mp.AEMultiLoss(num_joints=K, num_stages=2, stage_sizes=[(w0, h0), (w1, h1)])
    assert out["mask"].dtype == torch.uint8
    loss = loss_fn(preds, target, out["mask"], tag_ind)
    loss.sum().backward()
    assert loss.shape == (3,) and torch.isfinite(loss).all() and float(loss[0]) > 0
    for p in preds:
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0


def test_cpu_tensors_raise():
    cfg = _cfg("vector")
    affine, flip = mp.BottomUpRandomAffine(config=cfg), mp.BottomUpHorizontalRandomFlip(config=cfg)
    image, mask = torch.zeros(20, 30, 3, dtype=torch.uint8), torch.ones(20, 30, dtype=torch.uint8)
    kp = [np.zeros((1, K, 3), np.float32)]
    with pytest.raises(_lib.MindposeHipError):
        mp.bottomup_augment_batch(affine, flip, [image], [mask.to(DEV)], kp)
    with pytest.raises(_lib.MindposeHipError):
        mp.bottomup_augment_batch(affine, flip, [image.to(DEV)], [mask], kp)
