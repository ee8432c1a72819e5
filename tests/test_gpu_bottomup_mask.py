"""``bottomup_masks_batch`` / ``mp_bottomup_train_masks`` and the per-stage planes of ``bottomup_augment_batch`` on the GPU.  The oracle
of the masks is ``decode_mask_info`` (itself checked against scipy in tests/test_bottomup_mask_cpu.py), bit for bit: the arithmetic is
integer.  Output buffers are prefilled with 0xAB and carry guard bytes behind every image, so an unwritten byte and a byte written
outside a block both show."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

import mindpose_amd as mp  # noqa: E402
from mindpose_amd import _lib  # noqa: E402
from mindpose_amd.data.transform import bottomup_mask as bm  # noqa: E402
from tests import bottomup_mask_cases as cases  # noqa: E402

DEV = torch.device("cuda:0")
RADII = [(24, 12), (6,), (0, 0)]
FILL = 0xAB


@functools.lru_cache(maxsize=None)
def _reference(layout, h, w, radii):
    """The host mask of one case, computed once and shared (read-only)."""
    ref = bm.decode_mask_info(cases.mask_info(layout, h, w, radii))
    ref.setflags(write=False)
    return ref


def _run_guarded(infos, guard=5, shift=0):
    """The launch on a 0xAB buffer, image blocks ``guard`` bytes apart from ``shift`` on; returns the per-image arrays after
    checking that nothing outside the blocks was written."""
    offsets, total = [], shift
    for info in infos:
        offsets.append(total)
        total += int(np.prod(info["shape"])) + guard
    buf = torch.full((total,), FILL, dtype=torch.uint8, device=DEV)
    views = bm.launch_bottomup_masks(infos, buf, offsets)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    inside = np.zeros(total, bool)
    for info, off, view in zip(infos, offsets, views):
        size = int(np.prod(info["shape"]))
        inside[off:off + size] = True
        assert tuple(view.shape) == tuple(info["shape"]) and view.is_contiguous() and view.data_ptr() == buf.data_ptr() + off
    assert (host[~inside] == FILL).all(), "a byte outside the image blocks was written"
    return [host[off:off + int(np.prod(info["shape"]))].reshape(info["shape"]) for info, off in zip(infos, offsets)]


@pytest.mark.parametrize("radii", RADII, ids=lambda r: "r" + "_".join(map(str, r)))
@pytest.mark.parametrize("h, w", cases.SHAPES, ids=lambda v: str(v))
def test_single_image_bit_equal_to_the_host(h, w, radii):
    for layout in cases.LAYOUTS:
        want = _reference(layout, h, w, radii)
        for shift in (0, 1):  # 16-byte aligned blocks (dword stores where the width allows) and odd addresses (byte stores)
            (got,) = _run_guarded([cases.mask_info(layout, h, w, radii)], shift=shift)
            assert got.max() <= 1, (layout, shift, "an output byte was left unwritten")
            assert np.array_equal(got, want), (layout, shift, int((got != want).sum()))
    assert _reference("none", h, w, radii).all() and not _reference("whole", h, w, radii).any()
    if radii[0] and h > 1:  # the cases are there to erode: the interior pixel prints a disc, a larger radius removes more
        r0 = _reference("pixel_interior", h, w, radii)[0]
        assert (r0 == 0).sum() > 1
        if len(radii) > 1:
            assert (r0 == 0).sum() > (_reference("pixel_interior", h, w, radii)[1] == 0).sum()


MIXED = [("crowd300", 53, 70), ("borders", 40, 37), ("overlap", 64, 128), ("wrap", 1, 9), ("pixel_corner", 64, 128)]
MIXED_EMPTY = [("none", 64, 128), ("crowd300", 40, 37), ("none", 53, 70), ("starts_with_0", 64, 128), ("none", 1, 9)]


@pytest.mark.parametrize("radii", RADII, ids=lambda r: "r" + "_".join(map(str, r)))
@pytest.mark.parametrize("batch", [MIXED, MIXED_EMPTY, [("none", 40, 37)] * 2], ids=["mixed", "with_empty", "all_empty"])
def test_batches_of_mixed_sizes(batch, radii):
    infos = [cases.mask_info(layout, h, w, radii) for layout, h, w in batch]
    for guard, shift in ((16, 0), (5, 3)):  # every block dword-aligned / most blocks not
        got = _run_guarded(infos, guard=guard, shift=shift)
        for (layout, h, w), g in zip(batch, got):
            assert np.array_equal(g, _reference(layout, h, w, radii)), (layout, h, w, guard)
    # the public function: views of one packed buffer, bit-identical on a repeat
    first = mp.bottomup_masks_batch(infos, DEV)
    again = mp.bottomup_masks_batch(infos, DEV)
    lo, hi = min(t.data_ptr() for t in first), max(t.data_ptr() + t.numel() for t in first)
    assert hi - lo <= sum(t.numel() + 16 for t in first)  # one packed buffer
    for (layout, h, w), a, b in zip(batch, first, again):
        assert a.is_cuda and a.dtype == torch.uint8 and a.is_contiguous() and tuple(a.shape) == (len(radii), h, w)
        assert np.array_equal(a.cpu().numpy(), _reference(layout, h, w, radii)) and torch.equal(a, b)


def test_refusals_return_their_codes():
    lib = _lib.load()
    info = cases.mask_info("overlap", 40, 37, (6,))
    out = torch.full((40 * 37,), FILL, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(40 * 37, dtype=torch.uint8, device=DEV)
    good = np.cumsum(info["regions"][0], dtype=np.uint32)
    tab_dev = torch.zeros(64, dtype=torch.int64, device=DEV)  # never read: every call below is refused before a launch

    def call(prefix=good, tab=(40, 37, 0, 1), radii=(6,), s=1, n=1, out_ptr=out.data_ptr()):
        prefix = np.ascontiguousarray(prefix, np.uint32)
        region_ptr = (ctypes.c_int * 2)(0, len(prefix))
        return lib.mp_bottomup_train_masks(prefix.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), region_ptr, (ctypes.c_int * 4)(*tab),
                                           (ctypes.c_longlong * 2)(0, 0), tab_dev.data_ptr(), tab_dev.data_ptr(), tab_dev.data_ptr(),
                                           tab_dev.data_ptr(), (ctypes.c_int * len(radii))(*radii), (ctypes.c_uint8 * 1024)(), out_ptr,
                                           out.numel(), ws.data_ptr(), ws.numel(), n, s, _lib.stream())

    assert call(out_ptr=None) == -1
    assert call(s=0) == _lib.MP_ERR_UNSUPPORTED and call(s=9) == _lib.MP_ERR_UNSUPPORTED and call(radii=(128,)) == _lib.MP_ERR_UNSUPPORTED
    assert call(n=0) == -2 and call(n=65536) == -2 and call(tab=(0, 37, 0, 1)) == -2 and call(tab=(40, -37, 0, 1)) == -2
    short = good.copy()
    short[-1] -= 1
    assert call(prefix=short) == -2 and call(tab=(41, 37, 0, 1)) == -2  # counts that do not sum to H * W
    torch.cuda.synchronize()
    assert (out == FILL).all()  # nothing was launched
    with pytest.raises(_lib.MindposeHipError, match="bad shape"):
        bm.launch_bottomup_masks([dict(info, regions=[np.array([5, 5], np.uint32)])], out, [0])
    with pytest.raises(ValueError):
        mp.bottomup_masks_batch([info, cases.mask_info("none", 40, 37, (12,))], DEV)  # radii differ inside a batch


# ---- per-stage planes into the augmentation
AUG_CFG = dict(image_size=[64, 48], max_image_size=[64, 48], heatmap_sizes=[[16, 12], [32, 24]], flip_pairs=[[1, 2], [3, 4]], pixel_std=200.0,
               tag_per_joint=True)


def test_stage_planes_equal_one_run_per_plane():
    rng = np.random.RandomState(11)
    shapes = [(53, 37), (61, 80), (64, 64), (33, 47)]
    images = [torch.from_numpy(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).to(DEV) for h, w in shapes]
    planes = [rng.randint(1, 256, (2, h, w)).astype(np.uint8) for h, w in shapes]  # the two planes of an image differ everywhere it matters
    keypoints = [np.concatenate([rng.uniform(0, w, (m, 5, 1)), rng.uniform(0, h, (m, 5, 1)), rng.randint(0, 3, (m, 5, 1))], axis=2).astype(np.float32)
                 for m, (h, w) in zip((2, 0, 3, 1), shapes)]
    affine, flip = mp.BottomUpRandomAffine(config=AUG_CFG), mp.BottomUpHorizontalRandomFlip(config=AUG_CFG, flip_prob=0.5)
    seed = 7

    def run(masks):
        np.random.seed(seed)
        out = mp.bottomup_augment_batch(affine, flip, images, masks, keypoints)
        return out, np.random.rand()

    staged, after = run([torch.from_numpy(p).to(DEV) for p in planes])
    assert tuple(staged["mask"].shape) == (4, 2, 24, 32)
    for stage in range(2):
        single, after_single = run([torch.from_numpy(np.ascontiguousarray(p[stage])).to(DEV) for p in planes])
        assert after_single == after
        assert torch.equal(staged["mask"][:, stage], single["mask"][:, stage]), stage
        assert torch.equal(staged["image"].view(torch.int32), single["image"].view(torch.int32))  # the image is today's, to the bit
        assert torch.equal(staged["keypoints"], single["keypoints"])
    assert not torch.equal(staged["mask"][:, 0], run([torch.from_numpy(np.ascontiguousarray(p[1])).to(DEV) for p in planes])[0]["mask"][:, 0])
    # both forms in one batch: an [H, W] mask is tiled over the stages as before
    mixed, _ = run([torch.from_numpy(planes[0]).to(DEV), torch.from_numpy(np.ascontiguousarray(planes[1][0])).to(DEV),
                    torch.from_numpy(planes[2]).to(DEV), torch.from_numpy(np.ascontiguousarray(planes[3][1])).to(DEV)])
    first, _ = run([torch.from_numpy(np.ascontiguousarray(p[0])).to(DEV) for p in planes])
    second, _ = run([torch.from_numpy(np.ascontiguousarray(p[1])).to(DEV) for p in planes])
    assert torch.equal(mixed["mask"][0], staged["mask"][0]) and torch.equal(mixed["mask"][2], staged["mask"][2])
    assert torch.equal(mixed["mask"][1], first["mask"][1]) and torch.equal(mixed["mask"][3], second["mask"][3])
    with pytest.raises(ValueError):  # three planes for two stages
        mp.bottomup_augment_batch(affine, flip, images[:1], [torch.ones(3, 53, 37, dtype=torch.uint8, device=DEV)], keypoints[:1])


def test_chain_record_masks_augment_targets_loss(tmp_path):
    """record -> bottomup_masks_batch -> bottomup_augment_batch -> generate_batch -> AEMultiLoss."""
    ds = mp.COCOBottomUpDataset(str(tmp_path), cases.write_records_json(tmp_path), is_train=False, num_joints=cases.K, config=cases.RECORD_CFG)
    records = [ds._load_coco_keypoint_annotations_per_img(i) for i in (5, 2)]
    masks = mp.bottomup_masks_batch([r["mask_info"] for r in records], DEV)
    for r, m in zip(records, masks):
        assert np.array_equal(m.cpu().numpy(), bm.decode_mask_info(r["mask_info"]))
    assert not masks[0].all() and masks[1].all()
    rng = np.random.RandomState(5)
    images = [torch.from_numpy(rng.randint(0, 256, tuple(m.shape[1:]) + (3,)).astype(np.uint8)).to(DEV) for m in masks]
    keypoints = [r["keypoints"][0].astype(np.float32) if r["keypoints"].ndim == 4 else np.zeros((0, cases.K, 3), np.float32) for r in records]
    affine, flip = mp.BottomUpRandomAffine(config=AUG_CFG), mp.BottomUpHorizontalRandomFlip(config=AUG_CFG, flip_prob=0.5)
    target_gen = mp.BottomUpGenerateTarget(config=AUG_CFG, sigma=2.0, max_num=4)
    np.random.seed(3)
    out = mp.bottomup_augment_batch(affine, flip, images, masks, keypoints)
    assert out["num_persons"].tolist() == [4, 0] and tuple(out["mask"].shape) == (2, 2, 24, 32)
    assert out["mask"][0].any() and not out["mask"][0, 1].all()  # part of the image is masked out, part is not
    target, tag_ind = target_gen.generate_batch(out["keypoints"], out["num_persons"])
    n, (w0, h0), (w1, h1) = 2, *AUG_CFG["heatmap_sizes"]
    g = torch.Generator().manual_seed(0)
    preds = [torch.randn(n, 2 * cases.K, h0, w0, generator=g).to(DEV), torch.randn(n, cases.K, h1, w1, generator=g).to(DEV)]
    loss_fn = mp.AEMultiLoss(num_joints=cases.K, num_stages=2, stage_sizes=[(w0, h0), (w1, h1)])
    loss = loss_fn(preds, target, out["mask"], tag_ind)
    plain = loss_fn(preds, target, torch.ones_like(out["mask"]), tag_ind)
    assert torch.isfinite(loss).all() and torch.isfinite(plain).all()
    assert not torch.equal(loss, plain) and float(loss[0]) < float(plain[0])  # the heat-map term sums fewer pixels
