"""Bottom-up flip TTA on the MI355X: ``decode_flip_aggregated`` against a torch-CPU restatement of the flip test's semantics
(bit-equal on dyadic inputs), the mirror identity against the plain ``decode``, and the inferencer end to end in fp32 and amp O2.

The oracle restates the intent of the reference's ``_MultiRunNet`` (engine/inferencer/bottomup_inferencer.py:252-297), whose own
``(heatmap + flipped_heatmap) * 0.5`` on Python lists cannot run: per stage, at stage resolution,
``heat_i = (A_i[:, :K] + B_i[:, f][..., ::-1]) * 0.5``; the tag list is the plain tags in stage order, then ``B_i[:, K + f][..., ::-1]``
in the same order; the reference's ``decode`` follows unchanged."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mindpose_amd as mp  # noqa: E402
from mindpose_amd.data.transform.utils import transform_keypoints  # noqa: E402
from mindpose_amd.engine.inferencer.bottomup_inferencer import refine_missing_joint  # noqa: E402
from mindpose_amd.utils.match import match_by_tag  # noqa: E402
from tests.test_gpu_bottomup import oracle_decode  # noqa: E402

DEV = torch.device("cuda:0")
K = 17
COCO_FLIP_PAIRS = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]
COCO_FLIP_INDEX = [0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15]
THREE_CYCLE = [0, 2, 1, 4, 3, 6, 7, 5, 8, 10, 9, 12, 11, 14, 13, 16, 15]  # 5 -> 6 -> 7 -> 5: f differs from its inverse
NAMES = ("val_k", "tag_k", "ind_k", "heatmap_raw", "tagging")


def oracle_flip_decode(outputs, flipped, flip_index, mask, with_ae, use_nms, nms_kernel, max_num, shift):
    """The five outputs of the flip test.  ``oracle_decode`` of [heat_i | plain tags] gives everything but the second half of the
    tag axis, ``oracle_decode`` of [heat_i | flipped-back tags] gives that half (same heat maps, hence the same peaks)."""
    f = torch.as_tensor(flip_index, dtype=torch.long)
    plain, back = [], []
    for a, b, ae in zip(outputs, flipped, with_ae):
        a, b = a.detach().cpu().float(), b.detach().cpu().float()
        heat = (a[:, :K] + b[:, f].flip(3)) * 0.5
        plain.append(torch.cat([heat, a[:, K:]], 1) if ae else heat)
        back.append(torch.cat([heat, b[:, K + f].flip(3)], 1) if ae else heat)
    args = (mask, len(outputs), with_ae, use_nms, nms_kernel, max_num, True, shift)
    val, tag_a, ind, raw, tagging_a = oracle_decode(plain, *args)
    val_b, tag_b, ind_b, raw_b, tagging_b = oracle_decode(back, *args)
    assert torch.equal(val, val_b) and torch.equal(ind, ind_b) and torch.equal(raw, raw_b)
    return val, torch.cat([tag_a, tag_b], -1), ind, raw, torch.cat([tagging_a, tagging_b], -1)


def _dyadic(shape, gen):
    return torch.randint(-1024, 1025, shape, generator=gen).float() / 1024.0


MAP = (48, 80)  # three tile rows; one full and one ragged 64-column tile
LAYOUTS = {
    # stage sizes (last = the map), with_ae_loss
    "one_stage": ([MAP], [True]),
    "lower_24x40": ([(24, 40), MAP], [True, False]),                 # a lower stage that divides the map
    "lower_20x33": ([(20, 33), MAP], [True, False]),                 # odd width, resize scales 20/48 and 33/80 round
    "lower_24x40_two_tag_stages": ([(24, 40), MAP], [True, True]),   # num_tags 4
    "lower_20x33_two_tag_stages": ([(20, 33), MAP], [True, True]),
}


def _stage_outputs(n, sizes, with_ae, gen, dyadic=True):
    shapes = [(n, K * (2 if ae else 1), h, w) for (h, w), ae in zip(sizes, with_ae)]
    return [_dyadic(s, gen) if dyadic else torch.randn(s, generator=gen) for s in shapes]


def _mask(n):
    """image-resolution mask (2x the map) that blanks a different right / bottom band per image"""
    h, w = 2 * MAP[0], 2 * MAP[1]
    m = torch.zeros(n, h, w, dtype=torch.bool)
    for i in range(n):
        m[i, : h - 10 - 14 * i, : w - 22 - 18 * i] = True
    return m


def _decoder(sizes, with_ae, nms_kernel, shift, max_num):
    return mp.create_decoder("bottomup_heatmap_ae", num_joints=K, num_stages=len(sizes), with_ae_loss=with_ae, use_nms=True,
                             nms_kernel=nms_kernel, max_num=max_num, shift_coordinate=shift)


def _check_bit_equal(layout, nms_kernel, shift, max_num, flip_index, seed):
    sizes, with_ae = LAYOUTS[layout]
    gen = torch.Generator().manual_seed(seed)
    a, b = _stage_outputs(2, sizes, with_ae, gen), _stage_outputs(2, sizes, with_ae, gen)
    mask = _mask(2)
    dec = _decoder(sizes, with_ae, nms_kernel, shift, max_num)
    got = dec.decode_flip_aggregated([t.to(DEV) for t in a], [t.to(DEV) for t in b], flip_index, mask.to(DEV))
    torch.cuda.synchronize()
    ref = oracle_flip_decode(a, b, flip_index, mask, with_ae, True, nms_kernel, max_num, shift)
    num_tags = 2 * sum(with_ae)
    assert tuple(ref[4].shape) == (2, K, *MAP, num_tags) and tuple(ref[1].shape) == (2, K, max_num, num_tags)
    for name, g, r in zip(NAMES, got, ref):
        assert g.dtype == torch.float32 and g.is_cuda
        assert tuple(g.shape) == tuple(r.shape), name
        assert torch.equal(g.cpu(), r), f"{name} differs"


@pytest.mark.parametrize("max_num", [1, 30, 64])
@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("nms_kernel", [3, 5])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_flip_decode_bit_equal_on_dyadic_inputs(layout, nms_kernel, shift, max_num):
    """Dyadic inputs: the mean (a + b) * 0.5 and, where the lower stage divides the map, every lerp product are exact; where it
    does not, the kernel restates the oracle's fp32 expressions operation by operation (fp contraction off), so all five outputs
    are bit-equal either way."""
    _check_bit_equal(layout, nms_kernel, shift, max_num, COCO_FLIP_INDEX, seed=11 + 7 * max_num + nms_kernel + len(layout))


@pytest.mark.parametrize("layout", ["lower_20x33", "lower_24x40_two_tag_stages"])
def test_flip_decode_with_a_three_cycle_permutation(layout):
    """A flip index that is no involution: joint k must read channel f[k] of the mirrored run, not f^-1[k]."""
    assert [THREE_CYCLE[i] for i in THREE_CYCLE] != list(range(K))
    _check_bit_equal(layout, 3, True, 30, THREE_CYCLE, seed=5)


@pytest.mark.parametrize("layout", ["one_stage", "lower_20x33", "lower_24x40_two_tag_stages"])
def test_flip_decode_of_a_mirrored_copy_is_the_plain_decode(layout):
    """B_i[n, f[c], y, Ws - 1 - x] := A_i[n, c, y, x] for heat and tag channels alike, on random-normal inputs: (a + a) * 0.5 is
    exact in fp32, so the flip decode of (A, B) is the existing plain decode of A bit for bit, and both halves of the tag axis are
    the plain tags."""
    sizes, with_ae = LAYOUTS[layout]
    gen = torch.Generator().manual_seed(31)
    a = [t.to(DEV) for t in _stage_outputs(2, sizes, with_ae, gen, dyadic=False)]
    f = torch.tensor(COCO_FLIP_INDEX)
    b = []
    for t, ae in zip(a, with_ae):
        channels = torch.cat([f, K + f]) if ae else f
        m = torch.empty_like(t)
        m[:, channels.to(DEV)] = t.flip(3)
        b.append(m)
    mask = _mask(2).to(DEV)
    dec = _decoder(sizes, with_ae, 3, True, 30)
    val, tag, ind, raw, tagging = (t.cpu() for t in dec.decode_flip_aggregated(a, b, COCO_FLIP_INDEX, mask))
    pval, ptag, pind, praw, ptagging = (t.cpu() for t in dec(a, mask))
    num = sum(with_ae)
    assert torch.equal(val, pval) and torch.equal(ind, pind) and torch.equal(raw, praw)
    assert torch.equal(tag[..., :num], ptag) and torch.equal(tag[..., num:], ptag)
    assert torch.equal(tagging[..., :num], ptagging) and torch.equal(tagging[..., num:], ptagging)


# ---- the inferencer -----------------------------------------------------------------------------------------------------------------
JOINT_ORDER = [0, 1, 2, 3, 4, 5, 6, 11, 12, 7, 8, 9, 10, 13, 14, 15, 16]
CFG = dict(has_heatmap_output=True, hflip_tta=True, joint_order=JOINT_ORDER, vis_thr=0.1, ignore_too_much=False, use_rounded_norm=True,
           tag_thr=1.0, pixel_std=200.0, downsample_scale=2, refine_missing_joint=True, flip_pairs=COCO_FLIP_PAIRS)
H, W = 256, 192  # the backbone's own top-down size; H != W: a mirror along the wrong axis cannot pass


def _net(amp_level="O0"):
    net = mp.init_synthetic(mp.create_network("hrnet_w32", "higher_hrnet_head"), seed=0).to(DEV).eval()
    if amp_level != "O0":
        mp.models.auto_mixed_precision(net, amp_level)
    return net


def _batch(seed):
    x = torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(seed))
    mask = torch.ones(1, H, W, dtype=torch.bool)
    mask[:, :, W - 40:] = False  # a blank right band: the mask is NOT mirrored for the second run
    return dict(image=x.to(DEV), mask=mask.to(DEV), center=np.array([[W / 2, H / 2]], np.float32),
                scale=np.array([[W / 200.0, H / 200.0]], np.float32), image_shape=np.array([[H, W]], np.float32),
                image_file=np.array(["a.jpg"]))


def test_inferencer_flip_tta_end_to_end_fp32(monkeypatch):
    monkeypatch.setenv("MINDPOSE_AUTOTUNE", "0")  # the library's own choice of kernel per layer: no candidate timing in this test
    net = _net()
    dec = mp.create_decoder("bottomup_heatmap_ae", use_nms=True, nms_kernel=3, max_num=30)
    inf = mp.create_inferencer(mp.create_eval_network(net, dec), "bottomup_heatmap_ae", config=CFG, decoder=dec)
    batch = _batch(13)
    records = inf.infer([batch])
    assert len(records) == 1 and records[0]["image_path"] == "a.jpg"

    plain = [o.clone() for o in net(batch["image"])]
    flipped = net(batch["image"], flip_width=True)
    assert tuple(plain[0].shape) == (1, 2 * K, H // 4, W // 4) and tuple(plain[1].shape) == (1, K, H // 2, W // 2)
    ref = oracle_flip_decode(plain, flipped, COCO_FLIP_INDEX, batch["mask"].cpu(), [True, False], True, 3, 30, False)
    assert ref[1].shape[-1] == 2
    people = match_by_tag(ref[0][0].numpy(), ref[1][0].numpy(), ref[2][0].numpy(), JOINT_ORDER, 0.1, 1.0, False, True)
    scores = [p[:, 2].mean() for p in people]
    for j in range(len(people)):
        people[j] = refine_missing_joint(ref[3][0].numpy(), ref[4][0].numpy(), people[j])
    expect = transform_keypoints([people], batch["center"], batch["scale"], batch["image_shape"] / 2, pixel_std=200.0)[0]
    assert len(people) > 0  # the synthetic network's maps do group into persons: the comparison is not of empty lists
    assert np.array_equal(records[0]["pred"], expect)
    assert records[0]["score"] == scores


def test_inferencer_flip_tta_amp_o2_batched_equals_two_forwards(monkeypatch):
    """amp O2: one 2N forward of [image | mirror] (MINDPOSE_FLIP_BATCHED on, the default) gives the records of the two N forwards;
    the fp16 kernels give the same bits whatever the batch."""
    net = _net("O2")
    dec = mp.create_decoder("bottomup_heatmap_ae", use_nms=True, nms_kernel=3, max_num=30)
    inf = mp.create_inferencer(mp.create_eval_network(net, dec), "bottomup_heatmap_ae", config=CFG, decoder=dec)
    batch = _batch(14)
    monkeypatch.setenv("MINDPOSE_FLIP_BATCHED", "0")
    two = inf.infer([batch])
    assert not any(key[0][0] == 2 for key in net._plans)
    monkeypatch.setenv("MINDPOSE_FLIP_BATCHED", "1")
    one = inf.infer([batch])
    assert any(key[0] == (2, 3, H, W) for key in net._plans)  # the batched run recorded a 2N plan
    assert len(one) == len(two) == 1
    assert np.array_equal(one[0]["pred"], two[0]["pred"]) and one[0]["score"] == two[0]["score"]
