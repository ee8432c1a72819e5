"""Bottom-up (HigherHRNet, associative embedding) inference on the MI355X: decoder kernels against a torch-CPU restatement of the
reference's decode (bit-equal on dyadic inputs), the HigherHRNet network plan against oracle/nets.py plus a restatement of the
head, and the inferencer end to end."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import mindpose_amd as mp  # noqa: E402
from mindpose_amd.data.transform.utils import transform_keypoints  # noqa: E402
from mindpose_amd.utils.match import match_by_tag  # noqa: E402
from oracle import nets as onets  # noqa: E402

DEV = torch.device("cuda:0")
K = 17


# ---- torch-CPU restatement of bottom_up_decoder.py ------------------------------------------------------------------------------
def _resize_bilinear(x, oh, ow):
    """ops.ResizeBilinear((oh, ow)), align_corners=False, half_pixel_centers=False: src = dst * in / out (gathers, no
    F.interpolate, whose align_corners=False form uses half-pixel centres)."""
    h, w = x.shape[2], x.shape[3]
    fy = torch.arange(oh, dtype=torch.float32) * torch.tensor(np.float32(h) / np.float32(oh))
    fx = torch.arange(ow, dtype=torch.float32) * torch.tensor(np.float32(w) / np.float32(ow))
    y0, x0 = fy.floor().long().clamp(max=h - 1), fx.floor().long().clamp(max=w - 1)
    y1, x1 = (y0 + 1).clamp(max=h - 1), (x0 + 1).clamp(max=w - 1)
    dy, dx = (fy - y0.float())[:, None], fx - x0.float()
    a, b = x[:, :, y0][:, :, :, x0], x[:, :, y0][:, :, :, x1]
    c, d = x[:, :, y1][:, :, :, x0], x[:, :, y1][:, :, :, x1]
    top = a + (b - a) * dx
    bot = c + (d - c) * dx
    return top + (bot - top) * dy


def _resize_nearest(m, oh, ow):
    h, w = m.shape[1], m.shape[2]
    ys = (torch.arange(oh, dtype=torch.float32) * torch.tensor(np.float32(h) / np.float32(oh))).floor().long().clamp(max=h - 1)
    xs = (torch.arange(ow, dtype=torch.float32) * torch.tensor(np.float32(w) / np.float32(ow))).floor().long().clamp(max=w - 1)
    return m[:, ys][:, :, xs]


def oracle_decode(outputs, mask, num_stages, with_ae_loss, use_nms, nms_kernel, max_num, tag_per_joint, shift_coordinate):
    outputs = [o.detach().cpu().float() for o in outputs]
    heat = [outputs[i][:, :K] for i in range(num_stages)]
    tags = [outputs[i][:, K:] for i in range(num_stages) if with_ae_loss[i]]
    base = heat[-1].clone()
    n, _, h, w = base.shape
    for i in range(num_stages - 1):
        base = base + _resize_bilinear(heat[i], h, w)
    if num_stages > 1:
        base = base / num_stages
    tagging = torch.stack([_resize_bilinear(t, h, w) for t in tags], dim=-1)
    keep = _resize_nearest(mask.cpu().bool(), h, w)[:, None]
    raw = base.masked_fill(~keep, 0)
    hm = raw
    if use_nms:
        pooled = F.max_pool2d(raw, nms_kernel, 1, nms_kernel // 2)
        hm = torch.where(pooled == raw, raw, torch.zeros_like(raw))
    flat = hm.reshape(n, K, -1)
    val, ind = torch.sort(flat, dim=2, descending=True, stable=True)  # ops.top_k order: ties in ascending index
    val, ind = val[..., :max_num], ind[..., :max_num]
    tg = tagging.reshape(tagging.shape[0], tagging.shape[1], h * w, -1)
    if not tag_per_joint:
        tg = tg.expand(-1, K, -1, -1)
    tag_k = torch.stack([torch.gather(tg[..., l], 2, ind) for l in range(tg.shape[3])], dim=3)
    ind_k = torch.stack((ind % w, ind // w), dim=3).float()
    if shift_coordinate:
        dxm, dym = torch.zeros_like(raw), torch.zeros_like(raw)
        dxm[:, :, :, 1:-1] = raw[:, :, :, 2:] - raw[:, :, :, :-2]
        dym[:, :, 1:-1, :] = raw[:, :, 2:, :] - raw[:, :, :-2, :]
        by_index = ind.sort(dim=2).values  # masked_select: the selected pixels in flat-index order
        ox = torch.gather(torch.sign(dxm).reshape(n, K, -1), 2, by_index) * 0.25
        oy = torch.gather(torch.sign(dym).reshape(n, K, -1), 2, by_index) * 0.25
        ind_k[..., 0] += ox
        ind_k[..., 1] += oy
    return val, tag_k, ind_k, raw, tagging


def _dyadic(shape, gen):
    return torch.randint(-1024, 1025, shape, generator=gen).float() / 1024.0


def _outputs(n, size, with_ae_loss, tag_per_joint, num_stages, gen, dyadic=True):
    h, w = size
    ktag = K if tag_per_joint else 1
    outs = []
    for i in range(num_stages):
        s = 2 ** (num_stages - 1 - i)
        c = K + (ktag if with_ae_loss[i] else 0)
        shape = (n, c, h // s, w // s)
        outs.append(_dyadic(shape, gen) if dyadic else torch.randn(shape, generator=gen))
    return outs


def _mask(n, size, gen):
    """image-resolution mask (2x the map) with a zero padding region on the right / bottom, different per image"""
    h, w = 2 * size[0], 2 * size[1]
    m = torch.zeros(n, h, w, dtype=torch.bool)
    for i in range(n):
        m[i, : h - 24 * i, : w - 40 - 16 * i] = True
    return m


CASES = [
    # n, map size, num_stages, use_nms, nms_kernel, tag_per_joint, shift, max_num
    (1, (256, 416), 2, True, 3, True, False, 30),
    (3, (256, 256), 2, True, 5, True, True, 30),
    (1, (256, 256), 1, False, 5, True, True, 64),
    (3, (256, 416), 2, False, 3, False, True, 1),
    (1, (256, 256), 2, True, 3, False, False, 64),
    (3, (256, 256), 1, True, 3, True, False, 30),
    (1, (256, 416), 2, True, 5, True, True, 64),
]


@pytest.mark.parametrize("n,size,num_stages,use_nms,nms_kernel,tag_per_joint,shift,max_num", CASES)
def test_decoder_bit_equal_on_dyadic_inputs(n, size, num_stages, use_nms, nms_kernel, tag_per_joint, shift, max_num):
    gen = torch.Generator().manual_seed(7 + n + size[1] + max_num)
    with_ae = [True, False] if num_stages == 2 else [True]
    outs = _outputs(n, size, with_ae, tag_per_joint, num_stages, gen)
    # dyadic values repeat, so equal values among the selected peaks exercise the (value desc, index asc) key order; the case
    # where fewer than max_num peaks survive is test_decoder_zero_tail_in_flat_index_order
    mask = _mask(n, size, gen)
    dec = mp.create_decoder("bottomup_heatmap_ae", num_joints=K, num_stages=num_stages, with_ae_loss=with_ae, use_nms=use_nms,
                            nms_kernel=nms_kernel, max_num=max_num, tag_per_joint=tag_per_joint, shift_coordinate=shift)
    got = dec([o.to(DEV) for o in outs], mask.to(DEV))
    torch.cuda.synchronize()
    ref = oracle_decode(outs, mask, num_stages, with_ae, use_nms, nms_kernel, max_num, tag_per_joint, shift)
    names = ("val_k", "tag_k", "ind_k", "heatmap_raw", "tagging")
    for name, g, r in zip(names, got, ref):
        assert g.dtype == torch.float32 and g.is_cuda
        assert tuple(g.shape) == tuple(r.shape), name
        assert torch.equal(g.cpu(), r), f"{name} differs"


@pytest.mark.parametrize("num_stages,shift", [(1, False), (2, True)])
def test_decoder_zero_tail_in_flat_index_order(num_stages, shift):
    """Fewer than max_num positive peaks: the tail of the top-k is the zeros (NMS-suppressed and masked pixels, -0.0 included),
    which ops.top_k returns in ascending flat index."""
    gen = torch.Generator().manual_seed(5)
    size = (256, 416)
    with_ae = [True, False] if num_stages == 2 else [True]
    outs = [-o.abs() for o in _outputs(2, size, with_ae, True, num_stages, gen)]
    for j in range(7):  # a handful of isolated positive peaks per joint
        outs[-1][:, :K, 20 + 30 * j, 15 + 50 * j] = 0.25 * (j + 1)
    mask = _mask(2, size, gen)
    dec = mp.create_decoder("bottomup_heatmap_ae", num_stages=num_stages, with_ae_loss=with_ae, use_nms=True, nms_kernel=3,
                            max_num=30, shift_coordinate=shift)
    got = [t.cpu() for t in dec([o.to(DEV) for o in outs], mask.to(DEV))]
    ref = oracle_decode(outs, mask, num_stages, with_ae, True, 3, 30, True, shift)
    assert (ref[0][..., -1] == 0).all() and (ref[0][..., 0] > 0).all()  # the tail really is zeros
    for g, r in zip(got, ref):
        assert torch.equal(g, r)


def test_decoder_shift_takes_offsets_in_flat_index_order():
    """The reference quirk: value-order entry m gets the offset of the m-th smallest selected flat index."""
    h = w = 16
    out = torch.zeros(1, 2 * K, h, w)
    out[0, :K, 5, 9] = 1.0    # highest value, larger flat index; neighbours make its own offset (+x)
    out[0, :K, 5, 10] = 0.5
    out[0, :K, 2, 3] = 0.75   # second value, smaller flat index; its own offset would be (-x)
    out[0, :K, 2, 2] = 0.25
    mask = torch.ones(1, h, w, dtype=torch.bool)
    dec = mp.create_decoder("bottomup_heatmap_ae", num_stages=1, with_ae_loss=[True], use_nms=True, nms_kernel=3, max_num=2,
                            shift_coordinate=True)
    _, _, ind_k, _, _ = dec([out.to(DEV)], mask.to(DEV))
    ref = oracle_decode([out], mask, 1, [True], True, 3, 2, True, True)[2]
    assert torch.equal(ind_k.cpu(), ref)
    # entry 0 is pixel (9, 5) (own offset +x) but carries the offset of pixel (3, 2), the smaller flat index: left 0.25, right 0 -> -x
    assert ind_k[0, 0, 0].tolist() == [9.0 - 0.25, 5.0]


def test_decoder_random_inputs():
    gen = torch.Generator().manual_seed(3)
    size = (256, 416)
    outs = _outputs(2, size, [True, False], True, 2, gen, dyadic=False)
    mask = _mask(2, size, gen)
    dec = mp.create_decoder("bottomup_heatmap_ae", use_nms=True, nms_kernel=3, max_num=30)
    val, tag, ind, raw, tagging = (t.cpu() for t in dec([o.to(DEV) for o in outs], mask.to(DEV)))
    rv, rt, ri, rraw, rtagging = oracle_decode(outs, mask, 2, [True, False], True, 3, 30, True, False)
    tol = 1e-6
    assert torch.allclose(raw, rraw, rtol=tol, atol=tol * rraw.abs().max())
    assert torch.allclose(tagging, rtagging, rtol=tol, atol=tol * rtagging.abs().max())
    assert torch.allclose(val, rv, rtol=tol, atol=tol * rv.abs().max())
    gap = (rv[..., :-1] - rv[..., 1:]).abs() > 2 * tol * rv.abs().max()
    safe = torch.cat([gap[..., :1], gap[..., 1:] & gap[..., :-1], gap[..., -1:]], dim=-1)
    assert safe.float().mean() > 0.5
    assert torch.equal(ind[safe], ri[safe])
    assert torch.allclose(tag[safe], rt[safe], rtol=tol, atol=tol * rt.abs().max())


def test_decoder_refuses_max_num_above_64():
    with pytest.raises(ValueError):
        mp.create_decoder("bottomup_heatmap_ae", max_num=65)


# ---- the decoder's edges: ragged tiles, stage layouts, tag stages, NMS sizes, top-k limits, mask ratios ------------------------------
def _sized_outputs(n, sizes, with_ae, tag_per_joint, gen):
    ktag = K if tag_per_joint else 1
    return [_dyadic((n, K + (ktag if ae else 0), h, w), gen) for (h, w), ae in zip(sizes, with_ae)]


def _ratio_mask(n, size, gen, blank=None):
    """mask of any size with a per-image zero border on the right / bottom; image ``blank`` all false"""
    h, w = size
    m = torch.zeros(n, h, w, dtype=torch.bool)
    for i in range(n):
        m[i, : h - (h // 8) * (i % 3), : w - w // 6 - (w // 10) * (i % 2)] = True
    if blank is not None:
        m[blank] = False
    return m


EDGE_CASES = {
    # n, stage sizes (last = the map), with_ae_loss, nms_kernel, tag_per_joint, shift, max_num, mask size, all-false image
    "40x24_ragged_tile_rows": (2, [(20, 12), (40, 24)], [True, False], 3, True, True, 30, (80, 48), None),
    "50x70_two_tile_columns": (1, [(25, 35), (50, 70)], [True, False], 5, True, False, 30, (50, 70), None),   # mask at 1x
    "416x256_transposed": (1, [(208, 128), (416, 256)], [True, False], 3, True, True, 30, (832, 512), None),
    "three_stages_4_2_1": (2, [(10, 6), (20, 12), (40, 24)], [True, False, False], 3, True, True, 20, (120, 72), None),  # mask at 3x
    "two_tag_stages_nms7": (2, [(20, 12), (40, 24)], [True, True], 7, True, True, 30, (80, 48), None),
    "two_tag_stages_one_tag_map_no_nms": (2, [(25, 35), (50, 70)], [True, True], 1, False, True, 30, (100, 140), None),
    "mask_ratio_2p5_by_2p375_blank_image": (3, [(20, 12), (40, 24)], [True, False], 3, True, False, 30, (100, 57), 1),
    "n_times_k_204": (12, [(20, 12), (40, 24)], [True, False], 5, True, True, 30, (80, 48), 7),
}


@pytest.mark.parametrize("name", list(EDGE_CASES))
def test_decoder_edges_bit_equal_on_dyadic_inputs(name):
    """Map heights that are not a multiple of the 16-row tile, widths below and just above the 64-column tile, the transposed
    recipe shape, three stages, two tag-carrying stages (num_tags = 2), NMS windows 1 and 7, masks at 1x / 3x / a non-integer
    ratio of the map, an all-false mask for one image, a few hundred (image, joint) workgroups.  Every resize scale here is a
    power of two, so the lerp products are exact and the outputs are bit-equal to the CPU restatement."""
    n, sizes, with_ae, nms_kernel, tag_per_joint, shift, max_num, mask_size, blank = EDGE_CASES[name]
    gen = torch.Generator().manual_seed(len(name) + n)
    outs = _sized_outputs(n, sizes, with_ae, tag_per_joint, gen)
    mask = _ratio_mask(n, mask_size, gen, blank)
    dec = mp.create_decoder("bottomup_heatmap_ae", num_joints=K, num_stages=len(sizes), with_ae_loss=with_ae, use_nms=True,
                            nms_kernel=nms_kernel, max_num=max_num, tag_per_joint=tag_per_joint, shift_coordinate=shift)
    got = dec([o.to(DEV) for o in outs], mask.to(DEV))
    torch.cuda.synchronize()
    ref = oracle_decode(outs, mask, len(sizes), with_ae, True, nms_kernel, max_num, tag_per_joint, shift)
    assert ref[4].shape[-1] == sum(with_ae) and ref[1].shape[-1] == sum(with_ae)
    if blank is not None:
        assert (ref[3][blank] == 0).all() and (ref[0][blank] == 0).all()  # the blank image really decodes to zeros
        assert torch.equal(ref[2][blank, :, :, 0] + ref[2][blank, :, :, 1] * sizes[-1][1],
                           torch.arange(max_num).float().expand(K, -1))    # ... returned in flat-index order
    for nm, g, r in zip(("val_k", "tag_k", "ind_k", "heatmap_raw", "tagging"), got, ref):
        assert tuple(g.shape) == tuple(r.shape), nm
        assert torch.equal(g.cpu(), r), f"{nm} differs"


def test_decoder_lower_stage_that_does_not_divide_the_map():
    """A 13 x 11 stage under a 40 x 24 map: the resize scales 13/40 and 11/24 are not dyadic, so the source coordinates and the
    lerp products round.  The kernel is built with fp contraction off and restates the oracle's fp32 expressions operation by
    operation, so every rounding is the same and bit equality holds here too."""
    gen = torch.Generator().manual_seed(21)
    sizes, with_ae = [(13, 11), (40, 24)], [True, False]
    outs = _sized_outputs(2, sizes, with_ae, True, gen)
    mask = _ratio_mask(2, (80, 48), gen)
    dec = mp.create_decoder("bottomup_heatmap_ae", use_nms=True, nms_kernel=3, max_num=30)
    got = [t.cpu() for t in dec([o.to(DEV) for o in outs], mask.to(DEV))]
    ref = oracle_decode(outs, mask, 2, with_ae, True, 3, 30, True, False)
    frac = ref[3] * 1024.0
    assert (frac != frac.round()).any()  # the resized term really left the dyadic grid of the inputs
    for nm, g, r in zip(("val_k", "tag_k", "ind_k", "heatmap_raw", "tagging"), got, ref):
        assert torch.equal(g, r), f"{nm} differs"


@pytest.mark.parametrize("shift", [False, True])
def test_decoder_returns_every_pixel_when_max_num_is_the_map(shift):
    """max_num == h * w on an 8 x 8 map: every pixel comes back - the NMS survivors in value order, then the zeros (suppressed and
    masked pixels) in ascending flat index."""
    gen = torch.Generator().manual_seed(9)
    outs = _sized_outputs(2, [(8, 8)], [True], True, gen)
    mask = _ratio_mask(2, (16, 16), gen)
    dec = mp.create_decoder("bottomup_heatmap_ae", num_stages=1, with_ae_loss=[True], use_nms=True, nms_kernel=3, max_num=64,
                            shift_coordinate=shift)
    got = [t.cpu() for t in dec([o.to(DEV) for o in outs], mask.to(DEV))]
    ref = oracle_decode(outs, mask, 1, [True], True, 3, 64, True, shift)
    assert (ref[0][..., -1] <= 0).all() and (ref[0][..., 0] > 0).all() and (ref[0] == 0).any()  # a real mix of peaks and zeros
    if not shift:
        idx = (ref[2][..., 0] + ref[2][..., 1] * 8).long()
        assert torch.equal(idx.sort(dim=2).values, torch.arange(64).expand(2, K, -1))           # every pixel exactly once
    for g, r in zip(got, ref):
        assert torch.equal(g, r)


def test_decoder_multi_pass_merge_with_a_zero_tail():
    """112 tiles x max_num 64 = 7168 keys per (image, joint): the merge runs over two chunks of 4096, and with only seven positive
    peaks the global top-64 is completed by zeros from the FIRST tiles, in flat-index order."""
    gen = torch.Generator().manual_seed(6)
    size = (256, 416)
    assert (size[0] // 16) * -(-size[1] // 64) * 64 > 4096
    outs = [-o.abs() for o in _outputs(2, size, [True, False], True, 2, gen)]
    for j in range(7):
        outs[-1][:, :K, 250 - 30 * j, 400 - 50 * j] = 2.0 * (j + 1)   # above the lower stage's term; the last tiles: past the first chunk
    mask = _mask(2, size, gen)
    mask[:, 400:, :] = True
    mask[:, :, 700:] = True
    dec = mp.create_decoder("bottomup_heatmap_ae", use_nms=True, nms_kernel=3, max_num=64, shift_coordinate=True)
    got = [t.cpu() for t in dec([o.to(DEV) for o in outs], mask.to(DEV))]
    ref = oracle_decode(outs, mask, 2, [True, False], True, 3, 64, True, True)
    assert (ref[0][..., 7:] == 0).all() and (ref[0][..., :7] > 0).all()  # seven peaks, then the tail really is zeros
    for g, r in zip(got, ref):
        assert torch.equal(g, r)


def test_decoder_error_paths_through_the_c_abi():
    from mindpose_amd import _lib
    lib = _lib.load()
    n, h, w, m = 1, 16, 16, 8
    stage = torch.zeros(n, 2 * K, h, w, device=DEV)
    mask = torch.ones(n, h, w, dtype=torch.uint8, device=DEV)
    raw, tagging = torch.empty(n, K, h, w, device=DEV), torch.empty(n, K, h, w, 4, device=DEV)
    ws_bytes = lib.mp_bottomup_workspace_bytes(n, K, h, w, m)
    assert ws_bytes == n * K * 1 * m * 8
    ws = torch.empty(ws_bytes // 8 + 64, device=DEV, dtype=torch.int64)
    val, ind, tag = torch.empty(n, K, 64, device=DEV), torch.empty(n, K, 64, 2, device=DEV), torch.empty(n, K, 64, 4, device=DEV)

    def parse(stages=1, nms=3, max_num=m, bytes_=ws_bytes, ws_ptr=True):
        descs = (_lib.BottomUpStage * stages)(*[_lib.BottomUpStage(data=stage.data_ptr(), c=2 * K, h=h, w=w, has_tags=1)] * stages)
        return lib.mp_bottomup_parse_nms_topk(descs, stages, _lib.ptr(mask), h, w, n, K, 1, nms, max_num, _lib.ptr(raw), _lib.ptr(tagging),
                                              _lib.ptr(ws) if ws_ptr else None, bytes_, _lib.stream())

    def gather(max_num=m, bytes_=ws_bytes, num_tags=1, hh=h, ww=w):
        return lib.mp_bottomup_gather(_lib.ptr(raw), _lib.ptr(tagging), _lib.ptr(ws), bytes_, n, K, hh, ww, 1, num_tags, max_num, 0,
                                      _lib.ptr(val), _lib.ptr(ind), _lib.ptr(tag), _lib.stream())

    assert parse() == 0 and gather() == 0
    assert parse(bytes_=ws_bytes - 8) == -5 and gather(bytes_=ws_bytes - 8) == -5   # MP_ERR_WORKSPACE: too small
    assert parse(ws_ptr=False) == -5                                                 # ... or missing
    assert parse(nms=9) == -3 and parse(nms=2) == -3 and parse(nms=0) == -3          # MP_ERR_UNSUPPORTED
    assert parse(max_num=65, bytes_=ws_bytes * 16) == -3 and parse(max_num=0) == -3
    assert gather(max_num=65, bytes_=ws_bytes * 16) == -3
    assert gather(max_num=5, hh=2, ww=2) == -2                                       # max_num > h * w: MP_ERR_SHAPE
    assert parse(stages=5) == -2                                                     # more stages than the kernel carries
    assert parse(stages=4) == 0                                                      # four tag stages are the limit ...
    assert gather(num_tags=5) == -3                                                  # ... five are refused
    torch.cuda.synchronize()


# ---- network ---------------------------------------------------------------------------------------------------------------------
def _head_forward(params, x, amp=False):
    """higher_hrnet_head.py:217-229 restated: final_layers[0], concat, Conv2dTranspose(4, 2, 1) + BN + ReLU, 4 BasicBlocks,
    final_layers[1]; ``amp``: the op-by-op fp16 emulation of oracle/nets.py."""
    p = onets._P(params, "head.", False, amp)
    y0 = onets._conv(p.sub("final_layers.0"), x)
    cat = torch.cat([x, y0], 1)
    dp = p.sub("deconv_layers.0.0.0")
    z = onets._r(p, F.conv_transpose2d(cat, onets._r(p, dp["weight"]), stride=2, padding=1))
    z = F.relu(onets._bn(p.sub("deconv_layers.0.0.1"), z))
    for b in range(1, 5):
        z = onets._basic_block(p.sub(f"deconv_layers.0.{b}"), z)
    return [y0, onets._conv(p.sub("final_layers.1"), z)]


def _net_forward(params, x, amp=False):
    return _head_forward(params, onets.hrnet_forward(params, x, "hrnet_w32", prefix="backbone.", amp=amp), amp=amp)


def _check(got, ref, tol):
    err = float((got - ref).abs().max() / ref.abs().max())
    assert err < tol, f"normalised max error {err}"
    n, c = got.shape[:2]
    rf = ref.reshape(n, c, -1)
    top2 = rf.topk(2, dim=2).values
    safe = (top2[..., 0] - top2[..., 1]) > 2.0 * tol * ref.abs().max()
    assert safe.float().mean() > 0.5
    assert torch.equal(got.reshape(n, c, -1).argmax(2)[safe], rf.argmax(2)[safe])
    return err


def _net(amp_level="O0"):
    net = mp.init_synthetic(mp.create_network("hrnet_w32", "higher_hrnet_head"), seed=0).to(DEV).eval()
    if amp_level != "O0":
        mp.models.auto_mixed_precision(net, amp_level)
    return net


# the eval sizes of the bottom-up recipe (configs/higher_hrnet/higher_hrnet_w32_ascend.yaml: 512 x 512, up to 832 x 512)
# ... and an in-between size whose column bands are ragged (176 / 352 / 704-column layers)
@pytest.mark.parametrize("n,h,w", [(2, 512, 512), (1, 512, 832), (1, 576, 704)])
def test_higher_hrnet_fp32_vs_oracle(n, h, w):
    net = _net()
    x = torch.randn(n, 3, h, w, generator=torch.Generator().manual_seed(11))
    got = net(x.to(DEV))
    assert isinstance(got, list) and len(got) == 2
    assert tuple(got[0].shape) == (n, 2 * K, h // 4, w // 4) and tuple(got[1].shape) == (n, K, h // 2, w // 2)
    got = [g.cpu() for g in got]
    kinds = {e["kind"] for e in net.get_plan((n, 3, h, w), DEV).layer_info}
    assert "concat" in kinds and "col_slice" in kinds  # the wide layers ran as output-column bands
    ref = _net_forward({k: v.cpu() for k, v in net.state_dict().items()}, x)
    for g, r in zip(got, ref):
        _check(g, r, 1e-3)


@pytest.mark.parametrize("n,h,w", [(1, 512, 512), (1, 512, 832), (1, 576, 704)])
def test_higher_hrnet_amp_o2_vs_amp_oracle(n, h, w):
    net = _net("O2")
    x = torch.randn(n, 3, h, w, generator=torch.Generator().manual_seed(12))
    got = [g.cpu() for g in net(x.to(DEV))]
    kinds = [e["kind"] for e in net.get_plan((n, 3, h, w), DEV).layer_info]
    assert "conv" not in kinds and "deconv_phase" not in kinds  # the whole network, head included, on the fp16 kernels
    params = {k: v.cpu() for k, v in net.state_dict().items()}
    ref32, ref16 = _net_forward(params, x), _net_forward(params, x, amp=True)
    for g, r32, r16 in zip(got, ref32, ref16):
        e_hip = float((g - r32).abs().max() / r32.abs().max())
        e_emul = float((r16 - r32).abs().max() / r32.abs().max())
        assert e_hip <= 1.5 * e_emul + 1e-3, f"HIP fp16 {e_hip} vs op-by-op amp-O2 emulation {e_emul}"


def test_end_to_end_eval_network_and_inferencer():
    net = _net()
    dec = mp.create_decoder("bottomup_heatmap_ae", use_nms=True, nms_kernel=3, max_num=30)
    eval_net = mp.create_eval_network(net, dec)
    x = torch.randn(1, 3, 512, 512, generator=torch.Generator().manual_seed(13))
    mask = torch.ones(1, 512, 512, dtype=torch.bool)
    mask[:, :, 448:] = False
    (val_k, tag_k, ind_k, raw, tagging), outputs = eval_net(x.to(DEV), mask.to(DEV))
    ref = oracle_decode([o.cpu() for o in outputs], mask, 2, [True, False], True, 3, 30, True, False)
    for g, r in zip((val_k, tag_k, ind_k, raw, tagging), ref):
        assert torch.equal(g.cpu(), r)  # the same fp32 operations in the same order: bit-equal on the network's own outputs

    cfg = dict(has_heatmap_output=True, hflip_tta=False, joint_order=[0, 1, 2, 3, 4, 5, 6, 11, 12, 7, 8, 9, 10, 13, 14, 15, 16],
               vis_thr=0.1, ignore_too_much=False, use_rounded_norm=True, tag_thr=1.0, pixel_std=200.0, downsample_scale=2,
               refine_missing_joint=False, flip_pairs=[[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]])
    inf = mp.create_inferencer(eval_net, "bottomup_heatmap_ae", config=cfg)
    center, scale = np.array([[256.0, 256.0]], np.float32), np.array([[2.56, 2.56]], np.float32)
    image_shape = np.array([[512, 512]], np.float32)
    records = inf.infer([dict(image=x.to(DEV), mask=mask.to(DEV), center=center, scale=scale, image_shape=image_shape,
                              image_file=np.array(["a.jpg"]))])
    assert len(records) == 1 and records[0]["image_path"] == "a.jpg"
    # the same grouping and back-projection on the oracle's decoded arrays
    people = match_by_tag(ref[0][0].numpy(), ref[1][0].numpy(), ref[2][0].numpy(), cfg["joint_order"], 0.1, 1.0, False, True)
    expect = transform_keypoints([people], center, scale, image_shape / 2, pixel_std=200.0)[0]
    assert np.array_equal(records[0]["pred"], expect)
    assert records[0]["score"] == [p[:, 2].mean() for p in people]
