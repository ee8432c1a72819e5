"""Bottom-up multi-scale test on the MI355X: ``resize_bilinear`` and ``decode_multi_scale`` against a torch-CPU restatement of the
protocol composed from the decoder oracle of tests/test_gpu_bottomup.py, bit for bit; the identities that tie the
new launch to ``decode`` and ``decode_flip_aggregated``; the refusals of the C entry.

Every comparison is ``torch.equal``: the kernel restates the oracle's fp32 operations in the oracle's order
with fp contraction off, whatever the resize ratios."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

import mindpose_amd as mp  # noqa: E402
from mindpose_amd import _lib  # noqa: E402
from mindpose_amd.models.decoders import resize_bilinear  # noqa: E402
from tests.test_gpu_bottomup import _dyadic, _resize_bilinear, oracle_decode  # noqa: E402
from tests.test_gpu_bottomup_flip import COCO_FLIP_INDEX, THREE_CYCLE, oracle_flip_decode  # noqa: E402

DEV = torch.device("cuda:0")
K = 17
NAMES = ("val_k", "tag_k", "ind_k", "heatmap_raw", "tagging")


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------
def oracle_multi_heat(runs, flipped_runs, flip_index, base):
    """total of DESIGN.md 4.13 before the mask, in the order written there."""
    f = None if flip_index is None else torch.as_tensor(flip_index, dtype=torch.long)
    hm, wm = runs[base][-1].shape[2:]
    total = None
    for r, outs in enumerate(runs):
        taps = []
        for i, a in enumerate(outs):
            a = a.detach().cpu().float()
            if flipped_runs is None:
                taps.append(a[:, :K])
            else:
                b = flipped_runs[r][i].detach().cpu().float()
                taps.append((a[:, :K] + b[:, f].flip(3)) * 0.5)
        v = taps[-1] if r == base else _resize_bilinear(taps[-1], hm, wm)
        for t in taps[:-1]:
            v = v + _resize_bilinear(t, hm, wm)
        if len(taps) > 1:
            v = v / len(taps)
        total = v if total is None else total + v
    if len(runs) > 1:
        total = total / len(runs)
    return total


def oracle_multi_decode(runs, flipped_runs, flip_index, base, mask, with_ae, use_nms, nms_kernel, max_num, shift):
    """The five outputs: the tagging map from the decoder oracle on the base run (the flip oracle's two halves under the flip test),
    the peaks from the decoder oracle on the aggregated map as a single stage - with tag slot l beside it as that stage's tags, so
    that the oracle's own gather yields tag_k[..., l] (stage mean and resize are the identity on a single stage at map size)."""
    ns = len(with_ae)
    if flipped_runs is None:
        tagging = oracle_decode(runs[base], mask, ns, with_ae, use_nms, nms_kernel, max_num, True, shift)[4]
    else:
        tagging = oracle_flip_decode(runs[base], flipped_runs[base], flip_index, mask, with_ae, use_nms, nms_kernel, max_num, shift)[4]
    total = oracle_multi_heat(runs, flipped_runs, flip_index, base)
    tag_k = []
    for l in range(tagging.shape[-1]):
        val, tag_l, ind, raw, same = oracle_decode([torch.cat([total, tagging[..., l]], 1)], mask, 1, [True], use_nms, nms_kernel,
                                                   max_num, True, shift)
        assert torch.equal(same[..., 0], tagging[..., l])
        tag_k.append(tag_l[..., 0])
    return val, torch.stack(tag_k, -1), ind, raw, tagging


# ---- 1. the resize entry --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src,dst", [((24, 40), (48, 80)), ((48, 80), (24, 40)), ((20, 33), (48, 80)), ((48, 80), (48, 80)),
                                     ((24, 40), (45, 75)), ((17, 9), (5, 3))])
def test_resize_bilinear_bit_equal(src, dst):
    """Up, down, a non-dividing ratio, the identity and two widths that are no multiple of 4 (the scalar-store form)."""
    x = torch.randn(2, 3, *src, generator=torch.Generator().manual_seed(src[1] + dst[1]))
    got = resize_bilinear(x.to(DEV), dst)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (2, 3, *dst)
    assert torch.equal(got.cpu(), _resize_bilinear(x, *dst))


def test_resize_bilinear_into_an_offset_view_and_argument_checks():
    """``out=`` a contiguous view whose address is 4 mod 16 (scalar stores although the width divides by 4), and the refusals."""
    x = torch.randn(1, 2, 12, 20, generator=torch.Generator().manual_seed(2))
    store = torch.full((2 * 24 * 40 + 1,), 7.0, device=DEV)
    out = store[1:].view(1, 2, 24, 40)
    assert out.data_ptr() % 16 == 4
    got = resize_bilinear(x.to(DEV), (24, 40), out=out)
    assert got.data_ptr() == out.data_ptr() and store[0].item() == 7.0
    assert torch.equal(out.cpu(), _resize_bilinear(x, 24, 40))
    xd = x.to(DEV)
    for bad in (torch.empty(1, 2, 24, 41, device=DEV), torch.empty(1, 2, 24, 40, device=DEV, dtype=torch.float16),
                torch.empty(1, 2, 24, 80, device=DEV)[..., ::2], torch.empty(1, 2, 24, 40)):
        with pytest.raises(ValueError):
            resize_bilinear(xd, (24, 40), out=bad)
    with pytest.raises(ValueError):
        resize_bilinear(xd, (12, 20), out=xd)
    with pytest.raises(ValueError):
        resize_bilinear(xd, (0, 20))
    with pytest.raises(ValueError):
        resize_bilinear(xd[0], (24, 40))


# ---- 2. dyadic bit-equality of all five outputs ---------------------------------------------------------------------------------------
MAP = (48, 80)  # three tile rows; one full and one ragged 64-column tile
RUNS = {"half": [(12, 20), (24, 40)], "base": [(24, 40), MAP], "double": [MAP, (96, 160)], "nondiv": [(20, 33), (40, 66)]}
LAYOUTS = {  # run names, position of the base run
    "half_base": (["half", "base"], 1),
    "base_double": (["base", "double"], 0),
    "half_base_double": (["half", "base", "double"], 1),
    "nondiv_base_double_half": (["nondiv", "base", "double", "half"], 1),
}
AE = {"one_tag_stage": [True, False], "two_tag_stages": [True, True]}
PARAMS = [(3, False, 30), (5, True, 30), (3, True, 64), (5, False, 1), (3, True, 1), (5, False, 64)]  # nms_kernel, shift, max_num


def _mask(n):
    """image-resolution mask (2x the map) that blanks a different right / bottom band per image"""
    h, w = 2 * MAP[0], 2 * MAP[1]
    m = torch.zeros(n, h, w, dtype=torch.bool)
    for i in range(n):
        m[i, : h - 10 - 14 * i, : w - 22 - 18 * i] = True
    return m


def _run_outputs(n, names, with_ae, gen, dyadic=True):
    runs = []
    for name in names:
        shapes = [(n, K * (2 if ae else 1), h, w) for (h, w), ae in zip(RUNS[name], with_ae)]
        runs.append([_dyadic(s, gen) if dyadic else torch.randn(s, generator=gen) for s in shapes])
    return runs


def _decoder(with_ae, nms_kernel, shift, max_num):
    return mp.create_decoder("bottomup_heatmap_ae", num_joints=K, num_stages=2, with_ae_loss=with_ae, use_nms=True,
                             nms_kernel=nms_kernel, max_num=max_num, shift_coordinate=shift)


def _to_dev(runs):
    return None if runs is None else [[t.to(DEV) for t in outs] for outs in runs]


def _check_bit_equal(layout, ae, flip_index, nms_kernel, shift, max_num, seed):
    names, base = LAYOUTS[layout]
    with_ae = AE[ae]
    gen = torch.Generator().manual_seed(seed)
    runs = _run_outputs(2, names, with_ae, gen)
    flipped = None if flip_index is None else _run_outputs(2, names, with_ae, gen)
    mask = _mask(2)
    dec = _decoder(with_ae, nms_kernel, shift, max_num)
    got = dec.decode_multi_scale(_to_dev(runs), mask.to(DEV), base, _to_dev(flipped), flip_index)
    torch.cuda.synchronize()
    ref = oracle_multi_decode(runs, flipped, flip_index, base, mask, with_ae, True, nms_kernel, max_num, shift)
    num_tags = sum(with_ae) * (1 if flip_index is None else 2)
    assert tuple(ref[4].shape) == (2, K, *MAP, num_tags) and tuple(ref[1].shape) == (2, K, max_num, num_tags)
    for name, g, r in zip(NAMES, got, ref):
        assert g.dtype == torch.float32 and g.is_cuda
        assert tuple(g.shape) == tuple(r.shape), name
        assert torch.equal(g.cpu(), r), f"{name} differs"


def _matrix():
    cases, c = [], 0
    for layout in LAYOUTS:
        for ae in AE:
            for flip in (False, True):
                for j in range(3):  # three of the six parameter sets per combination, rotating: every set meets every layout
                    cases.append(pytest.param(layout, ae, flip, *PARAMS[(c + 2 * j) % 6],
                                              id=f"{layout}-{ae}-{'flip' if flip else 'plain'}-{j}"))
                c += 1
    return cases


@pytest.mark.parametrize("layout,ae,flip,nms_kernel,shift,max_num", _matrix())
def test_multi_scale_decode_bit_equal_on_dyadic_inputs(layout, ae, flip, nms_kernel, shift, max_num):
    """Runs below, at and above the map, a run no stage of which divides the map, the base run first or second, two to four runs
    (the division by 3 rounds), with and without the flip test.  Dyadic inputs keep many equal values among the peaks, so the
    (value descending, index ascending) order of the top-k is exercised on the averaged map too."""
    _check_bit_equal(layout, ae, COCO_FLIP_INDEX if flip else None, nms_kernel, shift, max_num,
                     seed=3 + len(layout) + 5 * max_num + nms_kernel + int(flip))


@pytest.mark.parametrize("layout,ae", [("half_base_double", "one_tag_stage"), ("nondiv_base_double_half", "two_tag_stages")])
def test_multi_scale_decode_with_a_three_cycle_permutation(layout, ae):
    """A flip index that is no involution: joint k reads channel f[k] of every run's mirrored partner, not f^-1[k]."""
    _check_bit_equal(layout, ae, THREE_CYCLE, 3, True, 30, seed=5)


# ---- 3. identities on random-normal inputs --------------------------------------------------------------------------------------------
def _equal(got, ref):
    for name, g, r in zip(NAMES, got, ref):
        assert torch.equal(g, r), f"{name} differs"


@pytest.mark.parametrize("sizes", [[(24, 40), MAP], [(20, 33), MAP]], ids=["lower_24x40", "lower_20x33"])
@pytest.mark.parametrize("ae", list(AE))
def test_multi_scale_identities(sizes, ae):
    """One run is ``decode`` (with mirrored partners ``decode_flip_aggregated``) operation for operation; two and four copies of a
    run are that decode too: the copies' last stage goes through the resize at ratio 1, which returns the tap itself, and
    (v + v) / 2 and ((v + v) + v + v) / 4 are exact in fp32 (3v rounds by less than half an ulp of 4v)."""
    with_ae = AE[ae]
    gen = torch.Generator().manual_seed(41)
    shapes = [(2, K * (2 if t else 1), h, w) for (h, w), t in zip(sizes, with_ae)]
    a = [torch.randn(s, generator=gen).to(DEV) for s in shapes]
    b = [torch.randn(s, generator=gen).to(DEV) for s in shapes]
    mask = _mask(2).to(DEV)
    dec = _decoder(with_ae, 3, True, 30)
    plain = dec(a, mask)
    flip = dec.decode_flip_aggregated(a, b, COCO_FLIP_INDEX, mask)
    assert not torch.equal(plain[3], flip[3])
    _equal(dec.decode_multi_scale([a], mask, 0), plain)
    _equal(dec.decode_multi_scale([a], mask, 0, [b], COCO_FLIP_INDEX), flip)
    _equal(dec.decode_multi_scale([a, a], mask, 1), plain)
    _equal(dec.decode_multi_scale([a, a, a, a], mask, 2), plain)
    _equal(dec.decode_multi_scale([a, a], mask, 0, [b, b], COCO_FLIP_INDEX), flip)


# ---- 4. tags come from the base run only ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", [False, True])
def test_multi_scale_never_reads_the_tags_of_the_other_runs(flip):
    with_ae = AE["two_tag_stages"]
    names, base = LAYOUTS["half_base_double"]
    gen = torch.Generator().manual_seed(17)
    runs = _to_dev(_run_outputs(2, names, with_ae, gen, dyadic=False))
    flipped = _to_dev(_run_outputs(2, names, with_ae, gen, dyadic=False)) if flip else None
    index = COCO_FLIP_INDEX if flip else None
    mask = _mask(2).to(DEV)
    dec = _decoder(with_ae, 3, True, 30)
    clean = dec.decode_multi_scale(runs, mask, base, flipped, index)
    for group in (runs, flipped or []):
        for r, outs in enumerate(group):
            if r != base:
                for t in outs:
                    t[:, K:] = float("nan")
    assert all(torch.isnan(t[:, K:]).all() for r, outs in enumerate(runs) if r != base for t in outs)
    got = dec.decode_multi_scale(runs, mask, base, flipped, index)
    for name, g, c in zip(NAMES, got, clean):
        assert not torch.isnan(g).any(), name
        assert torch.equal(g, c), f"{name} differs"


# ---- 5. refusals through the C ABI ----------------------------------------------------------------------------------------------------
def test_multi_entry_refusals_reach_no_launch():
    lib = _lib.load()
    n, h, w, m = 1, 16, 16, 8
    base_t = [torch.zeros(n, 2 * K, h // 2, w // 2, device=DEV), torch.zeros(n, K, h, w, device=DEV)]
    half_t = [torch.zeros(n, 2 * K, h // 4, w // 4, device=DEV), torch.zeros(n, K, h // 2, w // 2, device=DEV)]
    mask = torch.ones(n, h, w, dtype=torch.uint8, device=DEV)
    raw, tagging = torch.full((n, K, h, w), 5.0, device=DEV), torch.full((n, K, h, w, 2), 5.0, device=DEV)
    ws_bytes = lib.mp_bottomup_workspace_bytes(n, K, h, w, m)
    ws = torch.full((ws_bytes // 8,), -1, device=DEV, dtype=torch.int64)

    def stages(tensors, **kw):
        fields = [dict(data=t.data_ptr(), c=t.shape[1], h=t.shape[2], w=t.shape[3], has_tags=int(i == 0)) for i, t in enumerate(tensors)]
        for f in fields:
            f.update(kw)
        return (_lib.BottomUpStage * len(fields))(*[_lib.BottomUpStage(**f) for f in fields])

    def call(run_stages=None, flipped=None, flip_index=None, num_runs=2, base_run=1, tag_per_joint=1, bytes_=ws_bytes, table=True):
        run_stages = run_stages or [stages(half_t), stages(base_t)]
        flipped = flipped or [None] * len(run_stages)
        runs = (_lib.BottomUpRun * len(run_stages))(*[_lib.BottomUpRun(stages=a, flipped=b) for a, b in zip(run_stages, flipped)])
        index = None if flip_index is None else (ctypes.c_int32 * K)(*flip_index)
        return lib.mp_bottomup_parse_nms_topk_multi(runs if table else None, num_runs, base_run, index, 2, _lib.ptr(mask), h, w, n, K,
                                                    tag_per_joint, 3, m, _lib.ptr(raw), _lib.ptr(tagging), _lib.ptr(ws), bytes_,
                                                    _lib.stream())

    both = [stages(half_t), stages(base_t)]
    assert call(table=False) == -1                                                     # MP_ERR_NULL: no run table
    assert call([stages(half_t), None]) == -1                                          # ... a run without a stage array
    assert call(flipped=both) == -1                                                    # ... mirrored arrays without a flip index
    assert call(num_runs=0) == -2 and call([stages(base_t)] * 5, num_runs=5, base_run=0) == -2   # MP_ERR_SHAPE: 1..4 runs
    assert call(base_run=-1) == -2 and call(base_run=2) == -2
    assert call(flipped=[stages(half_t, w=3), stages(base_t)], flip_index=COCO_FLIP_INDEX) == -2  # mirrored stage shaped otherwise
    assert call(flipped=both, flip_index=COCO_FLIP_INDEX[:-1] + [K]) == -2             # flip index entry outside [0, k)
    assert call(flipped=both, flip_index=[-1] + COCO_FLIP_INDEX[1:]) == -2
    assert call(flipped=both, flip_index=COCO_FLIP_INDEX, tag_per_joint=0) == -3       # MP_ERR_UNSUPPORTED: one tag map with flip
    assert call(bytes_=ws_bytes - 8) == -5                                             # MP_ERR_WORKSPACE
    assert call(flipped=both, flip_index=COCO_FLIP_INDEX, bytes_=ws_bytes - 8) == -5
    torch.cuda.synchronize()
    assert (raw == 5.0).all() and (tagging == 5.0).all() and (ws == -1).all()          # nothing was launched
    assert call() == 0 and call(flipped=both, flip_index=COCO_FLIP_INDEX) == 0         # the same arguments, valid: both forms run
    torch.cuda.synchronize()
    assert (raw == 0.0).all() and (tagging == 0.0).all()
