"""Bottom-up multi-scale test without a GPU: the argument checks of ``decode_multi_scale`` / ``resize_bilinear``, and the host-side
refusals of ``mp_bottomup_parse_nms_topk_multi`` and ``mp_resize_bilinear_nchw`` (every case returns before a launch; its pointers are dummy
addresses that are never dereferenced)."""
import ctypes

import pytest
import torch

import mindpose_amd as mp
from mindpose_amd import _lib
from mindpose_amd.models.decoders import resize_bilinear

K = 17
COCO_FLIP_INDEX = [0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15]
MP_ERR_NULL, MP_ERR_SHAPE, MP_ERR_UNSUPPORTED, MP_ERR_WORKSPACE = -1, -2, -3, -5
DUMMY = 0x1000  # a non-null address that no refused call reads


# ---- decoder ------------------------------------------------------------------------------------------------------------------------
def _cpu_outputs(h=4, w=4):
    return [torch.zeros(1, 2 * K, h, w), torch.zeros(1, K, 2 * h, 2 * w)]


def test_decode_multi_scale_refuses_on_shape_before_the_device():
    dec = mp.create_decoder("bottomup_heatmap_ae")
    mask = torch.ones(1, 16, 16, dtype=torch.bool)
    run = _cpu_outputs()
    with pytest.raises(ValueError):
        dec.decode_multi_scale([], mask, 0)
    with pytest.raises(ValueError):
        dec.decode_multi_scale([run] * 5, mask, 0)
    for base in (-1, 2, None):
        with pytest.raises(ValueError):
            dec.decode_multi_scale([run, run], mask, base)
    with pytest.raises(ValueError):
        dec.decode_multi_scale([run, run], mask, 0, flipped_runs=[run, run])             # mirrored runs without a flip index
    with pytest.raises(ValueError):
        dec.decode_multi_scale([run, run], mask, 0, flip_index=COCO_FLIP_INDEX)          # ... and the reverse
    with pytest.raises(ValueError):
        dec.decode_multi_scale([run, run], mask, 0, [run, run], COCO_FLIP_INDEX[:-1])    # no permutation
    with pytest.raises(ValueError):
        dec.decode_multi_scale([run, run], mask, 0, [run], COCO_FLIP_INDEX)              # one mirrored run for two runs
    with pytest.raises(ValueError):
        dec.decode_multi_scale([run[:1], run], mask, 1)                                  # a run with a stage missing
    with pytest.raises(ValueError):
        dec.decode_multi_scale([[torch.zeros(1, K + 1, 4, 4), run[1]], run], mask, 1)    # a run with another channel layout


def test_resize_bilinear_is_exported_and_refuses_cpu_tensors():
    assert mp.models.decoders.resize_bilinear is resize_bilinear
    with pytest.raises(_lib.MindposeHipError):
        resize_bilinear(torch.zeros(1, 3, 8, 8), (16, 16))  # no CPU fallback


# ---- C ABI --------------------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared():
    assert "mp_bottomup_parse_nms_topk_multi" in _lib.EXPORTED_SYMBOLS
    assert "mp_resize_bilinear_nchw" in _lib.EXPORTED_SYMBOLS


def _stages(specs):
    return (_lib.BottomUpStage * len(specs))(*[_lib.BottomUpStage(data=d, c=c, h=h, w=w, has_tags=t) for d, c, h, w, t in specs])


BASE = [(DUMMY, 2 * K, 8, 8, 1), (DUMMY, K, 16, 16, 0)]
HALF = [(DUMMY, 2 * K, 4, 4, 1), (DUMMY, K, 8, 8, 0)]
DOUBLE = [(DUMMY, 2 * K, 16, 16, 1), (DUMMY, K, 32, 32, 0)]


def _with(specs, i, **kw):
    names = ("data", "c", "h", "w", "has_tags")
    out = [list(s) for s in specs]
    for name, v in kw.items():
        out[i][names.index(name)] = v
    return [tuple(s) for s in out]


def _call(runs, flipped=None, flip_index=None, base_run=0, num_runs=None, num_stages=2, k=K, tag_per_joint=1, nms=3, max_num=8,
          workspace=DUMMY, workspace_bytes=1 << 24, null_table=False):
    """the entry on a 16 x 16 base map with every argument not named valid"""
    lib = _lib.load()
    keep = [(None if s is None else _stages(s), None if flipped is None or flipped[r] is None else _stages(flipped[r]))
            for r, s in enumerate(runs)]
    table = (_lib.BottomUpRun * max(len(keep), 1))(*[_lib.BottomUpRun(stages=a, flipped=b) for a, b in keep])
    index = None if flip_index is None else (ctypes.c_int32 * len(flip_index))(*flip_index)
    return lib.mp_bottomup_parse_nms_topk_multi(None if null_table else table, len(runs) if num_runs is None else num_runs, base_run,
                                                index, num_stages, DUMMY, 32, 32, 1, k, tag_per_joint, nms, max_num, DUMMY, DUMMY,
                                                workspace, workspace_bytes, None)


FLIP = dict(flipped=[HALF, BASE], flip_index=COCO_FLIP_INDEX)
REFUSALS = {
    "null_run_table": (dict(runs=[HALF, BASE], base_run=1, null_table=True), MP_ERR_NULL),
    "null_stage_array": (dict(runs=[HALF, None], base_run=0), MP_ERR_NULL),
    "null_stage_data": (dict(runs=[_with(HALF, 1, data=None), BASE], base_run=1), MP_ERR_NULL),
    "null_mirrored_data": (dict(runs=[HALF, BASE], base_run=1, flipped=[_with(HALF, 0, data=None), BASE],
                                flip_index=COCO_FLIP_INDEX), MP_ERR_NULL),
    "mirrored_without_flip_index": (dict(runs=[HALF, BASE], base_run=1, flipped=[HALF, BASE]), MP_ERR_NULL),
    "flip_index_without_mirrored": (dict(runs=[HALF, BASE], base_run=1, flip_index=COCO_FLIP_INDEX), MP_ERR_NULL),
    "zero_runs": (dict(runs=[BASE], num_runs=0), MP_ERR_SHAPE),
    "five_runs": (dict(runs=[BASE] * 5, num_runs=5), MP_ERR_SHAPE),
    "base_run_minus_one": (dict(runs=[HALF, BASE], base_run=-1), MP_ERR_SHAPE),
    "base_run_past_the_end": (dict(runs=[HALF, BASE], base_run=2), MP_ERR_SHAPE),
    "mirrored_in_one_run_only": (dict(runs=[HALF, BASE], base_run=1, flipped=[HALF, None], flip_index=COCO_FLIP_INDEX), MP_ERR_SHAPE),
    "run_with_other_channels": (dict(runs=[_with(HALF, 0, c=K), BASE], base_run=1), MP_ERR_SHAPE),
    "run_with_other_tag_stages": (dict(runs=[_with(HALF, 0, has_tags=0), BASE], base_run=1), MP_ERR_SHAPE),
    "run_with_zero_height": (dict(runs=[_with(HALF, 0, h=0), BASE], base_run=1), MP_ERR_SHAPE),
    "mirrored_other_width": (dict(runs=[HALF, BASE], base_run=1, flipped=[_with(HALF, 1, w=7), BASE], flip_index=COCO_FLIP_INDEX),
                             MP_ERR_SHAPE),
    "flip_entry_minus_one": (dict(runs=[HALF, BASE], base_run=1, flipped=[HALF, BASE],
                                  flip_index=COCO_FLIP_INDEX[:5] + [-1] + COCO_FLIP_INDEX[6:]), MP_ERR_SHAPE),
    "flip_entry_k": (dict(runs=[HALF, BASE], base_run=1, flipped=[HALF, BASE], flip_index=COCO_FLIP_INDEX[:-1] + [K]), MP_ERR_SHAPE),
    "one_tag_map_with_flip": (dict(runs=[_with(HALF, 0, c=K + 1), _with(BASE, 0, c=K + 1)], base_run=1,
                                   flipped=[_with(HALF, 0, c=K + 1), _with(BASE, 0, c=K + 1)], flip_index=COCO_FLIP_INDEX,
                                   tag_per_joint=0), MP_ERR_UNSUPPORTED),
    "nms_kernel_4": (dict(runs=[HALF, BASE], base_run=1, nms=4), MP_ERR_UNSUPPORTED),
    "max_num_65": (dict(runs=[HALF, BASE], base_run=1, max_num=65), MP_ERR_UNSUPPORTED),
    "short_workspace": (dict(runs=[DOUBLE, BASE], base_run=1, workspace_bytes=K * 8 * 8 - 8), MP_ERR_WORKSPACE),
    "no_workspace": (dict(runs=[DOUBLE, BASE], base_run=1, workspace=None), MP_ERR_WORKSPACE),
    "short_workspace_with_flip": (dict(runs=[HALF, BASE], base_run=1, workspace_bytes=K * 8 * 8 - 8, **FLIP), MP_ERR_WORKSPACE),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_multi_entry_refuses_on_the_host(name):
    kwargs, code = REFUSALS[name]
    assert _call(**kwargs) == code


def test_workspace_is_the_base_maps_whatever_the_other_runs():
    assert _lib.load().mp_bottomup_workspace_bytes(1, K, 16, 16, 8) == K * 8 * 8  # one tile; the bound short_workspace undercuts


def test_resize_entry_refuses_on_the_host():
    lib = _lib.load()
    assert lib.mp_resize_bilinear_nchw(None, DUMMY, 3, 8, 8, 16, 16, None) == MP_ERR_NULL
    assert lib.mp_resize_bilinear_nchw(DUMMY, None, 3, 8, 8, 16, 16, None) == MP_ERR_NULL
    for planes, ih, iw, oh, ow in [(0, 8, 8, 16, 16), (3, 0, 8, 16, 16), (3, 8, -1, 16, 16), (3, 8, 8, 0, 16), (3, 8, 8, 16, 0),
                                   (1, 1 << 16, 1 << 16, 4, 4), (1, 4, 4, 1 << 16, 1 << 16)]:
        assert lib.mp_resize_bilinear_nchw(DUMMY, DUMMY, planes, ih, iw, oh, ow, None) == MP_ERR_SHAPE
