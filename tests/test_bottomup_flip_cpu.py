"""Bottom-up flip TTA without a GPU: the host-side refusals of ``mp_bottomup_parse_nms_topk_flip`` (every case returns before a
launch, its pointers are dummy addresses that are never dereferenced), the argument checks of ``decode_flip_aggregated`` and the
constructor checks of the inferencer."""
import ctypes

import numpy as np
import pytest
import torch

import mindpose_amd as mp
from mindpose_amd import _lib

K = 17
COCO_FLIP_PAIRS = [[1, 2], [3, 4], [5, 6], [7, 8], [9, 10], [11, 12], [13, 14], [15, 16]]
COCO_FLIP_INDEX = [0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15]
MP_ERR_NULL, MP_ERR_SHAPE, MP_ERR_UNSUPPORTED = -1, -2, -3
DUMMY = 0x1000  # a non-null address that no refused call reads


def _stages(specs):
    return (_lib.BottomUpStage * len(specs))(*[_lib.BottomUpStage(data=DUMMY, c=c, h=h, w=w, has_tags=t) for c, h, w, t in specs])


def _call(stages, flipped, flip_index, k=K, tag_per_joint=1):
    """the entry on a 16 x 16 map with every other argument valid: workspace large enough, NMS 3, max_num 8"""
    lib = _lib.load()
    index = None if flip_index is None else (ctypes.c_int32 * len(flip_index))(*flip_index)
    return lib.mp_bottomup_parse_nms_topk_flip(
        None if stages is None else _stages(stages), None if flipped is None else _stages(flipped), index,
        0 if stages is None else len(stages), DUMMY, 32, 32, 1, k, tag_per_joint, 3, 8, DUMMY, DUMMY, DUMMY, 1 << 24, None)


TWO = [(2 * K, 8, 8, 1), (K, 16, 16, 0)]


def _with(specs, i, **kw):
    names = ("c", "h", "w", "has_tags")
    out = [list(s) for s in specs]
    for name, v in kw.items():
        out[i][names.index(name)] = v
    return [tuple(s) for s in out]


REFUSALS = {
    "null_stage_array": (dict(stages=None, flipped=TWO, flip_index=COCO_FLIP_INDEX), MP_ERR_NULL),
    "null_flipped_array": (dict(stages=TWO, flipped=None, flip_index=COCO_FLIP_INDEX), MP_ERR_NULL),
    "null_flip_index": (dict(stages=TWO, flipped=TWO, flip_index=None), MP_ERR_NULL),
    "flip_entry_minus_one": (dict(stages=TWO, flipped=TWO, flip_index=COCO_FLIP_INDEX[:5] + [-1] + COCO_FLIP_INDEX[6:]), MP_ERR_SHAPE),
    "flip_entry_k": (dict(stages=TWO, flipped=TWO, flip_index=COCO_FLIP_INDEX[:-1] + [K]), MP_ERR_SHAPE),
    "flipped_other_width": (dict(stages=TWO, flipped=_with(TWO, 0, w=7), flip_index=COCO_FLIP_INDEX), MP_ERR_SHAPE),
    "flipped_other_has_tags": (dict(stages=TWO, flipped=_with(TWO, 1, has_tags=1), flip_index=COCO_FLIP_INDEX), MP_ERR_SHAPE),
    "three_tag_stages": (dict(stages=[(2 * K, 4, 4, 1), (2 * K, 8, 8, 1), (2 * K, 16, 16, 1)],
                              flipped=[(2 * K, 4, 4, 1), (2 * K, 8, 8, 1), (2 * K, 16, 16, 1)], flip_index=COCO_FLIP_INDEX),
                         MP_ERR_UNSUPPORTED),
    "one_tag_map": (dict(stages=[(K + 1, 8, 8, 1), (K, 16, 16, 0)], flipped=[(K + 1, 8, 8, 1), (K, 16, 16, 0)],
                         flip_index=COCO_FLIP_INDEX, tag_per_joint=0), MP_ERR_UNSUPPORTED),
    "k_above_the_flip_cap": (dict(stages=[(130, 8, 8, 1), (65, 16, 16, 0)], flipped=[(130, 8, 8, 1), (65, 16, 16, 0)],
                                  flip_index=list(range(65)), k=65), MP_ERR_UNSUPPORTED),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_flip_entry_refuses_on_the_host(name):
    kwargs, code = REFUSALS[name]
    assert _call(**kwargs) == code


def test_flip_entry_is_declared():
    assert "mp_bottomup_parse_nms_topk_flip" in _lib.EXPORTED_SYMBOLS


# ---- decoder ------------------------------------------------------------------------------------------------------------------------
def _cpu_outputs(ktag=K):
    return [torch.zeros(1, K + ktag, 4, 4), torch.zeros(1, K, 8, 8)]


@pytest.mark.parametrize("flip_index", [COCO_FLIP_INDEX[:-1], COCO_FLIP_INDEX + [0], [0, 1, 1] + COCO_FLIP_INDEX[3:]],
                         ids=["short", "long", "repeated_entry"])
def test_decode_flip_aggregated_refuses_a_flip_index_that_is_no_permutation(flip_index):
    dec = mp.create_decoder("bottomup_heatmap_ae")
    with pytest.raises(ValueError):
        dec.decode_flip_aggregated(_cpu_outputs(), _cpu_outputs(), flip_index, torch.ones(1, 16, 16, dtype=torch.bool))


def test_decode_flip_aggregated_refuses_one_tag_map():
    dec = mp.create_decoder("bottomup_heatmap_ae", tag_per_joint=False)
    with pytest.raises(ValueError):
        dec.decode_flip_aggregated(_cpu_outputs(1), _cpu_outputs(1), COCO_FLIP_INDEX, torch.ones(1, 16, 16, dtype=torch.bool))


# ---- inferencer ---------------------------------------------------------------------------------------------------------------------
def _cfg(flip_pairs):
    return dict(has_heatmap_output=True, hflip_tta=True, joint_order=list(range(K)), vis_thr=0.1, ignore_too_much=False,
                use_rounded_norm=True, tag_thr=1.0, pixel_std=200.0, downsample_scale=2, refine_missing_joint=False,
                flip_pairs=flip_pairs)


def test_inferencer_constructs_with_flip_tta():
    inf = mp.BottomUpHeatMapAEInferencer(net=None, config=_cfg(COCO_FLIP_PAIRS), decoder=mp.create_decoder("bottomup_heatmap_ae"))
    assert np.asarray(inf._multi_run_net.flip_index).tolist() == COCO_FLIP_INDEX
    assert inf._inference_cfg["flip_index"].tolist() == COCO_FLIP_INDEX


def test_inferencer_refuses_flip_pairs_that_leave_joints_out():
    with pytest.raises(ValueError):
        mp.BottomUpHeatMapAEInferencer(net=None, config=_cfg([[1, 2], [3, 4]]), decoder=mp.create_decoder("bottomup_heatmap_ae"))


def test_inferencer_refuses_flip_tta_with_one_tag_map():
    with pytest.raises(ValueError):
        mp.BottomUpHeatMapAEInferencer(net=None, config=_cfg(COCO_FLIP_PAIRS),
                                       decoder=mp.create_decoder("bottomup_heatmap_ae", tag_per_joint=False))
