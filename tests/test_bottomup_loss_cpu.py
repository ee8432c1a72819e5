"""CPU-side checks of the bottom-up training ends: registry names, constructor defaults and ``forward`` parameter order as
the reference declares them (mindpose/models/loss/{mse,ae,multi_loss}.py, data/transform/bottomup_transform.py:463-490), the loud
errors, the argument validation of every new ``mp_*`` entry (it runs before any HIP call), and the host ``transform`` of
``BottomUpGenerateTarget`` bit-equal to the reference's recorded outputs (tests/golden/bottomup_target.npz)."""
import inspect
import os

import numpy as np
import pytest
import torch

import mindpose_amd as mp
from mindpose_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bottomup_target.npz")


def _params(fn):
    return [(k, v.default) for k, v in list(inspect.signature(fn).parameters.items())[1:]]


def test_registry_names_and_exports():
    for module, names in (("loss", ["JointsMSELossWithMask", "joint_mse_with_mask", "AELoss", "ae", "AEMultiLoss", "ae_multi_loss"]),
                          ("transform", ["BottomUpGenerateTarget", "bottomup_generate_target"])):
        for name in names:
            assert callable(mp.entrypoint(module, name)), name
    from mindpose_amd.models import loss as loss_pkg
    for name in ("JointsMSELossWithMask", "AELoss", "AEMultiLoss"):
        assert getattr(mp, name) is getattr(loss_pkg, name) is mp.entrypoint("loss", name)
    assert mp.BottomUpGenerateTarget is mp.entrypoint("transform", "bottomup_generate_target")
    assert isinstance(mp.create_loss("ae_multi_loss"), mp.AEMultiLoss)
    assert isinstance(mp.create_loss("ae", tag_per_joint=False), mp.AELoss)
    assert isinstance(mp.create_loss("joint_mse_with_mask"), mp.JointsMSELossWithMask)


def test_constructor_defaults_and_forward_order_match_reference():
    assert _params(mp.JointsMSELossWithMask.__init__) == [("reduction", "mean")]
    assert _params(mp.AELoss.__init__) == [("tag_per_joint", True), ("reduction", "mean")]
    assert _params(mp.AEMultiLoss.__init__) == [
        ("num_joints", 17), ("num_stages", 2), ("stage_sizes", [(128, 128), (256, 256)]), ("mse_loss_factor", [1.0, 1.0]),
        ("ae_loss_factor", [0.001, 0.001]), ("with_mse_loss", [True, True]), ("with_ae_loss", [True, False]), ("tag_per_joint", True)]
    assert _params(mp.BottomUpGenerateTarget.__init__) == [("is_train", True), ("config", None), ("sigma", 2.0), ("max_num", 30)]
    assert [k for k, _ in _params(mp.JointsMSELossWithMask.forward)] == ["pred", "target", "mask"]
    assert [k for k, _ in _params(mp.AELoss.forward)] == ["pred", "target"]
    assert [k for k, _ in _params(mp.AEMultiLoss.forward)] == ["preds", "target", "mask", "tag_ind"]
    assert mp.AELoss().eps == 0.01
    multi = mp.AEMultiLoss()
    assert isinstance(multi.mse_criterion, mp.JointsMSELossWithMask) and isinstance(multi.ae_criterion, mp.AELoss)


def test_loud_errors():
    for cls in (mp.JointsMSELossWithMask, mp.AELoss):
        for reduction in ("sum", "none"):
            with pytest.raises(NotImplementedError):
                cls(reduction=reduction)
    with pytest.raises(_lib.MindposeHipError):
        mp.JointsMSELossWithMask()(torch.zeros(1, 1, 2, 2), torch.zeros(1, 1, 2, 2), torch.ones(1, 2, 2))
    with pytest.raises(_lib.MindposeHipError):
        mp.AELoss()(torch.zeros(1, 2, 4, 4), torch.zeros(1, 3, 2, 2, dtype=torch.int32))
    multi = mp.AEMultiLoss(num_joints=2, stage_sizes=[(4, 4), (8, 8)])
    args = ([torch.zeros(1, 4, 4, 4), torch.zeros(1, 2, 8, 8)], torch.zeros(1, 2, 2, 8, 8), torch.ones(1, 2, 8, 8),
            torch.zeros(1, 2, 3, 2, 2, dtype=torch.int32))
    with pytest.raises(_lib.MindposeHipError):
        multi(*args)
    with pytest.raises(ValueError):
        mp.AEMultiLoss(num_stages=3)
    # the pins of the rest of the training path stay where they are
    with pytest.raises(ValueError):
        mp.TopDownHeatMapInferencer(None, config=dict(has_heatmap_output=True, hflip_tta=True, shift_heatmap=False, flip_pairs=[[1, 2]]))


def _cfg(sizes, tag_per_joint):
    return dict(image_size=[512, 512], max_image_size=[512, 512], heatmap_sizes=[list(map(int, s)) for s in sizes],
                flip_pairs=[[1, 2]], pixel_std=200.0, tag_per_joint=bool(tag_per_joint))


def test_generate_target_errors():
    t = mp.BottomUpGenerateTarget(config=_cfg([(16, 16)], True), max_num=2)
    with pytest.raises(ValueError, match="exceeds the maximum num"):
        t.transform(dict(keypoints=[np.ones((3, 4, 3), np.float32)]))
    with pytest.raises(_lib.MindposeHipError):
        t.generate_batch(torch.zeros(1, 1, 2, 4, 3), [1])
    with pytest.raises(KeyError):
        mp.BottomUpGenerateTarget(config=dict(image_size=[512, 512]))


def test_entry_points_validate_before_any_hip_call():
    lib = _lib.load()
    P = 4096  # a non-null address: validation must answer before anything dereferences or launches
    assert lib.mp_joints_mse_mask_workspace_bytes(32, 17) >= 32 * 17 * 4 and lib.mp_joints_mse_mask_workspace_bytes(0, 17) == 0
    assert lib.mp_ae_loss_workspace_bytes(32) >= 32 * 2 * 8 and lib.mp_ae_loss_workspace_bytes(0) == 0

    def fwd(pred=P, target=P, mask=P, loss=P, ws=P, ws_bytes=1 << 20, n=2, k=3, h=4, w=8, strides=(96, 32, 8, 96, 32, 8), ms=(32, 8)):
        return lib.mp_joints_mse_mask_fwd(pred, *strides[:3], target, *strides[3:], mask, 0, *ms, loss, ws, ws_bytes, n, k, h, w, None)

    for kw in (dict(pred=None), dict(target=None), dict(mask=None), dict(loss=None)):
        assert fwd(**kw) == -1, kw
    for kw in (dict(n=0), dict(k=0), dict(h=0), dict(w=-1), dict(strides=(96, 32, 8, 96, 32, -8)), dict(strides=(96, 32, 4, 96, 32, 8)),
               dict(ms=(32, 4))):
        assert fwd(**kw) == -2, kw
    assert fwd(ws=None) == -5 and fwd(ws_bytes=4) == -5

    def bwd(pred=P, target=P, mask=P, grad=P, n=2, k=3, h=4, w=8, gs=(96, 32, 8)):
        return lib.mp_joints_mse_mask_bwd(pred, 96, 32, 8, target, 96, 32, 8, mask, 1, 32, 8, None, grad, *gs, n, k, h, w, None)

    for kw in (dict(pred=None), dict(target=None), dict(mask=None), dict(grad=None)):
        assert bwd(**kw) == -1, kw
    for kw in (dict(n=0), dict(k=-3), dict(h=0), dict(w=0), dict(gs=(96, 32, 4)), dict(gs=(96, 16, 8)), dict(gs=(64, 32, 8))):
        assert bwd(**kw) == -2, kw

    def ae_fwd(tags=P, ind=P, out=P, ws=P, ws_bytes=1 << 16, n=2, m=3, k=4, hw=16, bs=64):
        return lib.mp_ae_loss_fwd(tags, bs, ind, out, ws, ws_bytes, n, m, k, hw, None)

    for kw in (dict(tags=None), dict(ind=None), dict(out=None)):
        assert ae_fwd(**kw) == -1, kw
    for kw in (dict(n=0), dict(m=0), dict(k=0), dict(hw=0), dict(bs=63)):
        assert ae_fwd(**kw) == -2, kw
    assert ae_fwd(m=257) == _lib.MP_ERR_UNSUPPORTED
    assert ae_fwd(ws=None) == -5 and ae_fwd(ws_bytes=8) == -5

    def ae_bwd(tags=P, ind=P, gout=P, grad=P, n=2, m=3, k=4, hw=16, bs=64, gbs=64):
        return lib.mp_ae_loss_bwd(tags, bs, ind, gout, grad, gbs, n, m, k, hw, None)

    for kw in (dict(tags=None), dict(ind=None), dict(gout=None), dict(grad=None)):
        assert ae_bwd(**kw) == -1, kw
    for kw in (dict(n=0), dict(m=-1), dict(k=0), dict(hw=0), dict(bs=10), dict(gbs=63)):
        assert ae_bwd(**kw) == -2, kw
    assert ae_bwd(m=1000) == _lib.MP_ERR_UNSUPPORTED

    import ctypes
    wh = (ctypes.c_int * 4)(16, 12, 32, 24)

    def tgt(kp=P, counts=P, sizes=wh, target=P, tag=P, n=2, s=2, m=3, k=4, hmax=24, wmax=32, max_num=5, sigma=2.0):
        return lib.mp_bottomup_target(kp, counts, sizes, target, tag, n, s, m, k, hmax, wmax, max_num, 1, sigma, None)

    for kw in (dict(kp=None), dict(counts=None), dict(sizes=None), dict(target=None), dict(tag=None)):
        assert tgt(**kw) == -1, kw
    for kw in (dict(n=0), dict(s=0), dict(m=0), dict(k=0), dict(hmax=0), dict(wmax=0), dict(max_num=0), dict(sigma=0.0),
               dict(wmax=31), dict(hmax=23), dict(sizes=(ctypes.c_int * 4)(16, 0, 32, 24))):
        assert tgt(**kw) == -2, kw
    for kw in (dict(m=257), dict(max_num=300), dict(sigma=1.5)):
        assert tgt(**kw) == _lib.MP_ERR_UNSUPPORTED, kw


def _groups():
    z = np.load(GOLDEN)
    for name in z["names"]:
        name = str(name)
        g = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")}
        target = np.zeros(int(np.prod(g["target_shape"])), np.float32)
        target[g["target_nz_idx"]] = g["target_nz_val"]
        g["target"] = target.reshape(g["target_shape"])
        yield name, float(z["sigma"]), g


def test_fixture_covers_the_listed_cases():
    groups = {name: g for name, _, g in _groups()}
    assert {bool(g["tag_per_joint"]) for g in groups.values()} == {True, False}
    assert groups["recipe_tpj"]["heatmap_sizes"].tolist() == [[128, 128], [256, 256]] and groups["recipe_tpj"]["counts"].max() > 1
    assert any(len({tuple(s) for s in g["heatmap_sizes"].tolist()}) > 1 for g in groups.values())  # padding
    assert all((g["counts"] == 0).any() for name, g in groups.items() if name != "recipe_tpj")  # zero persons
    kp = groups["small_tpj"]["keypoints"]
    assert (kp[..., 2] <= 0).any() and ((kp[..., 0] % 1) == 0.5).any() and (kp[..., 0] < -6).any() and (kp[..., 0] == -1).any()
    assert os.path.getsize(GOLDEN) < (1 << 20)


def test_host_transform_bit_equal_to_reference():
    checked = 0
    for name, sigma, g in _groups():
        t = mp.BottomUpGenerateTarget(is_train=True, config=_cfg(g["heatmap_sizes"], g["tag_per_joint"]), sigma=sigma,
                                      max_num=int(g["max_num"]))
        for i, count in enumerate(g["counts"]):
            out = t.transform(dict(keypoints=[g["keypoints"][i, s, :count] for s in range(g["keypoints"].shape[1])]))
            assert out["target"].dtype == np.float32 and out["tag_ind"].dtype == np.int32
            assert np.array_equal(out["target"].view(np.uint32), g["target"][i].view(np.uint32)), (name, i)
            assert np.array_equal(out["tag_ind"], g["tag_ind"][i]), (name, i)
            checked += 1
    assert checked >= 30
