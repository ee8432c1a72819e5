"""The top-down decode, target and loss entries give the bits of the commit their kernels were merged from.

tests/pose_loss_bits.py runs every decode case of tests/pose_matrix.py through mp_decode_topdown, mp_decode_topdown_debug and
mp_flip_aggregate_decode, every target case through mp_gaussian_target, every loss size through mp_joints_mse_fwd / _bwd and
mp_joints_ohkm_fwd / _bwd, the masked MSE on its three views under four mask kinds and the AE loss on its random cases.
tests/golden/pose_loss_bits.json holds the SHA-256 of every output (for an output with NaNs: the digest of the other values and the
index runs of the NaNs), recorded by tests/golden/gen_pose_loss_bits.py on the GPU FROM THE PARENT COMMIT'S LIBRARY: a changed
association, contraction or path predicate inside a folded kernel changes a digest.  logf runs on the device, so for the DARK terms
this is the only pin to the bit.

One case is outside the digests because it pins a behaviour the parent did not have: test_mse_on_a_misaligned_base.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import pose_matrix as pm

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from mindpose_amd import _lib  # noqa: E402
from tests import pose_loss_bits  # noqa: E402

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_loss_bits.json")) as _f:
    GOLDEN = json.load(_f)


def test_every_group_is_recorded():
    assert sorted(GOLDEN) == sorted(pose_loss_bits.GROUPS)
    assert len(pose_loss_bits.GROUPS) == len(pm.DECODE_MAPS) * len(pm.REFINE_FORMS) + len(pm.TARGET_CASES) + len(pm.MSE_HW_SCALAR + pm.MSE_HW_QUAD) + 3 + 1
    for group, rec in GOLDEN.items():
        if group.startswith("decode/"):
            assert set(rec) == {"preds", "boxes", "argmax", "avg_out"} | ({"dark_terms"} if "/dark" in group else set()), group
        if group.startswith("loss/"):
            assert set(rec) == {"mse_loss", "mse_partial", "mse_grad", "ohkm_loss", "ohkm_row_sum", "ohkm_sel", "ohkm_grad"}, group
            assert rec["ohkm_row_sum"] == rec["mse_partial"], group  # one row pass: the parent kept this equality by copy-paste


@pytest.mark.parametrize("group", pose_loss_bits.GROUPS)
def test_bits_equal_parent(group):
    got = pose_loss_bits.digest(group)
    assert sorted(got) == sorted(GOLDEN[group]), group
    for name in got:
        assert got[name] == GOLDEN[group][name], f"{group}: {name}"
    if group.startswith("loss/"):
        assert got["ohkm_row_sum"] == got["mse_partial"], group


@pytest.mark.parametrize("hw", [v for v in pm.MSE_HW_QUAD if v >= 252])
def test_mse_on_a_misaligned_base(hw):
    """Plain MSE with hw % 4 == 0 on bases 4 bytes past a 16-byte boundary takes the scalar loop: forward and backward equal the
    scalar-path restatement bit for bit, and the OHKM row sums are the same bits.  The library this change started from took the
    16-byte path on hw % 4 == 0 alone and read such a base through a misaligned float4 pointer, adding in the quad path's order; the
    restated quad-path sums differ from the scalar-path ones in some row of these inputs, which is asserted first."""
    lib = _lib.load()
    rows, (n, k) = 600, pm.MSE_ROWS[600]
    pred, target, w = pm.mse_inputs(hw, rows, "mix")
    want_rows = pm.mse_rows_restated(pred, target, w, "scalar")
    assert (want_rows.view(np.uint32) != pm.mse_rows_restated(pred, target, w, "quad").view(np.uint32)).any()

    def shifted(a):
        buf = torch.empty(a.size + 4, dtype=torch.float32, device="cuda:0")
        assert buf.data_ptr() % 16 == 0
        view = buf[1:1 + a.size]
        view.copy_(torch.from_numpy(a.reshape(-1)))
        assert view.data_ptr() % 16 == 4
        return view

    tp, tt, tw = shifted(pred), shifted(target), torch.from_numpy(w).cuda()
    ws_bytes = lib.mp_joints_mse_workspace_bytes(n, k)
    ws = torch.full((ws_bytes // 4,), float("nan"), device="cuda:0")
    loss = torch.full((1,), float("nan"), device="cuda:0")
    _lib.check(lib.mp_joints_mse_fwd(tp.data_ptr(), tt.data_ptr(), tw.data_ptr(), loss.data_ptr(), ws.data_ptr(), ws_bytes, n, k, hw, _lib.stream()),
               "mp_joints_mse_fwd")
    got_rows = ws[:rows].cpu().numpy()
    assert np.array_equal(got_rows.view(np.uint32), want_rows.view(np.uint32)), (got_rows, want_rows)
    want = pm.mse_fwd_restated(pred, target, w, "scalar")
    assert loss.cpu().numpy().view(np.uint32)[0] == np.float32(want).view(np.uint32), (float(loss), float(want))
    # OHKM on the same bases: the same row sums
    ows_bytes = lib.mp_joints_ohkm_workspace_bytes(n, k)
    ows = torch.zeros(ows_bytes // 8, dtype=torch.float64, device="cuda:0")
    row_sum = torch.full((rows,), float("nan"), device="cuda:0")
    sel = torch.zeros(rows, dtype=torch.uint8, device="cuda:0")
    _lib.check(lib.mp_joints_ohkm_fwd(tp.data_ptr(), tt.data_ptr(), tw.data_ptr(), loss.data_ptr(), row_sum.data_ptr(), sel.data_ptr(), ows.data_ptr(),
                                      ows_bytes, n, k, hw, 3, _lib.stream()), "mp_joints_ohkm_fwd")
    assert np.array_equal(row_sum.cpu().numpy().view(np.uint32), want_rows.view(np.uint32))
    # backward into a misaligned gradient: the element-wise result does not depend on the path, every element is written
    grad = torch.full((rows * hw + 4,), float("nan"), device="cuda:0")
    gview = grad[1:1 + rows * hw]
    g = torch.tensor([0.375], dtype=torch.float32, device="cuda:0")
    _lib.check(lib.mp_joints_mse_bwd(tp.data_ptr(), tt.data_ptr(), tw.data_ptr(), g.data_ptr(), gview.data_ptr(), n, k, hw, _lib.stream()),
               "mp_joints_mse_bwd")
    want_grad = pm.mse_bwd_restated(pred, target, w, 0.375)
    assert np.array_equal(gview.cpu().numpy().view(np.uint32), want_grad.reshape(-1).view(np.uint32))
    edge = grad.cpu().numpy()
    assert np.isnan(edge[0]) and np.isnan(edge[1 + rows * hw:]).all()  # nothing outside the rows was written
