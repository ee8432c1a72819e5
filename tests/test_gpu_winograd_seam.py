"""GPU parity of the fp32 Winograd kernel (csrc/conv_wino_f32.hip) across the seam between two tiles of one workgroup.

In the one-team form with an even chunk count the staging slots of a tile's last two chunks carry chunks 0 and 1 of the workgroup's
NEXT tile, its first U fragments ride in the last chunk's refill slot, and the tile's coordinates switch inside the chunk loop; odd
chunk counts and the two-team forms keep the per-tile prologue.  `MP_WINO_TILES=1` makes every tile a workgroup's first one -
nothing crosses a seam - so it is the reference form here: a launch that walks 2, 3, 8 or the default number of tiles per workgroup computes the same chunk-ordered sums through the
same output transform and must agree with it BIT FOR BIT (`torch.equal`), for one team and, where a second team has output
channels to compute, for two.  Every form is also held to the fp64 bar of tests/test_gpu_winograd.py (normalised max error <= 2e-5),
and output buffers start as NaN: every element has to be written.

The shapes are the smallest at which a seam can go wrong (each launch is far below a millisecond)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_gpu_winograd_forms import _operands, _winograd  # noqa: E402

CASES = [
    # n, cin, cout, h, w
    (1, 64, 32, 64, 48),   # the headline row geometry (16 bands of 4 rows, QROW, three staging units per thread): consecutive tiles
                           # go from the image top through the interior to the bottom - stale halo rows must come back as zeros;
                           # 8 tiles per workgroup: two workgroups
    (3, 32, 32, 12, 16),   # one band per image: the next tile is another image; the last workgroup is short
    (2, 8, 32, 16, 16),    # one chunk (odd: per-tile prologue); the second band is partial (H % R != 0, no QROW)
    (2, 16, 64, 8, 8),     # two chunks - both are "the last two"; two teams possible
    (2, 24, 40, 20, 8),    # odd chunk count; the cout tile changes inside a workgroup's run and its second half is empty
    (2, 64, 64, 32, 24),   # the two-team QROW form with two tiles per workgroup: the headline's 64-channel layout
    (5, 32, 64, 8, 6),     # image-grouped bands, four chunks; the last group is clipped to one image
    (3, 8, 16, 4, 10),     # image-grouped bands, one chunk; the group is clipped to the batch
]
EPILOGUES = {"res_relu": (True, True, True), "plain": (False, False, False)}  # relu, res1, res2
TILES = (2, 3, 8, None)  # against MP_WINO_TILES=1; None: the launch's own choice


@functools.lru_cache(maxsize=None)
def _case_operands(case):
    """Operands and the fp64 reference of one (shape, epilogue) case: computed once, shared by the one- and two-team tests."""
    return _operands(case)


def _params():
    for shape in CASES:
        for ep_name, ep in EPILOGUES.items():
            for teams in (1, 2):
                if teams == 2 and shape[2] <= 32:  # a second team would have no output channel
                    continue
                yield pytest.param(shape + ep, teams, id=f"n{shape[0]}_{shape[1]}to{shape[2]}_{shape[3]}x{shape[4]}-{ep_name}-teams{teams}")


@pytest.mark.parametrize("case,teams", list(_params()))
def test_tiles_after_a_seam_are_bit_equal_to_first_tiles_and_within_fp64_bar(case, teams, monkeypatch):
    ops = _case_operands(case)
    ref = ops[-1]
    span = float(ref.abs().max())
    first = _winograd(case, ops, monkeypatch, MP_WINO_TEAMS=teams, MP_WINO_TILES=1)
    outs = {1: first}
    for tiles in TILES:
        outs[tiles] = _winograd(case, ops, monkeypatch, MP_WINO_TEAMS=teams, MP_WINO_TILES=tiles)
    errs = {}
    for tiles, out in outs.items():
        assert torch.isfinite(out).all(), f"MP_WINO_TILES={tiles}: an output element was not written (or is not finite)"
        errs[tiles] = float((out.double().cpu() - ref).abs().max()) / span
    print("normalised max error vs fp64 per MP_WINO_TILES: " + ", ".join(f"{t}: {e:.3e}" for t, e in errs.items()))
    assert all(e <= 2e-5 for e in errs.values()), errs
    for tiles in TILES:
        assert torch.equal(first, outs[tiles]), f"MP_WINO_TILES={tiles} differs from MP_WINO_TILES=1"
