"""Geometry of the output-column bands a too-wide convolution is cut into (mindpose_amd/models/layers.py `conv_column_bands`,
`deconv_phase_column_bands`), against a brute-force statement of which input columns an output column reads.

Pure arithmetic: the helpers only fill `mp_conv_desc` structures, no library and no GPU.  For every layer width the bottom-up recipe
produces (input widths 512 ... 832 in steps of 64, at scales 1, 1/2, 1/4), some ragged widths, k in {1, 3}, stride in {1, 2}, the
four 2x2 phases of the transposed conv and every band count the plan may try (2 ... 32):
  * the bands tile the output columns [0, wo) exactly once;
  * the input window [start, start + width_in) of a band holds every in-image tap of its output columns, at the position the band's
    descriptor addresses it; what the band's kernel reads outside the window is zero padding of the FULL layer - `pad_left` columns
    on the left (first band only), beyond the right edge only where the full layer pads too;
  * the descriptor passes the inequalities of the library's `validate_desc` / `f16_validate` (csrc/conv_api.hip, csrc/conv_f16.hip);
  * phase px of band column j lands on output column 2 (c0 + j) + px.
"""
import pytest

from mindpose_amd.models.layers import conv_column_bands, deconv_phase_column_bands

RECIPE_WIDTHS = sorted({w // sc for w in range(512, 833, 64) for sc in (1, 2, 4)})
RAGGED_WIDTHS = [193, 250, 385, 417]
WIDTHS = RECIPE_WIDTHS + RAGGED_WIDTHS
BAND_COUNTS = list(range(2, 33))
N, CIN, COUT, H = 2, 5, 7, 6


def _check_desc_inequalities(d):
    """validate_desc (fp32) and f16_validate (fp16), the parts that depend on the band."""
    assert d.n > 0 and d.cin > 0 and d.h > 0 and d.w > 0 and d.cout > 0
    assert d.kh == d.kw and d.kh in (1, 2, 3) and d.stride in (1, 2) and not (d.kh == 2 and d.stride != 1)
    assert 0 <= d.pad_top <= d.kh and 0 <= d.pad_left <= d.kw
    assert d.conv_h > 0 and d.conv_w > 0 and d.out_h > 0 and d.out_w > 0
    assert d.out_mul >= 1 and d.out_rep == 1 and d.out_off_y >= 0 and d.out_off_x >= 0 and d.flags == 0
    assert (d.conv_h - 1) * d.out_mul + d.out_off_y + d.out_rep <= d.out_h
    assert (d.conv_w - 1) * d.out_mul + d.out_off_x + d.out_rep <= d.out_w


def _check_taps(d, start, width_in, w_full, taps_of, out_col_of):
    """Every tap of every band column: band-buffer column j * stride - pad_left + t is input column `taps_of(X)[t]` of the full layer
    when it lies inside the buffer; outside it, the full layer's tap is padding too (left of column 0 / right of column w - 1)."""
    assert 0 <= start and width_in >= 1 and start + width_in <= w_full and d.w == width_in
    for j in range(d.conv_w):
        taps = taps_of(out_col_of(j))
        assert len(taps) == d.kw
        for t, col in enumerate(taps):
            b = j * d.stride - d.pad_left + t  # what the band's kernel addresses
            if 0 <= b < width_in:
                assert start + b == col, (j, t, start, b, col)
            elif b < 0:
                assert col < 0, f"band column {j} tap {t}: the kernel pads on the left where the layer reads column {col}"
            else:
                assert col >= w_full, f"band column {j} tap {t}: the kernel pads on the right where the layer reads column {col}"


@pytest.mark.parametrize("k,s", [(1, 1), (1, 2), (3, 1), (3, 2)])
@pytest.mark.parametrize("w", WIDTHS)
def test_conv_bands_partition_the_output_and_hold_their_taps(k, s, w):
    pad = k // 2
    wo = (w + 2 * pad - k) // s + 1
    ho = (H + 2 * pad - k) // s + 1
    for nb in BAND_COUNTS:
        bands = conv_column_bands(N, CIN, H, w, COUT, k, s, pad, True, nb)
        assert 1 <= len(bands) <= nb
        covered = []
        for start, width_in, d in bands:
            _check_desc_inequalities(d)
            assert (d.n, d.cin, d.h, d.cout, d.kh, d.stride, d.pad_top, d.relu) == (N, CIN, H, COUT, k, s, pad, 1)
            assert (d.conv_h, d.out_h, d.out_w, d.out_mul, d.out_off_y) == (ho, ho, wo, 1, 0)
            assert d.pad_left == (pad if d.out_off_x == 0 else 0), "only the first band keeps the layer's left padding"
            covered += list(range(d.out_off_x, d.out_off_x + d.conv_w))
            # brute force: output column X of the full layer reads input columns X * s - pad + t
            _check_taps(d, start, width_in, w, lambda X: [X * s - pad + t for t in range(k)], lambda j, c0=d.out_off_x: c0 + j)
        assert covered == list(range(wo)), f"w {w} k {k} s {s} nb {nb}: bands do not tile [0, {wo})"
        widths = [d.conv_w for _, _, d in bands]
        assert all(cw == widths[0] for cw in widths[:-1]) and 1 <= widths[-1] <= widths[0]


@pytest.mark.parametrize("py,px", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("w", WIDTHS)
def test_deconv_phase_bands_partition_the_phase_and_hold_their_taps(py, px, w):
    def taps_of(X):
        # Conv2dTranspose(k=4, s=2, p=1): out[X] = sum_i in[i] * W[X + 1 - 2 i]; ascending i = descending kernel index, the order
        # of the phase's 2-tap kernel
        return [i for i in range(X // 2 - 4, X // 2 + 5) if 0 <= X + 1 - 2 * i < 4]

    for nb in BAND_COUNTS:
        bands = deconv_phase_column_bands(N, CIN, H, w, COUT, py, px, True, nb)
        assert 1 <= len(bands) <= nb
        covered = []
        c0 = 0
        for start, width_in, d in bands:
            _check_desc_inequalities(d)
            assert (d.n, d.cin, d.h, d.cout, d.kh, d.stride, d.pad_top, d.relu) == (N, CIN, H, COUT, 2, 1, 1 - py, 1)
            assert (d.conv_h, d.out_h, d.out_w, d.out_mul, d.out_off_y) == (H, 2 * H, 2 * w, 2, py)
            assert d.out_off_x == 2 * c0 + px, "band column j of phase px lands on output column 2 (c0 + j) + px"
            assert d.pad_left == (1 - px if c0 == 0 else 0)
            cols = [d.out_off_x + d.out_mul * j for j in range(d.conv_w)]
            assert cols == [2 * (c0 + j) + px for j in range(d.conv_w)]
            covered += cols
            _check_taps(d, start, width_in, w, taps_of, lambda j, off=d.out_off_x: off + 2 * j)
            c0 += d.conv_w
        assert covered == list(range(px, 2 * w, 2)), f"w {w} phase ({py}, {px}) nb {nb}: bands do not tile the phase's columns"


def test_the_widths_cover_the_recipe():
    assert RECIPE_WIDTHS[0] == 128 and RECIPE_WIDTHS[-1] == 832 and {208, 416, 176, 352, 704} <= set(RECIPE_WIDTHS)
