"""tests/bn_matrix.py checked without a GPU: every row takes the form and meets the conditions it is listed for, the slice
enumerators partition the tensor, the multiply-high division the kernels index with is exact wherever their own condition says so,
and the knob-shaped rows produce the stated batches and empty chunks."""
import random

import pytest
import torch

from tests import bn_matrix as bm


@pytest.mark.parametrize("shape,props", bm.REDUCING_ROWS, ids=[bm.row_id(s) for s, _ in bm.REDUCING_ROWS])
def test_reducing_row_reaches_what_it_is_listed_for(shape, props):
    n, c, hw = shape
    c8 = bm.c8_of(c)
    assert bm.form(n, c, hw) == props["form"]
    assert 8 * n * c8 * hw * 2 <= 19 * 2 ** 20  # the largest tensor is 18 MB of fp16
    if "c8" in props:
        assert c8 == props["c8"]
    if "exact" in props:
        assert bm.apply_exact(n, hw) == props["exact"]
        assert c8 >= 2  # a wrong image index is invisible with one channel block (img_extra == 0)
    if props.get("near_bound"):
        assert bm.apply_exact(n, hw) and not bm.apply_exact(n + 1, hw)
    if "pad" in props:
        assert c8 * 8 - c == props["pad"]
    if props.get("hw1"):
        assert hw == 1
    if props.get("odd_hw"):
        assert hw % 2 == 1
    if props["form"] == "coop":
        ns = bm.coop_plan(n, c8, hw)
        assert n * c8 * hw <= bm.COOP_MAX_ELEMS and c8 <= bm.COOP_MAX_GRID
        if "nsplit" in props:
            assert ns == props["nsplit"]
        if "slice_len" in props:
            assert bm.ceil_div(n * hw, ns) == props["slice_len"]
        if props.get("straddles"):
            assert ns & (ns - 1) != 0
            idx = [bm.coop_slice(n, hw, ns, sp) for sp in range(ns)]
            assert sum(int(i[0]) // hw != int(i[-1]) // hw for i in idx) >= n - 1  # slices that hold two images' pixels
    else:
        gi, gp = bm.split(n, c8, hw)
        assert 1 <= gi * gp <= bm.MAX_SPLIT
        if "gi" in props:
            assert (gi, gp) == (props["gi"], props["gp"])
        if "chunk" in props:
            chunk = bm.ceil_div(hw, gp)
            assert chunk == props["chunk"] and hw - (gp - 1) * chunk == props["last"] and props["last"] < chunk
        if "two_images" in props:  # n > gi: the first n - gi image groups take two images
            assert n > gi and sum(len(range(ig, n, gi)) == 2 for ig in range(gi)) == props["two_images"]
        if "apply_len" in props:
            assert bm.ceil_div(n * hw, bm.apply_chunks(n, c8, hw)) == props["apply_len"]
        if props.get("under_threshold"):  # small enough for the one-launch form: only c8 > 128 keeps it out
            assert n * c8 * hw <= bm.COOP_MAX_ELEMS and c8 > bm.COOP_MAX_GRID
        if props.get("hw1"):  # len <= 1 branch of bn16_reduce_kernel: one pixel per chunk
            assert gp == 1 and bm.ceil_div(hw, gp) <= 1
        # bn16_reduce_kernel's own multiply-high condition holds on every row (its `e / len` fallback needs len^2 * images >= 2^32)
        for sp in range(gi * gp):
            ln = min(bm.ceil_div(hw, gp), hw - (sp // gi) * bm.ceil_div(hw, gp))
            assert ln * ln * len(range(sp % gi, n, gi)) < 2 ** 32


def test_reducing_table_meets_every_condition():
    rows = dict(bm.REDUCING_ROWS)
    forms = {p["form"] for p in rows.values()}
    assert forms == {"coop", "two"}
    for f in forms:  # both sides of the exact / non-exact division, with c8 >= 2, in both forms
        assert {p["exact"] for p in rows.values() if p["form"] == f and "exact" in p} == {True, False}
    c8s = {bm.c8_of(c) for (_, c, _) in rows}
    assert {127, 128, 129} <= c8s
    assert any(p.get("hw1") for p in rows.values() if p["form"] == "coop") and any(p.get("hw1") for p in rows.values() if p["form"] == "two")
    assert {p["pad"] for p in rows.values() if "pad" in p} >= {4, 7}
    ns = [bm.nsplit16(*s) for s, p in bm.REDUCING_ROWS if p["form"] == "coop"]
    assert len(set(ns)) >= 3  # barrier slots are reused across launches of different grid sizes
    assert all(s in rows for s in bm.ILL_ROWS) and {rows[s]["form"] for s in bm.ILL_ROWS} == {"coop", "two"}
    assert bm.F32_ILL_ROW in dict(bm.F32_ROWS)


@pytest.mark.parametrize("shape,n_parts,knobs,props", bm.APPLY_ROWS, ids=[bm.row_id(r[0], f"p{r[1]}", *r[2].values()) for r in bm.APPLY_ROWS])
def test_apply_only_row_reaches_what_it_is_listed_for(shape, n_parts, knobs, props):
    n, c, hw = shape
    c8 = bm.c8_of(c)
    blocks, floor = bm.pre_knobs(knobs)
    chunks = bm.pre_chunks(n, c8, hw, blocks, floor)
    ranges = bm.chunk_ranges(n * hw, chunks)
    assert ranges[0][0] == 0 and max(e1 for e0, e1 in ranges if e1 > e0) == n * hw
    assert all(a[1] == b[0] or b[0] >= n * hw for a, b in zip(ranges, ranges[1:]))
    if "fold" in props:
        assert bm.prefold(n_parts, int(knobs.get("MP_BN_PREFOLD_ABOVE", bm.MAX_FOLD_PARTS)))[0] == props["fold"]
    if "exact" in props:
        assert bm.apply_exact(n, hw) == props["exact"] and c8 >= 2
    if "chunks" in props:
        assert chunks == props["chunks"]
    if "chunk_len" in props:
        assert bm.ceil_div(n * hw, chunks) == props["chunk_len"]
    if "batches" in props:  # the prefetch loop: `more` true on all but the last batch, which is partially filled
        assert bm.batches(*ranges[0]) == props["batches"]
    if "empty" in props:
        assert sum(e0 >= n * hw for e0, _ in ranges) == props["empty"]


def test_apply_only_table_meets_every_condition():
    small = [r for r in bm.APPLY_ROWS if r[0] == (6, 17, 48) and not r[2]]
    assert [r[1] for r in small] == [1, 63, 64, 65, 511, 512, 513, 4097]
    # at the shapes the older tests use, every chunk is one batch; the table has two- and three-batch chunks
    assert {len(r[3]["batches"]) for r in bm.APPLY_ROWS if "batches" in r[3]} == {1, 2, 3}
    assert any(r[2].get("MP_BN_PREFOLD_ABOVE") == "4" and r[1] == 37 for r in bm.APPLY_ROWS)
    # fold launch: the slot ranges cover every slot once; 513 and 4097 leave a short last range
    for n_parts in (5, 37, 513, 4097, 4096):
        got = [s for s0, s1 in bm.fold_ranges(n_parts) for s in range(s0, s1)]
        assert got == list(range(n_parts))
    assert bm.fold_ranges(513)[-1] == (455, 513) and bm.fold_ranges(4097)[-1] == (3591, 4097)
    assert bm.fold_ranges(37)[-1] == (35, 37) and all(s0 == s1 for s0, s1 in bm.fold_ranges(5)[5:])
    assert len(bm.GROUPED_JOBS) == 4 and len({s for s, _ in bm.GROUPED_JOBS}) == 4
    assert sum(bm.prefold(k)[0] for _, k in bm.GROUPED_JOBS) == 1


@pytest.mark.parametrize("shape,props", bm.F32_ROWS, ids=[bm.row_id(s) for s, _ in bm.F32_ROWS])
def test_f32_row_reaches_what_it_is_listed_for(shape, props):
    n, c, hw = shape
    assert (hw % 4 == 0) == props["float4"]
    per_trip = 1024 if props["float4"] else 256
    assert bm.ceil_div(hw, per_trip) == props["trips"]
    if not props["float4"]:
        assert hw > 256  # no hw % 4 != 0 plane of the older tests exceeds one trip
    if "two_images" in props:
        assert n > bm.BN_SPLIT and sum(len(range(sp, n, bm.BN_SPLIT)) == 2 for sp in range(bm.BN_SPLIT)) == props["two_images"]
    if props.get("idle_threads"):
        assert hw // 4 < 256 and hw < 256


def _assert_partition(slices, total):
    got = torch.cat(slices)
    assert got.numel() == total and torch.equal(torch.sort(got).values, torch.arange(total))


def test_slices_partition_the_tensor():
    """every (image, pixel) of a channel block lands in exactly one slot, on the rows and on 500 random shapes per form"""
    for (n, c, hw), _ in bm.REDUCING_ROWS:
        _assert_partition(bm.slices16(n, c, hw), n * hw)
    for (n, c, hw), _ in bm.F32_ROWS:
        _assert_partition(bm.slices32(n, hw), n * hw)
    rng = random.Random(5)
    seen = {"coop": 0, "two": 0, "f32": 0}
    while min(seen.values()) < 500:
        n, c8, hw = rng.randint(1, 70), rng.choice([1, 2, 3, 5, 17, 64, 127, 128, 129, 200]), rng.choice([1, 2, 7, 63, 255, 256, 257, 919, 3000])
        hw = hw if rng.random() < 0.5 else rng.randint(1, 4000)
        ns = bm.coop_plan(n, c8, hw)
        if ns is not None and seen["coop"] < 500:
            assert 1 <= ns <= 32 and ns * c8 <= bm.COOP_MAX_GRID
            _assert_partition([bm.coop_slice(n, hw, ns, sp) for sp in range(ns)], n * hw)
            seen["coop"] += 1
        if seen["two"] < 500:  # the two-launch geometry is defined for every shape (the capture-time fallback takes it)
            gi, gp = bm.split(n, c8, hw)
            assert 1 <= gi * gp <= bm.MAX_SPLIT
            _assert_partition([bm.two_slice(n, hw, gi, gp, sp) for sp in range(gi * gp)], n * hw)
            seen["two"] += 1
        if seen["f32"] < 500:
            _assert_partition(bm.slices32(n, hw), n * hw)
            seen["f32"] += 1


def _assert_mulhi(d, count):
    """the kernels' division of e in [0, count) by d: exact whenever count * d < 2^32 (their `exact` condition)"""
    assert count * d < 2 ** 32 and d > 1
    probes = {count - 1}
    for k in {1, 2, 3, count // d, max(count // d - 1, 1), max(count // (2 * d), 1)}:
        probes.update((k * d - 1, k * d))
    for e in probes:
        if 0 <= e < count:
            assert bm.mulhi_div(e, d) == e // d, (e, d, count)


def test_multiply_high_division_is_exact_under_the_kernels_condition():
    for shape in [s for s, _ in bm.REDUCING_ROWS] + [r[0] for r in bm.APPLY_ROWS]:
        n, c, hw = shape
        if hw > 1 and bm.apply_exact(n, hw):  # the apply / one-launch kernels divide by hw
            _assert_mulhi(hw, n * hw)
        if bm.form(n, c, hw) == "two":  # bn16_reduce_kernel divides by the chunk length
            gi, gp = bm.split(n, bm.c8_of(c), hw)
            chunk = bm.ceil_div(hw, gp)
            for ln in {chunk, hw - (gp - 1) * chunk}:
                if ln > 1:
                    _assert_mulhi(ln, ln * bm.ceil_div(n, gi))
    rng = random.Random(11)
    for i in range(2000):
        d = rng.randint(2, 70000) if i % 2 else rng.choice([2, 3, 255, 256, 257, 12288, 24576, 49152, 65535, 65536, 65537])
        top = (2 ** 32 - 1) // d  # the largest count with count * d < 2^32
        count = top - rng.randint(0, 3) if i % 4 < 2 else rng.randint(1, top)
        if count >= 1:
            _assert_mulhi(d, count)
    # ... and the fallback is needed: on a non-exact row the multiply-high quotient is wrong inside the tensor
    n, c, hw = 6, 32, 49152
    assert not bm.apply_exact(n, hw) and any(bm.mulhi_div(k * hw - 1, hw) != k - 1 for k in range(1, n + 1))


def test_reference_matches_torch_batch_norm():
    """the float64 reference against torch's own batch_norm and autograd (float64) on a small shape"""
    import torch.nn.functional as F
    inp = bm.make_inputs((3, 5, 14))
    z, gamma, beta = inp["z"].clone().requires_grad_(True), inp["gamma"].clone().requires_grad_(True), inp["beta"].clone().requires_grad_(True)
    res = inp["res"].clone().requires_grad_(True)
    mm, mv = inp["mm"].clone(), inp["mv"].clone()
    ref = bm.forward_ref(inp["z"], inp["gamma"], inp["beta"], inp["res"], 1, inp["mm"], inp["mv"])
    y = F.relu(F.batch_norm(z, mm, mv, gamma, beta, training=True, momentum=1.0 - ref["mom"], eps=ref["eps"]) + res)
    assert torch.allclose(ref["y"], y.detach(), rtol=1e-12, atol=1e-12)
    assert torch.allclose(ref["mm"], mm, rtol=1e-12) and torch.allclose(ref["mv"], mv, rtol=1e-12)
    y.backward(inp["dy"])
    back = bm.backward_ref(inp["dy"], inp["z"], ref["y"], inp["gamma"], ref["mean"], ref["invstd"], 1)
    assert torch.allclose(back["dz"], z.grad, rtol=1e-10, atol=1e-12) and torch.allclose(back["g"], res.grad)
    assert torch.allclose(back["dgamma"], gamma.grad, rtol=1e-10) and torch.allclose(back["dbeta"], beta.grad, rtol=1e-10)
    # the slot sums add up to the channel sums, on a form of each kind; the c8 packing round-trips
    for shape in [(7, 40, 919), (40, 136, 800)]:
        zz = bm.make_inputs(shape)["z"]
        assert torch.allclose(bm.slot_sums(zz, bm.slices16(*shape)).sum(dim=1), zz.sum(dim=(0, 2)), rtol=1e-12, atol=1e-9)
    packed = bm.pack_c8(inp["z"])
    back_z, pad = bm.unpack_c8(packed, 5)
    assert torch.equal(back_z, inp["z"]) and packed.shape == (3, 1, 14, 8) and (pad == torch.tensor(float("nan")).half().view(torch.int16)).all()
    p = bm.spread_partials(inp["z"].sum(dim=(0, 2)), (inp["z"] ** 2).sum(dim=(0, 2)), 5, 65, seed=1)
    tot, mag = bm.partial_totals(p, 5)
    assert p.shape == (1, 65, 8, 2) and ((tot[:, 0] - inp["z"].sum(dim=(0, 2))).abs() <= bm.U32 * mag[:, 0]).all()
