"""Every form of the training BatchNorm kernels (csrc/train_ops.hip) against a float64 reference, through the C ABI.

The rows of tests/bn_matrix.py choose the form by shape: the one-launch form (bn16_coop_kernel), the two-launch form
(bn16_reduce_kernel + bn16_apply_kernel / bn16_bwd_apply_kernel), the apply-only form on given partial slots (bn16_apply_pre_*,
bn16_bwd_apply_pre_*, bn16_fold_kernel, bn16_finalize_kernel) and the fp32 pair.  A reducing call is checked slot by slot: the fp64
partials it leaves in the workspace are exactly the restated c x nsplit x 2 (which proves the form and the split), and each equals
the float64 sum over its restated slice.  Tolerances (tests/bn_matrix.py): fp16 tensors 2^-9 |ref| + 2e-4 max |ref|; dgamma / dbeta
1e-4 max |ref|; slots (k + 6) 2^-24 sum |terms| for a chain of k fp32 terms; statistics from the slot bounds.  Every test prints the
measured maximum of each quantity as a fraction of its bound (pytest -s).
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from mindpose_amd import _lib  # noqa: E402
from mindpose_amd.models.act_c8 import ActC8  # noqa: E402
from tests import bn_matrix as bm  # noqa: E402

DEV = torch.device("cuda:0")
LIB = _lib.load()
GUARD = 64                 # sentinel elements on either side of every output
SENT16, SENT32 = 1234.0, -777.0
NAN_BITS = torch.tensor([float("nan")], dtype=torch.float64).view(torch.int64).item()
P = _lib.ptr


class Guarded:
    """an output buffer between two sentinel guards, itself pre-filled with the sentinel (whatever stays unwritten shows)"""

    def __init__(self, shape, dtype):
        self.numel = 1
        for s in shape:
            self.numel *= s
        self.fill = SENT16 if dtype == torch.float16 else SENT32
        self.buf = torch.full((self.numel + 2 * GUARD,), self.fill, dtype=dtype, device=DEV)
        self.t = self.buf[GUARD:GUARD + self.numel].view(shape)

    def intact(self):
        return bool((self.buf[:GUARD] == self.fill).all()) and bool((self.buf[GUARD + self.numel:] == self.fill).all())


def _act(x):
    """float64 [n, c, hw] -> channel-blocked fp16 activation on the device, NaN in the padding-channel lanes"""
    n, c, hw = x.shape
    a = ActC8(n, c, hw, 1, DEV)
    a.c8_tensor.copy_(bm.pack_c8(x).reshape(a.c8_tensor.shape))
    return a


def _vec(x):
    return x.float().to(DEV).contiguous()


def _workspace(c):
    nb = LIB.mp_bn_workspace_bytes(c)
    return torch.full((nb // 8 + 1,), float("nan"), dtype=torch.float64, device=DEV), nb


def _untouched(ws, first):
    """everything from double `first` on still holds the NaN fill, bit for bit"""
    return bool((ws[first:].view(torch.int64) == NAN_BITS).all())


def _frac(diff, bound):
    """max |diff| / bound; a zero bound admits only a zero difference"""
    diff, bound = diff.abs().double(), bound.double()
    assert not (diff[bound == 0] > 0).any()
    return float((diff / bound.clamp_min(1e-300)).max())


def _report(what, **fracs):
    print("BN-FRACTION " + what + " " + " ".join(f"{k}={v:.3f}" for k, v in fracs.items()))
    for k, v in fracs.items():
        assert v <= 1.0, f"{what}: {k} at {v:.3f} of its bound"


def _out16(g, c):
    """Guarded c8 output -> (float64 [n, c, hw], padding lanes all zero bits)"""
    t = g.t.cpu()
    val, pad = bm.unpack_c8(t.reshape(t.shape[0], t.shape[1], -1, 8), c)
    return val, bool((pad == 0).all())


@functools.lru_cache(maxsize=1)
def _row(shape, ill):
    """inputs, slices and the mode-independent forward slot sums of a reducing row: computed once, shared, never modified"""
    inp = bm.make_inputs(shape, ill)
    sl = bm.slices16(*shape)
    z = inp["z"]
    fw = dict(s0=bm.slot_sums(z, sl), s1=bm.slot_sums(z * z, sl), b0=bm.slot_bounds(z, sl), b1=bm.slot_bounds(z * z, sl))
    dev = dict(z=_act(z), res=_act(inp["res"]), dy=_act(inp["dy"]), gamma=_vec(inp["gamma"]), beta=_vec(inp["beta"]))
    return inp, sl, fw, dev


def _fwd16(shape, dev, with_res, relu, mm, mv, ws, nb):
    n, c, hw = shape
    c8 = bm.c8_of(c)
    out = dict(y=Guarded((n, c8, hw, 8), torch.float16), mean=Guarded((c,), torch.float32), invstd=Guarded((c,), torch.float32),
               mm=Guarded((c,), torch.float32), mv=Guarded((c,), torch.float32))
    out["mm"].t.copy_(mm.float())
    out["mv"].t.copy_(mv.float())
    _lib.check(LIB.mp_f16_bn_train_fwd(P(dev["z"]), P(dev["gamma"]), P(dev["beta"]), P(dev["res"]) if with_res else None, P(out["y"].t),
                                       P(out["mean"].t), P(out["invstd"].t), P(out["mm"].t), P(out["mv"].t), n, c, hw, bm.EPS, bm.MOMENTUM,
                                       relu, P(ws), nb, _lib.stream()), "bn fwd")
    return out


def _bwd16(shape, dev, y, mean, invstd, with_res, relu, ws, nb):
    n, c, hw = shape
    c8 = bm.c8_of(c)
    out = dict(dz=Guarded((n, c8, hw, 8), torch.float16), dres=Guarded((n, c8, hw, 8), torch.float16) if with_res else None,
               dgamma=Guarded((c,), torch.float32), dbeta=Guarded((c,), torch.float32), acc_g=Guarded((c,), torch.float32),
               acc_b=Guarded((c,), torch.float32))
    out["acc_g"].t.fill_(1.0)
    out["acc_b"].t.fill_(2.0)
    _lib.check(LIB.mp_f16_bn_train_bwd(P(dev["dy"]), P(dev["z"]), P(y), P(dev["gamma"]), P(dev["beta"]), P(mean), P(invstd), P(out["dz"].t),
                                       P(out["dres"].t) if with_res else None, P(out["dgamma"].t), P(out["dbeta"].t), P(out["acc_g"].t),
                                       P(out["acc_b"].t), n, c, hw, relu, P(ws), nb, _lib.stream()), "bn bwd")
    return out


def _same(a, b):
    return all(torch.equal(a[k].buf, b[k].buf) for k in a if a[k] is not None)


@functools.lru_cache(maxsize=2)
def _interloper(shape):
    inp = bm.make_inputs(shape)
    dev = dict(z=_act(inp["z"]), res=None, dy=_act(inp["dy"]), gamma=_vec(inp["gamma"]), beta=_vec(inp["beta"]))
    ws, nb = _workspace(shape[1])
    return inp, dev, ws, nb


def _run_interloper(row):
    """another one-launch row of another grid size (nsplit 25, or 1 for the nsplit-25 row itself), launched between two identical
    launches of a one-launch row on the same stream: the barrier slots must come back clean for any grid size"""
    shape = (7, 40, 919) if row != (7, 40, 919) else (5, 12, 63)
    assert bm.form(*shape) == "coop" and bm.form(*row) == "coop" and bm.nsplit16(*shape) != bm.nsplit16(*row)
    inp, dev, ws, nb = _interloper(shape)
    f = _fwd16(shape, dev, 0, 1, inp["mm"], inp["mv"], ws, nb)
    _bwd16(shape, dev, f["y"].t, f["mean"].t, f["invstd"].t, 0, 1, ws, nb)


_REDUCING = [(s, m, False) for s, _ in bm.REDUCING_ROWS for m in bm.MODES] + [(s, (1, 0), True) for s in bm.ILL_ROWS]


@pytest.mark.parametrize("shape,mode,ill", _REDUCING, ids=[bm.row_id(s, f"relu{m[0]}res{m[1]}", *(["ill"] if i else [])) for s, m, i in _REDUCING])
def test_reducing_entries_vs_float64(shape, mode, ill):
    n, c, hw = shape
    relu, with_res = mode
    c8, count = bm.c8_of(c), n * hw
    inp, sl, fw, dev = _row(shape, ill)
    ns = bm.nsplit16(n, c, hw)
    coop = bm.form(n, c, hw) == "coop"
    tag = bm.row_id(shape, bm.form(n, c, hw), f"relu{relu}res{with_res}", *(["ill"] if ill else []))
    z, gamma, beta = inp["z"], inp["gamma"], inp["beta"]
    res = inp["res"] if with_res else None
    ref = bm.forward_ref(z, gamma, beta, res, relu, inp["mm"], inp["mv"])

    # ---- forward
    ws, nb = _workspace(c)
    f1 = _fwd16(shape, dev, with_res, relu, inp["mm"], inp["mv"], ws, nb)
    part = ws[:c * ns * 2].cpu().reshape(c, ns, 2)
    assert torch.isfinite(part).all() and _untouched(ws, c * ns * 2), "the partial slots are not the restated c x nsplit x 2"
    if coop:
        _run_interloper(shape)
    f2 = _fwd16(shape, dev, with_res, relu, inp["mm"], inp["mv"], ws, nb)
    assert _same(f1, f2), "a second identical forward launch differs"
    assert all(g.intact() for g in f1.values()), "forward wrote outside an output"
    mean_k, inv_k = f1["mean"].t.cpu().double(), f1["invstd"].t.cpu().double()
    dmean, dvar, dinv = bm.stat_bounds(z, fw["b0"].sum(dim=1), fw["b1"].sum(dim=1), ref)
    unbiased = ref["var"] * count / (count - 1) if count > 1 else ref["var"]
    dunb = dvar * (count / (count - 1) if count > 1 else 1.0) + bm.U32 * unbiased
    assert (1.0 / inv_k ** 2 - ref["eps"] > 0).all(), "the variance clamp fired"
    y_k, pad_ok = _out16(f1["y"], c)
    assert pad_ok, "padding lanes of y are not zero"
    y_ref = bm.forward_ref(z, gamma, beta, res, relu, inp["mm"], inp["mv"], stats=(mean_k, inv_k))["y"] if ill else ref["y"]
    _report(tag + " fwd",
            slot_sum=_frac(part[..., 0] - fw["s0"], fw["b0"]), slot_sumsq=_frac(part[..., 1] - fw["s1"], fw["b1"]),
            mean=_frac(mean_k - ref["mean"], dmean), invstd=_frac(inv_k / ref["invstd"] - 1.0, dinv),
            moving_mean=_frac(f1["mm"].t.cpu().double() - ref["mm"], bm.moving_bound(ref, inp["mm"], ref["mm"], dmean)),
            moving_var=_frac(f1["mv"].t.cpu().double() - ref["mv"], bm.moving_bound(ref, inp["mv"], ref["mv"], dunb)),
            y=_frac(y_k - y_ref, bm.tol16(y_ref)))

    # ---- backward, independent of the kernel's forward: the reference's y (as fp16) and statistics (as fp32) go in
    y_given = ref["y"].half().double()
    mean32, inv32 = ref["mean"].float(), ref["invstd"].float()
    back = bm.backward_ref(inp["dy"], z, y_given, gamma, mean32.double(), inv32.double(), relu)
    y_dev, mean_dev, inv_dev = (_act(y_given) if relu else None), mean32.to(DEV), inv32.to(DEV)
    ws.fill_(float("nan"))
    b1 = _bwd16(shape, dev, y_dev, mean_dev, inv_dev, with_res, relu, ws, nb)
    part = ws[:c * ns * 2].cpu().reshape(c, ns, 2)
    assert torch.isfinite(part).all() and _untouched(ws, c * ns * 2), "the partial slots are not the restated c x nsplit x 2"
    if coop:
        _run_interloper(shape)
    b2 = _bwd16(shape, dev, y_dev, mean_dev, inv_dev, with_res, relu, ws, nb)
    assert _same(b1, b2), "a second identical backward launch differs"
    assert all(g.intact() for g in b1.values() if g is not None), "backward wrote outside an output"
    dg_k, db_k = b1["dgamma"].t.cpu(), b1["dbeta"].t.cpu()
    assert torch.equal(b1["acc_g"].t.cpu(), dg_k + 1.0) and torch.equal(b1["acc_b"].t.cpu(), db_k + 2.0)
    dz_k, pad_ok = _out16(b1["dz"], c)
    assert pad_ok, "padding lanes of dz are not zero"
    if with_res:  # the residual branch's gradient is the masked dy itself, bit for bit, zeros in the padding lanes
        assert torch.equal(b1["dres"].t.cpu().reshape(n, c8, hw, 8), bm.pack_c8(back["g"], 0.0)), "dres is not the masked dy"
    gx = back["g"] * back["xh"]
    _report(tag + " bwd",
            slot_g=_frac(part[..., 0] - bm.slot_sums(back["g"], sl), bm.slot_bounds(back["g"], sl)),
            slot_gxhat=_frac(part[..., 1] - bm.slot_sums(gx, sl), bm.slot_bounds(gx, sl)),
            dbeta=_frac(db_k.double() - back["dbeta"], 1e-4 * back["dbeta"].abs().max().expand(c)),
            dgamma=_frac(dg_k.double() - back["dgamma"], 1e-4 * back["dgamma"].abs().max().expand(c)),
            dz=_frac(dz_k - back["dz"], bm.tol16(back["dz"])))

    # ---- ReLU without residual: the mask re-derived from z (y == NULL) against the launch given the kernel's own forward y,
    # mean and invstd - bit-identical.  (Against the reference the re-derived mask may differ only where |y_ref| is within the y
    # tolerance: that is the forward y comparison above, which leaves no element out.)
    if relu and not with_res:
        given = _bwd16(shape, dev, f1["y"].t, f1["mean"].t, f1["invstd"].t, 0, 1, ws, nb)
        derived = _bwd16(shape, dev, None, f1["mean"].t, f1["invstd"].t, 0, 1, ws, nb)
        assert _same(given, derived), "mask from z differs from mask from the kernel's own y"
        flips = (y_k > 0) != (y_ref > 0)
        assert (y_ref.abs()[flips] <= bm.tol16(y_ref)[flips]).all()


# ---- apply-only entries -----------------------------------------------------------------------------------------------------------
def _apply_case(shape, n_parts, relu, with_res, seed=0):
    """device tensors and exact float64 partials (spread unevenly over n_parts fp32 slots) of one apply-only call, both directions"""
    n, c, hw = shape
    inp = bm.make_inputs(shape)
    z = inp["z"]
    res = inp["res"] if with_res else None
    pf = bm.spread_partials(z.sum(dim=(0, 2)), (z * z).sum(dim=(0, 2)), c, n_parts, seed=n_parts + seed)
    ref = bm.forward_ref(z, inp["gamma"], inp["beta"], res, relu, inp["mm"], inp["mv"])
    g = inp["dy"] * (ref["y"].half() > 0) if relu else inp["dy"]  # the pre-masked gradient a data-gradient conv leaves
    pb = bm.spread_partials(g.sum(dim=(0, 2)), (g * z).sum(dim=(0, 2)), c, n_parts, seed=n_parts + seed + 1)
    mean32, inv32 = ref["mean"].float(), ref["invstd"].float()
    back = bm.backward_ref(g, z, None, inp["gamma"], mean32.double(), inv32.double(), 0)
    ws, nb = _workspace(c)
    dev = dict(z=_act(z), res=_act(res) if with_res else None, g=_act(g), gamma=_vec(inp["gamma"]), beta=_vec(inp["beta"]),
               pf=pf.to(DEV), pb=pb.to(DEV), mean=mean32.to(DEV), invstd=inv32.to(DEV), ws=ws, nb=nb)
    return dict(shape=shape, n_parts=n_parts, relu=relu, inp=inp, res=res, ref=ref, back=back, pf=pf, pb=pb, dev=dev)


def _apply_outputs(case):
    n, c, hw = case["shape"]
    c8 = bm.c8_of(c)
    o = dict(y=Guarded((n, c8, hw, 8), torch.float16), mean=Guarded((c,), torch.float32), invstd=Guarded((c,), torch.float32),
             mm=Guarded((c,), torch.float32), mv=Guarded((c,), torch.float32), dz=Guarded((n, c8, hw, 8), torch.float16),
             dgamma=Guarded((c,), torch.float32), dbeta=Guarded((c,), torch.float32), acc_g=Guarded((c,), torch.float32),
             acc_b=Guarded((c,), torch.float32))
    o["mm"].t.copy_(case["inp"]["mm"].float())
    o["mv"].t.copy_(case["inp"]["mv"].float())
    o["acc_g"].t.fill_(1.0)
    o["acc_b"].t.fill_(2.0)
    return o


def _launch_apply_single(case, o):
    n, c, hw = case["shape"]
    d = case["dev"]
    _lib.check(LIB.mp_f16_bn_train_fwd_stats(P(d["z"]), P(d["gamma"]), P(d["beta"]), P(d["res"]), P(o["y"].t), P(o["mean"].t), P(o["invstd"].t),
                                             P(o["mm"].t), P(o["mv"].t), n, c, hw, bm.EPS, bm.MOMENTUM, case["relu"], P(d["pf"]),
                                             case["n_parts"], P(d["ws"]), d["nb"], _lib.stream()), "fwd_stats")
    _lib.check(LIB.mp_f16_bn_train_bwd_stats(P(d["g"]), P(d["z"]), P(d["gamma"]), P(d["mean"]), P(d["invstd"]), P(o["dz"].t), P(o["dgamma"].t),
                                             P(o["dbeta"].t), P(o["acc_g"].t), P(o["acc_b"].t), n, c, hw, P(d["pb"]), case["n_parts"],
                                             P(d["ws"]), d["nb"], _lib.stream()), "bwd_stats")


def _check_apply(case, o, folded, tag):
    n, c, hw = case["shape"]
    ref, back, inp = case["ref"], case["back"], case["inp"]
    count = n * hw
    assert all(g.intact() for g in o.values()), "wrote outside an output"
    # the slots hold the exact sums to one fp32 rounding each; the fold launch rounds its eight range totals to fp32 once more
    _, mag = bm.partial_totals(case["pf"], c)
    rounds = (2.0 if folded else 1.0) * bm.U32
    dmean, dvar, dinv = bm.stat_bounds(inp["z"], rounds * mag[:, 0], rounds * mag[:, 1], ref)
    unbiased = ref["var"] * count / (count - 1) if count > 1 else ref["var"]
    dunb = dvar * (count / (count - 1) if count > 1 else 1.0) + bm.U32 * unbiased
    y_k, pad_y = _out16(o["y"], c)
    dz_k, pad_dz = _out16(o["dz"], c)
    assert pad_y and pad_dz, "padding lanes are not zero"
    dg_k, db_k = o["dgamma"].t.cpu(), o["dbeta"].t.cpu()
    assert torch.equal(o["acc_g"].t.cpu(), dg_k + 1.0) and torch.equal(o["acc_b"].t.cpu(), db_k + 2.0)
    _report(tag,
            mean=_frac(o["mean"].t.cpu().double() - ref["mean"], dmean), invstd=_frac(o["invstd"].t.cpu().double() / ref["invstd"] - 1.0, dinv),
            moving_mean=_frac(o["mm"].t.cpu().double() - ref["mm"], bm.moving_bound(ref, inp["mm"], ref["mm"], dmean)),
            moving_var=_frac(o["mv"].t.cpu().double() - ref["mv"], bm.moving_bound(ref, inp["mv"], ref["mv"], dunb)),
            y=_frac(y_k - ref["y"], bm.tol16(ref["y"])), dz=_frac(dz_k - back["dz"], bm.tol16(back["dz"])),
            dbeta=_frac(db_k.double() - back["dbeta"], 1e-4 * back["dbeta"].abs().max().expand(c)),
            dgamma=_frac(dg_k.double() - back["dgamma"], 1e-4 * back["dgamma"].abs().max().expand(c)))
    return dmean, dinv


@pytest.mark.parametrize("shape,n_parts,knobs,props", bm.APPLY_ROWS, ids=[bm.row_id(r[0], f"p{r[1]}", *r[2].values()) for r in bm.APPLY_ROWS])
def test_apply_only_entries_vs_float64(shape, n_parts, knobs, props, monkeypatch):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    n, c, hw = shape
    c8 = bm.c8_of(c)
    folded = bm.prefold(n_parts, int(knobs.get("MP_BN_PREFOLD_ABOVE", bm.MAX_FOLD_PARTS)))[0]
    # the two large rows are there for the division and the batch loop, which do not depend on the mode: one mode keeps them quick
    for relu, with_res in ((1, 1), (0, 0)) if n * c * hw < 2 ** 20 else ((1, 1),):
        case = _apply_case(shape, n_parts, relu, with_res)
        o = _apply_outputs(case)
        _launch_apply_single(case, o)
        ws = case["dev"]["ws"]
        # the fold launch leaves [c8][8][16] floats at the head of the workspace; nothing else is written there
        assert _untouched(ws, c8 * bm.FOLD_SPLIT * 16 // 2 if folded else 0)
        assert bool(torch.isfinite(ws[:c8 * bm.FOLD_SPLIT * 16 // 2].view(torch.float32)).all()) == folded
        dmean, dinv = _check_apply(case, o, folded, bm.row_id(shape, f"p{n_parts}", f"relu{relu}res{with_res}", *knobs.values()))
        o2 = _apply_outputs(case)
        _launch_apply_single(case, o2)
        assert _same(o, o2), "a second identical launch differs"
        # the statistics prologue as a launch of its own: the same statistics bit for bit, scale / shift for the consumer
        ref, inp, d = case["ref"], case["inp"], case["dev"]
        fin = dict(mean=Guarded((c,), torch.float32), invstd=Guarded((c,), torch.float32), mm=Guarded((c,), torch.float32),
                   mv=Guarded((c,), torch.float32), sc=Guarded((c8 * 8,), torch.float32), sh=Guarded((c8 * 8,), torch.float32))
        fin["mm"].t.copy_(inp["mm"].float())
        fin["mv"].t.copy_(inp["mv"].float())
        _lib.check(LIB.mp_f16_bn_train_finalize(P(d["gamma"]), P(d["beta"]), P(fin["mean"].t), P(fin["invstd"].t), P(fin["mm"].t), P(fin["mv"].t), n, c,
                                                hw, bm.EPS, bm.MOMENTUM, P(d["pf"]), n_parts, P(fin["sc"].t), P(fin["sh"].t), P(d["ws"]), d["nb"],
                                                _lib.stream()), "finalize")
        assert all(g.intact() for g in fin.values())
        assert all(torch.equal(fin[k].t, o[k].t) for k in ("mean", "invstd", "mm", "mv"))
        sc, sh = fin["sc"].t.cpu().double(), fin["sh"].t.cpu().double()
        assert (sc[c:] == 0).all() and (sh[c:] == 0).all()
        sc_ref = inp["gamma"] * ref["invstd"]
        # scale: invstd's bound and one product; shift = fma(-mean, scale, beta): both inputs' bounds and one rounding
        sc_tol = sc_ref.abs() * (dinv + 2 * bm.U32)
        sh_tol = ref["mean"].abs() * sc_tol + sc_ref.abs() * dmean + 2 * bm.U32 * (inp["beta"].abs() + (ref["mean"] * sc_ref).abs())
        _report("finalize", scale=_frac(sc[:c] - sc_ref, sc_tol), shift=_frac(sh[:c] - (inp["beta"] - ref["mean"] * sc_ref), sh_tol))


def test_grouped_apply_only_entries_equal_single_launches():
    """one grouped call of four jobs drawn from different rows (the first above the fold limit): every output bit-identical to the
    single-entry launches, which test_apply_only_entries_vs_float64's checks hold against float64 here as well"""
    cases = [_apply_case(shape, n_parts, 1, j % 2, seed=j) for j, (shape, n_parts) in enumerate(bm.GROUPED_JOBS)]
    single, grouped = [_apply_outputs(cs) for cs in cases], [_apply_outputs(cs) for cs in cases]
    fwd, bwd = [], []
    for cs, o, q in zip(cases, single, grouped):
        n, c, hw = cs["shape"]
        d = cs["dev"]
        _launch_apply_single(cs, o)
        _check_apply(cs, o, bm.prefold(cs["n_parts"])[0], bm.row_id(cs["shape"], f"p{cs['n_parts']}", "single"))
        d["ws"].fill_(float("nan"))
        fwd.append(_lib.BnFwdJob(z=P(d["z"]), gamma=P(d["gamma"]), beta=P(d["beta"]), res=P(d["res"]), y=P(q["y"].t), save_mean=P(q["mean"].t),
                                 save_invstd=P(q["invstd"].t), moving_mean=P(q["mm"].t), moving_var=P(q["mv"].t), partials=P(d["pf"]),
                                 workspace=P(d["ws"]), workspace_bytes=d["nb"], n=n, c=c, hw=hw, relu=1, n_parts=cs["n_parts"], reserved=0))
        bwd.append(_lib.BnBwdJob(g=P(d["g"]), z=P(d["z"]), gamma=P(d["gamma"]), save_mean=P(d["mean"]), save_invstd=P(d["invstd"]), dz=P(q["dz"].t),
                                 dgamma=P(q["dgamma"].t), dbeta=P(q["dbeta"].t), dgamma_acc=P(q["acc_g"].t), dbeta_acc=P(q["acc_b"].t),
                                 partials=P(d["pb"]), workspace=P(d["ws"]), workspace_bytes=d["nb"], n=n, c=c, hw=hw, n_parts=cs["n_parts"]))
    _lib.check(LIB.mp_f16_bn_train_fwd_stats_grouped((_lib.BnFwdJob * 4)(*fwd), 4, bm.EPS, bm.MOMENTUM, _lib.stream()), "fwd grouped")
    _lib.check(LIB.mp_f16_bn_train_bwd_stats_grouped((_lib.BnBwdJob * 4)(*bwd), 4, _lib.stream()), "bwd grouped")
    torch.cuda.synchronize()
    for j, (o, q) in enumerate(zip(single, grouped)):
        assert _same(o, q), f"job {j}: the grouped launch differs from the single-entry launches"


# ---- fp32 entries -----------------------------------------------------------------------------------------------------------------
_F32 = [(s, m, False) for s, _ in bm.F32_ROWS for m in bm.MODES] + [(bm.F32_ILL_ROW, (1, 0), True)]


@pytest.mark.parametrize("shape,mode,ill", _F32, ids=[bm.row_id(s, f"relu{m[0]}res{m[1]}", *(["ill"] if i else [])) for s, m, i in _F32])
def test_f32_entries_vs_float64(shape, mode, ill):
    n, c, hw = shape
    relu, with_res = mode
    count, u = n * hw, bm.U32
    inp = bm.make_inputs(shape, ill, half=False)
    sl = bm.slices32(n, hw)
    z, gamma, beta = inp["z"], inp["gamma"], inp["beta"]
    res = inp["res"] if with_res else None
    ref = bm.forward_ref(z, gamma, beta, res, relu, inp["mm"], inp["mv"])
    dev = {k: _vec(inp[k]) for k in ("z", "res", "dy", "gamma", "beta")}
    tag = bm.row_id(shape, "f32", f"relu{relu}res{with_res}", *(["ill"] if ill else []))
    nslots = c * bm.BN_SPLIT * 2

    def fwd():
        ws, nb = _workspace(c)
        o = dict(y=Guarded((n, c, hw), torch.float32), mean=Guarded((c,), torch.float32), invstd=Guarded((c,), torch.float32),
                 mm=Guarded((c,), torch.float32), mv=Guarded((c,), torch.float32))
        o["mm"].t.copy_(inp["mm"].float())
        o["mv"].t.copy_(inp["mv"].float())
        _lib.check(LIB.mp_bn_train_fwd(P(dev["z"]), P(dev["gamma"]), P(dev["beta"]), P(dev["res"]) if with_res else None, P(o["y"].t), P(o["mean"].t),
                                       P(o["invstd"].t), P(o["mm"].t), P(o["mv"].t), n, c, hw, bm.EPS, bm.MOMENTUM, relu, P(ws), nb, _lib.stream()),
                   "bn fwd f32")
        return o, ws

    f1, ws = fwd()
    f2, _ = fwd()
    assert _same(f1, f2) and all(g.intact() for g in f1.values())
    part = ws[:nslots].cpu().reshape(c, bm.BN_SPLIT, 2)
    assert torch.isfinite(part).all() and _untouched(ws, nslots)
    b0, b1 = bm.slot_bounds(z, sl), bm.slot_bounds(z * z, sl)
    dmean, dvar, dinv = bm.stat_bounds(z, b0.sum(dim=1), b1.sum(dim=1), ref)
    unbiased = ref["var"] * count / (count - 1)
    dunb = dvar * count / (count - 1) + u * unbiased
    mean_k, inv_k = f1["mean"].t.cpu().double(), f1["invstd"].t.cpu().double()
    assert (1.0 / inv_k ** 2 - ref["eps"] > 0).all(), "the variance clamp fired"
    # y in fp32 at the kernel's own saved statistics (their error is judged once, by its bound): scale = gamma * invstd (one rounding),
    # shift = beta - mean * scale (two), z * scale + shift (two), + res (one): 6 u on the magnitudes of the terms
    a = gamma * inv_k
    y_ref = bm.forward_ref(z, gamma, beta, res, relu, inp["mm"], inp["mv"], stats=(mean_k, inv_k))["y"]
    y_tol = 6 * u * ((z * a[None, :, None]).abs() + ((mean_k * a).abs() + beta.abs())[None, :, None] + (res.abs() if with_res else 0.0))
    _report(tag + " fwd",
            slot_sum=_frac(part[..., 0] - bm.slot_sums(z, sl), b0), slot_sumsq=_frac(part[..., 1] - bm.slot_sums(z * z, sl), b1),
            mean=_frac(mean_k - ref["mean"], dmean), invstd=_frac(inv_k / ref["invstd"] - 1.0, dinv),
            moving_mean=_frac(f1["mm"].t.cpu().double() - ref["mm"], bm.moving_bound(ref, inp["mm"], ref["mm"], dmean)),
            moving_var=_frac(f1["mv"].t.cpu().double() - ref["mv"], bm.moving_bound(ref, inp["mv"], ref["mv"], dunb)),
            y=_frac(f1["y"].t.cpu().double() - y_ref, y_tol))

    # ---- backward at the reference's y and statistics (as fp32)
    y_given = ref["y"].float()
    mean32, inv32 = ref["mean"].float(), ref["invstd"].float()
    back = bm.backward_ref(inp["dy"], z, y_given.double(), gamma, mean32.double(), inv32.double(), relu)
    y_dev, mean_dev, inv_dev = y_given.to(DEV), mean32.to(DEV), inv32.to(DEV)

    def bwd():
        ws, nb = _workspace(c)
        o = dict(dz=Guarded((n, c, hw), torch.float32), dres=Guarded((n, c, hw), torch.float32) if with_res else None,
                 dgamma=Guarded((c,), torch.float32), dbeta=Guarded((c,), torch.float32), acc_g=Guarded((c,), torch.float32),
                 acc_b=Guarded((c,), torch.float32))
        o["acc_g"].t.fill_(1.0)
        o["acc_b"].t.fill_(2.0)
        _lib.check(LIB.mp_bn_train_bwd_acc(P(dev["dy"]), P(dev["z"]), P(y_dev) if relu else None, P(dev["gamma"]), P(mean_dev), P(inv_dev), P(o["dz"].t),
                                           P(o["dres"].t) if with_res else None, P(o["dgamma"].t), P(o["dbeta"].t), P(o["acc_g"].t), P(o["acc_b"].t),
                                           n, c, hw, relu, P(ws), nb, _lib.stream()), "bn bwd f32")
        return o, ws

    g1, ws = bwd()
    g2, _ = bwd()
    assert _same(g1, g2) and all(g.intact() for g in g1.values() if g is not None)
    part = ws[:nslots].cpu().reshape(c, bm.BN_SPLIT, 2)
    assert torch.isfinite(part).all() and _untouched(ws, nslots)
    dg_k, db_k = g1["dgamma"].t.cpu(), g1["dbeta"].t.cpu()
    assert torch.equal(g1["acc_g"].t.cpu(), dg_k + 1.0) and torch.equal(g1["acc_b"].t.cpu(), db_k + 2.0)
    if with_res:
        assert torch.equal(g1["dres"].t.cpu(), back["g"].float()), "dres is not the masked dy"
    gx = back["g"] * back["xh"]
    bg, bgx = bm.slot_bounds(back["g"], sl), bm.slot_bounds(gx, sl)
    # dz = k (g - mean g - xhat mean(g xhat)) in fp32: eight roundings on the magnitudes of the three terms, and the bounds of the
    # two channel sums (their slots' bounds, the fp32 store) carried through
    k = (gamma * inv32.double()).abs()[None, :, None]
    d_b, d_g = bg.sum(dim=1) + u * back["dbeta"].abs(), bgx.sum(dim=1) + u * back["dgamma"].abs()
    dz_tol = k * (8 * u * (back["g"].abs() + (back["dbeta"].abs() / count)[None, :, None] + (back["xh"] * (back["dgamma"] / count)[None, :, None]).abs())
                  + (d_b[None, :, None] + back["xh"].abs() * d_g[None, :, None]) / count)
    _report(tag + " bwd",
            slot_g=_frac(part[..., 0] - bm.slot_sums(back["g"], sl), bg), slot_gxhat=_frac(part[..., 1] - bm.slot_sums(gx, sl), bgx),
            dbeta=_frac(db_k.double() - back["dbeta"], 1e-4 * back["dbeta"].abs().max().expand(c)),
            dgamma=_frac(dg_k.double() - back["dgamma"], 1e-4 * back["dgamma"].abs().max().expand(c)),
            dz=_frac(g1["dz"].t.cpu().double() - back["dz"], dz_tol))
