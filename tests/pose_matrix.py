"""The case lists, designed inputs and CPU references that force the top-down kernels of csrc/pose_ops.hip - decode_kernel<FLIP>,
flip_aggregate_kernel, gaussian_target_kernel - and the joint MSE kernels of csrc/joints_loss.hip - joints_sq_row_kernel /
joints_mse_final_kernel / joints_bwd_kernel - through every path and edge.
Importable without a GPU; tests/test_pose_matrix_cpu.py holds the floors of the lists and checks the builders on the CPU oracle alone,
tests/test_gpu_pose_edges.py runs every case on the device.

The kernels pick their paths by the predicates restated below; SOURCE_LINES quotes the line each one restates.

Decoder inputs are DESIGNED, not drawn: every value is dyadic (a multiple of 2^-6, 2^-12 under the DARK blob, magnitude below 4), so
the flip average (a + b) * 0.5 is exact and a tie is a tie.  A plane is designed as the map the decoder SEES; under the flip test
the two run outputs are derived from it (a = 2 m - flip_back(hf) for a random dyadic hf), so peak positions and tie lists hold for
the averaged map, not for either input.

Out of scope: a plane that mixes NaN with numbers.  The reference's `ops.max` is unpinned there, numpy's argmax (first NaN) and the
kernel's strict `>` (NaN never wins) disagree by design, and nothing in the project produces such a map.  The `empty` planes are all
-inf or all NaN, where both give index 0 and the value of pixel (0, 0).
"""
import collections

import numpy as np

F32 = np.float32
U24 = 2.0 ** -24  # unit round-off of fp32
Q6, Q12 = 2.0 ** -6, 2.0 ** -12

# (file of csrc/, line) the predicates and the loop counts below restate
SOURCE_LINES = {
    "decode_path": ("pose_ops.hip", "if ((hw & 3) == 0 && (!FLIP || (w & 3) == 0)) {"),
    "decode_round": ("pose_ops.hip", "for (int q0 = lane; q0 < nq; q0 += 64 * B) {"),
    "decode_batch": ("pose_ops.hip", "constexpr int B = 4;"),
    "decode_scalar": ("pose_ops.hip", "for (int x = lane; x < w; x += 64) {"),
    "decode_empty": ("pose_ops.hip", "if (bidx == 0x7fffffff) {"),
    "dark_path": ("pose_ops.hip", "constexpr int kDarkFastKs = 17;"),
    "dark_fast": ("pose_ops.hip", "const bool dark_fast = p.refine == MP_REFINE_DARK && p.ks <= kDarkFastKs;"),
    "dark_ks_range": ("pose_ops.hip", "if (ks < 1 || (ks & 1) == 0 || ks > 63) return MP_ERR_UNSUPPORTED;"),
    "target_zero_path": ("pose_ops.hip", "if ((w & 3) == 0) {"),
    "target_window_guard": ("pose_ops.hip", "if (stamp && ix1 > ix0 && iy1 > iy0) {"),
    "target_oob": ("pose_ops.hip", "const bool oob = (ulx >= w) || (uly >= h) || (brx < 0) || (bry < 0);"),
    "target_clamp": ("pose_ops.hip", "fx = fmin(fmax(fx, -1.0e9), 1.0e9);"),
    # the one host predicate of the four loss entries; the case lists below keep every base 16-byte aligned, where it is hw % 4 == 0
    "mse_path": ("joints_loss.hip", "return (hw & 3) == 0 && (((uintptr_t)pred | (uintptr_t)target | (uintptr_t)grad) & 15u) == 0;"),
    "mse_final_stride": ("joints_loss.hip", "for (int i = threadIdx.x; i < rows; i += blockDim.x) acc += (double)partial[i];"),
    "mse_row_sum": ("reduce.h", "if (threadIdx.x == 0) v = (ws4[0] + ws4[1]) + (ws4[2] + ws4[3]);"),
}

DARK_FAST_KS = 17


def ceil_div(a, b):
    return -(-a // b)


def decode_path(h, w, flip):
    """(hw & 3) == 0 && (!FLIP || (w & 3) == 0)"""
    return "quad" if (h * w) % 4 == 0 and (not flip or w % 4 == 0) else "scalar"


def dark_path(ks):
    """p.ks <= kDarkFastKs, kDarkFastKs = 17"""
    return "patch" if ks <= DARK_FAST_KS else "loop"


def target_zero_path(w):
    """(w & 3) == 0"""
    return "quad" if w % 4 == 0 else "scalar"


def mse_path(hw):
    """(hw & 3) == 0, on 16-byte aligned bases"""
    return "quad" if hw % 4 == 0 else "scalar"


# ---- decoder: maps, row counts, refine and flip forms ------------------------------------------------------------------------------

# (h, w) -> what the map reaches
DECODE_MAPS = {
    (1, 1): "single pixel",
    (1, 5): "dy never defined",
    (5, 1): "dx never defined; no UDP",
    (2, 2): "hw = 4 but w = 2: quad without flip, scalar with flip",
    (7, 9): "scalar path",
    (6, 10): "hw % 4 == 0, w % 4 != 0",
    (3, 67): "scalar path, w > 64: a lane takes two columns",
    (8, 4): "fewer than 64 quads: idle lanes keep the sentinel",
    (4, 68): "quad path, w > 64",
    (20, 52): "260 quads: a second q0 += 256 round with a ragged end",
    (64, 48): "the workload's own shape",
}
# (n, k): 1, 5, 7 and 8 rows - fewer than the four rows of a block, a count that is no multiple of four, a full block
ROW_SHAPES = [(1, 1), (1, 5), (1, 7), (2, 4)]
# permutations with fixed points and swaps
FLIP_INDEX = {1: [0], 4: [0, 2, 1, 3], 5: [0, 2, 1, 4, 3], 7: [0, 2, 1, 4, 3, 6, 5]}
# (refine, ks)
REFINE_FORMS = [("none", 0), ("shift", 0)] + [("dark", ks) for ks in (1, 3, 11, 17, 19, 21, 63)]
# (flip, shift_heatmap); every flip case runs with avg_out given and with avg_out NULL
FLIP_FORMS = [(0, 0), (1, 0), (1, 1)]
AVG_FORMS = (True, False)
# (to_original, use_udp); UDP only on maps with h >= 2 and w >= 2 (the reference divides by w - 1)
ORIGINAL_FORMS = [(0, 0), (1, 0), (1, 1)]

DecodeCase = collections.namedtuple("DecodeCase", "h w n k refine ks flip shift_heatmap to_original use_udp")


def refine_id(refine, ks):
    return refine if refine != "dark" else f"dark{ks}"


def _decode_cases():
    cases = []
    for mi, (h, w) in enumerate(DECODE_MAPS):
        for ri, (refine, ks) in enumerate(REFINE_FORMS):
            for bi, (n, k) in enumerate(ROW_SHAPES):
                for fi, (flip, sh) in enumerate(FLIP_FORMS):
                    to_original, use_udp = ORIGINAL_FORMS[(mi + ri + bi + fi) % 3]
                    if use_udp and (h < 2 or w < 2):
                        use_udp = 0
                    cases.append(DecodeCase(h, w, n, k, refine, ks, flip, sh, to_original, use_udp))
    return cases


DECODE_CASES = _decode_cases()

PEAK_NAMES = ("corner_tl", "corner_tr", "corner_bl", "corner_br", "edge_top", "edge_bottom", "edge_left", "edge_right", "interior",
              "flat_first", "flat_last")


def peak_positions(h, w):
    """name -> (y, x) of the positions the map admits: the corners and the two flat ends always, an edge mid-point where the edge has
    one that is no corner (extent >= 3), an interior point where both extents are >= 3"""
    pos = {"corner_tl": (0, 0), "corner_tr": (0, w - 1), "corner_bl": (h - 1, 0), "corner_br": (h - 1, w - 1)}
    if w >= 3:
        pos["edge_top"], pos["edge_bottom"] = (0, w // 2), (h - 1, w // 2)
    if h >= 3:
        pos["edge_left"], pos["edge_right"] = (h // 2, 0), (h // 2, w - 1)
    if h >= 3 and w >= 3:
        pos["interior"] = (h // 2, w // 2 - 1 if w >= 4 else w // 2)
    pos["flat_first"], pos["flat_last"] = (0, 0), (h - 1, w - 1)
    return pos


TIE_KINDS = ("same_quad", "same_round", "lane_steps", "two_rounds", "scalar_i_i64", "three", "constant")


def tie_indices(h, w):
    """kind -> the flat indices that hold the equal maxima, for the kinds the map admits; the lowest index is expected.
    same_quad: two of one lane's float4; same_round: two lanes of one q0 round (for a scalar map simply two lanes); lane_steps: one
    lane's quads q and q + 64 of one round; two_rounds: one lane's quads q and q + 256; scalar_i_i64: columns x and x + 64 of one row,
    one lane's two trips of the scalar loop; three: three maxima, the first and the last pixel's neighbours among them; constant: every
    pixel."""
    hw = h * w
    nq = hw // 4
    ties = {}
    if hw >= 4:
        ties["same_quad"] = (1, 3)
    if nq >= 2:
        ties["same_round"] = (2, 4 * (min(nq, 64) - 1) + 1)
    if hw > 5 + 256:
        ties["lane_steps"] = (5, 5 + 256)
    if hw > 6 + 1024:
        ties["two_rounds"] = (6, 6 + 1024)
    if w >= 66:
        ties["scalar_i_i64"] = ((h - 1) * w + 1, (h - 1) * w + 65)
    if hw >= 9:
        ties["three"] = (3, hw // 2, hw - 2)
    if hw >= 2:
        ties["constant"] = tuple(range(hw))
    return ties


PlaneSpec = collections.namedtuple("PlaneSpec", "kind names index")  # index: the expected flat arg-max


def plane_specs(h, w, dark=False):
    """The designed planes of a map, in the order the rows of its cases take them (cyclically).  DARK cases take the peak planes only:
    their builder puts the blob at the designed position."""
    by_pos = collections.OrderedDict()
    for name, (y, x) in peak_positions(h, w).items():
        by_pos.setdefault((y, x), []).append(name)
    specs = [PlaneSpec("peak_at", tuple(names), y * w + x) for (y, x), names in by_pos.items()]
    if dark:
        return specs
    specs += [PlaneSpec("ties", (kind,), min(idx)) for kind, idx in tie_indices(h, w).items()]
    if h >= 3 or w >= 3:
        specs.append(PlaneSpec("plateau", ("plateau",), (h // 2) * w + w // 2))
    specs.append(PlaneSpec("negative", ("negative",), (h * w) // 2))
    specs += [PlaneSpec("empty", ("inf",), 0), PlaneSpec("empty", ("nan",), 0)]
    return specs


def _dyadic(rng, lo, hi, shape):
    """multiples of 2^-6 in [lo, hi] / 64"""
    return (rng.integers(lo, hi + 1, size=shape) * Q6).astype(F32)


def build_plane(h, w, spec, rng, dark=False):
    """one designed [h, w] fp32 plane"""
    hw = h * w
    y, x = divmod(spec.index, w)
    if spec.kind == "peak_at" and dark:
        # a positive blob (sigma 2, amplitude 3/4, on a 2^-12 grid) on a background in [-3/64, 0]: the blur stays inside the clip
        # [1e-3, 50] at the centre and falls below it far away; the centre's nearest rival is 0.75 exp(-1/8) = 0.662 < 0.75 - 3/64
        ys, xs = np.mgrid[0:h, 0:w]
        blob = np.round(0.75 * np.exp(-((xs - x) ** 2 + (ys - y) ** 2) / 8.0) / Q12) * Q12
        return (_dyadic(rng, -3, 0, (h, w)).astype(np.float64) + blob).astype(F32)
    if spec.kind == "peak_at":
        p = _dyadic(rng, -64, 32, (h, w))
        p[y, x] = 1.0
        return p
    if spec.kind == "ties":
        if spec.names[0] == "constant":
            return np.full((h, w), 0.25, dtype=F32)
        p = _dyadic(rng, -64, 32, hw)
        p[list(tie_indices(h, w)[spec.names[0]])] = 1.0
        return p.reshape(h, w)
    if spec.kind == "plateau":
        p = _dyadic(rng, -64, 32, (h, w))
        p[y, x] = 1.0
        if 1 <= x <= w - 2:
            p[y, x - 1] = p[y, x + 1] = 0.75
        if 1 <= y <= h - 2:
            p[y - 1, x] = p[y + 1, x] = 0.625
        return p
    if spec.kind == "negative":
        p = _dyadic(rng, -96, -48, (h, w))
        p[y, x] = -0.5
        return p
    assert spec.kind == "empty"
    return np.full((h, w), -np.inf if spec.names[0] == "inf" else np.nan, dtype=F32)


def row_specs(h, w, n, k, dark=False):
    """the specs the n * k rows of a case take: the map's list, cyclically, continued from where the smaller row shapes stopped"""
    specs = plane_specs(h, w, dark)
    start = sum(a * b for a, b in ROW_SHAPES[:ROW_SHAPES.index((n, k))])
    return [specs[(start + i) % len(specs)] for i in range(n * k)]


def flip_back(flipped, flip_index, shift_heatmap):
    """joint flip_index[k] of the mirrored run, mirrored back; under shift_heatmap columns 1 ... take their left neighbour and column 0
    keeps its own value"""
    out = flipped[:, list(flip_index)][..., ::-1].copy()
    if shift_heatmap:
        out[..., 1:] = out[..., :-1].copy()
    return out


def decode_inputs(case):
    """dict(seen [n,k,h,w]: the map the decoder sees; hm (and hf, flip_index under the flip test): what it is given; center, scale,
    score; specs: one PlaneSpec per row; index [n,k]: the designed arg-max)"""
    h, w, n, k = case.h, case.w, case.n, case.k
    dark = case.refine == "dark"
    rng = np.random.default_rng([11, h, w, n, k, int(dark)])
    specs = row_specs(h, w, n, k, dark)
    seen = np.stack([build_plane(h, w, s, rng, dark) for s in specs]).reshape(n, k, h, w)
    d = dict(seen=seen, specs=specs, index=np.array([s.index for s in specs], dtype=np.int32).reshape(n, k),
             center=(rng.integers(0, 1600, size=(n, 2)) * 0.25).astype(F32), scale=_dyadic(rng, 20, 192, (n, 2)),
             score=_dyadic(rng, 0, 64, (n,)))
    if case.flip:
        d["flip_index"] = FLIP_INDEX[k]
        d["hf"] = _dyadic(rng, -63, 63, (n, k, h, w))
        with np.errstate(invalid="ignore"):
            d["hm"] = (F32(2) * seen - flip_back(d["hf"], d["flip_index"], case.shift_heatmap)).astype(F32)
    else:
        d["hm"] = seen
    return d


# ---- targets -------------------------------------------------------------------------------------------------------------------------

TARGET_K = 5
JOINT_WEIGHTS = [1.0, 1.2, 1.5, 0.5, 0.0]
# (h, w, sigma): 3 sigma is an integer (the reference's own slice assignment does not broadcast otherwise)
TARGET_MAPS = [(7, 9, 1), (7, 9, 2), (10, 6, 1), (10, 6, 3), (5, 5, 2), (1, 8, 1), (8, 1, 1), (16, 12, 2), (16, 12, 3), (64, 48, 2),
               (64, 48, 3)]
TargetCase = collections.namedtuple("TargetCase", "h w sigma use_udp joint_weights stride")
# stride 4 everywhere, and one map at stride 1 where a coordinate of 3e9 lies beyond the +-1e9 clamp (and beyond int32).  UDP needs
# h >= 2 and w >= 2: its stride is (image - 1) / (map - 1).
TARGET_CASES = [TargetCase(h, w, s, udp, jw, 4) for h, w, s in TARGET_MAPS for udp in (0, 1) for jw in (0, 1) if not udp or min(h, w) >= 2] + \
               [TargetCase(10, 6, 1, udp, 0, 1) for udp in (0, 1)]

AXIS_CLASSES = ("br0", "br-1", "ul_last", "ul_end", "centre", "border_lo", "border_hi")
HALVES = (2, 3, -2, -3)       # fx = m + 0.5 with an even and an odd integer part, positive and negative
VISIBILITIES = (0.0, 0.5, 1.0, 2.0)
HUGE = 3.0e9


def axis_mu(cls, extent, tmp):
    """the rounded position of an axis class: ul = mu - tmp, br = mu + tmp + 1"""
    return {"br0": -tmp - 1, "br-1": -tmp - 2, "ul_last": extent - 1 + tmp, "ul_end": extent + tmp, "centre": extent // 2,
            "border_lo": 0, "border_hi": extent - 1}[cls]


def axis_coord(mu, case):
    """the coordinate (input-image px) that rounds to mu: mu strides, or under UDP for a negative mu half a stride less - int(fx + 0.5)
    truncates toward zero, so fx = mu would land on mu + 1"""
    return (mu - 0.5 if case.use_udp and mu < 0 else mu) * float(case.stride)


def axis_class_holds(cls, mu, ul, br, extent):
    """does (mu, ul, br) of one axis lie in the class it was designed for?"""
    if cls.startswith("half") or cls in ("udp_trunc", "huge+", "huge-"):
        return True  # their rounding is checked by value (tests/test_pose_matrix_cpu.py)
    return {"br0": br == 0, "br-1": br == -1, "ul_last": ul == extent - 1, "ul_end": ul == extent, "centre": mu == extent // 2,
            "border_lo": mu == 0, "border_hi": mu == extent - 1}[cls]


def target_image_size(case):
    """(W, H) of the input image that gives the case's stride exactly: map * stride, or under UDP (map - 1) * stride + 1"""
    if case.use_udp:
        return [(case.w - 1) * case.stride + 1, (case.h - 1) * case.stride + 1]
    return [case.w * case.stride, case.h * case.stride]


def target_points(case):
    """[(class of x, class of y, kx, ky, visibility)] computed from the map, sigma and stride"""
    h, w, tmp, st = case.h, case.w, 3 * case.sigma, float(case.stride)
    at = lambda cls, extent: axis_coord(axis_mu(cls, extent, tmp), case)  # noqa: E731
    cx, cy = at("centre", w), at("centre", h)
    pts = []
    for cls in AXIS_CLASSES:
        kx, ky = at(cls, w), at(cls, h)
        pts += [(cls, "centre", kx, cy, 1.0), ("centre", cls, cx, ky, 1.0), (cls, cls, kx, ky, 1.0)]
    for m in HALVES:
        v = (m + 0.5) * st
        pts += [(f"half{m}", "centre", v, cy, 1.0), ("centre", f"half{m}", cx, v, 1.0), (f"half{m}", f"half{m}", v, v, 2.0)]
    pts += [("udp_trunc", "centre", -0.75 * st, cy, 1.0), ("centre", "udp_trunc", cx, -0.75 * st, 1.0),
            ("udp_trunc", "udp_trunc", -0.75 * st, -0.75 * st, 1.0)]
    pts += [("centre", "centre", cx, cy, v) for v in VISIBILITIES]
    pts += [("border_lo", "border_hi", 0.0, at("border_hi", h), 0.5), ("ul_last", "br0", at("ul_last", w), at("br0", h), 2.0)]
    for sx, sy in ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1)):
        pts.append(("huge+" if sx > 0 else "huge-" if sx < 0 else "centre", "huge+" if sy > 0 else "huge-" if sy < 0 else "centre",
                    sx * HUGE if sx else cx, sy * HUGE if sy else cy, 1.0))
    return pts


def target_keypoints(case):
    """[N, TARGET_K, 3] fp32: the points of target_points, padded with centred ones to whole samples"""
    pts = target_points(case)
    rows = [(kx, ky, v) for _, _, kx, ky, v in pts]
    centre = rows[AXIS_CLASSES.index("centre") * 3]
    while len(rows) % TARGET_K:
        rows.append(centre)
    return np.array(rows, dtype=F32).reshape(-1, TARGET_K, 3)


# ---- JointsMSELoss -------------------------------------------------------------------------------------------------------------------

MSE_HW_SCALAR = [1, 3, 63, 255, 257, 1023]
MSE_HW_QUAD = [4, 252, 1028, 3072]
# rows -> (n, k): joints_mse_final_kernel strides 256 threads over the rows, so 257 and 600 take a second and a third ragged stride
MSE_ROWS = {1: (1, 1), 5: (1, 5), 257: (257, 1), 600: (24, 25)}
MSE_WEIGHTS = ("none", "ones", "mix")
MSE_GRADS = (None, 0.375)  # grad_out NULL, or a one-element tensor
MSE_CASES = [(hw, rows, wk) for hw in MSE_HW_SCALAR + MSE_HW_QUAD for rows in MSE_ROWS for wk in MSE_WEIGHTS]


def mse_additions(hw):
    """the additions one thread of joints_sq_row_kernel makes: one per element of its stride on the scalar path, four per float4"""
    return ceil_div(hw, 256) if mse_path(hw) == "scalar" else 4 * ceil_div(hw, 1024)


def mse_fwd_tolerance(hw):
    """Relative to sum(|w| d^2) / (rows hw): (A + 12) 2^-24.  A = mse_additions(hw) roundings of one thread's accumulator; 12 covers
    the subtraction, the two multiplies, the six butterfly steps, the two adds of ws[] and the final rounding to fp32 (the sum over
    the rows is fp64)."""
    return (mse_additions(hw) + 12) * U24


def mse_inputs(hw, rows, weights):
    """pred, target [rows, hw] and the weights [rows] or None, fp32"""
    rng = np.random.default_rng([13, hw, rows, MSE_WEIGHTS.index(weights)])
    pred = rng.standard_normal((rows, hw), dtype=F32)
    target = rng.standard_normal((rows, hw), dtype=F32)
    w = {"none": None, "ones": np.ones(rows, dtype=F32), "mix": rng.choice(np.array([0.0, 0.5, 2.0], dtype=F32), size=rows)}[weights]
    return pred, target, w


def mse_rows_restated(pred, target, w, path):
    """joints_sq_row_kernel in IEEE fp32, [rows] fp32: thread t of 256 adds (d * d) * w over its elements in ascending order - on the
    scalar path elements t, t + 256, ..., on the quad path the four floats of quads t, t + 256, ... - then the xor butterfly 32 ... 1
    inside each wave of 64 and (w0 + w1) + (w2 + w3).  No weights: w = 1 (the kernel multiplies by 1.f)."""
    rows, hw = pred.shape
    d = (pred - target).astype(F32)
    wv = np.ones(rows, dtype=F32) if w is None else w.astype(F32)
    terms = ((d * d).astype(F32) * wv[:, None]).astype(F32)
    unit = 1 if path == "scalar" else 4
    assert hw % unit == 0
    trips = ceil_div(hw // unit, 256)
    padded = np.zeros((rows, trips * 256 * unit), dtype=F32)  # + 0.0 leaves every partial sum as it is: they start at +0.0
    padded[:, :hw] = terms
    steps = padded.reshape(rows, trips, 256, unit)
    acc = np.zeros((rows, 256), dtype=F32)
    for t in range(trips):
        for e in range(unit):
            acc = (acc + steps[:, t, :, e]).astype(F32)
    lanes = acc.reshape(rows, 4, 64)
    for off in (32, 16, 8, 4, 2, 1):
        lanes = (lanes + lanes[:, :, np.arange(64) ^ off]).astype(F32)
    ws = lanes[:, :, 0]
    return ((ws[:, 0] + ws[:, 1]).astype(F32) + (ws[:, 2] + ws[:, 3]).astype(F32)).astype(F32)


def mse_fwd_restated(pred, target, w, path):
    """mp_joints_mse_fwd in IEEE arithmetic, fp32 scalar: mse_rows_restated, then joints_mse_final_kernel - thread t of 256 adds rows
    t, t + 256, ... in fp64, slot t takes slot t + s for s = 128 ... 1, the sum times 1.0 / (rows hw), rounded to fp32"""
    part = mse_rows_restated(pred, target, w, path).astype(np.float64)
    rows, hw = pred.shape
    sm = np.zeros(256)
    for t in range(min(rows, 256)):
        for v in part[t::256]:
            sm[t] += v
    s = 128
    while s >= 1:
        sm[:s] = sm[:s] + sm[s:2 * s]
        s >>= 1
    return F32(sm[0] * (1.0 / (float(rows) * float(hw))))


def mse_fwd_ref(pred, target, w):
    """float64 on the fp32 inputs: (sum(w d^2) / (rows hw), sum(|w| d^2) / (rows hw))"""
    d2 = (pred.astype(np.float64) - target.astype(np.float64)) ** 2
    wv = np.ones(pred.shape[0]) if w is None else w.astype(np.float64)
    return float((d2 * wv[:, None]).sum() / pred.size), float((d2 * np.abs(wv)[:, None]).sum() / pred.size)


def mse_bwd_restated(pred, target, w, g):
    """joints_bwd_kernel in IEEE fp32 (contraction is off in joints_loss.hip): (a - b) * (w * (g * float32(2 / (rows hw)))), g = 1 for a NULL
    grad_out and no multiply by w without weights"""
    c = F32(1.0 if g is None else g) * F32(2.0 / pred.size)
    c = np.full(pred.shape[0], c, dtype=F32) if w is None else (w.astype(F32) * c).astype(F32)
    return ((pred - target).astype(F32) * c[:, None]).astype(F32)


def mse_bwd_ref(pred, target, w, g):
    """float64: g 2 w (a - b) / (rows hw)"""
    wv = np.ones(pred.shape[0]) if w is None else w.astype(np.float64)
    return (pred.astype(np.float64) - target.astype(np.float64)) * wv[:, None] * (float(F32(1.0 if g is None else g)) * 2.0 / pred.size)


MSE_BWD_TOLERANCE = 4 * U24  # relative to the float64 value: the subtraction, float32(2 / count), g * c, w * c, the product
