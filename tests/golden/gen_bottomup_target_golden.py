"""Generate tests/golden/bottomup_target.npz: outputs of the REFERENCE's own numpy ``BottomUpGenerateTarget``
(mindpose/data/transform/bottomup_transform.py:463-598).

Run ONLY where a checkout of the reference is present:  python tests/golden/gen_bottomup_target_golden.py <reference root>

The class is loaded by file path, as gen_golden.py loads the top-down one: ``mindpose/__init__.py`` (which imports MindSpore) is
bypassed and an empty ``cv2`` module object stands in for the import (the module calls ``cv2.setNumThreads`` at import; target
generation never touches cv2).  No reference source or bytecode is written anywhere: only the inputs and the returned arrays.

Groups of images share one configuration (heat-map sizes, tag_per_joint, max_num); per group the file holds the padded key
points [N, S, Mmax, K, 3], the person counts [N], the targets [N, S, K, Hmax, Wmax] (non-zero entries only) and tag_ind.

The issue behind these fixtures asks the generator to assert, on the CPU, that a float64 ``exp`` of the reference's float32
argument, rounded to float32, stays within 1 float32 ulp of the reference everywhere and differs at all in fewer than 1e-3 of the
non-zero elements, for every recorded group.  It does NOT: numpy's vectorised float32 ``exp`` is itself up to 2 ulp off the
correctly rounded value on about 39 % of arguments, so ``check_device_model`` reports max 2 ulp and 42 - 48 % differing for every
group, whatever the inputs.  The figures are printed and stored, the file is written, and the assertion is then made as asked -
and fails; it is left so rather than widened.  The device kernel does not use a float64 exponential for that reason: it restates
numpy's float32 algorithm (``numpy_expf`` in csrc/bottomup_train_ops.hip) and the GPU test holds it to the two conditions against
these fixtures.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if len(sys.argv) != 2:
    sys.exit(__doc__)
REF = os.path.join(sys.argv[1], "mindpose")
SIGMA = 2.0


def load_reference_class():
    for name in ["mindpose", "mindpose.data", "mindpose.data.transform"]:
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
    cv2 = types.ModuleType("cv2")
    cv2.setNumThreads = lambda n: None
    sys.modules["cv2"] = cv2

    def load(modname, path):
        spec = importlib.util.spec_from_file_location(modname, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[modname] = mod
        spec.loader.exec_module(mod)
        return mod

    load("mindpose.register", REF + "/register.py")
    load("mindpose.data.column_names", REF + "/data/column_names.py")
    load("mindpose.data.transform.transform", REF + "/data/transform/transform.py")
    load("mindpose.data.transform.utils", REF + "/data/transform/utils.py")
    return load("mindpose.data.transform.bottomup_transform", REF + "/data/transform/bottomup_transform.py").BottomUpGenerateTarget


def config(sizes, tag_per_joint):
    return dict(image_size=[512, 512], max_image_size=[512, 512], heatmap_sizes=[list(s) for s in sizes],
                flip_pairs=[[1, 2]], pixel_std=200.0, tag_per_joint=tag_per_joint)


def border_points(w, h):
    """Centres just outside each border, exactly 3 sigma + 1 outside (the last window that still touches / the first that does
    not), on the last row / column, and halves for the rounding rule."""
    return [(-1.0, h / 2), (float(w), h / 2), (w / 2, -1.0), (w / 2, float(h)),
            (-7.0, 3.0), (-8.0, 3.0), (w + 5.0, 3.0), (w + 6.0, 3.0), (3.0, -7.0), (3.0, -8.0), (3.0, h + 5.0), (3.0, h + 6.0),
            (-0.4, -0.4), (w - 0.6, h - 0.6), (w - 0.5, h - 0.5), (w - 1.5, h - 1.5), (-0.5, 0.5), (2.5, 3.5), (0.5, 1.5),
            (10.5, 7.5), (6.25, 4.75), (-30.0, -30.0), (w + 40.0, h + 40.0)]


def small_group(sizes, k, max_num, seed):
    """Hand-built images: [per stage [M, K, 3]] each."""
    rng = np.random.RandomState(seed)
    images = []

    def scaled(base):  # base in stage-0 pixels -> every stage
        out = []
        for w, h in sizes:
            kp = base.copy()
            kp[..., 0] *= w / sizes[0][0]
            kp[..., 1] *= h / sizes[0][1]
            out.append(kp.astype(np.float32))
        return out

    w0, h0 = sizes[0]
    # random persons, some joints invisible (flag 0) or flagged negative, visible flag 2 as COCO has
    for m in (1, 3, max_num):
        base = np.concatenate([rng.uniform(-3, w0 + 3, (m, k, 1)), rng.uniform(-3, h0 + 3, (m, k, 1)),
                               rng.choice([0.0, 1.0, 2.0, -1.0], (m, k, 1), p=[0.2, 0.5, 0.2, 0.1])], axis=2)
        images.append(scaled(base))
    # the border and rounding points, per stage in that stage's own pixels: persons of k joints each, in order
    per_stage = []
    count = None
    for w, h in sizes:
        pts = border_points(w, h)
        pts += [pts[-1]] * (-len(pts) % k)
        arr = np.array([[x, y, 1.0] for x, y in pts], np.float32).reshape(-1, k, 3)[:max_num]
        count = arr.shape[0]
        per_stage.append(arr)
    images.append(per_stage)
    if count < len(border_points(*sizes[0])) / k:  # the rest of the points as a second image
        per_stage = []
        for w, h in sizes:
            pts = border_points(w, h)[count * k:]
            pts += [pts[-1]] * (-len(pts) % k)
            per_stage.append(np.array([[x, y, 1.0] for x, y in pts], np.float32).reshape(-1, k, 3)[:max_num])
        images.append(per_stage)
    # two persons on one pixel (same rounded centre, different sub-pixel offsets), a third nearby; person 1 has an invisible joint
    base = np.zeros((3, k, 3))
    for j in range(k):
        base[0, j] = (5.2 + j, 6.1, 1.0)
        base[1, j] = (4.9 + j, 5.8, 1.0)
        base[2, j] = (7.0 + j, 6.0, 1.0)
    base[1, k - 1, 2] = 0.0
    images.append(scaled(base))
    # only the first joints visible (without tag_per_joint the last VISIBLE joint wins), and one person with none
    base = np.concatenate([rng.uniform(2, w0 - 2, (3, k, 1)), rng.uniform(2, h0 - 2, (3, k, 1)), np.ones((3, k, 1))], axis=2)
    base[0, 1:, 2] = 0.0
    base[1, :, 2] = 0.0
    base[2, k - 1, 0] = w0 + 2.0  # last joint visible, window inside, centre outside: does not win
    images.append(scaled(base))
    # zero persons
    images.append([np.zeros((0, k, 3), np.float32) for _ in sizes])
    return images


def recipe_group(sizes, k, seed):
    rng = np.random.RandomState(seed)
    images = []
    for m in (6, 3):
        centre = np.concatenate([rng.uniform(10, sizes[0][0] - 10, (m, 1, 1)), rng.uniform(10, sizes[0][1] - 10, (m, 1, 1))], axis=2)
        xy = centre + rng.normal(0, 9.0, (m, k, 2))
        xy = np.round(xy * 4) / 4  # quarters: halves occur
        vis = (rng.rand(m, k, 1) > 0.2).astype(np.float64)
        base = np.concatenate([xy, vis], axis=2)
        stages = []
        for w, h in sizes:
            kp = base.copy()
            kp[..., 0] *= w / sizes[0][0]
            kp[..., 1] *= h / sizes[0][1]
            stages.append(kp.astype(np.float32))
        images.append(stages)
    return images


def device_model(keypoints, size, k):
    """The kernel's arithmetic for one level in numpy: the reference's float32 argument, exp in float64, rounded to float32."""
    w, h = size
    target = np.zeros((k, h, w), np.float32)
    gx = np.arange(0, 13, 1, np.float32)
    gy = gx[:, None]
    for person in keypoints:
        for j, pt in enumerate(person):
            if not pt[2] > 0:
                continue
            mu_x, mu_y = round(pt[0]), round(pt[1])
            ulx, uly, brx, bry = mu_x - 6, mu_y - 6, mu_x + 7, mu_y + 7
            if ulx >= w or uly >= h or brx < 0 or bry < 0:
                continue
            x0p = (np.float32(6.0) + pt[0]) - np.float32(mu_x)
            y0p = (np.float32(6.0) + pt[1]) - np.float32(mu_y)
            arg = -((gx - x0p) ** 2 + (gy - y0p) ** 2) / np.float32(8.0)
            assert arg.dtype == np.float32
            g = np.exp(arg.astype(np.float64)).astype(np.float32)
            x0, x1, y0, y1 = max(0, ulx), min(brx, w), max(0, uly), min(bry, h)
            target[j, y0:y1, x0:x1] = np.maximum(target[j, y0:y1, x0:x1], g[y0 - uly:y1 - uly, x0 - ulx:x1 - ulx])
    return target


def check_device_model(name, model, ref):
    """Max ulp distance and the number of differing non-zero elements; the two conditions are asserted by main() once the file
    is written, so that a failing run still leaves the figures and the fixture to look at."""
    assert ((model != 0) == (ref != 0)).all(), name
    nz = ref != 0
    ulp = np.abs(model.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
    differing = int((ulp[nz] != 0).sum())
    print(f"{name}: float64-exp model vs reference: max {int(ulp.max())} ulp, {differing} of {int(nz.sum())} non-zero elements differ")
    return int(ulp.max()), differing, int(nz.sum())


def main():
    cls = load_reference_class()
    groups = [
        ("small_tpj", [(20, 16), (40, 32)], 4, 6, True, small_group([(20, 16), (40, 32)], 4, 6, 11)),
        ("small_notpj", [(20, 16), (40, 32)], 4, 6, False, small_group([(20, 16), (40, 32)], 4, 6, 11)),
        ("odd_tpj", [(14, 10), (27, 21)], 3, 5, True, small_group([(14, 10), (27, 21)], 3, 5, 12)),
        ("wide_first_notpj", [(36, 12), (24, 28)], 3, 5, False, small_group([(36, 12), (24, 28)], 3, 5, 13)),
        ("recipe_tpj", [(128, 128), (256, 256)], 17, 30, True, recipe_group([(128, 128), (256, 256)], 17, 14)),
    ]
    out = dict(names=np.array([g[0] for g in groups]), sigma=SIGMA,
               source="reference:mindpose/data/transform/bottomup_transform.py BottomUpGenerateTarget (numpy %s)" % np.__version__)
    figures = {}
    for name, sizes, k, max_num, tpj, images in groups:
        t = cls(is_train=True, config=config(sizes, tpj), sigma=SIGMA, max_num=max_num)
        n, s = len(images), len(sizes)
        mmax = max(1, max(st[0].shape[0] for st in images))
        kp = np.zeros((n, s, mmax, k, 3), np.float32)
        counts = np.zeros(n, np.int32)
        targets, tags, models = [], [], []
        wmax, hmax = max(w for w, _ in sizes), max(h for _, h in sizes)
        for i, stages in enumerate(images):
            counts[i] = stages[0].shape[0]
            for si, a in enumerate(stages):
                kp[i, si, :a.shape[0]] = a
            res = t.transform({"keypoints": [a.copy() for a in stages]})
            assert res["target"].dtype == np.float32 and res["target"].shape == (s, k, hmax, wmax), res["target"].shape
            targets.append(res["target"])
            tags.append(res["tag_ind"].astype(np.int32))
            model = np.zeros_like(res["target"])
            for si, (a, (w, h)) in enumerate(zip(stages, sizes)):
                model[si, :, :h, :w] = device_model(a, (w, h), k)
            models.append(model)
        target, tag_ind = np.stack(targets), np.stack(tags)
        figures[name] = check_device_model(name, np.stack(models), target)
        out[name + "/model_max_ulp"], out[name + "/model_differing"] = np.array(figures[name][0]), np.array(figures[name][1])
        flat = target.reshape(-1)
        nz = np.flatnonzero(flat)
        out[name + "/heatmap_sizes"] = np.array(sizes, np.int32)
        out[name + "/tag_per_joint"] = np.array(tpj)
        out[name + "/max_num"] = np.array(max_num, np.int32)
        out[name + "/keypoints"] = kp
        out[name + "/counts"] = counts
        out[name + "/target_shape"] = np.array(target.shape, np.int64)
        out[name + "/target_nz_idx"] = nz.astype(np.int32)
        out[name + "/target_nz_val"] = flat[nz]
        out[name + "/tag_ind"] = tag_ind
        print(name, "images", n, "persons", counts.tolist(), "target", target.shape, "nnz", nz.size, "tags", int(tag_ind[..., 1].sum()))
    path = os.path.join(HERE, "bottomup_target.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    for name, (max_ulp, differing, nonzero) in figures.items():
        assert max_ulp <= 1, (name, "max ulp", max_ulp)
        assert differing < 1e-3 * nonzero, (name, "differing", differing, "of", nonzero)


if __name__ == "__main__":
    main()
