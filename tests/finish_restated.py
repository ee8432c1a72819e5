"""The tail of a bottom-up batch restated without numpy's reductions: the executable specification of what
``mp_bottomup_finish_people`` (``bottomup_ops.hip``) computes per person, rule by rule.  Everything here is scalar arithmetic on
``np.float32`` in a stated order; ``tests/test_bottomup_finish_cpu.py`` holds each rule to the numpy expression of the host path
(``person[:, 2].mean()``, ``np.mean(tags, axis=0)``, ``refine_missing_joint``).

(a) ``numpy_sum``: numpy's float32 sum of a 1-D view of n <= 64 values, whatever its stride: below eight values sequential from 0;
    from eight on eight accumulators over the whole blocks of eight, ((r0+r1)+(r2+r3)) + ((r4+r5)+(r6+r7)), the tail added in order.
(b) ``score``: ``person[:, 2].mean()`` - (a) over the K values of the strided column, one float32 division by K.
(c) ``mean_tag``: ``np.mean(tags, axis=0)`` of [J, L]: L == 1 is a 1-D view, (a); L >= 2 a sequential sum in joint order from the
    first tag; one float32 division by J.
(d) ``map_coord``: ``np.clip(np.float32(v).astype(np.int32), 0, size - 1)`` for a finite v in int32 range: truncation toward zero, then
    the clamp; a NaN reads 0 (outside the bit-equality contract, inside the memory-safety one).
(e) ``located_tags``: the tags of the joints with value > 0, in joint order, read at (map_coord(x), map_coord(y)) of tag channel j
    (channel 0 when the map has one channel).
(f) ``arg_max``: the first maximum in flat index of ``heat - rint(sqrt(sum_l (tag_l - mean_l)^2))`` in float32, the squares summed in l
    order; the winner's centre (+0.5) shifted +-0.25 by the two clamped neighbour comparisons ("greater" -> +0.25), and its value.
(g) the fill rule: joint j takes (x, y, value) of its winner when ``person[j, 2] == 0`` and the winner's value is > 0; a person
    without a located joint is left alone.
"""
from typing import List, Sequence

import numpy as np

F = np.float32


def numpy_sum(a: Sequence[np.float32]) -> np.float32:
    n = len(a)
    assert n <= 64
    res = F(0)
    if n < 8:
        for x in a:
            res = F(res + F(x))
        return res
    r = [F(a[j]) for j in range(8)]
    i = 8
    while i + 8 <= n:
        for j in range(8):
            r[j] = F(r[j] + F(a[i + j]))
        i += 8
    res = F(F(F(r[0] + r[1]) + F(r[2] + r[3])) + F(F(r[4] + r[5]) + F(r[6] + r[7])))
    while i < n:
        res = F(res + F(a[i]))
        i += 1
    return res


def score(person: np.ndarray) -> np.float32:
    k = person.shape[0]
    return F(numpy_sum([person[j, 2] for j in range(k)]) / F(k))


def mean_tag(tags: Sequence[Sequence[np.float32]]) -> List[np.float32]:
    count, num_tags = len(tags), len(tags[0])
    assert count >= 1
    if num_tags == 1:
        return [F(numpy_sum([t[0] for t in tags]) / F(count))]
    out = []
    for l in range(num_tags):
        s = F(tags[0][l])
        for t in tags[1:]:
            s = F(s + F(t[l]))
        out.append(F(s / F(count)))
    return out


def map_coord(v, size: int) -> int:
    v = float(v)
    if v != v:
        return 0
    return min(max(int(min(max(v, -2.0), float(size))), 0), size - 1)  # int() truncates toward zero


def located_tags(person: np.ndarray, tagging: np.ndarray) -> List[np.ndarray]:
    """tagging [K or 1, H, W, L] of the person's image."""
    ktag, h, w, _ = tagging.shape
    return [tagging[j if ktag > 1 else 0, map_coord(person[j, 1], h), map_coord(person[j, 0], w)]
            for j in range(person.shape[0]) if person[j, 2] > 0]


def arg_max(heat: np.ndarray, tags: np.ndarray, mean: Sequence[np.float32]):
    """heat [H, W], tags [H, W, L] of one joint -> (x, y, value) of rule (f)."""
    h, w = heat.shape
    best, best_v = 0, None
    for y in range(h):
        for x in range(w):
            s = F(0)
            for l in range(len(mean)):
                d = F(tags[y, x, l] - mean[l])
                s = F(s + F(d * d))
            v = F(heat[y, x] - F(np.rint(F(np.sqrt(s)))))
            if best_v is None or v > best_v:
                best, best_v = y * w + x, v
    y, x = divmod(best, w)
    xs = F(F(x) + F(0.5)) + (F(0.25) if heat[y, min(x + 1, w - 1)] > heat[y, max(x - 1, 0)] else F(-0.25))
    ys = F(F(y) + F(0.5)) + (F(0.25) if heat[min(y + 1, h - 1), x] > heat[max(y - 1, 0), x] else F(-0.25))
    return F(xs), F(ys), F(heat[y, x])


def finish_person_restated(person: np.ndarray, heatmap: np.ndarray, tagging: np.ndarray, refine: bool):
    """person [K, 3 + L], heatmap [K, H, W], tagging [K or 1, H, W, L] of its image -> (score, the person after the fill rule)."""
    out = person.copy()
    result = score(person)
    tags = located_tags(person, tagging)
    if refine and tags:
        mean = mean_tag(tags)
        for j in range(person.shape[0]):
            if person[j, 2] == 0:
                x, y, value = arg_max(heatmap[j], tagging[j if tagging.shape[0] > 1 else 0], mean)
                if value > 0:
                    out[j, :3] = (x, y, value)
    return result, out
