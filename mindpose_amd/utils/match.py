"""Associative-embedding grouping (reference: mindpose/utils/match.py:15-116), host numpy.

Joints are visited in ``joint_order``; the detections of a joint above ``vis_thr`` are assigned to the existing person groups by
the Hungarian algorithm on the L2 distance between their tag and each group's mean tag (rounded to integers with
``use_rounded_norm``), through ``scipy.optimize.linear_sum_assignment`` - the reference's own solver.  With rounded costs the
matrix is full of ties and another solver could return another optimum, so it is not replaced.  A detection without a match
closer than ``tag_thr`` opens a new group keyed by its first tag value (a later detection with the same key overwrites that
group, as the reference's dict does).
"""
from typing import Dict, List

import numpy as np
import scipy.optimize


def _assign(cost: np.ndarray) -> np.ndarray:
    """[num_pairs, 2] int32 (row, column) of a minimum-cost assignment."""
    rows, cols = scipy.optimize.linear_sum_assignment(cost)
    return np.array((rows, cols)).T.astype(np.int32)


def match_by_tag(val_k: np.ndarray, tag_k: np.ndarray, ind_k: np.ndarray, joint_order: List[int], vis_thr: float = 0.1,
                 tag_thr: float = 1, ignore_too_much: bool = False, use_rounded_norm: bool = True) -> np.ndarray:
    """val_k [K, M], tag_k [K, M, L], ind_k [K, M, 2 (x, y)] of one image -> [P, K, 3 + L] float32 (x, y, value, tags) per
    person group, in the order the groups were opened; an empty array when nothing passes ``vis_thr``."""
    num_joints, max_num, num_tags = tag_k.shape
    # per joint and candidate: x, y, value, tags
    candidates = np.concatenate((ind_k, val_k[..., None], tag_k), axis=2)
    empty_person = np.zeros((num_joints, 3 + num_tags), np.float32)
    people: Dict = {}      # group key -> [K, 3 + L] joints of that person
    group_tags: Dict = {}  # group key -> list of the tags assigned to it

    def open_group(key, joint, row, tag):
        people.setdefault(key, empty_person.copy())[joint] = row
        group_tags[key] = [tag]

    for step in range(num_joints):
        joint = joint_order[step]
        visible = candidates[joint][:, 2] > vis_thr
        tags = tag_k[joint][visible]
        if tags.shape[0] == 0:
            continue
        rows = candidates[joint][visible]

        if step == 0 or not people:
            for j in range(tags.shape[0]):
                open_group(tags[j, 0], joint, rows[j], tags[j])
            continue

        keys = list(people)
        means = [np.mean(np.stack(group_tags[key]), axis=0) for key in keys]
        if ignore_too_much and len(keys) == max_num:
            continue
        means = np.stack(means)

        dist = np.linalg.norm(rows[:, None, 3:] - means[None, :, :], ord=2, axis=2)
        cost = np.round(dist) if use_rounded_norm else dist.copy()
        n_new, n_groups = dist.shape
        if n_new > n_groups:  # more detections than groups: dummy columns that no real match undercuts
            cost = np.concatenate((cost, np.zeros((n_new, n_new - n_groups), np.float32) + 1e10), axis=1)

        for r, c in _assign(cost):
            if r < n_new and c < n_groups and dist[r][c] < tag_thr:
                key = keys[c]
                people[key][joint] = rows[r]
                group_tags[key].append(tags[r])
            else:
                open_group(tags[r, 0], joint, rows[r], tags[r])

    return np.array(list(people.values())).astype(np.float32)
