"""XGBoost model import: the JSON that ``Booster.save_model("m.json")`` writes ->
``TreeEnsemble`` (general-tree kernel, csrc/kernels/score_forest.hip).

What is read:

* ``learner.gradient_booster.model.trees[*]``: parallel per-node arrays ``left_children``,
  ``right_children``, ``split_indices``, ``split_conditions``; a leaf has
  ``left_children == -1`` and its value in ``split_conditions``;
* ``learner.learner_model_param.base_score``: a probability (plain ``"5E-1"`` or bracketed
  ``"[5E-1]"``), so base = logit(base_score);
* ``learner.objective.name``: ``binary:logistic`` only (sigmoid link);
* ``trees[*].sum_hessian``, when every tree has it: the ensemble's ``cover`` (the background of
  its Shapley attributions, models/explain_forest.py); otherwise the ensemble has none.

XGBoost sends a row LEFT on ``x < t`` with a float32 ``t``; the kernels go right on
``x > thr``.  ``thr = nextafter(t, -inf)`` makes ``x > thr`` <=> ``x >= t`` for every float32
``x``.  Missing values (XGBoost's ``default_left``) are out of scope: transactions are dense.

Refused with a clear error: ``gbtree`` with more than one output group, ``dart``, categorical
splits, feature indices >= 30.

No XGBoost is installed here, so the importer is pinned by hand-built documents of that
schema (tests/test_forest_cpu.py); parity with a real dump is unpinned.
"""
from __future__ import annotations

import json
import math
from typing import Any, Dict, Union

import numpy as np

from ..contracts.transaction import N_FEATURES
from .forest import TreeEnsemble


def _base_score(s: Any) -> float:
    if isinstance(s, (list, tuple)):
        if len(s) != 1:
            raise ValueError(f"base_score has {len(s)} entries; the fraud scorer is binary")
        s = s[0]
    if isinstance(s, str):
        s = s.strip()
        if s.startswith("[") and s.endswith("]"):
            parts = [p for p in s[1:-1].split(",") if p.strip()]
            if len(parts) != 1:
                raise ValueError(f"base_score {s!r}: expected one value")
            s = parts[0]
    p = float(s)
    if not 0.0 < p < 1.0:
        raise ValueError(f"base_score {p} is not a probability in (0, 1)")
    return math.log(p / (1.0 - p))


def from_xgboost_json(doc: Union[str, Dict[str, Any]]) -> TreeEnsemble:
    """XGBoost JSON model (path, JSON text or parsed dict) -> TreeEnsemble."""
    if isinstance(doc, str):
        if doc.lstrip().startswith("{"):
            doc = json.loads(doc)
        else:
            with open(doc) as f:
                doc = json.load(f)
    learner = doc.get("learner")
    if not learner:
        raise ValueError("not an XGBoost JSON model: no 'learner'")
    obj = (learner.get("objective") or {}).get("name")
    if obj != "binary:logistic":
        raise ValueError(f"objective {obj!r}: only binary:logistic is imported")
    gb = learner.get("gradient_booster") or {}
    name = gb.get("name", "gbtree")
    if name != "gbtree":
        raise ValueError(f"booster {name!r}: only gbtree is imported (dart drops trees at inference scale; "
                         "gblinear has no trees)")
    model = gb.get("model") or {}
    trees = model.get("trees")
    if not trees:
        raise ValueError("XGBoost model has no trees")
    lmp = learner.get("learner_model_param") or {}
    if int(lmp.get("num_class", 0) or 0) > 1 or any(int(g) != 0 for g in model.get("tree_info", [])):
        raise ValueError("gbtree with more than one output group (multi-class); the fraud scorer is binary")
    base = _base_score(lmp.get("base_score", "5E-1"))

    feat, value, child, leaf, root = [], [], [], [], []
    cover = [] if all("sum_hessian" in tree for tree in trees) else None
    for t, tree in enumerate(trees):
        left = [int(v) for v in tree["left_children"]]
        right = [int(v) for v in tree["right_children"]]
        split = [int(v) for v in tree["split_indices"]]
        cond = np.asarray(tree["split_conditions"], np.float32)
        if any(int(v) != 0 for v in tree.get("split_type", [])) or tree.get("categories"):
            raise ValueError(f"tree {t}: categorical splits are not supported (transactions are 30 floats)")
        if not (len(left) == len(right) == len(split) == cond.size) or not left:
            raise ValueError(f"tree {t}: inconsistent node arrays")
        base_i = len(feat)
        order = [0]                       # XGBoost node id of our node base_i + i (breadth-first)
        feat.append(0); value.append(0.0); child.append(0); leaf.append(True)
        root.append(base_i)
        i = 0
        while i < len(order):
            s = order[i]
            if left[s] == -1:
                value[base_i + i] = cond[s]
            else:
                if not 0 <= split[s] < N_FEATURES:
                    raise ValueError(f"tree {t}: feature index {split[s]} outside 0..{N_FEATURES - 1}")
                if not (0 <= left[s] < len(left) and 0 <= right[s] < len(left)) or len(order) + 2 > len(left):
                    raise ValueError(f"tree {t}: child index out of range")
                feat[base_i + i] = split[s]
                # left on x < t  <=>  right on x >= t  <=>  x > pred(t)
                value[base_i + i] = np.nextafter(cond[s], np.float32(-np.inf))
                leaf[base_i + i] = False
                child[base_i + i] = base_i + len(order)
                order += [left[s], right[s]]
                for _ in range(2):
                    feat.append(0); value.append(0.0); child.append(0); leaf.append(True)
            i += 1
        if cover is not None:
            hess = np.asarray(tree["sum_hessian"], np.float64)
            if hess.size != len(left):
                raise ValueError(f"tree {t}: sum_hessian has {hess.size} entries for {len(left)} nodes")
            cover.append(hess[order])
    return TreeEnsemble(np.array(feat, np.int32), np.array(value, np.float32), np.array(child, np.int32),
                        np.array(leaf, bool), np.array(root, np.int32), base, "sigmoid",
                        cover=None if cover is None else np.concatenate(cover).astype(np.float32))
