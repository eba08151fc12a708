"""scikit-learn model import: bring a fraud model trained in the reference's Python workbench
(the JupyterHub / Spark notebooks, deploy/frauddetection_cr.yaml:7-53; the Seldon
``modelfull`` container serves a Python model, deploy/model/modelfull.json:24) onto the
MI355X kernels.

Accepted estimators, fitted on the 30 transaction columns (Time, V1..V28, Amount):

* ``LogisticRegression`` (binary)                       -> ``LogisticModel`` (K2 kernel);
* ``MLPClassifier(hidden_layer_sizes=(128, 64), activation="relu")`` (binary)
                                                       -> ``MLPModel`` (K3 MFMA kernel);
* either of them behind a ``StandardScaler`` in a ``Pipeline`` (or ``make_pipeline``): the
  scaler becomes the model's ``Normalizer`` (mu = mean_, 1/sigma = 1/scale_), which the
  kernels fuse into their prologue -- or, on W64 rows, fold into the first layer;
* ``DecisionTreeClassifier``, ``RandomForestClassifier``, ``ExtraTreesClassifier`` (binary)
                                                       -> ``TreeEnsemble`` (general-tree kernel):
  leaf value = class-1 fraction of ``tree_.value`` / T, identity link, base 0;
* ``GradientBoostingClassifier`` (log-loss, default prior init) -> ``TreeEnsemble``:
  base = log(prior_1 / prior_0), leaf value = learning_rate * value, sigmoid link.
  Every tree model carries ``tree_.weighted_n_node_samples`` as the ensemble's ``cover``, the
  background of its Shapley attributions (models/explain_forest.py).

Trees take RAW features: a ``StandardScaler`` in front of a tree model is refused (the tree
kernels have no normaliser; refit the trees on raw columns, they are scale invariant).

Threshold rounding.  scikit-learn sends a row left on ``x <= t`` with float32 ``x`` and a
float64 ``t``; the kernels go right on ``x > thr`` with a float32 ``thr``.  The two agree for
every float32 ``x`` only when ``thr`` is the LARGEST float32 <= t (rounded toward -inf):
round-to-nearest can land above ``t`` and then sends ``x = float32(t)`` left where
scikit-learn sends it right.

The MLP kernel is specialised to 30 -> 128 -> 64 -> 1; other architectures are refused
with a clear error.  The estimator object is taken as-is: loading it from disk (joblib /
pickle) is the caller's decision -- only ever do that with files you produced yourself.

    from ccfd_demo_summit_amd.models.sklearn_import import from_sklearn
    model = from_sklearn(fitted_pipeline)      # then save_model(model, "m.safetensors")
"""
from __future__ import annotations

from typing import Any, Optional

import numpy as np

from ..contracts.transaction import N_FEATURES
from .common import Normalizer
from .forest import TreeEnsemble
from .lr import LogisticModel
from .mlp import H1, H2, MLPModel


def _normalizer(scaler: Optional[Any]) -> Normalizer:
    if scaler is None:
        return Normalizer.identity()
    name = type(scaler).__name__
    if name != "StandardScaler":
        raise ValueError(f"unsupported preprocessing step {name} (only StandardScaler folds into the kernels)")
    mean = getattr(scaler, "mean_", None)
    scale = getattr(scaler, "scale_", None)
    mu = np.zeros(N_FEATURES, np.float32) if mean is None else np.asarray(mean, np.float32)
    isg = np.ones(N_FEATURES, np.float32) if scale is None else (1.0 / np.asarray(scale, np.float64)).astype(np.float32)
    if mu.shape != (N_FEATURES,) or isg.shape != (N_FEATURES,):
        raise ValueError(f"scaler was fitted on {mu.shape[0]} features, transactions have {N_FEATURES}")
    return Normalizer(mu, isg, log_amount=False)


def _binary(est: Any) -> None:
    classes = getattr(est, "classes_", None)
    if classes is None:
        raise ValueError(f"{type(est).__name__} is not fitted")
    if len(classes) != 2:
        raise ValueError(f"{type(est).__name__} has {len(classes)} classes; the fraud scorer is binary")


def f32_floor(t: np.ndarray) -> np.ndarray:
    """The largest float32 <= t, elementwise (float64 in): float32(t) stepped down where
    round-to-nearest went above t."""
    t = np.asarray(t, np.float64)
    r = t.astype(np.float32)
    return np.where(r.astype(np.float64) > t, np.nextafter(r, np.float32(-np.inf)), r).astype(np.float32)


_FORESTS = ("DecisionTreeClassifier", "RandomForestClassifier", "ExtraTreesClassifier")
_TREE_MODELS = _FORESTS + ("GradientBoostingClassifier",)


def _sk_trees(trees, leaf_value) -> tuple:
    """Concatenate sklearn ``tree_`` objects into TreeEnsemble arrays.  sklearn stores children
    anywhere (depth-first); each inner node's two children get a fresh adjacent pair here,
    in breadth-first order per tree, so child indices point forward.  Returns (the five node
    arrays, cover): ``weighted_n_node_samples`` re-indexed like the nodes."""
    feat, value, child, leaf, root, cover = [], [], [], [], [], []
    for k, tr in enumerate(trees):
        left, right = tr.children_left, tr.children_right
        thr = f32_floor(tr.threshold)
        lv = leaf_value(k, tr)                       # float64 [node_count]
        if tr.n_features != N_FEATURES:
            raise ValueError(f"tree was fitted on {tr.n_features} features, transactions have {N_FEATURES}")
        base = len(feat)
        order = [0]                                  # sklearn node id of our node base + i
        feat.append(0); value.append(0.0); child.append(0); leaf.append(True)
        root.append(base)
        i = 0
        while i < len(order):
            s = order[i]
            if left[s] == -1:
                value[base + i] = np.float32(lv[s])
            else:
                feat[base + i] = int(tr.feature[s])
                value[base + i] = thr[s]
                leaf[base + i] = False
                child[base + i] = base + len(order)
                order += [int(left[s]), int(right[s])]
                for _ in range(2):
                    feat.append(0); value.append(0.0); child.append(0); leaf.append(True)
            i += 1
        cover.append(np.asarray(tr.weighted_n_node_samples, np.float64)[order])
    return (np.array(feat, np.int32), np.array(value, np.float32), np.array(child, np.int32),
            np.array(leaf, bool), np.array(root, np.int32)), np.concatenate(cover).astype(np.float32)


def _forest(est: Any, name: str) -> TreeEnsemble:
    if name in _FORESTS:
        trees = [est.tree_] if name == "DecisionTreeClassifier" else [e.tree_ for e in est.estimators_]
        if getattr(est, "n_outputs_", 1) != 1:
            raise ValueError(f"{name} has {est.n_outputs_} outputs; the fraud scorer has one")
        T = len(trees)

        def frac(_k, tr):                            # class-1 fraction of the node's samples, / T
            v = np.asarray(tr.value, np.float64)[:, 0, :]
            return v[:, 1] / v.sum(1) / T
        arrays, cover = _sk_trees(trees, frac)
        return TreeEnsemble(*arrays, 0.0, "identity", cover=cover)
    loss = getattr(est, "loss", "log_loss")
    if loss not in ("log_loss", "deviance"):
        raise ValueError(f"GradientBoostingClassifier loss {loss!r}: only log-loss maps onto the sigmoid link")
    init = getattr(est, "init", None)
    if init == "zero":
        base = 0.0
    elif init is None:
        prior = np.asarray(est.init_.class_prior_, np.float64)
        if prior.shape != (2,) or not (prior > 0).all():
            raise ValueError("GradientBoostingClassifier prior init needs both classes in the training data")
        base = float(np.log(prior[1] / prior[0]))
    else:
        raise ValueError(f"GradientBoostingClassifier init={type(init).__name__}: only the default class-prior "
                         "init (init=None) or init='zero' is imported")
    trees = [e.tree_ for e in np.asarray(est.estimators_)[:, 0]]
    lr = float(est.learning_rate)
    arrays, cover = _sk_trees(trees, lambda _k, tr: lr * np.asarray(tr.value, np.float64)[:, 0, 0])
    return TreeEnsemble(*arrays, base, "sigmoid", cover=cover)


def from_sklearn(est: Any) -> Any:
    """Fitted scikit-learn estimator or ``Pipeline`` -> LogisticModel / MLPModel / TreeEnsemble
    whose ``predict_proba`` equals the estimator's ``predict_proba(X)[:, 1]`` (up to float32)."""
    scaler = None
    if type(est).__name__ == "Pipeline":
        steps = [s for _, s in est.steps if s is not None and s != "passthrough"]
        if not steps:
            raise ValueError("empty pipeline")
        *pre, est = steps
        if len(pre) > 1:
            raise ValueError(f"pipeline has {len(pre)} preprocessing steps; at most one StandardScaler folds in")
        scaler = pre[0] if pre else None
    name = type(est).__name__
    if name in _TREE_MODELS:
        if scaler is not None:
            raise ValueError(f"{name} behind a {type(scaler).__name__}: trees take raw features (the tree kernels "
                             "have no normaliser; fit the trees on the raw transaction columns)")
        _binary(est)
        return _forest(est, name)
    norm = _normalizer(scaler)
    _binary(est)
    if name == "LogisticRegression":
        coef = np.asarray(est.coef_, np.float64)
        if coef.shape != (1, N_FEATURES):
            raise ValueError(f"LogisticRegression coef_ shape {coef.shape}, expected (1, {N_FEATURES})")
        return LogisticModel(coef[0].astype(np.float32), float(np.asarray(est.intercept_)[0]), norm)
    if name == "MLPClassifier":
        if est.activation != "relu":
            raise ValueError(f"MLPClassifier activation {est.activation!r}: the kernel implements relu")
        shapes = [tuple(w.shape) for w in est.coefs_]
        want = [(N_FEATURES, H1), (H1, H2), (H2, 1)]
        if shapes != want:
            raise ValueError(f"MLPClassifier layer shapes {shapes}; the MLP kernel is 30 -> {H1} -> {H2} -> 1 "
                             f"(hidden_layer_sizes=({H1}, {H2}))")
        W1, W2, W3 = (np.asarray(w, np.float32) for w in est.coefs_)
        b1, b2, b3 = (np.asarray(b, np.float32) for b in est.intercepts_)
        return MLPModel(W1.T.copy(), b1.copy(), W2.T.copy(), b2.copy(), W3[:, 0].copy(), float(b3[0]), norm)
    raise ValueError(f"unsupported estimator {name}: LogisticRegression or MLPClassifier (optionally after a "
                     "StandardScaler), DecisionTree / RandomForest / ExtraTrees / GradientBoosting classifiers "
                     "(raw features) map onto the kernels; CatBoost imports via models.gbdt_import, XGBoost via "
                     "models.xgboost_import")
