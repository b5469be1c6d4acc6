"""Node classification on the device (reference protocol:
tools/graph_model_downstream_classification.py:58-86).

Per experiment the labelled nodes are split by the configured split algorithm (re-seeded with the
experiment index), a multinomial logistic regression is fitted on the training nodes' input
embeddings and scored on the test nodes. The table stays in fp32 on the device and no float64
copy of the features is made:

  * ``softmax_sums``: dw_node_softmax — loss, gradient, hit count and predictions of one
    evaluation over the rows ``table[ids]``, both products on the float64 MFMA;
  * ``NodeLogisticRegression``: sklearn's objective C * sum(loss) + 0.5 * ||W||^2 (intercepts not
    penalised) minimised by ``linkpred.lbfgs_minimize``, every evaluation one pass. Two classes
    are fitted in sklearn's binary form: one coefficient row w, evaluated as the softmax over
    (0, z), which is the logistic loss;
  * ``node_classification_device``: the experiment loop.

Multi-label node classification, the DeepWalk / node2vec papers' benchmark protocol (a departure:
the reference has no multi-label task), goes through the same pass with another per-sample stage:

  * ``ovr_sums``: dw_node_ovr — loss, gradient, predicted label sets and per-class counts of a
    one-vs-rest logistic regression, a node's labels one uint64 bit mask;
  * ``NodeOvRLogisticRegression``: the sum over classes of sklearn's binary objective, minimised
    jointly (it is separable, so every class ends at its own minimiser) with one pass per
    evaluation;
  * ``micro_macro_f1`` and ``node_multilabel_device``: the metrics and the experiment loop.

``ids`` are vocabulary ids (row 0 = ``<unk>`` is never a sample), ``y`` class indices, ``masks``
int64 arrays or tensors that hold uint64 bit patterns (bit c: the node has label c).
"""
import ctypes
import logging
from typing import Callable, List, Optional

import numpy as np
import torch

from shallow_encoders import _native
from shallow_encoders.graph.linkpred import CLASSIFIER_PARAMS, lbfgs_minimize

logger = logging.getLogger('NodeClassification')

MAX_CLASSES = 64
MAX_DIM = 512

# coef float64 [K, d + 1] -> sums float64 [K * (d + 1) + 2] (dw_node_softmax's out)
Closure = Callable[[np.ndarray], np.ndarray]


def _check_shapes(table: torch.Tensor, ids: torch.Tensor, n_classes: int,
                  min_classes: int = 2) -> None:
    if table.dim() != 2 or table.dtype != torch.float32:
        raise ValueError('table must be a float32 [V, d] device tensor')
    if not 1 <= table.shape[1] <= MAX_DIM:
        raise ValueError(f'embedding size {table.shape[1]} outside [1, {MAX_DIM}]')
    if not min_classes <= int(n_classes) <= MAX_CLASSES:
        raise ValueError(f'n_classes {n_classes} outside [{min_classes}, {MAX_CLASSES}]')
    if ids.dtype != torch.int64 or ids.dim() != 1:
        raise ValueError('ids must be an int64 [n] device tensor')
    if ids.device != table.device:
        raise ValueError('ids and table live on different devices')


def softmax_workspace(n: int, d: int, n_classes: int, device) -> torch.Tensor:
    """A dw_node_softmax workspace for n samples of dimension d and n_classes classes."""
    nb = ctypes.c_size_t(0)
    _native.call('dw_node_softmax_workspace_bytes', int(n), int(d), int(n_classes),
                 ctypes.byref(nb))
    return torch.empty(max(int(nb.value) // 8, 1), dtype=torch.float64, device=device)


def softmax_sums(table: torch.Tensor, ids: torch.Tensor, labels: torch.Tensor,
                 coef: torch.Tensor, n_classes: int, workspace: Optional[torch.Tensor] = None,
                 pred: Optional[torch.Tensor] = None, check: bool = True) -> torch.Tensor:
    """One dw_node_softmax pass: float64 [K * (d + 1) + 2] device tensor (per class sum r_k x and
    sum r_k, then sum loss, then the count of samples whose argmax is their label) at ``coef``
    (float64 [K, d + 1] on the device). ``pred``: an optional int32 [n] destination of the
    argmax (-1 where the sample's id or label is out of range)."""
    _check_shapes(table, ids, n_classes)
    dev = table.device
    n, d, K = ids.shape[0], table.shape[1], int(n_classes)
    if labels.dtype != torch.int32 or labels.shape != (n,) or labels.device != dev:
        raise ValueError('labels must be an int32 [n] tensor on the table\'s device')
    if coef.dtype != torch.float64 or coef.shape != (K, d + 1) or coef.device != dev:
        raise ValueError('coef must be a float64 [n_classes, d + 1] tensor on the table\'s device')
    if pred is not None and (pred.dtype != torch.int32 or pred.shape != (n,)
                             or pred.device != dev):
        raise ValueError('pred must be an int32 [n] tensor on the table\'s device')
    out = torch.zeros(K * (d + 1) + 2, dtype=torch.float64, device=dev)
    if n == 0:
        return out
    if workspace is None:
        workspace = softmax_workspace(n, d, K, dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _native.call('dw_node_softmax', _native.ptr(table.contiguous()), table.shape[0], d,
                     _native.ptr(ids.contiguous()), _native.ptr(labels.contiguous()), n, K,
                     _native.ptr(coef.contiguous()), _native.ptr(out), _native.ptr(pred),
                     _native.ptr(workspace), workspace.numel() * workspace.element_size(),
                     _native.ptr(st), _native.stream(dev))
    if check:
        _native.check_status(st, 'node_softmax')
    return out


class NodeLogisticRegression:
    """Multinomial logistic regression on the rows ``table[ids]`` with sklearn's objective
    C * sum(loss) + 0.5 * ||W||^2 (lbfgs, l2; intercepts not penalised). The features are never
    stored: every objective / gradient evaluation is one dw_node_softmax pass. As sklearn does,
    the classes are those present in the training labels, and two classes are fitted in the
    binary form (``coef_`` has one row, positive for the higher class)."""

    def __init__(self, C: float = 1.0, fit_intercept: bool = True, max_iter: int = 100,
                 tol: float = 1e-4):
        if not C > 0:
            raise ValueError('C must be positive')
        self.C, self.fit_intercept = float(C), bool(fit_intercept)
        self.max_iter, self.tol = int(max_iter), float(tol)
        self.coef_: Optional[np.ndarray] = None        # [K or 1, d]
        self.intercept_: Optional[np.ndarray] = None   # [K or 1]
        self.classes_: Optional[np.ndarray] = None     # class index of each fitted class
        self.n_classes_ = 0
        self.n_iter_ = 0
        self.objective_ = float('nan')

    @classmethod
    def from_params(cls, classifier_params: Optional[dict] = None):
        """From a config's ``classifier_params``: only C, fit_intercept, max_iter and tol."""
        params = dict(classifier_params or {})
        unknown = sorted(set(params) - set(CLASSIFIER_PARAMS))
        if unknown:
            raise ValueError(f'classifier_params {unknown} are not supported by the device '
                             f'backend (supported: {list(CLASSIFIER_PARAMS)})')
        return cls(**params)

    # ---- the driver, without the kernel ------------------------------------------------------
    def objective(self, x: np.ndarray, sums: np.ndarray, d: int, n_classes: int):
        """(objective, gradient) at the free variables ``x`` from one pass's sums at
        ``expand(x)``: the binary form's gradient is row 1 of the two-row pass."""
        K, ld = int(n_classes), d + 1
        sums = np.asarray(sums, dtype=np.float64)
        G = sums[:K * ld].reshape(K, ld)
        W = x.reshape(-1, ld)
        if K == 2:
            G = G[1:2]
        obj = self.C * float(sums[K * ld]) + 0.5 * float(np.sum(W[:, :d] * W[:, :d]))
        grad = self.C * G
        grad[:, :d] += W[:, :d]
        if not self.fit_intercept:
            grad[:, d] = 0.0
        return obj, grad.reshape(-1)

    @staticmethod
    def expand(x: np.ndarray, d: int, n_classes: int) -> np.ndarray:
        """The kernel's [K, d + 1] coefficients of the free variables: K rows, or [0; w]."""
        W = np.asarray(x, dtype=np.float64).reshape(-1, d + 1)
        if int(n_classes) == 2:
            W = np.concatenate([np.zeros((1, d + 1)), W])
        return np.ascontiguousarray(W)

    def fit_closure(self, closure: Closure, d: int, n_classes: int) -> 'NodeLogisticRegression':
        """Fit through ``closure: coef [K, d + 1] -> sums [K (d + 1) + 2]`` — the sums of any
        implementation of dw_node_softmax's contract."""
        K = int(n_classes)
        if not 2 <= K <= MAX_CLASSES:
            raise ValueError(f'n_classes {K} outside [2, {MAX_CLASSES}]')
        rows = 1 if K == 2 else K

        def f(x):
            return self.objective(x, closure(self.expand(x, d, K)), d, K)
        x, obj, it = lbfgs_minimize(f, np.zeros(rows * (d + 1)), self.max_iter, self.tol)
        W = x.reshape(rows, d + 1)
        self.coef_, self.intercept_ = W[:, :d].copy(), W[:, d].copy()
        self.n_classes_, self.objective_, self.n_iter_ = K, obj, it
        if self.classes_ is None or len(self.classes_) != K:
            self.classes_ = np.arange(K)
        return self

    def full_coef(self) -> np.ndarray:
        """float64 [K, d + 1]: the coefficients as dw_node_softmax takes them."""
        if self.coef_ is None:
            raise RuntimeError('fit first')
        x = np.concatenate([self.coef_, self.intercept_[:, None]], axis=1)
        return self.expand(x, self.coef_.shape[1], self.n_classes_)

    # ---- on the device ---------------------------------------------------------------------
    def fit(self, table: torch.Tensor, ids: torch.Tensor, y) -> 'NodeLogisticRegression':
        """``y``: one class index per id (any integer array or tensor)."""
        y = np.asarray(y.cpu() if isinstance(y, torch.Tensor) else y).astype(np.int64)
        if ids.shape[0] == 0 or y.shape != (ids.shape[0],):
            raise ValueError('fit needs at least one sample and one label per id')
        classes, local = np.unique(y, return_inverse=True)
        if len(classes) < 2:
            raise ValueError('fit needs samples of at least 2 classes, got '
                             f'{len(classes)}')
        K = len(classes)
        _check_shapes(table, ids, K)
        table, ids = table.contiguous(), ids.contiguous()
        dev, d = table.device, table.shape[1]
        labels = torch.from_numpy(local.astype(np.int32)).to(dev)
        ws = softmax_workspace(ids.shape[0], d, K, dev)

        def sums(coef: np.ndarray) -> np.ndarray:
            c = torch.from_numpy(coef).to(dev)
            return softmax_sums(table, ids, labels, c, K, ws).cpu().numpy()
        self.classes_ = classes
        return self.fit_closure(sums, d, K)

    def predict(self, table: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
        """int64 [n] device tensor of class indices: the argmax of the logits, ties to the
        lowest class."""
        coef = torch.from_numpy(self.full_coef()).to(table.device)
        n = ids.shape[0]
        pred = torch.full((n,), -1, dtype=torch.int32, device=table.device)
        if n:
            labels = torch.zeros(n, dtype=torch.int32, device=table.device)
            softmax_sums(table, ids, labels, coef, self.n_classes_, pred=pred)
        classes = torch.from_numpy(np.asarray(self.classes_, dtype=np.int64)).to(table.device)
        return classes[pred.to(torch.int64)]

    def score(self, table: torch.Tensor, ids: torch.Tensor, y) -> float:
        """Accuracy: the share of samples whose prediction is their class."""
        y = torch.as_tensor(np.asarray(y.cpu() if isinstance(y, torch.Tensor) else y)
                            .astype(np.int64)).to(table.device)
        return int((self.predict(table, ids) == y).sum()) / ids.shape[0]


def macro_f1(confusion: np.ndarray) -> float:
    """Macro-averaged F1 of a confusion matrix [true, predicted] (sklearn's f1_score with
    average='macro' over the classes that occur; a class without a true positive scores 0)."""
    c = np.asarray(confusion, dtype=np.float64)
    tp = np.diag(c)
    denom = c.sum(axis=0) + c.sum(axis=1)
    seen = denom > 0
    return float(np.mean(2 * tp[seen] / denom[seen])) if seen.any() else 0.0


def node_classification_device(table: torch.Tensor, rows, y, split_algorithm,
                               n_experiments: int, classifier_params: Optional[dict] = None,
                               device=None, return_accuracies: bool = False):
    """(mean accuracy, best accuracy, confusion counts [true, predicted] of the best experiment)
    over ``n_experiments``, plus the per-experiment accuracies with ``return_accuracies``.
    ``table``: float32 [V, d] input embeddings; ``rows``: the labelled nodes' vocabulary ids;
    ``y``: their class indices. The split algorithms never look at X's values, so splitting the
    index column gives exactly the partitions the host path gets from the feature matrix."""
    NodeLogisticRegression.from_params(classifier_params)   # refuse early
    rows = np.asarray(rows, dtype=np.int64)
    y_host = np.asarray(y)
    n = len(rows)
    if n == 0 or y_host.shape != (n,):
        raise ValueError('node classification needs labelled nodes and one label per node')
    yi = y_host.astype(np.int64)
    K = int(yi.max()) + 1
    dev = _native.require_device(device if device is not None else
                                 (table.device if table.is_cuda else None))
    table = table.to(device=dev, dtype=torch.float32).contiguous()
    rows_d = torch.from_numpy(rows).to(dev)
    index = np.arange(n)[:, None]
    accs: List[float] = []
    best, best_conf = None, None
    for i in range(n_experiments):
        split_algorithm.random_state = i
        sp = split_algorithm(index, y_host)
        tr, te = sp['X_train'][:, 0], sp['X_test'][:, 0]
        clf = NodeLogisticRegression.from_params(classifier_params)
        clf.fit(table, rows_d[torch.from_numpy(tr).to(dev)], yi[tr])
        pred = clf.predict(table, rows_d[torch.from_numpy(te).to(dev)])
        truth = torch.from_numpy(yi[te]).to(dev)
        acc = int((pred == truth).sum()) / len(te)   # the correctly rounded fraction
        logger.info(f'Experiment {i}: accuracy {100 * acc:.2f}% ({clf.n_iter_} L-BFGS '
                    f'iterations, objective {clf.objective_:.6g}).')
        accs.append(acc)
        if best is None or acc >= best:
            best = acc
            best_conf = torch.bincount(truth * K + pred, minlength=K * K).reshape(K, K)
    assert best is not None, 'No experiments performed!'
    mean = float(np.mean(accs))
    confusion = best_conf.cpu().numpy()
    logger.info(f'Node classification accuracy (device): {100 * mean:.2f}% (averaged over '
                f'{n_experiments} experiments); best {100 * best:.2f}%.')
    if return_accuracies:
        return mean, best, confusion, accs
    return mean, best, confusion


# ---- multi-label: one-vs-rest --------------------------------------------------------------------
RULES = {'threshold': _native.DW_OVR_THRESHOLD, 'top_k': _native.DW_OVR_TOP_K}


def _rule_id(rule) -> int:
    if rule in RULES:
        return RULES[rule]
    if rule in RULES.values():
        return int(rule)
    raise ValueError(f'rule must be one of {list(RULES)}, got {rule!r}')


def ovr_workspace(n: int, d: int, n_classes: int, device) -> torch.Tensor:
    """A dw_node_ovr workspace for n samples of dimension d and n_classes classes."""
    nb = ctypes.c_size_t(0)
    _native.call('dw_node_ovr_workspace_bytes', int(n), int(d), int(n_classes), ctypes.byref(nb))
    return torch.empty(max(int(nb.value) // 8, 1), dtype=torch.float64, device=device)


def ovr_sums(table: torch.Tensor, ids: torch.Tensor, masks: torch.Tensor, coef: torch.Tensor,
             n_classes: int, rule='top_k', workspace: Optional[torch.Tensor] = None,
             pred: Optional[torch.Tensor] = None, check: bool = True) -> torch.Tensor:
    """One dw_node_ovr pass: float64 [K * (d + 1) + 1 + 3 K] device tensor (per class sum r_c x
    and sum r_c, then sum loss, then tp[K], predicted[K] and true[K] under ``rule``) at ``coef``
    (float64 [K, d + 1] on the device). ``masks``: int64 [n] holding the uint64 label masks.
    ``pred``: an optional int64 [n] destination of the predicted masks (0 where the sample's id
    or mask is out of range)."""
    _check_shapes(table, ids, n_classes, min_classes=1)
    rule = _rule_id(rule)
    dev = table.device
    n, d, K = ids.shape[0], table.shape[1], int(n_classes)
    if masks.dtype != torch.int64 or masks.shape != (n,) or masks.device != dev:
        raise ValueError('masks must be an int64 [n] tensor on the table\'s device')
    if coef.dtype != torch.float64 or coef.shape != (K, d + 1) or coef.device != dev:
        raise ValueError('coef must be a float64 [n_classes, d + 1] tensor on the table\'s device')
    if pred is not None and (pred.dtype != torch.int64 or pred.shape != (n,)
                             or pred.device != dev):
        raise ValueError('pred must be an int64 [n] tensor on the table\'s device')
    out = torch.zeros(K * (d + 1) + 1 + 3 * K, dtype=torch.float64, device=dev)
    if n == 0:
        return out
    if workspace is None:
        workspace = ovr_workspace(n, d, K, dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _native.call('dw_node_ovr', _native.ptr(table.contiguous()), table.shape[0], d,
                     _native.ptr(ids.contiguous()), _native.ptr(masks.contiguous()), n, K,
                     _native.ptr(coef.contiguous()), rule, _native.ptr(out), _native.ptr(pred),
                     _native.ptr(workspace), workspace.numel() * workspace.element_size(),
                     _native.ptr(st), _native.stream(dev))
    if check:
        _native.check_status(st, 'node_ovr')
    return out


def _host_masks(masks) -> np.ndarray:
    """uint64 [n] view of label masks given as an int64 / uint64 array or tensor."""
    m = np.asarray(masks.cpu() if isinstance(masks, torch.Tensor) else masks)
    if m.dtype.kind not in 'iu' or m.ndim != 1:
        raise ValueError('masks must be a 1-d integer array of uint64 bit patterns')
    if m.dtype != np.uint64:
        m = m.astype(np.int64)
    return np.ascontiguousarray(m).view(np.uint64)


def mask_bits(masks, n_classes: int) -> np.ndarray:
    """bool [n, K] indicator matrix of label masks."""
    m = _host_masks(masks)
    return ((m[:, None] >> np.arange(n_classes, dtype=np.uint64)) & np.uint64(1)).astype(bool)


def bits_mask(bits: np.ndarray, classes=None) -> np.ndarray:
    """int64 [n] label masks (uint64 bit patterns) of a bool [n, len(classes)] matrix whose
    column i is class ``classes[i]`` (default: i)."""
    bits = np.asarray(bits, dtype=bool)
    classes = np.arange(bits.shape[1]) if classes is None else np.asarray(classes)
    out = np.zeros(bits.shape[0], dtype=np.uint64)
    for i, c in enumerate(classes):
        out |= bits[:, i].astype(np.uint64) << np.uint64(c)
    return out.view(np.int64)


class NodeOvRLogisticRegression:
    """One-vs-rest logistic regression on the rows ``table[ids]``: per class sklearn's binary
    objective C * sum(loss) + 0.5 * ||w_c||^2 (lbfgs, l2; intercepts not penalised), what
    ``OneVsRestClassifier(LogisticRegression())`` fits class by class. The sum of the K
    objectives is minimised jointly over the K (d + 1) free variables: it is separable, so the
    joint minimiser is every class's own, and a fit costs ``n_iter_`` dw_node_ovr passes instead
    of one series of passes per class; ``max_iter`` bounds the joint iterations, where sklearn's
    bounds each class's, so nearly separable labels want a larger one. A class that no training node or every training node has
    is not a problem of two classes: the first is left unfitted and never predicted, the second
    is a ValueError. ``classes_`` are the fitted classes, in which order the kernel sees them."""

    def __init__(self, C: float = 1.0, fit_intercept: bool = True, max_iter: int = 100,
                 tol: float = 1e-4):
        if not C > 0:
            raise ValueError('C must be positive')
        self.C, self.fit_intercept = float(C), bool(fit_intercept)
        self.max_iter, self.tol = int(max_iter), float(tol)
        self.coef_: Optional[np.ndarray] = None        # [fitted classes, d]
        self.intercept_: Optional[np.ndarray] = None   # [fitted classes]
        self.classes_: Optional[np.ndarray] = None     # label index of each fitted class
        self.n_labels_ = 0                             # labels the masks range over
        self.n_iter_ = 0
        self.objective_ = float('nan')

    from_params = classmethod(NodeLogisticRegression.from_params.__func__)

    # ---- the driver, without the kernel ------------------------------------------------------
    def objective(self, x: np.ndarray, sums: np.ndarray, d: int, n_classes: int):
        """(objective, gradient) at the free variables ``x`` [K (d + 1)] from one pass's sums."""
        K, ld = int(n_classes), d + 1
        sums = np.asarray(sums, dtype=np.float64)
        W = x.reshape(K, ld)
        obj = self.C * float(sums[K * ld]) + 0.5 * float(np.sum(W[:, :d] * W[:, :d]))
        grad = self.C * sums[:K * ld].reshape(K, ld)
        grad[:, :d] += W[:, :d]
        if not self.fit_intercept:
            grad[:, d] = 0.0
        return obj, grad.reshape(-1)

    def fit_closure(self, closure: Closure, d: int, n_classes: int) -> 'NodeOvRLogisticRegression':
        """Fit through ``closure: coef [K, d + 1] -> sums [K (d + 1) + 1 + 3 K]`` — the sums of
        any implementation of dw_node_ovr's contract (the counts are not read)."""
        K = int(n_classes)
        if not 1 <= K <= MAX_CLASSES:
            raise ValueError(f'n_classes {K} outside [1, {MAX_CLASSES}]')

        def f(x):
            return self.objective(x, closure(np.ascontiguousarray(x.reshape(K, d + 1))), d, K)
        x, obj, it = lbfgs_minimize(f, np.zeros(K * (d + 1)), self.max_iter, self.tol)
        if it >= self.max_iter:   # sklearn's max_iter counts per class, this one for all K
            logger.warning(f'the joint one-vs-rest fit of {K} classes used all of its '
                           f'max_iter={self.max_iter} iterations: raise max_iter')
        W = x.reshape(K, d + 1)
        self.coef_, self.intercept_ = W[:, :d].copy(), W[:, d].copy()
        self.objective_, self.n_iter_ = obj, it
        if self.classes_ is None or len(self.classes_) != K:
            self.classes_, self.n_labels_ = np.arange(K), K
        return self

    def full_coef(self) -> np.ndarray:
        """float64 [fitted classes, d + 1]: the coefficients as dw_node_ovr takes them."""
        if self.coef_ is None:
            raise RuntimeError('fit first')
        return np.ascontiguousarray(np.concatenate([self.coef_, self.intercept_[:, None]], axis=1))

    def fitted_classes(self, masks, n_classes: int) -> np.ndarray:
        """The classes that some but not all of the training masks carry; an all-positive class
        is a ValueError."""
        bits = mask_bits(masks, n_classes)
        if (_host_masks(masks) >> np.uint64(n_classes - 1) >> np.uint64(1)).any():
            raise ValueError(f'a mask has a label at or above n_classes = {n_classes}')
        pos = bits.sum(axis=0)
        if (pos == len(bits)).any():
            raise ValueError(f'every training node has label {int(np.argmax(pos == len(bits)))}: '
                             f'a one-vs-rest class needs a node without it')
        return np.flatnonzero(pos > 0)

    def compact(self, masks) -> np.ndarray:
        """int64 [n]: the masks over the fitted classes, bit i = label ``classes_[i]``."""
        return bits_mask(mask_bits(masks, self.n_labels_)[:, self.classes_])

    # ---- on the device ---------------------------------------------------------------------
    def fit(self, table: torch.Tensor, ids: torch.Tensor, masks,
            n_classes: int) -> 'NodeOvRLogisticRegression':
        """``masks``: one label mask per id over ``n_classes`` labels."""
        K = int(n_classes)
        if not 1 <= K <= MAX_CLASSES:
            raise ValueError(f'n_classes {K} outside [1, {MAX_CLASSES}]')
        if ids.shape[0] == 0 or _host_masks(masks).shape != (ids.shape[0],):
            raise ValueError('fit needs at least one sample and one mask per id')
        self.classes_, self.n_labels_ = self.fitted_classes(masks, K), K
        F = len(self.classes_)
        if F == 0:
            raise ValueError('fit needs at least one label that some training node has')
        _check_shapes(table, ids, F, min_classes=1)
        table, ids = table.contiguous(), ids.contiguous()
        dev, d = table.device, table.shape[1]
        m = torch.from_numpy(self.compact(masks)).to(dev)
        ws = ovr_workspace(ids.shape[0], d, F, dev)

        def sums(coef: np.ndarray) -> np.ndarray:
            c = torch.from_numpy(coef).to(dev)
            return ovr_sums(table, ids, m, c, F, 'threshold', ws).cpu().numpy()
        return self.fit_closure(sums, d, F)

    def _pass(self, table, ids, masks, rule):
        """(predicted masks over all labels int64 [n] on the device, the pass's sums on the
        host) at the fitted coefficients; the sums' counts are over the fitted classes."""
        rule = _rule_id(rule)
        n, F, dev = ids.shape[0], len(self.classes_), table.device
        if masks is None:
            if rule == RULES['top_k']:
                raise ValueError('the top-k rule needs the nodes\' masks: it predicts as many '
                                 'labels as a node has')
            m = torch.zeros(n, dtype=torch.int64, device=dev)
        else:
            m = torch.from_numpy(self.compact(masks)).to(dev)
        pred = torch.zeros(n, dtype=torch.int64, device=dev)
        coef = torch.from_numpy(self.full_coef()).to(dev)
        sums = ovr_sums(table, ids, m, coef, F, rule, pred=pred).cpu().numpy()
        if not np.array_equal(self.classes_, np.arange(F)):   # back to the labels' own bits
            full = torch.zeros_like(pred)
            for i, c in enumerate(self.classes_):
                full |= ((pred >> i) & 1) << int(c)
            pred = full
        return pred, sums

    def predict(self, table: torch.Tensor, ids: torch.Tensor, masks=None,
                rule='top_k') -> torch.Tensor:
        """int64 [n] device tensor of predicted label masks (uint64 bit patterns). ``rule``
        'threshold': every fitted class whose decision function is positive (sklearn's
        predict). 'top_k': as many labels as ``masks`` gives the node among the fitted classes,
        from the top of its ranking, ties to the lowest class."""
        return self._pass(table, ids, masks, rule)[0]

    def counts(self, table: torch.Tensor, ids: torch.Tensor, masks, rule='top_k'):
        """(tp, n_pred, n_true) int64 [n_labels_] of the predictions against ``masks``: the
        kernel's counts at the fitted classes; a true label of an unfitted class is never
        predicted, so it is a false negative of its class."""
        K, F = self.n_labels_, len(self.classes_)
        sums = self._pass(table, ids, masks, rule)[1]
        tail = sums[-3 * F:].reshape(3, F).astype(np.int64)
        out = np.zeros((3, K), dtype=np.int64)
        out[2] = mask_bits(masks, K).sum(axis=0)
        assert np.array_equal(out[2][self.classes_], tail[2])
        out[:2, self.classes_] = tail[:2]
        return out[0], out[1], out[2]


def micro_macro_f1(tp, n_pred, n_true):
    """(micro-F1, macro-F1) from per-class counts of true positives, predicted and true labels:
    sklearn's f1_score(Y, P, average=..., zero_division=0) on the indicator matrices, macro over
    all K columns (a class neither present nor predicted scores 0)."""
    tp, denom = np.asarray(tp, dtype=np.float64), np.asarray(n_pred, dtype=np.float64) + n_true
    micro = float(2 * tp.sum() / denom.sum()) if denom.sum() > 0 else 0.0
    per = np.divide(2 * tp, denom, out=np.zeros_like(tp), where=denom > 0)
    return micro, float(per.mean())


def node_multilabel_device(table: torch.Tensor, rows, masks, split_algorithm, n_experiments: int,
                           classifier_params: Optional[dict] = None, rule='top_k', device=None,
                           return_scores: bool = False, n_classes: Optional[int] = None):
    """(mean micro-F1, mean macro-F1, best micro-F1) over ``n_experiments``, plus the
    per-experiment (micro, macro) pairs with ``return_scores``. ``table``: float32 [V, d] input
    embeddings; ``rows``: the labelled nodes' vocabulary ids; ``masks``: their label masks;
    ``n_classes``: the number of labels (default: the highest bit set, plus one). As in
    ``node_classification_device`` the split is re-seeded per experiment and splits the index
    column, with the masks as its opaque 1-D ``y``. A stratified split would treat every distinct
    mask as a class of its own: it is not supported, and sklearn's own error (a class with one
    member) surfaces unchanged."""
    NodeOvRLogisticRegression.from_params(classifier_params)   # refuse early
    _rule_id(rule)
    rows = np.asarray(rows, dtype=np.int64)
    m_host = _host_masks(masks).view(np.int64)
    n = len(rows)
    if n == 0 or m_host.shape != (n,):
        raise ValueError('node classification needs labelled nodes and one mask per node')
    K = int(n_classes) if n_classes is not None else \
        max(int(np.bitwise_or.reduce(m_host.view(np.uint64))).bit_length(), 1)
    dev = _native.require_device(device if device is not None else
                                 (table.device if table.is_cuda else None))
    table = table.to(device=dev, dtype=torch.float32).contiguous()
    rows_d = torch.from_numpy(rows).to(dev)
    index = np.arange(n)[:, None]
    scores = []
    for i in range(n_experiments):
        split_algorithm.random_state = i
        sp = split_algorithm(index, m_host)
        tr, te = sp['X_train'][:, 0], sp['X_test'][:, 0]
        clf = NodeOvRLogisticRegression.from_params(classifier_params)
        clf.fit(table, rows_d[torch.from_numpy(tr).to(dev)], m_host[tr], K)
        micro, macro = micro_macro_f1(*clf.counts(
            table, rows_d[torch.from_numpy(te).to(dev)], m_host[te], rule))
        logger.info(f'Experiment {i}: micro-F1 {100 * micro:.2f}%, macro-F1 {100 * macro:.2f}% '
                    f'({clf.n_iter_} L-BFGS iterations, {len(clf.classes_)} of {K} classes '
                    f'fitted).')
        scores.append((micro, macro))
    assert scores, 'No experiments performed!'
    mean_micro, mean_macro = (float(v) for v in np.mean(scores, axis=0))
    best = max(s[0] for s in scores)
    logger.info(f'Multi-label node classification (device, {rule}): micro-F1 '
                f'{100 * mean_micro:.2f}%, macro-F1 {100 * mean_macro:.2f}% (averaged over '
                f'{n_experiments} experiments); best micro-F1 {100 * best:.2f}%.')
    if return_scores:
        return mean_micro, mean_macro, best, scores
    return mean_micro, mean_macro, best
