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

``ids`` are vocabulary ids (row 0 = ``<unk>`` is never a sample), ``y`` class indices.
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


def _check_shapes(table: torch.Tensor, ids: torch.Tensor, n_classes: int) -> None:
    if table.dim() != 2 or table.dtype != torch.float32:
        raise ValueError('table must be a float32 [V, d] device tensor')
    if not 1 <= table.shape[1] <= MAX_DIM:
        raise ValueError(f'embedding size {table.shape[1]} outside [1, {MAX_DIM}]')
    if not 2 <= int(n_classes) <= MAX_CLASSES:
        raise ValueError(f'n_classes {n_classes} outside [2, {MAX_CLASSES}]')
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
