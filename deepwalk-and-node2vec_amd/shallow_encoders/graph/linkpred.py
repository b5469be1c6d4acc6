"""Link prediction on the device (reference protocol:
tools/graph_model_downstream_classification.py:170-200, 241-299).

Per experiment the edges are shuffled, the first round(train_ratio * E) are the positive
training edges, as many negative pairs are sampled for training and E - n_train more for
evaluation, a logistic regression is fitted on operator(n1, n2) and scored on all edges plus
both negative sets. Everything that scales with E runs on the device and no feature matrix is
stored:

  * ``negative_edges``: dw_negative_edges — u uniform over the nodes, v the k-th non-neighbour of
    u by rank (one Philox call, one binary search of u's sorted row; no rejection);
  * ``edge_embeddings_device``: dw_edge_features — edge_operators.edge_embeddings in float32;
  * ``EdgeLogisticRegression``: sklearn's objective C * sum(loss) + 0.5 * ||w||^2 (intercept not
    penalised) minimised by L-BFGS over the float64 (d + 1)-vector, every evaluation one
    dw_edge_logreg pass over the pairs (loss, gradient and accuracy sums in float64);
  * ``edge_classification_device``: the experiment loop.

Held-out link prediction (node2vec §4.4) reuses the sampler and the fit on a
graph whose test edges were hidden before training (graph/holdout.py):

  * ``edge_scores`` / ``EdgeLogisticRegression.decision_function``: dw_edge_scores — the score
    z of every pair, the same gather as the fit's pass;
  * ``roc_auc`` / ``roc_auc_counts``: dw_roc_auc — the tie-aware Mann-Whitney count as exact
    integers, divided once on the host;
  * ``heldout_edge_classification``: fit on the train graph's edges, rank the held edges against
    fresh non-edges of the full graph.

The graph is a ``CSRGraph`` in vocabulary ids (row 0 = ``<unk>``, nodes 1 .. V - 1).
"""
import ctypes
import logging
from typing import Callable, List, Optional, Tuple

import numpy as np
import torch

from shallow_encoders import _native
from shallow_encoders.graph.edge_operators import EDGE_OPERATORS

logger = logging.getLogger('LinkPrediction')

FIRST_NODE = 1   # row 0 of a CSRGraph is <unk>
OPERATOR_IDS = {name: i for i, name in enumerate(
    ('average', 'hadamard', 'weighted_l1', 'weighted_l2'))}
CLASSIFIER_PARAMS = ('C', 'fit_intercept', 'max_iter', 'tol')


def operator_id(name: str) -> int:
    """dw_edge_features / dw_edge_logreg op of an operator name (edge_operator_factory's names
    and its AssertionError for an unknown one)."""
    name = name.lower()
    assert name in EDGE_OPERATORS, \
        f'Operator "{name}" is not supported. Available: {list(EDGE_OPERATORS.keys())}'
    return OPERATOR_IDS[name]


# ------------------------------------------------------------------------------ negative pairs
def check_negative_graph(row_ptr: np.ndarray, first_node: int = FIRST_NODE,
                         simple_status: int = 0) -> None:
    """Refuse a graph dw_negative_edges cannot sample: a repeated neighbour (``simple_status``:
    the word dw_csr_check_simple left), neighbours on the rows below ``first_node``, or a node
    adjacent to every node (itself included), which has no non-neighbour."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    n_nodes = len(row_ptr) - 1 - first_node
    if n_nodes < 1:
        raise ValueError('link prediction needs at least one node')
    if simple_status & _native.DW_S_DUP_NEIGHBOR:
        raise ValueError('negative_edges: a CSR row lists the same neighbour twice (the rank '
                         'rule needs distinct neighbours)')
    if row_ptr[first_node] != 0:
        raise ValueError(f'negative_edges: rows below {first_node} (<unk>) have neighbours')
    deg = np.diff(row_ptr[first_node:])
    if deg.size and int(deg.max()) >= n_nodes:
        u = first_node + int(deg.argmax())
        raise ValueError(f'negative_edges: node {u} has degree {int(deg.max())} >= {n_nodes} '
                         f'nodes: it has no non-neighbour')


def _checked_tensors(csr, device):
    """The CSR's device tensors with the sorted rows. The graph is checked once: from the host
    row_ptr before any device work, then dw_csr_check_simple's word (once per device)."""
    if not csr.__dict__.get('_linkpred_host_ok'):
        check_negative_graph(csr.row_ptr, FIRST_NODE)
        csr.__dict__['_linkpred_host_ok'] = True
    dev = _native.require_device(device)
    d = csr.device_tensors(dev, need_sorted=True)
    if not d.get('linkpred_ok'):
        check_negative_graph(csr.row_ptr, FIRST_NODE, int(d['simple_status'].item()))
        d['linkpred_ok'] = True
    return dev, d


def negative_edges(csr, n: int, seed: int, offset: int = 0, device=None) -> torch.Tensor:
    """int64 [n, 2] device tensor of non-adjacent pairs (u, v): u uniform over the nodes, v
    uniform over the nodes not adjacent to u (u itself allowed). Sample i is a pure function of
    (seed, offset + i): disjoint offset ranges give independent sets."""
    n = int(n)
    if n < 0:
        raise ValueError('n must be >= 0')
    dev, d = _checked_tensors(csr, device)
    pairs = torch.empty((n, 2), dtype=torch.int64, device=dev)
    if n == 0:
        return pairs
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _native.call('dw_negative_edges', _native.ptr(d['row_ptr']), _native.ptr(d['col_sorted']),
                     csr.vocab_size, FIRST_NODE, n, int(seed) & (2 ** 64 - 1),
                     int(offset) & (2 ** 64 - 1), _native.ptr(pairs), _native.ptr(st),
                     _native.stream(dev))
    _native.check_status(st, 'negative_edges')
    return pairs


# ------------------------------------------------------------------------------ edge features
def _table_and_pairs(table: torch.Tensor, pairs: torch.Tensor):
    if table.dim() != 2 or table.dtype != torch.float32:
        raise ValueError('table must be a float32 [V, d] device tensor')
    if not 1 <= table.shape[1] <= 512:
        raise ValueError(f'embedding size {table.shape[1]} outside [1, 512]')
    if pairs.dtype != torch.int64 or pairs.dim() != 2 or pairs.shape[1] != 2:
        raise ValueError('pairs must be an int64 [n, 2] device tensor')
    if pairs.device != table.device:
        raise ValueError('pairs and table live on different devices')
    return table.contiguous(), pairs.contiguous()


def edge_embeddings_device(table: torch.Tensor, pairs: torch.Tensor, operator_name: str,
                           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float32 [n, d] = operator(table[pairs[:, 0]], table[pairs[:, 1]]) on the device
    (edge_operators.edge_embeddings in float32). ``out``: an optional contiguous destination."""
    op = operator_id(operator_name)
    table, pairs = _table_and_pairs(table, pairs)
    dev = table.device
    n, d = pairs.shape[0], table.shape[1]
    if out is None:
        out = torch.empty((n, d), dtype=torch.float32, device=dev)
    elif out.shape != (n, d) or out.dtype != torch.float32 or out.device != dev:
        raise ValueError('out must be a float32 [n, d] tensor on the table\'s device')
    if n == 0:
        return out
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _native.call('dw_edge_features', _native.ptr(table), table.shape[0], d, op,
                     _native.ptr(pairs), n, _native.ptr(out), _native.ptr(st),
                     _native.stream(dev))
    _native.check_status(st, 'edge_embeddings_device')
    return out


def edge_logreg_sums(table: torch.Tensor, op: int, pairs: torch.Tensor, labels: torch.Tensor,
                     coef: torch.Tensor, workspace: Optional[torch.Tensor] = None,
                     check: bool = True) -> torch.Tensor:
    """One dw_edge_logreg pass: float64 [d + 3] device tensor (sum r x, sum r, sum loss, the
    count of correctly classified samples) at ``coef`` (float64 [d + 1] on the device)."""
    table, pairs = _table_and_pairs(table, pairs)
    dev = table.device
    n, d = pairs.shape[0], table.shape[1]
    if labels.dtype != torch.uint8 or labels.shape != (n,) or labels.device != dev:
        raise ValueError('labels must be a uint8 [n] tensor on the table\'s device')
    if coef.dtype != torch.float64 or coef.shape != (d + 1,) or coef.device != dev:
        raise ValueError('coef must be a float64 [d + 1] tensor on the table\'s device')
    out = torch.zeros(d + 3, dtype=torch.float64, device=dev)
    if n == 0:
        return out
    if workspace is None:
        workspace = logreg_workspace(n, d, dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _native.call('dw_edge_logreg', _native.ptr(table), table.shape[0], d, op,
                     _native.ptr(pairs), _native.ptr(labels.contiguous()), n,
                     _native.ptr(coef.contiguous()), _native.ptr(out), _native.ptr(workspace),
                     workspace.numel() * workspace.element_size(), _native.ptr(st),
                     _native.stream(dev))
    if check:
        _native.check_status(st, 'edge_logreg')
    return out


def logreg_workspace(n: int, d: int, device) -> torch.Tensor:
    """A dw_edge_logreg workspace for n samples of dimension d."""
    nb = ctypes.c_size_t(0)
    _native.call('dw_edge_logreg_workspace_bytes', int(n), int(d), ctypes.byref(nb))
    return torch.empty(max(int(nb.value) // 8, 1), dtype=torch.float64, device=device)


# ------------------------------------------------------------------------------ scores and AUC
def edge_scores(table: torch.Tensor, pairs: torch.Tensor, operator_name: str,
                coef: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float64 [n] device tensor z = w . operator(table[n1], table[n2]) + b0 (dw_edge_scores).
    ``coef``: float64 [d + 1] (weights, then the intercept) on the device or as numpy; None means
    unit weights and a zero intercept — with 'hadamard' the plain dot product of the rows."""
    op = operator_id(operator_name)
    table, pairs = _table_and_pairs(table, pairs)
    dev = table.device
    n, d = pairs.shape[0], table.shape[1]
    if coef is not None:
        coef = torch.as_tensor(coef, dtype=torch.float64).to(dev).contiguous()
        if coef.shape != (d + 1,):
            raise ValueError('coef must hold d + 1 float64 values (weights, then the intercept)')
    z = torch.empty(n, dtype=torch.float64, device=dev)
    if n == 0:
        return z
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _native.call('dw_edge_scores', _native.ptr(table), table.shape[0], d, op,
                     _native.ptr(pairs), n, _native.ptr(coef), _native.ptr(z), _native.ptr(st),
                     _native.stream(dev))
    _native.check_status(st, 'edge_scores')
    return z


def _check_auc_inputs(scores, labels) -> None:
    if getattr(scores, 'ndim', None) != 1 or getattr(labels, 'shape', None) != scores.shape:
        raise ValueError('scores and labels must be 1-d and of the same length')


def auc_from_counts(u2: int, n_pos: int, n_neg: int) -> float:
    """U2 / (2 n_pos n_neg); an empty class has no AUC (ValueError, as sklearn)."""
    if n_pos == 0 or n_neg == 0:
        raise ValueError('ROC AUC needs at least one positive and one negative sample')
    return u2 / (2 * n_pos * n_neg)


def roc_auc_counts(scores: torch.Tensor, labels: torch.Tensor) -> Tuple[int, int, int]:
    """(U2, n_pos, n_neg) of float64 device scores and uint8 labels (dw_roc_auc): U2 = sum over
    positives of 2 #{lower negatives} + #{tied negatives}, exact integers."""
    _check_auc_inputs(scores, labels)
    if scores.dtype != torch.float64 or labels.dtype != torch.uint8 or \
            labels.device != scores.device:
        raise ValueError('scores must be float64 and labels uint8, on one device')
    dev = scores.device
    n = scores.shape[0]
    if n >= 1 << 31:
        raise ValueError('roc_auc takes fewer than 2^31 scores')
    out = torch.zeros(3, dtype=torch.int64, device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    nb = ctypes.c_size_t(0)
    with torch.cuda.device(dev):
        _native.call('dw_roc_auc_workspace_bytes', n, ctypes.byref(nb))
        ws = torch.empty(max(int(nb.value), 1), dtype=torch.uint8, device=dev)
        _native.call('dw_roc_auc', _native.ptr(scores.contiguous()),
                     _native.ptr(labels.contiguous()), n, _native.ptr(out), _native.ptr(st),
                     _native.ptr(ws), ws.numel(), _native.stream(dev))
    _native.check_status(st, 'roc_auc')
    u2, n_pos, n_neg = (int(v) for v in out.tolist())
    return u2, n_pos, n_neg


def roc_auc(scores: torch.Tensor, labels: torch.Tensor) -> float:
    """Exact ROC AUC (ties count a half), sklearn's roc_auc_score up to one division."""
    return auc_from_counts(*roc_auc_counts(scores, labels))


# ------------------------------------------------------------------------------ the optimiser
Closure = Callable[[np.ndarray], Tuple[float, np.ndarray]]


def lbfgs_minimize(closure: Closure, x0: np.ndarray, max_iter: int = 100,
                   tol: float = 1e-4) -> Tuple[np.ndarray, float, int]:
    """Minimise ``closure: x -> (objective, gradient)`` (float64 numpy in and out) by L-BFGS with
    a strong-Wolfe line search (torch.optim.LBFGS on a host float64 vector). Stops when
    max|gradient| <= tol or after ``max_iter`` iterations. Returns (x, objective at x,
    iterations)."""
    x = torch.tensor(np.asarray(x0, dtype=np.float64), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.LBFGS([x], lr=1.0, max_iter=int(max_iter), max_eval=10 * int(max_iter),
                            tolerance_grad=float(tol), tolerance_change=0.0, history_size=10,
                            line_search_fn='strong_wolfe')

    def step_closure():
        f, g = closure(x.detach().numpy().copy())
        x.grad = torch.as_tensor(np.asarray(g, dtype=np.float64)).reshape(x.shape).clone()
        return torch.tensor(float(f), dtype=torch.float64)

    opt.step(step_closure)
    n_iter = int(opt.state[x]['n_iter'])
    xf = x.detach().numpy().copy()
    f, _ = closure(xf)
    return xf, float(f), n_iter


def penalised(sums: np.ndarray, coef: np.ndarray, C: float,
              fit_intercept: bool) -> Tuple[float, np.ndarray]:
    """sklearn's objective C * sum(loss) + 0.5 * ||w||^2 and its gradient from one pass's sums
    (dw_edge_logreg's out, or the restatement's): the intercept is not penalised, and stays
    fixed (zero gradient) without fit_intercept."""
    d = len(coef) - 1
    w = coef[:d]
    obj = C * float(sums[d + 1]) + 0.5 * float(w @ w)
    grad = np.empty(d + 1, dtype=np.float64)
    grad[:d] = C * sums[:d] + w
    grad[d] = C * sums[d] if fit_intercept else 0.0
    return obj, grad


class EdgeLogisticRegression:
    """Binary logistic regression on operator(table[n1], table[n2]) with sklearn's objective
    C * sum(loss) + 0.5 * ||w||^2 (lbfgs, l2; the intercept is not penalised). The features are
    never stored: every objective / gradient evaluation is one dw_edge_logreg pass."""

    def __init__(self, operator_name: str, C: float = 1.0, fit_intercept: bool = True,
                 max_iter: int = 100, tol: float = 1e-4):
        self.operator_name = operator_name.lower()
        self.op = operator_id(operator_name)
        if not C > 0:
            raise ValueError('C must be positive')
        self.C, self.fit_intercept = float(C), bool(fit_intercept)
        self.max_iter, self.tol = int(max_iter), float(tol)
        self.coef_: Optional[np.ndarray] = None
        self.intercept_ = 0.0
        self.n_iter_ = 0
        self.objective_ = float('nan')

    @classmethod
    def from_params(cls, operator_name: str, classifier_params: Optional[dict] = None):
        """From a config's ``classifier_params``: only C, fit_intercept, max_iter and tol."""
        params = dict(classifier_params or {})
        unknown = sorted(set(params) - set(CLASSIFIER_PARAMS))
        if unknown:
            raise ValueError(f'classifier_params {unknown} are not supported by the device '
                             f'backend (supported: {list(CLASSIFIER_PARAMS)})')
        return cls(operator_name, **params)

    def fit_closure(self, closure: Closure, d: int) -> 'EdgeLogisticRegression':
        """Fit through ``closure: coef (d + 1) -> (sums (d + 3))`` — the driver without the
        kernel (the sums of any implementation of dw_edge_logreg's contract)."""
        def objective(coef):
            return penalised(np.asarray(closure(coef), dtype=np.float64), coef, self.C,
                             self.fit_intercept)
        x, f, it = lbfgs_minimize(objective, np.zeros(d + 1), self.max_iter, self.tol)
        self.coef_, self.intercept_ = x[:d].copy(), float(x[d])
        self.objective_, self.n_iter_ = f, it
        return self

    def _device_closure(self, table, pairs, labels):
        table, pairs = _table_and_pairs(table, pairs)
        labels = labels.to(torch.uint8).contiguous()
        ws = logreg_workspace(pairs.shape[0], table.shape[1], table.device)

        def sums(coef: np.ndarray) -> np.ndarray:
            c = torch.from_numpy(np.ascontiguousarray(coef, dtype=np.float64)).to(table.device)
            return edge_logreg_sums(table, self.op, pairs, labels, c, ws).cpu().numpy()
        return sums

    def fit(self, table: torch.Tensor, pairs: torch.Tensor,
            labels: torch.Tensor) -> 'EdgeLogisticRegression':
        if pairs.shape[0] == 0:
            raise ValueError('fit needs at least one sample')
        return self.fit_closure(self._device_closure(table, pairs, labels), table.shape[1])

    def full_coef(self) -> np.ndarray:
        if self.coef_ is None:
            raise RuntimeError('fit first')
        return np.concatenate([self.coef_, [self.intercept_]])

    def score(self, table: torch.Tensor, pairs: torch.Tensor, labels: torch.Tensor) -> float:
        """Accuracy: the share of samples with (z > 0) == label."""
        n = pairs.shape[0]
        sums = self._device_closure(table, pairs, labels)(self.full_coef())
        return float(sums[-1]) / n

    def decision_function(self, table: torch.Tensor, pairs: torch.Tensor) -> torch.Tensor:
        """float64 [n] device tensor of z = w . x + b per pair (dw_edge_scores)."""
        return edge_scores(table, pairs, self.operator_name, self.full_coef())


# ------------------------------------------------------------------------------ the experiment
def positive_edges(csr, device=None, loops: bool = True) -> torch.Tensor:
    """int64 [E, 2] device tensor: the CSR entries with col >= row (each undirected edge once,
    self-loops included; col > row without ``loops``), in row order."""
    dev = _native.require_device(device)
    d = csr.device_tensors(dev)
    row_ptr, col = d['row_ptr'], d['col']
    if csr.nnz == 0:
        return torch.empty((0, 2), dtype=torch.int64, device=dev)
    deg = row_ptr[1:] - row_ptr[:-1]
    rows = torch.repeat_interleave(torch.arange(csr.vocab_size, dtype=torch.int64, device=dev),
                                   deg, output_size=csr.nnz)
    cols = col[:csr.nnz].to(torch.int64)
    keep = cols >= rows if loops else cols > rows
    return torch.stack([rows[keep], cols[keep]], dim=1).contiguous()


def edge_classification_device(table: torch.Tensor, csr, train_ratio: float, n_experiments: int,
                               operator_name: str, classifier_params: Optional[dict] = None,
                               seed: int = 0, device=None,
                               return_accuracies: bool = False):
    """Mean and best link-prediction accuracy over ``n_experiments`` (and the per-experiment
    accuracies with ``return_accuracies``). ``table``: float32 [V, d] input embeddings in the
    CSR's row order (row 0 = <unk>)."""
    EdgeLogisticRegression.from_params(operator_name, classifier_params)   # refuse early
    if table.shape[0] != csr.vocab_size:
        raise ValueError(f'table has {table.shape[0]} rows, the graph {csr.vocab_size}')
    dev, _ = _checked_tensors(csr, device if device is not None else
                              (table.device if table.is_cuda else None))
    table = table.to(device=dev, dtype=torch.float32).contiguous()
    pos = positive_edges(csr, dev)
    n_edges = pos.shape[0]
    if n_edges == 0:
        raise ValueError('the graph has no edges')
    n_train = round(train_ratio * n_edges)
    n_val = n_edges - n_train
    if n_train < 1:
        raise ValueError('train_ratio leaves no training edge')
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    y_train = torch.cat([torch.ones(n_train, dtype=torch.uint8, device=dev),
                         torch.zeros(n_train, dtype=torch.uint8, device=dev)])
    y_all = torch.cat([torch.ones(n_edges, dtype=torch.uint8, device=dev),
                       torch.zeros(n_edges, dtype=torch.uint8, device=dev)])
    accs: List[float] = []
    for i in range(n_experiments):
        perm = torch.randperm(n_edges, generator=gen, device=dev)
        edges = pos[perm]
        # experiment i owns the samples [i * E, (i + 1) * E) of the negative stream
        neg_train = negative_edges(csr, n_train, seed, offset=i * n_edges, device=dev)
        neg_val = negative_edges(csr, n_val, seed, offset=i * n_edges + n_train, device=dev)
        clf = EdgeLogisticRegression.from_params(operator_name, classifier_params)
        clf.fit(table, torch.cat([edges[:n_train], neg_train]), y_train)
        acc = clf.score(table, torch.cat([edges, neg_train, neg_val]), y_all)
        logger.info(f'Experiment {i}: accuracy {100 * acc:.2f}% ({clf.n_iter_} L-BFGS '
                    f'iterations, objective {clf.objective_:.6g}).')
        accs.append(acc)
    assert accs, 'No experiments performed!'
    mean, best = float(np.mean(accs)), float(max(accs))
    logger.info(f'Edge classification accuracy (device): {100 * mean:.2f}% (averaged over '
                f'{n_experiments} experiments); best {100 * best:.2f}%.')
    if return_accuracies:
        return mean, best, accs
    return mean, best


# ------------------------------------------------------------------------------ held-out edges
SCORERS = ('classifier', 'dot')


def heldout_negative_offsets(i: int, n_train: int, n_test: int) -> Tuple[int, int]:
    """Experiment i owns the samples [i * (n_train + n_test), (i + 1) * (n_train + n_test)) of
    the negative stream: its training negatives first, then its test negatives."""
    base = i * (n_train + n_test)
    return base, base + n_train


def heldout_pairs(full_csr, train_pos: torch.Tensor, held: torch.Tensor, i: int, seed: int,
                  device=None):
    """Experiment i's (train pairs, train labels, test pairs, test labels): the train graph's
    edges and the held edges as positives, as many negatives each — non-edges of the FULL graph,
    from disjoint offset ranges of one stream."""
    dev = train_pos.device
    n_train, n_test = train_pos.shape[0], held.shape[0]
    off_train, off_test = heldout_negative_offsets(i, n_train, n_test)
    neg_train = negative_edges(full_csr, n_train, seed, offset=off_train, device=device)
    neg_test = negative_edges(full_csr, n_test, seed, offset=off_test, device=device)

    def labels(n):
        return torch.cat([torch.ones(n, dtype=torch.uint8, device=dev),
                          torch.zeros(n, dtype=torch.uint8, device=dev)])
    return (torch.cat([train_pos, neg_train]), labels(n_train),
            torch.cat([held, neg_test]), labels(n_test))


def heldout_edge_classification(table: torch.Tensor, full_csr, train_csr, held,
                                n_experiments: int, operator_name: str,
                                classifier_params: Optional[dict] = None,
                                scorer: str = 'classifier', seed: int = 0, device=None,
                                return_experiments: bool = False):
    """Link prediction on held-out edges (node2vec §4.4): ``table`` was trained on ``train_csr``
    (graph/holdout.py's residual graph of ``full_csr``), ``held`` int64 [n, 2] are the hidden
    edges. Per experiment the classifier is fitted on the train graph's non-loop edges against
    as many non-edges of the full graph and tested on the held edges against ``len(held)`` more;
    experiments differ only in their negatives. ``scorer='dot'`` ranks by the rows' dot product
    instead and fits nothing (its accuracy thresholds the dot product at 0).

    Returns {'edge_auc', 'edge_auc_std', 'edge_accuracy', 'edge_best'}: mean and (population)
    standard deviation of the exact ROC AUC of the test scores, mean and best test accuracy; with
    ``return_experiments`` also the per-experiment (aucs, accuracies)."""
    if scorer not in SCORERS:
        raise ValueError(f'scorer must be one of {SCORERS}, got {scorer!r}')
    EdgeLogisticRegression.from_params(operator_name, classifier_params)   # refuse early
    if table.shape[0] != full_csr.vocab_size or train_csr.vocab_size != full_csr.vocab_size:
        raise ValueError(f'table has {table.shape[0]} rows, the full graph '
                         f'{full_csr.vocab_size}, the train graph {train_csr.vocab_size}')
    dev, _ = _checked_tensors(full_csr, device if device is not None else
                              (table.device if table.is_cuda else None))
    table = table.to(device=dev, dtype=torch.float32).contiguous()
    held = torch.as_tensor(held, dtype=torch.int64).to(dev).reshape(-1, 2).contiguous()
    train_pos = positive_edges(train_csr, dev, loops=False)
    if held.shape[0] == 0 or train_pos.shape[0] == 0:
        raise ValueError('held-out link prediction needs held edges and training edges')
    aucs: List[float] = []
    accs: List[float] = []
    for i in range(n_experiments):
        x_train, y_train, x_test, y_test = heldout_pairs(full_csr, train_pos, held, i, seed, dev)
        if scorer == 'dot':
            z = edge_scores(table, x_test, 'hadamard', None)
            acc = float(((z > 0) == (y_test != 0)).double().mean())
        else:
            clf = EdgeLogisticRegression.from_params(operator_name, classifier_params)
            clf.fit(table, x_train, y_train)
            z = clf.decision_function(table, x_test)
            acc = clf.score(table, x_test, y_test)
        auc = roc_auc(z, y_test)
        logger.info(f'Experiment {i}: held-out AUC {auc:.4f}, accuracy {100 * acc:.2f}%.')
        aucs.append(auc)
        accs.append(acc)
    assert aucs, 'No experiments performed!'
    result = {'edge_auc': float(np.mean(aucs)), 'edge_auc_std': float(np.std(aucs)),
              'edge_accuracy': float(np.mean(accs)), 'edge_best': float(max(accs))}
    logger.info(f'Held-out link prediction ({scorer}): AUC {result["edge_auc"]:.4f} +- '
                f'{result["edge_auc_std"]:.4f}, accuracy {100 * result["edge_accuracy"]:.2f}% '
                f'over {n_experiments} experiments.')
    if return_experiments:
        return result, aucs, accs
    return result
