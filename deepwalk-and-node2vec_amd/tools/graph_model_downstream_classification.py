"""Downstream quality of trained graph embeddings (reference:
tools/graph_model_downstream_classification.py; README.md:225-248, 276-281, 320-325).

    python tools/graph_model_downstream_classification.py --config-name=sge_sg_karate_club

Loads ``{output_dir}/{dataset}/{experiment}/checkpoints/{analysis.checkpoint}`` (written by
tools/train.py) and runs the two tasks of the reference:
  * node classification: logistic regression on the input embeddings (``<unk>`` row skipped,
    node features appended when the dataset has them); the configured split algorithm is
    re-seeded with the experiment index; mean and best accuracy over ``n_experiments``;
  * edge classification (link prediction): edge embedding = operator(n1, n2); per
    experiment the edges are shuffled, the first round(train_ratio * E) are the positive
    training edges, as many negative (non-adjacent) pairs are sampled for training and the rest
    for evaluation; the classifier is evaluated on ALL edges plus both negative sets
    (transductive, as the reference does).
Negative pairs follow the reference's law: a uniform node, then a uniform node among its
non-neighbours (itself included). sklearn's LogisticRegression with the config's
``classifier_params``. The model only needs the checkpoint: no GPU is used here, unless
``downstream.edge_classification.backend=device`` selects the device path for the edge task
(shallow_encoders/graph/linkpred.py: the graph's CSR, so ``graph_rmat`` datasets work too) or
``downstream.node_classification.backend=device`` the one for the node task
(shallow_encoders/graph/nodeclf.py: the fp32 table stays on the GPU; embeddings only, no node
features, no 2-D plot; macro-F1 is logged beside the accuracy). A multi-label dataset
(``graph_edge_list`` with ``multilabel=true``) runs on the device backend only: one-vs-rest
logistic regression, micro- and macro-F1 under ``downstream.node_classification.prediction``.
``downstream.edge_classification.protocol=heldout`` (device backend, a dataset with
``holdout_ratio`` > 0) replaces the in-sample edge task by node2vec §4.4's: the edges the dataset
hid before training are ranked against non-edges, reported as ``edge_auc`` (exact ROC AUC),
``edge_auc_std``, ``edge_accuracy`` and ``edge_best``.
``downstream.embeddings_path=<file>`` scores a word2vec text file (this project's export, the
node2vec or DeepWalk reference programs' output, gensim's) instead of the checkpoint: the file's
rows are laid out by the dataset's vocabulary, ``downstream.embeddings_missing=zero`` lets nodes
the file does not hold stay zero rows. With a device backend the HIP reader parses it.
Only the labelled vertices are classified: a ``graph_edge_list`` dataset's label file may cover
a part of the nodes.
``downstream.clustering.enable=true`` adds the third task of the DeepWalk / node2vec papers
(a departure: the reference has none): k-means communities of the embeddings
(shallow_encoders/graph/cluster.py; ``backend=device`` keeps the fp32 table on the GPU), reported
as ``cluster_inertia``, ``cluster_modularity`` (structural, needs no labels) and
``cluster_iterations``, and with one label per node ``cluster_nmi`` and ``cluster_ari`` against
the labels over the labelled nodes.
"""
import argparse
import logging
import os
import random
import sys
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from shallow_encoders.common.path import CONFIG_PATH  # noqa: E402
from shallow_encoders.config_parser import load_config_dict  # noqa: E402
from shallow_encoders.graph import edge_operators  # noqa: E402
from tools import conventions  # noqa: E402
from tools.utils import setup_pipeline  # noqa: E402

logger = logging.getLogger('DownstreamTask-Classification')


def labels_to_integers(labels: List[str]) -> List[int]:
    """Unique string labels -> 0..C-1 (sorted order, so runs are reproducible)."""
    index = {label: i for i, label in enumerate(sorted(set(labels)))}
    return [index[label] for label in labels]


def fit_and_score(X_train, y_train, X, y, classifier_params: Optional[dict] = None):
    """LogisticRegression fitted on (X_train, y_train); accuracy on (X, y)."""
    from sklearn.linear_model import LogisticRegression
    clf = LogisticRegression(**(classifier_params or {}))
    clf.fit(X_train, y_train)
    return clf, float(np.mean(clf.predict(X) == y))


def node_classification(embeddings: np.ndarray, itos: List[str], labels: Dict[str, str],
                        split_algorithm, n_experiments: int,
                        features: Optional[Dict[str, np.ndarray]] = None,
                        classifier_params: Optional[dict] = None,
                        plot_path: Optional[str] = None) -> Tuple[float, float]:
    """Mean and best accuracy over ``n_experiments`` (rows of ``embeddings`` follow ``itos``,
    row 0 = ``<unk>`` is skipped, and so is a vertex without a label)."""
    keep = [i for i, v in enumerate(itos[1:], start=1) if v in labels]
    vertices = [itos[i] for i in keep]
    X = np.asarray(embeddings, dtype=np.float64)[keep]
    if features is not None:
        X = np.concatenate([X, np.stack([features[v] for v in vertices])], axis=1)
    y = np.asarray(labels_to_integers([labels[v] for v in vertices]), dtype=np.float32)
    logger.info(f'Dataset info: X.shape={X.shape}, y.shape={y.shape}.')
    total, best, best_clf = 0.0, None, None
    for i in range(n_experiments):
        split_algorithm.random_state = i
        sp = split_algorithm(X, y)
        clf, acc = fit_and_score(sp['X_train'], sp['y_train'], sp['X_test'], sp['y_test'],
                                 classifier_params)
        total += acc
        if best is None or acc >= best:
            best, best_clf = acc, clf
    assert best is not None, 'No experiments performed!'
    mean = total / n_experiments
    logger.info(f'Node classification accuracy: {100 * mean:.2f}% (averaged over '
                f'{n_experiments} experiments); best {100 * best:.2f}%.')
    if plot_path is not None:
        plot_node_classification(X, y, best_clf, best, plot_path)
    return mean, best


def is_multilabel(dataset) -> bool:
    return bool(getattr(getattr(dataset, 'dataset', dataset), 'is_multilabel', False))


def check_node_backend(dataset, nc) -> None:
    """The host path fits one label per node: a multi-label dataset needs the device backend."""
    if nc.backend != 'device' and is_multilabel(dataset):
        raise ValueError('a multi-label dataset is classified on the device only: set '
                         'downstream.node_classification.backend=device')


def node_classification_on_device(embeddings: np.ndarray, dataset, nc) -> Dict[str, float]:
    """``backend: device``: the same protocol with the table and the logistic regression on the
    GPU (shallow_encoders/graph/nodeclf.py). The labelled rows come from the dataset's
    ``label_arrays()`` where it has one, from ``labels`` and the vocabulary otherwise."""
    import torch
    from shallow_encoders import _native
    from shallow_encoders.graph import nodeclf
    if dataset.has_features:
        raise ValueError('downstream.node_classification.backend=device classifies the '
                         'embeddings alone: this dataset has node features (use backend=sklearn)')
    inner = getattr(dataset, 'dataset', dataset)
    if is_multilabel(dataset):
        rows, masks, classes = inner.label_arrays()
        logger.info(f'Dataset info: {len(rows)} labelled nodes, {len(classes)} labels, '
                    f'd={embeddings.shape[1]}.')
        dev = _native.require_device(None)
        table = _device_table(embeddings, dev)
        micro, macro, best = nodeclf.node_multilabel_device(
            table, rows, masks, nc.instantiate_split_algorithm(), nc.n_experiments,
            classifier_params=nc.classifier_params, rule=nc.prediction, device=dev,
            n_classes=len(classes))
        return {'node_micro_f1': micro, 'node_macro_f1': macro, 'node_best_micro_f1': best}
    if hasattr(inner, 'label_arrays'):
        rows, y, _ = inner.label_arrays()
    else:
        itos, labels = dataset.vocab.get_itos(), dataset.labels
        rows = [i for i, v in enumerate(itos[1:], start=1) if v in labels]
        y = labels_to_integers([labels[itos[i]] for i in rows])
    y = np.asarray(y, dtype=np.float32)   # the host path's label dtype (the splits see it)
    logger.info(f'Dataset info: {len(rows)} labelled nodes, d={embeddings.shape[1]}.')
    dev = _native.require_device(None)
    table = _device_table(embeddings, dev)
    mean, best, confusion = nodeclf.node_classification_device(
        table, rows, y, nc.instantiate_split_algorithm(), nc.n_experiments,
        classifier_params=nc.classifier_params, device=dev)
    f1 = nodeclf.macro_f1(confusion)
    logger.info(f'Best experiment: macro-F1 {100 * f1:.2f}% (micro-F1 = accuracy '
                f'{100 * best:.2f}%).')
    return {'node_accuracy': mean, 'node_best': best, 'node_macro_f1': f1}


def plot_node_classification(X, y, clf, accuracy, path) -> None:
    """Scatter of 2-D embeddings per class with the classifier's decision lines."""
    if X.shape[1] != 2:
        logger.info('Embeddings are not 2-D: skipping the decision-boundary figure.')
        return
    import matplotlib
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    fig = plt.figure(figsize=(10, 10))
    for c in np.unique(y):
        pts = X[y == c]
        plt.scatter(pts[:, 0], pts[:, 1], label=f'class {int(c)}')
    xs = np.linspace(X[:, 0].min() - 1, X[:, 0].max() + 1, 100)
    for i in range(clf.coef_.shape[0]):
        t1, t2 = clf.coef_[i]
        plt.plot(xs, (-clf.intercept_[i] - t1 * xs) / t2, color='red',
                 label=f'Decision Boundary {i:03d}')
    plt.title(f'Classification on embeddings - Accuracy {100 * accuracy:.2f}')
    plt.xlabel('Dimension 1')
    plt.ylabel('Dimension 2')
    plt.legend()
    fig.savefig(path)
    plt.close(fig)
    logger.info(f'Saved figure at path "{path}".')


def sample_negative_edges(nodes: List[str], neighbors: Dict[str, set], n: int,
                          rng: random.Random) -> List[Tuple[str, str]]:
    """``n`` pairs (u, v): u uniform over nodes, v uniform over the nodes not adjacent to u
    (u itself allowed) — drawn by rejection, the same law as the reference's set difference."""
    out = []
    node_set_size = len(nodes)
    while len(out) < n:
        u = rng.choice(nodes)
        if len(neighbors[u]) >= node_set_size:
            continue
        while True:
            v = rng.choice(nodes)
            if v not in neighbors[u]:
                break
        out.append((u, v))
    return out


def edge_classification(embeddings: np.ndarray, graph, stoi: Dict[str, int], train_ratio: float,
                        n_experiments: int, operator_name: str,
                        classifier_params: Optional[dict] = None,
                        seed: int = 0) -> Tuple[float, float]:
    """Mean and best link-prediction accuracy over ``n_experiments``."""
    op = edge_operators.edge_operator_factory(operator_name)
    emb = np.asarray(embeddings, dtype=np.float64)
    edges = list(graph.edges)
    nodes = list(graph.nodes)
    neighbors = {u: set(graph.neighbors(u)) for u in nodes}
    n_edges = len(edges)
    rng = random.Random(seed)

    def ids(pairs):
        return np.asarray([(stoi[a], stoi[b]) for a, b in pairs], dtype=np.int64).reshape(-1, 2)

    total, best = 0.0, None
    for _ in range(n_experiments):
        n_train = round(train_ratio * n_edges)
        n_val = n_edges - n_train
        rng.shuffle(edges)
        neg_train = sample_negative_edges(nodes, neighbors, n_train, rng)
        neg_val = sample_negative_edges(nodes, neighbors, n_val, rng)
        X_train = edge_operators.edge_embeddings(emb, ids(edges[:n_train] + neg_train), op)
        y_train = np.asarray([1] * n_train + [0] * n_train, dtype=np.float32)
        X = edge_operators.edge_embeddings(emb, ids(edges + neg_train + neg_val), op)
        y = np.asarray([1] * n_edges + [0] * (n_train + n_val), dtype=np.float32)
        _, acc = fit_and_score(X_train, y_train, X, y, classifier_params)
        total += acc
        best = acc if best is None else max(best, acc)
    assert best is not None, 'No experiments performed!'
    mean = total / n_experiments
    logger.info(f'Edge classification accuracy: {100 * mean:.2f}% (averaged over '
                f'{n_experiments} experiments); best {100 * best:.2f}%.')
    return mean, best


def edge_classification_on_device(embeddings: np.ndarray, graph, ec) -> Tuple[float, float]:
    """``backend: device``: the same protocol over the graph's CSR (a networkx graph or a
    ``CSRGraph``, so ``graph_rmat`` datasets too) with the table, the negative sampler and the
    logistic regression on the GPU (shallow_encoders/graph/linkpred.py)."""
    import torch
    from shallow_encoders import _native
    from shallow_encoders.graph import linkpred
    from shallow_encoders.graph.random_walk_generator import _csr_of
    dev = _native.require_device(None)
    table = _device_table(embeddings, dev)
    return linkpred.edge_classification_device(
        table, _csr_of(graph), ec.train_ratio, ec.n_experiments, ec.operator_name,
        classifier_params=ec.classifier_params, device=dev)


def heldout_edge_classification_on_device(embeddings: np.ndarray, dataset, ec) -> Dict[str, float]:
    """``protocol: heldout``: the dataset hid edges before training (``holdout_ratio`` > 0, the
    same split here as in tools/train.py: it is a function of graph, ratio and seed); they are
    ranked against non-edges of the full graph (linkpred.heldout_edge_classification)."""
    import torch
    from shallow_encoders import _native
    from shallow_encoders.graph import linkpred
    inner = getattr(dataset, 'dataset', dataset)
    if getattr(inner, 'heldout_edges', None) is None:
        raise ValueError('downstream.edge_classification.protocol=heldout needs a dataset that '
                         'held edges out: set datamodule.additional_parameters.holdout_ratio=<r> '
                         '(0 < r < 1; graph_rmat or graph_edge_list), for training as well')
    dev = _native.require_device(None)
    from shallow_encoders.graph.holdout import connected_components
    n_components = connected_components(inner.full_csr, device=dev)[1]
    logger.info(f'Held-out link prediction: the full graph has {n_components} connected '
                f'component(s); holdout_info={inner.holdout_info}.')
    if n_components > 1:
        logger.warning(f'The full graph has {n_components} connected components: node2vec '
                       f'§4.4 splits a connected graph, so its figures are not comparable '
                       f'one to one (the largest component is not extracted here).')
    table = _device_table(embeddings, dev)
    return linkpred.heldout_edge_classification(
        table, inner.full_csr, inner.csr, inner.heldout_edges, ec.n_experiments,
        ec.operator_name, classifier_params=ec.classifier_params, scorer=ec.scorer, device=dev)


def clustering(embeddings, dataset, cc) -> Dict[str, float]:
    """``downstream.clustering``: k-means communities of the input embeddings (row 0 skipped;
    shallow_encoders/graph/cluster.py), scored without labels by the structural modularity of the
    graph's CSR and, where the dataset has one label per node, by NMI and ARI against the labels
    over the labelled nodes. ``n_clusters=0`` takes the number of label classes."""
    import torch
    from shallow_encoders.graph import cluster
    from shallow_encoders.graph.random_walk_generator import _csr_of
    if is_multilabel(dataset):
        raise ValueError('downstream.clustering compares one label per node: this dataset is '
                         'multi-label (NMI and ARI are not defined for label sets)')
    inner = getattr(dataset, 'dataset', dataset)
    rows, y = None, None
    if not dataset.has_labels:
        pass
    elif hasattr(inner, 'label_arrays'):
        rows, y, _ = inner.label_arrays()
    else:
        itos, labels = dataset.vocab.get_itos(), dataset.labels
        rows = [i for i, v in enumerate(itos[1:], start=1) if v in labels]
        y = labels_to_integers([labels[itos[i]] for i in rows])
    if rows is not None and len(rows) == 0:
        rows, y = None, None
    K = cc.n_clusters
    if K == 0:
        if y is None:
            raise ValueError('downstream.clustering.n_clusters=0 takes the number of label '
                             'classes: this dataset has no labels, name n_clusters')
        K = len(set(int(c) for c in y))
    V = embeddings.shape[0]
    csr = getattr(inner, 'csr', None) or _csr_of(dataset.graph)
    ids = np.arange(1, V, dtype=np.int64)
    if cc.backend == 'device':
        from shallow_encoders import _native
        dev = _native.require_device(None)
        table = _device_table(embeddings, dev)
        labels, _, inertia, n_iter = cluster.kmeans(
            table, torch.from_numpy(ids).to(dev), K, n_init=cc.n_init, max_iter=cc.max_iter,
            seed=cc.seed, device=dev)
        full = torch.cat([torch.full((1,), -1, dtype=torch.int64, device=dev), labels])
    else:
        labels, _, inertia, n_iter = cluster.kmeans(
            np.ascontiguousarray(_host_table(embeddings), dtype=np.float32), ids, K,
            n_init=cc.n_init, max_iter=cc.max_iter, seed=cc.seed)
        full = np.concatenate([[-1], labels])
    result = {'cluster_inertia': inertia, 'cluster_modularity': cluster.modularity(csr, full, K),
              'cluster_iterations': float(n_iter)}
    if y is not None:
        rows = np.asarray(rows, dtype=np.int64)
        truth = np.asarray(y, dtype=np.int64)
        if cc.backend == 'device':
            found = full[torch.from_numpy(rows).to(full.device)]
            truth = torch.from_numpy(truth).to(full.device)
        else:
            found = full[rows]
        table = cluster.contingency(truth, found)
        result['cluster_nmi'] = cluster.nmi_from_table(table)
        result['cluster_ari'] = cluster.ari_from_table(table)
    logger.info('Clustering: ' + ', '.join(f'{k}={v:.6g}' for k, v in result.items())
                + f' (K={K}, {V - 1} nodes).')
    return result


def _device_table(embeddings, dev):
    """The float32 table on ``dev``: a checkpoint's numpy array, or a tensor a file was read to."""
    import torch
    if isinstance(embeddings, torch.Tensor):
        return embeddings.to(device=dev, dtype=torch.float32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(embeddings, dtype=np.float32)).to(dev)


def _host_table(embeddings) -> np.ndarray:
    return embeddings if isinstance(embeddings, np.ndarray) else embeddings.cpu().numpy()


def load_file_embeddings(cfg, dataset):
    """``downstream.embeddings_path``: the table of a word2vec text file (this project's export,
    the node2vec or DeepWalk reference programs', gensim's) laid out by the dataset's vocabulary
    (embeddings_io.align_word2vec: keys as export_embeddings.py writes them, ids first, then
    vocabulary tokens). The HIP reader parses it when a GPU is visible and a device backend is
    chosen (the table then stays on the GPU), the same code on the host otherwise."""
    import torch
    from shallow_encoders.word2vec.embeddings_io import align_word2vec, read_word2vec_format
    ds = cfg.downstream
    nc, ec = ds.node_classification, ds.edge_classification
    on_device = torch.cuda.is_available() and (
        (nc.enable and nc.backend == 'device') or
        (ec.enable and (ec.backend == 'device' or ec.protocol == 'heldout')) or
        (ds.clustering.enable and ds.clustering.backend == 'device'))
    read = read_word2vec_format(ds.embeddings_path, device='cuda' if on_device else None)
    vocab = getattr(getattr(dataset, 'dataset', None), 'csr', None) or dataset.vocab
    try:
        emb = align_word2vec(read, vocab, missing=ds.embeddings_missing, style='id')
    except ValueError as by_id:
        try:
            emb = align_word2vec(read, vocab, missing=ds.embeddings_missing, style='token')
        except ValueError:
            raise by_id from None
    logger.info(f'Read {read.n} x {read.d} embeddings from "{ds.embeddings_path}" '
                f'({"the GPU" if on_device else "the host"}).')
    return emb if on_device else np.asarray(emb)


def load_input_embeddings(cfg, dataset, checkpoint_path: str) -> np.ndarray:
    """Input-embedding table of a tools/train.py checkpoint (weights-only load)."""
    import torch
    state = torch.load(checkpoint_path, map_location='cpu', weights_only=True)
    sd = state.get('state_dict', state)
    key = '_model._input_embedding.weight'
    if key not in sd:
        key = '_input_embedding.weight'
    w = sd[key].numpy()
    assert w.shape[0] == len(dataset.vocab), \
        f'checkpoint has {w.shape[0]} rows, the dataset vocabulary {len(dataset.vocab)}'
    return w


def parse_args(argv):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('--config-name', '-cn', default='sge_sg_graph_triplets')
    ap.add_argument('--config-path', '-cp', default=CONFIG_PATH)
    ap.add_argument('overrides', nargs='*', help='key.sub=value overrides')
    return ap.parse_args(argv)


def main(argv=None) -> Dict[str, float]:
    logging.basicConfig(level=logging.INFO)
    args = parse_args(sys.argv[1:] if argv is None else argv)
    raw = load_config_dict(args.config_name, args.config_path, args.overrides)
    cfg = setup_pipeline(raw, task='downstream-classification')
    assert cfg.datamodule.is_graph, 'This script supports only graph datasets!'
    dataset = cfg.datamodule.instantiate_dataset()
    out, ds, exp = cfg.path.output_dir, cfg.datamodule.dataset_name, cfg.train.experiment
    ckpt = conventions.get_checkpoint_path(out, ds, exp, cfg.analysis.checkpoint)
    if cfg.downstream.embeddings_path is not None:
        emb = load_file_embeddings(cfg, dataset)
    else:
        emb = load_input_embeddings(cfg, dataset, ckpt)
    analysis_dir = conventions.get_analysis_experiment_path(out, ds, exp)
    Path(analysis_dir).mkdir(parents=True, exist_ok=True)
    result: Dict[str, float] = {}
    nc = cfg.downstream.node_classification
    if nc.enable:
        check_node_backend(dataset, nc)
    if nc.enable and nc.backend == 'device':
        result.update(node_classification_on_device(emb, dataset, nc))
    elif nc.enable:
        plot = os.path.join(analysis_dir, 'downstream-node-classification.jpg') \
            if nc.visualize else None
        result['node_accuracy'], result['node_best'] = node_classification(
            _host_table(emb), dataset.vocab.get_itos(), dataset.labels, nc.instantiate_split_algorithm(),
            nc.n_experiments, features=dataset.features if dataset.has_features else None,
            classifier_params=nc.classifier_params, plot_path=plot)
    ec = cfg.downstream.edge_classification
    if ec.enable and ec.protocol == 'heldout':
        result.update(heldout_edge_classification_on_device(emb, dataset, ec))
    elif ec.enable and ec.backend == 'device':
        result['edge_accuracy'], result['edge_best'] = edge_classification_on_device(
            emb, dataset.graph, ec)
    elif ec.enable:
        result['edge_accuracy'], result['edge_best'] = edge_classification(
            _host_table(emb), dataset.graph, dataset.vocab.get_stoi(), ec.train_ratio, ec.n_experiments,
            ec.operator_name, classifier_params=ec.classifier_params)
    cc = cfg.downstream.clustering
    scores = dict(result)
    if cc.enable:
        result.update(clustering(emb, dataset, cc))
    print(' '.join([f'{k}={100 * v:.2f}%' for k, v in scores.items()] +
                   [f'{k}={v:.6g}' for k, v in result.items() if k not in scores]), flush=True)
    return result


if __name__ == '__main__':
    main()
