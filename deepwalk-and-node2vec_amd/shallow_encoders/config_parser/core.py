"""Config schema and object factories (reference: config_parser/core.py:28-334).

The reference composes YAML with Hydra and validates it with pydantic dataclasses; neither
Hydra nor OmegaConf is installed in this image, so this module carries the same schema
(``GlobalConfig`` with ``train`` / ``datamodule`` / ``model`` / ``analysis`` / ``path`` /
``downstream`` sections, same field names and defaults) plus a small loader that accepts the
reference's YAML files unchanged: ``defaults: [w2v_config]``, ``_target_`` instantiation, and
``key.sub=value`` command-line overrides.

MI355X additions (all optional, defaulted, so reference configs load as they are):
  datamodule.backend      'hip' (device walks straight into the fused kernel) | 'collate'
                          (the reference's DataLoader + W2VCollateFunctional batches)
  datamodule.additional_parameters.rng / seed   walker sampling mode (random_walk_generator)
  train.noise             'torch' (reference-exact CPU noise) | 'device' (Philox on device) |
                          'unigram' (graph datasets: negatives in proportion to
                          degree ** train.noise_power, the word2vec / node2vec law; a departure
                          from the reference's uniform noise)
  train.noise_power       the unigram law's exponent (0.75)
  train.seed              seed for torch / Philox
  train.shared_negatives  0 (off) | S in {32, 64, 96, 128}: the centres of a walk share S negatives
                          drawn once per walk (noise 'device' or 'unigram'), the step one MFMA
                          kernel (dw_sgns_walks_shared) and the optimizer's dense Adam; a departure
                          from the reference's negatives per pair
  export.*                tools/export_embeddings.py: the table, path, key style and device of
                          the word2vec-text export (ExportConfig)
  downstream.embeddings_path     a word2vec text file whose table the downstream tool scores
                          instead of the checkpoint's (any program's .emb output)
  downstream.embeddings_missing  'error' | 'zero': vocabulary rows that file does not hold
``_target_: torch.optim.Adam`` instantiates the HIP Adam and ``_target_: torch.optim.SGD`` the HIP
SGD (word2vec/optim.py, same math).
"""
import copy
import dataclasses
import importlib
import logging
import os
import re
from dataclasses import dataclass, field
from typing import Any, Dict, Iterator, List, Optional, Union

import torch
import yaml
from torch import nn
from torch.optim import Optimizer

from shallow_encoders.common.path import CONFIG_PATH, RUNS_PATH

logger = logging.getLogger('ConfigParser')

# reference `_target_`s whose MI355X-native equivalent is substituted at instantiation
TARGET_SUBSTITUTES = {
    'torch.optim.Adam': 'shallow_encoders.word2vec.optim.Adam',
    'torch.optim.SGD': 'shallow_encoders.word2vec.optim.SGD',
}


def _locate(path: str):
    module, _, name = path.rpartition('.')
    try:
        return getattr(importlib.import_module(module), name)
    except (ImportError, AttributeError):
        # nested attribute (e.g. pkg.mod.Class.method)
        mod, _, outer = module.rpartition('.')
        return getattr(getattr(importlib.import_module(mod), outer), name)


def instantiate(cfg: Dict[str, Any], **kwargs):
    """Hydra-style ``_target_`` instantiation (recursive on nested ``_target_`` dicts)."""
    cfg = dict(cfg)
    target = cfg.pop('_target_')
    target = TARGET_SUBSTITUTES.get(target, target)
    params = {}
    for k, v in cfg.items():
        params[k] = instantiate(v) if isinstance(v, dict) and '_target_' in v else v
    params.update(kwargs)
    return _locate(target)(**params)


@dataclass
class TrainLossConfig:
    negative_samples: int


@dataclass
class TrainConfig:
    experiment: str
    optimizer: dict
    scheduler: dict
    loss: TrainLossConfig
    max_epochs: int
    accelerator: str
    devices: str
    noise: str = 'torch'
    seed: int = 0
    noise_power: float = 0.75
    shared_negatives: int = 0

    def instantiate_optimizer(self, params: Iterator[nn.Parameter]) -> Optimizer:
        return instantiate(self.optimizer, params=params)

    def instantiate_scheduler(self, optimizer: Optimizer):
        """Option 1: ``{_target_: ...}`` (stepped per epoch); option 2: PL dict with a nested
        ``scheduler`` plus ``interval`` / ``frequency`` (core.py:55-94)."""
        if '_target_' in self.scheduler:
            return instantiate(self.scheduler, optimizer=optimizer)
        assert 'scheduler' in self.scheduler, 'Missing scheduler object in scheduler configuration.'
        scheduler = copy.deepcopy(self.scheduler)
        scheduler['scheduler'] = instantiate(scheduler['scheduler'], optimizer=optimizer)
        return scheduler


@dataclass
class DatamoduleConfig:
    dataset_name: str
    mode: str
    context_radius: int
    max_length: int
    is_graph: bool
    batch_size: int
    num_workers: int
    min_word_frequency: int = 0
    lemmatize: bool = False
    additional_parameters: dict = field(default_factory=dict)
    backend: str = 'hip'

    def instantiate_dataset(self):
        from shallow_encoders.word2vec.dataloader.torch_dataset import GraphDataset, W2VDataset
        if self.is_graph:
            if self.min_word_frequency > 0:
                logger.warning('Min word frequency has no effect for graph datasets.')
            if self.lemmatize:
                logger.warning('Lemmatization does not have effect on graph datasets.')
            return GraphDataset(dataset_name=self.dataset_name,
                                context_radius=self.context_radius,
                                additional_parameters=self.additional_parameters)
        return W2VDataset(dataset_name=self.dataset_name, context_radius=self.context_radius,
                          min_word_frequency=self.min_word_frequency, lemmatize=self.lemmatize,
                          additional_parameters=self.additional_parameters)

    def instantiate_collate_fn(self):
        from shallow_encoders.word2vec.dataloader.torch_dataset import W2VCollateFunctional
        return W2VCollateFunctional(mode=self.mode, context_radius=self.context_radius,
                                    max_length=self.max_length)

    def instantiate_dataloader(self, dataset=None):
        """backend 'hip' + graph + sg: an iterable of device walk batches; otherwise the
        reference's torch DataLoader with W2VCollateFunctional (num_workers honoured)."""
        dataset = self.instantiate_dataset() if dataset is None else dataset
        if self.backend == 'hip' and self.is_graph and self.mode.lower() == 'sg':
            return WalkBatchLoader(dataset, self.batch_size)
        from torch.utils.data import DataLoader
        return DataLoader(dataset, batch_size=self.batch_size, num_workers=self.num_workers,
                          collate_fn=self.instantiate_collate_fn())


class WalkBatchLoader:
    """Re-iterable epoch source of device walk batches (int32 [batch_size, L])."""

    def __init__(self, dataset, batch_size: int):
        self.dataset = dataset
        self.batch_size = batch_size

    def __iter__(self):
        return iter(self.dataset.walk_batches(self.batch_size))

    def __len__(self) -> int:
        n = len(self.dataset.dataset)
        return (n + self.batch_size - 1) // self.batch_size


@dataclass
class ModelClosestPairAnalysisConfig:
    enable: bool = True
    max_words: int = 100
    pairs_per_word: int = 5


@dataclass
class ModelVisualizeEmbeddingsAnalysisConfig:
    enable: bool = True
    annotate: bool = True
    max_words: int = 1000
    skip_unk: bool = True


@dataclass
class ModelSemanticsTestAnalysisConfig:
    enable: bool = True


@dataclass
class ModelAnalysisConfig:
    checkpoint: str = 'last.ckpt'
    closest_pairs: ModelClosestPairAnalysisConfig = field(
        default_factory=ModelClosestPairAnalysisConfig)
    visualize_embeddings: ModelVisualizeEmbeddingsAnalysisConfig = field(
        default_factory=ModelVisualizeEmbeddingsAnalysisConfig)
    semantics_test: ModelSemanticsTestAnalysisConfig = field(
        default_factory=ModelSemanticsTestAnalysisConfig)


DEFAULT_SPLIT_ALGORITHM = {'_target_': 'shallow_encoders.split.TrainTestRatioSplit',
                           'random_state': 42, 'train_ratio': 0.5, 'stratify': False}


@dataclass
class GraphDownstreamNodeClassificationConfig:
    enable: bool = True
    n_experiments: int = 10
    visualize: bool = True
    split_algorithm: Optional[dict] = None
    classifier_params: Optional[dict] = None
    # 'sklearn': the reference's host path over a float64 copy of the table; 'device': the
    # fp32 table stays in HBM (shallow_encoders/graph/nodeclf.py)
    backend: str = 'sklearn'
    # a multi-label dataset's decision rule: 'top_k' gives a node as many labels as it truly
    # has (the DeepWalk / node2vec papers' protocol), 'threshold' is sklearn's predict
    prediction: str = 'top_k'

    def __post_init__(self):
        if self.backend not in ('sklearn', 'device'):
            raise ValueError(f'downstream.node_classification.backend must be "sklearn" or '
                             f'"device", got {self.backend!r}')
        if self.prediction not in ('top_k', 'threshold'):
            raise ValueError(f'downstream.node_classification.prediction must be "top_k" or '
                             f'"threshold", got {self.prediction!r}')

    def instantiate_split_algorithm(self):
        """The configured split (reference: config_parser/core.py:217-232). Without one, the
        reference's intended default (train_ratio 0.5, seed 42, not stratified) is used; the
        reference records that default but then instantiates the missing entry."""
        if self.split_algorithm is None:
            self.split_algorithm = dict(DEFAULT_SPLIT_ALGORITHM)
        return instantiate(self.split_algorithm)


@dataclass
class GraphDownstreamEdgeClassificationConfig:
    enable: bool = True
    operator_name: str = 'hadamard'
    train_ratio: float = 0.5
    n_experiments: int = 10
    classifier_params: Optional[dict] = None
    # 'sklearn': the reference's host path over a networkx graph; 'device': the CSR path of
    # shallow_encoders/graph/linkpred.py (any graph dataset, graph_rmat included)
    backend: str = 'sklearn'
    # 'reference': the reference's in-sample protocol (every edge is walked, then classified);
    # 'heldout': node2vec §4.4 — the dataset hides edges (holdout_ratio > 0), the table is trained
    # on the rest, the hidden edges are ranked against non-edges (ROC AUC; backend=device only)
    protocol: str = 'reference'
    # 'classifier': the fitted logistic regression's score; 'dot': the rows' dot product, no fit
    scorer: str = 'classifier'

    def __post_init__(self):
        if self.backend not in ('sklearn', 'device'):
            raise ValueError(f'downstream.edge_classification.backend must be "sklearn" or '
                             f'"device", got {self.backend!r}')
        if self.protocol not in ('reference', 'heldout'):
            raise ValueError(f'downstream.edge_classification.protocol must be "reference" or '
                             f'"heldout", got {self.protocol!r}')
        if self.scorer not in ('classifier', 'dot'):
            raise ValueError(f'downstream.edge_classification.scorer must be "classifier" or '
                             f'"dot", got {self.scorer!r}')
        if self.protocol == 'heldout' and self.backend != 'device':
            raise ValueError('downstream.edge_classification.protocol=heldout runs on the device '
                             'only: set downstream.edge_classification.backend=device')


@dataclass
class GraphDownstreamClusteringConfig:
    """k-means communities of the embeddings (node2vec §4.1; a departure: the reference has no
    clustering task), shallow_encoders/graph/cluster.py."""
    enable: bool = False
    # 0: the number of label classes (a dataset without labels must name it)
    n_clusters: int = 0
    n_init: int = 1
    max_iter: int = 100
    seed: int = 0
    # 'device': the fp32 table stays in HBM (dw_kmeans_step); 'host': the same loop in numpy
    backend: str = 'device'

    def __post_init__(self):
        if self.backend not in ('host', 'device'):
            raise ValueError(f'downstream.clustering.backend must be "host" or "device", got '
                             f'{self.backend!r}')
        if isinstance(self.n_clusters, bool) or not isinstance(self.n_clusters, int) \
                or not 0 <= self.n_clusters <= 1024:
            raise ValueError(f'downstream.clustering.n_clusters must be an integer in [0, 1024] '
                             f'(0: the number of label classes), got {self.n_clusters!r}')
        if not isinstance(self.n_init, int) or self.n_init < 1:
            raise ValueError(f'downstream.clustering.n_init must be >= 1, got {self.n_init!r}')
        if not isinstance(self.max_iter, int) or self.max_iter < 1:
            raise ValueError(f'downstream.clustering.max_iter must be >= 1, got '
                             f'{self.max_iter!r}')
        if not isinstance(self.seed, int) or self.seed < 0:
            raise ValueError(f'downstream.clustering.seed must be >= 0, got {self.seed!r}')


@dataclass
class GraphDownstreamTaskConfig:
    checkpoint: str = 'last.ckpt'
    node_classification: GraphDownstreamNodeClassificationConfig = field(
        default_factory=GraphDownstreamNodeClassificationConfig)
    edge_classification: GraphDownstreamEdgeClassificationConfig = field(
        default_factory=GraphDownstreamEdgeClassificationConfig)
    clustering: GraphDownstreamClusteringConfig = field(
        default_factory=GraphDownstreamClusteringConfig)
    embeddings_path: Optional[str] = None   # a word2vec text file instead of the checkpoint
    embeddings_missing: str = 'error'       # 'error' | 'zero' (embeddings_io.align_word2vec)

    def __post_init__(self):
        if self.embeddings_missing not in ('error', 'zero'):
            raise ValueError(f'downstream.embeddings_missing must be "error" or "zero", got '
                             f'{self.embeddings_missing!r}')


@dataclass
class ExportConfig:
    """tools/export_embeddings.py: a checkpoint's table (analysis.checkpoint) as word2vec text."""
    table: str = 'input'          # 'input' | 'output': the input table is what downstream reads
    path: Optional[str] = None    # default: embeddings.emb in the experiment's analysis directory
    keys: str = 'id'              # 'id': the user's node names or ids | 'token': vocabulary tokens
    include_unk: bool = False
    nonfinite: str = 'error'      # 'error' | 'write'
    device: str = 'auto'          # 'auto': the GPU when one is visible | 'cpu' | 'cuda[:i]'

    def __post_init__(self):
        if self.table not in ('input', 'output'):
            raise ValueError(f'export.table must be "input" or "output", got {self.table!r}')
        if self.keys not in ('id', 'token'):
            raise ValueError(f'export.keys must be "id" or "token", got {self.keys!r}')
        if self.nonfinite not in ('error', 'write'):
            raise ValueError(f'export.nonfinite must be "error" or "write", got '
                             f'{self.nonfinite!r}')


@dataclass
class PathConfig:
    output_dir: str = RUNS_PATH


@dataclass
class GlobalConfig:
    train: TrainConfig
    datamodule: DatamoduleConfig
    model: dict
    analysis: ModelAnalysisConfig = field(default_factory=ModelAnalysisConfig)
    path: PathConfig = field(default_factory=PathConfig)
    downstream: GraphDownstreamTaskConfig = field(default_factory=GraphDownstreamTaskConfig)
    export: ExportConfig = field(default_factory=ExportConfig)

    def instantiate_model(self, dataset=None):
        dataset = self.datamodule.instantiate_dataset() if dataset is None else dataset
        return instantiate(self.model, vocab_size=len(dataset.vocab))

    def instantiate_trainer(self, model=None, optimizer=None, scheduler=None, dataset=None,
                            checkpoint_path: Optional[str] = None, device=None):
        from shallow_encoders.word2vec.trainer import Word2VecTrainer
        dataset = self.datamodule.instantiate_dataset() if dataset is None else dataset
        model = self.instantiate_model(dataset=dataset) if model is None else model
        if checkpoint_path is not None:
            state = torch.load(checkpoint_path, map_location='cpu', weights_only=True)
            sd = state.get('state_dict', state)
            sd = {k[len('_model.'):] if k.startswith('_model.') else k: v for k, v in sd.items()}
            model.load_state_dict(sd)
        if device is not None:
            model = model.to(device)
        elif torch.cuda.is_available():
            model = model.cuda()
        optimizer = self.train.instantiate_optimizer(model.parameters()) \
            if optimizer is None else optimizer
        scheduler = self.train.instantiate_scheduler(optimizer) if scheduler is None else scheduler
        extra = {}
        if self.train.noise == 'unigram':
            extra = dict(noise_weights=unigram_weights(dataset),
                         noise_power=self.train.noise_power)
        return Word2VecTrainer(model=model, optimizer=optimizer, scheduler=scheduler,
                               neg_samples=self.train.loss.negative_samples,
                               vocab_size=len(dataset.vocab), noise=self.train.noise,
                               seed=self.train.seed,
                               context_radius=self.datamodule.context_radius,
                               shared_negatives=self.train.shared_negatives, **extra)


def unigram_weights(dataset) -> torch.Tensor:
    """train.noise='unigram': float64 [V] weights by vocabulary id for a graph dataset — the
    CSR's degrees, or the weighted degrees (each row's weights summed in order) of a weighted
    graph; row 0 (``<unk>``, no neighbours) gets 0 and is never drawn. A text dataset has no
    such table here: build the trainer with its own ``noise_weights``."""
    import numpy as np
    csr = getattr(getattr(dataset, 'dataset', None), 'csr', None)
    if csr is None:
        raise ValueError('train.noise=unigram takes its weights from a graph dataset\'s degrees; '
                         'for a text dataset construct Word2VecTrainer(noise="unigram", '
                         'noise_weights=<count per vocabulary id>) yourself')
    deg = np.diff(csr.row_ptr)
    if not csr.weighted:
        return torch.from_numpy(deg.astype(np.float64))
    rows = np.repeat(np.arange(len(deg)), deg)
    return torch.from_numpy(np.bincount(rows, weights=csr.weights, minlength=len(deg)))


# ------------------------------------------------------------------------------- loading
def _from_dict(cls, data):
    if not dataclasses.is_dataclass(cls):
        return data
    if data is None:
        data = {}
    if not isinstance(data, dict):
        raise TypeError(f'{cls.__name__}: expected a mapping, got {type(data).__name__}')
    kwargs = {}
    names = {f.name: f for f in dataclasses.fields(cls)}
    unknown = set(data) - set(names)
    if unknown:
        raise KeyError(f'{cls.__name__}: unknown config keys {sorted(unknown)}')
    for name, f in names.items():
        if name not in data:
            continue
        ftype = f.type if not isinstance(f.type, str) else _resolve_type(f.type)
        kwargs[name] = _from_dict(ftype, data[name]) if dataclasses.is_dataclass(ftype) \
            else data[name]
    return cls(**kwargs)


class _ConfigLoader(yaml.SafeLoader):
    """SafeLoader whose floats follow YAML 1.2 / OmegaConf (the reference's loader): ``1e-3``
    and ``1E+2`` are floats, not strings."""


_ConfigLoader.add_implicit_resolver(
    'tag:yaml.org,2002:float',
    re.compile(r'''^(?:[-+]?(?:[0-9][0-9_]*)\.[0-9_]*(?:[eE][-+]?[0-9]+)?
                |[-+]?(?:[0-9][0-9_]*)(?:[eE][-+]?[0-9]+)
                |\.[0-9_]+(?:[eE][-+]?[0-9]+)?
                |[-+]?\.(?:inf|Inf|INF)
                |\.(?:nan|NaN|NAN))$''', re.X),
    list('-+0123456789.'))


def _yaml(text_or_stream):
    return yaml.load(text_or_stream, Loader=_ConfigLoader)


def _resolve_type(name: str):
    return globals().get(name, object)


def _parse_value(text: str):
    return _yaml(text)


def apply_overrides(cfg: Dict[str, Any], overrides: List[str]) -> Dict[str, Any]:
    """Apply ``a.b.c=value`` overrides (YAML-typed values) to a nested dict in place."""
    for ov in overrides:
        key, sep, value = ov.partition('=')
        if not sep:
            raise ValueError(f'override "{ov}" is not key=value')
        key = key.lstrip('+')
        node = cfg
        parts = key.split('.')
        for p in parts[:-1]:
            node = node.setdefault(p, {})
        node[parts[-1]] = _parse_value(value)
    return cfg


def load_config_dict(config_name: str, config_path: str = CONFIG_PATH,
                     overrides: Optional[List[str]] = None) -> Dict[str, Any]:
    name = config_name if config_name.endswith('.yaml') else config_name + '.yaml'
    path = name if os.path.isabs(name) else os.path.join(config_path, name)
    with open(path, 'r', encoding='utf-8') as f:
        raw = _yaml(f) or {}
    defaults = raw.pop('defaults', [])
    for d in defaults:
        if d not in ('w2v_config', '_self_'):
            raise ValueError(f'unsupported defaults entry {d!r} (only w2v_config)')
    return apply_overrides(raw, list(overrides or []))


def config_from_dict(data: Dict[str, Any]) -> GlobalConfig:
    data = copy.deepcopy(data)
    data.pop('output_dir', None)  # top-level key read by tools/utils.py (reference quirk)
    return _from_dict(GlobalConfig, data)


def load_config(config_name: str, config_path: str = CONFIG_PATH,
                overrides: Optional[List[str]] = None) -> GlobalConfig:
    """Load a reference-style YAML config (``defaults: [w2v_config]``) into GlobalConfig."""
    return config_from_dict(load_config_dict(config_name, config_path, overrides))


def to_yaml(cfg: Union[GlobalConfig, Dict[str, Any]]) -> str:
    data = dataclasses.asdict(cfg) if dataclasses.is_dataclass(cfg) else cfg
    return yaml.safe_dump(data, sort_keys=False)
