"""Export a trained model's embeddings as word2vec text (``node_id v_0 ... v_{d-1}`` lines).

    python tools/export_embeddings.py --config-name=sge_sg_edge_list [key=value ...]

Loads ``{output_dir}/{dataset}/{experiment}/checkpoints/{analysis.checkpoint}`` (tools/train.py
output) and writes ``{output_dir}/{dataset}/{experiment}/analysis/embeddings.emb``, the format the
node2vec and DeepWalk reference programs emit and gensim's ``KeyedVectors.load_word2vec_format``
reads. The first column holds the user's own node names: an edge-list graph's ids, a synthetic
graph's node numbers, a networkx graph's node names, a text vocabulary's tokens. The config's
optional ``export`` section (config_parser/core.py: ExportConfig) picks the table, the path, the
key style, whether ``<unk>`` is written, what happens to nan / inf, and the device: with a GPU
visible the HIP kernels convert the table, otherwise the same code on the host.
"""
import argparse
import logging
import os
import sys
from pathlib import Path

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from shallow_encoders.common.path import CONFIG_PATH  # noqa: E402
from shallow_encoders.config_parser import load_config_dict  # noqa: E402
from shallow_encoders.word2vec.embeddings_io import save_word2vec_format  # noqa: E402
from tools import conventions  # noqa: E402
from tools.model_analysis import load_tables  # noqa: E402
from tools.utils import setup_pipeline  # noqa: E402

logger = logging.getLogger('ExportEmbeddings')


def dataset_keys(dataset, style: str, include_unk: bool):
    """The file's first column for the dataset's vocabulary (rows 1 .. V - 1, or 0 .. V - 1)."""
    csr = getattr(getattr(dataset, 'dataset', None), 'csr', None)
    if csr is not None:
        return csr.export_keys(style, include_unk)
    return list(dataset.vocab.get_itos()[0 if include_unk else 1:])


def parse_args(argv):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument('--config-name', '-cn', default='sge_sg_karate_club')
    ap.add_argument('--config-path', '-cp', default=CONFIG_PATH)
    ap.add_argument('overrides', nargs='*', help='key.sub=value overrides')
    return ap.parse_args(argv)


def main(argv=None) -> str:
    logging.basicConfig(level=logging.INFO)
    args = parse_args(sys.argv[1:] if argv is None else argv)
    raw = load_config_dict(args.config_name, args.config_path, args.overrides)
    cfg = setup_pipeline(raw, task='export')
    ex = cfg.export
    dataset = cfg.datamodule.instantiate_dataset()
    out, ds, exp = cfg.path.output_dir, cfg.datamodule.dataset_name, cfg.train.experiment
    w_in, w_out = load_tables(conventions.get_checkpoint_path(out, ds, exp,
                                                              cfg.analysis.checkpoint))
    table = (w_in if ex.table == 'input' else w_out).contiguous()
    if table.shape[0] != len(dataset.vocab):
        raise ValueError(f'the checkpoint holds {table.shape[0]} rows, the dataset\'s vocabulary '
                         f'{len(dataset.vocab)}')
    device = ex.device
    if device == 'auto':
        device = 'cuda' if torch.cuda.is_available() else 'cpu'
    table = table.to(device)
    first = 0 if ex.include_unk else 1
    keys = dataset_keys(dataset, ex.keys, ex.include_unk)
    path = ex.path
    if path is None:
        path = os.path.join(conventions.get_analysis_experiment_path(out, ds, exp),
                            'embeddings.emb')
    Path(os.path.dirname(os.path.abspath(path))).mkdir(parents=True, exist_ok=True)
    n_bytes = save_word2vec_format(path, table, keys=keys,
                                   rows=np.arange(first, table.shape[0], dtype=np.int64),
                                   nonfinite=ex.nonfinite)
    logger.info(f'Saved {table.shape[0] - first} x {table.shape[1]} embeddings ({ex.table} table, '
                f'{n_bytes} bytes, {device}) at path "{path}".')
    return path


if __name__ == '__main__':
    main()
