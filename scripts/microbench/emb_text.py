"""Cost of writing an embedding table as word2vec text (shallow_encoders/word2vec/
embeddings_io.py; dw_embtext_sizes and dw_embtext_write in csrc/dw_embtext.hip) at the headline
shape C3: V = 2^20 + 1 rows, d = 128, int64 keys. The values are N(0, 0.3^2) draws (seed 0), not
a trained checkpoint. Everything is reported, nothing is gated.

  kernels  pass 1 (sizes + scan) and pass 2 (the whole table into one device buffer), device
           events, medians of `--reps` runs after a warm-up, in one process; the text's GB/s over
           pass 2 and over both; the byte model (the table read twice, the text written once)
           over dw_stream_copy's measured rate, and the text's rate beside the edge-list
           parser's 161 GB/s: where the writer falls between a copy and the sibling parser;
  file     save_word2vec_format of the device table to a file (wall clock, workspace and pinned
           buffers included), medians;
  host     the host path (dw_embtext_host, one thread) and numpy.savetxt(fmt='%.9g') on the first
           2^16 rows of the same table.

    python scripts/microbench/emb_text.py [--part kernels|file|host|all] [--json PATH]

One JSON line per part on stdout (and appended to --json, default profiles/emb_text.jsonl).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(REPO, 'deepwalk-and-node2vec_amd'))

from shallow_encoders import _native  # noqa: E402
from shallow_encoders.word2vec.embeddings_io import (f32text_table,  # noqa: E402
                                                     save_word2vec_format)

V, D, HOST_ROWS = (1 << 20) + 1, 128, 1 << 16
PARSER_GBPS = 161.0   # the edge-list text parser's measured rate (profiles/edge_list.jsonl)


def emit(rec, path):
    line = json.dumps(rec)
    print(line, flush=True)
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')


def event_ms(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize(dev)
    return a.elapsed_time(b)


def stream_copy_gbps(nbytes, dev, reps=10):
    nbytes -= nbytes % 16
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)

    def copy():
        _native.call('dw_stream_copy', _native.ptr(src), _native.ptr(dst), nbytes,
                     _native.stream(dev))
    copy()
    torch.cuda.synchronize(dev)
    ms = statistics.median(event_ms(copy, dev) for _ in range(reps))
    return 2 * nbytes / ms / 1e6


def part_kernels(table, dev, path, reps):
    keys = torch.arange(V, dtype=torch.int64, device=dev)
    tab = f32text_table(dev)
    line_off = torch.empty(V + 1, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    nb = ctypes.c_size_t(0)
    _native.call('dw_embtext_workspace_bytes', V, D, ctypes.byref(nb))
    ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    ins = (table.data_ptr(), V, D, None, V, keys.data_ptr(), None, None, tab.data_ptr())

    def sizes():
        _native.call('dw_embtext_sizes', *ins, line_off.data_ptr(), status.data_ptr(),
                     ws.data_ptr(), ws.numel(), _native.stream(dev))
    sizes()
    total = int(line_off[-1].item())
    out = torch.empty(total, dtype=torch.uint8, device=dev)

    def write():
        _native.call('dw_embtext_write', *ins, line_off.data_ptr(), 0, V, out.data_ptr(), total,
                     status.data_ptr(), _native.stream(dev))
    write()
    torch.cuda.synchronize(dev)
    t1, t2 = [], []
    for _ in range(reps):
        t1.append(event_ms(sizes, dev))
        t2.append(event_ms(write, dev))
    assert int(status.item()) == 0
    ms1, ms2 = statistics.median(t1), statistics.median(t2)
    model = 2 * table.numel() * 4 + total
    copy = stream_copy_gbps(table.numel() * 4, dev)
    copy_ms = model / copy / 1e6
    parser_ms = total / PARSER_GBPS / 1e6
    emit({'part': 'kernels', 'rows': V, 'd': D, 'values': 'normal(0, 0.3), seed 0',
          'text_bytes': total, 'bytes_per_value': total / table.numel(),
          'pass1_ms': ms1, 'pass2_ms': ms2, 'pass1_ms_all': t1, 'pass2_ms_all': t2,
          'text_GBps_pass2': total / ms2 / 1e6, 'text_GBps_both': total / (ms1 + ms2) / 1e6,
          'model_bytes': model, 'stream_copy_GBps': copy, 'model_at_stream_copy_ms': copy_ms,
          'text_at_parser_rate_ms': parser_ms, 'both_over_copy_bound': (ms1 + ms2) / copy_ms,
          'both_over_parser_rate': (ms1 + ms2) / parser_ms}, path)
    return out, total


def part_file(table, dev, path, reps):
    keys = np.arange(V, dtype=np.int64)
    times = []
    with tempfile.TemporaryDirectory() as tmp:
        name = os.path.join(tmp, 'c3.emb')
        save_word2vec_format(name, table[:1024], keys=keys[:1024])   # warm-up
        for _ in range(reps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            n_bytes = save_word2vec_format(name, table, keys=keys)
            times.append(time.perf_counter() - t0)
        assert os.path.getsize(name) == n_bytes
    s = statistics.median(times)
    emit({'part': 'file', 'rows': V, 'd': D, 'file_bytes': n_bytes, 'chunk_bytes': 256 << 20,
          'save_s': s, 'save_s_all': times, 'file_GBps': n_bytes / s / 1e9}, path)


def part_host(table, path):
    host = table[:HOST_ROWS].cpu().numpy()
    keys = np.arange(HOST_ROWS, dtype=np.int64)
    with tempfile.TemporaryDirectory() as tmp:
        name = os.path.join(tmp, 'h.emb')
        save_word2vec_format(name, host[:64], keys=keys[:64])
        t0 = time.perf_counter()
        n_bytes = save_word2vec_format(name, host, keys=keys)
        host_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        np.savetxt(os.path.join(tmp, 's.txt'), host, fmt='%.9g')
        savetxt_s = time.perf_counter() - t0
    emit({'part': 'host', 'rows': HOST_ROWS, 'd': D, 'file_bytes': n_bytes,
          'host_path_s': host_s, 'host_us_per_value': host_s / host.size * 1e6,
          'savetxt_9g_s': savetxt_s, 'savetxt_us_per_value': savetxt_s / host.size * 1e6,
          'host_path_scaled_to_table_s': host_s * V / HOST_ROWS,
          'savetxt_scaled_to_table_s': savetxt_s * V / HOST_ROWS}, path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', default='all', choices=['all', 'kernels', 'file', 'host'])
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--json', default=os.path.join(REPO, 'profiles', 'emb_text.jsonl'))
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    _native.require_device(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    table = torch.randn((V, D), dtype=torch.float32, device=dev, generator=gen) * 0.3
    if args.part in ('all', 'kernels'):
        part_kernels(table, dev, args.json, args.reps)
    if args.part in ('all', 'file'):
        part_file(table, dev, args.json, max(3, args.reps // 2))
    if args.part in ('all', 'host'):
        part_host(table, args.json)


if __name__ == '__main__':
    main()
