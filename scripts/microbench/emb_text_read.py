"""Cost of reading word2vec text back into an embedding table (shallow_encoders/word2vec/
embeddings_io.py: read_word2vec_format; dw_embread_lines and dw_embread_parse in
csrc/dw_embread.hip) at the headline shape C3: the writer's own text of V = 2^20 + 1 rows, d = 128,
int64 keys, values N(0, 0.3^2) (seed 0). Everything is reported, nothing is gated.

  kernels  pass 1 (the line index) and pass 2 (the tokens), the whole text resident in HBM, device
           events; beside them, in the same windows (one repetition runs each of them once, so
           they alternate), three yardsticks: dw_edgelist_parse_weighted on a ~316 MB "u v w" text
           (the nearest existing parser), dw_embtext_write of the same table (the inverse
           operation) and dw_stream_copy, whose rate turns the byte floor — the text read twice,
           the table written once — into a time. Medians of `--reps` windows after a warm-up. The
           parsed table is compared with the written one, and the undecided count reported;
  file     read_word2vec_format of the file on the device (wall clock: file reads, pinned
           staging, copies, both passes, keys), medians;
  host     the first 2^16 rows: load_word2vec_format (the existing Python loader) and
           read_word2vec_format on the host path (dw_embread_host, one thread), scaled to the
           table by rows.

    python scripts/microbench/emb_text_read.py [--part kernels|file|host|all] [--json PATH]

One JSON line per part on stdout (and appended to --json, default profiles/emb_text_read.jsonl).
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
from shallow_encoders.word2vec.embeddings_io import (f32text_table, load_word2vec_format,  # noqa: E402
                                                     pow5_table, read_word2vec_format,
                                                     save_word2vec_format)

V, D, HOST_ROWS = (1 << 20) + 1, 128, 1 << 16
EDGE_LINES = 11_700_000   # of ~27 bytes: the weighted edge-list yardstick's ~316 MB


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


def write_text(table, keys_i64, key_bytes, key_off, dev):
    """(text on the device, the write as a callable) of dw_embtext_sizes / dw_embtext_write."""
    n, d = table.shape
    tab = f32text_table(dev)
    line_off = torch.empty(n + 1, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    nb = ctypes.c_size_t(0)
    _native.call('dw_embtext_workspace_bytes', n, d, ctypes.byref(nb))
    ws = torch.empty(max(1, nb.value), dtype=torch.uint8, device=dev)

    def p(t):
        return None if t is None else t.data_ptr()
    ins = (table.data_ptr(), n, d, None, n, p(keys_i64), p(key_bytes), p(key_off), tab.data_ptr())
    _native.call('dw_embtext_sizes', *ins, line_off.data_ptr(), status.data_ptr(), ws.data_ptr(),
                 ws.numel(), _native.stream(dev))
    total = int(line_off[-1].item())
    out = torch.empty(total, dtype=torch.uint8, device=dev)

    def write():
        _native.call('dw_embtext_write', *ins, line_off.data_ptr(), 0, n, out.data_ptr(), total,
                     status.data_ptr(), _native.stream(dev))
    write()
    assert int(status.item()) == 0
    return out, write


def edge_text(dev):
    """A "u v w" text of EDGE_LINES lines on the device: the writer with d = 1 and the two ids,
    zero-padded to 7 digits, as the key's bytes; weights uniform in [0.5, 1.5)."""
    gen = torch.Generator(device=dev).manual_seed(1)
    ids = torch.randint(0, 10 ** 7, (EDGE_LINES, 2), device=dev, generator=gen)
    w = torch.rand((EDGE_LINES, 1), device=dev, generator=gen) + 0.5
    digits = torch.full((EDGE_LINES, 15), ord(' '), dtype=torch.uint8, device=dev)
    for c in range(2):
        v = ids[:, c].clone()
        for k in range(6, -1, -1):
            digits[:, 8 * c + k] = (v % 10 + ord('0')).to(torch.uint8)
            v //= 10
    off = torch.arange(EDGE_LINES + 1, dtype=torch.int64, device=dev) * 15
    text, _ = write_text(w.contiguous(), None, digits.reshape(-1), off, dev)
    return text, w


def part_kernels(table, dev, path, reps):
    s = _native.stream(dev)
    keys = torch.arange(V, dtype=torch.int64, device=dev)
    text, write = write_text(table, keys, None, None, dev)
    n_bytes = text.numel()
    # the reader
    pow5 = pow5_table(dev)
    nb = ctypes.c_size_t(0)
    _native.call('dw_embread_workspace_bytes', n_bytes, ctypes.byref(nb))
    ws = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    back = torch.zeros_like(table)
    key_off, key_len, key_i64 = (torch.zeros(V, dtype=torch.int64, device=dev) for _ in range(3))
    line_off = torch.zeros(V + 1, dtype=torch.int64, device=dev)
    und = torch.zeros(4 << 16, dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    err = torch.zeros(1, dtype=torch.int64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def lines():
        _native.call('dw_embread_lines', text.data_ptr(), n_bytes, line_off.data_ptr(), V,
                     counts.data_ptr(), err.data_ptr(), ws.data_ptr(), ws.numel(), s)

    def parse():
        _native.call('dw_embread_parse', text.data_ptr(), n_bytes, line_off.data_ptr(), V, D,
                     pow5.data_ptr(), back.data_ptr(), V, 0, key_off.data_ptr(),
                     key_len.data_ptr(), key_i64.data_ptr(), und.data_ptr(), 1 << 16,
                     counts.data_ptr(), err.data_ptr(), status.data_ptr(), s)
    lines()
    parse()
    n_lines, n_und = counts.tolist()
    assert n_lines == V and int(status.item()) == 0 and int(err.item()) == -1
    bits_equal = bool(torch.equal(back.view(torch.int32), table.view(torch.int32)))
    keys_equal = bool(torch.equal(key_i64, keys))
    # the weighted edge-list parser on its own text
    etext, w = edge_text(dev)
    e_bytes = etext.numel()
    _native.call('dw_edgelist_workspace_bytes', e_bytes, 0, ctypes.byref(nb))
    ews = torch.empty(nb.value, dtype=torch.uint8, device=dev)
    cap = EDGE_LINES + 1
    src, dst = (torch.empty(cap, dtype=torch.int64, device=dev) for _ in range(2))
    wt = torch.empty(cap, dtype=torch.float64, device=dev)
    eund = torch.empty(2 << 16, dtype=torch.int64, device=dev)
    info = torch.zeros(4, dtype=torch.int64, device=dev)
    estatus = torch.zeros(1, dtype=torch.int32, device=dev)

    def edges():
        _native.call('dw_edgelist_parse_weighted', etext.data_ptr(), e_bytes, 0, pow5.data_ptr(),
                     src.data_ptr(), dst.data_ptr(), wt.data_ptr(), cap, eund.data_ptr(), 1 << 16,
                     info.data_ptr(), info[3:].data_ptr(), estatus.data_ptr(), ews.data_ptr(),
                     ews.numel(), s)
    edges()
    assert int(info[0]) == EDGE_LINES and int(estatus.item()) == 0
    edge_exact = bool(torch.equal(wt[:EDGE_LINES].to(torch.float32), w[:, 0]))
    # the copy
    nb16 = table.numel() * 4 - table.numel() * 4 % 16
    csrc = torch.empty(nb16, dtype=torch.uint8, device=dev)
    cdst = torch.empty_like(csrc)

    def copy():
        _native.call('dw_stream_copy', csrc.data_ptr(), cdst.data_ptr(), nb16, s)
    copy()
    torch.cuda.synchronize(dev)
    t = {k: [] for k in ('lines', 'parse', 'write', 'edges', 'copy')}
    for _ in range(reps):   # one window: each of the five once
        for name, fn in (('lines', lines), ('parse', parse), ('write', write), ('edges', edges),
                         ('copy', copy)):
            t[name].append(event_ms(fn, dev))
    ms = {k: statistics.median(v) for k, v in t.items()}
    copy_gbps = 2 * nb16 / ms['copy'] / 1e6
    floor_bytes = 2 * n_bytes + table.numel() * 4
    floor_ms = floor_bytes / copy_gbps / 1e6
    both = ms['lines'] + ms['parse']
    emit({'part': 'kernels', 'rows': V, 'd': D, 'values': 'normal(0, 0.3), seed 0',
          'text_bytes': n_bytes, 'pass1_ms': ms['lines'], 'pass2_ms': ms['parse'],
          'pass1_ms_all': t['lines'], 'pass2_ms_all': t['parse'],
          'text_GBps_pass1': n_bytes / ms['lines'] / 1e6,
          'text_GBps_pass2': n_bytes / ms['parse'] / 1e6, 'text_GBps_both': n_bytes / both / 1e6,
          'table_bits_equal': bits_equal, 'keys_equal': keys_equal, 'undecided_tokens': n_und,
          'writer_pass2_ms': ms['write'], 'writer_text_GBps': n_bytes / ms['write'] / 1e6,
          'edge_text_bytes': e_bytes, 'edge_parse_weighted_ms': ms['edges'],
          'edge_parse_weighted_GBps': e_bytes / ms['edges'] / 1e6,
          'edge_weights_equal': edge_exact, 'stream_copy_GBps': copy_gbps,
          'floor_bytes': floor_bytes, 'floor_at_stream_copy_ms': floor_ms,
          'both_over_floor': both / floor_ms,
          'reader_over_edge_parser_rate': (n_bytes / both) / (e_bytes / ms['edges']),
          'reader_over_writer_rate': ms['write'] / both, 'reps': reps}, path)


def part_file(table, dev, path, reps):
    keys = np.arange(V, dtype=np.int64)
    times = []
    with tempfile.TemporaryDirectory() as tmp:
        name = os.path.join(tmp, 'c3.emb')
        n_bytes = save_word2vec_format(name, table, keys=keys)
        small = os.path.join(tmp, 'w.emb')
        save_word2vec_format(small, table[:1024], keys=keys[:1024])
        read_word2vec_format(small, device=dev)   # warm-up
        for _ in range(reps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            back = read_word2vec_format(name, device=dev)
            torch.cuda.synchronize(dev)
            times.append(time.perf_counter() - t0)
        ok = bool(torch.equal(back.table.view(torch.int32), table.view(torch.int32)))
        ok = ok and bool(np.array_equal(back.keys_i64, keys))
    s = statistics.median(times)
    emit({'part': 'file', 'rows': V, 'd': D, 'file_bytes': n_bytes, 'chunk_bytes': 256 << 20,
          'read_s': s, 'read_s_all': times, 'file_GBps': n_bytes / s / 1e9, 'equal': ok,
          'host_tokens': back.host_tokens}, path)


def part_host(table, path):
    host = table[:HOST_ROWS].cpu().numpy()
    keys = np.arange(HOST_ROWS, dtype=np.int64)
    with tempfile.TemporaryDirectory() as tmp:
        name = os.path.join(tmp, 'h.emb')
        n_bytes = save_word2vec_format(name, host, keys=keys)
        t0 = time.perf_counter()
        back = read_word2vec_format(name)
        host_s = time.perf_counter() - t0
        t0 = time.perf_counter()
        _, loaded = load_word2vec_format(name)
        loader_s = time.perf_counter() - t0
    ok = bool(np.array_equal(back.table.view(np.uint32), host.view(np.uint32)) and
              np.array_equal(loaded.view(np.uint32), host.view(np.uint32)))
    emit({'part': 'host', 'rows': HOST_ROWS, 'd': D, 'file_bytes': n_bytes, 'equal': ok,
          'host_path_s': host_s, 'host_us_per_value': host_s / host.size * 1e6,
          'python_loader_s': loader_s, 'python_loader_us_per_value': loader_s / host.size * 1e6,
          'host_path_scaled_to_table_s': host_s * V / HOST_ROWS,
          'python_loader_scaled_to_table_s': loader_s * V / HOST_ROWS}, path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', default='all', choices=['all', 'kernels', 'file', 'host'])
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--json', default=os.path.join(REPO, 'profiles', 'emb_text_read.jsonl'))
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
